// CPU emulation driver for hsds_amd/csrc/query.h (TEST INFRASTRUCTURE ONLY): every lane of
// every mask word of the query_mask / query_emit grids in turn, over host buffers, so the
// predicate programs, the word padding, the ranks, the limit, the response records and the
// update are checked against the reference's goldens and a numpy model on CPU.  Same
// argument lists as the C ABI (include/hsds_amd.h); returns 0 or HSDS_ERR_ARG.  Never used
// by the product.
#include "../../hsds_amd/csrc/query.h"

static int make_segs(const hsds_point_seg* segs, int nsegs, int chunk_elem, int out_elem, pt::Segs& g) {
  if (!segs || nsegs < 1 || nsegs > HSDS_POINT_MAX_SEGS) return 0;
  g.n = nsegs;
  g.out_elem = out_elem;
  for (int k = 0; k < HSDS_POINT_MAX_SEGS; k++) g.s[k] = k < nsegs ? segs[k] : hsds_point_seg{0, 0, 0};
  return pt::segs_ok(g, chunk_elem);
}

extern "C" int emu_query_mask(const uint8_t* arena, const hsds_query_chunk* chunks, int64_t nchunks, int64_t nwords,
                              int rowsize, const hsds_query_prog* prog, const uint8_t* isin, int64_t isin_bytes,
                              uint64_t* mask, int32_t* count) {
  if (nchunks < 0 || nwords < 0 || !prog || isin_bytes < 0 || !qy::prog_ok(*prog, rowsize, isin ? isin_bytes : 0))
    return HSDS_ERR_ARG;
  if (nwords == 0) return 0;
  if (!arena || !chunks || nchunks < 1 || !mask || !count) return HSDS_ERR_ARG;
  qy::MaskArgs a;
  a.arena = arena;
  a.chunks = chunks;
  a.nchunks = nchunks;
  a.nwords = nwords;
  a.rowsize = rowsize;
  a.isin = isin;
  a.mask = mask;
  a.count = count;
  a.prog = *prog;
  for (int64_t w = 0; w < nwords; w++) qy::mask_word(a, w, 0);
  return 0;
}

extern "C" int emu_query_emit(uint8_t* arena, const hsds_query_chunk* chunks, int64_t nchunks, int64_t nwords,
                              int rowsize, const uint64_t* mask, const int64_t* base, int64_t limit,
                              const hsds_point_seg* segs, int nsegs, int out_elem, uint8_t* out,
                              const hsds_point_seg* upd_segs, int n_upd_segs, int upd_elem, const uint8_t* upd) {
  qy::EmitArgs a;
  if (nchunks < 0 || nwords < 0 || limit < 0 || !make_segs(segs, nsegs, rowsize, out_elem, a.segs)) return HSDS_ERR_ARG;
  if (a.segs.s[0].out_off < 8) return HSDS_ERR_ARG;
  a.upd = 0;
  a.upd_segs = a.segs;
  if (upd_segs) {
    if (!upd || !make_segs(upd_segs, n_upd_segs, rowsize, upd_elem, a.upd_segs)) return HSDS_ERR_ARG;
    a.upd = upd;
  }
  if (nwords == 0) return 0;
  if (!arena || !chunks || nchunks < 1 || !mask || !base || !out) return HSDS_ERR_ARG;
  a.arena = arena;
  a.chunks = chunks;
  a.nchunks = nchunks;
  a.nwords = nwords;
  a.rowsize = rowsize;
  a.mask = mask;
  a.base = base;
  a.limit = limit;
  a.out = out;
  for (int64_t w = 0; w < nwords; w++)
    for (uint32_t l = 0; l < 64; l++) qy::emit_row(a, w, l);
  return 0;
}
