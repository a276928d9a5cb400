// CPU emulation driver for hsds_amd/csrc/points.h (TEST INFRASTRUCTURE ONLY): every thread
// of the points_locate / points_gather / points_scatter grids in turn, over host buffers, so
// the point paths (16-byte destination slots with straddling elements, typed moves, segment
// tables, fill, the duplicate rule) are checked against the reference's goldens and a numpy
// model on CPU.  Same argument lists as the C ABI (include/hsds_amd.h) plus the number of
// emulated threads; returns 0 or HSDS_ERR_ARG.  Never used by the product.
#include "../../hsds_amd/csrc/points.h"

static int make_segs(const hsds_point_seg* segs, int nsegs, int chunk_elem, int out_elem, pt::Segs& g) {
  if (!segs || nsegs < 1 || nsegs > HSDS_POINT_MAX_SEGS) return 0;
  g.n = nsegs;
  g.out_elem = out_elem;
  for (int k = 0; k < HSDS_POINT_MAX_SEGS; k++) g.s[k] = k < nsegs ? segs[k] : hsds_point_seg{0, 0, 0};
  return pt::segs_ok(g, chunk_elem);
}

extern "C" int emu_points_locate(const hsds_point_geom* geom, const uint64_t* pts, int64_t n, int64_t* chunk,
                                 int64_t* eoff, int32_t* nbad, uint32_t nthreads) {
  if (!geom || geom->rank < 1 || geom->rank > HSDS_MAX_RANK || geom->itemsize < 1 || n < 0) return HSDS_ERR_ARG;
  for (int d = 0; d < geom->rank; d++)
    if (geom->layout[d] < 1) return HSDS_ERR_ARG;
  for (uint32_t t = 0; t < nthreads; t++) pt::locate_thread(*geom, pts, n, chunk, eoff, nbad, t, nthreads);
  return 0;
}

extern "C" int emu_points_gather(const uint8_t* arena, const int64_t* slot, const int64_t* which, const int64_t* eoff,
                                 int64_t n, const hsds_point_seg* segs, int nsegs, int chunk_elem, int out_elem,
                                 const uint8_t* fill, uint8_t* out, const int64_t* dst_index, uint32_t nthreads) {
  pt::GatherArgs a;
  if (n < 0 || !make_segs(segs, nsegs, chunk_elem, out_elem, a.segs)) return HSDS_ERR_ARG;
  a.arena = arena;
  a.slot = slot;
  a.which = which;
  a.eoff = eoff;
  a.n = n;
  a.fill = fill;
  a.out = out;
  a.dst_index = dst_index;
  for (uint32_t t = 0; t < nthreads; t++) pt::gather_thread(a, t, nthreads);
  return 0;
}

extern "C" int emu_points_scatter(uint8_t* arena, const int64_t* slot, const int64_t* which, const int64_t* eoff,
                                  const int64_t* order, int64_t n, const hsds_point_seg* segs, int nsegs,
                                  int chunk_elem, int out_elem, const uint8_t* vals, uint32_t nthreads) {
  pt::ScatterArgs a;
  if (n < 0 || !make_segs(segs, nsegs, chunk_elem, out_elem, a.segs)) return HSDS_ERR_ARG;
  a.arena = arena;
  a.slot = slot;
  a.which = which;
  a.eoff = eoff;
  a.order = order;
  a.n = n;
  a.vals = vals;
  for (uint32_t t = 0; t < nthreads; t++) pt::scatter_thread(a, t, nthreads);
  return 0;
}
