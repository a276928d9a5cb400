// query.h -- where-clause queries over 1-D compound datasets: the row filter, ordered
// compaction and in-place update of the DN's GET_Chunk / PUT_Chunk with query=
// (hsds/chunk_dn.py:192-240 -> chunkUtil.chunkQuery, hsds/util/chunkUtil.py:1375-1569, one
// numpy eval of a string per chunk there), over all of a request's chunks resident in the HBM
// cache.
//
//  program  the predicate, compiled on the host (hsds_amd/query.py) to at most 32 postfix ops
//           over a stack of bits held in one 32-bit register: CMP (field against a constant),
//           CMP_FIELD (field against field), CMP_BYTES (an S<n> field against a bytes constant
//           in the program's pool, or another S field; numpy's order: bytes compared as if
//           padded with NULs), ISIN (binary search of sorted elements in a device buffer),
//           CONST, AND, OR.  Numbers compare in one of three domains (int64, uint64, double)
//           that the host chose as numpy would; a signed field against a uint64 field
//           compares exactly, as numpy's mixed int64 / uint64 loops do.
//  mask     one lane per selected row, each chunk's rows padded to whole 64-row words: the
//           wave's ballot is the word's 64-bit mask, its popcount the word's count.
//  emit     (after an exclusive scan of the counts) one lane per row: a matching row's rank is
//           base[word] + popcount(mask below the lane); a rank under the limit optionally
//           stores the update record's segments into the row, then writes response record
//           `rank`: the uint64 dataset index and the row's selected segments.
// Neither pass waits on another workgroup: the order comes from the scan alone.
//
// SINGLE SOURCE for the HIP kernels (engine.hip query_*_kernel) and the CPU emulation
// (tests/emu/query_emu.cpp), which runs every lane of every word in turn.
#pragma once
#include "points.h"

namespace qy {

// ---- loads safe at any alignment (a 14-byte record puts an f4 at offset 2) ------------
RG_HD uint64_t load_any(const uint8_t* p, int n) {
  const uintptr_t a = (uintptr_t)p;
  if (!(a & (uintptr_t)(n - 1))) {
    switch (n) {
      case 1: return *p;
      case 2: return *(const uint16_t*)p;
      case 4: return *(const uint32_t*)p;
      default: return *(const uint64_t*)p;
    }
  }
  if (n == 8 && !(a & 3u)) return (uint64_t)*(const uint32_t*)p | ((uint64_t)*(const uint32_t*)(p + 4) << 32);
  if (!(a & 1u)) {
    uint64_t v = 0;
    for (int b = 0; b < n; b += 2) v |= (uint64_t)*(const uint16_t*)(p + b) << (8 * b);
    return v;
  }
  uint64_t v = 0;
  for (int b = 0; b < n; b++) v |= (uint64_t)p[b] << (8 * b);
  return v;
}

RG_HD void store_u64_any(uint8_t* p, uint64_t v) {
  const uintptr_t a = (uintptr_t)p;
  if (!(a & 7u)) { *(uint64_t*)p = v; return; }
  if (!(a & 3u)) { *(uint32_t*)p = (uint32_t)v; *(uint32_t*)(p + 4) = (uint32_t)(v >> 32); return; }
  for (int b = 0; b < 8; b++) p[b] = (uint8_t)(v >> (8 * b));
}

PT_BOTH int kind_size(int kind) { return kind < 8 ? 1 << (kind & 3) : kind == HSDS_Q_KIND_F4 ? 4 : 8; }

RG_HD double bits_f64(uint64_t b) { double d; __builtin_memcpy(&d, &b, 8); return d; }
RG_HD float bits_f32(uint32_t b) { float f; __builtin_memcpy(&f, &b, 4); return f; }

// the field's value as a sign-extended (signed kinds) or zero-extended 64-bit integer
RG_HD int64_t field_int(const uint8_t* p, int kind) {
  const uint64_t raw = load_any(p, kind_size(kind));
  switch (kind) {
    case 0: return (int8_t)raw;
    case 1: return (int16_t)raw;
    case 2: return (int32_t)raw;
    default: return (int64_t)raw;
  }
}

RG_HD double field_f64(const uint8_t* p, int kind) {
  if (kind == HSDS_Q_KIND_F8) return bits_f64(load_any(p, 8));
  if (kind == HSDS_Q_KIND_F4) return (double)bits_f32((uint32_t)load_any(p, 4));
  if (kind >= 4) return (double)load_any(p, kind_size(kind));
  return (double)field_int(p, kind);
}

template <class T> RG_HD int rel(int cmp, T a, T b) {
  switch (cmp) {
    case HSDS_Q_EQ: return a == b;
    case HSDS_Q_NE: return a != b;
    case HSDS_Q_LT: return a < b;
    case HSDS_Q_LE: return a <= b;
    case HSDS_Q_GT: return a > b;
    default: return a >= b;
  }
}

// -1 / 0 / 1: a[0, la) against b[0, lb), the shorter one continued with NULs
RG_HD int bytes_order(const uint8_t* a, int la, const uint8_t* b, int lb) {
  const int L = la > lb ? la : lb;
  for (int k = 0; k < L; k++) {
    const int x = k < la ? a[k] : 0, y = k < lb ? b[k] : 0;
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

// the same with b = the program's constant at pool[off, off + lb): read by index from the
// by-value program (no pointer into it, so it stays in the kernel-argument segment)
RG_HD int bytes_order_pool(const uint8_t* a, int la, const hsds_query_prog& g, int off, int lb) {
  const int L = la > lb ? la : lb;
  for (int k = 0; k < L; k++) {
    const int x = k < la ? a[k] : 0, y = k < lb ? g.pool[off + k] : 0;
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

RG_HD int isin(const hsds_query_op& o, const uint8_t* row, const uint8_t* elems) {
  const uint8_t* p = row + o.off;
  const uint8_t* e = elems + o.off_b;
  int64_t lo = 0, hi = (int64_t)o.imm;        // first element >= the value
  if (o.kind == HSDS_Q_KIND_S) {
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (bytes_order(e + mid * o.len, o.len, p, o.len) < 0) lo = mid + 1; else hi = mid;
    }
    return lo < (int64_t)o.imm && bytes_order(e + lo * o.len, o.len, p, o.len) == 0;
  }
  if (o.dom == HSDS_Q_DOM_F64) {
    const double v = field_f64(p, o.kind);
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (bits_f64(load_any(e + mid * 8, 8)) < v) lo = mid + 1; else hi = mid;
    }
    return lo < (int64_t)o.imm && bits_f64(load_any(e + lo * 8, 8)) == v;     // NaN: never
  }
  if (o.dom == HSDS_Q_DOM_U64) {
    const uint64_t v = (uint64_t)field_int(p, o.kind);
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (load_any(e + mid * 8, 8) < v) lo = mid + 1; else hi = mid;
    }
    return lo < (int64_t)o.imm && load_any(e + lo * 8, 8) == v;
  }
  const int64_t v = field_int(p, o.kind);
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)load_any(e + mid * 8, 8) < v) lo = mid + 1; else hi = mid;
  }
  return lo < (int64_t)o.imm && (int64_t)load_any(e + lo * 8, 8) == v;
}

// the program on one row: 1 when the row matches
RG_HD int eval_row(const hsds_query_prog& g, const uint8_t* row, const uint8_t* elems) {
  uint32_t st = 0;
  for (int k = 0; k < g.nops; k++) {
    const hsds_query_op o = g.ops[k];
    uint32_t b;
    switch (o.op) {
      case HSDS_Q_CONST: b = (uint32_t)(o.imm & 1u); break;
      case HSDS_Q_CMP:
        if (o.dom == HSDS_Q_DOM_F64) b = rel<double>(o.cmp, field_f64(row + o.off, o.kind), bits_f64(o.imm));
        else if (o.dom == HSDS_Q_DOM_U64) b = rel<uint64_t>(o.cmp, (uint64_t)field_int(row + o.off, o.kind), o.imm);
        else b = rel<int64_t>(o.cmp, field_int(row + o.off, o.kind), (int64_t)o.imm);
        break;
      case HSDS_Q_CMP_FIELD:
        if (o.dom == HSDS_Q_DOM_F64)
          b = rel<double>(o.cmp, field_f64(row + o.off, o.kind), field_f64(row + o.off_b, o.kind_b));
        else if (o.dom == HSDS_Q_DOM_U64)
          b = rel<uint64_t>(o.cmp, (uint64_t)field_int(row + o.off, o.kind), (uint64_t)field_int(row + o.off_b, o.kind_b));
        else if (o.dom == HSDS_Q_DOM_SU) {
          // signed against unsigned, exact: a negative A is below every B
          const int64_t x = field_int(row + o.off, o.kind);
          const uint64_t y = (uint64_t)field_int(row + o.off_b, o.kind_b);
          b = x < 0 ? rel<int>(o.cmp, -1, 0) : rel<uint64_t>(o.cmp, (uint64_t)x, y);
        }
        else b = rel<int64_t>(o.cmp, field_int(row + o.off, o.kind), field_int(row + o.off_b, o.kind_b));
        break;
      case HSDS_Q_CMP_BYTES:
        b = rel<int>(o.cmp, o.kind_b ? bytes_order(row + o.off, o.len, row + o.off_b, o.len_b)
                                     : bytes_order_pool(row + o.off, o.len, g, o.off_b, o.len_b), 0);
        break;
      case HSDS_Q_ISIN: b = (uint32_t)isin(o, row, elems); break;
      case HSDS_Q_AND: b = st & (st >> 1) & 1u; st >>= 2; break;
      default: b = (st | (st >> 1)) & 1u; st >>= 2; break;
    }
    st = (st << 1) | (b & 1u);
  }
  return (int)(st & 1u);
}

// 1 when the program is usable on rows of `rowsize` bytes with `isin_bytes` of elements:
// 1..32 ops, a stack that never underflows or passes 32 bits and ends with one bit, every
// read inside the row, the pool or the element buffer
PT_BOTH int prog_ok(const hsds_query_prog& g, int rowsize, int64_t isin_bytes) {
  if (g.nops < 1 || g.nops > HSDS_QUERY_MAX_OPS || rowsize < 1) return 0;
  int depth = 0;
  for (int k = 0; k < g.nops; k++) {
    const hsds_query_op& o = g.ops[k];
    if (o.op == HSDS_Q_AND || o.op == HSDS_Q_OR) {
      if (depth < 2) return 0;
      depth--;
      continue;
    }
    if (o.op > HSDS_Q_OR) return 0;
    if (++depth > 32) return 0;
    if (o.op == HSDS_Q_CONST) continue;
    if (o.cmp > HSDS_Q_GE || o.off < 0) return 0;
    const int is_s = o.kind == HSDS_Q_KIND_S;
    if (o.kind > HSDS_Q_KIND_S) return 0;
    const int64_t wa = is_s ? o.len : kind_size(o.kind);
    if (wa < 1 || (int64_t)o.off + wa > rowsize) return 0;
    if (o.op == HSDS_Q_CMP_BYTES) {
      if (!is_s || o.off_b < 0 || o.len_b < 0) return 0;
      if ((int64_t)o.off_b + o.len_b > (o.kind_b ? rowsize : HSDS_QUERY_POOL)) return 0;
    } else if (o.op == HSDS_Q_ISIN) {
      if (o.imm < 1 || o.imm > HSDS_QUERY_MAX_ISIN || o.off_b < 0) return 0;
      if (!is_s && o.dom > HSDS_Q_DOM_F64) return 0;
      if ((int64_t)o.off_b + (int64_t)o.imm * (is_s ? wa : 8) > isin_bytes) return 0;
    } else {
      if (is_s || o.dom > (o.op == HSDS_Q_CMP_FIELD ? HSDS_Q_DOM_SU : HSDS_Q_DOM_F64)) return 0;
      if (o.op == HSDS_Q_CMP_FIELD) {
        if (o.dom == HSDS_Q_DOM_SU && (o.kind > 3 || o.kind_b < 4 || o.kind_b > 7)) return 0;
        if (o.kind_b >= HSDS_Q_KIND_S || o.off_b < 0 || (int64_t)o.off_b + kind_size(o.kind_b) > rowsize) return 0;
      }
    }
  }
  return depth == 1;
}

// the chunk that owns mask word w: the last one with word0 <= w
RG_HD int64_t find_chunk(const hsds_query_chunk* t, int64_t n, int64_t w) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (t[mid].word0 <= w) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- mask -----------------------------------------------------------------------------
struct MaskArgs {
  const uint8_t* arena;
  const hsds_query_chunk* chunks;
  int64_t nchunks;
  int64_t nwords;
  int32_t rowsize;
  const uint8_t* isin;
  uint64_t* mask;
  int32_t* count;
  hsds_query_prog prog;
};

RG_HD int mask_row(const MaskArgs& a, const hsds_query_chunk& c, int64_t w, uint32_t lane) {
  const int64_t i = (w - c.word0) * 64 + lane;
  if (c.slot < 0 || i >= c.count) return 0;
  return eval_row(a.prog, a.arena + c.slot + (c.first + i * c.step) * (int64_t)a.rowsize, a.isin);
}

// word w; on the GPU every lane of the wave calls it with its lane number, the emulation
// calls it once
RG_HD void mask_word(const MaskArgs& a, int64_t w, uint32_t lane) {
  const hsds_query_chunk c = a.chunks[find_chunk(a.chunks, a.nchunks, w)];
#if RG_GPU
  const uint64_t m = __ballot(mask_row(a, c, w, lane));
  if (lane == 0) {
    a.mask[w] = m;
    a.count[w] = (int32_t)__popcll(m);
  }
#else
  uint64_t m = 0;
  for (uint32_t l = 0; l < 64; l++) m |= (uint64_t)mask_row(a, c, w, l) << l;
  a.mask[w] = m;
  a.count[w] = (int32_t)__builtin_popcountll(m);
  (void)lane;
#endif
}

// ---- emit -----------------------------------------------------------------------------
struct EmitArgs {
  uint8_t* arena;
  const hsds_query_chunk* chunks;
  int64_t nchunks;
  int64_t nwords;
  int32_t rowsize;
  const uint64_t* mask;
  const int64_t* base;       // exclusive scan of the word counts
  int64_t limit;             // 0: none
  uint8_t* out;
  const uint8_t* upd;        // the update record (NULL: read only)
  pt::Segs segs;             // row -> response record (out_off >= 8)
  pt::Segs upd_segs;         // update record -> row
};

// lane `lane` of word w
RG_HD void emit_row(const EmitArgs& a, int64_t w, uint32_t lane) {
  const uint64_t m = a.mask[w];
  if (!((m >> lane) & 1u)) return;
#if RG_GPU
  const int below = (int)__popcll(m & (((uint64_t)1 << lane) - 1u));
#else
  const int below = __builtin_popcountll(m & (((uint64_t)1 << lane) - 1u));
#endif
  const int64_t r = a.base[w] + below;
  if (a.limit > 0 && r >= a.limit) return;
  const hsds_query_chunk c = a.chunks[find_chunk(a.chunks, a.nchunks, w)];
  const int64_t i = (w - c.word0) * 64 + lane;
  if (c.slot < 0 || i >= c.count) return;
  const int64_t rowno = c.first + i * c.step;
  uint8_t* row = a.arena + c.slot + rowno * (int64_t)a.rowsize;
  if (a.upd)
    for (int q = 0; q < a.upd_segs.n; q++)
      pt::move_bytes(a.upd + a.upd_segs.s[q].out_off, row + a.upd_segs.s[q].chunk_off, a.upd_segs.s[q].nbytes);
  uint8_t* d = a.out + r * (int64_t)a.segs.out_elem;
  store_u64_any(d, (uint64_t)(c.index0 + rowno));
  int32_t end = 8;
  for (int q = 0; q < a.segs.n; q++) {
    const hsds_point_seg& s = a.segs.s[q];
    if (s.out_off > end) pt::zero_bytes(d + end, s.out_off - end);
    pt::move_bytes(row + s.chunk_off, d + s.out_off, s.nbytes);
    end = s.out_off + s.nbytes;
  }
  if (end < a.segs.out_elem) pt::zero_bytes(d + end, a.segs.out_elem - end);
}

}  // namespace qy
