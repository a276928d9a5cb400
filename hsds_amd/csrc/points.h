// points.h -- point (coordinate-list) selections: the element gathers and scatters of the
// DN's POST_Chunk point read / write (hsds/util/chunkUtil.py:998-1148 chunkReadPoints /
// chunkWritePoints, one Python iteration per point there) and the SN's per-point chunk
// lookup (hsds/dset_lib.py:459-484 with chunkUtil.getChunkId, chunkUtil.py:353-371, and
// getChunkRelativePoint, chunkUtil.py:793-810), over chunks resident in the HBM cache.
//
//  locate   one thread per point: the C-order linear index of its chunk in the chunk grid
//           ceil(dims / layout) and the byte offset of its element inside the chunk array.
//           A coordinate at or past the extent (unsigned compare: no wrap for huge uint64
//           values) gives chunk index -1 and counts in a device counter.
//  gather   out element i (out_elem bytes, at out + dst_index[i] * out_elem, dst_index ==
//           NULL: i) = the selected bytes of the element at arena + slot[which[i]] + eoff[i].
//           The selection is a segment table {chunk_off, out_off, nbytes} sorted by out_off
//           (one segment: the whole element; one per field: a compound subset); bytes of the
//           output element that no segment covers are zero.  slot < 0 (no such chunk): the
//           fill pattern (out_elem bytes, NULL: zeros).
//           Contiguous output (dst_index == NULL): a lane owns one 16-byte slot of the
//           DESTINATION, assembles it in registers from the elements that overlap it
//           (elements of 12 or 24 bytes straddle slots) and stores it once; only the
//           first and last slot of the output move bytes singly.
//           Scattered output: one element per lane, the widest typed moves its alignment
//           allows (16 / 8 / 4 / 2 bytes, else bytes).
//  scatter  the write direction over the same table: the segments of value i go to the
//           chunk element, the rest of the element is left alone.  `order` holds the point
//           indices stably sorted by (which, eoff); entry j writes only if entry j + 1 has a
//           different key, so of repeated points the last request position wins, as in the
//           reference's loop, without atomics.
//
// SINGLE SOURCE for the HIP kernels (engine.hip points_*_kernel) and the CPU emulation
// (tests/emu/points_emu.cpp), which runs every thread of the grid in turn.
#pragma once
#include "region.h"

#if RG_GPU
#define PT_COUNT(p) atomicAdd((p), 1)
#define PT_BOTH __host__ __device__ inline      // also called by the host launchers
#else
#define PT_COUNT(p) (++*(p))
#define PT_BOTH static inline
#endif

namespace pt {

struct Segs {
  int32_t n;
  int32_t out_elem;
  hsds_point_seg s[HSDS_POINT_MAX_SEGS];
};

// 1 when the table is usable, else 0: 1..16 segments, sorted by out_off, not overlapping, inside the
// output element, chunk side inside the chunk element
PT_BOTH int segs_ok(const Segs& g, int chunk_elem) {
  if (g.n < 1 || g.n > HSDS_POINT_MAX_SEGS || g.out_elem < 1 || chunk_elem < 1) return 0;
  int32_t end = 0;
  for (int k = 0; k < g.n; k++) {
    const hsds_point_seg& s = g.s[k];
    if (s.nbytes < 1 || s.out_off < end || s.chunk_off < 0) return 0;
    if ((int64_t)s.out_off + s.nbytes > g.out_elem || (int64_t)s.chunk_off + s.nbytes > chunk_elem) return 0;
    end = s.out_off + s.nbytes;
  }
  return 1;
}

// ---- locate -------------------------------------------------------------------
RG_HD void locate_point(const hsds_point_geom& g, const uint64_t* p, int64_t* chunk, int64_t* eoff, int32_t* nbad) {
  uint64_t lin = 0, off = 0;
  bool bad = false;
  for (int d = 0; d < g.rank; d++) {
    const uint64_t c = p[d], n = g.dims[d], l = g.layout[d];
    if (c >= n) { bad = true; break; }
    uint64_t ci, rel;
    if (!((c | l) >> 32)) {
      ci = (uint32_t)c / (uint32_t)l;
      rel = (uint32_t)c - (uint32_t)ci * (uint32_t)l;
    } else {
      ci = c / l;
      rel = c - ci * l;
    }
    const uint64_t grid = (n + l - 1) / l;
    lin = lin * grid + ci;
    off = off * l + rel;
  }
  if (bad) {
    *chunk = -1;
    *eoff = 0;
    PT_COUNT(nbad);
  } else {
    *chunk = (int64_t)lin;
    *eoff = (int64_t)(off * (uint64_t)g.itemsize);
  }
}

// thread t of T
RG_HD void locate_thread(const hsds_point_geom& g, const uint64_t* pts, int64_t n, int64_t* chunk, int64_t* eoff,
                         int32_t* nbad, uint64_t t, uint64_t T) {
  for (uint64_t i = t; i < (uint64_t)n; i += T) locate_point(g, pts + i * (uint64_t)g.rank, chunk + i, eoff + i, nbad);
}

// ---- moves ----------------------------------------------------------------------
// n bytes s -> d by the widest unit that the addresses and the length are all multiples of
RG_HD void move_bytes(const uint8_t* s, uint8_t* d, int32_t n) {
  const uintptr_t a = (uintptr_t)s | (uintptr_t)d | (uintptr_t)(uint32_t)n;
  if (!(a & 15u)) { for (int32_t b = 0; b < n; b += 16) *(rg_v4*)(d + b) = *(const rg_v4*)(s + b); return; }
  if (!(a & 7u)) { for (int32_t b = 0; b < n; b += 8) *(uint64_t*)(d + b) = *(const uint64_t*)(s + b); return; }
  if (!(a & 3u)) { for (int32_t b = 0; b < n; b += 4) *(uint32_t*)(d + b) = *(const uint32_t*)(s + b); return; }
  if (!(a & 1u)) { for (int32_t b = 0; b < n; b += 2) *(uint16_t*)(d + b) = *(const uint16_t*)(s + b); return; }
  for (int32_t b = 0; b < n; b++) d[b] = s[b];
}

RG_HD void zero_bytes(uint8_t* d, int32_t n) {
  const uintptr_t a = (uintptr_t)d | (uintptr_t)(uint32_t)n;
  if (!(a & 7u)) { for (int32_t b = 0; b < n; b += 8) *(uint64_t*)(d + b) = 0; return; }
  if (!(a & 3u)) { for (int32_t b = 0; b < n; b += 4) *(uint32_t*)(d + b) = 0; return; }
  for (int32_t b = 0; b < n; b++) d[b] = 0;
}

struct GatherArgs {
  const uint8_t* arena;
  const int64_t* slot;       // byte offset of chunk k's array in arena, < 0: no such chunk
  const int64_t* which;      // per point: index into slot (NULL: 0; < 0: no such chunk)
  const int64_t* eoff;       // per point: byte offset of the element in its chunk
  int64_t n;
  const uint8_t* fill;       // out_elem bytes (NULL: zeros)
  uint8_t* out;
  const int64_t* dst_index;  // NULL: contiguous output
  Segs segs;
};

// source of point i: the chunk element (whole = 0) or the fill pattern (whole = 1: a plain
// run of out_elem bytes; NULL: zeros)
RG_HD const uint8_t* point_src(const GatherArgs& a, uint64_t i, int& whole) {
  const int64_t k = a.which ? a.which[i] : 0;
  const int64_t s = k < 0 ? -1 : a.slot[k];
  if (s < 0) { whole = 1; return a.fill; }
  whole = 0;
  return a.arena + s + a.eoff[i];
}

// bytes [b0, b1) of an output element, from `base` through the table (or as a plain run),
// into the 16-byte register pair at byte position p
RG_HD void fetch_range(const uint8_t* base, const Segs& g, int whole, int32_t b0, int32_t b1, uint32_t p, uint64_t& lo,
                       uint64_t& hi) {
  if (!base) return;
  const int nk = whole ? 1 : g.n;
  for (int k = 0; k < nk; k++) {
    const int32_t oo = whole ? 0 : g.s[k].out_off, co = whole ? 0 : g.s[k].chunk_off;
    const int32_t nb = whole ? g.out_elem : g.s[k].nbytes;
    const int32_t x0 = b0 > oo ? b0 : oo, x1 = b1 < oo + nb ? b1 : oo + nb;
    if (x0 >= x1) continue;
    const uint8_t* s = base + co + (x0 - oo);
    uint32_t q = p + (uint32_t)(x0 - b0);
    int32_t left = x1 - x0;
    while (left > 0) {
      uint64_t v;
      uint32_t w;
      if (left >= 4 && !(q & 3u) && !((uintptr_t)s & 3u)) { v = *(const uint32_t*)s; w = 4; }
      else { v = *s; w = 1; }
      if (q < 8u) lo |= v << (8u * q); else hi |= v << (8u * (q - 8u));
      s += w; q += w; left -= (int32_t)w;
    }
  }
}

// unit u of the gather: a destination slot (contiguous output) or a point
PT_BOTH uint64_t gather_units(const GatherArgs& a) {
  if (a.n <= 0) return 0;
  if (a.dst_index) return (uint64_t)a.n;
  const uintptr_t d0 = (uintptr_t)a.out, dend = d0 + (uintptr_t)a.n * (uintptr_t)a.segs.out_elem;
  return (uint64_t)((dend - (d0 & ~(uintptr_t)15) + 15u) >> 4);
}

RG_HD void gather_unit(const GatherArgs& a, uint64_t u) {
  const Segs& g = a.segs;
  const int32_t E = g.out_elem;
  const bool plain = g.n == 1 && g.s[0].out_off == 0 && g.s[0].chunk_off == 0 && g.s[0].nbytes == E;
  if (a.dst_index) {
    int whole;
    const uint8_t* s = point_src(a, u, whole);
    uint8_t* d = a.out + a.dst_index[u] * (int64_t)E;
    if (!s) { zero_bytes(d, E); return; }
    if (whole || plain) { move_bytes(s, d, E); return; }
    int32_t end = 0;
    for (int k = 0; k < g.n; k++) {
      if (g.s[k].out_off > end) zero_bytes(d + end, g.s[k].out_off - end);
      move_bytes(s + g.s[k].chunk_off, d + g.s[k].out_off, g.s[k].nbytes);
      end = g.s[k].out_off + g.s[k].nbytes;
    }
    if (end < E) zero_bytes(d + end, E - end);
    return;
  }
  const uintptr_t d0 = (uintptr_t)a.out, dend = d0 + (uintptr_t)a.n * (uintptr_t)E;
  const uintptr_t x0 = (d0 & ~(uintptr_t)15) + 16u * (uintptr_t)u;
  const uintptr_t xl = x0 > d0 ? x0 : d0, xh = x0 + 16u < dend ? x0 + 16u : dend;
  const bool full = xl == x0 && xh == x0 + 16u;
  uint64_t lo = 0, hi = 0;
  if (full && plain && (E == 1 || E == 2 || E == 4 || E == 8) && !(d0 & (uintptr_t)(E - 1))) {
    // 16 / E whole elements, one typed load each
    const uint64_t e0 = (uint64_t)((x0 - d0) / (uintptr_t)E);
    const uint32_t G = 16u / (uint32_t)E;
    for (uint32_t k = 0; k < G; k++) {
      int whole;
      const uint8_t* s = point_src(a, e0 + k, whole);
      const uint64_t x = s ? rg::load_elem(s, E) : 0;
      const uint32_t bit = k * (uint32_t)E * 8u;
      if (bit < 64u) lo |= x << bit; else hi |= x << (bit - 64u);
    }
    *(rg_v4*)x0 = RG_V4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    return;
  }
  if (full && plain && !(E & 15) && !(d0 & 15u)) {
    // the slot lies inside one element: one 16-byte load (aligned dwords and funnel shifts
    // when the source is not 16-aligned)
    const uint64_t e = (uint64_t)((x0 - d0) / (uintptr_t)E);
    const int32_t b = (int32_t)((x0 - d0) - (uintptr_t)e * (uintptr_t)E);
    int whole;
    const uint8_t* s = point_src(a, e, whole);
    *(rg_v4*)x0 = s ? rg::load16_any(s + b) : RG_V4(0u, 0u, 0u, 0u);
    return;
  }
  uint64_t e = (uint64_t)((xl - d0) / (uintptr_t)E);
  int32_t b = (int32_t)((xl - d0) - (uintptr_t)e * (uintptr_t)E);
  for (uintptr_t x = xl; x < xh; e++, b = 0) {
    const int32_t take = (int32_t)(xh - x) < E - b ? (int32_t)(xh - x) : E - b;
    int whole;
    const uint8_t* s = point_src(a, e, whole);
    fetch_range(s, g, whole, b, b + take, (uint32_t)(x - x0), lo, hi);
    x += (uintptr_t)take;
  }
  if (full) {
    *(rg_v4*)x0 = RG_V4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
  } else {
    for (uintptr_t x = xl; x < xh; x++) {
      const uint32_t q = (uint32_t)(x - x0);
      *(uint8_t*)x = (uint8_t)(q < 8u ? lo >> (8u * q) : hi >> (8u * (q - 8u)));
    }
  }
}

RG_HD void gather_thread(const GatherArgs& a, uint64_t t, uint64_t T) {
  const uint64_t nu = gather_units(a);
  for (uint64_t u = t; u < nu; u += T) gather_unit(a, u);
}

// ---- scatter --------------------------------------------------------------------
struct ScatterArgs {
  uint8_t* arena;
  const int64_t* slot;
  const int64_t* which;      // NULL: 0
  const int64_t* eoff;
  const int64_t* order;      // point indices stably sorted by (which, eoff); NULL: 0 .. n-1
  int64_t n;
  const uint8_t* vals;       // value i at vals + i * out_elem, laid out as the table's out side
  Segs segs;
};

RG_HD void scatter_entry(const ScatterArgs& a, uint64_t j) {
  const uint64_t i = a.order ? (uint64_t)a.order[j] : j;
  const int64_t k = a.which ? a.which[i] : 0;
  if (j + 1 < (uint64_t)a.n) {
    const uint64_t i2 = a.order ? (uint64_t)a.order[j + 1] : j + 1;
    const int64_t k2 = a.which ? a.which[i2] : 0;
    if (k2 == k && a.eoff[i2] == a.eoff[i]) return;      // a later request writes this element
  }
  const int64_t s = k < 0 ? -1 : a.slot[k];
  if (s < 0) return;
  uint8_t* d = a.arena + s + a.eoff[i];
  const uint8_t* v = a.vals + i * (uint64_t)a.segs.out_elem;
  for (int q = 0; q < a.segs.n; q++) move_bytes(v + a.segs.s[q].out_off, d + a.segs.s[q].chunk_off, a.segs.s[q].nbytes);
}

RG_HD void scatter_thread(const ScatterArgs& a, uint64_t t, uint64_t T) {
  for (uint64_t j = t; j < (uint64_t)a.n; j += T) scatter_entry(a, j);
}

}  // namespace pt
