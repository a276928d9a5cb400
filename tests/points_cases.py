"""Shared pieces of the point-selection tests (tests/test_points_golden.py,
tests/test_points_emu.py, tests/test_gpu_points.py): the reference goldens
(tests/golden/make_points_golden.py), a numpy model of the three kernels' contract
(include/hsds_amd.h hsds_points_*), random cases, and thin drivers for the CPU emulator
(tests/emu/points_emu.cpp).  Test infrastructure only."""
import ctypes
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpoints_emu.so")

# dataset / layout pairs whose chunks do not divide the extent (one of rank 8)
GEOMS = [((23,), (10,)), ((20, 11), (7, 5)), ((9, 7, 5), (4, 3, 2)),
         ((3, 2, 3, 2, 2, 3, 2, 2), (2, 1, 2, 2, 1, 2, 1, 2))]
ABC = np.dtype([("a", "<i4"), ("b", "<f4"), ("c", "S4")])
# element sizes 1, 2, 4, 8, 12, 16, 24, a padded (align=True) compound and one with an array field
DTYPES = [np.dtype("u1"), np.dtype("<i2"), np.dtype("<f4"), np.dtype("<f8"), ABC, np.dtype("<c16"),
          np.dtype([("x", "<f8"), ("y", "<i8"), ("z", "<f8")]),
          np.dtype([("u", "u1"), ("v", "<f8"), ("w", "<i2")], align=True),
          np.dtype([("k", "<i2"), ("m", "<f4", (3,))])]
COUNTS = [0, 1, 63, 64, 65, 4099]


@functools.lru_cache(maxsize=None)
def goldens():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "points_cases.json")))
    arrs = np.load(os.path.join(ROOT, "tests", "golden", "points_cases.npz"))
    return d, {k: arrs[k] for k in arrs.files}


def _tuples(descr):
    return [(e[0], _tuples(e[1]) if isinstance(e[1], list) else e[1]) + ((tuple(e[2]),) if len(e) > 2 else ())
            for e in descr]


def descr_dtype(descr):
    """a dtype from its JSON-stored numpy descr (padding entries included)"""
    if isinstance(descr, str):
        return np.dtype(descr)
    return np.lib.format.descr_to_dtype(_tuples(descr))


def golden_dtype(meta, name):
    return descr_dtype(meta["dtypes"][name])


def field_mask(dt):
    """bool per byte of an element: True where a field lives (False: padding)"""
    m = np.zeros(dt.itemsize, bool)
    if not dt.names:
        m[:] = True
        return m
    for name in dt.names:
        f, off = dt.fields[name][0], dt.fields[name][1]
        m[off:off + f.itemsize] = True
    return m


def subset_dtype(dt, fields):
    """getSubType (hdf5dtype.py:857-876): the named fields, packed, in the dataset's order"""
    return np.dtype([(f, dt.fields[f][0]) for f in dt.names if f in fields])


# ---- numpy model -----------------------------------------------------------------------
def locate_model(dims, layout, itemsize, pts):
    """(chunk linear index or -1, element byte offset, number of points outside)"""
    n = len(pts)
    dims_a, lay = np.array(dims, dtype=object), np.array(layout, dtype=object)
    grid = [-(-int(d) // int(c)) for d, c in zip(dims, layout)]
    chunk, eoff, bad = np.zeros(n, np.int64), np.zeros(n, np.int64), 0
    for i in range(n):
        p = [int(x) for x in pts[i]]
        if any(c >= d for c, d in zip(p, dims_a)):
            chunk[i], eoff[i] = -1, 0
            bad += 1
            continue
        lin = off = 0
        for d in range(len(dims)):
            lin = lin * grid[d] + p[d] // int(lay[d])
            off = off * int(lay[d]) + p[d] % int(lay[d])
        chunk[i], eoff[i] = lin, off * itemsize
    return chunk, eoff, bad


def gather_model(arena, slot, which, eoff, segs, out_elem, fill, out0, dst_index=None):
    """out0: the destination's bytes before the call (element 0 at byte 0)"""
    out = out0.copy()
    for i in range(len(eoff)):
        k = 0 if which is None else int(which[i])
        s = -1 if k < 0 else int(slot[k])
        el = np.zeros(out_elem, np.uint8)
        if s < 0:
            if fill is not None:
                el[:] = fill
        else:
            for c, o, nb in segs:
                el[o:o + nb] = arena[s + int(eoff[i]) + c:s + int(eoff[i]) + c + nb]
        pos = i if dst_index is None else int(dst_index[i])
        out[pos * out_elem:(pos + 1) * out_elem] = el
    return out


def scatter_model(arena0, slot, which, eoff, segs, out_elem, vals):
    """request order: a repeated element keeps the last value"""
    arena = arena0.copy()
    for i in range(len(eoff)):
        k = 0 if which is None else int(which[i])
        s = -1 if k < 0 else int(slot[k])
        if s < 0:
            continue
        for c, o, nb in segs:
            arena[s + int(eoff[i]) + c:s + int(eoff[i]) + c + nb] = vals[i * out_elem + o:i * out_elem + o + nb]
    return arena


def sort_order(which, eoff, chunk_bytes):
    """the caller's stable sort by (chunk, offset)"""
    w = np.zeros(len(eoff), np.int64) if which is None else np.asarray(which, np.int64)
    return np.argsort(w * np.int64(chunk_bytes) + np.asarray(eoff, np.int64), kind="stable").astype(np.int64)


# ---- random cases ------------------------------------------------------------------------
def random_case(seed, dims, layout, dt, n, fields=None, missing=True):
    """a dataset's chunks laid out in one arena (some missing: slot -1), n random points
    over all of it in random order with repeats, values to write.  Returns a dict."""
    from hsds_amd.selection import point_segments
    rng = np.random.default_rng(seed)
    grid = [-(-d // c) for d, c in zip(dims, layout)]
    nchunks = int(np.prod(grid))
    cb = int(np.prod(layout)) * dt.itemsize
    stride = (cb + 255) // 256 * 256
    perm = rng.permutation(nchunks)
    slot = (perm * stride + 256).astype(np.int64)               # chunks shuffled in the arena
    if missing and nchunks > 1:
        slot[rng.random(nchunks) < 0.25] = -1
    arena = rng.integers(0, 256, nchunks * stride + 512, dtype=np.uint8)
    pts = np.stack([rng.integers(0, d, n) for d in dims], axis=1).astype(np.uint64).reshape(n, len(dims))
    if n > 4:
        pts[rng.integers(0, n, n // 3)] = pts[rng.integers(0, n, n // 3)]   # repeats
    sdt = subset_dtype(dt, fields) if fields else None
    segs, out_dt = point_segments(dt, sdt)
    E = out_dt.itemsize
    fill = rng.integers(1, 256, E, dtype=np.uint8)
    vals = rng.integers(0, 256, n * E, dtype=np.uint8)
    return dict(dims=dims, layout=layout, dt=dt, n=n, slot=slot, arena=arena, pts=pts, segs=segs, E=E, fill=fill,
                vals=vals, chunk_bytes=cb)


# ---- emulator ------------------------------------------------------------------------------
class Emu:
    def __init__(self):
        assert os.path.exists(EMU), "build() the emulators first (tests/emu/libpoints_emu.so)"
        from hsds_amd import _native as nat
        self.nat = nat
        L = ctypes.CDLL(EMU)
        P, I, I64, U32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32
        L.emu_points_locate.argtypes = [P, P, I64, P, P, P, U32]
        L.emu_points_gather.argtypes = [P, P, P, P, I64, P, I, I, I, P, P, P, U32]
        L.emu_points_scatter.argtypes = [P, P, P, P, P, I64, P, I, I, I, P, U32]
        self.L = L

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data

    def locate(self, dims, layout, itemsize, pts, nthreads=7):
        n = len(pts)
        pts = np.ascontiguousarray(pts, np.uint64)
        chunk, eoff = np.full(n, 77, np.int64), np.full(n, 77, np.int64)
        nbad = np.zeros(1, np.int32)
        geom = self.nat.point_geom(dims, layout, itemsize)
        rc = self.L.emu_points_locate(ctypes.addressof(geom), self._p(pts), n, self._p(chunk), self._p(eoff),
                                      self._p(nbad), nthreads)
        assert rc == 0, rc
        return chunk, eoff, int(nbad[0])

    def gather(self, arena, slot, which, eoff, segs, chunk_elem, out_elem, fill, out0, dst_index=None, shift=0,
               nthreads=5):
        """`shift`: bytes from a 16-byte boundary to the output's first byte; the bytes
        around the output must come back untouched"""
        n = len(eoff)
        buf, base = aligned(len(out0) + 64, shift + 16)
        guard = buf.copy()
        buf[base:base + len(out0)] = out0
        guard[base:base + len(out0)] = 0
        eoff = np.ascontiguousarray(eoff, np.int64)
        slot = np.ascontiguousarray(slot, np.int64)
        which = None if which is None else np.ascontiguousarray(which, np.int64)
        dst_index = None if dst_index is None else np.ascontiguousarray(dst_index, np.int64)
        fill = None if fill is None else np.ascontiguousarray(fill, np.uint8)
        rc = self.L.emu_points_gather(self._p(arena), self._p(slot), self._p(which), self._p(eoff), n,
                                      self._segs(segs), len(segs), chunk_elem, out_elem, self._p(fill), buf.ctypes.data + base,
                                      self._p(dst_index), nthreads)
        if rc != 0:
            return rc
        after = buf.copy()
        after[base:base + len(out0)] = 0
        assert (after == guard).all(), "bytes outside the output were written"
        return buf[base:base + len(out0)].copy()

    def _segs(self, segs):
        self._keep = self.nat.point_segs(segs)
        return ctypes.addressof(self._keep)

    def scatter(self, arena0, slot, which, eoff, order, segs, chunk_elem, out_elem, vals, nthreads=5):
        arena = arena0.copy()
        eoff = np.ascontiguousarray(eoff, np.int64)
        slot = np.ascontiguousarray(slot, np.int64)
        which = None if which is None else np.ascontiguousarray(which, np.int64)
        order = None if order is None else np.ascontiguousarray(order, np.int64)
        vals = np.ascontiguousarray(vals, np.uint8)
        rc = self.L.emu_points_scatter(self._p(arena), self._p(slot), self._p(which), self._p(eoff), self._p(order),
                                       len(eoff), self._segs(segs), len(segs), chunk_elem, out_elem, self._p(vals),
                                       nthreads)
        if rc != 0:
            return rc
        return arena


def aligned(nbytes, shift):
    """(uint8 buffer of random bytes, index of a byte `shift` past a 16-byte boundary)"""
    buf = np.random.default_rng(nbytes).integers(0, 256, nbytes + 48, dtype=np.uint8)
    base = (-buf.ctypes.data) % 16 + shift
    return buf, base
