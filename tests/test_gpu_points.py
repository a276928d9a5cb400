"""GPU parity of point selections: the HIP kernels behind hsds_points_locate / _gather /
_scatter bit for bit against the reference's goldens and the numpy model (the same cases as
the CPU emulation tests), hsds_amd.selection.chunkReadPoints / chunkWritePoints,
ChunkStore.get_points / put_points over a store whose fetch serves oracle-encoded objects
(as in tests/test_gpu_write.py), and the sharded point read / write over three simulated
ranks, one of which owns no chunk."""
import numpy as np
import pytest

import points_cases as pc

pytestmark = pytest.mark.gpu
DSET = "d-9e8d7c6b-5a4f3e2d-1c0b-9a8f7e-6d5c4b"
META, ARRS = pc.goldens()


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def eng(dev):
    from hsds_amd.engine import ChunkEngine
    return ChunkEngine(dev.index)


def _t(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).to(dev)


def _out_at(dev, out0, shift):
    """a device copy of out0 whose first byte is `shift` past a 16-byte boundary, inside a
    larger buffer: returns (buffer, view)"""
    import torch
    buf = torch.full((len(out0) + 64,), 0x77, dtype=torch.uint8, device=dev)
    base = (-buf.data_ptr()) % 16 + 16 + shift
    view = buf[base:base + len(out0)]
    view.copy_(torch.from_numpy(out0.copy()))
    return buf, view, base


def _gather(eng, dev, arena, slot, which, eoff, segs, chunk_elem, E, fill, out0, dst_index=None, shift=0):
    buf, view, base = _out_at(dev, out0, shift)
    eng.gather_points(_t(arena, dev), _t(np.asarray(slot, np.int64), dev), None if which is None else _t(which, dev),
                      _t(eoff, dev), segs, chunk_elem, E, view, fill=None if fill is None else _t(fill, dev),
                      dst_index=None if dst_index is None else _t(np.asarray(dst_index, np.int64), dev), n=len(eoff))
    host = buf.cpu().numpy()
    assert (host[:base] == 0x77).all() and (host[base + len(out0):] == 0x77).all(), "bytes outside the output written"
    return host[base:base + len(out0)]


def _scatter(eng, dev, arena, slot, which, eoff, segs, chunk_elem, E, vals, chunk_bytes):
    import torch
    d_arena = _t(arena, dev)
    d_which = None if which is None else _t(which, dev)
    d_eoff = _t(eoff, dev)
    key = d_eoff if d_which is None else d_which * int(chunk_bytes) + d_eoff
    order = torch.sort(key, stable=True)[1]
    eng.scatter_points(d_arena, _t(np.asarray(slot, np.int64), dev), d_which, d_eoff, order, segs, chunk_elem, E,
                       _t(vals, dev), n=len(eoff))
    return d_arena.cpu().numpy()


def _locate(eng, dev, dims, layout, itemsize, pts):
    chunk, eoff, nbad = eng.locate_points(_t(pts.reshape(-1, len(dims)), dev), dims, layout, itemsize)
    return chunk.cpu().numpy(), eoff.cpu().numpy(), int(nbad.item())


# ---- kernel parity ---------------------------------------------------------------------
@pytest.mark.parametrize("case", META["locate"], ids=lambda c: c["name"])
def test_locate_matches_getChunkId(eng, dev, case):
    dims, layout = META["geoms"][case["geom"]]
    pts, idx = ARRS[case["name"] + "__pts"], ARRS[case["name"] + "__idx"]
    chunk, eoff, nbad = _locate(eng, dev, dims, layout, 4, pts)
    grid = [-(-d // c) for d, c in zip(dims, layout)]
    assert nbad == 0
    assert (np.stack(np.unravel_index(chunk, grid), axis=1) == idx).all()
    mc, me, _ = pc.locate_model(dims, layout, 4, pts)
    assert (eoff == me).all()


def test_locate_out_of_extent_is_unsigned(eng, dev):
    dims, layout = (20, 11), (7, 5)
    pts = np.array([[0, 0], [19, 10], [20, 0], [0, 11], [2 ** 63, 0], [3, 2 ** 64 - 1], [2 ** 63 + 5, 2 ** 63 + 3],
                    [2 ** 32 + 3, 1], [7, 5]], np.uint64)
    chunk, eoff, nbad = _locate(eng, dev, dims, layout, 8, pts)
    mc, me, mb = pc.locate_model(dims, layout, 8, pts)
    assert nbad == mb == 6 and (chunk == mc).all() and (eoff == me).all()
    dims, layout = (2 ** 40, 2 ** 33 + 7), (2 ** 20 + 3, 2 ** 32 + 1)
    pts = np.array([[2 ** 40 - 1, 2 ** 33 + 6], [12345678901, 2 ** 32], [5, 2 ** 32 + 1], [2 ** 40, 0]], np.uint64)
    chunk, eoff, nbad = _locate(eng, dev, dims, layout, 1, pts)
    mc, me, mb = pc.locate_model(dims, layout, 1, pts)
    assert nbad == mb == 1 and (chunk == mc).all() and (eoff == me).all()


def _golden_setup(eng, dev, case):
    from hsds_amd.selection import point_segments
    dims, layout = META["geoms"][case["geom"]]
    dt = pc.golden_dtype(META, case["dtype"])
    sdt = pc.descr_dtype(case["select_descr"]) if case["fields"] else None
    segs, out_dt = point_segments(dt, sdt)
    pts = ARRS[case["name"] + "__pts"].reshape(-1, len(dims))
    chunk, eoff, nbad = _locate(eng, dev, dims, layout, dt.itemsize, pts)
    grid = [-(-d // c) for d, c in zip(dims, layout)]
    assert nbad == 0 and (chunk == np.ravel_multi_index(case["chunk_index"], grid)).all()
    return dt, out_dt, segs, eoff


@pytest.mark.parametrize("case", META["read"], ids=lambda c: c["name"])
def test_gather_matches_chunkReadPoints(eng, dev, case):
    dt, out_dt, segs, eoff = _golden_setup(eng, dev, case)
    want, chunk = ARRS[case["name"] + "__out"], ARRS[case["name"] + "__chunk"]
    out0 = np.full(want.size, 0xA5, np.uint8)
    for shift in (0, 4):
        got = _gather(eng, dev, chunk, [0], None, eoff, segs, dt.itemsize, out_dt.itemsize, None, out0, shift=shift)
        assert (got == want).all(), (case["name"], shift)
    got = _gather(eng, dev, chunk, [0], None, eoff, segs, dt.itemsize, out_dt.itemsize, None, out0,
                  dst_index=np.arange(case["n"]), shift=4)
    assert (got == want).all(), case["name"]


def _prefix(case):
    dt = pc.golden_dtype(META, case["dtype"])
    return not case["fields"] or list(dt.names[:len(case["fields"])]) == list(case["fields"])


@pytest.mark.parametrize("case", [c for c in META["write"] if _prefix(c)], ids=lambda c: c["name"])
def test_scatter_matches_chunkWritePoints(eng, dev, case):
    dt, val_dt, segs, eoff = _golden_setup(eng, dev, case)
    chunk0, want, vals = (ARRS[case["name"] + k] for k in ("__chunk", "__out", "__vals"))
    got = _scatter(eng, dev, chunk0, [0], None, eoff, segs, dt.itemsize, val_dt.itemsize, vals, chunk0.size)
    mask = np.tile(pc.field_mask(dt), chunk0.size // dt.itemsize)
    assert (got[mask] == want[mask]).all(), case["name"]
    assert (got[~mask] == chunk0[~mask]).all(), "padding bytes of the chunk were written"


RANDOM = [(1, 2, 4099), (0, 4, 65), (2, 6, 4099), (3, 0, 64), (1, 7, 63), (2, 8, 65), (1, 5, 4099), (0, 1, 1),
          (1, 3, 0), (3, 4, 4099)]


@pytest.mark.parametrize("gi,di,n", RANDOM)
def test_random_points_match_the_model(eng, dev, gi, di, n):
    dims, layout = pc.GEOMS[gi]
    dt = pc.DTYPES[di]
    c = pc.random_case(1000 * gi + 10 * di + n, dims, layout, dt, n)
    which, eoff, nbad = _locate(eng, dev, dims, layout, dt.itemsize, c["pts"])
    mc, me, _ = pc.locate_model(dims, layout, dt.itemsize, c["pts"])
    assert nbad == 0 and (which == mc).all() and (eoff == me).all()
    E, segs = c["E"], c["segs"]
    out0 = np.full(n * E, 0x5A, np.uint8)
    for shift, fill in ((0, c["fill"]), (4, None)):
        got = _gather(eng, dev, c["arena"], c["slot"], which, eoff, segs, dt.itemsize, E, fill, out0, shift=shift)
        assert (got == pc.gather_model(c["arena"], c["slot"], which, eoff, segs, E, fill, out0)).all(), shift
    rng = np.random.default_rng(n)
    dst_index = rng.permutation(n + 5)[:n]
    big = rng.integers(0, 256, (n + 5) * E, dtype=np.uint8)
    got = _gather(eng, dev, c["arena"], c["slot"], which, eoff, segs, dt.itemsize, E, c["fill"], big,
                  dst_index=dst_index, shift=4)
    assert (got == pc.gather_model(c["arena"], c["slot"], which, eoff, segs, E, c["fill"], big, dst_index)).all()
    got = _scatter(eng, dev, c["arena"], c["slot"], which, eoff, segs, dt.itemsize, E, c["vals"], c["chunk_bytes"])
    assert (got == pc.scatter_model(c["arena"], c["slot"], which, eoff, segs, E, c["vals"])).all()


@pytest.mark.parametrize("fields", [["a"], ["a", "b"], ["b", "c"], ["c"]])
def test_field_subsets_match_the_model(eng, dev, fields):
    dims, layout = pc.GEOMS[1]
    c = pc.random_case(7 + len(fields), dims, layout, pc.ABC, 65, fields=fields)
    which, eoff, _ = _locate(eng, dev, dims, layout, 12, c["pts"])
    E, segs = c["E"], c["segs"]
    out0 = np.full(65 * E, 0x33, np.uint8)
    for shift in (0, 4):
        got = _gather(eng, dev, c["arena"], c["slot"], which, eoff, segs, 12, E, c["fill"], out0, shift=shift)
        assert (got == pc.gather_model(c["arena"], c["slot"], which, eoff, segs, E, c["fill"], out0)).all()
    got = _scatter(eng, dev, c["arena"], c["slot"], which, eoff, segs, 12, E, c["vals"], c["chunk_bytes"])
    assert (got == pc.scatter_model(c["arena"], c["slot"], which, eoff, segs, E, c["vals"])).all()


def test_argument_checks(eng, dev):
    from hsds_amd import _native as nat
    import torch
    a = torch.zeros(64, dtype=torch.uint8, device=dev)
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    for segs in ([(0, 0, 5)], [(2, 0, 4)], [(0, 2, 2), (0, 0, 2)], [(0, 0, 3), (0, 2, 2)], [(0, 0, 0)]):
        with pytest.raises(nat.NativeError):
            eng.gather_points(a, z, None, z, segs, 4, 4, a)
        with pytest.raises(nat.NativeError):
            eng.scatter_points(a, z, None, z, None, segs, 4, 4, a)
    with pytest.raises(nat.NativeError):
        eng.locate_points(z.reshape(1, 1), (5,), (0,), 4)


# ---- selection.chunkReadPoints / chunkWritePoints ------------------------------------------
def _write_points(pts, vals, rank, sdt):
    rec = np.dtype([("coord", "<u8", (rank,)) if rank > 1 else ("coord", "<u8"), ("value", sdt)])
    arr = np.zeros(len(pts), rec)
    arr["coord"] = pts if rank > 1 else pts[:, 0]
    arr["value"] = vals
    return arr


@pytest.mark.parametrize("k", [3, 5, 8, 11, 12, 17, 19, 21, 22, 23, 27])
def test_selection_functions_match_the_reference(dev, k):
    from hsds_amd import selection as sel
    case = META["read"][k]
    dims, layout = META["geoms"][case["geom"]]
    dt = pc.golden_dtype(META, case["dtype"])
    sdt = pc.descr_dtype(case["select_descr"]) if case["fields"] else None
    chunk = ARRS[case["name"] + "__chunk"].view(dt).reshape(layout)
    pts = ARRS[case["name"] + "__pts"].reshape(-1, len(dims))
    out = sel.chunkReadPoints(chunk_id=case["chunk_id"], chunk_layout=layout, chunk_arr=chunk, point_arr=pts,
                              select_dt=sdt)
    assert out.shape == (case["n"],) and out.dtype.itemsize == case["select_itemsize"]
    assert (out.view(np.uint8).reshape(-1) == ARRS[case["name"] + "__out"]).all()
    case = META["write"][k]
    vals = ARRS[case["name"] + "__vals"].view(sdt if sdt is not None else dt)
    arr = ARRS[case["name"] + "__chunk"].view(dt).reshape(layout).copy()
    sel.chunkWritePoints(chunk_id=case["chunk_id"], chunk_layout=layout, chunk_arr=arr,
                         point_arr=_write_points(pts, vals, len(dims), vals.dtype), select_dt=sdt)
    if _prefix(case):
        want = ARRS[case["name"] + "__out"].view(dt).reshape(layout)
    else:
        # (b, c) and (c): the numpy model of "update the named fields" (the reference raises
        # for the first and writes nothing for the second)
        want = ARRS[case["name"] + "__chunk"].view(dt).reshape(layout).copy()
        corner = np.array(case["chunk_index"]) * np.array(layout)
        for p, v in zip(pts.astype(np.int64) - corner, vals):
            for f in case["fields"]:
                want[f][tuple(p)] = v[f]
    for f in dt.names or [None]:
        assert np.array_equal(arr[f] if f else arr, want[f] if f else want), (case["name"], f)


# ---- ChunkStore.get_points / put_points ---------------------------------------------------
def _ops(dt, layout):
    from hsds_amd.filters import getFilterOps
    return getFilterOps({"filter_map": {}}, DSET, [{"class": "H5Z_FILTER_SHUFFLE", "id": 2, "name": "shuffle"},
                                                   {"class": "H5Z_FILTER_DEFLATE", "id": 1, "level": 4}],
                        dtype=dt, chunk_shape=layout)


def _cid(idx):
    return "c-" + DSET[2:] + "_" + "_".join(str(i) for i in idx)


def _region(idx, layout, dims):
    return tuple(slice(i * c, min((i + 1) * c, n)) for i, c, n in zip(idx, layout, dims))


def _existing(orc, dims, layout, dt, before, which):
    from hsds_amd.partition import getS3Key
    objs = {}
    for idx in which:
        region = _region(idx, layout, dims)
        a = np.zeros(layout, dt)
        a[tuple(slice(0, s.stop - s.start) for s in region)] = before[region]
        objs[getS3Key(_cid(idx))] = orc.blosc_encode(a.tobytes(), typesize=1, clevel=4, shuffle=1)
    return objs


def _decode(orc, blob, layout, dt):
    raw = orc.uncompress(blob, "zlib", 1, dt.itemsize, int(np.prod(layout)) * dt.itemsize)
    assert not isinstance(raw, int), raw
    return np.frombuffer(raw, dt).reshape(layout)


DIMS, LAYOUT = (50, 37), (16, 10)
GRID = [(i, j) for i in range(4) for j in range(4)]


@pytest.fixture(scope="module")
def f4_dataset(oracle_lib):
    """a (50, 37) f4 dataset in (16, 10) chunks, stored objects for all chunks but four"""
    dt = np.dtype("<f4")
    rng = np.random.default_rng(11)
    before = np.round(np.cumsum(rng.normal(size=DIMS), axis=1), 2).astype(dt)
    have = [g for g in GRID if g not in ((0, 3), (1, 1), (3, 0), (3, 3))]
    return dt, before, have, _existing(oracle_lib, DIMS, LAYOUT, dt, before, have)


def _points(rng, n, rows=(0, DIMS[0]), cols=(0, DIMS[1])):
    return np.stack([rng.integers(rows[0], rows[1], n), rng.integers(cols[0], cols[1], n)], axis=1).astype(np.uint64)


def _expected(before, have, pts, fill):
    want = before[pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)].copy()
    for i, p in enumerate(pts):
        if (int(p[0]) // LAYOUT[0], int(p[1]) // LAYOUT[1]) not in have:
            want[i] = fill
    return want


@pytest.mark.parametrize("fill", [None, -7.5])
def test_get_points_hits_misses_and_missing_chunks(dev, f4_dataset, fill):
    import torch
    from hsds_amd.datanode import ChunkStore
    dt, before, have, stored = f4_dataset
    fetched = []
    store = ChunkStore(lambda k, o, n: (fetched.append(k), stored.get(k))[1], mem_target=64 << 20, device=dev)
    ops = _ops(dt, LAYOUT)
    rng = np.random.default_rng(3)
    first = _points(rng, 65, rows=(0, 16))                 # the first chunk row only
    out = store.get_points(DSET, DIMS, LAYOUT, first, dt, filter_ops=ops, fill_value=fill)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(dt) == _expected(before, have, first, fill or 0)).all()
    assert len(store.cache) == 3                           # (0, 3) has no object: nothing cached for it
    nfetch, hits0 = len(fetched), store.reader.stats["cache_hits"]
    pts = _points(rng, 4099)                               # every chunk: hits and misses in one request
    out = store.get_points(DSET, DIMS, LAYOUT, pts, dt, filter_ops=ops, fill_value=fill)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(dt) == _expected(before, have, pts, fill or 0)).all()
    assert store.reader.stats["cache_hits"] - hits0 == 3 and len(fetched) - nfetch == 13
    assert len(store.cache) == len(have) and store.cache.dirtyCount == 0
    # into a caller's buffer at request positions
    dst = torch.zeros(5000 * 4, dtype=torch.uint8, device=dev)
    dst_index = np.random.default_rng(4).permutation(5000)[:4099]
    got = store.get_points(DSET, DIMS, LAYOUT, pts, dt, filter_ops=ops, fill_value=fill, dst=dst, dst_index=dst_index)
    assert got is dst
    torch.cuda.synchronize()
    want = np.zeros(5000, dt)
    want[dst_index] = _expected(before, have, pts, fill or 0)
    assert (dst.cpu().numpy().view(dt) == want).all()
    # a buffer too small for the request is refused before anything is written
    small = torch.zeros(4098 * 4, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        store.get_points(DSET, DIMS, LAYOUT, pts, dt, filter_ops=ops, dst=small)
    with pytest.raises(ValueError):
        store.get_points(DSET, DIMS, LAYOUT, pts, dt, filter_ops=ops, dst=dst, dst_index=dst_index + 901)
    with pytest.raises(ValueError):
        store.get_points(DSET, DIMS, LAYOUT, pts, dt, filter_ops=ops, dst=dst,
                         dst_index=np.where(dst_index == dst_index.min(), -1, dst_index))
    with pytest.raises(ValueError):
        store.get_points(DSET, DIMS, LAYOUT, pts, dt, filter_ops=ops, dst=dst, dst_index=dst_index[:100])
    torch.cuda.synchronize()
    assert not small.any().item() and (dst.cpu().numpy().view(dt) == want).all()
    assert all(n.pinned == 0 for n in store.cache._lru.values())
    assert store.get_points(DSET, DIMS, LAYOUT, np.zeros((0, 2), np.uint64), dt, filter_ops=ops).numel() == 0


def test_get_points_when_the_cache_cannot_hold_the_chunks(dev, f4_dataset):
    """chunks that find no room in the cache (memFree below a chunk) are read into a batch
    buffer outside the arena: same values, nothing cached"""
    import torch
    from hsds_amd.datanode import ChunkStore
    dt, before, have, stored = f4_dataset
    store = ChunkStore(lambda k, o, n: stored.get(k), mem_target=100, device=dev)
    pts = _points(np.random.default_rng(8), 4099)
    out = store.get_points(DSET, DIMS, LAYOUT, pts, dt, filter_ops=_ops(dt, LAYOUT), fill_value=2.5)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(dt) == _expected(before, have, pts, 2.5)).all()
    assert len(store.cache) == 0


def test_get_points_compound_subset_and_fill(dev, oracle_lib):
    import torch
    from hsds_amd.datanode import ChunkStore
    dt = pc.ABC
    rng = np.random.default_rng(12)
    before = np.zeros(DIMS, dt)
    before["a"] = rng.integers(-1000, 1000, DIMS)
    before["b"] = np.round(rng.normal(size=DIMS), 2)
    before["c"] = rng.integers(65, 91, DIMS + (4,), dtype=np.uint8).view("S4").reshape(DIMS)
    have = [g for g in GRID if g != (2, 2)]
    stored = _existing(oracle_lib, DIMS, LAYOUT, dt, before, have)
    store = ChunkStore(lambda k, o, n: stored.get(k), mem_target=64 << 20, device=dev)
    pts = _points(rng, 4099)
    fillv = np.array((5, 1.5, b"zz"), dt)
    for fields in (None, ["b", "c"], ["a"]):
        sdt = pc.subset_dtype(dt, fields) if fields else None
        out = store.get_points(DSET, DIMS, LAYOUT, pts, dt, filter_ops=_ops(dt, LAYOUT), fill_value=fillv,
                               select_dt=sdt)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(sdt or dt)
        want = _expected(before, have, pts, fillv)
        for f in fields or dt.names:
            assert np.array_equal(got[f], want[f]), (fields, f)


def test_get_points_corrupt_object_and_bad_point(dev, f4_dataset):
    from hsds_amd.codec import HTTPInternalServerError
    from hsds_amd.datanode import ChunkStore
    from hsds_amd.partition import getS3Key
    dt, before, have, stored = f4_dataset
    stored = dict(stored)
    blob = bytearray(stored[getS3Key(_cid((1, 2)))])
    blob[16:] = bytes(len(blob) - 16)                 # header intact, stream zeroed: decode fails
    stored[getS3Key(_cid((1, 2)))] = bytes(blob)
    fetched = []
    store = ChunkStore(lambda k, o, n: (fetched.append(k), stored.get(k))[1], mem_target=64 << 20, device=dev)
    with pytest.raises(HTTPInternalServerError):
        store.get_points(DSET, DIMS, LAYOUT, _points(np.random.default_rng(1), 257), dt, filter_ops=_ops(dt, LAYOUT))
    assert _cid((1, 2)) not in store.cache
    assert all(n.pinned == 0 for n in store.cache._lru.values())
    nfetch = len(fetched)
    with pytest.raises(ValueError):
        store.get_points(DSET, DIMS, LAYOUT, np.array([[0, 0], [50, 0]], np.uint64), dt, filter_ops=_ops(dt, LAYOUT))
    assert len(fetched) == nfetch


def test_put_points_flush_and_decode(dev, oracle_lib, f4_dataset):
    from hsds_amd.datanode import ChunkStore
    from hsds_amd.partition import getS3Key
    orc = oracle_lib
    dt, before, have, stored = f4_dataset
    store = ChunkStore(lambda k, o, n: stored.get(k), mem_target=64 << 20, device=dev)
    ops = _ops(dt, LAYOUT)
    rng = np.random.default_rng(9)
    pts = np.concatenate([_points(rng, 2000, rows=(0, 32)), _points(rng, 2099, rows=(40, 50), cols=(0, 25))])
    pts[rng.integers(0, 4099, 1500)] = pts[rng.integers(0, 4099, 1500)]          # repeats
    rng.shuffle(pts)
    vals = np.round(rng.normal(size=4099) * 100, 1).astype(dt)
    touched = store.put_points(DSET, DIMS, LAYOUT, pts, vals, dt, filter_ops=ops, fill_value=-7.5)
    want_ids = {_cid((int(p[0]) // 16, int(p[1]) // 10)) for p in pts}
    assert set(touched) == want_ids and len(touched) == len(want_ids) < len(GRID)
    assert store.cache.dirtyCount == len(want_ids)
    out = {}
    store.flush(lambda k, b: out.__setitem__(k, b), filter_ops=ops)
    assert set(out) == {getS3Key(c) for c in want_ids}                          # only touched chunks are written
    want = before.copy()
    for g in GRID:
        if g not in have:
            want[_region(g, LAYOUT, DIMS)] = -7.5                               # chunk_init from the fill value
    for p, v in zip(pts.astype(np.int64), vals):
        want[tuple(p)] = v                                                       # in order: the last value stands
    for g in GRID:
        if _cid(g) not in want_ids:
            continue
        got = _decode(orc, out[getS3Key(_cid(g))], LAYOUT, dt)
        r = _region(g, LAYOUT, DIMS)
        assert np.array_equal(got[tuple(slice(0, s.stop - s.start) for s in r)], want[r]), g
    # read back through the same store
    back = store.get_points(DSET, DIMS, LAYOUT, pts, dt, filter_ops=ops, fill_value=-7.5)
    assert (back.cpu().numpy().view(dt) == want[pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)]).all()


def test_put_points_field_subset(dev, oracle_lib):
    """(b, c) of (a, b, c): the named fields are updated, a is left alone"""
    from hsds_amd.datanode import ChunkStore
    dt = pc.ABC
    rng = np.random.default_rng(13)
    before = np.zeros(DIMS, dt)
    before["a"] = rng.integers(-1000, 1000, DIMS)
    before["b"] = np.round(rng.normal(size=DIMS), 2)
    stored = _existing(oracle_lib, DIMS, LAYOUT, dt, before, GRID)
    store = ChunkStore(lambda k, o, n: stored.get(k), mem_target=64 << 20, device=dev)
    pts = _points(rng, 257)
    sdt = pc.subset_dtype(dt, ["b", "c"])
    vals = np.zeros(257, sdt)
    vals["b"] = np.round(rng.normal(size=257), 2)
    vals["c"] = rng.integers(65, 91, (257, 4), dtype=np.uint8).view("S4").reshape(257)
    store.put_points(DSET, DIMS, LAYOUT, pts, vals, dt, filter_ops=_ops(dt, LAYOUT))
    want = before.copy()
    for p, v in zip(pts.astype(np.int64), vals):
        want["b"][tuple(p)], want["c"][tuple(p)] = v["b"], v["c"]
    allpts = np.stack(np.meshgrid(np.arange(DIMS[0]), np.arange(DIMS[1]), indexing="ij"), axis=-1).reshape(-1, 2)
    back = store.get_points(DSET, DIMS, LAYOUT, allpts.astype(np.uint64), dt, filter_ops=_ops(dt, LAYOUT))
    assert np.array_equal(back.cpu().numpy().view(dt).reshape(DIMS), want)


def test_put_points_out_of_extent_changes_nothing(dev, f4_dataset):
    from hsds_amd.datanode import ChunkStore
    dt, before, have, stored = f4_dataset
    fetched = []
    store = ChunkStore(lambda k, o, n: (fetched.append(k), stored.get(k))[1], mem_target=64 << 20, device=dev)
    pts = np.array([[1, 1], [20, 20], [49, 37], [3, 3]], np.uint64)              # column 37 is past the extent
    with pytest.raises(ValueError):
        store.put_points(DSET, DIMS, LAYOUT, pts, np.ones(4, dt), dt, filter_ops=_ops(dt, LAYOUT))
    assert not fetched and len(store.cache) == 0 and store.cache.dirtyCount == 0
    out = {}
    store.flush(lambda k, b: out.__setitem__(k, b), filter_ops=_ops(dt, LAYOUT))
    assert not out


# ---- sharded paths: three simulated ranks, one owns no chunk ----------------------------------
def _three_rank_points(rng, n):
    """points only in chunks that two of three ranks own"""
    from hsds_amd import crawl
    idx = np.array(GRID, np.int64)
    owner = crawl.partition_ids("c-" + DSET[2:] + "_", idx, 3)
    counts = np.bincount(owner, minlength=3)
    idle = int(np.argmin(counts))
    chunks = idx[owner != idle]
    assert len(chunks) >= 4 and len(set(owner[owner != idle])) == 2
    pick = chunks[rng.integers(0, len(chunks), n)]
    hi = np.minimum((pick + 1) * np.array(LAYOUT), np.array(DIMS))
    lo = pick * np.array(LAYOUT)
    pts = (lo + (rng.random((n, 2)) * (hi - lo)).astype(np.int64)).astype(np.uint64)
    return pts, idle


@pytest.mark.parametrize("host_response", [False, True])
def test_sharded_point_read(dev, f4_dataset, host_response):
    import torch
    from hsds_amd import crawl
    from hsds_amd.datanode import ChunkStore
    from hsds_amd.engine import HostBuffer
    dt, before, have, stored = f4_dataset
    pts, idle = _three_rank_points(np.random.default_rng(21), 4099)
    plan = crawl.PointPlan(DSET, DIMS, LAYOUT, pts, dt, 3, device=dev.index)
    assert plan.by_rank[idle].numel() == 0 and sum(int(b.numel()) for b in plan.by_rank) == 4099
    response = HostBuffer(4099 * 4, dev) if host_response else torch.zeros(4099 * 4, dtype=torch.uint8, device=dev)
    served = 0
    for r in range(3):
        store = ChunkStore(lambda k, o, n: stored.get(k), mem_target=64 << 20, device=dev)
        served += crawl.ShardedPointReader(plan, r, store).read(response, filter_ops=_ops(dt, LAYOUT), fill_value=-1.0)
        if r == idle:
            assert len(store.cache) == 0
        else:
            assert set(store.cache) <= set(plan.chunk_ids(r))
    torch.cuda.synchronize()
    assert served == 4099
    got = (response.array.copy() if host_response else response.cpu().numpy()).view(dt)
    assert (got == _expected(before, have, pts, -1.0)).all()
    if host_response:
        response.close()


def test_sharded_point_write(dev, oracle_lib, f4_dataset):
    from hsds_amd import crawl
    from hsds_amd.datanode import ChunkStore
    from hsds_amd.partition import getS3Key
    dt, before, have, stored = f4_dataset
    rng = np.random.default_rng(22)
    pts, idle = _three_rank_points(rng, 4099)
    pts[rng.integers(0, 4099, 1000)] = pts[rng.integers(0, 4099, 1000)]          # repeats
    vals = np.round(rng.normal(size=4099) * 10, 2).astype(dt)
    plan = crawl.PointPlan(DSET, DIMS, LAYOUT, pts, dt, 3, device=dev.index)
    out, ops = {}, _ops(dt, LAYOUT)
    for r in range(3):
        store = ChunkStore(lambda k, o, n: stored.get(k), mem_target=64 << 20, device=dev)
        touched = crawl.ShardedPointWriter(plan, r, store).write(vals, filter_ops=ops, fill_value=0)
        assert set(touched) == {c for c in plan.chunk_ids(r)} and (r != idle or not touched)
        store.flush(lambda k, b: out.__setitem__(k, b), filter_ops=ops)
    assert set(out) == {getS3Key(c) for c in plan.ids}
    want = before.copy()
    for g in GRID:
        if g not in have:
            want[_region(g, LAYOUT, DIMS)] = 0
    for p, v in zip(pts.astype(np.int64), vals):
        want[tuple(p)] = v
    for row in plan.idx.tolist():
        got = _decode(oracle_lib, out[getS3Key(_cid(row))], LAYOUT, dt)
        r = _region(row, LAYOUT, DIMS)
        assert np.array_equal(got[tuple(slice(0, s.stop - s.start) for s in r)], want[r]), row


def test_selection_plan_still_rejects_coordinate_lists():
    from hsds_amd import crawl
    with pytest.raises(NotImplementedError):
        crawl.SelectionPlan(DSET, DIMS, LAYOUT, (slice(0, 10, 1), [1, 2, 3]), np.dtype("<f4"), 2)
