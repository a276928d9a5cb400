"""GPU parity of query selections: the HIP kernels behind hsds_query_mask / hsds_query_emit
bit for bit against the reference's goldens and the numpy model (the same cases as the CPU
emulation tests, tests/query_cases.py), hsds_amd.selection.chunkQuery against the reference,
ChunkStore.query over a store whose fetch serves oracle-encoded objects (as in
tests/test_gpu_points.py), and crawl.QueryPlan over three simulated ranks, one of which owns
no chunk."""
import numpy as np
import pytest

import points_cases as pc
import query_cases as qc
from hsds_amd import _native as nat
from hsds_amd import query as qry

pytestmark = pytest.mark.gpu
DSET = "d-9e8d7c6b-5a4f3e2d-1c0b-9a8f7e-6d5c4b"
META, ARRS = qc.goldens()


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda", 0)


def _t(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).to(dev)


class Gpu:
    """the emulator driver's two calls (qc.Emu) over the C ABI"""

    def __init__(self, dev):
        from hsds_amd.engine import ChunkEngine
        self.dev = dev
        self.eng = ChunkEngine(dev.index)

    def mask(self, arena, table, nwords, rowsize, prog, isin):
        import torch
        mask = torch.zeros(max(nwords, 1), dtype=torch.int64, device=self.dev)
        count = torch.zeros(max(nwords, 1), dtype=torch.int32, device=self.dev)
        try:
            self.eng.query_mask(_t(arena, self.dev), _t(table.view(np.int64).reshape(-1), self.dev), len(table), nwords,
                                rowsize, prog, None if isin is None else _t(isin, self.dev), mask, count)
        except nat.NativeError as e:
            return e.code
        return mask.cpu().numpy().view(np.uint64)[:nwords], count.cpu().numpy()[:nwords]

    def emit(self, arena, table, nwords, rowsize, mask, base, limit, segs, out_elem, outbuf, shift, upd_segs=None,
             upd=None, lead=0):
        import torch
        d_arena = _t(arena, self.dev)
        buf = torch.zeros(len(outbuf) + 32, dtype=torch.uint8, device=self.dev)
        o = (-(buf.data_ptr() + lead)) % 16 + shift
        view = buf[o:o + len(outbuf)]
        view.copy_(torch.from_numpy(outbuf.copy()))
        try:
            self.eng.query_emit(d_arena, _t(table.view(np.int64).reshape(-1), self.dev), len(table), nwords, rowsize,
                                _t(mask, self.dev), _t(base, self.dev), limit, segs, out_elem, view[lead:],
                                upd_segs=upd_segs, upd_elem=0 if upd is None else len(upd),
                                upd=None if upd is None else _t(upd, self.dev))
        except nat.NativeError as e:
            return e.code
        host = buf.cpu().numpy()
        assert not host[:o].any() and not host[o + len(outbuf):].any(), "bytes outside the buffer written"
        return host[o:o + len(outbuf)].copy(), d_arena.cpu().numpy()


@pytest.fixture(scope="module")
def gpu(dev):
    return Gpu(dev)


# ---- kernel parity (the emulation tests' cases) ------------------------------------------
@pytest.mark.parametrize("name", list(qc.DTYPES))
def test_row_counts(gpu, name):
    for n in qc.COUNTS:
        c = qc.kernel_case(n + len(name), name, [n])
        assert qc.check(gpu, c) <= n


@pytest.mark.parametrize("name", list(qc.DTYPES))
def test_selectivity_and_missing_chunks(gpu, name):
    none, every = qc.NONE_ALL[name]
    c = qc.kernel_case(3, name, [65, 128, 5], query=none, pred=lambda r: np.zeros(len(r), bool))
    assert qc.check(gpu, c) == 0
    c = qc.kernel_case(4, name, [65, 128, 5], query=every, pred=lambda r: np.ones(len(r), bool))
    assert qc.check(gpu, c) == 198
    for nchunks in (1, 3, 17):
        counts = [(37 * (k + 1)) % 131 for k in range(nchunks)]
        c = qc.kernel_case(nchunks, name, counts, missing=nchunks // 2 if nchunks > 1 else None)
        qc.check(gpu, c)
        qc.check(gpu, c, limit=sum(counts) // 5 + 1)


def test_limit_edges(gpu):
    c = qc.kernel_case(7, "abc", [100, 64, 30], query="a >= -1000", pred=lambda r: np.ones(len(r), bool))
    d = qc.kernel_case(8, "e24", [100, 64, 30])
    for limit in (1, 37, 64, 100, 128, 164, 193, 194, 1000):
        assert qc.check(gpu, c, limit=limit) == min(limit, 194)
        qc.check(gpu, d, limit=limit)


@pytest.mark.parametrize("name", ["abc", "u14", "pad"])
def test_selections(gpu, name):
    for first, step in ((0, 1), (1, 1), (0, 2), (1, 2), (0, 3), (2, 3)):
        c = qc.kernel_case(10 * first + step, name, [129, 64, 7], step=step, first=first)
        qc.check(gpu, c)
        qc.check(gpu, c, limit=70)


@pytest.mark.parametrize("name,fields", [("abc", None), ("abc", ["b"]), ("u14", None), ("arrf", ["m"]),
                                         ("e24", ["x", "z"]), ("pad", None), ("pad", ["w"])])
def test_response_placement(gpu, name, fields):
    for shift in (0, 1, 4, 8, 12):
        c = qc.kernel_case(shift, name, [130, 3])
        qc.check(gpu, c, fields=fields, shift=shift)


@pytest.mark.parametrize("name,update", [("abc", {"a": 7}), ("abc", {"c": b"zz", "b": 1.5}), ("u14", {"f": -2.25}),
                                         ("u14", {"k": 1, "g": 3.0}), ("e24", {"y": -1}), ("pad", {"u": 3, "w": -1}),
                                         ("pad", {"v": 0.25})])
def test_update(gpu, name, update):
    for limit in (0, 1, 40, 64):
        c = qc.kernel_case(len(update) + limit, name, [70, 0, 130], step=2, first=1)
        assert qc.check(gpu, c, limit=limit, update=update) > 0


def test_many_words_grid_stride(gpu):
    """more mask words than the grid has waves (8192 blocks of four): the grid-stride loop"""
    c = qc.kernel_case(5, "abc", [64 * 8192 * 4 + 777, 100])
    assert qc.check(gpu, c, limit=0) > 1000000


def test_golden_kernels(gpu):
    for k, rec in enumerate(META["cases"]):
        qc.check_golden(gpu, rec, ARRS.get(f"case_{k}"))
    for k, rec in enumerate(META["updates"]):
        qc.check_golden(gpu, rec, ARRS[f"upd_{k}"], update=rec["update"], want_chunk=ARRS[f"upd_chunk_{k}"])


def test_isin_by_value(gpu):
    dt = np.dtype([("f", "<f4"), ("d", "<f8"), ("i", "i1"), ("u", "<u8"), ("s", "S3")])
    a = np.zeros(9, dt)
    a["f"] = [0.0, -0.0, np.nan, 1.5, 2.5, np.inf, -np.inf, 0.1, 3.0]
    a["d"] = a["f"]
    a["i"] = [-128, -1, 0, 1, 127, 5, 6, 7, 8]
    a["u"] = [0, 1, 2 ** 63, 2 ** 64 - 1, 5, 6, 7, 8, 9]
    a["s"] = [b"a", b"ab", b"abc", b"", b"b", b"a\0b", b"ab", b"c", b"abd"]
    for q in ("where f in (0, nan, 2.5, inf)", "where d in (-inf, 0.1, 1.5)", "where i in (-128, 127, 0)",
              "where u in (18446744073709551615, 0, 9223372036854775808)", "where s in (ab, abcd, b'')"):
        field = qry.where_field_name(q)
        want = np.isin(a[field], np.array(qry.where_elements(q), dtype=dt[field]))
        assert (qc.row_mask(gpu, a, qry.compile_query(q, dt)) == want).all(), q


def test_conversions_on_the_device(gpu):
    """a sample of the compile tests' matrix through the HIP kernel: limits, 2^53 + 1, NaN,
    float32 rounding, signed against unsigned"""
    dt = np.dtype([("p", "u1"), ("a", "<i8"), ("b", "<u8"), ("f", "<f4"), ("g", "<f8"), ("h", "i1")])
    arr = np.zeros(8, dt)
    arr["a"] = [-2 ** 63, -1, 0, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 63 - 1, 5]
    arr["b"] = [0, 2 ** 64 - 1, 2 ** 63, 2 ** 53, 2 ** 53 + 1, 5, 2 ** 63 - 1, 4]
    arr["f"] = [0.1, 16777216.0, np.nan, np.inf, -0.0, 1.5, -1.5, 3.0]
    arr["g"] = [0.1, 16777217.0, np.nan, -np.inf, 0.0, 1.5, -1.5, 9007199254740992.0]
    arr["h"] = [-128, 127, 0, -1, 1, 5, 6, 7]
    r = {n: arr[n] for n in dt.names}
    with np.errstate(all="ignore"):
        cases = {"a == 9007199254740993": r["a"] == 9007199254740993, "a > 9007199254740993.0": r["a"] > 9007199254740993.0,
                 "f == 0.1": r["f"] == 0.1, "g == 0.1": r["g"] == 0.1, "f == 16777217": r["f"] == 16777217,
                 "f != nan": r["f"] != float("nan"), "g <= -0.0": r["g"] <= -0.0, "h < 128": r["h"] < 128,
                 "h >= -129": r["h"] >= -129, "h == 300": r["h"] == 300, "b > -1": r["b"] > -1, "a < b": r["a"] < r["b"],
                 "b <= a": r["b"] <= r["a"], "a == b": r["a"] == r["b"], "f < g": r["f"] < r["g"], "h > f": r["h"] > r["f"],
                 "a >= g": r["a"] >= r["g"]}
    for q, want in cases.items():
        assert (qc.row_mask(gpu, arr, qry.compile_query(q, dt)) == want).all(), q


def test_argument_checks(gpu):
    c = qc.kernel_case(1, "abc", [10])
    table, nwords = qry.query_chunk_table([(c["slots"][0],) + c["sels"][0]])

    def prog(*ops):
        p = nat.QueryProg()
        p.nops = len(ops)
        for k, kw in enumerate(ops[:nat.QUERY_MAX_OPS]):
            for name, v in kw.items():
                setattr(p.ops[k], name, v)
        return p
    cmp_a = dict(op=nat.Q_CMP, kind=2, off=0)
    bad = [prog(*([cmp_a] + [cmp_a, dict(op=nat.Q_AND)] * 16)),            # a program over 32 operations
           prog(dict(op=nat.Q_CMP, kind=2, off=9)),                         # a field past the row size
           prog(dict(op=nat.Q_CMP_BYTES, kind=10, off=8, len=5, len_b=1)),
           prog(dict(op=nat.Q_ISIN, kind=2, off=0, imm=2)),                 # elements past the buffer
           prog(cmp_a, dict(op=nat.Q_AND)), prog(cmp_a, cmp_a), prog()]
    for p in bad:
        assert gpu.mask(c["arena"], table, nwords, 12, p, None) == qc.ERR_ARG
    mask, count = gpu.mask(c["arena"], table, nwords, 12, c["cq"].prog, None)
    base = np.cumsum(count, dtype=np.int64) - count
    out = np.zeros(20 * 10 + 16, np.uint8)
    assert not isinstance(gpu.emit(c["arena"], table, nwords, 12, mask, base, 0, [(0, 8, 12)], 20, out, 0), int)
    for segs, E in ([(0, 0, 12)], 20), ([(0, 8, 13)], 21), ([(4, 8, 12)], 20), ([(0, 12, 4), (4, 8, 4)], 20), \
            ([(0, 8, 4), (4, 10, 4)], 20), ([(0, 8, 0)], 20), ([(0, 8 + k, 1) for k in range(17)], 32):
        assert gpu.emit(c["arena"], table, nwords, 12, mask, base, 0, segs, E, out, 0) == qc.ERR_ARG, segs
    assert gpu.emit(c["arena"], table, nwords, 12, mask, base, 0, [(0, 8, 12)], 20, out, 0, upd_segs=[(10, 0, 4)],
                    upd=np.zeros(4, np.uint8)) == qc.ERR_ARG


# ---- selection.chunkQuery against the reference -------------------------------------------
def _chunk_query(rec, update=None):
    from hsds_amd.selection import chunkQuery
    arr = qc.golden_chunk(rec["dtype"])
    rsp = chunkQuery(chunk_id="c-" + META["dset"][2:] + "_" + str(rec["cidx"]), chunk_layout=(len(arr),), chunk_arr=arr,
                     slices=[slice(*rec["sel"])] if rec["sel"] else None, query=rec["query"], query_update=update,
                     select_dt=qc.golden_select(META, rec), limit=rec["limit"])
    return arr, rsp


def test_chunkQuery_matches_the_reference(dev):
    seen = 0
    for k, rec in enumerate(META["cases"]):
        arr, rsp = _chunk_query(rec)
        if rec["none"]:
            assert rsp is None
            continue
        assert rsp.dtype == pc.descr_dtype(rec["rsp_descr"]) and len(rsp) == rec["nrows"]
        if rec["deviates"]:
            start, count, step, index0 = qc.golden_sel(rec, len(arr))
            idx = start + np.arange(count) * step
            hits = idx[qc.golden_mask(rec, arr[idx])]
            assert (rsp["index"] == index0 + hits).all() and (rsp["open"] == arr["open"][hits]).all()
            continue
        assert rsp.tobytes() == ARRS[f"case_{k}"].tobytes(), rec["query"]
        seen += 1
    assert seen > 70


def test_chunkQuery_update_matches_the_reference(dev):
    for k, rec in enumerate(META["updates"]):
        before = qc.golden_chunk(rec["dtype"])
        arr, rsp = _chunk_query(rec, update=rec["update"])
        assert len(rsp) == rec["nrows"]
        if rec["deviates"]:
            # the matched rows are updated (the reference updates chunk_arr[selection-relative index])
            start, count, step, index0 = qc.golden_sel(rec, len(arr))
            idx = start + np.arange(count) * step
            hits = idx[qc.golden_mask(rec, before[idx])]
            want = before.copy()
            for f, v in rec["update"].items():
                want[f][hits] = v
            assert (arr == want).all() and (rsp["index"] == index0 + hits).all()
            assert not (ARRS[f"upd_chunk_{k}"].view(arr.dtype) == want).all()          # on record: the reference differs
            continue
        assert rsp.tobytes() == ARRS[f"upd_{k}"].tobytes()
        assert (arr == ARRS[f"upd_chunk_{k}"].view(arr.dtype)).all()
        pad = ~np.tile(pc.field_mask(arr.dtype), len(arr))
        assert (arr.view(np.uint8)[pad] == before.view(np.uint8)[pad]).all()


# ---- ChunkStore.query ----------------------------------------------------------------------
STOCK = np.dtype([("sym", "S4"), ("date", "S8"), ("open", "<i4"), ("close", "<f4")])
NROWS, CHUNK = 1000, 150            # 7 chunks, the last one partial


def _ops(dt):
    from hsds_amd.filters import getFilterOps
    return getFilterOps({"filter_map": {}}, DSET, [{"class": "H5Z_FILTER_SHUFFLE", "id": 2, "name": "shuffle"},
                                                   {"class": "H5Z_FILTER_DEFLATE", "id": 1, "level": 4}],
                        dtype=dt, chunk_shape=(CHUNK,))


def _cid(i):
    return "c-" + DSET[2:] + "_" + str(i)


@pytest.fixture(scope="module")
def table(oracle_lib):
    """a 1000-row stock table in chunks of 150 rows; chunk 3 has no stored object"""
    from hsds_amd.partition import getS3Key
    rng = np.random.default_rng(21)
    rows = np.zeros(NROWS, STOCK)
    rows["sym"] = rng.choice(np.array([b"AAPL", b"IBM", b"GO", b"X"], "S4"), NROWS)
    rows["date"] = np.array([b"2020%04d" % (i % 1231) for i in range(NROWS)], "S8")
    rows["open"] = rng.integers(3000, 3200, NROWS)
    rows["close"] = np.round(rows["open"] + rng.normal(size=NROWS) * 20, 1)
    have = [0, 1, 2, 4, 5, 6]
    stored = {}
    for i in have:
        a = np.zeros(CHUNK, STOCK)
        part = rows[i * CHUNK:(i + 1) * CHUNK]
        a[:len(part)] = part
        stored[getS3Key(_cid(i))] = oracle_lib.blosc_encode(a.tobytes(), typesize=1, clevel=4, shuffle=1)
    return rows, have, stored


def _want(rows, have, pred, sel=slice(0, NROWS, 1), limit=0, fields=None):
    idx = np.arange(NROWS)[sel]
    idx = idx[np.isin(idx // CHUNK, have)]
    hits = idx[pred(rows[idx])]
    hits = hits[:limit] if limit else hits
    sdt = pc.subset_dtype(STOCK, fields) if fields else STOCK
    out = np.zeros(len(hits), qry.query_dtype(sdt))
    out["index"] = hits
    for f in sdt.names:
        out[f] = rows[f][hits]
    return out


def _pred(r):
    return (r["sym"] == b"AAPL") & (r["open"] > 3100)


QUERY = "(sym == b'AAPL') & (open > 3100)"


def test_store_query_hits_misses_and_a_missing_chunk(dev, table):
    from hsds_amd.datanode import ChunkStore
    rows, have, stored = table
    fetched = []
    store = ChunkStore(lambda k, o, n: (fetched.append(k), stored.get(k))[1], mem_target=64 << 20, device=dev)
    ops = _ops(STOCK)
    res = store.query(DSET, (NROWS,), (CHUNK,), [slice(0, 300, 1)], QUERY, STOCK, filter_ops=ops)
    want = _want(rows, have, _pred, slice(0, 300, 1))
    assert res.rows.cpu().numpy().tobytes() == want.tobytes() and res.dtype == want.dtype and len(want) > 5
    assert len(store.cache) == 2 and res.chunk_ids == [_cid(0), _cid(1)] and res.touched == []
    nfetch, hits0 = len(fetched), store.reader.stats["cache_hits"]
    # every chunk: two hits, four misses and one missing object in one request
    res = store.query(DSET, (NROWS,), (CHUNK,), None, QUERY, STOCK, filter_ops=ops)
    want = _want(rows, have, _pred)
    assert res.rows.cpu().numpy().tobytes() == want.tobytes()
    assert store.reader.stats["cache_hits"] - hits0 == 2 and len(fetched) - nfetch == 5
    assert len(store.cache) == len(have) and store.cache.dirtyCount == 0       # nothing cached for chunk 3
    assert res.starts[3] == res.starts[4] and res.starts[-1] == len(want)
    assert all(n.pinned == 0 for n in store.cache._lru.values())
    # limit across chunks: the first rows in dataset order; a field subset; a stepped selection
    for limit in (1, int(res.starts[1]), int(res.starts[2]) + 1, len(want), len(want) + 5):
        got = store.query(DSET, (NROWS,), (CHUNK,), None, QUERY, STOCK, filter_ops=ops, limit=limit)
        assert got.rows.cpu().numpy().tobytes() == _want(rows, have, _pred, limit=limit).tobytes(), limit
    sdt = pc.subset_dtype(STOCK, ["date", "close"])
    got = store.query(DSET, (NROWS,), (CHUNK,), [slice(7, 990, 3)], QUERY, STOCK, filter_ops=ops, select_dt=sdt, limit=40)
    want = _want(rows, have, _pred, slice(7, 990, 3), limit=40, fields=["date", "close"])
    assert got.rows.cpu().numpy().tobytes() == want.tobytes() and got.dtype.names == ("index", "date", "close")
    # a where-in tail, and a selection that selects nothing
    got = store.query(DSET, (NROWS,), (CHUNK,), None, "open > 3150 where sym in (GO, b'X')", STOCK, filter_ops=ops)
    want = _want(rows, have, lambda r: (r["open"] > 3150) & np.isin(r["sym"], [b"GO", b"X"]))
    assert got.rows.cpu().numpy().tobytes() == want.tobytes() and len(want) > 5
    got = store.query(DSET, (NROWS,), (CHUNK,), [slice(5, 5, 1)], QUERY, STOCK, filter_ops=ops)
    assert got.rows.numel() == 0 and got.chunk_ids == []
    with pytest.raises(ValueError, match="query variable: nofield"):
        store.query(DSET, (NROWS,), (CHUNK,), None, "nofield > 1", STOCK, filter_ops=ops)


def test_store_query_when_the_cache_cannot_hold_the_chunks(dev, table):
    from hsds_amd.datanode import ChunkStore
    rows, have, stored = table
    store = ChunkStore(lambda k, o, n: stored.get(k), mem_target=100, device=dev)
    res = store.query(DSET, (NROWS,), (CHUNK,), None, QUERY, STOCK, filter_ops=_ops(STOCK))
    assert res.rows.cpu().numpy().tobytes() == _want(rows, have, _pred).tobytes() and len(store.cache) == 0
    with pytest.raises(MemoryError):
        store.query(DSET, (NROWS,), (CHUNK,), None, QUERY, STOCK, filter_ops=_ops(STOCK), query_update={"open": 1})


def test_store_query_corrupt_object(dev, table):
    from hsds_amd.codec import HTTPInternalServerError
    from hsds_amd.datanode import ChunkStore
    from hsds_amd.partition import getS3Key
    rows, have, stored = table
    stored = dict(stored)
    blob = bytearray(stored[getS3Key(_cid(2))])
    blob[16:] = bytes(len(blob) - 16)                 # header intact, stream zeroed: decode fails
    stored[getS3Key(_cid(2))] = bytes(blob)
    store = ChunkStore(lambda k, o, n: stored.get(k), mem_target=64 << 20, device=dev)
    for update in (None, {"open": 1}):
        with pytest.raises(HTTPInternalServerError):
            store.query(DSET, (NROWS,), (CHUNK,), None, QUERY, STOCK, filter_ops=_ops(STOCK), query_update=update)
        assert _cid(2) not in store.cache and store.cache.dirtyCount == 0
        assert all(n.pinned == 0 for n in store.cache._lru.values())
    # the other chunks are as stored: the failed update wrote nothing
    res = store.query(DSET, (NROWS,), (CHUNK,), [slice(0, 300, 1)], QUERY, STOCK, filter_ops=_ops(STOCK))
    assert res.rows.cpu().numpy().tobytes() == _want(rows, have, _pred, slice(0, 300, 1)).tobytes()


def test_store_query_update_flush_and_decode(dev, oracle_lib, table):
    from hsds_amd.datanode import ChunkStore
    from hsds_amd.partition import getS3Key
    rows, have, stored = table
    store = ChunkStore(lambda k, o, n: stored.get(k), mem_target=64 << 20, device=dev)
    ops = _ops(STOCK)
    # rows 0..599 only, limit inside chunk 2: chunks 0, 1, 2 are updated; 3 has no object
    base = _want(rows, have, _pred, slice(0, 600, 1))
    limit = int((base["index"] < 2 * CHUNK).sum()) + 2
    res = store.query(DSET, (NROWS,), (CHUNK,), [slice(0, 600, 1)], QUERY, STOCK, filter_ops=ops, limit=limit,
                      query_update={"open": 7, "sym": "UPD"})
    hits = base["index"][:limit].astype(np.int64)
    want_rows = rows.copy()
    want_rows["open"][hits] = 7
    want_rows["sym"][hits] = b"UPD"
    want = np.zeros(limit, base.dtype)
    want["index"] = hits
    for f in STOCK.names:
        want[f] = want_rows[f][hits]
    assert res.rows.cpu().numpy().tobytes() == want.tobytes()
    assert res.touched == [_cid(0), _cid(1), _cid(2)] and store.cache.dirtyCount == 3
    assert _cid(3) not in store.cache                                        # no chunk_init for a query
    out = {}
    store.flush(lambda k, b: out.__setitem__(k, b), filter_ops=ops)
    assert set(out) == {getS3Key(_cid(i)) for i in (0, 1, 2)}                # only updated chunks are written
    for i in (0, 1, 2):
        raw = oracle_lib.uncompress(out[getS3Key(_cid(i))], "zlib", 1, STOCK.itemsize, CHUNK * STOCK.itemsize)
        assert not isinstance(raw, int), raw
        assert (np.frombuffer(raw, STOCK) == want_rows[i * CHUNK:(i + 1) * CHUNK]).all(), i
    # a query that matches nothing updates and dirties nothing
    res = store.query(DSET, (NROWS,), (CHUNK,), None, "open > 5000", STOCK, filter_ops=ops, query_update={"open": 1})
    assert res.rows.numel() == 0 and res.touched == [] and store.cache.dirtyCount == 0
    with pytest.raises(ValueError, match="not supported with where in"):
        store.query(DSET, (NROWS,), (CHUNK,), None, "open > 1 where sym in (GO)", STOCK, query_update={"open": 1})
    with pytest.raises(ValueError, match="no fields found"):
        store.query(DSET, (NROWS,), (CHUNK,), None, "open > 1", STOCK, query_update={"nofield": 1})


def test_query_plan_over_three_ranks(dev, table):
    """every rank queries the chunks it owns (md5 partition); the merge restores dataset
    order and applies the limit; a rank that owns no chunk contributes nothing"""
    from hsds_amd.crawl import QueryPlan
    from hsds_amd.datanode import ChunkStore
    rows, have, stored = table
    world = 3
    probe = QueryPlan(DSET, (NROWS,), (CHUNK,), None, QUERY, STOCK, world)
    assert sorted(sum((probe.chunk_ids(r) for r in range(world)), [])) == sorted(probe.ids) and len(probe.ids) == 7
    # a selection whose chunks leave one rank without any
    sel = None
    for lo in range(7):
        for hi in range(lo + 1, 8):
            p = QueryPlan(DSET, (NROWS,), (CHUNK,), [slice(lo * CHUNK, min(hi * CHUNK, NROWS), 1)], QUERY, STOCK, world)
            owners = {int(o) for o in p.owner}
            if len(owners) == 2 and len(p.ids) >= 3 and sel is None:
                sel = [slice(lo * CHUNK, min(hi * CHUNK, NROWS), 1)]
    assert sel is not None
    for selection, limit in ((None, 0), (None, 25), (sel, 0), (sel, 9), ([slice(3, 997, 2)], 30)):
        plan = QueryPlan(DSET, (NROWS,), (CHUNK,), selection, QUERY, STOCK, world, limit=limit)
        results = []
        for r in range(world):
            store = ChunkStore(lambda k, o, n: stored.get(k), mem_target=64 << 20, device=dev)
            results.append(plan.query(r, store, filter_ops=_ops(STOCK)) if plan.chunk_ids(r) else None)
            if results[-1] is not None:
                assert set(results[-1].chunk_ids) == set(plan.chunk_ids(r))
        if selection is sel:
            assert any(x is None for x in results)
        got = plan.merge(results)
        want = _want(rows, have, _pred, selection[0] if selection else slice(0, NROWS, 1), limit=limit)
        assert got.tobytes() == want.tobytes() and got.dtype == want.dtype, (selection, limit)
