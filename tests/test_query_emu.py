"""CPU emulation of the query kernels (hsds_amd/csrc/query.h, run lane by lane by
tests/emu/query_emu.cpp) against the reference's goldens and the numpy model of the
hsds_query_mask / hsds_query_emit contract (include/hsds_amd.h): row counts around the
64-row mask words, chunks that match nothing or everything, the limit at every kind of edge,
stepped selections, unaligned records, missing chunks, a response 4 bytes off a 16-byte
boundary inside a guarded buffer, and the update.  Test infrastructure only."""
import numpy as np
import pytest

import query_cases as qc
from hsds_amd import _native as nat
from hsds_amd import query as qry


@pytest.fixture(scope="module")
def emu():
    return qc.Emu()


@pytest.mark.parametrize("n", qc.COUNTS)
@pytest.mark.parametrize("name", list(qc.DTYPES))
def test_row_counts(emu, name, n):
    c = qc.kernel_case(n + len(name), name, [n])
    assert qc.check(emu, c) <= n


@pytest.mark.parametrize("name", list(qc.DTYPES))
def test_selectivity(emu, name):
    """chunks where no row matches and chunks where every row matches"""
    dt = qc.DTYPES[name]
    none, every = qc.NONE_ALL[name]
    c = qc.kernel_case(3, name, [65, 128, 5], query=none, pred=lambda r: np.zeros(len(r), bool))
    assert qc.check(emu, c) == 0
    c = qc.kernel_case(4, name, [65, 128, 5], query=every, pred=lambda r: np.ones(len(r), bool))
    assert qc.check(emu, c) == 198
    # a chunk of each kind around an ordinary one
    q, p = qc.QUERIES[name]
    c = qc.kernel_case(5, name, [70, 64, 130])
    for k, verdict in ((0, True), (2, False)):
        arr = c["chunks"][k]
        keep = np.nonzero(p(arr) == verdict)[0]
        assert len(keep)
        raw = arr.view(np.uint8).reshape(len(arr), dt.itemsize)
        raw[:] = raw[keep[np.arange(len(arr)) % len(keep)]]
        c["arena"][c["slots"][k]:c["slots"][k] + arr.nbytes] = raw.reshape(-1)
    n = qc.check(emu, c)
    assert 70 <= n <= 70 + 64


@pytest.mark.parametrize("limit", [1, 37, 64, 100, 128, 164, 193, 194, 1000])
def test_limit_edges(emu, limit):
    """every row matches over chunks of 100, 64 and 30 rows (words 0-1, 2, 3): the limit of
    1, inside a word, at a word edge, at a chunk edge, at both, one under and at the total,
    above it"""
    c = qc.kernel_case(7, "abc", [100, 64, 30], query="a >= -1000", pred=lambda r: np.ones(len(r), bool))
    assert qc.check(emu, c, limit=limit) == min(limit, 194)
    c = qc.kernel_case(8, "e24", [100, 64, 30])
    qc.check(emu, c, limit=limit)


@pytest.mark.parametrize("first,step", [(0, 1), (1, 1), (0, 2), (1, 2), (0, 3), (2, 3)])
@pytest.mark.parametrize("name", ["abc", "u14", "pad"])
def test_selections(emu, name, first, step):
    c = qc.kernel_case(10 * first + step, name, [129, 64, 7], step=step, first=first)
    qc.check(emu, c)
    qc.check(emu, c, limit=70)


@pytest.mark.parametrize("nchunks", [1, 3, 17])
@pytest.mark.parametrize("name", list(qc.DTYPES))
def test_chunks_with_a_missing_one(emu, name, nchunks):
    counts = [(37 * (k + 1)) % 131 for k in range(nchunks)]
    c = qc.kernel_case(nchunks, name, counts, missing=nchunks // 2 if nchunks > 1 else None)
    qc.check(emu, c)
    qc.check(emu, c, limit=sum(counts) // 5 + 1)


@pytest.mark.parametrize("shift", [0, 1, 4, 8, 12])
@pytest.mark.parametrize("name,fields", [("abc", None), ("abc", ["b"]), ("u14", None), ("arrf", ["m"]),
                                         ("e24", ["x", "z"]), ("pad", None), ("pad", ["w"])])
def test_response_placement(emu, name, fields, shift):
    """the response `shift` bytes past a 16-byte boundary inside a guard-filled buffer, whole
    records and field subsets (qc.run checks the guards)"""
    c = qc.kernel_case(shift, name, [130, 3])
    qc.check(emu, c, fields=fields, shift=shift)


def test_padding_is_dropped_from_the_response(emu):
    dt = qc.DTYPES["pad"]
    segs, rsp = qry.query_segments(dt)
    assert rsp.itemsize == 8 + 1 + 8 + 2 and segs == [(0, 8, 1), (8, 9, 10)]
    assert rsp.names == ("index", "u", "v", "w")
    assert qry.query_dtype(np.dtype([("index", "i4"), ("_index", "i4")])).names[0] == "__index"


UPDATES = [("abc", {"a": 7}), ("abc", {"c": b"zz", "b": 1.5}), ("u14", {"f": -2.25}), ("u14", {"k": 1, "g": 3.0}),
           ("e24", {"y": -1}), ("pad", {"u": 3, "w": -1}), ("pad", {"v": 0.25})]


@pytest.mark.parametrize("limit", [0, 1, 40, 64])
@pytest.mark.parametrize("name,update", UPDATES)
def test_update(emu, name, update, limit):
    """field bytes change only in matched rows under the limit; padding, other fields and
    other rows stay (qc.check compares the whole arena)"""
    c = qc.kernel_case(len(update) + limit, name, [70, 0, 130], step=2, first=1, missing=None)
    n = qc.check(emu, c, limit=limit, update=update)
    assert n > 0


def _golden_ids(key):
    meta, _ = qc.goldens()
    return [f"{k}-{r['dtype']}-{r['query']}" for k, r in enumerate(meta[key])]


@pytest.mark.parametrize("k", range(len(qc.goldens()[0]["cases"])), ids=_golden_ids("cases"))
def test_golden_queries(emu, k):
    meta, arrs = qc.goldens()
    qc.check_golden(emu, meta["cases"][k], arrs.get(f"case_{k}"))


@pytest.mark.parametrize("k", range(len(qc.goldens()[0]["updates"])), ids=_golden_ids("updates"))
def test_golden_updates(emu, k):
    meta, arrs = qc.goldens()
    rec = meta["updates"][k]
    qc.check_golden(emu, rec, arrs[f"upd_{k}"], update=rec["update"], want_chunk=arrs[f"upd_chunk_{k}"])


def test_stepped_selection_deviation_is_recorded():
    """the reference's own output for rows 5, 7, 9 of a chunk at offset 20 under slice(1, 10, 2)
    style selections is on record: its indices differ from offset + start + i * step"""
    meta, arrs = qc.goldens()
    seen = 0
    for k, rec in enumerate(meta["cases"]):
        if rec["deviates"] != "stepped selection":
            continue
        arr = qc.golden_chunk(rec["dtype"])
        start, count, step, index0 = qc.golden_sel(rec, len(arr))
        idx = start + np.arange(count) * step
        ours = index0 + idx[qc.golden_mask(rec, arr[idx])]
        ref = arrs[f"case_{k}"].view(qc.pc.descr_dtype(rec["rsp_descr"]))["index"]
        assert len(ref) == len(ours) and (ref != ours).any() and (ref <= ours).all()
        seen += 1
    assert seen == 2


def test_isin_by_value(emu):
    dt = np.dtype([("f", "<f4"), ("d", "<f8"), ("i", "i1"), ("u", "<u8"), ("s", "S3")])
    a = np.zeros(9, dt)
    a["f"] = [0.0, -0.0, np.nan, 1.5, 2.5, np.inf, -np.inf, 0.1, 3.0]
    a["d"] = a["f"]
    a["i"] = [-128, -1, 0, 1, 127, 5, 6, 7, 8]
    a["u"] = [0, 1, 2 ** 63, 2 ** 64 - 1, 5, 6, 7, 8, 9]
    a["s"] = [b"a", b"ab", b"abc", b"", b"b", b"a\0b", b"ab", b"c", b"abd"]
    for q in ("where f in (0, nan, 2.5, inf)", "where f in (-0.0, 0.1)", "where d in (-inf, 0.1, 1.5)",
              "where i in (-128, 127, 0)", "where i in ('5', 8)", "where u in (18446744073709551615, 0, 9223372036854775808)",
              "where s in (ab, abcd, b'')", "where s in (b'a', c)"):
        cq = qry.compile_query(q, dt)
        field = qry.where_field_name(q)
        want = np.isin(a[field], np.array(qry.where_elements(q), dtype=dt[field]))
        assert (qc.row_mask(emu, a, cq) == want).all(), q


def test_argument_checks(emu):
    c = qc.kernel_case(1, "abc", [10])
    dt = c["dt"]
    table, nwords = qry.query_chunk_table([(c["slots"][0],) + c["sels"][0]])
    ok = c["cq"].prog
    assert not isinstance(emu.mask(c["arena"], table, nwords, 12, ok, None), int)

    def prog(*ops):
        p = nat.QueryProg()
        p.nops = len(ops)
        for k, kw in enumerate(ops[:nat.QUERY_MAX_OPS]):
            for name, v in kw.items():
                setattr(p.ops[k], name, v)
        return p
    cmp_a = dict(op=nat.Q_CMP, kind=2, off=0)
    bad = [prog(*([cmp_a] + [cmp_a, dict(op=nat.Q_AND)] * 16)),            # 33 operations
           prog(),                                                          # none
           prog(dict(op=nat.Q_CMP, kind=2, off=9)),                         # an i4 past a 12-byte row
           prog(dict(op=nat.Q_CMP, kind=3, off=8)),                         # an i8 past it
           prog(dict(op=nat.Q_CMP, kind=2, off=-1)),
           prog(dict(op=nat.Q_CMP_BYTES, kind=10, off=8, len=5, len_b=1)),  # an S5 past it
           prog(dict(op=nat.Q_CMP_BYTES, kind=10, off=8, len=4, off_b=250, len_b=7)),     # past the pool
           prog(dict(op=nat.Q_CMP_FIELD, kind=2, off=0, kind_b=3, off_b=8)),
           prog(dict(op=nat.Q_ISIN, kind=2, off=0, imm=2)),                 # elements past the buffer
           prog(dict(op=nat.Q_ISIN, kind=2, off=0, imm=2000)),
           prog(cmp_a, dict(op=nat.Q_AND)),                                 # stack underflow
           prog(cmp_a, cmp_a),                                              # two results
           prog(dict(op=9)), prog(dict(op=nat.Q_CMP, kind=11, off=0)), prog(dict(op=nat.Q_CMP, kind=2, cmp=6))]
    for p in bad:
        assert emu.mask(c["arena"], table, nwords, 12, p, None) == qc.ERR_ARG
    assert not isinstance(emu.mask(c["arena"], table, nwords, 12, prog(*([cmp_a] + [cmp_a, dict(op=nat.Q_AND)] * 15)),
                                   None), int)
    mask, count = emu.mask(c["arena"], table, nwords, 12, ok, None)
    base = np.cumsum(count, dtype=np.int64) - count
    out = np.zeros(20 * 10 + 16, np.uint8)
    good = [(0, 8, 12)]
    assert not isinstance(emu.emit(c["arena"], table, nwords, 12, mask, base, 0, good, 20, out, 0), int)
    for segs, E in ([(0, 0, 12)], 20), ([(0, 8, 13)], 21), ([(4, 8, 12)], 20), ([(0, 12, 4), (4, 8, 4)], 20), \
            ([(0, 8, 4), (4, 10, 4)], 20), ([(0, 8, 0)], 20), ([(0, 8 + k, 1) for k in range(17)], 32):
        assert emu.emit(c["arena"], table, nwords, 12, mask, base, 0, segs, E, out, 0) == qc.ERR_ARG, segs
    upd = np.zeros(4, np.uint8)
    assert emu.emit(c["arena"], table, nwords, 12, mask, base, 0, good, 20, out, 0, upd_segs=[(10, 0, 4)],
                    upd=upd) == qc.ERR_ARG
    assert emu.emit(c["arena"], table, nwords, 12, mask, base, -1, good, 20, out, 0) == qc.ERR_ARG
    assert dt.itemsize == 12
