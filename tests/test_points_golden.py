"""Point selections against the REFERENCE's own results (tests/golden/points_cases.*,
written by tests/golden/make_points_golden.py from hsds.util.chunkUtil getChunkId,
chunkReadPoints and chunkWritePoints): the kernels of hsds_amd/csrc/points.h run thread by
thread on CPU (tests/emu/points_emu.cpp), and the host-side validation of
hsds_amd.selection.chunkReadPoints / chunkWritePoints raises the recorded exception types.

Field subsets: the reference's write is only right for a prefix of the dataset's fields (it
pairs the subset's values with the dataset's field names by position), so write goldens are
taken for whole elements and prefix subsets; other subsets are checked against the numpy
model in tests/test_points_emu.py.  Padding bytes of an align=True compound are
indeterminate in the reference (numpy moves structured elements field by field into
uninitialised memory): a read must give zeros there, as the golden does, and a write must
leave the chunk's padding bytes alone."""
import numpy as np
import pytest

import points_cases as pc

META, ARRS = pc.goldens()


@pytest.fixture(scope="module")
def emu():
    return pc.Emu()


def _geom(case):
    dims, layout = META["geoms"][case["geom"]]
    return tuple(dims), tuple(layout)


def _case_setup(emu, case, kind):
    """segment table, element offsets of the case's points (emulated locate over the whole
    dataset: every point must fall in the case's chunk)"""
    from hsds_amd.selection import point_segments
    dims, layout = _geom(case)
    dt = pc.golden_dtype(META, case["dtype"])
    sdt = pc.descr_dtype(case["select_descr"]) if case["fields"] else None
    segs, out_dt = point_segments(dt, sdt)
    assert out_dt.itemsize == case["select_itemsize"]
    pts = ARRS[case["name"] + "__pts"].reshape(-1, len(dims))
    chunk, eoff, nbad = emu.locate(dims, layout, dt.itemsize, pts)
    grid = [-(-d // c) for d, c in zip(dims, layout)]
    assert nbad == 0
    assert (chunk == np.ravel_multi_index(case["chunk_index"], grid)).all()
    return dt, out_dt, segs, eoff


@pytest.mark.parametrize("case", META["locate"], ids=lambda c: c["name"])
def test_locate_matches_getChunkId(emu, case):
    dims, layout = _geom(case)
    pts, idx = ARRS[case["name"] + "__pts"], ARRS[case["name"] + "__idx"]
    chunk, eoff, nbad = emu.locate(dims, layout, 4, pts)
    grid = [-(-d // c) for d, c in zip(dims, layout)]
    assert nbad == 0
    assert (np.stack(np.unravel_index(chunk, grid), axis=1) == idx).all()
    rel = pts.astype(np.int64) - idx * np.array(layout)
    assert (eoff == 4 * np.ravel_multi_index(tuple(rel.T), layout)).all()


@pytest.mark.parametrize("case", META["read"], ids=lambda c: c["name"])
def test_gather_matches_chunkReadPoints(emu, case):
    assert "error" not in case
    dt, out_dt, segs, eoff = _case_setup(emu, case, "read")
    want = ARRS[case["name"] + "__out"]
    chunk = ARRS[case["name"] + "__chunk"]
    for shift in (0, 4):
        got = emu.gather(chunk, [0], None, eoff, segs, dt.itemsize, out_dt.itemsize, None,
                         np.full(want.size, 0xA5, np.uint8), shift=shift)
        assert (got == want).all(), (case["name"], shift)
    # through dst_index (the identity here), the element-per-lane path
    got = emu.gather(chunk, [0], None, eoff, segs, dt.itemsize, out_dt.itemsize, None,
                     np.full(want.size, 0xA5, np.uint8), dst_index=np.arange(case["n"]), shift=4)
    assert (got == want).all(), case["name"]


def _prefix(case):
    dt = pc.golden_dtype(META, case["dtype"])
    return not case["fields"] or list(dt.names[:len(case["fields"])]) == list(case["fields"])


@pytest.mark.parametrize("case", [c for c in META["write"] if _prefix(c)], ids=lambda c: c["name"])
def test_scatter_matches_chunkWritePoints(emu, case):
    assert "error" not in case
    dt, val_dt, segs, eoff = _case_setup(emu, case, "write")
    chunk0, want = ARRS[case["name"] + "__chunk"], ARRS[case["name"] + "__out"]
    vals = ARRS[case["name"] + "__vals"]
    order = pc.sort_order(None, eoff, chunk0.size)
    got = emu.scatter(chunk0, [0], None, eoff, order, segs, dt.itemsize, val_dt.itemsize, vals)
    mask = np.tile(pc.field_mask(dt), chunk0.size // dt.itemsize)
    assert (got[mask] == want[mask]).all(), case["name"]
    assert (got[~mask] == chunk0[~mask]).all(), "padding bytes of the chunk were written"


def test_reference_defect_is_recorded():
    """the non-prefix subset (b, c) raised in the reference, and (c) silently wrote nothing"""
    by = {tuple(c["fields"] or ()): c for c in META["write"] if c["dtype"] == "abc" and c["geom"] == "g2"}
    assert by[("b", "c")].get("error") == "ValueError"
    c = by[("c",)]
    assert (ARRS[c["name"] + "__out"] == ARRS[c["name"] + "__chunk"]).all()


# ---- host-side validation (no GPU: every case raises before a device is needed) ---------
def _err_inputs():
    e = META["err_chunk"]
    dims, layout = META["geoms"][e["geom"]]
    dt = pc.golden_dtype(META, e["dtype"])
    chunk = ARRS["err__chunk"].view(dt).reshape(layout).copy()
    good = np.array([[7, 5], [13, 9], [8, 6], [10, 7], [7, 9]], np.uint64)
    return e["chunk_id"], tuple(layout), dt, chunk, good


def _write_points(pts, vals, rank, sdt, coord="<u8"):
    rec = np.dtype([("coord", coord, (rank,)) if rank > 1 else ("coord", coord), ("value", sdt)])
    arr = np.zeros(len(pts), rec)
    arr["coord"] = pts if rank > 1 else pts[:, 0]
    arr["value"] = vals
    return arr


def _read_args(tag):
    cid, layout, dt, chunk, good = _err_inputs()
    args = dict(chunk_id=cid, chunk_layout=layout, chunk_arr=chunk, point_arr=good)
    if tag == "points_int64":
        args["point_arr"] = good.astype(np.int64)
    elif tag == "points_1d":
        args["point_arr"] = good.reshape(-1)
    elif tag == "points_rank3":
        args["point_arr"] = np.zeros((4, 3), np.uint64)
    elif tag == "layout_rank1":
        args["chunk_layout"] = (7,)
    elif tag == "chunk_rank0":
        args["chunk_arr"] = np.zeros((), dt)
    elif tag == "before_corner":
        args["point_arr"] = good.copy()
        args["point_arr"][2] = [6, 5]
    elif tag == "past_chunk":
        args["point_arr"] = good.copy()
        args["point_arr"][3] = [14, 6]
    return args


def _write_args(tag):
    cid, layout, dt, chunk, good = _err_inputs()
    vals = np.arange(5, dtype=dt)
    ok = _write_points(good, vals, 2, dt)
    args = dict(chunk_id=cid, chunk_layout=layout, chunk_arr=chunk, point_arr=ok)
    if tag == "points_2d":
        args["point_arr"] = ok.reshape(5, 1)
    elif tag == "not_compound":
        args["point_arr"] = good
    elif tag == "coord_int64":
        args["point_arr"] = _write_points(good.astype(np.int64), vals, 2, dt, coord="<i8")
    elif tag == "coord_rank3":
        args["point_arr"] = _write_points(np.zeros((5, 3), np.uint64), vals, 3, dt)
    elif tag == "value_dtype":
        args["point_arr"] = _write_points(good, vals, 2, np.dtype("<f8"))
    elif tag == "chunk_rank0":
        args["chunk_arr"] = np.zeros((), dt)
    elif tag == "past_chunk":
        past = good.copy()
        past[3] = [14, 6]
        args["point_arr"] = _write_points(past, vals, 2, dt)
    return args


def _write1d_args(tag):
    _, _, dt, _, _ = _err_inputs()
    pts = {"before_corner": [[10], [9]], "past_chunk": [[10], [20]]}[tag]
    pts = np.array(pts, np.uint64)
    cid = "c-" + META["dset"][2:] + "_1"
    return dict(chunk_id=cid, chunk_layout=(10,), chunk_arr=np.zeros(10, dt),
                point_arr=_write_points(pts, np.ones(len(pts), dt), 1, dt))


ERRORS = [c for c in META["errors"] if c["error"]]


@pytest.mark.parametrize("case", ERRORS, ids=lambda c: c["op"] + "-" + c["tag"])
def test_validation_errors_match_the_reference(case):
    from hsds_amd import selection as sel
    exc = {"ValueError": ValueError, "IndexError": IndexError}[case["error"]]
    if case["op"] == "read":
        with pytest.raises(exc):
            sel.chunkReadPoints(**_read_args(case["tag"]))
        return
    args = _write_args(case["tag"]) if case["op"] == "write" else _write1d_args(case["tag"])
    before = args["chunk_arr"].copy()
    with pytest.raises(exc):
        sel.chunkWritePoints(**args)
    assert np.array_equal(args["chunk_arr"], before)          # a write that raises modifies nothing


def test_every_recorded_error_is_covered():
    tags = {(c["op"], c["tag"]) for c in ERRORS}
    assert tags == {("read", t) for t in ("points_int64", "points_1d", "points_rank3", "layout_rank1", "chunk_rank0",
                                          "before_corner", "past_chunk")} | \
        {("write", t) for t in ("points_2d", "not_compound", "coord_int64", "coord_rank3", "value_dtype",
                                "chunk_rank0", "past_chunk")} | \
        {("write1d", t) for t in ("before_corner", "past_chunk")}
