"""Goldens for point selections, from the REFERENCE itself: hsds.util.chunkUtil.getChunkId
(chunkUtil.py:353-371, the SN's per-point chunk lookup of dset_lib.py:459-484),
chunkReadPoints (chunkUtil.py:998-1061) and chunkWritePoints (chunkUtil.py:1064-1148), with
select_dt = hsds.util.hdf5dtype.getSubType(dtype, fields) for the field subsets.  Run in
the build container only:  python tests/golden/make_points_golden.py

Outputs: points_cases.json (geometry, dtype descrs, recorded exception types) and
points_cases.npz (chunk arrays, points, values and expected outputs as raw bytes)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refshim  # noqa: E402,F401  (puts the reference on sys.path)

from hsds.util import chunkUtil as cu  # noqa: E402
from hsds.util.hdf5dtype import getSubType  # noqa: E402

DSET = "d-12345678-1234-1234-1234-1234567890ab"
GEOMS = {
    "g1": ((23,), (10,)),
    "g2": ((20, 11), (7, 5)),
    "g3": ((9, 7, 5), (4, 3, 2)),
    "g8": ((3, 2, 3, 2, 2, 3, 2, 2), (2, 1, 2, 2, 1, 2, 1, 2)),
}
DTYPES = {
    "u1": np.dtype("u1"), "i2": np.dtype("<i2"), "f4": np.dtype("<f4"), "f8": np.dtype("<f8"),
    "abc": np.dtype([("a", "<i4"), ("b", "<f4"), ("c", "S4")]),                       # 12 bytes
    "c16": np.dtype("<c16"),
    "e24": np.dtype([("x", "<f8"), ("y", "<i8"), ("z", "<f8")]),                      # 24 bytes
    "pad": np.dtype([("u", "u1"), ("v", "<f8"), ("w", "<i2")], align=True),           # 24 bytes, 13 of padding
    "arrf": np.dtype([("k", "<i2"), ("m", "<f4", (3,))]),                            # 14 bytes, an array field
}


def fill(dt, shape, rng):
    """random values; every byte of a compound (padding included) random first"""
    a = np.zeros(shape, dt)
    raw = a.reshape(-1).view(np.uint8)
    if dt.names:
        raw[...] = rng.integers(0, 256, raw.shape, dtype=np.uint8)
        for name in dt.names:
            f = dt.fields[name][0]
            base = f.base if f.subdtype else f
            if base.kind == "f":
                a[name] = np.round(rng.normal(size=a[name].shape) * 100, 1).astype(base)
    elif dt.kind == "f":
        a[...] = np.round(rng.normal(size=shape) * 100, 2)
    elif dt.kind == "c":
        a[...] = np.round(rng.normal(size=shape) * 100, 2) + 1j * np.round(rng.normal(size=shape), 2)
    else:
        raw[...] = rng.integers(0, 256, raw.shape, dtype=np.uint8)
    return a


def chunk_points(rng, dims, layout, cidx, n):
    """n points of the dataset inside chunk `cidx`, random order with repeats"""
    lo = [i * c for i, c in zip(cidx, layout)]
    hi = [min((i + 1) * c, d) for i, c, d in zip(cidx, layout, dims)]
    return np.stack([rng.integers(a, b, n) for a, b in zip(lo, hi)], axis=1).astype(np.uint64).reshape(n, len(dims))


def cid_of(cidx):
    return "c-" + DSET[2:] + "_" + "_".join(str(i) for i in cidx)


def write_points(pts, vals, rank, sdt):
    """the DN's write records (coord | value), chunk_dn.py:758-782"""
    rec = np.dtype([("coord", "<u8", (rank,)) if rank > 1 else ("coord", "<u8"), ("value", sdt)])
    arr = np.zeros(len(pts), rec)
    arr["coord"] = pts if rank > 1 else pts[:, 0]
    arr["value"] = vals
    return arr


def main():
    rng = np.random.default_rng(53)
    meta = {"dset": DSET, "geoms": {k: [list(d), list(c)] for k, (d, c) in GEOMS.items()},
            "dtypes": {k: np.lib.format.dtype_to_descr(v) for k, v in DTYPES.items()},
            "itemsizes": {k: v.itemsize for k, v in DTYPES.items()},
            "aligned": ["pad"], "locate": [], "read": [], "write": [], "errors": []}
    arrs = {}

    # ---- locate: getChunkId per point -------------------------------------------------
    for gname, (dims, layout) in GEOMS.items():
        for n in (1, 65, 4099 if gname == "g2" else 257):
            pts = np.stack([rng.integers(0, d, n) for d in dims], axis=1).astype(np.uint64)
            idx = np.zeros((n, len(dims)), np.int64)
            for i in range(n):
                cid = cu.getChunkId(DSET, int(pts[i, 0]) if len(dims) == 1 else pts[i], layout)
                idx[i] = [int(x) for x in cid.split("_")[1:]]
            name = f"loc_{gname}_{n}"
            arrs[name + "__pts"], arrs[name + "__idx"] = pts, idx
            meta["locate"].append({"name": name, "geom": gname})

    # ---- read / write ------------------------------------------------------------------
    plan = [("g1", (1,), "u1", 65, None), ("g1", (2,), "i2", 64, None), ("g1", (0,), "f4", 4099, None),
            ("g1", (1,), "abc", 63, None), ("g1", (1,), "f8", 1, None), ("g1", (0,), "f8", 0, None),
            ("g2", (1, 1), "f4", 65, None), ("g2", (2, 2), "f8", 63, None), ("g2", (0, 1), "abc", 4099, None),
            ("g2", (1, 0), "c16", 65, None), ("g2", (2, 1), "e24", 64, None), ("g2", (0, 0), "pad", 65, None),
            ("g2", (1, 1), "arrf", 63, None), ("g2", (1, 2), "i2", 4099, None), ("g2", (0, 2), "u1", 64, None),
            ("g3", (1, 1, 1), "f4", 65, None), ("g3", (2, 2, 2), "abc", 63, None), ("g3", (0, 1, 2), "e24", 65, None),
            ("g8", (1, 1, 1, 0, 1, 1, 0, 0), "f4", 64, None), ("g8", (0, 0, 0, 0, 0, 0, 0, 0), "abc", 65, None),
            ("g2", (1, 1), "abc", 65, ["a"]), ("g2", (1, 1), "abc", 63, ["a", "b"]),
            ("g2", (1, 1), "abc", 64, ["b", "c"]), ("g2", (1, 1), "abc", 65, ["c"]),
            ("g1", (1,), "abc", 65, ["a", "b"]), ("g3", (1, 0, 1), "abc", 65, ["a"]),
            ("g2", (0, 0), "pad", 63, ["u"]), ("g2", (0, 0), "pad", 63, ["u", "v"]),
            ("g2", (1, 1), "arrf", 64, ["k"])]
    for k, (gname, cidx, dn, n, fields) in enumerate(plan):
        dims, layout = GEOMS[gname]
        dt = DTYPES[dn]
        sdt = getSubType(dt, fields) if fields else dt
        cid = cid_of(cidx)
        chunk = fill(dt, layout, rng)
        pts = chunk_points(rng, dims, layout, cidx, n)
        base = {"geom": gname, "chunk_index": list(cidx), "chunk_id": cid, "dtype": dn, "fields": fields, "n": n,
                "select_descr": np.lib.format.dtype_to_descr(sdt), "select_itemsize": sdt.itemsize}
        # read
        name = f"read{k}"
        case = dict(base, name=name)
        arrs[name + "__chunk"] = chunk.reshape(-1).view(np.uint8).copy()
        arrs[name + "__pts"] = pts
        try:
            out = cu.chunkReadPoints(chunk_id=cid, chunk_layout=layout, chunk_arr=chunk, point_arr=pts,
                                     select_dt=sdt if fields else None)
            assert out.dtype == sdt and out.shape == (n,)
            arrs[name + "__out"] = np.ascontiguousarray(out).view(np.uint8).reshape(-1)
        except Exception as e:          # noqa: BLE001 - the reference's error is the golden
            case["error"] = type(e).__name__
        meta["read"].append(case)
        # write
        name = f"write{k}"
        case = dict(base, name=name)
        vals = fill(sdt, (n,), rng)
        parr = write_points(pts, vals, len(dims), sdt)
        arrs[name + "__chunk"] = chunk.reshape(-1).view(np.uint8).copy()
        arrs[name + "__pts"] = pts
        arrs[name + "__vals"] = np.ascontiguousarray(vals).view(np.uint8).reshape(-1)
        a2 = chunk.copy()
        try:
            cu.chunkWritePoints(chunk_id=cid, chunk_layout=layout, chunk_arr=a2, point_arr=parr,
                                select_dt=sdt if fields else None)
            arrs[name + "__out"] = a2.reshape(-1).view(np.uint8)
        except Exception as e:          # noqa: BLE001
            case["error"] = type(e).__name__
        meta["write"].append(case)

    # ---- host-side validation errors ---------------------------------------------------
    dims, layout = GEOMS["g2"]
    dt = DTYPES["f4"]
    chunk = fill(dt, layout, rng)
    cid = cid_of((1, 1))
    good = chunk_points(rng, dims, layout, (1, 1), 5)
    arrs["err__chunk"] = chunk.reshape(-1).view(np.uint8).copy()
    meta["err_chunk"] = {"geom": "g2", "chunk_id": cid, "dtype": "f4"}

    def rd(tag, **kw):
        args = dict(chunk_id=cid, chunk_layout=layout, chunk_arr=chunk, point_arr=good)
        args.update(kw)
        try:
            cu.chunkReadPoints(**args)
            err = None
        except Exception as e:          # noqa: BLE001
            err = type(e).__name__
        meta["errors"].append({"op": "read", "tag": tag, "error": err})

    rd("ok")
    rd("points_int64", point_arr=good.astype(np.int64))
    rd("points_1d", point_arr=good.reshape(-1))
    rd("points_rank3", point_arr=np.zeros((4, 3), np.uint64))
    rd("layout_rank1", chunk_layout=(7,))
    rd("chunk_rank0", chunk_arr=np.zeros((), dt))
    before = good.copy()
    before[2] = [6, 5]              # row before the corner (7, 5)
    rd("before_corner", point_arr=before)
    past = good.copy()
    past[3] = [14, 6]               # row 14 is the next chunk
    rd("past_chunk", point_arr=past)

    vals = fill(dt, (5,), rng)

    def wr(tag, parr, arr=None, **kw):
        a2 = (chunk if arr is None else arr).copy()
        args = dict(chunk_id=cid, chunk_layout=layout, chunk_arr=a2, point_arr=parr)
        args.update(kw)
        try:
            cu.chunkWritePoints(**args)
            err = None
        except Exception as e:          # noqa: BLE001
            err = type(e).__name__
        meta["errors"].append({"op": "write", "tag": tag, "error": err})

    ok = write_points(good, vals, 2, dt)
    wr("ok", ok)
    wr("points_2d", ok.reshape(5, 1))
    wr("not_compound", good)
    wr("coord_int64", ok.astype(np.dtype([("coord", "<i8", (2,)), ("value", dt)])))
    wr("coord_rank3", write_points(np.zeros((5, 3), np.uint64), vals, 3, dt))
    wr("value_dtype", ok.astype(np.dtype([("coord", "<u8", (2,)), ("value", "<f8")])))
    wr("chunk_rank0", ok, arr=np.zeros((), dt))
    wr("past_chunk", write_points(past, vals, 2, dt))
    c1, l1 = fill(dt, (10,), rng), (10,)
    p1 = np.array([[10], [19], [15]], np.uint64)

    def wr1(tag, pts):
        a2 = c1.copy()
        try:
            cu.chunkWritePoints(chunk_id=cid_of((1,)), chunk_layout=l1, chunk_arr=a2,
                                point_arr=write_points(pts, vals[:len(pts)], 1, dt))
            err = None
        except Exception as e:          # noqa: BLE001
            err = type(e).__name__
        meta["errors"].append({"op": "write1d", "tag": tag, "error": err})

    wr1("ok", p1)
    wr1("before_corner", np.array([[10], [9]], np.uint64))
    wr1("past_chunk", np.array([[10], [20]], np.uint64))

    with open(os.path.join(HERE, "points_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)
    np.savez_compressed(os.path.join(HERE, "points_cases.npz"), **arrs)
    for c in meta["read"] + meta["write"]:
        print(c["name"], c["geom"], c["dtype"], c["fields"], c["n"], c.get("error"))
    for c in meta["errors"]:
        print(c)


if __name__ == "__main__":
    main()
