"""Goldens for query selections, from the REFERENCE itself: hsds.util.chunkUtil.chunkQuery
(chunkUtil.py:1375-1569) fed with hsds.util.boolparser.BooleanParser(query).getEvalStr()
(plus the query's own `where ... in` tail), the form PUT_Chunk passes on
(chunk_dn.py:192-228), and select_dt = hsds.util.hdf5dtype.getSubType(dtype, fields).
Run in the build container only:  python tests/golden/make_query_golden.py

Outputs: query_cases.json (queries, eval strings, selections, recorded exception types and
messages) and query_cases.npz (chunk arrays and expected responses as raw bytes).

Cases with "deviates" record what the reference returns where the engine does something
else on purpose (DESIGN.md "Query selections"): stepped selections and updates under a
partial selection."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refshim  # noqa: E402,F401  (puts the reference on sys.path)

from hsds.util import chunkUtil as cu  # noqa: E402
from hsds.util.boolparser import BooleanParser  # noqa: E402
from hsds.util.hdf5dtype import getSubType  # noqa: E402

DSET = "d-12345678-1234-1234-1234-1234567890ab"
DTYPES = {
    "stock": np.dtype([("sym", "S4"), ("date", "S8"), ("open", "<i4"), ("close", "<f4")]),         # 20 bytes
    "abc": np.dtype([("a", "<i4"), ("b", "<f4"), ("c", "S4")]),                                    # 12 bytes
    "e24": np.dtype([("x", "<f8"), ("y", "<i8"), ("z", "<f8")]),                                   # 24 bytes
    "pad": np.dtype([("u", "u1"), ("v", "<f8"), ("w", "<i2")], align=True),                        # 24, 13 of padding
    "arrf": np.dtype([("k", "<i2"), ("m", "<f4", (3,))]),                                          # 14, array field
    "wide": np.dtype([("p", "i1"), ("q", "<u2"), ("r", "<i8"), ("s", "<u8"), ("t", "<f8"), ("n", "S3"),
                      ("g", "<u4"), ("h", "<i2")]),                                                # 8 fields, 36 bytes
}
N = 150          # rows per chunk array: three mask words, the last one partial


def make(name, rng):
    dt = DTYPES[name]
    a = np.zeros(N, dt)
    a.view(np.uint8)[...] = rng.integers(0, 256, a.view(np.uint8).shape, dtype=np.uint8)     # padding is random
    if name == "stock":
        a["sym"] = rng.choice(np.array([b"AAPL", b"IBM", b"GO", b"X"], "S4"), N)
        a["date"] = np.array([b"202001%02d" % (1 + i % 28) for i in range(N)], "S8")
        a["open"] = rng.integers(3000, 3200, N)
        a["close"] = np.round(a["open"] + rng.normal(size=N) * 20, 1)
    elif name == "abc":
        a["a"] = rng.integers(-50, 50, N)
        a["b"] = np.round(rng.normal(size=N) * 10, 1)
        a["c"] = rng.choice(np.array([b"ab", b"abc", b"abcd", b"b", b""], "S4"), N)
    elif name == "e24":
        a["x"] = np.round(rng.normal(size=N), 2)
        a["y"] = rng.integers(-1000, 1000, N)
        a["z"] = np.round(rng.normal(size=N) * 5, 1)
        a["z"][::17] = np.nan
    elif name == "pad":
        a["u"] = rng.integers(0, 256, N)
        a["v"] = np.round(rng.normal(size=N), 2)
        a["w"] = rng.integers(-300, 300, N)
    elif name == "arrf":
        a["k"] = rng.integers(-20, 20, N)
        a["m"] = np.round(rng.normal(size=(N, 3)), 1)
    else:
        a["p"] = rng.integers(-128, 128, N)
        a["q"] = rng.integers(0, 65536, N)
        a["r"] = rng.integers(-2 ** 40, 2 ** 40, N)
        a["s"] = rng.integers(0, 2 ** 50, N).astype("u8")
        a["t"] = np.round(rng.normal(size=N) * 100, 1)
        a["n"] = rng.choice(np.array([b"a", b"bb", b"ccc"], "S3"), N)
        a["g"] = rng.integers(0, 2 ** 32, N)
        a["h"] = rng.integers(-100, 100, N)
    return a


# (dtype, query, options): sel = (start, stop, step), fields = select_dt subset, limit, cidx = chunk index
CASES = [
    ("stock", "open == 3100", {}), ("stock", "open != 3100", {}), ("stock", "open < 3050", {}),
    ("stock", "open <= 3050", {}), ("stock", "open > 3150", {}), ("stock", "open >= 3150", {}),
    ("stock", "close > 3100.5", {}), ("stock", "3100 < open", {}),
    ("stock", "sym == b'AAPL'", {}), ("stock", "sym != b'AAPL'", {}), ("stock", "sym < b'H'", {}),
    ("stock", "sym >= b'GO'", {}), ("stock", "date > b'20200115'", {}),
    ("stock", "(sym == b'AAPL') & (open > 3100)", {}),
    ("stock", "(sym == b'AAPL') | (open > 3190)", {}),
    ("stock", "sym == b'AAPL' AND open > 3100", {}),
    ("stock", "sym == b'IBM' OR open < 3010 AND close > 3000", {}),
    ("stock", "open > 3100 & close < 3120", {}),
    ("stock", "((open > 3050) & (open < 3150)) | ((sym == b'X') & (close >= 3000.0))", {}),
    ("stock", "(open > 3050 AND (sym == b'GO' OR sym == b'X')) OR date == b'20200101'", {}),
    ("stock", "open > close", {}), ("stock", "sym == 'AAPL'", {}), ("stock", "open > 5000", {}),
    ("stock", "where sym in (b'AAPL', b'GO')", {}), ("stock", "where sym in (AAPL, X)", {}),
    ("stock", "where sym in ('IBM')", {}), ("stock", "where open in (3001, 3100, 3150, 3199)", {}),
    ("stock", "where sym in (b'ZZZZ')", {}), ("stock", "where 'sym' in (b'AAPLXX')", {}),
    ("stock", "open > 3100 where sym in (b'AAPL', b'IBM')", {}),
    ("stock", "open > 5000 where sym in (b'AAPL')", {}),
    ("stock", "(open > 3100) & (close < 3150) where sym in (GO)", {"limit": 3}),
    ("stock", "open > 3050", {"limit": 1}), ("stock", "open > 3050", {"limit": 64}),
    ("stock", "open > 3050", {"limit": 1000}), ("stock", "open >= 3000", {"limit": 128}),
    ("stock", "open > 3100", {"fields": ["open"]}), ("stock", "open > 3100", {"fields": ["sym", "close"]}),
    ("stock", "sym == b'GO'", {"fields": ["date", "open"], "limit": 5, "cidx": 3}),
    ("stock", "open > 3100", {"cidx": 7}), ("stock", "open > 3100", {"sel": (0, 70, 1), "cidx": 2}),
    ("stock", "open > 3100", {"sel": (10, 140, 1), "cidx": 1}),
    ("stock", "open > 3100", {"sel": (1, 150, 2), "cidx": 1, "deviates": "stepped selection"}),
    ("stock", "open > 3100", {"sel": (5, 149, 3), "deviates": "stepped selection"}),
    ("abc", "a > 0", {}), ("abc", "b <= -2.5", {}), ("abc", "c == b'ab'", {}), ("abc", "c > b'ab'", {}),
    ("abc", "c <= b'abc'", {}), ("abc", "c == b'abcde'", {}), ("abc", "c < b'abcde'", {}),
    ("abc", "(a > -10) & (a < 10) & (b > 0)", {}), ("abc", "a < b", {}),
    ("abc", "where c in (ab, b)", {"fields": ["a"]}),
    ("e24", "x > 0.5", {}), ("e24", "y >= -3", {}), ("e24", "z != 0.0", {}), ("e24", "z < 100", {}),
    ("e24", "(x < 0) | (y > 500)", {"fields": ["y", "z"]}), ("e24", "x < z", {}),
    ("e24", "where y in (1, 2, 3, 4, 5, -7, 100)", {}),
    ("pad", "u > 128", {}), ("pad", "(v < 0.5) & (w >= -100)", {}), ("pad", "u < w", {}),
    ("pad", "w == 7", {"fields": ["u", "w"]}), ("pad", "where u in (1, 2, 3, 4, 5, 6, 7, 8, 9, 200)", {}),
    ("arrf", "k > 3", {}), ("arrf", "k <= -3", {"fields": ["m"]}),
    ("wide", "p < 0", {}), ("wide", "q >= 32768", {}), ("wide", "r > 0", {}), ("wide", "s < 562949953421312", {}),
    ("wide", "t > 12.5", {}), ("wide", "n == b'bb'", {}), ("wide", "g > 2147483648", {}),
    ("wide", "(p > 0) & (h < 0) | (n != b'a')", {"fields": ["p", "n", "h"]}), ("wide", "p < h", {}),
    ("wide", "q < g", {}), ("wide", "r < s", {}), ("wide", "where n in (a, ccc)", {"limit": 10}),
]

UPDATES = [
    ("stock", "open > 3150", {"open": 1}, {}),
    ("stock", "sym == b'GO'", {"sym": "NEW", "close": 1.5}, {"limit": 4}),
    ("stock", "open > 5000", {"open": 1}, {}),
    ("pad", "u > 200", {"w": -1, "u": 3}, {"cidx": 2}),
    ("stock", "open > 3150", {"open": 1}, {"sel": (10, 150, 1), "deviates": "update under a partial selection"}),
    ("stock", "open > 3150", {"close": 2.5}, {"sel": (0, 150, 2), "deviates": "update under a partial selection"}),
]

ERRORS = [
    ("stock", "foo > 5", {}), ("stock", "open > 5)", {}), ("stock", "(open > 5", {}), ("stock", "5 > 3", {}),
    ("stock", "sym == b'AAPL", {}), ("stock", "open > 5 where ", {}), ("stock", "where  in (1)", {}),
    ("stock", "where 'sym in (1)", {}), ("stock", "where sym (b'A')", {}), ("stock", "where sym in b'A'", {}),
    ("stock", "where sym in (b'A)", {}), ("stock", "where sym in ('A)')", {}), ("stock", "where foo in (1, 2)", {}),
    ("stock", "where sym in ()", {}), ("stock", "where open in (1, x)", {}),
    ("stock", "open > 1", {"rank2": True}), ("stock", "open > 1", {"notarray": True}),
    ("stock", "open > 1", {"sel2": True}),
    ("stock", "open > 1 where sym in (GO)", {"update": {"open": 1}}), ("stock", "open > 1", {"update": {"nofield": 1}}),
    ("stock", "sym < 'AAPL'", {}),
]


def cid_of(i):
    return "c-" + DSET[2:] + "_" + str(i)


def ref_query(query):
    """the text chunkQuery gets: getEvalStr of the expression, then the query's own where tail"""
    if query.startswith("where "):
        return query, None
    es = BooleanParser(query).getEvalStr()
    n = query.find(" where ")
    # (in parentheses: _getEvalStr never closes a field name that ends the text, so `a < b` would
    # reach eval as `a < ` -- chunkUtil.py:1298-1307 flush a name only at the next character)
    text = "(" + es + ")"
    return (text + query[n:] if n > 0 else text), es


def main():
    rng = np.random.default_rng(71)
    chunks = {k: make(k, rng) for k in DTYPES}
    arrs = {"chunk_" + k: v.view(np.uint8).reshape(-1).copy() for k, v in chunks.items()}
    meta = {"dset": DSET, "rows": N, "dtypes": {k: np.lib.format.dtype_to_descr(v) for k, v in DTYPES.items()},
            "aligned": ["pad"], "cases": [], "updates": [], "errors": []}

    def common(name, query, opt):
        sel = opt.get("sel")
        cidx = opt.get("cidx", 0)
        kw = {"chunk_id": cid_of(cidx), "chunk_layout": (N,), "chunk_arr": chunks[name].copy(),
              "slices": [slice(*sel)] if sel else None, "limit": opt.get("limit", 0)}
        if opt.get("fields"):
            kw["select_dt"] = getSubType(DTYPES[name], opt["fields"])
        rec = {"dtype": name, "query": query, "sel": list(sel) if sel else None, "cidx": cidx,
               "limit": opt.get("limit", 0), "fields": opt.get("fields"), "deviates": opt.get("deviates")}
        return kw, rec

    for k, (name, query, opt) in enumerate(CASES):
        kw, rec = common(name, query, opt)
        kw["query"], rec["eval_str"] = ref_query(query)
        rsp = cu.chunkQuery(**kw)
        rec["none"] = rsp is None
        if rsp is not None:
            rec["rsp_descr"] = np.lib.format.dtype_to_descr(rsp.dtype)
            rec["nrows"] = len(rsp)
            arrs[f"case_{k}"] = np.ascontiguousarray(rsp).view(np.uint8).reshape(-1).copy()
        meta["cases"].append(rec)

    for k, (name, query, upd, opt) in enumerate(UPDATES):
        kw, rec = common(name, query, opt)
        kw["query"], rec["eval_str"] = ref_query(query)
        kw["query_update"] = upd
        rec["update"] = upd
        rsp = cu.chunkQuery(**kw)
        rec["rsp_descr"] = np.lib.format.dtype_to_descr(rsp.dtype)
        rec["nrows"] = len(rsp)
        arrs[f"upd_{k}"] = np.ascontiguousarray(rsp).view(np.uint8).reshape(-1).copy()
        arrs[f"upd_chunk_{k}"] = kw["chunk_arr"].view(np.uint8).reshape(-1).copy()
        meta["updates"].append(rec)

    for name, query, opt in ERRORS:
        kw, rec = common(name, query, opt)
        kw["query"] = query
        for flag in ("rank2", "notarray", "sel2"):
            rec[flag] = bool(opt.get(flag))
        if opt.get("rank2"):
            kw["chunk_arr"] = kw["chunk_arr"].reshape(N // 2, 2)
        if opt.get("notarray"):
            kw["chunk_arr"] = kw["chunk_arr"].tolist()
        if opt.get("sel2"):
            kw["slices"] = [slice(0, 5, 1), slice(0, 1, 1)]
        if opt.get("update"):
            kw["query_update"] = rec["update"] = opt["update"]
        try:
            cu.chunkQuery(**kw)
        except Exception as e:
            rec["error"] = type(e).__name__
            rec["bases"] = [b.__name__ for b in type(e).__mro__]
            rec["message"] = str(e)
        else:
            raise SystemExit(f"no error from the reference for {query!r} {opt}")
        meta["errors"].append(rec)

    with open(os.path.join(HERE, "query_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)
    np.savez_compressed(os.path.join(HERE, "query_cases.npz"), **arrs)
    print(len(meta["cases"]), "cases,", len(meta["updates"]), "updates,", len(meta["errors"]), "errors")


if __name__ == "__main__":
    main()
