"""Shared pieces of the query-selection tests (tests/test_query_compile.py,
tests/test_query_emu.py, tests/test_gpu_query.py): the reference goldens
(tests/golden/make_query_golden.py), a numpy model of the two kernels' contract
(include/hsds_amd.h hsds_query_mask / hsds_query_emit), the kernel cases, a thin driver for
the CPU emulator (tests/emu/query_emu.cpp) and the checks that run over any backend with the
emulator's two calls (the GPU tests pass one over the C ABI).  Test infrastructure only."""
import ctypes
import functools
import json
import os

import numpy as np

import points_cases as pc
from hsds_amd import _native as nat
from hsds_amd import query as qry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libquery_emu.so")
ERR_ARG = -6

# row sizes 12, 14 (an f4 at offset 2, an f8 at offset 6), 14 with an array field that is only
# copied, 24 and a padded 24; each with a query and the same predicate in numpy
DTYPES = {
    "abc": np.dtype([("a", "<i4"), ("b", "<f4"), ("c", "S4")]),
    "u14": np.dtype([("k", "<i2"), ("f", "<f4"), ("g", "<f8")]),
    "arrf": np.dtype([("k", "<i2"), ("m", "<f4", (3,))]),
    "e24": np.dtype([("x", "<f8"), ("y", "<i8"), ("z", "<f8")]),
    "pad": np.dtype([("u", "u1"), ("v", "<f8"), ("w", "<i2")], align=True),
}
QUERIES = {
    "abc": ("(a > 0) & (b < 5.0) | (c == b'ab')", lambda r: (r["a"] > 0) & (r["b"] < 5.0) | (r["c"] == b"ab")),
    "u14": ("(f > 0.5) | (g < -1.0) & (k >= 0)", lambda r: (r["f"] > 0.5) | (r["g"] < -1.0) & (r["k"] >= 0)),
    "arrf": ("k > 3", lambda r: r["k"] > 3),
    "e24": ("(x < 0) | (y > 500)", lambda r: (r["x"] < 0) | (r["y"] > 500)),
    "pad": ("(v < 0.5) & (w >= -100)", lambda r: (r["v"] < 0.5) & (r["w"] >= -100)),
}
NONE_ALL = {"abc": ("a > 1000", "a >= -1000"), "u14": ("k > 1000", "k <= 1000"), "arrf": ("k > 1000", "k != 1000"),
            "e24": ("y > 5000", "y < 5000"), "pad": ("w > 5000", "u >= 0")}
COUNTS = [0, 1, 63, 64, 65, 127, 128, 129, 4099]


@functools.lru_cache(maxsize=None)
def goldens():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "query_cases.json")))
    arrs = np.load(os.path.join(ROOT, "tests", "golden", "query_cases.npz"))
    return d, {k: arrs[k] for k in arrs.files}


def golden_chunk(name):
    meta, arrs = goldens()
    return arrs["chunk_" + name].copy().view(pc.descr_dtype(meta["dtypes"][name]))     # (padding bytes kept)


def golden_select(meta, rec):
    dt = pc.descr_dtype(meta["dtypes"][rec["dtype"]])
    return pc.subset_dtype(dt, rec["fields"]) if rec["fields"] else None


def golden_mask(rec, rows):
    """the rows of `rows` that the case's recorded eval string (BooleanParser.getEvalStr) and
    its where tail select, by numpy"""
    m = np.ones(len(rows), bool)
    if rec["eval_str"]:
        m &= eval(rec["eval_str"], {}, {n: rows[n] for n in rows.dtype.names})
    field = qry.where_field_name(rec["query"])
    if field:
        m &= np.isin(rows[field], np.array(qry.where_elements(rec["query"]), dtype=rows.dtype[field]))
    return m


def random_rows(dt, n, rng):
    a = np.zeros(n, dt)
    a.view(np.uint8)[...] = rng.integers(0, 256, a.view(np.uint8).shape, dtype=np.uint8)     # padding is random
    for name in dt.names:
        f = dt.fields[name][0]
        base = f.base if f.subdtype else f
        if base.kind == "f":
            a[name] = np.round(rng.normal(size=a[name].shape) * 2, 1).astype(base)
        elif base.kind == "i" and base.itemsize >= 2:
            a[name] = rng.integers(-900, 900, a[name].shape)
        elif base.kind == "S":
            a[name] = rng.choice(np.array([b"ab", b"abc", b"b", b""], base), n)
    return a


# ---- numpy model -----------------------------------------------------------------------
def model(chunks, sels, pred, dt, segs, out_elem, limit=0, upd_segs=None, upd=None):
    """chunks: structured arrays (None: no such object); sels: (first, count, step, index0)
    per chunk; pred: rows -> bool.  Returns (response bytes, chunks after the update, running
    match counts at the chunk boundaries)."""
    recs, after, starts, r = [], [], [0], 0
    for arr, (first, count, step, index0) in zip(chunks, sels):
        if arr is None:
            after.append(None)
            starts.append(starts[-1])
            continue
        raw = arr.view(np.uint8).reshape(len(arr), dt.itemsize).copy()     # (a structured copy drops the padding)
        new = raw.reshape(-1).view(dt)
        idx = first + np.arange(count) * step
        hits = idx[pred(arr[idx])] if count else idx
        starts.append(starts[-1] + len(hits))
        if limit:
            hits = hits[:max(limit - r, 0)]
        r += len(hits)
        if upd_segs is not None:
            for c, o, nb in upd_segs:
                raw[hits, c:c + nb] = upd[o:o + nb]
        rec = np.zeros((len(hits), out_elem), np.uint8)
        rec[:, :8] = (index0 + hits).astype("<u8").view(np.uint8).reshape(-1, 8)
        for c, o, nb in segs:
            rec[:, o:o + nb] = raw[hits, c:c + nb]
        recs.append(rec.reshape(-1))
        after.append(new)
    return (np.concatenate(recs) if recs else np.zeros(0, np.uint8)), after, np.array(starts, np.int64)


# ---- arena -----------------------------------------------------------------------------
def make_arena(chunks, rng, gap=40):
    """the chunk arrays in one guard-filled byte buffer at slots that are multiples of 4 only;
    returns (arena, slots) with slot -1 for a missing chunk"""
    parts, slots, pos = [rng.integers(0, 256, 4, dtype=np.uint8)], [], 4
    for arr in chunks:
        if arr is None:
            slots.append(-1)
            continue
        slots.append(pos)
        raw = arr.view(np.uint8).reshape(-1)
        pad = rng.integers(0, 256, gap + (-len(raw)) % 4, dtype=np.uint8)
        parts += [raw, pad]
        pos += len(raw) + len(pad)
    return np.concatenate(parts), slots


# ---- emulator ---------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Emu:
    """mask(arena, table, nwords, rowsize, prog, isin) -> (mask uint64, count int32) or the
    error code; emit(...) -> (out buffer after, arena after) or the error code"""

    def __init__(self):
        assert os.path.exists(EMU), "build() the emulators first (tests/emu/libquery_emu.so)"
        self.lib = ctypes.CDLL(EMU)
        P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        self.lib.emu_query_mask.argtypes = [P, P, I64, I64, I, P, P, I64, P, P]
        self.lib.emu_query_emit.argtypes = [P, P, I64, I64, I, P, P, I64, P, I, I, P, P, I, I, P]

    def mask(self, arena, table, nwords, rowsize, prog, isin):
        mask = np.zeros(max(nwords, 1), np.uint64)
        count = np.zeros(max(nwords, 1), np.int32)
        rc = self.lib.emu_query_mask(_p(arena), _p(table), len(table), nwords, rowsize, ctypes.byref(prog), _p(isin),
                                     0 if isin is None else len(isin), _p(mask), _p(count))
        return rc if rc else (mask[:nwords], count[:nwords])

    def emit(self, arena, table, nwords, rowsize, mask, base, limit, segs, out_elem, outbuf, shift, upd_segs=None,
             upd=None, lead=0):
        """the response goes to outbuf[lead:], which is placed `shift` bytes past a 16-byte
        boundary; the whole buffer comes back"""
        arena = arena.copy()
        buf = aligned_copy(outbuf, (shift - lead) % 16)
        rc = self.lib.emu_query_emit(_p(arena), _p(table), len(table), nwords, rowsize, _p(mask), _p(base), limit,
                                     nat.point_segs(segs), len(segs), out_elem, _p(buf[lead:]),
                                     None if upd_segs is None else nat.point_segs(upd_segs),
                                     0 if upd_segs is None else len(upd_segs), 0 if upd is None else len(upd), _p(upd))
        return rc if rc else (buf.copy(), arena)


def aligned_copy(buf, shift):
    """a copy of `buf` that starts `shift` bytes past a 16-byte boundary"""
    big = np.zeros(len(buf) + 32, np.uint8)
    o = (-big.ctypes.data) % 16 + shift
    v = big[o:o + len(buf)]
    v[:] = buf
    return v


def run(backend, arena, slots, sels, dt, cq, segs, out_elem, limit=0, upd_segs=None, upd=None, shift=4, guard=24):
    """mask, scan (numpy), emit over a backend: (response bytes, arena after, starts).  The
    response lies `shift` bytes past a 16-byte boundary inside a guard-filled buffer whose
    other bytes must stay as they were."""
    table, nwords = qry.query_chunk_table([(s,) + tuple(sel) for s, sel in zip(slots, sels)])
    res = backend.mask(arena, table, nwords, dt.itemsize, cq.prog, cq.isin)
    assert not isinstance(res, int), res
    mask, count = res
    assert (count == [bin(int(m)).count("1") for m in mask]).all()
    incl = np.cumsum(count, dtype=np.int64)
    base = incl - count
    total = int(incl[-1]) if nwords else 0
    nout = min(total, limit) if limit else total
    outbuf = np.full(guard + nout * out_elem + guard, 0xA5, np.uint8)
    if nwords == 0:
        return np.zeros(0, np.uint8), arena, np.zeros(len(table) + 1, np.int64)
    res = backend.emit(arena, table, nwords, dt.itemsize, mask, base, limit, segs, out_elem, outbuf, shift,
                       upd_segs=upd_segs, upd=upd, lead=guard)
    assert not isinstance(res, int), res
    out, after = res
    assert (out[:guard] == 0xA5).all() and (out[len(out) - guard:] == 0xA5).all()
    starts = np.concatenate([[0], incl])[np.minimum(np.append(table["word0"], nwords), nwords)]
    return out[guard:len(out) - guard], after, starts


def kernel_case(seed, name, counts, step=1, first=0, missing=None, query=None, pred=None):
    """chunks of counts[k] selected rows (rows first + i * step), chunk `missing` absent"""
    rng = np.random.default_rng(seed)
    dt = DTYPES[name]
    chunks, sels, index0 = [], [], 0
    for k, n in enumerate(counts):
        nrows = first + max(n - 1, 0) * step + 1 + int(rng.integers(0, 3))
        chunks.append(None if k == missing else random_rows(dt, nrows, rng))
        sels.append((first, n, step, index0))
        index0 += nrows
    arena, slots = make_arena(chunks, rng)
    q, p = QUERIES[name] if query is None else (query, pred)
    return {"dt": dt, "chunks": chunks, "sels": sels, "arena": arena, "slots": slots, "cq": qry.compile_query(q, dt),
            "pred": p}


def check(backend, c, limit=0, fields=None, update=None, shift=4):
    """one kernel case over a backend against the model"""
    dt = c["dt"]
    segs, rsp_dt = qry.query_segments(dt, pc.subset_dtype(dt, fields) if fields else None)
    upd_segs, upd = qry.update_record(dt, update) if update else (None, None)
    want, want_after, want_starts = model(c["chunks"], c["sels"], c["pred"], dt, segs, rsp_dt.itemsize, limit,
                                          upd_segs, upd)
    got, after, starts = run(backend, c["arena"], c["slots"], c["sels"], dt, c["cq"], segs, rsp_dt.itemsize,
                             limit=limit, upd_segs=upd_segs, upd=upd, shift=shift)
    assert (starts == want_starts).all(), (starts, want_starts)
    assert len(got) == len(want) and (got == want).all()
    # the arena: only the update's bytes of matched rows under the limit changed
    want_arena = c["arena"].copy()
    for s, a in zip(c["slots"], want_after):
        if a is not None:
            want_arena[s:s + a.nbytes] = a.view(np.uint8).reshape(-1)
    assert (after == want_arena).all()
    if not update:
        assert (after == c["arena"]).all()
    return len(want) // rsp_dt.itemsize


def row_mask(backend, arr, cq):
    """the program's verdict per row of one chunk array, through the mask pass alone"""
    table, nwords = qry.query_chunk_table([(0, 0, len(arr), 1, 0)])
    arena = arr.view(np.uint8).reshape(-1).copy()
    mask, _ = backend.mask(arena, table, nwords, arr.dtype.itemsize, cq.prog, cq.isin)
    bits = np.unpackbits(mask.view(np.uint8), bitorder="little")
    assert not bits[len(arr):].any()
    return bits[:len(arr)].astype(bool)


def golden_sel(rec, nrows):
    """(first, count, step, index0) of a golden case"""
    start, stop, step = slice(*rec["sel"]).indices(nrows) if rec["sel"] else (0, nrows, 1)
    return start, len(range(start, stop, step)), step, rec["cidx"] * nrows


def check_golden(backend, rec, want_bytes, update=None, want_chunk=None):
    """a golden case through the two kernels: against the reference's recorded response where
    the engine follows it, against the model over the recorded eval string where it deviates
    on purpose (stepped selections, updates under a partial selection)"""
    meta, _ = goldens()
    arr = golden_chunk(rec["dtype"])
    dt = arr.dtype
    cq = qry.compile_query(rec["query"], dt)
    assert cq.eval_str == rec["eval_str"]
    segs, rsp_dt = qry.query_segments(dt, golden_select(meta, rec))
    upd_segs, upd = qry.update_record(dt, update) if update else (None, None)
    sel = golden_sel(rec, len(arr))
    arena = arr.view(np.uint8).reshape(-1).copy()
    got, after, starts = run(backend, arena, [0], [sel], dt, cq, segs, rsp_dt.itemsize, limit=rec["limit"],
                             upd_segs=upd_segs, upd=upd)
    if rec.get("none"):
        assert starts[-1] == 0
        return
    assert rsp_dt == pc.descr_dtype(rec["rsp_descr"])
    if rec["deviates"]:
        want, want_after, _ = model([arr], [sel], lambda rows: golden_mask(rec, rows), dt, segs, rsp_dt.itemsize,
                                    rec["limit"], upd_segs, upd)
        assert (got == want).all() and (after == want_after[0].view(np.uint8)).all()
        return
    assert len(got) == len(want_bytes) and (got == want_bytes).all()
    if want_chunk is not None:
        # the reference's structured assignment leaves padding alone: compare the fields
        assert (after.view(dt) == want_chunk.view(dt)).all()
        pad = ~np.tile(pc.field_mask(dt), len(arr))
        assert (after[pad] == arena[pad]).all()
