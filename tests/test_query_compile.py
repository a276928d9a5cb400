"""The host query compiler (hsds_amd/query.py) on CPU: the parser against the eval strings
and the errors the reference recorded (tests/golden/make_query_golden.py), and the constant
conversion against numpy itself -- every field kind and operator with literals at and just
outside the dtype's limits, 2^53 + 1 against int64, NaN, infinities, -0.0, float32 rounding,
S fields with trailing NULs and longer literals, field against field.  The compiled programs
are run by the CPU emulation of the kernels (tests/emu/query_emu.cpp)."""
import operator
import warnings

import numpy as np
import pytest

import query_cases as qc
from hsds_amd import _native as nat
from hsds_amd import query as qry
from hsds_amd import selection

OPS = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt,
       ">=": operator.ge}


@pytest.fixture(scope="module")
def emu():
    return qc.Emu()


def test_eval_strings_match_the_reference():
    meta, _ = qc.goldens()
    n = 0
    for rec in meta["cases"] + meta["updates"]:
        dt = qc.golden_chunk(rec["dtype"]).dtype
        cq = qry.compile_query(rec["query"], dt)
        assert cq.eval_str == rec["eval_str"], rec["query"]
        n += rec["eval_str"] is not None
    assert n > 60


@pytest.mark.parametrize("k", range(len(qc.goldens()[0]["errors"])))
def test_errors_match_the_reference(k):
    """every recorded error is raised before the GPU is touched, with the reference's type
    (or a base of it: numpy's UFuncTypeError is a TypeError) and, for a bad request, its text"""
    meta, _ = qc.goldens()
    rec = meta["errors"][k]
    arr = qc.golden_chunk(rec["dtype"])
    n = len(arr)
    kw = {"chunk_id": "c-" + meta["dset"][2:] + "_" + str(rec["cidx"]), "chunk_layout": (n,), "chunk_arr": arr,
          "query": rec["query"], "query_update": rec.get("update")}
    if rec["rank2"]:
        kw["chunk_arr"] = arr.reshape(n // 2, 2)
    if rec["notarray"]:
        kw["chunk_arr"] = arr.tolist()
    if rec["sel2"]:
        kw["slices"] = [slice(0, 5, 1), slice(0, 1, 1)]
    with pytest.raises(Exception) as info:
        selection.chunkQuery(**kw)
    assert type(info.value).__name__ in rec["bases"] and type(info.value) is not Exception, (rec, info.value)
    if rec["error"] == "ValueError" or rec["notarray"]:
        assert str(info.value) == rec["message"]


def test_where_scanning():
    assert qry.where_field_name("open > 1") is None
    assert qry.where_field_name("open > 1 where sym in (a)") == "sym"
    assert qry.where_field_name("where 'my field' in (1)") == "my field"
    assert qry.where_elements("where s in (b'AA', 'b c', \"d\", e f, 12, )") == [b"AA", "b c", "d", "ef", "12"]
    assert qry.where_elements("where s in (b'a b',b\"c\", '')") == [b"a b", b"c", ""]
    cq = qry.compile_query("where open in (3, 1, 2, 3, 1)", np.dtype([("open", "<i4")]))
    assert cq.prog.nops == 1 and cq.prog.ops[0].imm == 3 and not cq.has_expr and cq.where_field == "open"
    assert (cq.isin.view("<i8") == [1, 2, 3]).all()


def test_literal_text_decides_int_or_float():
    dt = np.dtype([("a", "<i8")])
    o = qry.compile_query("a > 5", dt).prog.ops[0]
    assert (o.op, o.dom, o.imm) == (nat.Q_CMP, nat.Q_DOM_I64, 5)
    o = qry.compile_query("a > 5.0", dt).prog.ops[0]
    assert (o.op, o.dom) == (nat.Q_CMP, nat.Q_DOM_F64)
    o = qry.compile_query("5 > a", dt).prog.ops[0]
    assert (o.cmp, o.imm) == (nat.Q_LT, 5)
    # a condition over constants folds on the host
    p = qry.compile_query("(a > 1) & (3 > 2)", dt).prog
    assert p.nops == 3 and (p.ops[1].op, p.ops[1].imm) == (nat.Q_CONST, 1)
    # an int literal outside the dtype's range folds too
    p = qry.compile_query("a < 9223372036854775808", dt).prog
    assert (p.ops[0].op, p.ops[0].imm) == (nat.Q_CONST, 1)


KINDS = ["i1", "<i2", "<i4", "<i8", "u1", "<u2", "<u4", "<u8", "<f4", "<f8"]


def _values(dt):
    dt = np.dtype(dt)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        vals = [info.min, info.min + 1, -1 if dt.kind == "i" else 1, 0, 1, 2, 100, info.max - 1, info.max]
        if dt.itemsize == 8:
            vals += [2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2] + ([-2 ** 53 - 1] if dt.kind == "i" else [2 ** 63, 2 ** 63 + 1])
        return np.array(vals, dt)
    return np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 0.1, -0.1, 1.0, 1.5, 16777216.0, 16777218.0, 127.0, 128.0,
                     -129.0, 255.0, 3.4028234663852886e38, 1e-45, 2.0 ** 53, 2.0 ** 63, 2.0 ** 64], dt)


def _literals(dt):
    dt = np.dtype(dt)
    lits = ["0", "1", "-1", "2", "100", "0.0", "-0.0", "0.5", "1.5", "0.1", "nan", "inf", "-inf", "16777217",
            "16777217.0", "127", "128", "-128", "-129", "255", "256", "1e39", "-1e39", "1e-46"]
    if dt.kind in "iu":
        info = np.iinfo(dt)
        lits += [str(v) for v in (info.min - 1, info.min, info.min + 1, info.max - 1, info.max, info.max + 1)]
        lits += [str(float(info.max)), str(float(info.min))]
    lits += ["9007199254740993", "9007199254740993.0", "9007199254740992", "18446744073709551615",
             "18446744073709551616", "-9223372036854775808", "-9223372036854775809", "9223372036854775808.0"]
    return lits


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("kind", KINDS)
def test_constant_conversion_matrix(emu, kind, op):
    """field kind x operator x literal: the compiled program gives what numpy gives for the
    same Python literal"""
    vals = _values(kind)
    arr = np.zeros(len(vals), np.dtype([("pad", "u1"), ("f", kind)]))      # (the field is unaligned)
    arr["f"] = vals
    for text in _literals(kind):
        lit = int(text) if text.lstrip("-").isdigit() else float(text)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            want = OPS[op](arr["f"], lit)
        got = qc.row_mask(emu, arr, qry.compile_query(f"f {op} {text}", arr.dtype))
        assert (got == want).all(), (kind, op, text, vals[got != want])
        # the literal on the left
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            want = OPS[op](lit, arr["f"])
        got = qc.row_mask(emu, arr, qry.compile_query(f"{text} {op} f", arr.dtype))
        assert (got == want).all(), (kind, op, text, "left")


PAIRS = [("<i4", "<u4"), ("<i8", "<u8"), ("<f4", "<i2"), ("<f4", "<i4"), ("<u8", "i1"), ("<i8", "<f4"),
         ("<u2", "<u8"), ("i1", "<i8"), ("<f8", "<u8"), ("<f4", "<f8"), ("u1", "<u2")]


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("ka,kb", PAIRS)
def test_field_against_field(emu, ka, kb, op):
    """np.result_type of the two fields picks the domain"""
    va, vb = _values(ka), _values(kb)
    a, b = np.meshgrid(va, vb, indexing="ij")
    arr = np.zeros(a.size, np.dtype([("p", "u1"), ("a", ka), ("b", kb)]))
    arr["a"], arr["b"] = a.reshape(-1), b.reshape(-1)
    with np.errstate(all="ignore"):
        want = OPS[op](arr["a"], arr["b"])
    got = qc.row_mask(emu, arr, qry.compile_query(f"a {op} b", arr.dtype))
    assert (got == want).all(), (ka, kb, op)


@pytest.mark.parametrize("op", list(OPS))
def test_bytes_fields(emu, op):
    """numpy's order: bytes compared after trailing NULs are stripped; a literal longer than
    the field; S against S of another width"""
    vals = [b"", b"a", b"ab", b"ab\0", b"abc", b"abcd", b"ab\0d", b"b", b"\xff", b"abd", b"aa", b"ab\0\0"]
    arr = np.zeros(len(vals) ** 2, np.dtype([("n", "<i2"), ("c", "S4"), ("d", "S6")]))
    c, d = np.meshgrid(np.array(vals, "S4"), np.array(vals + [b"abcd\0x"], "S6")[1:], indexing="ij")
    arr["c"], arr["d"] = c.reshape(-1), d.reshape(-1)
    for lit in (b"ab", b"ab\x00", b"ab\x00\x00\x00\x00\x00", b"abcd", b"abcde", b"abcd\x00x", b"abc\x00e", b"a", b"\xff\xff",
                b"ab\x00d", b"zzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzz"):
        want = OPS[op](arr["c"], lit)
        got = qc.row_mask(emu, arr, qry.compile_query(f"c {op} {lit!r}", arr.dtype))
        assert (got == want).all(), (op, lit)
        want = OPS[op](lit, arr["c"])
        got = qc.row_mask(emu, arr, qry.compile_query(f"{lit!r} {op} c", arr.dtype))
        assert (got == want).all(), (op, lit, "left")
    want = OPS[op](arr["c"], arr["d"])
    got = qc.row_mask(emu, arr, qry.compile_query(f"c {op} d", arr.dtype))
    assert (got == want).all()


def test_str_literal_against_bytes_field(emu):
    """numpy 2 compares a str with an S field unequal everywhere and has no ordering for them
    (the goldens record both)"""
    arr = np.zeros(3, np.dtype([("c", "S4"), ("a", "<i4")]))
    arr["c"] = [b"ab", b"abc", b""]
    assert not qc.row_mask(emu, arr, qry.compile_query("c == 'ab'", arr.dtype)).any()
    assert qc.row_mask(emu, arr, qry.compile_query("c != 'ab'", arr.dtype)).all()
    assert not qc.row_mask(emu, arr, qry.compile_query("a == 'ab'", arr.dtype)).any()
    for q in ("c < 'ab'", "c >= 'ab'", "a > b'x'", "a < c"):
        with pytest.raises(TypeError):
            qry.compile_query(q, arr.dtype)


def test_field_kinds_outside_the_predicate():
    dt = np.dtype([("h", "<f2"), ("u", "U3"), ("b", "?"), ("z", "<c8"), ("arr", "<i4", (2,)),
                   ("nest", [("x", "<i4")]), ("big", "S65"), ("be", ">i4"), ("ok", "<i4"), ("s", "S64")])
    for f in ("h", "u", "b", "z", "arr", "nest", "big", "be"):
        with pytest.raises(NotImplementedError, match=f"field {f} "):
            qry.compile_query(f"{f} == 1", dt)
        with pytest.raises(NotImplementedError, match=f"field {f} "):
            qry.compile_query(f"where {f} in (1)", dt)
        with pytest.raises(NotImplementedError, match=f"field {f} "):
            qry.compile_query(f"ok < {f}", dt)
    # copied to the response, they may be any fixed-size type
    assert qry.compile_query("(ok > 1) & (s == b'x')", dt).prog.nops == 3
    segs, rsp = qry.query_segments(dt)
    assert rsp.itemsize == 8 + dt.itemsize and segs == [(0, 8, dt.itemsize)]


def test_program_limits():
    dt = np.dtype([("a", "<i4"), ("s", "S64")])
    ok = " & ".join(["(a > 1)"] * 16)                          # 16 compares + 15 ANDs
    assert qry.compile_query(ok, dt).prog.nops == 31
    with pytest.raises(ValueError, match="more than 32 operations"):
        qry.compile_query(ok + " & (a > 1)", dt)
    with pytest.raises(ValueError, match="more than 32 operations"):
        qry.compile_query(ok + " where a in (1, 2)", dt)
    lit = "x" * 64
    assert qry.compile_query(" | ".join([f"(s == b'{lit}')"] * 4), dt).prog.nops == 7
    with pytest.raises(ValueError, match="pool"):
        qry.compile_query(" | ".join([f"(s == b'{lit}')"] * 5), dt)
    assert qry.compile_query("where a in (" + ",".join(str(i) for i in range(1024)) + ")", dt).prog.ops[0].imm == 1024
    with pytest.raises(ValueError, match="more than 1024 elements"):
        qry.compile_query("where a in (" + ",".join(str(i) for i in range(1025)) + ")", dt)
    with pytest.raises(ValueError):
        qry.compile_query("a >", dt)
    with pytest.raises(ValueError):
        qry.compile_query("a > 1 a", dt)
    with pytest.raises(ValueError):
        qry.compile_query("a 1", dt)
    with pytest.raises(ValueError, match="compound"):
        qry.compile_query("a > 1", np.dtype("<i4"))
