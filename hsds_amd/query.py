"""Host compiler of where-clause queries: query text -> the postfix predicate program of the
query kernels (include/hsds_amd.h hsds_query_prog, csrc/query.h).

The grammar is the reference's (hsds/util/boolparser.py):
    Expression := AndTerm { (OR | '|') AndTerm }
    AndTerm    := Condition { (AND | '&') Condition }
    Condition  := Terminal (== != < <= > >=) Terminal | '(' Expression ')'
    Terminal   := number | 'str' | "str" | b'bytes' | field name
with the optional tail `where <field> in (<elements>)` scanned as chunkUtil._getWhereFieldName /
_getWhereElements do (hsds/util/chunkUtil.py:1151-1257).  The PARSED TREE is what is
evaluated: it equals numpy evaluating BooleanParser(query).getEvalStr() (the form PUT_Chunk
passes on, chunk_dn.py:192-228); the reference's GET path evals the raw text instead, where an
unparenthesised `a > 5 & b < 12` or the AND / OR spellings fail (DESIGN.md "Query
selections").  Constants are converted as numpy (NEP 50) converts them for the field's dtype.
"""
import ast
import re

import numpy as np

from . import _native as nat

_SPLIT = re.compile(r"(\bAND\b|\bOR\b|!=|==|<=|>=|<|>|\(|\)|\&|\|)")
_CMP = {"==": nat.Q_EQ, "!=": nat.Q_NE, "<": nat.Q_LT, "<=": nat.Q_LE, ">": nat.Q_GT, ">=": nat.Q_GE}
_MIRROR = {nat.Q_EQ: nat.Q_EQ, nat.Q_NE: nat.Q_NE, nat.Q_LT: nat.Q_GT, nat.Q_LE: nat.Q_GE, nat.Q_GT: nat.Q_LT,
           nat.Q_GE: nat.Q_LE}
_SYM = {v: k for k, v in _CMP.items()}
_KINDS = {"i1": 0, "i2": 1, "i4": 2, "i8": 3, "u1": 4, "u2": 5, "u4": 6, "u8": 7, "f4": 8, "f8": 9}
MAX_S = 64


class Node:
    """NUM (value: int or float, by the literal's own text), STR, BYTES, VAR, a comparison
    (kind = the HSDS_Q_* code), AND, OR"""

    def __init__(self, kind, value=None, left=None, right=None):
        self.kind, self.value, self.left, self.right = kind, value, left, right


def _tokens(expr):
    out = []
    for t in (x.strip() for x in _SPLIT.split(expr)):
        if t == "":
            continue
        if t in ("AND", "&"):
            out.append(("AND", t))
        elif t in ("OR", "|"):
            out.append(("OR", t))
        elif t in ("(", ")"):
            out.append((t, t))
        elif t in _CMP:
            out.append(("CMP", t))
        elif len(t) >= 2 and t[0] == t[-1] and t[0] in "'\"":
            out.append(("STR", t[1:-1]))
        elif len(t) > 3 and t[0] == "b" and t[1] == "'" and t[-1] == "'":
            try:
                out.append(("BYTES", ast.literal_eval(t)))
            except (SyntaxError, ValueError):
                raise ValueError(f"bad bytes literal: {t}")
        else:
            try:
                out.append(("NUM", int(t)))            # `5` is an int, `5.0` a float
            except ValueError:
                try:
                    out.append(("NUM", float(t)))
                except ValueError:
                    out.append(("VAR", t))
    return out


class _Parser:
    def __init__(self, toks):
        self.t, self.i = toks, 0

    def peek(self):
        return self.t[self.i][0] if self.i < len(self.t) else None

    def take(self, what):
        if self.i >= len(self.t):
            raise ValueError(f"{what} expected, but the query ends")
        self.i += 1
        return self.t[self.i - 1]

    def expression(self):
        n = self.and_term()
        while self.peek() == "OR":
            self.take("OR")
            n = Node("OR", left=n, right=self.and_term())
        return n

    def and_term(self):
        n = self.condition()
        while self.peek() == "AND":
            self.take("AND")
            n = Node("AND", left=n, right=self.condition())
        return n

    def condition(self):
        if self.peek() == "(":
            self.take("(")
            n = self.expression()
            if self.peek() != ")":
                raise ValueError("Closing ) expected, but got " + str(self.take(")")[1]))
            self.take(")")
            return n
        a = self.terminal()
        if self.peek() != "CMP":
            raise ValueError("Operator expected, but got " + str(self.take("Operator")[1]))
        op = _CMP[self.take("Operator")[1]]
        return Node(op, left=a, right=self.terminal())

    def terminal(self):
        kind, v = self.take("NUM, STR, or VAR")
        if kind not in ("NUM", "STR", "BYTES", "VAR"):
            raise ValueError("NUM, STR, or VAR expected, but got " + str(v))
        return Node(kind, v)


def _scan(expr, names):
    """the request errors of chunkUtil._getEvalStr (chunkUtil.py:1260-1353), in its order:
    an unknown field or a `)` too many where it stands, then an open quote, no field at all,
    an open paren"""
    if "import" in names:
        raise ValueError("invalid field name")
    quote, depth, nvar = None, 0, 0
    i, n = 0, len(expr)
    while i < n:
        ch = expr[i]
        if quote:
            quote = None if ch == quote else quote
        elif ch in "'\"":
            quote = ch
        elif ch == "b" and i + 1 < n and expr[i + 1] in "'\"" and (i == 0 or not (expr[i - 1].isalnum() or
                                                                                  expr[i - 1] == "_")):
            pass
        elif ch.isalpha() and (i == 0 or not (expr[i - 1].isalnum() or expr[i - 1] == "_")):
            j = i
            while j < n and (expr[j].isalnum() or expr[j] == "_"):
                j += 1
            word = expr[i:j]
            if word in names:
                nvar += 1
            elif word not in ("AND", "OR") and not _is_number(word):      # (nan, inf)
                raise ValueError(f"query variable: {word}")
            i = j
            continue
        elif ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
            if depth < 0:
                raise ValueError("Mismatched paren")
        i += 1
    if quote:
        raise ValueError("no matching quote character")
    if nvar == 0:
        raise ValueError("No field value")
    if depth != 0:
        raise ValueError("Mismatched paren")


def _is_number(word):
    try:
        float(word)
        return True
    except ValueError:
        return False


def where_field_name(query):
    """chunkUtil._getWhereFieldName: the field of a `where <field> in (...)` tail, or None"""
    if query.startswith("where "):
        i = len("where ")
    else:
        i = query.find(" where ")
        if i <= 0:
            return None
        i += len(" where ")
    name, quote = "", None
    while i < len(query):
        ch = query[i]
        i += 1
        if quote and ch == quote:
            quote = None
            break
        if ch in "'\"":
            quote = ch
            continue
        ident = ch.isalnum() or ch == "_"
        if name and not ident and not quote:
            break
        if quote or ident:
            name += ch
    if not name:
        raise ValueError("query where with no fieldname")
    if quote:
        raise ValueError("unclosed quote")
    return name


def where_elements(query):
    """chunkUtil._getWhereElements: the elements of the `in (...)` list -- quoted text (bytes
    after a b prefix) or bare tokens, separated by commas"""
    n = query.find(" in ")
    if n < 0:
        raise ValueError("where query with no 'in' keyword")
    n += 4
    i = query.find("(", n)
    if i < 0:
        raise ValueError("where in query with no '(' character)")
    i += 1
    out, quote, s = [], None, None
    while i < len(query):
        ch = query[i]
        i += 1
        if quote and ch == quote:
            quote = None
            out.append("" if s is None else s)
            s = None
        elif ch in "'\"":
            quote = ch
            s = b"" if s == "b" else ""
        elif ch == ",":
            if s is not None:
                out.append(s)
                s = None
        elif ch == ")":
            if quote:
                raise ValueError("unclosed quote in 'where in' list")
            if s is not None:
                out.append(s)
            break
        elif ch.isspace() and not quote:
            pass
        else:
            c = ch.encode("utf8") if isinstance(s, bytes) else ch
            s = c if s is None else s + c
    if quote:
        raise ValueError("unclosed quote")
    return out


def parse(expr):
    """expression text -> tree"""
    p = _Parser(_tokens(expr))
    root = p.expression()
    if p.i != len(p.t):
        raise ValueError("unexpected " + str(p.t[p.i][1]))
    return root


def eval_str(node, arr_name=None):
    """the tree as BooleanParser.getEvalStr writes it (numbers as floats, & and |, operands
    that contain a space parenthesised); with arr_name, fields as arr_name['field']"""
    if node.kind == "NUM":
        return float(node.value)
    if node.kind == "STR":
        return f"'{node.value}'"
    if node.kind == "BYTES":
        return repr(node.value)
    if node.kind == "VAR":
        return f"{arr_name}['{node.value}']" if arr_name else node.value
    a, b = eval_str(node.left, arr_name), eval_str(node.right, arr_name)
    a = f"({a})" if isinstance(a, str) and " " in a else a
    b = f"({b})" if isinstance(b, str) and " " in b else b
    sym = {"AND": "&", "OR": "|"}.get(node.kind) or _SYM[node.kind]
    return f"{a} {sym} {b}"


# ---- compiler ---------------------------------------------------------------------------
def _field(dt, name):
    """(kind code, byte offset, width) of a field usable in a predicate"""
    if name not in dt.names:
        raise ValueError(f"query variable: {name}")
    fdt, off = dt.fields[name][0], dt.fields[name][1]
    if fdt.shape == () and fdt.names is None and fdt.byteorder in ("=", "<", "|"):
        code = _KINDS.get(fdt.kind + str(fdt.itemsize))
        if code is not None and fdt.kind in "iuf":
            return code, off, fdt.itemsize
        if fdt.kind == "S" and 1 <= fdt.itemsize <= MAX_S:
            return nat.Q_KIND_S, off, fdt.itemsize
    raise NotImplementedError(f"field {name} of type {fdt} in a query predicate")


def _f64_bits(v):
    return int(np.array([v], "<f8").view("<u8")[0])


_ALWAYS_BELOW = {nat.Q_EQ: 0, nat.Q_NE: 1, nat.Q_LT: 0, nat.Q_LE: 0, nat.Q_GT: 1, nat.Q_GE: 1}   # literal < every value


class CompiledQuery:
    """prog: nat.QueryProg; isin: the ISIN elements (uint8 array) or None; where_field: the
    `where in` field or None; has_expr: the query has an expression; eval_str: the
    expression as getEvalStr writes it (None without one)"""

    def __init__(self, dt):
        self.dt = dt
        self.prog = nat.QueryProg()
        self.isin = None
        self.where_field = None
        self.has_expr = False
        self.eval_str = None
        self.tree = None
        self._pool = 0
        self._depth = 0

    def _push(self, **kw):
        n = self.prog.nops
        if n >= nat.QUERY_MAX_OPS:
            raise ValueError(f"query needs more than {nat.QUERY_MAX_OPS} operations")
        o = self.prog.ops[n]
        for k, v in kw.items():
            setattr(o, k, v)
        self.prog.nops = n + 1
        if kw["op"] in (nat.Q_AND, nat.Q_OR):
            self._depth -= 1
        else:
            self._depth += 1
            if self._depth > 32:
                raise ValueError("query nests deeper than 32 pending conditions")

    def _const(self, truth):
        self._push(op=nat.Q_CONST, imm=1 if truth else 0)

    def _mismatch(self, cmp, what):
        # numpy 2 compares values of unrelated types unequal everywhere and has no ordering for them
        if cmp == nat.Q_EQ:
            self._const(False)
        elif cmp == nat.Q_NE:
            self._const(True)
        else:
            raise TypeError(f"'{_SYM[cmp]}' not supported between {what}")

    def _cmp_const(self, cmp, name, lit):
        kind, off, width = _field(self.dt, name)
        v = lit.value
        if kind == nat.Q_KIND_S:
            if lit.kind != "BYTES":
                return self._mismatch(cmp, f"bytes field {name} and {type(v).__name__} literal")
            c = v.rstrip(b"\0")
            if len(c) > width:
                c = c[:width] + b"\x01"        # any longer constant sorts after every value it extends
            if self._pool + len(c) > nat.QUERY_POOL:
                raise ValueError("query holds more bytes constants than the program's pool")
            for k, byte in enumerate(c):
                self.prog.pool[self._pool + k] = byte
            self._push(op=nat.Q_CMP_BYTES, cmp=cmp, kind=kind, off=off, len=width, off_b=self._pool, len_b=len(c))
            self._pool += len(c)
            return
        if lit.kind != "NUM":
            return self._mismatch(cmp, f"field {name} and {type(v).__name__} literal")
        fdt = self.dt.fields[name][0]
        if fdt.kind in "iu" and isinstance(v, int):
            info = np.iinfo(fdt)
            if v < info.min:
                return self._const(_ALWAYS_BELOW[cmp])
            if v > info.max:
                below = _ALWAYS_BELOW[cmp]
                return self._const(below if cmp in (nat.Q_EQ, nat.Q_NE) else 1 - below)
            dom = nat.Q_DOM_I64 if fdt.kind == "i" else nat.Q_DOM_U64
            self._push(op=nat.Q_CMP, cmp=cmp, dom=dom, kind=kind, off=off, imm=v & 0xFFFFFFFFFFFFFFFF)
            return
        if fdt == np.dtype("f4"):
            with np.errstate(over="ignore"):
                c = float(np.float32(v))
        else:
            c = float(v)
        self._push(op=nat.Q_CMP, cmp=cmp, dom=nat.Q_DOM_F64, kind=kind, off=off, imm=_f64_bits(c))

    def _cmp_fields(self, cmp, a, b):
        ka, oa, wa = _field(self.dt, a)
        kb, ob, wb = _field(self.dt, b)
        if ka == nat.Q_KIND_S and kb == nat.Q_KIND_S:
            self._push(op=nat.Q_CMP_BYTES, cmp=cmp, kind=ka, kind_b=1, off=oa, len=wa, off_b=ob, len_b=wb)
            return
        if ka == nat.Q_KIND_S or kb == nat.Q_KIND_S:
            return self._mismatch(cmp, f"fields {a} and {b}")
        da, db = self.dt.fields[a][0], self.dt.fields[b][0]
        rt = np.result_type(da, db)
        if rt.kind == "f" and da.kind in "iu" and db.kind in "iu":
            # int64 against uint64 has no common integer type; numpy compares the two exactly
            # (not as doubles): the signed field goes first
            if da.kind == "u":
                cmp, ka, oa, kb, ob = _MIRROR[cmp], kb, ob, ka, oa
            self._push(op=nat.Q_CMP_FIELD, cmp=cmp, dom=nat.Q_DOM_SU, kind=ka, kind_b=kb, off=oa, off_b=ob)
            return
        dom = {"i": nat.Q_DOM_I64, "u": nat.Q_DOM_U64, "f": nat.Q_DOM_F64}[rt.kind]
        self._push(op=nat.Q_CMP_FIELD, cmp=cmp, dom=dom, kind=ka, kind_b=kb, off=oa, off_b=ob)

    def _emit(self, node):
        if node.kind in ("AND", "OR"):
            self._emit(node.left)
            self._emit(node.right)
            self._push(op=nat.Q_AND if node.kind == "AND" else nat.Q_OR)
            return
        a, b = node.left, node.right
        if a.kind == "VAR" and b.kind == "VAR":
            self._cmp_fields(node.kind, a.value, b.value)
        elif a.kind == "VAR":
            self._cmp_const(node.kind, a.value, b)
        elif b.kind == "VAR":
            self._cmp_const(_MIRROR[node.kind], b.value, a)
        else:
            # constants only: folded on the host (Python's own comparison, as eval gives)
            x, y = a.value, b.value
            self._const({nat.Q_EQ: lambda: x == y, nat.Q_NE: lambda: x != y, nat.Q_LT: lambda: x < y,
                         nat.Q_LE: lambda: x <= y, nat.Q_GT: lambda: x > y, nat.Q_GE: lambda: x >= y}[node.kind]())

    def _isin(self, name, elements):
        kind, off, width = _field(self.dt, name)
        fdt = self.dt.fields[name][0]
        try:
            arr = np.array(elements, dtype=fdt)
        except ValueError:
            raise ValueError("where elements are not compatible with field datatype")
        if fdt.kind == "S":
            vals, dom = np.unique(arr), 0
            raw = vals.tobytes()
        else:
            dom = {"i": nat.Q_DOM_I64, "u": nat.Q_DOM_U64, "f": nat.Q_DOM_F64}[fdt.kind]
            wide = arr.astype({"i": "<i8", "u": "<u8", "f": "<f8"}[fdt.kind])
            if fdt.kind == "f":
                wide = wide[~np.isnan(wide)] + 0.0          # NaN is never a member; -0.0 == 0.0
            vals = np.unique(wide)
            raw = vals.tobytes()
        if len(vals) > nat.QUERY_MAX_ISIN:
            raise ValueError(f"where in list of more than {nat.QUERY_MAX_ISIN} elements")
        if len(vals) == 0:
            return self._const(False)
        self.isin = np.frombuffer(raw, np.uint8).copy()
        self._push(op=nat.Q_ISIN, dom=dom, kind=kind, off=off, len=width, off_b=0, imm=len(vals))


def compile_query(query, dtype):
    """query text over rows of the compound `dtype` -> CompiledQuery.  ValueError with the
    reference's texts for a bad request, NotImplementedError for a field type that the
    kernels do not compare, TypeError for an ordering numpy does not have."""
    dt = np.dtype(dtype)
    if not dt.names:
        raise ValueError("queries need a compound dataset type")
    cq = CompiledQuery(dt)
    if query.startswith("where "):
        expr = None
    else:
        n = query.find(" where ")
        expr = query[:n] if n > 0 else query
        _scan(expr, dt.names)
    field = where_field_name(query)
    elements = None
    if field:
        if field not in dt.names:
            raise ValueError(f"where field {field} is not a member of dataset type")
        elements = where_elements(query)
        if not elements:
            raise ValueError("query: where key word with no elements")
    if expr is not None:
        root = parse(expr)
        cq.has_expr = True
        cq.eval_str = eval_str(root)
        cq.tree = root
        cq._emit(root)
    if field:
        cq.where_field = field
        cq._isin(field, elements)
        if cq.has_expr:
            cq._push(op=nat.Q_AND)
    return cq


def query_dtype(select_dt):
    """chunkUtil.getQueryDtype (chunkUtil.py:1356-1372): the response record -- a uint64
    index (named index, with underscores in front while a field has that name), then the
    fields packed"""
    select_dt = np.dtype(select_dt)
    name = "index"
    for _ in range(len(select_dt.names)):
        if name in select_dt.names:
            name = "_" + name
        else:
            break
    return np.dtype([(name, "uint64")] + [(n, select_dt[n]) for n in select_dt.names])


def query_segments(dset_dt, select_dt=None):
    """(segment table row -> response record, response dtype): one hsds_point_seg per
    selected field, neighbours merged; the record's padding (an aligned compound) is dropped"""
    dset_dt = np.dtype(dset_dt)
    select_dt = dset_dt if select_dt is None else np.dtype(select_dt)
    if not select_dt.names:
        raise ValueError("select_dt names no field")
    rsp = query_dtype(select_dt)
    segs = []
    for f in select_dt.names:
        if f not in dset_dt.names:
            raise ValueError(f"no field of name {f}")
        if select_dt.fields[f][0] != dset_dt.fields[f][0]:
            raise NotImplementedError("field selection with a converted field type")
        c, o, n = dset_dt.fields[f][1], rsp.fields[f][1], dset_dt.fields[f][0].itemsize
        if segs and segs[-1][0] + segs[-1][2] == c and segs[-1][1] + segs[-1][2] == o:
            segs[-1] = (segs[-1][0], segs[-1][1], segs[-1][2] + n)
        else:
            segs.append((c, o, n))
    if len(segs) > nat.POINT_MAX_SEGS:
        raise NotImplementedError(f"a query response of more than {nat.POINT_MAX_SEGS} separate byte runs")
    return segs, rsp


def update_record(dset_dt, query_update):
    """PUT_Chunk's query_update {field: value} -> (segment table update record -> row, the
    packed record's bytes): the values converted by numpy to their fields' types
    (chunkUtil.py:1473-1486, 1535-1540)"""
    dset_dt = np.dtype(dset_dt)
    names = [n for n in dset_dt.names if n in query_update]
    if not names:
        raise ValueError("chunkQuery - no fields found in query_update")
    rec_dt = np.dtype([(n, dset_dt[n]) for n in names])
    rec = np.zeros(1, rec_dt)
    for n in names:
        rec[n] = query_update[n]
    segs = []
    for n in names:
        c, o, nb = dset_dt.fields[n][1], rec_dt.fields[n][1], dset_dt[n].itemsize
        if segs and segs[-1][0] + segs[-1][2] == c and segs[-1][1] + segs[-1][2] == o:
            segs[-1] = (segs[-1][0], segs[-1][1], segs[-1][2] + nb)
        else:
            segs.append((c, o, nb))
    if len(segs) > nat.POINT_MAX_SEGS:
        raise NotImplementedError(f"an update of more than {nat.POINT_MAX_SEGS} separate byte runs")
    return segs, rec.view(np.uint8).reshape(-1).copy()


QUERY_CHUNK_DTYPE = np.dtype(nat.QUERY_CHUNK_FIELDS)


def query_chunk_table(chunks):
    """(slot, first, count, step, index0) per chunk -> (hsds_query_chunk records with their
    word0, total mask words): each chunk's rows are padded to whole 64-row words"""
    table = np.zeros(len(chunks), QUERY_CHUNK_DTYPE)
    for k, (slot, first, count, step, index0) in enumerate(chunks):
        if first < 0 or count < 0 or step < 1:
            raise ValueError("query selections have first >= 0, count >= 0 and step >= 1")
        table[k] = (slot, first, count, step, index0, 0)
    words = (table["count"] + 63) // 64
    table["word0"] = np.cumsum(words) - words
    return table, int(words.sum())
