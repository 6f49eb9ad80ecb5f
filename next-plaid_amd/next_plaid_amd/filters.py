"""Metadata filters, host side: columns -> typed arrays + dictionaries, and the WHERE compiler.

The reference validates a condition against an allowlist grammar (filtering.rs:571-583) and lets SQLite evaluate it over
metadata.db.  Here the same grammar is compiled to the postfix program of include/nextplaid_hip.h (np_filter): strings never
cross the ABI, text columns are dictionary-coded with the dictionary sorted by UTF-8 bytes (= SQLite's BINARY collation), and
every text leaf is resolved against the dictionary here -- except over a column whose dictionary text is kept on the device
(text_on_device): there REGEXP and LIKE compile to a byte DFA (regexes.py) that the NP_F_MATCH leaf runs over the dictionary
in HBM.  Pure host code: no device, no library."""
from __future__ import annotations

import bisect
import math
import re
import struct
from dataclasses import dataclass, field

import numpy as np

from .api import NextPlaidError, ShapeError
from . import regexes
from .regexes import FilterError   # one class for the WHERE compiler and the pattern compiler

NP_COL_I64, NP_COL_F64, NP_COL_CODE = 0, 1, 2
NP_F_CMP, NP_F_BETWEEN, NP_F_IN, NP_F_IS_NULL, NP_F_CONST, NP_F_AND, NP_F_OR, NP_F_NOT = range(8)
NP_F_MATCH = 16
CMP_ARG = {"=": 0, "!=": 1, "<>": 1, "<": 2, "<=": 3, ">": 4, ">=": 5}
CONST_FALSE, CONST_TRUE, CONST_UNKNOWN = 0, 1, 2
MAX_COLUMNS, MAX_OPS, MAX_DEPTH, MAX_VALUES = 64, 256, 32, 1 << 20
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


@dataclass
class Column:
    name: str
    index: int
    type: int                       # NP_COL_*
    data: np.ndarray                # i64 / f64 / i32 [num_documents]
    valid: np.ndarray | None        # u8 [num_documents], 0 = NULL; None = no NULLs
    dictionary: list | None = None  # CODE columns: the distinct strings as UTF-8 bytes, ascending
    text_on_device: bool = False    # the dictionary's text is kept in HBM: REGEXP and LIKE compile to NP_F_MATCH
    first_non_ascii: int | None = None   # ... and the code of its first string that is not ASCII (None: all are)

    def text_arrays(self):
        """(bytes u8, offsets i64 [n + 1]) of the dictionary, as np_hip_index_set_column_text takes them"""
        off = np.zeros(len(self.dictionary) + 1, np.int64)
        np.cumsum([len(s) for s in self.dictionary], out=off[1:])
        return np.frombuffer(b"".join(self.dictionary), np.uint8), off


@dataclass
class Schema:
    """The columns of a handle by name, in the order they were given (= their index in the library)."""
    columns: dict = field(default_factory=dict)

    def __len__(self):
        return len(self.columns)

    def __getitem__(self, name) -> Column:
        return self.columns[name]

    def __contains__(self, name):
        return name in self.columns

    def shrunk(self, keep) -> "Schema":
        """The schema of the rows `keep` (a boolean array over the documents) selects, in their order: what a handle holds
        after MmapIndex.remove(..., keep_attachments=True).  Names, types, dictionaries (a code keeps its string, also one no
        surviving row uses) and text_on_device stay; a column whose surviving rows hold no NULL has no validity array."""
        keep = np.asarray(keep, bool)
        out = Schema()
        for name, c in self.columns.items():
            valid = None if c.valid is None else np.ascontiguousarray(c.valid[keep])
            out.columns[name] = Column(name, c.index, c.type, np.ascontiguousarray(c.data[keep]),
                                       None if valid is None or valid.all() else valid, c.dictionary, c.text_on_device,
                                       c.first_non_ascii)
        return out

    def extended(self, new_columns: dict):
        """The schema after MmapIndex.append(..., rows=): `new_columns` holds, under exactly this schema's names, the new
        documents' entries (as set_columns takes them).  Returns (schema, rows, remaps):
          schema  all rows -- each text column's new strings merged into its sorted dictionary, the old rows' codes moved
                  with it; it equals make_schema of the concatenated columns when every old string is still in use;
          rows    name -> Column of the NEW rows alone, text coded against the merged dictionary;
          remaps  name -> int32 table old code -> new code (strictly increasing), or None when no string is new."""
        if set(new_columns) != set(self.columns) or len(new_columns) != len(self.columns):
            raise FilterError(f"the rows' columns {sorted(map(str, new_columns))} are not exactly the schema's {sorted(self.columns)}")
        n_new = None
        out, rows, remaps = Schema(), {}, {}
        for name, c in self.columns.items():
            new = _column(name, c.index, new_columns[name], n_new)
            n_new = new.data.shape[0]
            if n_new == 0 or (new.valid is not None and not new.valid.any()):   # no row, or all NULL: the column's own type
                new = Column(name, c.index, c.type, np.zeros(n_new, c.data.dtype), new.valid, [] if c.type == NP_COL_CODE else None)
            if c.type == NP_COL_F64 and new.type == NP_COL_I64:
                new = Column(name, c.index, NP_COL_F64, new.data.astype(np.float64), new.valid)
            if new.type != c.type:
                raise FilterError(f"column '{name}' has type {c.type}, its new rows type {new.type}")
            data, remap, dic, first = c.data, None, c.dictionary, c.first_non_ascii
            if c.type == NP_COL_CODE:
                have = set(c.dictionary)
                if any(s not in have for s in new.dictionary):
                    dic = sorted(have | set(new.dictionary))
                    remap = np.array([bisect.bisect_left(dic, s) for s in c.dictionary], np.int32)
                    live = np.ones(data.shape[0], bool) if c.valid is None else c.valid.astype(bool)
                    data = np.where(live, remap[np.where(live, data, 0)] if len(remap) else 0, data).astype(np.int32)
                code = np.array([bisect.bisect_left(dic, s) for s in new.dictionary], np.int32)
                live = np.ones(n_new, bool) if new.valid is None else new.valid.astype(bool)
                new.data = np.ascontiguousarray(np.where(live, code[np.where(live, new.data, 0)] if len(code) else 0, 0).astype(np.int32))
                new.dictionary = dic
                if c.text_on_device:
                    for s in dic:
                        try:
                            s.decode("utf-8")
                        except UnicodeDecodeError:
                            raise FilterError(f"text_on_device: column '{name}': a new string is not UTF-8") from None
                    first = next((i for i, s in enumerate(dic) if not s.isascii()), None)
                    new.text_on_device, new.first_non_ascii = True, first
            valid = None
            if c.valid is not None or new.valid is not None:
                valid = np.concatenate([np.ones(c.data.shape[0], np.uint8) if c.valid is None else c.valid,
                                        np.ones(n_new, np.uint8) if new.valid is None else new.valid])
            out.columns[name] = Column(name, c.index, c.type, np.ascontiguousarray(np.concatenate([data, new.data])), valid, dic,
                                       c.text_on_device, first)
            rows[name], remaps[name] = new, remap
        return out, rows, remaps


@dataclass
class CompiledFilter:
    """A postfix program: ops = (op, column, arg, n_values, first_value) tuples, values = i64 (f64 as bit patterns)."""
    ops: list
    values: np.ndarray

    def key(self):
        return (tuple(self.ops), self.values.tobytes())


def _f64_bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def _column(name: str, index: int, values, n_docs: int | None) -> Column:
    """One caller-given column as a typed array: ints and bools I64, floats F64 (NaN = NULL), strings dictionary codes;
    None entries and numpy masked entries are NULL."""
    mask = None
    if isinstance(values, np.ma.MaskedArray):
        mask = np.ma.getmaskarray(values).copy()
        values = values.filled(values.dtype.type() if values.dtype.kind != "O" else None)
    arr = values if isinstance(values, np.ndarray) else np.asarray(list(values), dtype=object)
    if arr.ndim != 1:
        raise ShapeError(f"Shape error: column '{name}' must be one-dimensional, got shape {arr.shape}")
    if n_docs is not None and arr.shape[0] != n_docs:
        raise ShapeError(f"Shape error: column '{name}' has {arr.shape[0]} entries, the index has {n_docs} documents")
    n = arr.shape[0]
    valid = np.ones(n, np.uint8) if mask is None else (~mask).astype(np.uint8)
    if arr.dtype.kind in "biu":
        if arr.dtype.kind == "u" and arr.size and int(arr.max()) > _I64_MAX:
            raise FilterError(f"column '{name}': value {int(arr.max())} does not fit a 64-bit integer")
        data, typ, dic = arr.astype(np.int64), NP_COL_I64, None
    elif arr.dtype.kind == "f":
        data, typ, dic = arr.astype(np.float64), NP_COL_F64, None
        valid &= ~np.isnan(data)
    elif arr.dtype.kind in "US":
        strs = [s if isinstance(s, bytes) else str(s).encode("utf-8") for s in arr.tolist()]
        dic = sorted(set(s for s, v in zip(strs, valid) if v))
        code = {s: i for i, s in enumerate(dic)}
        data, typ = np.array([code.get(s, 0) if v else 0 for s, v in zip(strs, valid)], np.int32).reshape(n), NP_COL_CODE
    elif arr.dtype.kind == "O":
        items = arr.tolist()
        for i, v in enumerate(items):
            if v is None or v is np.ma.masked:
                valid[i] = 0
        live = [v for v, ok in zip(items, valid) if ok]
        if live and all(isinstance(v, (str, bytes)) for v in live):
            strs = [None if not ok else (v if isinstance(v, bytes) else v.encode("utf-8")) for v, ok in zip(items, valid)]
            dic = sorted(set(s for s in strs if s is not None))
            code = {s: i for i, s in enumerate(dic)}
            data, typ = np.array([0 if s is None else code[s] for s in strs], np.int32).reshape(n), NP_COL_CODE
        elif all(isinstance(v, (bool, int, np.integer, np.bool_)) for v in live):
            for v in live:
                if not _I64_MIN <= int(v) <= _I64_MAX:
                    raise FilterError(f"column '{name}': value {v} does not fit a 64-bit integer")
            data, typ, dic = np.array([int(v) if ok else 0 for v, ok in zip(items, valid)], np.int64).reshape(n), NP_COL_I64, None
        elif all(isinstance(v, (bool, int, float, np.integer, np.floating, np.bool_)) for v in live):
            data, typ, dic = np.array([float(v) if ok else 0.0 for v, ok in zip(items, valid)], np.float64).reshape(n), NP_COL_F64, None
            valid &= ~np.isnan(data)
        else:
            raise FilterError(f"column '{name}': entries must be all integers, all numbers or all strings (None = NULL)")
    else:
        raise FilterError(f"column '{name}': unsupported dtype {arr.dtype}")
    return Column(name, index, typ, np.ascontiguousarray(data), None if valid.all() else np.ascontiguousarray(valid), dic)


def make_schema(columns: dict, n_docs: int | None = None, text_on_device=()) -> Schema:
    """dict name -> array  =>  Schema (typed arrays, validity, dictionaries).  Lengths are checked against n_docs.  The
    columns named in text_on_device must be text; their strings must be UTF-8 (FilterError naming the row otherwise), and
    REGEXP and LIKE over them compile to NP_F_MATCH."""
    if len(columns) > MAX_COLUMNS:
        raise FilterError(f"{len(columns)} columns, at most {MAX_COLUMNS}")
    sch = Schema()
    for i, (name, values) in enumerate(columns.items()):
        if not isinstance(name, str) or not re.fullmatch(r"[A-Za-z_][A-Za-z0-9_]*", name):
            raise FilterError(f"column name {name!r} is not an identifier")
        sch.columns[name] = _column(name, i, values, n_docs)
    for name in text_on_device:
        if name not in sch:
            raise FilterError(f"text_on_device names '{name}', which is not one of the columns")
        col = sch[name]
        if col.type != NP_COL_CODE:
            raise FilterError(f"text_on_device: column '{name}' is not a text column")
        for code, s in enumerate(col.dictionary):
            try:
                s.decode("utf-8")
            except UnicodeDecodeError:
                row = int(np.flatnonzero((col.data == code) & (col.valid if col.valid is not None else 1))[0])
                raise FilterError(f"text_on_device: column '{name}', row {row}: the string is not UTF-8") from None
            if col.first_non_ascii is None and not s.isascii():
                col.first_non_ascii = code
        col.text_on_device = True
    return sch


# ---- the compiler ------------------------------------------------------------------------------------------------------

_KEYWORDS = {"AND", "OR", "NOT", "IS", "NULL", "BETWEEN", "IN", "LIKE", "REGEXP"}
_DANGEROUS = ("SELECT", "UNION", "INSERT", "UPDATE", "DELETE", "DROP", "CREATE", "ALTER", "TRUNCATE", "EXEC", "EXECUTE",
              "GRANT", "REVOKE")   # filtering.rs:164-167
_TOKEN = re.compile(r"\s*(?:(?P<id>[A-Za-z_][A-Za-z0-9_]*)|(?P<op><=|>=|<>|!=|=|<|>)|(?P<p>\?)|(?P<lp>\()|(?P<rp>\))|(?P<c>,))")


def _tokenize(cond: str):
    toks, pos = [], 0
    end = len(cond.rstrip())
    while pos < end:
        m = _TOKEN.match(cond, pos)
        if not m:
            at = pos + (len(cond[pos:]) - len(cond[pos:].lstrip()))
            raise FilterError(f"unexpected character {cond[at]!r} at position {at} of the condition (literals and function "
                              f"calls are not part of the grammar: use ? placeholders)")
        kind = m.lastgroup
        text, start = m.group(kind), m.start(kind)
        if kind == "id" and text.upper() in _KEYWORDS:
            kind, text = "kw", text.upper()
        toks.append((kind, text, start))
        pos = m.end()
    return toks


def like_to_regex(pattern: str):
    """SQLite's LIKE: % any run of characters, _ any one character, ASCII letters fold case, no escape character."""
    out = []
    for ch in pattern:
        out.append(".*" if ch == "%" else "." if ch == "_" else re.escape(ch))
    return re.compile("".join(out), re.DOTALL | re.IGNORECASE | re.ASCII)


class _Compiler:
    def __init__(self, cond, params, schema):
        self.cond, self.params, self.schema = cond, list(params), schema
        self.toks = _tokenize(cond)
        self.i = 0
        self.n_param = 0
        self.ops, self.values = [], []
        self.depth = self.max_depth = 0

    # -- token helpers
    def peek(self):
        return self.toks[self.i] if self.i < len(self.toks) else ("end", "", len(self.cond))

    def peek2(self):
        return self.toks[self.i + 1] if self.i + 1 < len(self.toks) else ("end", "", len(self.cond))

    def take(self, kind=None, text=None):
        t = self.peek()
        if (kind and t[0] != kind) or (text and t[1] != text):
            want = text or {"id": "a column name", "p": "a ? placeholder", "lp": "'('", "rp": "')'"}.get(kind, kind)
            got = "the end of the condition" if t[0] == "end" else repr(t[1])
            raise FilterError(f"expected {want} at position {t[2]}, found {got}")
        self.i += 1
        return t

    def param(self):
        t = self.take("p")
        if self.n_param >= len(self.params):
            raise FilterError(f"the condition has more ? placeholders than the {len(self.params)} parameters given "
                              f"(placeholder at position {t[2]})")
        self.n_param += 1
        return self.params[self.n_param - 1], t[2]

    # -- emit
    def push(self, op, column=-1, arg=0, vals=()):
        first = len(self.values) if vals else 0
        self.values.extend(int(v) for v in vals)
        self.ops.append((op, column, arg, len(vals), first))
        if op in (NP_F_AND, NP_F_OR):
            self.depth -= 1
        elif op != NP_F_NOT:
            self.depth += 1
            self.max_depth = max(self.max_depth, self.depth)

    # -- grammar (filtering.rs:571-583)
    def expr(self):
        self.and_expr()
        while self.peek()[:2] == ("kw", "OR"):
            self.take()
            self.and_expr()
            self.push(NP_F_OR)

    def and_expr(self):
        self.unary()
        while self.peek()[:2] == ("kw", "AND"):
            self.take()
            self.unary()
            self.push(NP_F_AND)

    def unary(self):
        if self.peek()[:2] == ("kw", "NOT"):
            self.take()
            self.primary()
            self.push(NP_F_NOT)
        else:
            self.primary()

    def primary(self):
        t = self.peek()
        if t[0] == "lp":
            self.take()
            self.expr()
            self.take("rp")
            return
        name, pos = self.take("id")[1:]
        if name.upper() in _DANGEROUS:
            raise FilterError(f"SQL keyword '{name.upper()}' is not allowed in conditions (position {pos})")
        if self.peek()[0] == "lp":
            raise FilterError(f"function calls are not part of the grammar ('{name}(' at position {pos})")
        if name not in self.schema:
            raise FilterError(f"unknown column '{name}' at position {pos}")
        col = self.schema[name]
        t = self.peek()
        if t[0] == "op":
            self.take()
            v, ppos = self.param()
            self.comparison(col, t[1], v, ppos)
        elif t[:2] == ("kw", "LIKE"):
            self.take()
            v, ppos = self.param()
            self.like(col, v, ppos)
        elif t[:2] == ("kw", "REGEXP") or (t[:2] == ("kw", "NOT") and self.peek2()[:2] == ("kw", "REGEXP")):
            neg = t[1] == "NOT"
            if neg:
                self.take()
            t = self.take()
            if not col.text_on_device:
                raise FilterError(f"REGEXP at position {t[2]} is not supported over column '{name}': the crate's REGEXP is a "
                                  f"Rust-regex function that runs on the device as a DFA over the column's text; keep that "
                                  f"text on the device with set_columns(..., text_on_device=['{name}'])")
            v, ppos = self.param()
            self.regexp(col, v, ppos)
            if neg:
                self.push(NP_F_NOT)
        elif t[:2] == ("kw", "IS"):
            self.take()
            neg = self.peek()[:2] == ("kw", "NOT")
            if neg:
                self.take()
            self.take("kw", "NULL")
            self.push(NP_F_IS_NULL, col.index)
            if neg:
                self.push(NP_F_NOT)
        else:
            neg = t[:2] == ("kw", "NOT")
            if neg:
                self.take()
                t = self.peek()
            if t[:2] == ("kw", "BETWEEN"):
                self.take()
                lo, lpos = self.param()
                self.take("kw", "AND")
                hi, hpos = self.param()
                self.between(col, lo, lpos, hi, hpos)
            elif t[:2] == ("kw", "IN"):
                self.take()
                self.take("lp")
                items = [self.param()]
                while self.peek()[0] == "c":
                    self.take()
                    items.append(self.param())
                self.take("rp")
                self.in_list(col, items)
            else:
                got = "the end of the condition" if t[0] == "end" else repr(t[1])
                raise FilterError(f"expected a comparison, IS, BETWEEN, IN or LIKE after '{name}' at position {t[2]}, found {got}")
            if neg:
                self.push(NP_F_NOT)

    # -- leaves.  A parameter becomes: None (SQL NULL), or the i64 the device compares
    def constant(self, col: Column, v, pos):
        """-> ('null', None) | ('num', i64 value as the column stores it) | ('text', bytes)"""
        if v is None:
            return "null", None
        if isinstance(v, (np.generic,)):
            v = v.item()
        if col.type == NP_COL_CODE:
            if not isinstance(v, (str, bytes)):
                raise FilterError(f"type mismatch at position {pos}: column '{col.name}' is text, the parameter is {type(v).__name__}")
            return "text", v if isinstance(v, bytes) else v.encode("utf-8")
        if isinstance(v, (str, bytes)):
            raise FilterError(f"type mismatch at position {pos}: column '{col.name}' is numeric, the parameter is a string")
        if isinstance(v, bool):
            v = int(v)
        if col.type == NP_COL_I64:
            if isinstance(v, float):
                raise FilterError(f"type mismatch at position {pos}: column '{col.name}' holds integers, the parameter is a float")
            if not isinstance(v, int) or not _I64_MIN <= v <= _I64_MAX:
                raise FilterError(f"parameter at position {pos} is not a 64-bit integer: {v!r}")
            return "num", v
        if isinstance(v, int):
            # SQLite compares an integer with a REAL exactly; a conversion would not
            if abs(v) > (1 << 1023) or int(float(v)) != v:
                raise FilterError(f"type mismatch at position {pos}: the integer {v} is not exactly a double, and column "
                                  f"'{col.name}' holds doubles (SQLite compares the two exactly)")
            v = float(v)
        if not isinstance(v, float):
            raise FilterError(f"parameter at position {pos} is not a number: {v!r}")
        if math.isnan(v):
            return "null", None   # SQLite binds NaN as NULL
        return "num", _f64_bits(v)

    def comparison(self, col, op, v, pos):
        kind, c = self.constant(col, v, pos)
        if kind == "null":
            return self.push(NP_F_CONST, -1, CONST_UNKNOWN)
        arg = CMP_ARG[op]
        if kind == "text":
            d = col.dictionary
            lo, hi = bisect.bisect_left(d, c), bisect.bisect_right(d, c)
            if arg in (0, 1):
                return self.push(NP_F_CMP, col.index, arg, [lo if hi > lo else -1])
            # ordered: the codes below / from a position of the dictionary
            if arg == 2:
                return self.push(NP_F_CMP, col.index, 2, [lo])     # s <  v : code <  first entry >= v
            if arg == 3:
                return self.push(NP_F_CMP, col.index, 2, [hi])     # s <= v : code <  first entry >  v
            if arg == 4:
                return self.push(NP_F_CMP, col.index, 5, [hi])     # s >  v : code >= first entry >  v
            return self.push(NP_F_CMP, col.index, 5, [lo])         # s >= v : code >= first entry >= v
        self.push(NP_F_CMP, col.index, arg, [c])

    def between(self, col, lo, lpos, hi, hpos):
        kl, cl = self.constant(col, lo, lpos)
        kh, ch = self.constant(col, hi, hpos)
        if kl == "null" or kh == "null":
            # x BETWEEN a AND b is x >= a AND x <= b: a NULL bound leaves the other comparison to decide FALSE
            for kind, c, op, pos in ((kl, lo, ">=", lpos), (kh, hi, "<=", hpos)):
                if kind == "null":
                    self.push(NP_F_CONST, -1, CONST_UNKNOWN)
                else:
                    self.comparison(col, op, c, pos)
            return self.push(NP_F_AND)
        if kl == "text":
            d = col.dictionary
            return self.push(NP_F_BETWEEN, col.index, 0, [bisect.bisect_left(d, cl), bisect.bisect_right(d, ch) - 1])
        self.push(NP_F_BETWEEN, col.index, 0, [cl, ch])

    def in_list(self, col, items):
        has_null, vals = 0, []
        for v, pos in items:
            kind, c = self.constant(col, v, pos)
            if kind == "null":
                has_null = 1
            elif kind == "text":
                i = bisect.bisect_left(col.dictionary, c)
                if i < len(col.dictionary) and col.dictionary[i] == c:
                    vals.append(i)
            else:
                vals.append(c)
        if col.type == NP_COL_F64:   # ascending and distinct as doubles (-0.0 and 0.0 are one value)
            seen = {}
            for b in vals:
                x = struct.unpack("<d", struct.pack("<q", b))[0]
                seen.setdefault(x + 0.0 if x != 0 else 0.0, b)
            vals = [seen[x] for x in sorted(seen)]
        else:
            vals = sorted(set(vals))
        self.push(NP_F_IN, col.index, has_null, vals)

    def like(self, col, v, pos):
        if col.type != NP_COL_CODE:
            raise FilterError(f"LIKE at position {pos} needs a text column, '{col.name}' is numeric")
        kind, c = self.constant(col, v, pos)
        if kind == "null":
            return self.push(NP_F_CONST, -1, CONST_UNKNOWN)
        if col.text_on_device:
            return self.match(col, regexes.compile_like(c))
        rx = like_to_regex(c.decode("utf-8", "surrogateescape"))
        self.push(NP_F_IN, col.index, 0, [i for i, s in enumerate(col.dictionary)
                                           if rx.fullmatch(s.decode("utf-8", "surrogateescape"))])

    def regexp(self, col, v, pos):
        kind, c = self.constant(col, v, pos)
        if kind == "null":
            return self.push(NP_F_CONST, -1, CONST_UNKNOWN)
        try:
            pattern = c.decode("utf-8")
        except UnicodeDecodeError:
            raise FilterError(f"the REGEXP pattern at position {pos} is not UTF-8") from None
        self.match(col, regexes.compile_regex(pattern, col.first_non_ascii is None, first_non_ascii=col.first_non_ascii))

    def match(self, col, dfa):
        if not col.dictionary:   # every cell is NULL (there is no text to set on the device): UNKNOWN everywhere
            return self.push(NP_F_CONST, -1, CONST_UNKNOWN)
        self.push(NP_F_MATCH, col.index, 0, dfa.pack().tolist())   # one packed word per value

    def run(self) -> CompiledFilter:
        self.expr()
        t = self.peek()
        if t[0] != "end":
            raise FilterError(f"unexpected {t[1]!r} at position {t[2]} of the condition")
        if self.n_param != len(self.params):
            raise FilterError(f"the condition has {self.n_param} ? placeholders, {len(self.params)} parameters were given")
        if len(self.ops) > MAX_OPS:
            raise FilterError(f"the condition compiles to {len(self.ops)} ops, at most {MAX_OPS}")
        if self.max_depth > MAX_DEPTH:
            raise FilterError(f"the condition nests {self.max_depth} deep, at most {MAX_DEPTH}")
        if len(self.values) > MAX_VALUES:
            raise FilterError(f"the condition holds {len(self.values)} constants, at most {MAX_VALUES}")
        return CompiledFilter(self.ops, np.array(self.values, np.int64).reshape(-1))


_NUMERIC_EQ = re.compile(r"^(\d+)\s*=\s*(\d+)$")   # filtering.rs:584-594


def compile_filter(condition: str, params=(), schema: Schema | None = None) -> CompiledFilter:
    """A WHERE condition of the crate's grammar (filtering.rs:571-583: OR, AND, NOT, parentheses; ident op ?, IS [NOT] NULL,
    [NOT] BETWEEN ? AND ?, [NOT] IN (?, ...), LIKE ? on text, [NOT] REGEXP ? (filtering.rs:500) over a text column kept on
    the device, and the 1=1 / 0=1 idiom) as a program for np_hip_filter_eval,
    with SQLite's semantics.  ? placeholders are bound in order; None is SQL NULL.  Everything the grammar does not hold is a
    FilterError (a NextPlaidError) that names the spot -- before any library call: REGEXP, unknown columns, a parameter count
    that does not match, type mismatches (a string against a numeric column, a number against text, a float against an I64
    column, an int a double does not hold exactly against an F64 column), ';', comments, function calls, literals."""
    if not isinstance(condition, str):
        raise FilterError("the condition must be a string")
    schema = schema if schema is not None else Schema()
    params = list(params)
    m = _NUMERIC_EQ.match(condition.strip())
    if m:
        if params:
            raise FilterError(f"the condition has 0 ? placeholders, {len(params)} parameters were given")
        return CompiledFilter([(NP_F_CONST, -1, CONST_TRUE if int(m.group(1)) == int(m.group(2)) else CONST_FALSE, 0, 0)],
                              np.zeros(0, np.int64))
    for bad, what in (("--", "SQL comments"), ("/*", "SQL comments"), ("*/", "SQL comments"), (";", "Semicolons")):
        if bad in condition:
            raise FilterError(f"{what} are not allowed in conditions ({bad!r} at position {condition.index(bad)})")
    if not condition.strip():
        raise FilterError("empty condition")
    return _Compiler(condition, params, schema).run()
