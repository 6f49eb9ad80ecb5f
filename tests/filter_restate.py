"""A numpy restatement of the metadata filters: a compiled program (next_plaid_amd.filters.CompiledFilter) evaluated over a
Schema's columns with explicit (true, known) arrays, the fixed list of conditions the issue names, a seeded generator of
random expressions, and the same rows as an in-memory SQLite table.  tests/test_filter_restate_cpu.py pins the restatement
and the compiler to SQLite itself; the GPU tests then use the restatement as their reference (building the SQLite table is
the slow part at 70 001 rows).  Test infrastructure: no device, no library."""
import sqlite3
import struct

import numpy as np

from next_plaid_amd import filters as F

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ---- the evaluator ------------------------------------------------------------------------------------------------------

def _cmp(arg, x, v):
    return [x == v, x != v, x < v, x <= v, x > v, x >= v][arg]


def evaluate(prog: F.CompiledFilter, schema: F.Schema, lo: int = 0, hi: int | None = None):
    """(true, known) bool arrays over documents [lo, hi) for a compiled program: every stack entry is a pair of arrays."""
    cols = sorted(schema.columns.values(), key=lambda c: c.index)
    n = (cols[0].data.shape[0] if cols else 0) if hi is None else hi
    n -= lo
    stack = []
    vals = prog.values
    for op, ci, arg, nv, first in prog.ops:
        if op in (F.NP_F_CMP, F.NP_F_BETWEEN, F.NP_F_IN, F.NP_F_IS_NULL):
            c = cols[ci]
            valid = np.ones(n, bool) if c.valid is None else c.valid[lo:lo + n].astype(bool)
            if op == F.NP_F_IS_NULL:
                stack.append((~valid, np.ones(n, bool)))
                continue
            x = c.data[lo:lo + n]
            v = vals[first:first + nv]
            if c.type == F.NP_COL_F64:
                v = v.view(np.float64)
                x = np.where(valid, x, 0.0)
            else:
                x = x.astype(np.int64)
            if op == F.NP_F_CMP:
                t, k = _cmp(arg, x, v[0]), valid
            elif op == F.NP_F_BETWEEN:
                t, k = (x >= v[0]) & (x <= v[1]), valid
            else:
                t = np.isin(x, v)
                k = valid & (t | ((arg & 1) == 0))
            stack.append((t & k, k.copy()))
        elif op == F.NP_F_CONST:
            stack.append((np.full(n, arg == 1), np.full(n, arg != 2)))
        elif op == F.NP_F_NOT:
            t, k = stack.pop()
            stack.append((k & ~t, k))
        else:
            tb, kb = stack.pop()
            ta, ka = stack.pop()
            fa, fb = ka & ~ta, kb & ~tb
            if op == F.NP_F_AND:
                t = ta & tb
                stack.append((t, t | fa | fb))
            else:
                t = ta | tb
                stack.append((t, t | (fa & fb)))
    assert len(stack) == 1
    return stack[0]


def select(prog, schema, lo: int = 0, hi: int | None = None) -> np.ndarray:
    """The global ids a program selects among documents [lo, hi): ascending int64."""
    t, k = evaluate(prog, schema, lo, hi)
    return (np.nonzero(t & k)[0] + lo).astype(np.int64)


def ids_of(cond, params, schema, lo=0, hi=None):
    return select(F.compile_filter(cond, params, schema), schema, lo, hi)


# ---- rows ---------------------------------------------------------------------------------------------------------------

WORDS70 = [f"{a}{b}" for a in ("al", "Be", "ca", "Do", "el", "fa", "Émi") for b in ("pha", "_x", "%y", "ta", "TA", "é", "z9", "", "Zz", "mm")]
SPECIAL_S = ["Abc", "a_c", "abd", "abc", "Émile", "émile", "ABD", "a%c", "", "abcd"]
SPECIAL_X = [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 9007199254740992.0, 1.5, -1.5, 7.0, 1e308, np.nan]
SPECIAL_Y = [I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1, 0, -1, 1, 7, 9007199254740993, 9007199254740992]


def make_rows(n: int, seed: int = 11, null_share: float = 0.2) -> dict:
    """n rows over 2 I64 (y, z), 2 F64 (x, w) and 2 text columns (s: a 10-entry dictionary, t: a 70-entry one), about
    null_share NULLs each (x: only through NaN; z has none at all), the special values first and cycled."""
    rng = np.random.default_rng(seed)
    def nulls():
        m = rng.random(n) < null_share
        m[0] = False          # (a column of NULLs alone has no type: the first row always holds a value)
        return m
    y = np.array([SPECIAL_Y[i % len(SPECIAL_Y)] if i < 3 * len(SPECIAL_Y) else int(rng.integers(-20, 20)) for i in range(n)], np.int64)
    z = rng.integers(0, 5, n).astype(np.int64)
    x = np.array([SPECIAL_X[i % len(SPECIAL_X)] if i < 3 * len(SPECIAL_X) else float(rng.integers(-8, 8)) / 2 for i in range(n)], np.float64)
    x[3 * len(SPECIAL_X):][nulls()[3 * len(SPECIAL_X):]] = np.nan        # NULLs only from NaN, no validity array
    w = rng.standard_normal(n)
    s = np.array([SPECIAL_S[int(i)] for i in rng.integers(0, len(SPECIAL_S), n)], dtype=object)
    if n >= len(SPECIAL_S):
        s[:len(SPECIAL_S)] = SPECIAL_S
    t = np.array([WORDS70[int(i)] for i in rng.integers(0, len(WORDS70), n)], dtype=object)
    if n >= 70:
        t[:70] = WORDS70   # the 70-entry dictionary is complete
    return {"y": np.ma.MaskedArray(y, nulls()), "z": z, "x": x, "w": np.ma.MaskedArray(w, nulls()),
            "s": np.ma.MaskedArray(s, nulls()), "t": np.ma.MaskedArray(t, nulls())}


def sqlite_table(rows: dict):
    """The rows as an in-memory table t(id INTEGER PRIMARY KEY, y INTEGER, z INTEGER, x REAL, w REAL, s TEXT, t TEXT)."""
    con = sqlite3.connect(":memory:")
    kinds = {"y": "INTEGER", "z": "INTEGER", "x": "REAL", "w": "REAL", "s": "TEXT", "t": "TEXT"}
    names = list(rows)
    con.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, " + ", ".join(f"{c} {kinds[c]}" for c in names) + ")")
    def cell(col, i):
        v = col[i]
        if v is np.ma.masked or v is None:
            return None
        v = v.item() if isinstance(v, np.generic) else v
        return v          # (a NaN binds as NULL by itself)
    n = len(rows[names[0]])
    con.executemany("INSERT INTO t VALUES (" + ", ".join("?" * (len(names) + 1)) + ")",
                    ([i] + [cell(rows[c], i) for c in names] for i in range(n)))
    return con


def sqlite_ids(con, cond, params) -> np.ndarray:
    return np.array([r[0] for r in con.execute(f"SELECT id FROM t WHERE {cond} ORDER BY id", list(params))], np.int64)


# ---- conditions ---------------------------------------------------------------------------------------------------------

def fixed_conditions():
    """The issue's fixed list, as (condition, params).  Every one is checked against sqlite3 on the CPU."""
    out = [
        ("x = ?", [float("nan")]),                          # NaN binds as NULL
        ("x IN (?, ?)", [float("nan"), 1.5]),
        ("NOT (x > ?)", [0.0]),                             # drops NULL rows
        ("y NOT IN (?, ?)", [7, None]),                     # selects nothing
        ("y IN (?, ?)", [7, None]),                         # the 7s
        ("y NOT BETWEEN ? AND ?", [-3, 7]),
        ("x NOT BETWEEN ? AND ?", [-1.0, 1.5]),
        ("y BETWEEN ? AND ?", [None, 0]),
        ("NOT (y BETWEEN ? AND ?)", [None, 0]),
        ("x = ?", [9007199254740992]),                      # (…993 is refused: a double does not hold it)
        ("y = ?", [9007199254740993]),
        ("s < ?", ["abd"]),                                 # bytes: 'Abc', 'a_c' below, 'Émile' above
        ("s <= ?", ["abd"]), ("s > ?", ["abd"]), ("s >= ?", ["abd"]), ("s >= ?", ["abc\x00"]), ("s < ?", ["zzz"]),
        ("s = ?", ["Émile"]), ("s != ?", ["Émile"]), ("s = ?", ["no such string"]), ("s <> ?", ["no such string"]),
        ("s BETWEEN ? AND ?", ["ABD", "abc"]), ("s NOT BETWEEN ? AND ?", ["abc", "ABD"]), ("s BETWEEN ? AND ?", ["b", "a"]),
        ("s LIKE ?", ["a%"]),                               # matches 'Abc'
        ("s LIKE ?", ["é%"]),                               # does not match 'Émile'
        ("s LIKE ?", ["É%"]), ("s LIKE ?", ["a_c"]), ("s LIKE ?", ["%C%"]), ("s LIKE ?", [""]), ("s LIKE ?", ["%"]),
        ("NOT s LIKE ?", ["a%"]), ("t LIKE ?", ["%\\_x"]), ("t LIKE ?", ["_e%"]), ("s LIKE ?", [None]),
        ("s IN (?, ?, ?)", ["abc", "nope", "Émile"]), ("t NOT IN (?, ?)", ["alpha", None]),
        ("1=1", []), ("0=1", []), ("1 = 1", []), ("2=2", []),
        ("x = ?", [0]), ("x = ?", [-0.0]), ("x IN (?, ?)", [-0.0, 0.0]), ("x < ?", [0.0]),
        ("x = ?", [float("inf")]), ("x < ?", [float("inf")]), ("x > ?", [float("-inf")]), ("x <= ?", [float("-inf")]),
        ("x BETWEEN ? AND ?", [float("-inf"), float("inf")]),
        ("x > ?", [0]), ("x >= ?", [5e-324]), ("x < ?", [5e-324]), ("x > ?", [-5e-324]),
        ("x IS NULL", []), ("x IS NOT NULL", []), ("y IS NULL OR s IS NOT NULL", []), ("z IS NULL", []),
        ("x IS NULL AND y = ?", [7]), ("x > ? OR y IS NULL", [1.0]), ("NOT (x > ? AND y < ?)", [0.0, 0]),
        ("y = ?", [None]), ("NOT y = ?", [None]), ("y = ? OR z = ?", [None, 3]), ("y = ? AND z = ?", [None, 3]),
        ("z = ?", [True]),
    ]
    for v in (I64_MIN, I64_MAX):
        for op in ("=", "!=", "<>", "<", "<=", ">", ">="):
            out.append((f"y {op} ?", [v]))
        out.append(("y BETWEEN ? AND ?", [I64_MIN, v]))
        out.append(("y IN (?, ?)", [v, 0]))
    return out


def random_conditions(count: int = 300, seed: int = 5, max_depth: int = 6):
    """`count` seeded random expressions of depth <= max_depth over the six columns of make_rows."""
    rng = np.random.default_rng(seed)
    num_i = [I64_MIN, I64_MAX, 0, 1, -1, 7, 3, -20, 19, 9007199254740992, None]
    num_f = [0.0, -0.0, 1.5, -1.5, 0.5, 3.5, float("inf"), float("-inf"), 5e-324, float("nan"), 7, 0, None, 9007199254740992.0]
    txt_s = SPECIAL_S + ["b", "A", "zz", None]
    txt_t = WORDS70[::7] + ["m", "Émi", None]
    likes = ["a%", "%c", "_b%", "%", "A_C", "%É%", "é%", "%\\_x", "%a%a%", "", "el_"]
    pools = {"y": num_i, "z": [0, 1, 2, 3, 4, 5, None], "x": num_f, "w": [0.0, -0.5, 0.5, 1.0, None], "s": txt_s, "t": txt_t}

    def pick(col):
        p = pools[col]
        return p[int(rng.integers(0, len(p)))]

    def leaf():
        col = list(pools)[int(rng.integers(0, 6))]
        kind = int(rng.integers(0, 6 if col in "st" else 5))
        neg = "NOT " if rng.random() < 0.4 else ""
        if kind == 0:
            return f"{col} IS {neg}NULL", []
        if kind == 1:
            return f"{col} {neg}BETWEEN ? AND ?", [pick(col), pick(col)]
        if kind == 2:
            k = int(rng.integers(1, 6))
            return f"{col} {neg}IN ({', '.join('?' * k)})", [pick(col) for _ in range(k)]
        if kind == 5:
            return f"{col} LIKE ?", [likes[int(rng.integers(0, len(likes)))]]
        op = ["=", "!=", "<>", "<", "<=", ">", ">="][int(rng.integers(0, 7))]
        return f"{col} {op} ?", [pick(col)]

    def expr(depth):
        if depth <= 1 or rng.random() < 0.25:
            return leaf()
        r = rng.random()
        if r < 0.2:
            c, p = expr(depth - 1)
            return f"NOT ({c})", p
        a, pa = expr(depth - 1)
        b, pb = expr(depth - 1)
        op = "AND" if r < 0.6 else "OR"
        if rng.random() < 0.5:
            return f"({a}) {op} ({b})", pa + pb
        return f"({a} {op} {b})", pa + pb

    return [expr(int(rng.integers(1, max_depth + 1))) for _ in range(count)]
