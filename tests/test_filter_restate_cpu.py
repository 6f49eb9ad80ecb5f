"""The WHERE compiler and the numpy restatement of the filter programs against SQLite itself (stdlib sqlite3:
SELECT id FROM t WHERE <cond> ORDER BY id over an in-memory table with INTEGER / REAL / TEXT columns holding the same
rows), the compiler's rejections, and the stand-alone check of the host-side program checks (np_filter_plan.h).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import next_plaid_amd as npa
from next_plaid_amd import filters as F
import filter_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS = 700


@pytest.fixture(scope="module")
def table():
    rows = R.make_rows(N_ROWS)
    return rows, npa.make_schema(rows, N_ROWS), R.sqlite_table(rows)


def test_rows_hold_what_the_conditions_need(table):
    rows, sch, con = table
    assert [c.type for c in sch.columns.values()] == [F.NP_COL_I64, F.NP_COL_I64, F.NP_COL_F64, F.NP_COL_F64, F.NP_COL_CODE,
                                                      F.NP_COL_CODE]
    assert len(sch["t"].dictionary) == 70 and len(sch["s"].dictionary) == len(R.SPECIAL_S)
    assert sch["s"].dictionary == sorted(s.encode() for s in R.SPECIAL_S)          # UTF-8 byte order = BINARY collation
    assert sch["z"].valid is None and sch["x"].valid is not None                    # x: NULLs from NaN alone
    for c in "ywst":
        share = 1.0 - sch[c].valid.mean()
        assert 0.12 < share < 0.28, (c, share)
    assert con.execute("SELECT count(*) FROM t WHERE x IS NULL").fetchone()[0] == int((sch["x"].valid == 0).sum())


@pytest.mark.parametrize("cond,params", R.fixed_conditions(), ids=lambda v: str(v)[:40])
def test_fixed_conditions_equal_sqlite(table, cond, params):
    rows, sch, con = table
    want = R.sqlite_ids(con, cond, params)
    got = R.ids_of(cond, params, sch)
    assert np.array_equal(got, want), f"{cond} {params}: {got[:10]} vs sqlite {want[:10]} ({got.size} vs {want.size})"


def test_the_fixed_list_says_what_the_issue_says(table):
    rows, sch, con = table
    ids = lambda c, p: R.ids_of(c, p, sch)
    x, y, s = rows["x"], rows["y"], rows["s"]
    assert ids("x = ?", [float("nan")]).size == 0
    null_x = np.isnan(x)
    assert not np.isin(np.nonzero(null_x)[0], ids("NOT (x > ?)", [0.0])).any() and ids("NOT (x > ?)", [0.0]).size > 0
    assert ids("y NOT IN (?, ?)", [7, None]).size == 0
    sevens = np.nonzero((y.filled(0) == 7) & ~np.ma.getmaskarray(y))[0]
    assert np.array_equal(ids("y IN (?, ?)", [7, None]), sevens) and sevens.size > 0
    # the cell 9007199254740992.0 against the integer ...993: SQLite compares exactly and selects nothing, a conversion to
    # double would select the cell -- so the compiler refuses the parameter
    assert R.sqlite_ids(con, "x = ?", [9007199254740993]).size == 0 and ids("x = ?", [9007199254740992]).size > 0
    with pytest.raises(npa.NextPlaidError, match="not exactly a double"):
        ids("x = ?", [9007199254740993])
    below = ids("s < ?", ["abd"])
    word = lambda i: None if s[i] is np.ma.masked else s[i]
    assert {"Abc", "a_c"} <= {word(i) for i in below} and "Émile" not in {word(i) for i in below}
    assert "Émile" in {word(i) for i in ids("s > ?", ["abd"])}
    assert "Abc" in {word(i) for i in ids("s LIKE ?", ["a%"])}
    assert "Émile" not in {word(i) for i in ids("s LIKE ?", ["é%"])} and "émile" in {word(i) for i in ids("s LIKE ?", ["é%"])}
    assert ids("1=1", []).size == N_ROWS and ids("0=1", []).size == 0
    zeros = ids("x = ?", [0])
    assert {np.signbit(x[i]) for i in zeros} == {True, False}                     # -0.0 = 0
    pos = x[ids("x > ?", [0])]
    assert (pos == 5e-324).any() and (pos > 0).all() and pos.size == int((x > 0).sum())           # 5e-324 > 0


def test_random_expressions_equal_sqlite(table):
    rows, sch, con = table
    conds = R.random_conditions(300)
    assert len(conds) == 300
    depth_seen, nonempty = 0, 0
    for cond, params in conds:
        prog = npa.compile_filter(cond, params, sch)
        want = R.sqlite_ids(con, cond, params)
        got = R.select(prog, sch)
        assert np.array_equal(got, want), f"{cond} {params}: {got.size} ids vs sqlite {want.size}"
        depth_seen = max(depth_seen, cond.count("("))
        nonempty += 0 < want.size < N_ROWS
    assert depth_seen >= 6 and nonempty > 100     # the generator nests, and most expressions select a proper part


def test_slices_restate_a_shard(table):
    rows, sch, con = table
    for cond, params in R.random_conditions(20, seed=9):
        prog = npa.compile_filter(cond, params, sch)
        whole = R.select(prog, sch)
        parts = [R.select(prog, sch, lo, hi) for lo, hi in ((0, 233), (233, 466), (466, N_ROWS))]
        assert np.array_equal(np.concatenate(parts), whole)


REJECTED = [
    ("s REGEXP ?", ["a.*"], "REGEXP"),
    ("nope = ?", [1], "unknown column 'nope'"),
    ("y = ? AND z = ?", [1], "placeholders"),
    ("y = ?", [1, 2], "parameters"),
    ("y = ?", ["seven"], "numeric, the parameter is a string"),
    ("s = ?", [7], "is text"),
    ("s LIKE ?", [7], "is text"),
    ("y LIKE ?", ["7%"], "needs a text column"),
    ("y = ?", [7.0], "holds integers, the parameter is a float"),
    ("y IN (?, ?)", [1, 2.5], "holds integers"),
    ("x = ?", [9007199254740993], "not exactly a double"),
    ("x BETWEEN ? AND ?", [0, (1 << 60) + 1], "not exactly a double"),
    ("y = ?", [1 << 63], "64-bit"),
    ("y = ?; DROP TABLE t", [1], "Semicolons"),                 # quick_safety_check: statement terminators
    ("y = ? -- tail", [1], "comments"),                         # ... comment syntax
    ("y = ? /* x */", [1], "comments"),
    ("y IN (SELECT ?)", [1], "SELECT"),                         # ... dangerous keywords
    ("y = ? UNION z = ?", [1, 2], "UNION"),
    ("abs(y) = ?", [1], "function calls"),
    ("y = 7", [], "literals"),
    ("s = 'abc'", [], "literals"),
    ("y = ? AND", [1], "expected a column name"),
    ("(y = ?", [1], r"expected '\)'"),
    ("y = ? z = ?", [1, 2], "unexpected 'z'"),
    ("y IN ()", [], "placeholder"),
    ("y NOT = ?", [1], "expected a comparison"),
    ("1=1 AND y = ?", [1], "literals"),
    ("", [], "empty"),
]


@pytest.mark.parametrize("cond,params,what", REJECTED, ids=lambda v: str(v)[:30])
def test_compiler_rejects(table, cond, params, what):
    rows, sch, con = table
    with pytest.raises(npa.NextPlaidError, match=what):
        npa.compile_filter(cond, params, sch)


def test_equal_filters_share_one_program(table):
    rows, sch, con = table
    progs, qf = npa.pack_filters([("y = ?", [7]), None, ("y  =  ?", (7,)), "1=1", ("y = ?", [8])], 5, sch)
    assert qf.tolist() == [0, -1, 0, 1, 2] and len(progs) == 3
    with pytest.raises(ValueError):
        npa.pack_filters([None], 2, sch)


def test_set_columns_checks_lengths_before_the_library():
    with pytest.raises(npa.ShapeError):
        npa.make_schema({"y": [1, 2, 3]}, 4)
    sch = npa.make_schema({"b": np.array([True, False]), "m": np.ma.MaskedArray([1.5, 2.5], [False, True]), "o": ["a", None]}, 2)
    assert [c.type for c in sch.columns.values()] == [F.NP_COL_I64, F.NP_COL_F64, F.NP_COL_CODE]
    assert sch["m"].valid.tolist() == [1, 0] and sch["o"].valid.tolist() == [1, 0] and sch["b"].valid is None


def test_program_checks_stand_alone(tmp_path):
    """tests/cpp/filter_plan_check.cpp: np_filter_plan.h with the host compiler alone, under AddressSanitizer and UBSan: malformed
    programs get their error code, well-formed ones pass, and the chunk plan keeps its budget."""
    exe = tmp_path / "filter_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "next-plaid_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "filter_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
