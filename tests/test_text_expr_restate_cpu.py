"""The compiler of the full FTS5 grammar (text.compile_text_expr) and the rule tests/text_expr_restate.py restates, pinned to
SQLite's own FTS5 in memory.  CPU only.

What is asserted, over fixed seeds of the generator in text_expr_restate (twelve words that share prefixes and an unknown one,
documents of 0..13 tokens, tables of 5..200 rows, random trees up to depth 4):
  * the matching set equals SQLite's on every query, with and without parentheses, and what SQLite rejects as a syntax error
    the compiler rejects;
  * bm25() is bit-equal on every row of every query of class A (no NOT, single-token phrases, prefixes allowed) and of class B
    (A plus NOTs without an OR ancestor whose right side holds no NOT);
  * on all other queries the scores differ from SQLite's on at most 0.5 % of the matched rows (SQLite's cursor leftovers:
    a phrase right of a NOT counted when its cursor rests on the row, an OR below an AND next to phrases of several tokens);
  * seven planted misreadings of the rule each break the bit-equality of class A or B, or exceed that cap."""
import os
import random
import re
import sqlite3
import struct
import subprocess

import pytest

from helpers import ROOT

from next_plaid_amd import text as T
import text_expr_restate as X

SEEDS = range(8)            # tables; QUERIES queries each
QUERIES = 300
OTHER_CAP = 0.005           # share of matched rows of the other queries whose score may differ from SQLite's


def bits(x):
    return struct.pack("<d", x)


def sqlite_table(texts, tokenizer="unicode61"):
    conn = sqlite3.connect(":memory:")
    T.create_fts_tables(conn, tokenizer, content_synced=False)
    T.insert_fts_rows(conn, texts, range(len(texts)), tokenizer, content_synced=False)
    return conn


def sqlite_rows(conn, match):
    """{rowid: -bm25()} of a MATCH."""
    return {int(r[0]): -float(r[1]) for r in
            conn.execute(f'SELECT rowid, bm25("{T.FTS_TABLE}") FROM "{T.FTS_TABLE}" WHERE "{T.FTS_TABLE}" MATCH ?', (match,))}


@pytest.fixture(scope="module")
def tables():
    out = []
    for seed in SEEDS:
        rng = random.Random(1000 + seed)
        texts = X.make_table(rng, [5, 17, 60, 200][seed % 4])
        data = T.TextIndexData.from_texts(texts)
        out.append((seed, texts, data, X.RestatedExpr(data, len(texts)), sqlite_table(texts)))
    yield out
    for t in out:
        t[4].close()


def generated(seed):
    """[(class, text)] of a table's queries: a third without NOT and with single-token phrases (class A), a third with NOTs,
    a third with phrases of several tokens too."""
    rng = random.Random(2000 + seed)
    out = []
    for qi in range(QUERIES):
        tree = X.random_tree(rng, rng.randint(1, 4), multi=qi % 3 == 2, nots=qi % 3 != 0)
        out.append((X.tree_class(tree), X.tree_text(tree, True, rng)))
    return out


def compare(tables, defect=None):
    """{class: [queries, matched rows, rows whose bits differ]} and the queries whose matching set differs."""
    tot, sets = {"A": [0, 0, 0], "B": [0, 0, 0], "other": [0, 0, 0]}, []
    for seed, texts, data, rs, conn in tables:
        for cls, text in generated(seed):
            want = sqlite_rows(conn, text)
            got = rs.expr_scores(T.compile_text_expr(text, data), defect)
            if set(got) != set(want):
                sets.append(text)
                continue
            t = tot[cls]
            t[0] += 1
            t[1] += len(got)
            t[2] += sum(1 for d in got if bits(got[d]) != bits(want[d]))
    return tot, sets


def test_scores_against_sqlite(tables):
    tot, sets = compare(tables)
    print("queries, matched rows, rows that differ from SQLite:", tot)
    assert not sets, sets[:5]
    assert tot["A"][0] >= 700 and tot["A"][1] > 10_000 and tot["B"][0] >= 100 and tot["B"][1] > 500 and tot["other"][1] > 5_000
    assert tot["A"][2] == 0 and tot["B"][2] == 0                       # bit-equal on every row
    assert tot["other"][2] <= OTHER_CAP * tot["other"][1], tot["other"]


@pytest.mark.parametrize("defect", X.DEFECTS)
def test_a_planted_defect_is_caught(tables, defect):
    """Each misreading of the rule breaks a class-A/B assertion or exceeds the cap of the other queries."""
    tot, sets = compare(tables, defect)
    print(defect, tot, len(sets))
    assert tot["A"][2] > 0 or tot["B"][2] > 0 or tot["other"][2] > OTHER_CAP * tot["other"][1]


def test_precedence_without_parentheses_and_syntax_errors(tables):
    """Token soup over words, operators, +, *, parentheses, a quoted phrase, "" and an unknown word: SQLite and the compiler
    accept the same strings, and the accepted ones match the same rows -- implicit AND (between phrases only) binds
    tightest, then NOT, AND, OR.  Then the generator's trees written without any parentheses."""
    seed, texts, data, rs, conn = tables[2]
    alphabet = X.WORDS + ["AND", "OR", "NOT", "+", "*", "(", ")", '"ab c"', '""', X.UNKNOWN]
    weights = [3] * len(X.WORDS) + [6, 6, 6, 3, 3, 3, 3, 2, 1, 1]
    rng = random.Random(7)
    n_ok = n_err = n_mid = 0
    for _ in range(3000):
        text = " ".join(rng.choices(alphabet, weights, k=rng.randint(1, 9)))
        try:
            want = set(sqlite_rows(conn, text))
        except sqlite3.OperationalError:
            want = None
        try:
            got = set(rs.expr_scores(T.compile_text_expr(text, data)))
        except T.TextQueryError as e:
            got = None
            if "before the end of a phrase" in str(e):
                # the ONE construct SQLite takes and the compiler refuses by name: a* + b, a prefix inside a phrase
                # (np_text_expr has one prefix range per phrase, for its last token).  Nothing else is left out
                assert re.search(r"\*\s*\+", text), text
                n_mid += 1
                continue
        assert (want is None) == (got is None) and want == got, text
        n_ok += want is not None
        n_err += want is None
    print(f"accepted by both {n_ok}, rejected by both {n_err}, left out for a prefix inside a phrase {n_mid}")
    assert n_ok > 500 and n_err > 500 and n_mid < 0.03 * 3000
    rng = random.Random(8)
    for _ in range(600):
        text = X.tree_text(X.random_tree(rng, rng.randint(1, 4)), False, rng)
        assert set(rs.expr_scores(T.compile_text_expr(text, data))) == set(sqlite_rows(conn, text)), text


def test_known_trees_and_what_they_compile_to(tables):
    seed, texts, data, rs, conn = tables[3]
    v = data.vocab
    q = T.compile_text_expr('ab b OR c NOT d AND "ca da" *', data)     # ab b OR ((c NOT d) AND "ca da"*)
    P, AND, OR, NOT = T.NP_TEXT_NODE_PHRASE, T.NP_TEXT_NODE_AND, T.NP_TEXT_NODE_OR, T.NP_TEXT_NODE_NOT
    assert q.phrases() == [[v["ab"]], [v["b"]], [v["c"]], [v["d"]], [v["ca"], v["da"]]]
    assert q.prefix == [None, None, None, None, T.prefix_range("da", data)] and q.prefix_hi().tolist() == [0, 0, 0, 0, v["da"] + 1]
    assert q.nodes.tolist() == [[P, 0, 0], [P, 1, 0], [AND, 0, 1], [P, 2, 0], [P, 3, 0], [NOT, 3, 4], [P, 4, 0], [AND, 5, 6], [OR, 2, 7]]
    assert T.prefix_range("ab", data) == (v["ab"], v["abd"] + 1) and T.prefix_range("a", data) == (0, v["abd"] + 1)
    lo, hi = T.prefix_range("zz", data)
    assert lo == hi == data.n_terms
    q = T.compile_text_expr("zq* OR a + b*", data)                     # an empty range; + makes one phrase
    assert q.phrases() == [[-1], [-1, v["b"]]] and q.prefix_hi().tolist() == [0, v["bab"] + 1] and q.prefix[0][0] == q.prefix[0][1]
    for text in ("ab NOT b NOT c", "ab OR b AND c", "ab AND b OR c", "ab b NOT c d", "(ab OR b) AND c"):
        assert set(rs.expr_scores(T.compile_text_expr(text, data))) == set(sqlite_rows(conn, text))
    # a lifted flat query is the chain from the left
    flat = T.TextQuery.from_phrases([[1], [2, 3], [4]], T.NP_TEXT_OR)
    e = T.TextExpr.from_query(flat)
    assert e.phrases() == flat.phrases() and e.nodes.tolist() == [[P, 0, 0], [P, 1, 0], [OR, 0, 1], [P, 2, 0], [OR, 2, 3]]
    assert e.prefix == [None] * 3 and not e.prefix_hi().any()


@pytest.mark.parametrize("text", ['"" OR ab', 'ab OR ""', 'ab AND ""', '"" AND ab', 'ab NOT ""', '"" NOT ab', 'ab "" b', '"" ""',
                                  '("" OR ab) NOT b', '"!!" ab OR "?" c', '"" *', 'ab NOT ("" "")'])
def test_phrases_without_tokens_do_what_sqlite_does(tables, text):
    for seed, texts, data, rs, conn in tables[2:4]:
        want = sqlite_rows(conn, text)
        got = rs.expr_scores(T.compile_text_expr(text, data))
        assert set(got) == set(want) and all(bits(got[d]) == bits(want[d]) for d in got), text


def test_trigram_phrases_and_its_refused_prefix():
    texts = ["abcdef ghij", "bcdefg", "ab", "xyz abcd", "cdef ghi"]
    data = T.TextIndexData.from_texts(texts, "trigram")
    rs, conn = X.RestatedExpr(data, len(texts)), sqlite_table(texts, "trigram")
    for text in ("abcd NOT ghi", "(bcd OR xyz) AND cde", "ab OR cdef", "abc NOT ab", "ab NOT cde", "xy + zab OR ghij"):
        want = sqlite_rows(conn, text)
        got = rs.expr_scores(T.compile_text_expr(text, data))
        assert set(got) == set(want) and all(bits(got[d]) == bits(want[d]) for d in got), text
    with pytest.raises(T.TextQueryError, match=r"prefix query \(\*\) under the trigram tokenizer"):
        T.compile_text_expr("abc* OR def", data)
    conn.close()


@pytest.mark.parametrize("text,names", [("NEAR(ab b)", "NEAR"), ("ab AND NEAR(ab b, 3)", "NEAR"), ("^ab", r"\^"), ("ab OR ^b", r"\^"),
                                        ("c : ab", ":"), ("{c} : ab", "column filter"), ("- c : ab", "column filter"),
                                        ("ab* + b", "before the end of a phrase"), ("(ab) (b)", "syntax error"),
                                        ('("ab" "b") "c"', "syntax error"), ("ab (b)", "syntax error"), ("ab AND", "syntax error"),
                                        ("OR ab", "syntax error"), ("(ab", "syntax error"), ("ab)", "syntax error"), ("ab NOT NOT b", "syntax error"),
                                        ("*", "syntax error"), ("ab + ", "syntax error"), ('"ab', "unterminated"), ("ab & b", "syntax error"),
                                        ("", "empty query"), ("ab , b", "NEAR")])
def test_refusals_name_the_construct(tables, text, names):
    data = tables[0][2]
    with pytest.raises(T.TextQueryError, match=names):
        T.compile_text_expr(text, data)


def test_limits_of_a_compiled_tree(tables):
    data = tables[3][2]
    q = T.compile_text_expr(" OR ".join(["ab"] * 64), data)
    assert q.n_phrases == 64 and q.n_nodes == T.NP_TEXT_MAX_NODES
    with pytest.raises(T.TextQueryError, match="more than 64 phrases"):
        T.compile_text_expr(" OR ".join(["ab"] * 65), data)
    assert T.compile_text_expr('"' + "ab " * 250 + '" NOT "' + "b " * 6 + '"', data).terms.size == 256
    with pytest.raises(T.TextQueryError, match="more than 256 tokens"):
        T.compile_text_expr('"' + "ab " * 250 + '" NOT "' + "b " * 7 + '"', data)
    # the cap of a phrase of several tokens that ends in a prefix; a single-token prefix has none
    wide = T.TextIndexData.from_texts([" ".join(f"px{i:04d}" for i in range(d, 1100, 10)) for d in range(10)] + ["head px0001"])
    assert T.compile_text_expr("px*", wide).prefix[0] == (wide.vocab["px0000"], wide.vocab["px0000"] + 1100)
    assert T.compile_text_expr('"head px0" *', wide).prefix_hi()[0] == wide.vocab["px0000"] + 1000
    with pytest.raises(T.TextQueryError, match="NP_TEXT_MAX_PREFIX_TERMS = 1024"):
        T.compile_text_expr("ab OR head + px*", wide)


def test_the_flat_compiler_still_refuses_what_it_refused(tables):
    data = tables[0][2]
    for text, name in (("ab NOT b", "NOT"), ("(ab OR b) AND c", "parentheses"), ("ab*", r"prefix query \(\*\)"),
                       ("ab + b", r"phrase concatenation \(\+\)"), ("ab AND b OR c", "AND mixed with OR")):
        with pytest.raises(T.TextQueryError, match=name):
            T.compile_text_query(text, data)


def test_tree_check_of_the_host_code_stands_alone(tmp_path):
    """tests/cpp/text_expr_plan_check.cpp: text_check_expr of np_text_plan.h with the host compiler alone (no device, no
    library), plain and as its own program under AddressSanitizer + UBSan."""
    src = os.path.join(ROOT, "tests", "cpp", "text_expr_plan_check.cpp")
    inc = os.path.join(ROOT, "next-plaid_amd", "csrc")
    for name, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / f"text_expr_plan_check_{name}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, src, "-o", str(exe)])
        out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "all checks passed" in out.stdout, name + ": " + out.stdout + out.stderr
