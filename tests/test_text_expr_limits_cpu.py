"""The corpora and trees of tests/test_gpu_text_expr_limits.py (tests/text_limit_shapes.py) at a reduced size through SQLite's
own FTS5: the restatement that the device is compared with there is pinned here on the very shapes it is used on.  CPU only.

For every tree the FTS5 text is compiled by text.compile_text_expr, which must give the tree the GPU test builds without the
compiler; the matching set equals SQLite's; bm25() is bit-equal on every row of the trees of class A and B
(text_expr_restate.tree_class).  The trees that hold a phrase of several tokens are of neither class: for them the cap of
tests/test_text_expr_restate_cpu.py applies, at most 0.5 % of the matched rows may differ from SQLite's bits."""
import sqlite3
import struct

import numpy as np
import pytest

import text_limit_shapes as S

from next_plaid_amd import text as T
import text_expr_restate as X

OTHER_CAP = 0.005


def bits(x):
    return struct.pack("<d", x)


def sqlite_table(texts):
    conn = sqlite3.connect(":memory:")
    T.create_fts_tables(conn, "unicode61", content_synced=False)
    T.insert_fts_rows(conn, texts, range(len(texts)), "unicode61", content_synced=False)
    return conn


def sqlite_rows(conn, match):
    return {int(r[0]): -float(r[1]) for r in
            conn.execute(f'SELECT rowid, bm25("{T.FTS_TABLE}") FROM "{T.FTS_TABLE}" WHERE "{T.FTS_TABLE}" MATCH ?', (match,))}


def pin(data, named_trees, multi_token=()):
    """{name: {document: f64 score}} of the restatement, after the comparison with SQLite."""
    texts = S.texts_of(data)
    again = T.TextIndexData.from_texts(texts)        # the arrays the generator built are the tokenizer's
    assert again.terms == data.terms and again.n_rows == data.n_rows and np.array_equal(again.term_offsets, data.term_offsets)
    assert np.array_equal(again.inst_doc, data.inst_doc) and np.array_equal(again.inst_pos, data.inst_pos)
    rs = S.CachedExpr(data, data.n_rows)
    conn = sqlite_table(texts)
    out = {}
    try:
        for name, tree in named_trees:
            text = X.tree_text(tree)
            q, built = T.compile_text_expr(text, data), X.tree_expr(tree, data)
            assert q.phrases() == built.phrases() and q.prefix_hi().tolist() == built.prefix_hi().tolist(), name
            assert q.nodes.tolist() == built.nodes.tolist(), name
            want, got = sqlite_rows(conn, text), rs.expr_scores(built)
            assert set(got) == set(want), name
            differ = sum(1 for d in got if bits(got[d]) != bits(want[d]))
            cls = X.tree_class(tree)
            assert (cls == "other") == (name in multi_token), (name, cls)
            assert differ <= (OTHER_CAP * len(got) if cls == "other" else 0), (name, cls, differ, len(got))
            out[name] = got
    finally:
        conn.close()
    return rs, out


def test_long_run_corpus_and_trees_against_sqlite():
    n = 3000
    data, rev, big = S.long_run_corpus(n)
    multi = {"h + pa*", "h + pa* OR pc1*", "h + pa* NOT pb2*", "p* AND h + pa*"}
    rs, scores = pin(data, S.long_run_trees(), multi)
    S.check_long_run(data, rs, rev, big, None)
    assert len(scores) == 7 and all(len(set(sc.values())) >= 30 for sc in scores.values()), {k: len(set(v.values())) for k, v in scores.items()}
    assert big in scores["p*"] and all(int(r) in scores["p*"] and int(r) not in scores["h + pa*"] for r in rev)
    assert len(scores["p* NOT pc1*"]) < len(scores["p*"]) < len(scores["p* OR x1*"])


def test_families_corpus_and_trees_against_sqlite():
    n = 400
    data = S.families_corpus(n)
    trees = S.families_trees()
    rs, scores = pin(data, list(trees.items()), {"flat phrase"})
    assert [S.n_arrays(X.tree_expr(trees[k], data)) for k in S.UNEVEN] == S.UNEVEN_ARRAYS
    assert [S.n_arrays(X.tree_expr(trees[k], data)) for k in S.SHAPES_64] == [64, 64, 32, 33]
    assert sorted(scores["AND of 64 prefixes"]) == [17, n - 1] and len(scores["OR of 64 prefixes"]) == n
    assert 0 < len(scores["32 prefixes NOT a prefix"]) < len(scores["32 prefixes and 32 words"]) < n


@pytest.mark.parametrize("extra", [(), (10, 20, 30)])
def test_ties_corpus_and_trees_against_sqlite(extra):
    n = 50
    rs, scores = pin(S.ties_corpus(n, extra), S.ties_trees())
    for name, sc in scores.items():
        assert len(sc) == n and len(set(sc.values())) == (2 if extra else 1), name
