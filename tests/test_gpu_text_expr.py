"""Keyword search with FTS5's boolean grammar and prefix queries on the device: np_hip_text_search_expr, its filtered form
and np_hip_search_hybrid_expr.  Needs a real MI355X.

The reference is tests/text_expr_restate.py (which tests/test_text_expr_restate_cpu.py pins to SQLite's own FTS5): ids, f32
scores and counts bit for bit, without exception.  Flat queries sent as trees are compared with np_hip_text_search's bytes,
the hybrid call with the composition of the separate calls."""
import os
import random
import subprocess

import numpy as np
import pytest

from helpers import ROOT, hip_index, make_arrays

import next_plaid_amd as npa
from next_plaid_amd import api, synth, text as T
import text_restate as R
import text_expr_restate as X

pytestmark = pytest.mark.gpu

SLICE = 4096   # documents per slice of the kernel (NP_TEXT_SLICE_DOCS, np_text_plan.h)
COUNTS = [1, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 1]
CAP = T.NP_TEXT_MAX_TOPK
E = T.TextExpr.from_tree


def tiny_index(n_docs, **opts):
    """An index of n_docs one-token documents: the keyword search only needs its document count."""
    spec, a = make_arrays(num_docs=n_docs, num_centroids=16, dim=32, nbits=2, doc_len_min=1, doc_len_max=1, seed=3)
    return a, hip_index(a, **opts)


def corpus_texts(n):
    """Documents of 0..13 words that share prefixes (text_expr_restate.WORDS).  "lefty" stands in document SLICE - 1 alone
    and "righty" in document SLICE alone (where the table has them): the two sides of the first slice boundary; documents
    10..13 are copies of one another (ties); "solo" stands in the last document."""
    rng = random.Random(n)
    texts = X.make_table(rng, n)
    for d in range(10, min(14, n)):
        texts[d] = "ab abc ca ab"
    if n > SLICE - 1:
        texts[SLICE - 1] = "lefty ab abd"
    if n > SLICE:
        texts[SLICE] = "righty cab cab"
    texts[n - 1] = (texts[n - 1] + " solo ab").strip()
    return texts


def special_trees(data):
    v = data.vocab
    ph = lambda *ws, star=None: ("phrase", [v.get(w, -1) for w in ws], T.prefix_range(star, data) if star else None)
    return [
        # the documents next to the slice boundary, reached through different branches of one tree
        E(("or", ("and", ph("lefty"), ph("ab", star="ab")), ("not", ph("righty"), ph("zq")))),
        E(("not", ("or", ph("lefty"), ph("righty")), ph("abd"))),                      # only the right one is left
        E(("and", ("or", ph("lefty"), ph("righty")), ("or", ph("abd"), ph("cab")))),
        E(("or", ph("solo"), ph("lefty"))),
        E(("not", ph("ab"), ph("ab"))),                                               # a NOT that removes every row
        E(("not", ph("ab"), ph("a", star="a"))),                                      # ... by a prefix
        E(("or", ph("zq"), ph("ca"))),                                                # an unknown token under OR
        E(("not", ph("ca"), ph("zq"))),                                               # ... on a NOT's right: nothing is removed
        E(("and", ph("ab"), ("or", ph("ab"), ph("ab")))),                             # one phrase three times: three idf terms
        E(ph("ab", star="ab")), E(ph("a", star="a")), E(ph("zq", star="zq")),          # prefixes: some, some, none
        E(("phrase", [0], (0, data.n_terms))),                                        # the whole vocabulary
        E(("and", ph("ab", "abc", star="abc"), ph("c", star="c"))),
        E(("or", ph("ab", "a", star="a"), ("not", ph("b", star="b"), ph("ca", "c", star="c")))),
        E(("not", ph("ab", star="ab"), ("not", ph("abc"), ph("abd")))),                # a NOT inside a NOT's right
    ]


@pytest.fixture(scope="module", params=COUNTS)
def sized(request):
    n = request.param
    data = T.TextIndexData.from_texts(corpus_texts(n))
    a, hx = tiny_index(n)
    hx.set_text(data)
    rs = X.RestatedExpr(data, n)
    rng = random.Random(n + 1)
    queries = special_trees(data) + [X.tree_expr(X.random_tree(rng, rng.randint(1, 4)), data) for _ in range(56)]
    yield n, data, hx, rs, queries, {}
    hx.close()


def expect(rs, want, qi, q, k, subset=None, tag=None):
    key = (qi, k, tag)
    if key not in want:
        if (qi, "scores") not in want:
            want[(qi, "scores")] = rs.expr_scores(q)
        want[key] = rs.rank(want[(qi, "scores")], k, subset)
    return want[key]


def same(r, ids, sc):
    return (r.passage_ids.dtype == np.int64 and r.scores.dtype == np.float32 and np.array_equal(r.passage_ids, ids)
            and np.array_equal(r.scores.view(np.uint32), sc.view(np.uint32)))


def same_rows(a, b):
    return len(a) == len(b) and all(same(x, y.passage_ids, y.scores) for x, y in zip(a, b))


def test_more_than_64_trees_equal_the_restatement(sized):
    n, data, hx, rs, queries, want = sized
    assert len(queries) > 64
    got = hx.text_search(queries, 10)
    hits = 0
    for i, (q, r) in enumerate(zip(queries, got)):
        ids, sc = expect(rs, want, i, q, 10)
        assert same(r, ids, sc), f"n={n} query {i} {q.phrases()} {q.prefix} {q.nodes.tolist()}: {r.passage_ids[:5]} {r.scores[:5]} vs {ids[:5]} {sc[:5]}"
        hits += ids.size
    assert hits > 0 and hx.last_stats["n_queries"] == len(queries)
    assert got[4].passage_ids.size == 0 and got[5].passage_ids.size == 0         # the NOTs that remove every row
    assert same(got[7], *expect(rs, want, 7, queries[7], 10)) and (n < 20 or got[7].passage_ids.size > 0)
    if n > SLICE:
        assert SLICE - 1 in got[0].passage_ids and SLICE in got[0].passage_ids   # both sides of the boundary, two branches
        assert got[1].passage_ids.tolist() == [SLICE] and sorted(got[2].passage_ids.tolist()) == [SLICE - 1, SLICE]
    assert same_rows(hx.text_search(queries, 10), got)                           # the same bits from run to run


@pytest.mark.parametrize("top_k", [1, CAP])
def test_top_k_one_and_the_cap_and_ties(sized, top_k):
    n, data, hx, rs, queries, want = sized
    pick = list(range(16)) + [20, 30, 40]
    got = hx.text_search([queries[i] for i in pick], top_k)
    for i, r in zip(pick, got):
        assert same(r, *expect(rs, want, i, queries[i], top_k)), f"n={n} top_k={top_k} query {i}"
    if n > 2 * CAP and top_k == CAP:
        assert max(r.passage_ids.size for r in got) == CAP
    if n > 14 and top_k == CAP:   # the copies 10..13 tie and come in ascending order
        ids = got[8].passage_ids.tolist()
        at = ids.index(10)
        assert ids[at: at + 4] == [10, 11, 12, 13] and len(set(got[8].scores[at: at + 4].tolist())) == 1


def test_subset_subsets_and_filters_equal_the_restatement_on_the_ids(sized):
    n, data, hx, rs, queries, want = sized
    pick = [0, 1, 2, 3, 6, 8, 9, 10, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25]
    qs = [queries[i] for i in pick]
    everything, nothing, last = np.arange(n), np.zeros(0, np.int64), np.array([n - 1])
    some = np.array(sorted({0, 2, n // 2, n - 1, n + 5, -3} | set(range(1, n, 3)) | {SLICE - 1}), np.int64)
    subsets = [[None, nothing, everything, last, some, some][j % 6] for j in range(len(qs))]
    got = hx.text_search(qs, 10, subsets=subsets)
    for j, (i, r) in enumerate(zip(pick, got)):
        assert same(r, *expect(rs, want, i, queries[i], 10, subsets[j], tag=j % 6)), f"n={n} query {i} subset {j % 6}"
    got = hx.text_search(qs, 10, subset=some)
    for i, r in zip(pick, got):
        assert same(r, *expect(rs, want, i, queries[i], 10, some, tag=4)), f"n={n} query {i}"
    hx.set_columns({"docno": np.arange(n, dtype=np.int64), "z": np.arange(n, dtype=np.int64) % 5})
    try:
        conds = [("z = ?", [1]), None, ("docno >= ?", [n - 1]), ("0 = 1", []), ("1 = 1", []), ("z = ?", [1])]
        it = iter(hx.filter_ids([c for c in conds if c is not None]))
        subs = [None if c is None else next(it) for c in conds]
        a = hx.text_search(qs[:6], 10, filters=conds)
        for j, (i, r) in enumerate(zip(pick[:6], a)):
            assert same(r, *expect(rs, want, i, queries[i], 10, subs[j], tag=("f", j))), f"n={n} query {i} filter {j}"
        assert a[3].passage_ids.size == 0
    finally:
        hx.set_columns({})


def test_flat_queries_as_trees_return_the_flat_entrys_bytes(sized):
    n, data, hx, rs, queries, want = sized
    flat = R.random_queries(data, 60, seed=n) + [T.TextQuery.from_phrases([[0]] * 64, m) for m in (T.NP_TEXT_AND, T.NP_TEXT_OR)]
    for k in (10, CAP):
        a = hx.text_search(flat, k)
        b = hx.text_search([T.TextExpr.from_query(q) for q in flat], k)
        assert same_rows(b, a) and hx.last_stats["n_queries"] == len(flat), f"n={n} top_k={k}"
    assert n < 20 or sum(r.passage_ids.size for r in a) > 0


def test_a_query_alone_in_a_mixed_batch_and_in_chunks_has_the_same_bytes():
    """2 slices + 1 document are 3 slices.  A batch of flat queries and trees (prefixes among them: every query of a chunk
    then owns frequency arrays of 4 * 8256 bytes each) under max_batch = 5 (chunks of queries) and under a workspace of
    120 kB, which at top_k = 1024 holds the results of three queries (37 kB), one query's share (12 kB of lists and one
    frequency array) and two of its three slices (12 292 bytes each): chunks of slices.  40 kB do not hold one query."""
    n = 2 * SLICE + 1
    data = T.TextIndexData.from_texts(corpus_texts(n))
    rng = random.Random(5)
    trees = special_trees(data) + [X.tree_expr(X.random_tree(rng, 3), data) for _ in range(10)]
    flat = R.random_queries(data, 8, seed=3)
    mixed = [q for pair in zip(trees, flat + flat + flat + flat) for q in pair]
    a, hx = tiny_index(n)
    hx.set_text(data)
    try:
        batch = hx.text_search(mixed, 10)
        for i in (0, 1, 2, 3, 10, 18, 19, 24, 26, 28, 30):
            assert same_rows(hx.text_search([mixed[i]], 10), [batch[i]]), f"query {i} alone"
        assert same_rows(hx.text_search(mixed[::-1], 10)[::-1], batch)
        assert same_rows(hx.text_search(flat, 10), [batch[2 * j + 1] for j in range(8)])      # the flat entry's bytes
        wide3 = [trees[9], trees[10], trees[12]]   # prefixes with more matches than the cap
        cap = hx.text_search(wide3, CAP)
        assert max(r.passage_ids.size for r in cap) == CAP
    finally:
        hx.close()
    for opts, qs, k, want in (({"max_batch": 5}, mixed, 10, batch), ({"workspace_bytes": 120_000}, wide3, CAP, cap),
                              ({"workspace_bytes": 400_000}, mixed, 10, batch)):
        a, hx = tiny_index(n, **opts)
        hx.set_text(data)
        try:
            assert same_rows(hx.text_search(qs, k), want), str(opts)
        finally:
            hx.close()
    a, tight = tiny_index(n, workspace_bytes=40_000)   # the frequency arrays of one query do not fit
    tight.set_text(data)
    try:
        with pytest.raises(MemoryError, match="workspace budget"):
            tight.text_search([trees[14]], 10)
    finally:
        tight.close()


# ---- the limits of a tree ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def limits():
    n = 40
    data = T.TextIndexData.from_texts(R.limit_texts(n))
    a, hx = tiny_index(n)
    hx.set_text(data)
    yield n, data, hx, X.RestatedExpr(data, n)
    hx.close()


def chain(leaves, op, left_deep):
    if left_deep:
        t = leaves[0]
        for x in leaves[1:]:
            t = (op, t, x)
        return t
    t = leaves[-1]
    for x in reversed(leaves[:-1]):
        t = (op, x, t)
    return t


def test_trees_at_the_limits(limits):
    n, data, hx, rs = limits
    v = data.vocab
    w = [("phrase", [v[x]]) for x in R.LIMIT_WORDS]
    aa, bb = ("phrase", [v["aa"]]), ("phrase", [v["bb"]])
    trees = {
        "64 words OR, left-deep": chain(w, "or", True), "64 words OR, right-deep": chain(w, "or", False),
        "64 words AND, left-deep": chain(w, "and", True), "64 words AND, right-deep": chain(w, "and", False),
        "aa NOT 63 words, left-deep": chain([aa] + w[:63], "not", True),
        "63 NOTs, right-deep": chain(w[:63] + [aa], "not", False),
        "alternating": chain([("or", x, y) for x, y in zip(w[0::2], w[1::2])], "and", True),
        "256 tokens": ("or", ("phrase", [v["aa"]] * 250), ("phrase", [v["bb"], v["aa"]] * 3)),
        "aa NOT aa": ("not", aa, aa), "unknown OR aa": ("or", ("phrase", [-1]), aa), "aa NOT unknown": ("not", aa, ("phrase", [-1])),
        "aa three times": ("and", aa, ("or", aa, ("not", aa, bb))),
    }
    names = list(trees)
    exprs = [E(trees[k]) for k in names]
    assert exprs[0].n_phrases == 64 and exprs[0].n_nodes == 127 and exprs[1].nodes[-1].tolist()[1] == 0
    got = hx.text_search(exprs, n)
    for name, q, r in zip(names, exprs, got):
        ids, sc = rs.expr_search(q, n)
        assert same(r, ids, sc), f"{name}: {r.passage_ids} {r.scores} vs {ids} {sc}"
    by = dict(zip(names, got))
    assert by["aa NOT aa"].passage_ids.size == 0 and by["64 words OR, left-deep"].passage_ids.size > 4
    assert by["64 words AND, left-deep"].passage_ids.size > 0 and by["256 tokens"].passage_ids.size > 0
    assert same(by["aa NOT unknown"], by["unknown OR aa"].passage_ids, by["unknown OR aa"].scores)
    assert same(by["64 words OR, left-deep"], by["64 words OR, right-deep"].passage_ids, by["64 words OR, right-deep"].scores)
    one = hx.text_search([E(aa)], n)[0]                      # each occurrence of a phrase adds its own term
    assert by["aa three times"].passage_ids.size > 0 and not np.array_equal(by["aa three times"].scores, one.scores[: by["aa three times"].scores.size])


@pytest.fixture(scope="module")
def wide():
    """1200 terms px0000.. that share a prefix, four per document in a row, behind the word "head", in 300 documents; the
    last document holds two of them, one twice."""
    n = 301
    texts = [" ".join(["head"] + [f"px{(4 * d + j) % 1200:04d}" for j in range(4)] + ["tail"]) for d in range(n - 1)]
    texts.append("head px0003 px0003 head px0004 other")
    data = T.TextIndexData.from_texts(texts)
    a, hx = tiny_index(n)
    hx.set_text(data)
    yield n, data, hx, X.RestatedExpr(data, n)
    hx.close()


def test_prefix_ranges_of_no_one_and_every_term_and_the_cap_of_a_phrase(wide):
    n, data, hx, rs = wide
    v = data.vocab
    lo = v["px0000"]
    assert T.prefix_range("px", data) == (lo, lo + 1200) and T.prefix_range("px0003", data) == (v["px0003"], v["px0003"] + 1)
    assert T.prefix_range("pz", data)[0] == T.prefix_range("pz", data)[1]
    head = v["head"]
    cap = T.NP_TEXT_MAX_PREFIX_TERMS
    trees = [("phrase", [lo], (lo, lo + 1200)), ("phrase", [v["px0003"]], T.prefix_range("px0003", data)),
             ("phrase", [-1], T.prefix_range("pz", data)), ("phrase", [0], (0, data.n_terms)),
             ("phrase", [head, lo], (lo, lo + cap)),                                   # several tokens, at the cap
             ("phrase", [head, lo], (lo, lo + 4)), ("phrase", [v["px0003"], head, lo], (lo, lo + 5)),
             ("not", ("phrase", [lo], (lo, lo + 1200)), ("phrase", [head, lo], (lo, lo + 8))),
             ("or", ("phrase", [lo], (lo, lo + 3)), ("phrase", [lo + 2], (lo + 2, lo + 6)))]   # overlapping ranges
    exprs = [E(t) for t in trees]
    got = hx.text_search(exprs, n)
    for i, (q, r) in enumerate(zip(exprs, got)):
        ids, sc = rs.expr_search(q, n)
        assert same(r, ids, sc), f"tree {i}: {r.passage_ids[:6]} {r.scores[:6]} vs {ids[:6]} {sc[:6]}"
    assert got[0].passage_ids.size == n and got[2].passage_ids.size == 0 and got[3].passage_ids.size == n
    hx.text_search(exprs[:1], n)
    assert hx.last_stats["n_ivf_ids"] == 1200 + 2                # the postings of the range: its pre-pass walked them once
    # the last document holds px0003 twice and px0004 once: the frequencies add (3) and nHit counts it once
    f, hit = rs.expr_phrase_freqs([lo], (lo, lo + 1200))
    assert f[n - 1] == 3 and hit == n and n - 1 in got[1].passage_ids
    assert got[4].passage_ids.size > 250 and got[6].passage_ids.tolist() == [n - 1]
    with pytest.raises(ValueError, match="NP_TEXT_MAX_PREFIX_TERMS = 1024"):   # beyond the cap: refused, nothing is launched
        hx.text_search([exprs[0], E(("phrase", [head, lo], (lo, lo + cap + 1)))], 5)
    assert same_rows(hx.text_search(["px* NOT px0003", '"head px00" *', "head + px0 *"], n, full_grammar=True),
                     hx.text_search([T.compile_text_expr(s, data) for s in ("px* NOT px0003", '"head px00" *', "head + px0 *")], n))
    assert hx.text_search(['"head px00" *'], n, full_grammar=True)[0].passage_ids.size > 0
    with pytest.raises(T.TextQueryError, match=r"\*"):        # the default keeps refusing what compile_text_query refuses
        hx.text_search(["px*"], 5)


# ---- the hybrid request -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hybrid():
    spec, a = make_arrays(num_docs=1500, num_centroids=64, dim=32, nbits=2, doc_len_min=4, doc_len_max=12, seed=11)
    hx = hip_index(a)
    data = T.TextIndexData.from_texts(corpus_texts(1500))
    hx.set_text(data)
    qs, _ = synth.make_queries(spec, 9, n_tokens=8, cen=a["centroids"])
    yield spec, a, hx, data, list(qs)
    hx.close()


@pytest.mark.parametrize("fusion,alpha", [("relative_score", 0.75), ("rrf", 0.5)])
def test_search_hybrid_with_trees_equals_the_calls_composed(hybrid, fusion, alpha):
    spec, a, hx, data, qs = hybrid
    texts = ["ab NOT ca", "(ab OR b) AND c NOT d", "ca*", "", "zq", '"ab ab" OR solo', "a* NOT (b* OR c*)", "d + a* OR e", "ab"]
    p = npa.SearchParameters(n_full_scores=128, top_k=7, n_ivf_probe=4)
    some = np.arange(0, 1500, 3)
    hx.set_columns({"z": np.arange(1500, dtype=np.int64) % 3})
    try:
        for scope in ({}, {"subsets": [None, some, some, None, some, np.zeros(0, np.int64), None, some, np.arange(1500)]},
                      {"subset": some}, {"filters": [("z = ?", [0])] * 9}):
            fk = 21
            sem = hx.search_batch(qs, npa.SearchParameters(n_full_scores=128, top_k=fk, n_ivf_probe=4), **scope)
            kw = hx.text_search(texts, fk, full_grammar=True, **scope)
            assert kw[3].passage_ids.size == 0 and kw[4].passage_ids.size == 0 and kw[0].passage_ids.size > 0
            want = npa.fuse(fusion, alpha, 7, [r.passage_ids for r in sem], [r.scores for r in sem], [r.passage_ids for r in kw],
                            [r.scores for r in kw], index=hx)
            got = hx.search_hybrid(qs, texts, p, alpha=alpha, fusion=fusion, full_grammar=True, **scope)
            for i, (r, (ids, sc)) in enumerate(zip(got, want)):
                assert np.array_equal(r.passage_ids, ids) and r.scores.tobytes() == sc.tobytes(), f"{fusion} {list(scope)} q{i}"
        assert sum(r.passage_ids.size for r in got) > 0
    finally:
        hx.set_columns({})


def test_errors_are_reported_before_any_launch(hybrid):
    spec, a, hx, data, qs = hybrid
    q1 = E(("not", ("phrase", [0]), ("phrase", [1])))
    p = npa.SearchParameters(n_full_scores=128, top_k=5, n_ivf_probe=4)
    bare = hip_index(a)
    try:
        with pytest.raises(ValueError, match="no keyword index"):
            bare.text_search([q1], 5)
        with pytest.raises(ValueError, match="no keyword index"):
            bare.search_hybrid(qs[:1], [q1], p)
    finally:
        bare.close()
    for k in (0, CAP + 1):
        with pytest.raises(ValueError, match="top_k"):
            hx.text_search([q1], k)

    def raw(nodes, phrases=((0,), (1,)), prefix_hi=None):
        """np_hip_text_search_expr with a node list as given"""
        q = T.TextExpr.from_tree(chain([("phrase", list(x)) for x in phrases], "and", True))
        q.nodes = np.asarray(nodes, np.int32).reshape(-1, 3)
        tq = api._CTextExprs([q1, q])
        if prefix_hi is not None:
            hi = np.asarray(prefix_hi, np.int32)
            tq.keep.append(hi)
            tq.arr[1].prefix_hi = hi.ctypes.data
        rows = api._ResultRows(2, 5)
        api._check(api.lib().np_hip_text_search_expr(hx._h, tq.arr, 2, 5, None, None, 0, None, *rows.ptrs(), None))
        return rows.results()

    P, AND, NOT = T.NP_TEXT_NODE_PHRASE, T.NP_TEXT_NODE_AND, T.NP_TEXT_NODE_NOT
    assert raw([(P, 0, 0), (P, 1, 0), (NOT, 0, 1)])[1].passage_ids.tolist() == hx.text_search([q1], 5)[0].passage_ids.tolist()
    for nodes, what in (([(P, 0, 0), (AND, 0, 0), (P, 1, 0)], "text query 1: node 1: the stack holds 1"),
                        ([(P, 0, 0), (P, 1, 0)], "2 nodes are left on the stack"),
                        ([(P, 0, 0), (P, 0, 0), (AND, 0, 1)], "names phrase 0 a second time"),
                        ([(P, 0, 0), (P, 2, 0), (AND, 0, 1)], "names phrase 2, which the query does not have"),
                        ([(P, 0, 0), (P, 1, 0), (AND, 1, 0)], "not the two nodes on top of the stack"),
                        ([(P, 0, 0), (P, 1, 0), (AND, 0, 2)], "not below the node's own"),
                        ([(P, 0, 0), (P, 1, 0), (7, 0, 1)], "unknown op 7"),
                        ([(P, 0, 0)], "phrase 1 is named by no node")):
        with pytest.raises(ValueError, match=what):
            raw(nodes)
    ok = [(P, 0, 0), (P, 1, 0), (AND, 0, 1)]
    with pytest.raises(ValueError, match="prefix range ends at"):
        raw(ok, prefix_hi=[0, data.n_terms + 1])
    with pytest.raises(ValueError, match="prefix range ends at"):
        raw(ok, prefix_hi=[0, 1])
    with pytest.raises(ValueError, match="n_nodes"):
        raw(np.zeros((0, 3), np.int32))
    assert hx.text_search([], 5, full_grammar=True) == [] and hx.text_search([""], 5, full_grammar=True)[0].passage_ids.size == 0


def test_cpp_mirror_prints_the_same_bits(tmp_path):
    """tests/cpp/text_expr.cpp: TextExpr, text_search and search_hybrid of next_plaid.hpp against the Python calls."""
    spec, a = make_arrays(num_docs=96, num_centroids=16, dim=32, nbits=2, doc_len_min=3, doc_len_max=9, seed=5)
    exe = tmp_path / "text_expr"
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "text_expr.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    ixdir = tmp_path / "ix"
    ixdir.mkdir()
    synth.write_index(str(ixdir), {k: v for k, v in a.items() if k != "_prep"}, chunk_docs=40)
    data = T.TextIndexData.from_texts(R.make_texts(96, 8, seed=2, every="wo0", lens=(0, 1, 2, 3, 5, 8)))
    assert data.n_terms >= 5
    data.term_offsets.astype("<i8").tofile(tmp_path / "toff.i64")
    data.inst_doc.astype("<i8").tofile(tmp_path / "idoc.i64")
    data.inst_pos.astype("<i4").tofile(tmp_path / "ipos.i32")
    qs = list(synth.make_queries(spec, 6, n_tokens=5, cen=a["centroids"])[0])
    np.concatenate(qs, 0).astype("<f4").tofile(tmp_path / "q.f32")
    np.array([q.shape[0] for q in qs], "<i8").tofile(tmp_path / "lens.i64")
    out = subprocess.check_output([str(exe), str(ixdir), str(tmp_path / "toff.i64"), str(tmp_path / "idoc.i64"), str(tmp_path / "ipos.i32"),
                                   str(data.n_rows), str(tmp_path / "q.f32"), str(tmp_path / "lens.i64")], text=True)
    tq = [[E(("not", ("or", ("phrase", [0]), ("phrase", [1])), ("phrase", [2]))),
           E(("or", ("phrase", [2, 3]), ("phrase", [1], (1, 4)))),
           E(("or", ("and", ("phrase", [0]), ("phrase", [-1])), ("phrase", [4])))][i % 3] for i in range(6)]
    evens = np.arange(0, 60, 2)
    subsets = [evens if i % 2 == 1 else None for i in range(6)]

    def lines(stage, res):
        s = ""
        for i, r in enumerate(res):
            s += f"{stage} {i} {r.passage_ids.size}" + "".join(
                f" {d}:{b:08x}" for d, b in zip(r.passage_ids.tolist(), r.scores.view(np.uint32).tolist())) + "\n"
        return s

    hx = npa.MmapIndex.load(str(ixdir))
    try:
        hx.set_text(data)
        kw = hx.text_search(tq, 9, subsets=subsets)
        p = npa.SearchParameters(n_full_scores=64, top_k=5, n_ivf_probe=4)
        hy = hx.search_hybrid(qs, tq, p, alpha=0.75, fusion="relative_score", fetch_k=15, subsets=subsets)
        assert out == lines("text", kw) + lines("hybrid", hy)
        assert sum(r.passage_ids.size for r in kw) > 10 and sum(r.passage_ids.size for r in hy) > 10
        rs = X.RestatedExpr(data, 96)
        assert all(same(r, *rs.expr_search(q, 9, s)) for r, q, s in zip(kw, tq, subsets))
    finally:
        hx.close()
