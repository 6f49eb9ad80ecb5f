"""The keyword search and the fusion at their limits: 64 phrases and 256-token phrases (text_score_kernel, text_phrase_freq), a
first posting list longer than the counting pass's grid (text_hit_kernel's second stride), corpora where every score is equal
(the order inside a slice, across slices, across the merge window's refill and across chunks of slices) and a fusion that
fills the whole 2048-entry window (fuse_kernel).  Needs a real MI355X.

The reference is tests/text_restate.py, ids equal and f32 scores equal as uint32; tests/test_text_restate_cpu.py pins it to
SQLite on the very query shapes used here."""
import numpy as np
import pytest

from text_limit_shapes import index_data, plan_constant, same, tiny_index

import next_plaid_amd as npa
from next_plaid_amd import text as T
import text_restate as R

pytestmark = pytest.mark.gpu

SLICE = 4096   # documents per slice of the scoring kernel (NP_TEXT_SLICE_DOCS, np_text_plan.h)
CAP = T.NP_TEXT_MAX_TOPK
WINDOW = 2 * CAP   # entries of the merge window and of a fusion


def test_the_constants_are_the_plans():
    assert plan_constant("NP_TEXT_SLICE_DOCS") == SLICE and T.NP_TEXT_MAX_PHRASES == 64 and T.NP_TEXT_MAX_TOKENS == 256


# ---- 1: the limits of a query ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def limits():
    n = SLICE + 1
    data = T.TextIndexData.from_texts(R.limit_texts(n))
    a, hx = tiny_index(n)
    hx.set_text(data)
    rs = R.Restated(data, n)
    named = R.limit_queries(data)
    scores = [rs.scores(q) for _, q in named]                              # one scoring per query serves every top_k
    # more than 64 queries in one call: the limit queries among small ones, AND and OR mixed
    small = R.random_queries(data, 60, seed=7)
    batch = small[:20] + [q for _, q in named[:4]] + small[20:40] + [q for _, q in named[4:]] + small[40:]
    where = list(range(20, 24)) + list(range(44, 48))
    yield n, data, hx, rs, named, scores, batch, where, {}
    hx.close()


@pytest.mark.parametrize("top_k", [1, 10, CAP])
def test_queries_at_the_limits_alone_and_in_a_batch(limits, top_k):
    n, data, hx, rs, named, scores, batch, where, want_small = limits
    assert len(batch) > 64 and [batch[i] for i in where] == [q for _, q in named]
    assert max(q.n_phrases for q in batch) == T.NP_TEXT_MAX_PHRASES and max(len(p) for q in batch for p in q.phrases()) == T.NP_TEXT_MAX_TOKENS
    got = hx.text_search(batch, top_k)
    sizes = {}
    for (name, q), sc, i in zip(named, scores, where):
        ids, f32 = rs.rank(sc, top_k)
        alone = hx.text_search([q], top_k)[0]
        assert same(alone, ids, f32), f"{name} alone, top_k={top_k}: {alone.passage_ids[:6]} {alone.scores[:6]} vs {ids[:6]} {f32[:6]}"
        assert same(got[i], ids, f32), f"{name} at {i} of the batch, top_k={top_k}: {got[i].passage_ids[:6]} vs {ids[:6]}"
        sizes[name] = ids.size
    # the copies at the slice boundary and in the last document are among the matches; the unknown phrase empties the AND
    assert sizes["63 words and an unknown AND"] == 0 and sizes["63 unknown OR aa"] == min(top_k, CAP) and sizes["256 x aa"] == min(top_k, 3)
    assert {n - 3, n - 1} <= set(scores[0]) and {n - 2, n - 1} <= set(scores[3]) and n - 2 in scores[1] and len(scores[7]) > CAP
    if top_k == 10:                                                         # the small queries around them are not disturbed
        for i, q in enumerate(batch):
            if i not in where:
                if i not in want_small:
                    want_small[i] = rs.search(q, 10)
                assert same(got[i], *want_small[i]), f"query {i} of the batch"


# ---- 2: a first posting list longer than the counting pass's grid -------------------------------------------------------

N_LONG = 140_000


def long_corpus():
    """140 000 documents over a, b, c: "a b" (even) or "a c" (odd); every 1000th + 7 is "a b c", four are "b a" (the tokens
    without the phrase), one carries "a b" 200 times."""
    d = np.arange(N_LONG)
    kind = (d % 2).astype(np.int64)                    # 0 "a b", 1 "a c"
    kind[d % 1000 == 7] = 2                            # "a b c"
    rev = np.array([5, SLICE, 70_001, N_LONG - 1])
    kind[rev] = 3                                      # "b a"
    big = 100_001
    kind[big] = 4                                      # "a b" x 200
    ab, ac, abc = d[kind == 0], d[kind == 1], d[kind == 2]
    z = lambda x: np.zeros(x.size, np.int64)
    one = lambda x: np.ones(x.size, np.int64)
    r200 = np.arange(200)
    a_post = (np.concatenate([ab, ac, abc, rev, np.full(200, big)]), np.concatenate([z(ab), z(ac), z(abc), one(rev), 2 * r200]))
    b_post = (np.concatenate([ab, abc, rev, np.full(200, big)]), np.concatenate([one(ab), one(abc), z(rev), 2 * r200 + 1]))
    c_post = (np.concatenate([ac, abc]), np.concatenate([one(ac), 2 * one(abc)]))
    return index_data(["a", "b", "c"], [a_post, b_post, c_post], N_LONG), rev, big


@pytest.fixture(scope="module")
def long_list():
    data, rev, big = long_corpus()
    a, hx = tiny_index(N_LONG)
    hx.set_text(data)
    rs = R.Restated(data, N_LONG)
    A, B, Cc = 0, 1, 2
    AND, OR = T.NP_TEXT_AND, T.NP_TEXT_OR
    queries = [('"a b"', T.TextQuery.from_phrases([[A, B]], AND)), ('"a c" OR "a b"', T.TextQuery.from_phrases([[A, Cc], [A, B]], OR)),
               ('"a b" AND c', T.TextQuery.from_phrases([[A, B], [Cc]], AND)), ('"b a"', T.TextQuery.from_phrases([[B, A]], AND))]
    scores = [rs.scores(q) for _, q in queries]
    yield data, hx, rs, queries, scores, rev, big
    hx.close()


@pytest.mark.parametrize("top_k", [10, CAP])
def test_a_first_list_longer_than_the_hit_grid(long_list, top_k):
    data, hx, rs, queries, scores, rev, big = long_list
    grid = plan_constant("NP_TEXT_HIT_BLOCKS") * 256
    df_a = len(rs.post[0])
    assert grid == 512 * 256 and df_a > grid, "the counting pass walks the list of a in one stride"
    n_slices = (N_LONG + SLICE - 1) // SLICE
    assert n_slices == 35 and (top_k < CAP or 3 * CAP > WINDOW)            # at the cap every slice after the second refills the window
    # what the corpus was built for: the phrase counts differ from the token counts, and the big document holds 200
    assert rs.phrase_freqs([0, 1])[big] == 200 and all(int(r) not in scores[0] for r in rev)
    assert sorted(scores[3]) == sorted(rev.tolist() + [big])               # ("a b" 200 times holds "b a" 199 times)
    assert len(scores[1]) == N_LONG - rev.size and len(scores[2]) == 140 and len(scores[0]) > 65_536
    got = hx.text_search([q for _, q in queries], top_k)
    for (name, q), sc, r in zip(queries, scores, got):
        ids, f32 = rs.rank(sc, top_k)
        assert same(r, ids, f32), f"{name} top_k={top_k}: {r.passage_ids[:6]} {r.scores[:6]} vs {ids[:6]} {f32[:6]}"
        alone = hx.text_search([q], top_k)[0]
        assert same(alone, ids, f32), f"{name} alone"
    assert got[0].passage_ids.size == top_k and got[3].passage_ids.size == min(top_k, 5)


# ---- 3: ties ------------------------------------------------------------------------------------------------------------------

N_TIES = 3 * SLICE + 5
EXTRA = [SLICE - 1, SLICE, 2 * SLICE]


def ties_data(extra=()):
    """N_TIES documents of the one word w; the documents of `extra` hold it twice."""
    d = np.concatenate([np.arange(N_TIES), np.asarray(extra, np.int64)])
    p = np.concatenate([np.zeros(N_TIES, np.int64), np.ones(len(extra), np.int64)])
    return index_data(["w"], [(d, p)], N_TIES)


def check_ties(hx, label):
    q = T.TextQuery.from_phrases([[0]], T.NP_TEXT_AND)
    subset = np.arange(5, N_TIES, 2)
    # every score equal: the answer is the lowest ids
    data = ties_data()
    hx.set_text(data)
    rs = R.Restated(data, N_TIES)
    sc = rs.scores(q)
    assert len(sc) == N_TIES and len(set(sc.values())) == 1
    for k in (1, 7, CAP - 1, CAP):
        r = hx.text_search([q], k)[0]
        assert r.passage_ids.tolist() == list(range(k)), f"{label} top_k={k}: {r.passage_ids[:8]}"
        assert same(r, *rs.rank(sc, k))
        r = hx.text_search([q], k, subset=subset)[0]
        assert r.passage_ids.tolist() == subset[:k].tolist(), f"{label} top_k={k}, subset: {r.passage_ids[:8]}"
        assert same(r, *rs.rank(sc, k, subset))
    # three documents of three slices rank first with equal scores, every other document ties behind them
    data = ties_data(EXTRA)
    hx.set_text(data)
    rs = R.Restated(data, N_TIES)
    sc = rs.scores(q)
    assert len(set(sc.values())) == 2 and all(sc[d] > sc[0] for d in EXTRA) and len({sc[d] for d in EXTRA}) == 1
    for k in (1, 2, 3, 4, CAP):
        r = hx.text_search([q], k)[0]
        rest = [d for d in range(k) if d not in EXTRA]
        assert r.passage_ids.tolist() == (EXTRA + rest)[:k], f"{label} top_k={k}: {r.passage_ids[:8]}"
        assert same(r, *rs.rank(sc, k))
    batch = hx.text_search([q] * 3, 2, subsets=[None, subset, np.array(EXTRA[1:] + [0, 1])])   # the cut between slices, per query
    assert [r.passage_ids.tolist() for r in batch] == [EXTRA[:2], [EXTRA[0], 5], EXTRA[1:]], label


def test_equal_scores_come_back_by_ascending_id():
    a, hx = tiny_index(N_TIES)
    try:
        check_ties(hx, "default workspace")
    finally:
        hx.close()


def test_equal_scores_with_a_small_workspace():
    """100 kB hold one query over three of the four slices at top_k = 1024 (tests/test_gpu_text.py): the best-so-far list is
    carried across two chunks of slices and must tie the same way."""
    a, hx = tiny_index(N_TIES, workspace_bytes=100_000)
    try:
        check_ties(hx, "workspace of 100 kB")
    finally:
        hx.close()


# ---- 4: fusion --------------------------------------------------------------------------------------------------------------

def fusion_cases():
    inf = float("inf")
    desc = lambda n, top: (top - np.arange(n) * 0.25).astype(np.float32).tolist()
    sem, kw = list(range(0, 2 * CAP, 2)), list(range(1, 2 * CAP, 2))       # interleaved ids, disjoint
    far = list(range(50_000, 50_000 + CAP))
    hi_a, hi_b = [(1 << 62) - CAP + i for i in range(CAP)], [(1 << 62) + 3 * i for i in range(CAP)]
    cases = [("full window", sem, desc(CAP, 900.0), kw, desc(CAP, 300.0)),
             ("small", [5, 3, 8], [9.0, 4.0, 1.0], [3, 11], [7.0, 6.5]),
             ("full window, equal scores", sem, [2.5] * CAP, kw, [0.125] * CAP),
             ("negative", [4, 9, 2, 7], [-1.0, -2.5, -2.5, -80.0], [7, 1, 4], [-0.5, -3.0, -3.0]),
             ("full window, ids near 2^62", hi_a, desc(CAP, 10.0), hi_b, desc(CAP, 500.0)),
             ("zeros", [1, 2, 3, 4], [0.0, -0.0, 0.0, -0.0], [4, 5, 6], [-0.0, 0.0, -1.0]),
             ("full window, far lists", far, desc(CAP, 1.0), kw, [1.0] * CAP),
             ("+inf", [1, 2, 3], [inf, 2.0, 1.0], [3, 4, 5], [inf, inf, -4.0]),
             ("-inf", [1, 2, 3], [3.0, 2.0, -inf], [9, 2, 8], [1.0, -inf, -inf]),
             ("both inf", [6, 5, 4], [inf, 0.0, -inf], [4, 5], [-1.0, -2.0]),
             ("empty", [], [], [], []),
             ("half window", sem[:CAP // 2], desc(CAP // 2, 7.0), sem[:CAP // 2][::-1], desc(CAP // 2, -7.0))]
    return cases


@pytest.mark.parametrize("mode,alpha", [("rrf", 0.75), ("rrf", 0.5), ("relative_score", 0.75), ("relative_score", 0.5)])
def test_fusion_fills_the_whole_window(mode, alpha):
    cases = fusion_cases()
    full = [c for c in cases if c[0].startswith("full window")]
    assert len(full) == 4 and all(len(c[1]) == CAP and len(c[3]) == CAP and len(set(c[1]) | set(c[3])) == WINDOW for c in full)
    assert [c[0].startswith("full window") for c in cases[:7]] == [True, False] * 3 + [True]      # mixed order in the batch
    a, hx = tiny_index(8)
    try:
        for top_k in (WINDOW, WINDOW - 1):
            got = npa.fuse(mode, alpha, top_k, [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases],
                           index=hx)
            for c, (ids, sc) in zip(cases, got):
                w_ids, w_sc = R.fuse(mode, alpha, top_k, *c[1:])
                assert np.array_equal(ids, w_ids), f"{mode} {alpha} top_k={top_k} {c[0]}: {ids[:6]} vs {w_ids[:6]}"
                bad = np.nonzero(sc.view(np.uint32) != w_sc.view(np.uint32))[0]
                assert bad.size == 0, f"{mode} {alpha} top_k={top_k} {c[0]}: at {bad[:4]}: {sc[bad[:4]]} vs {w_sc[bad[:4]]} " \
                                      f"({sc.view(np.uint32)[bad[:4]]} vs {w_sc.view(np.uint32)[bad[:4]]})"
                if c[0].startswith("full window"):
                    assert ids.size == top_k
            if mode == "relative_score" and alpha == 0.5:                    # every fused score equal: the window in id order
                ids, sc = got[2]
                assert ids.tolist() == list(range(top_k)) and np.unique(sc).size == 1
    finally:
        hx.close()
