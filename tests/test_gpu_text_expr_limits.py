"""Tree keyword queries at the kernels' own constants: runs longer than the counting grid (the second grid stride of
text_prefix_kernel and text_hit_kernel<true>), 64 frequency arrays per query in uneven batches cut into chunks of queries
(px_at, the skipped pre-pass, text_plan halving a chunk for per_query_extra), text_expr_kernel's own sort with 4096 equal
scores in a slice and ties carried across chunks of slices, and more than 65 535 counted phrases and prefix entries (the
`i0 += 65535` loops around text_hit_kernel<false>, <true> and text_prefix_kernel).  Needs a real MI355X.

The reference is tests/text_expr_restate.py: ids equal and f32 scores equal as uint32, without exception.  The corpora and
trees come from tests/text_limit_shapes.py; tests/test_text_expr_limits_cpu.py pins the restatement to SQLite on the same
generators at a reduced size."""
import numpy as np
import pytest

import text_limit_shapes as S
from text_limit_shapes import CAP, SLICE, plan_constant, same, same_rows
from helpers import hip_index

from next_plaid_amd import text as T
import text_restate as R
import text_expr_restate as X

pytestmark = pytest.mark.gpu


def test_the_constants_are_the_plans():
    assert plan_constant("NP_TEXT_SLICE_DOCS") == SLICE and T.NP_TEXT_MAX_PHRASES == 64 and CAP == 1024


# ---- A1: runs longer than the counting grid -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def long_run():
    grid = plan_constant("NP_TEXT_HIT_BLOCKS") * 256
    n = S.long_run_size(grid)
    data, rev, big = S.long_run_corpus(n)
    rs = S.CachedExpr(data, n)
    # everything the corpus was built for holds on the restatement, before any device call
    postings, holders = S.check_long_run(data, rs, rev, big, grid)
    named = S.long_run_trees()
    exprs = [X.tree_expr(t, data) for _, t in named]
    scores = [rs.expr_scores(q) for q in exprs]
    assert len(exprs) == 7 and all(len(set(sc.values())) >= 30 for sc in scores), [len(set(sc.values())) for sc in scores]
    assert [S.n_arrays(q) for q in exprs] == [1, 0, 2, 1, 2, 1, 1]
    subsets = S.long_run_subsets(data, grid, len(exprs))
    a, hx = S.tiny_index(n)
    hx.set_text(data)
    yield grid, n, data, hx, rs, named, exprs, scores, subsets, postings
    hx.close()


@pytest.mark.parametrize("top_k", [10, CAP])
def test_runs_longer_than_the_counting_grid(long_run, top_k):
    """The run of p* holds more postings than one stride of text_prefix_kernel's grid covers, the list of "h" more than one
    of text_hit_kernel<true>'s.  The documents of "pz" have all their postings of the run behind the first stride: without
    the second one they are no match and nHit, so every score, changes; under the subsets the ranking is made of documents
    from both sides of the stride."""
    grid, n, data, hx, rs, named, exprs, scores, subsets, postings = long_run
    assert grid == plan_constant("NP_TEXT_HIT_BLOCKS") * 256 and postings > grid and n > grid
    batch = hx.text_search(exprs, top_k)
    scoped = hx.text_search(exprs, top_k, subsets=subsets)
    for i, ((name, _), q, sc) in enumerate(zip(named, exprs, scores)):
        ids, f32 = rs.rank(sc, top_k)
        assert ids.size == top_k
        assert same(batch[i], ids, f32), f"{name} top_k={top_k}: {batch[i].passage_ids[:6]} {batch[i].scores[:6]} vs {ids[:6]} {f32[:6]}"
        assert same(hx.text_search([q], top_k)[0], ids, f32), f"{name} alone, top_k={top_k}"
        ids, f32 = rs.rank(sc, top_k, subsets[i])
        assert ids.size == top_k or (top_k == CAP and ids.size > 300)
        assert same(scoped[i], ids, f32), f"{name} under its subset, top_k={top_k}: {scoped[i].passage_ids[:6]} vs {ids[:6]}"
        assert same(hx.text_search([q], top_k, subset=subsets[i])[0], ids, f32), f"{name} alone under its subset, top_k={top_k}"
    if top_k == CAP:   # what the second stride contributes is in the answer: documents of "pz" under the bare prefix
        o = data.term_offsets
        pz = data.inst_doc[o[data.vocab["pz"]]: o[data.vocab["pz"] + 1]]
        assert np.isin(scoped[0].passage_ids, pz).sum() >= 32 and (scoped[1].passage_ids >= grid).sum() > 50
        hx.text_search(exprs[:1], top_k)
        assert hx.last_stats["n_ivf_ids"] == postings                 # the pre-pass walked the run once


# ---- A2: sixty-four frequency arrays, uneven batches, chunks of queries -------------------------------------------------------

N_FAM = SLICE + 1


@pytest.fixture(scope="module")
def families():
    data = S.families_corpus(N_FAM)
    rs = S.CachedExpr(data, N_FAM)
    exprs = {name: X.tree_expr(t, data) for name, t in S.families_trees().items()}
    scores = {name: rs.expr_scores(q) for name, q in exprs.items()}
    return data, rs, exprs, scores, S.tiny_arrays(N_FAM)


def halving_budget():
    """A query of the batch owns 64 arrays of 4160 entries (4097 documents rounded up to 64): per_query_extra = 64 * 4160 * 4
    = 1 064 960 bytes, and with the best-so-far list of top_k = 10 (256 + 256 + 8) a query costs 1 065 480 bytes.  A budget of
    five such queries cannot hold the eight of the batch (left < 0), so text_plan halves to four: 5 - 4 = one query's bytes
    are left for the fixed part and the 2 * 4 slice lists of 124 bytes.  The fixed part (results, programs, 5 kB) is not
    visible here; the plan is evaluated with 0 and with 64 kB for it."""
    pq = S.per_query_bytes(N_FAM, 10, False, 64)
    assert pq == 1_065_480
    budget = 5 * pq
    for fixed in (0, 65536):
        assert S.restated_plan(budget, fixed, pq, S.n_slices_of(N_FAM), 8, 64, 10) == (4, 2)
        assert S.restated_plan(budget, fixed, pq, S.n_slices_of(N_FAM), 4, 64, 10) == (4, 2)
    return budget


def test_64_frequency_arrays_in_uneven_batches_and_chunks_of_queries(families):
    """One batch whose queries own [64, 0, 1, 0, 0, 0, 3, 64] arrays (the zeros are flat queries sent as trees), and the four
    shapes of 64 phrases, on a default handle, under max_batch = 3 (chunks {0,1,2}, {3,4,5}, {6,7}: the middle one has no prefix
    phrase, its pre-pass is skipped and the arrays keep the first chunk's counts; the last has 3 and 64 arrays at places 0 and
    1), under max_batch = 1, and under halving_budget()."""
    data, rs, exprs, scores, a = families
    uneven, shapes = [exprs[k] for k in S.UNEVEN], [exprs[k] for k in S.SHAPES_64]
    assert [S.n_arrays(q) for q in uneven] == S.UNEVEN_ARRAYS and [S.n_arrays(q) for q in shapes] == [64, 64, 32, 33]
    assert all(q.n_phrases == 64 for q in shapes[:3]) and shapes[3].n_phrases == 33
    assert sorted(scores["AND of 64 prefixes"]) == [17, N_FAM - 1] and len(scores["OR of 64 prefixes"]) == N_FAM
    budget = halving_budget()
    want = {}
    for k in (10, CAP):
        for name in set(S.UNEVEN + S.SHAPES_64):
            want[(name, k)] = rs.rank(scores[name], k)
    default = {}
    for label, opts, ks in (("default", {}, (10, CAP)), ("max_batch=3", {"max_batch": 3}, (10, CAP)), ("max_batch=1", {"max_batch": 1}, (10,)),
                            ("workspace", {"workspace_bytes": budget}, (10,))):
        hx = hip_index(a, **opts)
        try:
            hx.set_text(data)
            if label == "workspace":
                assert hx.workspace_bytes() == budget
            for k in ks:
                for tag, names, qs in (("uneven", S.UNEVEN, uneven), ("shapes", S.SHAPES_64, shapes)):
                    got = hx.text_search(qs, k)
                    for i, (name, r) in enumerate(zip(names, got)):
                        ids, f32 = want[(name, k)]
                        assert same(r, ids, f32), f"{label}, top_k={k}, {tag} batch, query {i} ({name}): {r.passage_ids[:6]} {r.scores[:6]} vs {ids[:6]} {f32[:6]}"
                    if label == "default":
                        default[(tag, k)] = got
                        for i, q in enumerate(qs):
                            assert same_rows(hx.text_search([q], k), [got[i]]), f"top_k={k}, {tag} batch, query {i} alone"
                    else:
                        assert same_rows(got, default[(tag, k)]), f"{label}, top_k={k}, {tag} batch: not the default handle's bytes"
        finally:
            hx.close()
    assert default[("uneven", CAP)][0].passage_ids.size == CAP and sorted(default[("uneven", 10)][7].passage_ids.tolist()) == [17, N_FAM - 1]


# ---- A3: ties through the tree kernel -----------------------------------------------------------------------------------------

N_TIES = 3 * SLICE + 5
EXTRA = [SLICE - 1, SLICE, 2 * SLICE]


def carry_budget(slots, subset_size):
    """A workspace under which ONE query at top_k = 1024 runs over fewer than the four slices at a time, so that the
    best-so-far list is carried across chunks of slices.  text_plan halves the queries before it cuts the slices: only a
    single query gets 1 <= slices < n_slices, and then
        slices = (budget - fixed - per_query) / 12 292                        (a slice's list of 1024: 1024 * 12 + 4 bytes)
    with per_query = 8192 + 4096 + 8 (the best-so-far list) + 1792 under a subset (12 293 bits) + 49 408 for each frequency
    array (w* owns one: 12 352 entries).  The window of three slices is 36 876 bytes wide, so the fixed part has to be known
    better than to 64 kB.  It is   results + staged subset + programs + 5120:   the results of one query are 8192 + 4096 + 256
    bytes, a staged subset of m ids is up256(8 m) + 256 + 256, and the programs of a one-query batch of at most three phrases
    are fifteen regions of 256 bytes (3840); they are bracketed here by 0 and 16 kB.  The budget holds one slice at the upper
    bound; at the lower one it holds two.  Returns (the budget, a budget one byte short of one slice at the LOWER bound:
    the call must be refused under it, which shows that the bracket's lower end is not above the library's fixed part, as the
    call's success under the budget shows for the upper end)."""
    pq = S.per_query_bytes(N_TIES, CAP, subset_size > 0, slots)
    assert pq == 12_296 + (1792 if subset_size else 0) + 49_408 * slots and S.pair_bytes(CAP) == 12_292
    lo = S.result_bytes(1, CAP) + 5120 + (S.subset_stage_bytes(1, 1, subset_size) if subset_size else 0)
    hi = lo + 16_384
    budget = hi + pq + S.pair_bytes(CAP)
    n_slices = S.n_slices_of(N_TIES)
    for fixed in (lo, hi):
        for k in (CAP - 1, CAP):
            queries, slices = S.restated_plan(budget, fixed, pq, n_slices, 1, 64, k)
            assert n_slices == 4 and queries == 1 and 1 <= slices < n_slices
    assert S.restated_plan(lo + pq + S.pair_bytes(CAP) - 1, lo, pq, n_slices, 1, 64, CAP) is None
    return budget, lo + pq + S.pair_bytes(CAP) - 1


class Handles:
    """search(query, k, subset): on the default handle, or (carried) on the handle whose workspace carries the best-so-far
    list for a query with that many frequency arrays and that subset."""

    def __init__(self, a, carried, subset):
        self.a, self.carried, self.subset_size, self.open, self.data = a, carried, int(subset.size), {}, None

    def set_text(self, data):
        self.data = data
        for hx in self.open.values():
            hx.set_text(data)

    def search(self, q, k, subset=None):
        key = (S.n_arrays(q), subset is not None) if self.carried else None
        if key not in self.open:
            opts = {"workspace_bytes": carry_budget(key[0], self.subset_size if key[1] else 0)[0]} if self.carried else {}
            self.open[key] = hip_index(self.a, **opts)
            self.open[key].set_text(self.data)
        return self.open[key].text_search([q], k, subset=subset)[0]

    def close(self):
        for hx in self.open.values():
            hx.close()


def check_tree_ties(hs, label):
    subset = np.arange(5, N_TIES, 2)
    named = S.ties_trees()
    # every score equal: the answer is the lowest ids
    data = S.ties_corpus(N_TIES)
    hs.set_text(data)
    rs = S.CachedExpr(data, N_TIES)
    assert data.terms == ["w"]
    for name, tree in named:
        q = X.tree_expr(tree, data)
        sc = rs.expr_scores(q)
        assert len(sc) == N_TIES and len(set(sc.values())) == 1, name
        for k in (1, 7, CAP - 1, CAP):
            r = hs.search(q, k)
            assert r.passage_ids.tolist() == list(range(k)), f"{label}, {name}, top_k={k}: {r.passage_ids[:8]}"
            assert same(r, *rs.rank(sc, k))
            r = hs.search(q, k, subset)
            assert r.passage_ids.tolist() == subset[:k].tolist(), f"{label}, {name}, top_k={k}, subset: {r.passage_ids[:8]}"
            assert same(r, *rs.rank(sc, k, subset))
    # three documents of three slices tie with one another, every other document ties with every other.  The three hold wx as
    # well: under w* they hold two instances of the range and rank FIRST; under the trees that count w alone they are only
    # longer (two tokens, one w) and bm25 ranks them LAST -- the restatement says which, SQLite says the same
    # (tests/test_text_expr_limits_cpu.py), and either way the cut runs through a tie
    data = S.ties_corpus(N_TIES, EXTRA)
    hs.set_text(data)
    rs = S.CachedExpr(data, N_TIES)
    assert data.terms == ["w", "wx"]
    others = [d for d in range(2 * CAP) if d not in EXTRA]
    ends = np.array(EXTRA + [0, 1, SLICE + 1, N_TIES - 1])
    firsts = []
    for name, tree in named:
        q = X.tree_expr(tree, data)
        sc = rs.expr_scores(q)
        assert len(sc) == N_TIES and len(set(sc.values())) == 2 and len({sc[d] for d in EXTRA}) == 1 and sc[0] == sc[N_TIES - 1], name
        first = sc[EXTRA[0]] > sc[0]
        firsts.append(first)
        for k in (1, 2, 3, 4, CAP):
            r = hs.search(q, k)
            assert r.passage_ids.tolist() == ((EXTRA + others) if first else others)[:k], f"{label}, {name}, top_k={k}: {r.passage_ids[:8]}"
            assert same(r, *rs.rank(sc, k))
        for k in (2, 5, ends.size):
            r = hs.search(q, k, ends)
            rest = sorted(set(ends.tolist()) - set(EXTRA))
            assert r.passage_ids.tolist() == ((EXTRA + rest) if first else (rest + EXTRA))[:k], f"{label}, {name}, top_k={k}, subset: {r.passage_ids}"
            assert same(r, *rs.rank(sc, k, ends))
    assert firsts == [True, False, False, False]


def test_equal_scores_through_the_tree_kernel():
    hs = Handles(S.tiny_arrays(N_TIES), False, np.arange(5, N_TIES, 2))
    try:
        check_tree_ties(hs, "default workspace")
        data = hs.data                                          # the cut between slices, per query of one batch
        rs = S.CachedExpr(data, N_TIES)
        q = X.tree_expr(S.ties_trees()[0][1], data)
        subs = [None, np.arange(5, N_TIES, 2), np.array(EXTRA[1:] + [0, 1])]
        batch = hs.open[None].text_search([q] * 3, 2, subsets=subs)
        assert [r.passage_ids.tolist() for r in batch] == [EXTRA[:2], [EXTRA[0], 5], EXTRA[1:]]
        assert all(same(r, *rs.expr_search(q, 2, s)) for r, s in zip(batch, subs))
    finally:
        hs.close()


def test_equal_scores_through_the_tree_kernel_carried_across_chunks_of_slices():
    """carry_budget(): every single query runs on a handle whose workspace holds one or two of its four slices at top_k =
    1023 and 1024, so the best-so-far list is merged with two to four chunks of slices and must tie the same way."""
    subset = np.arange(5, N_TIES, 2)
    for slots in (0, 1):
        for m in (0, int(subset.size)):
            assert carry_budget(slots, m)[0] < 200_000
    a = S.tiny_arrays(N_TIES)
    hs = Handles(a, True, subset)
    try:
        check_tree_ties(hs, "carried")
        assert sorted(hs.open) == [(0, False), (0, True), (1, False), (1, True)]
        for (slots, scoped), hx in sorted(hs.open.items()):          # the bracket of the fixed part holds on the library itself
            budget, short = carry_budget(slots, int(subset.size) if scoped else 0)
            assert hx.workspace_bytes() == budget
            tight = hip_index(a, workspace_bytes=short)
            try:
                tight.set_text(hs.data)
                q = X.tree_expr(S.ties_trees()[0 if slots else 1][1], hs.data)
                assert S.n_arrays(q) == slots
                with pytest.raises(MemoryError, match="workspace budget"):
                    tight.text_search([q], CAP, subset=subset if scoped else None)
            finally:
                tight.close()
    finally:
        hs.close()


# ---- A4: more than 65 535 grid entries ----------------------------------------------------------------------------------------

B_WIDE = 1100
PER_QUERY = 60


def interleave(a, b):
    assert len(a) == len(b)
    return [x for pair in zip(a, b) for x in pair]


def or_chain(leaves):
    t = leaves[0]
    for x in leaves[1:]:
        t = ("or", t, x)
    return t


def wide_phrases():
    """Three distinct lists of 60 two-word phrases over limit_texts(): neighbours in a list stand in different numbers of
    documents (a pair of the 64 words in order: four or five; "zz fillN": one; ...)."""
    lw = R.LIMIT_WORDS
    fwd = [(lw[i], lw[i + 1]) for i in range(63)]
    back = [(lw[i + 1], lw[i]) for i in range(63)]
    zz = [("zz", f"fill{i}") for i in range(27)]
    q0 = interleave(fwd[:30], zz + [("aa", "bb"), ("bb", "aa"), ("aa", "aa")])
    q1 = interleave(fwd[30:60], [(f"fill{3 * i}", "aa") for i in range(9)] + back[:21])
    q2 = interleave(back[21:51], fwd[33:63])
    return [q0, q1, q2]


def wide_prefixes():
    """Three distinct lists of 60 single-word prefixes over limit_texts()."""
    lw = R.LIMIT_WORDS
    fills = [f"fill{i}" for i in range(27)]
    q0 = interleave(lw[:30], fills + ["aa", "bb", "zz"])
    q1 = interleave(lw[30:60], [f"lw{i}" for i in range(6)] + ["fill1", "fill2", "f", "a", "b", "z", "l", "lw", "fi", "zz", "aa", "bb"] + fills[3:15])
    q2 = interleave(fills + ["aa", "bb", "zz"], lw[34:64])
    return [q0, q1, q2]


@pytest.fixture(scope="module")
def wide():
    n = 40
    data = T.TextIndexData.from_texts(R.limit_texts(n))
    return n, data, S.CachedExpr(data, n), S.tiny_arrays(n)


def entry_65535(lists):
    """The (list, place) of the entries 65 534 and 65 535 of a batch that cycles through `lists`: the last one of the first
    launch and the first one of the second."""
    out = []
    for e in (65534, 65535):
        out.append(((e // PER_QUERY) % len(lists), e % PER_QUERY))
    return out


def test_more_than_65535_counted_phrases_in_a_call(wide):
    """1100 queries of 60 two-word phrases are 66 000 counted phrases: text_hit_kernel<false> (flat) and text_hit_kernel<true>
    (trees; with a prefix range at every phrase's end) take them as a grid dimension in two launches, the second one offset
    by 65 535 in item_phr and nhit.  The phrases on the two sides of that place have different nHit."""
    n, data, rs, a = wide
    v = data.vocab
    lists = wide_phrases()
    assert len({tuple(l) for l in lists}) == 3 and all(len(l) == PER_QUERY for l in lists)
    ids_of = [[[v[x], v[y]] for x, y in l] for l in lists]             # (every word is known: every phrase is counted)
    assert B_WIDE * PER_QUERY == 66_000 > 65_535
    (la, pa), (lb, pb) = entry_65535(lists)
    hit_a, hit_b = len(rs.phrase_freqs(ids_of[la][pa])), len(rs.phrase_freqs(ids_of[lb][pb]))
    assert (la, pa, lb, pb) == (0, 14, 0, 15) and hit_a != hit_b and hit_a > 0 and hit_b > 0, (hit_a, hit_b)
    flat = [T.TextQuery.from_phrases(p, T.NP_TEXT_OR) for p in ids_of]
    trees = [T.TextExpr.from_query(q) for q in flat]
    ranged = [T.TextExpr.from_tree(or_chain([("phrase", p, T.prefix_range(w[1], data)) for p, w in zip(ps, l)]))
              for ps, l in zip(ids_of, lists)]
    assert all(S.n_arrays(q) == 0 and q.prefix_hi().all() for q in ranged) and any(r[1] - r[0] > 1 for q in ranged for r in q.prefix)
    hit_a = rs.expr_phrase_freqs(ranged[la].phrases()[pa], ranged[la].prefix[pa])[1]
    hit_b = rs.expr_phrase_freqs(ranged[lb].phrases()[pb], ranged[lb].prefix[pb])[1]
    assert hit_a != hit_b and hit_a > 0 and hit_b > 0
    want_flat = [rs.search(q, 10) for q in flat]
    want_tree = [rs.expr_search(q, 10) for q in trees]
    want_ranged = [rs.expr_search(q, 10) for q in ranged]
    assert all(w[0].size >= 5 for w in want_flat + want_ranged) and len({w[1].tobytes() for w in want_flat}) == 3
    hx = hip_index(a)
    try:
        hx.set_text(data)
        got_flat = hx.text_search([flat[i % 3] for i in range(B_WIDE)], 10)
        got_tree = hx.text_search([trees[i % 3] for i in range(B_WIDE)], 10)
        got_ranged = hx.text_search([ranged[i % 3] for i in range(B_WIDE)], 10)
    finally:
        hx.close()
    assert len(got_flat) == len(got_tree) == len(got_ranged) == B_WIDE
    for i in range(B_WIDE):
        assert same(got_flat[i], *want_flat[i % 3]), f"flat, query {i}"
        assert same(got_tree[i], *want_tree[i % 3]) and same(got_tree[i], got_flat[i].passage_ids, got_flat[i].scores), f"trees, query {i}"
        assert same(got_ranged[i], *want_ranged[i % 3]), f"prefix ranges, query {i}"


def test_more_than_65535_prefix_entries_in_a_chunk(wide):
    """max_batch = 2048 leaves the 1100 queries in one chunk: 66 000 single-token prefix phrases, which text_prefix_kernel
    takes as a grid dimension in two launches, the second one offset by 65 535 in px_phr and px_at.  A query owns 60 arrays
    of 64 entries: 15 360 bytes, 17 MB for the chunk."""
    n, data, rs, a = wide
    lists = wide_prefixes()
    assert len({tuple(l) for l in lists}) == 3 and all(len(l) == PER_QUERY for l in lists)
    exprs = [T.TextExpr.from_tree(or_chain([("phrase", [0], T.prefix_range(w, data)) for w in l])) for l in lists]
    assert all(S.n_arrays(q) == PER_QUERY for q in exprs) and B_WIDE * PER_QUERY == 66_000 > 65_535
    (la, pa), (lb, pb) = entry_65535(lists)
    fa, hit_a = rs.expr_phrase_freqs(exprs[la].phrases()[pa], exprs[la].prefix[pa])
    fb, hit_b = rs.expr_phrase_freqs(exprs[lb].phrases()[pb], exprs[lb].prefix[pb])
    assert (la, pa, lb, pb) == (0, 14, 0, 15) and hit_a != hit_b and hit_a > 0 and hit_b > 0 and fa != fb, (hit_a, hit_b)
    want = [rs.expr_search(q, 10) for q in exprs]
    assert all(w[0].size >= 5 for w in want) and len({w[1].tobytes() for w in want}) == 3
    pq = S.per_query_bytes(n, 10, False, PER_QUERY)
    assert pq == 520 + 15_360
    hx = hip_index(a, max_batch=2048)
    try:
        hx.set_text(data)
        for fixed in (0, 1 << 26):   # (the programs of 66 000 phrases and the results are a few MB)
            assert S.restated_plan(hx.workspace_bytes(), fixed, pq, 1, B_WIDE, 2048, 10) == (B_WIDE, 1)
        got = hx.text_search([exprs[i % 3] for i in range(B_WIDE)], 10)
        alone = hx.text_search(exprs, 10)
    finally:
        hx.close()
    assert len(got) == B_WIDE
    for i in range(B_WIDE):
        assert same(got[i], *want[i % 3]), f"query {i}: {got[i].passage_ids} {got[i].scores} vs {want[i % 3]}"
    assert same_rows(alone, got[:3])
