"""The C oracle's tie rules are the reference's (no GPU needed).

On the dyadic corpora of tie_corpus.py every value before the exact stage is exact, so the oracle's stage traces must
equal a brute-force float64 restatement written from search.rs (ties_restate.py) bit for bit: probed cells (dense
per-token cut with the lowest ids taken at ties; batched slab heaps with the strict push rule and the threshold over
pushed pairs only), the candidate union, the approximate scores and the S5 selection (stable over ascending ids).  The
final order must be the stable S7 sort of the selection by exact score.  The GPU tie tests trust the oracle there.
"""
import numpy as np
import pytest

import ties_restate as R
import tie_corpus as TC
from helpers import O, oracle_index

N = 3000
GROUPS = [[7, 8, 1500, 2999], [100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111] + list(range(2000, 2040))]
PAIR = (40, 2600, 41, 2601)


@pytest.fixture(scope="module")
def corpus():
    a = TC.build(K=512, N=N, seed=11, dup_centroids=[(9, 10), (9, 40), (9, 300), (77, 200), (100, 101)],
                 dup_docs=GROUPS, pair=PAIR)
    return a, oracle_index(a)


def _check(a, ox, q, n_probe, nfs, top_k, thr, cbs=100_000, subset=None, what=""):
    p = O.SearchParameters(n_full_scores=nfs, top_k=top_k, n_ivf_probe=n_probe, centroid_batch_size=cbs,
                           centroid_score_threshold=thr)
    r = ox.search(q, p, subset, trace=True)
    t = r.trace
    cells, cand, approx, sel = R.search(a, q, n_probe, nfs, top_k, thr, cbs, subset)
    assert np.array_equal(t.cells, cells), f"{what}: cells {np.setxor1d(t.cells, cells)[:10]}"
    assert np.array_equal(t.cand, cand), f"{what}: candidates"
    assert np.array_equal(t.approx.view(np.uint32), approx.view(np.uint32)), f"{what}: approximate scores"
    assert np.array_equal(t.sel, sel), f"{what}: S5 selection"
    assert np.array_equal(r.passage_ids, R.final_order(t.sel, t.sel_exact, top_k)), f"{what}: S7 order"
    return r


def _queries(a):
    qs = TC.queries(a, 6, 8, seed=3) + TC.queries(a, 2, 32, seed=4)
    z = qs[0].copy()
    z[2] = 0.0                 # an all-zero token: QC row of +0.0, ties across all K
    n = qs[1].copy()
    n[5] = np.nan              # a NaN token: every score non-finite, ties across all K
    return qs + [z, n]


@pytest.mark.parametrize("thr", [None, 3.0])
@pytest.mark.parametrize("n_probe", [1, 3, 8, 40])
def test_dense_probe_ties_match_restatement(corpus, n_probe, thr):
    """Scores take a few hundred values over 512 centroids: ties straddle the per-token cut at every n_probe, and the
    duplicate centroids 9 = 10 = 40 = 300 sit in one 32-group, across groups and far apart."""
    a, ox = corpus
    for i, q in enumerate(_queries(a)):
        _check(a, ox, q, n_probe, 64, 10, thr, what=f"dense np={n_probe} thr={thr} q{i}")


@pytest.mark.parametrize("thr", [None, 3.0])
@pytest.mark.parametrize("cbs,n_probe", [(100, 2), (64, 5), (300, 3)])
def test_batched_probe_ties_match_restatement(corpus, cbs, n_probe, thr):
    a, ox = corpus
    for i, q in enumerate(_queries(a)[:4] + _queries(a)[-2:]):
        r = _check(a, ox, q, n_probe, 64, 10, thr, cbs=cbs, what=f"batched cbs={cbs} np={n_probe} thr={thr} q{i}")
        assert r.trace.used_batched


def test_batched_threshold_ignores_unpushed_tied_pair():
    """A tied centroid that a token did not take is not in its slab heap (search.rs:177-199): c2 ties c1 at token
    e0's cut (>= t_cs) but b and c1 come first in its slab, so only token e1's sub-threshold score counts for it."""
    a, q = TC.threshold_scenario()
    ox = oracle_index(a)
    r = _check(a, ox, q, 2, 64, 10, 0.25, cbs=100, what="threshold scenario")
    assert 10 in r.trace.cells and 20 in r.trace.cells and 30 not in r.trace.cells
    # the dense path keeps it: its threshold takes the max over every token
    rd = _check(a, ox, q, 2, 64, 10, 0.25, what="threshold scenario, dense")
    assert {10, 20, 30} <= set(rd.trace.cells.tolist())


def test_selection_cut_inside_a_duplicate_group(corpus):
    """52 byte-identical documents (ids 100-111, 2000-2039) share every score; the n_sel cut falls inside the group and
    keeps its lowest ids, in ascending order."""
    a, ox = corpus
    g = np.array(GROUPS[1])
    off = np.concatenate([[0], np.cumsum(a["doc_lengths"])])
    toks = a["codes"][off[g[0]]: off[g[0] + 1]]
    q = a["centroids"][toks]                          # a query made of the group's own tokens
    for nfs, top_k in ((40, 10), (160, 30), (400, 60)):
        r = _check(a, ox, q, 2, nfs, top_k, None, what=f"group cut nfs={nfs}")
        sel = r.trace.sel
        got = sel[np.isin(sel, g)]
        assert got.size and np.array_equal(got, g[: got.size]), f"nfs={nfs}: {got}"
        res = r.passage_ids[np.isin(r.passage_ids, g)]
        assert np.array_equal(res, g[: res.size])


def test_equal_exact_scores_keep_approximate_rank(corpus):
    """The constructed pair: exact(A) == exact(B), approx(B) > approx(A), id(B) > id(A).  S7 is a stable sort of the
    S5 order (search.rs:496), so B comes first -- an (exact, id) order would put A first."""
    a, ox = corpus
    P = a["pair"]
    q1, q2 = TC.pair_queries(a["centroids"].shape[1])
    r = _check(a, ox, q1, 2, 64, 4, None, what="pair, one token")
    assert sorted(r.trace.cand.tolist()) == sorted([P["A1"], P["B1"], P["A2"], P["B2"]])
    ex = dict(zip(r.trace.sel.tolist(), r.trace.sel_exact.tolist()))
    assert ex[P["A1"]] == ex[P["B1"]] == ex[P["A2"]] == ex[P["B2"]]
    assert r.passage_ids.tolist() == [P["B1"], P["B2"], P["A1"], P["A2"]]
    r = _check(a, ox, q2, 2, 64, 4, None, what="pair, two tokens")
    ex = dict(zip(r.trace.sel.tolist(), r.trace.sel_exact.tolist()))
    assert ex[P["A2"]] == ex[P["B2"]]
    ids = r.passage_ids.tolist()
    assert ids.index(P["B2"]) < ids.index(P["A2"])


def test_subset_with_ties(corpus):
    a, ox = corpus
    sub = np.concatenate([np.arange(0, N, 3), GROUPS[1]]).astype(np.int64)
    for i, q in enumerate(_queries(a)[:3]):
        for n_probe in (2, 40):
            _check(a, ox, q, n_probe, 64, 10, None, subset=sub, what=f"subset np={n_probe} q{i}")
