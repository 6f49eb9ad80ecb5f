"""Exact ties and probes wider than 64 cells through the HIP search path.  Needs a real MI355X.

The corpora (tie_corpus.py) are dyadic: every value before the exact stage is exact, so the HIP stage traces must equal
the oracle's bit for bit even where scores tie -- and the oracle's tie rules are checked against the reference's in
test_ties_oracle_cpu.py.  Ties: the probe cut takes the lowest centroid ids, S5 keeps ascending ids among equal
approximate scores, S7 keeps the S5 order among equal exact scores ("Ties").
"""
import numpy as np
import pytest

import tie_corpus as TC
from helpers import (RTOL_BF16, RTOL_BF16_PLAIN, RTOL_F32, assert_ranking_close, assert_ties_strict, hip_index,
                     oracle_index, to_oracle_params)

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu

N = 40000
# byte-identical document groups: across the 32768-document range boundary, across shard boundaries (G = 2, 3) and one
# larger than the selection windows below, so that a cut falls inside it
GROUPS = [[5, 13332, 13334, 20000, 20001, 32750, 32790, 39999],
          list(range(300, 340)) + list(range(26660, 26700)) + list(range(32760, 32780))]
PAIR = (1000, 33000, 1001, 33001)
# duplicate centroids: inside one 32-group (9, 10), across groups (9 -> 40, 3000), across centroid_batch_size = 1000
# slabs (77 -> 1077, 2077)
DUP_CEN = [(9, 10), (9, 40), (9, 3000), (77, 1077), (77, 2077), (500, 501)]


def P(**kw):
    return npa.SearchParameters(**kw)


def rtol_of(prec):
    return RTOL_F32 if prec in (0, 2) else (RTOL_BF16 if prec == 1 else RTOL_BF16_PLAIN)


def check_trace(hx, ox, q, p, subset=None, what=""):
    tr = hx.debug_trace(q, p, subset)
    r = ox.search(q, to_oracle_params(p), subset, trace=True)
    t = r.trace
    assert np.array_equal(tr["cells"], t.cells), f"{what}: S2 cells differ: {np.setxor1d(tr['cells'], t.cells)[:16]}"
    assert np.array_equal(tr["cand"], t.cand), f"{what}: S3 candidates differ ({tr['cand'].size} vs {t.cand.size})"
    bad = np.nonzero(tr["approx"].view(np.uint32) != t.approx.view(np.uint32))[0]
    assert bad.size == 0, f"{what}: S4 approx not bit-exact at {bad[:5]}"
    assert np.array_equal(tr["sel"], t.sel), f"{what}: S5 selection/order differs"
    tol = rtol_of(p.precision) * np.maximum(np.abs(t.sel_exact), 1.0)
    assert np.all(np.abs(tr["sel_exact"] - t.sel_exact) <= tol), f"{what}: S6 exact scores differ"
    return r


@pytest.fixture(scope="module")
def tie():
    a = TC.build(K=4096, N=N, seed=21, dup_centroids=DUP_CEN, dup_docs=GROUPS, pair=PAIR)
    qs = TC.queries(a, 4, 8, seed=5) + TC.queries(a, 2, 32, seed=6)
    return a, oracle_index(a), hip_index(a), qs


def groups_of(a):
    return a["groups"]


def pairs_of(a):
    P_ = a["pair"]
    return [(P_["B1"], P_["A1"]), (P_["B2"], P_["A2"])]


def group_query(a, g):
    off = np.concatenate([[0], np.cumsum(a["doc_lengths"])])
    return np.ascontiguousarray(a["centroids"][a["codes"][off[g]: off[g + 1]]])


@pytest.mark.parametrize("thr", [None, 3.0])
def test_probe_cut_ties_dense_and_batched(tie, thr):
    """Scores take a few hundred values over 4096 centroids, so equal scores straddle every per-token cut (1, 3, 8,
    40); the duplicate centroids 9 = 10 = 40 = 3000 and 77 = 1077 = 2077 tie inside a group, across groups and across
    centroid_batch_size slabs.  Dense and batched (cbs 1000) paths, t_cs None and set."""
    a, ox, hx, qs = tie
    for n_probe in (1, 3, 8, 40):
        for cbs in (100_000, 1000):
            p = P(n_full_scores=256, top_k=10, n_ivf_probe=n_probe, centroid_score_threshold=thr, centroid_batch_size=cbs)
            for i, q in enumerate(qs[:2] + qs[4:5]):
                r = check_trace(hx, ox, q, p, what=f"np={n_probe} cbs={cbs} thr={thr} q{i}")
                assert r.trace.used_batched == (cbs == 1000)


def test_batched_threshold_ignores_unpushed_tied_pair():
    """Batched path, n_ivf_probe 2, t_cs 0.25: c2 = 30 ties c1 = 20 at token e0's cut with a score >= t_cs, but token
    e0 takes b = 10 and c1, and b, c1 come first in c2's slab, so (e0, c2) never enters the slab heap
    (search.rs:177-199); token e1's score for c2 is below t_cs.  c2 must be dropped by the threshold."""
    a, q = TC.threshold_scenario()
    ox, hx = oracle_index(a), hip_index(a)
    p = P(n_full_scores=64, top_k=10, n_ivf_probe=2, centroid_score_threshold=0.25, centroid_batch_size=100)
    r = check_trace(hx, ox, q, p, what="batched threshold scenario")
    assert r.trace.used_batched and 20 in r.trace.cells and 30 not in r.trace.cells
    res = hx.search(q, p)
    assert_ranking_close(res.passage_ids, res.scores, r.passage_ids, r.scores, RTOL_F32, "batched threshold scenario")


@pytest.mark.parametrize("n_probe", [65, 96, 128])
def test_wide_probe_fallback_lds_maxima(tie, n_probe):
    """G = 128 > n_probe > 64 at K = 4096: more than NP_PROBE_CAPG = 64 groups survive the group cut, so
    probe_mark_kernel takes its re-reading fallback (group maxima in LDS).  Dense with t_cs None / set, batched
    (cbs 1000), and a subset (eligible-centroid branch of the fallback: the scaled probe exceeds G, every group
    survives)."""
    a, ox, hx, qs = tie
    for thr in (None, 3.0):
        p = P(n_full_scores=256, top_k=10, n_ivf_probe=n_probe, centroid_score_threshold=thr)
        for i, q in enumerate(qs[:2] + qs[4:5]):
            check_trace(hx, ox, q, p, what=f"np={n_probe} thr={thr} q{i}")
    pb = P(n_full_scores=256, top_k=10, n_ivf_probe=n_probe, centroid_score_threshold=3.0, centroid_batch_size=1000)
    check_trace(hx, ox, qs[0], pb, what=f"batched np={n_probe}")
    sub = np.concatenate([np.arange(0, N, 3), GROUPS[1]]).astype(np.int64)
    ps = P(n_full_scores=256, top_k=10, n_ivf_probe=n_probe, centroid_score_threshold=None)
    for i, q in enumerate(qs[:2]):
        check_trace(hx, ox, q, ps, subset=sub, what=f"subset np={n_probe} q{i}")


def test_wide_probe_fallback_memory_maxima():
    """K = 2^17: G = 4096 > n_probe in {65, 96, 128} > 64; the group maxima do not fit LDS, so the fallback re-reads
    them from memory (probe_mark_kernel<8>)."""
    a = TC.build(K=1 << 17, N=3000, seed=23, dup_centroids=[(9, 10), (9, 70000), (131000, 131071)],
                 dup_docs=[[1, 2, 1500, 2999]])
    ox, hx = oracle_index(a), hip_index(a)
    qs = TC.queries(a, 2, 8, seed=7)
    for n_probe in (65, 96, 128):
        for thr in (None, 3.0):
            p = P(n_full_scores=256, top_k=10, n_ivf_probe=n_probe, centroid_score_threshold=thr)
            for i, q in enumerate(qs):
                check_trace(hx, ox, q, p, what=f"K=2^17 np={n_probe} thr={thr} q{i}")
    hx.close()


def test_degenerate_tokens_tie_across_all_groups(tie):
    """An all-zero token (every QC +0.0) and a NaN token (every QC non-finite) tie across all 128 groups at K = 4096:
    more than 64 tied groups, so n_ivf_probe = 8 takes the fallback and must take centroids 0-7."""
    a, ox, hx, qs = tie
    z = qs[0].copy()
    z[3] = 0.0
    n = qs[1].copy()
    n[2] = np.nan
    for thr in (None, 3.0):
        for cbs in (100_000, 1000):
            p = P(n_full_scores=256, top_k=10, n_ivf_probe=8, centroid_score_threshold=thr, centroid_batch_size=cbs)
            check_trace(hx, ox, z, p, what=f"zero token thr={thr} cbs={cbs}")
            check_trace(hx, ox, n, p, what=f"NaN token thr={thr} cbs={cbs}")
    # the tied token alone: exactly the lowest ids
    p = P(n_full_scores=256, top_k=10, n_ivf_probe=8, centroid_score_threshold=None)
    assert np.array_equal(hx.debug_trace(np.zeros((1, 128), np.float32), p)["cells"], np.arange(8))


@pytest.mark.parametrize("prec", [0, 1, 2, 3])
def test_selection_and_order_ties(tie, prec):
    """S5: the 100-document duplicate group ties at the n_sel cut (nfs 64 / 160 / 320), so the radix select reads the
    document-id half of its key.  S7: the constructed pairs have equal exact scores and approximate ranks opposite
    to their ids.  Every precision: ids ascend inside each duplicate group, a cut keeps the lowest, pairs keep the
    approximate-rank order."""
    a, ox, hx, qs = tie
    g = GROUPS[1][0]
    q1, q2 = TC.pair_queries(128)
    cases = [(group_query(a, g), nfs, tk) for nfs, tk in ((64, 16), (160, 40), (320, 80))]
    cases += [(q1, 64, 4), (q2, 64, 4), (np.concatenate([q1, group_query(a, g)]), 160, 40)]
    for i, (q, nfs, tk) in enumerate(cases):
        p = P(n_full_scores=nfs, top_k=tk, n_ivf_probe=2, centroid_score_threshold=None, precision=prec)
        o = check_trace(hx, ox, q, p, what=f"prec={prec} case {i}")
        r = hx.search(q, p)
        assert_ranking_close(r.passage_ids, r.scores, o.passage_ids, o.scores, rtol_of(prec), f"prec={prec} case {i}")
        assert_ties_strict(r.passage_ids, groups_of(a), pairs_of(a), f"prec={prec} case {i}")
        assert_ties_strict(o.passage_ids, groups_of(a), pairs_of(a), f"oracle case {i}")
        if i < 3:
            sel = hx.debug_trace(q, p)["sel"]
            gg = np.array(GROUPS[1])
            inside = sel[np.isin(sel, gg)]
            assert 0 < inside.size < gg.size, f"case {i}: the n_sel cut does not fall inside the group"
    P_ = a["pair"]
    r = hx.search(q1, P(n_full_scores=64, top_k=4, n_ivf_probe=2, centroid_score_threshold=None, precision=prec))
    assert r.passage_ids.tolist() == [P_["B1"], P_["B2"], P_["A1"], P_["A2"]]


@pytest.fixture
def tuned(tie):
    hx = tie[2]
    yield hx
    for k, v in (("s4_mode", 4), ("s4_minb", 8), ("s4_swz", 1), ("s4_filter", 1), ("s6_xcd", 1), ("s6_lds", 1), ("s6_tiles", 1), ("exact_rowmax", 0), ("ub_nt", 2), ("ub_steal", 16384), ("ub_nbx", 96), ("s4_hot", 60), ("ub_direct", 8), ("ub_static", 0), ("hot_static", 1), ("s4_planes", 1), ("s4_lpd", 2), ("s4_qm", 1), ("s4_warm", 0), ("s4_hot_auto", 200000), ("s3_bisect", 1), ("s3_gain", 1), ("s3_gain_mult", 3),
                 ("s3_gain_direct", 16)):
        hx.tune(k, v)


def _tie_batch(a, qs):
    g = GROUPS[1][0]
    q1, q2 = TC.pair_queries(128)
    return list(qs) + [group_query(a, g), q1, q2, np.concatenate([q2, group_query(a, GROUPS[0][0])])]


def test_kernel_choice_keeps_tied_selection(tie, tuned):
    """S4 kernel family (s4_mode 0-8, with and without the upper-bound filter), the single-level filter (s4_hot 0) and
    the zeroth level (s3_gain 0 / 2) must not change which tied documents are kept: results bit-identical.  The
    filters' cuts must keep every document tied at them."""
    a, ox, hx, qs = tie
    batch = _tie_batch(a, qs)
    p = P(n_full_scores=160, top_k=40, n_ivf_probe=8, centroid_score_threshold=None)
    ref = hx.search_batch(batch, p)
    for i, r in enumerate(ref):
        assert_ties_strict(r.passage_ids, groups_of(a), pairs_of(a), f"default q{i}")
    for o, r in zip(ox.search_batch(batch, to_oracle_params(p)), ref):
        assert_ranking_close(r.passage_ids, r.scores, o.passage_ids, o.scores, RTOL_F32)

    def same(what):
        for i, (g, r) in enumerate(zip(hx.search_batch(batch, p), ref)):
            assert np.array_equal(g.passage_ids, r.passage_ids) and np.array_equal(g.scores, r.scores), f"{what} q{i}"

    hx.tune("s4_minb", 1)
    for filt in (0, 1):
        hx.tune("s4_filter", filt)
        for mode in range(9):
            hx.tune("s4_mode", mode)
            same(f"s4_mode={mode} s4_filter={filt}")
    hx.tune("s4_mode", 4)
    hx.tune("s4_minb", 8)
    hx.tune("s4_hot", 0)
    same("s4_hot=0")
    hx.tune("s4_hot", 60)
    for gain in (0, 2):
        hx.tune("s3_gain", gain)
        same(f"s3_gain={gain}")
        if gain == 2:
            assert hx.last_stats["n_level0"] > 0


def test_zeroth_level_gate_at_its_edge(tie, tuned):
    """gain_possible needs max(n_ivf_probe, 32) x maxLq <= 16384: n_ivf_probe 512 with 32-token queries and 256 with
    64-token queries sit exactly on it (n_level0 > 0 in last_stats: the level ran, its 15-bit scaled gains at their
    largest sum), 513 x 32 is past it (n_level0 == 0).  Results bit-equal to s3_gain = 0."""
    a, ox, hx, qs = tie
    q32 = TC.queries(a, 3, 32, seed=8) + [group_query(a, GROUPS[1][0])]
    q64 = TC.queries(a, 3, 64, seed=9)
    for batch, n_probe, runs in ((q32, 512, True), (q64, 256, True), (q32, 513, False)):
        p = P(n_full_scores=160, top_k=40, n_ivf_probe=n_probe, centroid_score_threshold=None)
        hx.tune("s3_gain", 0)
        ref = hx.search_batch(batch, p)
        hx.tune("s3_gain", 2)
        got = hx.search_batch(batch, p)
        st = dict(hx.last_stats)
        assert (st["n_level0"] > 0) == runs, (n_probe, st)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert np.array_equal(g.passage_ids, r.passage_ids) and np.array_equal(g.scores, r.scores), f"np={n_probe} q{i}"
            assert_ties_strict(g.passage_ids, groups_of(a), (), f"np={n_probe} q{i}")
    o = ox.search(q32[0], to_oracle_params(p))
    r = hx.search(q32[0], p)
    assert_ranking_close(r.passage_ids, r.scores, o.passage_ids, o.scores, RTOL_F32, "wide probe vs oracle")


def test_candidate_pool_rounds_with_ties(tie):
    """A small workspace_bytes splits the batch into candidate-pool rounds; ties must resolve as in one round."""
    a, ox, hx, qs = tie
    small = hip_index(a, workspace_bytes=11 << 20, max_batch=16)
    small.tune("s3_gain", 0)
    batch = _tie_batch(a, qs)
    p = P(n_full_scores=160, top_k=40, n_ivf_probe=64, centroid_score_threshold=None)
    res = small.search_batch(batch, p)
    assert small.last_stats["n_rounds"] >= 2, small.last_stats
    ref = hx.search_batch(batch, p)
    assert hx.last_stats["n_rounds"] == 1
    for i, (r, f) in enumerate(zip(res, ref)):
        assert np.array_equal(r.passage_ids, f.passage_ids) and np.array_equal(r.scores, f.scores), f"rounds q{i}"
        assert_ties_strict(r.passage_ids, groups_of(a), pairs_of(a), f"rounds q{i}")
    small.close()


@pytest.mark.parametrize("G", [2, 3])
def test_sharded_ties_equal_unsharded(tie, G):
    """Duplicate groups split across the shards: the sharded cut and merge (select_cut, merge_topk, merge_packed) see
    tied keys from several shards and must keep the unsharded result bit for bit; also the C-level sharded entry."""
    import torch
    from next_plaid_amd.dist import CShardedSearcher, HipShardBackend, ShardComm, ShardedSearcher
    a, ox, hx, qs = tie
    shards = [hip_index(a, shard_rank=r, shard_count=G) for r in range(G)]
    bounds = [int(s.info.shard_doc_begin) for s in shards[1:]]
    for b in bounds:     # every shard boundary splits a duplicate group
        assert any(min(g) < b <= max(g) for g in GROUPS), (bounds, b)
    stream = torch.cuda.Stream()
    ss = ShardedSearcher([HipShardBackend(s, stream=stream) for s in shards], use_dist=False)
    batch = _tie_batch(a, qs)
    for nfs, tk, thr in ((160, 40, None), (64, 16, 3.0), (400, 100, None)):
        p = P(n_full_scores=nfs, top_k=tk, n_ivf_probe=8, centroid_score_threshold=thr)
        ref = hx.search_batch(batch, p)
        for i, (r, f) in enumerate(zip(ss.search_batch(batch, p), ref)):
            assert np.array_equal(r.passage_ids, f.passage_ids), f"G={G} nfs={nfs} q{i}: {r.passage_ids} vs {f.passage_ids}"
            assert np.array_equal(r.scores, f.scores), f"G={G} nfs={nfs} q{i} scores"
            assert_ties_strict(r.passage_ids, groups_of(a), pairs_of(a), f"G={G} q{i}")
    comm = ShardComm(hx, 0, 1, rccl=False)
    cs = CShardedSearcher(hx, comm)
    p = P(n_full_scores=160, top_k=40, n_ivf_probe=8, centroid_score_threshold=None)
    for r, f in zip(cs.search_batch(batch, p), hx.search_batch(batch, p)):
        assert np.array_equal(r.passage_ids, f.passage_ids) and np.array_equal(r.scores, f.scores)
    comm.close()
    for s in shards:
        s.close()
