"""np_hip_index_expand at the limits of its own kernels: ivf_keep_kernel, ivf_cut_offsets_kernel, ivf_cut_merge_kernel and
widen_codes_kernel, and the token stages that start at a cut inside the old tokens (tests/expand_limit_shapes.py holds the
cases, tests/test_expand_limits_cpu.py proves that each reaches its edge).  Needs a real MI355X.

Per case the base is opened, the reservation applied and the case's expand made (twice where the case says so).  The handle is
then held to the six points of tests/test_gpu_append_limits.py, with expand_restate.expanded_arrays -- the base's OWN lists cut
at the first dropped document, the given ids behind them -- in the place of grown_arrays:
  1. export() equals expanded_arrays: doc_lengths, codes, residuals, ivf, ivf_lengths;
  2. a fresh handle of those arrays: _assert_equal_to_fresh of tests/test_gpu_index_expand.py;
  3. the oracle on those arrays, stage by stage and through search_batch under s3_gain 0 and 2 (RTOL_F32), for queries made of
     given documents' tokens -- the first of tokens that sit on NEW centroids wherever the case has such a token;
  4. the fresh handle's last_stats counters, split into COUNTERS and UPSTREAM_AND_SELECTION by range count as that suite documents;
  5. the zeroth level runs, or stays off, where the case states it;
  6. decompress_documents of every given document inside decompress_limit_shapes.e_gpu for the inverse-norm, capacity and
     empty cases.
An index without a single token (every document replaced by an empty one) has no document to make a query of: it is held to
points 1, to the fresh handle's info and, after a plain append of documents, to point 2.

The way back (np_hip_index_tune "expand_fail", stages 1-4) is walked at three shapes the contract test leaves out: nothing
replaced, a replaced tail of empty documents, and given tokens that reach past T0 inside a reservation.
"""
import time

import numpy as np
import pytest

import append_restate as A
import expand_limit_shapes as S
import expand_restate as E
from append_limit_shapes import rand_docs
from helpers import hip_index
from test_gpu_append_limits import P, _against_the_oracle, _counters, _decompress_all
from test_gpu_index_expand import _assert_equal_to_fresh, _info, _queries, _refused

pytestmark = pytest.mark.gpu

EXPORTED = ("doc_lengths", "codes", "residuals", "ivf", "ivf_lengths")


def _case_queries(final, n_keep, K0):
    """queries of given documents' tokens: one of the tokens on new centroids (where there is one), then the longest given
    documents'"""
    lens = np.asarray(final["doc_lengths"], np.int64)
    off = A.offsets(lens)
    tok = np.arange(off[n_keep], off[-1])
    if tok.size == 0:
        return []
    qs = []
    on_new = tok[np.asarray(final["codes"])[tok] >= K0]
    if on_new.size:
        view = dict(final, doc_lengths=np.array([on_new.size], np.int64), codes=final["codes"][on_new], residuals=final["residuals"][on_new])
        qs += _queries(view, [0])
    longest = (n_keep + np.argsort(-lens[n_keep:], kind="stable")[:3]).tolist()
    qs += _queries(final, longest)
    if len(qs) < 2:      # a single given document on old centroids: a second draw of its tokens
        qs += _queries(final, longest, seed=12)
    assert len(qs) >= 2
    return qs


def _held_to_the_six_points(hx, final, n_keep, K0, level, decompress_all, what):
    got = hx.export()
    for k in EXPORTED:                                                                               # 1
        assert np.array_equal(got[k], final[k]), f"{what}: export()[{k!r}] against expanded_arrays"
    assert hx.num_partitions() == final["centroids"].shape[0]
    fresh = hip_index(final)
    try:
        queries = _case_queries(final, n_keep, K0)
        if not queries:      # no token anywhere: nothing to ask for
            assert int(final["doc_lengths"].sum()) == 0 and _info(hx) == _info(fresh), what
            more = rand_docs(np.random.default_rng(3), [4, 9, 1], K0)
            grown = A.grown_arrays(final, more)
            hx.append_arrays(*more)
            n = final["doc_lengths"].size
            for k in EXPORTED:
                assert np.array_equal(hx.export()[k], grown[k]), f"{what}: export()[{k!r}] after an append"
            fresh.close()
            fresh = hip_index(grown)
            _assert_equal_to_fresh(hx, fresh, _queries(grown, [n, n + 1, n + 2]), n, what + " + an append")
            return
        _assert_equal_to_fresh(hx, fresh, queries, n_keep, what)                                     # 2
        _against_the_oracle(hx, final, queries, what)                                                # 3
        _counters(hx, fresh, queries, level, final["doc_lengths"].size, what)                        # 4, 5
        if decompress_all:
            _decompress_all(hx, final, n_keep, what)                                                 # 6
    finally:
        fresh.close()


def _opened(case):
    hx = hip_index(case.base)
    if case.remove_all:
        n = case.base["doc_lengths"].size
        assert hx.remove_ids(np.arange(n)) == n and hx.num_documents() == 0
    if case.reserve:
        hx.reserve(*case.reserve)
        assert hx.capacity() == (case.N0 + case.reserve[0], case.T0 + case.reserve[1])
    return hx


@pytest.mark.parametrize("case", S.all_cases(), ids=lambda c: c.name)
def test_expand_at_the_limit(case, monkeypatch):
    for k, v in (case.env or {}).items():
        monkeypatch.setenv(k, v)
    t0 = time.perf_counter()
    final = case.final()
    hx = _opened(case)
    try:
        before = hx.capacity()
        ids = hx.expand_arrays(case.new_centroids, *case.given, n_replace=case.n_replace)
        assert ids.tolist() == list(range(case.Nk, case.N1))
        want_cap = (max(before[0], case.N1), max(before[1], case.T1))      # grow_capacity's rule
        assert hx.capacity() == want_cap, (hx.capacity(), want_cap)
        if not case.remove_all:
            assert want_cap == S.capacity_after(case)
        _held_to_the_six_points(hx, final, case.Nk, case.K0, case.level, case.decompress_all and case.T1 > case.Tk, case.name)
        if case.then is not None:
            cen, given, n_replace = case.then
            final2 = case.final2()
            n_keep = final["doc_lengths"].size - n_replace
            ids = hx.expand_arrays(cen, *given, n_replace=n_replace)
            assert ids.tolist() == list(range(n_keep, n_keep + len(given[0])))
            _held_to_the_six_points(hx, final2, n_keep, final["centroids"].shape[0], case.level, False, case.name + " (second expand)")
    finally:
        hx.close()
    print(f"{case.name}: {time.perf_counter() - t0:.2f} s")


def test_widening_across_the_stride_loops_second_turn():
    """Tk = 8 * (8192 * 256 + 1) + 5 = 16 777 229 kept tokens: widen_codes_kernel's grid is capped at 8192 blocks and thread 0
    takes a second turn of the stride loop.  The one large case, with lean checks only: export()'s codes and doc_lengths and
    info against numpy, one search_batch equal to the fresh handle's.

    Measured on an MI355X, one run of this test behind test_the_range_table_across_a_range_boundary of
    tests/test_gpu_index_expand.py: 0.74 s here (building the arrays included) against 0.34 s + 0.06 s for that test's two
    cases, the first of which also paid the process's first open.  It is kept because it takes less than three times that
    test (1.20 s)."""
    t0 = time.perf_counter()
    case = S.big_widen()
    assert case.Tk == S.BIG_TK and E.expected_widen(case.Tk)["max_turns"] == 2
    lens = np.concatenate([case.base["doc_lengths"][:case.Nk], case.given[0]])
    codes = np.concatenate([case.base["codes"][:case.Tk], case.given[1]])
    hx = hip_index(case.base)
    try:
        hx.expand_arrays(case.new_centroids, *case.given, n_replace=case.n_replace)
        got = hx.export()
        assert np.array_equal(got["doc_lengths"], lens)
        assert np.array_equal(got["codes"], codes), "export()['codes'] after the widening"
        assert hx.num_documents() == lens.size and hx.num_partitions() == case.K1 and int(hx.info.shard_embeddings) == codes.size
        final = case.final()
        queries = _case_queries(final, case.Nk, case.K0)
        mine = [(r.passage_ids.tobytes(), np.asarray(r.scores, np.float32).tobytes()) for r in hx.search_batch(queries, P(0.4))]
        info = _info(hx)
    finally:
        hx.close()
    fresh = hip_index(final)
    try:
        assert info == _info(fresh)
        assert mine == [(r.passage_ids.tobytes(), np.asarray(r.scores, np.float32).tobytes()) for r in fresh.search_batch(queries, P(0.4))]
    finally:
        fresh.close()
    print(f"widening across the stride loop's second turn: {time.perf_counter() - t0:.2f} s")


# ---- the way back ------------------------------------------------------------------------------------------------------------------
WAY_BACK = ("nothing replaced, new centroids",                    # nothing saved, but offsets and tokens behind the end were written
            "a replaced tail of empty documents",                 # offsets saved, no token
            "capacity: the reservation filled exactly")           # the given tokens reach past T0 inside the reservation


@pytest.mark.parametrize("stage", [1, 2, 3, 4])
@pytest.mark.parametrize("name", WAY_BACK)
def test_a_failure_before_the_swap_puts_the_handle_back(name, stage):
    case = S.case(name)
    base = case.base
    assert case.T1 > case.T0 and (case.reserve is None or case.T1 <= case.T0 + case.reserve[1])
    qs = _queries(base, list(range(case.N0 - 4, case.N0)) + [0, 1])
    assert len(qs) >= 2
    more = rand_docs(np.random.default_rng(stage), [6, 0, 11], case.K0)
    grown = A.grown_arrays(base, more)
    hx, fresh = _opened(case), hip_index(grown)
    try:
        cap = hx.capacity()
        hx.tune("expand_fail", stage)
        _refused(hx, qs, lambda: hx.expand_arrays(case.new_centroids, *case.given, n_replace=case.n_replace), MemoryError,
                 f"out of memory after stage {stage}")
        assert hx.num_partitions() == case.K0 and hx.num_documents() == case.N0
        got = hx.export()
        for k in EXPORTED:
            assert np.array_equal(got[k], base[k]), f"{name}, stage {stage}: export()[{k!r}] after the failure"
        if case.reserve:
            assert hx.capacity() == cap
        hx.tune("expand_fail", 0)
        assert hx.append_arrays(*more).tolist() == list(range(case.N0, case.N0 + 3))
        _assert_equal_to_fresh(hx, fresh, _queries(grown, [case.N0, case.N0 + 2, 0, 1]), case.N0, f"{name}, an append after stage {stage}")
    finally:
        hx.close()
        fresh.close()
