"""The forms a call's scope can take, through the host-scope helper that np_hip_search_exact, np_hip_text_search,
np_hip_search_hybrid and their filtered forms share, at its branch points.  Needs a real MI355X.

Every case reaches the C ABI with the arguments it names (the Python wrappers would normalise some of these forms away, so
the calls go through api's ctypes layer); forms that mean the same scope must give the same bits."""
import ctypes as C

import numpy as np
import pytest

from helpers import hip_index, make_arrays

import next_plaid_amd as npa
from next_plaid_amd import api, synth, text as T
import text_restate as R

pytestmark = pytest.mark.gpu

N, B, TOP_K = 200, 3, 5
CALLS = ["search_exact", "text_search", "search_hybrid"]


class Csr:
    """A host CSR as it reaches the library: ids / offsets (None = NULL), n_subsets, the query map."""

    def __init__(self, ids, offsets, query_subset):
        self.ids = None if ids is None else np.ascontiguousarray(ids, np.int64)
        self.off = None if offsets is None else np.ascontiguousarray(offsets, np.int64)
        self.n = 0 if self.off is None else self.off.size - 1
        self.qsub = None if query_subset is None else np.ascontiguousarray(query_subset, np.int32)


class Filters:
    """Compiled filters as they reach the library: the programs (an empty list: n_filters = 0) and the query map."""

    def __init__(self, hx, conds, query_filter):
        from next_plaid_amd import filters as F
        self.cf = api._CFilters([F.compile_filter(c, p, hx.schema) for c, p in conds])
        self.qf = np.ascontiguousarray(query_filter, np.int32)


NO_SCOPE = Csr(None, None, None)


@pytest.fixture(scope="module")
def world():
    spec, a = make_arrays(num_docs=N, num_centroids=16, dim=32, nbits=2, doc_len_min=4, doc_len_max=12, seed=11)
    hx = hip_index(a)
    hx.set_text(T.TextIndexData.from_texts(R.make_texts(N, 12, seed=N, every="wo0", lens=(1, 2, 3, 5, 8))))
    hx.set_columns({"z": np.arange(N, dtype=np.int64) % 4})
    queries, _ = synth.make_queries(spec, B, n_tokens=8, cen=a["centroids"])
    text_queries = hx._text_queries(["wo0", "wo1 OR wo2", "wo0 wo3"], True)
    want = {}   # the unscoped result of every call, computed once
    yield hx, queries, text_queries, want
    hx.close()


def run(world, call, scope):
    """One call through ctypes with the scope as given; per query (ids, score bits) cut at its count."""
    hx, queries, text_queries, _ = world
    lib = api.lib()
    ids, sc, cnt = np.zeros(B * TOP_K, np.int64), np.zeros(B * TOP_K, np.float32), np.full(B, -7, np.int32)
    out = (api._ptr(ids), api._ptr(sc), api._ptr(cnt))
    flat, off = hx._pack(queries)
    tq = api._CTextQueries(text_queries)
    st = api.np_stats()
    filt = isinstance(scope, Filters)
    if call == "search_exact":
        head = (hx._h, api._ptr(flat), api._ptr(off), B, hx.embedding_dim(), TOP_K, 0)
        if filt:
            rc = lib.np_hip_search_exact_filtered(*head, scope.cf.arr, scope.cf.n, api._ptr(scope.qf), *out, C.byref(st))
        else:
            rc = lib.np_hip_search_exact(*head, api._ptr(scope.ids), api._ptr(scope.off), scope.n, api._ptr(scope.qsub), *out,
                                         C.byref(st))
    elif call == "text_search":
        if filt:
            rc = lib.np_hip_text_search_filtered(hx._h, tq.arr, B, TOP_K, scope.cf.arr, scope.cf.n, api._ptr(scope.qf), *out,
                                                 C.byref(st))
        else:
            rc = lib.np_hip_text_search(hx._h, tq.arr, B, TOP_K, api._ptr(scope.ids), api._ptr(scope.off), scope.n,
                                        api._ptr(scope.qsub), *out, C.byref(st))
    else:
        p = npa.SearchParameters(n_full_scores=64, top_k=TOP_K, n_ivf_probe=4)._c()
        head = (hx._h, api._ptr(flat), api._ptr(off), B, hx.embedding_dim(), C.byref(p), tq.arr, 3 * TOP_K, 0.75,
                T.FUSION_MODES["relative_score"])
        if filt:
            rc = lib.np_hip_search_hybrid(*head, None, None, scope.cf.n, api._ptr(scope.qf), scope.cf.arr, scope.cf.n, *out, C.byref(st))
        else:
            rc = lib.np_hip_search_hybrid(*head, api._ptr(scope.ids), api._ptr(scope.off), scope.n, api._ptr(scope.qsub), None, 0,
                                          *out, C.byref(st))
    api._check(rc)
    assert ((cnt >= 0) & (cnt <= TOP_K)).all(), cnt
    return [(ids[b * TOP_K: b * TOP_K + cnt[b]].copy(), sc[b * TOP_K: b * TOP_K + cnt[b]].view(np.uint32).copy()) for b in range(B)]


def unscoped(world, call):
    want = world[3]
    if call not in want:
        want[call] = run(world, call, NO_SCOPE)
        assert all(ids.size > 0 for ids, _ in want[call]), f"{call}: a query without a result checks nothing"
    return want[call]


def same(got, want):
    return all(np.array_equal(gi, wi) and np.array_equal(gs, ws) for (gi, gs), (wi, ws) in zip(got, want))


@pytest.mark.parametrize("call", CALLS)
def test_a_csr_no_query_refers_to_is_no_scope(world, call):
    scope = Csr(np.arange(20), [0, 10, 20], [-1] * B)
    assert scope.n == 2
    assert same(run(world, call, scope), unscoped(world, call))


@pytest.mark.parametrize("call", CALLS)
def test_every_subset_empty_returns_nothing(world, call):
    scope = Csr(None, [0, 0, 0], [0, 1, 0])                                 # total = 0: no ids at all, NULL
    assert all(ids.size == 0 for ids, _ in run(world, call, scope))


@pytest.mark.parametrize("call", CALLS)
def test_filters_no_query_is_mapped_to_are_no_scope(world, call):
    scope = Filters(world[0], [("z = ?", [1]), ("0 = 1", [])], [-1] * B)
    assert scope.cf.n == 2
    assert same(run(world, call, scope), unscoped(world, call))


@pytest.mark.parametrize("call", CALLS)
def test_the_filtered_call_without_filters_is_no_scope(world, call):
    scope = Filters(world[0], [], [-1] * B)
    assert scope.cf.n == 0
    assert same(run(world, call, scope), unscoped(world, call))


@pytest.mark.parametrize("call", CALLS)
def test_a_filter_matching_nothing_returns_nothing(world, call):
    scope = Filters(world[0], [("0 = 1", [])], [0] * B)
    assert all(ids.size == 0 for ids, _ in run(world, call, scope))


@pytest.mark.parametrize("call", CALLS)
def test_filters_equal_the_host_csr_of_their_ids(world, call):
    hx = world[0]
    conds, qmap = [("z = ?", [1]), ("z >= ?", [2])], [0, -1, 1]
    sets = hx.filter_ids(conds)
    assert [s.size for s in sets] == [N // 4, N // 2]
    csr = Csr(np.concatenate(sets), np.cumsum([0] + [s.size for s in sets]), qmap)
    by_filter, by_csr, free = run(world, call, Filters(hx, conds, qmap)), run(world, call, csr), unscoped(world, call)
    assert same(by_filter, by_csr)
    for b, q in enumerate(qmap):
        ids = by_filter[b][0]
        if q < 0:
            assert np.array_equal(ids, free[b][0])
        else:
            assert ids.size > 0 and np.isin(ids, sets[q]).all()
    assert not same(by_filter, free)                                        # the scope did cut something
