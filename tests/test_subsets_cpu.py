"""One subset per query, the parts that need no device: the CSR packing of `subsets=` and the semantics the GPU tests hold
the batch to -- query i of a batch with subsets[i] gets what the reference's single-subset search returns for that query and
that subset alone (search.rs:350-382, 434-437), stated with the oracle's existing search."""
import numpy as np
import pytest

from helpers import make_arrays, oracle_index, synth

from next_plaid_amd import api
from oracle import oracle as O


def test_pack_shares_by_identity_and_keeps_none():
    a = np.array([4, 2, 2, 9], np.int64)
    b = np.array([4, 2, 2, 9], np.int64)   # equal contents, another object: another subset
    ids, off, qsub = api.pack_subsets([a, None, b, a, None], 5)
    assert qsub.dtype == np.int32 and qsub.tolist() == [0, -1, 1, 0, -1]
    assert off.dtype == np.int64 and off.tolist() == [0, 4, 8]
    assert ids.dtype == np.int64 and ids.tolist() == [4, 2, 2, 9, 4, 2, 2, 9]   # duplicates and order as given


def test_pack_empty_arrays_and_no_subsets():
    e = np.zeros(0, np.int64)
    ids, off, qsub = api.pack_subsets([e, np.array([7]), e, np.zeros(0, np.int32)], 4)
    assert qsub.tolist() == [0, 1, 0, 2] and off.tolist() == [0, 0, 1, 1] and ids.tolist() == [7]
    ids, off, qsub = api.pack_subsets([None, None], 2)
    assert ids.size == 0 and ids.dtype == np.int64 and off.tolist() == [0] and qsub.tolist() == [-1, -1]
    ids, off, qsub = api.pack_subsets([], 0)
    assert ids.size == 0 and off.tolist() == [0] and qsub.size == 0


def test_pack_coerces_dtypes_and_sequences():
    lst = [3, 1, -3]
    ids, off, qsub = api.pack_subsets([np.array([5, 6], np.int32), lst, np.array([[1, 2], [3, 4]], np.uint8), lst], 4)
    assert ids.dtype == np.int64 and ids.tolist() == [5, 6, 3, 1, -3, 1, 2, 3, 4]
    assert off.tolist() == [0, 2, 5, 9] and qsub.tolist() == [0, 1, 2, 1]
    assert ids.flags["C_CONTIGUOUS"] and off.flags["C_CONTIGUOUS"] and qsub.flags["C_CONTIGUOUS"]


def test_pack_argument_errors():
    with pytest.raises(ValueError):
        api.pack_subsets([None, None], 3)
    with pytest.raises(ValueError):
        api.pack_subsets([None, None, None], 2)

    class NoLibrary:   # both= is refused before anything reaches the library
        def __getattr__(self, name):
            raise AssertionError("the library was touched")
    ix = api.MmapIndex.__new__(api.MmapIndex)
    ix._h = NoLibrary()
    with pytest.raises(ValueError):
        api.MmapIndex.search_batch(ix, [np.zeros((2, 8), np.float32)], api.SearchParameters(), subset=[1], subsets=[None])
    with pytest.raises(ValueError):
        api.MmapIndex.search_batch(ix, [np.zeros((2, 8), np.float32)], api.SearchParameters(), subsets=[None, None])


def per_query_reference(ox, queries, params, subsets):
    """THE statement: a batch with one subset per query is the single-subset search, query by query."""
    return [ox.search(q, params, s, trace=True) for q, s in zip(queries, subsets)]


def test_per_query_semantics_of_the_gpu_case():
    """The index, parameters and subsets of test_gpu_subsets.test_one_query_many_subsets: what the single-subset reference
    gives each copy of the query -- the probe depths of search.rs:370-382 differ in one batch, an empty subset empties one
    result only, and sharing a subset object changes nothing."""
    spec, a = make_arrays(num_docs=2000, num_centroids=256, dim=128, nbits=4, doc_len_min=10, doc_len_max=40, seed=31)
    ox = oracle_index(a)
    q = synth.make_queries(spec, 8, n_tokens=16, cen=a["centroids"])[0][0]
    evens = np.arange(0, 2000, 2, dtype=np.int64)
    few = np.array([5, 17, 1999, 4000, -3], np.int64)
    subsets = [evens, None, few, np.arange(100, dtype=np.int64), np.zeros(0, np.int64), evens]
    p = O.SearchParameters(n_full_scores=256, top_k=10, n_ivf_probe=4, centroid_score_threshold=None)
    ref = per_query_reference(ox, [q] * 6, p, subsets)
    codes, doc_off = np.asarray(a["codes"]), np.concatenate([[0], np.cumsum(a["doc_lengths"])])

    def eligible(sub):
        return np.unique(np.concatenate([codes[doc_off[d]:doc_off[d + 1]] for d in sub if 0 <= d < 2000]))
    # effective probe depth per query: nprobe * N / |subset| clamped to [nprobe, n_elig]; every token marks that many cells
    n_elig = [eligible(s).size if s is not None and s.size else None for s in subsets]
    assert n_elig[2] <= 120 and 4 * 2000 // 5 == 1600 > n_elig[2]      # take-all: the cells ARE the eligible centroids
    assert np.array_equal(ref[2].trace.cells, eligible(few))
    depth = [8, 4, n_elig[2], min(80, n_elig[3]), 0, 8]
    for r, s, d in zip(ref, subsets, depth):
        assert d <= r.trace.cells.size <= 16 * d                        # 16 tokens, each marks `depth` cells
        if s is not None:
            assert set(r.trace.cells.tolist()) <= set(eligible(s).tolist()) if s.size else r.trace.cells.size == 0
            assert set(r.passage_ids.tolist()) <= set(s.tolist())
            assert np.all(np.isin(r.trace.cand, s))
    assert len({tuple(r.trace.cells.tolist()) for r in ref[:5]}) >= 3   # the subsets separate the queries
    assert ref[4].passage_ids.size == 0 and ref[1].passage_ids.size == 10 and ref[0].passage_ids.size == 10
    assert np.array_equal(ref[0].passage_ids, ref[5].passage_ids) and np.array_equal(ref[0].scores, ref[5].scores)
    # ... and a query without a subset is the query of a batch without any
    plain = ox.search(q, p)
    assert np.array_equal(ref[1].passage_ids, plain.passage_ids) and np.array_equal(ref[1].scores, plain.scores)
