"""The checker of the GPU pooling is checked itself: tests/pool_restate.py against the reference's own known answers
(next-plaid-onnx/src/hierarchy.rs:829-907), against scipy (merge sets, and the distance-ordered cut against fcluster), and
np_hip_pooled_lengths against the formula.  The last test shows that the corpus tests/test_gpu_pool.py uses can tell the
two cut orders apart and that the nearest-neighbour cache decides a document.  CPU only."""
import numpy as np
import pytest
from scipy.cluster.hierarchy import fcluster, linkage
from scipy.spatial.distance import squareform

import pool_restate as R

from next_plaid_amd.api import np_pool_opts, pooled_lengths   # the pooling ABI: absent before np_pool.hip


def test_reference_known_answers():
    # test_linkage_ward_simple
    Z = R.linkage_ward(squareform(np.array([1.0, 2.0, 3.0, 1.5, 2.5, 1.0])))
    assert Z.shape == (3, 4) and np.all(Z[:, 2] >= 0.0) and np.all(Z[:, 3] >= 2.0)
    # test_fcluster_maxclust
    Z = R.linkage_ward(squareform(np.array([1.0, 4.0, 5.0, 3.0, 4.5, 2.0])))
    lab = R.fcluster_maxclust(Z, 4, 2)
    assert lab.shape == (4,) and len(set(lab.tolist())) == 2
    assert R.fcluster_maxclust(Z, 4, 4).tolist() == [1, 2, 3, 4] and R.fcluster_maxclust(Z, 4, 0).tolist() == [1, 1, 1, 1]
    # test_pdist_cosine
    d = R.pdist_cosine_square(np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]], np.float32))
    assert abs(d[0, 1]) < 1e-10 and abs(d[0, 2] - 1.0) < 1e-10 and abs(d[1, 2] - 1.0) < 1e-10
    # zero rows: cosine 0, distance 1
    d = R.pdist_cosine_square(np.array([[0.0, 0.0], [1.0, 0.0]], np.float32))
    assert d[0, 1] == 1.0
    assert np_pool_opts().pool_factor == 0


def _members(Z, m):
    mem = [frozenset([i]) for i in range(m)]
    for a, b, _, c in Z:
        mem.append(mem[int(a)] | mem[int(b)])
        assert len(mem[-1]) == int(c)
    return set(mem[m:])


def _docs(seed, count, lo, hi, dim=64, dup=False):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        x = R.clustered_document(rng, int(rng.integers(lo, hi + 1)), dim)
        if dup:
            for _ in range(3):
                i, j = rng.integers(0, x.shape[0], 2)
                x[i] = x[j]
        out.append(x)
    return out


def test_merge_sets_equal_scipy():
    for x in _docs(11, 12, 20, 160):
        d = R.pdist_cosine_square(x)
        Z = R.linkage_ward(d)
        Zs = linkage(squareform(d, checks=False), "ward")
        assert np.allclose(np.sort(Z[:, 2]), np.sort(Zs[:, 2]), rtol=0, atol=1e-10)
        assert _members(Z, x.shape[0]) == _members(Zs, x.shape[0])


@pytest.mark.parametrize("dup", [False, True])
def test_distance_cut_equals_scipy_fcluster(dup):
    n_checked = 0
    for x in _docs(23 + dup, 14, 20, 200, dup=dup):
        d = R.pdist_cosine_square(x)
        Z = R.linkage_ward(d)
        Zs = linkage(squareform(d, checks=False), "ward")
        m = x.shape[0]
        for f in (2, 3, 4):
            k = max(m // f, 1)
            mine = R.fcluster_maxclust(Z, m, k, cut_order=1)
            ref = fcluster(Zs, k, "maxclust")
            assert np.array_equal(R.partition_of(mine), R.partition_of(ref))
            assert mine.max() == k
            n_checked += 1
    assert n_checked == 42


def test_pooled_lengths_against_the_formula():
    lens = np.arange(0, 70)
    for f in (-1, 0, 1, 2, 3, 4, 7, 1000):
        for p in (0, 1, 2, 5):
            got = pooled_lengths(lens, f, p)
            want = [R.pooled_length(int(n), f, p) for n in lens]
            assert got.tolist() == want, (f, p)
    assert pooled_lengths([], 2).size == 0
    assert pooled_lengths([300, 1030, 2, 3], 2).tolist() == [150, 515, 2, 2]
    with pytest.raises(ValueError):
        pooled_lengths([4, -1], 2)
    with pytest.raises(ValueError):
        pooled_lengths([4], 2, protected_tokens=-1)


def test_corpus_is_discriminating():
    """The two cut orders give different partitions on most documents, and the cache rule decides a tied document."""
    docs = [d for d in R.gpu_corpus(128, stride=9) if R.pooled_length(d.shape[0], 2) != d.shape[0] and d.shape[0] >= 20]
    assert len(docs) >= 25
    differ = 0
    for x in docs:
        _, l0, Z = R.pool_document(x, 2, cut_order=0)
        _, l1, _ = R.pool_document(x, 2, cut_order=1, linkage=Z)
        assert l0.max() == l1.max() == (x.shape[0] - 1) // 2
        differ += not np.array_equal(l0, l1)
    assert differ > len(docs) // 2, (differ, len(docs))
    x = R.cache_sensitive_document()
    o0, l0, Z0 = R.pool_document(x, 2)
    o1, l1, Z1 = R.pool_document(x, 2, use_cache=False)
    assert not np.array_equal(Z0, Z1) and not np.array_equal(l0, l1) and not np.array_equal(o0, o1)
    d = R.pdist_cosine_square(x[1:])
    assert np.unique(d[np.triu_indices(d.shape[0], 1)]).size < d.shape[0] * (d.shape[0] - 1) // 4      # exact ties
