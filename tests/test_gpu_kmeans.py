"""np_hip_kmeans (FastKMeans::train on the GPU) against a numpy restatement of its rules (include/nextplaid_hip.h):
nearest-centroid assignment with the lowest index on ties, means, re-initialisation from the seeded stream, the
subsample, the early stop, byte-identical reruns and the refused inputs.  Needs a real MI355X."""
import numpy as np
import pytest

import kmeans_restate as R

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu


def _blobs(n, k, d, seed, spread=0.05):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((k, d)).astype(np.float32)
    lab = rng.integers(0, k, n)
    x = mu[lab] + spread * rng.standard_normal((n, d)).astype(np.float32)
    return x.astype(np.float32), mu


def _check_assign(x, c, a):
    """every assignment is a nearest centroid within 1e-5 (|x|^2 + |c|^2), and equals numpy's argmin where the gap
    between the best two exceeds that"""
    D = R.sq_dist(x, c)
    scale = 1e-5 * ((x.astype(np.float64) ** 2).sum(1)[:, None] + (c.astype(np.float64) ** 2).sum(1)[None, :])
    best = D.min(1)
    got = D[np.arange(x.shape[0]), a]
    tol = scale[np.arange(x.shape[0]), a]
    assert np.all(got <= best + tol), "an assignment is not a nearest centroid"
    if c.shape[0] > 1:
        part = np.partition(D, 1, axis=1)
        gap = part[:, 1] - part[:, 0]
        ok = gap > scale.max(1)
        assert np.array_equal(a[ok], D.argmin(1)[ok])
        assert ok.mean() > 0.9


@pytest.mark.parametrize("d", [128, 96, 100, 4])
def test_one_iteration_from_init(d):
    x, mu = _blobs(20000, 64, d, seed=d)
    init = x[:64].copy()
    cen, asg, rep = npa.kmeans(x, 64, max_iters=1, init=init, seed=5, max_points_per_centroid=0, return_assign=True)
    assert rep["iterations"] == 1 and rep["n_points"] == x.shape[0]
    _check_assign(x, init, asg)
    for j in range(64):                          # means of the GPU-assigned points
        sel = asg == j
        if sel.any():
            assert np.allclose(cen[j], x[sel].astype(np.float64).mean(0), rtol=1e-6, atol=1e-7)


def test_duplicate_init_reinitialised_from_stream():
    x, _ = _blobs(5000, 16, 32, seed=3)
    init = x[:16].copy()
    init[9] = init[4]                            # equal distances: the lower index (4) wins, 9 stays empty
    cen, asg, rep = npa.kmeans(x, 16, max_iters=1, init=init, seed=1234, max_points_per_centroid=0, return_assign=True)
    assert not np.any(asg == 9) and rep["n_reinit"] >= 1
    empties = [j for j in range(16) if not np.any(asg == j)]
    g = R.SplitMix64(1234)
    for j in empties:                            # ascending cluster order, one draw each
        assert np.array_equal(cen[j], x[g.below(x.shape[0])])


def test_subsample_indices():
    x, _ = _blobs(3000, 4, 16, seed=11)
    k, mppc = 4, 100
    cen, asg, rep = npa.kmeans(x, k, max_iters=2, seed=77, max_points_per_centroid=mppc, return_assign=True)
    assert rep["n_points"] == k * mppc
    assert int((asg >= 0).sum()) == k * mppc
    g = R.SplitMix64(77)
    sub = R.partial_sample(g, x.shape[0], k * mppc)
    assert sorted(np.nonzero(asg >= 0)[0].tolist()) == sorted(sub)
    pick = R.partial_sample(g, k * mppc, k)      # init = subset[pick] drawn from the same stream
    c1, _ = npa.kmeans(x, k, max_iters=0, seed=77, max_points_per_centroid=mppc)
    assert np.array_equal(c1, x[[sub[p] for p in pick]])


def test_early_stop_at_the_means():
    rng = np.random.default_rng(5)
    mu = np.eye(8, 32, dtype=np.float32) * 10
    x = np.repeat(mu, 50, 0) + 0.01 * rng.standard_normal((400, 32)).astype(np.float32)
    lab = np.repeat(np.arange(8), 50)
    init = np.stack([x[lab == j].astype(np.float64).mean(0) for j in range(8)]).astype(np.float32)
    cen, asg, rep = npa.kmeans(x, 8, max_iters=10, init=init, return_assign=True)
    # the mean of the points is recomputed in fixed point: equal to the f64 mean rounded, so the shift is at most ulps
    assert rep["iterations"] <= 2 and np.array_equal(asg, lab)
    cen2, rep2 = npa.kmeans(x, 8, max_iters=10, init=cen)
    assert rep2["iterations"] == 1 and rep2["shift"] == 0.0 and np.array_equal(cen2, cen)


def test_deterministic_bytes():
    x, _ = _blobs(200_000, 512, 128, seed=21, spread=0.3)
    a1 = npa.kmeans(x, 512, max_iters=3, seed=9, return_assign=True)
    a2 = npa.kmeans(x, 512, max_iters=3, seed=9, return_assign=True)
    assert a1[0].tobytes() == a2[0].tobytes() and np.array_equal(a1[1], a2[1])
    assert a1[2]["shift"] == a2[2]["shift"]


def test_quality_matches_numpy_lloyd():
    x, _ = _blobs(30000, 100, 64, seed=8, spread=0.6)
    g = R.SplitMix64(3)
    pick = R.partial_sample(g, x.shape[0], 100)   # the GPU's own init draws (no subsample)
    init = x[pick]
    cen, rep = npa.kmeans(x, 100, max_iters=4, seed=3, max_points_per_centroid=0)
    ref, _ = R.lloyd(x, init, 4, g)
    gi, ri = R.inertia(x, cen), R.inertia(x, ref)
    assert abs(gi - ri) <= 0.005 * ri, (gi, ri)


def test_shapes_and_refusals():
    x, _ = _blobs(1000, 5, 24, seed=2)
    c, rep = npa.kmeans(x, 1, max_iters=2, max_points_per_centroid=0)
    assert np.allclose(c[0], x.astype(np.float64).mean(0), rtol=1e-6, atol=1e-7)
    y = x[:300]
    c, a, rep = npa.kmeans(y, 300, max_iters=1, seed=4, return_assign=True)   # k = n: every point its own centroid
    assert rep["n_points"] == 300
    _check_assign(y, y[R.partial_sample(R.SplitMix64(4), 300, 300)], a)
    with pytest.raises(npa.IndexCreationError, match="0 centroids"):
        npa.kmeans(x, 0)
    with pytest.raises(npa.IndexCreationError):
        npa.kmeans(x[:3], 4)
    with pytest.raises(npa.ShapeError):
        npa.kmeans(np.zeros((10, 129), np.float32), 2)
    bad = x.copy()
    bad[7, 3] = np.nan
    with pytest.raises(npa.IndexCreationError, match="finite"):
        npa.kmeans(bad, 4)
