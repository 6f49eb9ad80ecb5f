"""np_hip_kmeans bit for bit against the rules of include/nextplaid_hip.h: the assignment of every point equals the
oracle's po_kmeans_assign (k-ordered f32 FMA chains, lowest index on ties) at every storage width, across centroid
tiles and chunks; each mean is within 1 ulp of the exact mean plus a quantisation term of the cluster's own points;
re-initialisation, shift, stopping and the centroid ping-pong follow the stated rules; power-of-two scaling is exact;
the magnitude bound keeps every distance finite.  Needs a real MI355X."""
import math

import numpy as np
import pytest

import kmeans_restate as R
from oracle import oracle as O

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


def _km1(x, init, seed=0, **kw):
    """one Lloyd iteration from init, no subsample: (centroids, assignment, report)"""
    return npa.kmeans(x, init.shape[0], max_iters=kw.pop("max_iters", 1), init=init, seed=seed,
                      max_points_per_centroid=kw.pop("max_points_per_centroid", 0), return_assign=True, **kw)


def _assert_assign_exact(x, c, a):
    """a == the oracle's rule for every point; then, independently, every assignment is nearest in f64 within the f32
    error bound, and equals the f64 argmin wherever the gap between the best two exceeds that bound."""
    ref, dist = O.kmeans_assign(x, c)
    assert np.all(np.isfinite(dist))
    bad = np.nonzero(a != ref)[0]
    if bad.size:
        i = int(bad[0])
        D = R.sq_dist(x[i:i + 1], c)[0]
        o = np.argsort(D)
        pytest.fail(f"{bad.size} of {x.shape[0]} points differ from the f32 rule (n={x.shape[0]} k={c.shape[0]} "
                    f"d={x.shape[1]}); first: point {i} gpu {a[i]} rule {ref[i]}, f64 best {o[0]} gap "
                    f"{D[o[1]] - D[o[0]] if o.size > 1 else 0:.3e}, f64 dist gpu {D[a[i]]:.9e} rule {D[ref[i]]:.9e}")
    d = x.shape[1]
    cn = (c.astype(np.float64) ** 2).sum(1)
    for r0 in range(0, x.shape[0], 8192):
        xs = x[r0:r0 + 8192]
        D = R.sq_dist(xs, c)
        tol = (d + 3) * 2.0 ** -23 * ((xs.astype(np.float64) ** 2).sum(1)[:, None] + cn[None, :])
        rows = np.arange(xs.shape[0])
        aa, best = a[r0:r0 + 8192], D.argmin(1)
        assert np.all(D[rows, aa] <= D[rows, best] + tol[rows, aa] + tol[rows, best])
        if c.shape[0] > 1:
            part = np.partition(D, 1, axis=1)
            ok = part[:, 1] - part[:, 0] > 2 * tol.max(1)
            assert np.array_equal(aa[ok], best[ok])


def _ulp(v):
    """f32 ulp of the exact value v (f64): 2^(floor(log2 |v|) - 23), subnormal spacing at the bottom"""
    _, e = np.frexp(np.abs(v))
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def _assert_means_exact(x, a, cen):
    """every non-empty cluster c: |gpu - exact| <= ulp(exact) + 2 max_c|x| count_c 2^-62 (the quantisation of a
    fixed-point sum scaled by the cluster's own max |x| and size); exact = fsum of the f64 values / count"""
    order = np.argsort(a, kind="stable")
    xs, as_ = x[order].astype(np.float64), a[order]
    worst, n_bad = None, 0
    cuts = np.flatnonzero(np.diff(as_)) + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [as_.size]])
    for b, e in zip(starts, ends):
        c, blk = int(as_[b]), xs[b:e]
        exact = np.array([math.fsum(col) for col in blk.T]) / (e - b)
        quant = 2.0 * np.abs(blk).max() * (e - b) * 2.0 ** -62
        err = np.abs(cen[c].astype(np.float64) - exact)
        lim = _ulp(exact) + quant
        if np.any(err > lim):
            n_bad += int((err > lim).sum())
            j = int(np.argmax(err / lim))
            u = err[j] / _ulp(exact)[j]
            if worst is None or u > worst[0]:
                worst = (u, f"cluster {c} ({e - b} points) dim {j}: gpu {cen[c][j]!r} exact {exact[j]!r}")
    if worst:
        pytest.fail(f"{n_bad} mean components over the bound; worst {worst[0]:.1f} ulp: {worst[1]}")


def _blobs(n, k, d, seed, spread=0.3, scale=1.0):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((k, d))
    x = mu[rng.integers(0, k, n)] + spread * rng.standard_normal((n, d))
    return (scale * x).astype(np.float32)


# (d, k, n): every storage width Dp (32, 64, 96, 128) with and without zero padding; k from 1 to > 1000; n below 64 and
# not multiples of 64 or 256; small n with many tiles (many centroid chunks), n >= 130 817 (one chunk of several tiles)
CASES = [(1, 2, 37), (1, 257, 3001), (8, 31, 63), (8, 1000, 1777), (31, 33, 1000), (31, 1, 50), (32, 32, 4097),
         (32, 1031, 10_001), (33, 257, 513), (33, 2, 20_000), (48, 300, 200_003), (48, 31, 255), (64, 33, 2049),
         (64, 1000, 5000), (65, 257, 1500), (65, 1, 9), (96, 1031, 3000), (96, 2, 61), (100, 31, 8191),
         (100, 257, 40_000), (127, 32, 129), (127, 1000, 2500), (128, 1031, 1100), (128, 33, 131_071)]


@pytest.mark.parametrize("d,k,n", CASES)
def test_assign_bit_exact(d, k, n):
    i = CASES.index((d, k, n))
    x = _blobs(n, min(k, 64), d, seed=i, spread=0.5, scale=(1.0, 1e-3, 1e3)[i % 3])
    init = x[np.random.default_rng(100 + i).choice(n, k, replace=False)].copy()
    init[k // 2] += np.float32(0.25 * (1.0, 1e-3, 1e3)[i % 3])     # one centroid that is no data point
    cen, a, rep = _km1(x, init)
    assert rep["iterations"] == 1 and rep["n_points"] == n
    _assert_assign_exact(x, init, a)
    _assert_means_exact(x, a, cen)


@pytest.mark.parametrize("n", [1100, 5000])
def test_ties_across_tiles_and_chunks(n):
    """n = 1100: one tile per chunk (33 chunks); n = 5000: 17 chunks of 2 tiles, the last (tile 32, index 1030) with
    half the work, so the chunk of the higher duplicate tends to finish first.  The lower index must win every tie."""
    d, k = 64, 1040
    rng = np.random.default_rng(n)
    c = rng.standard_normal((k, d)).astype(np.float32)
    pairs = [(3, 1030), (40, 75), (33, 34), (5, 517), (64, 1039)]
    for j, jj in pairs:
        c[jj] = c[j]
    lo = np.array([p[0] for p in pairs])
    x = (c[lo[rng.integers(0, lo.size, n)]] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    x[: lo.size] = c[lo]                                       # exact hits: distance 0 to both of a pair
    _, a, _ = _km1(x, c)
    _assert_assign_exact(x, c, a)
    assert not np.isin(a, [p[1] for p in pairs]).any()
    assert np.array_equal(a[: lo.size], lo)


def test_degenerate_inputs():
    rng = np.random.default_rng(4)
    v = rng.standard_normal(48).astype(np.float32)
    x = np.repeat(v[None], 1000, 0)                            # every point identical, every centroid identical
    cen, a, rep = _km1(x, x[:40].copy(), seed=17)
    assert np.all(a == 0) and np.array_equal(cen[0], v)
    assert rep["n_reinit"] == 39 and all(np.array_equal(r, v) for r in cen[1:])
    z = np.zeros((300, 48), np.float32)                        # zero points: the argmin of |c|^2, lowest index on ties
    init = rng.standard_normal((70, 48)).astype(np.float32)
    init[50] = init[int((init.astype(np.float64) ** 2).sum(1).argmin())]   # equal |c|^2 at two indices
    cen, a, _ = _km1(z, init)
    _assert_assign_exact(z, init, a)
    assert np.all(cen[a[0]] == 0)
    cen, a, _ = _km1(z, np.zeros((33, 48), np.float32))
    assert np.all(a == 0) and np.all(cen == 0)
    y = rng.standard_normal((300, 33)).astype(np.float32)      # k = n: every point its own centroid
    cen, a, rep = _km1(y, y.copy())
    _assert_assign_exact(y, y, a)
    assert np.array_equal(a, np.arange(300)) and np.array_equal(cen, y) and rep["shift"] == 0.0


@pytest.mark.parametrize("d,n,k", [(128, 20_000, 64), (64, 12_345, 100), (31, 5000, 40), (96, 7000, 33)])
def test_means_within_one_ulp(d, n, k):
    x = _blobs(n, k, d, seed=d, spread=0.4)
    x[:: 7] *= -3                                              # mixed signs and magnitudes inside clusters
    init = x[np.random.default_rng(d).choice(n, k, replace=False)].copy()
    cen, a, _ = _km1(x, init)
    _assert_assign_exact(x, init, a)
    _assert_means_exact(x, a, cen)


@pytest.mark.parametrize("outlier", [2.0 ** 20, 2.0 ** 12])
def test_means_do_not_depend_on_other_clusters(outlier):
    """64 clusters x 300 points, d = 32, values near N(0, 0.1^2), one value of 2^20 (2^12) in one point: a scale shared
    by all clusters quantised every mean on the outlier's scale (thousands of ulps off for the means near 0)."""
    rng = np.random.default_rng(64)
    mu = 0.1 * rng.standard_normal((64, 32))
    x = (np.repeat(mu, 300, 0) + 0.1 * rng.standard_normal((64 * 300, 32))).astype(np.float32)
    x[0, 5] = outlier
    init = mu.astype(np.float32)
    cen, a, _ = _km1(x, init)
    _assert_assign_exact(x, init, a)
    _assert_means_exact(x, a, cen)


@pytest.mark.parametrize("sub", [False, True])
def test_reinit_from_the_stream(sub):
    """empty clusters take x[subset[below(m)]] in ascending cluster order, after the subsample draws"""
    n, k, d, seed = (20_000 if sub else 3000), 70, 40, 2024
    x = _blobs(n, 20, d, seed=5)
    init = x[np.random.default_rng(6).choice(n, k, replace=False)].copy()
    init[50], init[65], init[20] = init[2], init[60], 1e3       # 50, 65 lose their ties; 20 is far from everything
    mppc = 50 if sub else 0
    cen, a, rep = _km1(x, init, seed=seed, max_points_per_centroid=mppc)
    g = R.SplitMix64(seed)
    m = k * mppc if sub else n
    rows = R.partial_sample(g, n, m) if sub else list(range(n))
    assert rep["n_points"] == m
    if sub:
        outside = np.ones(n, bool)
        outside[rows] = False
        assert np.all(a[outside] == -1)
    asub = a[rows]
    _assert_assign_exact(x[rows], init, asub)
    empties = [j for j in range(k) if not np.any(asub == j)]
    assert {20, 50, 65} <= set(empties) and rep["n_reinit"] == len(empties)
    for j in empties:
        assert np.array_equal(cen[j], x[rows[g.below(m)]]), f"cluster {j}"
    full = np.array([j not in empties for j in range(k)])
    sel = np.isin(a, np.nonzero(full)[0])
    _assert_means_exact(x[sel], a[sel], cen)


def test_shift_stopping_and_ping_pong():
    d, k = 64, 24
    x = np.random.default_rng(9).standard_normal((6000, d)).astype(np.float32)   # no clusters: every step moves
    init = x[:k].copy()
    chain, shifts = [init], []
    for _ in range(4):                                         # four chained single iterations
        c, _, rep = _km1(x, chain[-1], tol=0.0)
        assert rep["n_reinit"] == 0
        parts = O.kmeans_shift_parts(chain[-1], c)
        assert abs(rep["shift"] - math.fsum(parts.astype(np.float64))) <= 1e-12 * rep["shift"]
        chain.append(c)
        shifts.append(rep["shift"])
    assert min(shifts) > 0
    c4, rep = npa.kmeans(x, k, max_iters=4, tol=0.0, init=init, max_points_per_centroid=0)
    assert rep["iterations"] == 4 and c4.tobytes() == chain[4].tobytes() and rep["shift"] == shifts[3]
    for tol in (shifts[1], np.nextafter(shifts[1], np.inf), shifts[0] * 2, 0.0):
        stop = next((i + 1 for i, s in enumerate(shifts) if s < tol), 4)
        c, rep = npa.kmeans(x, k, max_iters=4, tol=float(tol), init=init, max_points_per_centroid=0)
        assert rep["iterations"] == stop and c.tobytes() == chain[stop].tobytes() and rep["shift"] == shifts[stop - 1]


@pytest.mark.parametrize("s", [30, -30])
def test_power_of_two_scaling_is_exact(s):
    """|x_j| in [0.5, 2): every product, sum and mean stays a normal f32 at 2^+-30, so scaling is exact"""
    rng = np.random.default_rng(30)
    x = (rng.choice([-1.0, 1.0], (5000, 48)) * rng.uniform(0.5, 2.0, (5000, 48))).astype(np.float32)
    init = x[rng.choice(5000, 40, replace=False)].copy()
    c0, a0, _ = _km1(x, init, max_iters=2)
    f = np.float32(2.0 ** s)
    c1, a1, _ = _km1(x * f, init * f, max_iters=2)
    assert np.array_equal(a0, a1)
    assert (c0 * f).tobytes() == c1.tobytes()


@pytest.mark.parametrize("d", [128, 100, 8])
def test_magnitude_limit(d):
    bound = min(1e18, math.sqrt(0.999 * FLT_MAX / (4 * d)))
    under = np.float32(bound)
    if float(under) > bound:
        under = np.nextafter(under, np.float32(0))
    rng = np.random.default_rng(d)
    x = (rng.choice([-1.0, 1.0], (300, d)) * under).astype(np.float32)
    x[:: 3] *= np.float32(0.5)
    init = np.concatenate([x[:20], -x[20:40]])                 # antipodal centroids: distances up to 4 d bound^2
    cen, a, _ = _km1(x, init)
    _assert_assign_exact(x, init, a)
    assert np.all(np.isfinite(cen))
    over = np.nextafter(np.float32(bound), np.float32(np.inf)) * np.float32(1.001)
    for bad_x, bad_c in ((x * (over / under), init), (x, init * (over / under))):
        with pytest.raises(npa.IndexCreationError, match="overflow"):
            _km1(bad_x.astype(np.float32), bad_c.astype(np.float32))
