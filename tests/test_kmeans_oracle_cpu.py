"""The k-means reference of the oracle (po_kmeans_assign, po_kmeans_shift_parts), checked without a device: against an
exact rational restatement of the f32 FMA rule, against the f64 argmin where the f32 error cannot decide, and on
hand-built ties (equal and clamped-to-zero distances go to the lowest index).  The GPU k-means is compared with this
reference bit for bit in test_gpu_kmeans_exact.py."""
from fractions import Fraction as F

import numpy as np
import pytest

from oracle import oracle as O


def _f32_round(q):
    """q (a Fraction) rounded to the nearest f32, ties to even (normal and subnormal range)."""
    if q == 0:
        return 0.0
    s, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    while F(2) ** e > q:
        e -= 1
    while F(2) ** (e + 1) <= q:
        e += 1
    ulp = F(2) ** (max(e, -126) - 23)
    m = q / ulp
    n = m.numerator // m.denominator
    r = m - n
    if r > F(1, 2) or (r == F(1, 2) and n % 2):
        n += 1
    return s * float(n * ulp)


def _fmaf(a, b, c):
    return _f32_round(F(float(a)) * F(float(b)) + F(float(c)))


def _chain(a, b):
    s = 0.0
    for u, v in zip(a, b):
        s = _fmaf(u, v, s)
    return s


def _assign_exact(x, c):
    """the assign rule of include/nextplaid_hip.h evaluated with exact rationals and one rounding per f32 operation"""
    cn = [_chain(r, r) for r in c]
    out_a, out_d = [], []
    for p in x:
        xn = _chain(p, p)
        best, bd = 0, None
        for j, r in enumerate(c):
            d = max(_f32_round(F(-2) * F(_chain(p, r)) + F(_f32_round(F(xn) + F(cn[j])))), 0.0)
            if bd is None or d < bd:
                best, bd = j, d
        out_a.append(best)
        out_d.append(bd)
    return np.array(out_a), np.array(out_d, np.float32)


def _f64_dist(x, c):
    x, c = x.astype(np.float64), c.astype(np.float64)
    return ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1)


def _f32_bound(x, c):
    """|f32 rule - exact distance| <= (d + 3) 2^-23 (|x|^2 + |c|^2): two norm chains, the dot chain, the add and the fma"""
    d = x.shape[1]
    nx = (x.astype(np.float64) ** 2).sum(1)
    nc = (c.astype(np.float64) ** 2).sum(1)
    return (d + 3) * 2.0 ** -23 * (nx[:, None] + nc[None, :])


@pytest.mark.parametrize("n,k,d,seed", [(7, 5, 1, 0), (9, 6, 3, 1), (6, 9, 33, 2), (5, 4, 17, 3)])
def test_assign_is_the_stated_f32_rule(n, k, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    c = rng.standard_normal((k, d)).astype(np.float32)
    c[k - 1] = x[0]                                     # one exact hit: distance 0
    a, dist = O.kmeans_assign(x, c)
    ea, ed = _assign_exact(x, c)
    assert np.array_equal(a, ea)
    assert np.array_equal(dist.view(np.uint32), ed.view(np.uint32))
    assert dist[0] == 0


@pytest.mark.parametrize("d", [1, 8, 64, 128])
def test_assign_agrees_with_f64_where_the_gap_decides(d):
    rng = np.random.default_rng(d)
    k = 40
    c = rng.standard_normal((k, d)).astype(np.float32)
    x = (c[rng.integers(0, k, 3000)] + 0.7 * rng.standard_normal((3000, d))).astype(np.float32)
    a, dist = O.kmeans_assign(x, c)
    D = _f64_dist(x, c)
    tol = _f32_bound(x, c)
    rows = np.arange(x.shape[0])
    best = D.argmin(1)
    assert np.all(np.abs(dist.astype(np.float64) - D[rows, a]) <= tol[rows, a])
    assert np.all(D[rows, a] <= D[rows, best] + tol[rows, a] + tol[rows, best])
    part = np.partition(D, 1, axis=1)
    decided = part[:, 1] - part[:, 0] > 2 * tol.max(1)
    assert decided.mean() > 0.9
    assert np.array_equal(a[decided], best[decided])


def test_equal_distances_go_to_the_lowest_index():
    rng = np.random.default_rng(7)
    d, k = 24, 70
    c = rng.standard_normal((k, d)).astype(np.float32)
    for j in (17, 40, 69):                              # duplicates of centroid 3 at higher indices
        c[j] = c[3]
    x = (c[3] + 0.01 * rng.standard_normal((50, d))).astype(np.float32)
    a, _ = O.kmeans_assign(x, c)
    assert np.all(a == 3)
    # a zero point is |c|^2 from every centroid: unit basis vectors (and their negatives) tie everywhere -> index 0
    e = np.concatenate([np.eye(d, dtype=np.float32), -np.eye(d, dtype=np.float32)])
    a, dist = O.kmeans_assign(np.zeros((4, d), np.float32), e)
    assert np.all(a == 0) and np.all(dist == 1)
    # every point identical, every centroid identical: distance 0 everywhere -> index 0
    a, dist = O.kmeans_assign(np.repeat(x[:1], 9, 0), np.repeat(x[:1], 5, 0))
    assert np.all(a == 0) and np.all(dist == 0)


def test_clamped_distances_tie_at_the_lowest_index():
    """A centroid 1 ulp from x has a true distance far below the f32 cancellation error; where its computed distance
    is negative it clamps to 0 and ties with x itself (computed exactly 0): the lower index wins, not the true nearest."""
    rng = np.random.default_rng(11)
    d = 16
    found = 0
    for _ in range(200):
        x = (100 * rng.standard_normal(d)).astype(np.float32)
        near = x.copy()
        j = rng.integers(0, d)
        near[j] = np.nextafter(near[j], np.float32(np.inf))
        raw = _f32_round(F(-2) * F(_chain(x, near)) + F(_f32_round(F(_chain(x, x)) + F(_chain(near, near)))))
        if raw > 0:
            continue
        c = np.stack([x + 1000, near, x]).astype(np.float32)
        a, dist = O.kmeans_assign(x[None], c)
        assert a[0] == 1 and dist[0] == 0
        a, dist = O.kmeans_assign(x[None], c[[0, 2, 1]])
        assert a[0] == 1 and dist[0] == 0
        found += 1
    assert found >= 20


def test_shift_parts():
    rng = np.random.default_rng(5)
    old = rng.standard_normal((6, 19)).astype(np.float32)
    new = (old + rng.standard_normal((6, 19)) * np.array([0, 1e-3, 1, 10, 1e-7, 3])[:, None]).astype(np.float32)
    p = O.kmeans_shift_parts(old, new)
    for c in range(6):
        df = (new[c] - old[c]).astype(np.float32)
        s = _chain(df, df)
        assert p[c] == np.sqrt(np.float32(s))
    assert p[0] == 0
    assert np.allclose(p, np.linalg.norm(new.astype(np.float64) - old, axis=1), rtol=1e-5)
