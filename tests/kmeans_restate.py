"""numpy restatement of the index-creation rules of include/nextplaid_hip.h (test infrastructure): the SplitMix64 stream,
the document shuffle, the point subsample / init, Lloyd's iteration and the codec statistics of index.rs:182-287."""
import math

import numpy as np

M64 = (1 << 64) - 1


class SplitMix64:
    def __init__(self, seed):
        self.s = int(seed) & M64

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def below(self, b):
        thr = ((1 << 64) - b) % b
        while True:
            r = self.next()
            if r >= thr:
                return r % b


def shuffled_docs(n, seed):
    a = list(range(n))
    g = SplitMix64(seed)
    for i in range(n - 1, 0, -1):
        j = g.below(i + 1)
        a[i], a[j] = a[j], a[i]
    return a


def partial_sample(g, n, m):
    a = list(range(n))
    for i in range(m):
        j = i + g.below(n - i)
        a[i], a[j] = a[j], a[i]
    return a[:m]


def n_samples(N, given=None):
    """kmeans.rs:273-277"""
    return min(given if given else int(min(1.0 + 16.0 * math.sqrt(120.0 * N), N)), N)


def codec_samples(N):
    """index.rs:199-201"""
    return max(1, min(N, int(16.0 * math.sqrt(120.0 * N))))


def quantile(sorted_vals, q):
    """utils.rs:94-149 on an already sorted f32 array."""
    n = sorted_vals.size
    if n == 0:
        return np.float32(0)
    idx = q * (n - 1)
    lo, hi = math.floor(idx), math.ceil(idx)
    if lo == hi:
        return sorted_vals[lo]
    w = np.float32(idx - lo)
    return np.float32(np.float32(sorted_vals[lo] * (np.float32(1) - w)) + np.float32(sorted_vals[hi] * w))


def sq_dist(x, c):
    """f64 squared distances [n, k]."""
    x = x.astype(np.float64)
    c = c.astype(np.float64)
    return np.maximum((x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * x @ c.T, 0.0)


def lloyd(x, init, iters, g, tol=1e-8):
    """f64 Lloyd from a given init, empty clusters re-initialised from the stream g (no subsample).
    Returns (centroids f64, last assignment)."""
    c = init.astype(np.float64).copy()
    a = None
    for _ in range(iters):
        a = sq_dist(x, c).argmin(1)
        new = c.copy()
        for j in range(c.shape[0]):
            sel = a == j
            new[j] = x[sel].astype(np.float64).mean(0) if sel.any() else x[g.below(x.shape[0])]
        shift = np.linalg.norm(new - c, axis=1).sum()
        c = new
        if shift < tol:
            break
    return c, a


def inertia(x, c):
    return sq_dist(x, c).min(1).sum()
