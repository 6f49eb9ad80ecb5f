"""The expansion mode of the index update at its kernels' own edges: cases with their expected answers (test
infrastructure; host code only: numpy, the restatements and the oracle's encode, none of the product's code).

    outlier_cases()   documents for find_outliers (km_norm_kernel, one nearest_step, ol_flag_kernel, ol_recheck_kernel):
                      token recipes with a known membership, mixed per case, at K and dim with padded centroid tiles and
                      padded storage rows, with large norms, at threshold 0, with a recheck list fed from several blocks
                      and with 0, 1, 3 and 5 outliers
    second_case()     the same recipes around the centroids an earlier expansion left
    norm_cases()      n tokens c + r_i u_i of distinct radii, ordered so that the token whose residual norm IS the 0.75
                      quantile sits at a chosen position: the slices of encode_tokens_impl read out one token at a time

The recipes (thr2 = thr^2, d = min_c |x - c|^2):
    near      centroid + Gaussian noise of squared length ~ near_r2     not an outlier (an outlier at thr 0)
    far       3 x Gaussian                                               outlier
    edge      d = thr2 (1 +- 2e-6)                                       inside the window: the f64 recheck decides
    outside   d = thr2 (1 +- 1e-3)                                       the sign decides; at unit norms outside the window
    origin    |x| = 1e-3 and one all-zero row                            outliers (a zero-padded centroid slot would be at d ~ 0)
    on        exact copies of centroid rows                              d = 0: not an outlier, also at thr 0

n_rechecked is stated exactly.  With w the device's window restated in f64 (update_restate.outlier_window) and a = |d - thr2|
in f64, a case may hold no token with w/2 < a <= 2 w; then the tokens the f32 pass lists are those with a <= w/2, as long
as the f32 minimum lies within w/2 of d (tests/test_update_limits_cpu.py shows both on the restatement).
"""
from dataclasses import dataclass
from functools import cached_property

import numpy as np

import kmeans_restate as R
import update_restate as U
from oracle import oracle as O

F32, F64 = np.float32, np.float64
KMEANS_NITERS, SEED = 3, 11
SLICE = 64 * 32          # tokens per pass of encode_tokens_impl through the update's own codec handle (max_batch 64 x 32)


def unit_centroids(K, dim, seed, scale=1.0):
    g = np.random.default_rng(seed)
    c = g.standard_normal((K, dim))
    return (c / np.linalg.norm(c, axis=1, keepdims=True) * scale).astype(F32)


def bucket_tables(nbits):
    """(cutoffs, weights) of a codec: any ascending tables serve the update path"""
    return (np.linspace(-0.1, 0.1, (1 << nbits) - 1).astype(F32), np.linspace(-0.12, 0.12, 1 << nbits).astype(F32))


def base_index(cen, nbits, n_docs=200, seed=1):
    """Arrays of a small index around a centroid table: documents of 0..8 tokens next to centroids."""
    g = np.random.default_rng(seed)
    K, dim = cen.shape
    lens = g.integers(0, 9, n_docs).astype(np.int64) if n_docs > 1 else np.ones(1, np.int64)
    T = int(lens.sum())
    flat = (cen[g.integers(0, K, T)] + (0.02 / np.sqrt(dim)) * g.standard_normal((T, dim))).astype(F32)
    cut, wts = bucket_tables(nbits)
    codes, packed = O.encode_tokens(flat, cen, nbits, cut)
    return dict(centroids=cen, bucket_weights=wts, bucket_cutoffs=cut, doc_lengths=lens, codes=codes, residuals=packed,
                nbits=nbits)


def split_docs(g, flat, max_len):
    """Documents of uneven length 1..max_len, with one zero-length document in the middle."""
    docs, i = [], 0
    while i < flat.shape[0]:
        n = int(g.integers(1, max_len + 1))
        docs.append(np.ascontiguousarray(flat[i:i + n]))
        i += n
    docs.insert(len(docs) // 2, np.zeros((0, flat.shape[1]), F32))
    return docs


def _ortho_units(g, C):
    """one random unit vector per row of C (f64), orthogonal to that row"""
    u = g.standard_normal(C.shape)
    cc = (C * C).sum(1, keepdims=True)
    u -= np.where(cc > 0, (u * C).sum(1, keepdims=True) / np.where(cc > 0, cc, 1.0), 0.0) * C
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _around(g, cen, r2):
    """tokens at squared distance r2[i] from a random centroid each, offset orthogonally to it (built in f64)"""
    C = cen[g.integers(0, cen.shape[0], len(r2))].astype(F64)
    return (C + np.sqrt(np.asarray(r2, F64))[:, None] * _ortho_units(g, C)).astype(F32)


# ---- A. the outlier search ---------------------------------------------------------------------------------------------
RECIPES = ("near", "far", "edge", "outside", "origin", "on")


@dataclass
class OutlierCase:
    name: str
    centroids: np.ndarray
    nbits: int
    thr: np.float32
    docs: list
    labels: np.ndarray        # the recipe of every token
    expect: np.ndarray        # 1 outlier, 0 not, -1 the f64 recheck decides
    mppc: int = 256           # max_points_per_centroid
    n_base: int = 200
    base_seed: int = 1

    @cached_property
    def flat(self):
        dim = self.centroids.shape[1]
        return np.concatenate(self.docs, 0) if self.docs else np.zeros((0, dim), F32)

    @cached_property
    def thr2(self):
        return float(F32(self.thr) * F32(self.thr))

    @cached_property
    def d64(self):
        return U.min_dist_sq_f64(self.flat, self.centroids)

    @cached_property
    def w(self):
        return U.outlier_window(self.flat, self.centroids, self.thr)

    @cached_property
    def outliers(self):
        return U.find_outliers(self.flat, self.centroids, self.thr)

    @property
    def n_rechecked(self):
        return int((np.abs(self.d64 - self.thr2) <= self.w / 2).sum())

    def band(self):
        """tokens inside (w/2, 2w] of thr2: a case may have none"""
        a = np.abs(self.d64 - self.thr2)
        return np.nonzero((a > self.w / 2) & (a <= 2 * self.w))[0]


def recipe_rows(g, cen, thr, counts, near_r2):
    """(tokens, labels, expect) of the recipes in `counts`, recipe by recipe"""
    K, dim = cen.shape
    thr2 = float(thr) ** 2
    rows, labels, expect = [], [], []

    def add(x, label, e):
        rows.append(np.asarray(x, F32).reshape(-1, dim))
        labels.extend([label] * rows[-1].shape[0])
        expect.extend(np.broadcast_to(e, rows[-1].shape[0]).tolist())
    for label in RECIPES:
        n = counts.get(label, 0)
        if n == 0:
            continue
        if label == "near":
            x = cen[g.integers(0, K, n)] + np.sqrt(near_r2 / dim) * g.standard_normal((n, dim))
            add(x, label, 0 if near_r2 < thr2 else 1)
        elif label == "far":
            add(3 * g.standard_normal((n, dim)), label, 1)
        elif label == "edge":
            s = np.where(np.arange(n) % 2 == 1, 1.0, -1.0)
            add(_around(g, cen, thr2 * (1 + 2e-6 * s)), label, -1)
        elif label == "outside":
            s = np.where(np.arange(n) % 2 == 1, 1.0, -1.0)
            add(_around(g, cen, thr2 * (1 + 1e-3 * s)), label, (s > 0).astype(int))
        elif label == "origin":
            x = g.standard_normal((n, dim))
            x = 1e-3 * x / np.linalg.norm(x, axis=1, keepdims=True)
            x[-1] = 0.0
            add(x, label, 1)
        elif label == "on":
            add(cen[g.integers(0, K, n)].copy(), label, 0)
    return np.concatenate(rows), np.array(labels), np.array(expect, np.int8)


def outlier_case(name, cen, nbits, thr, counts, seed, mppc=256, near_r2=None, max_len=9):
    g = np.random.default_rng(seed)
    thr = F32(thr)
    if near_r2 is None:
        near_r2 = 0.01 * float(thr) ** 2
    x, labels, expect = recipe_rows(g, cen, thr, counts, near_r2)
    perm = g.permutation(x.shape[0])                 # every recipe in every block of 256 tokens
    x, labels, expect = x[perm], labels[perm], expect[perm]
    docs = split_docs(g, x, max_len)
    return OutlierCase(name, cen, nbits, thr, docs, labels, expect, mppc)


MIX = dict(near=60, far=8, edge=24, outside=16, origin=6, on=6)
# (K, dim, nbits, thr, max_points_per_centroid).  thr 0.5 at the storage dims 96 and 128: the "outside" tokens, thr2 1e-3 from
# the threshold, must clear 2 w, and w grows with the storage dim (1.4e-4 at 128 against 9e-5 for thr 0.3)
GEOMETRIES = ((1, 32, 2, 0.3, 256), (31, 48, 4, 0.3, 1), (33, 64, 2, 0.3, 256), (255, 96, 4, 0.5, 256), (257, 100, 2, 0.5, 256),
              (300, 128, 4, 0.5, 256))
COUNTS = ((0, 256), (1, 1), (3, 256), (5, 256), (5, 1))       # (outliers, max_points_per_centroid)


def second_case(cen_after, thr_after, nbits=2):
    """The recipes around the centroids a first expansion of the (33, 64) case left: K = 33 + k_update, so the last tile
    holds real centroids next to padding.  Only the band condition is stated for it (the new centroids are k-means')."""
    return outlier_case(f"second-K{cen_after.shape[0]}-d{cen_after.shape[1]}", cen_after, nbits, thr_after, MIX, 4242)


def _build_outlier_cases():
    out = []
    for i, (K, dim, nbits, thr, mppc) in enumerate(GEOMETRIES):
        out.append(outlier_case(f"mix-K{K}-d{dim}b{nbits}", unit_centroids(K, dim, 100 + i), nbits, thr, MIX, 200 + i, mppc))
    # norm 25: the f32 pass misplaces planted tokens that lie outside the crate's 1e-5 window; only the second term of w
    # sends them to the recheck
    for dim in (64, 128):
        out.append(outlier_case(f"large-K33-d{dim}", unit_centroids(33, dim, 300 + dim, 25.0), 4, 0.3,
                                dict(outside=400, near=40, far=6), 310 + dim))
    out.append(outlier_case("thr0-K33-d64", unit_centroids(33, 64, 320), 2, 0.0, dict(on=12, near=40, far=4), 321, near_r2=1e-2))
    out.append(outlier_case("list-K31-d48", unit_centroids(31, 48, 330), 4, 0.3, dict(edge=720, near=60, far=8), 331, max_len=24))
    for n_out, mppc in COUNTS:
        out.append(outlier_case(f"count{n_out}-mppc{mppc}", unit_centroids(33, 64, 340), 2, 0.3, dict(near=50, far=n_out),
                                341 + n_out, mppc))
    cen = unit_centroids(33, 64, 350)
    g = np.random.default_rng(351)
    out.append(OutlierCase("single-token", cen, 2, F32(0.3), [(3 * g.standard_normal((1, 64))).astype(F32)], np.array(["far"]),
                           np.array([1], np.int8)))
    out.append(OutlierCase("all-empty", cen, 2, F32(0.3), [np.zeros((0, 64), F32)] * 3, np.zeros(0, "<U4"), np.zeros(0, np.int8)))
    return out


# ---- B. the residual norms through the threshold -----------------------------------------------------------------------
@dataclass
class NormCase:
    name: str
    centroids: np.ndarray
    nbits: int
    docs: list
    probes: tuple             # positions of the tokens that decide the quantile (one for odd 0.75 (n - 1), else two)
    ranks: np.ndarray         # rank of every token's radius
    old_thr: float = None     # None: cluster_threshold.npy is deleted before the update
    n_base: int = 200

    @cached_property
    def flat(self):
        return np.concatenate(self.docs, 0)

    @cached_property
    def codes(self):
        return O.encode_tokens(self.flat, self.centroids, self.nbits, bucket_tables(self.nbits)[0])[0]

    @cached_property
    def norms(self):
        return U.residual_norms(self.flat, self.centroids, self.codes)

    @property
    def quantile(self):
        return R.quantile(np.sort(self.norms), 0.75)


def norm_case(name, K, dim, nbits, n, probes, seed, old_thr=None, n_base=200):
    """n tokens c + r u with radii 0.05 .. 0.30 in n distinct steps (1.2e-4 apart at n = 2081, far above the f32 error of a
    norm), in random order except that the tokens whose ranks are floor and ceil of 0.75 (n - 1) sit at `probes`."""
    g = np.random.default_rng(seed)
    cen = unit_centroids(K, dim, seed + 1)
    idx = 0.75 * (n - 1)
    want = sorted({int(np.floor(idx)), int(np.ceil(idx))})
    assert len(want) == len(probes)
    ranks = g.permutation(n)
    for pos, rk in zip(probes, want):
        j = int(np.nonzero(ranks == rk)[0][0])
        ranks[j], ranks[pos] = ranks[pos], ranks[j]
    radii = 0.05 + 0.25 * (ranks + 0.5) / n
    x = _around(g, cen, radii ** 2)
    return NormCase(name, cen, nbits, split_docs(g, x, 40), tuple(probes), ranks, old_thr, n_base)


N_ODD, N_EVEN = 2081, 2082      # 2081 = 4 * 520 + 1: slice 1 full, slice 2 = one group of 32 and a ragged group of one token
NORM_GEOMETRIES = ((64, 32, 2), (65, 100, 4))
PROBES = (0, 31, 32, SLICE - 1, SLICE, N_ODD - 1)


def _build_norm_cases():
    out = []
    for gi, (K, dim, nbits) in enumerate(NORM_GEOMETRIES):
        for pi, p in enumerate(PROBES):
            out.append(norm_case(f"p{p}-K{K}-d{dim}b{nbits}", K, dim, nbits, N_ODD, (p,), 500 + 10 * gi + pi))
    out.append(norm_case("even-K65-d100b4", 65, 100, 4, N_EVEN, (SLICE - 1, SLICE), 540))
    # the threshold file present (far above every distance: no outliers, the codec stays) over a one-token index: the blend
    out.append(norm_case("blend-K64-d32b2", 64, 32, 2, N_ODD, (SLICE,), 550, old_thr=4.0, n_base=1))
    return out


_cache = {}


def outlier_cases():
    if "a" not in _cache:
        _cache["a"] = _build_outlier_cases()
    return _cache["a"]


def norm_cases():
    if "b" not in _cache:
        _cache["b"] = _build_norm_cases()
    return _cache["b"]
