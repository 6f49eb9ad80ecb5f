"""decompress_documents (codec.rs:423-470, index.rs:1197-1245) at decompress_kernel's edges: small hand-made indexes
with rows whose norm is exactly 0, tiny and huge (test infrastructure; numpy only: imports neither the package nor the
oracle).

Every index has six centroids and the bucket weights w[0] = 0.0, w[1] = 2^-3, further dyadic values after them:
    rows 0..2   random unit vectors: the generic rows, with random buckets
    row 3       -2^-3 in every component: with bucket 1 everywhere the sum is exactly 0, the norm clamp max(norm, 1e-12)
                applies and the output row is 0
    row 4       components of about 1e-20 (bucket 0): the squares underflow in f32; the norm is below the clamp
    row 5       components of about 5e17 (bucket 0): the squares are near 1e35, their sum stays finite
Documents: generic, EMPTY, the zero row alone, (tiny, generic, huge), 70 generic tokens (18 blocks of four waves), and
as the last document (generic, zero row).  REQUEST asks for them with an id past the end, a far one and a negative one,
each of length 0 (index.rs:1202-1204).

The error bounds (relative, per component, against float64; u = 2^-24, m = ceil(dim / 64) terms per lane):
  the kernel   x = f32(c + w)                                  u
               x * x, accumulated: counted as NOT contracted   2 u (x twice) + u (product) + m u (the lane's additions)
               six shuffle additions                           6 u             -> the sum of squares (all terms >= 0): (m + 9) u
               the square root halves that                     (m + 9) / 2 u
               sqrtf at 1 ulp, the divide at 2.5 ulp           2 u + 5 u
      E_GPU = (m + 9) / 2 + 8.  hipcc's default is an IEEE divide and square root (u each); the bound does not lean on a
      compiler default and counts the figures that hold without it.
  the oracle   unrolled_dot: a term passes floor(dim / 8) additions of its partial sum, one pairing, at most four
               additions into the total and dim % 8 tail additions; IEEE sqrtf and divide:
      E_CPU = 1 + (3 + floor(dim / 8) + 5 + dim % 8) / 2 + 2
Both are multiplied by 1 + 2^-10 for the products of two error terms.
"""
import numpy as np

import encode_limit_shapes as E

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
GEOMETRIES = [(dim, nbits) for nbits in (1, 2, 4, 8) for dim in (8, 96, 100, 128) if dim * nbits % 8 == 0]
ZERO_ROW, TINY_ROW, HUGE_ROW = 3, 4, 5
REQUEST = np.array([0, 1, 2, 3, 4, 5, 6, 10 ** 6, -1], np.int64)
LENGTHS = np.array([3, 0, 1, 3, 70, 2], np.int64)


def e_gpu(dim):
    return ((-(-dim // 64) + 9) / 2 + 8) * (1 + 2.0 ** -10)


def e_cpu(dim):
    return (1 + (3 + dim // 8 + 5 + dim % 8) / 2 + 2) * (1 + 2.0 ** -10)


def make_index(dim, nbits):
    """(index arrays, kind per token): kind is "generic", "zero", "tiny" or "huge"."""
    g = np.random.default_rng(9600 + 10 * dim + nbits)
    nb = 1 << nbits
    w = np.zeros(nb, F32)
    w[1] = 0.125
    w[2:] = ((np.arange(2, nb) * 37) % 64 - 32) / 256.0
    cen = g.standard_normal((6, dim)).astype(F32)
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    v = g.choice([1.0, -1.0, 0.5, -0.5], dim).astype(F32)
    cen[ZERO_ROW], cen[TINY_ROW], cen[HUGE_ROW] = -0.125, F32(1e-20) * v, F32(5e17) * v
    kinds = (["generic"] * 3 + ["zero"] + ["tiny", "generic", "huge"] + ["generic"] * 70 + ["generic", "zero"])
    T = len(kinds)
    codes = g.integers(0, 3, T)
    bk = g.integers(0, nb, (T, dim))
    for t, k in enumerate(kinds):
        if k != "generic":
            codes[t] = {"zero": ZERO_ROW, "tiny": TINY_ROW, "huge": HUGE_ROW}[k]
            bk[t] = 1 if k == "zero" else 0
    n = LENGTHS.size
    doc = np.repeat(np.arange(n), LENGTHS)
    key = np.unique(codes.astype(np.int64) * n + doc)          # per centroid the ascending distinct documents
    a = dict(nbits=nbits, centroids=cen, bucket_weights=w, ivf=(key % n).astype(np.int64),
             ivf_lengths=np.bincount(key // n, minlength=6).astype(np.int32), doc_lengths=LENGTHS.copy(),
             codes=codes.astype(np.int64), residuals=E.pack_buckets(bk, nbits))
    assert a["residuals"].shape == (T, dim * nbits // 8) and T == LENGTHS.sum()
    return a, np.array(kinds)


def requested_tokens():
    """Token indices REQUEST returns, in order, and the lengths it reports."""
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    ok = (REQUEST >= 0) & (REQUEST < LENGTHS.size)
    lens = np.where(ok, LENGTHS[np.clip(REQUEST, 0, LENGTHS.size - 1)], 0)
    toks = np.concatenate([np.arange(off[d], off[d + 1]) for d in REQUEST[ok]])
    return toks, lens


def check(what, got, ref64, ref32, kinds, bound):
    """got [T, dim] f32 against the float64 rows within `bound` u relative per component; the zero rows exactly 0; the
    tiny rows against the f32 rows ref32 under the same bound (float64 does not underflow where f32 does, and its clamp
    constant is the double 1e-12, not the float)."""
    got64 = np.asarray(got, F64)
    for k, ref in (("generic", ref64), ("huge", ref64), ("tiny", np.asarray(ref32, F64))):
        sel = kinds == k
        err = np.abs(got64[sel] - ref[sel])
        lim = bound * U * np.abs(ref[sel])
        worst = float(np.max(err / np.maximum(np.abs(ref[sel]), 1e-300) / U, initial=0.0))
        print(f"{what} {k}: {int(sel.sum())} rows, worst error {worst:.3f} u, bound {bound:.3f} u")
        bad = np.argwhere(~(err <= lim))
        assert bad.size == 0, f"{what}: {k} row {np.nonzero(sel)[0][bad[0][0]]} component {bad[0][1]}: " \
                              f"{got64[sel][tuple(bad[0])]!r} vs {ref[sel][tuple(bad[0])]!r}, {worst:.3f} u over {bound:.3f} u"
        assert np.isfinite(got64[sel]).all()
    z = np.asarray(got)[kinds == "zero"]
    assert z.size and np.all(z == 0) and not np.signbit(z).any(), f"{what}: a zero row is not +0: {z[np.nonzero(z)][:4]}"
