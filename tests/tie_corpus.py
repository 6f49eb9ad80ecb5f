"""Corpora with exact ties at known places (test infrastructure).

Every centroid and query entry is a small multiple of 1/8, so each query-centroid score is a multiple of 1/64 with
few significant bits: every f32 product and sum of S1-S4 (QC, group maxima, approximate scores) is exact, in f32 and in
the split-bf16 form alike.  The HIP path, the C oracle and a float64 numpy computation therefore agree bit for bit on
every value before the exact stage, and any disagreement in cells, candidates or selection is a tie-rule bug, not
rounding.  Scores take only a few hundred distinct values, so ties straddle almost every cut on their own; the builder
adds the ties that matter on purpose:

- duplicate centroids (`dup_centroids`: (src, dst) pairs);
- groups of byte-identical documents (`dup_docs`: lists of ids; the first id's codes and residuals are copied);
- the constructed pair (`pair`): documents with EQUAL exact scores and DIFFERENT approximate scores, the one with the
  better approximate score holding the higher id, so (exact, id) and (exact, approximate rank) order them apart.
"""
from __future__ import annotations

import numpy as np

from next_plaid_amd import synth

E = np.float32(0.125)


def _dyadic(rng, shape, lo, hi):
    return (rng.integers(lo, hi + 1, shape).astype(np.float32) * E).astype(np.float32)


def bucket_weights(nbits):
    n = 1 << nbits
    w = (np.arange(n, dtype=np.float32) - (n - 1) / 2) / n      # multiples of 1/(2n), symmetric, none zero
    return w.astype(np.float32)


# Constructed pair (ids into the centroid table; the builder reserves them):
#   cA : 0.5 e0                     a1 = cA + residual pulling dim 0 UP      -> exact(e0 . a1) ~ 0.53
#   cA2: 0.5 e1                     a2 = cA2 + residual pulling dim 1 UP
#   c3 : 0.625 e0 + 0.625 e1        t3 = c3 + residual pulling dims 0, 1 DOWN, every other dim far out -> exact ~ 0.06
# A1 = [a1], B1 = [a1, t3]; A2 = [a1, a2], B2 = [a1, a2, t3].  One-token query e0: approx(B*) = 0.625 > approx(A*) = 0.5,
# exact all equal (a1 is every document's best token).  Two-token query [e0, e1]: exact(A2) = exact(B2), approx(B2) >
# approx(A2).  Every other centroid keeps dims 0 and 1 <= 0.25, and no other document uses cA, cA2 or c3.
PAIR_CENTROIDS = (3, 4, 5)


def build(K, N, dim=128, nbits=2, len_lo=3, len_hi=8, seed=0, dup_centroids=(), dup_docs=(), pair=None,
          zero_dims01=False):
    """Host arrays for MmapIndex.from_arrays / OracleIndex plus the tie bookkeeping:
    'groups' -- sorted id arrays of byte-identical documents (dup_docs and the pair's shared tokens are separate);
    'pair'   -- dict(A1, B1, A2, B2, cA, cA2, c3) when pair = (A1, B1, A2, B2) ids are given (A1 < B1, A2 < B2).
    zero_dims01: every centroid's dims 0 and 1 are <= 0 (the batched-threshold scenario builds its own values there)."""
    rng = np.random.default_rng(seed)
    cen = _dyadic(rng, (K, dim), -2, 2)
    dead = ~cen.any(1)
    cen[dead, 0] = E                                    # no zero rows
    if zero_dims01:
        cen[:, :2] = -np.abs(cen[:, :2])
    for s, d in dup_centroids:
        cen[d] = cen[s]
    lens = rng.integers(len_lo, len_hi + 1, N).astype(np.int64)
    reserved = set()
    if pair is not None:
        cA, cA2, c3 = PAIR_CENTROIDS
        cen[[cA, cA2, c3]] = 0
        cen[cA, 0] = 0.5
        cen[cA2, 1] = 0.5
        cen[c3, 0] = cen[c3, 1] = 0.625
        reserved = {cA, cA2, c3}
        A1, B1, A2, B2 = pair
        lens[[A1, B1, A2, B2]] = (1, 2, 2, 3)
    groups = [np.sort(np.asarray(g, np.int64)) for g in dup_docs]
    allg = np.concatenate(groups) if groups else np.zeros(0, np.int64)
    assert np.unique(allg).size == allg.size, "duplicate groups overlap"
    for g in groups:
        lens[g] = lens[g[0]]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(off[-1])
    codes = rng.integers(0, K, T).astype(np.int64)
    if reserved:
        bad = np.isin(codes, list(reserved))
        codes[bad] = (codes[bad] + 7) % K
        while np.isin(codes, list(reserved)).any():
            bad = np.isin(codes, list(reserved))
            codes[bad] = (codes[bad] + 1) % K
    pd = dim * nbits // 8
    res = rng.integers(0, 256, (T, pd)).astype(np.uint8)
    top = (1 << nbits) - 1
    if pair is not None:
        def packed(buckets):
            bits = ((np.asarray(buckets)[:, None] >> np.arange(nbits)) & 1).astype(np.uint8).reshape(-1)
            return np.packbits(bits, bitorder="big")

        far = np.where(rng.integers(0, 2, dim) == 0, 0, top)          # every other dim at an extreme bucket
        b_a1 = np.where(rng.integers(0, 2, dim) == 0, top // 2, top // 2 + 1)   # near-zero weights elsewhere
        b_a1[0] = top
        b_a2 = b_a1.copy()
        b_a2[0] = top // 2
        b_a2[1] = top
        b_t3 = far.copy()
        b_t3[0] = b_t3[1] = 0
        toks = {A1: [(cA, b_a1)], B1: [(cA, b_a1), (c3, b_t3)], A2: [(cA, b_a1), (cA2, b_a2)],
                B2: [(cA, b_a1), (cA2, b_a2), (c3, b_t3)]}
        for doc, tl in toks.items():
            for j, (c, b) in enumerate(tl):
                codes[off[doc] + j] = c
                res[off[doc] + j] = packed(b)
    for g in groups:
        s0, l = off[g[0]], lens[g[0]]
        for d in g[1:]:
            codes[off[d]: off[d] + l] = codes[s0: s0 + l]
            res[off[d]: off[d] + l] = res[s0: s0 + l]
    ivf, ivf_lengths = synth.build_ivf(codes, lens, K)
    a = dict(nbits=nbits, centroids=cen, bucket_weights=bucket_weights(nbits), ivf=ivf, ivf_lengths=ivf_lengths,
             doc_lengths=lens, codes=codes, residuals=res, groups=groups)
    if pair is not None:
        a["pair"] = dict(A1=A1, B1=B1, A2=A2, B2=B2, cA=cA, cA2=cA2, c3=c3)
    return a


def queries(a, n, n_tokens, seed=1):
    """Dyadic queries near random documents' tokens: centroid of a token's code plus noise in {-1, 0, 1} / 8."""
    rng = np.random.default_rng(seed)
    lens = a["doc_lengths"]
    off = np.concatenate([[0], np.cumsum(lens)])
    cen = a["centroids"]
    qs = []
    for _ in range(n):
        doc = int(rng.integers(0, lens.size))
        t = off[doc] + rng.integers(0, max(int(lens[doc]), 1), n_tokens)
        q = cen[a["codes"][t]] + _dyadic(rng, (n_tokens, cen.shape[1]), -1, 1)
        qs.append(np.ascontiguousarray(q, np.float32))
    return qs


def pair_queries(dim):
    e = np.eye(dim, dtype=np.float32)
    return e[:1].copy(), e[:2].copy()


def threshold_scenario(K=256, dim=128, N=3000, seed=5, cbs=100, b=10, c1=20, c2=30):
    """The batched path's threshold with a duplicate pair tied at a token's cut (centroid_batch_size = cbs,
    n_ivf_probe = 2, centroid_score_threshold = 0.25, query [e0, e1]):
      token e0: b scores 0.5, then c1 = c2 at 0.375 -> it takes b and c1; (e0, c2) is never pushed (b and c1 come
                before c2 in its slab and score >= it), although 0.375 >= t_cs;
      token e1: c1 = c2 at 0.125 are its top two, below t_cs.
    search.rs:177-199 + 243-251: c2's max over PUSHED pairs is 0.125 < 0.25, so c2 is dropped; b and c1 stay."""
    assert b < c1 < c2 and b // cbs == c2 // cbs and K > cbs
    a = build(K, N, dim=dim, seed=seed, zero_dims01=True)
    cen = a["centroids"]
    cen[b, :2] = (0.5, 0.0)
    cen[c1, :2] = cen[c2, :2] = (0.375, 0.125)
    cen[c2] = cen[c1]
    return a, np.eye(dim, dtype=np.float32)[:2].copy()
