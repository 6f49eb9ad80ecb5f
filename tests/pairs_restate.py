"""Checker of np_hip_score_pairs: given (query, document) pairs with per-token matches (test infrastructure; no GPU).

    check_pairs(a, q, doc_ids, scores, sims, pos)    the conditions one query's outputs have to meet
    Tally                                            entries checked / ambiguous, and the cap on their ratio
    sims32(a, q)                                     the kernel's arithmetic in f32 numpy: [Lq, T] scaled similarities

exact_restate is imported and not modified: the float64 similarities (_sims64), the per-(query token, document token) error
bound at precision 0 (bound) and the per-document bound (doc_bound) are the ones the S6 kernels are already held to.

For a pair and a query token write S = the float64 similarities to the document's tokens, B = their bounds, and
i* = argmax S over the finite entries.  A device similarity of token i lies in [S_i - B_i, S_i + B_i], so the device maximum
lies at or above S_i* - B_i*, and a token i can be the device's winner only if S_i + B_i >= S_i* - B_i*: the CANDIDATES.
    (a) |sim - S[pos]| <= B[pos]                    the reported value is the similarity of the reported token
    (b) pos is a candidate
    (c) where exactly one candidate exists, pos is that one (follows from (b); asserted on its own)
    (d) on the repeated-token document pos == 0: its 40 identical tokens span two tiles and every MFMA row takes the same
        operation sequence, so all similarities are bit-equal and the lowest index has to win
    (e) pos == -1 and sim == -inf exactly where no finite similarity exists (an empty document, a NaN query token)
    (f) the score is the f32 sum of the row's entries above -inf in token order from 0.0f, bit for bit (NaN when not finite)
    (g) |score - reference| <= doc_bound
With more than one candidate (c) says nothing, so a checker that met many such entries would check little.  The cap: outside
the repeated-token document at most 0.5 % of the checked entries may be ambiguous.  The float64 reference alone gives
0.012-0.053 % on make_corpus (six geometries, query lengths 1 / 33 / 65, 73 377 entries each), so the cap is ten times what
the data has and still leaves 99.5 % of the positions decided by (c).  It is a ratio over a sample, not a property of one call: a Tally
collects the counts of several calls and its owner asserts the cap once -- over one corpus and several query lengths
(test_pairs_restate_cpu.py), or over the corpora that run one kernel instantiation (test_gpu_pairs.py: the unit a wrong
position would come from; a corpus of nearly equal tokens such as d128b4w-6 is 1.1-1.3 % ambiguous by the reference alone,
the five corpora of its instantiation together 0.25-0.31 %).  A call without a Tally asserts the cap on its own entries.
"""
import numpy as np

import exact_restate as X

F32, F64 = np.float32, np.float64
AMBIGUOUS_CAP = 0.005


class Tally:
    def __init__(self):
        self.checked = 0
        self.ambiguous = 0

    def add(self, checked, ambiguous):
        self.checked += int(checked)
        self.ambiguous += int(ambiguous)

    def assert_cap(self, what=""):
        assert self.ambiguous <= AMBIGUOUS_CAP * self.checked, \
            f"{what}: {self.ambiguous} of {self.checked} entries have more than one candidate position " \
            f"({100.0 * self.ambiguous / max(self.checked, 1):.3f} % > {100 * AMBIGUOUS_CAP} %): the checker decides too little"


def ordered_sum(row):
    """f32 sum of the entries above -inf, in order, from 0.0f; NaN when the total is not finite (as S7 returns it)."""
    tot = F32(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for x in np.asarray(row, F32):
            if x > -np.inf:
                tot = F32(tot + x)
    return tot if np.isfinite(tot) else F32(np.nan)


def same_bits(x, y):
    x, y = F32(x), F32(y)
    return (np.isnan(x) and np.isnan(y)) or x.view(np.uint32) == y.view(np.uint32)


def sims32(a, q):
    """The arithmetic of the f32 kernel in numpy: x = f32(c + w), the sum of squares over the stored width minus pad_ss,
    1 / max(sqrt, 1e-12), the product as one chain of fused multiply-adds over the dims in order (the exact f64 product
    added to the f32 accumulator, one rounding per term -- and, unlike a BLAS call, the same operation sequence for every
    (query token, document token), so identical tokens get identical bits), one multiplication.  [Lq, T]."""
    p = X.prepare(a)
    q = np.ascontiguousarray(q, F32)
    x = (p.C[p.codes] + p.w[p.bkt]).astype(F32)
    xs = np.concatenate([x, np.full((x.shape[0], p.npad), p.w[0], F32)], 1)
    w0 = p.w[0]
    pad_ss = F32(F32(p.npad) * F32(w0 * w0)) if p.npad else F32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        tot = (X._sumsq(xs, "f32") - pad_ss).astype(F32)
        rn = (F32(1) / np.maximum(np.sqrt(tot), F32(1e-12))).astype(F32)
        acc = np.zeros((q.shape[0], x.shape[0]), F32)
        q64, x64 = q.astype(F64), x.astype(F64)
        for d in range(x.shape[1]):
            acc = (acc.astype(F64) + q64[:, d, None] * x64[None, :, d]).astype(F32)
        return (acc * rn[None, :]).astype(F32)


def repeated_token_doc(a):
    """The id of the last document when it is make_corpus's repeated-token document (several copies of one token), else -1."""
    p = X.prepare(a)
    d = p.off.size - 2
    if d < 0 or p.off[d + 1] - p.off[d] < 2:
        return -1
    o0, o1 = int(p.off[d]), int(p.off[d + 1])
    return d if np.all(p.codes[o0:o1] == p.codes[o0]) and np.all(p.bkt[o0:o1] == p.bkt[o0]) else -1


def check_pairs(a, q, doc_ids, scores, sims, pos, what="", tally=None):
    """Asserts (a)-(g) of the module docstring for one query `q` [Lq, dim] against the documents `doc_ids` (global ids of an
    unsharded index): scores [n], sims [n, Lq] f32, pos [n, Lq] i32.  Returns (entries checked, ambiguous entries), both
    outside the repeated-token document."""
    p = X.prepare(a)
    q = np.ascontiguousarray(q, F32)
    lq = q.shape[0]
    doc_ids = np.asarray(doc_ids, np.int64).reshape(-1)
    n = doc_ids.size
    scores = np.asarray(scores, F32).reshape(-1)
    sims = np.asarray(sims, F32).reshape(n, lq)
    pos = np.asarray(pos).reshape(n, lq)
    assert scores.size == n and pos.dtype == np.int32, f"{what}: shapes"
    S64 = X._sims64(p, q)
    Bd = X.bound(a, q, 0)
    ref = X.reference(a, q)
    dbd = X.doc_bound(a, q, 0)
    rep = repeated_token_doc(a)
    own = tally is None
    tally = Tally() if own else tally
    rows = np.arange(lq)
    for j, d in enumerate(doc_ids.tolist()):
        w = f"{what} pair {j} (document {d})"
        o0, o1 = int(p.off[d]), int(p.off[d + 1])
        ln = o1 - o0
        S, B = S64[:, o0:o1], Bd[:, o0:o1]
        fin = np.isfinite(S)
        some = fin.any(1) if ln else np.zeros(lq, bool)
        pj, sj = pos[j].astype(np.int64), sims[j]
        # (e)
        none = ~some
        assert np.all(pj[none] == -1) and np.all(np.isneginf(sj[none])), \
            f"{w}: tokens {rows[none][:5]} have no finite similarity: pos {pj[none][:5]} sim {sj[none][:5]}, expected -1 / -inf"
        assert np.all((pj[some] >= 0) & (pj[some] < ln)), f"{w}: position outside the document: {pj[some][:8]} (length {ln})"
        assert np.all(np.isfinite(sj[some])), f"{w}: tokens {rows[some][~np.isfinite(sj[some])][:5]}: sim not finite"
        if some.any():
            r = rows[some]
            Sm = np.where(fin, S, -np.inf)[r]
            star = Sm.argmax(1)
            floor = Sm[np.arange(r.size), star] - B[r, star]
            cand = fin[r] & (S[r] + B[r] >= floor[:, None])
            at = pj[r]
            # (a)
            err = np.abs(sj[r].astype(F64) - S[r, at])
            bad = ~(err <= B[r, at])
            assert not bad.any(), f"{w}: tokens {r[bad][:5]}: |sim - S64[pos]| = {err[bad][:5]} over {B[r, at][bad][:5]} (pos {at[bad][:5]})"
            # (b)
            bad = ~cand[np.arange(r.size), at]
            assert not bad.any(), f"{w}: tokens {r[bad][:5]}: pos {at[bad][:5]} cannot hold the maximum (float64 argmax {star[bad][:5]})"
            # (c)
            nc = cand.sum(1)
            one = nc == 1
            assert np.all(at[one] == cand[one].argmax(1)), f"{w}: a decided position is wrong"
            # (d)
            if d == rep:
                assert np.all(at == 0), f"{w}: identical tokens, position {at[at != 0][:5]} instead of 0 (tokens {r[at != 0][:5]})"
            else:
                tally.add(r.size, int((nc > 1).sum()))
        # (f)
        want = ordered_sum(sj)
        assert same_bits(scores[j], want), f"{w}: score {scores[j]!r} ({F32(scores[j]).view(np.uint32):08x}) is not the ordered " \
                                           f"f32 sum of its row {want!r} ({F32(want).view(np.uint32):08x})"
        # (g)
        assert abs(float(scores[j]) - ref[d]) <= dbd[d], f"{w}: |score - reference| = {abs(float(scores[j]) - ref[d])} over {dbd[d]}"
    if own:
        tally.assert_cap(what)
    return tally.checked, tally.ambiguous
