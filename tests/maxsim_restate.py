"""Float64 reference and derived error bound of np_hip_maxsim_batch (test infrastructure; numpy only, no GPU), plus the
one table of refused calls that the CPU and the GPU test share.

Bound, as tests/exact_restate.py derives S6's: u = 2^-24, DIMP = dim rounded up to the MFMA step (2 for f32, 16 for bf16),
gamma_m = m u / (1 - m u) for an f32 accumulation of m terms (F1 there).  For one (q, t), A = sum_d |q_d| |d_d| over the
values the kernel multiplies:
    precision 0                  gamma_DIMP A (1 + 2^-10)
    precision 3 from f32 rows    (eta_Q + eta_D + eta_Q eta_D + gamma_DIMP) A (1 + 2^-10), eta = the rows' own bf16 rounding ratios
    bf16 rows                    gamma_DIMP A (1 + 2^-10), against the f64 product of the bf16 values (products are exact, F2)
    per pair                     sum_q max_t bound + (Lq - 1) u sum_q (|max_t ref| + max_t bound)
"""
import ctypes as C

import numpy as np

from exact_restate import U, SECOND_ORDER, bf16, _ratios

F32, F64 = np.float32, np.float64
MODES = ("f32", "bf16_from_f32", "bf16_rows")     # (precision, input): (0, f32), (3, f32), (3, bf16)


def unit_rows(g, n, dim):
    v = g.standard_normal((n, dim))
    return (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)).astype(F32)


def pair(q, d, mode):
    """Reference and bound of one (query, document): dict(score, bound, sims [Lq, T] f64, tb [Lq, T], best, bmax)."""
    q, d = np.asarray(q, F32), np.asarray(d, F32)
    step = 2 if mode == "f32" else 16
    dimp = -(-q.shape[1] // step) * step
    gamma = dimp * U / (1 - dimp * U)
    qm, dm = (q, d) if mode != "bf16_from_f32" else (bf16(q), bf16(d))      # what the kernel multiplies
    with np.errstate(invalid="ignore", over="ignore"):
        sims = q.astype(F64) @ d.astype(F64).T
        aq, ad = np.abs(qm.astype(F64)), np.abs(dm.astype(F64))
        A = np.where(np.isfinite(aq), aq, 0.0) @ np.where(np.isfinite(ad), ad, 0.0).T
    a = gamma
    if mode == "bf16_from_f32":
        eq, ed = _ratios(q, axis=1)[0][:, None], _ratios(d, axis=1)[0][None, :]
        a = eq + ed + eq * ed + gamma
    ok = np.isfinite(sims)
    tb = np.where(ok, a * A * SECOND_ORDER, 0.0)
    lq = q.shape[0]
    has = ok.any(1) if d.shape[0] else np.zeros(lq, bool)
    best = np.where(ok, sims, -np.inf).max(1, initial=-np.inf)
    best = np.where(has, best, 0.0)
    bmax = tb.max(1, initial=0.0)
    return dict(score=best.sum(), bound=bmax.sum() + max(lq - 1, 0) * U * (np.abs(best) + bmax).sum(), sims=sims, tb=tb,
                best=best, bmax=bmax, has=has)


def batch(qs, ds, mode):
    """(score [B, N], bound [B, N]) of every (query, document): pair()'s figures for finite rows, over the concatenated documents."""
    lens = np.array([d.shape[0] for d in ds])
    off, ne, D = np.r_[0, np.cumsum(lens)], np.nonzero(lens)[0], np.concatenate(ds).astype(F32)
    step = 2 if mode == "f32" else 16
    dimp = -(-D.shape[1] // step) * step
    gamma, rnd = dimp * U / (1 - dimp * U), mode == "bf16_from_f32"
    aD, ed = np.abs((bf16(D) if rnd else D).astype(F64)).T, _ratios(D, axis=1)[0][None, :] if rnd else 0.0
    score, bound = np.zeros((len(qs), len(ds))), np.zeros((len(qs), len(ds)))
    for i, q in enumerate(qs):
        eq = _ratios(q, axis=1)[0][:, None] if rnd else 0.0
        tb = (eq + ed + eq * ed + gamma) * (np.abs((bf16(q) if rnd else q).astype(F64)) @ aD) * SECOND_ORDER
        best, bmax = np.zeros((q.shape[0], len(ds))), np.zeros((q.shape[0], len(ds)))
        best[:, ne] = np.maximum.reduceat(q.astype(F64) @ D.astype(F64).T, off[ne], axis=1)
        bmax[:, ne] = np.maximum.reduceat(tb, off[ne], axis=1)
        score[i], bound[i] = best.sum(0), bmax.sum(0) + max(q.shape[0] - 1, 0) * U * (np.abs(best) + bmax).sum(0)
    return score, bound


# ---- the refused calls: (name, overrides of a valid call, status, a word the message must hold) ---------------------------
REFUSALS = [
    ("dim0", dict(dim=0), 3, "dim"), ("dim1025", dict(dim=1025), 3, "dim"), ("query257", dict(qoff=[0, 257]), 3, "q_tok_offsets"),
    ("precision1", dict(precision=1), 8, "precision"), ("matches_p3", dict(precision=3, matches=True), 8, "out_match"),
    ("bf16_p0", dict(dtype=1), 8, "dtype"), ("doc_offsets_decrease", dict(doff=[0, 5, 3, 9]), 8, "doc_tok_offsets"),
    ("pair_id_n_docs", dict(ids=[0, 3]), 8, "pair_docs"),
]


def refused_call(lib, over):
    """A small valid listed call (1 query of 4 tokens, 3 documents, 2 pairs, dim 8) with `over` applied, through the C entry.
    Returns (status, message, outputs_untouched)."""
    a = dict(dim=8, qoff=[0, 4], doff=[0, 5, 7, 9], ids=[2, 0], precision=0, dtype=0, matches=False)
    a.update(over)
    qoff, doff = np.asarray(a["qoff"], np.int32), np.asarray(a["doff"], np.int64)
    ids, poff = np.asarray(a["ids"], np.int64), np.asarray([0, len(a["ids"])], np.int64)
    q = np.ones((300, 1100), F32)
    sc, sims, pos = np.full(8, 7.0, F32), np.full(2048, 7.0, F32), np.full(2048, 7, np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib.np_hip_maxsim_batch(0, a["dtype"], a["precision"], a["dim"], p(q), p(qoff), 1, p(q), p(doff), 3, p(ids), p(poff),
                                 p(sc), p(sims) if a["matches"] else None, p(pos) if a["matches"] else None)
    return rc, lib.np_hip_last_error().decode(), bool((sc == 7).all() and (sims == 7).all() and (pos == 7).all())
