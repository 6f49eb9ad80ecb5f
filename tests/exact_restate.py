"""Numpy restatement of S6, the exact MaxSim stage, with a float64 reference and a derived error bound
(test infrastructure; no GPU; does not import oracle/ and does not use synth.reconstruct / synth.unpack_buckets).

    reference(arrays, q)             float64 MaxSim per document, straight from the f32 index arrays
    emulate(arrays, q, precision)    the arithmetic of each S6 kernel (np_kernels.h), bf16 by integer bit operations
    bound(arrays, q, precision)      |kernel - reference| per (query token, document token), from operation counts
    doc_bound(...)                   the same per document
    MUTANTS                          emulate() with one defect each; CASES / CATCHES: the shared case list

Storage.  The library stores a file of dim <= 128 at DIM = dim rounded up to 32: pad centroid values are 0, pad residual
bytes are 0 (bucket 0), the query is zero-padded.  A 1-bit file is stored as 2-bit with the same weights.  So a stored
row is x_d = c_d + w[bucket_d] on the file dims and x_d = w[0] on the DIM - dim pad dims; every pad PRODUCT is exactly 0.

Derivation of the bound.  u = 2^-24 (f32 round to nearest).  For one query token q and one document token t write
    A = sum_d |q_d| |c_d|,   R = sum_d |q_d| |r_d|   (file dims; r_d = w[bucket_d]),   n = ||c + r||  in exact arithmetic,
    reference = (q.c + q.r) / n.
Every bound is  (a_C A + a_R R) / n  * (1 + 2^-10)   (the last factor covers the products of two error terms).
Facts used: (F1) adding m terms into an f32 accumulator, in any order, one rounding per addition, is within
gamma_m sum|terms| of the exact sum, gamma_m = m u / (1 - m u); an fmaf chain is one rounding per term.  A bf16 MFMA is
counted at one rounding per product (16 per instruction): its internal order is not documented, this is the worst case.
(F2) products of two bf16 values are exact in f32.  (F3) bf16 has 8 significant bits: |x - hi(x)| <= 2^-8 |x| and, with
lo = bf16(x - hi), |x - hi - lo| <= 2^-16 |x|.  Instead of these worst cases the bound uses the ratios the INPUTS
actually have (computed below from the query, the bucket weights and the centroids; never from any output):
    eta = max |x - hi| / |x|,   lam = max |lo| / |x|,   rho = max |x - hi - lo| / |x|       (eta, lam <= 2^-8, rho <= 2^-16)
per query token for q, over the bucket weights for r, over the centroid table for c.

  norm, QC-reuse forms (precisions 1, 2): inv_norm is an f32 computed at open over the FILE dims only: each x_d is one
    rounding (2 u on its square), a lane sums ceil(dim/64) squares by fmaf, six butterfly additions follow:
    ss is within (ceil(dim/64) + 8) u; the square root halves that; sqrtf and the reciprocal are counted at 2 u each:
        nu1 = ((ceil(dim/64) + 8) / 2 + 4) u
  norm, exact_f32_kernel / exact_bf16_kernel (precisions 0, 3, and nbits 8): the sum runs inline over the STORED width,
    DIM/2 fmaf terms per lane + 1 addition, then pad_ss = (DIM - dim) w[0]^2 (two f32 products) is subtracted.  The sum
    carries (DIM/2 + 3) u relative to tot + pad_ss, so relative to tot = ||c + r||^2 it is amplified by
    kappa_t = (tot + pad_ss) / tot; the two roundings of pad_ss add 2 u pad_ss / tot = 2 u (kappa_t - 1), the subtraction u:
        nu0_t = (((DIM/2 + 3) kappa_t + 2 (kappa_t - 1) + 1) / 2 + 4) u            (kappa_t = 1 on an unpadded index)
  precision 0:  x_d = f32(c_d + w_d) (u), a DIM-long fmaf chain (gamma_DIM), the product with 1/n (u):
        a_C = a_R = (DIM + 2) u + nu0_t
  precision 3:  x_d (u), bf16(x_d) (eta_X of that row), bf16(q) (eta_Q), DIM exact products accumulated (gamma_DIM), 1/n (u):
        a_C = a_R = eta_X + eta_Q + eta_X eta_Q + (DIM + 2) u + nu0_t
  precision 1:  (QC + hi(R).hi(Q)) inv_norm.  QC is S1's DIM-long f32 fmaf chain (gamma_DIM on A); it is the accumulator
    the DIM products are added to, so their DIM roundings act on A as well; then 1/n (u):
        a_C = (2 DIM + 1) u + nu1
        a_R = eta_R + eta_Q + eta_R eta_Q + (DIM + 1) u (1 + 2^-6) + nu1     (1 + 2^-6 >= (1 + eta)^2: |hi| vs |x|)
  precision 2:  (QC + hi.hi + lo(R).hi(Q) + hi(R).lo(Q)) inv_norm.  r q = (rh + rl + er)(qh + ql + eq) leaves out
    rl ql + er q + (r - er) eq, and 3 DIM products are accumulated:
        a_C = (4 DIM + 1) u + nu1
        a_R = lam_R lam_Q + rho_R + (1 + rho_R) rho_Q + (3 DIM + 1) u (1 + 2^-5) + nu1
  split S1 (s1_split = 1, qc_gemm_b3_kernel): QC itself is hi.hi + lo.hi + hi.lo from 0, so a_C takes the form of a_R(2):
        a_C = lam_C lam_Q + rho_C + (1 + rho_C) rho_Q + (3 DIM + m + 1) u (1 + 2^-5) + nu1,   m = DIM or 3 DIM as above
The part of a bound without eta / lam / rho is its ACCUMULATION part: a kernel and emulate(..., acc="f64") (same
rounded operands, exact sums) may differ by that much and no more.
Per document:  |max_t a - max_t b| <= max_t |a - b|, so the bound is sum_q max_t bound(q, t), plus the q-ordered f32 sum:
(Lq - 1) u sum_q (|max_t reference| + max_t bound).  Entries whose reference is not finite are ignored on both sides.
"""
import os
import sys
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "next-plaid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from next_plaid_amd import synth  # noqa: E402  (corpus generator only; never its decompression)

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -10
F32, F64 = np.float32, np.float64


# ---- bf16 by integer bit operations -------------------------------------------------------------------------------------
def bf16(x):
    """f32 -> nearest bf16 (ties to even), returned as the f32 holding that value."""
    x = np.ascontiguousarray(x, F32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    r = np.where(np.isnan(x), np.uint32(0x7FC00000), r).astype(np.uint32)
    return r.view(F32).reshape(x.shape)


def split(x):
    hi = bf16(x)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = bf16((np.asarray(x, F32) - hi).astype(F32))
    return hi, lo


def _ratios(x, axis=None):
    """(eta, lam, rho) of the values in x: see the module docstring.  Zeros and non-finite values are left out."""
    x32 = np.asarray(x, F32)
    hi, lo = split(x32)
    x64, hi, lo = x32.astype(F64), hi.astype(F64), lo.astype(F64)
    ok = np.isfinite(x64) & (x64 != 0)
    ax = np.where(ok, np.abs(x64), 1.0)

    def rel(v):
        return np.max(np.where(ok, np.abs(v) / ax, 0.0), axis=axis)
    with np.errstate(invalid="ignore"):
        return rel(x64 - hi), rel(lo), rel(x64 - hi - lo)


# ---- the index, unpacked independently ----------------------------------------------------------------------------------
def unpack(residuals, nbits, dim):
    """Packed residual bytes -> bucket index per (token, dim).  The first dim of a byte sits in its highest bits, and a
    field's bits are stored in reverse order (the on-disk layout: most significant stored bit = bit 0 of the bucket)."""
    res = np.ascontiguousarray(residuals, np.uint8)
    per, mask = 8 // nbits, (1 << nbits) - 1
    rev = np.array([int(format(v, f"0{nbits}b")[::-1], 2) for v in range(1 << nbits)], np.int64)
    out = np.empty((res.shape[0], res.shape[1] * per), np.int64)
    for e in range(per):
        out[:, e::per] = rev[(res >> (8 - nbits * (e + 1))) & mask]
    return out[:, :dim]


@dataclass
class Prep:
    C: np.ndarray          # [K, dim] f32
    w: np.ndarray          # [2^nbits] f32
    codes: np.ndarray      # [T]
    bkt: np.ndarray        # [T, dim]
    off: np.ndarray        # [N + 1]
    dim: int
    DIM: int               # stored width
    nbits: int
    cache: dict = field(default_factory=dict)

    @property
    def npad(self):
        return self.DIM - self.dim


def prepare(a):
    if isinstance(a, Prep):
        return a
    if "_prep" in a:
        return a["_prep"]
    C = np.ascontiguousarray(a["centroids"], F32)
    dim, nbits = C.shape[1], int(a["nbits"])
    lens = np.asarray(a["doc_lengths"], np.int64)
    p = Prep(C=C, w=np.ascontiguousarray(a["bucket_weights"], F32), codes=np.asarray(a["codes"], np.int64),
             bkt=unpack(a["residuals"], nbits, dim), off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
             dim=dim, DIM=(dim + 31) // 32 * 32 if dim <= 128 else dim, nbits=nbits)
    if isinstance(a, dict):
        a["_prep"] = p
    return p


def _rows64(p):
    """(C[code], w[bucket], their sum, squared norm, norm) per token in float64, computed once per index."""
    if "rows" not in p.cache:
        Cc, W = p.C[p.codes].astype(F64), p.w[p.bkt].astype(F64)
        x = Cc + W
        tot = (x * x).sum(1)
        p.cache["rows"] = (Cc, W, x, tot, np.maximum(np.sqrt(tot), 1e-12))
    return p.cache["rows"]


def decompress64(a):
    """Normalised rows in float64 (the rule the golden decompress fixtures were minted by)."""
    _, _, x, _, n = _rows64(prepare(a))
    return x / n[:, None]


def _docmax(S, off):
    """[Lq, T] -> [Lq, N]: max over each document's tokens, -inf for an empty document."""
    N = off.size - 1
    out = np.full((S.shape[0], N), -np.inf, S.dtype)
    ne = np.nonzero(off[1:] > off[:-1])[0]
    if ne.size and S.shape[1]:
        out[:, ne] = np.maximum.reduceat(S, off[ne], axis=1)
    return out


def _maxsim(S, off, q_sum="f64", init=-np.inf):
    """sum_q max_t S[q, t], non-finite entries ignored; q_sum = "f32": the kernels' q-ordered f32 sum."""
    with np.errstate(invalid="ignore"):
        V = np.where(np.isfinite(S), S, -np.inf)
    M = np.maximum(_docmax(V, off), init)
    M = np.where(M > -np.inf, M, 0.0)
    if q_sum == "f64":
        return M.astype(F64).sum(0)
    tot = np.zeros(M.shape[1], F32)
    for i in range(M.shape[0]):
        tot = (tot + M[i].astype(F32)).astype(F32)
    return tot


def _sims64(p, q):
    key = ("ref", q.tobytes())
    if key not in p.cache:
        _, _, x, _, n = _rows64(p)
        with np.errstate(invalid="ignore", over="ignore"):
            p.cache[key] = (np.asarray(q, F32).astype(F64) @ x.T) / n[None, :]
    return p.cache[key]


def reference(a, q):
    p = prepare(a)
    return _maxsim(_sims64(p, np.ascontiguousarray(q, F32)), p.off)


# ---- the kernels' arithmetic -------------------------------------------------------------------------------------------
def _mm(q, rows, acc):
    """q [Lq, d] . rows [T, d]^T -> [Lq, T]; both hold f32 values; accumulated in f32 or in float64."""
    ft = F32 if acc == "f32" else F64
    with np.errstate(invalid="ignore", over="ignore"):
        return np.matmul(np.asarray(rows, ft), np.ascontiguousarray(np.asarray(q, ft).T)).T


def _sumsq(x, acc):
    if acc == "f32":
        return (x * x).astype(F32).sum(1, dtype=F32)
    return (x.astype(F64) ** 2).sum(1)


def kernel_class(precision, nbits):
    """Which arithmetic launch_exact runs: nbits 8 takes the f32 kernel at every precision."""
    return 0 if (nbits == 8 or precision == 0) else precision


def emulate(a, q, precision, s1_split=False, acc="f32", mutant=None):
    """Per-document scores of the kernel arithmetic `precision` selects.  acc = "f32": f32 accumulation throughout (what
    the kernels do, in numpy's order); "f64": the same rounded operands with exact sums and one rounding less at the end
    (assertion B of the GPU test compares against this one).  mutant: a key of MUTANTS."""
    p = prepare(a)
    q = np.ascontiguousarray(q, F32)
    ft = F32 if acc == "f32" else F64
    cls = kernel_class(precision, p.nbits)
    okey = ("emulate", q.tobytes(), cls, bool(s1_split) and cls in (1, 2), acc)
    if mutant is None and okey in p.cache:
        return p.cache[okey]
    if mutant == "c" and cls == 2:
        cls = 1
    if mutant == "d" and cls == 1:
        cls = 3
    bkt = p.bkt
    if mutant == "e":   # one bucket off by one in the last dim of each document's best token
        S = _sims64(p, q)
        with np.errstate(invalid="ignore"):
            best = np.where(np.isfinite(S), S, -np.inf).max(0)
        bkt = bkt.copy()
        for d in range(p.off.size - 1):
            if p.off[d + 1] > p.off[d]:
                t = p.off[d] + int(np.argmax(best[p.off[d]:p.off[d + 1]]))
                bkt[t, -1] += 1 if bkt[t, -1] + 1 < p.w.size else -1
    off = p.off
    if mutant == "i":   # the last tile of document tokens dropped when len % 32 == 1: hide that token
        lens = np.diff(off)
        hide = off[1:][lens % 32 == 1] - 1
    else:
        hide = np.zeros(0, np.int64)
    if mutant == "h":
        q = q[:32]
    wh, wl = split(p.w)
    ck = ("emu", acc)
    if mutant == "e" or ck not in p.cache:
        Cc = p.C[p.codes]
        x = (Cc + p.w[bkt]).astype(F32)
        xs = np.concatenate([x, np.full((x.shape[0], p.npad), p.w[0], F32)], 1)        # the stored row
        ch, cl = split(Cc)
        rows = dict(Cc=Cc, x=x, xb=bf16(x), ss_stored=_sumsq(xs, acc), ss_file=_sumsq(x, acc), ch=ch, cl=cl,
                    Rh=wh[bkt], Rl=wl[bkt])
        rows = {k: (v.astype(F32 if acc == "f32" or v.ndim == 1 else F64)) for k, v in rows.items()}
        if mutant != "e":
            p.cache[ck] = rows
    else:
        rows = p.cache[ck]
    Cc, x = rows["Cc"], rows["x"]
    with np.errstate(invalid="ignore", over="ignore"):
        if cls in (0, 3):
            w0 = p.w[0]
            pad_ss = F32(F32(p.npad) * F32(w0 * w0)) if p.npad else F32(0)
            ss = rows["ss_stored"].astype(ft)
            tot = ss if mutant == "g" else (ss - ft(pad_ss)).astype(ft)
            rn = (ft(1) / np.maximum(np.sqrt(tot), ft(1e-12))).astype(ft)
            if cls == 0:
                S = _mm(q, x, acc)
            else:
                S = _mm(bf16(q), rows["xb"], acc)
        else:
            rn = (ft(1) / np.maximum(np.sqrt(rows["ss_file"].astype(ft)), ft(1e-12))).astype(ft)     # inv_norm: file dims only
            qh, ql = split(q)
            if s1_split:
                S = (_mm(qh, rows["ch"], acc) + _mm(qh, rows["cl"], acc)).astype(ft)
                S = (S + _mm(ql, rows["ch"], acc)).astype(ft)
            else:
                S = _mm(q, Cc, acc)
            Rh, Rl = rows["Rh"], rows["Rl"]
            S = (S + _mm(qh, Rh, acc)).astype(ft)
            if cls == 2:
                # k-step 0 of the QC-reuse kernels holds dims [0, 8) and [DIM/2, DIM/2 + 8)
                k0 = np.array([d for d in list(range(8)) + list(range(p.DIM // 2, p.DIM // 2 + 8)) if d < p.dim])
                keep = np.ones(p.dim, F32)
                keep[k0] = 0
                if mutant != "a":
                    S = (S + _mm(qh * (keep if mutant == "k" else 1), Rl, acc)).astype(ft)
                if mutant != "b":
                    S = (S + _mm(ql * (keep if mutant == "j" else 1), Rh, acc)).astype(ft)
        S = (S * rn[None, :]).astype(ft)
    if hide.size:
        S[:, hide] = np.nan
    out = _maxsim(S, off, q_sum=acc, init=0.0 if mutant == "f" else -np.inf).astype(F64)
    if mutant is None:
        p.cache[okey] = out
    return out


MUTANTS = {
    "a": "precision 2 without lo(R).hi(Q)",
    "b": "precision 2 without hi(R).lo(Q)",
    "c": "precision 2 run as precision 1",
    "d": "precision 1 with the centroid term through bf16 as well (run as precision 3)",
    "e": "one bucket index off by one in the last dim of each document's best token",
    "f": "running maxima start at 0 instead of -inf",
    "g": "pad_ss not subtracted on a padded geometry",
    "h": "query tiles after the first dropped",
    "i": "the tile of document tokens after position 32 k dropped when len % 32 == 1",
    "j": "precision 2 without hi(R).lo(Q) in k-step 0 of DIM/16",
    "k": "precision 2 without lo(R).hi(Q) in k-step 0 of DIM/16",
}


# ---- the bound ---------------------------------------------------------------------------------------------------------
def bound_terms(a, q, precision, s1_split=False):
    """dict(total=[Lq, T], acc=[Lq, T], kappa=[T]): the bound of the module docstring and its accumulation part."""
    p = prepare(a)
    q = np.ascontiguousarray(q, F32)
    cls = kernel_class(precision, p.nbits)
    key = ("bound", q.tobytes(), cls, bool(s1_split))
    if key in p.cache:
        return p.cache[key]
    DIM, dim = p.DIM, p.dim
    Cc, W, x, tot, n = _rows64(p)
    if "abs" not in p.cache:
        p.cache["abs"] = (np.abs(Cc).T.copy(), np.abs(W).T.copy())
    akey = ("AR", q.tobytes())
    if akey not in p.cache:
        with np.errstate(invalid="ignore", over="ignore"):
            aq = np.abs(q.astype(F64))
            aq = np.where(np.isfinite(aq), aq, 0.0)
            p.cache[akey] = (aq @ p.cache["abs"][0], aq @ p.cache["abs"][1])
    A, R = p.cache[akey]
    eta_q, lam_q, rho_q = (v[:, None] for v in _ratios(q, axis=1))
    kappa = np.ones(x.shape[0])
    if cls in (0, 3):
        if p.npad:
            pad = p.npad * float(p.w[0]) ** 2
            kappa = (tot + pad) / np.maximum(tot, 1e-300)
        nu = (((DIM / 2 + 3) * kappa + 2 * (kappa - 1) + 1) / 2 + 4) * U
        acc_c = acc_r = ((DIM + 2) * U + nu)[None, :]
        if cls == 0:
            a_c = a_r = acc_c
        else:
            if "eta_x" not in p.cache:
                p.cache["eta_x"] = _ratios((p.C[p.codes] + p.w[p.bkt]).astype(F32), axis=1)[0][None, :]
            eta_x = p.cache["eta_x"]
            a_c = a_r = eta_x + eta_q + eta_x * eta_q + acc_c
    else:
        nu = ((-(-dim // 64) + 8) / 2 + 4) * U
        eta_r, lam_r, rho_r = _ratios(p.w)
        m = DIM if cls == 1 else 3 * DIM
        acc_r = (m + 1) * U * (1 + 2.0 ** -5) + nu
        a_r = acc_r + (eta_r + eta_q + eta_r * eta_q if cls == 1 else lam_r * lam_q + rho_r + (1 + rho_r) * rho_q)
        if s1_split:
            if "ratios_c" not in p.cache:
                p.cache["ratios_c"] = _ratios(p.C)
            _, lam_c, rho_c = p.cache["ratios_c"]
            acc_c = (3 * DIM + m + 1) * U * (1 + 2.0 ** -5) + nu
            a_c = acc_c + lam_c * lam_q + rho_c + (1 + rho_c) * rho_q
        else:
            a_c = acc_c = (DIM + m + 1) * U + nu
    valid = np.isfinite(_sims64(p, q))
    total = np.where(valid, (a_c * A + a_r * R) / n[None, :] * SECOND_ORDER, 0.0)
    acc = np.where(valid, (acc_c * A + acc_r * R) / n[None, :] * SECOND_ORDER, 0.0)
    p.cache[key] = dict(total=total, acc=acc, kappa=kappa, valid=valid)
    return p.cache[key]


def drop_query_cache(a):
    """Forget what was cached per query (the float64 similarities and bounds); the per-index pieces stay."""
    p = prepare(a)
    for k in [k for k in p.cache if isinstance(k, tuple)]:
        del p.cache[k]


def bound(a, q, precision, s1_split=False):
    return bound_terms(a, q, precision, s1_split)["total"]


def doc_bound(a, q, precision, s1_split=False, part="total"):
    """Per-document bound; part = "acc": the accumulation part alone (against emulate(..., acc="f64"))."""
    p = prepare(a)
    q = np.ascontiguousarray(q, F32)
    t = bound_terms(p, q, precision, s1_split)
    Bm = _docmax(np.where(t["valid"], t[part], -np.inf), p.off)
    Bm = np.where(Bm > -np.inf, Bm, 0.0)
    with np.errstate(invalid="ignore"):
        M = _docmax(np.where(t["valid"], _sims64(p, q), -np.inf), p.off)
    M = np.where(M > -np.inf, np.abs(M), 0.0)
    return Bm.sum(0) + max(q.shape[0] - 1, 0) * U * (M + Bm).sum(0) * SECOND_ORDER


# ---- corpora, queries and the case list ---------------------------------------------------------------------------------
PLANTED = (0, 1, 31, 32, 33, 63, 64, 65, 200, 1, 33, 65, 0)   # document lengths at the 32-token tile edges
N_RANDOM, K = 80, 64
QUERY_LENGTHS = (1, 31, 32, 33, 64, 65, 200, 256)
QUERY_KINDS = ("near", "negated", "random", "nan", "huge", "tiny", "near", "near")   # one batch of 8 per case
# (file dim, nbits, log2 of the bucket-weight scale): every kernel width at 2 and 4 bits, 8 bits, 1 bit, padded rows
GEOMETRIES = [(32, 2, 0), (32, 4, 0), (64, 2, 0), (64, 4, 0), (96, 2, 0), (96, 4, 0), (128, 2, 0), (128, 4, 0),
              (64, 8, 0), (128, 8, 0), (64, 1, 0), (100, 4, 0), (48, 4, 0), (48, 2, 0),
              (128, 4, -6), (128, 4, 2), (100, 4, 2), (32, 4, 2)]


def geo_name(g):
    return f"d{g[0]}b{g[1]}" + ("" if g[2] == 0 else f"w{g[2]:+d}")


_corpora = {}


def make_corpus(geo):
    """Index arrays of one (geometry, weight scale): random documents, then the planted lengths, two duplicates of
    document 3, and one document of a single repeated token (REPEATED_DOC)."""
    if geo in _corpora:
        return _corpora[geo]
    dim, nbits, ws = geo
    spec = synth.SynthSpec(num_docs=N_RANDOM, num_centroids=K, dim=dim, nbits=nbits, doc_len_min=3, doc_len_max=32,
                           seed=4100 + dim + 7 * nbits)
    codes, res, lens = synth.doc_tokens(spec, 0, N_RANDOM)
    pc, pr, _ = synth.doc_tokens(spec, N_RANDOM, N_RANDOM + 60)     # a token pool for the planted documents
    assert pc.size > sum(PLANTED)
    off = np.concatenate([[0], np.cumsum(lens)])
    cs, rs, ls, at = [codes], [res], list(lens), 0
    for n in PLANTED:
        cs.append(pc[at:at + n]); rs.append(pr[at:at + n]); ls.append(n); at += n
    for _ in range(2):
        cs.append(codes[off[3]:off[4]]); rs.append(res[off[3]:off[4]]); ls.append(int(lens[3]))
    cs.append(np.repeat(pc[at:at + 1], 40)); rs.append(np.repeat(pr[at:at + 1], 40, axis=0)); ls.append(40)
    codes, res, lens = np.concatenate(cs), np.concatenate(rs), np.asarray(ls, np.int64)
    ivf, ivf_lengths = synth.build_ivf(codes, lens, K)
    _, wts = synth.bucket_tables(spec)
    a = dict(nbits=nbits, centroids=synth.centroids(spec), bucket_weights=(wts * F32(2.0 ** ws)).astype(F32), ivf=ivf,
             ivf_lengths=ivf_lengths, doc_lengths=lens, codes=codes, residuals=np.ascontiguousarray(res))
    _corpora[geo] = a
    return a


def repeated_doc(a):
    return len(a["doc_lengths"]) - 1


def make_queries(a, lq, seed):
    """One batch: QUERY_KINDS in order.  near: noised tokens of one document; negated: minus the (noised) token of the
    repeated-token document, so every similarity to that document is negative; random: unit vectors; nan: one NaN value;
    huge / tiny: scaled by 3e13 / 1e-20."""
    p = prepare(a)
    D = decompress64(p)
    g = np.random.default_rng(seed)
    dim, N = p.dim, p.off.size - 1

    def unit(v):
        return (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)).astype(F32)

    def near(doc):
        t = p.off[doc] + g.integers(0, p.off[doc + 1] - p.off[doc], lq)
        return unit(D[t] + (0.5 / np.sqrt(dim)) * g.standard_normal((lq, dim)))
    out = []
    for kind in QUERY_KINDS:
        doc = int(g.integers(0, N_RANDOM))
        while p.off[doc + 1] == p.off[doc]:
            doc = (doc + 1) % N_RANDOM
        if kind == "negated":
            v = -near(repeated_doc(a))
        elif kind == "random":
            v = unit(g.standard_normal((lq, dim)))
        else:
            v = near(doc)
        if kind == "nan":
            v[lq // 2, dim // 3] = np.nan
        elif kind == "huge":
            v = (v * F32(3e13)).astype(F32)
        elif kind == "tiny":
            v = (v * F32(1e-20)).astype(F32)
        out.append(np.ascontiguousarray(v, F32))
    return out


DEFAULT_KNOBS = dict(s6_lds=1, s6_tiles=1, exact_rowmax=0, s6_xcd=1)


@dataclass(frozen=True)
class Case:
    geo: tuple
    lq: int
    precision: int
    knobs: tuple = ()          # ((name, value), ...) over DEFAULT_KNOBS
    s1_split: bool = False     # knob on and 0 < centroid_batch_size < K, through search_batch

    @property
    def name(self):
        k = "".join(f"-{n}{v}" for n, v in self.knobs)
        return f"{geo_name(self.geo)}-q{self.lq}-p{self.precision}{k}" + ("-split" if self.s1_split else "")

    def knob(self, n):
        return dict(self.knobs).get(n, DEFAULT_KNOBS[n])

    @property
    def form(self):
        return kernel_form(self.precision, self.geo[1], self.lq, self.knob)


FORMS = ("exact_f32_kernel", "exact_bf16_kernel", "exact_qc_kernel", "exact_qct_kernel<one tile>",
         "exact_qct_kernel<two tiles>", "exact_qcl_kernel<3 waves>", "exact_qcl_kernel<4 waves>")


def kernel_form(precision, nbits, lq, knob):
    """Mirror of launch_exact / launch_exact_qt (np_search.hip): (kernel form, NQT) a search of queries of `lq` tokens
    takes.  nbits: of the file (1 bit is stored as 2); knob(name): the tuning value."""
    lqp = (max(lq, 1) + 31) // 32 * 32
    nqt = 1 if lqp <= 32 else (2 if lqp <= 64 else 8)
    if nbits == 8 or precision == 0:
        return FORMS[0], nqt
    if precision == 3:
        return FORMS[1], nqt
    if not knob("exact_rowmax") and (nqt == 1 or knob("s6_tiles")):      # one launch per 32-token query tile
        return {0: FORMS[3], 1: FORMS[5], 2: FORMS[6]}[knob("s6_lds")], nqt
    if nqt <= 2 and not knob("exact_rowmax"):
        return FORMS[4], nqt
    return FORMS[2], nqt


def _cases():
    out = []
    # every geometry x every precision at the default knobs; the query length rotates so that every length meets every
    # precision (18 geometries over 8 lengths)
    for gi, geo in enumerate(GEOMETRIES):
        for prec in range(4):
            out.append(Case(geo, QUERY_LENGTHS[(gi + 3 * prec) % 8], prec))
    # the plain bf16 kernel and the f32 kernel at every query length
    native = [g for g in GEOMETRIES if g[1] in (2, 4)]
    for li, lq in enumerate(QUERY_LENGTHS):
        out.append(Case(native[(2 * li + 1) % len(native)], lq, 3))
        out.append(Case(GEOMETRIES[(3 * li + 2) % len(GEOMETRIES)], lq, 0))
    # every knob value x every query length x precisions 1 and 2 (the QC-reuse kernel forms)
    forms = [(("s6_lds", 0),), (("s6_lds", 2),), (("s6_lds", 0), ("s6_tiles", 0)), (("exact_rowmax", 1),),
             (("s6_xcd", 0),), (("s6_lds", 0), ("s6_xcd", 0)), (("s6_tiles", 0),)]
    i = 0
    for kn in forms:
        for lq in QUERY_LENGTHS:
            for prec in (1, 2):
                out.append(Case(native[i % len(native)], lq, prec, kn))
                i += 5
    # the split-bf16 S1 table as C-in
    for geo, lq in (((128, 4, 0), 32), ((64, 2, 0), 65), ((100, 4, 0), 33), ((128, 4, -6), 64)):
        for prec in (1, 2):
            out.append(Case(geo, lq, prec, (), True))
    # built for the mutants: one-token queries against a residual-dominated corpus
    for prec in (1, 2):
        out.append(Case((128, 4, 2), 1, prec))
    return list(dict.fromkeys(out))


CASES = _cases()


def case_queries(c):
    return make_queries(make_corpus(c.geo), c.lq, seed=9000 + 31 * c.lq + c.geo[0] + c.geo[1] + 5 * c.geo[2])


# which cases are built to catch which mutant (tests/test_exact_bounds_cpu.py asserts every entry)
CATCHES = {
    "a": ["d128b4w+2-q1-p2", "d128b4w+2-q65-p2"],
    "b": ["d128b4w+2-q1-p2"],
    "c": ["d128b4w+2-q1-p2", "d128b4-q65-p2"],
    "d": ["d128b4w-6-q31-p1"],
    "e": ["d128b4-q65-p2", "d64b2-q32-p0"],
    "f": ["d32b4-q256-p2", "d128b4-q65-p2"],
    "g": ["d100b4w+2-q1-p0", "d48b4-q64-p0"],
    "h": ["d32b2-q200-p2", "d128b4-q65-p2"],
    "i": ["d128b4-q65-p2", "d32b2-q1-p0"],
    "j": ["d128b4w+2-q1-p2"],
    "k": ["d128b4w+2-q1-p2"],
}
