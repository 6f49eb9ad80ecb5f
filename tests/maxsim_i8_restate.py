"""np_hip_quantize_rows_i8 and np_hip_maxsim_batch_i8 restated in numpy, bit for bit (test infrastructure; no GPU): every
step is exact integer arithmetic or ONE f32 rounding, so np.float32 and exact integers reproduce the kernels' bits.  Plus the table
of refused calls that the CPU and the GPU test share."""
import ctypes as C

import numpy as np

F32 = np.float32


def quantize(x):
    """(codes int8, scales f32) of f32 rows: scale = a / 127, code = clip(rint(x * (127 / a))); NaN scale for a non-finite row."""
    x = np.asarray(x, F32)
    a = np.abs(x).max(1, initial=F32(0))
    bad, zero = ~np.isfinite(x).all(1), ~(a > 0)
    with np.errstate(all="ignore"):
        inv = np.where(bad | zero, F32(0), F32(127) / a).astype(F32)
        codes = np.clip(np.rint(np.where((bad | zero)[:, None], F32(0), x * inv[:, None])), -127, 127).astype(np.int8)
        return codes, np.where(bad, F32(np.nan), a / F32(127)).astype(F32)


def okey(x):
    """np_exact.h okey: 0 for a non-finite value, otherwise growing with the f32 (in total order: -0.0 below +0.0)."""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.int64)
    return np.where((b & 0x7F800000) == 0x7F800000, 0, np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000))


def pair(cq, sq, cd, sd):
    """(score f32, sims f32 [Lq], pos i32 [Lq]) of one (query, document) of int8 codes and f32 row scales."""
    lq = cq.shape[0]
    sims, pos = np.zeros(lq, F32), np.full(lq, -1, np.int32)
    if cd.shape[0]:
        with np.errstate(all="ignore"):
            dot = cq.astype(np.float64) @ cd.astype(np.float64).T   # integers below 2^24: exact in f64 (BLAS) as in i32 and f32
            prod = dot.astype(F32) * np.asarray(sd, F32)[None, :]    # one rounding each
            keys = okey(prod)
            best = keys.argmax(1)                                   # the first maximum: the lowest t
            m = prod[np.arange(lq), best] * np.asarray(sq, F32)      # one more
        ok = (keys.max(1) > 0) & np.isfinite(m)
        sims, pos = np.where(ok, m, F32(0)).astype(F32), np.where(ok, best, -1).astype(np.int32)
    score = F32(0)
    for x in sims[pos >= 0]:
        score = F32(score + x)
    return score, sims, pos


# (name, entry: "s" = maxsim_batch_i8 / "q" = quantize_rows_i8, overrides of a valid call, status, a word of the message)
REFUSALS = [("dim0", "s", dict(dim=0), 3, "dim"), ("dim1025", "s", dict(dim=1025), 3, "dim"), ("query257", "s", dict(qoff=[0, 257]), 3, "q_tok_offsets"),
            ("q_scales_null", "s", dict(qs=None), 8, "q_scales"), ("d_scales_null", "s", dict(ds=None), 8, "d_scales"),
            ("doc_offsets_decrease", "s", dict(doff=[0, 5, 3, 9]), 8, "doc_tok_offsets"), ("pair_id_n_docs", "s", dict(ids=[0, 3]), 8, "pair_docs"),
            ("quant_dtype_i8", "q", dict(dtype=2), 8, "dtype"), ("quant_dim0", "q", dict(dim=0), 3, "dim"), ("quant_dim1025", "q", dict(dim=1025), 3, "dim")]


def refused_call(lib, entry, over):
    """A small valid call (1 query of 4 tokens, 3 documents, 2 listed pairs, dim 8; or 4 rows to quantise) with `over` applied,
    through the C entry.  Returns (status, message, outputs_untouched)."""
    a = dict(dim=8, qoff=[0, 4], doff=[0, 5, 7, 9], ids=[2, 0], qs=np.ones(300, F32), ds=np.ones(300, F32), dtype=0)
    a.update(over)
    p = lambda x: None if x is None else np.asarray(x).ctypes.data_as(C.c_void_p)   # noqa: E731
    rows, codes = np.ones((300, 1100), F32), np.full((300, 1100), 7, np.int8)
    sc, sims, pos = np.full(300, 7.0, F32), np.full(2048, 7.0, F32), np.full(2048, 7, np.int32)
    if entry == "q":
        rc = lib.np_hip_quantize_rows_i8(0, a["dtype"], a["dim"], p(rows), 4, p(codes), p(sc))
    else:
        keep = [np.asarray(a["qoff"], np.int32), np.asarray(a["doff"], np.int64), np.asarray(a["ids"], np.int64), np.asarray([0, len(a["ids"])], np.int64)]
        rc = lib.np_hip_maxsim_batch_i8(0, a["dim"], p(codes), p(a["qs"]), p(keep[0]), 1, p(codes), p(a["ds"]), p(keep[1]), 3, p(keep[2]), p(keep[3]),
                                        p(sc), p(sims), p(pos))
    return rc, lib.np_hip_last_error().decode(), bool((sc == 7).all() and (sims == 7).all() and (pos == 7).all() and (codes == 7).all())
