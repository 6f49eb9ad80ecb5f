"""np_hip_quantize_rows_i4 restated in numpy, bit for bit, and the unpacking that turns int4 rows into the int8 codes
maxsim_i8_restate.pair scores (test infrastructure; no GPU).  Plus the table of refused calls the CPU test walks."""
import ctypes as C

import numpy as np

F32 = np.float32


def unpack(words, dim):
    """[n, ceil(dim / 8)] words -> [n, dim] int8 in -8 .. 7: nibble j of word w is dim 8 w + j, sign-extended; pad nibbles are dropped."""
    w = np.ascontiguousarray(words).view(np.uint32)
    nib = ((w[:, :, None] >> (4 * np.arange(8, dtype=np.uint32))) & 15).reshape(len(w), 8 * w.shape[1])[:, :dim].astype(np.int16)
    return (nib - 16 * (nib >> 3)).astype(np.int8)


def quantize4(x, el=4):
    """(words uint32 [n, W], scales f32 [n]) of f32 rows: scale = a / 7, code = clamp(rint(x * (7 / a)), -7, 7), pad nibbles 0; NaN
    scale and codes 0 for a non-finite row.  el (dims per 16-byte unit of the input) changes nothing: no step depends on an order."""
    x = np.asarray(x, F32)
    n, dim = x.shape
    a = np.abs(x).max(1, initial=F32(0))
    bad, zero = ~np.isfinite(x).all(1), ~(a > 0)
    with np.errstate(all="ignore"):
        inv = np.where(bad | zero, F32(0), F32(7) / a).astype(F32)
        codes = np.zeros((n, (dim + 7) // 8 * 8), np.int64)
        codes[:, :dim] = np.fmin(np.fmax(np.rint(np.where((bad | zero)[:, None], F32(0), x * inv[:, None])), -7), 7)
        words = ((codes & 15).reshape(n, -1, 8) << (4 * np.arange(8))).sum(2).astype(np.uint32)
        return words, np.where(bad, F32(np.nan), a / F32(7)).astype(F32)


# (name, entry: "s" = maxsim_batch_i4 / "q" = quantize_rows_i4, overrides of a valid call, status, a word of the message)
REFUSALS = [("dim0", "s", dict(dim=0), 3, "dim"), ("dim1025", "s", dict(dim=1025), 3, "dim"), ("query257", "s", dict(qoff=[0, 257]), 3, "q_tok_offsets"),
            ("q_scales_null", "s", dict(qs=None), 8, "q_scales"), ("d_scales_null", "s", dict(ds=None), 8, "d_scales"),
            ("doc_words_null", "s", dict(words=None), 8, "doc_words"),
            ("doc_offsets_decrease", "s", dict(doff=[0, 5, 3, 9]), 8, "doc_tok_offsets"), ("pair_id_n_docs", "s", dict(ids=[0, 3]), 8, "pair_docs"),
            ("quant_dtype_i8", "q", dict(dtype=2), 8, "dtype"), ("quant_dim0", "q", dict(dim=0), 3, "dim"), ("quant_dim1025", "q", dict(dim=1025), 3, "dim")]


def refused_call(lib, entry, over):
    """A small valid call (1 query of 4 tokens, 3 documents, 2 listed pairs, dim 8; or 4 rows to quantise) with `over` applied,
    through the C entry.  Returns (status, message, outputs_untouched)."""
    a = dict(dim=8, qoff=[0, 4], doff=[0, 5, 7, 9], ids=[2, 0], qs=np.ones(300, F32), ds=np.ones(300, F32), dtype=0,
             words=np.full((300, 130), 7, np.uint32))
    a.update(over)
    p = lambda x: None if x is None else np.asarray(x).ctypes.data_as(C.c_void_p)   # noqa: E731
    rows, codes, out = np.ones((300, 1100), F32), np.full((300, 1100), 7, np.int8), np.full((300, 130), 7, np.uint32)
    sc, sims, pos = np.full(300, 7.0, F32), np.full(2048, 7.0, F32), np.full(2048, 7, np.int32)
    if entry == "q":
        rc = lib.np_hip_quantize_rows_i4(0, a["dtype"], a["dim"], p(rows), 4, p(out), p(sc))
    else:
        keep = [np.asarray(a["qoff"], np.int32), np.asarray(a["doff"], np.int64), np.asarray(a["ids"], np.int64), np.asarray([0, len(a["ids"])], np.int64)]
        rc = lib.np_hip_maxsim_batch_i4(0, a["dim"], p(codes), p(a["qs"]), p(keep[0]), 1, p(a["words"]), p(a["ds"]), p(keep[1]), 3, p(keep[2]),
                                        p(keep[3]), p(sc), p(sims), p(pos))
    return rc, lib.np_hip_last_error().decode(), bool((sc == 7).all() and (sims == 7).all() and (pos == 7).all() and (out == 7).all())
