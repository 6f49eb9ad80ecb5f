"""np_hip_pack_rows_b1 restated in numpy, bit for bit, and the unpacking that turns binary rows into the +-1 int8 codes
maxsim_i8_restate.pair scores (test infrastructure; no GPU).  Plus the table of refused calls the CPU test walks."""
import ctypes as C

import numpy as np

F32 = np.float32


def unpack(bits, dim):
    """[n, ceil(dim / 32)] words -> [n, dim] int8 of +-1: bit j of word w is dim 32 w + j, set = +1; pad bits are dropped."""
    b = np.ascontiguousarray(bits).view(np.uint32)
    on = (b[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return (2 * on.reshape(len(b), 32 * b.shape[1])[:, :dim].astype(np.int8) - 1).astype(np.int8)


def pack(x, el=4):
    """(bits uint32 [n, W], scales f32 [n]) of f32 rows; el = dims per 16-byte unit of the input, 4 (f32) or 8 (bf16).  The
    sum of |x|: unit u belongs to lane u % 64, a lane adds its elements in ascending dim order, then the xor butterfly 32 .. 1."""
    x = np.asarray(x, F32)
    n, dim = x.shape
    on = np.zeros((n, (dim + 31) // 32 * 32), np.uint32)
    on[:, :dim] = x >= 0
    bits = (on.reshape(n, -1, 32) << np.arange(32, dtype=np.uint32)).sum(2).astype(np.uint32)
    a = np.zeros((n, 1024), F32)
    a[:, :dim] = np.abs(x)
    a = a.reshape(n, 1024 // (64 * el), 64, el)
    with np.errstate(all="ignore"):
        s = np.zeros((n, 64), F32)
        for u in range(a.shape[1]):
            for i in range(el):
                s = s + a[:, u, :, i]
        for d in (32, 16, 8, 4, 2, 1):
            s = s + s[:, np.arange(64) ^ d]
        scale = np.where(np.isfinite(x).all(1), s[:, 0] / F32(dim), F32(np.nan)).astype(F32)
    return bits, scale


# (name, entry: "s" = maxsim_batch_b1 / "p" = pack_rows_b1, overrides of a valid call, status, a word of the message)
REFUSALS = [("dim0", "s", dict(dim=0), 3, "dim"), ("dim1025", "s", dict(dim=1025), 3, "dim"), ("query257", "s", dict(qoff=[0, 257]), 3, "q_tok_offsets"),
            ("q_scales_null", "s", dict(qs=None), 8, "q_scales"), ("d_scales_null", "s", dict(ds=None), 8, "d_scales"),
            ("doc_bits_null", "s", dict(bits=None), 8, "doc_bits"),
            ("doc_offsets_decrease", "s", dict(doff=[0, 5, 3, 9]), 8, "doc_tok_offsets"), ("pair_id_n_docs", "s", dict(ids=[0, 3]), 8, "pair_docs"),
            ("pack_dtype_i8", "p", dict(dtype=2), 8, "dtype"), ("pack_dim0", "p", dict(dim=0), 3, "dim"), ("pack_dim1025", "p", dict(dim=1025), 3, "dim")]


def refused_call(lib, entry, over):
    """A small valid call (1 query of 4 tokens, 3 documents, 2 listed pairs, dim 8; or 4 rows to pack) with `over` applied,
    through the C entry.  Returns (status, message, outputs_untouched)."""
    a = dict(dim=8, qoff=[0, 4], doff=[0, 5, 7, 9], ids=[2, 0], qs=np.ones(300, F32), ds=np.ones(300, F32), dtype=0,
             bits=np.full((300, 40), 7, np.uint32))
    a.update(over)
    p = lambda x: None if x is None else np.asarray(x).ctypes.data_as(C.c_void_p)   # noqa: E731
    rows, codes, words = np.ones((300, 1100), F32), np.full((300, 1100), 7, np.int8), np.full((300, 40), 7, np.uint32)
    sc, sims, pos = np.full(300, 7.0, F32), np.full(2048, 7.0, F32), np.full(2048, 7, np.int32)
    if entry == "p":
        rc = lib.np_hip_pack_rows_b1(0, a["dtype"], a["dim"], p(rows), 4, p(words), p(sc))
    else:
        keep = [np.asarray(a["qoff"], np.int32), np.asarray(a["doff"], np.int64), np.asarray(a["ids"], np.int64), np.asarray([0, len(a["ids"])], np.int64)]
        rc = lib.np_hip_maxsim_batch_b1(0, a["dim"], p(codes), p(a["qs"]), p(keep[0]), 1, p(a["bits"]), p(a["ds"]), p(keep[1]), 3, p(keep[2]),
                                        p(keep[3]), p(sc), p(sims), p(pos))
    return rc, lib.np_hip_last_error().decode(), bool((sc == 7).all() and (sims == 7).all() and (pos == 7).all() and (words == 7).all())
