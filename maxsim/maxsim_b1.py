"""Binary document rows for batched MaxSim: pack_rows_b1 (np_hip_pack_rows_b1) and maxsim_scores_b1 (np_hip_maxsim_batch_b1),
the Python mirror of maxsim/np_maxsim_b1.hip.  It builds on next_plaid_amd.api, whose conventions it keeps: numpy arrays go
through the host entries, torch tensors on the device through the device entries on torch's current stream."""
import ctypes as C

import numpy as np

from next_plaid_amd import api
from next_plaid_amd.api import NP_DT_BF16, NP_DT_F32, ShapeError, _check, _is_torch, _maxsim_pack, _ptr

_typed = False


def lib():
    """api.lib() with the argument types of the four entries set."""
    global _typed
    L = api.lib()
    if not _typed:
        i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
        L.np_hip_maxsim_batch_b1.argtypes = [i32, i32, vp, vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp]
        L.np_hip_maxsim_batch_b1_device.argtypes = [i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
        L.np_hip_pack_rows_b1.argtypes = [i32, i32, i32, vp, i64, vp, vp]
        L.np_hip_pack_rows_b1_device.argtypes = [i32, i32, i32, vp, i64, vp, vp, vp]
        _typed = True
    return L


def pack_rows_b1(rows, device: int = 0):
    """[n, dim] rows -> (bits [n, ceil(dim / 32)], scales f32 [n]): bit j of word w is x[32 w + j] >= 0 (pad bits 0), scale =
    sum|x| / dim; a row with a non-finite element gets scale NaN.  numpy (float32; anything else is converted) gives uint32
    words; a float32 or bfloat16 torch tensor on the device gives tensors, the words as int32 (the same bits)."""
    if rows.ndim != 2:
        raise ShapeError(f"Shape error: rows has shape {tuple(rows.shape)}")
    n, dim = int(rows.shape[0]), int(rows.shape[1])
    W = (dim + 31) // 32
    if _is_torch(rows):
        import torch
        if rows.dtype not in (torch.float32, torch.bfloat16) or not rows.is_cuda:
            raise ValueError("pack_rows_b1: a tensor must be float32 or bfloat16, on the GPU")
        rows = rows.contiguous()
        bits = torch.zeros((n, W), dtype=torch.int32, device=rows.device)
        scales = torch.zeros(n, dtype=torch.float32, device=rows.device)
        tp = lambda x: C.c_void_p(x.data_ptr())    # noqa: E731
        _check(lib().np_hip_pack_rows_b1_device(
            rows.device.index or 0, NP_DT_BF16 if rows.dtype == torch.bfloat16 else NP_DT_F32, dim, tp(rows), n, tp(bits),
            tp(scales), C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)))
        return bits, scales
    rows = np.ascontiguousarray(rows, np.float32)
    bits, scales = np.zeros((n, W), np.uint32), np.zeros(n, np.float32)
    _check(lib().np_hip_pack_rows_b1(int(device), NP_DT_F32, dim, _ptr(rows), n, _ptr(bits), _ptr(scales)))
    return bits, scales


def _scales(s, rows, what, name):
    """One f32 scale per row of `rows`, flat and where the rows are (a list that parallels the row list is concatenated)."""
    if _is_torch(rows):
        import torch
        s = s if _is_torch(s) else torch.cat([x.reshape(-1) for x in s] + [torch.zeros(0, device=rows.device)])
        s = torch.cat([s.to(rows.device, torch.float32).reshape(-1), torch.zeros(1, device=rows.device)])   # never NULL
    else:
        s = np.concatenate([np.ravel(x) for x in ([s] if isinstance(s, np.ndarray) else s)] + [np.zeros(1)]).astype(np.float32)
    if s.shape[0] - 1 != rows.shape[0]:
        raise ValueError(f"{name}: {what}_scales holds one scale per {what} row")
    return s


def maxsim_scores_b1(queries, query_scales, doc_bits, document_scales, pairs=None, return_matches: bool = False, device: int = 0,
                     query_offsets=None, document_offsets=None):
    """np_hip_maxsim_batch_b1: MaxSim of int8 query rows [tokens, dim] against binary document rows [tokens, ceil(dim / 32)]
    (pack_rows_b1's words; a set bit is +1, a clear bit -1), one f32 scale per row on both sides: sim = (integer dot
    product) * document scale * query scale.  Lists of arrays, or flat arrays with query_offsets / document_offsets; scales
    as lists that parallel them or flat.  numpy (int8 / uint32) or torch device tensors (int8 / int32).  pairs: one list of
    document ids per query, None = all pairs.  Returns what api.maxsim_scores returns: per query its scores, with
    return_matches a tuple (scores, sims [n_i, Lq_i], positions i32 [n_i, Lq_i])."""
    L = lib()
    return _scores_words("maxsim_scores_b1", "doc_bits", 32, L.np_hip_maxsim_batch_b1, L.np_hip_maxsim_batch_b1_device, queries,
                         query_scales, doc_bits, document_scales, pairs, return_matches, device, query_offsets, document_offsets)


def _scores_words(name, words, per_word, host_entry, device_entry, queries, query_scales, doc_bits, document_scales, pairs,
                  return_matches, device, query_offsets, document_offsets):
    """maxsim_scores_b1 for any form whose document rows are 32-bit words of `per_word` dims (maxsim_i4.py: 8) and whose two C
    entries take the _b1 argument lists; `name` and `words` are what the messages call the function and the rows."""
    qf, qoff = _maxsim_pack(queries, query_offsets, "query")
    df, doff = _maxsim_pack(doc_bits, document_offsets, "document")
    if qoff.size <= 1:
        return []
    on_dev = _is_torch(qf)
    if on_dev != _is_torch(df):
        raise ValueError(f"{name}: queries and {words} must both be numpy arrays or both torch tensors")
    if qf.ndim != 2 or df.ndim != 2 or df.shape[1] != (qf.shape[1] + per_word - 1) // per_word:
        raise ShapeError(f"Shape error: queries {tuple(qf.shape)} must be [tokens, dim] and {words} {tuple(df.shape)} [tokens, ceil(dim / {per_word})]")
    qs, ds = _scales(query_scales, qf, "query", name), _scales(document_scales, df, "document", name)
    dim = int(qf.shape[1])
    B, n_docs = qoff.size - 1, doff.size - 1
    qoff32 = np.ascontiguousarray(qoff, np.int32)
    if pairs is None:
        ids = poff = None
        n = np.full(B, n_docs, np.int64)
    else:
        lists = [np.ascontiguousarray(x, np.int64).reshape(-1) for x in pairs]
        if len(lists) != B:
            raise ValueError(f"pairs has {len(lists)} entries for {B} queries")
        n = np.array([x.size for x in lists], np.int64)
        poff = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        ids = np.concatenate(lists + [np.zeros(1, np.int64)])    # never NULL
    lq = np.maximum(np.diff(qoff), 0)
    P, R = int(n.sum()), int((n * lq).sum())
    if on_dev:
        import torch
        if qf.dtype != torch.int8 or df.dtype != torch.int32 or not qf.is_cuda or not df.is_cuda:
            raise ValueError(f"{name}: device tensors must be int8 queries and int32 words, on the GPU")
        dev = qf.device
        qf, df = qf.contiguous(), df.contiguous()
        t = lambda a: None if a is None else torch.from_numpy(a).to(dev)   # noqa: E731
        tp = lambda x: None if x is None else C.c_void_p(x.data_ptr())    # noqa: E731
        d_qoff, d_doff, d_ids, d_poff = t(qoff32), t(doff), t(ids), t(poff)
        sc = torch.zeros(max(P, 1), dtype=torch.float32, device=dev)
        sims = torch.zeros(max(R, 1), dtype=torch.float32, device=dev) if return_matches else None
        pos = torch.zeros(max(R, 1), dtype=torch.int32, device=dev) if return_matches else None
        _check(device_entry(dev.index or 0, dim, tp(qf), tp(qs), tp(d_qoff), _ptr(qoff32), B, tp(df), tp(ds), tp(d_doff), _ptr(doff),
                            n_docs, tp(d_ids), tp(d_poff), _ptr(poff), tp(sc), tp(sims), tp(pos),
                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    else:
        qf, df = np.ascontiguousarray(qf, np.int8), np.ascontiguousarray(df, np.uint32)
        sc = np.zeros(max(P, 1), np.float32)
        sims = np.zeros(max(R, 1), np.float32) if return_matches else None
        pos = np.zeros(max(R, 1), np.int32) if return_matches else None
        _check(host_entry(int(device), dim, _ptr(qf), _ptr(qs), _ptr(qoff32), B, _ptr(df), _ptr(ds), _ptr(doff), n_docs, _ptr(ids),
                          _ptr(poff), _ptr(sc), _ptr(sims), _ptr(pos)))
    out, p0, r0 = [], 0, 0
    for i in range(B):
        ni, li = int(n[i]), int(lq[i])
        if return_matches:
            out.append((sc[p0:p0 + ni], sims[r0:r0 + ni * li].reshape(ni, li), pos[r0:r0 + ni * li].reshape(ni, li)))
        else:
            out.append(sc[p0:p0 + ni])
        p0, r0 = p0 + ni, r0 + ni * li
    return out
