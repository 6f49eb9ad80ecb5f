"""Queries of any length for batched MaxSim: maxsim_scores_long (np_hip_maxsim_batch_long) and maxsim_scores_long_i8
(np_hip_maxsim_batch_long_i8), the Python mirrors of maxsim/np_maxsim_long.hip and maxsim/np_maxsim_long_i8.hip.  The
conventions are maxsim_f16.py's: numpy arrays go through the host entry, torch tensors on the device through the device entry
on torch's current stream.  Nothing is converted: rows are float32, or bf16 as torch.bfloat16 or raw uint16 words, queries and
documents alike; the int8 mirror takes int8 rows with float32 scales."""
import ctypes as C

import numpy as np

from next_plaid_amd import api
from next_plaid_amd.api import NP_DT_BF16, NP_DT_F32, ShapeError, _check, _is_torch, _maxsim_pack, _maxsim_scales, _ptr

_typed = False


def lib():
    """api.lib() with the argument types of the four entries set."""
    global _typed
    L = api.lib()
    if not _typed:
        i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
        L.np_hip_maxsim_batch_long.argtypes = [i32, i32, i32, i32, vp, vp, i32, vp, vp, i64, vp, vp, vp, vp, vp]
        L.np_hip_maxsim_batch_long_device.argtypes = [i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
        L.np_hip_maxsim_batch_long_i8.argtypes = [i32, i32, vp, vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp]
        L.np_hip_maxsim_batch_long_i8_device.argtypes = [i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
        _typed = True
    return L


def _rows(queries, documents, query_offsets, document_offsets, allowed, message):
    """What both mirrors check first: every matrix numpy or every matrix a torch tensor on the GPU, of one dtype out of
    `allowed` (ValueError(message) otherwise).  Returns (on_dev, dtype name, flat queries, their offsets, flat documents, their
    offsets), the flat arrays contiguous; the query offsets have one entry when there is no query."""
    mats = ([queries] if query_offsets is not None else list(queries)) + ([documents] if document_offsets is not None else list(documents))
    on_dev = bool(mats) and _is_torch(mats[0])
    kinds = {str(x.dtype).replace("torch.", "") for x in mats}
    if on_dev:
        ok = all(_is_torch(x) and x.is_cuda for x in mats)
    else:
        ok = all(isinstance(x, np.ndarray) for x in mats)
    if not ok or len(kinds) > 1 or not kinds <= allowed:
        raise ValueError(message)
    qf, qoff = _maxsim_pack(queries, query_offsets, "query")
    if qoff.size <= 1:
        return on_dev, "", qf, qoff, None, None
    df, doff = _maxsim_pack(documents, document_offsets, "document")
    if doff.size <= 1:
        df = qf[:0]
    if qf.ndim != 2 or df.ndim != 2 or qf.shape[1] != df.shape[1]:
        raise ShapeError(f"Shape error: queries {tuple(qf.shape)} and documents {tuple(df.shape)} must be [tokens, dim] of one dim")
    qf, df = (x.contiguous() for x in (qf, df)) if on_dev else (np.ascontiguousarray(x) for x in (qf, df))
    return on_dev, "".join(kinds), qf, qoff, df, doff


def _call(host, dev, head, on_dev, q, qoff, d, doff, pairs, return_matches, device):
    """One call of an entry pair whose argument lists are (device, *head, *q, query offsets, B, *d, document offsets, n_docs,
    pairs, outputs): q / d = the flat rows, followed by their scales where the entries take them.  Returns what
    api.maxsim_scores returns."""
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
    lq = np.diff(qoff)
    P, R = int(n.sum()), int((n * lq).sum())
    if on_dev:
        import torch
        where = q[0].device
        t = lambda a: None if a is None else torch.from_numpy(a).to(where)   # noqa: E731
        tp = lambda x: None if x is None else C.c_void_p(x.data_ptr())    # noqa: E731
        d_qoff, d_doff, d_ids, d_poff = t(qoff32), t(doff), t(ids), t(poff)
        sc = torch.zeros(max(P, 1), dtype=torch.float32, device=where)
        sims = torch.zeros(max(R, 1), dtype=torch.float32, device=where) if return_matches else None
        pos = torch.zeros(max(R, 1), dtype=torch.int32, device=where) if return_matches else None
        _check(dev(where.index or 0, *head, *map(tp, q), tp(d_qoff), _ptr(qoff32), B, *map(tp, d), tp(d_doff), _ptr(doff), n_docs,
                   tp(d_ids), tp(d_poff), _ptr(poff), tp(sc), tp(sims), tp(pos), C.c_void_p(torch.cuda.current_stream(where).cuda_stream)))
    else:
        sc = np.zeros(max(P, 1), np.float32)
        sims = np.zeros(max(R, 1), np.float32) if return_matches else None
        pos = np.zeros(max(R, 1), np.int32) if return_matches else None
        _check(host(int(device), *head, *map(_ptr, q), _ptr(qoff32), B, *map(_ptr, d), _ptr(doff), n_docs, _ptr(ids), _ptr(poff),
                    _ptr(sc), _ptr(sims), _ptr(pos)))
    out, p0, r0 = [], 0, 0
    for i in range(B):
        ni, li = int(n[i]), int(lq[i])
        if return_matches:
            out.append((sc[p0:p0 + ni], sims[r0:r0 + ni * li].reshape(ni, li), pos[r0:r0 + ni * li].reshape(ni, li)))
        else:
            out.append(sc[p0:p0 + ni])
        p0, r0 = p0 + ni, r0 + ni * li
    return out


def maxsim_scores_long(queries, documents, pairs=None, precision: int = 0, return_matches: bool = False, device: int = 0,
                       query_offsets=None, document_offsets=None):
    """np_hip_maxsim_batch_long: api.maxsim_scores for queries of any number of tokens (f32 or bf16 rows; no int8 scales).
    queries / documents: lists of [tokens, dim] arrays, or one flat [tokens, dim] array each with query_offsets /
    document_offsets; all numpy (the host entry) or all torch tensors on the GPU (the device entry, torch's current stream;
    tensors come back), all float32, or all bf16 (torch.bfloat16, or uint16 words in numpy or torch) with precision 3.
    Anything else raises ValueError and is not converted.  pairs: one list of document ids per query (any order, repeats
    allowed), None = all pairs.  Returns what api.maxsim_scores returns: per query its scores, with return_matches a tuple
    (scores, sims [n_i, Lq_i], positions i32 [n_i, Lq_i])."""
    on_dev, kind, qf, qoff, df, doff = _rows(
        queries, documents, query_offsets, document_offsets, {"float32", "bfloat16", "uint16"},
        "maxsim_scores_long: queries and documents must all be numpy arrays or all torch tensors on the GPU, "
        "all float32 or all bf16 (bfloat16 / uint16 words)")
    if qoff.size <= 1:
        return []
    L = lib()
    head = (NP_DT_F32 if kind == "float32" else NP_DT_BF16, int(precision), int(qf.shape[1]))
    return _call(L.np_hip_maxsim_batch_long, L.np_hip_maxsim_batch_long_device, head, on_dev, [qf], qoff, [df], doff, pairs,
                 return_matches, device)


def maxsim_scores_long_i8(queries, documents, query_scales, document_scales, pairs=None, return_matches: bool = False,
                          device: int = 0, query_offsets=None, document_offsets=None):
    """np_hip_maxsim_batch_long_i8: api.maxsim_scores(..., query_scales=, document_scales=) for queries of any number of
    tokens.  Rows are int8 codes (numpy int8, or torch.int8 on the GPU: see api.quantize_rows), the scales float32 with one per
    row -- lists that parallel the row lists, or flat arrays -- and both are there; anything else raises ValueError before the
    library is called, and nothing is converted.  The other arguments and the result are maxsim_scores_long's; matches are
    allowed (the arithmetic is exact)."""
    if query_scales is None or document_scales is None:
        raise ValueError("maxsim_scores_long_i8: query_scales and document_scales go together")
    on_dev, _, qf, qoff, df, doff = _rows(
        queries, documents, query_offsets, document_offsets, {"int8"},
        "maxsim_scores_long_i8: queries and documents must all be numpy arrays or all torch tensors on the GPU, all int8")
    if qoff.size <= 1:
        return []
    for s in (query_scales, document_scales):
        if any("float32" not in str(x.dtype) for x in ([s] if _is_torch(s) or isinstance(s, np.ndarray) else s)):
            raise ValueError("maxsim_scores_long_i8: scales must be float32")
    qs, ds = _maxsim_scales(query_scales, qf, "query"), _maxsim_scales(document_scales, df, "document")   # one per row, or ValueError
    L = lib()
    return _call(L.np_hip_maxsim_batch_long_i8, L.np_hip_maxsim_batch_long_i8_device, (int(qf.shape[1]),), on_dev, [qf, qs], qoff,
                 [df, ds], doff, pairs, return_matches, device)
