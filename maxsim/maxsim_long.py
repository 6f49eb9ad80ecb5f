"""Queries of any length for batched MaxSim: maxsim_scores_long (np_hip_maxsim_batch_long), the Python mirror of
maxsim/np_maxsim_long.hip.  The conventions are maxsim_f16.py's: numpy arrays go through the host entry, torch tensors on the
device through the device entry on torch's current stream.  Nothing is converted: rows are float32, or bf16 as torch.bfloat16
or raw uint16 words, queries and documents alike."""
import ctypes as C

import numpy as np

from next_plaid_amd import api
from next_plaid_amd.api import NP_DT_BF16, NP_DT_F32, ShapeError, _check, _is_torch, _maxsim_pack, _ptr

_typed = False


def lib():
    """api.lib() with the argument types of the two entries set."""
    global _typed
    L = api.lib()
    if not _typed:
        i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
        L.np_hip_maxsim_batch_long.argtypes = [i32, i32, i32, i32, vp, vp, i32, vp, vp, i64, vp, vp, vp, vp, vp]
        L.np_hip_maxsim_batch_long_device.argtypes = [i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
        _typed = True
    return L


def maxsim_scores_long(queries, documents, pairs=None, precision: int = 0, return_matches: bool = False, device: int = 0,
                       query_offsets=None, document_offsets=None):
    """np_hip_maxsim_batch_long: api.maxsim_scores for queries of any number of tokens (f32 or bf16 rows; no int8 scales).
    queries / documents: lists of [tokens, dim] arrays, or one flat [tokens, dim] array each with query_offsets /
    document_offsets; all numpy (the host entry) or all torch tensors on the GPU (the device entry, torch's current stream;
    tensors come back), all float32, or all bf16 (torch.bfloat16, or uint16 words in numpy or torch) with precision 3.
    Anything else raises ValueError and is not converted.  pairs: one list of document ids per query (any order, repeats
    allowed), None = all pairs.  Returns what api.maxsim_scores returns: per query its scores, with return_matches a tuple
    (scores, sims [n_i, Lq_i], positions i32 [n_i, Lq_i])."""
    mats = ([queries] if query_offsets is not None else list(queries)) + ([documents] if document_offsets is not None else list(documents))
    on_dev = bool(mats) and _is_torch(mats[0])
    kinds = {str(x.dtype).replace("torch.", "") for x in mats}
    if on_dev:
        ok = all(_is_torch(x) and x.is_cuda for x in mats)
    else:
        ok = all(isinstance(x, np.ndarray) for x in mats)
    if not ok or len(kinds) > 1 or not kinds <= {"float32", "bfloat16", "uint16"}:
        raise ValueError("maxsim_scores_long: queries and documents must all be numpy arrays or all torch tensors on the GPU, "
                         "all float32 or all bf16 (bfloat16 / uint16 words)")
    dtype = NP_DT_F32 if kinds <= {"float32"} else NP_DT_BF16
    qf, qoff = _maxsim_pack(queries, query_offsets, "query")
    if qoff.size <= 1:
        return []
    df, doff = _maxsim_pack(documents, document_offsets, "document")
    if doff.size <= 1:
        df = qf[:0]
    if qf.ndim != 2 or df.ndim != 2 or qf.shape[1] != df.shape[1]:
        raise ShapeError(f"Shape error: queries {tuple(qf.shape)} and documents {tuple(df.shape)} must be [tokens, dim] of one dim")
    qf, df = (x.contiguous() for x in (qf, df)) if on_dev else (np.ascontiguousarray(x) for x in (qf, df))
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
    lq = np.diff(qoff)
    P, R = int(n.sum()), int((n * lq).sum())
    L = lib()
    if on_dev:
        import torch
        dev = qf.device
        t = lambda a: None if a is None else torch.from_numpy(a).to(dev)   # noqa: E731
        tp = lambda x: None if x is None else C.c_void_p(x.data_ptr())    # noqa: E731
        d_qoff, d_doff, d_ids, d_poff = t(qoff32), t(doff), t(ids), t(poff)
        sc = torch.zeros(max(P, 1), dtype=torch.float32, device=dev)
        sims = torch.zeros(max(R, 1), dtype=torch.float32, device=dev) if return_matches else None
        pos = torch.zeros(max(R, 1), dtype=torch.int32, device=dev) if return_matches else None
        _check(L.np_hip_maxsim_batch_long_device(dev.index or 0, dtype, int(precision), dim, tp(qf), tp(d_qoff), _ptr(qoff32), B,
                                                 tp(df), tp(d_doff), _ptr(doff), n_docs, tp(d_ids), tp(d_poff), _ptr(poff), tp(sc),
                                                 tp(sims), tp(pos), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    else:
        sc = np.zeros(max(P, 1), np.float32)
        sims = np.zeros(max(R, 1), np.float32) if return_matches else None
        pos = np.zeros(max(R, 1), np.int32) if return_matches else None
        _check(L.np_hip_maxsim_batch_long(int(device), dtype, int(precision), dim, _ptr(qf), _ptr(qoff32), B, _ptr(df), _ptr(doff),
                                          n_docs, _ptr(ids), _ptr(poff), _ptr(sc), _ptr(sims), _ptr(pos)))
    out, p0, r0 = [], 0, 0
    for i in range(B):
        ni, li = int(n[i]), int(lq[i])
        if return_matches:
            out.append((sc[p0:p0 + ni], sims[r0:r0 + ni * li].reshape(ni, li), pos[r0:r0 + ni * li].reshape(ni, li)))
        else:
            out.append(sc[p0:p0 + ni])
        p0, r0 = p0 + ni, r0 + ni * li
    return out
