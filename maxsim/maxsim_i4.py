"""Int4 document rows for batched MaxSim: quantize_rows_i4 (np_hip_quantize_rows_i4) and maxsim_scores_i4
(np_hip_maxsim_batch_i4), the Python mirror of maxsim/np_maxsim_i4.hip.  The conventions are maxsim_b1.py's, whose staging
it shares: numpy arrays go through the host entries, torch tensors on the device through the device entries on torch's
current stream."""
import ctypes as C

import numpy as np

from maxsim.maxsim_b1 import _scores_words
from next_plaid_amd import api
from next_plaid_amd.api import NP_DT_BF16, NP_DT_F32, ShapeError, _check, _is_torch, _ptr

_typed = False


def lib():
    """api.lib() with the argument types of the four entries set."""
    global _typed
    L = api.lib()
    if not _typed:
        i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
        L.np_hip_maxsim_batch_i4.argtypes = [i32, i32, vp, vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp]
        L.np_hip_maxsim_batch_i4_device.argtypes = [i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
        L.np_hip_quantize_rows_i4.argtypes = [i32, i32, i32, vp, i64, vp, vp]
        L.np_hip_quantize_rows_i4_device.argtypes = [i32, i32, i32, vp, i64, vp, vp, vp]
        _typed = True
    return L


def quantize_rows_i4(rows, device: int = 0):
    """[n, dim] rows -> (words [n, ceil(dim / 8)], scales f32 [n]): nibble j of word w is the two's-complement code of
    x[8 w + j], clamp(rint(x * (7 / a)), -7, 7) with a = max|x| (pad nibbles 0), scale = a / 7; a row with a non-finite
    element gets scale NaN and codes 0.  numpy (float32; anything else is converted) gives uint32 words; a float32 or bfloat16
    torch tensor on the device gives tensors, the words as int32 (the same bits)."""
    if rows.ndim != 2:
        raise ShapeError(f"Shape error: rows has shape {tuple(rows.shape)}")
    n, dim = int(rows.shape[0]), int(rows.shape[1])
    W = (dim + 7) // 8
    if _is_torch(rows):
        import torch
        if rows.dtype not in (torch.float32, torch.bfloat16) or not rows.is_cuda:
            raise ValueError("quantize_rows_i4: a tensor must be float32 or bfloat16, on the GPU")
        rows = rows.contiguous()
        words = torch.zeros((n, W), dtype=torch.int32, device=rows.device)
        scales = torch.zeros(n, dtype=torch.float32, device=rows.device)
        tp = lambda x: C.c_void_p(x.data_ptr())    # noqa: E731
        _check(lib().np_hip_quantize_rows_i4_device(
            rows.device.index or 0, NP_DT_BF16 if rows.dtype == torch.bfloat16 else NP_DT_F32, dim, tp(rows), n, tp(words),
            tp(scales), C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)))
        return words, scales
    rows = np.ascontiguousarray(rows, np.float32)
    words, scales = np.zeros((n, W), np.uint32), np.zeros(n, np.float32)
    _check(lib().np_hip_quantize_rows_i4(int(device), NP_DT_F32, dim, _ptr(rows), n, _ptr(words), _ptr(scales)))
    return words, scales


def maxsim_scores_i4(queries, query_scales, doc_words, document_scales, pairs=None, return_matches: bool = False, device: int = 0,
                     query_offsets=None, document_offsets=None):
    """np_hip_maxsim_batch_i4: MaxSim of int8 query rows [tokens, dim] against int4 document rows [tokens, ceil(dim / 8)]
    (quantize_rows_i4's words: eight two's-complement nibbles each, -8 .. 7), one f32 scale per row on both sides: sim =
    (integer dot product) * document scale * query scale.  Arguments, forms (numpy int8 / uint32 or torch device tensors int8 /
    int32) and the result are maxsim_b1.maxsim_scores_b1's."""
    L = lib()
    return _scores_words("maxsim_scores_i4", "doc_words", 8, L.np_hip_maxsim_batch_i4, L.np_hip_maxsim_batch_i4_device, queries,
                         query_scales, doc_words, document_scales, pairs, return_matches, device, query_offsets, document_offsets)
