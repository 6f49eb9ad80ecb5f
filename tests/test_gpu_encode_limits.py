"""np_hip_encode_tokens (the S1 GEMM's group keys, encode_argmax_kernel, encode_pack_kernel) held to the answers that
tests/encode_limit_shapes.py states by construction, and to the oracle's, with no tolerance.

tests/test_encode_limits_cpu.py shows on the CPU that the oracle gives those answers and that each wrong rule (>= for >,
first of equal maxima, padded rows admitted, non-finite ordered by value, bits MSB-first) changes one of them.
"""
import numpy as np
import pytest

import encode_limit_shapes as E
from helpers import O, hip_index

pytestmark = pytest.mark.gpu

CASES = E.all_cases()


def _compare(what, case, take, codes, packed, want_codes, want_packed):
    """Names the case, the token and both codes / bytes on the first mismatch.  take: the case's token index per row."""
    bad = np.nonzero(codes != want_codes)[0]
    if bad.size:
        t = int(bad[0])
        note = [text for i, text, _ in case.notes if i == int(take[t])]
        raise AssertionError(f"{case.name} {what}: token {int(take[t])} {note}: code {int(codes[t])}, expected "
                             f"{int(want_codes[t])} ({bad.size} of {codes.size} differ)")
    bad = np.argwhere(packed != want_packed)
    if bad.size:
        t, b = (int(v) for v in bad[0])
        raise AssertionError(f"{case.name} {what}: token {int(take[t])} byte {b}: {int(packed[t, b]):#04x}, expected "
                             f"{int(want_packed[t, b]):#04x} (code {int(codes[t])}, {bad.shape[0]} bytes differ)")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_encode_gives_the_answers_by_construction(case):
    """Every case under gemm_cpw 1 and 2 (one and two 32-centroid fragments per wave in the S1 GEMM): the by-construction
    answers, the oracle's, and the two GEMM forms byte for byte."""
    cen, cut, nbits, x, want_codes, want_packed = case
    rc, rp = O.encode_tokens(x, cen, nbits, cut)
    take = np.arange(x.shape[0])
    hx = hip_index(E.codec_arrays(cen, nbits))
    try:
        got = {}
        for cpw in (1, 2):
            hx.tune("gemm_cpw", cpw)
            codes, packed = hx.encode_tokens(x, cut)
            assert packed.shape == want_packed.shape and codes.dtype == np.int64
            _compare(f"gemm_cpw={cpw} against the construction", case, take, codes, packed, want_codes, want_packed)
            _compare(f"gemm_cpw={cpw} against the oracle", case, take, codes, packed, rc, rp)
            got[cpw] = (codes.copy(), packed.copy())
        assert np.array_equal(got[1][0], got[2][0]) and np.array_equal(got[1][1], got[2][1])
    finally:
        hx.tune("gemm_cpw", 1)
        hx.close()


SLICE_CASES = ("K2113-dupB", "K300-dupA", "K33-neg", "K65-dupB", "pack-d100b4K65-zero", "pack-d8b8K5-ascending",
               "pack-d104b1K7-nan")


@pytest.mark.parametrize("prefix", SLICE_CASES)
def test_slices_of_32_tokens(prefix):
    """A handle opened with max_batch=1 encodes 32 tokens per pass: encode_tokens_impl takes
    S = max(1, min(budget / per_query_bytes, max_batch, 256)) slices of 32 tokens, so max_batch=1 gives S = 1 whatever the
    workspace budget is.  n = 33, 65 and 97 end on a ragged slice of one token, 31 on one of 31; every pass after the first
    reuses the offsets and the workspace.  The result must equal, byte for byte, the same tokens encoded one at a time, in
    reversed order, and through a default handle (one pass), and the answers by construction."""
    case = next(c for c in CASES if c.name.startswith(prefix))
    cen, cut, nbits, x, want_codes, want_packed = case
    take97 = np.arange(97) % x.shape[0]
    if x.shape[0] > 97:                     # the non-finite rows sit at the end of a pack case
        take97 = np.concatenate([np.arange(91), np.arange(x.shape[0] - 6, x.shape[0])])
    h1 = hip_index(E.codec_arrays(cen, nbits), max_batch=1)
    hd = hip_index(E.codec_arrays(cen, nbits))
    try:
        single = [h1.encode_tokens(x[i:i + 1], cut) for i in take97]
        for n in (1, 31, 32, 33, 64, 65, 97):
            take = take97[:n]
            codes, packed = h1.encode_tokens(x[take], cut)
            _compare(f"n={n} in slices of 32", case, take, codes, packed, want_codes[take], want_packed[take])
            c1 = np.concatenate([s[0] for s in single[:n]])
            p1 = np.concatenate([s[1] for s in single[:n]])
            _compare(f"n={n} sliced against one at a time", case, take, codes, packed, c1, p1)
            cr, pr = h1.encode_tokens(x[take[::-1]], cut)
            _compare(f"n={n} sliced against reversed order", case, take, codes, packed, cr[::-1], pr[::-1])
            cd, pd_ = hd.encode_tokens(x[take], cut)
            _compare(f"n={n} sliced against a default handle", case, take, codes, packed, cd, pd_)
    finally:
        h1.close()
        hd.close()


@pytest.mark.parametrize("K,dim,nbits", [(1, 8, 4), (2, 100, 2), (31, 128, 4), (33, 96, 1), (2049, 104, 1), (2113, 128, 8)])
def test_rounded_scores_at_the_same_K(K, dim, nbits):
    """The K values of the grid cases on data whose scores DO round (a centroid plus Gaussian noise, normalised): 203
    distinct tokens against the oracle, through a default handle, under both GEMM forms, and in slices of 32."""
    g = np.random.default_rng(7700 + K)
    cen = g.standard_normal((K, dim)).astype(np.float32)
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    x = cen[g.integers(0, K, 203)] + (0.3 / np.sqrt(dim)) * g.standard_normal((203, dim)).astype(np.float32)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    x[100] = -x[100]                          # for K = 1 and 2: every score negative
    cut = E.ascending_cutoffs(nbits)
    rc, rp = O.encode_tokens(x, cen, nbits, cut)
    case = E.Case(f"rounded-K{K}-d{dim}b{nbits}", cen, cut, nbits, x, rc, rp)
    take = np.arange(203)
    hd, h1 = hip_index(E.codec_arrays(cen, nbits)), hip_index(E.codec_arrays(cen, nbits), max_batch=1)
    try:
        for cpw in (1, 2):
            hd.tune("gemm_cpw", cpw)
            codes, packed = hd.encode_tokens(x, cut)
            _compare(f"gemm_cpw={cpw} against the oracle", case, take, codes, packed, rc, rp)
        codes, packed = h1.encode_tokens(x, cut)
        _compare("in slices of 32 against the oracle", case, take, codes, packed, rc, rp)
    finally:
        hd.tune("gemm_cpw", 1)
        hd.close()
        h1.close()
