"""decompress_kernel against float64 inside a bound derived from its operation count, at rows whose norm is 0, tiny
and huge, at nbits 1, 2, 4, 8 and dims 8, 96, 100, 128 (tests/decompress_limit_shapes.py holds the cases and the
derivation; tests/test_decompress_limits_cpu.py holds the oracle to the analogous bound).

The kernel sums the squares in a shuffle tree, so it cannot equal the reference's summation order bit for bit.  Each
component is held to exact_restate.decompress64 within E_GPU 2^-24 relative, E_GPU = (ceil(dim / 64) + 9) / 2 + 8 (13 for
dim <= 64, 13.5 up to 128): one rounding of c + w, the squares with their products and additions counted as not
contracted, six shuffle additions, the square root halving all that, sqrtf at 1 ulp and the divide at 2.5 ulp.  The
zero rows must be exactly +0.  The tiny rows (components of 1e-20: their squares underflow in f32 and not in float64) are
compared with the CPU oracle's f32 rows under the same bound.
"""
import numpy as np
import pytest

import decompress_limit_shapes as D
import exact_restate as X
from helpers import hip_index, oracle_index

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("geo", D.GEOMETRIES, ids=lambda g: f"d{g[0]}b{g[1]}")
def test_rows_within_the_derived_bound(geo, monkeypatch):
    dim, nbits = geo
    a, kinds = D.make_index(dim, nbits)
    ref64 = X.decompress64(dict(a))
    ox = oracle_index(a)
    ref32 = np.concatenate([ox.get_document_embeddings(d) for d in range(D.LENGTHS.size) if D.LENGTHS[d]])
    toks, want_lens = D.requested_tokens()
    plain = hip_index(a)
    monkeypatch.setenv("NP_TOK_SORT", "1")       # tokens stored ordered by code: rows go back through tok_pos
    srt = hip_index(a)
    monkeypatch.delenv("NP_TOK_SORT")
    try:
        assert srt.info.device_bytes > plain.info.device_bytes          # the position array: the sorted layout was taken
        got, lens = plain.decompress_documents(D.REQUEST)
        assert lens.tolist() == want_lens.tolist() and got.shape == (toks.size, dim)
        D.check(f"d{dim}b{nbits}", got, ref64[toks], ref32[toks], kinds[toks], D.e_gpu(dim))
        assert np.allclose(got, ref32[toks], rtol=0, atol=3e-7)          # the suite's older, absolute check holds as well
        g2, l2 = srt.decompress_documents(D.REQUEST)
        assert np.array_equal(l2, lens) and np.array_equal(g2.view(np.uint32), got.view(np.uint32))
        # the last document alone, an empty one alone, and ids past the end alone
        g1, l1 = plain.decompress_documents([D.LENGTHS.size - 1])
        assert l1.tolist() == [2] and np.array_equal(g1, got[-2:])
        for ids in ([1], [6, -1], []):
            g0, l0 = plain.decompress_documents(ids)
            assert g0.shape == (0, dim) and l0.tolist() == [0] * len(ids)
    finally:
        plain.close()
        srt.close()
