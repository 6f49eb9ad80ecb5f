"""The decompress cases of tests/decompress_limit_shapes.py on the CPU: the oracle's f32 rows meet, against float64
(exact_restate.decompress64), the bound derived for ITS summation order by the rules that give the kernel's bound, the
zero rows are exactly 0, and the tiny rows are the clamp's quotient bit for bit."""
import numpy as np
import pytest

import decompress_limit_shapes as D
import exact_restate as X
from helpers import oracle_index


@pytest.mark.parametrize("geo", D.GEOMETRIES, ids=lambda g: f"d{g[0]}b{g[1]}")
def test_oracle_rows_within_the_derived_bound(geo):
    dim, nbits = geo
    a, kinds = D.make_index(dim, nbits)
    ox = oracle_index(a)
    ref64 = X.decompress64(dict(a))
    rows = np.concatenate([ox.get_document_embeddings(d) for d in range(D.LENGTHS.size) if D.LENGTHS[d]])
    assert rows.shape == ref64.shape == (kinds.size, dim) and rows.dtype == np.float32
    D.check(f"oracle d{dim}b{nbits}", rows, ref64, rows, kinds, D.e_cpu(dim))
    # what the rows are by construction
    x = a["centroids"][a["codes"]].astype(np.float64) + a["bucket_weights"][X.unpack(a["residuals"], nbits, dim)]
    n = np.sqrt((x * x).sum(1))
    assert np.all(n[kinds == "zero"] == 0) and np.all(n[kinds == "tiny"] < 1e-15) and np.all(n[kinds == "tiny"] > 0)
    assert np.all(n[kinds == "huge"] > 1e17) and np.all((x[kinds == "huge"] ** 2).sum(1) < 3e38)
    tiny = x[kinds == "tiny"].astype(np.float32)
    assert np.all(tiny.astype(np.float64) ** 2 < 1.2e-38)                       # every square is below the f32 normal range
    assert np.array_equal(rows[kinds == "tiny"], tiny / np.float32(1e-12))      # the clamp's quotient, bit for bit
    assert np.all(np.abs(np.linalg.norm(rows[kinds == "generic"].astype(np.float64), axis=1) - 1) < 1e-6)


def test_request_shape():
    toks, lens = D.requested_tokens()
    assert lens.tolist() == [3, 0, 1, 3, 70, 2, 0, 0, 0] and toks.size == D.LENGTHS.sum()
