"""np_hip_maxsim_batch_i8 and np_hip_quantize_rows_i8 without a GPU: the symbols are exported under ABI 6, and every refusal
answers before any device lookup, through the C entries and through the Python mirror."""
import numpy as np
import pytest

import maxsim_i8_restate as R

import next_plaid_amd as npa
from next_plaid_amd import api


def test_abi_and_exports():
    assert api.NP_ABI_VERSION == 6 and int(api.lib().np_hip_abi_version()) == 6
    assert (api.NP_DT_I8, api.MAXSIM_CHUNK_I8) == (2, 128)
    for name in ("np_hip_maxsim_batch_i8", "np_hip_maxsim_batch_i8_device", "np_hip_quantize_rows_i8", "np_hip_quantize_rows_i8_device"):
        assert name in api.EXPORTS and hasattr(api.lib(), name)
    import maxsim_restate as M
    rc, msg, untouched = M.refused_call(api.lib(), dict(dtype=2))        # the existing entries keep refusing dtype 2
    assert rc == 8 and "dtype must be NP_DT_F32 (0) or NP_DT_BF16 (1)" in msg and untouched


@pytest.mark.parametrize("name,entry,over,status,word", R.REFUSALS, ids=[r[0] for r in R.REFUSALS])
def test_refused_by_the_c_entry(name, entry, over, status, word):
    rc, msg, untouched = R.refused_call(api.lib(), entry, over)
    assert rc == status and word in msg and untouched, (rc, msg)


def test_refused_by_the_python_mirror():
    c = lambda n, dim=8: np.ones((n, dim), np.int8)   # noqa: E731
    q, d, qs, ds = [c(4)], [c(5), c(2)], [np.ones(4, np.float32)], [np.ones(5, np.float32), np.ones(2, np.float32)]
    for kw in (dict(query_scales=qs), dict(document_scales=ds), dict(query_scales=qs, document_scales=ds, precision=3)):
        with pytest.raises(ValueError, match="go together"):
            npa.maxsim_scores(q, d, **kw)
    with pytest.raises(ValueError, match="int8 query rows"):
        npa.maxsim_scores([np.ones((4, 8), np.float32)], d, query_scales=qs, document_scales=ds)
    with pytest.raises(ValueError, match="one scale per row"):
        npa.maxsim_scores(q, d, query_scales=qs, document_scales=ds[:1])
    with pytest.raises(npa.ShapeError, match="dim"):
        npa.maxsim_scores([c(4, 1025)], [c(5, 1025), c(2, 1025)], query_scales=qs, document_scales=ds)
    with pytest.raises(npa.ShapeError, match="q_tok_offsets"):
        npa.maxsim_scores([c(257)], d, query_scales=[np.ones(257, np.float32)], document_scales=ds)
    with pytest.raises(ValueError, match="pair_docs"):
        npa.maxsim_scores(q, d, pairs=[[0, 2]], query_scales=qs, document_scales=ds)
    with pytest.raises(npa.ShapeError, match="dim"):
        npa.quantize_rows(np.ones((3, 1025), np.float32))
    assert npa.maxsim_scores(q, d, pairs=[[]], query_scales=qs, document_scales=ds)[0].size == 0     # no pairs: NP_OK
    assert npa.quantize_rows(np.zeros((0, 8), np.float32))[0].shape == (0, 8)
