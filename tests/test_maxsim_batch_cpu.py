"""np_hip_maxsim_batch without a GPU: every refusal answers before any device lookup, through the C entry and the Python
mirror; the ABI version is unchanged and the new symbols are exported."""
import numpy as np
import pytest

import maxsim_restate as M

import next_plaid_amd as npa
from next_plaid_amd import api


def test_abi_and_exports():
    assert api.NP_ABI_VERSION == 6 and int(api.lib().np_hip_abi_version()) == 6
    for name in ("np_hip_maxsim_batch", "np_hip_maxsim_batch_device"):
        assert name in api.EXPORTS and hasattr(api.lib(), name)


@pytest.mark.parametrize("name,over,status,word", M.REFUSALS, ids=[r[0] for r in M.REFUSALS])
def test_refused_by_the_c_entry(name, over, status, word):
    rc, msg, untouched = M.refused_call(api.lib(), over)
    assert rc == status and word in msg and untouched, (rc, msg)


def test_refused_by_the_python_mirror():
    g = np.random.default_rng(0)
    q, d = [M.unit_rows(g, 4, 8)], [M.unit_rows(g, 5, 8), M.unit_rows(g, 2, 8)]
    with pytest.raises(npa.ShapeError, match="dim"):
        npa.maxsim_scores([np.zeros((2, 1025), np.float32)], [np.zeros((2, 1025), np.float32)])
    with pytest.raises(npa.ShapeError, match="q_tok_offsets"):
        npa.maxsim_scores([M.unit_rows(g, 257, 8)], d)
    with pytest.raises(ValueError, match="precision"):
        npa.maxsim_scores(q, d, precision=1)
    with pytest.raises(ValueError, match="out_match"):
        npa.maxsim_scores(q, d, precision=3, return_matches=True)
    with pytest.raises(ValueError, match="doc_tok_offsets"):
        npa.maxsim_scores(q, np.concatenate(d), document_offsets=[0, 5, 3, 7])
    with pytest.raises(ValueError, match="pair_docs"):
        npa.maxsim_scores(q, d, pairs=[[0, 2]])
    assert npa.maxsim_scores([], d) == [] and npa.maxsim_scores(q, d, pairs=[[]])[0].size == 0     # no pairs: NP_OK
