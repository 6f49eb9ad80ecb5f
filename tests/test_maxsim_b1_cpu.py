"""np_hip_maxsim_batch_b1 and np_hip_pack_rows_b1 without a GPU: the symbols are exported, and every refusal answers before
any device lookup, through the C entries and through the Python mirror (maxsim/maxsim_b1.py)."""
import numpy as np
import pytest

import maxsim_b1_restate as R

import next_plaid_amd as npa
from maxsim import maxsim_b1 as B1
from next_plaid_amd import api


def test_exports():
    assert int(api.lib().np_hip_abi_version()) == 6
    for name in ("np_hip_maxsim_batch_b1", "np_hip_maxsim_batch_b1_device", "np_hip_pack_rows_b1", "np_hip_pack_rows_b1_device"):
        assert name in api.EXPORTS and hasattr(B1.lib(), name)


@pytest.mark.parametrize("name,entry,over,status,word", R.REFUSALS, ids=[r[0] for r in R.REFUSALS])
def test_refused_by_the_c_entry(name, entry, over, status, word):
    rc, msg, untouched = R.refused_call(B1.lib(), entry, over)
    assert rc == status and word in msg and untouched, (rc, msg)


def test_refused_by_the_python_mirror():
    q, qs = [np.ones((4, 40), np.int8)], [np.ones(4, np.float32)]
    d, ds = [np.ones((5, 2), np.uint32), np.ones((2, 2), np.uint32)], [np.ones(5, np.float32), np.ones(2, np.float32)]
    with pytest.raises(npa.ShapeError, match="ceil"):
        B1.maxsim_scores_b1(q, qs, [np.ones((5, 3), np.uint32)], ds[:1])
    with pytest.raises(ValueError, match="one scale per document row"):
        B1.maxsim_scores_b1(q, qs, d, ds[:1])
    with pytest.raises(ValueError, match="pair_docs"):
        B1.maxsim_scores_b1(q, qs, d, ds, pairs=[[0, 2]])
    with pytest.raises(npa.ShapeError, match="q_tok_offsets"):
        B1.maxsim_scores_b1([np.ones((257, 40), np.int8)], [np.ones(257, np.float32)], d, ds)
    with pytest.raises(npa.ShapeError, match="dim"):
        B1.pack_rows_b1(np.ones((3, 1025), np.float32))
    assert B1.maxsim_scores_b1(q, qs, d, ds, pairs=[[]])[0].size == 0     # no pairs: NP_OK
    assert B1.pack_rows_b1(np.zeros((0, 40), np.float32))[0].shape == (0, 2)


def test_restatement_round_trip():
    """pack then unpack gives sign(x) with +-0.0 as +1, pad bits are 0, and garbage pad bits do not reach the codes."""
    x = np.array([[1.5, -2.0, 0.0, -0.0, 3.0] + [-1.0] * 28], np.float32)
    bits, scale = R.pack(x)
    assert bits.shape == (1, 2) and bits[0, 0] == 0b11101 and bits[0, 1] == 0 and scale[0] == np.float32(34.5) / np.float32(33)
    assert np.array_equal(R.unpack(bits | np.array([0, 0xFFFFFFFE], np.uint32), 33), np.where(x >= 0, 1, -1))
