"""np_hip_maxsim_batch_i4 and np_hip_quantize_rows_i4 without a GPU: the symbols are exported, and every refusal answers
before any device lookup, through the C entries and through the Python mirror (maxsim/maxsim_i4.py)."""
import numpy as np
import pytest

import maxsim_i4_restate as R

import next_plaid_amd as npa
from maxsim import maxsim_i4 as I4
from next_plaid_amd import api


def test_exports():
    assert int(api.lib().np_hip_abi_version()) == 6
    for name in ("np_hip_maxsim_batch_i4", "np_hip_maxsim_batch_i4_device", "np_hip_quantize_rows_i4", "np_hip_quantize_rows_i4_device"):
        assert name in api.EXPORTS and hasattr(I4.lib(), name)


@pytest.mark.parametrize("name,entry,over,status,word", R.REFUSALS, ids=[r[0] for r in R.REFUSALS])
def test_refused_by_the_c_entry(name, entry, over, status, word):
    rc, msg, untouched = R.refused_call(I4.lib(), entry, over)
    assert rc == status and word in msg and untouched, (rc, msg)


def test_refused_by_the_python_mirror():
    q, qs = [np.ones((4, 40), np.int8)], [np.ones(4, np.float32)]
    d, ds = [np.ones((5, 5), np.uint32), np.ones((2, 5), np.uint32)], [np.ones(5, np.float32), np.ones(2, np.float32)]
    with pytest.raises(npa.ShapeError, match="ceil"):
        I4.maxsim_scores_i4(q, qs, [np.ones((5, 6), np.uint32)], ds[:1])
    with pytest.raises(ValueError, match="maxsim_scores_i4: document_scales holds one scale per document row"):
        I4.maxsim_scores_i4(q, qs, d, ds[:1])
    with pytest.raises(ValueError, match="pair_docs"):
        I4.maxsim_scores_i4(q, qs, d, ds, pairs=[[0, 2]])
    with pytest.raises(npa.ShapeError, match="q_tok_offsets"):
        I4.maxsim_scores_i4([np.ones((257, 40), np.int8)], [np.ones(257, np.float32)], d, ds)
    with pytest.raises(npa.ShapeError, match="dim"):
        I4.quantize_rows_i4(np.ones((3, 1025), np.float32))
    assert I4.maxsim_scores_i4(q, qs, d, ds, pairs=[[]])[0].size == 0     # no pairs: NP_OK
    assert I4.quantize_rows_i4(np.zeros((0, 40), np.float32))[0].shape == (0, 5)


def test_restatement_round_trip():
    """Known words for a short row with the codes -7 and 7, pad nibbles 0, and garbage pad nibbles do not reach unpack."""
    x = np.array([[3.5, -3.5, 0.5, -0.5, 1.0, 2.5, -0.0, 1.25, -3.0, 1.5]], np.float32)   # a = 3.5: inv = 2, scale = 0.5; 1.25 * 2 is a tie, to even
    words, scale = R.quantize4(x)
    want = np.array([[7, -7, 1, -1, 2, 5, 0, 2, -6, 3]], np.int8)
    assert words.shape == (1, 2) and words[0, 0] == 0x2052F197 and words[0, 1] == 0x3A and scale[0] == 0.5
    assert np.array_equal(R.unpack(words, 10), want) and np.array_equal(R.unpack(words | np.array([0, 0xFFFFFF00], np.uint32), 10), want)
    assert np.array_equal(R.unpack(np.array([[0x89ABCDEF]], np.uint32), 8), [[-1, -2, -3, -4, -5, -6, -7, -8]])
