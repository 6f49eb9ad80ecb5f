"""np_hip_maxsim_batch_f16 without a GPU: the symbols are exported, every refusal answers before any device lookup through the
C entry, the Python mirror (maxsim/maxsim_f16.py) converts nothing, and np_hip_maxsim_batch keeps refusing the dtype."""
import ctypes as C

import numpy as np
import pytest

import maxsim_restate as M

from maxsim import maxsim_f16 as F16
from next_plaid_amd import api

# (name, overrides of a valid listed call: 1 query of 4 tokens, 3 documents, 2 pairs, dim 8; status; a word of the message)
REFUSALS = [("dim0", dict(dim=0), 3, "dim"), ("dim1025", dict(dim=1025), 3, "dim"), ("query257", dict(qoff=[0, 257]), 3, "q_tok_offsets"),
            ("doc_offsets_decrease", dict(doff=[0, 5, 3, 9]), 8, "doc_tok_offsets"), ("pair_id_n_docs", dict(ids=[0, 3]), 8, "pair_docs")]


def test_exports():
    assert int(api.lib().np_hip_abi_version()) == 6
    for name in ("np_hip_maxsim_batch_f16", "np_hip_maxsim_batch_f16_device"):
        assert name in api.EXPORTS and hasattr(F16.lib(), name)


@pytest.mark.parametrize("name,over,status,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_by_the_c_entry(name, over, status, word):
    a = dict(dim=8, qoff=[0, 4], doff=[0, 5, 7, 9], ids=[2, 0])
    a.update(over)
    qoff, doff, ids = np.asarray(a["qoff"], np.int32), np.asarray(a["doff"], np.int64), np.asarray(a["ids"], np.int64)
    poff, rows = np.asarray([0, ids.size], np.int64), np.ones((300, 1100), np.float16)
    sc, sims, pos = np.full(8, 7.0, np.float32), np.full(2048, 7.0, np.float32), np.full(2048, 7, np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = F16.lib().np_hip_maxsim_batch_f16(0, a["dim"], p(rows), p(qoff), 1, p(rows), p(doff), 3, p(ids), p(poff), p(sc), p(sims), p(pos))
    msg = api.lib().np_hip_last_error().decode()
    assert rc == status and word in msg and "maxsim_batch_f16" in msg, (rc, msg)
    assert (sc == 7).all() and (sims == 7).all() and (pos == 7).all()


def test_the_mirror_converts_nothing():
    h, f = np.ones((4, 8), np.float16), np.ones((4, 8), np.float32)
    for q, d in (([f], [h]), ([h], [f]), ([h], [h.astype(np.float64)])):
        with pytest.raises(ValueError, match="float16"):
            F16.maxsim_scores_f16(q, d)
    assert F16.maxsim_scores_f16([h], [h], pairs=[[]])[0].size == 0     # no pairs: NP_OK


def test_the_plain_entry_still_refuses_the_dtype():
    rc, msg, untouched = M.refused_call(api.lib(), dict(dtype=5))
    assert rc == 8 and "dtype must be NP_DT_F32 (0) or NP_DT_BF16 (1)" in msg and untouched
