"""np_hip_maxsim_batch_long without a GPU: the symbols are exported, every refusal answers before any device lookup through the
C entry, 257 tokens are no shape error, the Python mirror (maxsim/maxsim_long.py) converts nothing, and maxsim_long_plan's
passes (np_maxsim_plan.h, compiled here with g++) cover the query evenly within SPmax."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT
from test_maxsim_f16_cpu import REFUSALS

from maxsim import maxsim_long as ML
from next_plaid_amd import api

PLAN_CPP = """#include "np_maxsim_plan.h"
#include <stdio.h>
int main() {
  const int nqts[] = {1, 8, 9, 17, 33, 257};
  for (int mode = 0; mode < 3; ++mode)
    for (int nqt : nqts) {
      const int32_t qoff[2] = {0, nqt * 32 - 5};
      const np::MaxsimLongPlan p = np::maxsim_long_plan(mode, false, qoff, 1, 7, nullptr, 256);
      printf("%d %d %d %d %d %d", mode, nqt, p.nqt, p.passes, p.SP, p.NQT);
      for (int ps = 0; ps <= p.passes; ++ps) printf(" %d", np::maxsim_long_first(p.nqt, p.passes, ps));
      printf("\\n");
    }
}
"""


def call(qoff, dim=8, doff=(0, 5, 7, 9), ids=(2, 0)):
    """A listed call of 1 query against 2 of 3 documents through the host entry: (status, message, outputs untouched)."""
    qoff, doff, ids = np.asarray(qoff, np.int32), np.asarray(doff, np.int64), np.asarray(ids, np.int64)
    poff, rows = np.asarray([0, ids.size], np.int64), np.ones((300, 1100), np.float32)
    sc, sims, pos = np.full(8, 7.0, np.float32), np.full(2048, 7.0, np.float32), np.full(2048, 7, np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = ML.lib().np_hip_maxsim_batch_long(0, 0, 0, dim, p(rows), p(qoff), 1, p(rows), p(doff), 3, p(ids), p(poff), p(sc), p(sims), p(pos))
    return rc, api.lib().np_hip_last_error().decode(), bool((sc == 7).all() and (sims == 7).all() and (pos == 7).all())


def test_exports():
    assert api.NP_ABI_VERSION == 6 and int(api.lib().np_hip_abi_version()) == 6
    for name in ("np_hip_maxsim_batch_long", "np_hip_maxsim_batch_long_device"):
        assert name in api.EXPORTS and hasattr(ML.lib(), name)


@pytest.mark.parametrize("name,over,status,word", [r for r in REFUSALS if r[0] != "query257"], ids=[r[0] for r in REFUSALS if r[0] != "query257"])
def test_refused_by_the_c_entry(name, over, status, word):
    rc, msg, untouched = call([0, 4], **over)
    assert rc == status and word in msg and "maxsim_batch_long" in msg and untouched, (rc, msg)


def test_257_tokens_are_no_shape_error(gpu_available):
    rc, msg, untouched = call([0, 257])
    assert rc == (0 if gpu_available else 6) and untouched != gpu_available, (rc, msg)


def test_the_mirror_converts_nothing():
    f, h = np.ones((4, 8), np.float32), np.ones((4, 8), np.uint16)
    for q, d in (([f], [h]), ([h], [f]), ([f], [f.astype(np.float64)])):
        with pytest.raises(ValueError, match="float32"):
            ML.maxsim_scores_long(q, d)
    assert ML.maxsim_scores_long([f], [f], pairs=[[]])[0].size == 0     # no pairs: NP_OK


def test_passes_are_even_and_within_spmax(tmp_path):
    (tmp_path / "plan.cpp").write_text(PLAN_CPP)
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "maxsim"), "-o", str(tmp_path / "plan"), str(tmp_path / "plan.cpp")], check=True)
    lines = subprocess.run([str(tmp_path / "plan")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == 18
    for mode, want, nqt, passes, sp, inst, *first in (list(map(int, x.split())) for x in lines):
        sizes = np.diff(first)
        assert nqt == want and sp * passes >= nqt and first[0] == 0 and first[-1] == nqt and len(sizes) == passes
        assert sizes.max() == sp and sizes.max() - sizes.min() <= 1 and sp <= inst <= (4 if mode == 0 else 8), (mode, nqt, sizes)
    assert lines[10].split()[3:] == "5 7 8 0 7 14 21 27 33".split()      # bf16, 33 tiles: 7, 7, 7, 6, 6
