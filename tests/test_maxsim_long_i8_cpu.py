"""np_hip_maxsim_batch_long_i8 without a GPU: the symbols are exported, every refusal answers before any device lookup through
the C entry, 257 tokens are no shape error, the Python mirror (maxsim/maxsim_long.py) converts nothing and counts the scales,
and maxsim_long_i8_plan's passes (np_maxsim_plan.h, compiled here with g++) cover the query evenly within SPmax(dim) and the
LDS budget."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT
from maxsim_i8_restate import REFUSALS

from maxsim import maxsim_long as ML
from next_plaid_amd import api

I8_REFUSALS = [r for r in REFUSALS if r[1] == "s" and r[0] != "query257"]
DIMS, TILES = (1, 128, 129, 512, 1024), (1, 8, 9, 33, 257)

PLAN_CPP = """#include "np_maxsim_plan.h"
#include <initializer_list>
#include <stdio.h>
int main() {
  for (int dim : {%s})
    for (int nqt : {%s}) {
      const int32_t qoff[2] = {0, nqt * 32 - 5};
      const np::MaxsimLongPlan p = np::maxsim_long_i8_plan(dim, false, qoff, 1, 7, nullptr, 256);
      printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d", dim, nqt, p.nqt, p.passes, p.SP, p.NQT, np::maxsim_long_i8_spmax(dim),
             (int)np::maxsim_long_i8_lds(dim, p.NQT), np::NP_MS_LONG_I8_BUDGET);
      for (int ps = 0; ps <= p.passes; ++ps) printf(" %%d", np::maxsim_long_first(p.nqt, p.passes, ps));
      printf("\\n");
    }
}
""" % (", ".join(map(str, DIMS)), ", ".join(map(str, TILES)))


def call(qoff, dim=8, doff=(0, 5, 7, 9), ids=(2, 0), qs=np.ones(300, np.float32), ds=np.ones(300, np.float32)):
    """maxsim_i8_restate.refused_call's small listed call through the long host entry: (status, message, outputs untouched)."""
    keep = [np.asarray(qoff, np.int32), np.asarray(doff, np.int64), np.asarray(ids, np.int64), np.asarray([0, len(ids)], np.int64)]
    codes = np.full((300, 1100), 7, np.int8)
    sc, sims, pos = np.full(300, 7.0, np.float32), np.full(2048, 7.0, np.float32), np.full(2048, 7, np.int32)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = ML.lib().np_hip_maxsim_batch_long_i8(0, dim, p(codes), p(qs), p(keep[0]), 1, p(codes), p(ds), p(keep[1]), 3, p(keep[2]), p(keep[3]),
                                              p(sc), p(sims), p(pos))
    return rc, api.lib().np_hip_last_error().decode(), bool((sc == 7).all() and (sims == 7).all() and (pos == 7).all())


def test_exports():
    assert api.NP_ABI_VERSION == 6 and int(api.lib().np_hip_abi_version()) == 6
    for name in ("np_hip_maxsim_batch_long_i8", "np_hip_maxsim_batch_long_i8_device"):
        assert name in api.EXPORTS and hasattr(ML.lib(), name)


@pytest.mark.parametrize("name,entry,over,status,word", I8_REFUSALS, ids=[r[0] for r in I8_REFUSALS])
def test_refused_by_the_c_entry(name, entry, over, status, word):
    rc, msg, untouched = call([0, 4], **over)
    assert rc == status and word in msg and "maxsim_batch_long_i8" in msg and untouched, (rc, msg)


def test_257_tokens_are_no_shape_error(gpu_available):
    rc, msg, untouched = call([0, 257])
    assert rc == (0 if gpu_available else 6) and untouched != gpu_available, (rc, msg)


def test_the_mirror_converts_nothing_and_counts_the_scales():
    c, f, s = np.ones((4, 8), np.int8), np.ones((4, 8), np.float32), np.ones(4, np.float32)
    for q, d in (([c], [f]), ([f], [c]), ([c.view(np.uint8)], [c.view(np.uint8)])):
        with pytest.raises(ValueError, match="int8"):
            ML.maxsim_scores_long_i8(q, d, [s], [s])
    for qs, ds in ((None, [s]), ([s], None), ([s[:3]], [s]), ([s], [np.ones(5, np.float32)]), ([s.astype(np.float64)], [s])):
        with pytest.raises(ValueError, match="scales"):
            ML.maxsim_scores_long_i8([c], [c], qs, ds)
    assert ML.maxsim_scores_long_i8([c], [c], [s], [s], pairs=[[]])[0].size == 0     # no pairs: NP_OK


def test_passes_are_even_within_spmax_and_the_budget(tmp_path):
    (tmp_path / "plan.cpp").write_text(PLAN_CPP)
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "maxsim"), "-o", str(tmp_path / "plan"), str(tmp_path / "plan.cpp")], check=True)
    lines = subprocess.run([str(tmp_path / "plan")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(DIMS) * len(TILES)
    for dim, want, nqt, passes, sp, inst, spmax, lds, budget, *first in (list(map(int, x.split())) for x in lines):
        sizes = np.diff(first)
        assert nqt == want and first[0] == 0 and first[-1] == nqt and len(sizes) == passes, (dim, nqt, first)
        assert sizes.max() == sp and sizes.max() - sizes.min() <= 1 and sp <= inst <= spmax and lds <= budget == 80 * 1024, (dim, nqt, sizes)
        assert spmax == {1: 8, 128: 8, 129: 8, 512: 4, 1024: 2}[dim]
