"""search_exact_grouped's host code without a device: the Python binding against test_binding_calls_cpu.py's recording fake
and next_plaid.hpp against recording stubs (tests/cpp/search_exact_grouped.cpp with -DNP_STUBS, stand-alone under ASan and
UBSan): the entry reached, the argument values, the result slicing.  The plan of slices and passes is np_scan_plan.h's, which
tests/cpp/scan_plan_check.cpp runs stand-alone."""
import os
import subprocess

import pytest

import test_binding_calls_cpu as BC
from test_binding_calls_cpu import fake, ix  # noqa: F401  (fixtures)

BC.SPECS["np_hip_search_exact_grouped"] = f"{BC.HEAD} top_k group_size precision {BC.CSR} {BC.GROUPS} st"
BC.SPECS["np_hip_search_exact_grouped_filtered"] = f"{BC.HEAD} top_k group_size precision {BC.FILT} qsub {BC.GROUPS} st"


@pytest.mark.parametrize("group_size", [1, 2])
@pytest.mark.parametrize("form", BC.FORMS)
@pytest.mark.parametrize("B,top_k", BC.B_K)
def test_search_exact_grouped(ix, fake, form, B, top_k, group_size):
    qs, flat, off = BC.queries_of(B)
    kw, sid, soff, n_sub, qmap, filt = BC.scope_of(form, B)
    res = ix.search_exact_grouped(qs, top_k, group_size, 3, **kw)
    (r,) = fake.calls
    assert r["entry"] == ("np_hip_search_exact_grouped_filtered" if form == "filters" else "np_hip_search_exact_grouped")
    BC.check_queries(r, B, flat, off)
    assert (r["top_k"], r["group_size"], r["precision"]) == (top_k, group_size, 3)
    if form == "filters":
        assert r["n_f"] == n_sub and r["filt"] == filt and BC.same(r["qsub"], qmap)
    else:
        BC.check_csr(r, sid, soff, n_sub, qmap)
    BC.check_groups(res, BC.expected_groups(B, top_k, group_size))
    raw = ix.search_exact_grouped(qs, top_k, group_size, raw=True, **kw)
    k = max(top_k, 1)
    assert fake.calls[-1]["precision"] == 0 and [x.size for x in raw] == [max(B * k * group_size, 1)] * 2 + [max(B * k, 1)] * 3 + [max(B, 1)]
    assert raw[5][:B].tolist() == BC.counts_for(B, top_k)


def test_cpp_mirror_against_recording_stubs(tmp_path):
    exe = tmp_path / "stubs"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-DNP_STUBS", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(BC.ROOT, "tests", "cpp", "search_exact_grouped.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
