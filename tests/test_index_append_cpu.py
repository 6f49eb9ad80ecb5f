"""The resident append's surface without a device: the three C entries and their prototypes, the ABI version they leave alone,
the argument checks that run before any device work, what MmapIndex.append reads back from the directory an update_append
wrote (the restated update_index stands in for it here), and the C++ mirror against recording stubs
(tests/cpp/index_append_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import update_restate as U
from helpers import make_arrays, synth
from oracle import npy_index

from next_plaid_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_and_prototypes():
    L = api.lib()
    vp, i64 = C.c_void_p, C.c_int64
    assert {"np_hip_index_append", "np_hip_index_reserve", "np_hip_index_capacity"} <= set(api.EXPORTS)
    assert L.np_hip_index_append.argtypes == [vp, vp, i64, vp, vp]
    assert L.np_hip_index_reserve.argtypes == [vp, i64, i64]
    assert L.np_hip_index_capacity.argtypes == [vp, C.POINTER(i64), C.POINTER(i64)]
    assert L.np_hip_abi_version() == 6 == api.NP_ABI_VERSION   # new functions only: no struct changed


def test_null_handle_is_refused_by_name():
    L = api.lib()
    d, t = C.c_int64(-5), C.c_int64(-5)
    for call, entry in ((lambda: L.np_hip_index_append(None, None, 0, None, None), "np_hip_index_append"),
                        (lambda: L.np_hip_index_reserve(None, 1, 1), "np_hip_index_reserve"),
                        (lambda: L.np_hip_index_capacity(None, C.byref(d), C.byref(t)), "np_hip_index_capacity")):
        assert call() == 8 and api.last_error() == f"{entry}: index is NULL"
    assert (d.value, t.value) == (-5, -5)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def test_append_needs_a_directory(monkeypatch):
    """a handle made from arrays has no directory to update: refused before any library call"""
    hx = api.MmapIndex.__new__(api.MmapIndex)
    hx._h, hx.path, hx._open_opts = None, "<arrays>", {}
    monkeypatch.setattr(api, "_lib", _NoLibrary())
    with pytest.raises(api.IndexLoadError, match=r"append\(\) needs an index opened from a directory"):
        hx.append([np.zeros((2, 8), np.float32)])
    hx.path = ""
    with pytest.raises(api.IndexLoadError, match=r"append\(\) needs an index opened from a directory"):
        hx.append([])


@pytest.mark.parametrize("n_old,chunk_docs,batch,n_new", [(1200, 500, 50_000, 30), (2600, 2600, 7, 30), (40, 500, 50_000, 1)])
def test_append_reads_back_what_the_update_wrote(tmp_path, n_old, chunk_docs, batch, n_new):
    """the new documents join a short last chunk, or fill chunks of batch_size documents behind a full one: either way the tail
    of the directory's tokens is what the handle gets -- the same codes and residuals, not a second encoding"""
    spec, a = make_arrays(num_docs=n_old, num_centroids=64, dim=32, nbits=4, doc_len_min=0, doc_len_max=9, seed=4)
    cut, wts = synth.bucket_tables(spec)
    d = str(tmp_path / "ix")
    api.write_index_dir(d, a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=chunk_docs)
    rng = np.random.default_rng(n_old)
    docs = [(a["centroids"][rng.integers(0, 64, L)] + 0.02 * rng.standard_normal((L, 32))).astype(np.float32)
            for L in rng.integers(0, 12, n_new)]
    before = api._dir_counts(d)
    assert before == (n_old, int(a["doc_lengths"].sum()))
    U.update_index(d, docs, batch, False)
    lens, codes, res = api._appended_tokens(d, before)
    r = npy_index.read_index(d)
    t_new = sum(x.shape[0] for x in docs)
    assert lens.tolist() == [x.shape[0] for x in docs] == r["doc_lengths"][n_old:].tolist()
    assert codes.dtype == np.int64 and res.dtype == np.uint8 and res.shape == (t_new, 16)
    assert np.array_equal(codes, r["codes"][len(r["codes"]) - t_new:]) and np.array_equal(res, r["residuals"][len(r["codes"]) - t_new:])
    # a directory whose files hold less than metadata.json counts is refused, not padded
    with pytest.raises(api.IndexLoadError, match="metadata.json counts"):
        api._appended_tokens(d, (before[0], before[1] - 1))


def test_cpp_mirror_hands_over_what_the_update_wrote(tmp_path):
    """tests/cpp/index_append_check.cpp: next_plaid.hpp against recording stubs, with the host compiler alone, under ASan +
    UBSan: append passes exactly the arrays update_append wrote; append_arrays, reserve and capacity pass through"""
    exe, work = tmp_path / "index_append_check", tmp_path / "dir"
    work.mkdir()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "index_append_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(work)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
