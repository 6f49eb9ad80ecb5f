"""Index creation without a device: the plan formulas of kmeans.rs:261-311 / index.rs:199-226, the seeded document
sample against a Python restatement of the SplitMix64 stream, the quantile rule of utils.rs:94-149, the new structs'
layout, and the refusals (no documents; no GPU = DeviceUnavailableError, never a CPU fallback)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import kmeans_restate as R
from helpers import ROOT

import next_plaid_amd as npa
from next_plaid_amd import api


def _k(sample_tokens, ns, N):
    return 2 ** math.floor(math.log2(16.0 * math.sqrt(sample_tokens / ns * N)))


@pytest.mark.parametrize("lens", [[7], [0, 3, 9, 1, 4], list(range(1, 50)), [300] * 2000, [5, 0, 120, 33] * 700])
def test_plan_formulas(lens):
    lens = np.asarray(lens, np.int64)
    N = lens.size
    p, ids = npa.kmeans_plan(lens)
    ns = min(int(min(1.0 + 16.0 * math.sqrt(120.0 * N), N)), N)
    assert p["n_samples"] == ns == ids.size
    assert ids.tolist() == R.shuffled_docs(N, 42)[:ns]
    st = int(lens[ids].sum())
    assert p["sample_tokens"] == st
    assert p["num_partitions"] == _k(st, ns, N) and p["k"] == min(_k(st, ns, N), st)
    assert p["codec_samples"] == max(1, min(N, int(16.0 * math.sqrt(120.0 * N))))
    assert p["heldout_size"] == int(min(0.05 * lens.sum(), 50000.0))


def test_plan_bench_corpus_and_overrides():
    p, _ = npa.kmeans_plan(np.full(10_000_000, 300, np.int64))
    assert p["n_samples"] == 554257 and p["k"] == 2 ** 19
    p, ids = npa.kmeans_plan([4, 4, 4, 4], npa.IndexConfig(n_samples_kmeans=2), num_partitions=3)
    assert p["n_samples"] == 2 and p["num_partitions"] == 3 and p["k"] == 3 and ids.size == 2
    docs = [np.zeros((n, 8), np.float32) for n in (3, 5, 0, 9)]
    assert npa.estimate_num_partitions(docs) == npa.kmeans_plan([3, 5, 0, 9])[0]["k"]


@pytest.mark.parametrize("seed", [0, 42, 2 ** 63])
def test_sample_ids_follow_the_stream(seed):
    lens = np.arange(1, 5001, dtype=np.int64) % 17
    p, ids = npa.kmeans_plan(lens, npa.IndexConfig(seed=seed))
    assert ids.tolist() == R.shuffled_docs(lens.size, seed)[: p["n_samples"]]


def test_splitmix_known_values():
    # SplitMix64 reference outputs for seed 1234567 (the published test vector of the generator)
    g = R.SplitMix64(1234567)
    assert [g.next() for _ in range(3)] == [6457827717110365317, 3203168211198807973, 9817491932198370423]


def test_quantile_rule():
    a = np.array([1, 2, 3, 4, 5], np.float32)    # utils.rs:289-293
    assert R.quantile(a, 0.5) == 3 and R.quantile(a, 0.0) == 1 and R.quantile(a, 1.0) == 5
    b = np.array([0.0, 1.0], np.float32)
    assert R.quantile(b, 0.25) == np.float32(0.25)
    assert R.quantile(np.zeros(0, np.float32), 0.3) == 0


def test_new_struct_layouts(tmp_path):
    names = ["np_kmeans_opts", "np_kmeans_report", "np_index_config", "np_kmeans_plan"]
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "nextplaid_hip.h"', "int main(void) {"]
    for n in names:
        src.append(f'  printf("{n} %zu\\n", sizeof({n}));')
        for f, _ in getattr(api, n)._fields_:
            src.append(f'  printf("{n}.{f} %zu\\n", offsetof({n}, {f}));')
    src += ["  return 0;", "}"]
    c = tmp_path / "sz.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    L = api.lib()
    for i, n in enumerate(names):
        st = getattr(api, n)
        assert C.sizeof(st) == int(got[n]) == int(L.np_hip_struct_size(4 + i)), n
        for f, _ in st._fields_:
            assert getattr(st, f).offset == int(got[f"{n}.{f}"]), f"{n}.{f}"


def test_index_config_json():
    c = npa.IndexConfig.from_json('{"nbits": 2, "seed": 7, "force_cpu": true}')
    assert c.nbits == 2 and c.seed == 7 and c.batch_size == 50_000 and c.kmeans_niters == 4
    assert npa.IndexConfig.from_json(c.to_json()) == c
    with pytest.raises(ValueError):
        npa.IndexConfig.from_json('{"seed": 1}')


def test_empty_input_is_index_creation_error(tmp_path):
    with pytest.raises(npa.IndexCreationError, match="No documents"):
        npa.compute_kmeans([])
    with pytest.raises(npa.IndexCreationError, match="No documents"):
        npa.MmapIndex.create_with_kmeans([], str(tmp_path / "x"))
    with pytest.raises(npa.IndexCreationError, match="No documents"):
        npa.kmeans_plan([])


def test_no_gpu_no_fallback(tmp_path, gpu_available):
    if gpu_available:
        pytest.skip("a GPU is present: the device path is covered by the gpu tests")
    docs = [np.ones((4, 16), np.float32)] * 3
    with pytest.raises(npa.DeviceUnavailableError):
        npa.compute_kmeans(docs)
    with pytest.raises(npa.DeviceUnavailableError):
        npa.MmapIndex.create_with_kmeans(docs, str(tmp_path / "x"))
    with pytest.raises(npa.DeviceUnavailableError):
        npa.kmeans(np.ones((10, 4), np.float32), 2)
    assert not os.path.exists(tmp_path / "x")
