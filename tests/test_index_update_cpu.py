"""Index update and delete without a device: MmapIndex::delete (delete.rs:43-398) against the numpy restatement, the new
structs' layout, UpdateConfig serde, and update refusing to run without a GPU while leaving the directory unchanged."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import update_restate as U
from helpers import ROOT, make_arrays
from oracle import npy_index

import next_plaid_amd as npa
from next_plaid_amd import api


def _index(path, n_docs=300, chunk_docs=70, seed=5, K=64, dim=32, nbits=2):
    spec, a = make_arrays(num_docs=n_docs, num_centroids=K, dim=dim, nbits=nbits, doc_len_min=0, doc_len_max=12, seed=seed)
    npa.write_index_dir(str(path), a["centroids"], a["bucket_weights"], a["doc_lengths"], a["codes"], a["residuals"], nbits,
                        bucket_cutoffs=np.linspace(-0.1, 0.1, (1 << nbits) - 1).astype(np.float32),
                        cluster_threshold=0.25, chunk_docs=chunk_docs)
    return a


def _flat_files(path, n_docs, dim, buffered, seed=1):
    """embeddings.npy for every document and buffer.npy for the last `buffered` ones, as the update path leaves them"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 5, n_docs)
    flat = rng.standard_normal((int(lens.sum()), dim)).astype(np.float32)
    np.save(os.path.join(path, "embeddings.npy"), flat)
    json.dump([int(x) for x in lens], open(os.path.join(path, "embeddings_lengths.json"), "w"))
    off = int(lens[: n_docs - buffered].sum())
    np.save(os.path.join(path, "buffer.npy"), flat[off:])
    json.dump([int(x) for x in lens[n_docs - buffered:]], open(os.path.join(path, "buffer_lengths.json"), "w"))
    json.dump({"num_docs": buffered}, open(os.path.join(path, "buffer_info.json"), "w"))
    for m in ("merged_codes.npy", "merged_residuals.manifest.json"):
        open(os.path.join(path, m), "wb").write(b"stale")


def _both(tmp_path, ids, **kw):
    a = tmp_path / "a"
    _index(a, **kw)
    _flat_files(str(a), kw.get("n_docs", 300), kw.get("dim", 32), buffered=20)
    b = tmp_path / "b"
    shutil.copytree(a, b)
    got = npa.delete_from_index_dir(str(a), ids)
    want = U.delete(str(b), ids)
    return str(a), str(b), got, want


@pytest.mark.parametrize("ids", [
    [3, 71, 140, 141, 299, 150],            # scattered over several chunks, the last document included
    list(range(70, 140)),                   # chunk 1 emptied: it stays, with an empty doclens
    [5, 5, 5, 8, 8],                        # duplicates count once
    [300, 1000, 2, -7],                     # out-of-range ids are ignored
    list(range(280, 300)),                  # the buffered tail: the buffer files disappear
    [],
])
def test_delete_matches_restatement(tmp_path, ids):
    a, b, got, want = _both(tmp_path, ids)
    assert got == want == len({i for i in ids if 0 <= i < 300})
    assert U.dir_state(a) == U.dir_state(b)
    info = npa.probe_index_dir(a)
    ra, rb = npy_index.read_index(a), npy_index.read_index(b)
    assert info.num_documents == ra["doc_lengths"].size == 300 - got
    for k in ("doc_lengths", "codes", "residuals", "ivf", "ivf_lengths"):
        assert np.array_equal(ra[k], rb[k]), k
    assert not os.path.exists(os.path.join(a, "merged_codes.npy"))
    assert not os.path.exists(os.path.join(a, "merged_residuals.manifest.json"))


def test_delete_whole_chunk_keeps_it(tmp_path):
    a, _, got, _ = _both(tmp_path, list(range(70, 140)))
    assert got == 70
    assert json.load(open(os.path.join(a, "doclens.1.json"))) == []
    assert np.load(os.path.join(a, "1.codes.npy")).shape == (0,)
    cm = json.load(open(os.path.join(a, "1.metadata.json")))
    assert cm["num_documents"] == 0 and cm["num_embeddings"] == 0 and "embedding_offset" in cm
    assert json.load(open(os.path.join(a, "metadata.json")))["num_chunks"] == 5


def test_negative_id_rule(tmp_path):
    """delete([-1, 3]) writes the same files as delete([3]) (the crate would shift every posting-list entry)"""
    for name, ids in (("x", [-1, 3]), ("y", [3])):
        _index(tmp_path / name)
        assert npa.delete_from_index_dir(str(tmp_path / name), ids) == 1
    fx, fy = (sorted(os.listdir(tmp_path / n)) for n in ("x", "y"))
    assert fx == fy
    for f in fx:
        assert open(tmp_path / "x" / f, "rb").read() == open(tmp_path / "y" / f, "rb").read(), f


def test_delete_cleans_flat_files(tmp_path):
    a, _, _, _ = _both(tmp_path, [0, 285, 299])
    lens = json.load(open(os.path.join(a, "embeddings_lengths.json")))
    assert len(lens) == 297 and np.load(os.path.join(a, "embeddings.npy")).shape[0] == sum(lens)
    assert json.load(open(os.path.join(a, "buffer_info.json"))) == {"num_docs": 18}
    assert len(json.load(open(os.path.join(a, "buffer_lengths.json")))) == 18


def test_delete_everything(tmp_path):
    a, b, got, want = _both(tmp_path, list(range(300)))
    assert got == want == 300
    assert U.dir_state(a) == U.dir_state(b)
    for f in ("embeddings.npy", "buffer.npy", "buffer_info.json"):
        assert not os.path.exists(os.path.join(a, f))
    m = json.load(open(os.path.join(a, "metadata.json")))
    assert m["num_documents"] == 0 and m["avg_doclen"] == 0.0 and npa.probe_index_dir(a).num_documents == 0


def test_update_struct_layouts(tmp_path):
    names = ["np_update_config", "np_update_report"]
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
        assert C.sizeof(st) == int(got[n]) == int(L.np_hip_struct_size(8 + i)), n
        for f, _ in st._fields_:
            assert getattr(st, f).offset == int(got[f"{n}.{f}"]), f"{n}.{f}"


def test_update_config_json():
    d = npa.UpdateConfig()
    assert (d.batch_size, d.kmeans_niters, d.max_points_per_centroid, d.n_samples_kmeans, d.seed, d.start_from_scratch,
            d.buffer_size) == (50_000, 4, 256, None, 42, 999, 100)
    c = npa.UpdateConfig.from_json('{"batch_size": 10, "kmeans_niters": 2, "max_points_per_centroid": 64, '
                                   '"n_samples_kmeans": 500, "seed": 3, "start_from_scratch": 0, "buffer_size": 7, '
                                   '"force_cpu": true}')
    assert c == npa.UpdateConfig(10, 2, 64, 500, 3, 0, 7)
    assert npa.UpdateConfig.from_json(c.to_json()) == c
    assert json.loads(c.to_json())["force_cpu"] is False
    with pytest.raises(ValueError, match="buffer_size"):
        npa.UpdateConfig.from_json('{"batch_size": 1, "kmeans_niters": 1, "max_points_per_centroid": 1, "seed": 1, '
                                   '"start_from_scratch": 1}')
    # 0 keeps the crate's meaning: never start from scratch past an empty index, expand on every update
    assert c._c().start_from_scratch == -1 and npa.UpdateConfig(buffer_size=0)._c().buffer_size == -1


def test_handles_without_directory_refuse():
    h = npa.MmapIndex.__new__(npa.MmapIndex)   # the Python-side state of a from_arrays / synth handle
    h._h, h._open_opts = None, {}
    for path in ("<arrays>", "<synth>"):
        h.path = path
        with pytest.raises(npa.IndexLoadError, match="directory"):
            h.update([np.ones((2, 8), np.float32)])
        with pytest.raises(npa.IndexLoadError, match="directory"):
            h.delete([0])


def test_no_gpu_update_leaves_directory(tmp_path, gpu_available):
    if gpu_available:
        pytest.skip("a GPU is present: the device path is covered by the gpu tests")
    _index(tmp_path / "a", n_docs=1200, chunk_docs=500)
    before = {f: open(tmp_path / "a" / f, "rb").read() for f in os.listdir(tmp_path / "a")}
    docs = [np.ones((4, 32), np.float32)] * 3
    with pytest.raises(npa.DeviceUnavailableError):
        npa.update_index_dir(str(tmp_path / "a"), docs)
    with pytest.raises(npa.DeviceUnavailableError):
        npa.MmapIndex.update_append(docs, str(tmp_path / "a"))
    with pytest.raises(npa.ShapeError):
        npa.update_index_dir(str(tmp_path / "a"), [np.ones((4, 16), np.float32)])
    after = {f: open(tmp_path / "a" / f, "rb").read() for f in os.listdir(tmp_path / "a")}
    assert after == before
    ids, rep = npa.update_index_dir(str(tmp_path / "a"), [])
    assert ids.size == 0 and rep["mode"] == "none"
