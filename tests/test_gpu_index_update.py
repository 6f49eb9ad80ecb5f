"""MmapIndex::update / update_append / update_or_create / delete end to end on the GPU, against the numpy restatement in
update_restate.py (update_index, delete_from_index, the mode choice, find_outliers) and the oracle's encode and search.
Needs a real MI355X."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import update_restate as U
from helpers import ROOT, RTOL_F32, assert_ranking_close, make_arrays, synth, to_oracle_params
from oracle import npy_index
from oracle import oracle as O

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu

P = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=8)


def _synth_dir(path, n_docs, K=256, dim=64, nbits=4, chunk_docs=500, thr=0.3, seed=3, len_max=24):
    """an index directory of synthetic arrays with a full codec (cutoffs, cluster_threshold)"""
    spec, a = make_arrays(num_docs=n_docs, num_centroids=K, dim=dim, nbits=nbits, doc_len_min=1, doc_len_max=len_max,
                          seed=seed)
    cut, wts = synth.bucket_tables(spec)
    npa.write_index_dir(str(path), a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], nbits,
                        bucket_cutoffs=cut, cluster_threshold=thr, chunk_docs=chunk_docs)
    return a


def _near_docs(cen, n, seed, noise=0.02, len_max=20):
    """documents whose tokens sit close to existing centroids (no outliers at thr = 0.3)"""
    rng = np.random.default_rng(seed)
    docs = []
    for _ in range(n):
        L = int(rng.integers(1, len_max))
        x = cen[rng.integers(0, cen.shape[0], L)] + noise * rng.standard_normal((L, cen.shape[1])).astype(np.float32)
        docs.append(x.astype(np.float32))
    return docs


def _files(path):
    return {f: open(os.path.join(path, f), "rb").read() for f in sorted(os.listdir(path))}


def _search_parity(path, queries, what):
    r = npy_index.read_index(path)
    ox = O.OracleIndex(r["centroids"], r["bucket_weights"], r["ivf"], r["ivf_lengths"], r["doc_lengths"], r["codes"],
                       r["residuals"], r["nbits"])
    hx = npa.MmapIndex.load(path)
    try:
        res = hx.search_batch(queries, P)
        for i, (g, o) in enumerate(zip(res, ox.search_batch(queries, to_oracle_params(P)))):
            assert_ranking_close(g.passage_ids, g.scores, o.passage_ids, o.scores, RTOL_F32, f"{what} q{i}")
    finally:
        hx.close()
    return res


def _restated_buffer_update(path, docs, batch):
    buf = U._load_flat(path, "buffer.npy", "buffer_lengths.json")
    U._save_flat(path, "buffer.npy", "buffer_lengths.json", buf + list(docs), docs[0].shape[1])
    U._w(os.path.join(path, "buffer_info.json"), {"num_docs": len(buf) + len(docs)})
    U.update_index(path, docs, batch, False)


@pytest.mark.parametrize("n_old,chunk_docs,batch", [(1200, 500, 50_000), (2600, 2600, 7)])
def test_buffer_mode(tmp_path, n_old, chunk_docs, batch):
    """last chunk < 2000 documents: the new ones join it; >= 2000: new chunks of batch_size documents"""
    a = tmp_path / "a"
    arr = _synth_dir(a, n_old, chunk_docs=chunk_docs)
    b = tmp_path / "b"
    shutil.copytree(a, b)
    before = _files(a)
    docs = _near_docs(arr["centroids"], 30, seed=1)
    cfg = npa.UpdateConfig(batch_size=batch)
    hx = npa.MmapIndex.load(str(a))
    ids = hx.update(docs, cfg)
    assert hx.last_update["mode"] == "buffer" and U.mode(str(b), len(docs)) == "buffer"
    assert ids.tolist() == list(range(n_old, n_old + 30)) and hx.num_documents() == n_old + 30
    hx.close()
    _restated_buffer_update(str(b), docs, batch)
    assert U.dir_state(str(a)) == U.dir_state(str(b))
    after = _files(a)
    nch = json.load(open(a / "metadata.json"))["num_chunks"]
    assert nch == (3 if batch > 30 else 1 + 30 // 7 + 1)
    for f in ("0.codes.npy", "0.residuals.npy", "doclens.0.json", "centroids.npy", "bucket_weights.npy"):
        if chunk_docs == 500:
            assert after[f] == before[f], f
    assert json.load(open(a / "buffer_info.json")) == {"num_docs": 30}
    # new codes and residuals are the oracle's encode with the index's codec
    r = npy_index.read_index(str(a))
    cut = np.load(a / "bucket_cutoffs.npy")
    rc, rp = O.encode_tokens(np.concatenate(docs), arr["centroids"], 4, cut)
    T0 = int(arr["doc_lengths"].sum())
    assert np.array_equal(r["codes"][T0:], rc) and np.array_equal(r["residuals"][T0:], rp)
    res = _search_parity(str(a), [d[:8] for d in docs], "buffer")
    assert np.mean([x.passage_ids[0] == i for x, i in zip(res, ids)]) >= 0.8


def _planted(cen, thr, rng, n_far, n_edge):
    """far-away tokens, and tokens at thr^2 (1 +- 2e-6) from their centroid so that the f64 recheck decides"""
    dim = cen.shape[1]
    far = rng.standard_normal((n_far, dim)).astype(np.float32) * 3
    edge = []
    for i in range(n_edge):
        c = cen[rng.integers(0, cen.shape[0])].astype(np.float64)
        u = rng.standard_normal(dim)
        u -= (u @ c) / (c @ c) * c
        u /= np.linalg.norm(u)
        r2 = float(thr) ** 2 * (1 + (2e-6 if i % 2 else -2e-6))
        edge.append((c + np.sqrt(r2) * u).astype(np.float32))
    return far, np.array(edge, np.float32)


def test_expansion_mode(tmp_path):
    a = tmp_path / "a"
    arr = _synth_dir(a, 1200, thr=0.3)
    cen = arr["centroids"]
    cfg = npa.UpdateConfig(kmeans_niters=3, max_points_per_centroid=16, seed=11)
    first = _near_docs(cen, 30, seed=2)
    ids1, rep1 = npa.update_index_dir(str(a), first, cfg)
    assert rep1["mode"] == "buffer"
    b = tmp_path / "b"
    shutil.copytree(a, b)
    rng = np.random.default_rng(5)
    far, edge = _planted(cen, np.load(a / "cluster_threshold.npy")[0], rng, 40, 40)
    docs = _near_docs(cen, 80, seed=3)
    for i in range(40):
        docs[i] = np.concatenate([docs[i], far[i:i + 1], edge[i:i + 1]])
    assert U.mode(str(b), len(docs)) == "expansion"
    hx = npa.MmapIndex.load(str(a))
    ids = hx.update(docs, cfg)
    rep = hx.last_update
    hx.close()
    assert rep["mode"] == "expansion" and rep["n_reindexed"] == 30
    assert ids.tolist() == list(range(1230, 1310))
    # the outlier set = the restatement's (f64 distances), the planted edge tokens split by it
    comb = np.concatenate(first + docs)
    thr = np.load(b / "cluster_threshold.npy")[0]
    out = U.find_outliers(comb, cen, thr)
    assert rep["n_outliers"] == out.size and rep["n_rechecked"] > 0
    assert 40 < out.size < 80
    k_up = U.k_update(out.size, 16)
    kc = npa.compute_kmeans([comb[i][None] for i in out], npa.IndexConfig(kmeans_niters=3, max_points_per_centroid=16,
                                                                            seed=11), num_partitions=k_up)
    newc = np.load(a / "centroids.npy")
    assert rep["n_new_centroids"] == kc.shape[0] == newc.shape[0] - cen.shape[0]
    assert newc[cen.shape[0]:].tobytes() == kc.tobytes()
    # the whole directory = the restated sequence with those centroids
    U.delete(str(b), list(range(1200, 1230)), clean_buffer=False)
    np.save(b / "centroids.npy", newc)
    U._remove(str(b), ["buffer.npy", "buffer_lengths.json", "buffer_info.json"])
    U.update_index(str(b), first + docs, 50_000, True)
    sa, sb = U.dir_state(str(a)), U.dir_state(str(b))
    assert sa.keys() == sb.keys()
    for f in sa:
        assert sa[f] == sb[f], f
    assert not os.path.exists(a / "buffer.npy")
    _search_parity(str(a), [d[:8] for d in docs[:40]], "expansion")


def test_codes_go_wide(tmp_path):
    """K = 65 536 gains centroids: after the reload the codes are 32-bit on the device; search parity holds"""
    a = tmp_path / "a"
    arr = _synth_dir(a, 2000, K=65536, dim=32, nbits=2, thr=0.05, len_max=8)
    rng = np.random.default_rng(9)
    docs = [rng.standard_normal((4, 32)).astype(np.float32) * 2 for _ in range(100)]
    hx = npa.MmapIndex.load(str(a))
    hx.update(docs, npa.UpdateConfig(buffer_size=50))
    assert hx.last_update["mode"] == "expansion" and hx.last_update["n_new_centroids"] > 0
    assert hx.num_partitions() > 65536
    hx.close()
    _search_parity(str(a), docs[:16] + [np.asarray(arr["centroids"][:4])], "wide codes")


def _real_docs(n, dim, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((64, dim)).astype(np.float32)
    docs = []
    for _ in range(n):
        L = int(rng.integers(2, 20))
        x = base[rng.integers(0, 64, L)] + 0.3 * rng.standard_normal((L, dim)).astype(np.float32)
        docs.append((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))
    return docs


def test_start_from_scratch(tmp_path):
    docs = _real_docs(350, 64, 1)
    icfg = npa.IndexConfig(nbits=4, batch_size=100, seed=5)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    npa.MmapIndex.create_with_kmeans(docs[:300], a, icfg).close()
    assert os.path.exists(os.path.join(a, "embeddings.npy"))
    ucfg = npa.UpdateConfig(batch_size=100, seed=5, start_from_scratch=320)
    ids, rep = npa.update_index_dir(a, docs[300:], ucfg)
    assert rep["mode"] == "start_from_scratch" and ids.tolist() == list(range(300, 350))
    npa.MmapIndex.create_with_kmeans(docs, b, npa.IndexConfig(nbits=4, batch_size=100, seed=5, start_from_scratch=320)).close()
    assert _files(a) == _files(b)                            # 350 > 320: embeddings.npy cleared
    assert not os.path.exists(os.path.join(a, "embeddings.npy"))
    # above the threshold a delete leaves embeddings.npy out of sync: the next update takes the buffer mode
    assert npa.delete_from_index_dir(a, list(range(100))) == 100
    assert U.mode(a, 5, 999) == "buffer"
    ids, rep = npa.update_index_dir(a, docs[:5], npa.UpdateConfig())
    assert rep["mode"] == "buffer" and ids.tolist() == list(range(250, 255))


def test_update_or_create_and_append(tmp_path):
    docs = _real_docs(1100, 32, 2)
    p = str(tmp_path / "x")
    hx, ids = npa.MmapIndex.update_or_create(docs[:1000], p, npa.IndexConfig(nbits=2, seed=3))
    assert ids.tolist() == list(range(1000)) and hx.num_documents() == 1000
    hx.close()
    hx, ids = npa.MmapIndex.update_or_create(docs[1000:1010], p)
    assert ids.tolist() == list(range(1000, 1010)) and hx.last_update["mode"] == "buffer"
    hx.close()
    q = str(tmp_path / "q")
    shutil.copytree(p, q)
    ids = npa.MmapIndex.update_append(docs[1010:1100], q, npa.UpdateConfig(batch_size=40))
    assert ids.tolist() == list(range(1010, 1100))
    assert json.load(open(os.path.join(q, "buffer_info.json"))) == {"num_docs": 10}   # untouched, as the crate
    r = tmp_path / "r"
    shutil.copytree(p, r)
    U.update_index(str(r), docs[1010:1100], 40, False)
    assert U.dir_state(q) == U.dir_state(str(r))


def test_refused_inputs_leave_directory(tmp_path):
    a = tmp_path / "a"
    _synth_dir(a, 600)
    before = _files(a)
    with pytest.raises(npa.ShapeError):
        npa.update_index_dir(str(a), [np.ones((3, 32), np.float32)])
    bad = np.ones((3, 64), np.float32)
    bad[1, 5] = np.nan
    with pytest.raises(npa.IndexCreationError):
        npa.update_index_dir(str(a), [bad])
    with pytest.raises(npa.IndexCreationError):
        npa.MmapIndex.update_append([bad], str(a))
    ids, rep = npa.update_index_dir(str(a), [])
    assert ids.size == 0 and rep["mode"] == "none"
    assert _files(a) == before


def test_delete_then_reload(tmp_path):
    a = tmp_path / "a"
    arr = _synth_dir(a, 900)
    hx = npa.MmapIndex.load(str(a))
    dele = list(range(0, 900, 7)) + [450, 899]
    assert hx.delete(dele) == len(set(dele))
    assert hx.num_documents() == 900                         # no reload, as the crate
    hx.reload()
    assert hx.num_documents() == 900 - len(set(dele))
    keep = np.setdiff1d(np.arange(900), dele)
    off = np.concatenate([[0], np.cumsum(arr["doc_lengths"])])
    tok = np.concatenate([np.arange(off[d], off[d + 1]) for d in keep])
    ivf, il = npy_index.build_ivf(arr["codes"][tok], arr["doc_lengths"][keep], 256)
    ox = O.OracleIndex(arr["centroids"], arr["bucket_weights"], ivf, il, arr["doc_lengths"][keep], arr["codes"][tok],
                       arr["residuals"][tok], 4)
    rng = np.random.default_rng(4)
    qs = [arr["centroids"][rng.integers(0, 256, 6)] for _ in range(16)]
    for i, (g, o) in enumerate(zip(hx.search_batch(qs, P), ox.search_batch(qs, to_oracle_params(P)))):
        assert_ranking_close(g.passage_ids, g.scores, o.passage_ids, o.scores, RTOL_F32, f"after delete q{i}")
    hx.close()


def test_cpp_mirror_updates_the_same_directory(tmp_path):
    cpp = os.path.join(ROOT, "tests", "cpp", "update_index.cpp")
    exe = tmp_path / "update_index"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), cpp, "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"),
                           "-L", os.path.join(ROOT, "next-plaid_amd", "csrc"), "-lnextplaid_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "next-plaid_amd", "csrc")])
    arr = _synth_dir(tmp_path / "py", 700)
    shutil.copytree(tmp_path / "py", tmp_path / "cpp")
    docs = _near_docs(arr["centroids"], 40, seed=8)
    dele = np.array([1, 5, 699, 702, -3], np.int64)
    np.concatenate(docs).astype("<f4").tofile(tmp_path / "emb.f32")
    np.array([d.shape[0] for d in docs], "<i8").tofile(tmp_path / "lens.i64")
    dele.tofile(tmp_path / "del.i64")
    hx = npa.MmapIndex.load(str(tmp_path / "py"))
    hx.update(docs, npa.UpdateConfig(buffer_size=30))
    assert hx.delete(dele) == 4
    hx.close()
    subprocess.check_call([str(exe), str(tmp_path / "cpp"), str(tmp_path / "emb.f32"), str(tmp_path / "lens.i64"), "64", "30",
                           str(tmp_path / "del.i64")])
    assert _files(str(tmp_path / "py")) == _files(str(tmp_path / "cpp"))
