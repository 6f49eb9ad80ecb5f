"""MmapIndex.create_with_kmeans (index.rs:927-967) end to end on the GPU: the centroids are compute_kmeans' output, the
codec tables a numpy restatement of index.rs:182-287, the encoded data the oracle's encode, searches the oracle's search,
and a second creation is byte-identical.  Needs a real MI355X."""
import json
import os
import subprocess

import numpy as np
import pytest

import kmeans_restate as R
from helpers import ROOT, RTOL_F32, assert_ranking_close, make_arrays, synth, to_oracle_params
from oracle import oracle as O

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu


def _corpus(n_docs, dim, nbits, seed):
    spec, a = make_arrays(num_docs=n_docs, num_centroids=256, dim=dim, nbits=nbits, doc_len_min=0, doc_len_max=40,
                          seed=seed)
    _, wts = synth.bucket_tables(spec)
    lens = np.asarray(a["doc_lengths"], np.int64)
    emb = synth.reconstruct(a["codes"], a["residuals"], a["centroids"], wts, nbits)
    rng = np.random.default_rng(seed + 1)
    emb = emb + (0.05 / np.sqrt(dim)) * rng.standard_normal(emb.shape).astype(np.float32)
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(lens)])
    docs = [emb[off[i]:off[i + 1]] for i in range(n_docs)]
    assert (lens == 0).any()
    return docs, emb, lens


def _codec_restated(docs, lens, cen, nbits, seed):
    N, T = len(docs), int(lens.sum())
    sample = R.shuffled_docs(N, seed)[: R.codec_samples(N)]
    hs = int(min(0.05 * T, 50000.0))
    rows, got = [], 0
    for i in reversed(sample):
        if got >= hs:
            break
        take = min(hs - got, docs[i].shape[0])
        rows.append(docs[i][:take])
        got += take
    held = np.concatenate(rows, 0)
    codes, _ = O.encode_tokens(held, cen, nbits, np.zeros((1 << nbits) - 1, np.float32))
    r = (held - cen[codes]).astype(np.float32)
    flat = np.sort(r.ravel())
    nb = 1 << nbits
    cut = np.array([R.quantile(flat, i / nb) for i in range(1, nb)], np.float32)
    wts = np.array([R.quantile(flat, (i + 0.5) / nb) for i in range(nb)], np.float32)
    ss = np.cumsum(r * r, axis=1, dtype=np.float32)[:, -1]                 # sequential f32 sums
    thr = R.quantile(np.sort(np.sqrt(ss)), 0.75)
    avg = np.cumsum(np.abs(r), axis=0, dtype=np.float32)[-1] / np.float32(r.shape[0])
    return cut, wts, avg, thr


def _files(path):
    return {f: open(os.path.join(path, f), "rb").read() for f in sorted(os.listdir(path))}


@pytest.mark.parametrize("dim,nbits", [(96, 2), (128, 4), (104, 1), (48, 8), (8, 2)])
def test_create_with_kmeans(tmp_path, dim, nbits):
    docs, emb, lens = _corpus(1200, dim, nbits, seed=dim + nbits)
    cfg = npa.IndexConfig(nbits=nbits, batch_size=500, seed=7)
    d1 = str(tmp_path / "a")
    hx = npa.MmapIndex.create_with_kmeans(docs, d1, cfg)
    cen = npa.compute_kmeans(docs, cfg)
    plan, _ = npa.kmeans_plan(lens, cfg)
    assert cen.shape[0] == plan["k"] == npa.estimate_num_partitions(docs, cfg)
    assert np.array_equal(np.load(os.path.join(d1, "centroids.npy")), cen)
    art = npa.prepare_codec_artifacts(docs, cen, cfg)
    cut, wts, avg, thr = _codec_restated(docs, lens, cen, nbits, 7)
    assert np.array_equal(art["bucket_cutoffs"], cut) and np.array_equal(art["bucket_weights"], wts)
    assert np.allclose(art["avg_residual"], avg, rtol=1e-6) and np.isclose(art["cluster_threshold"], thr, rtol=1e-6)
    assert np.array_equal(np.load(os.path.join(d1, "bucket_cutoffs.npy")), cut)
    assert np.array_equal(np.load(os.path.join(d1, "bucket_weights.npy")), wts)
    # encoded data = the oracle's encode; posting lists = the crate's
    rc, rp = O.encode_tokens(emb, cen, nbits, cut)
    e = hx.export()
    assert np.array_equal(e["codes"], rc) and np.array_equal(e["residuals"], rp)
    ivf, il = synth.build_ivf(rc, lens, cen.shape[0])
    assert np.array_equal(e["ivf"], ivf) and np.array_equal(e["ivf_lengths"], il)
    # search = the oracle's search on the same arrays; a document's own tokens find it
    ox = O.OracleIndex(cen, wts, ivf, il, lens, rc, rp, nbits)
    off = np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng(3)
    ids = rng.choice(np.nonzero(lens >= 4)[0], 64, replace=False)
    qs = [docs[i][:16] for i in ids]
    p = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=8)
    res = hx.search_batch(qs, p)
    for i, (g, o) in enumerate(zip(res, ox.search_batch(qs, to_oracle_params(p)))):
        assert_ranking_close(g.passage_ids, g.scores, o.passage_ids, o.scores, RTOL_F32, f"created index q{i}")
    assert np.mean([r.passage_ids[0] == i for r, i in zip(res, ids)]) >= 0.95
    lx = npa.MmapIndex.load(d1)
    for g, h in zip(res, lx.search_batch(qs, p)):
        assert np.array_equal(g.passage_ids, h.passage_ids) and np.array_equal(g.scores, h.scores)
    # reproducible: a second directory is byte-identical; 1200 documents > 999: no embeddings.npy
    d2 = str(tmp_path / "b")
    npa.MmapIndex.create_with_kmeans(docs, d2, cfg).close()
    assert _files(d1) == _files(d2)
    assert not os.path.exists(os.path.join(d1, "embeddings.npy"))
    assert not os.path.exists(os.path.join(d1, "embeddings_lengths.json"))
    for h in (hx, lx):
        h.close()


@pytest.mark.parametrize("dim", [128, 100])
def test_compute_kmeans_is_kmeans_on_the_sample(dim):
    """compute_kmeans = np_hip_kmeans on the sampled documents' tokens (shuffled order), tol 1e-8, then every row
    divided by max(sqrtf(k-ordered fmaf chain of its squares), 1e-12): bit for bit"""
    docs, _, lens = _corpus(1500, dim, 4, seed=dim)
    cfg = npa.IndexConfig(seed=13, kmeans_niters=3, max_points_per_centroid=8)
    cen, rep = npa.compute_kmeans(docs, cfg, return_report=True)
    plan, ids = npa.kmeans_plan(lens, cfg)
    pts = np.concatenate([docs[i] for i in ids])
    raw, r2 = npa.kmeans(pts, plan["k"], max_iters=3, tol=1e-8, seed=13, max_points_per_centroid=8)
    assert r2["n_points"] < pts.shape[0]                      # the subsample is active
    nrm = np.maximum(O.kmeans_shift_parts(np.zeros_like(raw), raw), np.float32(1e-12))
    assert cen.tobytes() == (raw / nrm[:, None]).astype(np.float32).tobytes()
    for f in ("iterations", "shift", "n_points", "n_reinit"):
        assert rep[f] == r2[f], f


def test_corpus_without_heldout_tokens(tmp_path):
    """19 tokens: heldout_size = floor(0.05 * 19) = 0, so the codec statistics are those of no rows: avg_residual 0 / 0
    = NaN, cutoffs, weights and threshold the quantile of an empty array (0).  The index is still written and opens."""
    rng = np.random.default_rng(19)
    lens = np.array([3, 0, 5, 4, 7], np.int64)
    emb = rng.standard_normal((int(lens.sum()), 64)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    off = np.concatenate([[0], np.cumsum(lens)])
    docs = [emb[off[i]:off[i + 1]] for i in range(lens.size)]
    cfg = npa.IndexConfig(nbits=2, seed=5)
    plan, _ = npa.kmeans_plan(lens, cfg)
    assert plan["heldout_size"] == 0 and plan["heldout_tokens"] == 0
    cen = npa.compute_kmeans(docs, cfg)
    art = npa.prepare_codec_artifacts(docs, cen, cfg)
    assert np.all(np.isnan(art["avg_residual"])) and art["avg_residual"].shape == (64,)
    assert np.all(art["bucket_cutoffs"] == 0) and np.all(art["bucket_weights"] == 0) and art["cluster_threshold"] == 0
    d = str(tmp_path / "t")
    hx = npa.MmapIndex.create_with_kmeans(docs, d, cfg)
    assert np.array_equal(np.load(os.path.join(d, "centroids.npy")), cen)
    assert np.all(np.isnan(np.load(os.path.join(d, "avg_residual.npy"))))
    assert np.all(np.load(os.path.join(d, "bucket_cutoffs.npy")) == 0)
    assert np.all(np.load(os.path.join(d, "bucket_weights.npy")) == 0)
    rc, rp = O.encode_tokens(emb, cen, 2, np.zeros(3, np.float32))
    e = hx.export()
    assert np.array_equal(e["codes"], rc) and np.array_equal(e["residuals"], rp)
    assert np.array_equal(np.load(os.path.join(d, "embeddings.npy")), emb)
    lx = npa.MmapIndex.load(d)
    assert lx.num_partitions() == cen.shape[0]
    for h in (hx, lx):
        h.close()


def test_start_from_scratch_embeddings(tmp_path):
    docs, emb, lens = _corpus(500, 128, 4, seed=41)
    d = str(tmp_path / "i")
    npa.MmapIndex.create_with_kmeans(docs, d, npa.IndexConfig(seed=3)).close()
    assert np.array_equal(np.load(os.path.join(d, "embeddings.npy")), emb)
    assert json.load(open(os.path.join(d, "embeddings_lengths.json"))) == lens.tolist()


def test_cpp_mirror_creates_the_same_directory(tmp_path):
    cpp = os.path.join(ROOT, "tests", "cpp", "create_index.cpp")
    exe = tmp_path / "create_index"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), cpp, "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"),
                           "-L", os.path.join(ROOT, "next-plaid_amd", "csrc"), "-lnextplaid_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "next-plaid_amd", "csrc")])
    docs, emb, lens = _corpus(700, 96, 2, seed=5)
    emb.astype("<f4").tofile(tmp_path / "emb.f32")
    lens.astype("<i8").tofile(tmp_path / "lens.i64")
    cfg = npa.IndexConfig(nbits=2, batch_size=300, seed=11)
    npa.MmapIndex.create_with_kmeans(docs, str(tmp_path / "py"), cfg).close()
    subprocess.check_call([str(exe), str(tmp_path / "emb.f32"), str(tmp_path / "lens.i64"), "96", "2", "300", "11",
                           str(tmp_path / "cpp")])
    assert _files(str(tmp_path / "py")) == _files(str(tmp_path / "cpp"))
