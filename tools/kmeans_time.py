#!/usr/bin/env python3
"""Times the GPU k-means (np_hip_kmeans) and the whole create path; one JSON line per measurement.

  python tools/kmeans_time.py --shape 16777216,65536,128,2 --shape 67108864,262144,128,1
  python tools/kmeans_time.py --create 200000,100,128 --numpy-ref

--shape n,k,d,iters: clustered synthetic points (k/4 centres + noise), seeded init, no subsample, `iters` Lloyd iterations
(tol 0: every iteration runs).  Per line: ms per iteration split into assign (distance GEMM + argmin) and update (count,
counting sort, fixed-point means, re-initialisation, shift), the assign rate 2 n k d / t in TFLOP/s and its share of the
157.3 TF f32-MFMA peak, and the update's bytes/s (its minimum traffic: the points read once by the means, the ids written
and read by the counting sort, the centroids read and written).
--create docs,tokens,dim: MmapIndex.create_with_kmeans on a synth-style corpus, split into k-means, codec artifacts,
encode and write (the pieces timed one by one through the public API, then the whole call).
--numpy-ref: one host Lloyd iteration in numpy (f32 GEMM + argmin + means) on a slice of the create corpus' k-means
input, scaled to the full iteration by FLOPs: the CPU reference point, labelled as such.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "next-plaid_amd"))
import next_plaid_amd as npa  # noqa: E402

PEAK_TF = 157.3


def clustered(n, k, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((max(k // 4, 1), d), dtype=np.float32)
    x = np.empty((n, d), np.float32)
    step = 1 << 21
    for i in range(0, n, step):
        m = min(step, n - i)
        rng.standard_normal((m, d), dtype=np.float32, out=x[i:i + m])
        x[i:i + m] *= 0.3
        x[i:i + m] += centres[rng.integers(0, centres.shape[0], m)]
    return x


def time_shape(n, k, d, iters):
    x = clustered(n, k, d, 1)
    init = x[np.random.default_rng(2).choice(n, k, replace=False)]
    t = time.perf_counter()
    _, rep = npa.kmeans(x, k, max_iters=iters, tol=0.0, init=init, max_points_per_centroid=0)
    wall = time.perf_counter() - t
    it = rep["iterations"]
    ms_a, ms_u = rep["ms_assign"] / it, rep["ms_update"] / it
    tf = 2.0 * n * k * d / (ms_a * 1e-3) / 1e12
    upd_bytes = n * d * 4 + n * 4 * 4 + 2 * k * d * 4
    print(json.dumps(dict(what="kmeans", n=n, k=k, d=d, iterations=it, ms_per_iter=round(ms_a + ms_u, 3),
                          ms_assign=round(ms_a, 3), ms_update=round(ms_u, 3), assign_tflops=round(tf, 2),
                          assign_frac_f32_mfma_peak=round(tf / PEAK_TF, 4), update_share=round(ms_u / (ms_a + ms_u), 4),
                          update_gbps=round(upd_bytes / (ms_u * 1e-3) / 1e9, 1), n_reinit=rep["n_reinit"],
                          wall_s_incl_host=round(wall, 2))), flush=True)


def corpus(n_docs, tokens, d, seed=5):
    x = clustered(n_docs * tokens, 4096, d, seed)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return [x[i * tokens:(i + 1) * tokens] for i in range(n_docs)], x


def time_create(n_docs, tokens, d, numpy_ref):
    docs, flat = corpus(n_docs, tokens, d)
    cfg = npa.IndexConfig(nbits=4)
    out = {"what": "create_with_kmeans", "docs": n_docs, "tokens_per_doc": tokens, "dim": d}
    t = time.perf_counter()
    cen, rep = npa.compute_kmeans(docs, cfg, return_report=True)
    out["s_kmeans"] = round(time.perf_counter() - t, 3)
    out.update(K=int(cen.shape[0]), kmeans_points=rep["n_points"], kmeans_iterations=rep["iterations"],
               kmeans_ms_assign=round(rep["ms_assign"], 1), kmeans_ms_update=round(rep["ms_update"], 1))
    t = time.perf_counter()
    art = npa.prepare_codec_artifacts(docs, cen, cfg)
    out["s_artifacts"] = round(time.perf_counter() - t, 3)
    t = time.perf_counter()
    enc = npa.MmapIndex.from_arrays(cen, art["bucket_weights"], np.zeros(1, np.int64), np.eye(1, cen.shape[0], dtype=np.int32)[0],
                                    np.ones(1, np.int64), np.zeros(1, np.int64), np.zeros((1, d * 4 // 8), np.uint8), 4)
    codes, packed = enc.encode_tokens(flat, art["bucket_cutoffs"])
    enc.close()
    out["s_encode"] = round(time.perf_counter() - t, 3)
    tmp = tempfile.mkdtemp(prefix="np_create_")
    try:
        t = time.perf_counter()
        npa.write_index_dir(os.path.join(tmp, "w"), cen, art["bucket_weights"], np.full(n_docs, tokens, np.int64), codes,
                            packed, 4, bucket_cutoffs=art["bucket_cutoffs"], avg_residual=art["avg_residual"],
                            cluster_threshold=float(art["cluster_threshold"]))
        out["s_write"] = round(time.perf_counter() - t, 3)
        t = time.perf_counter()
        npa.MmapIndex.create_with_kmeans(docs, os.path.join(tmp, "c"), cfg).close()
        out["s_create_with_kmeans_total"] = round(time.perf_counter() - t, 3)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out), flush=True)
    if numpy_ref:
        p, ids = npa.kmeans_plan(np.full(n_docs, tokens, np.int64), cfg)
        pts = np.concatenate([docs[i] for i in ids[: max(1, 4096 // tokens)]], 0)[:4096]
        c = cen.astype(np.float32)
        t = time.perf_counter()
        dist = (pts * pts).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * pts @ c.T
        a = dist.argmin(1)
        sums = np.zeros_like(c)
        np.add.at(sums, a, pts)
        cnt = np.bincount(a, minlength=c.shape[0])
        _ = sums / np.maximum(cnt, 1)[:, None]
        s = time.perf_counter() - t
        full = s * p["sample_tokens"] / pts.shape[0]
        print(json.dumps(dict(what="numpy_lloyd_iteration_cpu_reference", threads=os.environ.get("OMP_NUM_THREADS"),
                              points_timed=int(pts.shape[0]), k=int(c.shape[0]), d=d, s_timed=round(s, 3),
                              s_per_iteration_scaled_to_points=round(full, 1), points=p["sample_tokens"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=[], help="n,k,d,iters")
    ap.add_argument("--create", default=None, help="docs,tokens,dim")
    ap.add_argument("--numpy-ref", action="store_true")
    a = ap.parse_args()
    if npa.device_count() < 1:
        raise SystemExit("kmeans_time.py needs a gfx950 GPU")
    for s in a.shape:
        n, k, d, it = (int(v) for v in s.split(","))
        time_shape(n, k, d, it)
    if a.create:
        n_docs, tokens, d = (int(v) for v in a.create.split(","))
        time_create(n_docs, tokens, d, a.numpy_ref)


if __name__ == "__main__":
    main()
