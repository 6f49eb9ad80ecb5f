#!/usr/bin/env python3
"""Times MmapIndex.update on a large index; one JSON line per measurement.

  python tools/update_time.py --docs 1000000 --k 65536 --new 100,10000

The index is a synthetic corpus (next_plaid_amd.synth, generated in HBM, exported and written as a directory with the
synthetic codec and cluster_threshold 0.3).  Each --new size n runs one update of n documents drawn near the index's
centroids, with buffer_size = 100, on a fresh copy of the directory: n < 100 takes the buffer mode, n >= 100 the
expansion mode (its outliers are the tokens farther than the threshold).  Per line: the report's stage times (host wall
time of encode, outlier search, k-means and the file reads and rewrites), the whole update call and the reload
(MmapIndex.load of the rewritten directory).
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
from next_plaid_amd import synth  # noqa: E402


def write_synth_index(path, n_docs, k, dim, lmin, lmax, seed):
    spec = synth.SynthSpec(num_docs=n_docs, num_centroids=k, dim=dim, doc_len_min=lmin, doc_len_max=lmax, seed=seed)
    cen = synth.centroids(spec)
    cut, wts = synth.bucket_tables(spec)
    hx = npa.MmapIndex.synth(spec, cen)
    e = hx.export()
    hx.close()
    npa.write_index_dir(path, cen, wts, e["doc_lengths"], e["codes"], e["residuals"], spec.nbits, ivf=e["ivf"],
                        ivf_lengths=e["ivf_lengths"], bucket_cutoffs=cut, cluster_threshold=0.3)
    return cen, int(e["codes"].size)


def new_docs(cen, n, lmin, lmax, seed):
    rng = np.random.default_rng(seed)
    docs = []
    for _ in range(n):
        L = int(rng.integers(lmin, lmax + 1))
        x = cen[rng.integers(0, cen.shape[0], L)] + 0.02 * rng.standard_normal((L, cen.shape[1])).astype(np.float32)
        docs.append(x.astype(np.float32))
    return docs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--len", default="16,48", help="document length range min,max")
    ap.add_argument("--new", default="100,10000", help="comma-separated update sizes")
    ap.add_argument("--dir", default=None, help="scratch directory (default: a temporary one)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    lmin, lmax = (int(x) for x in a.len.split(","))
    tmp = a.dir or tempfile.mkdtemp(prefix="np_update_time_")
    base = os.path.join(tmp, "base")
    t0 = time.perf_counter()
    cen, T = write_synth_index(base, a.docs, a.k, a.dim, lmin, lmax, 7)
    t_write = time.perf_counter() - t0
    lines = []
    try:
        for n in (int(x) for x in a.new.split(",")):
            d = os.path.join(tmp, f"u{n}")
            shutil.rmtree(d, ignore_errors=True)
            shutil.copytree(base, d)
            docs = new_docs(cen, n, lmin, lmax, n)
            t0 = time.perf_counter()
            ids, rep = npa.update_index_dir(d, docs, npa.UpdateConfig(buffer_size=100))
            t_update = time.perf_counter() - t0
            t0 = time.perf_counter()
            hx = npa.MmapIndex.load(d)
            t_reload = time.perf_counter() - t0
            assert hx.num_documents() == a.docs + n and ids[0] == a.docs
            hx.close()
            line = dict(what="update", index_docs=a.docs, index_tokens=T, k=a.k, dim=a.dim, new_docs=n,
                        new_tokens=int(sum(x.shape[0] for x in docs)), index_write_s=round(t_write, 2), **rep,
                        ms_update_call=round(1e3 * t_update, 1), ms_reload=round(1e3 * t_reload, 1))
            for f in ("ms_encode", "ms_outliers", "ms_kmeans", "ms_files"):
                line[f] = round(line[f], 1)
            print(json.dumps(line), flush=True)
            lines.append(line)
            shutil.rmtree(d, ignore_errors=True)
    finally:
        if not a.dir:
            shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
