#!/usr/bin/env python3
"""Times token pooling on the GPU (np_hip_pool_documents) beside a plain host implementation; one JSON line per corpus.

  python tools/pool_time.py                                   # both corpora at their full size
  python tools/pool_time.py --docs 20000 --short-docs 200000  # smaller, same shapes

Corpora (pool_factor 2, one protected token):
  long    --docs x --tokens x --dim           100 000 x 300 x 128: clustered unit rows
  short   --short-docs documents              lengths from the clipped LogNormal of SURVEY.md config 3 (mean ~73, max 180)
Each corpus is generated and pooled in slabs of --slab documents, so host memory stays bounded.  Per line: documents/s and
tokens/s of the whole call (host wall time, copies included) and of the device stages alone, the three stage times
(distances, linkage, means), and the same corpus through tools/pool_host.cpp (the same algorithm as plain C++ on --threads
host threads, compiled here with g++ -O2 -ffp-contract=off).  The two results are compared bit for bit on every document the
host run takes (--host-docs per slab, 0 = all) and the tool stops if they differ.  NP_POOL_LDS_MAX=0 in the environment
keeps every distance matrix in the global scratch instead of LDS (same results): run the tool twice to compare the two.
Lines are appended to --out (profiles/pool_time.jsonl)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "next-plaid_amd"))
import next_plaid_amd as npa  # noqa: E402
from next_plaid_amd import api, synth  # noqa: E402


def build_host(tmp):
    so = os.path.join(tmp, "pool_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-pthread",
                           os.path.join(ROOT, "tools", "pool_host.cpp"), "-o", so])
    L = C.CDLL(so)
    L.pool_host.argtypes = [C.c_void_p] * 3 + [C.c_int64] + [C.c_int] * 5 + [C.c_void_p]
    return L


def slab_tokens(rng, lens, dim):
    """Clustered unit rows: every document draws its tokens around max(1, n / 6) of its own topic directions."""
    T = int(lens.sum())
    x = rng.standard_normal((T, dim), dtype=np.float32)
    x *= 0.35
    topics = np.maximum(lens // 6, 1)
    first = np.concatenate([[0], np.cumsum(topics)])
    cen = rng.standard_normal((int(first[-1]), dim), dtype=np.float32)
    doc = np.repeat(np.arange(lens.size), lens)
    pick = first[doc] + (rng.integers(0, 1 << 30, T) % topics[doc])
    x += cen[pick]
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    return x


def run(name, all_lens, dim, a, host):
    rng = np.random.default_rng(9)
    tot = dict(docs=0, pooled=0, tokens_in=0, tokens_out=0, ms_distances=0.0, ms_linkage=0.0, ms_means=0.0, gpu_wall=0.0,
               host_docs=0, host_tokens=0, host_wall=0.0, chunks=0)
    o = api.np_pool_opts(a.factor, 1, 0, 0, 0)
    for s0 in range(0, all_lens.size, a.slab):
        lens = np.ascontiguousarray(all_lens[s0:s0 + a.slab], np.int64)
        x = slab_tokens(rng, lens, dim)
        plen = api.pooled_lengths(lens, a.factor, 1)
        out = np.empty((max(int(plen.sum()), 1), dim), np.float32)
        olen = np.zeros(lens.size, np.int64)
        rep = api.np_pool_report()
        t = time.perf_counter()
        api._check(api.lib().np_hip_pool_documents(a.device, api._ptr(x), api._ptr(lens), lens.size, dim, C.byref(o),
                                                   api._ptr(out), int(plen.sum()), api._ptr(olen), None, None, C.byref(rep)))
        tot["gpu_wall"] += time.perf_counter() - t
        assert np.array_equal(olen, plen)
        for k in ("ms_distances", "ms_linkage", "ms_means"):
            tot[k] += getattr(rep, k)
        tot["docs"] += lens.size
        tot["pooled"] += rep.n_pooled
        tot["tokens_in"] += rep.tokens_in
        tot["tokens_out"] += rep.tokens_out
        tot["chunks"] += rep.n_chunks
        nh = lens.size if a.host_docs == 0 else min(lens.size, a.host_docs)
        if host is not None and nh > 0:
            in_rows = np.concatenate([[0], np.cumsum(lens[:nh])]).astype(np.int64)
            out_rows = np.concatenate([[0], np.cumsum(plen[:nh])]).astype(np.int64)
            hout = np.empty((max(int(out_rows[-1]), 1), dim), np.float32)
            t = time.perf_counter()
            rc = host.pool_host(api._ptr(x), api._ptr(in_rows), api._ptr(out_rows), nh, dim, a.factor, 1, 0, a.threads,
                                api._ptr(hout))
            tot["host_wall"] += time.perf_counter() - t
            assert rc == 0, "the host run disagrees about a pooled length"
            n = int(out_rows[-1])
            if not np.array_equal(hout[:n].view(np.uint32), out[:n].view(np.uint32)):
                bad = np.nonzero((hout[:n].view(np.uint32) != out[:n].view(np.uint32)).any(1))[0]
                raise SystemExit(f"{name}: GPU and host results differ in {bad.size} rows of slab {s0}, first row {bad[0]}")
            tot["host_docs"] += nh
            tot["host_tokens"] += int(in_rows[-1])
    dev_s = (tot["ms_distances"] + tot["ms_linkage"] + tot["ms_means"]) * 1e-3
    line = dict(what="pool_documents", corpus=name, docs=tot["docs"], docs_pooled=tot["pooled"], dim=dim, pool_factor=a.factor,
                tokens_in=tot["tokens_in"], tokens_out=tot["tokens_out"], device_chunks=tot["chunks"],
                lds_max=os.environ.get("NP_POOL_LDS_MAX", "default"),
                ms_distances=round(tot["ms_distances"], 1), ms_linkage=round(tot["ms_linkage"], 1),
                ms_means=round(tot["ms_means"], 1), s_call_wall=round(tot["gpu_wall"], 3),
                docs_per_s_call=round(tot["docs"] / tot["gpu_wall"], 1), tokens_per_s_call=round(tot["tokens_in"] / tot["gpu_wall"], 1),
                docs_per_s_device=round(tot["docs"] / dev_s, 1), tokens_per_s_device=round(tot["tokens_in"] / dev_s, 1))
    if tot["host_docs"]:
        hd = tot["host_docs"] / tot["host_wall"]
        line.update(host_threads=a.threads, host_docs=tot["host_docs"], s_host_wall=round(tot["host_wall"], 3),
                    host_docs_per_s=round(hd, 1), host_tokens_per_s=round(tot["host_tokens"] / tot["host_wall"], 1),
                    results_equal=True,
                    gpu_call_over_host=round(tot["tokens_in"] / tot["gpu_wall"] / (tot["host_tokens"] / tot["host_wall"]), 2),
                    gpu_device_over_host=round(tot["tokens_in"] / dev_s / (tot["host_tokens"] / tot["host_wall"]), 2))
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--tokens", type=int, default=300)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--short-docs", type=int, default=1_000_000)
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--slab", type=int, default=20_000, help="documents generated and pooled per call")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-docs", type=int, default=0, help="documents of every slab the host run takes (0 = all, -1 = no host run)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_time.jsonl"))
    a = ap.parse_args()
    if npa.device_count() < 1:
        raise SystemExit("pool_time.py needs a gfx950 GPU")
    with tempfile.TemporaryDirectory(prefix="np_pool_") as tmp:
        host = None if a.host_docs < 0 else build_host(tmp)
        if a.docs > 0:
            run(f"long_{a.tokens}", np.full(a.docs, a.tokens, np.int64), a.dim, a, host)
        if a.short_docs > 0:
            tab = np.asarray(synth.lognormal_len_table(), np.int64)
            lens = tab[np.random.default_rng(3).integers(0, tab.size, a.short_docs)]
            run("short_lognormal", lens, a.dim, a, host)


if __name__ == "__main__":
    main()
