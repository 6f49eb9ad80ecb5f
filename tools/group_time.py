#!/usr/bin/env python3
"""Times grouped search beside the way to the same groups that exists without it.

  python tools/group_time.py                      # writes profiles/group_time.md and prints one JSON line per measurement

Corpus: the bench's synthetic generator in HBM (dim 128, --docs documents of 16-48 tokens, K = --k); document d belongs to
group d // 8 (eight units per file).  --queries queries of 32 tokens, top_k = 10 groups, group_size = 1.  Routes, wall-clock per
call from Python; the runs ALTERNATE (a, b, c, a, b, c, ...) after one untimed call of each and the table holds the medians:
    a   search_grouped(pool_k = 200): the pass with top_k = 200 and the collapse on the device; 10 groups come back
    b   ColGREP's way on the same build: search_batch(top_k = 200), the 200 results to the host, the walk of
        tests/collapse_restate.py over a host array of group ids
    c   search_batch(top_k = 10): what the pass costs without a pool
    d   collapse_kernel alone at strides 256, 1024 and 16384 (np_hip_collapse_device on resident lists, between two events on
        the call's stream), median of --kernel-repeats launches
--routes picks a subset (c alone runs on a build without the grouped entries).  a and b are checked to return the same groups.
No ratio is asserted anywhere; the table is what was measured.
"""
import argparse
import ctypes as C
import datetime
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "next-plaid_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import next_plaid_amd as npa  # noqa: E402
from next_plaid_amd import api, synth  # noqa: E402


def median(xs):
    return sorted(xs)[len(xs) // 2]


class Hip:
    """The HIP runtime this process has already loaded (the library's own): buffers, a stream and events."""

    def __init__(self):
        with open("/proc/self/maps") as f:
            paths = sorted({l.split()[-1] for l in f if "libamdhip64" in l})
        self.h = C.CDLL(paths[0])
        self.h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.h.hipFree.argtypes = [C.c_void_p]
        self.h.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.h.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.h.hipStreamDestroy.argtypes = [C.c_void_p]
        self.h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.h.hipEventDestroy.argtypes = [C.c_void_p]
        self.ptrs = []

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(f"HIP call failed with {rc}")

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        self.ok(self.h.hipMalloc(C.byref(p), max(a.nbytes, 8)))
        self.ptrs.append(p)
        self.ok(self.h.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1))
        return p

    def free(self):
        for p in self.ptrs:
            self.h.hipFree(p)
        self.ptrs = []


def kernel_ms(hx, hip, group_of, stride, B, top_k, group_size, repeats, rng):
    """collapse_kernel on B resident lists of `stride` random documents, between two events on one stream."""
    ids = rng.integers(0, group_of.size, (B, stride)).astype(np.int64)
    sc = -np.sort(-rng.standard_normal((B, stride)).astype(np.float32), axis=1)
    cnt = np.full(B, stride, np.int32)
    d_in = [hip.put(x) for x in (ids, sc, cnt)]
    n, g = B * top_k * group_size, B * top_k
    d_out = [hip.put(np.zeros(n, np.int64)), hip.put(np.zeros(n, np.float32))] + [hip.put(np.zeros(g, np.int32)) for _ in range(3)] + \
            [hip.put(np.zeros(B, np.int32))]
    st, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    hip.ok(hip.h.hipStreamCreate(C.byref(st)))
    hip.ok(hip.h.hipEventCreate(C.byref(e0)))
    hip.ok(hip.h.hipEventCreate(C.byref(e1)))
    ts = []
    for i in range(repeats + 1):
        hip.ok(hip.h.hipEventRecord(e0, st))
        api._check(api.lib().np_hip_collapse_device(hx._h, top_k, group_size, B, d_in[0], d_in[1], d_in[2], stride, *d_out, st))
        hip.ok(hip.h.hipEventRecord(e1, st))
        hip.ok(hip.h.hipStreamSynchronize(st))
        ms = C.c_float()
        hip.ok(hip.h.hipEventElapsedTime(C.byref(ms), e0, e1))
        if i:
            ts.append(ms.value)
    hip.h.hipEventDestroy(e0)
    hip.h.hipEventDestroy(e1)
    hip.h.hipStreamDestroy(st)
    hip.free()
    return median(ts)


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=65536)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--query-tokens", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--pool-k", type=int, default=200)
    ap.add_argument("--group-size", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--kernel-repeats", type=int, default=21)
    ap.add_argument("--routes", default="a,b,c,d")
    ap.add_argument("--commit", default=None, help="the commit the table is for (default: git's HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_time.md"))
    a = ap.parse_args()
    routes = [r for r in a.routes.split(",") if r]
    if npa.device_count() < 1:
        raise SystemExit("group_time.py needs a gfx950 GPU")
    dim = 128
    spec = synth.SynthSpec(num_docs=a.docs, num_centroids=a.k, dim=dim, nbits=a.nbits, doc_len_min=16, doc_len_max=48,
                           seed=1236, n_topics=8, rand256=51)
    cen = synth.centroids(spec)
    hx = npa.MmapIndex.synth(spec, centroids=cen, max_batch=a.queries, n_contexts=1)
    qs, _ = synth.make_queries(spec, a.queries, n_tokens=a.query_tokens, cen=cen)
    group_of = (np.arange(a.docs) // 8).astype(np.int32)
    P = npa.SearchParameters
    p_top = P(top_k=a.top_k)
    p_pool = P(top_k=a.pool_k)
    fns = {}
    if "a" in routes or "b" in routes or "d" in routes:
        import collapse_restate as R
        hx.set_groups(group_of, n_groups=int(group_of.max()) + 1)
        fns["a"] = lambda: hx.search_grouped(qs, p_top, group_size=a.group_size, pool_k=a.pool_k)
        fns["b"] = lambda: [R.walk(r.passage_ids, r.scores, group_of, a.top_k, a.group_size) for r in hx.search_batch(qs, p_pool)]
    fns["c"] = lambda: hx.search_batch(qs, p_top)
    timed = [r for r in ("a", "b", "c") if r in routes]
    line = dict(what="grouped", docs=a.docs, queries=a.queries, query_tokens=a.query_tokens, top_k=a.top_k, pool_k=a.pool_k,
                group_size=a.group_size, repeats=a.repeats, commit=a.commit or commit(), date=datetime.date.today().isoformat())
    if "a" in timed and "b" in timed:
        ga, gb = fns["a"](), fns["b"]()
        line["a_equals_b"] = bool(all(R.listed(x) == R.walked(y) for x, y in zip(ga, gb)))
        line["groups_per_query"] = round(float(np.mean([len(x) for x in ga])), 2)
        line["folded_per_query"] = round(float(np.mean([sum(g[3] - len(g[1]) for g in x) for x in ga])), 2)
    for r in timed:
        fns[r]()                                                   # one untimed call of each
    ts = {r: [] for r in timed}
    for _ in range(a.repeats):                                    # alternating runs
        for r in timed:
            t0 = time.perf_counter()
            fns[r]()
            ts[r].append(1e3 * (time.perf_counter() - t0))
    for r in timed:
        line[f"ms_{r}"] = round(median(ts[r]), 3)
        line[f"ms_{r}_min"] = round(min(ts[r]), 3)
        line[f"ms_{r}_max"] = round(max(ts[r]), 3)
    print(json.dumps(line), flush=True)
    kern = []
    if "d" in routes:
        hip = Hip()
        rng = np.random.default_rng(7)
        for stride in (256, 1024, 16384):
            ms = kernel_ms(hx, hip, group_of, stride, a.queries, a.top_k, a.group_size, a.kernel_repeats, rng)
            kern.append(dict(what="collapse_kernel", stride=stride, lists=a.queries, top_k=a.top_k, group_size=a.group_size,
                             ms=round(ms, 4), us_per_list=round(1e3 * ms / a.queries, 3)))
            print(json.dumps(kern[-1]), flush=True)
    T = hx.num_embeddings()
    hx.close()
    with open(a.out, "w") as f:
        f.write("# Grouped search beside the over-fetch it replaces (tools/group_time.py)\n\n")
        f.write(f"Recorded {line['date']} at commit {line['commit']}.  Synthetic corpus in HBM: {a.docs} documents x 16-48 tokens = {T} "
                f"tokens, dim {dim}, {a.nbits}-bit residuals, K = {a.k}; group of document d = d // 8.  {a.queries} queries of "
                f"{a.query_tokens} tokens, top_k = {a.top_k} groups, group_size = {a.group_size}, default search parameters otherwise.  "
                f"Wall-clock ms per call from Python; the routes alternate and each figure is the median of {a.repeats} runs after one "
                f"untimed call (min .. max beside it).\n\n")
        f.write("| route | what | ms (median) | min .. max |\n|---|---|---|---|\n")
        what = {"a": f"search_grouped(pool_k = {a.pool_k})",
                "b": f"search_batch(top_k = {a.pool_k}) + the walk on the host",
                "c": f"search_batch(top_k = {a.top_k})"}
        for r in timed:
            f.write(f"| {r} | {what[r]} | {line[f'ms_{r}']} | {line[f'ms_{r}_min']} .. {line[f'ms_{r}_max']} |\n")
        if "a_equals_b" in line:
            f.write(f"\na and b return the same groups: {line['a_equals_b']}; {line['groups_per_query']} groups and "
                    f"{line['folded_per_query']} folded entries per query on average.\n")
        if kern:
            f.write(f"\ncollapse_kernel alone, {a.queries} resident lists of random documents per launch, between two events on the "
                    f"call's stream, median of {a.kernel_repeats} launches:\n\n| stride | ms per launch | us per list |\n|---|---|---|\n")
            for k in kern:
                f.write(f"| {k['stride']} | {k['ms']} | {k['us_per_list']} |\n")
        f.write("\n```\n" + "\n".join(json.dumps(r) for r in [line] + kern) + "\n```\n")


if __name__ == "__main__":
    main()
