#!/usr/bin/env python3
"""Times a batch of filtered requests, each with its own subset; one JSON line per (build, mode, share).

  python tools/subsets_time.py --ab ../parent-checkout      # the method of profiles/subsets_time.md: two builds, alternated
  python tools/subsets_time.py --mode sequential            # one build, one mode
  python tools/subsets_time.py --mode batched

`sequential` is 64 single-subset calls of one query each (the old interface; it touches nothing this interface added, so
--tree may name a built checkout of an earlier commit: its package and its library are the ones imported).  `batched` is one
call with subsets= (np_hip_search_batch_subsets).

--ab PARENT starts two workers that live for the whole measurement -- PARENT's build in sequential mode, this build in batched
mode (and a third, this build in sequential mode) -- lets each build its index and warm up, and then, per share and per
repeat, tells them to run ONE timed repeat each, one after the other: the builds alternate repeat by repeat on the same
device in the same minutes.  Per (worker, share): median, minimum and maximum of the repeats.

The index is the synthetic 1 M-document configuration of bench.py (K = 2^16, generated in HBM), the queries are 32 tokens
long and the parameters are SearchParameters() as it stands (the REST API's defaults).  Every query gets its own seeded
random subset of --shares of the documents (sorted ids, host arrays: the upload of the ids is part of both modes).  A timed
repeat starts and ends with hipDeviceSynchronize.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_synchronize():
    """hipDeviceSynchronize of the HIP runtime this process has loaded (the library's own: found in the process's maps, so no
    second runtime is ever opened)"""
    with open("/proc/self/maps") as f:
        paths = {l.split()[-1] for l in f if "libamdhip64" in l}
    if not paths:
        raise RuntimeError("no HIP runtime is loaded in this process")
    rc = ctypes.CDLL(sorted(paths)[0]).hipDeviceSynchronize()
    if rc != 0:
        raise RuntimeError(f"hipDeviceSynchronize returned {rc}")


class Workload:
    def __init__(self, a):
        sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "next-plaid_amd"))
        import next_plaid_amd as npa
        from next_plaid_amd import synth
        self.a = a
        spec = synth.SynthSpec(num_docs=a.docs, num_centroids=a.k, dim=128, nbits=4, doc_len_min=a.doc_len, doc_len_max=a.doc_len,
                               seed=1236, n_topics=8, rand256=51)
        cen = synth.centroids(spec)
        t0 = time.perf_counter()
        self.hx = npa.MmapIndex.synth(spec, centroids=cen, max_batch=a.queries, n_contexts=1)
        self.t_build = time.perf_counter() - t0
        self.qs, _ = synth.make_queries(spec, a.queries, n_tokens=a.query_tokens, cen=cen)
        self.p = npa.SearchParameters()
        self.subs = {}

    def subsets(self, share):
        if share not in self.subs:
            rng = np.random.default_rng(int(share * 1e6))
            n = max(1, int(round(share * self.a.docs)))
            self.subs[share] = [np.sort(rng.choice(self.a.docs, n, replace=False)).astype(np.int64) for _ in range(self.a.queries)]
        return self.subs[share]

    def run(self, share):
        subs = self.subsets(share)
        if self.a.mode == "batched":
            return self.hx.search_batch(self.qs, self.p, subsets=subs)
        return [self.hx.search_batch([q], self.p, subset=s)[0] for q, s in zip(self.qs, subs)]

    def warm(self, share):
        """untimed; also: every result lies in its subset and is not empty"""
        res = self.run(share)
        for r, s in zip(res, self.subsets(share)):
            assert r.passage_ids.size > 0 and np.all(np.isin(r.passage_ids, s))
        return [int(r.passage_ids[0]) for r in res[:4]]

    def timed(self, share):
        device_synchronize()
        t0 = time.perf_counter()
        self.run(share)
        device_synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def line(self, share, ms, first):
        a, med = self.a, float(np.median(ms))
        return dict(what="subsets", mode=a.mode, label=a.label, docs=a.docs, k=a.k, doc_len=a.doc_len, queries=a.queries,
                    query_tokens=a.query_tokens, share=share, subset_ids=len(self.subsets(share)[0]), repeats=len(ms),
                    ms=[round(x, 3) for x in ms], ms_median=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
                    queries_per_s=round(1e3 * a.queries / med, 1), index_build_s=round(self.t_build, 2), first_ids=first)


def worker(a):
    """Answers lines on stdin: `warm SHARE` -> first ids, `time SHARE` -> milliseconds of one repeat, `line SHARE` -> the JSON line."""
    w = Workload(a)
    ms, first = {}, {}
    print(json.dumps(dict(ready=True, index_build_s=round(w.t_build, 2))), flush=True)
    for cmd in sys.stdin:
        op, share = cmd.split()
        share = float(share)
        if op == "warm":
            first[share] = w.warm(share)
            print(json.dumps(dict(ok=True)), flush=True)
        elif op == "time":
            ms.setdefault(share, []).append(w.timed(share))
            print(json.dumps(dict(ms=ms[share][-1])), flush=True)
        elif op == "line":
            print(json.dumps(w.line(share, ms[share], first[share])), flush=True)
    w.hx.close()


def alternate(a, shares):
    common = ["--docs", str(a.docs), "--k", str(a.k), "--doc-len", str(a.doc_len), "--queries", str(a.queries),
              "--query-tokens", str(a.query_tokens), "--worker"]
    specs = [("parent", a.ab, "sequential"), ("this", a.tree, "batched"), ("this", a.tree, "sequential")]
    procs = []
    lines = []
    try:
        for label, tree, mode in specs:   # one after the other: the index builds do not compete
            pr = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--mode", mode, "--tree", tree, "--label", label] + common,
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            procs.append(pr)
            assert json.loads(pr.stdout.readline())["ready"]

        def ask(pr, cmd):
            pr.stdin.write(cmd + "\n")
            pr.stdin.flush()
            out = pr.stdout.readline()
            if not out:
                raise RuntimeError(f"a worker ended at '{cmd}' (exit {pr.poll()})")
            return json.loads(out)
        for share in shares:
            for pr in procs:
                ask(pr, f"warm {share}")
            for _ in range(a.repeats):
                for pr in procs:       # parent sequential, this batched, this sequential; then again
                    ask(pr, f"time {share}")
            for pr in procs:
                lines.append(ask(pr, f"line {share}"))
                print(json.dumps(lines[-1]), flush=True)
    finally:
        for pr in procs:
            pr.stdin.close()
        for pr in procs:
            pr.wait(timeout=60)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["sequential", "batched"])
    ap.add_argument("--ab", default=None, metavar="PARENT", help="a built checkout of the parent commit: alternate it with this build")
    ap.add_argument("--tree", default=HERE, help="repository checkout whose package and built library are timed (default: this one)")
    ap.add_argument("--label", default="", help="copied into every line (which build this is)")
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=65536)
    ap.add_argument("--doc-len", type=int, default=300)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--query-tokens", type=int, default=32)
    ap.add_argument("--shares", default="0.5,0.1,0.01", help="comma-separated subset sizes as shares of the documents")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    shares = [float(x) for x in a.shares.split(",")]
    if a.worker:
        return worker(a)
    if a.ab:
        lines = alternate(a, shares)
    else:
        if not a.mode:
            ap.error("--mode or --ab")
        w = Workload(a)
        lines = []
        for share in shares:
            first = w.warm(share)
            lines.append(w.line(share, [w.timed(share) for _ in range(a.repeats)], first))
            print(json.dumps(lines[-1]), flush=True)
        w.hx.close()
    if a.out:
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
