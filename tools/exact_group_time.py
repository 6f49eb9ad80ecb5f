#!/usr/bin/env python3
"""Times the exact grouped search beside the plain exact scan and beside the pooled grouped search.

  python tools/exact_group_time.py                # writes profiles/exact_group_time.md, prints one JSON line per measurement

Corpus: the bench's synthetic generator in HBM (dim 128, --docs documents of 16-48 tokens, K = --k); document d belongs to
group d // 20 (50 000 groups at 1 M documents).  --queries queries of 32 tokens, top_k = 10.  Routes, wall-clock per call from
Python; the runs ALTERNATE (e1, e3, x, g, e1, ...) after one untimed call of each and the table holds the medians:
    e1  search_exact_grouped(group_size = 1): the scan with every pass folded into the group table, the selection
    e3  search_exact_grouped(group_size = 3): ... and the members pass
    x   np_hip_search_exact(top_k = 10) WITHOUT a stats struct (with one the scan synchronises after every pass, which the
        grouped calls never do): the plain exact scan, pipelined as the grouped calls are
    g   search_grouped(pool_k = 200): the pooled grouped search (approximate: it ranks a pool)
With --parent-package and --parent-lib (the parent commit's Python package and library), np_hip_search_exact of this tree and of
the parent is timed -- the same stats-free call, at precision 0 and 3 -- in ALTERNATING rounds, every round a process of its
own (this file with --child); the table gets both medians and the parent's spread over its rounds.  No ratio is asserted anywhere; the table is what was measured.
"""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def median(xs):
    return sorted(xs)[len(xs) // 2]


def open_corpus(a):
    import numpy as np
    import next_plaid_amd as npa
    from next_plaid_amd import synth
    if npa.device_count() < 1:
        raise SystemExit("exact_group_time.py needs a gfx950 GPU")
    spec = synth.SynthSpec(num_docs=a.docs, num_centroids=a.k, dim=128, nbits=a.nbits, doc_len_min=16, doc_len_max=48,
                           seed=1236, n_topics=8, rand256=51)
    cen = synth.centroids(spec)
    hx = npa.MmapIndex.synth(spec, centroids=cen, max_batch=a.queries, n_contexts=1)
    qs, _ = synth.make_queries(spec, a.queries, n_tokens=a.query_tokens, cen=cen)
    return np, npa, hx, qs


def exact_raw(hx, qs, top_k, precision):
    """np_hip_search_exact with stats = NULL: nothing waits inside the call but its last copy"""
    from next_plaid_amd import api
    flat, off = hx._pack(qs)
    rows = api._ResultRows(len(qs), top_k)
    api._check(api.lib().np_hip_search_exact(hx._h, api._ptr(flat), api._ptr(off), len(qs), hx.embedding_dim(), top_k, precision,
                                             None, None, 0, None, *rows.ptrs(), None))
    return rows


def child(a):
    """One round of the stats-free np_hip_search_exact on whatever package and library this process was given."""
    np, npa, hx, qs = open_corpus(a)
    exact_raw(hx, qs, a.top_k, a.precision)
    ts = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        exact_raw(hx, qs, a.top_k, a.precision)
        ts.append(1e3 * (time.perf_counter() - t0))
    hx.close()
    print(json.dumps(dict(ms=round(median(ts), 3))), flush=True)


def round_of(a, package, lib, precision):
    env = dict(os.environ, PYTHONPATH=package)
    if lib:
        env["NEXTPLAID_HIP_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--docs", str(a.docs), "--k", str(a.k), "--nbits", str(a.nbits),
           "--queries", str(a.queries), "--query-tokens", str(a.query_tokens), "--top-k", str(a.top_k), "--repeats", str(a.repeats),
           "--precision", str(precision)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"a round failed ({out.returncode}): {out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])["ms"]


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
    ap.add_argument("--units", type=int, default=20, help="documents per group")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-package", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--commit", default=None, help="the commit the table is for (default: git's HEAD)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--precision", type=int, default=0, help="of a --child round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_group_time.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, os.path.join(ROOT, "next-plaid_amd"))
    np, npa, hx, qs = open_corpus(a)
    group_of = (np.arange(a.docs) // a.units).astype(np.int32)
    hx.set_groups(group_of, n_groups=int(group_of.max()) + 1)
    fns = {"e1": lambda: hx.search_exact_grouped(qs, a.top_k, 1), "e3": lambda: hx.search_exact_grouped(qs, a.top_k, 3),
           "x": lambda: exact_raw(hx, qs, a.top_k, 0),
           "g": lambda: hx.search_grouped(qs, npa.SearchParameters(top_k=a.top_k), group_size=3, pool_k=a.pool_k)}
    line = dict(what="exact_grouped", docs=a.docs, groups=int(group_of.max()) + 1, queries=a.queries, query_tokens=a.query_tokens,
                top_k=a.top_k, pool_k=a.pool_k, repeats=a.repeats, commit=a.commit or commit(), date=datetime.date.today().isoformat())
    exact, pooled = fns["e3"](), fns["g"]()
    line["pooled_group_recall"] = round(float(np.mean([len({g[0] for g in x} & {g[0] for g in y}) / max(len(x), 1)
                                                       for x, y in zip(exact, pooled)])), 4)
    for f in fns.values():
        f()                                                       # one untimed call of each
    ts = {r: [] for r in fns}
    for _ in range(a.repeats):                                    # alternating runs
        for r, f in fns.items():
            t0 = time.perf_counter()
            f()
            ts[r].append(1e3 * (time.perf_counter() - t0))
    for r in fns:
        line[f"ms_{r}"], line[f"ms_{r}_min"], line[f"ms_{r}_max"] = round(median(ts[r]), 3), round(min(ts[r]), 3), round(max(ts[r]), 3)
    T = hx.num_embeddings()
    hx.close()
    print(json.dumps(line), flush=True)
    rounds = None
    if a.parent_package and a.parent_lib:
        rounds = {f"{who}_p{pr}": [] for pr in (0, 3) for who in ("parent", "this")}
        for _ in range(a.rounds):                                 # alternating rounds, a process each
            for pr in (0, 3):
                rounds[f"parent_p{pr}"].append(round_of(a, a.parent_package, a.parent_lib, pr))
                rounds[f"this_p{pr}"].append(round_of(a, os.path.join(ROOT, "next-plaid_amd"), None, pr))
        print(json.dumps(dict(what="search_exact rounds", **rounds)), flush=True)
    with open(a.out, "w") as f:
        f.write("# Exact grouped search beside the exact scan and the pooled grouped search (tools/exact_group_time.py)\n\n")
        f.write(f"Recorded {line['date']} at commit {line['commit']}.  Synthetic corpus in HBM: {a.docs} documents x 16-48 tokens = {T} "
                f"tokens, dim 128, {a.nbits}-bit residuals, K = {a.k}; group of document d = d // {a.units} ({line['groups']} groups).  "
                f"{a.queries} queries of {a.query_tokens} tokens, top_k = {a.top_k}, precision 0.  Wall-clock ms per call from Python; "
                f"the routes alternate and each figure is the median of {a.repeats} runs after one untimed call (min .. max beside it).\n\n")
        f.write("| route | what | ms (median) | min .. max |\n|---|---|---|---|\n")
        what = {"e1": "search_exact_grouped(group_size = 1)", "e3": "search_exact_grouped(group_size = 3)",
                "x": f"np_hip_search_exact(top_k = {a.top_k}), no stats", "g": f"search_grouped(pool_k = {a.pool_k}, group_size = 3), approximate"}
        for r in fns:
            f.write(f"| {r} | {what[r]} | {line[f'ms_{r}']} | {line[f'ms_{r}_min']} .. {line[f'ms_{r}_max']} |\n")
        f.write(f"\nThe grouped call over the plain exact scan: {line['ms_e1'] / line['ms_x']:.3f} x at group_size 1, "
                f"{line['ms_e3'] / line['ms_x']:.3f} x at group_size 3; the members pass and its emit cost "
                f"{line['ms_e3'] - line['ms_e1']:.3f} ms of the latter.  Of the true top-{a.top_k} groups the pooled search finds "
                f"{100 * line['pooled_group_recall']:.2f} % on average.\n")
        if rounds:
            f.write(f"\nnp_hip_search_exact(top_k = {a.top_k}, no stats) of this tree and of the parent commit, {a.rounds} alternating "
                    f"rounds, a process each, median of {a.repeats} calls per round:\n\n| precision | library | median of rounds, ms | "
                    f"rounds |\n|---|---|---|---|\n")
            for pr in (0, 3):
                p, t = rounds[f"parent_p{pr}"], rounds[f"this_p{pr}"]
                f.write(f"| {pr} | parent | {median(p)} | {p} (spread {max(p) - min(p):.3f}) |\n| {pr} | this tree | {median(t)} | {t} |\n")
        f.write("\n```\n" + json.dumps(line) + ("\n" + json.dumps(rounds) if rounds else "") + "\n```\n")


if __name__ == "__main__":
    main()
