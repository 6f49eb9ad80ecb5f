#!/usr/bin/env python3
"""Times the metadata filters beside today's route to the same filtered search.

  timeout 900 python tools/filter_time.py          # writes profiles/filter_time.md and prints one JSON line per measurement

Corpus: the bench's synthetic generator in HBM (dim 128, --docs documents of 16-48 tokens, K = --k) with three synthetic
columns: u (I64, uniform in [0, 1000)), v (F64, standard normal, 5 % NULL) and tag (text, 64 distinct strings).  64 queries
of 32 tokens that all carry the same filter `u < ? AND v IS NOT NULL OR tag = ?`, whose first parameter sets the selectivity.
Per selectivity, wall-clock per call from Python (median of --repeats after --warmup untimed calls; the GPU steps synchronise
inside the call):
    filter_ids            MmapIndex.filter_ids: the ids on the device, copied to the host
    filter counts         ... counts_only=True: masks, popcounts and the scan, no ids
    search(filters=)      MmapIndex.search_batch(filters=...): the ids never leave HBM
    sqlite                today's route, part 1: stdlib sqlite3, SELECT id ... ORDER BY id over the same rows in an in-memory
                          table with the id as its primary key
    search(subsets=)      today's route, part 2: search_batch(subsets=[those ids]) -- the host-to-device copy of the list is
                          inside
Both routes return the same bytes (checked).  No ratio is asserted anywhere; the table is what was measured.  Run it under a
time limit, as above: every step that touches the GPU is one bounded call, and the tool stops at the first error.
"""
import argparse
import json
import os
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "next-plaid_amd"))

import next_plaid_amd as npa  # noqa: E402
from next_plaid_amd import synth  # noqa: E402


def median_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=65536)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--query-tokens", type=int, default=32)
    ap.add_argument("--selectivity", default="0.001,0.01,0.1,0.5,0.9")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_time.md"))
    a = ap.parse_args()
    if npa.device_count() < 1:
        raise SystemExit("filter_time.py needs a gfx950 GPU")
    dim = 128
    spec = synth.SynthSpec(num_docs=a.docs, num_centroids=a.k, dim=dim, nbits=a.nbits, doc_len_min=16, doc_len_max=48,
                           seed=1236, n_topics=8, rand256=51)
    cen = synth.centroids(spec)
    hx = npa.MmapIndex.synth(spec, centroids=cen, max_batch=a.queries, n_contexts=1)
    qs, _ = synth.make_queries(spec, a.queries, n_tokens=a.query_tokens, cen=cen)
    g = np.random.default_rng(7)
    u = g.integers(0, 1000, a.docs).astype(np.int64)
    v = g.standard_normal(a.docs)
    v[g.random(a.docs) < 0.05] = np.nan
    words = np.array([f"tag{i:02d}" for i in range(64)])
    tag = words[g.integers(0, 64, a.docs)]
    t0 = time.perf_counter()
    hx.set_columns({"u": u, "v": v, "tag": tag})
    ms_set = 1e3 * (time.perf_counter() - t0)
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, u INTEGER, v REAL, tag TEXT)")
    con.executemany("INSERT INTO t VALUES (?, ?, ?, ?)",
                    ((i, int(u[i]), None if v[i] != v[i] else float(v[i]), str(tag[i])) for i in range(a.docs)))
    cond = "u < ? AND v IS NOT NULL OR tag = ?"
    p = npa.SearchParameters(top_k=10, n_full_scores=4096, n_ivf_probe=8)
    rows = []
    for sel in [float(x) for x in a.selectivity.split(",")]:
        params = [int(round(sel * 1000 / 0.95)), "no such tag"]

        def sqlite_ids():
            return np.array([r[0] for r in con.execute(f"SELECT id FROM t WHERE {cond} ORDER BY id", params)], np.int64)

        ids = sqlite_ids()
        dev = hx.filter_ids([(cond, params)])[0]
        same_ids = bool(np.array_equal(ids, dev))
        f_res = hx.search_batch(qs, p, filters=[(cond, params)] * len(qs))
        ms_filter_stat = hx.last_stats["ms_total"]
        s_res = hx.search_batch(qs, p, subsets=[ids] * len(qs))
        ms_subset_stat = hx.last_stats["ms_total"]
        same = all(x.passage_ids.tobytes() == y.passage_ids.tobytes() and x.scores.tobytes() == y.scores.tobytes()
                   for x, y in zip(f_res, s_res))
        ms_ids = median_ms(lambda: hx.filter_ids([(cond, params)]), a.repeats, a.warmup)
        ms_cnt = median_ms(lambda: hx.filter_ids([(cond, params)], counts_only=True), a.repeats, a.warmup)
        ms_fs = median_ms(lambda: hx.search_batch(qs, p, filters=[(cond, params)] * len(qs)), a.repeats, a.warmup)
        ms_sql = median_ms(sqlite_ids, a.repeats, 1)
        ms_ss = median_ms(lambda: hx.search_batch(qs, p, subsets=[ids] * len(qs)), a.repeats, a.warmup)
        line = dict(what="filter", docs=a.docs, queries=a.queries, selectivity=sel, selected=int(ids.size),
                    ms_filter_ids=round(ms_ids, 3), ms_filter_counts=round(ms_cnt, 3), ms_search_filters=round(ms_fs, 3),
                    ms_sqlite=round(ms_sql, 3), ms_search_subsets=round(ms_ss, 3), ms_today=round(ms_sql + ms_ss, 3),
                    stats_ms_total_filters=round(ms_filter_stat, 3), stats_ms_total_subsets=round(ms_subset_stat, 3),
                    today_over_filters=round((ms_sql + ms_ss) / ms_fs, 2), same_ids_as_sqlite=same_ids, same_search_bytes=bool(same))
        rows.append(line)
        print(json.dumps(line), flush=True)
    hx.close()
    with open(a.out, "w") as f:
        f.write("# Metadata filters on the device beside SQLite + an id list (tools/filter_time.py)\n\n")
        f.write(f"Synthetic corpus in HBM: {a.docs} documents x 16-48 tokens, dim {dim}, {a.nbits}-bit residuals, K = {a.k}; columns "
                f"u (I64), v (F64, 5 % NULL), tag (text, 64 strings); set_columns took {ms_set:.1f} ms.  {a.queries} queries of "
                f"{a.query_tokens} tokens, one shared filter `{cond}`.  Wall-clock ms per call from Python, median of {a.repeats} "
                f"after {a.warmup} untimed calls.  today = sqlite + search(subsets=).\n\n")
        f.write("| selectivity | selected | filter_ids | filter counts | search(filters=) | sqlite | search(subsets=) | today | "
                "today / search(filters=) | same ids | same bytes |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['selectivity']} | {r['selected']} | {r['ms_filter_ids']} | {r['ms_filter_counts']} | {r['ms_search_filters']} | "
                    f"{r['ms_sqlite']} | {r['ms_search_subsets']} | {r['ms_today']} | {r['today_over_filters']} | "
                    f"{r['same_ids_as_sqlite']} | {r['same_search_bytes']} |\n")
        f.write("\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
