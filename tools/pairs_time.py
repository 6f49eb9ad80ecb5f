#!/usr/bin/env python3
"""Times np_hip_score_pairs beside the two routes to the same numbers that exist without it.

  python tools/pairs_time.py                      # writes profiles/pairs_time.md and prints one JSON line per measurement

Corpus: the bench's synthetic generator in HBM (dim 128, --docs documents of 16-48 tokens, K = --k).  64 queries of 32 tokens,
each scored against --pairs (10 and 1000) random documents.  Three routes, wall-clock per call (median of --repeats after one
untimed call), all of them returning the exact f32 MaxSim of the same pairs:
    score_pairs     MmapIndex.score_pairs with the per-token rows, and with return_matches=False
    search_exact    MmapIndex.search_exact(subsets = the pair lists, top_k = n): the scan tests every document block of the
                    shard against the subset bitmaps, selects and sorts; it returns only the sums
    decompress      MmapIndex.decompress_documents to the host and a numpy MaxSim there (per query)
and the rate of score_pairs in document tokens decompressed per second (np_stats.n_exact_tokens / wall time).
No ratio is asserted anywhere; the table is what was measured.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "next-plaid_amd"))

import next_plaid_amd as npa  # noqa: E402
from next_plaid_amd import synth  # noqa: E402


def median_ms(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return sorted(ts)[len(ts) // 2]


def host_maxsim(hx, qs, ids):
    out = []
    for q, d in zip(qs, ids):
        emb, lens = hx.decompress_documents(d)
        S = q @ emb.T
        S = np.where(np.isfinite(S), S, -np.inf)
        off = np.concatenate([[0], np.cumsum(lens)])[:-1]
        M = np.maximum.reduceat(S, off, axis=1)
        out.append(np.where(M > -np.inf, M, 0).sum(0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=65536)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--query-tokens", type=int, default=32)
    ap.add_argument("--pairs", default="10,1000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_time.md"))
    a = ap.parse_args()
    if npa.device_count() < 1:
        raise SystemExit("pairs_time.py needs a gfx950 GPU")
    dim = 128
    spec = synth.SynthSpec(num_docs=a.docs, num_centroids=a.k, dim=dim, nbits=a.nbits, doc_len_min=16, doc_len_max=48,
                           seed=1236, n_topics=8, rand256=51)
    cen = synth.centroids(spec)
    hx = npa.MmapIndex.synth(spec, centroids=cen, max_batch=a.queries, n_contexts=1)
    qs, _ = synth.make_queries(spec, a.queries, n_tokens=a.query_tokens, cen=cen)
    g = np.random.default_rng(7)
    rows = []
    for n in [int(x) for x in a.pairs.split(",")]:
        ids = [np.sort(g.choice(a.docs, n, replace=False)).astype(np.int64) for _ in qs]   # distinct: search_exact counts an id once
        got = hx.score_pairs(qs, ids)
        st = dict(hx.last_stats)
        exact = hx.search_exact(qs, n, 0, subsets=ids)
        agree = all(np.array_equal(np.sort(s.view(np.uint32)), np.sort(r.scores.view(np.uint32))) for (s, _, _), r in zip(got, exact))
        host = host_maxsim(hx, qs, ids)
        close = max(float(np.max(np.abs(h - s) / np.maximum(np.abs(s), 1))) for h, (s, _, _) in zip(host, got))
        ms_pairs = median_ms(lambda: hx.score_pairs(qs, ids), a.repeats)
        ms_scores = median_ms(lambda: hx.score_pairs(qs, ids, return_matches=False), a.repeats)
        hx.score_pairs(qs, ids)
        ms_kernel = hx.last_stats["ms_exact"]
        ms_exact = median_ms(lambda: hx.search_exact(qs, n, 0, subsets=ids), a.repeats)
        ms_host = median_ms(lambda: host_maxsim(hx, qs, ids), a.repeats)
        line = dict(what="pairs", docs=a.docs, queries=a.queries, query_tokens=a.query_tokens, pairs_per_query=n,
                    ms_score_pairs=round(ms_pairs, 3), ms_score_pairs_scores_only=round(ms_scores, 3),
                    ms_score_pairs_kernel=round(ms_kernel, 3), ms_search_exact_subsets=round(ms_exact, 3),
                    ms_decompress_numpy=round(ms_host, 3), n_exact_tokens=int(st["n_exact_tokens"]),
                    mtokens_per_s=round(st["n_exact_tokens"] / ms_pairs * 1e-3, 1),
                    search_exact_over_pairs=round(ms_exact / ms_pairs, 2), decompress_over_pairs=round(ms_host / ms_pairs, 2),
                    same_bits_as_search_exact=bool(agree), host_max_rel_diff=float(f"{close:.2e}"))
        rows.append(line)
        print(json.dumps(line), flush=True)
    T = hx.num_embeddings()
    hx.close()
    with open(a.out, "w") as f:
        f.write("# np_hip_score_pairs beside the routes that existed before it (tools/pairs_time.py)\n\n")
        f.write(f"Synthetic corpus in HBM: {a.docs} documents x 16-48 tokens = {T} tokens, dim {dim}, {a.nbits}-bit residuals, "
                f"K = {a.k}.  {a.queries} queries of {a.query_tokens} tokens, each against n random documents.  Wall-clock ms per "
                f"call from Python, median of {a.repeats} after one untimed call; kernel = np_stats.ms_exact of one call.  "
                f"search_exact = one subset per query, top_k = n; decompress = decompress_documents + numpy MaxSim per query.\n\n")
        f.write("| n per query | score_pairs | ... scores only | ... kernel | search_exact | decompress + numpy | doc tokens | "
                "Mtokens/s | search_exact / score_pairs | decompress / score_pairs |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['pairs_per_query']} | {r['ms_score_pairs']} | {r['ms_score_pairs_scores_only']} | "
                    f"{r['ms_score_pairs_kernel']} | {r['ms_search_exact_subsets']} | {r['ms_decompress_numpy']} | "
                    f"{r['n_exact_tokens']} | {r['mtokens_per_s']} | {r['search_exact_over_pairs']} | {r['decompress_over_pairs']} |\n")
        slower = [r for r in rows if r["search_exact_over_pairs"] < 1 or r["decompress_over_pairs"] < 1]
        f.write("\n" + ("score_pairs is faster than both routes at every size measured.\n" if not slower else
                        "score_pairs is NOT faster than both routes at n = " + ", ".join(str(r["pairs_per_query"]) for r in slower) + ".\n"))
        f.write("\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
