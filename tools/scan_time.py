#!/usr/bin/env python3
"""Times np_hip_search_exact (the document-major exact scan) and sets it beside the per-pair cost of the existing S6 form.

  python tools/scan_time.py                       # writes profiles/scan_time.md and prints one JSON line per measurement

Corpus: the bench's synthetic generator in HBM (dim 128, --docs documents of --doc-len tokens, K = --k).  Queries: 64 of 32
tokens.  Per precision (0 = exact-f32 MFMA, 3 = bf16 MFMA) and per "scan_tiles" in 1 / 2 / 4 / 8 (32-token query tiles a
workgroup stages: with 32-token queries that is the number of queries a decompressed tile is scored against):
    ms per batch (np_stats.ms_exact, the scan kernel alone, and ms_topk, selection; median of --repeats),
    algorithmic flops 2 * sum(Lq) * dim * T per second as a fraction of the MFMA peak of that precision,
    residual bytes streamed per second (T * pd per query GROUP: every group reads the index once).
The comparison the kernel is justified by: in the same run, search_batch at n_full_scores = 65536 (every query exact-scores
its 16384 best candidates in the per-(query, document) S6 form of the same precision) gives
    np_stats.ms_exact / n_exact_docs        the per-pair cost of the existing form
beside
    scan ms / (queries * documents)         the per-pair cost of the scan.
No time is asserted anywhere; the table is what was measured.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "next-plaid_amd"))

import next_plaid_amd as npa  # noqa: E402
from next_plaid_amd import synth  # noqa: E402

PEAK_TF = {0: 157.3, 3: 2500.0}   # exact-f32 MFMA (v_mfma_f32_32x32x2_f32) and dense bf16 MFMA, as bench.py states them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--doc-len", type=int, default=300)
    ap.add_argument("--k", type=int, default=65536)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--query-tokens", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tiles", default="1,2,4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_time.md"))
    a = ap.parse_args()
    if npa.device_count() < 1:
        raise SystemExit("scan_time.py needs a gfx950 GPU")
    dim = 128
    spec = synth.SynthSpec(num_docs=a.docs, num_centroids=a.k, dim=dim, nbits=a.nbits, doc_len_min=a.doc_len, doc_len_max=a.doc_len,
                           seed=1236, n_topics=8, rand256=51)
    cen = synth.centroids(spec)
    hx = npa.MmapIndex.synth(spec, centroids=cen, max_batch=a.queries, n_contexts=1)
    qs, src = synth.make_queries(spec, a.queries, n_tokens=a.query_tokens, cen=cen)
    T = hx.num_embeddings()
    pd = dim * a.nbits // 8
    sum_lq = sum(q.shape[0] for q in qs)
    flops = 2.0 * sum_lq * dim * T
    rows, lines = [], []
    for prec in (0, 3):
        # the existing form: per-(query, document) S6 over each query's 16384 best candidates
        p = npa.SearchParameters(n_full_scores=65536, top_k=a.top_k, n_ivf_probe=32, centroid_score_threshold=None, precision=prec)
        hx.search_batch(qs, p)
        s6 = []
        for _ in range(a.repeats):
            hx.search_batch(qs, p)
            st = hx.last_stats
            s6.append((st["ms_exact"], st["n_exact_docs"], st["n_exact_tokens"]))
        s6_ms, s6_docs, s6_toks = sorted(s6)[len(s6) // 2]
        s6_pair_ns = 1e6 * s6_ms / max(s6_docs, 1)
        lines.append(dict(what="s6_per_pair", precision=prec, ms_exact=round(s6_ms, 3), n_exact_docs=int(s6_docs),
                          n_exact_tokens=int(s6_toks), ns_per_pair=round(s6_pair_ns, 2)))
        print(json.dumps(lines[-1]), flush=True)
        for tiles in [int(x) for x in a.tiles.split(",")]:
            hx.tune("scan_tiles", tiles)
            res = hx.search_exact(qs, a.top_k, prec)   # untimed
            hit = sum(int(r.passage_ids[0] == s) for r, s in zip(res, src))
            ms = []
            for _ in range(a.repeats):
                hx.search_exact(qs, a.top_k, prec)
                st = hx.last_stats
                ms.append((st["ms_exact"], st["ms_topk"], st["n_exact_docs"], st["n_exact_tokens"]))
            ms_scan, ms_topk, pairs, toks = sorted(ms)[len(ms) // 2]
            groups = toks / max(T, 1)
            line = dict(what="scan", precision=prec, scan_tiles=tiles, docs=a.docs, tokens=int(T), queries=a.queries,
                        query_tokens=a.query_tokens, ms_scan=round(ms_scan, 3), ms_topk=round(ms_topk, 3),
                        tflops=round(flops / ms_scan * 1e-9, 2), peak_fraction=round(flops / ms_scan * 1e-9 / PEAK_TF[prec], 4),
                        residual_gb_s=round(toks * pd / ms_scan * 1e-6, 1), index_passes=round(groups, 2),
                        ns_per_pair=round(1e6 * ms_scan / max(pairs, 1), 3), s6_ns_per_pair=round(s6_pair_ns, 2),
                        s6_over_scan=round(s6_pair_ns / (1e6 * ms_scan / max(pairs, 1)), 2), source_is_top_hit=f"{hit}/{len(qs)}")
            lines.append(line)
            rows.append(line)
            print(json.dumps(line), flush=True)
    hx.tune("scan_tiles", 8)
    hx.close()
    with open(a.out, "w") as f:
        f.write("# np_hip_search_exact: the document-major scan, timed (tools/scan_time.py)\n\n")
        f.write(f"Synthetic corpus in HBM: {a.docs} documents x {a.doc_len} tokens = {T} tokens, dim {dim}, {a.nbits}-bit residuals "
                f"({pd} bytes per token), K = {a.k}.  {a.queries} queries of {a.query_tokens} tokens.  Median of {a.repeats} timed "
                f"calls after one untimed; ms scan = np_stats.ms_exact (the scan kernel), ms top-k = selection.  Flops = "
                f"2 x {sum_lq} x {dim} x T.  Peaks: f32 MFMA {PEAK_TF[0]} TF, bf16 MFMA {PEAK_TF[3]} TF.  S6 per pair = "
                f"search_batch(n_full_scores = 65536, no threshold, nprobe 32): np_stats.ms_exact / n_exact_docs at the same precision.\n\n")
        f.write("| precision | scan_tiles | index passes | ms scan | ms top-k | TF/s | of MFMA peak | residual GB/s | scan ns / pair | "
                "S6 ns / pair | S6 / scan |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['precision']} | {r['scan_tiles']} | {r['index_passes']} | {r['ms_scan']} | {r['ms_topk']} | {r['tflops']} | "
                    f"{100 * r['peak_fraction']:.1f} % | {r['residual_gb_s']} | {r['ns_per_pair']} | {r['s6_ns_per_pair']} | "
                    f"{r['s6_over_scan']} |\n")
        f.write("\n```\n" + "\n".join(json.dumps(l) for l in lines) + "\n```\n")


if __name__ == "__main__":
    main()
