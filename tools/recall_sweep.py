#!/usr/bin/env python3
"""recall@10 and recall@100 of search_batch against the exact answer, search_exact(precision = 0), per search regime.

  python tools/recall_sweep.py                    # writes profiles/recall.md and prints one JSON line per regime

Corpus: the bench's synthetic generator in HBM (dim 128, K = --k, --docs documents of --doc-len tokens), once per nbits.
Queries: --queries of 32 tokens (noised tokens of a source document).  Ground truth: the exact top 100 of every query over
every document.  Regimes, the ones DESIGN.md section 4 lists: n_ivf_probe 8 / 32, centroid_score_threshold 0.4 / None,
n_full_scores 4096 / 8192, nbits 2 / 4; precision is the library default.  recall@k = |search top-k AND exact top-k| / k,
averaged over the queries (both lists are cut at k; a search that returns fewer than k documents loses the rest).
These are recorded, not asserted.
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


def recall(found, truth, k):
    return float(np.mean([np.isin(f.passage_ids[:k], t.passage_ids[:k]).sum() / min(k, max(t.passage_ids.size, 1))
                          for f, t in zip(found, truth)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=300_000)
    ap.add_argument("--doc-len", type=int, default=300)
    ap.add_argument("--k", type=int, default=65536)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--query-tokens", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recall.md"))
    a = ap.parse_args()
    if npa.device_count() < 1:
        raise SystemExit("recall_sweep.py needs a gfx950 GPU")
    lines = []
    for nbits in (2, 4):
        spec = synth.SynthSpec(num_docs=a.docs, num_centroids=a.k, dim=128, nbits=nbits, doc_len_min=a.doc_len, doc_len_max=a.doc_len,
                               seed=1236, n_topics=8, rand256=51)
        cen = synth.centroids(spec)
        hx = npa.MmapIndex.synth(spec, centroids=cen, max_batch=a.queries, n_contexts=1)
        qs, src = synth.make_queries(spec, a.queries, n_tokens=a.query_tokens, cen=cen)
        truth = hx.search_exact(qs, 100, 0)
        st = hx.last_stats
        exact_ms = st["ms_exact"] + st["ms_topk"]
        src_top = sum(int(t.passage_ids[0] == s) for t, s in zip(truth, src))
        for nprobe in (8, 32):
            for thr in (0.4, None):
                for nfs in (4096, 8192):
                    p = npa.SearchParameters(n_full_scores=nfs, top_k=100, n_ivf_probe=nprobe, centroid_score_threshold=thr)
                    found = hx.search_batch(qs, p)
                    s = hx.last_stats
                    line = dict(what="recall", docs=a.docs, doc_len=a.doc_len, k=a.k, nbits=nbits, queries=a.queries,
                                n_ivf_probe=nprobe, centroid_score_threshold=thr, n_full_scores=nfs, precision=p.precision,
                                recall_at_10=round(recall(found, truth, 10), 4), recall_at_100=round(recall(found, truth, 100), 4),
                                top1_agrees=sum(int(f.passage_ids.size > 0 and f.passage_ids[0] == t.passage_ids[0])
                                                for f, t in zip(found, truth)),
                                mean_returned=round(float(np.mean([f.passage_ids.size for f in found])), 1),
                                candidates_per_query=int(s["n_candidates"] // max(a.queries, 1)), search_ms=round(s["ms_total"], 3),
                                exact_ms=round(exact_ms, 1), source_is_exact_top1=src_top)
                    lines.append(line)
                    print(json.dumps(line), flush=True)
        hx.close()
    with open(a.out, "w") as f:
        f.write("# Recall of search_batch against the exact answer (tools/recall_sweep.py)\n\n")
        f.write(f"Synthetic corpus in HBM: {a.docs} documents x {a.doc_len} tokens, dim 128, K = {a.k}; {a.queries} queries of "
                f"{a.query_tokens} tokens.  Ground truth: search_exact(top_k = 100, precision = 0) over every document.  recall@k = "
                f"|search top-k AND exact top-k| / k, mean over the queries.  search ms = np_stats.ms_total of the batch; exact ms = "
                f"the scan and its selection for the same batch.  Recorded, not asserted.\n\n")
        f.write("| nbits | n_ivf_probe | threshold | n_full_scores | recall@10 | recall@100 | top-1 agrees | candidates / query | "
                "search ms | exact ms |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in lines:
            f.write(f"| {r['nbits']} | {r['n_ivf_probe']} | {r['centroid_score_threshold']} | {r['n_full_scores']} | {r['recall_at_10']:.4f} | "
                    f"{r['recall_at_100']:.4f} | {r['top1_agrees']}/{r['queries']} | {r['candidates_per_query']} | {r['search_ms']} | "
                    f"{r['exact_ms']} |\n")
        f.write("\n```\n" + "\n".join(json.dumps(l) for l in lines) + "\n```\n")


if __name__ == "__main__":
    main()
