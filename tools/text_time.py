#!/usr/bin/env python3
"""Times the keyword search and the hybrid request on the device beside SQLite FTS5 + host fusion on the same corpus.

  timeout 1100 python tools/text_time.py          # writes profiles/text_time.md and prints one JSON line per measurement

Corpus: the bench's synthetic generator in HBM (dim 128, --docs documents of 16-48 tokens, K = --k) and, for the same
documents, texts of 4-28 words over a Zipf vocabulary of --vocab words in an in-memory FTS5 table (unicode61) that Python's
sqlite3 builds.  The bench's own document count (10 M) is out of reach of that build -- every (term, document, position) row
passes through Python once -- so the default is the largest that builds in about a minute; the table states the count.
--queries keyword queries per kind, each paired with a semantic query of --query-tokens tokens:
    1 word / 3 words AND / 3 words OR / a 2-word phrase          words drawn by rank from the head, the middle and the tail
Per kind, wall-clock per call from Python (median of --repeats after --warmup untimed calls; every device call ends in a
synchronise inside the library):
    text_search           MmapIndex.text_search, the whole batch in one call, top_k = --fetch-k
    search_hybrid         MmapIndex.search_hybrid: semantic pass + keyword pass + fusion, nothing leaves HBM in between
    sqlite                text_search.rs's statement, once per query (as the handler runs it), on the host
    search_batch          the semantic pass alone with top_k = --fetch-k
    host fusion           the reference's fuse_relative_score restated in numpy-free Python (dict + sort), per query
    today                 sqlite + search_batch + host fusion
The device's keyword results are compared with SQLite's (ids where scores are distinct, scores as f32 bits).  No ratio is
asserted anywhere; the table is what was measured.  Run it under a time limit, as above: every step that touches the GPU is
one bounded call, and the tool stops at the first error.
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
from next_plaid_amd import synth, text as T  # noqa: E402


def median_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return sorted(ts)[len(ts) // 2]


def host_fuse_relative(sem_ids, sem_sc, kw_ids, kw_sc, alpha, top_k):
    """fuse_relative_score as a host would run it (text_search.rs:1040-1075): a dict and a sort."""
    def norm(ids, sc):
        if not len(sc):
            return []
        lo, hi = min(sc), max(sc)
        return [(i, 1.0) for i in ids] if hi == lo else [(i, (s - lo) / (hi - lo)) for i, s in zip(ids, sc)]
    fused = {}
    for i, s in norm(sem_ids, sem_sc):
        fused[i] = fused.get(i, 0.0) + alpha * s
    for i, s in norm(kw_ids, kw_sc):
        fused[i] = fused.get(i, 0.0) + (1.0 - alpha) * s
    return sorted(fused.items(), key=lambda kv: -kv[1])[:top_k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=300_000)
    ap.add_argument("--k", type=int, default=16384)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--query-tokens", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--fetch-k", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_time.md"))
    a = ap.parse_args()
    if npa.device_count() < 1:
        raise SystemExit("text_time.py needs a gfx950 GPU")
    dim = 128
    spec = synth.SynthSpec(num_docs=a.docs, num_centroids=a.k, dim=dim, nbits=a.nbits, doc_len_min=16, doc_len_max=48,
                           seed=1236, n_topics=8, rand256=51)
    cen = synth.centroids(spec)
    hx = npa.MmapIndex.synth(spec, centroids=cen, max_batch=a.queries, n_contexts=1)
    qs, _ = synth.make_queries(spec, a.queries, n_tokens=a.query_tokens, cen=cen)
    qs = list(qs)
    # the texts: Zipf ranks, 4-28 words per document
    g = np.random.default_rng(11)
    lens = g.integers(4, 29, a.docs)
    pr = 1.0 / np.arange(1, a.vocab + 1)
    toks = g.choice(a.vocab, int(lens.sum()), p=pr / pr.sum())
    words = np.array([f"w{i}" for i in range(a.vocab)])
    cuts = np.cumsum(lens)[:-1]
    t0 = time.perf_counter()
    con = sqlite3.connect(":memory:")
    T.create_fts_tables(con, "unicode61", content_synced=False)
    T.insert_fts_rows(con, (" ".join(w) for w in np.split(words[toks], cuts)), range(a.docs), "unicode61", content_synced=False)
    s_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    data = T.TextIndexData._read(con, T.FTS_TABLE, "unicode61")
    s_read = time.perf_counter() - t0
    t0 = time.perf_counter()
    hx.set_text(data)
    ms_set = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(dict(what="corpus", docs=a.docs, instances=int(data.inst_doc.size), terms=data.n_terms,
                          s_sqlite_build=round(s_build, 1), s_read_instances=round(s_read, 1), ms_set_text=round(ms_set, 1))), flush=True)
    sql = (f'SELECT rowid, CAST(-bm25("{T.FTS_TABLE}") AS REAL) AS score FROM "{T.FTS_TABLE}" WHERE "{T.FTS_TABLE}" MATCH ? '
           "ORDER BY score DESC LIMIT ?")
    rank = lambda: int(g.choice([g.integers(0, 20), g.integers(20, 500), g.integers(500, a.vocab)]))
    kinds = {"1 word": lambda: f'"w{rank()}"',
             "3 words AND": lambda: " ".join(f'"w{rank()}"' for _ in range(3)),
             "3 words OR": lambda: " OR ".join(f'"w{rank()}"' for _ in range(3)),
             "2-word phrase": lambda: f'"w{g.integers(0, 30)} w{g.integers(0, 30)}"'}
    p = npa.SearchParameters(top_k=a.top_k, n_full_scores=4096, n_ivf_probe=8)
    pf = npa.SearchParameters(top_k=a.fetch_k, n_full_scores=4096, n_ivf_probe=8)
    rows = []
    for kind, make in kinds.items():
        strings = [make() for _ in range(a.queries)]
        compiled = [T.compile_text_query(s, data) for s in strings]

        def sqlite_all():
            return [con.execute(sql, (s, a.fetch_k)).fetchall() for s in strings]

        want = sqlite_all()
        got = hx.text_search(compiled, a.fetch_k)
        postings = hx.last_stats["n_ivf_ids"]
        same = True
        for w, r in zip(want, got):
            w = sorted(w, key=lambda x: (-x[1], x[0]))
            same = same and np.array_equal(np.asarray([x[1] for x in w], np.float64).astype(np.float32).view(np.uint32),
                                           r.scores.view(np.uint32))
            safe = sum(x[1] > w[-1][1] for x in w) if len(w) == a.fetch_k else len(w)   # a cut inside equal scores: SQLite's choice
            same = same and [x[0] for x in w[:safe]] == r.passage_ids[:safe].tolist()
        sem = hx.search_batch(qs, pf)

        def fuse_all():
            return [host_fuse_relative(s.passage_ids.tolist(), s.scores.tolist(), [x[0] for x in w], [x[1] for x in w], 0.75, a.top_k)
                    for s, w in zip(sem, want)]

        ms_text = median_ms(lambda: hx.text_search(compiled, a.fetch_k), a.repeats, a.warmup)
        ms_hyb = median_ms(lambda: hx.search_hybrid(qs, compiled, p, fetch_k=a.fetch_k), a.repeats, a.warmup)
        ms_sem = median_ms(lambda: hx.search_batch(qs, pf), a.repeats, a.warmup)
        ms_sql = median_ms(sqlite_all, max(a.repeats // 2, 1), 1)
        ms_fuse = median_ms(fuse_all, a.repeats, 1)
        line = dict(what="text", kind=kind, docs=a.docs, queries=a.queries, fetch_k=a.fetch_k, matches=int(sum(len(w) for w in want)),
                    postings_visited=int(postings), ms_text_search=round(ms_text, 3), ms_search_hybrid=round(ms_hyb, 3),
                    ms_sqlite=round(ms_sql, 3), ms_search_batch=round(ms_sem, 3), ms_host_fusion=round(ms_fuse, 3),
                    ms_today=round(ms_sql + ms_sem + ms_fuse, 3), sqlite_over_text_search=round(ms_sql / ms_text, 2),
                    today_over_hybrid=round((ms_sql + ms_sem + ms_fuse) / ms_hyb, 2), same_as_sqlite=bool(same))
        rows.append(line)
        print(json.dumps(line), flush=True)
    hx.close()
    with open(a.out, "w") as f:
        f.write("# Keyword and hybrid search on the device beside SQLite FTS5 + host fusion (tools/text_time.py)\n\n")
        f.write(f"Synthetic corpus in HBM: {a.docs} documents x 16-48 tokens, dim {dim}, {a.nbits}-bit residuals, K = {a.k} (the bench "
                f"runs 10 M documents; this is the largest keyword index that Python's sqlite3 builds in about a minute: "
                f"{s_build:.0f} s to build the FTS5 table, {s_read:.0f} s to read its {data.inst_doc.size} instances of {data.n_terms} "
                f"terms, {ms_set:.0f} ms for set_text).  {a.queries} queries per call, top_k = {a.top_k}, fetch_k = {a.fetch_k}, "
                f"relative-score fusion, alpha 0.75.  Wall-clock ms per call of the whole batch from Python, median of {a.repeats} after "
                f"{a.warmup} untimed calls; sqlite and host fusion run once per query on the host, as the handler runs them.  "
                f"today = sqlite + search_batch + host fusion.\n\n")
        f.write("| queries | matches in the lists | postings visited | text_search | search_hybrid | sqlite | search_batch | host fusion | "
                "today | sqlite / text_search | today / search_hybrid | same as sqlite |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['kind']} | {r['matches']} | {r['postings_visited']} | {r['ms_text_search']} | {r['ms_search_hybrid']} | "
                    f"{r['ms_sqlite']} | {r['ms_search_batch']} | {r['ms_host_fusion']} | {r['ms_today']} | "
                    f"{r['sqlite_over_text_search']} | {r['today_over_hybrid']} | {r['same_as_sqlite']} |\n")
        f.write("\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
