#!/usr/bin/env python3
"""Times keyword search with tree queries (np_hip_text_search_expr) beside the flat entry and beside SQLite FTS5 on the host.

  timeout 1100 python tools/text_expr_time.py [--baseline-package DIR]   # writes profiles/text_expr_time.md, prints JSON lines

Corpus: the texts of tools/text_time.py -- --docs documents of 4-28 words over a Zipf vocabulary of --vocab words w0, w1, ...
in an in-memory FTS5 table (unicode61) -- behind a small synthetic index of as many documents (a keyword search reads the
document count only).  Per set of --queries queries, one call per batch, top_k = --top-k:
    flat       16 each of text_time's kinds (1 word, 3 words AND, 3 words OR, a 2-word phrase), as TextQuery objects through
               np_hip_text_search and lifted to trees through np_hip_text_search_expr (the results are compared byte for byte)
    tree       ("a" OR "b") AND "c" NOT "d" over words drawn by rank as text_time draws them
    prefix N   single-token prefixes w<digits>* whose term ranges hold about N postings (10, 1 000, 100 000)
    sqlite     the handler's statement for the same strings, once per query, on the host
Wall-clock per call from Python, every call ending in a synchronise inside the library: the median over --repeats samples of
--inner calls each, after --warmup untimed calls.  The device's results are compared with SQLite's (f32 score bits; ids where
the scores are distinct).

--baseline-package DIR: a built next-plaid_amd directory of another commit (its Python package beside its csrc/ library).  The
flat set is then timed through THAT package too, in child processes that alternate with child processes of this tree on the
same saved corpus: np_hip_text_search's time before and after, measured the same way.  No ratio is asserted anywhere; the
table is what was measured.  Run it under a time limit, as above: the tool stops at the first error."""
import argparse
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sample_ms(fn, repeats, warmup, inner):
    """ms per call: (median, min, max) over `repeats` samples of `inner` calls."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ts.append(1e3 * (time.perf_counter() - t0) / inner)
    ts.sort()
    return round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)


def open_index(npa, synth, docs, queries):
    spec = synth.SynthSpec(num_docs=docs, num_centroids=64, dim=32, nbits=2, doc_len_min=1, doc_len_max=1, seed=1236)
    return npa.MmapIndex.synth(spec, max_batch=queries, n_contexts=1)


def child(a):
    """The flat set through the package at a.package, on the corpus and queries saved in a.child."""
    sys.path.insert(0, a.package)
    import next_plaid_amd as npa
    from next_plaid_amd import synth, text as T
    z = np.load(a.child)
    data = T.TextIndexData("unicode61", [], z["term_offsets"], z["inst_doc"], z["inst_pos"], int(z["n_rows"]))
    data.terms = [None] * (z["term_offsets"].size - 1)   # (set_text reads the count)
    hx = open_index(npa, synth, int(z["docs"]), a.queries)
    hx.set_text(data)
    qs = [T.TextQuery(z["terms"][z["tok_off"][i]: z["tok_off"][i + 1]], z["phr_off"][z["phr_at"][i]: z["phr_at"][i + 1]], int(z["modes"][i]))
          for i in range(z["modes"].size)]
    got = hx.text_search(qs, a.top_k)
    digest = int(sum(int(r.scores.view(np.uint32).astype(np.uint64).sum()) + int(r.passage_ids.sum()) for r in got))
    med, lo, hi = sample_ms(lambda: hx.text_search(qs, a.top_k), a.repeats, a.warmup, a.inner)
    hx.close()
    print(json.dumps(dict(ms=med, ms_min=lo, ms_max=hi, digest=digest)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=300_000)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--top-k", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--baseline-package", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_expr_time.md"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--package", default=os.path.join(ROOT, "next-plaid_amd"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, a.package)
    import next_plaid_amd as npa
    from next_plaid_amd import synth, text as T
    if npa.device_count() < 1:
        raise SystemExit("text_expr_time.py needs a gfx950 GPU")
    # text_time.py's texts: Zipf ranks, 4-28 words per document
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
    data = T.TextIndexData._read(con, T.FTS_TABLE, "unicode61")
    s_build = time.perf_counter() - t0
    print(json.dumps(dict(what="corpus", docs=a.docs, instances=int(data.inst_doc.size), terms=data.n_terms, s_build=round(s_build, 1))),
          flush=True)
    sql = (f'SELECT rowid, CAST(-bm25("{T.FTS_TABLE}") AS REAL) AS score FROM "{T.FTS_TABLE}" WHERE "{T.FTS_TABLE}" MATCH ? '
           "ORDER BY score DESC LIMIT ?")
    rank = lambda: int(g.choice([g.integers(0, 20), g.integers(20, 500), g.integers(500, a.vocab)]))
    kinds = [lambda: f'"w{rank()}"', lambda: " ".join(f'"w{rank()}"' for _ in range(3)),
             lambda: " OR ".join(f'"w{rank()}"' for _ in range(3)), lambda: f'"w{g.integers(0, 30)} w{g.integers(0, 30)}"']
    flat_strings = [kinds[i * 4 // a.queries]() for i in range(a.queries)]
    tree_strings = [f'("w{rank()}" OR "w{rank()}") AND "w{rank()}" NOT "w{rank()}"' for _ in range(a.queries)]
    # prefixes w<digits>* by the postings of their term ranges (a posting = a (term, document) pair)
    off, doc = data.term_offsets, data.inst_doc
    first = np.ones(doc.size, bool)
    first[1:] = doc[1:] != doc[:-1]
    first[off[:-1][off[:-1] < doc.size]] = True
    post_cum = np.concatenate([[0], np.cumsum(first)])
    cands = {}
    for t in data.terms:
        for n in range(2, len(t) + 1):
            cands.setdefault(t[:n], None)
    for pre in cands:
        lo, hi = T.prefix_range(pre, data)
        cands[pre] = int(post_cum[off[hi]] - post_cum[off[lo]])
    prefix_sets = {}
    for target in (10, 1000, 100000):
        best = sorted(cands, key=lambda p: (abs(np.log(max(cands[p], 1) / target)), p))[: a.queries]
        prefix_sets[target] = ([p + "*" for p in best], float(np.mean([cands[p] for p in best])))

    hx = open_index(npa, synth, a.docs, a.queries)
    hx.set_text(data)

    def sqlite_all(strings):
        return [con.execute(sql, (s, a.top_k)).fetchall() for s in strings]

    def same_as_sqlite(strings, got):
        same = True
        for w, r in zip(sqlite_all(strings), got):
            w = sorted(w, key=lambda x: (-x[1], x[0]))
            same = same and np.array_equal(np.asarray([x[1] for x in w], np.float64).astype(np.float32).view(np.uint32),
                                           r.scores.view(np.uint32))
            safe = sum(x[1] > w[-1][1] for x in w) if len(w) == a.top_k else len(w)   # a cut inside equal scores: SQLite's choice
            same = same and [x[0] for x in w[:safe]] == r.passage_ids[:safe].tolist()
        return bool(same)

    rows = []

    def measure(name, strings, queries, note=""):
        got = hx.text_search(queries, a.top_k)
        entry = "np_hip_text_search_expr" if any(isinstance(q, T.TextExpr) for q in queries) else "np_hip_text_search"
        med, lo, hi = sample_ms(lambda: hx.text_search(queries, a.top_k), a.repeats, a.warmup, a.inner)
        sq = sample_ms(lambda: sqlite_all(strings), 3, 1, 1)
        line = dict(what="set", set=name, entry=entry, queries=len(queries), matches=int(sum(r.passage_ids.size for r in got)),
                    postings_visited=int(hx.last_stats["n_ivf_ids"]), ms=med, ms_min=lo, ms_max=hi, ms_sqlite=sq[0],
                    same_as_sqlite=same_as_sqlite(strings, got), note=note)
        rows.append(line)
        print(json.dumps(line), flush=True)
        return got

    flat = [T.compile_text_query(s, data) for s in flat_strings]
    got_flat = measure("flat", flat_strings, flat)
    got_lift = measure("flat as trees", flat_strings, [T.TextExpr.from_query(q) for q in flat])
    lifted_equal = all(np.array_equal(x.passage_ids, y.passage_ids) and x.scores.tobytes() == y.scores.tobytes()
                       for x, y in zip(got_flat, got_lift))
    measure("tree", tree_strings, [T.compile_text_expr(s, data) for s in tree_strings])
    for target, (strings, mean_post) in prefix_sets.items():
        measure(f"prefix {target}", strings, [T.compile_text_expr(s, data) for s in strings], note=f"{mean_post:.0f} postings per range")
    hx.close()
    # np_hip_text_search before and after: child processes of both packages, alternating, on the saved corpus
    base = []
    if a.baseline_package:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "corpus.npz")
            tok_off = np.concatenate([[0], np.cumsum([q.terms.size for q in flat])])
            phr_at = np.concatenate([[0], np.cumsum([q.phrase_offsets.size for q in flat])])
            np.savez(path, term_offsets=data.term_offsets, inst_doc=data.inst_doc, inst_pos=data.inst_pos, n_rows=data.n_rows, docs=a.docs,
                     terms=np.concatenate([q.terms for q in flat]), tok_off=tok_off, phr_off=np.concatenate([q.phrase_offsets for q in flat]),
                     phr_at=phr_at, modes=np.asarray([q.mode for q in flat]))
            for rnd in range(2):
                for label, pkg in (("parent", a.baseline_package), ("this tree", a.package)):
                    out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", path, "--package", pkg,
                                                   "--queries", str(a.queries), "--top-k", str(a.top_k), "--repeats", str(a.repeats),
                                                   "--warmup", str(a.warmup), "--inner", str(a.inner)], text=True, timeout=600)
                    line = dict(what="np_hip_text_search", package=label, round=rnd, **json.loads(out.strip().splitlines()[-1]))
                    base.append(line)
                    print(json.dumps(line), flush=True)
    with open(a.out, "w") as f:
        f.write("# Keyword search with tree queries beside the flat entry and SQLite FTS5 (tools/text_expr_time.py)\n\n")
        f.write(f"{a.docs} documents of 4-28 words over a Zipf vocabulary of {a.vocab} words ({data.inst_doc.size} instances of {data.n_terms} "
                f"terms; {s_build:.0f} s to build and read the FTS5 table).  {a.queries} queries per call, top_k = {a.top_k}.  Wall-clock ms "
                f"per call of the whole batch from Python (median, min - max over {a.repeats} samples of {a.inner} calls after {a.warmup} "
                f"untimed calls); sqlite runs the handler's statement once per query on the host (median of 3).  flat as trees returns "
                f"the flat entry's bytes: {lifted_equal}.\n\n")
        f.write("| set | entry | matches in the lists | postings visited | ms per call | min - max | sqlite ms | same as sqlite | |\n"
                "|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['set']} | {r['entry']} | {r['matches']} | {r['postings_visited']} | {r['ms']} | {r['ms_min']} - {r['ms_max']} | "
                    f"{r['ms_sqlite']} | {r['same_as_sqlite']} | {r['note']} |\n")
        if base:
            f.write("\nnp_hip_text_search on the flat set, parent commit and this tree, each in its own process, alternating:\n\n"
                    "| package | round | ms per call | min - max | digest of the results |\n|---|---|---|---|---|\n")
            for r in base:
                f.write(f"| {r['package']} | {r['round']} | {r['ms']} | {r['ms_min']} - {r['ms_max']} | {r['digest']} |\n")
        else:
            f.write("\nnp_hip_text_search of the parent commit: not measured (no --baseline-package).\n")
        f.write("\n```\n" + "\n".join(json.dumps(r) for r in rows + base) + "\n```\n")


if __name__ == "__main__":
    main()
