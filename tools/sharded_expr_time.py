#!/usr/bin/env python3
"""Times tree keyword queries through the sharded _expr entry over a one-rank communicator beside the unsharded _expr entry.

  timeout 1100 python tools/sharded_expr_time.py [--baseline-package DIR]   # writes profiles/sharded_expr_time.md, prints JSON lines

Corpus and query sets: tools/text_expr_time.py's -- --docs documents of 4-28 words over a Zipf vocabulary of --vocab words behind
a small synthetic index of as many documents; --queries queries per call, top_k = --top-k; the sets are `flat as trees` (16 each
of 1 word, 3 words AND, 3 words OR, a 2-word phrase, lifted to trees), `tree` (("a" OR "b") AND "c" NOT "d") and single-token
prefixes whose term ranges hold about 10, 1 000 and 100 000 postings.
Every set is timed through dist.CShardedSearcher.text_search over a one-rank communicator (np_hip_text_search_sharded_expr: the
whole protocol, no collective) and through MmapIndex.text_search (np_hip_text_search_expr) on the SAME handle in one process,
in --rounds alternating rounds; a round's figure is the median over --repeats samples of --inner calls after --warmup untimed
calls, wall-clock from Python with the results fetched to the host.  Reported: the median of the rounds' ratios and their
spread.  The results of the two entries are compared byte for byte.

--baseline-package DIR: a built next-plaid_amd directory of the parent commit.  np_hip_text_search_sharded (the flat set, one
rank) and np_hip_text_search_expr (the tree set and the prefix 1000 set, unsharded) share text_run with the new path: both are
timed through THAT package and through this tree in child processes that alternate, --rounds rounds, on the same saved corpus.
--trace-run SET: only that set through the sharded entry, --trace-calls calls, for a `rocprofv3 --kernel-trace --stats` run of
its own (the counting pre-pass is text_prefix_count_kernel).  No ratio is asserted anywhere; the table is what was measured."""
import argparse
import json
import os
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


def corpus(a, T):
    """text_expr_time.py's texts and query strings: (data, {set: strings}, {prefix set: mean postings per range})"""
    g = np.random.default_rng(11)
    lens = g.integers(4, 29, a.docs)
    pr = 1.0 / np.arange(1, a.vocab + 1)
    toks = g.choice(a.vocab, int(lens.sum()), p=pr / pr.sum())
    words = np.array([f"w{i}" for i in range(a.vocab)])
    data = T.TextIndexData.from_texts([" ".join(w) for w in np.split(words[toks], np.cumsum(lens)[:-1])])
    rank = lambda: int(g.choice([g.integers(0, 20), g.integers(20, 500), g.integers(500, a.vocab)]))
    kinds = [lambda: f'"w{rank()}"', lambda: " ".join(f'"w{rank()}"' for _ in range(3)),
             lambda: " OR ".join(f'"w{rank()}"' for _ in range(3)), lambda: f'"w{g.integers(0, 30)} w{g.integers(0, 30)}"']
    sets = {"flat as trees": [kinds[i * 4 // a.queries]() for i in range(a.queries)],
            "tree": [f'("w{rank()}" OR "w{rank()}") AND "w{rank()}" NOT "w{rank()}"' for _ in range(a.queries)]}
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
    postings = {}
    for target in (10, 1000, 100000):
        best = sorted(cands, key=lambda p: (abs(np.log(max(cands[p], 1) / target)), p))[: a.queries]
        sets[f"prefix {target}"] = [p + "*" for p in best]
        postings[f"prefix {target}"] = float(np.mean([cands[p] for p in best]))
    return data, sets, postings


def compiled(T, data, name, strings):
    if name == "flat as trees":
        return [T.TextExpr.from_query(T.compile_text_query(s, data)) for s in strings]
    return [T.compile_text_expr(s, data) for s in strings]


def one_rank(npa, hx):
    from next_plaid_amd.dist import CShardedSearcher, ShardComm
    comm = ShardComm(hx, 0, 1, rccl=False)
    return comm, CShardedSearcher(hx, comm)


def digest(rows):
    return int(sum(int(r.scores.view(np.uint32).astype(np.uint64).sum()) + int(r.passage_ids.sum()) for r in rows))


def child(a):
    """np_hip_text_search_sharded (flat, one rank) and np_hip_text_search_expr (unsharded) through the package at a.package"""
    sys.path.insert(0, a.package)
    import next_plaid_amd as npa
    from next_plaid_amd import synth, text as T
    z = np.load(a.child, allow_pickle=False)
    terms = [str(t) for t in z["terms"]]
    data = T.TextIndexData("unicode61", terms, z["term_offsets"], z["inst_doc"], z["inst_pos"], int(z["n_rows"]),
                           vocab={t: i for i, t in enumerate(terms)})
    sets = json.loads(str(z["sets"]))
    hx = open_index(npa, synth, int(z["docs"]), a.queries)
    hx.set_text_shard(data)
    comm, cs = one_rank(npa, hx)
    flat = [T.compile_text_query(s, data) for s in sets["flat as trees"]]
    out = {}
    for name, fn in (("np_hip_text_search_sharded flat", lambda: cs.text_search(flat, a.top_k)),
                     ("np_hip_text_search_expr tree", None), ("np_hip_text_search_expr prefix 1000", None)):
        if fn is None:
            qs = compiled(T, data, name.split(" ", 1)[1], sets[name.split(" ", 1)[1]])
            fn = lambda qs=qs: hx.text_search(qs, a.top_k)
        d = digest(fn())
        if d == 0:
            raise SystemExit(f"{name}: no query of the set matched anything")
        med, lo, hi = sample_ms(fn, a.repeats, a.warmup, a.inner)
        out[name] = dict(ms=med, ms_min=lo, ms_max=hi, digest=d)
    comm.close()
    hx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=300_000)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--top-k", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--baseline-package", default=None)
    ap.add_argument("--trace-run", default=None, metavar="SET")
    ap.add_argument("--trace-calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_expr_time.md"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--package", default=os.path.join(ROOT, "next-plaid_amd"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, a.package)
    import next_plaid_amd as npa
    from next_plaid_amd import synth, text as T
    if npa.device_count() < 1:
        raise SystemExit("sharded_expr_time.py needs a gfx950 GPU")
    t0 = time.perf_counter()
    data, sets, postings = corpus(a, T)
    print(json.dumps(dict(what="corpus", docs=a.docs, instances=int(data.inst_doc.size), terms=data.n_terms,
                          s_build=round(time.perf_counter() - t0, 1))), flush=True)
    hx = open_index(npa, synth, a.docs, a.queries)
    hx.set_text_shard(data)      # (on an unsharded handle this is set_text)
    comm, cs = one_rank(npa, hx)
    if a.trace_run:
        qs = compiled(T, data, a.trace_run, sets[a.trace_run])
        for _ in range(a.trace_calls):
            cs.text_search(qs, a.top_k)
        comm.close()
        hx.close()
        return
    rows = []
    for name, strings in sets.items():
        qs = compiled(T, data, name, strings)
        plain, shard = (lambda qs=qs: hx.text_search(qs, a.top_k)), (lambda qs=qs: cs.text_search(qs, a.top_k))
        want, got = plain(), shard()
        same = all(np.array_equal(x.passage_ids, y.passage_ids) and x.scores.tobytes() == y.scores.tobytes() for x, y in zip(want, got))
        ms_p, ms_s = [], []
        for _ in range(a.rounds):      # alternating rounds in one process
            ms_p.append(sample_ms(plain, a.repeats, a.warmup, a.inner)[0])
            ms_s.append(sample_ms(shard, a.repeats, a.warmup, a.inner)[0])
        ratios = sorted(s / p for s, p in zip(ms_s, ms_p))
        line = dict(what="set", set=name, queries=len(qs), matches=int(sum(r.passage_ids.size for r in want)),
                    ms_unsharded=round(float(np.median(ms_p)), 4), ms_1rank=round(float(np.median(ms_s)), 4),
                    ratio=round(ratios[len(ratios) // 2], 3), ratio_min=round(ratios[0], 3), ratio_max=round(ratios[-1], 3),
                    rounds_unsharded=ms_p, rounds_1rank=ms_s, same_bits=bool(same),
                    note=f"{postings[name]:.0f} postings per range" if name in postings else "")
        rows.append(line)
        print(json.dumps(line), flush=True)
    comm.close()
    hx.close()
    base = []
    if a.baseline_package:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "corpus.npz")
            np.savez(path, terms=np.asarray(data.terms), term_offsets=data.term_offsets, inst_doc=data.inst_doc, inst_pos=data.inst_pos,
                     n_rows=data.n_rows, docs=a.docs, sets=json.dumps(sets))
            for rnd in range(a.rounds):
                for label, pkg in (("parent", a.baseline_package), ("this tree", a.package)):
                    out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", path, "--package", pkg,
                                                   "--queries", str(a.queries), "--top-k", str(a.top_k), "--repeats", str(a.repeats),
                                                   "--warmup", str(a.warmup), "--inner", str(a.inner)], text=True, timeout=600)
                    for entry, v in json.loads(out.strip().splitlines()[-1]).items():
                        line = dict(what="shared path", entry=entry, package=label, round=rnd, **v)
                        base.append(line)
                        print(json.dumps(line), flush=True)
    with open(a.out, "w") as f:
        f.write("# Tree keyword queries over a one-rank communicator beside the unsharded entry (tools/sharded_expr_time.py)\n\n")
        f.write(f"{a.docs} documents of 4-28 words over a Zipf vocabulary of {a.vocab} words ({data.inst_doc.size} instances of "
                f"{data.n_terms} terms).  {a.queries} queries per call, top_k = {a.top_k}.  Wall-clock ms per call of the whole batch "
                f"from Python with the results on the host; {a.rounds} alternating rounds in one process, each the median over "
                f"{a.repeats} samples of {a.inner} calls after {a.warmup} untimed calls.  ms columns: the median of the rounds; "
                f"ratio: the median of the rounds' own ratios, with their smallest and largest.  The flat sharded calls stand at "
                f"1.06-1.09 of the unsharded ones (profiles/sharded_hybrid_time.md).\n\n")
        f.write("| set | matches in the lists | np_hip_text_search_expr ms | np_hip_text_search_sharded_expr, 1 rank, ms | 1 rank / unsharded | "
                "min - max over the rounds | same bits | |\n|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['set']} | {r['matches']} | {r['ms_unsharded']} | {r['ms_1rank']} | {r['ratio']} | {r['ratio_min']} - {r['ratio_max']} | "
                    f"{r['same_bits']} | {r['note']} |\n")
        if base:
            f.write("\nThe entries that share text_run with the new path, parent commit and this tree, each in its own process, "
                    "alternating:\n\n| entry | package | round | ms per call | min - max | digest of the results |\n|---|---|---|---|---|---|\n")
            for r in sorted(base, key=lambda r: (r["entry"], r["round"], r["package"])):
                f.write(f"| {r['entry']} | {r['package']} | {r['round']} | {r['ms']} | {r['ms_min']} - {r['ms_max']} | {r['digest']} |\n")
            f.write("\n| entry | parent: median, min - max of the rounds | this tree: median, min - max of the rounds | inside the parent's spread |\n"
                    "|---|---|---|---|\n")
            for entry in sorted({r["entry"] for r in base}):
                p = sorted(r["ms"] for r in base if r["entry"] == entry and r["package"] == "parent")
                t = sorted(r["ms"] for r in base if r["entry"] == entry and r["package"] == "this tree")
                mt = t[len(t) // 2]
                f.write(f"| {entry} | {p[len(p) // 2]}, {p[0]} - {p[-1]} | {mt}, {t[0]} - {t[-1]} | {p[0] <= mt <= p[-1]} |\n")
        else:
            f.write("\nThe parent commit's entries: not measured (no --baseline-package).\n")
        f.write("\n```\n" + "\n".join(json.dumps(r) for r in rows + base) + "\n```\n")


if __name__ == "__main__":
    main()
