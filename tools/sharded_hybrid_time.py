#!/usr/bin/env python3
"""Times the keyword search and the hybrid request over document shards beside the unsharded calls of the same build.

  timeout 900 python tools/sharded_hybrid_time.py     # writes profiles/sharded_hybrid_time.md, one JSON line per measurement

Corpus: the bench's synthetic generator in HBM (dim 128, --docs documents of 16-48 tokens, K = --k) and, for the same
documents, texts of 4-28 words over a Zipf vocabulary of --vocab words.  The keyword table is laid out in numpy the way
fts5vocab lists it (terms in byte order, instances by term, document, position) -- nothing here is compared with SQLite, so no
FTS5 table is built -- and handed to every handle whole (set_text, set_text_shard).
Per kind of query (3 words OR: no counting exchange; a 2-word phrase: the counting exchange), --queries queries per call:
    unsharded        MmapIndex.text_search / search_hybrid on the handle that holds the whole index
    1 rank           dist.CShardedSearcher on that same handle over a one-rank communicator (NP_COMM_LOCAL): every step of the
                     protocol -- records, status words, the rank merge -- and no transport at all
    2 hosted ranks   two processes that share this GPU, each with its document shard, exchanging through pinned host memory
                     and a gloo all-gather
Wall-clock ms per call from Python, every call ending in a synchronise; the unsharded and the one-rank call alternate inside
one loop (median of --repeats rounds after --warmup untimed ones), the two-rank call is timed by rank 0 the same way.  Two ranks
that share one device through host staging say nothing about xGMI: that column is the protocol's cost on the slowest transport
there is, not a speed-up.  The one figure to read is one rank / unsharded: what the protocol itself costs.  Nothing is asserted
about any time; the results of the three routes are compared (ids and f32 bits) and the table says whether they were equal.
Run it under a time limit, as above: the tool stops at the first error.
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "next-plaid_amd"))

import next_plaid_amd as npa  # noqa: E402
from next_plaid_amd import synth, text as T  # noqa: E402

DIM = 128


def make_spec(a):
    return synth.SynthSpec(num_docs=a.docs, num_centroids=a.k, dim=DIM, nbits=a.nbits, doc_len_min=16, doc_len_max=48, seed=1236,
                           n_topics=8, rand256=51)


def make_table(a):
    """The keyword table of --docs documents of 4-28 Zipf words, as TextIndexData."""
    g = np.random.default_rng(11)
    lens = g.integers(4, 29, a.docs)
    pr = 1.0 / np.arange(1, a.vocab + 1)
    word = g.choice(a.vocab, int(lens.sum()), p=pr / pr.sum())
    doc = np.repeat(np.arange(a.docs, dtype=np.int64), lens)
    pos = (np.arange(word.size) - np.repeat(np.cumsum(lens) - lens, lens)).astype(np.int32)
    names = sorted(f"w{i}" for i in np.unique(word))                 # fts5vocab's order: the terms' bytes
    term_of = np.full(a.vocab, -1, np.int64)
    for t, name in enumerate(names):
        term_of[int(name[1:])] = t
    term = term_of[word]
    order = np.lexsort((pos, doc, term))
    off = np.zeros(len(names) + 1, np.int64)
    np.cumsum(np.bincount(term, minlength=len(names)), out=off[1:])
    return T.TextIndexData("unicode61", names, off, doc[order], pos[order], a.docs, {n: i for i, n in enumerate(names)})


def make_queries(a, data):
    g = np.random.default_rng(5)
    rank = lambda: int(g.choice([g.integers(0, 20), g.integers(20, 500), g.integers(500, a.vocab)]))
    kinds = {"3 words OR": lambda: " OR ".join(f'"w{rank()}"' for _ in range(3)),
             "2-word phrase": lambda: f'"w{g.integers(0, 30)} w{g.integers(0, 30)}"'}
    return {kind: [T.compile_text_query(make(), data) for _ in range(a.queries)] for kind, make in kinds.items()}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def medians(fns, repeats, warmup):
    """The calls of `fns` alternate inside one loop; the median of each."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for t, fn in zip(ts, fns):
            t.append(timed(fn))
    return [sorted(t)[len(t) // 2] for t in ts]


def same(x, y):
    return all(np.array_equal(r.passage_ids, f.passage_ids) and r.scores.tobytes() == f.scores.tobytes() for r, f in zip(x, y))


def rank_main(rank, world, port, a, q):
    """One of the two hosted ranks: its shard, the whole table, the same calls as the parent; rank 0 reports."""
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch.distributed as dist
        from next_plaid_amd.dist import CShardedSearcher, ShardComm, gloo_all_gather
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            spec = make_spec(a)
            cen = synth.centroids(spec)
            shard = npa.MmapIndex.synth(spec, centroids=cen, max_batch=a.queries, shard_rank=rank, shard_count=world)
            data = make_table(a)
            shard.set_text_shard(data)
            qs = list(synth.make_queries(spec, a.queries, n_tokens=a.query_tokens, cen=cen)[0])
            comm = ShardComm(shard, rank, world, all_gather=gloo_all_gather())
            cs = CShardedSearcher(shard, comm)
            p = npa.SearchParameters(top_k=a.top_k, n_full_scores=4096, n_ivf_probe=8)
            out = {}
            for kind, tq in make_queries(a, data).items():
                ms = medians([lambda: cs.text_search(tq, a.fetch_k), lambda: cs.search_hybrid(qs, tq, p, fetch_k=a.fetch_k)],
                             a.repeats, a.warmup)
                kw, hy = cs.text_search(tq, a.fetch_k), cs.search_hybrid(qs, tq, p, fetch_k=a.fetch_k)
                out[kind] = dict(ms_text=ms[0], ms_hybrid=ms[1], kw=[(r.passage_ids, r.scores) for r in kw],
                                 hy=[(r.passage_ids, r.scores) for r in hy])
            dist.barrier()
        finally:
            dist.destroy_process_group()
        q.put(("ok", rank, out if rank == 0 else None))
    except BaseException as e:   # noqa: BLE001 -- reported to the parent
        import traceback
        q.put(("fail", rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))[-3000:]))


def two_ranks(a, timeout):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=rank_main, args=(r, 2, port, a, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=timeout))   # a rank stuck in a collective ends the tool here
    finally:
        for p in procs:
            p.join(timeout=20)
            if p.is_alive():
                p.kill()
    bad = [r for r in res if r[0] != "ok"]
    if bad:
        raise SystemExit("\n".join(f"rank {r[1]}:\n{r[2]}" for r in bad))
    return next(r[2] for r in res if r[1] == 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=16384)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--query-tokens", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--fetch-k", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rank-timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_hybrid_time.md"))
    a = ap.parse_args()
    if npa.device_count() < 1:
        raise SystemExit("sharded_hybrid_time.py needs a gfx950 GPU")
    from next_plaid_amd.dist import CShardedSearcher, ShardComm
    spec = make_spec(a)
    cen = synth.centroids(spec)
    hx = npa.MmapIndex.synth(spec, centroids=cen, max_batch=a.queries)
    t0 = time.perf_counter()
    data = make_table(a)
    s_table = time.perf_counter() - t0
    hx.set_text_shard(data)     # (on an unsharded handle: set_text)
    qs = list(synth.make_queries(spec, a.queries, n_tokens=a.query_tokens, cen=cen)[0])
    comm = ShardComm(hx, 0, 1, rccl=False)
    cs = CShardedSearcher(hx, comm)
    p = npa.SearchParameters(top_k=a.top_k, n_full_scores=4096, n_ivf_probe=8)
    print(json.dumps(dict(what="corpus", docs=a.docs, instances=int(data.inst_doc.size), terms=data.n_terms,
                          s_table=round(s_table, 1))), flush=True)
    rows, plain = [], {}
    for kind, tq in make_queries(a, data).items():
        calls = [lambda: hx.text_search(tq, a.fetch_k), lambda: cs.text_search(tq, a.fetch_k),
                 lambda: hx.search_hybrid(qs, tq, p, fetch_k=a.fetch_k), lambda: cs.search_hybrid(qs, tq, p, fetch_k=a.fetch_k)]
        ms = medians(calls, a.repeats, a.warmup)
        got = [fn() for fn in calls]
        plain[kind] = (got[0], got[2])
        rows.append(dict(what="sharded_hybrid", kind=kind, docs=a.docs, queries=a.queries, fetch_k=a.fetch_k,
                         matches=int(sum(r.passage_ids.size for r in got[0])),
                         ms_text_unsharded=round(ms[0], 3), ms_text_1rank=round(ms[1], 3), text_1rank_over_unsharded=round(ms[1] / ms[0], 3),
                         ms_hybrid_unsharded=round(ms[2], 3), ms_hybrid_1rank=round(ms[3], 3),
                         hybrid_1rank_over_unsharded=round(ms[3] / ms[2], 3), same_1rank=bool(same(got[1], got[0]) and same(got[3], got[2]))))
    comm.close()
    hx.close()
    two = two_ranks(a, a.rank_timeout)
    for r in rows:
        t = two[r["kind"]]
        kw, hy = plain[r["kind"]]
        r.update(ms_text_2ranks=round(t["ms_text"], 3), ms_hybrid_2ranks=round(t["ms_hybrid"], 3),
                 same_2ranks=bool(all(np.array_equal(x.passage_ids, i) and x.scores.tobytes() == s.tobytes() for x, (i, s) in zip(kw, t["kw"]))
                                  and all(np.array_equal(x.passage_ids, i) and x.scores.tobytes() == s.tobytes() for x, (i, s) in zip(hy, t["hy"]))))
        print(json.dumps(r), flush=True)
    with open(a.out, "w") as f:
        f.write("# Keyword and hybrid search over document shards beside the unsharded calls (tools/sharded_hybrid_time.py)\n\n")
        f.write(f"Synthetic corpus in HBM: {a.docs} documents x 16-48 tokens, dim {DIM}, {a.nbits}-bit residuals, K = {a.k}; keyword table "
                f"of {data.inst_doc.size} instances of {data.n_terms} terms.  {a.queries} queries per call, top_k = {a.top_k}, fetch_k = "
                f"{a.fetch_k}, relative-score fusion, alpha 0.75.  Wall-clock ms per call of the whole batch from Python, every call "
                f"ending in a synchronise; median of {a.repeats} rounds after {a.warmup} untimed ones, the unsharded and the one-rank "
                f"call alternating inside one loop.  **1 rank** is the sharded call on the unsharded handle over a one-rank communicator: "
                f"the protocol's own cost, no transport.  **2 hosted ranks** are two processes that share this one GPU and exchange "
                f"through pinned host memory and a gloo all-gather: they say nothing about xGMI or RCCL, and no speed-up is claimed or "
                f"expected from them.  Nothing is asserted about any time.\n\n")
        f.write("| queries | matches in the lists | text unsharded | text 1 rank | 1 rank / unsharded | text 2 hosted ranks | hybrid unsharded | "
                "hybrid 1 rank | 1 rank / unsharded | hybrid 2 hosted ranks | 1 rank same bits | 2 ranks same bits |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['kind']} | {r['matches']} | {r['ms_text_unsharded']} | {r['ms_text_1rank']} | {r['text_1rank_over_unsharded']} | "
                    f"{r['ms_text_2ranks']} | {r['ms_hybrid_unsharded']} | {r['ms_hybrid_1rank']} | {r['hybrid_1rank_over_unsharded']} | "
                    f"{r['ms_hybrid_2ranks']} | {r['same_1rank']} | {r['same_2ranks']} |\n")
        f.write("\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
