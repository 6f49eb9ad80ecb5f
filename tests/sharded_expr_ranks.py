"""The ranks of tests/test_gpu_sharded_expr.py: G spawned processes that share GPU 0 and exchange over the hosted transport (a
gloo all-gather), as tests/sharded_hybrid_ranks.py runs them.  One spawn per (G, mode) runs every case of that mode, so that a
test stays at seconds.  Every rank opens the unsharded handle too and compares with it bit for bit.  For the keyword calls rank
0's handle is opened with max_batch = 5: it runs every batch in chunks of five queries while its peers run one chunk.  (The
semantic half of a hybrid call must fit one chunk: that one runs on a handle with the default.)"""
import os
import sys

import numpy as np

from sharded_hybrid_ranks import _free_port, same_all

SEM_QUERIES = 12
GEOMETRY = dict(num_centroids=64, dim=32, nbits=2, doc_len_min=4, doc_len_max=12, seed=11)
RANK0_OPTS = dict(max_batch=5)


def fixtures():
    """What every rank and the in-process tests build alike: arrays, the keyword table and its restatement, the semantic queries,
    the tree queries (the CPU fixture's, a query at the limits of one tree, the f32 collision's lifted to a tree), flat queries,
    the columns."""
    from helpers import make_arrays, synth
    from next_plaid_amd import text as T
    import shard_text_expr_restate as X
    import shard_text_restate as S
    n = X.N_GPU
    spec, a = make_arrays(num_docs=n, **GEOMETRY)
    data = T.TextIndexData.from_texts(X.corpus_texts(n))
    rs = X.RestatedExpr(data, n)
    qs, _ = synth.make_queries(spec, SEM_QUERIES, n_tokens=8, cen=a["centroids"])
    exprs = X.special_exprs(data) + [limit_expr(data)]
    found = S.find_f32_collision(rs, data, n, [2, 3], tries=200)
    if found is not None:
        exprs.append(T.TextExpr.from_query(found[0]))
    v = data.vocab
    ids = lambda *ws: [v.get(w, -1) for w in ws]
    flat = [T.TextQuery.from_phrases([ids("wo0")], T.NP_TEXT_AND), T.TextQuery.from_phrases([ids("wo3"), ids("wo5")], T.NP_TEXT_OR),
            T.TextQuery.from_phrases([ids("wo1", "mida"), ids("wo4")], T.NP_TEXT_OR), T.TextQuery.from_phrases([ids("lefa")], T.NP_TEXT_AND),
            T.TextQuery.from_phrases([ids("tie"), ids("wo1")], T.NP_TEXT_AND), T.TextQuery.from_phrases([ids("nowhere"), ids("wo2")], T.NP_TEXT_OR)]
    d = np.arange(n, dtype=np.int64)
    rows = {"d": d, "z": d % 4}
    return n, spec, a, data, rs, list(qs), exprs, flat, rows


def limit_expr(data):
    """64 phrases under 127 nodes in one query: single-token prefixes, exact tokens, and phrases of two tokens that end in a
    prefix, joined by ORs with one NOT at the root."""
    from next_plaid_amd import text as T
    v = data.vocab
    words = ["lef", "mid", "wo1", "no", "ti", "wo", "lefa", "alp"]
    leaves = []
    for i in range(63):
        if i % 3 == 0:
            leaves.append(("phrase", [0], T.prefix_range(words[(i // 3) % len(words)], data)))
        elif i % 3 == 1:
            leaves.append(("phrase", [v[f"wo{i % 16}"]]))
        else:
            leaves.append(("phrase", [v[f"wo{i % 5}"], 0], T.prefix_range("mid" if i % 2 else "wo1", data)))
    tree = leaves[0]
    for leaf in leaves[1:]:
        tree = ("or", tree, leaf)
    e = T.TextExpr.from_tree(("not", tree, ("phrase", [v["notb"]])))
    assert e.n_phrases == 64 and e.n_nodes == 127
    return e


def filter_cases(n):
    """One filter per query: spread over the shards, none, everything, nothing anywhere, the first shard only, the last."""
    return [("z = ?", [1]), None, ("1=1", []), ("z = ?", [9]), ("d < ?", [n // 7]), ("d >= ?", [n - n // 7])]


def subset_cases(n, n_queries):
    """one subset per query: none, every third document, an empty one, ids outside the range and duplicates, everything"""
    some = np.arange(0, n, 3)
    odd = np.array([3, n - 2, n - 1, n + 7000, -1, 3, n // 2 + 9, n // 2 + 9, 18, n - 11, 15, 30, n // 2 + 5], np.int64)
    return [(None, some, np.zeros(0, np.int64), odd, some, np.arange(n))[i % 6] for i in range(n_queries)]


def keyword_parity(cs, full, rs, exprs, n, what):
    """every tree at top_k 1, 10 and 1024, without a scope and with one subset per query: the unsharded handle's _expr call and
    the restatement, bit for bit"""
    whole = [rs.expr_scores(e) for e in exprs]
    n_hits = 0
    for subsets in (None, subset_cases(n, len(exprs))):
        for k in (1, 10, 1024):
            got = cs.text_search(exprs, k, subsets=subsets)
            same_all(got, full.text_search(exprs, k, subsets=subsets), f"{what} text_search k={k} vs the unsharded handle")
            for i, r in enumerate(got):
                sub = None if subsets is None else subsets[i]
                ids, sc = rs.rank(whole[i], k, None if sub is None else sub[(sub >= 0) & (sub < n)])
                assert np.array_equal(r.passage_ids, ids) and np.array_equal(r.scores.view(np.uint32), sc.view(np.uint32)), \
                    f"{what} text_search k={k} q{i} vs the restatement"
                n_hits += ids.size
    assert n_hits > 0


def filtered_parity(cs, full, exprs, n, what):
    conds = filter_cases(n)
    qs = exprs[:len(conds)]
    for k in (10, 1024):
        want = full.text_search(qs, k, filters=conds)
        same_all(cs.text_search(qs, k, filters=conds), want, f"{what} text_search(filters) k={k}")
    assert want[3].passage_ids.size == 0 and want[1].passage_ids.size > 0


def hybrid_parity(cs, full, qs, exprs, n, npa, what):
    texts = list(exprs[:len(qs) - 2]) + ["", "wo1 wo2"]      # (strings compile to flat queries and are lifted with the batch)
    p = npa.SearchParameters(n_full_scores=128, top_k=7, n_ivf_probe=4)
    conds = [filter_cases(n)[i % 6] for i in range(len(qs))]
    scopes = [{}, {"subsets": subset_cases(n, len(qs))}, {"filters": conds}]
    n_hits = 0
    for fusion in ("relative_score", "rrf"):
        for alpha in (0.75, 0.5):
            for scope in scopes:
                want = full.search_hybrid(qs, texts, p, alpha=alpha, fusion=fusion, fetch_k=15, **scope)
                same_all(cs.search_hybrid(qs, texts, p, alpha=alpha, fusion=fusion, fetch_k=15, **scope), want,
                         f"{what} search_hybrid {fusion} {alpha} {list(scope)}")
                n_hits += sum(r.passage_ids.size for r in want)
    assert n_hits > 0


def lifted_parity(cs, flat, what):
    """a flat batch lifted to trees: the flat sharded entry's bytes"""
    from next_plaid_amd import text as T
    for k in (10, 1024):
        same_all(cs.text_search([T.TextExpr.from_query(q) for q in flat], k), cs.text_search(flat, k), f"{what} lifted k={k}")


def many_queries(exprs, n=300):
    return [exprs[i % len(exprs)] for i in range(n)]


def rank_main(rank, world, port, mode, q):
    """One rank = one process; all ranks use GPU 0.  Reports ("ok", rank) or ("fail", rank, message) through q."""
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        here = os.path.dirname(os.path.abspath(__file__))
        for p in (here, os.path.dirname(here), os.path.join(os.path.dirname(here), "next-plaid_amd")):
            if p not in sys.path:
                sys.path.insert(0, p)
        import pytest
        import torch.distributed as dist
        from helpers import hip_index
        import next_plaid_amd as npa
        from next_plaid_amd.dist import CShardedSearcher, ShardComm, gloo_all_gather
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            n, spec, a, data, rs, qs, exprs, flat, rows = fixtures()
            full = hip_index(a)
            full.set_text(data)
            full.set_columns(rows)
            shard = hip_index(a, shard_rank=rank, shard_count=world)
            shard.set_columns(rows)
            shard_kw = shard      # the keyword calls' handle
            if rank == 0:
                shard_kw = hip_index(a, shard_rank=rank, shard_count=world, **RANK0_OPTS)
                shard_kw.set_columns(rows)
            bad = world - 1
            if mode == "parity":
                shard.set_text_shard(data)
                if shard_kw is not shard:
                    shard_kw.set_text_shard(data)
                for deferred in (False, True):
                    comm = ShardComm(shard_kw, rank, world, all_gather=gloo_all_gather(), deferred_status=deferred)
                    cs = CShardedSearcher(shard_kw, comm)
                    what = f"G={world} rank {rank} deferred={deferred}:"
                    keyword_parity(cs, full, rs, exprs, n, what)
                    lifted_parity(cs, flat, what)
                    if not deferred:   # 300 queries at top_k 1024: two exchanges (np_dist_plan.h cuts by B and top_k alone)
                        many = many_queries(exprs)
                        got = cs.text_search(many, 1024)
                        same_all(got, full.text_search(many, 1024), what + " two exchanges")
                        same_all(got[:255], cs.text_search(many[:255], 1024), what + " one exchange")
                    filtered_parity(cs, full, exprs, n, what)
                    assert comm.status() == (-1, 0)
                    comm.close()
                    comm = ShardComm(shard, rank, world, all_gather=gloo_all_gather(), deferred_status=deferred)
                    cs = CShardedSearcher(shard, comm)
                    hybrid_parity(cs, full, qs, exprs, n, npa, what)
                    assert comm.status() == (-1, 0)
                    comm.close()
            elif mode == "failure":   # the last rank never calls set_text_shard: an argument-level failure of that rank alone
                if rank != bad:
                    shard.set_text_shard(data)
                counted, exact = [exprs[1], exprs[3]], [exprs[4]]      # mid*, wo1 mid*; nota NOT notb
                prm = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=4)
                for deferred in (False, True):
                    comm = ShardComm(shard, rank, world, all_gather=gloo_all_gather(), deferred_status=deferred)
                    cs = CShardedSearcher(shard, comm)
                    for batch in (counted, exact):      # with and without the counting exchange
                        rc, out = cs.text_search_device(batch, 10)
                        cs.stream.synchronize()
                        msg, cnt, status = npa.api.last_error() if rc else "", out[2].cpu().numpy()[: len(batch)], comm.status()
                        if rank == bad:
                            assert rc == 8 and "no keyword index" in msg, (rc, msg)             # its own error
                        elif not deferred:
                            assert rc == 2 and f"shard {bad} failed with status 8" in msg, (rc, msg)
                            assert status == (-1, 0), status                                   # reported by the return code alone
                        else:
                            assert rc == 0 and (cnt == -1).all() and status == (bad, 8), (rc, cnt, status)
                        err = (ValueError, "no keyword index") if rank == bad else (npa.SearchError, f"shard {bad} failed with status 8")
                        with pytest.raises(err[0], match=err[1]):
                            cs.text_search(batch, 10)
                        with pytest.raises(err[0], match=err[1]):
                            cs.search_hybrid(qs[:2], batch[:1] * 2, prm)
                    # the communicator serves the next batch: a flat keyword one, once the rank has its table
                    if rank == bad:
                        shard.set_text_shard(data)
                    same_all(cs.text_search(flat, 10), full.text_search(flat, 10), f"rank {rank}: the flat batch after the failures")
                    same_all(cs.text_search(counted, 10), full.text_search(counted, 10), f"rank {rank}: the tree batch after the failures")
                    assert comm.status() == (-1, 0)
                    comm.close()
                    if rank == bad:
                        shard.set_text_shard(None)
            else:
                raise ValueError(mode)
            dist.barrier()
        finally:
            dist.destroy_process_group()
        q.put(("ok", rank))
    except BaseException as e:   # noqa: BLE001 -- reported to the parent, which fails the test
        import traceback
        q.put(("fail", rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))[-3000:]))


def run_ranks(world, mode, timeout=300):
    """`world` rank processes (at most 3: with the parent no more than 4 hold the GPU), each under a time limit."""
    import multiprocessing as mp
    assert world <= 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=rank_main, args=(r, world, port, mode, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=timeout))   # a hang (a rank stuck in a collective) fails here, not at the box's limit
    finally:
        for p in procs:
            p.join(timeout=20)
            if p.is_alive():
                p.kill()
    bad = [r for r in res if r[0] != "ok"]
    assert not bad, "\n".join(f"rank {r[1]}:\n{r[2]}" for r in bad)
