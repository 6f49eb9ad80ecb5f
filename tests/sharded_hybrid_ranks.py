"""The ranks of tests/test_gpu_sharded_hybrid.py: G spawned processes that share GPU 0 and exchange over the hosted transport
(a gloo all-gather), the pattern of tests/test_gpu_sharded_ranks.py.  One spawn per (G, mode) runs every case of that mode, so
that a test stays at seconds.  Every rank opens the unsharded handle too and compares with it bit for bit."""
import dataclasses
import os
import socket
import sys

import numpy as np

SEM_QUERIES = 12


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def same(r, f):
    return (np.array_equal(r.passage_ids, f.passage_ids) and r.scores.dtype == f.scores.dtype == np.float32
            and r.scores.tobytes() == f.scores.tobytes())


def same_all(got, want, what):
    assert len(got) == len(want), what
    for i, (r, f) in enumerate(zip(got, want)):
        assert same(r, f), f"{what} q{i}: {r.passage_ids[:8]} {r.scores[:8]} vs {f.passage_ids[:8]} {f.scores[:8]}"


def fixtures():
    """What every rank and the one-rank test build alike: arrays, texts, the keyword table and its restatement, the semantic
    queries, the keyword queries (special_queries and the f32 collision's), the columns."""
    from helpers import make_arrays, synth
    from next_plaid_amd import text as T
    import shard_text_restate as S
    import text_restate as R
    spec, a = make_arrays(**S.GEOMETRY)
    data = T.TextIndexData.from_texts(S.corpus_texts())
    rs = R.Restated(data, S.N_DOCS)
    qs, _ = synth.make_queries(spec, SEM_QUERIES, n_tokens=8, cen=a["centroids"])
    tqs = S.special_queries(data)
    found = S.find_f32_collision(rs, data, S.N_DOCS, [2, 3])
    if found is not None:
        tqs.append(found[0])
    rows = dict(S.filter_rows(), d=np.arange(S.N_DOCS, dtype=np.int64))
    return spec, a, data, rs, list(qs), tqs, rows


def filter_cases():
    """One filter per semantic query: the spread filters of the CPU test, 1=1, nothing anywhere, nothing on the last shard, a
    REGEXP over a text column on the device, and queries without a filter."""
    import shard_text_restate as S
    even, skew = S.SPREAD_FILTERS
    return [even, skew, None, ("1=1", []), ("z = ?", [9]), ("d < ?", [400]), ("s REGEXP ?", ["^al"]), even, None,
            ("z = ? AND u = ?", [1, 1]), skew, ("s REGEXP ? AND d >= ?", ["a_x[0-3]$", 700])]


def hybrid_texts():
    return ["wo1 wo2", "wo3 OR righty OR lefty", '"alpha beta"', "", "nowhere", "wo0", '"beta alpha" OR tie', "wo5 AND wo1 AND wo0",
            "wo2", "tie", '"alpha beta" OR wo4', "lefty"]


def param_cases(npa):
    return [("dense", npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=4)),
            ("no threshold, f32", npa.SearchParameters(n_full_scores=64, top_k=7, n_ivf_probe=4, centroid_score_threshold=None,
                                                       precision=0)),
            ("batched probe", npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=4, centroid_score_threshold=None,
                                                   centroid_batch_size=32))]


def subset_cases(n_queries):
    """None; one subset per query with an empty one; ids outside the range and duplicates."""
    import shard_text_restate as S
    some = np.arange(0, S.N_DOCS, 3)
    odd = np.array([3, 1499, 1500, 7000, -1, 3, 750, 750, 10, 1490, 5, 25, 400, 900], np.int64)
    per_query = [(None, some, np.zeros(0, np.int64), odd, some, np.arange(S.N_DOCS))[i % 6] for i in range(n_queries)]
    return [None, per_query]


def keyword_parity(cs, full, rs, tqs, what):
    import text_restate as R
    whole = [rs.scores(q) for q in tqs]
    n_hits = 0
    for subsets in subset_cases(len(tqs)):
        for k in (1, 10, 1024):
            got = cs.text_search(tqs, k, subsets=subsets)
            same_all(got, full.text_search(tqs, k, subsets=subsets), f"{what} text_search k={k} vs the unsharded handle")
            for i, r in enumerate(got):
                sub = None if subsets is None else subsets[i]
                ids, sc = R.Restated.rank(whole[i], k, None if sub is None else sub[(sub >= 0) & (sub < rs.doc_len.size)])
                assert np.array_equal(r.passage_ids, ids) and np.array_equal(r.scores.view(np.uint32), sc.view(np.uint32)), \
                    f"{what} text_search k={k} q{i} vs the restatement"
                n_hits += ids.size
    assert n_hits > 0


def padding_check(cs, tqs, what):
    """The rows of the raw outputs behind a query's count: id 0 and score +0.0, whatever the buffers held."""
    import torch
    n, k = len(tqs), 40
    with torch.cuda.stream(cs.stream):
        out = (torch.full((n, k), 7, dtype=torch.int64, device=cs.device), torch.full((n, k), 7.0, dtype=torch.float32, device=cs.device),
               torch.full((n,), 7, dtype=torch.int32, device=cs.device))
        rc, out = cs.text_search_device(tqs, k, out=out)
        assert rc == 0, what
        ids, sc, cnt = (o.cpu().numpy() for o in out)
    cs.stream.synchronize()
    assert cs.comm.status() == (-1, 0)
    assert (cnt == k).any() and (cnt < k).any() and (cnt >= 0).all(), (what, cnt)
    for i in range(n):
        assert (ids[i, cnt[i]:] == 0).all() and (sc[i, cnt[i]:].view(np.uint32) == 0).all(), f"{what} padding of q{i}"


def filtered_parity(cs, full, qs, tqs, npa, what):
    conds = filter_cases()
    for name, prm in param_cases(npa):
        want = full.search_batch(qs, prm, filters=conds)
        same_all(cs.search_batch(qs, prm, filters=conds), want, f"{what} search_batch(filters) {name}")
        assert want[4].passage_ids.size == 0 and want[0].passage_ids.size > 0 and want[5].passage_ids.size > 0
    n = min(len(tqs), len(conds))
    for k in (10, 1024):
        same_all(cs.text_search(tqs[:n], k, filters=conds[:n]), full.text_search(tqs[:n], k, filters=conds[:n]),
                 f"{what} text_search(filters) k={k}")


def hybrid_parity(cs, full, qs, npa, what):
    texts = hybrid_texts()
    p = npa.SearchParameters(n_full_scores=128, top_k=7, n_ivf_probe=4)
    scopes = [{}, {"subsets": subset_cases(len(qs))[1]}, {"filters": filter_cases()}]
    n_hits = 0
    for fusion in ("relative_score", "rrf"):
        for alpha in (0.75, 0.5):
            for scope in scopes:
                want = full.search_hybrid(qs, texts, p, alpha=alpha, fusion=fusion, fetch_k=15, **scope)
                same_all(cs.search_hybrid(qs, texts, p, alpha=alpha, fusion=fusion, fetch_k=15, **scope), want,
                         f"{what} search_hybrid {fusion} {alpha} {list(scope)}")
                n_hits += sum(r.passage_ids.size for r in want)
    assert n_hits > 0


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
        from next_plaid_amd import text as T
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            spec, a, data, rs, qs, tqs, rows = fixtures()
            full = hip_index(a)
            full.set_text(data)
            full.set_columns(rows, text_on_device=["s"])
            shard = hip_index(a, shard_rank=rank, shard_count=world)
            shard.set_columns(rows, text_on_device=["s"])
            bad = world - 1
            prm = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=4)
            if mode == "parity":
                shard.set_text_shard(data)
                for deferred in (False, True):
                    comm = ShardComm(shard, rank, world, all_gather=gloo_all_gather(), deferred_status=deferred)
                    cs = CShardedSearcher(shard, comm)
                    what = f"G={world} rank {rank} deferred={deferred}:"
                    keyword_parity(cs, full, rs, tqs, what)
                    padding_check(cs, tqs, what)
                    if not deferred:   # 300 queries at top_k 1024: two exchanges (np_dist_plan.h cuts by B and top_k alone)
                        many = [tqs[i % len(tqs)] for i in range(300)]
                        same_all(cs.text_search(many, 1024), full.text_search(many, 1024), what + " two exchanges")
                    filtered_parity(cs, full, qs, tqs, npa, what)
                    hybrid_parity(cs, full, qs, npa, what)
                    assert comm.status() == (-1, 0)
                    comm.close()
            elif mode == "failure":   # the last rank never calls set_text_shard: an argument-level failure of that rank alone
                if rank != bad:
                    shard.set_text_shard(data)
                shard.text = data     # (the vocabulary, so that every rank compiles the same strings)
                phrase, single = tqs[3], tqs[0]
                assert len(phrase.phrases()[0]) == 2 and len(single.phrases()[0]) == 1
                for deferred in (False, True):
                    comm = ShardComm(shard, rank, world, all_gather=gloo_all_gather(), deferred_status=deferred)
                    cs = CShardedSearcher(shard, comm)
                    for batch in ([phrase, single], [single]):      # with and without the counting exchange
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
                        if rank == bad:
                            with pytest.raises(ValueError, match="no keyword index"):
                                cs.text_search(batch, 10)
                            with pytest.raises(ValueError, match="no keyword index"):
                                cs.search_hybrid(qs[:2], batch[:1] * 2, prm)
                        else:
                            with pytest.raises(npa.SearchError, match=f"shard {bad} failed with status 8"):
                                cs.text_search(batch, 10)
                            with pytest.raises(npa.SearchError, match=f"shard {bad} failed with status 8"):
                                cs.search_hybrid(qs[:2], batch[:1] * 2, prm)
                    # the communicator serves the next batch: a semantic one every rank can take
                    same_all(cs.search_batch(qs, prm), full.search_batch(qs, prm), f"rank {rank}: the batch after the failures")
                    assert comm.status() == (-1, 0)
                    comm.close()
                # ranks that were handed different tables: an argument error on every rank, then a healthy batch
                shard.set_text_shard(dataclasses.replace(data, n_rows=data.n_rows + 1) if rank == bad else data)
                for deferred in (False, True):
                    comm = ShardComm(shard, rank, world, all_gather=gloo_all_gather(), deferred_status=deferred)
                    cs = CShardedSearcher(shard, comm)
                    with pytest.raises(ValueError, match="different nRow"):
                        cs.text_search([phrase, single], 10)
                    same_all(cs.search_batch(qs, prm), full.search_batch(qs, prm), f"rank {rank}: the batch after the mismatch")
                    comm.close()
                shard.set_text_shard(data)
                comm = ShardComm(shard, rank, world, all_gather=gloo_all_gather())
                cs = CShardedSearcher(shard, comm)
                same_all(cs.text_search([phrase, single], 10), full.text_search([phrase, single], 10), f"rank {rank}: the table set again")
                comm.close()
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
    import multiprocessing as mp
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
