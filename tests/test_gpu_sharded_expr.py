"""Tree keyword queries (np_text_expr) on a document-sharded index and on device buffers: np_hip_text_search_sharded_expr,
np_hip_text_search_sharded_expr_filtered, np_hip_search_hybrid_sharded_expr through dist.CShardedSearcher, and
np_hip_text_search_expr_device.  Needs a real MI355X.

G = 2 and 3 ranks are spawned processes that share GPU 0 and exchange over the hosted transport (tests/sharded_expr_ranks.py).
Every result is compared with the unsharded handle's _expr call, bit for bit, and the keyword results with the restatement too
(tests/shard_text_expr_restate.py, whose CPU test shows that this corpus can see a shard's own prefix count, a prefix count
taken as the sum of document frequencies, a shard's own count of a phrase that ends in a prefix, a shard's own nRow and
average length, a merge on f32 scores and a merge without the id tie-break).  About 9 000 documents: a 2-rank shard spans two
slices of 4096 documents and no shard boundary is a slice's."""
import ctypes as C

import numpy as np
import pytest

from helpers import hip_index

import next_plaid_amd as npa
from next_plaid_amd import api, text as T
from next_plaid_amd.dist import CShardedSearcher, ShardComm
import sharded_expr_ranks as H
from sharded_hybrid_ranks import same_all

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return H.fixtures()


def open_one_rank(a, data, rows, **opts):
    hx = hip_index(a, **opts)
    hx.set_columns(rows)
    hx.set_text_shard(data)      # (on an unsharded handle this is set_text)
    comm = ShardComm(hx, 0, 1, rccl=False)
    assert comm.info()["transport"] == "local"
    return hx, comm, CShardedSearcher(hx, comm)


@pytest.mark.parametrize("G", [2, 3])
def test_sharded_tree_results_equal_the_unsharded_handle(G):
    """Keyword parity (every class of the CPU fixture, a query of 64 phrases and 127 nodes, prefixes of no, one and every term;
    top_k 1, 10, 1024; no scope and per-query subsets with an empty one and ids outside the range), a flat batch lifted to
    trees against the flat sharded entry, 300 queries at top_k 1024 in two exchanges against one, filters, and the hybrid
    request (both fusions, alpha 0.75 and 0.5; no scope, subsets, filters), host-checked and with deferred status.  Rank 0
    runs every batch in chunks of five queries while its peers run one chunk: the exchanges do not depend on a rank's plan."""
    H.run_ranks(G, "parity")


def test_one_failing_rank_blocks_nobody():
    """The last rank holds no keyword index: with a tree batch it returns its own error, host-checked peers return 'shard r
    failed', under deferred_status every count is -1 and comm.status() names the rank; the hybrid call behaves alike, with and
    without the counting exchange; a following flat batch and a tree batch on the same communicator are correct."""
    H.run_ranks(2, "failure")


def test_one_rank_communicator_equals_the_plain_calls(fx):
    """Over a one-rank communicator (NP_COMM_LOCAL: the whole protocol, no collective) the sharded _expr calls equal the plain
    _expr calls and the restatement: keyword, lifted, filtered and hybrid."""
    n, spec, a, data, rs, qs, exprs, flat, rows = fx
    hx, comm, cs = open_one_rank(a, data, rows)
    try:
        H.keyword_parity(cs, hx, rs, exprs, n, "one rank:")
        H.lifted_parity(cs, flat, "one rank:")
        H.filtered_parity(cs, hx, exprs, n, "one rank:")
        H.hybrid_parity(cs, hx, qs, exprs, n, npa, "one rank:")
        assert cs.text_search(["", "lef* NOT lefb"], 5, full_grammar=True)[0].passage_ids.size == 0
        with pytest.raises(ValueError, match="top_k"):
            cs.text_search(exprs[:1], 1025)
        assert comm.status() == (-1, 0)
        comm.close()
    finally:
        hx.close()


def test_a_one_chunk_and_a_multi_chunk_plan_give_the_same_bytes(fx):
    """300 queries with prefix phrases at top_k 1024 (two list exchanges) on a handle that runs 64 queries per chunk and on one
    that runs two -- 150 chunks, and a counting pre-pass that needs several groups of bitmaps for the batch's prefix phrases:
    the plain call's bytes on both, and the first 255 queries alone (one exchange) return their part of them."""
    n, spec, a, data, rs, qs, exprs, flat, rows = fx
    many = H.many_queries([e for e in exprs if any(r is not None for r in e.prefix)][:12])
    want = None
    for opts in ({}, {"max_batch": 2}):
        hx, comm, cs = open_one_rank(a, data, rows, **opts)
        try:
            if want is None:
                want = hx.text_search(many, 1024)
                assert max(r.passage_ids.size for r in want) == 1024
                same_all(cs.text_search(many[:255], 1024), want[:255], "one exchange")
            same_all(cs.text_search(many, 1024), want, f"300 queries at top_k 1024 {opts}")
            same_all(cs.text_search(exprs, 10), hx.text_search(exprs, 10), f"the special queries {opts}")
            assert comm.status() == (-1, 0)
            comm.close()
        finally:
            hx.close()


def device_call(hx, exprs, k, subsets=None, stream=None, out=None):
    """np_hip_text_search_expr_device on torch tensors: (np_status, ids, scores, counts) on the host."""
    import torch
    n = len(exprs)
    tq = api._CTextExprs(list(exprs))
    sub = (None, None, None, 0, None)
    keep = []
    if subsets is not None:
        sid, soff, qsub = api.pack_subsets(subsets, n)
        keep = [torch.from_numpy(x).cuda() for x in (sid, soff, qsub)]
        sub = (C.c_void_p(keep[0].data_ptr()) if keep[0].numel() else None, C.c_void_p(keep[1].data_ptr()),
               soff.ctypes.data_as(C.c_void_p), soff.size - 1, C.c_void_p(keep[2].data_ptr()))
    if out is None:
        out = (torch.full((n, k), 7, dtype=torch.int64, device="cuda"), torch.full((n, k), 7.0, dtype=torch.float32, device="cuda"),
               torch.full((n,), 7, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    s = torch.cuda.Stream() if stream is None else stream
    rc = api.lib().np_hip_text_search_expr_device(hx._h, tq.arr, n, k, *sub, *(None if o is None else C.c_void_p(o.data_ptr()) for o in out),
                                                  C.c_void_p(s.cuda_stream))
    s.synchronize()
    return (rc,) + tuple(None if o is None else o.cpu().numpy() for o in out)


def rows_equal(ids, sc, cnt, want, what):
    for i, r in enumerate(want):
        assert cnt[i] == r.passage_ids.size and ids[i, : cnt[i]].tolist() == r.passage_ids.tolist(), f"{what} q{i}"
        assert sc[i, : cnt[i]].view(np.uint32).tolist() == r.scores.view(np.uint32).tolist(), f"{what} q{i}"
        assert not ids[i, cnt[i]:].any() and not sc[i, cnt[i]:].view(np.uint32).any(), f"{what} q{i}: padding"


def test_the_device_entry_equals_the_host_entry(fx):
    """np_hip_text_search_expr_device: the host entry's bytes in device buffers, with and without subsets, for a query alone
    and in a batch, under a plan of two queries per chunk; NULL buffers and a top_k over the limit are refused by name."""
    n, spec, a, data, rs, qs, exprs, flat, rows = fx
    subsets = H.subset_cases(n, len(exprs))
    hx = hip_index(a)
    try:
        hx.set_text(data)
        want = {(k, s is not None): hx.text_search(exprs, k, subsets=s) for k in (10, 1024) for s in (None, subsets)}
        for (k, scoped), w in want.items():
            rc, ids, sc, cnt = device_call(hx, exprs, k, subsets if scoped else None)
            assert rc == 0, api.last_error()
            rows_equal(ids, sc, cnt, w, f"k={k} subsets={scoped}")
        for i in (0, 2, 6, len(exprs) - 2):      # batch-independent
            rc, ids, sc, cnt = device_call(hx, [exprs[i]], 10)
            assert rc == 0
            rows_equal(ids, sc, cnt, [want[(10, False)][i]], f"query {i} alone")
        import torch
        ok = (torch.zeros((1, 10), dtype=torch.int64, device="cuda"), torch.zeros((1, 10), dtype=torch.float32, device="cuda"),
              torch.zeros(1, dtype=torch.int32, device="cuda"))
        for hole in range(3):
            rc = device_call(hx, exprs[:1], 10, out=tuple(None if j == hole else o for j, o in enumerate(ok)))[0]
            assert rc == 8 and "NULL buffer" in api.last_error(), (hole, rc, api.last_error())
        rc = device_call(hx, exprs[:1], T.NP_TEXT_MAX_TOPK + 1)[0]
        assert rc == 8 and "top_k must be in 1..1024" in api.last_error()
    finally:
        hx.close()
    hx = hip_index(a, max_batch=2)      # chunk-independent: a synchronisation per chunk that holds a prefix phrase
    try:
        hx.set_text(data)
        rc, ids, sc, cnt = device_call(hx, exprs, 10, subsets)
        assert rc == 0
        rows_equal(ids, sc, cnt, want[(10, True)], "two queries per chunk")
    finally:
        hx.close()
