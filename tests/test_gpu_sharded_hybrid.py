"""Keyword, filtered and hybrid search on a document-sharded index: np_hip_index_set_text_shard, np_hip_text_search_sharded,
np_hip_search_batch_sharded_filtered, np_hip_search_hybrid_sharded through dist.CShardedSearcher.  Needs a real MI355X.

G = 2 and 3 ranks are spawned processes that share GPU 0 and exchange over the hosted transport (tests/sharded_hybrid_ranks.py);
everything around the collective is the code the RCCL transport runs.  Every result is compared with the unsharded handle's, bit
for bit, and the keyword results with the restatement too (tests/shard_text_restate.py, whose CPU test shows that this corpus
and these filters can see a shard's own nRow, average length, document frequency, phrase hit count, a merge on f32 scores, a
merge without the id tie-break, a dropped short list and a local subset length)."""
import numpy as np
import pytest

from helpers import hip_index

import next_plaid_amd as npa
from next_plaid_amd.dist import CShardedSearcher, ShardComm
import sharded_hybrid_ranks as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("G", [2, 3])
def test_sharded_results_equal_the_unsharded_handle(G):
    """Keyword parity (OR / AND, single- and multi-token phrases, an unknown term, terms on one shard only, a phrase that matches
    nowhere; top_k 1, 10, 1024; no subsets, per-query subsets with an empty one and with ids outside the range and duplicates),
    filtered parity (dense, no threshold at precision 0, batched probe; spread filters, 1=1, nothing anywhere, nothing on the last
    shard, REGEXP, queries without a filter; the same filters through text_search) and hybrid parity (both fusions, alpha 0.75 and
    0.5, fetch_k 15; no scope, subsets, filters), host-checked and with deferred status; comm.status() stays (-1, 0)."""
    H.run_ranks(G, "parity")


def test_one_failing_rank_blocks_nobody():
    """The last rank holds no keyword index: it returns its own error, host-checked peers return 'shard r failed', under
    deferred_status every count is -1 and comm.status() names the rank; the hybrid call behaves alike; a following semantic batch on
    the same communicator is correct.  Ranks handed tables with different n_rows all get a ValueError."""
    H.run_ranks(2, "failure")


def test_one_rank_communicator_equals_the_plain_calls():
    """On an unsharded handle set_text_shard is set_text, and the sharded calls over a one-rank communicator (NP_COMM_LOCAL: the
    whole protocol, no collective) equal the plain calls."""
    spec, a, data, rs, qs, tqs, rows = H.fixtures()
    hx = hip_index(a)
    try:
        hx.set_columns(rows, text_on_device=["s"])
        before = hx.info.device_bytes
        hx.set_text_shard(data)
        assert hx.info.device_bytes > before
        comm = ShardComm(hx, 0, 1, rccl=False)
        assert comm.info()["transport"] == "local"
        cs = CShardedSearcher(hx, comm)
        H.keyword_parity(cs, hx, rs, tqs, "one rank:")
        H.padding_check(cs, tqs, "one rank:")
        H.filtered_parity(cs, hx, qs, tqs, npa, "one rank:")
        H.hybrid_parity(cs, hx, qs, npa, "one rank:")
        assert cs.text_search(["", "wo1"], 5)[0].passage_ids.size == 0
        assert comm.status() == (-1, 0)
        with pytest.raises(ValueError, match="top_k"):
            cs.text_search(tqs[:1], 1025)
        comm.close()
        hx.set_text_shard(None)
        assert hx.info.device_bytes == before
    finally:
        hx.close()


def test_a_batch_in_several_exchanges_equals_one():
    """255 queries at top_k 1024 fit one exchange, 300 take two (np_dist_plan.h cuts by B and top_k alone): the same results,
    query by query, on a one-rank communicator and against the plain call."""
    spec, a, data, rs, qs, tqs, rows = H.fixtures()
    hx = hip_index(a)
    try:
        hx.set_text_shard(data)
        comm = ShardComm(hx, 0, 1, rccl=False)
        cs = CShardedSearcher(hx, comm)
        many = [tqs[i % len(tqs)] for i in range(300)]
        got = cs.text_search(many, 1024)
        H.same_all(got, hx.text_search(many, 1024), "300 queries at top_k 1024")
        H.same_all(got[:255], cs.text_search(many[:255], 1024), "one exchange")
        comm.close()
    finally:
        hx.close()
