"""The hot filter level's packed block staging (approx_hotp_kernel) at every block stride.  Needs a real MI355X.

A candidate's distinct-code block travels to an LDS row of stride + 16 bytes, 16 bytes per lane.  The lane of a row's 16
padding bytes issues no memory request (an out-of-range offset: zeros), so a block costs the 128-byte lines it occupies and
not one more; the other lanes, the LDS rows and everything read from them are as before.  One corpus per stride class
(64, 128, 192, 256 and 512 bytes of u16 codes, 256 bytes of u32 codes) covers every documents-per-instruction form
(4 / 2 / 1) with 2 and 4 lanes per document and both hot-queue forms.  For each, the two-level filter must select the
unfiltered path's documents, order and exact scores bit for bit, and agree with the oracle.

The stride a corpus opens with is not reported by the library: it is derived here from the per-document distinct-code counts
by choose_ublock_stride's rule and asserted, so that a generator change cannot silently move a case to another class.
"""
import numpy as np
import pytest

from append_restate import host_stride_bytes   # choose_ublock_stride's rule
from helpers import RTOL_F32, assert_ranking_close, hip_index, make_arrays, oracle_index, synth, to_oracle_params

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu

CASES = {
    # name: (generator arguments, code bytes, expected stride in bytes, n_ivf_probe, lanes per document the stride allows,
    #        shortest run of consecutive candidate ids the full-length queries must produce)
    # u16 codes, K small against 32 x 128 probed cells: practically every document is a candidate of a 32-token query, so
    # whole claims (32 or 16 candidates) have adjacent blocks -- a run of 63 ids holds a whole claim wherever the claims start
    "u16_64B": (dict(num_docs=12000, num_centroids=1024, doc_len_min=8, doc_len_max=20, rand256=51, seed=101), 2, 64, 128, (2, 4), 63),
    "u16_128B": (dict(num_docs=12000, num_centroids=2048, doc_len_min=30, doc_len_max=60, rand256=128, seed=102), 2, 128, 128, (2, 4), 63),
    "u16_192B": (dict(num_docs=12000, num_centroids=4096, doc_len_min=60, doc_len_max=100, rand256=160, seed=103), 2, 192, 128, (2, 4), 63),
    "u16_256B": (dict(num_docs=12000, num_centroids=4096, doc_len_min=90, doc_len_max=130, rand256=200, seed=104), 2, 256, 128, (2, 4), 63),
    # blocks above 256 bytes take 4 lanes per document whatever the knob; ~70 lists of this corpus overflow their block
    "u16_512B": (dict(num_docs=10000, num_centroids=4096, doc_len_min=230, doc_len_max=280, rand256=220, seed=105), 2, 512, 128, (4,), 63),
    # u32 codes (K > 65536): 4096 probed cells are 3 % of K, about two documents in three are candidates -- adjacent pairs
    # (the neighbour whose first line the padding lane used to fetch), not whole adjacent claims
    "u32_256B": (dict(num_docs=4000, num_centroids=131072, doc_len_min=40, doc_len_max=70, rand256=128, seed=106), 4, 256, 128, (2, 4), 2),
}


def P(**kw):
    return npa.SearchParameters(**kw)


def check_trace(hx, ox, q, p, what=""):
    """Stage-by-stage comparison for one query (as in test_gpu_parity.py)."""
    tr = hx.debug_trace(q, p)
    t = ox.search(q, to_oracle_params(p), trace=True).trace
    assert np.array_equal(tr["cells"], t.cells), f"{what}: S2 cells differ"
    assert np.array_equal(tr["cand"], t.cand), f"{what}: S3 candidates differ ({tr['cand'].size} vs {t.cand.size})"
    bad = np.nonzero(tr["approx"].view(np.uint32) != t.approx.view(np.uint32))[0]
    assert bad.size == 0, f"{what}: S4 approx not bit-exact at {bad[:5]}"
    assert np.array_equal(tr["sel"], t.sel), f"{what}: S5 selection/order differs"
    tol = RTOL_F32 * np.maximum(np.abs(t.sel_exact), 1.0)
    assert np.all(np.abs(tr["sel_exact"] - t.sel_exact) <= tol), f"{what}: S6 exact scores differ"
    return tr


def query_of_document(spec, a, doc, n_tokens):
    """A query made of the first tokens of one document (its own reconstructed embeddings): the document's cells are probed."""
    codes, res, lens = synth.doc_tokens(spec, doc, doc + 1)
    pick = np.arange(n_tokens) % int(lens[0])
    return synth.reconstruct(codes[pick], res[pick], a["centroids"], a["bucket_weights"], spec.nbits)


def longest_run(ids):
    ids = np.asarray(ids, np.int64)
    brk = np.nonzero(np.diff(ids) != 1)[0]
    edges = np.concatenate([[-1], brk, [ids.size - 1]])
    return int(np.diff(edges).max())


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def corpus(request):
    kw, code_bytes, want_stride, nprobe, lpds, min_run = CASES[request.param]
    spec, a = make_arrays(dim=128, nbits=4, **kw)
    stride, n_overflow = host_stride_bytes(a, code_bytes)
    assert (a["centroids"].shape[0] > 65536) == (code_bytes == 4)
    assert stride == want_stride, f"{request.param}: the corpus opens with a {stride}-byte stride, not {want_stride}"
    assert n_overflow <= spec.num_docs // 100
    hx = hip_index(a)
    ox = oracle_index(a)
    qs, src = synth.make_queries(spec, 8, n_tokens=32, cen=a["centroids"])
    last = query_of_document(spec, a, spec.num_docs - 1, 32)
    # six plain queries, the last document's own, one ragged, one single-token
    batch = list(qs[:6]) + [last, qs[6][:7], qs[7][:1]]
    p = P(n_full_scores=128, top_k=32, n_ivf_probe=nprobe, centroid_score_threshold=None)
    # the zeroth level off: every candidate of the posting-list union reaches the hot level, in ascending id order
    hx.tune("s3_gain", 0)
    hx.tune("s4_filter", 0)
    ref = hx.search_batch(batch, p)          # the unfiltered path, computed once for every test of the corpus
    n_union = hx.last_stats["n_candidates"]  # the batch's posting-list unions
    ref_one = hx.search_batch([last], p)
    hx.tune("s4_filter", 1)
    yield dict(name=request.param, spec=spec, a=a, hx=hx, ox=ox, batch=batch, last=last, p=p, ref=ref, ref_one=ref_one,
               lpds=lpds, min_run=min_run, n_union=n_union)
    hx.close()


def test_candidates_reach_the_staging_edges(corpus):
    """What the queries were chosen for: candidates of odd and even ids, of the last document (nothing lies behind its block but
    the overflow region or the end of the allocation), and runs of consecutive ids (blocks adjacent in memory)."""
    c = corpus
    n = c["spec"].num_docs
    cand = np.asarray(c["hx"].debug_trace(c["last"], c["p"])["cand"], np.int64)
    assert cand.size > n // 2, (cand.size, n)                       # most documents
    assert cand[-1] == n - 1 and np.all(np.diff(cand) > 0)
    assert np.any(cand % 2 == 0) and np.any(cand % 2 == 1)
    assert longest_run(cand) >= c["min_run"], (longest_run(cand), c["min_run"])


def test_two_level_filter_is_bit_equal_to_the_unfiltered_path(corpus):
    """s4_filter 0 against the two-level filter in plane form, 10 % hot: 2 and 4 lanes per document where the stride allows,
    both hot-queue forms, the whole batch and a batch of one.  One more configuration per corpus has the zeroth level hand the
    hot level its candidates (blocks of ascending ids in any order: block offsets from the claim's smallest id)."""
    c = corpus
    hx, p = c["hx"], c["p"]
    hx.tune("s4_hot", 100)
    hx.tune("s4_planes", 1)
    try:
        for gain, lpd, qm in [(0, lpd, qm) for lpd in c["lpds"] for qm in (0, 1)] + [(2, c["lpds"][0], 1)]:
            hx.tune("s3_gain", gain)
            hx.tune("s4_lpd", lpd)
            hx.tune("s4_qm", qm)
            what = f"{c['name']} lpd={lpd} qm={qm} gain={gain}"
            got = hx.search_batch(c["batch"], p)
            st = dict(hx.last_stats)
            for i, (g, r) in enumerate(zip(got, c["ref"])):
                assert np.array_equal(g.passage_ids, r.passage_ids), f"{what} q{i}: selected set / order changed"
                assert np.array_equal(g.scores, r.scores), f"{what} q{i}: scores changed"
            assert st["n_candidates"] == c["n_union"], (what, st)
            if gain == 0:
                assert 0 < st["n_level2"] < st["n_candidates"], (what, st)      # the hot level ran and pruned
            else:   # (n_level2 then also counts the exact bounds of the zeroth level's own list: no bound on it here)
                assert 0 < st["n_level0"] <= st["n_candidates"] and st["n_level2"] > 0, (what, st)
            one = hx.search_batch([c["last"]], p)                            # a batch of one
            assert np.array_equal(one[0].passage_ids, c["ref_one"][0].passage_ids), f"{what}: batch of one"
            assert np.array_equal(one[0].scores, c["ref_one"][0].scores), f"{what}: batch of one"
    finally:
        hx.tune("s3_gain", 0)


def test_filtered_search_matches_the_oracle(corpus):
    c = corpus
    hx, ox, p = c["hx"], c["ox"], c["p"]
    hx.tune("s3_gain", 0)
    hx.tune("s4_hot", 100)
    hx.tune("s4_planes", 1)
    hx.tune("s4_lpd", c["lpds"][0])
    hx.tune("s4_qm", 1)
    got = hx.search_batch(c["batch"], p)
    assert 0 < hx.last_stats["n_level2"] < hx.last_stats["n_candidates"]
    for i, (g, o) in enumerate(zip(got, ox.search_batch(c["batch"], to_oracle_params(p)))):
        assert_ranking_close(g.passage_ids, g.scores, o.passage_ids, o.scores, RTOL_F32, f"{c['name']} q{i}")
    check_trace(hx, ox, c["last"], p, what=f"{c['name']} last document's query")
    check_trace(hx, ox, c["batch"][7], p, what=f"{c['name']} ragged query")
