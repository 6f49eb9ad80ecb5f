"""Posting lists that do not state the codes exactly, against the oracle.  Needs a real MI355X.

The crate writes ivf.npy as exactly the (document, distinct code) pairs (index.rs:479-504), but the reference only uses the
lists to form the candidate set (index.rs:1142-1156: concatenate, sort, dedup) and scores from the codes, so ANY lists give a
defined answer.  The zeroth filter level (gain_sweep_kernel) bounds a document's approximate score by the gains of the probed
cells whose lists hold it: that is a bound only if every (d, c in codes(d)) pair is in list c.  Each case below opens a
perturbed copy of one corpus with the HIP path and with the oracle (the same perturbed arrays) and compares them under the
default knobs (s3_gain = 1, the run / skip policy), with the level forced whenever it applies (s3_gain = 2), and with the level
off (s3_gain = 0); and it asserts the gate at open: with s3_gain = 2 and no threshold the level runs iff the lists ascend and
cover the shard's codes (level_may_run below).
"""
import numpy as np
import pytest

from helpers import RTOL_F32, assert_ranking_close, hip_index, make_arrays, oracle_index, synth, to_oracle_params

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu

REGIMES = ((None, 8), (None, 32), (0.4, 32))   # (centroid_score_threshold, n_ivf_probe)
GAINS = (1, 2, 0)                              # s3_gain: default (run / skip policy), whenever it applies, off
S4_DEFAULTS = (("s4_mode", 4), ("s4_minb", 8), ("s4_filter", 1), ("s4_swz", 1), ("s3_gain", 1))


def P(thr, nprobe, **kw):
    kw.setdefault("n_full_scores", 256)
    kw.setdefault("top_k", 10)
    return npa.SearchParameters(n_ivf_probe=nprobe, centroid_score_threshold=thr, **kw)


# ---- posting-list perturbations (host numpy) ---------------------------------------------------------------------------

def list_entries(a):
    """(cell, document) of every posting-list entry, in file order."""
    lens = np.asarray(a["ivf_lengths"], np.int64)
    return np.repeat(np.arange(lens.size, dtype=np.int64), lens), np.asarray(a["ivf"], np.int64)


def with_lists(a, cells, docs):
    """A copy of `a` whose posting lists hold exactly the given (cell, document) entries, every list in ascending id order
    (duplicate entries kept, so such a list does not strictly ascend)."""
    cells, docs = np.asarray(cells, np.int64), np.asarray(docs, np.int64)
    o = np.lexsort((docs, cells))
    b = dict(a)
    b["ivf"] = np.ascontiguousarray(docs[o])
    b["ivf_lengths"] = np.bincount(cells, minlength=a["centroids"].shape[0]).astype(np.int32)
    return b


def doc_codes(a, d):
    off = int(np.asarray(a["doc_lengths"], np.int64)[:d].sum())
    return np.unique(np.asarray(a["codes"])[off:off + int(a["doc_lengths"][d])])


def code_pairs(a):
    """code * N + document for every distinct (document, code) pair of the codes, sorted."""
    lens = np.asarray(a["doc_lengths"], np.int64)
    n = max(lens.size, 1)
    return np.unique(np.asarray(a["codes"], np.int64) * n + np.repeat(np.arange(lens.size, dtype=np.int64), lens))


def ivf_covers_codes(a, shard=None):
    """Every (d, distinct c) pair of the shard's documents [lo, hi) is an entry of list c."""
    n = max(np.asarray(a["doc_lengths"]).size, 1)
    lo, hi = (0, n) if shard is None else shard
    want = code_pairs(a)
    want = want[(want % n >= lo) & (want % n < hi)]
    c, d = list_entries(a)
    return bool(np.isin(want, c * n + d).all())


def lists_ascend(a):
    """Every list strictly ascends (what open checks over the whole file before it restricts the lists to a shard)."""
    c, d = list_entries(a)
    same = c[1:] == c[:-1]
    return bool((d[1:][same] > d[:-1][same]).all())


def level_may_run(a, shard=None):
    return lists_ascend(a) and ivf_covers_codes(a, shard)


def drop_pairs(a, keep):
    """keep = {document: cells}: the document leaves every list except those of the given cells."""
    c, d = list_entries(a)
    n = max(np.asarray(a["doc_lengths"]).size, 1)
    drop = [cc * n + doc for doc, cells in keep.items() for cc in np.setdiff1d(doc_codes(a, doc), list(cells))]
    m = ~np.isin(c * n + d, np.asarray(drop, np.int64))
    return with_lists(a, c[m], d[m])


def smallest_gain_cell(q, cen, cells, codes, nprobe):
    """Of the document's codes that the query probes, the one whose cell contributes least to the zeroth level's sum: gain
    sum_q max(0, QC[q, c] - theta_q) with theta_q the nprobe-th best centroid score of token q (ties: smallest score sum)."""
    probed = np.intersect1d(cells, codes)
    assert probed.size > 0, "a candidate holds a probed cell"
    QC = q.astype(np.float64) @ cen.astype(np.float64).T
    theta = -np.sort(-QC, axis=1)[:, nprobe - 1]
    gain = np.maximum(QC[:, probed] - theta[:, None], 0).sum(axis=0)
    return int(probed[np.lexsort((QC[:, probed].sum(axis=0), gain))[0]])


# ---- comparisons ---------------------------------------------------------------------------------------------------

def compare_trace(tr, r, what):
    """Stage by stage (check_trace of test_gpu_parity.py, against a precomputed oracle trace)."""
    t = r.trace
    assert np.array_equal(tr["cells"], t.cells), f"{what}: S2 cells differ"
    assert np.array_equal(tr["cand"], t.cand), f"{what}: S3 candidates differ ({tr['cand'].size} vs {t.cand.size})"
    bad = np.nonzero(tr["approx"].view(np.uint32) != t.approx.view(np.uint32))[0]
    assert bad.size == 0, f"{what}: S4 approx not bit-exact at {bad[:5]}: {tr['approx'][bad[:5]]} vs {t.approx[bad[:5]]}"
    assert np.array_equal(tr["sel"], t.sel), f"{what}: S5 selection/order differs"
    tol = RTOL_F32 * np.maximum(np.abs(t.sel_exact), 1.0)
    assert np.all(np.abs(tr["sel_exact"] - t.sel_exact) <= tol), f"{what}: S6 exact scores differ"


def compare_index(hx, ox, batch, traced, may_run, what, regimes=REGIMES, shard_handles=()):
    """hx against ox for every regime and s3_gain setting; the gate: with s3_gain = 2 and no threshold the level runs iff
    may_run (and never with s3_gain = 0).  shard_handles = [(handle, may_run of its shard)]: each shard's own gate."""
    for thr, nprobe in regimes:
        p = P(thr, nprobe)
        op = to_oracle_params(p)
        ref = ox.search_batch(batch, op)
        otr = [ox.search(q, op, trace=True) for q in traced]
        for gain in GAINS:
            hx.tune("s3_gain", gain)
            got = hx.search_batch(batch, p)
            st = dict(hx.last_stats)
            tag = f"{what} thr={thr} nprobe={nprobe} s3_gain={gain}"
            for i, (g, o) in enumerate(zip(got, ref)):
                assert_ranking_close(g.passage_ids, g.scores, o.passage_ids, o.scores, RTOL_F32, f"{tag} q{i}")
            if gain == 0:
                assert st["n_level0"] == 0, (tag, st)
            elif gain == 2 and thr is None:
                assert (st["n_level0"] > 0) == may_run, (tag, st, may_run)
            for j, (q, o) in enumerate(zip(traced, otr)):
                compare_trace(hx.debug_trace(q, p), o, f"{tag} trace q{j}")
            for s, s_may in shard_handles:
                s.tune("s3_gain", gain)
                if gain == 2 and thr is None:
                    s.search_batch(batch, p)
                    assert (s.last_stats["n_level0"] > 0) == s_may, (tag, "shard", s.info.shard_doc_begin, s_may)
        hx.tune("s3_gain", 1)
    for s, _ in shard_handles:
        s.tune("s3_gain", 1)


def open_both(a, **opts):
    return hip_index(a, **opts), oracle_index(a)


# ---- the corpus ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus():
    """~100 k documents: four 32768-document ranges of the level's table; K = 4096, dim 128, nbits 4."""
    spec, a = make_arrays(num_docs=100000, num_centroids=4096, dim=128, nbits=4, doc_len_min=30, doc_len_max=70, seed=131)
    qs, src = synth.make_queries(spec, 34, n_tokens=32, cen=a["centroids"])
    batch = list(qs[:32]) + [qs[32][:7], qs[33][:1]]
    ox = oracle_index(a)
    op = to_oracle_params(P(None, 8))
    top = [ox.search(q, op, trace=True) for q in qs[:32]]
    assert level_may_run(a)
    return dict(spec=spec, a=a, qs=qs, batch=batch, traced=[qs[0], qs[1], qs[32][:7]], top=top)


def missing_pair_victims(C, queries, pick=lambda d: True, per_query=3):
    """For each query: its oracle top documents (unperturbed index, no threshold, nprobe 8), each keeping only the probed
    cell with the smallest gain of its codes -- still a candidate with an unchanged score, but its zeroth-level sum drops."""
    a, qs = C["a"], C["qs"]
    keep = {}
    for i in queries:
        r = C["top"][i]
        for d in [int(x) for x in r.passage_ids if pick(int(x))][:per_query]:
            keep.setdefault(d, set()).add(smallest_gain_cell(qs[i], a["centroids"], r.trace.cells, doc_codes(a, d), 8))
    return keep


def assert_still_top(b, C, keep, queries):
    """The construction's premise: on the perturbed index the victims are still in the oracle's top-k of their queries."""
    ox = oracle_index(b)
    op = to_oracle_params(P(None, 8))
    for i in queries:
        ids = ox.search(C["qs"][i], op).passage_ids
        for d in C["top"][i].passage_ids[:3]:
            if int(d) in keep:
                assert int(d) in ids, f"q{i}: victim {d} left the oracle's top-k {ids}"
    return ox


# ---- cases ---------------------------------------------------------------------------------------------------------

def test_missing_pairs(corpus):
    """A document that misses from lists of its codes but stays a candidate through one probed cell: the reference still
    scores it from its codes; the zeroth level, summing only the gains of the lists that hold it, would prune it."""
    C = corpus
    keep = missing_pair_victims(C, range(8))
    b = drop_pairs(C["a"], keep)
    assert not ivf_covers_codes(b) and lists_ascend(b)
    ox = assert_still_top(b, C, keep, range(8))
    hx = hip_index(b)
    try:
        compare_index(hx, ox, C["batch"], C["traced"], False, "missing pairs")
    finally:
        hx.close()


def test_swap_keeps_list_sizes(corpus):
    """One true pair dropped and one false pair added in the same list: ivf_size and every list length unchanged, so only a
    membership check tells this index from a canonical one."""
    C = corpus
    a = C["a"]
    c, d = list_entries(a)
    r = C["top"][0]
    victim = int(r.passage_ids[0])
    cell = smallest_gain_cell(C["qs"][0], a["centroids"], r.trace.cells, doc_codes(a, victim), 8)
    # the victim keeps its smallest-gain probed cell; it leaves the list of another of its probed cells, whose slot goes
    # to a document that holds no code in that cell
    other = [int(x) for x in np.intersect1d(r.trace.cells, doc_codes(a, victim)) if int(x) != cell]
    assert other, "the victim holds two probed cells"
    c_sw = other[0]
    members = set(d[c == c_sw].tolist())
    intruder = next(x for x in range(a["doc_lengths"].size) if x not in members)
    m = ~((c == c_sw) & (d == victim))
    b = with_lists(a, np.append(c[m], c_sw), np.append(d[m], intruder))
    assert b["ivf"].size == a["ivf"].size and np.array_equal(b["ivf_lengths"], a["ivf_lengths"])
    assert not ivf_covers_codes(b) and lists_ascend(b)
    hx, ox = open_both(b)
    try:
        compare_index(hx, ox, C["batch"], C["traced"], False, "swap")
    finally:
        hx.close()


def test_extra_pairs_keep_the_level(corpus):
    """Documents added to lists of probed cells they hold no code in: the reference makes them candidates, the bound only
    loosens, so the level still runs -- and the results still equal the oracle's."""
    C = corpus
    a = C["a"]
    rng = np.random.default_rng(5)
    c, d = list_entries(a)
    n = a["doc_lengths"].size
    have = set((c * n + d).tolist())
    add_c, add_d = [], []
    for i in range(4):
        for cell in rng.choice(C["top"][i].trace.cells, 6, replace=False):
            for doc in rng.choice(n, 300, replace=False):
                if int(cell) * n + int(doc) not in have:
                    have.add(int(cell) * n + int(doc))
                    add_c.append(int(cell))
                    add_d.append(int(doc))
    b = with_lists(a, np.append(c, add_c), np.append(d, add_d))
    assert level_may_run(b) and b["ivf"].size > a["ivf"].size + 5000
    hx, ox = open_both(b)
    try:
        compare_index(hx, ox, C["batch"], C["traced"], True, "extra pairs")
    finally:
        hx.close()


def test_duplicate_ids_take_the_full_sweep(corpus):
    """Ids repeated inside lists of probed cells: the reference dedups the candidates; the lists no longer strictly ascend,
    so the open takes the full sweep and the level does not run."""
    C = corpus
    a = C["a"]
    c, d = list_entries(a)
    rng = np.random.default_rng(6)
    cells = np.unique(np.concatenate([C["top"][i].trace.cells[:8] for i in range(4)]))
    dup = np.nonzero(np.isin(c, cells))[0]
    dup = rng.choice(dup, min(dup.size, 2000), replace=False)
    b = with_lists(a, np.append(c, c[dup]), np.append(d, d[dup]))
    assert ivf_covers_codes(b) and not lists_ascend(b)
    hx, ox = open_both(b)
    try:
        compare_index(hx, ox, C["batch"], C["traced"], False, "duplicates")
    finally:
        hx.close()


def test_empty_lists_and_listless_documents(corpus):
    """Empty lists for probed cells, and documents in no list at all: both leave (document, code) pairs uncovered."""
    C = corpus
    a = C["a"]
    c, d = list_entries(a)
    empty = np.unique(np.concatenate([C["top"][i].trace.cells[:3] for i in range(6)]))
    listless = np.unique(np.concatenate([C["top"][i].passage_ids[1:4] for i in range(6)]))
    m = ~np.isin(c, empty) & ~np.isin(d, listless)
    b = with_lists(a, c[m], d[m])
    assert (b["ivf_lengths"][empty] == 0).all() and not ivf_covers_codes(b)
    hx, ox = open_both(b)
    try:
        compare_index(hx, ox, C["batch"], C["traced"], False, "empty lists")
    finally:
        hx.close()


def test_zero_token_documents_in_lists(corpus):
    """Documents with no tokens (no codes, so the lists still cover every pair), some of them entries of probed lists: the
    reference makes them candidates with nothing to score; the level keeps running."""
    C = corpus
    a = C["a"]
    lens = np.asarray(a["doc_lengths"], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng(7)
    zero = np.sort(rng.choice(lens.size, 400, replace=False))
    tok = np.ones(int(off[-1]), bool)
    for z in zero:
        tok[off[z]:off[z + 1]] = False
    b = dict(a)
    b["codes"], b["residuals"] = a["codes"][tok], a["residuals"][tok]
    b["doc_lengths"] = lens.copy()
    b["doc_lengths"][zero] = 0
    c, d = list_entries(a)
    m = ~np.isin(d, zero)
    cells = np.unique(np.concatenate([C["top"][i].trace.cells[:4] for i in range(8)]))
    ins = [(int(cl), int(z)) for j, z in enumerate(zero[:200]) for cl in cells[j % cells.size::37]]
    b = with_lists(b, np.append(c[m], [x for x, _ in ins]), np.append(d[m], [y for _, y in ins]))
    assert level_may_run(b)
    hx, ox = open_both(b)
    try:
        compare_index(hx, ox, C["batch"], C["traced"], True, "zero-token documents")
    finally:
        hx.close()


def test_missing_pairs_through_the_index_files(corpus, tmp_path):
    """The same perturbation written as an index directory (write_index_dir with explicit lists) and opened with
    MmapIndex.load: the file-backed open runs the same gate."""
    C = corpus
    a = C["a"]
    keep = missing_pair_victims(C, range(8))
    b = drop_pairs(a, keep)
    npa.write_index_dir(str(tmp_path), b["centroids"], b["bucket_weights"], b["doc_lengths"], b["codes"], b["residuals"],
                        b["nbits"], ivf=b["ivf"], ivf_lengths=b["ivf_lengths"])
    ox = oracle_index(b)
    hx = npa.MmapIndex.load(str(tmp_path))
    try:
        compare_index(hx, ox, C["batch"], C["traced"], False, "files, missing pairs", regimes=REGIMES[:1])
    finally:
        hx.close()
    c_dir = tmp_path / "canonical"
    npa.write_index_dir(str(c_dir), a["centroids"], a["bucket_weights"], a["doc_lengths"], a["codes"], a["residuals"],
                        a["nbits"], ivf=a["ivf"], ivf_lengths=a["ivf_lengths"])
    hx = npa.MmapIndex.load(str(c_dir))
    try:
        compare_index(hx, oracle_index(a), C["batch"], C["traced"], True, "files, canonical", regimes=REGIMES[:1])
    finally:
        hx.close()


@pytest.mark.parametrize("G", [2, 3])
def test_missing_pairs_in_one_shard(corpus, G):
    """In-process shards of an index whose last shard misses pairs and whose first does not: each shard checks only its own
    documents, so the level runs on the first and not on the last; the merged result equals the unsharded one bit for bit,
    and the oracle's."""
    import torch
    from next_plaid_amd.dist import HipShardBackend, ShardedSearcher
    C = corpus
    a = C["a"]
    n = a["doc_lengths"].size
    keep = missing_pair_victims(C, range(32), pick=lambda d: d >= n * 2 // 3 + 1, per_query=2)
    assert len(keep) >= 4
    b = drop_pairs(a, keep)
    full, ox = open_both(b)
    shards = [hip_index(b, shard_rank=r, shard_count=G) for r in range(G)]
    try:
        bounds = [(int(s.info.shard_doc_begin), int(s.info.shard_doc_end)) for s in shards]
        may = [level_may_run(b, sh) for sh in bounds]
        assert may[0] and not may[-1], (bounds, may)
        stream = torch.cuda.Stream()
        ss = ShardedSearcher([HipShardBackend(s, stream=stream) for s in shards], use_dist=False)
        compare_index(full, ox, C["batch"], [], False, f"G={G} unsharded", regimes=REGIMES[:1],
                      shard_handles=list(zip(shards, may)))
        for thr, nprobe in REGIMES:
            p = P(thr, nprobe)
            orc = ox.search_batch(C["batch"], to_oracle_params(p))
            for gain in GAINS:
                full.tune("s3_gain", gain)
                for s in shards:
                    s.tune("s3_gain", gain)
                res = ss.search_batch(C["batch"], p)
                ref = full.search_batch(C["batch"], p)
                for i, (r, f, o) in enumerate(zip(res, ref, orc)):
                    tag = f"G={G} thr={thr} nprobe={nprobe} s3_gain={gain} q{i}"
                    assert np.array_equal(r.passage_ids, f.passage_ids) and np.array_equal(r.scores, f.scores), tag
                    assert_ranking_close(r.passage_ids, r.scores, o.passage_ids, o.scores, RTOL_F32, tag)
    finally:
        for s in shards:
            s.close()
        full.close()


def append_long_docs(a, lengths, rng):
    """Documents of 4097-9000 tokens made of the tokens of runs of existing documents (so their codes repeat); canonical
    posting lists rebuilt from the codes."""
    lens = np.asarray(a["doc_lengths"], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    codes, res = [a["codes"]], [a["residuals"]]
    for L in lengths:
        d0 = int(rng.integers(0, lens.size - 400))
        d1 = int(np.searchsorted(off, off[d0] + L)) + 1
        assert off[d1] - off[d0] >= L
        codes.append(a["codes"][off[d0]:off[d0] + L])
        res.append(a["residuals"][off[d0]:off[d0] + L])
    b = dict(a)
    b["codes"], b["residuals"] = np.concatenate(codes), np.concatenate(res)
    b["doc_lengths"] = np.concatenate([lens, np.asarray(lengths, np.int64)])
    b["ivf"], b["ivf_lengths"] = synth.build_ivf(b["codes"], b["doc_lengths"], a["centroids"].shape[0])
    return b


def test_documents_past_the_distinct_code_sort(corpus):
    """Documents longer than NP_UNIQ_MAX = 4096 tokens keep an unsorted distinct-code list with duplicates (unique_codes_kernel)
    and are flagged by useg_kernel.  Queries drawn from their tokens make them rank: every S4 kernel with and without the
    u8 filter, and the zeroth level (the lists are canonical, so it runs), must equal the oracle."""
    C = corpus
    a = C["a"]
    rng = np.random.default_rng(8)
    lengths = [4097, 5000, 7001, 9000]
    b = append_long_docs(a, lengths, rng)
    n0 = a["doc_lengths"].size
    assert level_may_run(b)
    off = np.concatenate([[0], np.cumsum(b["doc_lengths"])])
    g = np.random.default_rng(9)
    lq = []
    for j in range(len(lengths)):
        s = int(off[n0 + j])
        pick = s + g.choice(lengths[j], 32, replace=False)
        v = synth.reconstruct(b["codes"][pick], b["residuals"][pick], b["centroids"], b["bucket_weights"], b["nbits"])
        v = v + np.float32(0.5 / np.sqrt(v.shape[1])) * g.standard_normal(v.shape).astype(np.float32)
        lq.append(np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True), np.float32))
    batch = lq + [lq[0][:7], lq[1][:1]] + C["batch"][:16]
    hx, ox = open_both(b)
    try:
        top = ox.search_batch(lq, to_oracle_params(P(None, 8)))
        for j, r in enumerate(top):
            assert n0 + j in r.passage_ids, f"long document {n0 + j} does not rank for its own query: {r.passage_ids}"
        compare_index(hx, ox, batch, lq[:2], True, "long documents")
        hx.tune("s3_gain", 2)
        for thr, nprobe in ((0.4, 8), (None, 32)):
            p = P(thr, nprobe, n_full_scores=512)
            op = to_oracle_params(p)
            otr = [ox.search(q, op, trace=True) for q in (lq[0], lq[3], lq[2][:13])]
            ref = ox.search_batch(batch, op)
            for mode in range(9):
                for filt in (0, 1):
                    hx.tune("s4_mode", mode)
                    hx.tune("s4_minb", 1)
                    hx.tune("s4_filter", filt)
                    tag = f"long documents thr={thr} S4 mode {mode} filter {filt}"
                    for j, o in enumerate(otr):
                        compare_trace(hx.debug_trace((lq[0], lq[3], lq[2][:13])[j], p), o, f"{tag} q{j}")
                    hx.tune("s4_minb", 8)
                    for i, (r, o) in enumerate(zip(hx.search_batch(batch, p), ref)):
                        assert_ranking_close(r.passage_ids, r.scores, o.passage_ids, o.scores, RTOL_F32, f"{tag} batch q{i}")
        for k, v in S4_DEFAULTS:
            hx.tune(k, v)
    finally:
        hx.close()
