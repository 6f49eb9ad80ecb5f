"""The keyword half of a hybrid search on the device: set_text, np_hip_text_search, np_hip_fuse, np_hip_search_hybrid.  Needs
a real MI355X.

The reference is tests/text_restate.py (which tests/test_text_restate_cpu.py pins to SQLite's own FTS5, bm25() bit for bit):
ids equal and f32 scores bit for bit, for the keyword search and for the fusion.  The hybrid call is compared with the
composition of the three separate calls of the same build, byte for byte."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from helpers import ROOT, hip_index, make_arrays

import next_plaid_amd as npa
from next_plaid_amd import api, synth, text as T
import text_restate as R

pytestmark = pytest.mark.gpu

SLICE = 4096   # documents per slice of the scoring kernel (NP_TEXT_SLICE_DOCS, np_text_plan.h)
COUNTS = [1, 63, 64, 65, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 5]
CAP = T.NP_TEXT_MAX_TOPK


def test_the_slice_constant_is_the_plans():
    with open(os.path.join(ROOT, "next-plaid_amd", "csrc", "np_text_plan.h")) as f:
        assert f"NP_TEXT_SLICE_DOCS = {SLICE};" in f.read()


def tiny_index(n_docs, **opts):
    """An index of n_docs one-token documents: the keyword search only needs its document count."""
    spec, a = make_arrays(num_docs=n_docs, num_centroids=16, dim=32, nbits=2, doc_len_min=1, doc_len_max=1, seed=3)
    return a, hip_index(a, **opts)


def corpus_texts(n):
    """Documents 0..2 of 0, 1 and 130 tokens, "wo0" in every non-empty one, and posting lists of special shapes: "solo" in
    the last document only, "edge" exactly in the documents next to every slice boundary (its parts of a slice start or
    end at the boundary), "fin tail" as the last two tokens of every seventh document (a phrase that ends at a
    document's last position), "fin" elsewhere too."""
    texts = R.make_texts(n, 12, seed=n, every="wo0", lens=(0, 1, 2, 3, 5, 8, 13, 21))
    for d in range(3, n):
        if d % 7 == 0:
            texts[d] = (texts[d] + " fin tail").strip()
        elif d % 5 == 0:
            texts[d] = ("fin " + texts[d] + " tail wo1").strip()
        if d % SLICE in (0, SLICE - 1):
            texts[d] = (texts[d] + " edge").strip()
    texts[n - 1] = (texts[n - 1] + " solo").strip()
    return texts


def special_queries(data):
    v = data.vocab
    ids = lambda *ws: [v.get(w, -1) for w in ws]
    AND, OR = T.NP_TEXT_AND, T.NP_TEXT_OR
    q = [T.TextQuery.from_phrases([ids("wo0")], AND),                      # (nearly) every document: the idf clamp
         T.TextQuery.from_phrases([ids("solo")], AND),                     # a list of one entry
         T.TextQuery.from_phrases([ids("nowhere")], OR),                   # an empty list
         T.TextQuery.from_phrases([ids("edge")], AND), T.TextQuery.from_phrases([ids("edge"), ids("wo0")], AND),
         T.TextQuery.from_phrases([ids("fin", "tail")], AND), T.TextQuery.from_phrases([ids("fin", "tail"), ids("edge")], OR),
         T.TextQuery.from_phrases([ids("wo0")] * 3, AND),                  # a repeated phrase scores repeatedly
         T.TextQuery.from_phrases([ids("wo1", "wo0", "wo2"), ids("wo3", "nowhere")], OR),
         T.TextQuery.from_phrases([ids("solo"), ids("nowhere")], AND),
         T.TextQuery.from_phrases([ids("wo0", "wo0")], AND)]
    return q


@pytest.fixture(scope="module", params=COUNTS)
def sized(request):
    n = request.param
    texts = corpus_texts(n)
    data = T.TextIndexData.from_texts(texts)
    a, hx = tiny_index(n)
    before = hx.info.device_bytes
    hx.set_text(data)
    assert hx.info.device_bytes > before
    rs = R.Restated(data, n)
    queries = special_queries(data) + R.random_queries(data, 60, seed=n)   # more than 64 in one call, AND and OR mixed
    want = {}
    yield n, data, hx, rs, queries, want
    hx.set_text(None)
    assert hx.info.device_bytes == before
    hx.close()


def expect(rs, want, qi, q, k, subset=None, tag=None):
    key = (qi, k, tag)
    if key not in want:
        want[key] = rs.search(q, k, subset)
    return want[key]


def same(r, ids, sc):
    return (r.passage_ids.dtype == np.int64 and r.scores.dtype == np.float32 and np.array_equal(r.passage_ids, ids)
            and np.array_equal(r.scores.view(np.uint32), sc.view(np.uint32)))


def test_more_than_64_queries_equal_the_restatement(sized):
    n, data, hx, rs, queries, want = sized
    assert len(queries) > 64 and {q.mode for q in queries} == {T.NP_TEXT_AND, T.NP_TEXT_OR}
    got = hx.text_search(queries, 10)
    n_hits = 0
    for i, (q, r) in enumerate(zip(queries, got)):
        ids, sc = expect(rs, want, i, q, 10)
        assert same(r, ids, sc), f"n={n} query {i} {q.phrases()} mode {q.mode}: {r.passage_ids[:5]} {r.scores[:5]} vs {ids[:5]} {sc[:5]}"
        n_hits += ids.size
    assert n_hits > 0 and hx.last_stats["n_queries"] == len(queries) and hx.last_stats["n_ivf_ids"] > 0
    again = hx.text_search(queries, 10)                                     # the same bits from run to run
    assert all(same(a, b.passage_ids, b.scores) for a, b in zip(again, got))


@pytest.mark.parametrize("top_k", [1, CAP])
def test_top_k_one_and_the_cap(sized, top_k):
    n, data, hx, rs, queries, want = sized
    pick = list(range(12)) + [20, 30]
    got = hx.text_search([queries[i] for i in pick], top_k)
    for i, r in zip(pick, got):
        ids, sc = expect(rs, want, i, queries[i], top_k)
        assert same(r, ids, sc), f"n={n} top_k={top_k} query {i}"
    if n > 2 * CAP:
        assert max(r.passage_ids.size for r in got) == top_k                # the cut is reached at the cap too
    else:
        assert any(0 < r.passage_ids.size < top_k for r in got) or top_k == 1   # larger than the matches: count = matches


def test_each_query_alone_equals_its_place_in_the_batch(sized):
    n, data, hx, rs, queries, want = sized
    pick = [0, 1, 3, 5, 6, 8, 15, 40, 70]
    batch = hx.text_search(queries, 10)
    for i in pick:
        alone = hx.text_search([queries[i]], 10)[0]
        assert same(alone, batch[i].passage_ids, batch[i].scores), f"n={n} query {i}"
    rev = hx.text_search(queries[::-1], 10)[::-1]                           # at any position
    assert all(same(a, b.passage_ids, b.scores) for a, b in zip(rev, batch))


def test_subsets_none_empty_all_one_document(sized):
    n, data, hx, rs, queries, want = sized
    pick = [0, 3, 4, 5, 6, 7, 11, 12, 13, 14, 15, 16]
    qs = [queries[i] for i in pick]
    everything, nothing, last = np.arange(n), np.zeros(0, np.int64), np.array([n - 1])
    some = np.array(sorted({0, 2, n // 2, n - 1, n + 5, -3} | set(range(1, n, 3))), np.int64)   # ids outside the index are ignored
    subsets = [[None, nothing, everything, last, some, some][j % 6] for j in range(len(qs))]
    got = hx.text_search(qs, 10, subsets=subsets)
    for j, (i, r) in enumerate(zip(pick, got)):
        ids, sc = expect(rs, want, i, queries[i], 10, subsets[j], tag=j % 6)
        assert same(r, ids, sc), f"n={n} query {i} subset {j % 6}"
        if j % 6 == 1:
            assert r.passage_ids.size == 0
        if j % 6 == 2:
            assert same(r, *expect(rs, want, i, queries[i], 10))
    one = hx.text_search(qs, 10, subset=some)                               # one subset for the batch
    for i, r in zip(pick, one):
        assert same(r, *expect(rs, want, i, queries[i], 10, some, tag=4))


def test_filters_equal_subsets_on_the_filters_ids(sized):
    n, data, hx, rs, queries, want = sized
    hx.set_columns({"docno": np.arange(n, dtype=np.int64), "z": np.arange(n, dtype=np.int64) % 5})
    try:
        conds = [("z = ?", [1]), None, ("docno >= ?", [n - 1]), ("0 = 1", []), ("1 = 1", []), ("z = ?", [1])]
        ids = hx.filter_ids([c for c in conds if c is not None])
        it = iter(ids)
        subsets = [None if c is None else next(it) for c in conds]
        qs = [queries[i] for i in (0, 3, 4, 5, 12, 13)]
        a = hx.text_search(qs, 10, filters=conds)
        b = hx.text_search(qs, 10, subsets=subsets)
        assert all(same(x, y.passage_ids, y.scores) for x, y in zip(a, b))
        assert a[3].passage_ids.size == 0 and sum(r.passage_ids.size for r in a) > 0
    finally:
        hx.set_columns({})


def test_small_workspace_runs_in_chunks_with_the_same_bits():
    """3 slices + 5 documents are 4 slices.  At top_k = 1024 a (query, slice) pair is 12 292 bytes of lists: 100 kB hold one
    query over three slices at a time (two chunks of slices per query, one query per chunk), the default everything; at
    max_batch = 7 the 71 queries run in eleven chunks of queries, and 60 kB hold 32 queries at top_k = 10.  The bits must not depend on it; a budget that holds no
    chunk is an error, not a failed launch."""
    n = 3 * SLICE + 5
    data = T.TextIndexData.from_texts(corpus_texts(n))
    queries = special_queries(data) + R.random_queries(data, 60, seed=n)
    a, hx = tiny_index(n)
    hx.set_text(data)
    try:
        want10 = hx.text_search(queries, 10)
        want_cap = hx.text_search(queries[:3], CAP)
        assert max(r.passage_ids.size for r in want_cap) == CAP
    finally:
        hx.close()
    for opts, qs, k, want in (({"workspace_bytes": 100_000}, queries[:3], CAP, want_cap), ({"max_batch": 7}, queries, 10, want10),
                              ({"workspace_bytes": 60_000}, queries, 10, want10)):
        a, hx = tiny_index(n, **opts)
        hx.set_text(data)
        try:
            got = hx.text_search(qs, k)
            assert all(same(g, w.passage_ids, w.scores) for g, w in zip(got, want)), str(opts)
        finally:
            hx.close()
    a, tight = tiny_index(n, workspace_bytes=20_000)
    tight.set_text(data)
    try:
        with pytest.raises(MemoryError, match="workspace budget"):   # NP_ERR_OUT_OF_MEMORY
            tight.text_search(queries[:1], CAP)
    finally:
        tight.close()


class DeviceArrays:
    """Device copies of numpy arrays through the HIP runtime this process has already loaded (the library's own)."""

    def __init__(self):
        with open("/proc/self/maps") as f:
            paths = sorted({l.split()[-1] for l in f if "libamdhip64" in l})
        assert paths, "no HIP runtime is loaded in this process"
        self.hip = C.CDLL(paths[0])
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.ptrs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 8)) == 0
        self.ptrs.append(p)
        if a.nbytes:
            assert self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0      # host to device
        return p

    def get(self, p, like):
        out = np.empty_like(like)
        assert self.hip.hipDeviceSynchronize() == 0
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), p, out.nbytes, 2) == 0        # device to host
        return out

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)


# ---- fusion ---------------------------------------------------------------------------------------------------------------

def fuse_cases():
    nan = float("nan")
    hand = [([5, 3], [9.0, 4.0], [9, 7], [2.0, 1.0]),                       # disjoint
            ([5, 3, 8], [9.0, 4.0, 1.0], [5, 3, 8], [7.0, 6.5, 6.0]),       # identical
            ([], [], [4, 2], [3.0, 1.0]), ([4, 2], [3.0, 1.0], [], []), ([], [], [], []),   # one or both empty
            ([9, 4], [3.0, 3.0], [4, 1], [7.0, 7.0]),                       # all scores equal: range 0
            ([7, 3], [2.0, 1.0], [3, 7], [2.0, 1.0]),                       # mirrored: a tie broken by id
            ([1, 2, 3], [4.0, nan, 2.0], [3, 4], [nan, nan])]               # NaN ignored by min / max, last in the order
    rng = random.Random(5)
    rand = []
    for i in range(200):                                                     # overlap 0 .. 100 %
        ns, nk = rng.choice([0, 1, 2, 7, 64, 300, 1024]), rng.choice([1, 3, 8, 65, 300, 1024])
        pool = rng.sample(range(5000), ns + nk)
        sem = pool[:ns]
        share = int(round(min(ns, nk) * (i % 11) / 10.0))
        kw = rng.sample(sem, share) + pool[ns: ns + nk - share]
        rng.shuffle(kw)
        ss = sorted((rng.choice([rng.random() * 30, float(rng.randrange(4))]) for _ in sem), reverse=True)
        ks = sorted((rng.choice([rng.random() * 12, float(rng.randrange(3))]) for _ in kw), reverse=True)
        rand.append((sem, ss, kw, ks))
    return hand, rand


@pytest.mark.parametrize("mode", ["rrf", "relative_score"])
def test_fuse_equals_the_restatement_bit_for_bit(mode):
    hand, rand = fuse_cases()
    a, hx = tiny_index(8)
    try:
        for alpha, top_k, cases in ((0.75, 10, hand), (0.0, 10, hand), (1.0, 3, hand), (0.75, 10, rand), (0.3, 2048, rand[:40])):
            got = npa.fuse(mode, alpha, top_k, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases],
                           [c[3] for c in cases], index=hx)
            for c, (ids, sc) in zip(cases, got):
                w_ids, w_sc = R.fuse(mode, alpha, top_k, *c)
                assert np.array_equal(ids, w_ids), f"{mode} alpha={alpha}: {c[0][:4]} {c[2][:4]}: {ids[:6]} vs {w_ids[:6]}"
                assert np.array_equal(sc.view(np.uint32), w_sc.view(np.uint32)), f"{mode} alpha={alpha}: {sc[:6]} vs {w_sc[:6]}"
        # the module-level functions with the reference's argument order, and without a handle
        c = hand[0]
        assert np.array_equal(npa.fuse_rrf([c[0]], [c[2]], 0.75, 10)[0][0], R.fuse_rrf(c[0], c[2], 0.75, 10)[0])
        assert np.array_equal(npa.fuse_relative_score([c[0]], [c[1]], [c[2]], [c[3]], 0.75, 10, index=hx)[0][1],
                              R.fuse_relative_score(*c, 0.75, 10)[1])
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="alpha"):
                npa.fuse(mode, bad, 10, [c[0]], [c[1]], [c[2]], [c[3]], index=hx)
        with pytest.raises(ValueError, match="top_k"):
            npa.fuse(mode, 0.5, 0, [c[0]], [c[1]], [c[2]], [c[3]], index=hx)
        with pytest.raises(ValueError, match="stride"):
            npa.fuse(mode, 0.5, 5, [list(range(1025))], [[1.0] * 1025], [c[2]], [c[3]], index=hx)
    finally:
        hx.close()


# ---- the hybrid request -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hybrid():
    spec, a = make_arrays(num_docs=1500, num_centroids=64, dim=32, nbits=2, doc_len_min=4, doc_len_max=12, seed=11)
    hx = hip_index(a)
    data = T.TextIndexData.from_texts(corpus_texts(1500))
    hx.set_text(data)
    qs, _ = synth.make_queries(spec, 9, n_tokens=8, cen=a["centroids"])
    yield spec, a, hx, data, list(qs)
    hx.close()


@pytest.mark.parametrize("fusion,alpha", [("relative_score", 0.75), ("rrf", 0.75), ("rrf", 0.0), ("relative_score", 1.0)])
def test_search_hybrid_equals_the_three_calls_composed(hybrid, fusion, alpha):
    spec, a, hx, data, qs = hybrid
    texts = ["wo1 wo2", "wo3 OR solo OR fin", '"fin tail"', "", "nowhere", "wo0", '"wo1 wo0" OR edge', "wo5 AND wo1 AND wo0", "wo2"]
    p = npa.SearchParameters(n_full_scores=128, top_k=7, n_ivf_probe=4)
    some = np.arange(0, 1500, 3)
    for scope in ({}, {"subsets": [None, some, some, None, some, np.zeros(0, np.int64), None, some, np.arange(1500)]}, {"subset": some}):
        for fetch_k in (None, 40):
            fk = 21 if fetch_k is None else fetch_k
            pf = npa.SearchParameters(n_full_scores=128, top_k=fk, n_ivf_probe=4)
            sem = hx.search_batch(qs, pf, **scope)
            kw = hx.text_search(texts, fk, **scope)
            assert kw[3].passage_ids.size == 0 and kw[4].passage_ids.size == 0 and kw[0].passage_ids.size > 0
            want = npa.fuse(fusion, alpha, 7, [r.passage_ids for r in sem], [r.scores for r in sem], [r.passage_ids for r in kw],
                            [r.scores for r in kw], index=hx)
            got = hx.search_hybrid(qs, texts, p, alpha=alpha, fusion=fusion, fetch_k=fetch_k, **scope)
            for i, (r, (ids, sc)) in enumerate(zip(got, want)):
                assert np.array_equal(r.passage_ids, ids) and r.scores.tobytes() == sc.tobytes(), f"{fusion} {alpha} {list(scope)} q{i}"
            assert hx.last_stats["n_queries"] == len(qs)
    assert sum(r.passage_ids.size for r in got) > 0


def test_search_hybrid_with_filters_equals_subsets(hybrid):
    spec, a, hx, data, qs = hybrid
    hx.set_columns({"z": np.arange(1500, dtype=np.int64) % 4})
    try:
        texts = ["wo1", "wo2 OR wo3", '"fin tail"', "wo0", "wo4", "", "wo1 wo2", "edge OR wo1", "solo OR wo0"]
        conds = [("z = ?", [1]), None, ("z < ?", [2]), ("z = ?", [1]), None, ("z = ?", [9]), ("1 = 1", []), None, ("z < ?", [2])]
        ids = iter(hx.filter_ids([c for c in conds if c is not None]))
        subsets = [None if c is None else next(ids) for c in conds]
        p = npa.SearchParameters(n_full_scores=128, top_k=6, n_ivf_probe=4)
        a_ = hx.search_hybrid(qs, texts, p, filters=conds)
        b_ = hx.search_hybrid(qs, texts, p, subsets=subsets)
        assert all(np.array_equal(x.passage_ids, y.passage_ids) and x.scores.tobytes() == y.scores.tobytes() for x, y in zip(a_, b_))
        assert a_[5].passage_ids.size == 0 and a_[0].passage_ids.size > 0
    finally:
        hx.set_columns({})


def test_device_entries_equal_the_host_entries(hybrid):
    """np_hip_text_search_device and np_hip_fuse_device on device buffers equal the host entries, bit for bit."""
    spec, a, hx, data, qs = hybrid
    queries = special_queries(data)[:8]
    some = np.arange(0, 1500, 3)
    subsets = [None, some, None, np.zeros(0, np.int64), some, None, np.array([3, 14, 1499, 5000]), None]
    sid, soff, qsub = api.pack_subsets(subsets, 8)
    want = hx.text_search(queries, 10, subsets=subsets)
    tq = api._CTextQueries(queries)
    dev = DeviceArrays()
    try:
        d_ids, d_off, d_qsub = (dev.put(x) for x in (sid, soff, qsub))
        ids, sc, cnt = np.zeros((8, 10), np.int64), np.zeros((8, 10), np.float32), np.zeros(8, np.int32)
        o_ids, o_sc, o_cnt = dev.put(ids), dev.put(sc), dev.put(cnt)
        api._check(api.lib().np_hip_text_search_device(hx._h, tq.arr, 8, 10, d_ids, d_off, soff.ctypes.data_as(C.c_void_p),
                                                       soff.size - 1, d_qsub, o_ids, o_sc, o_cnt, None))
        g_ids, g_sc, g_cnt = dev.get(o_ids, ids), dev.get(o_sc, sc), dev.get(o_cnt, cnt)
        for i, r in enumerate(want):
            assert g_cnt[i] == r.passage_ids.size and g_ids[i, : g_cnt[i]].tolist() == r.passage_ids.tolist(), f"q{i}"
            assert g_sc[i, : g_cnt[i]].view(np.uint32).tolist() == r.scores.view(np.uint32).tolist(), f"q{i}"
            assert not g_ids[i, g_cnt[i]:].any() and not g_sc[i, g_cnt[i]:].any()       # padded as search_exact pads
        # the keyword lists fused with themselves shifted by one query, on the device
        f_ids, f_sc, f_cnt = np.zeros((8, 12), np.int64), np.zeros((8, 12), np.float32), np.zeros(8, np.int32)
        p_ids, p_sc, p_cnt = dev.put(f_ids), dev.put(f_sc), dev.put(f_cnt)
        r_ids, r_sc, r_cnt = (dev.put(np.roll(x, 1, axis=0)) for x in (g_ids, g_sc, g_cnt))
        api._check(api.lib().np_hip_fuse_device(hx._h, T.NP_FUSE_RELATIVE_SCORE, 0.75, 12, 8, o_ids, o_sc, o_cnt, 10, r_ids, r_sc, r_cnt,
                                                10, p_ids, p_sc, p_cnt, None))
        h_ids, h_sc, h_cnt = dev.get(p_ids, f_ids), dev.get(p_sc, f_sc), dev.get(p_cnt, f_cnt)
        lists = [(r.passage_ids, r.scores) for r in want]
        host = npa.fuse("relative_score", 0.75, 12, [l[0] for l in lists], [l[1] for l in lists],
                        [lists[i - 1][0] for i in range(8)], [lists[i - 1][1] for i in range(8)], index=hx)
        for i, (w_ids, w_sc) in enumerate(host):
            assert h_cnt[i] == w_ids.size and h_ids[i, : h_cnt[i]].tolist() == w_ids.tolist(), f"fuse q{i}"
            assert h_sc[i, : h_cnt[i]].tobytes() == w_sc.tobytes(), f"fuse q{i}"
    finally:
        dev.free()


def test_cpp_mirror_prints_the_same_bits(tmp_path):
    spec, a = make_arrays(num_docs=96, num_centroids=16, dim=32, nbits=2, doc_len_min=3, doc_len_max=9, seed=5)
    exe = tmp_path / "text_hybrid"
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "text_hybrid.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    ixdir = tmp_path / "ix"
    ixdir.mkdir()
    synth.write_index(str(ixdir), {k: v for k, v in a.items() if k != "_prep"}, chunk_docs=40)
    data = T.TextIndexData.from_texts(R.make_texts(96, 8, seed=2, every="wo0", lens=(0, 1, 2, 3, 5, 8)))
    assert data.n_terms >= 5
    data.term_offsets.astype("<i8").tofile(tmp_path / "toff.i64")
    data.inst_doc.astype("<i8").tofile(tmp_path / "idoc.i64")
    data.inst_pos.astype("<i4").tofile(tmp_path / "ipos.i32")
    qs = list(synth.make_queries(spec, 6, n_tokens=5, cen=a["centroids"])[0])
    np.concatenate(qs, 0).astype("<f4").tofile(tmp_path / "q.f32")
    np.array([q.shape[0] for q in qs], "<i8").tofile(tmp_path / "lens.i64")
    out = subprocess.check_output([str(exe), str(ixdir), str(tmp_path / "toff.i64"), str(tmp_path / "idoc.i64"), str(tmp_path / "ipos.i32"),
                                   str(data.n_rows), str(tmp_path / "q.f32"), str(tmp_path / "lens.i64")], text=True)
    AND, OR = T.NP_TEXT_AND, T.NP_TEXT_OR
    tq = [[T.TextQuery.from_phrases([[0], [1]], AND), T.TextQuery.from_phrases([[2, 3], [1]], OR),
           T.TextQuery.from_phrases([[0], [-1], [4]], OR)][i % 3] for i in range(6)]
    evens = np.arange(0, 60, 2)
    subsets = [evens if i % 2 == 1 else None for i in range(6)]

    def lines(stage, res):
        s = ""
        for i, (ids, sc) in enumerate(res):
            s += f"{stage} {i} {ids.size}" + "".join(f" {d}:{b:08x}" for d, b in zip(ids.tolist(), sc.view(np.uint32).tolist())) + "\n"
        return s

    hx = npa.MmapIndex.load(str(ixdir))
    try:
        hx.set_text(data)
        kw = [(r.passage_ids, r.scores) for r in hx.text_search(tq, 9, subsets=subsets)]
        p = npa.SearchParameters(n_full_scores=64, top_k=5, n_ivf_probe=4)
        hy = [(r.passage_ids, r.scores) for r in hx.search_hybrid(qs, tq, p, alpha=0.75, fusion="relative_score", fetch_k=15, subsets=subsets)]
        fu = npa.fuse("rrf", 0.5, 6, [k[0] for k in kw], [k[1] for k in kw], [k[0][::-1] for k in kw], [k[1][::-1] for k in kw], index=hx)
        assert out == lines("text", kw) + lines("hybrid", hy) + lines("fuse", fu)
        assert sum(k[0].size for k in kw) > 10 and sum(h[0].size for h in hy) > 10
    finally:
        hx.close()


def test_errors_are_reported_before_any_launch(hybrid):
    spec, a, hx, data, qs = hybrid
    q1 = T.TextQuery.from_phrases([[0]])
    p = npa.SearchParameters(n_full_scores=128, top_k=5, n_ivf_probe=4)
    # a sharded handle: refused by set_text and by every call
    sh = hip_index(a, shard_rank=0, shard_count=2)
    try:
        with pytest.raises(ValueError, match="shard_count"):
            sh.set_text(data)
        with pytest.raises(ValueError, match="shard_count"):
            sh.text_search([q1], 5)
    finally:
        sh.close()
    # no keyword index set
    bare = hip_index(a)
    try:
        with pytest.raises(ValueError, match="no keyword index"):
            bare.text_search([q1], 5)
        with pytest.raises(ValueError, match="no keyword index"):
            bare.search_hybrid(qs[:1], [q1], p)
        with pytest.raises(ValueError, match="no keyword index"):
            bare.text_search(["wo1"], 5)
    finally:
        bare.close()
    # limits of a call and of a query
    for k in (0, CAP + 1):
        with pytest.raises(ValueError, match="top_k"):
            hx.text_search([q1], k)
    with pytest.raises(ValueError, match="top_k"):
        hx.search_hybrid(qs[:1], [q1], p, fetch_k=CAP + 1)
    for alpha in (-0.5, 1.01, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            hx.search_hybrid(qs[:1], [q1], p, alpha=alpha)
    with pytest.raises(ValueError, match="text query 1.*n_phrases"):
        hx.text_search([q1, T.TextQuery.from_phrases([[0]] * 65)], 5)
    with pytest.raises(ValueError, match="text query 0.*n_phrases"):
        hx.text_search([T.TextQuery.from_phrases([])], 5)
    with pytest.raises(ValueError, match="no token"):
        hx.text_search([T.TextQuery.from_phrases([[0], []])], 5)
    with pytest.raises(ValueError, match="256 tokens"):
        hx.text_search([T.TextQuery.from_phrases([[0] * 257])], 5)
    with pytest.raises(ValueError, match="names no term"):
        hx.text_search([T.TextQuery.from_phrases([[data.n_terms]])], 5)
    with pytest.raises(ValueError, match="mode"):
        hx.text_search([T.TextQuery.from_phrases([[0]], 2)], 5)
    # a malformed keyword index names its first offender and leaves the handle's index in place
    bad = T.TextIndexData(data.tokenizer, data.terms, data.term_offsets, data.inst_doc.copy(), data.inst_pos, data.n_rows, data.vocab)
    bad.inst_doc[5] = 1500
    with pytest.raises(ValueError, match="instance 5"):
        hx.set_text(bad)
    few = T.TextIndexData(data.tokenizer, data.terms, data.term_offsets, data.inst_doc, data.inst_pos, 3, data.vocab)
    with pytest.raises(ValueError, match="n_rows = 3"):
        hx.set_text(few)
    assert hx.text_search(["wo1 wo2"], 5)[0].passage_ids.size > 0
    assert hx.text_search([""], 5)[0].passage_ids.size == 0 and hx.text_search([], 5) == []
