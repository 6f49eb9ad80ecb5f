"""np_hip_search_exact (np_scan.hip): the exhaustive exact search against the float64 truth, through scan_restate.check_topk.

Every margin is exact_restate's derived bound.  The corpora are exact_restate.make_corpus: about 96 documents with planted
lengths at the 32-token tile edges, empty documents, three byte-identical copies of document 3 and a repeated-token document.
Beyond the checker: a query's result must not depend on its batch, on the query slices, on the group size or on the number of
document passes (bit-equal ids and scores), and precision 0 gives a (query, document) pair the very bits the search path's
exact-f32 S6 kernel gives it (both call np_exact.h).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exact_restate as X
import scan_restate as S
from helpers import ROOT, hip_index, make_arrays, synth

import next_plaid_amd as npa
from next_plaid_amd import api

pytestmark = pytest.mark.gpu

G0 = (128, 4, 0)
LENGTHS = (1, 31, 32, 33, 65, 256)
MIXED = (1, 33, 256, 48, 32, 64, 200, 5)


@pytest.fixture(scope="module")
def indexes():
    opened = {}

    def get(geo, **opts):
        key = (geo, tuple(sorted(opts.items())))
        if key not in opened:
            opened[key] = hip_index(X.make_corpus(geo), max_query_tokens=256, **opts)
        return opened[key]
    yield get
    for h in opened.values():
        h.close()


def bits(r):
    return r.passage_ids.tolist(), r.scores.view(np.uint32).tolist()


def same(r, f):
    return bits(r) == bits(f)


def precisions(geo):
    return (0, 3) if geo[1] in (2, 4) else (0,)


def mixed_queries(a, seed=1234):
    return [X.make_queries(a, lq, seed + lq)[i] for i, lq in enumerate(MIXED)]


@pytest.mark.parametrize("lq", LENGTHS)
@pytest.mark.parametrize("geo", X.GEOMETRIES, ids=X.geo_name)
def test_main_sweep(indexes, geo, lq):
    a = X.make_corpus(geo)
    hx = indexes(geo)
    n = len(a["doc_lengths"])
    copies = [3, n - 3, n - 2]
    qs = X.make_queries(a, lq, 900 + lq)
    try:
        for prec in precisions(geo):
            tb = [(S.truth(a, q), X.doc_bound(a, q, X.kernel_class(prec, X.prepare(a).nbits))) for q in qs]
            for k in (1, 10, n + 5):
                res = hx.search_exact(qs, k, prec)
                assert len(res) == len(qs)
                for qi, (q, r) in enumerate(zip(qs, res)):
                    what = f"{X.geo_name(geo)} lq{lq} p{prec} k{k} q{qi} ({X.QUERY_KINDS[qi]})"
                    S.check_topk(a, q, r.passage_ids, r.scores, k, prec, what=what, truth_bd=tb[qi])
                    if k > n:   # the three copies of document 3: bit-equal scores, ascending ids
                        pos = [int(np.nonzero(r.passage_ids == c)[0][0]) for c in copies]
                        assert pos == sorted(pos) and np.unique(r.scores[pos].view(np.uint32)).size == 1, what
                    if lq == 1 and X.QUERY_KINDS[qi] == "nan":   # every score is 0: the lowest non-empty ids
                        assert np.array_equal(r.passage_ids, S.in_scope(a)[:k]) and not r.scores.any(), what
            assert hx.last_stats["n_queries"] == len(qs) and hx.last_stats["n_exact_docs"] == len(qs) * S.in_scope(a).size
    finally:
        X.drop_query_cache(a)


@pytest.mark.parametrize("geo", [G0, (96, 2, 0), (64, 8, 0)], ids=X.geo_name)
def test_batch_independence(indexes, geo):
    a = X.make_corpus(geo)
    n = len(a["doc_lengths"])
    hx, hx4 = indexes(geo), indexes(geo, max_batch=4)
    for qs in (X.make_queries(a, 33, 933), mixed_queries(a)):
        for prec in precisions(geo):
            for k in (10, n + 5):
                base = hx.search_exact(qs, k, prec)
                again = hx.search_exact(qs, k, prec)
                alone = [hx.search_exact([q], k, prec)[0] for q in qs]
                sliced = hx4.search_exact(qs, k, prec)
                try:
                    hx.tune("scan_tiles", 1)
                    hx.tune("scan_docs", 17)      # six passes over the 96 documents
                    passes = hx.search_exact(qs, k, prec)
                    hx.tune("scan_tiles", 3)
                    hx.tune("scan_docs", 40)
                    other = hx.search_exact(qs, k, prec)
                finally:
                    hx.tune("scan_tiles", 8)
                    hx.tune("scan_docs", 0)
                for i in range(len(qs)):
                    for name, r in (("second run", again), ("alone", alone), ("max_batch 4", sliced), ("six passes", passes),
                                    ("three tiles, three passes", other)):
                        assert same(r[i], base[i]), f"{X.geo_name(geo)} p{prec} k{k} q{i}: {name} differs from the batch"


def test_mixed_lengths_in_one_batch(indexes):
    a = X.make_corpus(G0)
    hx = indexes(G0)
    n = len(a["doc_lengths"])
    qs = mixed_queries(a, 77)
    assert [q.shape[0] for q in qs] == list(MIXED)
    try:
        for prec in (0, 3):
            res = hx.search_exact(qs, n + 5, prec)
            for i, (q, r) in enumerate(zip(qs, res)):
                assert same(r, hx.search_exact(q, n + 5, prec)[0]), f"p{prec} q{i}"
                S.check_topk(a, q, r.passage_ids, r.scores, n + 5, prec, what=f"mixed p{prec} q{i}")
    finally:
        X.drop_query_cache(a)


def test_subsets(indexes):
    a = X.make_corpus(G0)
    hx, hx4 = indexes(G0), indexes(G0, max_batch=4)
    n = len(a["doc_lengths"])
    lens = np.asarray(a["doc_lengths"])
    qs = X.make_queries(a, 33, 955)
    evens = np.arange(0, n, 2, dtype=np.int64)
    empties = np.nonzero(lens == 0)[0].astype(np.int64)
    messy = np.array([5, 5, 90, -3, n, n + 1000, 7, 5, 2 ** 40, 81, 3, n - 2, n - 3, 90], np.int64)
    none = np.zeros(0, np.int64)
    assert empties.size >= 2
    try:
        # one subset for the batch
        for k in (10, n + 5):
            for prec in (0, 3):
                res = hx.search_exact(qs, k, prec, subset=evens)
                for i, (q, r) in enumerate(zip(qs, res)):
                    S.check_topk(a, q, r.passage_ids, r.scores, k, prec, scope=evens, what=f"evens p{prec} k{k} q{i}")
                    assert same(r, hx.search_exact([q], k, prec, subset=evens)[0])
        # one per query, mixed with None; an empty one; only empty documents; duplicates and out-of-range ids
        subsets = [evens, None, none, empties, messy, evens, None, messy]
        for h in (hx, hx4):
            for k in (3, n + 5):
                res = h.search_exact(qs, k, 0, subsets=subsets)
                for i, (q, r, sub) in enumerate(zip(qs, res, subsets)):
                    S.check_topk(a, q, r.passage_ids, r.scores, k, 0, scope=sub, what=f"per-query k{k} q{i}")
                    assert same(r, hx.search_exact([q], k, 0, subset=sub)[0]), f"k{k} q{i}"
                assert res[2].passage_ids.size == 0 and res[3].passage_ids.size == 0
                assert set(res[4].passage_ids.tolist()) <= {5, 90, 7, 81, 3, n - 2, n - 3}
        # ... in several passes
        try:
            hx.tune("scan_docs", 17)
            hx.tune("scan_tiles", 2)
            for r, f in zip(hx.search_exact(qs, 10, 0, subsets=subsets), hx4.search_exact(qs, 10, 0, subsets=subsets)):
                assert same(r, f)
        finally:
            hx.tune("scan_docs", 0)
            hx.tune("scan_tiles", 8)
        with pytest.raises(ValueError):
            hx.search_exact(qs, 10, subset=evens, subsets=subsets)
    finally:
        X.drop_query_cache(a)


def test_shards_merge_to_the_unsharded_answer():
    a = X.make_corpus(G0)
    n = len(a["doc_lengths"])
    qs = X.make_queries(a, 33, 977)
    whole = hip_index(a, max_query_tokens=256)
    shards = [hip_index(a, max_query_tokens=256, shard_rank=r, shard_count=3) for r in range(3)]
    try:
        for prec in (0, 3):
            for k, sub in ((10, None), (n + 5, None), (10, np.arange(1, n, 3))):
                want = whole.search_exact(qs, k, prec, subset=sub)
                parts = [h.search_exact(qs, k, prec, subset=sub) for h in shards]
                for i in range(len(qs)):
                    ids = np.concatenate([p[i].passage_ids for p in parts])
                    sc = np.concatenate([p[i].scores for p in parts])
                    o = np.lexsort((ids, -S.order_key(sc)))[:k]
                    assert ids[o].tolist() == want[i].passage_ids.tolist(), f"p{prec} k{k} q{i}"
                    assert sc[o].view(np.uint32).tolist() == want[i].scores.view(np.uint32).tolist(), f"p{prec} k{k} q{i}"
    finally:
        for h in shards + [whole]:
            h.close()


def test_wide_codes():
    spec, a = make_arrays(num_docs=300, num_centroids=70_000, dim=32, nbits=2, doc_len_min=1, doc_len_max=40)
    hx = hip_index(a, max_query_tokens=256)
    g = np.random.default_rng(5)
    D = X.decompress64(a)
    try:
        qs = [(D[g.integers(0, D.shape[0], lq)] + 0.05 * g.standard_normal((lq, 32))).astype(np.float32) for lq in (1, 33, 40)]
        for prec in (0, 3):
            for k in (10, 305):
                for i, (q, r) in enumerate(zip(qs, hx.search_exact(qs, k, prec))):
                    S.check_topk(a, q, r.passage_ids, r.scores, k, prec, what=f"wide codes p{prec} k{k} q{i}")
    finally:
        hx.close()


def test_long_document():
    base = X.make_corpus(G0)
    g = np.random.default_rng(11)
    T = base["codes"].size
    pick = np.concatenate([g.permutation(T), g.permutation(T)])[:2049 + 64]
    codes = np.concatenate([base["codes"], base["codes"][pick]])
    res = np.concatenate([base["residuals"], base["residuals"][pick]])
    lens = np.concatenate([base["doc_lengths"], [2049, 64]]).astype(np.int64)
    ivf, ivf_lengths = synth.build_ivf(codes, lens, X.K)
    a = dict(base, codes=codes, residuals=np.ascontiguousarray(res), doc_lengths=lens, ivf=ivf, ivf_lengths=ivf_lengths)
    a.pop("_prep", None)
    n = lens.size
    long_doc = n - 2
    p = X.prepare(a)
    D = X.decompress64(a)
    rows = D[p.off[long_doc] + g.choice(2049, 40, replace=False)]
    qs = [rows.astype(np.float32), rows[:1].astype(np.float32)] + X.make_queries(base, 33, 991)[:2]
    hx = hip_index(a, max_query_tokens=256)
    try:
        for prec in (0, 3):
            for k in (1, n + 5):
                res_ = hx.search_exact(qs, k, prec)
                for i, (q, r) in enumerate(zip(qs, res_)):
                    S.check_topk(a, q, r.passage_ids, r.scores, k, prec, what=f"long document p{prec} k{k} q{i}")
                assert res_[0].passage_ids[0] == long_doc
    finally:
        hx.close()


@pytest.mark.parametrize("geo", [G0, (100, 4, 2), (64, 8, 0), (64, 1, 0)], ids=X.geo_name)
def test_same_bits_as_the_search_path(indexes, geo):
    """precision 0: exact_f32_kernel (search_batch's S6) and scan_kernel call the same decompression, scales, maxima and
    q-ordered sum, one query tile per MFMA: a (query, document) pair gets the same bits from both."""
    a = X.make_corpus(geo)
    hx = indexes(geo)
    n = len(a["doc_lengths"])
    p = npa.SearchParameters(n_full_scores=4 * n, top_k=n, n_ivf_probe=X.K, centroid_score_threshold=None, precision=0)
    for lq in (1, 33, 256):
        qs = [q for q, kind in zip(X.make_queries(a, lq, 900 + lq), X.QUERY_KINDS) if kind == "near"]
        found = hx.search_batch(qs, p)
        for i, (r, e) in enumerate(zip(found, hx.search_exact(qs, n + 5, 0))):
            assert r.passage_ids.size > 0 and np.isin(r.passage_ids, e.passage_ids).all()
            score = dict(zip(e.passage_ids.tolist(), e.scores.view(np.uint32).tolist()))
            got = [score[d] for d in r.passage_ids.tolist()]
            assert got == r.scores.view(np.uint32).tolist(), f"{X.geo_name(geo)} lq{lq} q{i}"
    X.drop_query_cache(a)


def test_errors(indexes):
    a = X.make_corpus(G0)
    hx = indexes(G0)
    qs = X.make_queries(a, 5, 3)[:3]
    want = hx.search_exact(qs, 5)
    with pytest.raises(npa.ShapeError):
        hx.search_exact([np.zeros((4, 64), np.float32)], 5)
    L = api.lib()
    flat, off = hx._pack(qs)
    ids, sc, cnt = np.zeros(15, np.int64), np.zeros(15, np.float32), np.zeros(3, np.int32)

    def call(dim=128, top_k=5, precision=0, qoff=off):
        return L.np_hip_search_exact(hx._h, api._ptr(flat), api._ptr(qoff), 3, dim, top_k, precision, None, None, 0, None,
                                     api._ptr(ids), api._ptr(sc), api._ptr(cnt), None)
    assert call() == 0
    assert call(dim=64) == 3 and "Shape error" in api.last_error()
    assert call(qoff=np.array([0, 5, 10, 300], np.int32)) == 3 and "256" in api.last_error()
    for k in (0, 16385, -1):
        assert call(top_k=k) == 8 and "top_k" in api.last_error()
        with pytest.raises(ValueError):
            hx.search_exact(qs, k)
    for prec in (1, 2, 4):
        assert call(precision=prec) == 8 and "precision" in api.last_error()
        with pytest.raises(ValueError):
            hx.search_exact(qs, 5, prec)
    # a 160-wide index opens and refuses, as search does
    spec, wide = make_arrays(num_docs=50, num_centroids=16, dim=160, nbits=4, doc_len_min=4, doc_len_max=4, seed=1)
    h = hip_index(wide)
    with pytest.raises(npa.ShapeError):
        h.search_exact([np.zeros((4, 160), np.float32)], 5)
    h.close()
    # malformed CSR: the errors of np_hip_search_batch_subsets
    sid = np.arange(10, dtype=np.int64)
    good = (sid, np.array([0, 4, 10], np.int64), np.array([0, -1, 1], np.int32))
    fine = hx.search_exact_csr(qs, 5, 0, *good)
    bad = {
        "offsets do not start at 0": (sid, np.array([1, 4, 10], np.int64), good[2]),
        "offsets decrease": (sid, np.array([0, 6, 4], np.int64), good[2]),
        "entry below -1": (sid, good[1], np.array([0, -2, 1], np.int32)),
        "entry >= n_subsets": (sid, good[1], np.array([0, 2, 1], np.int32)),
        "NULL ids with a positive count": (None, good[1], good[2]),
        "NULL query_subset with subsets": (sid, good[1], None),
    }
    p = npa.SearchParameters(n_full_scores=64, top_k=5, n_ivf_probe=4)
    for what, args in bad.items():
        with pytest.raises(ValueError) as e:
            hx.search_exact_csr(qs, 5, 0, *args)
        with pytest.raises(ValueError) as e2:
            hx.search_batch_csr(qs, p, *args)
        assert str(e.value) and str(e.value) == str(e2.value), what
        for r, f in zip(hx.search_exact_csr(qs, 5, 0, *good), fine):   # the handle still answers, and the same
            assert same(r, f), what
    rc = L.np_hip_search_exact(hx._h, None, None, 0, 128, 5, 0, None, None, 2, None, None, None, None, None)
    assert rc == 8 and "subset_offsets is NULL" in api.last_error()
    for r, f in zip(hx.search_exact(qs, 5), want):
        assert same(r, f)


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


def test_device_entry(indexes):
    """np_hip_search_exact_device on device buffers equals the host entry, bit for bit, also in slices of three queries."""
    a = X.make_corpus(G0)
    qs = mixed_queries(a, 31)
    subsets = [None, np.arange(0, 90, 2), None, np.zeros(0, np.int64), np.arange(0, 90, 2), None, np.array([3, 94, 93, 500]), None]
    sid, soff, qsub = api.pack_subsets(subsets, 8)
    hx = hip_index(a, max_query_tokens=256, max_batch=3)
    want = indexes(G0).search_exact(qs, 10, 0, subsets=subsets)
    flat, qoff = hx._pack(qs)
    dev = DeviceArrays()
    try:
        d_q, d_qoff, d_ids, d_off, d_qsub = (dev.put(x) for x in (flat, qoff, sid, soff, qsub))
        ids, sc, cnt = np.zeros((8, 10), np.int64), np.zeros((8, 10), np.float32), np.zeros(8, np.int32)
        o_ids, o_sc, o_cnt = dev.put(ids), dev.put(sc), dev.put(cnt)
        api._check(api.lib().np_hip_search_exact_device(
            hx._h, d_q, d_qoff, qoff.ctypes.data_as(C.c_void_p), 8, 128, 10, 0, d_ids, d_off, soff.ctypes.data_as(C.c_void_p),
            soff.size - 1, d_qsub, o_ids, o_sc, o_cnt, None))
        g_ids, g_sc, g_cnt = dev.get(o_ids, ids), dev.get(o_sc, sc), dev.get(o_cnt, cnt)
        for i, r in enumerate(want):
            assert g_cnt[i] == r.passage_ids.size, f"q{i}"
            assert g_ids[i, : g_cnt[i]].tolist() == r.passage_ids.tolist(), f"q{i}"
            assert g_sc[i, : g_cnt[i]].view(np.uint32).tolist() == r.scores.view(np.uint32).tolist(), f"q{i}"
        # the offsets are checked on the host here too; a NULL device copy is refused
        rc = api.lib().np_hip_search_exact_device(
            hx._h, d_q, d_qoff, qoff.ctypes.data_as(C.c_void_p), 8, 128, 10, 0, d_ids, None, soff.ctypes.data_as(C.c_void_p),
            soff.size - 1, d_qsub, o_ids, o_sc, o_cnt, None)
        assert rc == 8 and "device copy" in api.last_error()
    finally:
        hx.close()
        dev.free()


def test_cpp_mirror_prints_the_same_bits(tmp_path):
    a = X.make_corpus((96, 4, 0))
    exe = tmp_path / "search_exact"
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "search_exact.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    ixdir = tmp_path / "ix"
    ixdir.mkdir()
    synth.write_index(str(ixdir), {k: v for k, v in a.items() if k != "_prep"}, chunk_docs=40)
    qs = [X.make_queries(a, lq, 40 + lq)[i] for i, lq in enumerate((5, 33, 70, 1, 256, 32))]
    np.concatenate(qs, 0).astype("<f4").tofile(tmp_path / "q.f32")
    np.array([q.shape[0] for q in qs], "<i8").tofile(tmp_path / "lens.i64")
    evens, few = np.arange(0, 60, 2), np.arange(3, 10)
    subsets = [evens if i % 3 == 1 else few if i % 3 == 2 else None for i in range(len(qs))]
    hx = npa.MmapIndex.load(str(ixdir), max_query_tokens=256)
    try:
        for prec in (0, 3):
            out = subprocess.check_output([str(exe), str(ixdir), str(tmp_path / "q.f32"), str(tmp_path / "lens.i64"), "12", str(prec)],
                                          text=True)
            want = ""
            for r in hx.search_exact(qs, 12, prec, subsets=subsets):
                want += f"{r.query_id} {r.passage_ids.size}"
                want += "".join(f" {d}:{b:08x}" for d, b in zip(r.passage_ids.tolist(), r.scores.view(np.uint32).tolist())) + "\n"
            assert out == want, f"precision {prec}"
            assert out.count("\n") == len(qs) and " 12 " in out
    finally:
        hx.close()
