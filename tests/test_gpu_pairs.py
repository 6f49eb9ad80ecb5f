"""np_hip_score_pairs (np_pairs.hip): given (query, document) pairs with per-token matches, through pairs_restate.check_pairs.

Every margin is exact_restate's derived bound at precision 0.  The corpora are exact_restate.make_corpus: about 96 documents
with planted lengths at the 32-token tile edges, empty documents and a repeated-token document.  Beyond the checker: a pair's
three outputs must not depend on its batch, the query slices, the staging chunks or its place in the list (bit-equal), and the
score is the very bits the search path's exact-f32 S6 kernel and the exact scan give the pair (all call np_exact.h).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exact_restate as X
import pairs_restate as P
from helpers import ROOT, hip_index, make_arrays, synth

import next_plaid_amd as npa
from next_plaid_amd import api

pytestmark = pytest.mark.gpu

G0 = (128, 4, 0)
LENGTHS = (1, 31, 32, 33, 65, 200, 256)
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


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same(r, f):
    """Two (scores, sims, pos) triples, bit for bit."""
    return all(a.shape == b.shape for a, b in zip(r, f)) and np.array_equal(u32(r[0]), u32(f[0])) and \
        np.array_equal(u32(r[1]), u32(f[1])) and np.array_equal(r[2], f[2])


def mixed_queries(a, seed=1234):
    return [X.make_queries(a, lq, seed + lq)[i] for i, lq in enumerate(MIXED)]


def instantiation(geo):
    """(DIM, NBITS) of the kernel a geometry runs: rows are stored at the next multiple of 32, 1-bit residuals as 2-bit."""
    return (geo[0] + 31) // 32 * 32, 2 if geo[1] == 1 else geo[1]


INSTANTIATIONS = sorted({instantiation(g) for g in X.GEOMETRIES})


@pytest.mark.parametrize("lq", LENGTHS)
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=lambda i: f"D{i[0]}b{i[1]}")
def test_main_sweep(indexes, inst, lq):
    """Every geometry of exact_restate.GEOMETRIES x every query length, the 8-query batch against every document, through
    check_pairs.  Conditions (a)-(g) are asserted per query and geometry.  The cap on ambiguous entries (0.5 %) is asserted
    over what one case checks: the geometries that run ONE kernel instantiation pairs_kernel<DIM, NBITS, NQT of this length>
    -- the unit a wrong position would come from -- so every instantiation has at least 99.5 % of its positions decided by (c).

    The number of ambiguous entries follows from the float64 similarities and the bound alone, not from anything the device
    returns.  Per geometry it is 0-0.15 % of a case's entries, except at d128b4w-6: with the bucket weights scaled by 2^-6 the
    tokens of a document that share a centroid are nearly one vector, and the reference by itself leaves 7 / 651, 262 / 22 971,
    289 / 23 715, 328 / 24 459, 562 / 48 267, 1 684 / 148 707, 2 441 / 190 371 entries ambiguous (1.08-1.34 %, lengths 1 / 31 /
    32 / 33 / 65 / 200 / 256).  That corpus is one of five that run <128, 4>; together they give 0.25-0.31 % per length."""
    geos = [g for g in X.GEOMETRIES if instantiation(g) == inst]
    tally = P.Tally()
    for geo in geos:
        a = X.make_corpus(geo)
        hx = indexes(geo)
        docs = np.arange(len(a["doc_lengths"]), dtype=np.int64)
        qs = X.make_queries(a, lq, 900 + lq)
        try:
            res = hx.score_pairs(qs, [docs] * len(qs))
            assert len(res) == len(qs)
            for qi, (q, (sc, sims, pos)) in enumerate(zip(qs, res)):
                assert sc.shape == (docs.size,) and sims.shape == pos.shape == (docs.size, lq)
                assert sc.dtype == sims.dtype == np.float32 and pos.dtype == np.int32
                P.check_pairs(a, q, docs, sc, sims, pos, what=f"{X.geo_name(geo)} lq{lq} q{qi} ({X.QUERY_KINDS[qi]})", tally=tally)
            st = hx.last_stats
            assert st["n_queries"] == len(qs) and st["n_exact_docs"] == len(qs) * docs.size
            assert st["n_exact_tokens"] == len(qs) * int(np.sum(a["doc_lengths"]))
        finally:
            X.drop_query_cache(a)
    tally.assert_cap(f"pairs_kernel<{inst[0]}, {inst[1]}> lq{lq} ({', '.join(X.geo_name(g) for g in geos)})")


@pytest.mark.parametrize("geo", [G0, (100, 4, 2), (64, 8, 0), (64, 1, 0)], ids=X.geo_name)
def test_same_bits_as_the_search_path(indexes, geo):
    """The ids search_batch(precision=0) and search_exact(precision=0) return, scored as pairs: the same score bits."""
    a = X.make_corpus(geo)
    hx = indexes(geo)
    n = len(a["doc_lengths"])
    p = npa.SearchParameters(n_full_scores=4 * n, top_k=n, n_ivf_probe=X.K, centroid_score_threshold=None, precision=0)
    for lq in (1, 33, 256):
        qs = [q for q, kind in zip(X.make_queries(a, lq, 900 + lq), X.QUERY_KINDS) if kind == "near"]
        for name, found in (("search_batch", hx.search_batch(qs, p)), ("search_exact", hx.search_exact(qs, n + 5, 0))):
            got = hx.score_pairs(qs, [r.passage_ids for r in found], return_matches=False)
            for i, (r, sc) in enumerate(zip(found, got)):
                assert r.passage_ids.size > 0
                assert np.array_equal(u32(sc), u32(r.scores)), f"{X.geo_name(geo)} lq{lq} q{i}: {name}"


@pytest.mark.parametrize("geo", [G0, (96, 2, 0), (64, 8, 0)], ids=X.geo_name)
def test_independence(indexes, geo):
    a = X.make_corpus(geo)
    n = len(a["doc_lengths"])
    docs = np.arange(n, dtype=np.int64)
    hx, hx4 = indexes(geo), indexes(geo, max_batch=4)
    # 700 KiB: slices of four queries and staging chunks of fewer than 200 pairs, which end inside a query's list
    small = indexes(geo, workspace_bytes=700 << 10, max_batch=8)
    g = np.random.default_rng(17)
    perm = np.concatenate([g.permutation(n), g.integers(0, n, 40), [n - 1, n - 1, 3, 3]]).astype(np.int64)
    for qs in (X.make_queries(a, 33, 933), mixed_queries(a)):
        base = hx.score_pairs(qs, [docs] * len(qs))
        for name, r in (("second run", hx.score_pairs(qs, [docs] * len(qs))),
                        ("alone", [hx.score_pairs([q], [docs])[0] for q in qs]),
                        ("max_batch 4", hx4.score_pairs(qs, [docs] * len(qs))),
                        ("several chunks", small.score_pairs(qs, [docs] * len(qs)))):
            for i in range(len(qs)):
                assert same(r[i], base[i]), f"{X.geo_name(geo)} q{i}: {name} differs from the batch"
        for h in (hx, small):
            mixed = h.score_pairs(qs, [perm] * len(qs))
            for i in range(len(qs)):
                want = tuple(x[perm] for x in base[i])
                assert same(mixed[i], want), f"{X.geo_name(geo)} q{i}: permuted list with duplicates"
        one = hx.score_pairs(qs[1], docs[5:6])           # a single matrix and a single pair
        assert same(one[0], tuple(x[5:6] for x in base[1]))


def test_layout_edges(indexes):
    a = X.make_corpus(G0)
    hx = indexes(G0)
    n = len(a["doc_lengths"])
    docs = np.arange(n, dtype=np.int64)
    qs = mixed_queries(a, 55)[:3]
    none = np.zeros(0, np.int64)
    full = hx.score_pairs(qs, [docs] * 3)
    # a query with zero pairs between two with pairs
    res = hx.score_pairs(qs, [docs[:20], none, docs[7:40]])
    assert same(res[0], tuple(x[:20] for x in full[0])) and same(res[2], tuple(x[7:40] for x in full[2]))
    assert res[1][0].shape == (0,) and res[1][1].shape == (0, MIXED[1]) and res[1][2].shape == (0, MIXED[1])
    assert hx.score_pairs(qs, [none, none, none])[2][0].size == 0
    # B = 0
    assert hx.score_pairs([], []) == []
    assert api.lib().np_hip_score_pairs(hx._h, None, None, 0, 128, 0, None, None, None, None, None, None) == 0
    # an empty document: score 0.0, sims -inf, positions -1
    empty = int(np.nonzero(np.asarray(a["doc_lengths"]) == 0)[0][0])
    sc, sims, pos = hx.score_pairs(qs[1], [empty, 3, empty])[0]
    assert u32(sc[0]) == 0 and u32(sc[2]) == 0 and np.all(np.isneginf(sims[[0, 2]])) and np.all(pos[[0, 2]] == -1)
    assert same((sc[1:2], sims[1:2], pos[1:2]), tuple(x[3:4] for x in full[1]))
    # return_matches=False: the same score bits
    for s, f in zip(hx.score_pairs(qs, [docs] * 3, return_matches=False), full):
        assert isinstance(s, np.ndarray) and np.array_equal(u32(s), u32(f[0]))
    # a query without tokens: score 0.0 and empty rows
    sc, sims, pos = hx.score_pairs([np.zeros((0, 128), np.float32), qs[0]], [docs[:4], docs[:4]])[0]
    assert not u32(sc).any() and sims.shape == (4, 0)


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
    picked = g.choice(2049, 40, replace=False)
    qs = [D[p.off[long_doc] + picked].astype(np.float32), D[p.off[long_doc] + 2048][None, :].astype(np.float32)]
    docs = np.array([long_doc, n - 1, 5, long_doc], np.int64)
    hx = hip_index(a, max_query_tokens=256)
    try:
        tally = P.Tally()
        for i, (q, (sc, sims, pos)) in enumerate(zip(qs, hx.score_pairs(qs, [docs, docs]))):
            P.check_pairs(a, q, docs, sc, sims, pos, what=f"long document q{i}", tally=tally)
            assert same((sc[:1], sims[:1], pos[:1]), (sc[3:], sims[3:], pos[3:]))
        # a query made of the document's own tokens finds (a token equal to) each of them; the last token sits in tile 64
        sc, sims, pos = hx.score_pairs(qs, [docs, docs])[1]
        assert pos[0, 0] >= 0 and np.array_equal(D[p.off[long_doc] + pos[0, 0]], D[p.off[long_doc] + 2048])
    finally:
        hx.close()


def test_wide_codes():
    spec, a = make_arrays(num_docs=300, num_centroids=70_000, dim=32, nbits=2, doc_len_min=1, doc_len_max=40)
    hx = hip_index(a, max_query_tokens=256)
    g = np.random.default_rng(5)
    D = X.decompress64(a)
    docs = np.arange(300, dtype=np.int64)
    try:
        qs = [(D[g.integers(0, D.shape[0], lq)] + 0.05 * g.standard_normal((lq, 32))).astype(np.float32) for lq in (1, 33, 40)]
        tally = P.Tally()
        for i, (q, (sc, sims, pos)) in enumerate(zip(qs, hx.score_pairs(qs, [docs] * 3))):
            P.check_pairs(a, q, docs, sc, sims, pos, what=f"wide codes q{i}", tally=tally)
        tally.assert_cap("wide codes")
    finally:
        hx.close()


def test_shards():
    a = X.make_corpus(G0)
    n = len(a["doc_lengths"])
    docs = np.arange(n, dtype=np.int64)
    qs = X.make_queries(a, 33, 977)[:3] + [mixed_queries(a)[2]]
    whole = hip_index(a, max_query_tokens=256)
    shards = [hip_index(a, max_query_tokens=256, shard_rank=r, shard_count=3) for r in range(3)]
    try:
        want = whole.score_pairs(qs, [docs] * len(qs))
        parts = [h.score_pairs(qs, [docs] * len(qs)) for h in shards]
        owner = np.full(n, -1)
        for r, part in enumerate(parts):
            held = ~np.isnan(part[0][0])
            assert held.any() and np.all(owner[held] == -1), "shards overlap"
            owner[held] = r
            assert shards[r].last_stats["n_exact_docs"] == len(qs) * int(held.sum())
        assert np.all(owner >= 0) and np.all(np.diff(owner) >= 0)
        for i in range(len(qs)):
            for r, part in enumerate(parts):
                mine = owner == r
                assert same(tuple(x[mine] for x in part[i]), tuple(x[mine] for x in want[i])), f"q{i} shard {r}: its own pairs"
                sc, sims, pos = (x[~mine] for x in part[i])
                assert np.all(np.isnan(sc)) and np.all(np.isneginf(sims)) and np.all(pos == -1), f"q{i} shard {r}: the others'"
    finally:
        for h in shards + [whole]:
            h.close()


def test_errors(indexes):
    a = X.make_corpus(G0)
    hx = indexes(G0)
    n = len(a["doc_lengths"])
    qs = X.make_queries(a, 5, 3)[:3]
    ids = [np.arange(4, dtype=np.int64), np.zeros(0, np.int64), np.array([n - 1, 0], np.int64)]
    want = hx.score_pairs(qs, ids)
    L = api.lib()
    flat, off = hx._pack(qs)
    pd, po = np.concatenate(ids), np.array([0, 4, 4, 6], np.int64)
    sc, sims, pos = np.zeros(6, np.float32), np.zeros(30, np.float32), np.zeros(30, np.int32)

    def call(dim=128, precision=0, qoff=off, docs=pd, poff=po):
        return L.np_hip_score_pairs(hx._h, api._ptr(flat), api._ptr(qoff), 3, dim, precision, api._ptr(docs), api._ptr(poff),
                                    api._ptr(sc), api._ptr(sims), api._ptr(pos), None)

    def still_fine():
        for r, f in zip(hx.score_pairs(qs, ids), want):
            assert same(r, f)
    assert call() == 0 and np.array_equal(u32(sc), u32(np.concatenate([w[0] for w in want])))
    assert call(dim=64) == 3 and "Shape error" in api.last_error()
    with pytest.raises(npa.ShapeError):
        hx.score_pairs([np.zeros((4, 64), np.float32)], [ids[0]])
    still_fine()
    assert call(qoff=np.array([0, 5, 10, 267], np.int32)) == 3 and "256" in api.last_error()
    with pytest.raises(npa.ShapeError):
        hx.score_pairs([np.zeros((257, 128), np.float32)], [ids[0]])
    still_fine()
    for prec in (2, 3, 1):
        assert call(precision=prec) == 8 and "precision" in api.last_error()
        with pytest.raises(ValueError):
            hx.score_pairs(qs, ids, precision=prec)
    still_fine()
    assert call(poff=np.array([1, 4, 4, 6], np.int64)) == 8 and "pair_offsets[0]" in api.last_error()
    assert call(poff=np.array([0, 4, 3, 6], np.int64)) == 8 and "non-decreasing" in api.last_error()
    with pytest.raises(ValueError):
        hx.score_pairs_csr(qs, pd, np.array([0, 4, 3, 6], np.int64))
    still_fine()
    for bad in (n, -1):
        docs = pd.copy()
        docs[4] = bad
        assert call(docs=docs) == 8 and f"pair 4 names document {bad}" in api.last_error()
        with pytest.raises(ValueError):
            hx.score_pairs(qs, [ids[0], ids[1], np.array([bad, 0])])
        still_fine()
    with pytest.raises(ValueError):
        hx.score_pairs(qs, ids[:2])
    # a 160-wide index opens and refuses, as search does
    spec, wide = make_arrays(num_docs=50, num_centroids=16, dim=160, nbits=4, doc_len_min=4, doc_len_max=4, seed=1)
    h = hip_index(wide)
    with pytest.raises(npa.ShapeError):
        h.score_pairs([np.zeros((4, 160), np.float32)], [np.arange(3)])
    h.close()
    # a budget that cannot hold one query and one pair
    tiny = indexes(G0, workspace_bytes=100_000)
    with pytest.raises(MemoryError):
        tiny.score_pairs(qs, ids)
    still_fine()


def test_device_entry(indexes):
    """np_hip_score_pairs_device on torch tensors and a side stream equals the host entry, bit for bit, also in slices of
    three queries and with either row output left out."""
    import torch
    a = X.make_corpus(G0)
    n = len(a["doc_lengths"])
    qs = mixed_queries(a, 31)
    g = np.random.default_rng(3)
    ids = [g.integers(0, n, k).astype(np.int64) for k in (40, 0, 17, 1, 96, 16, 33, 5)]
    want = indexes(G0).score_pairs(qs, ids)
    hx = hip_index(a, max_query_tokens=256, max_batch=3)
    flat, qoff = hx._pack(qs)
    poff = np.concatenate([[0], np.cumsum([d.size for d in ids])]).astype(np.int64)
    P_, R = int(poff[-1]), int(sum(d.size * q.shape[0] for d, q in zip(ids, qs)))
    dev = torch.device("cuda", 0)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    try:
        d_q, d_qoff = torch.from_numpy(flat).to(dev), torch.from_numpy(qoff).to(dev)
        d_ids, d_poff = torch.from_numpy(np.concatenate(ids)).to(dev), torch.from_numpy(poff).to(dev)
        stream = torch.cuda.Stream()
        for with_sims, with_pos in ((True, True), (True, False), (False, True), (False, False)):
            o_sc = torch.full((P_,), 7.0, dtype=torch.float32, device=dev)
            o_sims = torch.full((R,), 7.0, dtype=torch.float32, device=dev) if with_sims else None
            o_pos = torch.full((R,), 7, dtype=torch.int32, device=dev) if with_pos else None
            torch.cuda.synchronize()
            api._check(api.lib().np_hip_score_pairs_device(
                hx._h, ptr(d_q), ptr(d_qoff), qoff.ctypes.data_as(C.c_void_p), 8, 128, 0, ptr(d_ids), ptr(d_poff),
                poff.ctypes.data_as(C.c_void_p), ptr(o_sc), ptr(o_sims), ptr(o_pos), C.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            assert np.array_equal(u32(o_sc.cpu().numpy()), u32(np.concatenate([w[0] for w in want])))
            if with_sims:
                assert np.array_equal(u32(o_sims.cpu().numpy()), u32(np.concatenate([w[1].reshape(-1) for w in want])))
            if with_pos:
                assert np.array_equal(o_pos.cpu().numpy(), np.concatenate([w[2].reshape(-1) for w in want]))
        # an id outside [0, num_documents) cannot be seen here: it reads as "outside the shard"
        d_bad = torch.from_numpy(np.array([n, -1, 3], np.int64)).to(dev)
        off1 = np.array([0, 3], np.int64)
        d_off1 = torch.from_numpy(off1).to(dev)
        o_sc = torch.zeros(3, dtype=torch.float32, device=dev)
        o_pos = torch.zeros(3, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        api._check(api.lib().np_hip_score_pairs_device(
            hx._h, ptr(d_q), ptr(d_qoff), qoff.ctypes.data_as(C.c_void_p), 1, 128, 0, ptr(d_bad), ptr(d_off1),
            off1.ctypes.data_as(C.c_void_p), ptr(o_sc), None, ptr(o_pos), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        sc = o_sc.cpu().numpy()
        assert np.isnan(sc[0]) and np.isnan(sc[1]) and o_pos.cpu().numpy().tolist()[:2] == [-1, -1]
        assert u32(sc[2:]) == u32(indexes(G0).score_pairs(qs[0], [3])[0][0])
        # the checks run on the host copies here too
        rc = api.lib().np_hip_score_pairs_device(
            hx._h, ptr(d_q), ptr(d_qoff), qoff.ctypes.data_as(C.c_void_p), 8, 128, 3, ptr(d_ids), ptr(d_poff),
            poff.ctypes.data_as(C.c_void_p), ptr(o_sc), None, None, None)
        assert rc == 8 and "precision" in api.last_error()
    finally:
        hx.close()


def test_cpp_mirror_prints_the_same_bits(tmp_path):
    a = X.make_corpus((96, 4, 0))
    n = len(a["doc_lengths"])
    exe = tmp_path / "score_pairs"
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "score_pairs.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    ixdir = tmp_path / "ix"
    ixdir.mkdir()
    synth.write_index(str(ixdir), {k: v for k, v in a.items() if k != "_prep"}, chunk_docs=40)
    qs = [X.make_queries(a, lq, 40 + lq)[i] for i, lq in enumerate((5, 33, 70, 1))]
    ids = [np.arange(0, n, 7, dtype=np.int64), np.zeros(0, np.int64), np.array([n - 1, 3, 3], np.int64), np.arange(20, dtype=np.int64)]
    np.concatenate(qs, 0).astype("<f4").tofile(tmp_path / "q.f32")
    np.array([q.shape[0] for q in qs], "<i8").tofile(tmp_path / "lens.i64")
    np.concatenate(ids).astype("<i8").tofile(tmp_path / "docs.i64")
    np.array([d.size for d in ids], "<i8").tofile(tmp_path / "counts.i64")
    hx = npa.MmapIndex.load(str(ixdir), max_query_tokens=256)
    try:
        out = subprocess.check_output([str(exe), str(ixdir), str(tmp_path / "q.f32"), str(tmp_path / "lens.i64"),
                                       str(tmp_path / "docs.i64"), str(tmp_path / "counts.i64")], text=True)
        want = ""
        for i, (d, (sc, sims, pos)) in enumerate(zip(ids, hx.score_pairs(qs, ids))):
            for j in range(d.size):
                want += f"{i} {d[j]} {u32(sc)[j]:08x}"
                want += "".join(f" {s:08x}:{p}" for s, p in zip(u32(sims[j]).tolist(), pos[j].tolist())) + "\n"
        assert out == want
        assert out.count("\n") == sum(d.size for d in ids) and ":-1" not in out.split("\n")[0]
    finally:
        hx.close()
