"""np_hip_index_expand / _expand_rows and their mirrors (MmapIndex.expand_arrays, update_resident): new centroids, the
buffered tail re-encoded and new documents on a handle that is resident in HBM -- the crate's update in expansion mode.

The contract is the append's sentence with K moving: after an expand the handle is indistinguishable from a handle freshly
opened on the resulting index -- from_arrays of old centroids ++ new and of the old documents without their last n_replace ++
the given ones, or load of the directory update() wrote.  "Equal to fresh" is equal export() arrays, equal info() fields but
device_bytes / workspace_bytes, and equal BYTES from search_batch at every precision (with a threshold, without one through
the zeroth filter level, with a subset), search_exact, score_pairs and decompress_documents.  Needs a real MI355X."""
import os
import subprocess
import threading

import numpy as np
import pytest

from helpers import ROOT, hip_index, make_arrays, synth

import next_plaid_amd as npa
from next_plaid_amd import api

pytestmark = pytest.mark.gpu

INFO_SKIPPED = ("device_bytes", "workspace_bytes")
P = dict(n_full_scores=128, top_k=10, n_ivf_probe=8)


def _base(n, K, dim=32, nbits=4, len_min=4, len_max=40, seed=5):
    return make_arrays(num_docs=n, num_centroids=K, dim=dim, nbits=nbits, doc_len_min=len_min, doc_len_max=len_max, seed=seed)[1]


def _new_centroids(rng, k, dim, scale=1.0):
    c = rng.standard_normal((k, dim)).astype(np.float32)
    return np.ascontiguousarray(scale * c / np.linalg.norm(c, axis=1, keepdims=True), np.float32)


def _docs(rng, lens, pd, lo, hi):
    """documents of the given lengths with uniform codes in [lo, hi) and random residual bytes"""
    T = int(np.sum(lens))
    return np.asarray(lens, np.int64), rng.integers(lo, hi, T).astype(np.int64), rng.integers(0, 256, (T, pd)).astype(np.uint8)


def _final(base, new_cen, given, n_replace):
    """the arrays of the index after the expand: old centroids ++ new, the old documents without their last n_replace ++ given"""
    n_keep = base["doc_lengths"].size - n_replace
    t_keep = int(base["doc_lengths"][:n_keep].sum())
    pd = base["residuals"].shape[1]
    cen = np.concatenate([base["centroids"], np.asarray(new_cen, np.float32).reshape(-1, base["centroids"].shape[1])])
    lens = np.concatenate([base["doc_lengths"][:n_keep], np.asarray(given[0], np.int64)])
    codes = np.concatenate([base["codes"][:t_keep], np.asarray(given[1], np.int64)])
    res = np.concatenate([base["residuals"][:t_keep], np.asarray(given[2], np.uint8).reshape(-1, pd)])
    ivf, il = synth.build_ivf(codes, lens, cen.shape[0])
    return dict(base, centroids=np.ascontiguousarray(cen), doc_lengths=lens, codes=codes, residuals=res, ivf=ivf, ivf_lengths=il)


def _queries(final, docs, n_tokens=8, seed=11):
    """queries made of the tokens of the named documents of `final` (decompressed, a little noise)"""
    lens, codes, res = final["doc_lengths"], final["codes"], final["residuals"]
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)])
    qs = []
    for d in docs:
        if lens[d] == 0:
            continue
        pick = off[d] + rng.integers(0, lens[d], n_tokens)
        v = synth.reconstruct(codes[pick], res[pick], final["centroids"], final["bucket_weights"], final["nbits"])
        v = np.where(np.isfinite(v), v, 0).astype(np.float32)
        v = v + np.float32(0.05) * rng.standard_normal(v.shape).astype(np.float32)
        qs.append(np.ascontiguousarray(v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12), np.float32))
    return qs


def _default_queries(final, n_keep, n=4):
    N = final["doc_lengths"].size
    tail = np.arange(n_keep, N)
    pick = tail[np.argsort(-final["doc_lengths"][tail], kind="stable")[:n]] if tail.size else np.zeros(0, np.int64)
    if pick.size < n:   # nothing (or little) given: the longest kept documents
        pick = np.concatenate([pick, np.argsort(-final["doc_lengths"][:n_keep], kind="stable")[:n - pick.size]])
    return _queries(final, pick.tolist())


def _info(hx):
    return {f: getattr(hx.info, f) for f, _ in api.np_info._fields_ if f not in INFO_SKIPPED}


def _rows(results):
    return [(r.passage_ids.tobytes(), np.asarray(r.scores, np.float32).tobytes()) for r in results]


def _answers(hx, queries, n_keep):
    """every answer the contract names, as bytes"""
    n = hx.num_documents()
    tail = np.arange(min(n_keep, n), n, dtype=np.int64)
    subset = np.concatenate([np.arange(0, min(n_keep, n), 3, dtype=np.int64), tail])
    out = {}
    for prec in (0, 1, 2, 3):
        p = npa.SearchParameters(centroid_score_threshold=0.4, precision=prec, **P)
        out["threshold", prec] = _rows(hx.search_batch(queries, p))
        out["subset", prec] = _rows(hx.search_batch(queries, p, subset=subset))
        p0 = npa.SearchParameters(centroid_score_threshold=None, precision=prec, **P)
        hx.tune("s3_gain", 2)   # the zeroth level whenever it applies: it reads the range table
        out["zeroth level", prec] = _rows(hx.search_batch(queries, p0))
        hx.tune("s3_gain", 1)
    out["exact"] = _rows(hx.search_exact(queries, 10))
    some = np.unique(np.concatenate([tail[:3], tail[-3:], [0, max(n - 1, 0)]]))
    out["pairs"] = [tuple(np.ascontiguousarray(x).tobytes() for x in r) for r in hx.score_pairs(queries, [some] * len(queries))]
    emb, lens = hx.decompress_documents(some[[0, -1]])
    out["decompress"] = (emb.tobytes(), np.asarray(lens).tobytes())
    return out


def _assert_equal_to_fresh(hx, fresh, queries, n_keep, what=""):
    a, b = hx.export(), fresh.export()
    for k in ("doc_lengths", "codes", "residuals", "ivf", "ivf_lengths"):
        assert np.array_equal(a[k], b[k]), f"{what}: export()[{k!r}]"
    assert _info(hx) == _info(fresh), f"{what}: {_info(hx)} vs {_info(fresh)}"
    if hx.num_documents() == 0:
        return
    got, want = _answers(hx, queries, n_keep), _answers(fresh, queries, n_keep)
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], f"{what}: {k}"


def _level_ran(hx, queries):
    p0 = npa.SearchParameters(centroid_score_threshold=None, **P)
    hx.tune("s3_gain", 2)
    hx.search_batch(queries, p0)
    hx.tune("s3_gain", 1)
    return hx.last_stats["n_level0"] > 0


def _check_expand(base, new_cen, given, n_replace=0, reserve=None, queries=None, level_runs=False, then=None, what="", **opts):
    """expand a handle of `base` and compare with a fresh handle of the resulting arrays; `then` = a second expand
    (new_cen, given, n_replace) on the result, compared in the same way"""
    n0 = base["doc_lengths"].size
    final = _final(base, new_cen, given, n_replace)
    hx, fresh = hip_index(base, **opts), hip_index(final, **opts)
    try:
        if reserve:
            hx.reserve(*reserve)
            cap = hx.capacity()
        ids = hx.expand_arrays(new_cen, *given, n_replace=n_replace)
        assert ids.tolist() == list(range(n0 - n_replace, n0 - n_replace + len(given[0])))
        assert hx.num_partitions() == final["centroids"].shape[0]
        if reserve:
            assert hx.capacity() == cap, "an expand within the reservation reallocated"
        qs = _default_queries(final, n0 - n_replace) if queries is None else queries
        _assert_equal_to_fresh(hx, fresh, qs, n0 - n_replace, what)
        if level_runs:
            assert _level_ran(fresh, qs) and _level_ran(hx, qs), "the zeroth level did not run: nothing read the range table"
        if then is not None:
            final2 = _final(final, *then)
            fresh2 = hip_index(final2, **opts)
            try:
                hx.expand_arrays(then[0], *then[1], n_replace=then[2])
                n_keep2 = final["doc_lengths"].size - then[2]
                _assert_equal_to_fresh(hx, fresh2, _default_queries(final2, n_keep2), n_keep2, what + " (second expand)")
                if reserve:
                    assert hx.capacity() == cap
            finally:
                fresh2.close()
    finally:
        hx.close()
        fresh.close()


# ---- K within a 64-multiple and across one ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["old codes", "new codes", "both"])
@pytest.mark.parametrize("K0,K1,dim", [(64, 65, 32), (60, 64, 128), (64, 200, 32), (64, 65, 128)])
def test_k_grows_within_and_across_a_multiple_of_64(K0, K1, dim, which):
    base = _base(300, K0, dim=dim)
    rng = np.random.default_rng(K1)
    lo, hi = {"old codes": (0, K0), "new codes": (K0, K1), "both": (0, K1)}[which]
    given = _docs(rng, rng.integers(4, 41, 24), base["residuals"].shape[1], lo, hi)
    _check_expand(base, _new_centroids(rng, K1 - K0, dim), given, what=f"K {K0} -> {K1}, {which}")


def test_the_eighths_of_the_centroid_range_move():
    """K 64 -> 128: an eighth is 8 centroids before and 16 after; old documents hold codes on both sides of both boundaries.
    The sliced S4 kernels (8, 4, 2 phases over the centroid range, lockstep and streamed) read d_useg"""
    base = _base(300, 64)
    off = np.concatenate([[0], np.cumsum(base["doc_lengths"])])
    edges = np.array([7, 8, 15, 16, 23, 24, 31, 32, 47, 48, 63, 0], np.int64)
    for d in range(0, 300, 2):
        L = int(base["doc_lengths"][d])
        base["codes"][off[d]:off[d + 1]] = edges[(np.arange(L) + d) % edges.size]
    base["ivf"], base["ivf_lengths"] = synth.build_ivf(base["codes"], base["doc_lengths"], 64)
    rng = np.random.default_rng(3)
    new_cen = _new_centroids(rng, 64, 32)
    given = _docs(rng, rng.integers(4, 41, 20), 16, 0, 128)
    final = _final(base, new_cen, given, 0)
    qs = _queries(final, list(range(0, 16, 2)) + list(range(300, 308)))
    _check_expand(base, new_cen, given, queries=qs[:4])
    hx, fresh = hip_index(base), hip_index(final)
    try:
        hx.expand_arrays(new_cen, *given)
        p = npa.SearchParameters(centroid_score_threshold=0.4, **P)
        for h in (hx, fresh):
            h.tune("s4_minb", 1)
        for filt in (0, 1):
            for mode in (1, 2, 3, 5, 6):
                for h in (hx, fresh):
                    h.tune("s4_filter", filt)
                    h.tune("s4_mode", mode)
                assert _rows(hx.search_batch(qs, p)) == _rows(fresh.search_batch(qs, p)), f"S4 mode {mode}, filter {filt}"
    finally:
        hx.close()
        fresh.close()


def test_centroids_only():
    """n_docs = 0: the new centroids have empty posting lists; a query placed on one probes an empty list"""
    base = _base(300, 64)
    rng = np.random.default_rng(4)
    new_cen = _new_centroids(rng, 5, 32)
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 16), np.uint8))
    q = np.ascontiguousarray(np.repeat(new_cen[2:3], 8, 0) + np.float32(0.01) * rng.standard_normal((8, 32)).astype(np.float32))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    qs = _queries(base, [0, 1, 2]) + [np.ascontiguousarray(q, np.float32)]
    _check_expand(base, new_cen, empty, queries=qs, what="centroids only")


def test_no_centroid_and_no_replacement_is_an_append():
    base = _base(300, 64)
    rng = np.random.default_rng(6)
    given = _docs(rng, rng.integers(0, 30, 12), 16, 0, 64)
    a, b = hip_index(base), hip_index(base)
    try:
        ia = a.expand_arrays(np.zeros((0, 32), np.float32), *given, n_replace=0)
        ib = b.append_arrays(*given)
        assert ia.tolist() == ib.tolist()
        ea, eb = a.export(), b.export()
        for k in ea:
            assert np.array_equal(ea[k], eb[k]), k
        assert _info(a) == _info(b)
        info, cap = _info(a), a.capacity()
        assert a.expand_arrays(np.zeros((0, 32), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 16), np.uint8)).size == 0
        assert _info(a) == info and a.capacity() == cap   # all three zero: nothing changes
    finally:
        a.close()
        b.close()


# ---- the tail replaced ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_replace,n_given", [(1, 3), (64, 70), (65, 65), (130, 140)])
def test_the_tail_is_replaced(n_replace, n_given):
    """1, 64, 65 (a ballot word crossed) and ALL of the handle's 130 documents; n_replace = n_docs (nothing new) at 65.  The
    replaced documents have other lengths than before, one of them none"""
    base = _base(130, 64)
    rng = np.random.default_rng(n_replace)
    lens = rng.integers(4, 41, n_given)
    lens[0] = 0
    lens[-1] = int(base["doc_lengths"][-1]) + 3
    _check_expand(base, _new_centroids(rng, 7, 32), _docs(rng, lens, 16, 0, 71), n_replace=n_replace,
                  what=f"replace {n_replace}, give {n_given}")


def test_the_tail_is_replaced_without_new_centroids():
    base = _base(130, 64)
    rng = np.random.default_rng(8)
    _check_expand(base, np.zeros((0, 32), np.float32), _docs(rng, rng.integers(0, 41, 9), 16, 0, 64), n_replace=5)


def test_the_longest_document_leaves():
    """max_doc_len follows the kept and the given documents"""
    base = _base(130, 64)
    rng = np.random.default_rng(9)
    long = _docs(rng, [700, 3], 16, 0, 64)
    hx = hip_index(base)
    try:
        hx.append_arrays(*long)
        grown = _final(base, np.zeros((0, 32), np.float32), long, 0)
        given = _docs(rng, [5, 6, 7], 16, 0, 66)
        new_cen = _new_centroids(rng, 2, 32)
        hx.expand_arrays(new_cen, *given, n_replace=2)
        final = _final(grown, new_cen, given, 2)
        fresh = hip_index(final)
        try:
            _assert_equal_to_fresh(hx, fresh, _default_queries(final, 130), 130)
        finally:
            fresh.close()
    finally:
        hx.close()


@pytest.mark.parametrize("n0,n_replace,n_given", [(32770, 5, 5), (32766, 1, 5)])
def test_the_range_table_across_a_range_boundary(n0, n_replace, n_given):
    """NP_IVF_SPLIT_RANGE = 32768.  32 770 one-to-three-token documents whose last 5 (ids on both sides of the boundary) are
    replaced; 32 766 documents, the last replaced and four new ones: n_ranges goes 1 -> 2.  (The shrinking direction, "replace
    the last 5 by 1", is n_replace > n_docs, which the entry refuses by name: test_refused_expands_change_nothing.)"""
    base = _base(n0, 64, len_min=1, len_max=3)
    rng = np.random.default_rng(n0)
    _check_expand(base, _new_centroids(rng, 3, 32), _docs(rng, rng.integers(1, 4, n_given), 16, 0, 67), n_replace=n_replace,
                  level_runs=True)


# ---- the codes widen ---------------------------------------------------------------------------------------------------------------
def _wide_case(K0, K1, reserve=None, n_replace=0, **opts):
    base = _base(200, K0, nbits=2, len_min=1, len_max=12)
    base["codes"][::7] = K0 - 1           # old documents hold the last old code (65 535 where K = 65 536)
    base["codes"][3::11] = 0
    base["ivf"], base["ivf_lengths"] = synth.build_ivf(base["codes"], base["doc_lengths"], K0)
    rng = np.random.default_rng(K1)
    lens = rng.integers(1, 13, 14)
    given = _docs(rng, lens, 8, 65000, K1)
    given[1][::3] = K1 - 1
    given[1][1::3] = max(K0, min(65536, K1 - 1))   # the first wide code where there is one
    given[1][2::5] = min(65535, K1 - 1)
    _check_expand(base, _new_centroids(rng, K1 - K0, 32), given, n_replace=n_replace, reserve=reserve, what=f"K {K0} -> {K1}", **opts)


@pytest.mark.parametrize("K0,K1", [(65530, 65542), (65536, 65537)])
@pytest.mark.parametrize("reserve", [None, (50, 600)])
def test_codes_widen(K0, K1, reserve):
    _wide_case(K0, K1, reserve=reserve, n_replace=3)


def test_codes_widen_in_the_code_ordered_token_layout(monkeypatch):
    monkeypatch.setenv("NP_TOK_SORT", "1")
    _wide_case(65536, 65537, n_replace=3)
    _wide_case(65530, 65542, reserve=(50, 600))


def test_wide_codes_get_wider():
    _wide_case(65600, 65700, n_replace=2)


# ---- the bounds of the centroid table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["magnitude 2e6", "inf"])
def test_bounds_follow_the_new_centroids(kind):
    """a new centroid of magnitude 2e6 (s6_fast_ok drops) or with an inf (filter_ok drops): answers as on the fresh handle"""
    base = _base(300, 64)
    rng = np.random.default_rng(12)
    new_cen = _new_centroids(rng, 3, 32)
    if kind == "inf":
        new_cen[1, 5] = np.inf
    else:
        new_cen[1] *= np.float32(2e6)
    given = _docs(rng, rng.integers(4, 41, 12), 16, 0, 67)
    given[1][given[1] == 65] = 64   # no token sits on the odd centroid: the queries stay finite
    final = _final(base, new_cen, given, 0)
    _check_expand(base, new_cen, given, queries=_queries(final, [300, 301, 2, 3]), what=kind)


# ---- reservation, other geometries ---------------------------------------------------------------------------------------------
def test_two_expands_inside_a_reservation():
    base = _base(300, 64)
    rng = np.random.default_rng(13)
    one = (_new_centroids(rng, 4, 32), _docs(rng, rng.integers(4, 41, 10), 16, 0, 68), 0)
    two = (_new_centroids(rng, 70, 32), _docs(rng, rng.integers(4, 41, 12), 16, 0, 138), 10)
    _check_expand(base, one[0], one[1], reserve=(40, 1200), then=two)


@pytest.mark.parametrize("nbits,dim", [(1, 96), (4, 48), (8, 64), (2, 128)])
def test_other_geometries(nbits, dim):
    """nbits 1 (file rows repacked to 2-bit storage rows), a dim that is no kernel width (rows padded), nbits 8"""
    base = _base(200, 64, dim=dim, nbits=nbits)
    rng = np.random.default_rng(dim)
    _check_expand(base, _new_centroids(rng, 9, dim), _docs(rng, rng.integers(4, 41, 10), dim * nbits // 8, 0, 73), n_replace=4)


# ---- refused, and the handle answers as before -----------------------------------------------------------------------------------
def _refused(hx, queries, call, exc, match):
    p = npa.SearchParameters(**P)
    before, info, ex = _rows(hx.search_batch(queries, p)), _info(hx), hx.export()
    with pytest.raises(exc, match=match):
        call()
    after = hx.export()
    assert _rows(hx.search_batch(queries, p)) == before and _info(hx) == info
    for k in ex:
        assert np.array_equal(ex[k], after[k]), k


def _raw(hx, cen, k_new, n_replace, lens, n_docs, codes, res):
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    api._check(api.lib().np_hip_index_expand(hx._h, ptr(cen), k_new, n_replace, ptr(lens), n_docs, ptr(codes), ptr(res)))


def test_refused_expands_change_nothing():
    base = _base(200, 64)
    rng = np.random.default_rng(14)
    cen = _new_centroids(rng, 3, 32)
    lens, codes, res = _docs(rng, rng.integers(4, 41, 6), 16, 0, 67)
    qs = _queries(base, [0, 1, 2])
    with pytest.raises(ValueError, match="np_hip_index_expand: index is NULL"):
        api._check(api.lib().np_hip_index_expand(None, None, 0, 0, None, 0, None, None))
    hx = hip_index(base, shard_rank=0, shard_count=2)
    try:
        _refused(hx, qs, lambda: hx.expand_arrays(cen, lens, codes, res), ValueError, r"np_hip_index_expand: index is a shard \(0 of 2\)")
    finally:
        hx.close()
    desc = dict(base)
    off = np.concatenate([[0], np.cumsum(base["ivf_lengths"])])
    desc["ivf"] = np.concatenate([base["ivf"][a:b][::-1] for a, b in zip(off[:-1], off[1:])])
    hx = hip_index(desc)
    try:
        _refused(hx, qs, lambda: hx.expand_arrays(cen, lens, codes, res), ValueError, "do not ascend")
    finally:
        hx.close()
    hx = hip_index(base)
    try:
        _refused(hx, qs, lambda: _raw(hx, cen, -1, 0, lens, 6, codes, res), ValueError, "k_new is negative")
        _refused(hx, qs, lambda: _raw(hx, None, 3, 0, lens, 6, codes, res), ValueError, "new_centroids is NULL")
        _refused(hx, qs, lambda: hx.expand_arrays(cen, lens, codes, res, n_replace=-1), ValueError, "n_replace is -1")
        _refused(hx, qs, lambda: hx.expand_arrays(cen, lens, codes, res, n_replace=7), ValueError, "n_replace is 7")
        many = _docs(rng, np.ones(201, np.int64), 16, 0, 67)
        _refused(hx, qs, lambda: hx.expand_arrays(cen, *many, n_replace=201), ValueError, "n_replace is 201.*handle's 200 documents")
        neg = lens.copy()
        neg[2] = -1
        _refused(hx, qs, lambda: hx.expand_arrays(cen, neg, codes, res), npa.ShapeError, r"doc_lengths\[2\] is negative")
        bad = codes.copy()
        bad[-1] = 67
        _refused(hx, qs, lambda: hx.expand_arrays(cen, lens, bad, res), ValueError, r"codes\[\d+\] = 67 is outside \[0, 67\)")
        bad[-1] = -1
        _refused(hx, qs, lambda: hx.expand_arrays(cen, lens, bad, res), ValueError, r"codes\[\d+\] = -1")
        _refused(hx, qs, lambda: _raw(hx, cen, (1 << 31) - 64, 0, lens, 6, codes, res), ValueError, "k_new: .*32-bit device id space")
        _refused(hx, qs, lambda: _raw(hx, cen, 3, 0, None, (1 << 31), None, None), ValueError, "doc_lengths is NULL")
        _refused(hx, qs, lambda: _raw(hx, cen, 3, 0, lens, -1, codes, res), ValueError, "n_docs is negative")
        _refused(hx, qs, lambda: _raw(hx, cen, 3, 0, lens, 1 << 31, codes, res), ValueError, "n_docs: a shard holds < 2\\^31 documents")
    finally:
        hx.close()


@pytest.mark.parametrize("stage", [1, 2, 3, 4])
@pytest.mark.parametrize("case", ["narrow", "widening, code-ordered tokens"])
def test_a_failure_before_the_swap_puts_the_handle_back(case, stage, monkeypatch):
    """np_hip_index_tune "expand_fail": the call returns OutOfMemory after the given stage, as a refused allocation there would
    -- the given tokens already lie on the old tail, K, the code width and the centroid table are already the grown ones.  The
    handle's export, info and answers are what they were, and the same expand then succeeds and equals the fresh handle"""
    if case == "narrow":
        base, k_new, n_replace = _base(130, 64), 7, 33
    else:
        monkeypatch.setenv("NP_TOK_SORT", "1")
        base, k_new, n_replace = _base(130, 65536, nbits=2), 1, 3
        base["codes"][::5] = 65535
        base["ivf"], base["ivf_lengths"] = synth.build_ivf(base["codes"], base["doc_lengths"], 65536)
    K0, pd = base["centroids"].shape[0], base["residuals"].shape[1]
    rng = np.random.default_rng(stage)
    new_cen = _new_centroids(rng, k_new, 32)
    given = _docs(rng, rng.integers(4, 41, n_replace + 9), pd, K0 - 40, K0 + k_new)
    given[1][::4] = K0 + k_new - 1
    final = _final(base, new_cen, given, n_replace)
    qs = _queries(base, [100, 127, 128, 129])
    hx, fresh = hip_index(base), hip_index(final)
    try:
        hx.tune("expand_fail", stage)
        _refused(hx, qs, lambda: hx.expand_arrays(new_cen, *given, n_replace=n_replace), MemoryError, f"out of memory after stage {stage}")
        assert hx.num_partitions() == K0
        hx.tune("expand_fail", 0)
        hx.expand_arrays(new_cen, *given, n_replace=n_replace)
        _assert_equal_to_fresh(hx, fresh, _default_queries(final, 130 - n_replace), 130 - n_replace, f"{case}, after stage {stage}")
    finally:
        hx.close()
        fresh.close()


# ---- attachments -----------------------------------------------------------------------------------------------------------------
LANGS = ["de", "en", "fr", "it"]


def _values(n, seed, extra=()):
    rng = np.random.default_rng(seed)
    r = rng.random((2, n))
    s = [None if r[1, d] < 0.2 else LANGS[j] for d, j in enumerate(rng.integers(0, len(LANGS), n))]
    for j, x in enumerate(extra):
        s[2 * j] = x
    return {"i": rng.integers(-5, 50, n), "f": np.where(r[0] < 0.25, np.nan, rng.standard_normal(n)), "s": s}


def _cat(a, b):
    return {k: (list(a[k]) + list(b[k]) if isinstance(a[k], list) else np.concatenate([a[k], b[k]])) for k in a}


FILTERS = [("i >= ?", (10,)), ("f < ? OR f IS NULL", (0.0,)), ("s = ?", ("fr",)), ("s IN (?, ?)", ("de", "ea"))]


def _attached_answers(hx, qs):
    p = npa.SearchParameters(**P)
    out = {"filter_ids": [x.tobytes() for x in hx.filter_ids(FILTERS)],
           "filtered": _rows(hx.search_batch(qs, p, filters=[FILTERS[i % len(FILTERS)] for i in range(len(qs))]))}
    raw = hx.search_grouped(qs, p, group_size=2, raw=True)
    out["grouped"] = [None if x is None else np.ascontiguousarray(x).tobytes() for x in raw]
    return out


def _rows_case(n0=130, n_replace=33, n_given=45, extra=("aa", "ea", "zz")):
    """(base, new centroids, given, n_replace, old values, old groups, new values, new groups, n_groups, final arrays)"""
    base = _base(n0, 64)
    rng = np.random.default_rng(21)
    new_cen = _new_centroids(rng, 6, 32)
    given = _docs(rng, rng.integers(4, 41, n_given), 16, 0, 70)
    n_new = n_given - n_replace
    old_vals, new_vals = _values(n0, 1), _values(n_new, 2, extra=extra)   # the dictionary grows in front, between, behind
    old_g, new_g = (np.arange(n0) % 9).astype(np.int32), (np.arange(n_new) % 11).astype(np.int32)
    return base, new_cen, given, n_replace, old_vals, old_g, new_vals, new_g, 11, _final(base, new_cen, given, n_replace)


def test_expand_rows_keeps_columns_and_groups():
    """i64, f64 with NULLs, text with a dictionary that grows, and groups through an expand with n_replace > 0: the replaced
    documents keep their rows, the rows given cover the new documents only"""
    base, new_cen, given, n_replace, old_vals, old_g, new_vals, new_g, n_groups, final = _rows_case()
    n0 = 130
    hx, fresh = hip_index(base), hip_index(final)
    try:
        hx.set_columns(old_vals)
        hx.set_groups(old_g, n_groups=9)
        ids = hx.expand_arrays(new_cen, *given, n_replace=n_replace, rows=api.AppendRows(columns=new_vals, groups=new_g, n_groups=n_groups))
        assert ids.tolist() == list(range(n0 - n_replace, n0 - n_replace + len(given[0]))) and hx.num_documents() == n0 + 12
        fresh.set_columns(_cat(old_vals, new_vals))
        fresh.set_groups(np.concatenate([old_g, new_g]), n_groups=n_groups)
        assert hx.group_count() == fresh.group_count() == n_groups
        assert np.array_equal(hx.get_groups(), fresh.get_groups())
        for name in old_vals:
            (d1, v1), (d2, v2) = hx.get_column(name), fresh.get_column(name)
            assert d1.tobytes() == d2.tobytes() and (v1 is None) == (v2 is None) and (v1 is None or np.array_equal(v1, v2)), name
            assert hx.schema[name].dictionary == fresh.schema[name].dictionary
        qs = _default_queries(final, n0 - n_replace)
        assert _attached_answers(hx, qs) == _attached_answers(fresh, qs)
        ea, eb = hx.export(), fresh.export()
        for k in ea:
            assert np.array_equal(ea[k], eb[k]), k
    finally:
        hx.close()
        fresh.close()


def test_plain_expand_drops_the_attachments():
    base, new_cen, given, n_replace, old_vals, old_g, *_ = _rows_case()
    hx = hip_index(base)
    try:
        hx.set_columns(old_vals)
        hx.set_groups(old_g, n_groups=9)
        hx.expand_arrays(new_cen, *given, n_replace=n_replace)
        assert hx.schema is None and hx.group_values is None and hx.group_count() == 0
        with pytest.raises(ValueError, match="outside the handle's 0 columns"):
            api._check(api.lib().np_hip_index_get_column(hx._h, 0, None, None, None, None))
    finally:
        hx.close()


def test_expand_rows_refusals_are_the_appends():
    base, new_cen, given, n_replace, old_vals, old_g, new_vals, new_g, n_groups, _ = _rows_case()
    hx = hip_index(base)
    try:
        hx.set_columns(old_vals)
        hx.set_groups(old_g, n_groups=9)
        want = hx.get_column("i")[0].tobytes()
        lens, codes, res = (np.ascontiguousarray(x) for x in given)
        cols = (api.np_column * 2)(api.np_column(0, 0, new_vals["i"].ctypes.data, None), api.np_column(1, 0, new_vals["f"].ctypes.data, None))
        rc = api.lib().np_hip_index_expand_rows(hx._h, new_cen.ctypes.data, 6, n_replace, lens.ctypes.data, lens.size, codes.ctypes.data,
                                                res.ctypes.data, cols, 2, None, new_g.ctypes.data, n_groups)
        assert rc != 0 and "np_hip_index_expand_rows: n_cols is 2, the handle has 3 columns" in api.last_error()
        assert hx.num_documents() == 130 and hx.num_partitions() == 64 and hx.get_column("i")[0].tobytes() == want
    finally:
        hx.close()


# ---- under traffic -----------------------------------------------------------------------------------------------------------------
def _beside(hx, answers, pre, post, expand, n_threads=2):
    """threads ask in a loop while the main thread expands once: every answer is the old index's or the new one's"""
    done = threading.Event()
    started = [threading.Event() for _ in range(n_threads)]
    seen, errors = [[] for _ in range(n_threads)], []

    def worker(i):
        try:
            after = 0
            while after < 2:
                was = done.is_set()
                seen[i].append((was, answers(hx)))
                started[i].set()
                after += was
        except Exception as e:   # noqa: BLE001
            errors.append(e)
            started[i].set()

    threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(n_threads)]
    for t in threads:
        t.start()
    for ev in started:
        assert ev.wait(60)
    expand()
    done.set()
    for t in threads:
        t.join(60)
    assert not errors and not any(t.is_alive() for t in threads), errors
    for i in range(n_threads):
        for was, got in seen[i]:
            for k in post:
                assert got[k] == post[k] or (not was and got[k] == pre[k]), f"thread {i}: {k}"
    assert answers(hx) == post


def test_expand_under_traffic():
    """n_replace > 0 and k_new > 0 beside searching threads: never an answer that lacks the replaced documents, never K1
    centroids without their documents"""
    base = _base(3000, 64)
    rng = np.random.default_rng(31)
    new_cen = _new_centroids(rng, 40, 32)
    given = _docs(rng, rng.integers(10, 41, 90), 16, 0, 104)
    final = _final(base, new_cen, given, 50)
    qs = _queries(final, [2950, 2951, 3000, 3001]) + _queries(base, [2960, 2961])
    p = npa.SearchParameters(**P)
    answers = lambda h: {"rows": _rows(h.search_batch(qs, p, parallel=False))}   # noqa: E731
    fresh = hip_index(final)
    try:
        post = answers(fresh)
    finally:
        fresh.close()
    hx = hip_index(base, n_contexts=2)
    try:
        pre = answers(hx)
        assert all(a != b for a, b in zip(pre["rows"], post["rows"])), "the queries do not tell the two states apart"
        _beside(hx, answers, pre, post, lambda: hx.expand_arrays(new_cen, *given, n_replace=50), n_threads=4)
    finally:
        hx.close()


def test_filtered_and_grouped_searches_beside_expand_rows():
    """filter_ids, filtered and grouped searches on a second thread see the old index with the old rows or the new with the
    new, never a mixture (no new string here: both states compile their filters against the same dictionaries)"""
    base, new_cen, given, n_replace, old_vals, old_g, new_vals, new_g, n_groups, final = _rows_case(n0=2000, n_replace=40, n_given=100,
                                                                                                    extra=())
    qs = _default_queries(final, 1960)
    fresh = hip_index(final)
    try:
        fresh.set_columns(_cat(old_vals, new_vals))
        fresh.set_groups(np.concatenate([old_g, new_g]), n_groups=n_groups)
        grown = fresh.schema["s"].dictionary
        assert len(grown) == len(LANGS)
        post = _attached_answers(fresh, qs)
    finally:
        fresh.close()
    hx = hip_index(base, n_contexts=2)
    try:
        hx.set_columns(old_vals)
        hx.set_groups(old_g, n_groups=9)
        assert hx.schema["s"].dictionary == grown   # no new string: one dictionary before and after
        pre = _attached_answers(hx, qs)
        assert pre["filtered"] != post["filtered"] and pre["grouped"] != post["grouped"], "the queries do not tell the two states apart"
        sch, new, remaps, gids, ng, _ = hx._plan_rows(api.AppendRows(columns=new_vals, groups=new_g, n_groups=n_groups), 60)
        assert all(r is None for r in remaps.values())
        cols = (api.np_column * 3)()
        for c in new.values():
            cols[c.index] = api.np_column(c.type, 0, c.data.ctypes.data, None if c.valid is None else c.valid.ctypes.data)
        lens, codes, res = (np.ascontiguousarray(x) for x in given)

        def expand():
            api._check(api.lib().np_hip_index_expand_rows(hx._h, new_cen.ctypes.data, new_cen.shape[0], n_replace, lens.ctypes.data,
                                                          lens.size, codes.ctypes.data, res.ctypes.data, cols, 3, None, gids.ctypes.data, ng))

        def answers(h):
            # the mirror's filter_ids counts and fetches in two library calls: an expand that lands between them is met by the
            # library's refusal of the now too small array, and the call is made again
            for attempt in range(3):
                try:
                    return _attached_answers(h, qs)
                except ValueError as e:
                    if "ids_capacity" not in str(e) or attempt == 2:
                        raise

        _beside(hx, answers, pre, post, expand, n_threads=1)
    finally:
        hx.close()


# ---- on a directory ----------------------------------------------------------------------------------------------------------------
def _far_docs(rng, n, dim, len_max=12):
    docs = []
    for _ in range(n):
        x = rng.standard_normal((int(rng.integers(2, len_max)), dim)).astype(np.float32)
        docs.append(np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), np.float32))
    return docs


def _assert_equal_to_load(hx, path, docs, what):
    fresh = npa.MmapIndex.load(path)
    try:
        qs = [np.ascontiguousarray(x[:8], np.float32) for x in docs[:4]]
        _assert_equal_to_fresh(hx, fresh, qs, max(hx.num_documents() - len(docs), 0), what)
    finally:
        fresh.close()


def test_update_resident_on_a_directory(tmp_path):
    """buffer_size 5: three documents are buffered, four more expand (the three re-indexed, new centroids), six expand again"""
    spec, a = make_arrays(num_docs=600, num_centroids=256, dim=64, nbits=4, doc_len_min=1, doc_len_max=24, seed=3)
    cut, wts = synth.bucket_tables(spec)
    d = str(tmp_path / "a")
    npa.write_index_dir(d, a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=500)
    cfg = npa.UpdateConfig(start_from_scratch=-1, buffer_size=5, kmeans_niters=3, max_points_per_centroid=16, seed=11)
    rng = np.random.default_rng(2)
    hx = npa.MmapIndex.load(d)
    try:
        hx.set_columns({"year": np.arange(600)})
        docs = _far_docs(rng, 3, 64)
        ids = hx.update_resident(docs, cfg)
        rep = hx.last_update
        assert rep["mode"] == "buffer" and ids.tolist() == [600, 601, 602] == list(range(rep["first_doc_id"], rep["first_doc_id"] + 3))
        assert hx.num_documents() == 603 and hx.schema is None
        _assert_equal_to_load(hx, d, docs, "buffered")
        docs = _far_docs(rng, 4, 64)
        ids = hx.update_resident(docs, cfg)
        rep = hx.last_update
        assert rep["mode"] == "expansion" and rep["n_reindexed"] == 3 and rep["n_new_centroids"] > 0
        assert ids.tolist() == [603, 604, 605, 606] == list(range(rep["first_doc_id"], rep["first_doc_id"] + 4))
        k1 = 256 + rep["n_new_centroids"]
        assert hx.num_documents() == 607 and hx.num_partitions() == k1
        _assert_equal_to_load(hx, d, docs, "expanded")
        docs = _far_docs(rng, 6, 64)
        ids = hx.update_resident(docs, cfg)
        rep = hx.last_update
        assert rep["mode"] == "expansion" and rep["n_reindexed"] == 0 and rep["n_new_centroids"] > 0
        assert ids.tolist() == list(range(607, 613)) and hx.num_partitions() == k1 + rep["n_new_centroids"]
        _assert_equal_to_load(hx, d, docs, "expanded again")
        npa.MmapIndex.update_append(docs[:1], d)   # somebody else's update: the handle is now behind its directory
        with pytest.raises(npa.IndexLoadError, match="not current"):
            hx.update_resident(docs, cfg)
    finally:
        hx.close()


def test_update_resident_reloads_a_small_index(tmp_path):
    """the default config on a small index takes the start-from-scratch mode: the handle is reloaded"""
    rng = np.random.default_rng(1)
    cen = rng.standard_normal((64, 64)).astype(np.float32)
    docs = []
    for _ in range(330):
        L = int(rng.integers(2, 20))
        x = cen[rng.integers(0, 64, L)] + 0.3 * rng.standard_normal((L, 64)).astype(np.float32)
        docs.append((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))
    d = str(tmp_path / "a")
    hx = npa.MmapIndex.create_with_kmeans(docs[:300], d, npa.IndexConfig(nbits=4, batch_size=100, seed=5))
    try:
        hx.set_columns({"year": np.arange(300)})
        ids = hx.update_resident(docs[300:])
        assert hx.last_update["mode"] == "start_from_scratch" and ids.tolist() == list(range(300, 330))
        assert hx.num_documents() == 330 and hx.schema is None
        _assert_equal_to_load(hx, d, docs[300:], "start from scratch")
    finally:
        hx.close()


def test_cpp_mirror_expands(tmp_path):
    """tests/cpp/expand_index.cpp: next_plaid.hpp's expand_arrays and update_resident on a written directory"""
    spec, a = make_arrays(num_docs=600, num_centroids=256, dim=64, nbits=4, doc_len_min=1, doc_len_max=24, seed=3)
    cut, wts = synth.bucket_tables(spec)
    d = tmp_path / "ix"
    npa.write_index_dir(str(d), a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=500)
    rng = np.random.default_rng(5)
    lens, codes, res = _docs(rng, rng.integers(1, 20, 9), 32, 0, 259)
    lens.tofile(tmp_path / "lens.bin")
    codes.tofile(tmp_path / "codes.bin")
    res.tofile(tmp_path / "res.bin")
    _new_centroids(rng, 3, 64).tofile(tmp_path / "cen.bin")
    far = _far_docs(rng, 7, 64)
    np.concatenate(far).tofile(tmp_path / "emb.bin")
    np.array([x.shape[0] for x in far], np.int64).tofile(tmp_path / "emb_lens.bin")
    exe = tmp_path / "expand_index"
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "expand_index.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    r = subprocess.run([str(exe), str(d), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    hx = npa.MmapIndex.load(str(d))   # the directory the C++ update_resident left loads, with the centroids it added
    try:
        assert hx.num_documents() == 607 and hx.num_partitions() > 256
    finally:
        hx.close()
