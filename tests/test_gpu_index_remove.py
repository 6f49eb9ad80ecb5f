"""np_hip_index_remove / MmapIndex.remove and remove_ids: documents taken out of a handle that is resident in HBM.

The contract under test is one sentence: after a remove the handle is indistinguishable from a handle freshly opened on the
resulting index -- from_arrays of remove_restate.shrunk_arrays (the base's OWN lists filtered and renumbered), or load of the
directory np_hip_index_delete wrote.  "Equal to fresh" (_assert_equal_to_fresh) is equal export() arrays, equal info() fields
but device_bytes / workspace_bytes, and equal BYTES from search_batch at every precision (with a threshold, without one
through the zeroth filter level, with a subset), search_exact, score_pairs and decompress_documents of the first and last
survivor.  Needs a real MI355X."""
import json
import os
import re
import shutil
import subprocess
import threading

import numpy as np
import pytest

import remove_restate as R
import update_restate as U
from helpers import ROOT, hip_index, make_arrays, synth

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu

GEOM = dict(num_centroids=256, dim=64, nbits=4, doc_len_min=1, doc_len_max=24)
INFO_SKIPPED = ("device_bytes", "workspace_bytes")
FILTER_TILE = 4096     # NP_FILTER_TILE: posting-list entries per workgroup of ivf_filter_kernel
COMPACT_TILE = 16384   # NP_COMPACT_TILE: destination bytes per workgroup of token_compact_kernel


def _base(n, seed=5, **kw):
    return make_arrays(num_docs=n, seed=seed, **dict(GEOM, **kw))[1]


def _custom(lens, seed, codes=None, **kw):
    """an index of documents with the given lengths: a synthetic codec, uniform codes (or the given ones), random residual
    bytes, the posting lists of the codes (index.rs:479-499)"""
    a = _base(8, **kw)
    K, pd = a["centroids"].shape[0], a["residuals"].shape[1]
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    T = int(lens.sum())
    codes = rng.integers(0, K, T).astype(np.int64) if codes is None else np.asarray(codes, np.int64)
    ivf, il = synth.build_ivf(codes, lens, K)
    return dict(a, doc_lengths=lens, codes=codes, residuals=rng.integers(0, 256, (T, pd)).astype(np.uint8), ivf=ivf, ivf_lengths=il)


def _queries(a, n_queries=4, n_tokens=8, seed=11):
    """queries made of the tokens of the longest documents of `a` (decompressed, a little noise)"""
    lens, codes, res = a["doc_lengths"], a["codes"], a["residuals"]
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)])
    qs = []
    for d in np.argsort(-np.asarray(lens), kind="stable")[:n_queries]:
        if lens[d] == 0:
            continue
        pick = off[d] + rng.integers(0, lens[d], n_tokens)
        v = synth.reconstruct(codes[pick], res[pick], a["centroids"], a["bucket_weights"], a["nbits"])
        v = v + np.float32(0.05) * rng.standard_normal(v.shape).astype(np.float32)
        qs.append(np.ascontiguousarray(v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12), np.float32))
    return qs


def _info(hx):
    return {f: getattr(hx.info, f) for f, _ in npa.api.np_info._fields_ if f not in INFO_SKIPPED}


def _rows(results):
    return [(r.passage_ids.tobytes(), np.asarray(r.scores, np.float32).tobytes()) for r in results]


def _answers(hx, queries):
    """every answer the contract names, as bytes"""
    n = hx.num_documents()
    subset = np.arange(0, n, 3, dtype=np.int64)
    out = {}
    for prec in (0, 1, 2, 3):
        p = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=8, centroid_score_threshold=0.4, precision=prec)
        out["threshold", prec] = _rows(hx.search_batch(queries, p))
        out["subset", prec] = _rows(hx.search_batch(queries, p, subset=subset))
        p0 = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=8, centroid_score_threshold=None, precision=prec)
        hx.tune("s3_gain", 2)   # the zeroth level whenever it applies: it reads the range table
        out["zeroth level", prec] = _rows(hx.search_batch(queries, p0))
        hx.tune("s3_gain", 1)
    out["exact"] = _rows(hx.search_exact(queries, 10))
    ids = np.unique(np.concatenate([np.arange(n)[:3], np.arange(n)[-3:]])).astype(np.int64)
    out["pairs"] = [tuple(np.ascontiguousarray(x).tobytes() for x in r) for r in hx.score_pairs(queries, [ids for _ in queries])]
    emb, lens = hx.decompress_documents(np.array([0, n - 1], np.int64))
    out["decompress"] = (emb.tobytes(), np.asarray(lens).tobytes())
    return out


def _assert_equal_to_fresh(hx, fresh, queries, what=""):
    a, b = hx.export(), fresh.export()
    for k in ("doc_lengths", "codes", "residuals", "ivf", "ivf_lengths"):
        assert np.array_equal(a[k], b[k]), f"{what}: export()[{k!r}]"
    assert _info(hx) == _info(fresh), what
    if hx.num_documents() == 0:
        return
    got, want = _answers(hx, queries), _answers(fresh, queries)
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], f"{what}: {k}"


def _level_ran(hx, queries):
    """the zeroth level, the range table's only reader, ran: s3_gain = 2 (whenever it applies) without a threshold"""
    p0 = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=8, centroid_score_threshold=None)
    hx.tune("s3_gain", 2)
    hx.search_batch(queries, p0)
    hx.tune("s3_gain", 1)
    return hx.last_stats["n_level0"] > 0


def _remove_in_calls(hx, ids, n_docs, n_calls):
    """the ids in n_calls calls: a later call names its documents by the ids the earlier ones left them"""
    rem = R.removed_ids(ids, n_docs)
    cuts = np.linspace(0, rem.size, n_calls + 1).astype(int)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert hx.remove_ids(rem[a:b] - a) == b - a
    return rem


def _check_remove(base, ids, n_calls=1, slab=None, level=None, **opts):
    """remove `ids` from a handle of `base` and compare with a fresh handle of the restated shrunk arrays.  level: whether the
    zeroth level must run (True) or stay off (False); it does the same on both handles in any case"""
    want = R.shrunk_arrays(base, ids)
    n0 = base["doc_lengths"].size
    hx, fresh = hip_index(base, **opts), hip_index(want, **opts)
    try:
        if slab:
            hx.tune("remove_slab", slab)
        cap = hx.capacity()
        if n_calls == 1:
            assert hx.remove_ids(ids) == n0 - want["doc_lengths"].size
        else:
            _remove_in_calls(hx, ids, n0, n_calls)
        assert hx.capacity() == cap, "a remove changed the capacity"
        assert hx.num_documents() == want["doc_lengths"].size
        queries = _queries(want)
        _assert_equal_to_fresh(hx, fresh, queries)
        if hx.num_documents() > 0:
            ran = _level_ran(fresh, queries)
            assert _level_ran(hx, queries) == ran and (level is None or ran == level), "the zeroth level"
    finally:
        hx.close()
        fresh.close()


# ---- plain removals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_calls", [1, 3])
def test_a_random_tenth(n_calls):
    base = _base(700)
    ids = np.random.default_rng(1).choice(700, 70, replace=False)
    _check_remove(base, np.concatenate([ids, ids[:5], [-3, 700, 1 << 40]]) if n_calls == 1 else ids, n_calls=n_calls)


def test_remove_on_a_directory(tmp_path):
    spec, a = make_arrays(num_docs=1200, seed=5, **GEOM)
    cut, wts = synth.bucket_tables(spec)
    d, e = str(tmp_path / "a"), str(tmp_path / "b")
    npa.write_index_dir(d, a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=500)
    shutil.copytree(d, e)
    ids = np.random.default_rng(2).choice(1200, 120, replace=False)
    hx = npa.MmapIndex.load(d)
    hx.set_columns({"year": np.arange(1200)})
    try:
        assert hx.remove(np.concatenate([ids, [-1, 1200]])) == 120
        assert hx.num_documents() == 1080 and hx.schema is None
        U.delete(e, ids)   # the files np_hip_index_delete leaves, restated
        assert U.dir_state(d) == U.dir_state(e)
        want = R.shrunk_arrays(a, ids)
        assert hx.info.avg_doclen == float(want["doc_lengths"].sum()) / 1080.0   # the same double, no tolerance
        assert hx.info.avg_doclen == U._j(f"{d}/metadata.json")["avg_doclen"]
        fresh = npa.MmapIndex.load(d)
        try:
            _assert_equal_to_fresh(hx, fresh, _queries(want), "remove vs load")
        finally:
            fresh.close()
    finally:
        hx.close()


def test_remove_refused_before_the_directory_is_touched(tmp_path):
    spec, a = make_arrays(num_docs=600, seed=5, **GEOM)
    cut, wts = synth.bucket_tables(spec)
    d = str(tmp_path / "a")
    npa.write_index_dir(d, a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=500)
    before = U.dir_state(d)
    shard = npa.MmapIndex.load(d, shard_rank=0, shard_count=2)
    try:
        with pytest.raises(ValueError, match="shard"):
            shard.remove([3])
        assert U.dir_state(d) == before
    finally:
        shard.close()
    hx = npa.MmapIndex.load(d)
    try:
        npa.api.delete_from_index_dir(d, [5])   # somebody else's delete: the handle is now behind its directory
        behind = U.dir_state(d)
        with pytest.raises(npa.IndexLoadError, match="not current"):
            hx.remove([7])
        assert U.dir_state(d) == behind and hx.num_documents() == 600
        hx.reload()
        assert hx.remove([7, 7, 9]) == 2 and hx.num_documents() == 597
    finally:
        hx.close()


# ---- token compaction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["first", "last", "every other", "all but one"])
def test_which_documents(which):
    base = _base(301)
    ids = {"first": [0], "last": [300], "every other": np.arange(0, 301, 2), "all but one": np.delete(np.arange(301), 150)}[which]
    _check_remove(base, ids)


def test_removed_run_longer_than_a_tile():
    """700 adjacent documents of ~12 tokens x 32 bytes: ~270 KB of residuals, many 16 KiB tiles, leave in the middle"""
    base = _base(1500)
    assert base["doc_lengths"][400:1100].sum() * base["residuals"].shape[1] > 4 * COMPACT_TILE
    _check_remove(base, np.arange(400, 1100))


@pytest.mark.parametrize("slab", [2000, 1500, None])
def test_long_survivor_behind_a_removed_token(slab):
    """a one-token document at id 1 leaves, the 4500-token one behind it moves by ONE row (32 bytes of residuals, 4 of inverse
    norm, 2 of codes: none of the wide loads is aligned for all three) -- with remove_slab 2000 / 1500 the move crosses three
    / four slabs, all through the staging buffer; a second removal of 2500 tokens further back makes the last slab direct"""
    lens = [7, 1, 4500, 3, 2500, 9, 1200, 5]
    base = _custom(lens, 21)
    for ids in ([1], [1, 4]):
        if slab:
            off = np.concatenate([[0], np.cumsum(lens)])
            keep = np.ones(len(lens), bool)
            keep[ids] = False
            modes = [l[0] for l in R.plan(off, keep, slab)[0]]
            assert R.GATHER in modes and len(modes) >= 3 and (ids == [1] or R.DIRECT in modes)
        _check_remove(base, ids, slab=slab)


@pytest.mark.parametrize("nbits,dim", [(1, 96), (8, 64)])
def test_other_row_sizes(nbits, dim):
    """file rows of 12 bytes (nbits 1, dim 96: stored as 24) and of 64 bytes (nbits 8, dim 64)"""
    base = _base(400, nbits=nbits, dim=dim)
    _check_remove(base, np.random.default_rng(3).choice(400, 40, replace=False), slab=700)


def test_empty_documents_removed_and_kept():
    lens = np.random.default_rng(4).integers(0, 9, 300)
    lens[[0, 1, 7, 8, 150, 298, 299]] = 0
    base = _custom(lens, 22)
    _check_remove(base, [0, 7, 20, 21, 150, 299])
    _check_remove(base, np.flatnonzero(lens > 0)[::2])


def test_code_ordered_token_layout(monkeypatch):
    """NP_TOK_SORT=1 (read at open): tokens are kept in code order with tok_pos beside them; both move with their document,
    and export() / decompress_documents() still return the on-disk order"""
    monkeypatch.setenv("NP_TOK_SORT", "1")
    base = _custom([5, 600, 3, 24, 0, 17, 300, 2], 23)
    _check_remove(base, [0, 3], slab=256)
    _check_remove(_base(300), np.arange(1, 300, 7))


def test_wide_codes():
    """K = 65 600 > 65 536: u32 codes"""
    base = _base(400, num_centroids=65600, dim=32)
    _check_remove(base, np.random.default_rng(5).choice(400, 40, replace=False))


# ---- posting lists -------------------------------------------------------------------------------------------------------------------
def test_hot_list_over_tile_edges():
    """9000 documents that all hold code 7: its list lies over more than two tiles of the old array; documents on both sides
    of every tile edge inside it leave"""
    n = 9000
    rng = np.random.default_rng(6)
    codes = rng.integers(0, 256, (n, 2))
    codes[:, 0] = 7
    base = _custom(np.full(n, 2), 24, codes=codes.reshape(-1))
    o7 = int(base["ivf_lengths"][:7].sum())
    assert base["ivf_lengths"][7] == n
    edges = [e for e in range(FILTER_TILE, o7 + n, FILTER_TILE) if o7 < e < o7 + n]
    assert len(edges) >= 2
    ids = np.concatenate([[e - o7 - 2, e - o7 - 1, e - o7, e - o7 + 1] for e in edges] + [[0, n - 1]])
    _check_remove(base, ids)
    _check_remove(base, np.concatenate([[e - o7 - 1] for e in edges]))
    _check_remove(base, np.concatenate([[e - o7] for e in edges]))


@pytest.mark.parametrize("extra", [0, 1])
def test_totals_at_a_tile_multiple(extra):
    n = FILTER_TILE + extra
    base = _custom(np.ones(n, np.int64), 25)
    assert base["ivf"].size == n
    _check_remove(base, [0, 5, n - 1])
    _check_remove(base, [n - 1])


def test_lists_that_lose_every_entry():
    """K = 257: lists 0 and 256 hold two documents each, which leave"""
    rng = np.random.default_rng(7)
    lens = rng.integers(1, 9, 300)
    codes = rng.integers(1, 256, int(lens.sum()))
    off = np.concatenate([[0], np.cumsum(lens)])
    for d, c in ((3, 0), (10, 0), (40, 256), (299, 256)):
        codes[off[d]:off[d + 1]] = c
    base = _custom(lens, 26, codes=codes, num_centroids=257)
    want = R.shrunk_arrays(base, [3, 10, 40, 299])
    assert base["ivf_lengths"][[0, 256]].tolist() == [2, 2] and want["ivf_lengths"][[0, 256]].tolist() == [0, 0]
    _check_remove(base, [3, 10, 40, 299])


def test_every_document_removed():
    """np_hip_index_from_arrays opens the empty arrays; the emptied handle equals that one (export and info: there is no
    document to search for), keeps its capacity, and takes documents again"""
    base = _base(200)
    _check_remove(base, np.arange(200))
    hx = hip_index(base)
    try:
        assert hx.remove_ids(np.arange(-5, 300)) == 200 and hx.num_documents() == 0 and hx.info.avg_doclen == 0.0
        cap = hx.capacity()
        off = np.concatenate([[0], np.cumsum(base["doc_lengths"])])
        hx.append_arrays(base["doc_lengths"][:50], base["codes"][:off[50]], base["residuals"][:off[50]])
        assert hx.capacity() == cap
        fresh = hip_index(R.shrunk_arrays(base, np.arange(50, 200)))
        try:
            _assert_equal_to_fresh(hx, fresh, _queries(base))
        finally:
            fresh.close()
    finally:
        hx.close()


def _permuted(base):
    off = np.concatenate([[0], np.cumsum(base["ivf_lengths"])])
    return dict(base, ivf=np.concatenate([base["ivf"][a:b][::-1] for a, b in zip(off[:-1], off[1:])]))


def test_permuted_lists_keep_their_order():
    """lists that do not ascend are accepted (the directory delete accepts them): each keeps its own order, and the zeroth
    level, which needs ascending lists, stays off"""
    base = _permuted(_base(500))
    _check_remove(base, np.random.default_rng(8).choice(500, 50, replace=False), level=False)


@pytest.mark.parametrize("of", ["a survivor", "a removed document"])
def test_lists_missing_a_pair(of):
    """the pair (document 100, its first code) is not in the lists: they do not cover the codes, so the zeroth level is off.
    When document 100 leaves, the filtered lists cover again -- the coverage is looked at afresh, as an open does"""
    base = _base(500)
    off = np.concatenate([[0], np.cumsum(base["ivf_lengths"])])
    c = int(base["codes"][int(base["doc_lengths"][:100].sum())])
    at = off[c] + int(np.flatnonzero(base["ivf"][off[c]:off[c + 1]] == 100)[0])
    il = base["ivf_lengths"].copy()
    il[c] -= 1
    base = dict(base, ivf=np.delete(base["ivf"], at), ivf_lengths=il)
    ids = np.arange(3, 500, 11)
    assert 100 not in ids
    if of == "a survivor":
        _check_remove(base, ids, level=False)
    else:
        _check_remove(base, np.concatenate([ids, [100]]))


def test_lists_with_extra_pairs():
    """documents 5 and 400 stand in a list of a code they do not hold: extra entries only loosen the level's bound"""
    base = _base(500)
    off = np.concatenate([[0], np.cumsum(base["ivf_lengths"])])
    doc_of = np.repeat(np.arange(500), base["doc_lengths"])
    ivf, il = base["ivf"], base["ivf_lengths"].copy()
    for d in (400, 5):
        c = next(c for c in range(256) if c not in set(base["codes"][doc_of == d].tolist()) and il[c] > 0)
        lst = ivf[off[c]:off[c] + il[c]]
        ivf = np.insert(ivf, off[c] + int(np.searchsorted(lst, d)), d)
        il[c] += 1
        off = np.concatenate([[0], np.cumsum(il)])
    base = dict(base, ivf=ivf, ivf_lengths=il)
    _check_remove(base, [4, 6, 399, 450])
    _check_remove(base, [5, 401])


# ---- the rebuilt layout ------------------------------------------------------------------------------------------------------------
def test_block_stride_returns():
    """ten documents of 200 tokens (~140 distinct codes: a 320-byte block) among 300 of at most 24; without them a block is 64"""
    lens = np.random.default_rng(9).integers(1, 25, 300)
    long_ids = np.arange(5, 300, 30)
    lens[long_ids] = 200
    base = _custom(lens, 27)
    _check_remove(base, long_ids)
    _check_remove(base, long_ids[:-1])


def test_range_table_loses_a_range():
    """32 769 documents minus two: n_ranges goes from 2 to 1 (NP_IVF_SPLIT_RANGE = 32768); the zeroth level reads the table"""
    _check_remove(_base(32769), [17, 32768], level=True)
    _check_remove(_base(32769), [0], level=True)   # 32 768: exactly one full range


def test_document_longer_than_the_distinct_code_sort():
    """the only document of more than NP_UNIQ_MAX = 4096 tokens leaves: sliced_ok comes back, as on a fresh open"""
    lens = np.random.default_rng(10).integers(1, 25, 300)
    lens[120] = 4097
    base = _custom(lens, 28)
    _check_remove(base, [120])
    _check_remove(base, [119])


# ---- capacity ------------------------------------------------------------------------------------------------------------------------
def test_freed_room_is_a_reservation():
    base = _base(700)
    n, off = 700, np.concatenate([[0], np.cumsum(base["doc_lengths"])])
    tail = (base["doc_lengths"][650:], base["codes"][off[650]:], base["residuals"][off[650]:])
    hx = hip_index(base)
    try:
        cap = hx.capacity()
        assert cap == (n, int(off[-1]))
        assert hx.remove_ids(np.arange(600, 700)) == 100 and hx.capacity() == cap
        hx.append_arrays(*tail)   # 50 documents into the room of 100
        assert hx.capacity() == cap
        want = R.shrunk_arrays(base, np.arange(600, 650))
        fresh = hip_index(want)
        try:
            _assert_equal_to_fresh(hx, fresh, _queries(want), "remove, append")
        finally:
            fresh.close()
        assert hx.remove_ids([0, 1, 640]) == 3 and hx.capacity() == cap
        want = R.shrunk_arrays(want, [0, 1, 640])
        fresh = hip_index(want)
        try:
            _assert_equal_to_fresh(hx, fresh, _queries(want), "remove, append, remove")
        finally:
            fresh.close()
    finally:
        hx.close()


# ---- attachments ---------------------------------------------------------------------------------------------------------------------
def _error_of(call):
    try:
        call()
    except Exception as e:   # noqa: BLE001 -- the comparison is of whatever is raised
        return type(e), str(e)
    return None


def test_attachments_are_dropped_and_come_back():
    base = _base(400)
    qs = _queries(base)
    p = npa.SearchParameters(n_full_scores=128, top_k=5, n_ivf_probe=8)
    texts = [f"w{i % 7} common" for i in range(400)]
    calls = [lambda h: h.filter_ids([("year >= ?", [100])]), lambda h: h.text_search(["common"], 5),
             lambda h: h.search_grouped(qs, p, group_size=2)]
    bare, hx = hip_index(base), hip_index(base)
    try:
        never = [_error_of(lambda: c(bare)) for c in calls]
        assert all(e is not None for e in never)
        hx.set_columns({"year": np.arange(400)})
        hx.build_text(texts)
        hx.set_groups(np.arange(400) % 9)
        assert [_error_of(lambda: c(hx)) for c in calls] == [None] * 3
        with_all = hx.info.device_bytes
        assert hx.remove_ids([-1, 400, 1 << 33]) == 0   # nothing in range: nothing changes, the attachments stay
        assert hx.schema is not None and hx.text is not None and hx.group_values is not None
        assert [_error_of(lambda: c(hx)) for c in calls] == [None] * 3 and hx.info.device_bytes == with_all
        assert hx.remove_ids(np.arange(0, 400, 50)) == 8
        assert hx.schema is None and hx.text is None and hx.group_values is None
        assert [_error_of(lambda: c(hx)) for c in calls] == never
        bare.remove_ids(np.arange(0, 400, 50))
        assert hx.info.device_bytes == bare.info.device_bytes < with_all   # their HBM is released and uncounted
        keep = np.delete(np.arange(400), np.arange(0, 400, 50))
        hx.set_columns({"year": keep})
        hx.build_text([texts[i] for i in keep])
        hx.set_groups(keep % 9)
        assert hx.filter_ids([("year >= ?", [100])])[0].tolist() == np.flatnonzero(keep >= 100).tolist()
        assert len(hx.text_search(["w1"], 392)) == 1
        assert len(hx.search_grouped(qs, p, group_size=2)) == len(qs)
    finally:
        bare.close()
        hx.close()


# ---- refused, and the handle answers as before ----------------------------------------------------------------------------------
def test_refusals_change_nothing():
    import ctypes as C
    base = _base(500)
    qs = _queries(base)
    p = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=8)
    hx = hip_index(base, shard_rank=0, shard_count=2)
    try:
        before, info = _rows(hx.search_batch(qs, p)), _info(hx)
        with pytest.raises(ValueError, match=r"np_hip_index_remove: index is a shard \(0 of 2\)"):
            hx.remove_ids([3])
        with pytest.raises(ValueError, match="shard"):
            hx.remove_ids([])
        assert _rows(hx.search_batch(qs, p)) == before and _info(hx) == info
    finally:
        hx.close()
    hx = hip_index(base)
    try:
        before, info, cap = _rows(hx.search_batch(qs, p)), _info(hx), hx.capacity()
        L, out = npa.api.lib(), C.c_int64(-5)
        ids = np.array([3], np.int64)
        assert L.np_hip_index_remove(hx._h, ids.ctypes.data, -1, C.byref(out)) == 8
        assert npa.api.last_error() == "np_hip_index_remove: n_ids is negative"
        assert L.np_hip_index_remove(hx._h, None, 1, C.byref(out)) == 8
        assert npa.api.last_error() == "np_hip_index_remove: doc_ids is NULL" and out.value == -5
        assert hx.remove_ids([]) == 0 and hx.remove_ids([500, -1]) == 0
        assert _rows(hx.search_batch(qs, p)) == before and _info(hx) == info and hx.capacity() == cap
    finally:
        hx.close()


# ---- under traffic -------------------------------------------------------------------------------------------------------------------
def test_remove_under_traffic():
    """four threads search in a loop while the main thread removes once: every answer is, in bytes, the old index's or the new
    one's for its query, and a search that starts after the remove has returned gets the new one's"""
    base = _base(3000)
    qs = _queries(base, n_queries=4)
    ids = np.argsort(-base["doc_lengths"], kind="stable")[:4]   # the queries' own documents leave: the answers change
    p = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=8)
    fresh = hip_index(R.shrunk_arrays(base, ids))
    try:
        post = _rows(fresh.search_batch(qs, p))
    finally:
        fresh.close()
    hx = hip_index(base, n_contexts=2)
    try:
        pre = _rows(hx.search_batch(qs, p))
        assert all(a != b for a, b in zip(pre, post)), "the queries do not tell the two states apart"
        removed, stop = threading.Event(), threading.Event()
        started = [threading.Event() for _ in range(4)]
        seen, errors = [[] for _ in range(4)], []

        def worker(i):
            try:
                after = 0
                while not stop.is_set() and after < 3:
                    was_removed = removed.is_set()
                    seen[i].append((was_removed, _rows(hx.search_batch(qs, p, parallel=False))))
                    started[i].set()
                    after += was_removed
            except Exception as e:   # noqa: BLE001
                errors.append(e)
                started[i].set()

        threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(4)]
        for t in threads:
            t.start()
        for ev in started:
            assert ev.wait(60)
        assert hx.remove_ids(ids) == 4
        removed.set()
        for t in threads:
            t.join(60)
        stop.set()
        assert not errors and not any(t.is_alive() for t in threads), errors
        for i in range(4):
            assert sum(a for a, _ in seen[i]) == 3
            for was_removed, rows in seen[i]:
                for q, row in enumerate(rows):
                    assert row == post[q] or (not was_removed and row == pre[q]), f"thread {i} query {q}"
        assert _rows(hx.search_batch(qs, p)) == post
    finally:
        hx.close()


GONE = re.compile(r"the handle has no (columns|keyword index|groups) \(np_hip_index_set_")


def test_calls_outside_a_context_under_remove():
    """decompress_documents reads the token arrays a remove compacts in place; grouped, filtered and keyword calls check their
    attachments before they take a context.  Beside a remove each of them gives its answer of before, or -- once the remove
    has dropped the attachments -- the error a handle without them gives; decompress of documents in front of the first
    removed one gives the same bytes throughout"""
    base = _base(2000)
    qs = _queries(base, n_queries=2)
    p = npa.SearchParameters(n_full_scores=128, top_k=5, n_ivf_probe=8)
    front = np.arange(0, 1000, 7, dtype=np.int64)
    calls = [lambda h: tuple(np.asarray(x).tobytes() for x in h.decompress_documents(front)),
             lambda h: [(g, tuple(map(repr, r))) for g, r in enumerate(h.search_grouped(qs, p, group_size=2))] and "grouped",
             lambda h: [x.tobytes() for x in h.filter_ids([("year >= ?", [100])])],
             lambda h: _rows(h.text_search(["common"], 5))]
    bare = hip_index(base)
    try:
        never = [_error_of(lambda: c(bare)) for c in calls[1:]]
    finally:
        bare.close()
    hx = hip_index(base, n_contexts=2)
    try:
        hx.set_columns({"year": np.arange(2000)})
        hx.build_text([f"w{i % 7} common" for i in range(2000)])
        hx.set_groups(np.arange(2000) % 9)
        pre = [c(hx) for c in calls]
        removed = threading.Event()
        started = [threading.Event() for _ in calls]
        bad = []

        def worker(i):
            after = 0
            while after < 3:
                was = removed.is_set()
                try:
                    got = calls[i](hx)
                    if got != pre[i] or (was and i > 0):
                        bad.append((i, was, "answer"))
                except Exception as e:   # noqa: BLE001
                    # the mirror's own refusal (its schema / vocabulary already gone) or the library's (they went in between)
                    if i == 0 or not ((type(e), str(e)) == never[i - 1] or (isinstance(e, ValueError) and GONE.search(str(e)))):
                        bad.append((i, was, repr(e)))
                started[i].set()
                after += was

        threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(len(calls))]
        for t in threads:
            t.start()
        for ev in started:
            assert ev.wait(60)
        assert hx.remove_ids(np.arange(1000, 2000, 3)) == 334
        removed.set()
        for t in threads:
            t.join(60)
        assert not bad and not any(t.is_alive() for t in threads), bad
    finally:
        hx.close()


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_removes_from_the_same_directory(tmp_path):
    """tests/cpp/remove_index.cpp: next_plaid.hpp's remove() on a copy of the directory leaves the files and gives the answers
    -- before and after, on one handle -- that the Python mirror's does"""
    exe = tmp_path / "remove_index"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "remove_index.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-L", os.path.join(ROOT, "next-plaid_amd", "csrc"),
                           "-lnextplaid_hip", "-Wl,-rpath," + os.path.join(ROOT, "next-plaid_amd", "csrc")])
    spec, a = make_arrays(num_docs=900, seed=5, **GEOM)
    cut, wts = synth.bucket_tables(spec)
    d, e = str(tmp_path / "py"), str(tmp_path / "cpp")
    npa.write_index_dir(d, a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=400)
    shutil.copytree(d, e)
    ids = np.concatenate([np.argsort(-a["doc_lengths"], kind="stable")[:4], [17, 17, 899, 900, -2]]).astype(np.int64)
    qs = _queries(a)
    ids.astype("<i8").tofile(tmp_path / "ids.i64")
    np.concatenate(qs).astype("<f4").tofile(tmp_path / "q.f32")
    p = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=8)
    hx = npa.MmapIndex.load(d)
    try:
        before = hx.search_batch(qs, p)
        assert hx.remove(ids) == 6
        after = hx.search_batch(qs, p)
    finally:
        hx.close()
    out = subprocess.check_output([str(exe), e, str(tmp_path / "ids.i64"), str(tmp_path / "q.f32"), str(len(qs)), "8"], text=True)
    lines = out.strip().splitlines()
    assert "removed 6 documents 894" in lines
    rows = [json.loads(x) for x in lines if x.startswith("{")]
    assert len(rows) == 2 * len(qs)
    for r in rows:
        y = (before if r["state"] == "before" else after)[r["query_id"]]
        assert r["passage_ids"] == y.passage_ids.tolist() and np.allclose(r["scores"], y.scores, rtol=1e-7)
    assert [r["passage_ids"] for r in rows[:len(qs)]] != [r["passage_ids"] for r in rows[len(qs):]]
    assert U.dir_state(d) == U.dir_state(e)
