"""np_hip_index_append / MmapIndex.append and append_arrays: documents appended to a handle that is resident in HBM.

The contract under test is one sentence: after an append the handle is indistinguishable from a handle freshly opened on the
resulting index -- from_arrays of the concatenated arrays, or load of the directory update_append wrote.  "Equal to fresh"
(_assert_equal_to_fresh) is equal export() arrays, equal info() fields but device_bytes / workspace_bytes, and equal BYTES
from search_batch at every precision (with a threshold, without one through the zeroth filter level, with a subset),
search_exact, score_pairs on the new documents and decompress_documents of the first and last new id.  Needs a real MI355X."""
import re
import shutil
import threading

import numpy as np
import pytest

import update_restate as U
from helpers import hip_index, make_arrays, synth

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu

GEOM = dict(num_centroids=256, dim=64, nbits=4, doc_len_min=1, doc_len_max=24)
INFO_SKIPPED = ("device_bytes", "workspace_bytes")


def _split(n_old, n_new, seed=5, **kw):
    """one synthetic corpus of n_old + n_new documents: (spec, the arrays of the first n_old, (lengths, codes, residuals) of
    the rest)"""
    geom = dict(GEOM, **kw)
    spec, full = make_arrays(num_docs=n_old + n_new, seed=seed, **geom)
    if n_new == 0:
        return spec, full, None
    base = synth.generate_arrays(spec, 0, n_old)
    codes, res, lens = synth.doc_tokens(spec, n_old, n_old + n_new)
    return spec, base, (lens, codes, res)


def _concat(base, new):
    """the arrays of the index after the append: the posting lists of all codes (index.rs:479-499)"""
    lens = np.concatenate([base["doc_lengths"], np.asarray(new[0], np.int64)])
    codes = np.concatenate([base["codes"], np.asarray(new[1], np.int64)])
    res = np.concatenate([base["residuals"], np.asarray(new[2], np.uint8).reshape(-1, base["residuals"].shape[1])])
    ivf, il = synth.build_ivf(codes, lens, base["centroids"].shape[0])
    return dict(base, doc_lengths=lens, codes=codes, residuals=res, ivf=ivf, ivf_lengths=il)


def _rand_docs(rng, lens, base, code_lo=0, code_hi=None):
    """documents of the given lengths with uniform codes in [code_lo, code_hi) and random residual bytes"""
    K, pd = base["centroids"].shape[0], base["residuals"].shape[1]
    T = int(np.sum(lens))
    codes = rng.integers(code_lo, K if code_hi is None else code_hi, T).astype(np.int64)
    return np.asarray(lens, np.int64), codes, rng.integers(0, 256, (T, pd)).astype(np.uint8)


def _queries(base, new, n_queries=4, n_tokens=8, seed=11):
    """queries made of the new documents' own tokens (decompressed, a little noise): their answers name new documents"""
    lens, codes, res = new
    cen, wts, nbits = base["centroids"], base["bucket_weights"], base["nbits"]
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)])
    docs = [d for d in np.argsort(-np.asarray(lens), kind="stable")[:n_queries] if lens[d] > 0]
    qs = []
    for d in docs:
        pick = off[d] + rng.integers(0, lens[d], n_tokens)
        v = synth.reconstruct(codes[pick], res[pick], cen, wts, nbits)
        v = v + np.float32(0.05) * rng.standard_normal(v.shape).astype(np.float32)
        qs.append(np.ascontiguousarray(v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12), np.float32))
    return qs


def _info(hx):
    return {f: getattr(hx.info, f) for f, _ in npa.api.np_info._fields_ if f not in INFO_SKIPPED}


def _rows(results):
    return [(r.passage_ids.tobytes(), np.asarray(r.scores, np.float32).tobytes()) for r in results]


def _answers(hx, queries, n_old):
    """every answer the contract names, as bytes"""
    n = hx.num_documents()
    new_ids = np.arange(n_old, n, dtype=np.int64)
    subset = np.concatenate([np.arange(0, n_old, 3, dtype=np.int64), new_ids])
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
    pairs = [np.concatenate([new_ids[:3], new_ids[-3:], [0]]) for _ in queries]
    out["pairs"] = [tuple(np.ascontiguousarray(x).tobytes() for x in r) for r in hx.score_pairs(queries, pairs)]
    if new_ids.size:
        emb, lens = hx.decompress_documents(new_ids[[0, -1]])
        out["decompress"] = (emb.tobytes(), np.asarray(lens).tobytes())
    return out


def _assert_equal_to_fresh(hx, fresh, queries, n_old, what=""):
    a, b = hx.export(), fresh.export()
    for k in ("doc_lengths", "codes", "residuals", "ivf", "ivf_lengths"):
        assert np.array_equal(a[k], b[k]), f"{what}: export()[{k!r}]"
    assert _info(hx) == _info(fresh), what
    got, want = _answers(hx, queries, n_old), _answers(fresh, queries, n_old)
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


def _check_append(base, new, n_appends=1, reserve=None, queries=None, level_runs=False, **opts):
    """append `new` to a handle of `base` in n_appends calls and compare with a fresh handle of the concatenation"""
    n_old = base["doc_lengths"].size
    lens, codes, res = new
    hx, fresh = hip_index(base, **opts), hip_index(_concat(base, new), **opts)
    try:
        if reserve:
            hx.reserve(*reserve)
            cap = hx.capacity()
            assert cap[0] >= n_old + reserve[0] and cap[1] >= int(base["doc_lengths"].sum()) + reserve[1]
        off = np.concatenate([[0], np.cumsum(lens)])
        cuts = np.linspace(0, len(lens), n_appends + 1).astype(int)
        for a, b in zip(cuts[:-1], cuts[1:]):
            ids = hx.append_arrays(lens[a:b], codes[off[a]:off[b]], res[off[a]:off[b]])
            assert ids.tolist() == list(range(n_old + a, n_old + b))
        if reserve:
            assert hx.capacity() == cap, "an append within the reservation reallocated"
        else:
            assert hx.capacity() == (n_old + len(lens), int(base["doc_lengths"].sum() + np.sum(lens)))
        queries = _queries(base, new) if queries is None else queries
        _assert_equal_to_fresh(hx, fresh, queries, n_old)
        if level_runs:
            assert _level_ran(fresh, queries) and _level_ran(hx, queries), "the zeroth level did not run: nothing read the range table"
    finally:
        hx.close()
        fresh.close()


# ---- append_arrays against from_arrays of the concatenation ---------------------------------------------------------------
@pytest.mark.parametrize("variant", ["one append", "three appends", "after reserve"])
def test_append_arrays_equals_fresh(variant):
    _, base, new = _split(700, 20)
    _check_append(base, new, n_appends=3 if variant == "three appends" else 1,
                  reserve=(50, 2000) if variant == "after reserve" else None)


# ---- append on a directory against load of that directory and the restated update_index -----------------------------------
def test_append_on_a_directory(tmp_path):
    spec, a, _ = _split(1200, 0)
    cut, wts = synth.bucket_tables(spec)
    d, e = str(tmp_path / "a"), str(tmp_path / "b")
    npa.write_index_dir(d, a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=500)
    shutil.copytree(d, e)
    rng = np.random.default_rng(2)
    docs = []
    for _ in range(30):
        L = int(rng.integers(1, 20))
        x = a["centroids"][rng.integers(0, 256, L)] + 0.02 * rng.standard_normal((L, 64)).astype(np.float32)
        docs.append(x.astype(np.float32))
    hx = npa.MmapIndex.load(d)
    hx.set_columns({"year": np.arange(1200)})
    try:
        ids = hx.append(docs)
        assert ids.tolist() == list(range(1200, 1230)) and hx.num_documents() == 1230 and hx.schema is None
        U.update_index(e, docs, 50_000, False)   # the files update_append leaves, restated
        assert U.dir_state(d) == U.dir_state(e)
        fresh = npa.MmapIndex.load(d)
        try:
            qs = [np.ascontiguousarray(x[:8] / np.linalg.norm(x[:8], axis=1, keepdims=True), np.float32) for x in docs[:4]]
            _assert_equal_to_fresh(hx, fresh, qs, 1200, "append vs load")
        finally:
            fresh.close()
    finally:
        hx.close()


def test_append_refused_before_the_directory_is_touched(tmp_path):
    """what the handle's half would refuse -- a shard, a handle behind its directory -- is found before update_append runs:
    the directory keeps its bytes, so nothing is persisted that the handle does not serve and a retry duplicates nothing"""
    spec, a, _ = _split(600, 0)
    cut, wts = synth.bucket_tables(spec)
    d = str(tmp_path / "a")
    npa.write_index_dir(d, a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=500)
    docs = [a["centroids"][:5].copy(), a["centroids"][7:9].copy()]
    before = U.dir_state(d)
    shard = npa.MmapIndex.load(d, shard_rank=0, shard_count=2)
    try:
        with pytest.raises(ValueError, match="shard"):
            shard.append(docs)
        assert U.dir_state(d) == before
    finally:
        shard.close()
    hx = npa.MmapIndex.load(d)
    try:
        npa.MmapIndex.update_append(docs, d)   # somebody else's update: the handle is now behind its directory
        behind = U.dir_state(d)
        with pytest.raises(npa.IndexLoadError, match="not current"):
            hx.append(docs)
        assert U.dir_state(d) == behind and hx.num_documents() == 600
        hx.reload()
        assert hx.append(docs).tolist() == [602, 603]
    finally:
        hx.close()


# ---- the edges of the kernels -------------------------------------------------------------------------------------------------
def test_range_table_gains_a_range():
    """32 760 + 20 documents: n_ranges goes from 1 to 2 (NP_IVF_SPLIT_RANGE = 32768); the zeroth level reads the table"""
    _, base, new = _split(32760, 20)
    _check_append(base, new, level_runs=True)


def test_bitmap_word_crossed():
    _, base, new = _split(63, 2)
    _check_append(base, new)


def test_empty_new_document():
    _, base, new = _split(300, 0)
    rng = np.random.default_rng(3)
    _check_append(base, _rand_docs(rng, [5, 0, 7, 0], base))


def test_document_longer_than_the_token_sort():
    """600 tokens > NP_SORT_MAX = 512 on a base whose longest document has 24: max_doc_len grows"""
    _, base, new = _split(300, 0)
    _check_append(base, _rand_docs(np.random.default_rng(4), [600, 3], base))


def test_code_ordered_token_layout(monkeypatch):
    """NP_TOK_SORT=1 (read at open): tokens are kept in code order with tok_pos beside them.  Only the new documents are
    sorted -- sorting an old one again would reset its tok_pos -- the 600-token one stays as it is, and export() and
    decompress_documents() still return the on-disk order of every document, old and new"""
    monkeypatch.setenv("NP_TOK_SORT", "1")
    _, base, new = _split(300, 0)
    docs = _rand_docs(np.random.default_rng(8), [600, 3, 24, 0, 17], base)
    _check_append(base, docs, n_appends=2)
    _check_append(base, docs, reserve=(5, 700))


def test_document_longer_than_the_distinct_code_sort():
    """4097 tokens > NP_UNIQ_MAX = 4096: its list stays unsorted and sliced_ok falls, as on a fresh open"""
    _, base, new = _split(300, 0)
    _check_append(base, _rand_docs(np.random.default_rng(5), [4097, 2], base))


def test_new_lists_go_to_the_overflow_region():
    """a base whose lists all fit their blocks (at most 24 codes in a 64-byte block); the new documents hold ~140 distinct codes"""
    _, base, new = _split(300, 0)
    assert base["doc_lengths"].max() <= 24
    _check_append(base, _rand_docs(np.random.default_rng(6), [200, 9, 220], base))


def test_new_codes_fill_empty_posting_lists():
    _, base, new = _split(300, 0)
    base["codes"] = base["codes"] % 128
    base["ivf"], base["ivf_lengths"] = synth.build_ivf(base["codes"], base["doc_lengths"], 256)
    assert (base["ivf_lengths"][128:] == 0).all()
    _check_append(base, _rand_docs(np.random.default_rng(7), [12, 20, 3, 17], base, code_lo=128))


def test_wide_codes():
    """K = 65 600 > 65 536: u32 codes"""
    _, base, new = _split(400, 12, num_centroids=65600, dim=32)
    _check_append(base, new)


@pytest.mark.parametrize("nbits,dim", [(1, 96), (8, 64)])
def test_other_residual_widths(nbits, dim):
    """nbits 1 at dim 96: file rows are repacked to storage rows (2 bits, dim 96 -> 96); nbits 8"""
    _, base, new = _split(400, 12, nbits=nbits, dim=dim)
    _check_append(base, new)


# ---- refused, and the handle answers as before ------------------------------------------------------------------------------
def _refused(hx, queries, call, exc, match):
    p = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=8)
    before, info = _rows(hx.search_batch(queries, p)), _info(hx)
    with pytest.raises(exc, match=match):
        call()
    assert _rows(hx.search_batch(queries, p)) == before and _info(hx) == info


def test_refused_appends_change_nothing():
    _, base, new = _split(500, 6)
    lens, codes, res = new
    qs = _queries(base, new)
    hx = hip_index(base, shard_rank=0, shard_count=2)
    try:
        _refused(hx, qs, lambda: hx.append_arrays(lens, codes, res), ValueError, "shard")
    finally:
        hx.close()
    desc = dict(base)
    off = np.concatenate([[0], np.cumsum(base["ivf_lengths"])])
    desc["ivf"] = np.concatenate([base["ivf"][a:b][::-1] for a, b in zip(off[:-1], off[1:])])
    hx = hip_index(desc)
    try:
        _refused(hx, qs, lambda: hx.append_arrays(lens, codes, res), ValueError, "do not ascend")
    finally:
        hx.close()
    hx = hip_index(base)
    try:
        bad = codes.copy()
        bad[-1] = 256
        _refused(hx, qs, lambda: hx.append_arrays(lens, bad, res), ValueError, r"codes\[\d+\] = 256")
        neg = lens.copy()
        neg[2] = -1
        _refused(hx, qs, lambda: hx.append_arrays(neg, codes, res), npa.ShapeError, r"doc_lengths\[2\] is negative")
        p = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=8)
        before, info, cap = _rows(hx.search_batch(qs, p)), _info(hx), hx.capacity()
        assert hx.append_arrays(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 32), np.uint8)).size == 0
        assert _rows(hx.search_batch(qs, p)) == before and _info(hx) == info and hx.capacity() == cap
    finally:
        hx.close()


# ---- attachments ---------------------------------------------------------------------------------------------------------------
def _error_of(call):
    try:
        call()
    except Exception as e:   # noqa: BLE001 -- the comparison is of whatever is raised
        return type(e), str(e)
    return None


def test_attachments_are_dropped_and_come_back():
    _, base, new = _split(400, 8)
    qs = _queries(base, new)
    p = npa.SearchParameters(n_full_scores=128, top_k=5, n_ivf_probe=8)
    texts = [f"w{i % 7} common" for i in range(408)]
    calls = [lambda h: h.filter_ids([("year >= ?", [100])]), lambda h: h.text_search(["common"], 5),
             lambda h: h.search_grouped(qs, p, group_size=2)]
    bare, hx = hip_index(base), hip_index(base)
    try:
        never = [_error_of(lambda: c(bare)) for c in calls]
        assert all(e is not None for e in never)
        hx.set_columns({"year": np.arange(400)})
        hx.build_text(texts[:400])
        hx.set_groups(np.arange(400) % 9)
        assert [_error_of(lambda: c(hx)) for c in calls] == [None] * 3
        with_all = hx.info.device_bytes
        hx.append_arrays(*new)
        assert hx.schema is None and hx.text is None and hx.group_values is None
        assert [_error_of(lambda: c(hx)) for c in calls] == never
        bare.append_arrays(*new)
        assert hx.info.device_bytes == bare.info.device_bytes < with_all   # their HBM is released and uncounted
        hx.set_columns({"year": np.arange(408)})
        hx.build_text(texts)
        hx.set_groups(np.arange(408) % 9)
        assert hx.filter_ids([("year >= ?", [100])])[0].tolist() == list(range(100, 408))
        assert 407 in np.concatenate([r.passage_ids for r in hx.text_search(["w1"], 408)]).tolist()
        assert len(hx.search_grouped(qs, p, group_size=2)) == len(qs)
    finally:
        bare.close()
        hx.close()


# ---- under traffic -----------------------------------------------------------------------------------------------------------
def test_append_under_traffic():
    """four threads search in a loop while the main thread appends once: every answer is, in bytes, the old index's or the new
    one's for its query, and a search that starts after the append has returned gets the new one's"""
    _, base, new = _split(3000, 40)
    qs = _queries(base, new, n_queries=4)
    p = npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=8)
    fresh = hip_index(_concat(base, new))
    try:
        post = _rows(fresh.search_batch(qs, p))
    finally:
        fresh.close()
    hx = hip_index(base, n_contexts=2)
    try:
        pre = _rows(hx.search_batch(qs, p))
        assert all(a != b for a, b in zip(pre, post)), "the queries do not tell the two states apart"
        appended, stop = threading.Event(), threading.Event()
        started = [threading.Event() for _ in range(4)]
        seen, errors = [[] for _ in range(4)], []

        def worker(i):
            try:
                after = 0
                while not stop.is_set() and after < 3:
                    was_appended = appended.is_set()
                    seen[i].append((was_appended, _rows(hx.search_batch(qs, p, parallel=False))))
                    started[i].set()
                    after += was_appended
            except Exception as e:   # noqa: BLE001
                errors.append(e)
                started[i].set()

        threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(4)]
        for t in threads:
            t.start()
        for ev in started:
            assert ev.wait(60)
        hx.append_arrays(*new)
        appended.set()
        for t in threads:
            t.join(60)
        stop.set()
        assert not errors and not any(t.is_alive() for t in threads), errors
        for i in range(4):
            assert sum(a for a, _ in seen[i]) == 3
            for was_appended, rows in seen[i]:
                for q, row in enumerate(rows):
                    assert row == post[q] or (not was_appended and row == pre[q]), f"thread {i} query {q}"
        assert _rows(hx.search_batch(qs, p)) == post
    finally:
        hx.close()


GONE = re.compile(r"the handle has no (columns|keyword index|groups) \(np_hip_index_set_")


def test_calls_outside_a_context_under_append():
    """decompress_documents reads the token arrays an unreserved append frees; grouped, filtered and keyword calls check their
    attachments before they take a context.  Beside an append each of them gives its answer of before, or -- once the append
    has dropped the attachments -- the error a handle without them gives; decompress gives the old documents' bytes throughout"""
    _, base, new = _split(2000, 30)
    qs = _queries(base, new, n_queries=2)
    p = npa.SearchParameters(n_full_scores=128, top_k=5, n_ivf_probe=8)
    old_ids = np.arange(0, 2000, 7, dtype=np.int64)
    calls = [lambda h: tuple(np.asarray(x).tobytes() for x in h.decompress_documents(old_ids)),
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
        appended = threading.Event()
        started = [threading.Event() for _ in calls]
        bad = []

        def worker(i):
            after = 0
            while after < 3:
                was = appended.is_set()
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
        hx.append_arrays(*new)
        appended.set()
        for t in threads:
            t.join(60)
        assert not bad and not any(t.is_alive() for t in threads), bad
    finally:
        hx.close()
