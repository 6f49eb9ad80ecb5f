"""np_hip_search_exact_grouped on the device: the true top-k groups over every document.  Needs a real MI355X.

Nothing here has a tolerance.  The entry is defined by composition -- np_hip_collapse of the complete search_exact list -- so
the reference is tests/collapse_restate.py's walk over what search_exact of the same build returns with top_k = every
document, or over score_pairs of every (query, document) pair where that list is longer than any collapse stride.  All six
output regions are compared for equality, padding and score bits included.  The entry takes no output strides (a row is top_k x
group_size slots, at most 16384): the refusal of a wrong stride has no counterpart here, the slot limit stands in its place."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, hip_index, make_arrays

import next_plaid_amd as npa
from next_plaid_amd import api, synth
import collapse_restate as R

pytestmark = pytest.mark.gpu
N = 2000


@pytest.fixture(scope="module")
def corpus():
    # documents of 0 .. 40 tokens (empty ones, and ones longer than a 32-token tile), eight queries of mixed length
    spec, a = make_arrays(num_docs=N, num_centroids=64, dim=64, nbits=4, doc_len_min=0, doc_len_max=40, seed=33)
    hx = hip_index(a)
    qs = [synth.make_queries(spec, 1, n_tokens=lq, cen=a["centroids"], first_query=i)[0][0]
          for i, lq in enumerate([5, 32, 1, 33, 8, 32, 3, 12])]
    hx.set_columns({"n": np.arange(N), "tag": [None if d % 3 else f"t{d % 4}" for d in range(N)]})
    yield spec, a, hx, qs, {}
    hx.close()


def group_keys(name):
    d = np.arange(N)
    if name == "own":
        return d.astype(np.int32), N
    if name == "one":
        return np.zeros(N, np.int32), 1
    if name == "runs":      # runs of 1, 2, 3 ... documents: they straddle a wave's 64 documents, a block's 256 and the pass edge
        return np.floor((np.sqrt(8.0 * d + 1) - 1) / 2).astype(np.int32), 64
    if name == "ends":      # group 0 is the first and the last document
        g = (1 + d // 3).astype(np.int32)
        g[[0, N - 1]] = 0
        return g, int(g.max()) + 1
    return [None if x % 5 == 0 else f"file{x % 11}" for x in range(N)], None     # the NULL group


def scope_args(scope, B):
    some = np.arange(0, N, 2)
    if scope == "subset":
        return dict(subset=some)
    if scope == "subsets":
        other = np.arange(100, 1400)
        return dict(subsets=[None, some, other, np.zeros(0, np.int64), some, None, other, np.array([3, 5, 7, 9, N - 1])][:B])
    if scope == "filters":
        return dict(filters=[None, ("n < ?", [900]), ("tag = ?", ["t0"]), ("n < ?", [-1]), ("n >= ? AND tag IS NULL", [50]), None,
                             ("n < ?", [900]), ("tag IS NOT NULL", [])][:B])
    return {}


def full_lists(hx, qs, n_docs, precision, cache, key, **kw):
    """search_exact with top_k = every document, in np_hip_collapse's layout; computed once per key"""
    if key not in cache:
        res = hx.search_exact(qs, n_docs, precision, **kw)
        ids, sc = np.zeros((len(qs), n_docs), np.int64), np.zeros((len(qs), n_docs), np.float32)
        cnt = np.array([r.passage_ids.size for r in res], np.int32)
        for i, r in enumerate(res):
            ids[i, : cnt[i]], sc[i, : cnt[i]] = r.passage_ids, r.scores
        cache[key] = (ids, sc, cnt)
    return cache[key]


@pytest.mark.parametrize("scope", ["none", "subset", "subsets", "filters"])
@pytest.mark.parametrize("pattern", ["own", "one", "runs", "ends", "null"])
def test_equals_collapse_of_the_complete_exact_list(corpus, scope, pattern):
    spec, a, hx, qs, cache = corpus
    keys, n_groups = group_keys(pattern)
    hx.set_groups(keys, n_groups=n_groups)
    g = np.asarray(keys) if n_groups is not None else api.group_ids_of_keys(keys)[0]
    hx.tune("scan_docs", 700)            # three passes: the pass edge falls inside a run of every pattern but "own"
    try:
        kw = scope_args(scope, len(qs))
        for precision in (0, 3):
            ids, sc, cnt = full_lists(hx, qs, N, precision, cache, (scope, precision), **kw)
            if scope in ("subsets", "filters"):
                assert cnt[3] == 0 and cnt[1] > 0              # the empty scope empties that query and no other
            for gs in (1, 2, 5):
                for top_k in (1, 10, min(hx.group_count() + 1, 16384 // gs)):
                    want = R.walk_batch(ids, sc, cnt, N, g, top_k, gs)
                    got = hx.search_exact_grouped(qs, top_k, gs, precision, raw=True, **kw)
                    R.check(got, want, f"{scope} / {pattern} / precision {precision} top_k {top_k} group_size {gs}")
    finally:
        hx.tune("scan_docs", 0)
        hx.set_groups(None)


def test_beyond_the_pool_and_beyond_the_collapse_stride():
    """17000 one-token documents.  Group 0 holds the 16500 documents query 0 ranks first -- more than any collapse stride
    (16384) holds -- and groups 1 .. 50 share the 500 it ranks last: every one of their leaders lies beyond any pool."""
    n, pool_k, top_k, gs = 17000, 32, 10, 3
    spec, a = make_arrays(num_docs=n, num_centroids=16, dim=32, nbits=2, doc_len_min=1, doc_len_max=1, seed=9)
    hx = hip_index(a)
    try:
        qs = list(synth.make_queries(spec, 3, n_tokens=4, cen=a["centroids"])[0])
        every = np.arange(n, dtype=np.int64)
        scores = np.stack(hx.score_pairs(qs, [every] * 3, return_matches=False))      # search_exact's bits, every pair
        assert np.isfinite(scores).all()
        order = [np.lexsort((every, -scores[i].astype(np.float64))) for i in range(3)]  # score descending, then id ascending
        g = np.zeros(n, np.int32)
        g[order[0][16500:]] = 1 + np.arange(500) % 50
        hx.set_groups(g, n_groups=51)
        want = R.padded([R.walk(order[i], scores[i][order[i]], g, top_k, gs) for i in range(3)], top_k, gs)
        assert want[5][0] == top_k and want[4][0, 0] == 16500 and want[2][0, 0] == 0
        got = hx.search_exact_grouped(qs, top_k, gs, raw=True)
        R.check(got, want, "beyond the pool")
        pooled = hx.search_grouped(qs, npa.SearchParameters(n_full_scores=4096, top_k=top_k, n_ivf_probe=16,
                                                            centroid_score_threshold=None), group_size=gs, pool_k=pool_k, raw=True)
        assert pooled[5][0] == 1 and pooled[4].reshape(3, top_k)[0, 0] <= pool_k     # one group for query 0, 32 members at most
        assert not np.array_equal(pooled[2], got[2]) and not np.array_equal(pooled[4], got[4])
    finally:
        hx.close()


def test_exact_ties_follow_ascending_id():
    """Byte-identical documents in one group and across groups: equal score bits, so leaders and members ascend by id."""
    spec, a = make_arrays(num_docs=200, num_centroids=16, dim=32, nbits=2, doc_len_min=6, doc_len_max=6, seed=4)
    qs, srcs = synth.make_queries(spec, 2, n_tokens=6, cen=a["centroids"])
    src = int(srcs[0])                                            # query 0 is made of this document's tokens: it ranks first
    same = sorted([src] + [c for c in (7, 8, 60, 121, 199) if c != src][:4])
    for c in same:
        a["codes"][6 * c: 6 * c + 6] = a["codes"][6 * src: 6 * src + 6]
        a["residuals"][6 * c: 6 * c + 6] = a["residuals"][6 * src: 6 * src + 6]
    hx = hip_index(a)
    try:
        g = (10 + np.arange(200) // 4).astype(np.int32)
        g[same[:3]], g[same[3]], g[same[4]] = 2, 0, 1             # three copies share a group, two have groups of their own
        hx.set_groups(g, n_groups=int(g.max()) + 1)
        ids, sc, cnt = full_lists(hx, qs, 200, 0, {}, 0)
        at = int(np.nonzero(ids[0] == same[0])[0][0])               # the copies are adjacent, in id order, with one score
        assert ids[0, at: at + 5].tolist() == same and len({x.tobytes() for x in sc[0, at: at + 5]}) == 1
        for top_k, gs in ((3, 1), (3, 2), (60, 4)):
            got = hx.search_exact_grouped(qs, top_k, gs, raw=True)
            R.check(got, R.walk_batch(ids, sc, cnt, 200, g, top_k, gs), f"ties top_k {top_k} group_size {gs}")
    finally:
        hx.close()


def test_a_query_is_independent_of_batch_passes_and_chunks(corpus):
    spec, a, hx, qs, cache = corpus
    keys, n_groups = group_keys("runs")
    small = hip_index(a, max_batch=3)                         # slices of three queries
    tight = hip_index(a, workspace_bytes=600_000)             # ~340 KB of queries, ~70 KB per query: a few queries a slice
    try:
        for h in (hx, small, tight):
            h.set_groups(keys, n_groups=n_groups)
        batch = [qs[3] if i in (0, 17, 39) else qs[(3 * i + 1) % 8] for i in range(40)]
        for gs in (1, 3):
            alone = hx.search_exact_grouped(qs[3:4], 7, gs, raw=True)
            assert alone[5][0] == 7 and (alone[4] > gs).any()
            runs = {what: h.search_exact_grouped(batch, 7, gs, raw=True)
                    for what, h in (("batch", hx), ("max_batch 3", small), ("tight", tight))}
            hx.tune("scan_tiles", 2)
            hx.tune("scan_docs", 37)                          # 55 passes
            runs["passes and tiles"] = hx.search_exact_grouped(batch, 7, gs, raw=True)
            hx.tune("scan_tiles", 8)
            hx.tune("scan_docs", 0)
            for what, many in runs.items():
                for name, one, all_ in zip(R.NAMES, alone, many):
                    for at in (0, 17, 39):
                        assert one.reshape(-1).tobytes() == all_.reshape(40, -1)[at].tobytes(), (what, gs, name, at)
    finally:
        small.close()
        tight.close()
        hx.set_groups(None)


def test_refusals_by_name(corpus):
    spec, a, hx, qs, cache = corpus
    hx.set_groups(None)
    with pytest.raises(ValueError, match="no groups"):
        hx.search_exact_grouped(qs[:1], 3)
    sh = hip_index(a, shard_rank=0, shard_count=2)
    with pytest.raises(ValueError, match="sharded"):
        sh.search_exact_grouped(qs[:1], 3)
    sh.close()
    hx.set_groups(np.zeros(N, np.int32), n_groups=1)
    try:
        # top_k * group_size is the stride of an output row: at most 16384 slots
        for top_k, gs, what in ((0, 1, "top_k"), (1, 0, "group_size"), (16385, 1, "16384"), (5, 3277, "16384")):
            with pytest.raises(ValueError, match=what):
                hx.search_exact_grouped(qs[:1], top_k, gs)
        with pytest.raises(ValueError, match="precision"):
            hx.search_exact_grouped(qs[:1], 3, 1, precision=2)
        assert hx.search_exact_grouped([], 3) == []
        few = hip_index(a, workspace_bytes=50_000)        # one query's staged tiles alone are larger
        few.set_groups(np.zeros(N, np.int32), n_groups=1)
        with pytest.raises(MemoryError, match="workspace budget"):
            few.search_exact_grouped(qs[:1], 3)
        few.close()
    finally:
        hx.set_groups(None)


def test_cpp_mirror_prints_the_same_bits(tmp_path):
    spec, a = make_arrays(num_docs=96, num_centroids=16, dim=32, nbits=2, doc_len_min=3, doc_len_max=9, seed=5)
    exe, lib_dir = tmp_path / "search_exact_grouped", os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "search_exact_grouped.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    synth.write_index(str(tmp_path / "ix"), {k: v for k, v in a.items() if k != "_prep"}, chunk_docs=40)
    qs = list(synth.make_queries(spec, 6, n_tokens=5, cen=a["centroids"])[0])
    groups = (np.arange(96) % 5).astype(np.int32)
    for name, arr in (("q.f32", np.concatenate(qs, 0).astype("<f4")), ("lens.i64", np.full(6, 5, "<i8")), ("groups.i32", groups)):
        arr.tofile(tmp_path / name)
    out = subprocess.check_output([str(exe)] + [str(tmp_path / x) for x in ("ix", "q.f32", "lens.i64", "groups.i32")], text=True)
    hx = npa.MmapIndex.load(str(tmp_path / "ix"))
    try:
        hx.set_groups(groups, n_groups=5)
        res = hx.search_exact_grouped(qs, 3, 2, subsets=[np.arange(0, 60, 2) if i % 2 else None for i in range(6)])
        bits = lambda ids, sc: "".join(f" {d}:{b:08x}" for d, b in zip(ids.tolist(), sc.view(np.uint32).tolist()))
        want = "".join(f"exact {i} {len(r)}" + "".join(f" | {g} {t}" + bits(ids, sc) for g, ids, sc, t in r) + "\n" for i, r in enumerate(res))
        assert out == want and any(gr[3] > 2 for r in res for gr in r)
    finally:
        hx.close()
