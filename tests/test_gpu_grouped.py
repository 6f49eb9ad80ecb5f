"""Grouped search on the device: set_groups, np_hip_collapse / _device, search_grouped, search_hybrid_grouped.  Needs a real
MI355X.

The reference is tests/collapse_restate.py's walk (pinned by tests/test_collapse_restate_cpu.py).  Nothing here has a
tolerance: ids, group figures and score bits are compared for equality, padding included.  The kernel is held to the walk at
its own edges on hand-made lists; the one-call entries are held, byte for byte, to the walk over what the ungrouped call of the
same build returns with top_k = pool_k."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, hip_index, make_arrays, oracle_index, to_oracle_params

import next_plaid_amd as npa
from next_plaid_amd import api, synth, text as T
import collapse_restate as R
import text_restate as TR

pytestmark = pytest.mark.gpu
P = npa.SearchParameters
CAP = api.NP_GROUP_MAX_LIST
STRIDES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, CAP]
N_TINY = 16400
TOP_GROUP = 2 ** 31 - 2


@pytest.fixture(scope="module")
def tiny():
    """16400 one-token documents: the collapse only needs ids to look groups up by; the search over it has a re-rank window
    of 16384 documents."""
    spec, a = make_arrays(num_docs=N_TINY, num_centroids=16, dim=32, nbits=2, doc_len_min=1, doc_len_max=1, seed=3)
    hx = hip_index(a)
    yield spec, a, hx
    hx.close()


# ---- the kernel against the walk at its own edges -------------------------------------------------------------------
def pattern_groups(name):
    d = np.arange(N_TINY)
    if name == "one group":
        return np.zeros(N_TINY, np.int32), 1
    if name == "all distinct":
        return d.astype(np.int32), N_TINY
    if name == "interleaved":
        return (d % 2).astype(np.int32), 2
    if name == "runs":            # runs of 1, 2, 3 ... documents: in sorted position they straddle every multiple of 64 and 1024
        return (np.floor((np.sqrt(8.0 * d + 1) - 1) / 2)).astype(np.int32), 200
    if name == "extreme ids":     # group ids 0 and 2^31 - 2 together, and one in between
        return np.where(d % 3 == 0, 0, np.where(d % 3 == 1, TOP_GROUP, 12345)).astype(np.int32), 2 ** 31 - 1
    if name == "leaders":         # documents 1..9 have groups of their own, everything else is group 0
        g = np.zeros(N_TINY, np.int32)
        g[1:10] = np.arange(1, 10)
        return g, 10
    raise KeyError(name)


PATTERNS = ["one group", "all distinct", "interleaved", "runs", "extreme ids", "leaders"]


def lists_for(name, stride, rng):
    """Four lists of one stride: full, one short of full (or empty where that is the same), empty, and a shorter one; the id
    order differs per list (ascending, permuted, descending)."""
    counts = [stride, max(stride - 1, 0), 0, (stride * 2) // 3]
    ids = np.zeros((4, stride), np.int64)
    if name == "leaders":
        # the leaders of new groups sit at ranks 0, 63, 64, 1023, 1024 and count - 1 (those the count reaches)
        for b, c in enumerate(counts):
            ids[b, :] = rng.integers(10, N_TINY, stride)           # group 0
            for j, r in enumerate(sorted({0, 63, 64, 1023, 1024, c - 1})):
                if 0 <= r < c:
                    ids[b, r] = 1 + j
        return ids, counts
    lo = 0 if stride >= 1024 else int(rng.integers(0, N_TINY - stride))
    ids[0] = np.arange(lo, lo + stride)
    ids[1] = rng.permutation(N_TINY)[:stride]
    ids[2] = 7
    ids[3] = np.arange(lo + stride - 1, lo - 1, -1) if lo else np.arange(stride - 1, -1, -1)
    if stride > 4:
        ids[1, 3] = ids[1, 0]                                       # a duplicate id is a separate entry
    return ids, counts


def param_sets(name, stride):
    n_distinct = {"one group": 1, "interleaved": 2, "extreme ids": 3, "leaders": 7}.get(name, min(stride, 150))
    ks = sorted({1, max(n_distinct - 1, 1), n_distinct, n_distinct + 3})
    out = [(k, gs) for k, gs in zip(ks * 2, [1, 2, 3, stride + 1, 2, 3, 1, 2])]
    return [(k, gs) for k, gs in out if k * gs <= CAP]


@pytest.mark.parametrize("name", PATTERNS)
def test_collapse_equals_the_walk(tiny, name):
    spec, a, hx = tiny
    g, n_groups = pattern_groups(name)
    hx.set_groups(g, n_groups=n_groups)
    assert hx.group_count() == n_groups
    rng = np.random.default_rng(len(name))
    nan = np.array([0x7FC00123, 0xFFC00001], np.uint32).view(np.float32)
    for stride in STRIDES:
        ids, counts = lists_for(name, stride, rng)
        sc = rng.standard_normal((4, stride)).astype(np.float32)
        sc[:, ::5] = nan[0]                                        # NaN payloads go through bit for bit
        sc[:, 1::7] = nan[1]
        for j, (top_k, gs) in enumerate(param_sets(name, stride)):
            scores = None if j % 3 == 2 else sc                    # scores = NULL
            want = R.walk_batch(ids, scores, counts, stride, g, top_k, gs)
            got = hx.collapse_raw(ids, scores, counts, stride, top_k, gs)
            R.check(got, want, f"{name} stride {stride} top_k {top_k} group_size {gs} scores {scores is not None}")
    hx.set_groups(None)


def test_collapse_fills_a_whole_output_row(tiny):
    """top_k * group_size = 16384, both ways, from a list of 16384 entries."""
    spec, a, hx = tiny
    for g, n_groups, top_k, gs in (((np.arange(N_TINY) % 128).astype(np.int32), 128, 128, 128),
                                   (np.arange(N_TINY, dtype=np.int32), N_TINY, CAP, 1)):
        hx.set_groups(g, n_groups=n_groups)
        ids = np.random.default_rng(5).permutation(N_TINY)[:CAP].reshape(1, CAP)
        sc = np.arange(CAP, dtype=np.float32).reshape(1, CAP)
        want = R.walk_batch(ids, sc, [CAP], CAP, g, top_k, gs)
        assert int(want[3].sum()) > CAP - 200                      # (nearly) every slot is written
        R.check(hx.collapse_raw(ids, sc, [CAP], CAP, top_k, gs), want, f"{top_k} x {gs}")
    hx.set_groups(None)


def test_public_collapse_returns_groups(tiny):
    spec, a, hx = tiny
    hx.set_groups(["b", None, "a", None, "b", "c", None, "a", "c", "c"] + [None] * (N_TINY - 10))
    assert hx.group_values == ["a", "b", "c"] and hx.group_count() == 4
    ids = [[5, 1, 0, 3, 8, 6, 4, 2, 9, 7], [], [2]]
    sc = [np.linspace(5, 1, 10).astype(np.float32), [], [0.25]]
    got = npa.collapse(ids, sc, 3, 2, hx)
    g = api.group_ids_of_keys(["b", None, "a", None, "b", "c", None, "a", "c", "c"])[0]
    for i in range(3):
        assert R.listed(got[i]) == R.walked(R.walk(ids[i], sc[i], g, 3, 2)), i
    assert [x[0] for x in got[0]] == [2, 3, 1] and got[0][1][3] == 3 and got[1] == []
    assert npa.collapse(ids, None, 3, 2, hx)[0][0][2] is None
    hx.set_groups(None)


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
        self.ptrs = []


def test_device_form_clamps_a_count_and_skips_an_id_out_of_range(tiny):
    spec, a, hx = tiny
    g = (np.arange(N_TINY) % 5).astype(np.int32)
    hx.set_groups(g, n_groups=5)
    stride, top_k, gs = 70, 4, 3
    rng = np.random.default_rng(11)
    ids = rng.integers(0, N_TINY, (3, stride))
    ids[0, [0, 5, 64]] = [N_TINY, -1, 2 ** 40]                     # absent: skipped, counted in no total
    sc = rng.standard_normal((3, stride)).astype(np.float32)
    counts = np.array([stride, stride + 9, -3], np.int32)          # clamped to the stride, and to 0
    want = R.walk_batch(ids, sc, counts, stride, g, top_k, gs, num_documents=N_TINY)
    assert want[5].tolist() == [4, 4, 0]
    dev = DeviceArrays()
    try:
        out = [np.full((3, top_k, gs), -1, np.int64), np.full((3, top_k, gs), -1.0, np.float32)] + \
              [np.full((3, top_k), -1, np.int32) for _ in range(3)] + [np.full(3, -1, np.int32)]
        d_out = [dev.put(o) for o in out]
        api._check(api.lib().np_hip_collapse_device(hx._h, top_k, gs, 3, dev.put(ids), dev.put(sc), dev.put(counts), stride,
                                                    *d_out, None))
        R.check([dev.get(p, o) for p, o in zip(d_out, out)], want, "device form")
        # the host form refuses both
        with pytest.raises(ValueError, match="outside its stride"):
            hx.collapse_raw(ids, sc, counts, stride, top_k, gs)
        with pytest.raises(ValueError, match=r"outside \[0, 16400\)"):
            hx.collapse_raw(ids, sc, [stride] * 3, stride, top_k, gs)
    finally:
        dev.free()
        hx.set_groups(None)


# ---- composition, byte for byte ---------------------------------------------------------------------------------------
N_COMP = 600


@pytest.fixture(scope="module")
def comp():
    spec, a = make_arrays(num_docs=N_COMP, num_centroids=64, dim=64, nbits=2, doc_len_min=4, doc_len_max=12, seed=21)
    hx = hip_index(a)
    qs = []
    for i, lq in enumerate([5, 32, 1, 17, 8, 32, 3, 12]):            # a batch whose queries differ in token count
        qs.append(synth.make_queries(spec, 1, n_tokens=lq, cen=a["centroids"], first_query=i)[0][0])
    hx.set_columns({"n": np.arange(N_COMP), "tag": [None if d % 3 else f"t{d % 4}" for d in range(N_COMP)]})
    yield spec, a, hx, qs
    hx.close()


def group_variants():
    d = np.arange(N_COMP)
    return {"doc % 7": (d % 7).tolist(), "one per document": d.tolist(),
            "NULL-heavy": [None if x % 5 else f"file{x % 11}" for x in range(N_COMP)]}


def pool_lists(results, pool_k):
    B = len(results)
    ids, sc = np.zeros((B, pool_k), np.int64), np.zeros((B, pool_k), np.float32)
    cnt = np.zeros(B, np.int32)
    for i, r in enumerate(results):
        cnt[i] = r.passage_ids.size
        ids[i, : cnt[i]], sc[i, : cnt[i]] = r.passage_ids, r.scores
    return ids, sc, cnt


def not_vacuous(want, ids, cnt, g, top_k, gs, tally):
    """some group's total exceeds group_size, some query sees more groups in its pool than top_k"""
    tally["folded"] += int((want[4] > gs).any())
    tally["skipped"] += int(any(len(set(g[ids[i, : cnt[i]]].tolist())) > top_k for i in range(len(cnt))))


def test_the_oracles_lists_make_the_composition_cases_meaningful():
    """Before any GPU run: the walk over the CPU oracle's ranked lists folds members and skips groups for these seeds."""
    spec, a = make_arrays(num_docs=N_COMP, num_centroids=64, dim=64, nbits=2, doc_len_min=4, doc_len_max=12, seed=21)
    ox = oracle_index(a)
    qs = [synth.make_queries(spec, 1, n_tokens=lq, cen=a["centroids"], first_query=i)[0][0] for i, lq in enumerate([5, 32, 1, 17])]
    res = ox.search_batch(qs, to_oracle_params(P(n_full_scores=256, top_k=64, n_ivf_probe=8)))
    for name, keys in group_variants().items():
        g = api.group_ids_of_keys(keys)[0]
        tally = {"folded": 0, "skipped": 0}
        ids, sc, cnt = pool_lists(res, 64)
        not_vacuous(R.walk_batch(ids, sc, cnt, 64, g, 3, 2), ids, cnt, g, 3, 2, tally)
        assert tally["skipped"] and (tally["folded"] or name == "one per document"), (name, tally)


SCOPES = ["none", "one subset", "per-query subsets", "filters"]


def scope_args(scope, B):
    some = np.arange(0, N_COMP, 2)
    if scope == "one subset":
        return dict(subset=some)
    if scope == "per-query subsets":
        other = np.arange(100, 400)
        return dict(subsets=[None, some, other, np.zeros(0, np.int64), some, None, other, np.array([3, 5, 7, 9, 590])][:B])
    if scope == "filters":
        f = [None, ("n < ?", [300]), ("tag = ?", ["t0"]), ("n < ?", [-1]), ("n >= ? AND tag IS NULL", [50]), None,
             ("n < ?", [300]), ("tag IS NOT NULL", [])]
        return dict(filters=f[:B])
    return {}


@pytest.mark.parametrize("scope", SCOPES)
def test_search_grouped_is_collapse_of_search_batch(comp, scope):
    spec, a, hx, qs = comp
    tally = {"folded": 0, "skipped": 0}
    for name, keys in group_variants().items():
        hx.set_groups(keys)
        g = api.group_ids_of_keys(keys)[0]
        for pool_k, cbs in ((32, 100_000), (64, 100_000), (128, 100_000), (64, 16)):   # below / equal to / above n_full_scores / 4;
            top_k, gs = (3, 2) if pool_k != 128 else (5, 1)                             # and the batched path (cbs < K = 64)
            kw = scope_args(scope, len(qs))
            base = hx.search_batch(qs, P(n_full_scores=256, top_k=pool_k, n_ivf_probe=8, centroid_batch_size=cbs), **kw)
            ids, sc, cnt = pool_lists(base, pool_k)
            want = R.walk_batch(ids, sc, cnt, pool_k, g, top_k, gs)
            got = hx.search_grouped(qs, P(n_full_scores=256, top_k=top_k, n_ivf_probe=8, centroid_batch_size=cbs), group_size=gs,
                                    pool_k=pool_k, raw=True, **kw)
            R.check(got, want, f"{scope} / {name} / pool_k {pool_k} cbs {cbs}")
            not_vacuous(want, ids, cnt, g, top_k, gs, tally)
            if scope in ("per-query subsets", "filters"):
                assert cnt[3] == 0 and got[5][3] == 0 and cnt[1] > 0      # the empty scope empties that query and no other
    assert tally["folded"] and tally["skipped"], tally
    hx.set_groups(None)


def test_search_grouped_returns_groups_and_takes_the_default_pool(comp):
    spec, a, hx, qs = comp
    keys = group_variants()["NULL-heavy"]
    hx.set_groups(keys)
    g, values, n = api.group_ids_of_keys(keys)
    p = P(n_full_scores=1024, top_k=4, n_ivf_probe=8)
    assert api.default_pool_k(4, N_COMP) == 200
    base = hx.search_batch(qs, P(n_full_scores=1024, top_k=200, n_ivf_probe=8))
    got = hx.search_grouped(qs, p, group_size=3)
    for i, r in enumerate(base):
        assert R.listed(got[i]) == R.walked(R.walk(r.passage_ids, r.scores, g, 4, 3)), i
    assert any(gr[0] == n - 1 for q in got for gr in q) and hx.group_values == values   # the NULL group is one group
    assert hx.last_stats["n_queries"] == len(qs)
    hx.set_groups(None)


def test_window_of_16384(tiny):
    spec, a, hx = tiny
    g = (np.arange(N_TINY) % 97).astype(np.int32)
    hx.set_groups(g, n_groups=97)
    qs = synth.make_queries(spec, 2, n_tokens=2, cen=a["centroids"])[0]
    base = hx.search_batch(qs, P(n_full_scores=65536, top_k=CAP, n_ivf_probe=16, centroid_score_threshold=None))
    ids, sc, cnt = pool_lists(base, CAP)
    assert cnt.min() > 12000
    want = R.walk_batch(ids, sc, cnt, CAP, g, 50, 4)
    got = hx.search_grouped(qs, P(n_full_scores=65536, top_k=50, n_ivf_probe=16, centroid_score_threshold=None), group_size=4,
                            pool_k=CAP, raw=True)
    R.check(got, want, "window 16384")
    assert (want[4] > 4).any() and want[5].tolist() == [50, 50]
    hx.set_groups(None)


def test_search_hybrid_grouped_is_collapse_of_search_hybrid(comp):
    spec, a, hx, qs = comp
    data = T.TextIndexData.from_texts(TR.make_texts(N_COMP, 12, seed=4, every="wo0", lens=(0, 1, 2, 3, 5, 8, 13)))
    hx.set_text(data)
    AND, OR = T.NP_TEXT_AND, T.NP_TEXT_OR
    tq = [[T.TextQuery.from_phrases([[1], [2]], OR), T.TextQuery.from_phrases([[0], [3]], AND), "",
           T.TextQuery.from_phrases([[1, 2], [4]], OR)][i % 4] for i in range(len(qs))]
    tally = {"folded": 0, "skipped": 0}
    try:
        for name, keys in group_variants().items():
            hx.set_groups(keys)
            g = api.group_ids_of_keys(keys)[0]
            for fusion, pool_k, fetch_k, kw in (("relative_score", 60, 40, {}), ("rrf", 100, 50, scope_args("per-query subsets", 8)),
                                                ("rrf", 2048, 1024, scope_args("filters", 8))):
                base = hx.search_hybrid(qs, tq, P(n_full_scores=256, top_k=pool_k, n_ivf_probe=8), alpha=0.6, fusion=fusion,
                                        fetch_k=fetch_k, **kw)
                got = hx.search_hybrid_grouped(qs, tq, P(n_full_scores=256, top_k=3, n_ivf_probe=8), group_size=2, pool_k=pool_k,
                                               alpha=0.6, fusion=fusion, fetch_k=fetch_k, **kw)
                ids, sc, cnt = pool_lists(base, pool_k)
                want = R.walk_batch(ids, sc, cnt, pool_k, g, 3, 2)
                for i in range(len(qs)):
                    assert R.listed(got[i]) == R.walked(R.walk(base[i].passage_ids, base[i].scores, g, 3, 2)), (name, fusion, i)
                not_vacuous(want, ids, cnt, g, 3, 2, tally)
        assert tally["folded"] and tally["skipped"], tally
        with pytest.raises(ValueError, match="top_k"):
            hx.search_hybrid_grouped(qs[:1], tq[:1], P(n_full_scores=256, top_k=3, n_ivf_probe=8), pool_k=2049, fetch_k=10)
    finally:
        hx.set_text(None)
        hx.set_groups(None)


def test_a_query_is_independent_of_its_batch(comp):
    spec, a, hx, qs = comp
    hx.set_groups(group_variants()["doc % 7"])
    p = P(n_full_scores=256, top_k=4, n_ivf_probe=8)
    alone = hx.search_grouped(qs[:1], p, group_size=3, pool_k=64, raw=True)
    batch = [qs[(i * 3 + 1) % 8] for i in range(64)]
    for at in (0, 17, 63):
        batch[at] = qs[0]
    many = hx.search_grouped(batch, p, group_size=3, pool_k=64, raw=True)
    rows = [x.reshape(64, -1) for x in many]
    for at in (0, 17, 63):
        for name, one, all_ in zip(R.NAMES, alone, rows):
            assert one.reshape(-1).tobytes() == all_[at].tobytes(), (name, at)
    assert alone[5][0] == 4 and (alone[4] > 3).any()
    hx.set_groups(None)


# ---- errors and lifecycle ---------------------------------------------------------------------------------------------
def test_errors_are_reported_before_any_launch(comp):
    spec, a, hx, qs = comp
    p = P(n_full_scores=256, top_k=3, n_ivf_probe=8)
    one = np.zeros(4, np.int64)
    hx.set_groups(None)
    with pytest.raises(ValueError, match="no groups"):               # no groups set
        hx.search_grouped(qs[:1], p)
    with pytest.raises(ValueError, match="no groups"):
        hx.collapse_raw(one, None, [4], 4, 2, 1)
    sh = hip_index(a, shard_rank=0, shard_count=2)                    # a sharded handle
    try:
        with pytest.raises(ValueError, match="sharded"):
            sh.set_groups(np.zeros(N_COMP, np.int32), n_groups=1)
        assert sh.group_count() == 0
    finally:
        sh.close()
    with pytest.raises(npa.ShapeError, match="per document"):        # bad arrays
        hx.set_groups(np.zeros(N_COMP - 1, np.int32), n_groups=1)
    bad = np.zeros(N_COMP, np.int32)
    bad[17] = 3
    with pytest.raises(ValueError, match="document 17 has group 3"):
        hx.set_groups(bad, n_groups=3)
    bad[17] = -1
    with pytest.raises(ValueError, match="document 17"):
        hx.set_groups(bad, n_groups=3)
    for n in (0, 2 ** 31):
        with pytest.raises(ValueError, match="n_groups"):
            hx.set_groups(np.zeros(N_COMP, np.int32), n_groups=n)
    assert hx.group_count() == 0
    hx.set_groups(np.zeros(N_COMP, np.int32), n_groups=1)
    for top_k, gs, stride, what in ((0, 1, 4, "top_k"), (1, 0, 4, "group_size"), (CAP + 1, 1, 4, "16384"), (5, 3277, 4, "16384"),
                                    (1, 1, 0, "stride"), (1, 1, CAP + 1, "stride")):          # limits exceeded by one
        with pytest.raises(ValueError, match=what):
            hx.collapse_raw(np.zeros(max(stride, 1), np.int64), None, [0], stride, top_k, gs)
    for pool_k in (0, CAP + 1):
        with pytest.raises(ValueError, match="pool_k"):
            hx.search_grouped(qs[:1], p, pool_k=pool_k)
    with pytest.raises(ValueError, match="16384"):
        hx.search_grouped(qs[:1], P(n_full_scores=256, top_k=129, n_ivf_probe=8), group_size=128, pool_k=10)
    with pytest.raises(ValueError, match="not both"):
        hx.search_grouped(qs[:1], p, subset=[1], filters=[None])
    assert hx.search_grouped([], p) == []
    hx.set_groups(None)


def test_lifecycle_and_device_bytes(comp, tmp_path):
    spec, a, hx, qs = comp
    p = P(n_full_scores=256, top_k=3, n_ivf_probe=8)
    before = hx.info.device_bytes
    hx.set_groups(np.arange(N_COMP) % 7)
    assert hx.info.device_bytes == before + 4 * N_COMP               # up by exactly the array
    first = hx.search_grouped(qs[:2], p, pool_k=40, raw=True)
    hx.set_groups(np.arange(N_COMP) % 3)                              # twice: the second replaces the first
    assert hx.info.device_bytes == before + 4 * N_COMP and hx.group_count() == 3 and hx.group_values == [0, 1, 2]
    second = hx.search_grouped(qs[:2], p, pool_k=40, raw=True)
    assert second[2].max() <= 2 and second[5].tolist() == [3, 3]
    hx.set_groups([])                                                 # n = 0, then a grouped call
    assert hx.info.device_bytes == before and hx.group_count() == 0 and hx.group_values is None
    with pytest.raises(ValueError, match="no groups"):
        hx.search_grouped(qs[:2], p, pool_k=40)
    # groups after reload() follow the columns: a new handle has neither
    ixdir = tmp_path / "ix"
    synth.write_index(str(ixdir), {k: v for k, v in a.items() if k != "_prep"}, chunk_docs=250)
    dx = npa.MmapIndex.load(str(ixdir))
    try:
        dx.set_columns({"n": np.arange(N_COMP)})
        dx.set_groups(np.arange(N_COMP) % 7)
        got = dx.search_grouped(qs[:2], p, pool_k=40, raw=True)
        assert all(np.array_equal(x, y) for x, y in zip(got, first))  # the same index from its directory: the same bytes
        dx.reload()
        assert dx.schema is None and dx.group_values is None and dx.group_count() == 0
        with pytest.raises(ValueError, match="no groups"):
            dx.search_grouped(qs[:2], p, pool_k=40)
        dx.set_groups(np.arange(N_COMP) % 7)
        assert all(np.array_equal(x, y) for x, y in zip(dx.search_grouped(qs[:2], p, pool_k=40, raw=True), first))
    finally:
        dx.close()


# ---- the C++ mirror -----------------------------------------------------------------------------------------------------
def test_cpp_mirror_prints_the_same_bits(tmp_path):
    spec, a = make_arrays(num_docs=96, num_centroids=16, dim=32, nbits=2, doc_len_min=3, doc_len_max=9, seed=5)
    exe = tmp_path / "search_grouped"
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "search_grouped.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    ixdir = tmp_path / "ix"
    ixdir.mkdir()
    synth.write_index(str(ixdir), {k: v for k, v in a.items() if k != "_prep"}, chunk_docs=40)
    data = T.TextIndexData.from_texts(TR.make_texts(96, 8, seed=2, every="wo0", lens=(0, 1, 2, 3, 5, 8)))
    data.term_offsets.astype("<i8").tofile(tmp_path / "toff.i64")
    data.inst_doc.astype("<i8").tofile(tmp_path / "idoc.i64")
    data.inst_pos.astype("<i4").tofile(tmp_path / "ipos.i32")
    qs = list(synth.make_queries(spec, 6, n_tokens=5, cen=a["centroids"])[0])
    np.concatenate(qs, 0).astype("<f4").tofile(tmp_path / "q.f32")
    np.array([q.shape[0] for q in qs], "<i8").tofile(tmp_path / "lens.i64")
    groups = (np.arange(96) % 5).astype(np.int32)
    groups.astype("<i4").tofile(tmp_path / "groups.i32")
    out = subprocess.check_output([str(exe), str(ixdir), str(tmp_path / "toff.i64"), str(tmp_path / "idoc.i64"), str(tmp_path / "ipos.i32"),
                                   str(data.n_rows), str(tmp_path / "q.f32"), str(tmp_path / "lens.i64"), str(tmp_path / "groups.i32")],
                                  text=True)
    tq = [[T.TextQuery.from_phrases([[0], [1]], T.NP_TEXT_AND), T.TextQuery.from_phrases([[2, 3], [1]], T.NP_TEXT_OR),
           T.TextQuery.from_phrases([[0], [-1], [4]], T.NP_TEXT_OR)][i % 3] for i in range(6)]
    evens = np.arange(0, 60, 2)
    subsets = [evens if i % 2 == 1 else None for i in range(6)]

    def lines(stage, res):
        s = ""
        for i, groups_ in enumerate(res):
            s += f"{stage} {i} {len(groups_)}"
            for gid, ids, sc, total in groups_:
                s += f" | {gid} {total}" + "".join(f" {d}:{b:08x}" for d, b in zip(ids.tolist(), sc.view(np.uint32).tolist()))
            s += "\n"
        return s

    hx = npa.MmapIndex.load(str(ixdir))
    try:
        hx.set_text(data)
        hx.set_groups(groups, n_groups=5)
        p = npa.SearchParameters(n_full_scores=64, top_k=3, n_ivf_probe=4)
        sg = hx.search_grouped(qs, p, group_size=2, pool_k=30, subsets=subsets)
        hy = hx.search_hybrid_grouped(qs, tq, p, group_size=2, pool_k=24, alpha=0.75, fusion="relative_score", fetch_k=15, subsets=subsets)
        base = hx.search_batch(qs, npa.SearchParameters(n_full_scores=64, top_k=20, n_ivf_probe=4))
        co = npa.collapse([r.passage_ids for r in base], [r.scores for r in base], 2, 3, hx)
        assert out == lines("grouped", sg) + lines("hybrid", hy) + lines("collapse", co)
        assert sum(len(x) for x in sg) > 10 and any(gr[3] > 2 for x in sg for gr in x)
    finally:
        hx.close()
