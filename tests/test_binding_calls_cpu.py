"""What the Python binding hands the library, and what it makes of the answer -- without a device and without the library.

A fake stands in for api._lib: np_hip_index_info fills the geometry, np_hip_last_error returns a fixed message, and every
other np_hip_* entry records its name and the values behind its arguments, writes chosen counts and recognisable ids and
scores through the output pointers and returns a chosen status.  The tests state, in their own few lines, the entry each call
must reach and the values it must carry (flat queries and offsets, the CSR of the subsets with the queries' map, the np_filter
and np_text_query arrays, fetch_k, pool_k, the fusion mode, top_k, precision), how the padded rows come back as results
(strides, query ids, copies), and the policies: rc == 2 under parallel, the mapped errors, both-given scopes refused before
the library is touched, '' text queries, the fetch_k / pool_k defaults."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from next_plaid_amd import api, dist, filters as F, text as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM, N_DOCS, MESSAGE = 8, 5000, "Search failed: the fake said so"

ROWS, GROUPS = "ids sc cnt", "ids sc grp mem tot cnt"
CSR, FILT, HEAD = "sid soff n_sub qsub", "filt n_f", "h flat off B dim"
SPECS = {
    "np_hip_search_batch": f"{HEAD} p sub n_sub {ROWS} st",
    "np_hip_search_batch_subsets": f"{HEAD} p {CSR} {ROWS} st",
    "np_hip_search_batch_filtered": f"{HEAD} p {FILT} qsub {ROWS} st",
    "np_hip_search_exact": f"{HEAD} top_k precision {CSR} {ROWS} st",
    "np_hip_search_exact_filtered": f"{HEAD} top_k precision {FILT} qsub {ROWS} st",
    "np_hip_text_search": f"h tq B top_k {CSR} {ROWS} st",
    "np_hip_text_search_filtered": f"h tq B top_k {FILT} qsub {ROWS} st",
    "np_hip_search_hybrid": f"{HEAD} p tq fetch_k alpha fusion {CSR} {FILT} {ROWS} st",
    "np_hip_search_batch_grouped": f"{HEAD} p {CSR} {FILT} pool_k group_size {GROUPS} st",
    "np_hip_search_hybrid_grouped": f"{HEAD} p tq fetch_k alpha fusion {CSR} {FILT} pool_k group_size {GROUPS} st",
    "np_hip_score_pairs": f"{HEAD} precision pair_docs pair_off p_sc p_sims p_pos st",
    "np_hip_fuse": "h fusion alpha top_k B sem_ids sem_sc sem_cnt sem_w kw_ids kw_sc kw_cnt kw_w ids sc cnt",
    "np_hip_collapse": f"h top_k group_size B l_ids l_sc l_cnt l_w {GROUPS}",
    "np_hip_filter_eval": "h filt n_f f_ids f_cap f_off",
}


def rd(ptr, dtype, n):
    """A copy of the n entries behind a pointer argument (None stays None)."""
    if ptr is None:
        return None
    addr = ptr if isinstance(ptr, int) else ptr.value
    n = int(n)
    if n == 0:
        return np.zeros(0, dtype)
    assert addr, "a NULL pointer where entries are read"
    return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(addr), dtype).copy()


def wr(ptr, dtype, values):
    """Write through an output pointer; where the pointer still knows its array, the array must hold what is written."""
    values = np.asarray(values, dtype).reshape(-1)
    arr = getattr(ptr, "_arr", None)
    if arr is not None:
        assert arr.dtype == dtype and arr.size >= max(values.size, 1), (arr.dtype, arr.size, values.size)
    if values.size:
        C.memmove(ptr.value, values.ctypes.data, values.nbytes)


def counts_for(B, k):
    """The counts the fake answers with: k, 0, 1 in turn (capped by k) -- 0, 1 and k in one batch of three."""
    return [min([k, 0, 1][i % 3], k) for i in range(B)]


def row_ids(i, c):
    return 1000 * (i + 1) + np.arange(c, dtype=np.int64)


def row_scores(i, c):
    return (i + 1 + np.arange(c) / 64).astype(np.float32)


class FakeLib:
    def __init__(self):
        self.calls, self.rc, self.filter_counts = [], {}, [2, 0, 3]

    def np_hip_index_info(self, h, info):
        info._obj.embedding_dim, info._obj.num_documents = DIM, N_DOCS
        return 0

    def np_hip_last_error(self):
        return MESSAGE.encode()

    def np_hip_index_close(self, h):
        return None

    def __getattr__(self, name):
        if name not in SPECS:
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        names = SPECS[name].split()
        assert len(args) == len(names), (name, len(args))
        a = dict(zip(names, args))
        r = {"entry": name}
        B = a.get("B")
        for key in ("B", "dim", "top_k", "precision", "fetch_k", "alpha", "fusion", "pool_k", "group_size", "n_sub", "n_f", "sem_w",
                    "kw_w", "l_w", "f_cap"):
            if key in a:
                r[key] = a[key]
        r["h"] = a["h"] if a["h"] is None else a["h"].value
        if "p" in a:
            r["p"] = {f: getattr(a["p"]._obj, f) for f, _ in api.np_search_params._fields_}
        if "off" in a:
            r["off"] = rd(a["off"], np.int32, B + 1)
            r["flat"] = rd(a["flat"], np.float32, int(r["off"][-1]) * a["dim"])
        if "sub" in a:
            r["sub"] = rd(a["sub"], np.int64, max(a["n_sub"], 0))
        if "soff" in a:
            r["soff"] = rd(a["soff"], np.int64, a["n_sub"] + 1)
            r["sid"] = rd(a["sid"], np.int64, 0 if r["soff"] is None else r["soff"][-1])
        if "qsub" in a:
            r["qsub"] = rd(a["qsub"], np.int32, B)
        if "filt" in a:
            r["filt"] = None if a["filt"] is None else [
                ([tuple(getattr(f.ops[i], x) for x, _ in api.np_filter_op._fields_) for i in range(f.n_ops)],
                 rd(f.values, np.int64, f.n_values).tolist() if f.values else []) for f in list(a["filt"])[: a["n_f"]]]
        if "tq" in a:
            r["tq"] = []
            for q in list(a["tq"])[:B]:
                off = rd(q.phrase_offsets, np.int32, q.n_phrases + 1)
                r["tq"].append((rd(q.terms, np.int32, off[-1]).tolist(), off.tolist(), q.n_phrases, q.mode))
        for side in ("sem", "kw", "l"):
            if side + "_ids" in a:
                w = a[side + "_w"]
                r[side + "_ids"] = rd(a[side + "_ids"], np.int64, B * w)
                r[side + "_sc"] = rd(a[side + "_sc"], np.float32, B * w)
                r[side + "_cnt"] = rd(a[side + "_cnt"], np.int32, B)
        rc = self.rc.get(name, 0)
        if name == "np_hip_filter_eval":
            cnt = [self.filter_counts[j % 3] for j in range(a["n_f"])]
            r["wants_ids"] = a["f_ids"] is not None
            if a["f_ids"] is not None:
                assert a["f_cap"] >= sum(cnt)
                wr(a["f_ids"], np.int64, 7 + np.arange(sum(cnt)))
            wr(a["f_off"], np.int64, np.concatenate([[0], np.cumsum(cnt)]))
        elif name == "np_hip_score_pairs":
            r["pair_off"] = rd(a["pair_off"], np.int64, B + 1)
            r["pair_docs"] = rd(a["pair_docs"], np.int64, r["pair_off"][-1])
            P = int(r["pair_off"][-1])
            R = int((np.diff(r["pair_off"]) * np.diff(r["off"])).sum())
            r["wants_matches"] = a["p_sims"] is not None
            assert (a["p_sims"] is None) == (a["p_pos"] is None)
            wr(a["p_sc"], np.float32, np.arange(P) + 0.5)
            if a["p_sims"] is not None:
                wr(a["p_sims"], np.float32, np.arange(R) + 0.25)
                wr(a["p_pos"], np.int32, np.arange(R))
        elif "grp" in a:
            top_k = a["top_k"] if "top_k" in a else a["p"]._obj.top_k
            k, g = max(top_k, 1), max(a["group_size"], 1)
            cnt = counts_for(B, top_k)
            ids, sc = np.zeros((max(B, 1), k, g), np.int64), np.zeros((max(B, 1), k, g), np.float32)
            grp, mem, tot = (np.zeros((max(B, 1), k), np.int32) for _ in range(3))
            for i in range(B):
                for j in range(cnt[i]):
                    grp[i, j], mem[i, j], tot[i, j] = 10 * i + j, [g, 1][j % 2], [g, 1][j % 2] + j
                    ids[i, j], sc[i, j] = row_ids(i, g) + 10 * j, row_scores(i, g) + j
            r["with_scores"] = a["sc"] is not None
            wr(a["ids"], np.int64, ids[:B] if top_k else [])   # (top_k = 0: every count is 0 and no row is written)
            if a["sc"] is not None:
                wr(a["sc"], np.float32, sc[:B] if top_k else [])
            for key, v in (("grp", grp), ("mem", mem), ("tot", tot)):
                wr(a[key], np.int32, v[:B])
            wr(a["cnt"], np.int32, cnt)
        else:
            top_k = a["top_k"] if "top_k" in a else a["p"]._obj.top_k
            k = max(top_k, 1)
            cnt = counts_for(B, top_k)
            ids, sc = np.zeros((max(B, 1), k), np.int64), np.zeros((max(B, 1), k), np.float32)
            for i in range(B):
                ids[i, : cnt[i]], sc[i, : cnt[i]] = row_ids(i, cnt[i]), row_scores(i, cnt[i])
            wr(a["ids"], np.int64, ids[:B] if top_k else [])   # (top_k = 0: every count is 0 and no row is written)
            wr(a["sc"], np.float32, sc[:B] if top_k else [])
            wr(a["cnt"], np.int32, cnt)
        self.calls.append(r)
        return rc


@pytest.fixture
def fake(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(api, "_lib", f)
    return f


@pytest.fixture
def ix(fake):
    index = api.MmapIndex(C.c_void_p(1))
    index.schema = F.make_schema({"year": np.arange(N_DOCS, dtype=np.int64)}, N_DOCS)
    yield index
    index.close()   # while the fake is still in place: the handle is not the real library's to close


def queries_of(B):
    """Query lengths 1 and 3 at dim 8; expected flat rows and offsets from these few lines."""
    lens = [3, 1, 3][:B]
    qs = [(np.arange(n * DIM, dtype=np.float32).reshape(n, DIM) + 100 * i) for i, n in enumerate(lens)]
    flat = np.concatenate([q.reshape(-1) for q in qs]) if qs else np.zeros(0, np.float32)
    return qs, flat, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


TQ_A = T.TextQuery.from_phrases([[3, 4], [7]])
TQ_B = T.TextQuery.from_phrases([[9]], T.NP_TEXT_OR)
TQ_A_C, TQ_B_C, NOTHING_C = ([3, 4, 7], [0, 2, 3], 2, 0), ([9], [0, 1], 1, 1), ([-1], [0, 1], 1, 0)
COND = ("year > ?", (2000,))
SUBSET = np.array([5, 1, 3], np.int64)
FORMS = ["none", "subset", "subsets", "filters"]


def scope_of(form, B):
    """(keyword arguments, expected sid, soff, n_sub, query map, filters) of a scope form for B queries."""
    prog = F.compile_filter(*COND, F.make_schema({"year": np.arange(N_DOCS, dtype=np.int64)}, N_DOCS))
    filt = [([tuple(o) for o in prog.ops], np.asarray(prog.values).tolist())]
    if form == "subset":
        return dict(subset=SUBSET), [5, 1, 3], [0, 3], 1, [0] * B, None
    if form == "subsets":
        a = np.array([4, 2, 9], np.int64)
        subs = [a, None, a][:B]   # a shared object and a None
        return dict(subsets=subs), [4, 2, 9] if B else [], [0, 3] if B else [0], min(B, 1), [0, -1, 0][:B], None
    if form == "filters":
        fl = [COND, None, ("year > ?", (2000,))][:B]   # two equal entries and a None
        return dict(filters=fl), None, None, min(B, 1), [0, -1, 0][:B], filt[: min(B, 1)]
    return {}, None, None, 0, None, None


def same(got, want):
    if want is None or got is None:
        return got is None and want is None
    return np.array_equal(np.asarray(got), np.asarray(want))


def check_queries(r, B, flat, off):
    assert r["h"] == 1 and r["B"] == B and r["dim"] == DIM
    assert r["off"].tolist() == off.tolist() and np.array_equal(r["flat"], flat)


def check_csr(r, sid, soff, n_sub, qmap):
    assert r["n_sub"] == n_sub and same(r["sid"], sid) and same(r["soff"], soff) and same(r["qsub"], qmap), r


def check_rows(res, B, top_k, live=None):
    """Counts k, 0, 1 in one batch: slices at stride max(top_k, 1), query ids, copies."""
    live = list(range(B)) if live is None else live
    cnt = counts_for(len(live), top_k)
    assert len(res) == B and [x.query_id for x in res] == list(range(B))
    for i, x in enumerate(res):
        c = cnt[live.index(i)] if i in live else 0
        j = live.index(i) if i in live else 0
        assert x.passage_ids.dtype == np.int64 and x.scores.dtype == np.float32
        assert np.array_equal(x.passage_ids, row_ids(j, c)) and np.array_equal(x.scores, row_scores(j, c))
        assert x.passage_ids.flags.owndata and x.scores.flags.owndata


def check_empty(res, B):
    assert len(res) == B and all(x.query_id == i and x.passage_ids.size == 0 and x.scores.size == 0 for i, x in enumerate(res))
    assert all(x.passage_ids.dtype == np.int64 and x.scores.dtype == np.float32 for x in res)


def expected_groups(B, top_k, g, scores=True):
    cnt = counts_for(B, top_k)
    return [[(10 * i + j, row_ids(i, [g, 1][j % 2]) + 10 * j, row_scores(i, [g, 1][j % 2]) + j if scores else None, [g, 1][j % 2] + j)
             for j in range(cnt[i])] for i in range(B)]


def check_groups(got, want):
    assert len(got) == len(want)
    for gq, wq in zip(got, want):
        assert len(gq) == len(wq)
        for (gid, gi, gs, gt), (wid, wi, ws, wt) in zip(gq, wq):
            assert (gid, gt) == (wid, wt) and isinstance(gid, int) and isinstance(gt, int)
            assert gi.dtype == np.int64 and np.array_equal(gi, wi) and gi.flags.owndata
            assert (gs is None) == (ws is None)
            if ws is not None:
                assert gs.dtype == np.float32 and np.array_equal(gs, ws) and gs.flags.owndata


B_K = [(B, k) for B in (0, 1, 3) for k in (0, 1, 5)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,top_k", B_K)
def test_search_batch(ix, fake, form, B, top_k):
    qs, flat, off = queries_of(B)
    kw, sid, soff, n_sub, qmap, filt = scope_of(form, B)
    p = api.SearchParameters(top_k=top_k, n_full_scores=77, n_ivf_probe=3, centroid_score_threshold=None, precision=1)
    res = ix.search_batch(qs, p, **kw)
    (r,) = fake.calls
    check_queries(r, B, flat, off)
    assert r["p"] == dict(top_k=top_k, n_full_scores=77, n_ivf_probe=3, centroid_batch_size=100_000, centroid_score_threshold=0.0,
                          has_threshold=0, precision=1)
    if form in ("none", "subset"):   # one subset for the batch stays on the one-subset entry, -1 = none
        assert r["entry"] == "np_hip_search_batch"
        assert (r["n_sub"], same(r["sub"], None)) == (-1, True) if form == "none" else (r["n_sub"] == 3 and same(r["sub"], sid))
    elif form == "subsets":
        assert r["entry"] == "np_hip_search_batch_subsets"
        check_csr(r, sid, soff, n_sub, qmap)
    else:
        assert r["entry"] == "np_hip_search_batch_filtered"
        assert r["n_f"] == n_sub and r["filt"] == filt and same(r["qsub"], qmap)
    check_rows(res, B, top_k)
    assert ix.last_stats is not None and "ms_total" in ix.last_stats


def test_search_batch_threshold_and_single_search(ix, fake):
    qs, flat, off = queries_of(1)
    one = ix.search(qs[0], api.SearchParameters(top_k=5), subset=SUBSET)
    r = fake.calls[-1]
    assert r["entry"] == "np_hip_search_batch" and r["n_sub"] == 3 and same(r["sub"], [5, 1, 3])
    assert r["p"]["has_threshold"] == 1 and r["p"]["centroid_score_threshold"] == np.float32(0.4) and r["p"]["precision"] == 2
    assert one.query_id == 0 and np.array_equal(one.passage_ids, row_ids(0, 5))
    ix.search(qs[0], api.SearchParameters(top_k=5), filter=COND)
    assert fake.calls[-1]["entry"] == "np_hip_search_batch_filtered" and fake.calls[-1]["qsub"].tolist() == [0]


def test_as_given_entries(ix, fake):
    """search_batch_csr / search_exact_csr / search_batch_filtered / search_exact_filtered: the arrays reach the library as
    given, None as NULL."""
    qs, flat, off = queries_of(3)
    p = api.SearchParameters(top_k=5)
    check_rows(ix.search_batch_csr(qs, p, [8, 9], [0, 1, 2], [1, -1, 0]), 3, 5)
    r = fake.calls[-1]
    assert r["entry"] == "np_hip_search_batch_subsets"
    check_csr(r, [8, 9], [0, 1, 2], 2, [1, -1, 0])
    check_rows(ix.search_batch_csr(qs, p, None, None, None), 3, 5)
    check_csr(fake.calls[-1], None, None, 0, None)
    check_rows(ix.search_exact_csr(qs, 5, 3, [8, 9], [0, 1, 2], [1, -1, 0]), 3, 5)
    r = fake.calls[-1]
    assert r["entry"] == "np_hip_search_exact" and (r["top_k"], r["precision"]) == (5, 3)
    check_csr(r, [8, 9], [0, 1, 2], 2, [1, -1, 0])
    n = len(fake.calls)
    for call in (lambda: ix.search_batch_csr(qs, p, [8], [0, 1], [0, 0]), lambda: ix.search_exact_csr(qs, 5, 0, [8], [0, 1], [0, 0])):
        with pytest.raises(ValueError, match="query_subset has 2 entries for 3 queries"):
            call()
    for call in (lambda: ix.search_batch_csr(qs, p, [8], [0, 4], [0, 0, 0]), lambda: ix.search_exact_csr(qs, 5, 0, [8], [0, 4], [0, 0, 0])):
        with pytest.raises(ValueError, match="subset_offsets count 4 ids, subset_ids has 1"):
            call()
    prog = F.compile_filter(*COND, ix.schema)
    with pytest.raises(ValueError, match="query_filter has 1 entries for 3 queries"):
        ix.search_batch_filtered(qs, p, [prog], [0])
    with pytest.raises(ValueError, match="query_filter has 1 entries for 3 queries"):
        ix.search_exact_filtered(qs, 5, 0, [prog], [0])
    assert len(fake.calls) == n
    check_rows(ix.search_exact_filtered(qs, 5, 3, [prog], [0, -1, 0]), 3, 5)
    r = fake.calls[-1]
    assert r["entry"] == "np_hip_search_exact_filtered" and r["filt"] == scope_of("filters", 3)[5] and r["qsub"].tolist() == [0, -1, 0]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,top_k", B_K)
def test_search_exact(ix, fake, form, B, top_k):
    """B = 0 with subset= is in the matrix on purpose: the one-subset query map has B entries here, not max(B, 1)."""
    qs, flat, off = queries_of(B)
    kw, sid, soff, n_sub, qmap, filt = scope_of(form, B)
    res = ix.search_exact(qs, top_k, precision=3, **kw)
    (r,) = fake.calls
    check_queries(r, B, flat, off)
    assert (r["top_k"], r["precision"]) == (top_k, 3)
    if form == "filters":
        assert r["entry"] == "np_hip_search_exact_filtered"
        assert r["n_f"] == n_sub and r["filt"] == filt and same(r["qsub"], qmap)
    else:
        assert r["entry"] == "np_hip_search_exact"
        check_csr(r, sid, soff, n_sub, qmap)
    check_rows(res, B, top_k)


def test_search_exact_takes_one_matrix_and_defaults_to_f32(ix, fake):
    q = queries_of(1)[0][0]
    check_rows(ix.search_exact(q, 5), 1, 5)
    assert fake.calls[-1]["B"] == 1 and fake.calls[-1]["precision"] == 0
    check_rows(ix.search_exact_csr([], 5, 0, None, None, np.zeros(0, np.int32)), 0, 5)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,top_k", B_K)
def test_text_search(ix, fake, form, B, top_k):
    """'' is skipped: the library sees the live queries and their entries of the query map; the skipped one gets an empty
    result under its own query id."""
    tqs = [TQ_A, "", TQ_B][:B]
    live = [i for i in range(B) if i != 1]
    kw, sid, soff, n_sub, qmap, filt = scope_of(form, B)
    res = ix.text_search(tqs, top_k, **kw)
    (r,) = fake.calls
    n = len(live)
    assert r["h"] == 1 and r["B"] == n and r["top_k"] == top_k and r["tq"] == [TQ_A_C, TQ_B_C][:n]
    lmap = None if qmap is None else [qmap[i] for i in live]
    if form == "filters":
        assert r["entry"] == "np_hip_text_search_filtered" and r["n_f"] == n_sub and r["filt"] == filt and same(r["qsub"], lmap)
    else:
        assert r["entry"] == "np_hip_text_search"
        check_csr(r, sid, soff, n_sub, lmap)
    check_rows(res, B, top_k, live)


def test_text_search_takes_one_string(ix, fake):
    check_rows(ix.text_search("", 5), 1, 5, [])
    assert fake.calls[-1]["B"] == 0
    with pytest.raises(ValueError, match="no keyword index"):
        ix.text_search("word", 5)


def hybrid_expect(r, form, B, sid, soff, n_sub, qmap, filt):
    if form == "filters":   # the filters ride behind the (NULL) CSR with the query map; n_subsets carries their count
        check_csr(r, None, None, n_sub, qmap)
        assert r["n_f"] == n_sub and r["filt"] == filt
    else:
        check_csr(r, sid, soff, n_sub, qmap)
        assert r["n_f"] == 0 and r["filt"] is None


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,top_k", B_K)
def test_search_hybrid(ix, fake, form, B, top_k):
    qs, flat, off = queries_of(B)
    tqs = [TQ_A, "", TQ_B][:B]
    kw, sid, soff, n_sub, qmap, filt = scope_of(form, B)
    res = ix.search_hybrid(qs, tqs, api.SearchParameters(top_k=top_k), **kw)
    (r,) = fake.calls
    assert r["entry"] == "np_hip_search_hybrid"
    check_queries(r, B, flat, off)
    assert r["tq"] == [TQ_A_C, NOTHING_C, TQ_B_C][:B]   # '' matches nothing, it is not skipped
    assert (r["fetch_k"], r["alpha"], r["fusion"], r["p"]["top_k"]) == (3 * top_k, 0.75, T.NP_FUSE_RELATIVE_SCORE, top_k)
    hybrid_expect(r, form, B, sid, soff, n_sub, qmap, filt)
    check_rows(res, B, top_k)
    ix.search_hybrid(qs, tqs, api.SearchParameters(top_k=top_k), alpha=0.25, fusion="rrf", fetch_k=11, **kw)
    r = fake.calls[-1]
    assert (r["fetch_k"], r["alpha"], r["fusion"]) == (11, 0.25, T.NP_FUSE_RRF)
    ix.search_hybrid(qs, tqs, api.SearchParameters(top_k=top_k), fusion=1, **kw)
    assert fake.calls[-1]["fusion"] == 1


def pool_k_default(top_k, limit):
    return max(1, min(max(20 * top_k, 200), max(N_DOCS, top_k), limit))


@pytest.mark.parametrize("group_size", [1, 2])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,top_k", B_K)
def test_search_grouped(ix, fake, form, B, top_k, group_size):
    qs, flat, off = queries_of(B)
    kw, sid, soff, n_sub, qmap, filt = scope_of(form, B)
    res = ix.search_grouped(qs, api.SearchParameters(top_k=top_k), group_size=group_size, **kw)
    (r,) = fake.calls
    assert r["entry"] == "np_hip_search_batch_grouped"
    check_queries(r, B, flat, off)
    assert (r["pool_k"], r["group_size"], r["p"]["top_k"]) == (pool_k_default(top_k, 16384), group_size, top_k)
    hybrid_expect(r, form, B, sid, soff, n_sub, qmap, filt)
    check_groups(res, expected_groups(B, top_k, group_size))
    raw = ix.search_grouped(qs, api.SearchParameters(top_k=top_k), group_size=group_size, pool_k=33, raw=True, **kw)
    assert fake.calls[-1]["pool_k"] == 33 and len(raw) == 6
    k = max(top_k, 1)
    assert [x.size for x in raw] == [max(B * k * group_size, 1)] * 2 + [max(B * k, 1)] * 3 + [max(B, 1)]
    assert raw[5][:B].tolist() == counts_for(B, top_k)


@pytest.mark.parametrize("group_size", [1, 2])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,top_k", B_K)
def test_search_hybrid_grouped(ix, fake, form, B, top_k, group_size):
    qs, flat, off = queries_of(B)
    tqs = [TQ_A, "", TQ_B][:B]
    kw, sid, soff, n_sub, qmap, filt = scope_of(form, B)
    res = ix.search_hybrid_grouped(qs, tqs, api.SearchParameters(top_k=top_k), group_size=group_size, **kw)
    (r,) = fake.calls
    assert r["entry"] == "np_hip_search_hybrid_grouped"
    check_queries(r, B, flat, off)
    pk = pool_k_default(top_k, 2048)
    assert r["tq"] == [TQ_A_C, NOTHING_C, TQ_B_C][:B]
    assert (r["pool_k"], r["fetch_k"], r["group_size"]) == (pk, min(3 * pk, 1024), group_size)
    assert (r["alpha"], r["fusion"], r["p"]["top_k"]) == (0.75, T.NP_FUSE_RELATIVE_SCORE, top_k)
    hybrid_expect(r, form, B, sid, soff, n_sub, qmap, filt)
    check_groups(res, expected_groups(B, top_k, group_size))
    ix.search_hybrid_grouped(qs, tqs, api.SearchParameters(top_k=top_k), group_size=group_size, pool_k=40, alpha=0.5, fusion="rrf", **kw)
    r = fake.calls[-1]
    assert (r["pool_k"], r["fetch_k"], r["alpha"], r["fusion"]) == (40, 120, 0.5, T.NP_FUSE_RRF)
    ix.search_hybrid_grouped(qs, tqs, api.SearchParameters(top_k=top_k), fetch_k=9, **kw)
    assert fake.calls[-1]["fetch_k"] == 9 and fake.calls[-1]["group_size"] == 1


@pytest.mark.parametrize("B", [0, 1, 3])
@pytest.mark.parametrize("matches", [True, False])
def test_score_pairs(ix, fake, B, matches):
    qs, flat, off = queries_of(B)
    docs = [[4, 4, 2], [], [9]][:B]   # an empty list of documents for one query
    out = ix.score_pairs(qs, docs, return_matches=matches, precision=3)
    (r,) = fake.calls
    assert r["entry"] == "np_hip_score_pairs" and r["precision"] == 3 and r["wants_matches"] == matches
    check_queries(r, B, flat, off)
    assert r["pair_off"].tolist() == [0, 3, 3, 4][: B + 1] and r["pair_docs"].tolist() == [4, 4, 2, 9][: r["pair_off"][-1]]
    p0 = r0 = 0
    assert len(out) == B
    for i in range(B):
        ni, li = len(docs[i]), qs[i].shape[0]
        sc, sims, pos = out[i] if matches else (out[i], None, None)
        assert sc.dtype == np.float32 and np.array_equal(sc, np.arange(p0, p0 + ni) + 0.5) and sc.flags.owndata
        if matches:
            assert sims.shape == (ni, li) and pos.shape == (ni, li) and pos.dtype == np.int32
            assert np.array_equal(sims.reshape(-1), np.arange(r0, r0 + ni * li) + 0.25)
            assert np.array_equal(pos.reshape(-1), np.arange(r0, r0 + ni * li))
        p0, r0 = p0 + ni, r0 + ni * li
    with pytest.raises(ValueError, match="doc_ids has"):
        ix.score_pairs(qs, docs + [[1]])


@pytest.mark.parametrize("B,top_k", B_K)
def test_fuse(ix, fake, B, top_k):
    sem = [[5, 6, 7], [], [1]][:B]
    kw = [[6], [8, 9], []][:B]
    ssc = [[.5, .25, .125], [], [1.]][:B]
    ksc = [[3.], [2., 1.], []][:B]
    out = api.fuse("relative_score", 0.5, top_k, sem, ssc, kw, ksc, index=ix)
    (r,) = fake.calls
    assert r["entry"] == "np_hip_fuse" and r["h"] == 1
    sw, kww = max([len(x) for x in sem] + [1]), max([len(x) for x in kw] + [1])
    assert (r["fusion"], r["alpha"], r["top_k"], r["B"], r["sem_w"], r["kw_w"]) == (T.NP_FUSE_RELATIVE_SCORE, 0.5, top_k, B, sw, kww)

    def padded(lists, w, dtype):
        m = np.zeros((B, w), dtype)
        for i, l in enumerate(lists):
            m[i, : len(l)] = l
        return m.reshape(-1)
    assert np.array_equal(r["sem_ids"], padded(sem, sw, np.int64)) and np.array_equal(r["kw_ids"], padded(kw, kww, np.int64))
    assert np.array_equal(r["sem_sc"], padded(ssc, sw, np.float32)) and np.array_equal(r["kw_sc"], padded(ksc, kww, np.float32))
    assert r["sem_cnt"].tolist() == [len(x) for x in sem] and r["kw_cnt"].tolist() == [len(x) for x in kw]
    cnt = counts_for(B, top_k)
    assert len(out) == B
    for i, (ids, sc) in enumerate(out):
        assert np.array_equal(ids, row_ids(i, cnt[i])) and np.array_equal(sc, row_scores(i, cnt[i]))
        assert ids.flags.owndata and sc.flags.owndata
    api.fuse_rrf(sem, kw, 0.5, top_k)   # no scores, no index: NULL score lists, NULL handle
    r = fake.calls[-1]
    assert r["fusion"] == T.NP_FUSE_RRF and r["h"] is None and r["sem_sc"] is None and r["kw_sc"] is None
    with pytest.raises(ValueError, match="semantic lists and"):
        api.fuse("rrf", 0.5, top_k, sem, None, kw + [[1]], None)


@pytest.mark.parametrize("group_size", [1, 2])
@pytest.mark.parametrize("scores", [True, False])
@pytest.mark.parametrize("B,top_k", B_K)
def test_collapse(ix, fake, B, top_k, group_size, scores):
    lists = [[5, 6, 7], [], [1]][:B]
    lsc = [[.5, .25, .125], [], [1.]][:B]
    out = api.collapse(lists, lsc if scores else None, top_k, group_size, ix)
    (r,) = fake.calls
    w = 3 if B else 1
    assert r["entry"] == "np_hip_collapse" and (r["top_k"], r["group_size"], r["B"], r["l_w"]) == (top_k, group_size, B, w)
    want = np.zeros((B, w), np.int64)
    for i, l in enumerate(lists):
        want[i, : len(l)] = l
    assert np.array_equal(r["l_ids"], want.reshape(-1)) and r["l_cnt"].tolist() == [len(x) for x in lists]
    assert (r["l_sc"] is not None) == scores and r["with_scores"] == scores
    check_groups(out, expected_groups(B, top_k, group_size, scores))


@pytest.mark.parametrize("n", [0, 1, 3])
def test_filter_ids(ix, fake, n):
    fl = [COND, "year IS NULL", F.compile_filter("year = ?", (7,), ix.schema)][:n]
    want = [F.compile_filter(*COND, ix.schema), F.compile_filter("year IS NULL", (), ix.schema), fl[2] if n == 3 else None][:n]
    want = [([tuple(o) for o in p.ops], np.asarray(p.values).tolist()) for p in want]
    counts = ix.filter_ids(fl, counts_only=True)
    (r,) = fake.calls
    assert r["entry"] == "np_hip_filter_eval" and r["n_f"] == n and r["filt"] == want and not r["wants_ids"] and r["f_cap"] == 0
    assert counts.tolist() == [2, 0, 3][:n]
    ids = ix.filter_ids(fl)
    assert [c["wants_ids"] for c in fake.calls[1:]] == [False, True] and fake.calls[-1]["f_cap"] == max(sum([2, 0, 3][:n]), 1)
    off = np.concatenate([[0], np.cumsum([2, 0, 3][:n])])
    assert len(ids) == n
    for j, x in enumerate(ids):
        assert x.dtype == np.int64 and np.array_equal(x, 7 + np.arange(off[j], off[j + 1])) and x.flags.owndata


def test_filters_without_columns_compile_against_an_empty_schema(ix, fake):
    ix.schema = None
    with pytest.raises(F.FilterError):
        ix.filter_ids([COND])
    with pytest.raises(F.FilterError):
        ix.search_batch(queries_of(1)[0], api.SearchParameters(), filters=[COND])
    assert fake.calls == []


# ---- policies ------------------------------------------------------------------------------------------------------------

BATCH_FORMS = [("np_hip_search_batch", "none"), ("np_hip_search_batch_subsets", "subsets"), ("np_hip_search_batch_filtered", "filters")]


@pytest.mark.parametrize("entry,form", BATCH_FORMS)
@pytest.mark.parametrize("B", [0, 1, 3])
def test_a_failed_search_is_empty_results_only_under_parallel(ix, fake, entry, form, B):
    qs = queries_of(B)[0]
    kw = scope_of(form, B)[0]
    fake.rc[entry] = 2
    check_empty(ix.search_batch(qs, api.SearchParameters(top_k=5), parallel=True, **kw), B)
    check_empty(ix.search_batch(qs, api.SearchParameters(top_k=5), **kw), B)   # parallel is the default
    with pytest.raises(api.SearchError, match=MESSAGE):
        ix.search_batch(qs, api.SearchParameters(top_k=5), parallel=False, **kw)
    assert [c["entry"] for c in fake.calls] == [entry] * 3
    fake.rc[entry] = 3
    with pytest.raises(api.ShapeError, match=MESSAGE):
        ix.search_batch(qs, api.SearchParameters(top_k=5), parallel=True, **kw)


def test_the_single_search_raises(ix, fake):
    fake.rc["np_hip_search_batch"] = 2
    with pytest.raises(api.SearchError, match=MESSAGE):
        ix.search(queries_of(1)[0][0], api.SearchParameters())


@pytest.mark.parametrize("rc,err", [(2, api.SearchError), (3, api.ShapeError), (7, MemoryError), (8, ValueError), (99, api.NextPlaidError)])
def test_every_other_entry_raises_the_mapped_error(ix, fake, rc, err):
    qs = queries_of(3)[0]
    tqs = [TQ_A, "", TQ_B]
    p = api.SearchParameters(top_k=5)
    calls = {
        "np_hip_search_exact": lambda: ix.search_exact(qs, 5),
        "np_hip_search_exact_filtered": lambda: ix.search_exact(qs, 5, filters=[COND] * 3),
        "np_hip_text_search": lambda: ix.text_search(tqs, 5),
        "np_hip_text_search_filtered": lambda: ix.text_search(tqs, 5, filters=[COND] * 3),
        "np_hip_search_hybrid": lambda: ix.search_hybrid(qs, tqs, p),
        "np_hip_search_batch_grouped": lambda: ix.search_grouped(qs, p),
        "np_hip_search_hybrid_grouped": lambda: ix.search_hybrid_grouped(qs, tqs, p),
        "np_hip_score_pairs": lambda: ix.score_pairs(qs, [[1], [2], [3]]),
        "np_hip_fuse": lambda: api.fuse("rrf", 0.5, 5, [[1]], None, [[2]], None, index=ix),
        "np_hip_collapse": lambda: api.collapse([[1]], None, 5, 1, ix),
        "np_hip_filter_eval": lambda: ix.filter_ids([COND]),
    }
    for entry, call in calls.items():
        fake.rc = {entry: rc}
        with pytest.raises(err, match=MESSAGE) as e:
            call()
        assert type(e.value) is err and fake.calls[-1]["entry"] == entry


def test_two_scopes_are_refused_before_the_library_is_touched(ix, fake):
    qs = queries_of(1)[0]
    p = api.SearchParameters(top_k=5)
    methods = {
        "search_batch": lambda **kw: ix.search_batch(qs, p, **kw),
        "search_exact": lambda **kw: ix.search_exact(qs, 5, **kw),
        "text_search": lambda **kw: ix.text_search([TQ_A], 5, **kw),
        "search_hybrid": lambda **kw: ix.search_hybrid(qs, [TQ_A], p, **kw),
        "search_grouped": lambda **kw: ix.search_grouped(qs, p, **kw),
        "search_hybrid_grouped": lambda **kw: ix.search_hybrid_grouped(qs, [TQ_A], p, **kw),
    }
    for name, call in methods.items():
        with pytest.raises(ValueError) as e:
            call(subset=SUBSET, subsets=[None])
        assert str(e.value) == f"{name} takes subset= (one for the batch) or subsets= (one per query), not both"
        for other in (dict(subset=SUBSET), dict(subsets=[None]), dict(subset=SUBSET, subsets=[None])):
            with pytest.raises(ValueError) as e:
                call(filters=[COND], **other)
            assert str(e.value) == f"{name} takes filters= or subset= / subsets=, not both"
        with pytest.raises(ValueError, match="subsets has 2 entries for 1 queries"):
            call(subsets=[None, None])
        with pytest.raises(ValueError, match="filters has 2 entries for 1 queries"):
            call(filters=[None, None])
    with pytest.raises(ValueError, match="search takes subset= or filter=, not both"):
        ix.search(qs[0], p, subset=SUBSET, filter=COND)
    for call in (lambda: ix.search_hybrid(qs, [TQ_A, TQ_B], p), lambda: ix.search_hybrid_grouped(qs, [TQ_A, TQ_B], p)):
        with pytest.raises(ValueError, match="1 queries and 2 text queries"):
            call()
    assert fake.calls == []


def test_a_query_of_the_wrong_shape_is_a_shape_error(ix, fake):
    bad = [np.zeros((2, DIM + 1), np.float32)]
    p = api.SearchParameters(top_k=5)
    for call in (lambda: ix.search_batch(bad, p), lambda: ix.search_batch(bad, p, subsets=[None]), lambda: ix.search_exact(bad, 5),
                 lambda: ix.search_hybrid(bad, [TQ_A], p), lambda: ix.search_grouped(bad, p), lambda: ix.score_pairs(bad, [[1]]),
                 lambda: ix.search_batch([np.zeros(DIM, np.float32)], p)):
        with pytest.raises(api.ShapeError, match="Shape error: query has shape"):
            call()
    assert fake.calls == []


def test_the_sharded_searcher_checks_query_shapes_before_anything_reaches_the_device(ix, fake):
    """CShardedSearcher.search_batch packs its queries as every other path does: a query that does not fit the index is a
    ShapeError raised on the host, before a tensor is made."""
    class NoTorch:
        def __getattr__(self, name):
            raise AssertionError("the device was touched")
    s = dist.CShardedSearcher.__new__(dist.CShardedSearcher)
    s.index, s.torch, s.stream, s.device, s.comm = ix, NoTorch(), None, None, None
    for bad in ([np.zeros((2, DIM + 1), np.float32)], [np.zeros(DIM, np.float32)]):
        with pytest.raises(api.ShapeError, match="Shape error: query has shape"):
            s.search_batch(bad, api.SearchParameters(top_k=5))
        with pytest.raises(api.ShapeError, match="Shape error: query has shape"):
            s.search_batch(bad, api.SearchParameters(top_k=5), subsets=[None])
    assert fake.calls == []


def test_header_calls_stand_alone(tmp_path):
    """tests/cpp/binding_calls_check.cpp: next_plaid.hpp against recording stubs of the entries it reaches, with the host
    compiler alone, under AddressSanitizer and UBSan -- the same three kinds of assertion for the C++ mirror."""
    exe = tmp_path / "binding_calls_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "binding_calls_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
