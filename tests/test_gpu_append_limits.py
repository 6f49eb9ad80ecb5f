"""np_hip_index_append at the limits of ivf_cut_merge_kernel and of the layouts it rebuilds (tests/append_limit_shapes.py holds the
cases, tests/test_append_limits_cpu.py proves that each reaches its edge).  Needs a real MI355X.

Per case the base is opened, the case's documents are appended in its stated calls, and the grown handle is held to
  1. append_restate.grown_arrays -- the base's OWN lists with the new ids behind them -- through export();
  2. a fresh handle of those arrays: _assert_equal_to_fresh of tests/test_gpu_index_append.py;
  3. the oracle on those arrays: stage by stage (compare_trace of tests/test_gpu_index_layouts.py: cells, candidates and
     selection equal, approximate scores bit-equal, exact scores within RTOL_F32) for two queries made of new documents'
     tokens, without a threshold under s3_gain 0 and 2 and with one under the default.  A debug trace turns the S4 filter
     off and with it the zeroth level (use_filter needs a call that is no trace), so the three regimes of the trace differ in
     the threshold alone; the level and the range table meet the oracle through search_batch instead: its answers under
     s3_gain 0 and 2 against the oracle's (assert_ranking_close, RTOL_F32), as compare_index does there;
  4. the fresh handle's integer counters of last_stats after the same call under s3_gain 0 and 2 (under s3_gain 1 the run /
     skip policy decides from earlier batches, so nothing is compared there).  Under s3_gain 0, and under s3_gain 2 on an
     index of ONE document range, all twelve (COUNTERS).  Under s3_gain 2 on an index of two or more ranges only
     UPSTREAM_AND_SELECTION, for this reason: gain_emit_kernel<1> fills S0 -- the documents whose exact bounds set the
     level's cut -- with the documents above the marginal level and then, as far as the slice goes, with those AT it, one
     atomicAdd(&n_marg[b]) reservation per range block; which marginal documents fall inside the slice depends on the order in
     which the ranges' blocks arrive ("any subset of the candidates is a valid S0").  The cut lcut, n_level0 (documents at
     levels >= lcut) and everything counted behind the cut -- n_cand_tokens, n_cand_codes, n_cand_dcodes, n_level2,
     n_survivors -- can therefore differ between two runs of one call on one handle; one range is one block per query and
     one order.  The filter preserves the selection, so n_exact_docs and n_exact_tokens stay compared, with the counters in
     front of S0 (n_cells, n_ivf_ids, n_candidates) and n_rounds.  n_rounds follows the pass's candidate pool, which comes
     from the workspace budget -- with the automatic workspace, the card's free memory at open -- and not from the index alone;
     at these sizes one round holds every candidate whatever the budget, and the comparison says so if that ever changes;
  5. the zeroth level: it must run (n_level0 > 0 under s3_gain 2 without a threshold) on every range-table case and on lists
     with extra pairs, and must stay off on lists that miss a pair;
  6. for the inverse-norm and capacity cases and the all-empty base, decompress_documents of EVERY new document against
     exact_restate.decompress64 inside decompress_limit_shapes.e_gpu, the decompress-limits suite's derived bound.
"""
import shutil

import numpy as np
import pytest

import append_limit_shapes as S
import append_restate as A
import decompress_limit_shapes as D
import exact_restate as X
import update_restate as U
from helpers import RTOL_F32, assert_ranking_close, hip_index, oracle_index, synth, to_oracle_params
from test_gpu_index_append import _assert_equal_to_fresh, _info, _queries, _split
from test_gpu_index_layouts import compare_trace

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu

COUNTERS = ("n_cells", "n_ivf_ids", "n_candidates", "n_cand_tokens", "n_cand_codes", "n_cand_dcodes", "n_level0", "n_level2",
            "n_survivors", "n_exact_docs", "n_exact_tokens", "n_rounds")
UPSTREAM_AND_SELECTION = ("n_cells", "n_ivf_ids", "n_candidates", "n_exact_docs", "n_exact_tokens", "n_rounds")


def P(thr):
    return npa.SearchParameters(n_full_scores=128, top_k=10, n_ivf_probe=8, centroid_score_threshold=thr)


def _against_the_oracle(hx, g, queries, what):
    ox = oracle_index(g)
    for thr, gain in ((None, 0), (None, 2), (0.4, 1)):
        hx.tune("s3_gain", gain)
        p = P(thr)
        for j, q in enumerate(queries[:2]):
            compare_trace(hx.debug_trace(q, p), ox.search(q, to_oracle_params(p), trace=True), f"{what} thr={thr} s3_gain={gain} q{j}")
    ref = ox.search_batch(queries, to_oracle_params(P(None)))
    for gain in (0, 2):      # untraced: the filter levels, and under 2 the zeroth level with its range table, are in the path
        hx.tune("s3_gain", gain)
        for i, (r, o) in enumerate(zip(hx.search_batch(queries, P(None)), ref)):
            assert_ranking_close(r.passage_ids, r.scores, o.passage_ids, o.scores, RTOL_F32, f"{what} s3_gain={gain} q{i}")
    hx.tune("s3_gain", 1)


def _counters(hx, fresh, queries, level, n_docs, what):
    for gain in (0, 2):
        compared = UPSTREAM_AND_SELECTION if gain == 2 and A.n_ranges(n_docs) > 1 else COUNTERS
        stats = []
        for h in (hx, fresh):
            h.tune("s3_gain", gain)
            h.search_batch(queries, P(None))
            stats.append({k: h.last_stats[k] for k in COUNTERS})
            h.tune("s3_gain", 1)
        print(f"{what} s3_gain={gain}: grown {stats[0]} fresh {stats[1]}")
        level0 = [st["n_level0"] for st in stats]
        stats = [{k: st[k] for k in compared} for st in stats]
        assert stats[0] == stats[1], f"{what} s3_gain={gain}: grown {stats[0]} fresh {stats[1]}"
        if gain == 0:
            assert level0 == [0, 0]
        elif level is not None:
            assert [n > 0 for n in level0] == [level, level], (what, level, level0)


def _decompress_all(hx, g, n_old, what):
    lens = np.asarray(g["doc_lengths"], np.int64)
    off = A.offsets(lens)
    ids = np.arange(n_old, lens.size, dtype=np.int64)
    got, got_lens = hx.decompress_documents(ids)
    assert np.asarray(got_lens).tolist() == lens[n_old:].tolist() and got.shape == (int(off[-1] - off[n_old]), S.DIM)
    ref = X.decompress64(dict(g))[off[n_old]:]
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = D.e_gpu(S.DIM)
    worst = float(np.max(err / np.maximum(np.abs(ref), 1e-300) / D.U, initial=0.0))
    print(f"{what}: {got.shape[0]} new rows, worst error {worst:.3f} u, bound {bound:.3f} u")
    assert np.all(err <= bound * D.U * np.abs(ref)), f"{what}: {worst:.3f} u over {bound:.3f} u"


@pytest.mark.parametrize("case", S.all_cases(), ids=lambda c: c.name)
def test_append_at_the_limit(case):
    base, n_old = case.base, case.n_old
    t_old = int(base["doc_lengths"].sum())
    new = case.new
    g = case.grown()
    queries = _queries(base, new)
    if len(queries) < 2:      # a single new document: a second draw of its tokens
        queries = queries + _queries(base, new, seed=12)
    assert len(queries) >= 2
    hx, fresh = hip_index(base), hip_index(g)
    try:
        if case.reserve:
            hx.reserve(*case.reserve)
            assert hx.capacity() == (n_old + case.reserve[0], t_old + case.reserve[1])
        first = n_old
        for lens, codes, res in case.steps:
            ids = hx.append_arrays(lens, codes, res)
            assert ids.tolist() == list(range(first, first + len(lens)))
            first += len(lens)
        want_cap = S.capacity_after(case) if case.reserve else (g["doc_lengths"].size, int(g["doc_lengths"].sum()))
        assert hx.capacity() == want_cap, (hx.capacity(), want_cap)
        got = hx.export()
        for k in ("doc_lengths", "codes", "residuals", "ivf", "ivf_lengths"):                       # 1
            assert np.array_equal(got[k], g[k]), f"{case.name}: export()[{k!r}] against grown_arrays"
        _assert_equal_to_fresh(hx, fresh, queries, n_old, case.name)                                 # 2
        _against_the_oracle(hx, g, queries, case.name)                                               # 3
        _counters(hx, fresh, queries, case.level, g["doc_lengths"].size, case.name)                                         # 4, 5
        if case.decompress_all:
            _decompress_all(hx, g, n_old, case.name)                                                 # 6
    finally:
        hx.close()
        fresh.close()


def test_several_appends_on_a_directory(tmp_path):
    """three MmapIndex.append calls of 7, 30 and 1 documents, then load of the directory: equal info -- avg_doclen, the
    repeated expression (old_avg * old_n + new_tokens) / n, as a double with no tolerance -- equal answers, and the files the
    restated update_index leaves after the same three steps"""
    spec, a, _ = _split(600, 0)
    cut, wts = synth.bucket_tables(spec)
    d, e = str(tmp_path / "a"), str(tmp_path / "b")
    npa.write_index_dir(d, a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=500)
    shutil.copytree(d, e)
    batches = S.directory_documents(a["centroids"])
    assert [len(b) for b in batches] == list(S.DIR_STEPS) and len(set(S.DIR_STEPS)) == 3
    hx = npa.MmapIndex.load(d)
    try:
        first = 600
        for batch in batches:
            assert hx.append(batch).tolist() == list(range(first, first + len(batch)))
            first += len(batch)
            U.update_index(e, batch, 50_000, False)
        assert U.dir_state(d) == U.dir_state(e)
        fresh = npa.MmapIndex.load(d)
        try:
            assert _info(hx) == _info(fresh)
            assert float(hx.info.avg_doclen) == float(fresh.info.avg_doclen) and hx.num_documents() == first
            docs = [x for b in batches for x in b]
            qs = [np.ascontiguousarray(x[:8] / np.linalg.norm(x[:8], axis=1, keepdims=True), np.float32)
                  for x in sorted(docs, key=lambda x: -x.shape[0])[:4]]
            _assert_equal_to_fresh(hx, fresh, qs, 600, "three appends vs load")
        finally:
            fresh.close()
    finally:
        hx.close()


# ---- the append under the expand's body: its way back, and a call with nothing to merge -------------------------------------
def _state(hx, queries):
    """what a refused append must leave as it was: the export, the info and the answers to the query set, as bytes"""
    a = hx.export()
    return ({k: np.ascontiguousarray(a[k]).tobytes() for k in ("doc_lengths", "codes", "residuals", "ivf", "ivf_lengths")}, _info(hx),
            [(r.passage_ids.tobytes(), np.asarray(r.scores, np.float32).tobytes()) for r in hx.search_batch(queries, P(None))])


WAY_BACK = [next(c for c in S.all_cases() if c.notes.get("residue") == 1), S.case("raw list over a tile edge")]


@pytest.mark.parametrize("case", WAY_BACK, ids=lambda c: c.name)
def test_a_refused_append_puts_the_handle_back(case):
    """np_hip_index_tune "expand_fail" governs the body that the append shares with the expand: after the token stages (the new
    tokens and doc offsets already lie behind the old ones), the distinct-code rebuild, the posting lists and the range table
    the call returns OutOfMemory as a refused allocation there would.  After each refusal the handle's export, info and
    answers are byte for byte what they were; with the knob back at 0 the same append succeeds and equals the fresh handle.
    The second case appends a document of more than NP_UNIQ_MAX = 4096 tokens, the raw-list path."""
    assert case.name.startswith("residue") or case.new[0].max() > A.NP_UNIQ_MAX
    base, n_old, new, g = case.base, case.n_old, case.new, case.grown()
    queries = _queries(base, new)
    hx, fresh = hip_index(base), hip_index(g)
    try:
        before = _state(hx, queries)
        for stage in (1, 2, 3, 4):
            hx.tune("expand_fail", stage)
            with pytest.raises(MemoryError, match=f"np_hip_index_append: out of memory after stage {stage}"):
                hx.append_arrays(*new)
            after = _state(hx, queries)
            for part, (x, y) in zip(("export", "info", "answers"), zip(before, after)):
                assert x == y, f"{case.name}: {part} changed by an append refused after stage {stage}"
        hx.tune("expand_fail", 0)
        assert hx.append_arrays(*new).tolist() == list(range(n_old, n_old + len(new[0])))
        got = hx.export()
        for k in ("doc_lengths", "codes", "residuals", "ivf", "ivf_lengths"):
            assert np.array_equal(got[k], g[k]), f"{case.name}: export()[{k!r}] against grown_arrays"
        _assert_equal_to_fresh(hx, fresh, queries, n_old, case.name)
    finally:
        hx.close()
        fresh.close()


def test_a_refused_append_rows_keeps_columns_and_groups():
    """the same four refusals through np_hip_index_append_rows: get_column / get_groups give the bytes they gave before, and
    the append that then succeeds leaves the old rows in front of the new ones"""
    case = WAY_BACK[0]
    base, n_old, new = case.base, case.n_old, case.new
    n_new = len(new[0])
    rng = np.random.default_rng(7300)
    langs = ["de", "en", "fr"]

    def values(n):
        r = rng.random(n)
        return ({"i": rng.integers(-5, 50, n), "f": np.where(r < 0.25, np.nan, rng.standard_normal(n)),
                 "s": [None if r[d] > 0.8 else langs[j] for d, j in enumerate(rng.integers(0, 3, n))]},
                [None if r[d] < 0.1 else int(k) for d, k in enumerate(rng.integers(0, 40, n))])

    (old_vals, old_keys), (new_vals, new_keys) = values(n_old), values(n_new)
    queries = _queries(base, new)

    def read_back(hx):
        out = {}
        for name in old_vals:
            data, valid = hx.get_column(name)
            out[name] = (data.tobytes(), None if valid is None else np.asarray(valid).tobytes())
        out["groups"] = hx.get_groups().tobytes()
        return out

    hx = hip_index(base)
    try:
        hx.set_columns(old_vals)
        hx.set_groups(old_keys)
        before, rows_before = _state(hx, queries), read_back(hx)
        for stage in (1, 2, 3, 4):
            hx.tune("expand_fail", stage)
            with pytest.raises(MemoryError, match=f"np_hip_index_append_rows: out of memory after stage {stage}"):
                hx.append_arrays(*new, rows=npa.api.AppendRows(columns=new_vals, groups=new_keys))
            assert read_back(hx) == rows_before, f"columns or groups changed by an append refused after stage {stage}"
            assert _state(hx, queries) == before, f"the handle changed by an append refused after stage {stage}"
        hx.tune("expand_fail", 0)
        ids = hx.append_arrays(*new, rows=npa.api.AppendRows(columns=new_vals, groups=new_keys))
        assert ids.tolist() == list(range(n_old, n_old + n_new))
        data, _ = hx.get_column("i")
        assert np.array_equal(data, np.concatenate([old_vals["i"], new_vals["i"]]))
        gids = hx.get_groups()
        assert gids.size == n_old + n_new and gids[:n_old].tobytes() == rows_before["groups"]
        got, g = hx.export(), case.grown()
        for k in ("doc_lengths", "codes", "residuals", "ivf", "ivf_lengths"):
            assert np.array_equal(got[k], g[k]), f"export()[{k!r}] against grown_arrays"
    finally:
        hx.close()


def test_documents_without_a_token_leave_the_lists_alone():
    """three documents of length 0 add no (code, document) pair: the append writes no new list array -- the export's lists
    are the base's, and np_hip_index_info reports the device bytes of a fresh handle of the same arrays.  np_hip_index_expand
    with k_new = 0 and n_replace = 0 of the same documents is the same call under the other entry's name."""
    base = S.short_base(np.random.default_rng(7301), 300)
    empty = (np.zeros(3, np.int64), np.zeros(0, np.int64), np.zeros((0, S.PD), np.uint8))
    g = A.grown_arrays(base, empty)
    assert np.array_equal(g["ivf"], base["ivf"]) and np.array_equal(g["ivf_lengths"], base["ivf_lengths"])
    queries = _queries(base, S.rand_docs(np.random.default_rng(7302), [8, 8, 8, 8], 256))
    hx, ex, fresh = hip_index(base), hip_index(base), hip_index(g)
    try:
        assert hx.append_arrays(*empty).tolist() == [300, 301, 302]
        assert ex.expand_arrays(np.zeros((0, S.DIM), np.float32), *empty, n_replace=0).tolist() == [300, 301, 302]
        for h, what in ((hx, "append"), (ex, "expand(0, 0)")):
            got = h.export()
            for k in ("doc_lengths", "codes", "residuals", "ivf", "ivf_lengths"):
                assert np.array_equal(got[k], g[k]), f"{what}: export()[{k!r}]"
            assert h.num_documents() == 303 and _info(h) == _info(fresh), what
            assert int(h.info.device_bytes) == int(fresh.info.device_bytes), (what, int(h.info.device_bytes), int(fresh.info.device_bytes))
        assert _state(hx, queries) == _state(ex, queries) == _state(fresh, queries)
    finally:
        hx.close()
        ex.close()
        fresh.close()
