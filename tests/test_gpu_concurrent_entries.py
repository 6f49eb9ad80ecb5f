"""Every host entry point that checks a context out of the handle's pool, from six threads at once on one handle.  All of them
carve the same per-context arena, pinned area, filter scratch and filter CSR, which grow on demand -- here while other threads
wait for, or run on, the other context.  Needs a real MI355X.

The entries that check a context out (ContextUse::begin), file by file, and the call of the list that drives each:
  np_search.hip  np_hip_search_batch, _subsets, _filtered             search_batch, with subsets, with filters
                 np_hip_search_batch_device, _subsets_device,          not in the list: the same pass behind the staging of the
                 np_hip_search_phase_a / _b                            host forms; the phases belong to the sharded search (ranks)
  np_scan.hip    np_hip_search_exact, _filtered                       search_exact
                 np_hip_search_exact_device                            not in the list: the same code behind the staging
  np_pairs.hip   np_hip_score_pairs                                   score_pairs
                 np_hip_score_pairs_device                             not in the list: the same code behind the staging
  np_filter.hip  np_hip_filter_eval                                   filter_ids
  np_match.hip   np_hip_text_match                                     not in the list: it needs a column's text in HBM
                                                                       (text_on_device), which would change how the LIKE filters
                                                                       of this list are evaluated
  np_text.hip    np_hip_text_search, _filtered                        text_search at top_k 1 and 1024
                 np_hip_text_search_expr, _expr_filtered              tree text_search at top_k 1 and 1024: single-token
                                                                       prefixes, a prefix at the end of a phrase of several
                                                                       tokens, NOTs.  The prefix pre-pass is the one place
                                                                       where a call synchronises in its middle and reads
                                                                       through the pinned area
                 np_hip_fuse                                          fuse
                 np_hip_search_hybrid, np_hip_search_hybrid_expr      search_hybrid, with filters, with trees
                 np_hip_search_hybrid_grouped                         search_hybrid_grouped
                 np_hip_text_search_device, np_hip_fuse_device         not in the list: the same code behind the staging
                 np_hip_text_search_sharded, _sharded_filtered,        not in the list: they need ranks
                 np_hip_search_hybrid_sharded
  np_group.hip   np_hip_collapse                                      collapse
                 np_hip_search_batch_grouped                          search_grouped
                 np_hip_collapse_device                                not in the list: the same code behind the staging

Every result must be, bit for bit, what the same call gave when it ran alone; the serial run is itself checked: the keyword
results against tests/text_restate.py, the trees against tests/text_expr_restate.py, the filters against
tests/filter_restate.py, and the grouped calls against the walk of tests/collapse_restate.py over the serial search_batch and
search_hybrid lists."""
import threading

import numpy as np
import pytest

from helpers import hip_index, make_arrays, synth

import next_plaid_amd as npa
from next_plaid_amd import text as T
import collapse_restate as CR
import filter_restate as FR
import text_restate as TR
import text_expr_restate as TX

pytestmark = pytest.mark.gpu

N_DOCS = 1500
N_THREADS = 6
ROUNDS = 3


def flat(x):
    """A result as bytes that compare: QueryResults, (ids, scores) pairs, arrays, tuples and lists of them."""
    if isinstance(x, npa.api.QueryResult):
        return (x.query_id, x.passage_ids.tobytes(), x.scores.tobytes())
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (list, tuple)):
        return tuple(flat(y) for y in x)
    return x


@pytest.fixture(scope="module")
def material():
    spec, a = make_arrays(num_docs=N_DOCS, num_centroids=64, dim=32, nbits=2, doc_len_min=4, doc_len_max=12, seed=11)
    qs = list(synth.make_queries(spec, 9, n_tokens=8, cen=a["centroids"])[0])
    rows = FR.make_rows(N_DOCS, seed=3)
    texts = TR.make_texts(N_DOCS, 12, seed=N_DOCS, every="wo0", lens=(0, 1, 2, 3, 5, 8, 13, 21))
    data = T.TextIndexData.from_texts(texts)
    return spec, a, qs, rows, data


@pytest.mark.parametrize("n_contexts", [1, 2])
def test_every_entry_point_from_six_threads(material, n_contexts):
    spec, a, qs, rows, data = material
    hx = hip_index(a, n_contexts=n_contexts)
    try:
        hx.set_columns(rows)
        hx.set_text(data)
        sch = hx.schema
        # everything that needs the compilers (and their SQLite connection) happens here, before any thread starts
        conds = [("y > ? AND s IS NOT NULL", [0]), None, ("z = ? AND z = ?", [1, 2]), ("1=1", []), ("x < ? OR t LIKE ?", [0.5, "%a%"]),
                 ("z < ?", [2]), None, ("w BETWEEN ? AND ?", [-0.5, 1.0]), ("NOT (x > ?)", [0.0])]
        progs = [None if c is None else npa.compile_filter(c[0], c[1], sch) for c in conds]
        live = [p for p in progs if p is not None]
        tq = [T.compile_text_query(s, data) for s in ("wo1 wo2", "wo3 OR wo5 OR wo7", '"wo1 wo0"', "wo0", "nowhere", "wo2",
                                                       '"wo1 wo0" OR wo4', "wo5 AND wo1 AND wo0", "wo0 OR wo1")]
        rs = TR.Restated(data, N_DOCS)
        trees = [T.compile_text_expr(s, data) for s in ("wo1*", "wo2 NOT wo1*", '"wo1 wo" *', "(wo3* OR wo5) AND wo0", "nowhere*",
                                                         "wo1* NOT (wo2 OR wo3*)", '"wo0 wo1" * OR wo4', "wo5 AND wo1* AND wo0",
                                                         "wo* NOT nowhere")]
        xs = TX.RestatedExpr(data, N_DOCS)
        groups = (np.arange(N_DOCS) * 7 % 37).astype(np.int32)
        hx.set_groups(groups, n_groups=37)
        pg = npa.SearchParameters(n_full_scores=128, top_k=3, n_ivf_probe=4)
        pool = lambda k: npa.SearchParameters(n_full_scores=128, top_k=k, n_ivf_probe=4)
        pooled = hx.search_batch(qs, pool(64))                         # the ranked lists that collapse walks
        some = np.arange(0, N_DOCS, 3)
        subsets = [None, some, some, None, np.zeros(0, np.int64), some, None, np.arange(N_DOCS), some]
        pairs = [np.array([3, 14, 15, 92, 653, 589, 793, 238][: i + 1]) for i in range(len(qs))]
        p = npa.SearchParameters(n_full_scores=128, top_k=7, n_ivf_probe=4)
        cap = T.NP_TEXT_MAX_TOPK
        calls = {
            "search_batch": lambda: hx.search_batch(qs, p),
            "search_batch subsets": lambda: hx.search_batch(qs, p, subsets=subsets),
            "search_exact": lambda: hx.search_exact(qs, 10),
            "score_pairs": lambda: hx.score_pairs(qs, pairs),
            "filter_ids": lambda: hx.filter_ids(live),
            "search_batch filters": lambda: hx.search_batch(qs, p, filters=progs),
            "text_search 1": lambda: hx.text_search(tq, 1),
            "text_search 1024": lambda: hx.text_search(tq, cap),
            "fuse": lambda: npa.fuse("relative_score", 0.75, 2 * cap, fuse_in[0], fuse_in[1], fuse_in[2], fuse_in[3], index=hx),
            "search_hybrid": lambda: hx.search_hybrid(qs, tq, p, alpha=0.75, fusion="relative_score", fetch_k=40),
            "search_hybrid filters": lambda: hx.search_hybrid(qs, tq, p, alpha=0.5, fusion="rrf", filters=progs),
            "text_search trees 1": lambda: hx.text_search(trees, 1),
            "text_search trees 1024": lambda: hx.text_search(trees, cap),
            "search_hybrid trees": lambda: hx.search_hybrid(qs, trees, p, alpha=0.75, fusion="relative_score", fetch_k=40),
            "collapse": lambda: npa.collapse([r.passage_ids for r in pooled], [r.scores for r in pooled], 5, 3, hx),
            "search_grouped": lambda: hx.search_grouped(qs, pg, group_size=2, pool_k=64),
            "search_hybrid_grouped": lambda: hx.search_hybrid_grouped(qs, tq, pg, group_size=2, pool_k=60, alpha=0.75,
                                                                      fusion="relative_score", fetch_k=40),
        }
        kw = hx.text_search(tq, cap)
        sem = hx.search_exact(qs, cap)
        fuse_in = ([r.passage_ids for r in sem], [r.scores for r in sem], [r.passage_ids for r in kw], [r.scores for r in kw])
        names = list(calls)
        serial = {name: flat(calls[name]()) for name in names}
        # the serial baseline is itself pinned: the keyword results and the filters' ids to their restatements
        for k_, name in ((1, "text_search 1"), (cap, "text_search 1024")):
            for q, r in zip(tq, calls[name]()):
                ids, sc = rs.search(q, k_)
                assert np.array_equal(r.passage_ids, ids) and np.array_equal(r.scores.view(np.uint32), sc.view(np.uint32)), name
        assert max(r.passage_ids.size for r in kw) == cap
        want_ids = [FR.select(f, sch) for f in live]
        assert all(np.array_equal(g, w) for g, w in zip(calls["filter_ids"](), want_ids)) and sum(w.size for w in want_ids) > N_DOCS
        by_subsets = hx.search_batch(qs, p, subsets=[None if f is None else FR.select(f, sch) for f in progs])
        assert flat(by_subsets) == serial["search_batch filters"]
        assert sum(r.passage_ids.size for r in calls["search_hybrid filters"]()) > 0
        # ... the trees to their restatement, the grouped calls to the walk over the serial lists
        assert [sum(1 for r in q.prefix if r is not None) for q in trees] == [1, 1, 1, 1, 1, 2, 1, 1, 1] and trees[2].phrases()[0][0] >= 0
        for k_, name in ((1, "text_search trees 1"), (cap, "text_search trees 1024")):
            for q, r in zip(trees, calls[name]()):
                ids, sc = xs.expr_search(q, k_)
                assert np.array_equal(r.passage_ids, ids) and np.array_equal(r.scores.view(np.uint32), sc.view(np.uint32)), name
        by_tree = calls["text_search trees 1024"]()
        assert max(r.passage_ids.size for r in by_tree) == cap and by_tree[2].passage_ids.size > 0 and by_tree[4].passage_ids.size == 0
        assert sum(r.passage_ids.size for r in calls["search_hybrid trees"]()) > 0
        walks = lambda base, top_k, gs: [CR.walked(CR.walk(r.passage_ids, r.scores, groups, top_k, gs)) for r in base]
        listed = lambda got: [CR.listed(g) for g in got]
        assert listed(calls["collapse"]()) == walks(pooled, 5, 3)
        assert listed(calls["search_grouped"]()) == walks(pooled, 3, 2)
        assert listed(calls["search_hybrid_grouped"]()) == walks(
            hx.search_hybrid(qs, tq, pool(60), alpha=0.75, fusion="relative_score", fetch_k=40), 3, 2)
        assert all(len(g) == 3 for g in calls["search_grouped"]()) and any(t > 1 for g in calls["collapse"]() for _, _, _, t in g)

        out, errs = {}, []
        start = threading.Barrier(N_THREADS)

        def work(t):
            try:
                start.wait(timeout=60)
                mine = []
                for r in range(ROUNDS):
                    for j in range(len(names)):
                        name = names[(j + 2 * t + r) % len(names)]           # every thread in another rotation
                        mine.append((name, flat(calls[name]())))
                out[t] = mine
            except BaseException as e:  # pragma: no cover
                errs.append((t, repr(e)))

        ts = [threading.Thread(target=work, args=(t,)) for t in range(N_THREADS)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert not errs, errs
        assert sorted(out) == list(range(N_THREADS))
        for t in range(N_THREADS):
            assert len(out[t]) == ROUNDS * len(names)
            for i, (name, got) in enumerate(out[t]):
                assert got == serial[name], f"n_contexts={n_contexts}, thread {t}, call {i} ({name}) differs from the serial result"
    finally:
        hx.close()
