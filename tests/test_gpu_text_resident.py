"""The resident keyword index: np_hip_index_set_text_build, np_hip_index_text_merge and the read-back, through
MmapIndex.build_text / update_text with resident=True and the routing of append and remove.  The oracle is the host path:
TextIndexData.from_texts (SQLite) -> set_text on a second handle of the same index.  Equal means: get_text_layout byte-equal
between the two handles, get_text array-equal to from_texts, and text_search / search_hybrid the same bytes."""
import ctypes as C
import threading

import numpy as np
import pytest

from helpers import hip_index, make_arrays, synth

import next_plaid_amd as npa
from next_plaid_amd import api
from next_plaid_amd import text as T
from next_plaid_amd.text import TextIndexData

import textres_restate as X
from textbuild_limit_shapes import assert_same as _same, rows_after, sqlite_rows

pytestmark = pytest.mark.gpu

CHUNK = X.CHUNK


def arrays(n_docs):
    return make_arrays(num_docs=max(n_docs, 1), num_centroids=16, dim=32, nbits=2, doc_len_min=1, doc_len_max=1, seed=3)


_PAIRS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_pairs():
    """The handles pair() opened leave HBM with this module."""
    yield
    for _, _, hx, ref in _PAIRS.values():
        hx.close()
        ref.close()
    _PAIRS.clear()


def pair(n_docs):
    """(spec, arrays, the handle under test, the reference handle), shared by the tests of one document count."""
    if n_docs not in _PAIRS:
        spec, a = arrays(n_docs)
        _PAIRS[n_docs] = (spec, a, hip_index(a), hip_index(a))
    return _PAIRS[n_docs]


def layouts_equal(hx, ref):
    got, want = hx.get_text_layout(), ref.get_text_layout()
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    a, b = hx.text_sizes(), ref.text_sizes()
    assert a == b, (a, b)
    return got


def searches_equal(hx, ref, spec, a, queries, k=7):
    if not queries:
        return
    for x, y in zip(hx.text_search(queries, k), ref.text_search(queries, k)):
        assert x.passage_ids.tobytes() == y.passage_ids.tobytes() and x.scores.tobytes() == y.scores.tobytes()
    qs, _ = synth.make_queries(spec, len(queries), n_tokens=4, cen=a["centroids"])
    p = npa.SearchParameters(n_full_scores=32, top_k=k, n_ivf_probe=4)
    for x, y in zip(hx.search_hybrid(qs, queries, p), ref.search_hybrid(qs, queries, p)):
        assert x.passage_ids.tobytes() == y.passage_ids.tobytes() and x.scores.tobytes() == y.scores.tobytes()


def equal_to_rows(hx, ref, spec, a, rows, tokenizer="unicode61", queries=()):
    """The handle under test against SQLite on `rows` ({id: text}) set on the reference handle by the host path."""
    want = sqlite_rows(rows, tokenizer)
    ref.set_text(want)
    if want.n_rows == 0 and want.inst_doc.size == 0:      # no instances and no rows: both paths drop the keyword index
        assert hx.text is None
        with pytest.raises(ValueError, match="no keyword index"):
            hx.text_sizes()
        return want
    lay = layouts_equal(hx, ref)
    _same(hx.get_text(), want)
    re = X.layout(want.term_offsets, want.inst_doc, hx.num_documents())
    for name, arr in zip(("post_off", "post_doc", "post_tf", "post_first", "doc_len"), re):
        assert np.array_equal(lay[name], arr), name
    searches_equal(hx, ref, spec, a, list(queries))
    return want


def build_and_check(texts, tokenizer="unicode61", n_docs=None, queries=(), fallback=()):
    spec, a, hx, ref = pair(len(texts) if n_docs is None else n_docs)
    data = hx.build_text(texts, tokenizer, resident=True)
    want = equal_to_rows(hx, ref, spec, a, dict(enumerate(texts)), tokenizer, queries)
    if data is not None:
        assert data.resident and data is hx.text and data.terms == want.terms and data.n_rows == want.n_rows
        assert data.fallback_docs == list(fallback)
    return hx, ref, data, want


# ---- install from a build ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokenizer", ["unicode61", "trigram", "identifier_aware"])
def test_the_three_tokenizers(tokenizer):
    texts = ["alpha beta gamma", "beta getUserName", "", "gamma gamma alpha_beta", "delta", "beta alpha", "", "gamma"]
    build_and_check(texts, tokenizer, queries=["beta", "gamma alpha"] if tokenizer != "trigram" else ["bet", "gamma"])


def test_tables_without_instances_and_one_instance():
    hx, ref, data, _ = build_and_check(["", "", ""])                      # rows without tokens: an index of no term
    assert data.n_rows == 3 and data.terms == [] and hx.text_sizes()["n_postings"] == 0
    assert data.term_offsets.tolist() == [0] and data.inst_doc.size == 0
    hx, ref, data, _ = build_and_check([], n_docs=3)                      # no rows: dropped, as set_text drops it
    assert data is None
    build_and_check(["", "a", ""], queries=["a"])                         # one instance


def test_every_instance_its_own_posting_and_terms_that_meet_in_one_document():
    build_and_check(["a b c", "b c d", "c d e", "d e a"], queries=["a", "c d"])
    # "a" ends with document 2 and "b" begins with it: without the term-start rule the two postings fuse
    hx, ref, data, want = build_and_check(["a", "", "a b", "c b"], queries=["a", "b", "a b"])
    lay = hx.get_text_layout()
    assert lay["post_doc"].tolist() == [0, 2, 2, 3, 3] and lay["post_off"].tolist() == [0, 2, 4, 5]
    build_and_check(["x y", "y y z", "z z"], queries=["y", "z"])           # ... with tf > 1 on both sides


def test_documents_without_tokens_and_n_rows_above_the_documents_that_hold_a_token():
    texts = ["", "", "a b", "", "b", "", "", "a a", "", ""]
    hx, ref, data, want = build_and_check(texts, queries=["a", "b"])
    assert want.n_rows == 10 and np.count_nonzero(hx.get_text_layout()["doc_len"]) == 3
    build_and_check(texts, n_docs=len(texts) + 5, queries=["a"])           # a handle of more documents than rows


def test_one_posting_across_a_scan_chunk_and_heads_at_its_edge():
    build_and_check(["m " * (CHUNK + 5)], queries=["m"])                  # one term, one document, 2053 positions
    # one posting of 2047 positions, then heads at instances 2047, 2048 and 2049
    hx, ref, data, want = build_and_check(["m " * (CHUNK - 1), "m", "m", "m m"], queries=["m", "m m"])
    assert hx.get_text_layout()["post_first"].tolist() == [0, CHUNK - 1, CHUNK, CHUNK + 1]


@pytest.fixture(scope="module")
def large():
    """More than 524 288 instances: the scan's block sums take a second round (256 chunks of 2048)."""
    rng = np.random.default_rng(11)
    words = np.asarray([f"w{i}" for i in range(400)])
    texts = [" ".join(words[rng.integers(0, 400, 1800)]) for _ in range(300)]
    assert 300 * 1800 > CHUNK * X.SCAN_ROUND
    return texts


def test_a_corpus_whose_scan_takes_a_second_round(large):
    hx, ref, data, want = build_and_check(large, queries=["w1 w2", "w399"])
    assert hx.text_sizes()["n_instances"] == 300 * 1800


def test_a_build_with_fallback_documents_is_uploaded():
    texts = ["plain text", "café au lait", "text again", "", "naïve text"]
    build_and_check(texts, queries=["text", "lait"], fallback=[1, 4])


# ---- merge from the handle ---------------------------------------------------------------------------------------------------
def update_and_check(hx, ref, spec, a, texts, new_texts=(), delete=(), replace=None, renumber=True, tokenizer="unicode61", queries=()):
    """A resident update of hx (which holds `texts`) against SQLite on the resulting rows and against
    np_hip_text_build_merge on the fetched base."""
    base = hx.get_text()
    by_host = base.updated(new_texts, delete=delete, replace=replace, renumber=renumber)
    old = hx.text
    got = hx.update_text(new_texts, delete=delete, replace=replace, renumber=renumber, resident=True)
    rows = rows_after(texts, new_texts, delete, replace, renumber)
    want = equal_to_rows(hx, ref, spec, a, rows, tokenizer, queries)
    if got is not None:
        _same(hx.get_text(), by_host)
        rep = got.build_report
        assert rep["n_base_instances"] == base.inst_doc.size and rep["n_instances"] == want.inst_doc.size
        assert rep["delta_uploaded"] == (0 if (list(new_texts) or replace) else 1)
        assert old is not got
    return got, rows


BASE = ["b c", "a b", "", "c c d", "b", "d a", "", "c"]


def fresh(texts, n_docs, tokenizer="unicode61", host=None):
    spec, a, hx, ref = pair(n_docs)
    if host is None:
        hx.build_text(texts, tokenizer, resident=True)
    else:
        hx.set_text(host)
    return spec, a, hx, ref


@pytest.mark.parametrize("renumber", [True, False])
def test_identity_empties_delete_replace_append(renumber):
    N = 12   # the handle's documents: room for the appended rows
    for kw in (dict(),                                                                   # identity
               dict(new_texts=[]),                                                       # empty batch
               dict(delete=[0, 3]), dict(delete=[7]), dict(delete=range(len(BASE))),     # delete; everything
               dict(replace={3: "a z", 0: "c"}), dict(replace={1: ""}),                  # replace
               dict(new_texts=["a e", "", "c"]),                                         # append
               dict(new_texts=["0 zz"], delete=[1, 5], replace={4: "b b q"})):           # all of them
        spec, a, hx, ref = fresh(BASE, N)
        got, rows = update_and_check(hx, ref, spec, a, BASE, renumber=renumber, queries=["b", "c d", "a"], **kw)
    spec, a, hx, ref = fresh(BASE, N)
    got, rows = update_and_check(hx, ref, spec, a, BASE, delete=range(len(BASE)))        # renumbered: no rows are left, the index goes
    assert got is None and hx.text is None
    # every row that holds a token goes and the two empty rows stay: an index of 2 rows, no term, no instance and no posting
    # -- the empty base of the merges that follow (with every row gone there is no index left to merge from)
    spec, a, hx, ref = fresh(BASE, N)
    wordy = [i for i, t in enumerate(BASE) if t]
    got, rows = update_and_check(hx, ref, spec, a, BASE, delete=wordy, renumber=renumber)
    z = hx.text_sizes()
    assert got.terms == [] and (z["n_terms"], z["n_postings"], z["n_instances"], z["n_rows"]) == (0, 0, 0, 2)
    if renumber:   # (without renumbering the two rows keep the ids 2 and 6: a table with holes, which update_text does not plan)
        got = hx.update_text(resident=True)                                                           # identity on it
        assert got.terms == [] and hx.text_sizes()["n_instances"] == 0 and got.build_report["n_base_instances"] == 0
        got = hx.update_text(["b a", "", "a"], resident=True)                                         # an append to it
        assert got.build_report["n_base_instances"] == 0 and got.build_report["n_base_terms"] == 0 and got.terms == ["a", "b"]
        equal_to_rows(hx, ref, spec, a, {0: "", 1: "", 2: "b a", 3: "", 4: "a"}, queries=["a", "b"])
        got = hx.update_text(delete=[2, 4], resident=True)                                            # ... and back to it
        assert got.terms == [] and hx.text_sizes()["n_rows"] == 3


def test_terms_die_are_reborn_and_arrive():
    texts = ["a m", "m", "m z", "k m", "m"]
    for renumber in (True, False):
        for dead, doc in (("a", 0), ("k", 3), ("z", 2)):        # the first, a middle and the last term of the vocabulary
            spec, a, hx, ref = fresh(texts, 8)
            got, _ = update_and_check(hx, ref, spec, a, texts, delete=[doc], renumber=renumber)
            assert dead not in got.vocab and got.build_report["n_terms_dropped"] == 1
        spec, a, hx, ref = fresh(texts, 8)
        got, _ = update_and_check(hx, ref, spec, a, texts, ["x a", "a"], delete=[0], renumber=renumber)   # dies in A, reborn in B
        assert "a" in got.vocab
        spec, a, hx, ref = fresh(texts, 8)
        got, _ = update_and_check(hx, ref, spec, a, texts, ["0 b zz", "l"], renumber=renumber)   # first, middle and last place
        assert got.terms == ["0", "a", "b", "k", "l", "m", "z", "zz"]


def test_a_host_base_with_empty_terms_in_the_middle_and_at_the_end():
    """np_hip_index_set_text allows terms without instances; a build never makes them."""
    toff, doc, pos, n_docs = X.shapes()["empty_terms_host"]
    terms = [f"t{i}" for i in range(toff.size - 1)]
    host = TextIndexData("unicode61", terms, toff, doc, pos, 2, {t: i for i, t in enumerate(terms)})
    spec, a, hx, ref = fresh(None, 6, host=host)
    back = hx.get_text()
    assert np.array_equal(back.term_offsets, toff) and np.array_equal(back.inst_doc, doc) and np.array_equal(back.inst_pos, pos)
    by_host = host.updated(["t3 t9"], delete=[0], renumber=True)
    # the resident path needs a resident self.text: the same vocabulary over the handle's arrays
    hx.text = T.ResidentTextIndexData("unicode61", terms, 2, hx._text_fetcher())
    got = hx.update_text(["t3 t9"], delete=[0], renumber=True, resident=True)
    ref.set_text(by_host)
    layouts_equal(hx, ref)
    _same(hx.get_text(), by_host)
    assert got.terms == by_host.terms == ["t3", "t5", "t9"]


def _run_corpus():
    n = 2 * CHUNK + 300
    texts = ["m"] * n
    texts[2 * CHUNK - 2] = "m m x m m"      # tf = 4 astride the second chunk edge
    texts[7] = "m zz m"                     # tf = 2
    return texts


def test_removed_documents_at_a_scan_chunk_edge_and_postings_with_tf_above_one():
    texts = _run_corpus()
    n = len(texts)
    spec, a, hx, ref = fresh(texts, n + 4)
    # removed at places 2047, 2048, 2049 of the run; the tf = 4 posting stays, the tf = 2 one goes
    update_and_check(hx, ref, spec, a, texts, ["m new", "q m m"], delete=[CHUNK - 1, CHUNK, CHUNK + 1, 7, n - 1],
                     replace={1000: "m other m"}, queries=["m", "m m"])
    spec, a, hx, ref = fresh(texts, n + 4)
    update_and_check(hx, ref, spec, a, texts, delete=[2 * CHUNK - 2, 3], queries=["m", "zz"])   # the tf = 4 posting goes, tf = 2 stays


def test_two_runs_give_the_same_bytes():
    texts = _run_corpus()
    out = []
    for _ in range(2):
        spec, a, hx, ref = fresh(texts, len(texts) + 4)
        hx.update_text(["m q"], delete=[5, CHUNK], replace={9: "x m"}, resident=True)
        lay, back = hx.get_text_layout(), hx.get_text()
        out.append(tuple(v.tobytes() for v in lay.values()) + (back.term_offsets.tobytes(), back.inst_doc.tobytes(), back.inst_pos.tobytes()))
    assert out[0] == out[1]


# ---- a sequence, and the lazily fetched arrays ---------------------------------------------------------------------------------
def test_a_sequence_of_resident_updates_equals_from_texts_of_the_final_rows():
    spec, a, hx, ref = pair(40)
    rows = [f"w{i % 5} w{i % 3} tail" for i in range(20)]
    first = hx.build_text(rows, resident=True)
    for batch in (["w1 new"], ["", "w9 w9"], ["tail w0 w0"]):
        hx.update_text(batch, resident=True)
        rows = rows + batch
    with pytest.raises(ValueError, match="replaced by a later resident update"):
        first.inst_doc                                   # never fetched, and the handle holds another index now
    hx.update_text(delete=[0, 7, 21], renumber=True, resident=True)
    rows = [t for i, t in enumerate(rows) if i not in (0, 7, 21)]
    kept = hx.text
    assert kept.inst_doc.size == hx.text_sizes()["n_instances"]      # fetched now, and kept
    hx.update_text(replace={2: "w4 other", 5: ""}, resident=True)
    rows[2], rows[5] = "w4 other", ""
    assert kept.inst_doc.size > 0                        # ... through the update that replaced the object
    want = equal_to_rows(hx, ref, spec, a, dict(enumerate(rows)), queries=["w4", "tail w0", "other"])
    _same(hx.text, want)                                 # the lazy arrays of self.text
    q = T.compile_text_query("w4 other", hx.text)
    e = T.compile_text_expr('(w4 OR oth*) NOT "w9 w9"', hx.text)
    assert T.prefix_range("w", hx.text) == T.prefix_range("w", want)
    for x, y in zip(hx.text_search([q], 5) + hx.text_search([e], 5, full_grammar=True),
                    ref.text_search([q], 5) + ref.text_search([e], 5, full_grammar=True)):
        assert x.passage_ids.tobytes() == y.passage_ids.tobytes() and x.scores.tobytes() == y.scores.tobytes()
    with pytest.raises(ValueError, match="base= is refused"):
        hx.update_text(["x"], base=want, resident=True)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _open_build(texts):
    raws = [t.encode() for t in texts]
    off = np.zeros(len(raws) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in raws])
    h, fb, rep = api._text_build_open(api.lib(), np.frombuffer(b"".join(raws), np.uint8), off, api.NP_TOK_UNICODE61, None, 0, 0, 0, 0, 0)
    return h


def test_refusals_name_the_argument_and_leave_the_index_in_place():
    L = api.lib()
    spec, a, hx, ref = fresh(BASE, 12)
    before = hx.get_text_layout()

    def unchanged():
        now = hx.get_text_layout()
        assert all(now[k].tobytes() == before[k].tobytes() for k in before)
        assert hx.text_search(["b"], 3)[0].passage_ids.size > 0

    # a document >= n_docs: the lowest offending instance is named
    texts = ["a"] * 12 + ["a b", "b"]
    h = _open_build(texts)
    want = TextIndexData.from_texts(texts)
    low = int(np.nonzero(want.inst_doc >= 12)[0][0])
    assert X.first_offender(want.term_offsets, want.inst_doc, want.inst_pos, 12) == (low, 1)
    with pytest.raises(ValueError, match="not finalised"):
        api._check(L.np_hip_index_set_text_build(hx._h, h))
    api._check(L.np_hip_text_build_sizes(h, None, None, None, None))
    with pytest.raises(ValueError, match=f"np_hip_index_set_text_build: build: instance {low}: document 12 is outside"):
        api._check(L.np_hip_index_set_text_build(hx._h, h))
    unchanged()
    out = api._text_build_read(L, h)             # a refused build is not consumed: the instance half still answers
    assert np.array_equal(out["inst_doc"], want.inst_doc)
    L.np_hip_text_build_free(h)
    # a consumed build: sizes and vocabulary answer, the instance half and a second install are refused, free works
    other = hip_index(a)
    h = _open_build(BASE)
    api._check(L.np_hip_text_build_sizes(h, None, None, None, None))
    api._check(L.np_hip_index_set_text_build(other._h, h))
    terms, n_rows, n_inst = api._text_build_vocab(L, h)
    assert terms == ["a", "b", "c", "d"] and n_rows == len(BASE) and n_inst == 11
    with pytest.raises(ValueError, match="np_hip_text_build_fetch: term_offsets: the build is consumed"):
        api._text_build_read(L, h)
    with pytest.raises(ValueError, match="build is consumed"):
        api._check(L.np_hip_index_set_text_build(hx._h, h))
    with pytest.raises(ValueError, match="delta is consumed"):
        hb = C.c_void_p()
        ids = np.arange(100, 100 + len(BASE), dtype=np.int64)
        remap = np.arange(len(BASE), dtype=np.int64)
        tb, tbo = np.frombuffer(b"abcd", np.uint8), np.arange(5, dtype=np.int64)
        api._check(L.np_hip_index_text_merge(hx._h, api._ptr(tb), api._ptr(tbo), api._ptr(remap), remap.size, h, api._ptr(ids),
                                             2 * len(BASE), None, C.byref(hb), None))
    L.np_hip_text_build_free(h)
    other.close()
    unchanged()
    # NULL arguments
    with pytest.raises(ValueError, match="index is NULL"):
        api._check(L.np_hip_index_set_text_build(None, None))
    with pytest.raises(ValueError, match="build is NULL"):
        api._check(L.np_hip_index_set_text_build(hx._h, None))
    # a build from another device
    if npa.device_count() > 1:
        raws = np.frombuffer(b"ab", np.uint8)
        h, _, _ = api._text_build_open(L, raws, np.asarray([0, 2], np.int64), api.NP_TOK_UNICODE61, None, 1, 0, 0, 0, 0)
        api._check(L.np_hip_text_build_sizes(h, None, None, None, None))
        with pytest.raises(ValueError, match="build was built on device 1"):
            api._check(L.np_hip_index_set_text_build(hx._h, h))
        L.np_hip_text_build_free(h)
    # a sharded handle
    sh = hip_index(a, shard_rank=0, shard_count=2)
    with pytest.raises(ValueError, match="np_hip_index_set_text_build: index is a shard"):
        sh.build_text(BASE[:6], resident=True)
    sh.set_text_shard(TextIndexData.from_texts(BASE))
    with pytest.raises(ValueError, match="index is a shard"):
        sh.text_sizes()
    sh.text = T.ResidentTextIndexData("unicode61", ["a", "b", "c", "d"], len(BASE), None)
    with pytest.raises(ValueError, match="index is a shard"):
        sh.update_text(["a"], resident=True)
    sh.close()
    # the merge: a handle without a keyword index, a vocabulary of another length
    bare = hip_index(a)
    bare.text = T.ResidentTextIndexData("unicode61", ["a", "b", "c", "d"], len(BASE), None)
    with pytest.raises(ValueError, match="no keyword index"):
        bare.update_text(["a"], resident=True)
    bare.close()
    keep = hx.text
    hx.text = T.ResidentTextIndexData("unicode61", ["a", "b", "c"], len(BASE), None)
    with pytest.raises(ValueError, match="base_term_byte_offsets describes 3 terms, the handle's keyword index holds 4"):
        hx.update_text(["a"], resident=True)
    hx.text = keep
    unchanged()


def test_the_merge_refuses_n_rows_out_too_small_and_a_workspace_one_byte_short():
    """(The install's own "n_rows below the documents that hold a token" is a backstop that no build the library makes can
    meet: np_hip_text_build's n_rows is its document count, and the merges check n_rows_out first, as here.)"""
    L = api.lib()
    spec, a, hx, ref = fresh(BASE, 12)
    # the merge: n_rows_out below the survivors that hold a token plus the batch's
    tb, tbo = np.frombuffer(b"abcd", np.uint8), np.arange(5, dtype=np.int64)
    remap = np.arange(len(BASE), dtype=np.int64)
    remap[0] = -1
    hb = C.c_void_p()
    with pytest.raises(ValueError, match="np_hip_index_text_merge: n_rows_out 4 is below the 5 documents of the result that hold"):
        api._check(L.np_hip_index_text_merge(hx._h, api._ptr(tb), api._ptr(tbo), api._ptr(remap), remap.size, None, None, 4, None,
                                             C.byref(hb), None))
    rep = api.np_text_merge_report()
    api._check(L.np_hip_index_text_merge(hx._h, api._ptr(tb), api._ptr(tbo), api._ptr(remap), remap.size, None, None, 5, None,
                                         C.byref(hb), C.byref(rep)))     # exactly the documents that hold a token: taken
    # a workspace one byte below the planned need: refused before any launch, and the plan's figure is the report's
    need = int(rep.workspace_bytes)
    o = api.np_text_merge_opts(need - 1)
    h2 = C.c_void_p()
    with pytest.raises(MemoryError, match=f"it needs {need}"):
        api._check(L.np_hip_index_text_merge(hx._h, api._ptr(tb), api._ptr(tbo), api._ptr(remap), remap.size, None, None, 5, C.byref(o),
                                             C.byref(h2), None))
    o = api.np_text_merge_opts(need)
    api._check(L.np_hip_index_text_merge(hx._h, api._ptr(tb), api._ptr(tbo), api._ptr(remap), remap.size, None, None, 5, C.byref(o),
                                         C.byref(h2), None))
    L.np_hip_text_build_free(h2)
    # the result with exactly as many rows as documents that hold a token installs
    api._check(L.np_hip_index_set_text_build(hx._h, hb))
    L.np_hip_text_build_free(hb)
    assert hx.text_sizes()["n_rows"] == 5


# ---- accounting ---------------------------------------------------------------------------------------------------------------
def test_device_bytes_grow_by_the_keyword_index_and_return():
    spec, a = arrays(16)
    hx = hip_index(a)
    before = hx.info.device_bytes
    hx.build_text(BASE, resident=True)
    grown = hx.info.device_bytes
    z = hx.text_sizes()
    exact = (z["n_terms"] + 1) * 8 + z["n_postings"] * 16 + 16 * 4      # post_off, post_doc + post_tf + post_first, doc_len
    assert exact + z["n_instances"] * 4 <= grown - before <= exact + 256 * ((z["n_instances"] * 4 + 255) // 256)
    hx.update_text(["a q"], resident=True)
    assert hx.info.device_bytes > before
    hx.set_text(None)
    assert hx.info.device_bytes == before and hx.text is None
    assert api.lib().np_hip_index_set_text_build_bytes(4, 11, 16) > 0
    hx.close()


# ---- beside traffic -----------------------------------------------------------------------------------------------------------
def test_searches_beside_three_resident_updates_see_one_of_the_four_states():
    spec, a, hx, ref = pair(40)
    rows = [f"w{i % 5} w{i % 3} tail" for i in range(20)]
    batches = (["w1 w1 w1"], ["tail w1"], ["w1"])
    states, cur = [], list(rows)
    for b in [None] + list(batches):
        cur = cur + (b or [])
        ref.set_text(TextIndexData.from_texts(cur))
        r = ref.text_search(["w1"], 30)[0]
        states.append((r.passage_ids.tobytes(), r.scores.tobytes()))
    assert len(set(states)) == 4
    hx.build_text(rows, resident=True)
    q = T.TextQuery.from_phrases([[hx.text.vocab["w1"]]])      # the term id of "w1" is the same in all four states
    seen, errors, done = [], [], threading.Event()

    def reader():
        try:
            for _ in range(400):
                r = hx.text_search([q], 30)[0]
                seen.append((r.passage_ids.tobytes(), r.scores.tobytes()))
                if done.is_set():
                    break
        except BaseException as e:   # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    t = threading.Thread(target=reader)
    t.start()
    try:
        for b in batches:
            hx.update_text(b, resident=True)
    finally:
        done.set()
        t.join(60)
    assert not t.is_alive() and not errors, errors
    assert seen and all(s in states for s in seen)
    r = hx.text_search([q], 30)[0]
    assert (r.passage_ids.tobytes(), r.scores.tobytes()) == states[3]


# ---- routing: append and remove on a handle with a resident keyword index, columns and groups ----------------------------------
WORDS = ["amber", "birch", "cedar", "delta", "ember", "fjord", "grove", "heath"]
ROUTE_QUERIES = ["amber", "birch cedar", "lonely", "delta OR heath"]


def _route_texts(n, seed=9):
    rng = np.random.default_rng(seed)
    return [" ".join(WORDS[j] for j in rng.integers(0, len(WORDS), 4)) + (" lonely" if d == 3 else "") for d in range(n)]


def _split(n0, n_new):
    import remove_restate as RR
    whole = make_arrays(num_docs=n0 + n_new, seed=5, num_centroids=64, dim=32, nbits=4, doc_len_min=1, doc_len_max=6)[1]
    base = RR.shrunk_arrays(whole, np.arange(n0, n0 + n_new))
    T0 = int(base["doc_lengths"].sum())
    return whole, base, (whole["doc_lengths"][n0:], whole["codes"][T0:], whole["residuals"][T0:])


def _fresh_equal(hx, arrays_now, texts, cols, groups, spec_queries):
    """hx against a handle freshly opened on the resulting index with the setters of the resulting rows."""
    ref = hip_index(arrays_now)
    try:
        ref.set_columns(cols)
        ref.set_groups(groups)
        ref.set_text(TextIndexData.from_texts(texts))
        layouts_equal(hx, ref)
        _same(hx.get_text(), ref.text)
        for x, y in zip(hx.text_search(ROUTE_QUERIES, 8), ref.text_search(ROUTE_QUERIES, 8)):
            assert x.passage_ids.tobytes() == y.passage_ids.tobytes() and x.scores.tobytes() == y.scores.tobytes()
        for x, y in zip(hx.text_search(ROUTE_QUERIES, 8, filters=[("i >= ?", (5,))] * 4), ref.text_search(ROUTE_QUERIES, 8, filters=[("i >= ?", (5,))] * 4)):
            assert x.passage_ids.tobytes() == y.passage_ids.tobytes() and x.scores.tobytes() == y.scores.tobytes()
        assert np.array_equal(hx.get_column("i")[0], ref.get_column("i")[0]) and np.array_equal(hx.get_groups(), ref.get_groups())
    finally:
        ref.close()


def test_append_and_remove_route_a_resident_keyword_index_through_merge_and_install():
    import append_restate as G
    import remove_restate as RR
    n0, n_new = 60, 9
    whole, base, tail = _split(n0, n_new)
    texts = _route_texts(n0 + n_new)
    col = np.arange(n0 + n_new)
    keys = [int(d % 7) for d in range(n0 + n_new)]
    hx = hip_index(base)
    try:
        hx.set_columns({"i": col[:n0]})
        hx.set_groups(keys[:n0])
        first = hx.build_text(texts[:n0], resident=True)
        # remove: document 3 holds the only "lonely"; the term dies and the survivors are renumbered
        gone = [3, 10, 59]
        assert hx.remove_ids(gone, keep_attachments=True) == 3
        assert hx.text.resident and hx.text is not first and "lonely" not in hx.text.vocab
        left = [t for d, t in enumerate(texts[:n0]) if d not in gone]
        keep = np.ones(n0, bool)
        keep[gone] = False
        shrunk = RR.shrunk_arrays(base, gone)
        _fresh_equal(hx, shrunk, left, {"i": col[:n0][keep]}, [k for d, k in enumerate(keys[:n0]) if keep[d]], None)
        # a refused vector step leaves the old keyword index searchable, and the merge's result is freed
        before = hx.get_text_layout()
        with pytest.raises(ValueError, match="rows.texts is None"):
            hx.append_arrays(*tail, rows=api.AppendRows(columns={"i": col[n0:]}, groups=keys[n0:]))
        bad = (tail[0], tail[1] + 10 ** 6, tail[2])          # codes outside the codec: np_hip_index_append_rows refuses
        kept = hx.text
        with pytest.raises(ValueError, match="np_hip_index_append_rows: codes"):
            hx.append_arrays(*bad, rows=api.AppendRows(columns={"i": col[n0:]}, groups=keys[n0:], texts=texts[n0:]))
        assert hx.text is kept and hx.num_documents() == n0 - 3
        now = hx.get_text_layout()
        assert all(now[k].tobytes() == before[k].tobytes() for k in before)
        assert hx.text_search(["amber"], 5)[0].passage_ids.size > 0
        # append
        ids = hx.append_arrays(*tail, rows=api.AppendRows(columns={"i": col[n0:]}, groups=keys[n0:], texts=texts[n0:]))
        assert ids.tolist() == list(range(n0 - 3, n0 - 3 + n_new)) and hx.text.resident and hx.text is not kept
        _fresh_equal(hx, G.grown_arrays(shrunk, tail), left + texts[n0:], {"i": np.concatenate([col[:n0][keep], col[n0:]])},
                     [k for d, k in enumerate(keys[:n0]) if keep[d]] + keys[n0:], None)
        # a remove of nothing keeps the object and the index
        kept = hx.text
        assert hx.remove_ids([10 ** 6], keep_attachments=True) == 0 and hx.text is kept
        # with a host keyword index the same calls do what they did: the result is a plain TextIndexData
        hx.set_text(TextIndexData.from_texts(left + texts[n0:]))
        assert hx.remove_ids([0], keep_attachments=True) == 1 and not hx.text.resident
    finally:
        hx.close()


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_gives_the_same_layout(tmp_path):
    """tests/cpp/text_resident.cpp: next_plaid.hpp's build_text_resident, update_text_resident (alone, and around a keeping
    remove) and the read-back, against the host path on the resulting rows."""
    import os
    import subprocess
    from helpers import ROOT
    spec, a = make_arrays(num_docs=70, seed=5, num_centroids=64, dim=32, nbits=4, doc_len_min=1, doc_len_max=6)
    cut, wts = synth.bucket_tables(spec)
    d = tmp_path / "ix"
    npa.write_index_dir(str(d), a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3)
    exe = tmp_path / "text_resident"
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "text_resident.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    n = 60
    r = subprocess.run([str(exe), str(d), str(n)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "done", r.stdout + r.stderr
    out = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] if " " in ln else "" for ln in r.stdout.splitlines()}
    rows = [f"w{i % 5} w{i % 3}" + (" tail" if i % 4 else "") for i in range(n)] + ["w1 fresh", "", "tail w9 w9"]
    rows = [t for i, t in enumerate(rows) if i not in (0, 7)]
    want = TextIndexData.from_texts(rows)
    assert out["removed"] == f"2 rows {len(rows)} docs 68" and out["refused"] == "1"
    assert out["terms"].split() == want.terms
    ref = npa.MmapIndex.load(str(d))
    try:
        ref.remove_ids([0, 7])
        ref.set_text(want)
        lay = ref.get_text_layout()
        for k in ("post_off", "post_doc", "post_tf", "post_first", "doc_len"):
            assert out[k].split() == [str(int(v)) for v in lay[k]], k
        for k in ("term_offsets", "inst_doc", "inst_pos"):
            assert out[k].split() == [str(int(v)) for v in getattr(want, k)], k
    finally:
        ref.close()


def test_expand_routes_a_resident_keyword_index_through_merge_and_install():
    """expand_arrays(rows=) -- what update_resident calls in expansion mode -- with new centroids, a replaced tail, columns
    and groups: the replaced documents keep their text, the rows given cover the new documents only."""
    n0, n_replace, n_given = 130, 33, 45
    base = make_arrays(num_docs=n0, num_centroids=64, dim=32, nbits=4, doc_len_min=4, doc_len_max=40, seed=5)[1]
    rng = np.random.default_rng(21)
    cen = rng.standard_normal((6, 32)).astype(np.float32)
    new_cen = np.ascontiguousarray(cen / np.linalg.norm(cen, axis=1, keepdims=True), np.float32)
    lens = rng.integers(4, 41, n_given).astype(np.int64)
    Tg = int(lens.sum())
    given = (lens, rng.integers(0, 70, Tg).astype(np.int64), rng.integers(0, 256, (Tg, 16)).astype(np.uint8))
    n_new = n_given - n_replace
    n_keep = n0 - n_replace
    t_keep = int(base["doc_lengths"][:n_keep].sum())
    codes = np.concatenate([base["codes"][:t_keep], given[1]])
    all_lens = np.concatenate([base["doc_lengths"][:n_keep], lens])
    all_cen = np.ascontiguousarray(np.concatenate([base["centroids"], new_cen]))
    ivf, il = synth.build_ivf(codes, all_lens, all_cen.shape[0])
    final = dict(base, centroids=all_cen, doc_lengths=all_lens, codes=codes,
                 residuals=np.concatenate([base["residuals"][:t_keep], given[2]]), ivf=ivf, ivf_lengths=il)
    texts = _route_texts(n0 + n_new)
    col = np.arange(n0 + n_new)
    keys = [int(d % 7) for d in range(n0 + n_new)]
    hx = hip_index(base)
    try:
        hx.set_columns({"i": col[:n0]})
        hx.set_groups(keys[:n0])
        first = hx.build_text(texts[:n0], resident=True)
        before = hx.get_text_layout()
        # a refused vector step (codes outside the grown codec) leaves the old keyword index in place and searchable
        bad = (given[0], given[1] + 10 ** 6, given[2])
        with pytest.raises(ValueError, match="np_hip_index_expand"):
            hx.expand_arrays(new_cen, *bad, n_replace=n_replace, rows=api.AppendRows(columns={"i": col[n0:]}, groups=keys[n0:], texts=texts[n0:]))
        now = hx.get_text_layout()
        assert hx.text is first and hx.num_documents() == n0 and all(now[k].tobytes() == before[k].tobytes() for k in before)
        assert hx.text_search(["amber"], 5)[0].passage_ids.size > 0
        ids = hx.expand_arrays(new_cen, *given, n_replace=n_replace, rows=api.AppendRows(columns={"i": col[n0:]}, groups=keys[n0:], texts=texts[n0:]))
        assert ids.tolist() == list(range(n_keep, n_keep + n_given)) and hx.num_documents() == n0 + n_new
        assert hx.text.resident and hx.text is not first and hx.text.n_rows == n0 + n_new
        _fresh_equal(hx, final, texts, {"i": col}, keys, None)
    finally:
        hx.close()


def test_append_update_resident_and_remove_on_a_directory_keep_the_resident_keyword_index(tmp_path):
    """The three calls the routing is for, on a handle of a written directory with a column, groups and a resident keyword
    index: update_resident in buffer mode (append_arrays) and in expansion mode (expand_arrays: the buffered documents are
    re-indexed and keep their rows), remove(keep_attachments=True) and append(rows=).  The handle then equals load() of the
    directory with the setters of the resulting rows."""
    spec, a = make_arrays(num_docs=600, num_centroids=256, dim=64, nbits=4, doc_len_min=1, doc_len_max=24, seed=3)
    cut, wts = synth.bucket_tables(spec)
    d = str(tmp_path / "a")
    npa.write_index_dir(d, a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=500)
    cfg = npa.UpdateConfig(start_from_scratch=-1, buffer_size=5, kmeans_niters=3, max_points_per_centroid=16, seed=11)
    rng = np.random.default_rng(2)

    def far_docs(n):
        docs = []
        for _ in range(n):
            x = rng.standard_normal((int(rng.integers(2, 12)), 64)).astype(np.float32)
            docs.append(np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), np.float32))
        return docs

    texts = _route_texts(600)
    col, keys = list(range(600)), [int(i % 7) for i in range(600)]

    def rows_of(n, tag):
        t = [f"{WORDS[i % 8]} {tag} fresh{i}" for i in range(n)]
        return api.AppendRows(columns={"i": np.arange(1000, 1000 + n)}, groups=[int(i % 5) for i in range(n)], texts=t), t

    hx = npa.MmapIndex.load(d)
    try:
        hx.set_columns({"i": np.asarray(col)})
        hx.set_groups(keys)
        hx.build_text(texts, resident=True)
        seen = [hx.text]
        for n, mode, tag in ((3, "buffer", "buffered"), (4, "expansion", "expanded")):
            rows, t = rows_of(n, tag)
            ids = hx.update_resident(far_docs(n), cfg, rows=rows)
            assert hx.last_update["mode"] == mode and ids.size == n
            texts, col, keys = texts + t, col + list(range(1000, 1000 + n)), keys + [int(i % 5) for i in range(n)]
            assert hx.text.resident and hx.text not in seen and hx.text.n_rows == len(texts) == hx.num_documents()
            seen.append(hx.text)
        assert hx.last_update["n_reindexed"] == 3
        gone = [3, 10, 601, 606]                      # document 3 holds the only "lonely"
        assert hx.remove(gone, keep_attachments=True) == 4
        texts, col, keys = ([x for i, x in enumerate(v) if i not in gone] for v in (texts, col, keys))
        assert hx.text.resident and hx.text not in seen and "lonely" not in hx.text.vocab
        rows, t = rows_of(2, "appended")
        ids = hx.append(far_docs(2), cfg, rows=rows)
        texts, col, keys = texts + t, col + [1000, 1001], keys + [0, 1]
        assert ids.size == 2 and hx.text.resident and hx.num_documents() == len(texts) == 605
        ref = npa.MmapIndex.load(d)
        try:
            ref.set_columns({"i": np.asarray(col)})
            ref.set_groups(keys)
            ref.set_text(TextIndexData.from_texts(texts))
            layouts_equal(hx, ref)
            _same(hx.get_text(), ref.text)
            qs = ROUTE_QUERIES + ["buffered", "expanded OR appended", "fresh1"]
            for kw in (dict(), dict(filters=[("i >= ?", (1000,))] * len(qs))):
                for x, y in zip(hx.text_search(qs, 8, **kw), ref.text_search(qs, 8, **kw)):
                    assert x.passage_ids.tobytes() == y.passage_ids.tobytes() and x.scores.tobytes() == y.scores.tobytes()
            assert np.array_equal(hx.get_column("i")[0], ref.get_column("i")[0]) and np.array_equal(hx.get_groups(), ref.get_groups())
        finally:
            ref.close()
    finally:
        hx.close()
