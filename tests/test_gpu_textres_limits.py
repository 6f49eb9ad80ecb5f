"""The resident keyword index (np_textres.hip, the resident branch of np_textmerge.hip) at the edges of its own kernels: the
device check's reduction, the two counts over the handle's documents, the scans sized by the documents, and the read-back.
The cases and their censuses are tests/textres_limit_shapes.py's; tests/test_textres_limits_cpu.py asserts the censuses and
that the planted defects of tests/textres_restate.py are rejected by them.  Every comparison is exact, bytes and dtypes:

  an accepted install   get_text_layout byte-equal to a second handle given set_text(from_texts(rows)), get_text equal to
                        from_texts, both equal to textres_restate.layout, text_search / search_hybrid the same bytes
  a refused install     the instance and document that set_text names on the reference handle and that
                        textres_restate.first_offender names; the layout unchanged; the build's instance half still fetches
  an accepted merge     the fetched result array-equal to np_hip_text_build_merge on the fetched base, same arguments
  a refused merge       the count in the message is the restatement's

Only rule 1 (a document outside [0, n_docs)) can be reached on a device: np_hip_text_build_add and the merges check positions
and order on the host before any build is finalised, so rules 2 and 3 are held at block edges on the restatement alone
(tests/test_textres_limits_cpu.py).  A refused install is an ordinary error return: the kernel compares the offending document
and never indexes with it, and the call returns before the postings are written.

  limit                                                             test                                      reached when
  tr_check_heads: a block's lowest, the host's minimum over blocks   C1 offender_at_chunk_and_thread_edges     low = 2047, 2048, 2049, 2055, 2056; block 0 clean
  name_offender's `first` branch: one instance fetched, not two      C2 offender_first_of_its_term_...         low = 2048 = term_offsets[2]
  the check on an uploaded build (fallback documents)                C3 offender_in_an_uploaded_build          fallback_docs = [5, 100], low = 2048
  flags, ranks, block sums sized by max(n_inst, n_docs) + 1          N1 documents_far_beyond_the_instances     n_docs - n_inst >= 2042, blocks(n_docs) = 1, 1, 2, 3
  textres_count_docs with remap, survivors at a chunk edge           N2 survivors_counted_at_a_chunk_edge      remap[2047 | 2048 | 2049] = -1, n_rows_out < survivors + batch
  the host loop over the batch's documents, empty rows               N2                                        batch rows 1 and 3 hold no token; a batch of none; no batch
  textres_count_docs on doc_len + n_told, unaligned                  N3 documents_behind_n_remap               n_told = 2049, 2047, 1 (n_told % 4 != 0), 4096, 0
  its refusal, the count spanning the chunks                         N3                                        k = 1, 2, 4; blocks(n_docs - n_told) = 2, 2, 3
  tr_expand_toff, n_post == 0 for every term                         W1 a_base_without_any_posting             n_terms = 2, n_postings = 0
  the read-back entries with one pointer given                       W2 each_pointer_alone                     3 + 5 calls, sizes with none
  IndexRead beside HoldContexts: read-backs and merges               P1 read_backs_and_merges_beside_installs  3 threads, 3 installs, 4 states of equal sizes
  device_bytes after a dropping install, after an upload             A1 device_bytes                           the figure before any keyword index
  a handle of no document                                            E1 a_handle_emptied_by_remove             n_docs = 0

Not here: L1, a handle of 256 * 2048 + 3 * 2048 + 7 = 530 439 documents whose two document scans take a second round of block
sums (sparse_corpus installed and merged once at the distinct count).  It passed, twice, but took 1.01 s and 1.26 s beside the
0.34 s and 0.33 s of tests/test_gpu_text_resident.py::test_a_corpus_whose_scan_takes_a_second_round in the same runs: 2.97 and
3.8 times, not reliably under the three times that were its condition -- nearly all of it SQLite's index of the 530 439 rows.
"""
import ctypes as C
import re
import threading

import numpy as np
import pytest

from helpers import hip_index

from next_plaid_amd import api
from next_plaid_amd import text as T
from next_plaid_amd.text import TextIndexData

import textres_limit_shapes as S
import textres_restate as X
from test_gpu_text_resident import arrays,equal_to_rows, layouts_equal, searches_equal, update_and_check
from textbuild_limit_shapes import assert_same as _same

pytestmark = pytest.mark.gpu

CHUNK = X.CHUNK
LAYOUT = ("post_off", "post_doc", "post_tf", "post_first", "doc_len")

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
    """(spec, arrays, the handle under test, the reference handle) of n_docs documents, shared by this module's tests."""
    if n_docs not in _PAIRS:
        spec, a = arrays(n_docs)
        _PAIRS[n_docs] = (spec, a, hip_index(a), hip_index(a))
    return _PAIRS[n_docs]


def raw_of(texts):
    """(bytes u8, offsets i64) of a batch as the build entries take it; (None, None) without a batch."""
    if texts is None:
        return None, None
    raws = [t.encode() for t in texts]
    off = np.zeros(len(raws) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in raws])
    return np.frombuffer(b"".join(raws), np.uint8), off


def resident_merge(hx, call, n_rows_out=None):
    """np_hip_index_text_merge on hx's keyword index with the call's remap and batch: the fetched result."""
    raw, off = raw_of(call["batch"])
    L = api.lib()
    h, rep, fb = api.text_merge_resident(hx._h, [t.encode() for t in hx.text.terms], call["remap"], call["delta_ids"],
                                         call["n_rows_out"] if n_rows_out is None else n_rows_out, raw, off, api.NP_TOK_UNICODE61)
    try:
        assert fb.size == 0
        return api._text_build_read(L, h), rep
    finally:
        L.np_hip_text_build_free(h)


def host_merge(base, call, n_rows_out=None):
    """np_hip_text_build_merge on the fetched base with the same arguments."""
    raw, off = raw_of(call["batch"])
    return api.text_merge([t.encode() for t in base.terms], base.term_offsets, base.inst_doc, base.inst_pos, base.n_rows, call["remap"],
                          call["delta_ids"], call["n_rows_out"] if n_rows_out is None else n_rows_out, raw, off, api.NP_TOK_UNICODE61)


def merges_equal(got, want):
    for k in ("term_bytes", "term_byte_offsets", "term_offsets", "inst_doc", "inst_pos"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert got["n_rows"] == want["n_rows"]


def layout_bytes(hx):
    lay = hx.get_text_layout()
    return tuple(lay[k].tobytes() for k in LAYOUT)


# ---- C: the check --------------------------------------------------------------------------------------------------------------
def refused_alike(hx, ref, rows, census, fallback=()):
    """The install of `rows` on hx is refused as set_text refuses SQLite's index of them on ref, and as the restatement says;
    hx's index is untouched and the build not consumed.  Returns the build, finalised, for the caller to free."""
    L = api.lib()
    want, low, doc = census["want"], census["low"], census["doc"]
    n_docs = hx.num_documents()
    assert ref.num_documents() == n_docs
    assert X.first_offender(want.term_offsets, want.inst_doc, want.inst_pos, n_docs) == (low, 1)
    assert X.reduced_offender(want.term_offsets, want.inst_doc, want.inst_pos, n_docs) == (low, 1)
    with pytest.raises(ValueError, match=f"set_text: instance {low}: document {doc} is outside the index"):
        ref.set_text(want)
    before = layout_bytes(hx)
    texts = [T.prepare_document_text(t, "unicode61") for t in rows]

    def tokenize_fallback(ids):
        return T._tokenize_rows(TextIndexData, [rows[int(i)] for i in ids], [int(i) for i in ids], "unicode61")

    raw, off = raw_of(texts)
    h, fb, rep = api._text_build_open(L, raw, off, api.NP_TOK_UNICODE61, tokenize_fallback if fallback else None, 0, 0, 0, 0, 0)
    try:
        assert fb.tolist() == list(fallback)
        api._check(L.np_hip_text_build_sizes(h, None, None, None, None))
        with pytest.raises(ValueError, match=f"np_hip_index_set_text_build: build: instance {low}: document {doc} is outside the index"):
            api._check(L.np_hip_index_set_text_build(hx._h, h))
        assert layout_bytes(hx) == before
        out = api._text_build_read(L, h)                     # not consumed: the instance half still answers
        assert np.array_equal(out["term_offsets"], want.term_offsets) and np.array_equal(out["inst_doc"], want.inst_doc)
        assert np.array_equal(out["inst_pos"], want.inst_pos)
    except BaseException:
        L.np_hip_text_build_free(h)
        raise
    return h


@pytest.fixture(scope="module")
def checked():
    """The pair of N_CHECK documents with a small resident index that every refusal must leave in place."""
    spec, a, hx, ref = pair(S.N_CHECK)
    hx.build_text(["kept b", "b", "", "kept"], resident=True)
    return hx, ref


@pytest.mark.parametrize("s", S.C1_LEADS)
def test_offender_at_chunk_and_thread_edges(checked, s):
    hx, ref = checked
    rows = S.offender_rows(s)
    census = S.check_census(rows, S.N_CHECK)
    assert census["low"] == s + S.N_CHECK == {7: 2047, 8: 2048, 9: 2049, 15: 2055, 16: 2056}[s]
    assert census["low"] // CHUNK == (0 if s == 7 else 1) and census["offending_blocks"] == ([0, 1, 2] if s == 7 else [1, 2])
    assert census["low"] % 8 == {7: 7, 8: 0, 9: 1, 15: 7, 16: 0}[s] and not census["first_of_term"]
    api.lib().np_hip_text_build_free(refused_alike(hx, ref, rows, census))
    assert sorted(hx.text_search(["kept"], 3)[0].passage_ids.tolist()) == [0, 3]


def test_offender_first_of_its_term_at_a_block_start(checked):
    hx, ref = checked
    rows = S.first_of_term_rows()
    census = S.check_census(rows, S.N_CHECK)
    assert census["low"] == CHUNK == census["want"].term_offsets[2] and census["first_of_term"] and census["offending_blocks"] == [1]
    api.lib().np_hip_text_build_free(refused_alike(hx, ref, rows, census))


def _index_bytes(hx):
    z = hx.text_sizes()
    return (z["n_terms"] + 1) * 8 + z["n_postings"] * 16 + z["n_docs"] * 4, z["n_instances"]


def test_offender_in_an_uploaded_build_which_a_larger_handle_takes(checked):
    hx, ref = checked
    L = api.lib()
    rows = S.uploaded_rows()
    census = S.check_census(rows, S.N_CHECK)
    assert census["low"] == CHUNK and census["low"] // CHUNK == 1 and S.UPLOADED_FALLBACK == [5, 100]
    h = refused_alike(hx, ref, rows, census, fallback=S.UPLOADED_FALLBACK)
    try:
        spec, a, big, big_ref = pair(S.N_UPLOADED)
        big.set_text(None)
        before = big.info.device_bytes
        api._check(L.np_hip_index_set_text_build(big._h, h))        # the same build, on a handle of enough documents
        terms, n_rows, n_inst = api._text_build_vocab(L, h)
    finally:
        L.np_hip_text_build_free(h)
    want = census["want"]
    assert terms == want.terms and n_rows == S.N_UPLOADED and n_inst == want.inst_doc.size
    big.text = T.ResidentTextIndexData("unicode61", terms, n_rows, big._text_fetcher())
    equal_to_rows(big, big_ref, spec, a, dict(enumerate(rows)), queries=["m", "a m", "zoe"])
    # A1, the uploaded route: the handle grew by the index -- its arrays exactly, the positions up to their rounding
    api._check(L.np_hip_index_info(big._h, C.byref(big._info)))
    exact, n = _index_bytes(big)
    assert exact + n * 4 <= big.info.device_bytes - before <= exact + 256 * ((n * 4 + 255) // 256)
    big.set_text(None)
    assert big.info.device_bytes == before


# ---- N: counts over the documents ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_docs", S.N_FAR)
def test_documents_far_beyond_the_instances(n_docs):
    spec, a, hx, ref = pair(n_docs)
    rows = S.far_rows(n_docs)
    hx.build_text(rows, resident=True)
    z = hx.text_sizes()
    assert z["n_docs"] == n_docs and z["n_instances"] == len(S.far_holders(n_docs)) and n_docs - z["n_instances"] >= 2042
    assert X.blocks(z["n_instances"]) == 1 and X.blocks(n_docs) == {2047: 1, 2048: 1, 2049: 2, 4097: 3}[n_docs]
    equal_to_rows(hx, ref, spec, a, dict(enumerate(rows)), queries=["w", "w w"])
    gone = min(CHUNK - 1, n_docs - 1)                                  # a holder at the chunk edge (the last one at 2047)
    got, now = update_and_check(hx, ref, spec, a, rows, delete=[gone], renumber=False, queries=["w"])
    assert hx.text_sizes()["n_instances"] == z["n_instances"] - 1
    hx.build_text(rows, resident=True)
    update_and_check(hx, ref, spec, a, rows, new_texts=[], queries=["w"])   # appends nothing


@pytest.fixture(scope="module")
def counted():
    return pair(S.N_COUNT)


@pytest.mark.parametrize("name", list(S.survivor_calls()))
def test_survivors_counted_at_a_chunk_edge(counted, name):
    spec, a, hx, ref = counted
    call = S.survivor_calls()[name]
    hx.build_text(S.holder_rows(S.N_COUNT, call["holders"]), resident=True)
    assert np.array_equal(hx.get_text_layout()["doc_len"], call["doc_len"])
    Y = call["distinct"]
    assert call["n_rows_out"] == Y < call["n_survivors"] + call["n_delta_docs"] and X.blocks(call["n_told"]) == 3
    base = hx.get_text()
    got, rep = resident_merge(hx, call)
    merges_equal(got, host_merge(base, call))
    assert got["n_rows"] == Y and rep["n_base_instances"] == 5
    with pytest.raises(ValueError, match=f"np_hip_index_text_merge: n_rows_out {Y - 1} is below the {Y} documents of the result that hold a token"):
        resident_merge(hx, call, Y - 1)
    with pytest.raises(ValueError, match=f"n_rows_out {Y - 1} is below the {Y} documents of the result that hold a token"):
        host_merge(base, call, Y - 1)


@pytest.mark.parametrize("n_remap", S.N_REMAPS)
def test_documents_behind_n_remap(counted, n_remap):
    spec, a, hx, ref = counted
    ok, refused = S.behind_calls()[n_remap]
    hx.build_text(S.holder_rows(S.N_COUNT, ok["holders"]), resident=True)
    assert np.array_equal(hx.get_text_layout()["doc_len"], ok["doc_len"])
    assert ok["n_told"] == n_remap == ok["remap"].size and ok["beyond"] == 0 and ok["n_rows_out"] == len(ok["holders"]) + 2
    got, rep = resident_merge(hx, ok)
    merges_equal(got, host_merge(hx.get_text(), ok))
    assert got["n_rows"] == ok["distinct"] and got["inst_doc"].size == len(ok["holders"]) + 3
    assert [c["beyond"] for c in refused] == {4097: [], 4096: [1], 2049: [1, 2], 2047: [1, 4], 1: [1, 4], 0: [1, 4]}[n_remap]
    for call in refused:
        hx.build_text(S.holder_rows(S.N_COUNT, call["holders"]), resident=True)
        before = layout_bytes(hx)
        k = call["beyond"]
        assert k == X.beyond(hx.get_text_layout()["doc_len"], n_remap) > 0
        with pytest.raises(ValueError, match=f"np_hip_index_text_merge: base: {k} documents of the handle's keyword index hold a token and "
                                             f"lie outside the index \\(the index is n_remap = {n_remap} old documents\\)"):
            resident_merge(hx, call)
        with pytest.raises(ValueError, match=f"base: instance \\d+: document {n_remap} is outside the index \\(the index is n_remap = {n_remap} old"):
            host_merge(hx.get_text(), call)                          # the host merge refuses the same base, naming an instance
        assert layout_bytes(hx) == before


# ---- W: the read-back ---------------------------------------------------------------------------------------------------------
def test_a_base_without_any_posting():
    host = S.host_data("only_empty_terms_host", 2)
    spec, a, hx, ref = pair(8)
    hx.set_text(host)
    z = hx.text_sizes()
    assert (z["n_terms"], z["n_postings"], z["n_instances"], z["n_rows"]) == (2, 0, 0, 2)
    back = hx.get_text()
    _same(back, host)
    assert back.term_offsets.tolist() == [0, 0, 0]
    new = ["t001 t9", "t000"]
    by_host = host.updated(new, renumber=True)
    hx.text = T.ResidentTextIndexData("unicode61", list(host.terms), 2, hx._text_fetcher())
    got = hx.update_text(new, renumber=True, resident=True)
    ref.set_text(by_host)
    layouts_equal(hx, ref)
    _same(hx.get_text(), by_host)
    assert got.terms == by_host.terms == ["t000", "t001", "t9"] and got.build_report["n_base_instances"] == 0
    searches_equal(hx, ref, spec, a, ["t9", "t000"])


def test_each_pointer_alone():
    L = api.lib()
    spec, a, hx, ref = pair(64)
    hx.set_text(S.host_data("random", 64))
    api._check(L.np_hip_index_text_sizes(hx._h, None, None, None, None, None))
    z = hx.text_sizes()
    full = hx.get_text_layout()
    toff, doc, pos = hx._fetch_text_arrays()
    table = dict(term_offsets=toff, inst_doc=doc, inst_pos=pos)
    assert z["n_postings"] > 0 and z["n_instances"] > z["n_postings"] and np.array_equal(toff, S.host_data("random", 64).term_offsets)
    for i, k in enumerate(("term_offsets", "inst_doc", "inst_pos")):
        out = np.full_like(table[k], -7)
        args = [None, None, None]
        args[i] = api._ptr(out)
        api._check(L.np_hip_index_get_text(hx._h, *args))
        assert out.dtype == table[k].dtype and np.array_equal(out, table[k]), k
    for i, k in enumerate(LAYOUT):
        out = np.full_like(full[k], -7)
        args = [None] * 5
        args[i] = api._ptr(out)
        api._check(L.np_hip_index_get_text_layout(hx._h, *args))
        assert out.dtype == full[k].dtype and np.array_equal(out, full[k]), k
    api._check(L.np_hip_index_get_text(hx._h, None, None, None))
    api._check(L.np_hip_index_get_text_layout(hx._h, None, None, None, None, None))


# ---- P: readers beside installs ------------------------------------------------------------------------------------------------
def test_read_backs_and_merges_beside_installs():
    L = api.lib()
    spec, a, hx, ref = pair(S.STATE_DOCS)
    rows, steps = S.states()
    keys = [S.state_keys(r) for r in rows]
    layouts, tables = [k[0] for k in keys], [k[1] for k in keys]
    assert len(set(layouts)) == 4 and len(set(tables)) == 4
    hx.build_text(rows[0], resident=True)
    assert layout_bytes(hx) == layouts[0]
    terms = [t.encode() for t in hx.text.terms]
    term_bytes = b"".join(terms)
    ident = np.arange(len(rows[0]), dtype=np.int64)
    seen = {"layout": [], "table": [], "merge": []}
    errors, done = [], threading.Event()

    def read_layout():
        seen["layout"].append(layout_bytes(hx))

    def read_table():
        d = hx.get_text()
        seen["table"].append((d.term_offsets.tobytes(), d.inst_doc.tobytes(), d.inst_pos.tobytes()))

    def read_merge():
        h, _, _ = api.text_merge_resident(hx._h, terms, ident, np.zeros(0, np.int64), ident.size)
        try:
            out = api._text_build_read(L, h)
        finally:
            L.np_hip_text_build_free(h)
        assert out["term_bytes"].tobytes() == term_bytes and out["n_rows"] == ident.size
        seen["merge"].append((out["term_offsets"].tobytes(), out["inst_doc"].tobytes(), out["inst_pos"].tobytes()))

    def loop(step):
        try:
            for _ in range(300):
                step()
                if done.is_set():
                    break
        except BaseException as e:   # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=loop, args=(f,)) for f in (read_layout, read_table, read_merge)]
    for t in threads:
        t.start()
    try:
        for step in steps:
            hx.update_text(replace=step, renumber=False, resident=True)
    finally:
        done.set()
        for t in threads:
            t.join(60)
    assert not any(t.is_alive() for t in threads) and not errors, errors
    assert seen["layout"] and all(s in layouts for s in seen["layout"])        # the five arrays together are one state's
    assert seen["table"] and all(s in tables for s in seen["table"])
    assert seen["merge"] and all(s in tables for s in seen["merge"])
    assert layout_bytes(hx) == layouts[3]
    equal_to_rows(hx, ref, spec, a, dict(enumerate(rows[3])), queries=["w1", "tail v3"])


# ---- A and E: small ones -------------------------------------------------------------------------------------------------------
def test_device_bytes_return_when_an_install_drops_the_index():
    spec, a = arrays(16)
    hx = hip_index(a)
    try:
        before = hx.info.device_bytes
        hx.build_text(["a b", "", "b"], resident=True)
        exact, n = _index_bytes(hx)
        assert exact + n * 4 <= hx.info.device_bytes - before <= exact + 256 * ((n * 4 + 255) // 256)
        assert hx.build_text([], resident=True) is None and hx.text is None          # the build of no row drops the index
        assert hx.info.device_bytes == before
        with pytest.raises(ValueError, match="no keyword index"):
            hx.text_sizes()
    finally:
        hx.close()


def test_a_handle_emptied_by_remove():
    spec, a = arrays(6)
    hx, ref = hip_index(a), hip_index(a)
    try:
        for h in (hx, ref):
            assert h.remove_ids(np.arange(6)) == 6 and h.num_documents() == 0
        assert hx.build_text([], resident=True) is None and hx.text is None
        with pytest.raises(ValueError, match="no keyword index"):
            hx.text_sizes()
        with pytest.raises(ValueError, match="set_text: instance 0: document 0 is outside the index"):
            ref.set_text(TextIndexData.from_texts(["x"]))
        with pytest.raises(ValueError, match="np_hip_index_set_text_build: build: instance 0: document 0 is outside the index"):
            hx.build_text(["x"], resident=True)
        assert hx.text is None
        want = TextIndexData.from_texts([""])                      # a row without a token: whatever set_text does with it
        try:
            ref.set_text(want)
        except ValueError as e:
            with pytest.raises(ValueError, match=re.escape(str(e).split(": ", 1)[-1][:40])):
                hx.build_text([""], resident=True)
        else:
            got = hx.build_text([""], resident=True)
            assert got.n_rows == 1 and got.terms == []
            lay = layouts_equal(hx, ref)
            assert lay["doc_len"].size == 0 and hx.text_sizes() == dict(n_terms=0, n_postings=0, n_instances=0, n_rows=1, n_docs=0)
            _same(hx.get_text(), want)
    finally:
        hx.close()
        ref.close()
