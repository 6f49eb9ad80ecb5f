"""np_hip_text_build and np_hip_text_build_merge at the constants of their own kernels (np_textbuild.hip, np_textmerge.hip and the
scan both share, np_textbuild_dev.h).  Every comparison is exact -- terms, term_offsets, inst_doc, inst_pos, n_rows and dtypes --
against SQLite itself, or, for the two shapes SQLite is too slow for, against the vectorised reference of
tests/textbuild_limit_shapes.py, which tests/test_textbuild_limits_cpu.py pins to SQLite on the same generators.  Pure-ASCII
corpora assert fallback_docs == [].  Every test proves from the report and its own sizes that it reached the path it names.

  limit                                                            test                                reached when
  tb_scan_sums, a second round with a ragged end, int64 out         B1a scan_of_the_document_counts     blocks(n_docs) = 260 > 256
  tb_scan_sums, two full rounds, uint32 out                         B1b flag_scan_of_a_table            2^20 slots / 2048 = 512 blocks
  tb_scan_sums in place over the radix histograms                   B2  histogram_scan                  256 * 2049 sort blocks -> 257
  tb_insert gives up after TB_MAX_PROBES in a table >= 1024 slots   B3  table_full_at_1024_probes       hash_bits 11, 12 < 5000 terms
  tile_lanes 64, 63, 32: the lane 63 -> lane 0 hand-over            B4  full_wave_tiles                 tile_bytes 1024, 1008, 512
  NP_TEXT_BUILD_MAX_TOKEN_BYTES, a token of 32768 and of 32769      B4  token_cap_at_the_abi_maximum    max_token_bytes 32768
  three radix passes for trigram                                    B5  trigram_three_passes            n_terms > 65536
  the planned workspace bounds every W.take                         B6  planned_workspace               N passes, N - 1 does not
  the merge's S scan above one round, removed rows at the edge      M1  merge_run_across_the_round      n_base_instances > 524288
  a merge on a base the device built above one round                M2  merge_on_the_device_built_base  the index of B1a
  build, merge and search from six threads at once                  P1  build_merge_search_in_parallel  bit-equal to the serial run
"""
import re
import threading

import numpy as np
import pytest

from helpers import hip_index, make_arrays

from next_plaid_amd import api, text as T
from next_plaid_amd.text import TextIndexData

import text_expr_restate as TX
import text_restate as TR
import textbuild_limit_shapes as S
from textbuild_limit_shapes import assert_same, blocks, rows_after, sqlite_rows

pytestmark = pytest.mark.gpu

ROUND = S.SCAN_ROUND * S.SCAN_CHUNK      # 524 288 items: what one round of tb_scan_sums covers
N_SPARSE = ROUND + 3 * S.SCAN_CHUNK + 7  # 530 439


def ascii_only(texts, tokenizer="unicode61"):
    return all(ord(c) < 0x80 and not (tokenizer == "trigram" and c == "\x00") for t in texts for c in t)


def check(texts, tokenizer="unicode61", fallback=None, **kw):
    got = TextIndexData.from_texts_device(texts, tokenizer, **kw)
    assert_same(got, TextIndexData.from_texts(texts, tokenizer))
    if fallback is None:
        assert ascii_only(texts, tokenizer)
        fallback = []
    assert got.fallback_docs == list(fallback)
    rep = got.build_report
    assert rep["n_docs"] == len(texts) and rep["n_fallback"] == len(got.fallback_docs)
    return got


# ---- B1: scans above one round -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse():
    """(the texts of B1a, the index the device built of them): M2 goes on from it."""
    texts = S.sparse_corpus(N_SPARSE, ROUND)
    return texts, TextIndexData.from_texts_device(texts)


def test_scan_of_the_document_counts_above_one_round(sparse):
    texts, got = sparse
    assert len(texts) == 530439 and blocks(len(texts)) == 260 > S.SCAN_ROUND       # a second round with four live entries
    assert_same(got, TextIndexData.from_texts(texts))
    rep = got.build_report
    assert got.fallback_docs == [] and rep["n_docs"] == len(texts) and rep["n_fallback"] == 0
    live = sum(1 for t in texts if t)
    assert rep["n_instances"] == 2 * live == got.inst_doc.size and rep["n_terms"] == 6
    assert {ROUND - 1, ROUND, ROUND + 1, len(texts) - 1} <= set(got.inst_doc.tolist())


def test_flag_scan_of_a_table_of_two_rounds():
    texts = S.wide_table_corpus()
    got = check(texts, hash_bits=20)
    rep = got.build_report
    assert rep["hash_bits"] == 20 and rep["table_retries"] == 0
    assert blocks(1 << rep["hash_bits"]) == 512 == 2 * S.SCAN_ROUND and 0 < rep["n_terms"] <= 500


# ---- B2: the histogram scan above one round, in place ------------------------------------------------------------------------
def test_histogram_scan_above_one_round_in_place():
    n_tokens = 2049 * S.SORT_CHUNK - 5
    words, flat, row_off = S.one_long_document(n_tokens)
    raw, off = S.raw_of(words, flat, row_off)
    assert n_tokens == 4196347 and off.tolist() == [0, 3 * n_tokens - 1, 3 * n_tokens - 1 + 8]
    r = api.text_build(raw, off, api.NP_TOK_UNICODE61)
    got = TextIndexData._of_build("unicode61", r)
    rep = got.build_report
    assert got.fallback_docs == [] and rep["n_fallback"] == 0 and rep["n_docs"] == 2
    n_inst = rep["n_instances"]
    assert n_inst == n_tokens + 3 and blocks(n_inst, S.SORT_CHUNK) == 2049
    assert 256 * 2049 == 524544 and blocks(256 * 2049) == 257 > S.SCAN_ROUND       # the scan of the histograms: a second round
    assert rep["n_terms"] == 300 and rep["sort_passes"] == 2
    assert blocks(1 << rep["hash_bits"]) > S.SCAN_ROUND and rep["table_retries"] == 0
    assert_same(got, S.as_data(S.ref_build(words, flat, row_off)))


# ---- B3: a table that is full at 1024 probes ---------------------------------------------------------------------------------
def test_table_full_at_1024_probes_is_grown():
    texts = S.many_terms_corpus(5000)
    assert len(texts) == 200
    got = check(texts, hash_bits=11)
    rep = got.build_report
    assert (1 << 11) - 1 >= S.MAX_PROBES                  # the probe limit is TB_MAX_PROBES, not the table's size
    assert rep["n_terms"] == 5000 == got.n_terms and rep["n_instances"] == 10000
    assert rep["table_retries"] >= 2 and (1 << rep["hash_bits"]) >= rep["n_terms"] and rep["hash_bits"] == 11 + rep["table_retries"]


# ---- B4: full-wave tiles and the token cap -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_bytes", [0, 1008, 512])
def test_tokens_at_and_across_full_wave_tile_edges(tile_bytes):
    tile = tile_bytes or 1024
    texts = S.tile_edge_corpus(tile)
    assert tile // 16 in (64, 63, 32) and max(len(t) for t in texts) > 5 * tile
    got = check(texts, "unicode61", tile_bytes=tile_bytes, max_token_bytes=4096)
    assert got.build_report["tile_bytes"] == tile and "t" * (3 * tile + 1) in got.vocab and "t" * (tile + 5) in got.vocab
    part = texts[::20]
    got = check(part, "trigram", tile_bytes=tile_bytes)
    assert got.build_report["tile_bytes"] == tile and max(len(t) for t in part) > 2 * tile
    assert got.build_report["n_instances"] == sum(max(len(t) - 2, 0) for t in part)


def test_token_cap_at_the_abi_maximum():
    cap = S.MAX_TOKEN
    texts, over = S.token_cap_corpus(cap)
    got = check(texts, "unicode61", fallback=over, max_token_bytes=cap)
    assert cap == 32768 and over == [2, 3, 7, 8]
    assert "x" * cap in got.vocab and "y" * cap in got.vocab and "y" * (cap + 1) not in got.vocab
    # the device's own instances: "x" alone, "a x b", twice, and "ok" twice; the fallback documents' are SQLite's
    assert got.build_report["n_instances"] == 2 * (1 + 3 + 1) and got.build_report["tile_bytes"] == 1024
    with pytest.raises(ValueError, match="max_token_bytes 32769"):
        TextIndexData.from_texts_device(["a"], max_token_bytes=cap + 1)


# ---- B5: trigram, three passes -----------------------------------------------------------------------------------------------
def test_trigram_three_radix_passes():
    texts = S.random_bytes_document(300_000)
    got = check(texts, "trigram")
    rep = got.build_report
    assert rep["n_terms"] > 65536 and rep["sort_passes"] == 3 and rep["n_instances"] == 300_000 - 2 + 1
    assert blocks(rep["n_instances"], S.SORT_CHUNK) > 1 and rep["tile_bytes"] == 1024 < len(texts[0])


# ---- B6: the planned workspace is a true upper bound -------------------------------------------------------------------------
@pytest.mark.parametrize("tokenizer", ["unicode61", "trigram"])
def test_planned_workspace_holds_the_call_and_one_byte_less_does_not(tokenizer):
    texts = S.workspace_corpus() if tokenizer == "unicode61" else S.workspace_corpus(100, 40)
    free = TextIndexData.from_texts_device(texts, tokenizer)
    assert 15000 <= free.build_report["n_instances"] <= 25000 and free.fallback_docs == []
    assert_same(free, TextIndexData.from_texts(texts, tokenizer))
    n_bytes = sum(len(t) for t in texts)
    holds_documents = n_bytes + 24 * (len(texts) + 1) + 4096          # the text, five per-document arrays, the block sums
    with pytest.raises(MemoryError, match="instances need") as refusal:
        TextIndexData.from_texts_device(texts, tokenizer, workspace_bytes=holds_documents)
    need = int(re.search(r"(\d+) instances need (\d+) bytes", str(refusal.value)).group(2))
    assert need > holds_documents + 9 * 4 * free.build_report["n_instances"]
    got = TextIndexData.from_texts_device(texts, tokenizer, workspace_bytes=need)
    assert S.flat_index(got) == S.flat_index(free) and 0 < got.build_report["workspace_bytes"] <= need
    assert got.build_report["hash_bits"] == free.build_report["hash_bits"] and got.build_report["table_retries"] == 0
    with pytest.raises(MemoryError, match=f"instances need {need} bytes"):      # the plan's check: before any instance array
        TextIndexData.from_texts_device(texts, tokenizer, workspace_bytes=need - 1)


# ---- M1: the merge's S above one round ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_bases():
    out = {}
    for lead in (0, 5):
        words, flat, row_off, big = S.run_corpus(ROUND, S.SCAN_CHUNK + 300, lead)
        out[lead] = (words, flat, row_off, big, S.ref_build(words, flat, row_off))
    return out


@pytest.mark.parametrize("lead", [0, 5])
@pytest.mark.parametrize("renumber", [True, False])
def test_merge_run_across_the_round_of_the_scan(run_bases, lead, renumber):
    words, flat, row_off, big, base = run_bases[lead]
    n = row_off.size - 1
    assert n == ROUND + 2048 + 300 and base["inst_doc"].size == n + 3 + lead + 2
    m = base["terms"].index(b"m")
    lo = int(base["term_offsets"][m])
    assert lo == lead and base["inst_doc"][lo + big: lo + big + 4].tolist() == [big] * 4
    assert (lo + big < ROUND < lo + big + 4) == (lead == 0)        # astride the round's edge; the lead shifts it past
    delete, replace, new, (bflat, boff) = S.run_update(base, ROUND, n, big)
    assert {int(d) for d in base["inst_doc"][ROUND - 1: ROUND + 2]} <= set(delete) and (big in delete) == (lead == 0)
    got = S.as_data(base).updated(new, delete=delete, replace=replace, renumber=renumber)
    rep = got.build_report
    assert rep["n_base_instances"] == base["inst_doc"].size > ROUND and blocks(rep["n_base_instances"]) == 258 > S.SCAN_ROUND
    gone = np.isin(base["inst_doc"], delete + sorted(replace))
    assert rep["n_instances_dropped"] == int(gone.sum()) == len(delete) + 3 + (4 if lead == 0 else 0)
    assert rep["n_old_docs"] == n and rep["delta_uploaded"] == 0 and got.fallback_docs == []
    assert rep["n_terms_dropped"] == (1 if lead == 0 else 0)          # "x" goes with the four-instance document
    want = S.ref_update(words, flat, row_off, bflat, boff, len(replace), delete, sorted(replace), renumber)
    assert_same(got, S.as_data(want))
    assert rep["n_instances"] == want["inst_doc"].size and rep["n_rows"] == n - len(delete) + 2


# ---- M2: a base the device built above one round -----------------------------------------------------------------------------
def test_merge_on_the_base_the_device_built_above_one_round(sparse):
    texts, base = sparse
    batch = [f"a b{i % 7} new{i}" if i % 5 else "" for i in range(50)]
    grown = base.updated(batch)
    assert grown.n_rows == len(texts) + 50 and grown.build_report["n_old_docs"] == len(texts) and blocks(grown.n_rows) > S.SCAN_ROUND
    delete = list(range(0, grown.n_rows, 1000))
    got = grown.updated(delete=delete)
    assert got.build_report["n_instances_dropped"] == 2 * sum(1 for d in delete if d % 97 == 0 and d < len(texts)) > 0
    assert got.fallback_docs == [] and grown.fallback_docs == []
    assert_same(got, sqlite_rows(rows_after(texts + batch, delete=delete)))


# ---- P1: build, merge and search from six threads at once --------------------------------------------------------------------
N_THREADS = 6
ROUNDS = 3


def flat_results(rs):
    return tuple((r.query_id, r.passage_ids.tobytes(), r.scores.tobytes()) for r in rs)


def test_build_merge_and_search_in_parallel():
    texts = S.thread_corpus(300)
    tri = [t[:40] for t in S.thread_corpus(200, seed=22)]
    base = TextIndexData.from_texts(texts)
    ascii_batch = S.thread_corpus(40, seed=23)
    mixed_batch = ascii_batch[:20] + ["naïve café wo1", "wo2 über"]
    delete = list(range(0, 300, 7))
    replace = {5: "wo1 replaced", 150: "", 299: "Alpha wo3 wo3"}
    spec, a = make_arrays(num_docs=300, num_centroids=32, dim=32, nbits=2, doc_len_min=4, doc_len_max=8, seed=13)
    hx = hip_index(a)
    try:
        hx.set_text(base)
        # everything that compiles against the vocabulary happens here, before any thread starts
        tq = [T.compile_text_query(s, base) for s in ("wo1 wo2", "wo3 OR wo5 OR wo7", '"wo1 wo0"', "alpha", "nowhere", "beta9 x")]
        trees = [T.compile_text_expr(s, base) for s in ("wo1*", "wo2 NOT wo1*", "(wo3* OR wo5) AND wo0", "nowhere*", "wo* NOT alpha")]
        calls = {
            "build unicode61, a table that retries": lambda: S.flat_index(TextIndexData.from_texts_device(texts, hash_bits=3)),
            "build trigram": lambda: S.flat_index(TextIndexData.from_texts_device(tri, "trigram")),
            "update, ascii batch": lambda: S.flat_index(base.updated(ascii_batch, delete=delete[:9], replace=replace)),
            "update, uploaded batch": lambda: S.flat_index(base.updated(mixed_batch, delete=delete[:3], renumber=False)),
            "update, deletes only": lambda: S.flat_index(base.updated(delete=delete)),
            "text_search": lambda: flat_results(hx.text_search(tq, 10)),
            "text_search trees": lambda: flat_results(hx.text_search(trees, 10)),
        }
        names = list(calls)
        serial = {name: calls[name]() for name in names}
        # the serial run is itself pinned: the builds and updates to SQLite, the searches to their restatements
        got = TextIndexData.from_texts_device(texts, hash_bits=3)
        assert got.build_report["table_retries"] > 0 and got.fallback_docs == []
        assert_same(got, base)
        assert_same(TextIndexData.from_texts_device(tri, "trigram"), TextIndexData.from_texts(tri, "trigram"))
        got = base.updated(ascii_batch, delete=delete[:9], replace=replace)
        assert got.build_report["delta_uploaded"] == 0 and got.fallback_docs == []
        assert_same(got, sqlite_rows(rows_after(texts, ascii_batch, delete[:9], replace)))
        got = base.updated(mixed_batch, delete=delete[:3], renumber=False)
        assert got.build_report["delta_uploaded"] == 1 and got.fallback_docs == [20, 21]
        assert_same(got, sqlite_rows(rows_after(texts, mixed_batch, delete[:3], renumber=False)))
        got = base.updated(delete=delete)
        assert got.build_report["n_delta_docs"] == 0
        assert_same(got, sqlite_rows(rows_after(texts, delete=delete)))
        rs, xs = TR.Restated(base, 300), TX.RestatedExpr(base, 300)
        for qs, search, name in ((tq, rs.search, "text_search"), (trees, xs.expr_search, "text_search trees")):
            res = hx.text_search(qs, 10)
            assert flat_results(res) == serial[name] and sum(r.passage_ids.size for r in res) > 0
            for q, r in zip(qs, res):
                ids, sc = search(q, 10)
                assert np.array_equal(r.passage_ids, ids) and np.array_equal(r.scores.view(np.uint32), sc.view(np.uint32)), name

        out, errs, refused = {}, [], []
        start = threading.Barrier(N_THREADS)

        def work(t):
            try:
                start.wait(timeout=60)
                mine = []
                for r in range(ROUNDS):
                    for j in range(len(names)):
                        name = names[(j + 2 * t + r) % len(names)]           # every thread in another rotation
                        mine.append((name, calls[name]()))
                        if t == 1 and j == 3:                                  # a refusal of its own, amid the others' calls
                            try:
                                TextIndexData.from_texts_device(texts, workspace_bytes=64)
                                refused.append("no refusal")
                            except MemoryError as e:
                                refused.append((str(e), api.last_error()))
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
                assert got == serial[name], f"thread {t}, call {i} ({name}) differs from the serial result"
        assert len(refused) == ROUNDS
        for msg in refused:
            assert msg != "no refusal" and msg[0] == msg[1] and "workspace of 64 bytes" in msg[0], msg
    finally:
        hx.close()
