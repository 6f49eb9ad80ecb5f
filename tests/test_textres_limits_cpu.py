"""tests/textres_limit_shapes.py bites: on the numpy restatement alone (no device) every case of
tests/test_gpu_textres_limits.py reaches the edge it names, the check's reduction restated block by block
(textres_restate.block_offenders, reduced_offender) names the offender that the serial rule names on every shape -- rules 2 and
3, which no device build can meet, at block and thread edges included --, and each planted defect of the reduction and of the
counts is rejected by a named case: the message or the result it leads to differs on that case's own inputs.
"""
import numpy as np
import pytest

from next_plaid_amd.text import TextIndexData

import textres_limit_shapes as S
import textres_restate as X

CHUNK = X.CHUNK

# planted defect -> the case that rejects it
REJECTED_BY = {
    "min_over_the_first_block_only": "C1 offender_at_chunk_and_thread_edges, s = 8",      # block 0 is clean: the install would pass
    "thread_keeps_its_last_offender": "C1 offender_at_chunk_and_thread_edges, s = 8",     # thread 0 of block 1 would say 2055
    "block_start_has_no_predecessor": "rule 3 at a block start (restatement only)",
    "count_ignores_remap": "N2 holder 2047 goes",
    "count_ignores_doc_len": "N2 empty 2049 goes",
    "beyond_counts_from_zero": "N3 n_remap = 2047, one",
    "beyond_skips_its_first_document": "N3 n_remap = 2047, one",
    "batch_documents_counted_per_instance": "N2 holder 2048 goes",
    "batch_empty_rows_counted": "N2 a batch of empty rows",
}


def test_every_new_defect_is_listed():
    assert set(REJECTED_BY) == set(X.CHECK_DEFECTS + X.COUNT_DEFECTS) and set(X.DEFECTS) == set(X.LAYOUT_DEFECTS) | set(REJECTED_BY)


# ---- C: the check --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1():
    return {s: S.check_census(S.offender_rows(s), S.N_CHECK) for s in S.C1_LEADS}


def test_c1_reaches_the_chunk_and_thread_edges(c1):
    assert [c["low"] for c in c1.values()] == [2047, 2048, 2049, 2055, 2056]
    for s, c in c1.items():
        w = c["want"]
        assert w.terms == ["a", "m"] and w.term_offsets.tolist() == [0, s, s + S.N_UPLOADED]
        assert (c["low"], c["rule"], c["doc"]) == (s + S.N_CHECK, 1, S.N_CHECK) and not c["first_of_term"]
        assert X.blocks(w.inst_doc.size) == 3
    # 2047: the last instance of block 0, the eighth of thread 255; from 2048 on block 0 is clean
    assert (c1[7]["block"], c1[7]["thread"], c1[7]["slot"]) == (0, 255, 7) and c1[7]["offending_blocks"] == [0, 1, 2]
    assert (c1[8]["block"], c1[8]["thread"], c1[8]["slot"]) == (1, 0, 0) and c1[8]["offending_blocks"] == [1, 2]
    assert (c1[9]["block"], c1[9]["thread"], c1[9]["slot"]) == (1, 0, 1)
    assert (c1[15]["block"], c1[15]["thread"], c1[15]["slot"]) == (1, 0, 7)          # a thread's eighth instance
    assert (c1[16]["block"], c1[16]["thread"], c1[16]["slot"]) == (1, 1, 0)          # ... and the next thread's first: the ninth
    for s in (8, 9, 15, 16):                                                         # several blocks offend: the lowest is named
        per_block = c1[s]["per_block"]
        assert per_block[0] == X.NO_OFFENDER and per_block[1] == c1[s]["low"] and per_block[2] == 2 * CHUNK


def test_c1_rejects_the_two_reduction_defects(c1):
    for s in (8, 9, 15, 16):
        w = c1[s]["want"]
        args = (w.term_offsets, w.inst_doc, w.inst_pos, S.N_CHECK)
        assert X.reduced_offender(*args) == (s + S.N_CHECK, 1)
        assert X.reduced_offender(*args, defect="min_over_the_first_block_only") is None
    w = c1[8]["want"]
    assert X.reduced_offender(w.term_offsets, w.inst_doc, w.inst_pos, S.N_CHECK, defect="thread_keeps_its_last_offender") == (2055, 1)
    assert REJECTED_BY["thread_keeps_its_last_offender"].endswith("s = 8")


def test_c2_offender_is_the_first_of_its_term_at_a_block_start():
    c = S.check_census(S.first_of_term_rows(), S.N_CHECK)
    w = c["want"]
    assert w.terms == ["a", "m", "z"] and w.term_offsets.tolist() == [0, 8, CHUNK, CHUNK + 1]
    assert (c["low"], c["rule"], c["doc"], c["first_of_term"]) == (CHUNK, 1, S.N_CHECK, True)
    assert (c["block"], c["thread"], c["slot"]) == (1, 0, 0) and c["offending_blocks"] == [1]
    assert X.reduced_offender(w.term_offsets, w.inst_doc, w.inst_pos, S.N_CHECK) == (CHUNK, 1)


def test_c3_is_c1_with_two_rows_for_the_host():
    rows = S.uploaded_rows()
    assert [d for d, t in enumerate(rows) if not t.isascii()] == S.UPLOADED_FALLBACK and max(S.UPLOADED_FALLBACK) < S.N_CHECK
    c = S.check_census(rows, S.N_CHECK)
    w = c["want"]
    assert w.terms[:2] == ["a", "m"] and len(w.terms) == 4 and w.term_offsets.tolist()[:3] == [0, 8, 8 + S.N_UPLOADED]
    assert (c["low"], c["rule"], c["doc"]) == (CHUNK, 1, S.N_CHECK)
    assert X.first_offender(w.term_offsets, w.inst_doc, w.inst_pos, S.N_UPLOADED) is None          # the larger handle takes it


def _rule_tables():
    """Tables that fail rule 2 or 3 -- np_hip_text_build_add and the merges refuse them on the host, so no device build holds
    one -- at the block and thread edges, with a later block that offends too."""
    toff, doc, pos, _ = X.table([[(0, q) for q in range(3 * CHUNK)]])
    for at in (CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 7, CHUNK + 8, 2 * CHUNK):
        p = pos.copy()
        p[at] = p[at - 1]                                       # rule 3: the position of its predecessor
        p[2 * CHUNK + 9] = -3                                   # rule 2, later
        yield f"rule 3 at {at}", (toff, doc, p, 1), (at, 3)
        p = pos.copy()
        p[at] = -1                                              # rule 2 (and its successor fails rule 3)
        yield f"rule 2 at {at}", (toff, doc, p, 1), (at, 2)
    two = X.table([[(0, q) for q in range(CHUNK)], [(0, q) for q in range(CHUNK)]])
    yield "a term that starts at a block start has no predecessor", two, None


@pytest.mark.parametrize("name,table,want", list(_rule_tables()), ids=lambda v: v if isinstance(v, str) else "")
def test_rules_2_and_3_at_block_edges_on_the_restatement(name, table, want):
    assert X.first_offender(*table) == want
    per_block = X.block_offenders(*table)
    assert (None if per_block.min() == X.NO_OFFENDER else int(per_block.min())) == (want[0] if want else None)
    assert X.reduced_offender(*table) == want
    if name == "rule 3 at 2048":
        assert X.reduced_offender(*table, defect="block_start_has_no_predecessor") == (2 * CHUNK + 9, 2)
        assert REJECTED_BY["block_start_has_no_predecessor"].startswith("rule 3 at a block start")


def test_the_block_minimum_is_the_first_offender_on_every_shape(c1):
    tables = dict(X.shapes())
    for s, c in c1.items():
        w = c["want"]
        tables[f"C1 s={s}"] = (w.term_offsets, w.inst_doc, w.inst_pos, S.N_CHECK)
    for n_docs in S.N_FAR:
        w = TextIndexData.from_texts(S.far_rows(n_docs))
        tables[f"N1 {n_docs}"] = (w.term_offsets, w.inst_doc, w.inst_pos, n_docs)
        tables[f"N1 {n_docs} on a handle one short"] = (w.term_offsets, w.inst_doc, w.inst_pos, n_docs - 1)
    for name, t in tables.items():
        per_block = X.block_offenders(*t)
        low = None if per_block.size == 0 or per_block.min() == X.NO_OFFENDER else int(per_block.min())
        want = X.first_offender(*t)
        assert low == (want[0] if want else None), name
        assert X.reduced_offender(*t) == want, name
        assert per_block.size == X.blocks(np.asarray(t[1]).size), name


# ---- N: counts over the documents ---------------------------------------------------------------------------------------------
def test_n1_documents_far_beyond_the_instances():
    for n_docs in S.N_FAR:
        rows = S.far_rows(n_docs)
        w = TextIndexData.from_texts(rows)
        n = w.inst_doc.size
        assert len(rows) == n_docs and n == len(S.far_holders(n_docs)) <= 5 and n_docs - n >= 2042
        assert X.blocks(n) == 1 and X.blocks(n_docs) == {2047: 1, 2048: 1, 2049: 2, 4097: 3}[n_docs]
        assert X.blocks(max(n, n_docs) + 1) == {2047: 1, 2048: 2, 2049: 2, 4097: 3}[n_docs]       # flags and ranks: a block more at 2048
        assert np.count_nonzero(S.doc_len_of(rows, n_docs)) == n
    assert S.far_holders(4097) == [0, 2046, 2047, 2048, 4096] and S.far_holders(2047) == [0, 2046]


def test_n2_survivors_counted_at_a_chunk_edge():
    calls = S.survivor_calls()
    assert list(calls) == ["holder 2047 goes", "holder 2048 goes", "empty 2049 goes", "no batch", "a batch of empty rows"]
    for name, c in calls.items():
        assert c["n_told"] == S.N_COUNT and X.blocks(c["n_told"]) == 3 and c["beyond"] == 0
        assert c["n_rows_out"] == c["distinct"] < c["n_survivors"] + c["n_delta_docs"], name      # the device has to count
        assert c["n_survivors"] == S.N_COUNT - 1
    gone = {name: int(np.nonzero(c["remap"] < 0)[0][0]) for name, c in calls.items()}
    assert gone["holder 2047 goes"] == CHUNK - 1 and gone["holder 2048 goes"] == CHUNK and gone["empty 2049 goes"] == CHUNK + 1
    assert [calls[k]["distinct"] for k in calls] == [4 + 2, 4 + 2, 5 + 2, 4, 4]
    assert calls["holder 2047 goes"]["delta_inst_doc"].tolist() == [0, 2, 2] and calls["a batch of empty rows"]["delta_inst_doc"].size == 0
    assert calls["no batch"]["batch"] is None and calls["no batch"]["n_delta_docs"] == 0


def _distinct(c, defect):
    return X.distinct_result(c["doc_len"], c["remap"], c["remap"].size, c["delta_inst_doc"], c["n_delta_docs"], defect=defect)


def test_n2_rejects_the_count_defects():
    calls = S.survivor_calls()
    for defect in ("count_ignores_remap", "count_ignores_doc_len", "batch_documents_counted_per_instance", "batch_empty_rows_counted"):
        name = REJECTED_BY[defect][3:]
        c = calls[name]
        assert _distinct(c, None) == c["distinct"] and _distinct(c, defect) != c["distinct"], defect
    assert _distinct(calls["holder 2047 goes"], "count_ignores_remap") == 7                      # the removed holder counted
    assert _distinct(calls["empty 2049 goes"], "count_ignores_doc_len") == S.N_COUNT - 1 + 2     # every survivor counted
    assert _distinct(calls["holder 2048 goes"], "batch_documents_counted_per_instance") == 4 + 3
    assert _distinct(calls["a batch of empty rows"], "batch_empty_rows_counted") == 4 + 3


def test_n3_documents_behind_n_remap():
    calls = S.behind_calls()
    assert tuple(calls) == S.N_REMAPS == (4097, 4096, 2049, 2047, 1, 0)
    unaligned = []
    for n_remap, (ok, refused) in calls.items():
        assert ok["beyond"] == 0 and ok["n_told"] == n_remap and all(d < n_remap for d in ok["holders"])
        assert ok["distinct"] == len(ok["holders"]) + 2 == ok["n_rows_out"] < ok["n_survivors"] + 4
        if n_remap < S.N_COUNT and n_remap % 4:
            unaligned.append(n_remap)                            # the second count runs, and doc_len + n_told is not 16-byte aligned
        ks = [c["beyond"] for c in refused]
        assert ks == {4097: [], 4096: [1], 2049: [1, 2], 2047: [1, 4], 1: [1, 4], 0: [1, 4]}[n_remap]
        for c in refused:
            behind = [d for d in c["holders"] if d >= n_remap]
            assert len(behind) == c["beyond"] and behind[0] == n_remap
        if refused and refused[-1]["beyond"] == 4:               # the count spans the chunks of the scan over doc_len + n_told
            rel = [d - n_remap for d in refused[-1]["holders"] if d >= n_remap]
            assert rel[:3] == [0, CHUNK - 1, CHUNK] and rel[3] == S.N_COUNT - 1 - n_remap
            assert X.blocks(S.N_COUNT - n_remap) >= 2 and len({r // CHUNK for r in rel}) >= 2
    assert unaligned == [2049, 2047, 1]
    assert calls[0][0]["holders"] == [] and calls[0][0]["distinct"] == 2            # a base of empty rows only
    assert calls[4097][0]["holders"] == [0, 2046, 2047, 2048, 4096]


def test_n3_rejects_the_beyond_defects():
    ok, refused = S.behind_calls()[2047]
    one = refused[0]
    assert REJECTED_BY["beyond_counts_from_zero"] == REJECTED_BY["beyond_skips_its_first_document"] == "N3 n_remap = 2047, one"
    assert X.beyond(one["doc_len"], 2047) == 1
    assert X.beyond(one["doc_len"], 2047, defect="beyond_counts_from_zero") == 3         # documents 0 and 2046 counted too
    assert X.beyond(one["doc_len"], 2047, defect="beyond_skips_its_first_document") == 0  # the call would be accepted
    assert X.beyond(ok["doc_len"], 2047, defect="beyond_counts_from_zero") == 2           # ... and the accepted one refused


# ---- W, P ----------------------------------------------------------------------------------------------------------------------
def test_w_shapes():
    toff, doc, pos, n_docs = X.shapes()["only_empty_terms_host"]
    assert toff.tolist() == [0, 0, 0] and doc.size == 0 and n_docs == 2           # two terms, no instance: n_post = 0 for every term
    lay = X.layout(toff, doc, n_docs)
    assert lay[0].tolist() == [0, 0, 0] and lay[1].size == 0 and lay[4].tolist() == [0, 0]
    d = S.host_data("random", 64)
    assert d.terms == sorted(d.terms) and len(d.terms) == 40 and d.inst_doc.size > 300 and int(d.inst_doc.max()) < 64


def test_p1_states_have_equal_sizes_and_differ():
    rows, steps = S.states()
    assert len(rows) == 4 and len(steps) == 3
    data = [TextIndexData.from_texts(r) for r in rows]
    lays = [X.layout(d.term_offsets, d.inst_doc, S.STATE_DOCS) for d in data]
    assert len({(tuple(d.terms), d.inst_doc.size, d.n_rows, lay[1].size) for d, lay in zip(data, lays)}) == 1
    keys = [S.state_keys(r) for r in rows]
    assert len({k[0] for k in keys}) == 4 and len({k[1] for k in keys}) == 4
    for k in range(3):                                           # state k + 1 is state k with two texts swapped
        (i, ti), (j, tj) = sorted(steps[k].items())
        assert (ti, tj) == (rows[k][j], rows[k][i]) and ti != tj
        assert [t for n, t in enumerate(rows[k + 1]) if n not in (i, j)] == [t for n, t in enumerate(rows[k]) if n not in (i, j)]
