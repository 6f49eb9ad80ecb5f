"""The generators and the vectorised reference of tests/textbuild_limit_shapes.py at a reduced size, on the CPU: what
tests/test_gpu_textbuild_limits.py compares the device with on its two largest shapes is pinned here, on the same generators,
array for array to SQLite's own FTS5, to tests/textbuild_restate.py (build) and to tests/textmerge_restate.py (merge).  Each
planted defect of the reference must fail that comparison.  The other generators are checked for what the GPU test relies on:
SQLite's treatment of a token at and over its 32768-byte limit, the sizes, and the restated fallback rule."""
import numpy as np
import pytest

import textbuild_limit_shapes as S
import textbuild_restate as R
import textmerge_restate as M

from next_plaid_amd.text import TextIndexData


def same_arrays(a, b):
    return R.same(a, b) and a["term_offsets"].dtype == b["term_offsets"].dtype == np.int64 and \
        a["inst_doc"].dtype == b["inst_doc"].dtype == np.int64 and a["inst_pos"].dtype == b["inst_pos"].dtype == np.int32


def build_case(n_tokens):
    words, flat, row_off = S.one_long_document(n_tokens)
    raw, off = S.raw_of(words, flat, row_off)
    texts = S.texts_of(raw, off)
    assert texts == [" ".join(words[w].decode() for w in flat[row_off[i]: row_off[i + 1]]) for i in range(row_off.size - 1)]
    sqlite = R.of_data(TextIndexData.from_texts(texts))
    restated = R.build([t.encode() for t in texts])
    assert restated.pop("fallback_docs") == [] and R.same(restated, sqlite)
    return (words, flat, row_off), sqlite


def build_matches(case, sqlite, defect=None):
    return same_arrays(S.ref_build(*case, defect=defect), sqlite)


def update_case(edge, tail, lead, renumber):
    """The M1 update at a reduced size: (the arguments of ref_update, SQLite's index of the resulting rows, the merge restated)."""
    words, flat, row_off, big = S.run_corpus(edge, tail, lead)
    n = row_off.size - 1
    base = S.ref_build(words, flat, row_off)
    texts = S.texts_of(*S.raw_of(words, flat, row_off))
    assert R.same(base, R.of_data(TextIndexData.from_texts(texts)))
    delete, replace, new, (bflat, boff) = S.run_update(base, edge, n, big)
    assert len(replace) == 3 and len(delete) >= 5
    sqlite = R.of_data(S.sqlite_rows(S.rows_after(texts, new, delete, replace, renumber)))
    remap, delta_ids, n_rows_out = M.plan_update(n, delete, sorted(replace), len(new), renumber)
    restated = M.merge(base, remap, S.ref_build(words, bflat, boff), delta_ids, n_rows_out)
    assert R.same(restated, sqlite)
    return (words, flat, row_off, bflat, boff, len(replace), delete, sorted(replace), renumber), sqlite


def update_matches(args, sqlite, defect=None):
    return same_arrays(S.ref_update(*args, defect=defect), sqlite)


# ---- the reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tokens", [100, 5000])
def test_reference_build_equals_sqlite_and_the_restated_build(n_tokens):
    case, sqlite = build_case(n_tokens)
    assert build_matches(case, sqlite)
    assert (len(sqlite["terms"]) < 300) == (n_tokens < 300)          # at 100 tokens most words have no instance and are no terms


@pytest.mark.parametrize("lead", [0, 5])
@pytest.mark.parametrize("renumber", [True, False])
def test_reference_update_equals_sqlite_and_the_restated_merge(lead, renumber):
    args, sqlite = update_case(700, 60, lead, renumber)
    assert update_matches(args, sqlite)
    assert b"zz" in sqlite["terms"] and b"other" in sqlite["terms"]


def test_every_planted_defect_of_the_reference_is_caught():
    assert len(S.REF_DEFECTS) >= 4
    case, built = build_case(5000)
    args, updated = update_case(700, 60, 5, True)
    died, updated_died = update_case(700, 60, 0, True)      # lead 0: the four-instance document goes, and "x" with it
    assert b"x" not in updated_died["terms"]
    caught = {}
    for defect in S.REF_DEFECTS:
        caught[defect] = [not build_matches(case, built, defect), not update_matches(args, updated, defect),
                          not update_matches(died, updated_died, defect)]
    assert all(any(v) for v in caught.values()), caught
    # each where it belongs: the order and the positions in the build, the ids and the dead term in the update
    assert caught["unstable_sort"][0] and caught["byte_pos"][0] and caught["byte_pos"][1]
    assert caught["ids_not_renumbered"][1] and caught["dead_term_kept"][2]


# ---- the other generators ----------------------------------------------------------------------------------------------------
def test_sparse_corpus_has_live_documents_on_both_sides_of_the_edge():
    n, edge = 2 * 2048 + 3 * 16 + 7, 4096
    texts = S.sparse_corpus(n, edge)
    live = [i for i, t in enumerate(texts) if t]
    assert len(texts) == n and {edge - 1, edge, edge + 1, n - 1, 0, 97} <= set(live) and len(live) == len(range(0, n, 97)) + 4
    got = R.build([t.encode() for t in texts])
    assert got.pop("fallback_docs") == [] and R.same(got, R.of_data(TextIndexData.from_texts(texts)))
    assert got["terms"] == [b"a", b"b0", b"b1", b"b2", b"b3", b"b4"]


def test_sqlite_keeps_a_token_of_32768_bytes_and_truncates_a_longer_one():
    texts, over = S.token_cap_corpus(S.MAX_TOKEN)
    assert over == [2, 3, 7, 8] and len(texts) == 10
    data = TextIndexData.from_texts(texts)
    assert "x" * S.MAX_TOKEN in data.vocab and "y" * S.MAX_TOKEN in data.vocab and "y" * (S.MAX_TOKEN + 1) not in data.vocab
    assert sorted(data.terms) == sorted(["a", "b", "ok", "x" * S.MAX_TOKEN, "y" * S.MAX_TOKEN])
    raws = [t.encode() for t in texts]
    assert [i for i, r in enumerate(raws) if R.is_fallback(r, "unicode61", S.MAX_TOKEN)] == over
    # what the device reproduces plus SQLite's instances of the fallback documents is SQLite's index
    dev = R.build(raws, "unicode61", S.MAX_TOKEN)
    assert dev.pop("fallback_docs") == over
    assert R.same(R.merge(dev, R.restrict(R.of_data(data), over)), R.of_data(data))


@pytest.mark.parametrize("tile", [32, 64])
def test_tile_edge_corpus_through_sqlite(tile):
    texts = S.tile_edge_corpus(tile)
    assert len(texts) > 6 * 6 * 6 * 3 and max(len(t) for t in texts) == 2 * tile + 1 + 3 * tile + 1 + 2
    for tokenizer, part in (("unicode61", texts), ("trigram", texts[::20])):
        got = R.build([t.encode() for t in part], tokenizer, 4 * tile)
        assert got.pop("fallback_docs") == [] and R.same(got, R.of_data(TextIndexData.from_texts(part, tokenizer))), tokenizer


def test_sizes_of_the_small_generators():
    texts = S.many_terms_corpus(500, 20)
    data = TextIndexData.from_texts(texts)
    assert data.n_terms == 500 and data.inst_doc.size == 1000 and len(texts) == 20
    doc, abc = S.random_bytes_document(3000)
    assert len(doc) == 3000 and abc == "abc" and min(map(ord, doc)) >= 1 and max(map(ord, doc)) < 0x80
    assert TextIndexData.from_texts([doc, abc], "trigram").inst_doc.size == 2998 + 1
    assert S.blocks(256 * 2048) == 256 and S.blocks(256 * 2048 + 1) == 257 and S.blocks(0) == 0
    assert len(S.wide_table_corpus()) == 300 and len(S.thread_corpus()) == 300
    assert all(ord(c) < 0x80 for t in S.workspace_corpus(5, 10) + S.thread_corpus(20) for c in t)
