"""tests/textmerge_restate.py (the keyword-index merge in numpy) pinned to SQLite itself: random mixes of the crate's four
operations (index, delete, delete + rebuild, update_rows) are applied to a LIVE FTS5 table, and what TextIndexData._read
makes of that table is compared with the restatement's merge and with a table built from scratch with the resulting rows.
Planted defects show that the comparison catches them.  The host logic of np_textmerge_plan.h runs stand-alone through
tests/cpp/textmerge_plan_check.cpp, plain and under ASan + UBSan.  CPU only; nothing here has a tolerance."""
import os
import sqlite3
import subprocess

import numpy as np
import pytest

from helpers import ROOT

import textbuild_restate as R
import textmerge_restate as M
from next_plaid_amd import text as T
from next_plaid_amd.text import TextIndexData

WORDS = ["a", "ab", "abc", "b", "ba", "Zed", "zed9", "q", "Q_q", "x1", "x10", "x9", "mm", "m", "000", "tail"]


def _text(rng):
    n = int(rng.integers(0, 7))
    if n == 0:
        return ""
    return " ".join(WORDS[int(i)] for i in rng.integers(0, len(WORDS), n))


def _read(conn, tokenizer):
    return R.of_data(TextIndexData._read(conn, T.FTS_TABLE, tokenizer))


def _scratch(rows, tokenizer, synced):
    conn = sqlite3.connect(":memory:")
    try:
        T.create_fts_tables(conn, tokenizer, content_synced=synced)
        ids = sorted(rows)
        T.insert_fts_rows(conn, [rows[i] for i in ids], ids, tokenizer, content_synced=synced)
        return _read(conn, tokenizer)
    finally:
        conn.close()


def _delete_rows(conn, rows, ids, tokenizer, synced):
    """delete (text_search.rs): the external-content layout needs FTS5's 'delete' command with the row's indexed text."""
    with conn:
        for d in ids:
            if synced:
                conn.execute(f'INSERT INTO "{T.FTS_TABLE}"("{T.FTS_TABLE}", rowid, "{T.FTS_CONTENT_COLUMN}") VALUES (\'delete\', ?, ?)',
                             (int(d), T.prepare_document_text(rows[d], tokenizer)))
                conn.execute(f'DELETE FROM "{T.FTS_CONTENT_TABLE}" WHERE rowid = ?', (int(d),))
            else:
                conn.execute(f'DELETE FROM "{T.FTS_TABLE}" WHERE rowid = ?', (int(d),))


def _rebuild(conn, rows, tokenizer, synced):
    """rebuild: drop the table and insert the surviving rows again, numbered densely in order."""
    conn.execute(f'DROP TABLE "{T.FTS_TABLE}"')
    if synced:
        conn.execute(f'DROP TABLE "{T.FTS_CONTENT_TABLE}"')
    T.create_fts_tables(conn, tokenizer, content_synced=synced)
    new = {n: rows[d] for n, d in enumerate(sorted(rows))}
    T.insert_fts_rows(conn, [new[i] for i in sorted(new)], sorted(new), tokenizer, content_synced=synced)
    return new


def _one_mix(seed, tokenizer, synced, kind):
    """A live table through 1..3 rounds of operations.  Yields, per round, the merge's inputs and the two SQLite answers."""
    rng = np.random.default_rng(seed)
    conn = sqlite3.connect(":memory:")
    out = []
    try:
        T.create_fts_tables(conn, tokenizer, content_synced=synced)
        n0 = 0 if kind == "empty_base" else int(rng.integers(1, 12))
        rows = {i: _text(rng) for i in range(n0)}
        T.insert_fts_rows(conn, [rows[i] for i in range(n0)], range(n0), tokenizer, content_synced=synced)
        n_ids = n0
        for _ in range(int(rng.integers(1, 4))):
            base = _read(conn, tokenizer)
            ids = sorted(rows)
            if kind == "delete_all":
                gone = list(ids)
            elif kind == "empty_batch" or rng.random() < 0.7:
                gone = [d for d in ids if rng.random() < 0.35]
            else:
                gone = []
            left = [d for d in ids if d not in gone]
            rep = [] if kind in ("empty_batch", "delete_all") else [d for d in left if rng.random() < 0.25]
            n_new = 0 if kind == "empty_batch" else int(rng.integers(0, 4))
            renumber = bool(rng.random() < 0.5)
            rep_texts = [_text(rng) for _ in rep]
            new_texts = [_text(rng) for _ in range(n_new)]
            # the live table: delete, update_rows (delete + insert at the same id), index, and rebuild where ids are renumbered
            _delete_rows(conn, rows, gone, tokenizer, synced)
            for d in gone:
                del rows[d]
            _delete_rows(conn, rows, rep, tokenizer, synced)
            T.insert_fts_rows(conn, rep_texts, rep, tokenizer, content_synced=synced)
            rows.update(zip(rep, rep_texts))
            if renumber:
                new_of = {d: n for n, d in enumerate(sorted(rows))}
                rows = _rebuild(conn, rows, tokenizer, synced)
                top = len(rows)
            else:
                new_of = {d: d for d in rows}
                top = n_ids
            T.insert_fts_rows(conn, new_texts, range(top, top + n_new), tokenizer, content_synced=synced)
            rows.update(zip(range(top, top + n_new), new_texts))
            # the merge's inputs
            remap = np.full(n_ids, -1, np.int64)
            for d in left:
                if d not in rep:
                    remap[d] = new_of[d]
            delta_ids = np.asarray([new_of[d] for d in rep] + list(range(top, top + n_new)), np.int64)
            batch = R.of_data(TextIndexData.from_texts(rep_texts + new_texts, tokenizer))
            n_ids = top + n_new
            out.append(dict(base=base, remap=remap, batch=batch, delta_ids=delta_ids, n_rows=len(rows), live=_read(conn, tokenizer),
                            scratch=_scratch(rows, tokenizer, synced)))
        return out
    finally:
        conn.close()


KINDS = ["mix"] * 5 + ["empty_base", "empty_batch", "delete_all"]


@pytest.fixture(scope="module")
def cases():
    got, seed = [], 100
    for tokenizer in ("unicode61", "trigram"):
        for synced in (False, True):
            for kind in KINDS:
                for _ in range(2):
                    seed += 1
                    got += _one_mix(seed, tokenizer, synced, kind)
    return got


def test_live_table_equals_a_table_built_from_scratch(cases):
    assert len(cases) >= 60
    for c in cases:
        assert R.same(c["live"], c["scratch"])


def test_merge_rule_equals_sqlite(cases):
    dead = reborn = 0
    for c in cases:
        got = M.merge(c["base"], c["remap"], c["batch"], c["delta_ids"], c["n_rows"])
        assert R.same(got, c["live"]), (c["remap"], c["delta_ids"])
        dead += len(set(c["base"]["terms"]) - set(got["terms"]))
        reborn += sum(1 for t in c["batch"]["terms"] if t in c["base"]["terms"])
    assert dead > 10 and reborn > 10           # terms died and terms met in both vocabularies


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_planted_defects_are_caught(defect, cases):
    caught = sum(1 for c in cases
                 if not R.same(M.merge(c["base"], c["remap"], c["batch"], c["delta_ids"], c["n_rows"], defect=defect), c["live"]))
    assert caught >= 1, defect


def test_le_in_the_a_side_bound_cannot_show(cases):
    """delta_ids never equals a survivor's id, so '<=' for '<' in the A side's lower bound is the same function on every
    valid input: the disjointness check of the entry is what keeps it so."""
    for c in cases:
        assert R.same(M.merge(c["base"], c["remap"], c["batch"], c["delta_ids"], c["n_rows"], defect=M.UNOBSERVABLE[0]), c["live"])


def test_plan_update_by_hand():
    remap, ids, n = M.plan_update(5, delete=[1], replace_ids=[3], n_new=2, renumber=True)
    assert remap.tolist() == [0, -1, 1, -1, 3] and ids.tolist() == [2, 4, 5] and n == 6
    remap, ids, n = M.plan_update(5, delete=[1], replace_ids=[3], n_new=2, renumber=False)
    assert remap.tolist() == [0, -1, 2, -1, 4] and ids.tolist() == [3, 5, 6] and n == 6
    remap, ids, n = M.plan_update(3, delete=[0, 1, 2])
    assert remap.tolist() == [-1, -1, -1] and ids.size == 0 and n == 0
    assert M.bounds([0, -1, 1, -1, 3], [2, 4, 5]).tolist() == [4, 5, 5]
    assert M.bounds([-1, 5, -1, 9], [0, 6, 9, 10]).tolist() == [1, 3, 3, 4]


# ---- np_textmerge_plan.h, stand-alone ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """tests/cpp/textmerge_plan_check.cpp built with the host compiler alone, plain and under ASan + UBSan; every run goes
    through BOTH and must print the same."""
    d = tmp_path_factory.mktemp("tmplan")
    src = os.path.join(ROOT, "tests", "cpp", "textmerge_plan_check.cpp")
    exes = []
    for name, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = d / f"textmerge_plan_check_{name}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, src, "-o", str(exe)])
        exes.append(str(exe))

    def run(script: str = ""):
        outs = []
        for exe in exes:
            r = subprocess.run([exe], input=script, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
            outs.append(r.stdout.splitlines())
        assert outs[0] == outs[1]
        return outs[0]
    return run


def test_plan_header_against_hand_written_answers(plan_check):
    out = plan_check()
    assert out and out[-1] == "all checks passed", out[-5:]


def _script(c):
    def strs(terms):
        return " ".join([str(len(terms))] + [" ".join([str(len(t))] + [str(x) for x in t]) for t in terms])

    def vec(v):
        v = np.asarray(v).reshape(-1)
        return " ".join([str(v.size)] + [str(int(x)) for x in v])
    a, b = c["base"], c["batch"]
    return "\n".join(["PLAN", strs(a["terms"]), vec(a["term_offsets"]), vec(a["inst_doc"]), vec(a["inst_pos"]), vec(c["remap"]),
                      strs(b["terms"]), vec(b["term_offsets"]), vec(b["inst_doc"]), vec(c["delta_ids"]),
                      str(b["n_rows"]), str(c["n_rows"])]) + "\n"


def test_plan_header_union_and_bound_equal_the_restatement(plan_check, cases):
    """The vocabulary union and `bound` of the header, for every SQLite case, against the numpy statement."""
    script = "".join(_script(c) for c in cases)
    lines = plan_check(script)
    assert len(lines) == 4 * len(cases)
    for n, c in enumerate(cases):
        rc, ua, ub, bound = lines[4 * n: 4 * n + 4]
        assert rc.startswith("rc 0"), rc
        _, want_a, want_b, _, _ = M.union_terms(c["base"]["terms"], c["batch"]["terms"])
        assert [int(x) for x in ua.split()[1:]] == want_a and [int(x) for x in ub.split()[1:]] == want_b
        assert [int(x) for x in bound.split()[1:]] == M.bounds(c["remap"], c["delta_ids"]).tolist()
