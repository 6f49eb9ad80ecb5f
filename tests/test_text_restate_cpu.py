"""The keyword search's host side against SQLite itself (no GPU, no library).

tests/text_restate.py restates FTS5's bm25() and the reference's fusions; here the restatement is pinned to SQLite's own
FTS5 -- bm25() bit-equal in f64 and the matching set equal for every row of every query -- over tables read through
text.TextIndexData exactly as the device's keyword index is.  The compiler from FTS5 query text to term-id phrases, the
crate's sanitizers and identifier tokenizer, and the stand-alone host code of np_text_plan.h are checked here too."""
import json
import math
import os
import random
import sqlite3
import struct
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, ROOT

from next_plaid_amd import text as T
import text_restate as R

N_DOCS = 700


def oracle_table(texts, tokenizer, content_synced):
    """The same FTS5 table from_texts builds, kept open for MATCH queries."""
    conn = sqlite3.connect(":memory:")
    T.create_fts_tables(conn, tokenizer, content_synced=content_synced)
    T.insert_fts_rows(conn, texts, range(len(texts)), tokenizer, content_synced=content_synced)
    return conn


def sqlite_rows(conn, match):
    """{rowid: -bm25()} of a MATCH."""
    return {int(r): -float(s) for r, s in
            conn.execute(f'SELECT rowid, bm25("{T.FTS_TABLE}") FROM "{T.FTS_TABLE}" WHERE "{T.FTS_TABLE}" MATCH ?', (match,))}


def sqlite_topk(conn, match, k):
    """search()'s statement (text_search.rs:1262-1266); the order among equal scores normalised to ascending id."""
    rows = conn.execute(f'SELECT rowid, CAST(-bm25("{T.FTS_TABLE}") AS REAL) AS score FROM "{T.FTS_TABLE}" WHERE "{T.FTS_TABLE}" '
                        f"MATCH ? ORDER BY score DESC LIMIT ?", (match, k)).fetchall()
    return rows


def bits(x):
    return struct.pack("<d", x)


CORPORA = [("unicode61", 3, True), ("unicode61", 10, False), ("unicode61", 40, False),
           ("trigram", 3, False), ("trigram", 10, True), ("trigram", 40, False)]


@pytest.fixture(scope="module", params=CORPORA, ids=lambda c: f"{c[0]}-v{c[1]}{'-synced' if c[2] else ''}")
def corpus(request):
    tok, vocab, synced = request.param
    texts = R.make_texts(N_DOCS, vocab, seed=vocab, every="wo0" if vocab == 3 else None)
    data = T.TextIndexData.from_texts(texts, tok, content_synced=synced)
    conn = oracle_table(texts, tok, synced)
    yield tok, vocab, texts, data, R.Restated(data, N_DOCS), conn
    conn.close()


def word_queries(vocab, n, seed):
    """Query strings for any tokenizer: AND / OR of 1..5 quoted phrases of 1..3 words, now and then an unknown word or a
    repeated phrase.  Under trigram every phrase becomes several tokens."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        phrases = []
        for _ in range(rng.randint(1, 5)):
            ws = [f"wo{rng.randrange(vocab)}" for _ in range(rng.choice([1, 1, 1, 2, 2, 3]))]
            if rng.random() < 0.05:
                ws[rng.randrange(len(ws))] = "zzq"
            phrases.append('"' + " ".join(ws) + '"')
        if rng.random() < 0.15:
            phrases.append(phrases[0])
        out.append(rng.choice([" AND ", " OR ", " "]).join(phrases))
    return out


def test_from_texts_reads_the_table_sqlite_built(corpus):
    tok, vocab, texts, data, rs, conn = corpus
    assert data.n_rows == N_DOCS and data.tokenize == tok
    assert data.term_offsets[0] == 0 and data.term_offsets[-1] == data.inst_doc.size == data.inst_pos.size
    assert list(data.terms) == sorted(data.terms, key=lambda t: t.encode()) and len(set(data.terms)) == len(data.terms)
    if tok == "unicode61":
        assert [len(t.split()) for t in texts] == rs.doc_len.tolist()      # a document's instances are its tokens
        assert data.terms == sorted({w for t in texts for w in t.split()})
        assert rs.doc_len[2] == rs.doc_len.max() == 130
    assert rs.doc_len[0] == 0 and rs.doc_len[1] == 1                       # (one word of three characters is one trigram too)
    # (term, document, position) order inside every term, as np_hip_index_set_text requires it
    for t in range(data.n_terms):
        a, b = int(data.term_offsets[t]), int(data.term_offsets[t + 1])
        key = data.inst_doc[a:b] * (1 << 32) + data.inst_pos[a:b]
        assert b > a and (np.diff(key) > 0).all()


def test_bm25_is_bit_equal_to_sqlite_and_the_matching_sets_are_equal(corpus):
    """At least 300 random AND / OR queries over the six tables: every row's bm25() the same f64 bits, the same rows, the
    same top-k; with an unknown term, a repeated phrase and (vocabulary of 3) a term in every document -- the idf clamp."""
    tok, vocab, texts, data, rs, conn = corpus
    strings = word_queries(vocab, 60, seed=100 + vocab)
    queries = [(s, T.compile_text_query(s, data)) for s in strings]
    if tok == "unicode61":
        queries += [(R.match_string(q, data), q) for q in R.random_queries(data, 40, seed=vocab)]
        queries.append(('"wo0" AND "wo0"', T.TextQuery.from_phrases([[data.vocab["wo0"]]] * 2)))
    n_rows = n_clamped = n_multi = n_unknown = 0
    for s, q in queries:
        want = sqlite_rows(conn, s)
        got = rs.scores(q)
        assert set(got) == set(want), f"{s}: {len(got)} vs {len(want)} rows"
        for d, v in want.items():
            assert bits(got[d]) == bits(v), f"{s}: document {d}: {got[d]!r} vs {v!r}"
        n_rows += len(want)
        n_multi += any(len(p) > 1 for p in q.phrases())
        n_unknown += any(t < 0 for t in q.terms)
        n_clamped += any(rs.idf(len(rs.phrase_freqs(p))) == 1e-6 for p in q.phrases())
        for k in (1, 10, 1000):
            rows = sqlite_topk(conn, s, k)
            ids, sc = rs.search(q, k)
            norm = sorted(rows, key=lambda r: (-r[1], r[0]))
            assert [r[1] for r in norm] == [float(got[d]) for d in ids]
            # SQLite may keep other ids among the scores equal to the last one when the cut falls inside them
            safe = len(norm) if len(want) <= k else sum(r[1] > norm[-1][1] for r in norm)
            assert [r[0] for r in norm[:safe]] == ids[:safe].tolist()
            assert np.array_equal(sc, np.asarray([r[1] for r in norm], np.float64).astype(np.float32))
    assert n_rows > 2000 and n_multi > 10 and n_unknown > 0
    assert n_clamped > 0 or vocab != 3
    assert len(queries) * len(CORPORA) >= 300


def test_queries_at_the_limits_are_bit_equal_to_sqlite():
    """64 phrases, a phrase of 256 tokens, overlapping occurrences of a repeated token and position lists of 300 entries, on
    a corpus of 40 documents: SQLite accepts every one of them, and the restatement has its bm25() bits and its rows.  The
    GPU tests run the same queries (R.limit_queries) against the restatement."""
    n = 40
    texts = R.limit_texts(n)
    data = T.TextIndexData.from_texts(texts)
    conn = oracle_table(texts, "unicode61", False)
    rs = R.Restated(data, n)
    try:
        queries = dict(R.limit_queries(data))
        assert len(queries) == 8
        # the frequencies the corpus was built for
        f = rs.phrase_freqs(queries["256 x aa"].phrases()[0])
        assert f == {1: 45, n - 3: 45, n - 1: 45}                          # positions 0 .. 44 of 300
        f = rs.phrase_freqs(queries["128 x aa bb"].phrases()[0])
        assert f == {3: 23, 4: 22, n - 2: 23}                              # every second position
        f = rs.phrase_freqs(queries["aa aa aa"].phrases()[0])
        assert f[2] == 3 and f[1] == 298 and f[9] == 1 and set(f) == {1, 2, 9, n - 3, n - 1}   # occurrences overlap
        assert sorted(rs.scores(queries["64 words AND"])) == [5, 6, 8, n - 2, n - 1]
        assert sorted(rs.scores(queries["64 words OR"])) == [5, 6, 7, 8, n - 2, n - 1]
        assert sorted(rs.scores(queries["16 x 4 AND"])) == [5, 8, n - 2, n - 1]
        assert rs.scores(queries["63 words and an unknown AND"]) == {}
        assert len(rs.scores(queries["63 unknown OR aa"])) > 12
        for name, q in queries.items():
            assert q.n_phrases in (1, 16, 64) and max(len(p) for p in q.phrases()) in (1, 3, 4, 256)
            s = R.match_string(q, data)
            want = sqlite_rows(conn, s)
            got = rs.scores(q)
            assert set(got) == set(want), f"{name}: {sorted(got)} vs {sorted(want)}"
            for d, v in want.items():
                assert bits(got[d]) == bits(v), f"{name}: document {d}: {got[d]!r} vs {v!r}"
            ids, sc = rs.search(q, 10)
            norm = sorted(sqlite_topk(conn, s, 10), key=lambda r: (-r[1], r[0]))
            assert [r[1] for r in norm] == [float(got[d]) for d in ids]
    finally:
        conn.close()


def test_compiled_strings_match_what_sqlite_matches(corpus):
    tok, vocab, texts, data, rs, conn = corpus
    accepted = ["wo0", "wo0 wo1", "wo0 AND wo1", "wo0 OR wo1 OR zzq", '"wo0 wo1"', '"wo1 wo0" wo2', 'wo0 "wo1"wo2', "wo1 and wo0",
                '"wo0" "wo0"', "NEAR", "wo0 NEAR wo1", 'wo0 AND "wo1 wo2" AND wo0', '"wo""1"', "wo0_wo1", "wo1\twO2\n",
                T.sanitize_fts5_query("wo1, (wo2)! and NOT wo0?"), T.sanitize_fts5_query_or("wo1Wo2 wo0_wo1")]
    # phrases without a token: what SQLite does with them is what the compiler does (text.compile_text_query's docstring)
    empties = ['""', '"!!!"', '"" AND wo0', 'wo0 AND ""', 'wo0 OR ""', '"" OR wo0', '"!!!" wo0', 'wo0 "!!!" wo1', 'wo0 AND "!!!" wo1',
               'wo0 "!!!" AND wo1', '"!!!" "???" AND wo0', '"!!!" "???"', '"!!!" OR "???"', 'wo0 OR "" OR wo1']
    for s in accepted + empties:
        q = T.compile_text_query(s, data)
        want = sqlite_rows(conn, s)
        got = rs.scores(q)
        assert set(got) == set(want), f"{s!r}: {len(got)} vs {len(want)} rows"
        assert all(bits(got[d]) == bits(want[d]) for d in want), s
    # pinned: an explicit AND with an empty side, and a query of empty phrases only, match nothing
    # ("!!!" has no token under unicode61; under trigram it is one, unknown, token -- and "!!" has none)
    e1, e2 = ('"!!!"', '"???"') if tok == "unicode61" else ('"!!"', '"wo"')
    for s in ('"" AND wo0', 'wo0 AND ""', '""', f"{e1} {e2}", f"{e1} OR {e2}", f"{e1} {e2} AND wo0"):
        assert T.compile_text_query(s, data).phrases() == T.MATCH_NOTHING and sqlite_rows(conn, s) == {}
    if tok == "unicode61":
        assert T.compile_text_query('wo0 "!!!" wo1', data).phrases() == T.compile_text_query("wo0 wo1", data).phrases()
        assert T.compile_text_query("wo0_wo1", data).phrases() == [[data.vocab["wo0"], data.vocab["wo1"]]]   # one word, two tokens
    else:
        assert len(T.compile_text_query("wo1", data).phrases()[0]) == 1 and len(T.compile_text_query('"wo1 wo2"', data).phrases()[0]) == 5
        assert T.compile_text_query("wo", data).phrases() == T.MATCH_NOTHING      # shorter than a trigram: no token


REFUSED = [("wo0 NOT wo1", "NOT"), ("NOT wo0", "NOT"), ("NEAR(wo0 wo1)", "NEAR"), ("NEAR (wo0 wo1, 3)", "NEAR"), ("wo*", "prefix"),
           ('"wo0" *', "prefix"), ("^wo0", "initial"), ("c:wo0", "column"), ("{a b}:wo0", "column"), ("-c:wo0", "column"),
           ("(wo0)", "parenthes"), ("wo0 AND (wo1 OR wo2)", "parenthes"), ("wo0 AND wo1 OR wo2", "mixed"),
           ("wo0 OR wo1 wo2", "mixed"), ("wo0 wo1 OR wo2", "mixed"), ("wo0 + wo1", "concatenation"), ("wo0.wo1", "syntax error"),
           ("wo0, wo1", "NEAR argument"), ("'wo0'", "syntax error"), ("AND wo0", "syntax error"), ("wo0 OR", "syntax error"),
           ("wo0 AND AND wo1", "syntax error"), ('"wo0', "unterminated"), ("", "empty"), ("   ", "empty")]


@pytest.mark.parametrize("text,names", REFUSED, ids=[repr(r[0]) for r in REFUSED])
def test_every_other_construct_is_refused_by_name(text, names):
    data = T.TextIndexData.from_texts(["wo0 wo1 wo2"])
    with pytest.raises(T.TextQueryError, match=names):
        T.compile_text_query(text, data)


def test_limits_of_a_compiled_query():
    data = T.TextIndexData.from_texts(["wo0 wo1 wo2"])
    assert T.compile_text_query(" ".join(["wo0"] * 64), data).n_phrases == 64
    with pytest.raises(T.TextQueryError, match="64 phrases"):
        T.compile_text_query(" ".join(["wo0"] * 65), data)
    assert T.compile_text_query('"' + " ".join(["wo0"] * 256) + '"', data).terms.size == 256
    with pytest.raises(T.TextQueryError, match="256 tokens"):
        T.compile_text_query('"' + " ".join(["wo0"] * 257) + '"', data)


def test_from_sqlite_reads_the_crates_layout(tmp_path):
    """A metadata.db laid out as text_search.rs:306-500 lays it out, built with plain SQL: the settings table, the content
    table keyed by document id, the external-content FTS5 table; rows deleted the way delete() does it."""
    texts = ["fn parseRequest(payload: Buffer) -> Response_Builder", "struct HandlerStack;", "", "let http_response = getHTTPResponse();",
             "parse the request"]
    for tok in ("unicode61", "trigram", "identifier_aware"):
        db = tmp_path / f"{tok}.db"
        conn = sqlite3.connect(str(db))
        conn.execute("CREATE TABLE METADATA (_subset_ INTEGER PRIMARY KEY, body TEXT)")
        conn.execute('CREATE TABLE "_FTS_SETTINGS_" (key TEXT PRIMARY KEY, value TEXT NOT NULL)')
        conn.execute('CREATE TABLE "METADATA_FTS_CONTENT" (rowid INTEGER PRIMARY KEY, "_fts_content_" TEXT NOT NULL DEFAULT \'\')')
        conn.execute('CREATE VIRTUAL TABLE "METADATA_FTS" USING fts5("_fts_content_", content=\'METADATA_FTS_CONTENT\', '
                     f"content_rowid='rowid', tokenize='{T.TOKENIZERS[tok]}')")
        conn.execute('INSERT OR REPLACE INTO "_FTS_SETTINGS_"(key, value) VALUES (\'tokenizer\', ?)', (tok,))
        for i, t in enumerate(texts + ["to be deleted"]):
            conn.execute('INSERT OR REPLACE INTO "METADATA_FTS_CONTENT"(rowid, "_fts_content_") VALUES (?, ?)', (i, t))
            conn.execute('INSERT INTO "METADATA_FTS"(rowid, "_fts_content_") VALUES (?, ?)', (i, T.prepare_document_text(t, tok)))
        conn.execute('INSERT INTO "METADATA_FTS"("METADATA_FTS", rowid, "_fts_content_") VALUES (\'delete\', ?, ?)',
                     (len(texts), T.prepare_document_text("to be deleted", tok)))
        conn.execute('DELETE FROM "METADATA_FTS_CONTENT" WHERE rowid = ?', (len(texts),))
        conn.commit()
        conn.close()
        data = T.TextIndexData.from_sqlite(str(db))
        same = T.TextIndexData.from_texts(texts, tok, content_synced=True)
        assert data.tokenizer == tok and data.n_rows == len(texts) == same.n_rows
        assert data.terms == same.terms and np.array_equal(data.term_offsets, same.term_offsets)
        assert np.array_equal(data.inst_doc, same.inst_doc) and np.array_equal(data.inst_pos, same.inst_pos)
        if tok == "identifier_aware":
            assert {"parserequest", "parse", "request", "handler", "stack", "http", "response"} <= set(data.terms)   # (unicode61 splits handler_stack again)
            q = T.compile_text_query(T.sanitize_fts5_query_or("HandlerStack"), data)
            assert q.mode == T.NP_TEXT_OR and sorted(R.Restated(data, len(texts)).scores(q)) == [1]
    with pytest.raises(ValueError, match="METADATA_FTS"):
        empty = tmp_path / "empty.db"
        sqlite3.connect(str(empty)).close()
        T.TextIndexData.from_sqlite(str(empty))


def test_identifier_tokenizer_and_sanitizers_give_the_references_known_answers():
    with open(os.path.join(GOLDEN, "identifier_tokens.json")) as f:
        g = json.load(f)
    for token, want in g["split_identifier"]:
        assert T.split_identifier(token) == want
    for text, want in g["tokenize_identifiers"]:
        assert T.tokenize_identifiers(text) == want
    for text, want in g["tokenize_identifiers_contains"]:
        assert set(want) <= set(T.tokenize_identifiers(text))
    for text, want in g["prepare_document_text_identifier_aware_contains"]:
        assert set(want) <= set(T.prepare_document_text(text, "identifier_aware").split())
        assert T.prepare_document_text(text, "unicode61") == text and T.prepare_document_text(text, "trigram") == text
    for text, want in g["sanitize_fts5_query_or"]:
        assert T.sanitize_fts5_query_or(text) == want
    for text in g["sanitize_fts5_query_or_distinct"]:
        terms = T.sanitize_fts5_query_or(text).split(" OR ")
        assert len(terms) == len(set(terms)) > 2
    # sanitize_fts5_query by its definition (text_search.rs:949-968): edges trimmed, operators dropped, words quoted
    assert T.sanitize_fts5_query('hello, (world)! AND not "quo"te" near ... or x') == '"hello" "world" "quo""te" "x"'
    assert T.sanitize_fts5_query("  ") == "" and T.sanitize_fts5_query("café! ¿qué?") == '"café" "qué"'
    assert T.tokenize_identifiers("café_x naïve9 _a1") == ["caf", "_x", "na", "ve9", "ve", "9", "ve_9", "_a1"]   # ASCII only


def f32(x):
    return np.float32(x)


def test_fusion_restatement_on_hand_computed_cases():
    a75, a25 = f32(0.75), f32(0.25)
    # RRF, disjoint lists: every entry keeps its own term; 0.75 / 61 > 0.75 / 62 > 0.25 / 61 > 0.25 / 62
    ids, sc = R.fuse_rrf([5, 3], [9, 7], 0.75, 10)
    assert ids.tolist() == [5, 3, 9, 7]
    assert sc.tolist() == [a75 / f32(61), a75 / f32(62), a25 / f32(61), a25 / f32(62)]
    # identical lists: the two terms add, semantic first
    ids, sc = R.fuse_rrf([5, 3], [5, 3], 0.75, 10)
    assert ids.tolist() == [5, 3] and sc.tolist() == [a75 / f32(61) + a25 / f32(61), a75 / f32(62) + a25 / f32(62)]
    # one list empty; alpha 0 and 1; top_k cuts
    assert R.fuse_rrf([], [4, 2], 0.75, 10)[0].tolist() == [4, 2] and R.fuse_rrf([4, 2], [], 0.75, 1)[0].tolist() == [4]
    ids, sc = R.fuse_rrf([8, 1], [1, 2], 1.0, 10)
    assert ids.tolist() == [8, 1, 2] and sc.tolist() == [f32(1) / f32(61), f32(1) / f32(62), 0.0]
    ids, sc = R.fuse_rrf([8, 1], [1, 2], 0.0, 10)
    assert ids.tolist() == [1, 2, 8] and sc.tolist() == [f32(1) / f32(61), f32(1) / f32(62), 0.0]
    # a tie broken by id: alpha 0.5, mirrored ranks
    ids, sc = R.fuse_rrf([7, 3], [3, 7], 0.5, 10)
    assert ids.tolist() == [3, 7] and sc[0] == sc[1]
    # relative score: (s - min) / (max - min) per list
    ids, sc = R.fuse_relative_score([1, 2, 3], [10.0, 6.0, 2.0], [3, 4], [5.0, 1.0], 0.75, 10)
    assert ids.tolist() == [1, 2, 3, 4]
    assert sc.tolist() == [a75 * f32(1), a75 * f32(0.5), f32(0) + a25 * f32(1), 0.0]
    # all scores equal: range 0, every entry 1.0
    ids, sc = R.fuse_relative_score([9, 4], [3.0, 3.0], [4], [7.0], 0.75, 10)
    assert ids.tolist() == [4, 9] and sc.tolist() == [a75 + a25, a75]
    # one list empty contributes nothing; alpha 0 / 1
    assert R.fuse_relative_score([], [], [6, 5], [2.0, 1.0], 0.75, 10)[1].tolist() == [a25, 0.0]
    ids, sc = R.fuse_relative_score([1, 2], [2.0, 1.0], [2, 3], [9.0, 8.0], 1.0, 10)
    assert ids.tolist() == [1, 2, 3] and sc.tolist() == [1.0, 0.0, 0.0]
    ids, sc = R.fuse_relative_score([1, 2], [2.0, 1.0], [2, 3], [9.0, 8.0], 0.0, 10)
    assert ids.tolist() == [2, 1, 3] and sc.tolist() == [1.0, 0.0, 0.0]
    # NaN: ignored by min / max, its own entry is NaN and sorts after every number
    ids, sc = R.fuse_relative_score([1, 2, 3], [4.0, float("nan"), 2.0], [], [], 0.75, 10)
    assert ids.tolist() == [1, 3, 2] and sc[0] == a75 and sc[1] == 0.0 and math.isnan(sc[2])
    # identical lists and a tie by id
    ids, sc = R.fuse_relative_score([4, 2], [1.0, 1.0], [4, 2], [5.0, 5.0], 0.75, 10)
    assert ids.tolist() == [2, 4] and sc.tolist() == [a75 + a25] * 2


def test_host_code_of_the_keyword_search_stands_alone(tmp_path):
    """tests/cpp/text_plan_check.cpp: np_text_plan.h with the host compiler alone (no device, no library), plain and under
    AddressSanitizer + UBSan."""
    src = os.path.join(ROOT, "tests", "cpp", "text_plan_check.cpp")
    inc = os.path.join(ROOT, "next-plaid_amd", "csrc")
    for name, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / f"text_plan_check_{name}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, src, "-o", str(exe)])
        out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "all checks passed" in out.stdout, name + ": " + out.stdout + out.stderr
