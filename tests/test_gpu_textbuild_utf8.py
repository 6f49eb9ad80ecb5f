"""The keyword build's UTF-8 mode (tb_walk_utf8, tb_insert_utf8) against SQLite itself: every case compares the device result
with TextIndexData.from_texts on the same texts, array for array, and fallback_docs with the predicted list exactly -- empty
for well-formed text inside the table -- so the fallback path never hides a wrong device result."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, hip_index, make_arrays

import next_plaid_amd as npa
from next_plaid_amd import api
from next_plaid_amd import text as T
from next_plaid_amd.text import TextIndexData

import textbuild_utf8_restate as U
from textbuild_limit_shapes import assert_same as _same, rows_after, sqlite_rows

pytestmark = pytest.mark.gpu

MARK = "́"
TWO, THREE, FOUR = "é", "中", "\U00010400"      # sequences of 2, 3 and 4 bytes; the last folds to U+10428


def check(texts, tokenizer="unicode61", fallback=(), **kw):
    got = TextIndexData.from_texts_device(texts, tokenizer, utf8=True, **kw)
    _same(got, TextIndexData.from_texts(texts, tokenizer))
    assert got.fallback_docs == list(fallback)
    assert got.build_report["n_docs"] == len(texts) and got.build_report["n_fallback"] == len(got.fallback_docs)
    return got


def test_the_issues_three_documents():
    texts = ["café crème", "Ⱥ ⱥ", "naïve"]
    got = check(texts)
    assert got.terms == ["cafe", "creme", "naive", "ⱥ"]
    plain = TextIndexData.from_texts_device(texts)
    _same(plain, TextIndexData.from_texts(texts))
    assert plain.fallback_docs == [0, 1, 2]


def test_every_code_point_of_planes_0_and_1():
    cps = [cp for cp in range(2 * 65536) if not 0xD800 <= cp < 0xE000]
    got = check(["x" + chr(cp) + "y" for cp in cps])
    assert got.build_report["n_instances"] == got.inst_doc.size and got.n_rows == len(cps)


@pytest.mark.parametrize("tile", [16, 32, 1024])
def test_sequences_at_every_alignment_and_across_lane_and_tile_edges(tile):
    """Every document is followed by one that is a byte longer, so the documents' own first bytes take every place of a
    16-byte line (r0 = -15..0) and every sequence every alignment; the pads put sequences across the edges of a lane
    (16), of the small tiles and of the 1024-byte tile."""
    texts = []
    for lead in range(17):
        for ch in (TWO, THREE, FOUR):
            for pad in list(range(18)) + [tile - 2, tile - 1, tile, 2 * tile - 1, 1021, 1022, 1023, 1024, 1025]:
                texts.append("-" * pad + ch + "a" + ch + ch + " " + ch + "-" + ch + "b")
            texts.append(ch)
            texts.append(ch * 9 + " " + ch * 340)          # a token across several lanes; one across a 1024-byte tile
        texts.append("q" * lead)
    # the coverage the docstring claims, computed from the offsets the build gets: per sequence length, every r0 of a
    # document that begins with such a sequence, every alignment, and every way to split it at a lane and at a tile edge
    r0s, aligns, lane_splits, tile_splits = ({n: set() for n in (2, 3, 4)} for _ in range(4))
    b = 0
    for t in texts:
        line, at = b & ~15, b
        for i, ch in enumerate(t):
            n = len(ch.encode("utf-8"))
            if n > 1:
                if i == 0:
                    r0s[n].add(line - b)
                aligns[n].add(at % 16)
                if at % 16 + n > 16:
                    lane_splits[n].add(16 - at % 16)
                if (at - line) % tile + n > tile:
                    tile_splits[n].add(tile - (at - line) % tile)
            at += n
        b = at
    for n in (2, 3, 4):
        assert r0s[n] == set(range(-15, 1)) and aligns[n] == set(range(16)), n
        assert lane_splits[n] == set(range(1, n)) and tile_splits[n] == set(range(1, n)), n
    check(texts, tile_bytes=tile, max_token_bytes=2048)


@pytest.mark.parametrize("tile", [16, 32, 1024])
def test_runs_of_marks(tile):
    """1, 8, 9 and 600 marks of two bytes: less than a lane, a full lane, a lane and one more, more than a 1024-byte tile --
    after a token character, after a separator, at the document's start and at its end, at every alignment."""
    texts = []
    for run in (1, 8, 9, 600):
        m = MARK * run
        for pad in range(17 if run < 600 else 3):
            p = "-" * pad
            texts += [p + "a" + m + "b c", p + " " + m + "b", p + "a " + m, p + "ab" + m, m + "b" + p, m, p + m + " " + m + "z" + m,
                      p + "é" + m + "é", p + "中" + m + ", " + m + "中"]
    got = check(texts, tile_bytes=tile, max_token_bytes=4096)
    assert "ab" in got.vocab and "ee" in got.vocab and "" not in got.vocab


def test_one_term_from_different_raw_lengths_and_a_table_that_retries():
    words = ["É é e e" + MARK + " Ｅ E" + MARK + MARK, "Ⱥ ⱥ Ⱥ" + MARK, "é", "E"] + [f"mot{i} Mot{i} mót{i} ＭＯＴ{i}" for i in range(40)]
    for bits in (1, 2, 5, 0):
        got = check(words, hash_bits=bits)
        if bits in (1, 2):
            assert got.build_report["table_retries"] > 0
    # É, é, e, e + mark, E + two marks, and é and E of their own documents are one term; SQLite folds the full-width Ｅ to the
    # full-width ｅ, a term of its own
    assert got.terms[:1] == ["e"] and got.term_offsets[1] == 7 and "ⱥ" in got.vocab and "ｅ" in got.vocab and got.n_terms == 83
    k = got.vocab["ⱥ"]
    assert got.term_offsets[k + 1] - got.term_offsets[k] == 3


def _raw_build(docs, **kw):
    """api.text_build on raw bytes; the fallback documents add nothing, so the result is the device's alone."""
    off = np.zeros(len(docs) + 1, np.int64)
    off[1:] = np.cumsum([len(d) for d in docs])
    none = lambda ids: (np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int32))
    return api.text_build(np.frombuffer(b"".join(docs), np.uint8), off, api.NP_TOK_UNICODE61, none, utf8=True, **kw)


@pytest.mark.parametrize("tile", [16, 1024])
def test_malformed_text_and_code_points_beyond_the_table_fall_back_alone(tile):
    bad = [b"\x80", b"ab\xbfcd", b"\xc3", b"ab \xe4\xb8", b"\xf0\x90\x90", b"\xc0\xaf", b"\xc1\xbf", b"\xe0\x9f\xbf", b"\xf0\x8f\xbf\xbf",
           b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xf8\x88\x80\x80\x80", b"\xff", b"\xfe ab",
           b"\xc3\x41", b"\xe4\xb8\x41", b"\xc3\xa9\xa9", "\U00020000".encode(), "ok \U0002A6D6 ok".encode(), "\U000E0041".encode(),
           "\U0010FFFF".encode()]
    good = ["café".encode(), b"ab", "\U0001FFFF \U00010400".encode(), "퟿  ￿".encode("utf-8", "surrogatepass"), b""]
    docs = []
    for i, b in enumerate(bad):
        docs += [good[i % len(good)], b"-" * (i % 16) + b + b"-" * (i % 3), b"x" * (i % 5)]
    # a lead byte at a document's end is not completed by the next document's bytes
    docs += [b"ab\xc3", b"\xa9cd", b"ok", b"zz\xe4\xb8", b"\xadzz", b"ok", b"\xf0\x90", b"\x90\x80", b"fin\xc3"]
    want_fb = U.predict_fallback(docs, 2)
    assert len(want_fb) == len(bad) + 7 and all(i % 3 == 1 for i in want_fb[:len(bad)])
    r = _raw_build(docs, tile_bytes=tile)
    assert r["fallback_docs"].tolist() == want_fb
    kept = [("" if i in set(want_fb) else d.decode("utf-8")) for i, d in enumerate(docs)]
    want = TextIndexData.from_texts(kept)
    _same(TextIndexData._of_build("unicode61", r), want)
    # the same bytes under a 3-plane table: the two documents of plane 2 stay on the device
    r3 = _raw_build(docs, tile_bytes=tile, unicode_planes=3)
    fb3 = U.predict_fallback(docs, 3)
    assert r3["fallback_docs"].tolist() == fb3 and len(fb3) == len(want_fb) - 2
    _same(TextIndexData._of_build("unicode61", r3), TextIndexData.from_texts([("" if i in set(fb3) else d.decode("utf-8")) for i, d in enumerate(docs)]))


def test_an_ascii_corpus_is_built_as_without_the_table():
    import textbuild_restate as R
    texts = R.random_ascii(71, 600, 60) + ["x" * 257 + " ok", "x" * 256, "", "a\x00b"]
    a = TextIndexData.from_texts_device(texts)
    b = check(texts, fallback=a.fallback_docs)
    assert a.fallback_docs == [600]
    assert a.terms == b.terms
    for k in ("term_offsets", "inst_doc", "inst_pos"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes()


def test_the_cap_counts_raw_bytes():
    texts = ["é" * 5, "é" * 5 + "a", "e" + MARK * 4 + "z", "e" + MARK * 5, "中中中a", "中中中ab", "ÀÀÀÀÀ b", "ÀÀÀÀÀÀ"]
    check(texts, max_token_bytes=10, fallback=[1, 3, 5, 7])          # 10 raw bytes stay, 11 and 12 go; the folds are shorter
    check(["é" * 128, "é" * 128 + "a"], fallback=[1])                # the default cap, 256
    big = "é" * 10922 + "a"                                          # 21845 raw bytes
    check([big, big + "a", "ok"], max_token_bytes=21845, fallback=[1])
    with pytest.raises(ValueError, match="max_token_bytes 21846"):
        TextIndexData.from_texts_device(["ok"], utf8=True, max_token_bytes=21846)
    assert TextIndexData.from_texts_device(["ok"], max_token_bytes=21846).fallback_docs == []   # the ASCII mode's limit is its own


def test_refusals_before_any_launch():
    import ctypes as C
    L, raw, off = api.lib(), np.frombuffer(b"abc", np.uint8), np.asarray([0, 3], np.int64)
    t = T.unicode61_table(2).copy()

    def call(table, n, **kw):
        o, h = api.np_text_build_opts(0, 0, kw.get("workspace_bytes", 0)), C.c_void_p()
        o.unicode_table, o.unicode_table_len = table.ctypes.data, n
        rc = L.np_hip_text_build(0, api._ptr(raw), api._ptr(off), 1, C.byref(o), C.byref(h), None)
        assert h.value is None or rc == 0
        if h.value:
            L.np_hip_text_build_free(h)
        return rc, api.last_error()

    assert call(t, t.size)[0] == 0
    rc, why = call(t, 65535)
    assert rc == 8 and "unicode_table_len 65535" in why
    t[0x41] = (1 << 30) | 0x41
    rc, why = call(t, t.size)
    assert rc == 8 and "unicode_table[0x41]" in why
    t = T.unicode61_table(2).copy()
    t[0x400] = 3 << 30
    rc, why = call(t, t.size)
    assert rc == 8 and "class 3" in why
    # the table's device copy counts: a workspace one byte short of text + per-document arrays + table is refused
    t = T.unicode61_table(2)
    need = 256 + 2 * 256 + 2 * 256 + 256 + 256 + t.size * 4        # textbuild_bytes_docs(3, 1, 131072)
    rc, why = call(t, t.size, workspace_bytes=need - 1)
    assert rc == 7 and f"workspace of {need - 1} bytes" in why
    rc, why = call(t, t.size, workspace_bytes=need - t.size * 4)   # enough for the ASCII call, not for the table
    assert rc == 7


def test_updated_with_a_delete_and_a_replace():
    texts = ["café crème", "plain ascii", "naïve Ⱥ", "über straße", "e" + MARK + "t" + "e" + MARK, ""]
    base = check(texts)
    new, gone, rep = ["Crème brûlée", "中文 text"], [1], {3: "ÜBER strasse ⱥ", 0: "cafe"}
    for renumber in (True, False):
        got = base.updated(new, delete=gone, replace=rep, renumber=renumber, utf8=True)
        _same(got, sqlite_rows(rows_after(texts, new, gone, rep, renumber)))
        assert got.fallback_docs == []
    plain = base.updated(new, delete=gone, replace=rep)
    _same(plain, sqlite_rows(rows_after(texts, new, gone, rep, True)))
    assert plain.fallback_docs == [1, 2, 3]                          # the batch: rows 0 and 3 replaced, then the new texts


def test_resident_build_update_and_search():
    texts = ["café crème", "plain ascii crème", "naïve Ⱥ", "über straße", "e" + MARK + "t" + "e" + MARK, "", "CRÈME crème creme", "x"]
    spec, a = make_arrays(num_docs=len(texts), num_centroids=16, dim=32, nbits=2, doc_len_min=1, doc_len_max=1, seed=3)
    hx, ref = hip_index(a), hip_index(a)
    try:
        data = hx.build_text(texts, resident=True, utf8=True)
        assert data.resident and data.fallback_docs == []
        ref.set_text(TextIndexData.from_texts(texts))
        for k, v in ref.get_text_layout().items():
            assert hx.get_text_layout()[k].tobytes() == v.tobytes(), k
        new, gone, rep = ["Crème brûlée"], [1], {3: "ÜBER crème ⱥ"}
        data = hx.update_text(new, delete=gone, replace=rep, resident=True, utf8=True)
        assert data.resident and data.fallback_docs == []
        want = sqlite_rows(rows_after(texts, new, gone, rep, True))
        ref.set_text(want)
        assert data.terms == want.terms and hx.text_sizes() == ref.text_sizes()
        for k, v in ref.get_text_layout().items():
            assert hx.get_text_layout()[k].tobytes() == v.tobytes(), k
        _same(hx.get_text(), want)
        x, y = hx.text_search(["crème"], 8)[0], ref.text_search(["crème"], 8)[0]
        assert x.passage_ids.tobytes() == y.passage_ids.tobytes() and x.scores.tobytes() == y.scores.tobytes()
        assert sorted(x.passage_ids.tolist()) == [0, 2, 5, 7]
        # the handle's own setting serves the calls without an argument
        hx.text_utf8 = True
        data = hx.update_text(replace={6: "garçon"}, resident=True)
        assert data.fallback_docs == [] and "garcon" in data.vocab
    finally:
        hx.close()
        ref.close()


def test_identifier_aware_with_accented_identifiers():
    texts = ["HandlerStack café_crème naïveValue", "résuméParser x_é", "plain_ascii HTTPResponse", "été"]
    got = check(texts, "identifier_aware")
    assert "handlerstack" in got.vocab and "handler" in got.vocab and "caf" in got.vocab and "cafe" not in got.vocab
    assert TextIndexData.from_texts_device(texts, "identifier_aware").fallback_docs == []   # the expansion keeps ASCII identifiers only


def test_trigram_ignores_the_table():
    texts = ["abcdef", "café crème", "xyz", "ab"]
    a = TextIndexData.from_texts_device(texts, "trigram")
    b = check(texts, "trigram", fallback=[1])
    assert a.fallback_docs == [1] and a.terms == b.terms and a.inst_doc.tobytes() == b.inst_doc.tobytes()


def test_cpp_mirror_given_a_table_file(tmp_path):
    exe = str(tmp_path / "text_build_utf8")
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "cpp", "text_build_utf8.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    texts = ["café crème", "plain", "Ⱥ ⱥ e" + MARK, "\U00020000 beyond", "中文", ""]
    src, tab = tmp_path / "texts.txt", tmp_path / "unicode61.u32"
    src.write_bytes("\n".join(texts).encode("utf-8") + b"\n")
    T.unicode61_table(2).tofile(str(tab))
    r = subprocess.run([exe, str(src), str(tab)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "ascii_fallback 0 2 3 4" and lines[1] == "fallback 3"
    kept = list(texts)
    kept[3] = ""
    want = TextIndexData.from_texts(kept)
    assert [bytes.fromhex(t).decode() for t in lines[2].split()[1:]] == want.terms
    assert np.array_equal(np.asarray(lines[3].split()[1:], np.int64), want.term_offsets)
    assert np.array_equal(np.asarray(lines[4].split()[1:], np.int64), want.inst_doc)
    assert np.array_equal(np.asarray(lines[5].split()[1:], np.int64), want.inst_pos)
    assert int(lines[6].split()[1]) == len(texts)
