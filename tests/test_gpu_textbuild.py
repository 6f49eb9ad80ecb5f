"""np_hip_text_build (the keyword index built on the device) against SQLite itself: every case compares
TextIndexData.from_texts_device with TextIndexData.from_texts on the same texts, array for array.  Wherever the corpus is pure
ASCII (NUL-free for trigram) fallback_docs == [] is asserted, so no case passes by sending its documents to SQLite."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, synth

import next_plaid_amd as npa
from next_plaid_amd import api
from next_plaid_amd.text import TextIndexData, compile_text_query

import textbuild_restate as R
from textbuild_limit_shapes import assert_same as _same

pytestmark = pytest.mark.gpu


def _reproducible(text, tokenizer):
    return all(ord(c) < 0x80 for c in text) and not (tokenizer == "trigram" and "\x00" in text)


def check(texts, tokenizer="unicode61", fallback=None, **kw):
    got = TextIndexData.from_texts_device(texts, tokenizer, **kw)
    _same(got, TextIndexData.from_texts(texts, tokenizer))
    if fallback is None and all(_reproducible(t, tokenizer) for t in texts):
        fallback = []
    if fallback is not None:
        assert got.fallback_docs == list(fallback)
    rep = got.build_report
    assert rep["n_docs"] == len(texts) and rep["n_fallback"] == len(got.fallback_docs)
    return got


# ---- document shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokenizer", ["unicode61", "trigram"])
def test_no_documents_and_empty_documents(tokenizer):
    got = check([], tokenizer)
    assert got.n_terms == 0 and got.term_offsets.tolist() == [0] and got.n_rows == 0
    got = check(["", "", ""], tokenizer)
    assert got.n_terms == 0 and got.n_rows == 3
    check(["", "alpha beta", "", "", "gamma alpha", "", ""], tokenizer)
    check(["  \t\n ", "!!! ...", "", "-"], tokenizer)
    check(["onlyonetokeninthewholedocument"], tokenizer)
    check(["x"], tokenizer)


def test_edge_corpora():
    check(R.edge_corpus_unicode61(), "unicode61")
    check(R.edge_corpus_trigram(), "trigram")


@pytest.mark.parametrize("tile", [16, 32, 64])
def test_tokens_at_and_across_tile_edges(tile):
    """Tokens that begin or end at tile_bytes - 1, tile_bytes and tile_bytes + 1 and straddle the edge, with the documents
    at every alignment to the 16-byte lines the walk loads (the documents are concatenated, so each lead shifts them)."""
    texts = []
    for lead in range(0, 17):
        for edge in (tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1):
            for tok in (1, 2, 3, tile, tile + 5, 3 * tile + 1):
                for start in (edge - tok, edge - tok + 1, edge - 1, edge):
                    if start < 0:
                        continue
                    texts.append("-" * start + "T" * tok + " z")           # ends / begins at the edge or straddles it
        texts.append("q" * lead)                                           # shifts every later document by one byte
    check(texts, "unicode61", tile_bytes=tile)
    check(texts, "trigram", tile_bytes=tile)
    check(texts[:200], "unicode61")


def test_every_ascii_byte_as_separator_and_in_tokens():
    seps = ["ab" + chr(c) + "cd" for c in range(0x80)]
    got = check(seps, "unicode61", tile_bytes=16)
    assert "ab" in got.vocab and "abacd" in got.vocab and "ab_cd" not in got.vocab
    check(["".join(chr(c) for c in range(0x80)), "".join(chr(c) * 2 for c in range(0x80))], "unicode61")
    check(["ab" + chr(c) + "cd" for c in range(1, 0x80)], "trigram", tile_bytes=16)
    check(["".join(chr(c) for c in range(1, 0x80))], "trigram")


# ---- tokens and terms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [8, None])
def test_token_of_exactly_the_cap_and_one_byte_more(cap):
    n = cap or 256
    texts = ["a " + "x" * n + " b", "ok", "a " + "x" * (n + 1) + " b", "y" * n, "y" * (n + 1), "-" * 7 + "z" * (n + 1)]
    got = check(texts, "unicode61", fallback=[2, 4, 5], max_token_bytes=cap, tile_bytes=16)
    assert "x" * n in got.vocab and "x" * (n + 1) in got.vocab
    assert got.build_report["n_instances"] == 3 + 1 + 1      # the fallback documents' instances are SQLite's


def test_prefix_terms_and_long_common_prefixes():
    base8, base16 = "abcdefgh", "abcdefghijklmnop"
    words = ["a", "ab", "abc", "abcd", base8, base8 + "1", base8 + "2", base8 + "12", base16, base16 + "x", base16 + "y",
             base16 + "xy", base16[:15], "A", "AB", "Abc", base8.upper() + "1"]
    rng = np.random.default_rng(3)
    texts = [" ".join(rng.choice(words, int(rng.integers(0, 12)))) for _ in range(300)]
    got = check(texts, "unicode61")
    assert got.n_terms == len({w.lower() for w in words})
    check(texts, "trigram")


def test_every_term_probes_and_a_full_table_is_retried():
    rng = np.random.default_rng(4)
    words = [f"w{i}" for i in range(40)]
    texts = [" ".join(rng.choice(words, 20)) for _ in range(50)]
    got = check(texts, "unicode61", hash_bits=2)
    assert got.build_report["table_retries"] > 0 and got.build_report["hash_bits"] >= 6 and got.n_terms == 40
    got = check(["aa bb cc", "bb aa", "cc"], "unicode61", hash_bits=2)      # three terms in four slots: probing, no retry
    assert got.build_report["table_retries"] == 0 and got.build_report["hash_bits"] == 2


@pytest.mark.parametrize("n_terms", [255, 256, 257, 65535, 65536, 65537])
def test_digit_boundaries_of_the_sort(n_terms):
    """Term ids 0 .. n_terms - 1 need 8, 9, 16 and 17 bits: one, two and three passes.  One document of decimal numbers,
    every number twice in two different orders."""
    rng = np.random.default_rng(n_terms)
    nums = np.arange(n_terms)
    doc = " ".join(str(int(v)) for v in np.concatenate([rng.permutation(nums), rng.permutation(nums)]))
    got = check([doc, "7 7 7"], "unicode61")
    assert got.n_terms == n_terms
    assert got.build_report["sort_passes"] == (int(n_terms - 1).bit_length() + 7) // 8


def test_one_term_across_many_sort_blocks_stays_in_document_order():
    rng = np.random.default_rng(6)
    texts = []
    for d in range(2000):
        words = ["the"] * 100
        for _ in range(3):
            words.insert(int(rng.integers(0, len(words))), f"rare{int(rng.integers(0, 5000))}")
        texts.append(" ".join(words))
    got = check(texts, "unicode61")
    t = got.vocab["the"]
    assert int(got.term_offsets[t + 1] - got.term_offsets[t]) == 200_000 and got.build_report["sort_passes"] == 2


# ---- trigram ------------------------------------------------------------------------------------------------------------------
def test_trigram_lengths_case_control_bytes_and_nul():
    got = check(["", "a", "ab", "abc", "abcd", "abcde"], "trigram")
    assert got.build_report["n_instances"] == 0 + 0 + 0 + 1 + 2 + 3
    got = check(["ABC abc AbC", "XYZ"], "trigram")
    assert "abc" in got.vocab and "ABC" not in got.vocab
    check(["a\tb\nc\rd\x01\x02\x1f\x7f e", "\x01\x02\x03"], "trigram")
    got = check(["abc", "ab\x00cd", "xyz"], "trigram", fallback=[1])
    assert got.build_report["n_instances"] == 2
    check(R.random_ascii(21, 400, 40, nul=False), "trigram")


# ---- fallback -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokenizer", ["unicode61", "trigram"])
def test_non_ascii_documents_go_to_the_fallback_list(tokenizer):
    texts = ["plain ascii", "école first", "last é", "é", "plain again", "Ünïcödé Straße", ""]
    got = check(texts, tokenizer, fallback=[1, 2, 3, 5])
    assert got.build_report["n_fallback"] == 4


@pytest.mark.parametrize("tokenizer", ["unicode61", "trigram"])
def test_mixed_corpus_goes_through_the_merge(tokenizer):
    texts = R.random_ascii(31, 1000, 50, nul=False)
    for i in range(0, len(texts), 7):
        texts[i] = texts[i] + " naïve café abc ab über ABC"
    check(texts, tokenizer, fallback=list(range(0, 1000, 7)))


def test_all_fallback_corpus():
    texts = ["é one", "two ü", "ß"]
    got = check(texts, "unicode61", fallback=[0, 1, 2])
    assert got.build_report["n_instances"] == 0 and got.n_terms > 0


def test_random_ascii_with_every_byte():
    check(R.random_ascii(41, 1500, 80), "unicode61")
    check(R.random_ascii(42, 300, 80), "unicode61", tile_bytes=16, hash_bits=3)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_build_text_then_keyword_and_hybrid_search():
    spec = synth.SynthSpec(num_docs=300, num_centroids=64, dim=64, nbits=4, doc_len_min=4, doc_len_max=12, seed=9)
    a = synth.generate_arrays(spec)
    words = ["alpha", "beta", "gamma", "delta", "parse", "request", "Handler", "stack", "x1", "x2"]
    rng = np.random.default_rng(8)
    texts = [" ".join(rng.choice(words, int(rng.integers(1, 9)))) for _ in range(300)]
    texts[5] += " café"
    qs, _ = synth.make_queries(spec, 3, n_tokens=8, cen=a["centroids"])
    tq = ["alpha beta", '"parse request"', "gamma OR delta"]
    out = []
    for build in (True, False):
        ix = npa.MmapIndex.from_arrays(a["centroids"], a["bucket_weights"], a["ivf"], a["ivf_lengths"], a["doc_lengths"],
                                       a["codes"], a["residuals"], a["nbits"], device=0)
        if build:
            data = ix.build_text(texts)
            assert data.fallback_docs == [5] and ix.text is data
        else:
            data = TextIndexData.from_texts(texts)
            ix.set_text(data)
        q = compile_text_query("alpha beta", data)
        assert q.n_phrases == 2 and all(t >= 0 for t in q.terms)
        kw = ix.text_search(tq, top_k=10)
        hy = ix.search_hybrid(qs, tq, npa.SearchParameters(n_full_scores=64, top_k=10, n_ivf_probe=4))
        out.append((kw, hy))
    for x, y in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        assert np.array_equal(x.passage_ids, y.passage_ids)
        assert np.asarray(x.scores).tobytes() == np.asarray(y.scores).tobytes()


def test_identifier_aware_runs_the_host_expansion_first():
    lines = ["fn parse_request(HandlerStack hs) { return hs.topFrame; }", "let HTTPResponse = getURL(x2);", "", "snake_case_name"]
    got = check(lines, "identifier_aware")
    assert got.fallback_docs == [] and got.tokenizer == "identifier_aware"
    assert all(t in got.vocab for t in ("handlerstack", "handler", "stack", "http", "geturl", "x2"))     # '_' separates again


# ---- other properties ---------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes():
    texts = R.random_ascii(51, 800, 60)
    a = TextIndexData.from_texts_device(texts, "unicode61")
    b = TextIndexData.from_texts_device(texts, "unicode61")
    c = TextIndexData.from_texts_device(texts, "unicode61", hash_bits=4, tile_bytes=48)
    for x in (b, c):
        assert x.terms == a.terms
        for k in ("term_offsets", "inst_doc", "inst_pos"):
            assert getattr(x, k).tobytes() == getattr(a, k).tobytes()


def _build(raw: bytes, offs, **kw):
    L, h = api.lib(), C.c_void_p()
    o = api.np_text_build_opts(kw.get("tokenizer", 0), kw.get("max_token_bytes", 0), kw.get("workspace_bytes", 0))
    data = np.frombuffer(raw, np.uint8)
    off = np.asarray(offs, np.int64)
    rc = L.np_hip_text_build(0, api._ptr(data), api._ptr(off), off.size - 1, C.byref(o), C.byref(h), None)
    return rc, h


def test_refusals_name_the_argument():
    L = api.lib()
    for kw, offs, rc, why in (({"tokenizer": 3}, [0, 3], 8, "tokenizer 3"), ({"max_token_bytes": 32769}, [0, 3], 8, "max_token_bytes 32769"),
                              ({}, [1, 3], 8, "offsets[0] is 1"), ({}, [0, 3, 2], 8, "offsets do not ascend"),
                              ({}, [0, 1 << 31], 3, "document 0 has 2147483648 bytes"),
                              ({"workspace_bytes": 64}, [0, 3], 7, "workspace of 64 bytes")):
        got, h = _build(b"abc", offs, **kw)
        assert got == rc and why in api.last_error() and h.value is None, (kw, offs, api.last_error())
    # a workspace that holds the documents but not the sort
    raw = b"a b c d e f g h " * 4096
    got, h = _build(raw, [0, len(raw)], workspace_bytes=len(raw) + 8192)
    assert got == 7 and "instances need" in api.last_error() and h.value is None
    # the fallback documents' instances: out of order, a document that is not on the list, twice, after the sizes
    raw = "ok é ok".encode()
    rc, h = _build(raw, [0, 2, 5, len(raw)])
    assert rc == 0
    try:
        n = C.c_int64()
        assert L.np_hip_text_build_fallback(h, None, C.byref(n)) == 0 and n.value == 1
        tb, tbo = np.frombuffer("é".encode(), np.uint8), np.asarray([0, 2], np.int64)

        def add(term, doc, pos):
            t, d, p = np.asarray(term, np.int32), np.asarray(doc, np.int64), np.asarray(pos, np.int32)
            return L.np_hip_text_build_add(h, api._ptr(tb), api._ptr(tbo), 1, api._ptr(t), api._ptr(d), api._ptr(p), t.size)

        assert add([0], [0], [0]) == 8 and "document 0, which is not on the fallback list" in api.last_error()
        assert add([0, 0], [1, 1], [1, 0]) == 8 and "instances out of order" in api.last_error()
        assert add([0], [1], [0]) == 0
        assert add([0], [1], [0]) == 8 and "added before" in api.last_error()
        nt = C.c_int64()
        assert L.np_hip_text_build_fetch(h, None, None, None, None, None) == 8 and "np_hip_text_build_sizes first" in api.last_error()
        assert L.np_hip_text_build_sizes(h, C.byref(nt), None, None, None) == 0 and nt.value == 2
    finally:
        L.np_hip_text_build_free(h)
    rc, h = _build(raw, [0, 2, 5, len(raw)])
    assert rc == 0
    try:
        assert L.np_hip_text_build_sizes(h, None, None, None, None) == 0
        t, d, p = np.asarray([0], np.int32), np.asarray([1], np.int64), np.asarray([0], np.int32)
        assert L.np_hip_text_build_add(h, api._ptr(tb), api._ptr(tbo), 1, api._ptr(t), api._ptr(d), api._ptr(p), 1) == 8
        assert "the sizes were read" in api.last_error()
    finally:
        L.np_hip_text_build_free(h)
    with pytest.raises(ValueError, match="no tokenize_fallback"):
        api.text_build(np.frombuffer(raw, np.uint8), [0, 2, 5, len(raw)], api.NP_TOK_UNICODE61)


def test_cpp_mirror_builds_the_same_index(tmp_path):
    exe = str(tmp_path / "text_build")
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "cpp", "text_build.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    texts = R.random_ascii(61, 200, 40, nul=False)
    texts = [t.replace("\n", " ").replace("\r", " ") for t in texts]
    texts[3] = "café ok"
    texts[9] = "über"
    src = tmp_path / "texts.txt"
    src.write_bytes("\n".join(texts).encode("utf-8") + b"\n")
    for tokenizer in ("unicode61", "trigram"):
        want = TextIndexData.from_texts(texts, tokenizer)
        fb = R.restrict(R.of_data(want), [3, 9])
        add = tmp_path / f"add_{tokenizer}.txt"
        b_term = np.repeat(np.arange(len(fb["terms"])), np.diff(fb["term_offsets"]))
        with open(add, "w") as f:
            f.write(f"{len(fb['terms'])}\n" + "".join(t.hex() + "\n" for t in fb["terms"]) + f"{b_term.size}\n" +
                    "".join(f"{int(t)} {int(d)} {int(p)}\n" for t, d, p in zip(b_term, fb["inst_doc"], fb["inst_pos"])))
        r = subprocess.run([exe, str(src), tokenizer, str(add)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert lines[0] == "fallback 3 9"
        got = dict(terms=[bytes.fromhex(t) for t in lines[1].split()[1:]],
                   term_offsets=np.asarray(lines[2].split()[1:], np.int64), inst_doc=np.asarray(lines[3].split()[1:], np.int64),
                   inst_pos=np.asarray(lines[4].split()[1:], np.int64).astype(np.int32), n_rows=int(lines[5].split()[1]))
        assert R.same(got, R.of_data(want)), tokenizer
