"""np_hip_text_build_merge (the device keyword index kept current: append, delete, delete + renumber, replace) against
SQLite itself: every case compares base.updated(...) with the FTS5 table of the resulting rows, array for array.  The base
of a case comes from SQLite (from_texts) unless the case is about a base that the device built."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, synth

import next_plaid_amd as npa
from next_plaid_amd import api
from next_plaid_amd.text import TextIndexData

import textbuild_restate as R
from textbuild_limit_shapes import assert_same as _same, rows_after, sqlite_rows

pytestmark = pytest.mark.gpu

CHUNK = 2048   # NP_TB_SCAN_CHUNK: instances per block of a scan launch


def check(texts, new_texts=(), delete=(), replace=None, renumber=True, tokenizer="unicode61", base=None, fallback=(), **kw):
    base = TextIndexData.from_texts(texts, tokenizer) if base is None else base
    got = base.updated(new_texts, delete=delete, replace=replace, renumber=renumber, **kw)
    want = sqlite_rows(rows_after(texts, new_texts, delete, replace, renumber), tokenizer)
    _same(got, want)
    assert got.fallback_docs == list(fallback)
    rep = got.build_report
    assert rep["n_instances"] == got.inst_doc.size and rep["n_terms"] == got.n_terms and rep["n_rows"] == got.n_rows
    assert rep["n_base_instances"] == base.inst_doc.size and rep["n_old_docs"] == len(texts)
    assert rep["delta_uploaded"] == (1 if fallback or not (list(new_texts) or replace) else 0)
    return got


BASE = ["b c", "a b", "", "c c d", "b", "d a", "", "c"]


# ---- identity, empties and wholesale cases -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tokenizer", ["unicode61", "trigram"])
def test_identity_empties_and_wholesale(tokenizer):
    base = ["bcd cde", "abc bcd", "", "cde cde def", "bcd", "def abc", "", "cde"]
    for renumber in (True, False):
        got = check(base, renumber=renumber, tokenizer=tokenizer)                                 # identity
        assert got.build_report["n_terms_dropped"] == 0 and got.build_report["n_instances_dropped"] == 0
        check([], ["abc bcd", "", "bcd"], renumber=renumber, tokenizer=tokenizer)                 # empty base, a batch
        got = check([], renumber=renumber, tokenizer=tokenizer)                                   # empty base, empty batch
        assert got.n_terms == 0 and got.n_rows == 0 and got.term_offsets.tolist() == [0]
        got = check(base, delete=range(len(base)), renumber=renumber, tokenizer=tokenizer)        # delete everything
        assert got.n_terms == 0 and got.n_rows == 0
        check(base, ["xyz abc", "abc"], delete=range(len(base)), renumber=renumber, tokenizer=tokenizer)
        got = check(base, ["", "", ""], renumber=renumber, tokenizer=tokenizer)                   # a batch of empty documents
        assert got.n_rows == len(base) + 3 and got.terms == TextIndexData.from_texts(base, tokenizer).terms
    check(["", "", ""], ["", "ab"], delete=[1], tokenizer=tokenizer)


# ---- terms and the vocabulary ------------------------------------------------------------------------------------------------
def test_terms_die_are_reborn_and_arrive():
    texts = ["a m", "m", "m z", "k m", "m"]
    for renumber in (True, False):
        for dead, doc in (("a", 0), ("k", 3), ("z", 2)):        # the first, a middle and the last term of the vocabulary
            got = check(texts, delete=[doc], renumber=renumber)
            assert dead not in got.vocab and got.build_report["n_terms_dropped"] == 1
        got = check(texts, ["x a", "a"], delete=[0], renumber=renumber)      # dies in A, reborn in B
        assert "a" in got.vocab
        got = check(texts, replace={3: "m K"}, renumber=renumber)          # ... in the same row
        assert "k" in got.vocab
        got = check(texts, ["0 b zz", "l"], renumber=renumber)             # before the first, between two, after the last
        assert got.terms == ["0", "a", "b", "k", "l", "m", "z", "zz"]
        check(["ab abc", "abc"], ["a abcd", "ab"], renumber=renumber)      # a new term that is a prefix of an old one, and the reverse
        check(["a abcd", "ab"], ["ab abc", "abc"], delete=[1], renumber=renumber)


# ---- runs and scan chunks ----------------------------------------------------------------------------------------------------
def _run_corpus(lead):
    """One term, "m", whose run spans three scan chunks.  Every document holds it once, so a document's place in the run is
    its id -- up to document 2 * CHUNK - 2, which holds it four times, astride the second chunk edge.  `lead` instances of
    "a" in document 3 shift the run against the chunks of the scan over all instances."""
    n = 2 * CHUNK + 300
    texts = ["m"] * n
    texts[2 * CHUNK - 2] = "m m x m m"
    texts[3] = "a " * lead + "m"
    texts[7] = "m zz"
    return texts


@pytest.fixture(scope="module")
def run_bases():
    return {lead: (_run_corpus(lead), TextIndexData.from_texts(_run_corpus(lead))) for lead in (0, 5)}


@pytest.mark.parametrize("lead", [0, 5])
@pytest.mark.parametrize("renumber", [True, False])
def test_a_run_across_three_scan_chunks(run_bases, lead, renumber):
    texts, base = run_bases[lead]
    n = len(texts)
    assert base.term_offsets[base.vocab["m"] + 1] - base.term_offsets[base.vocab["m"]] == n + 3 > 2 * CHUNK
    # removed documents at positions 0, 2047, 2048 and 2049 of the run and at its last; a replaced one in the middle; new rows
    got = check(texts, ["m new", "q m m"], delete=[0, CHUNK - 1, CHUNK, CHUNK + 1, n - 1], replace={1000: "m other m"},
                renumber=renumber, base=base)
    assert got.build_report["n_instances_dropped"] == 6
    # batch ids below every survivor (row 0 replaced), between two adjacent survivors (1000) and above all (the new row);
    # the document with four instances astride the chunk edge stays, its neighbours go
    check(texts, ["m"], delete=[2 * CHUNK - 3, 2 * CHUNK - 1, 5], replace={0: "m m first", 1000: "mid m", n - 1: "last"},
          renumber=renumber, base=base)
    # that document itself is replaced, and removed
    check(texts, replace={2 * CHUNK - 2: "m"}, renumber=renumber, base=base)
    check(texts, delete=[2 * CHUNK - 2, 3], renumber=renumber, base=base)


# ---- delete and renumber -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokenizer", ["unicode61", "trigram"])
def test_delete_sets_with_and_without_renumbering(tokenizer):
    texts = [t.replace("\x00", " ") for t in R.random_ascii(71, 700, 40, nul=False)]
    base = TextIndexData.from_texts(texts, tokenizer)
    rng = np.random.default_rng(72)
    some = sorted(int(i) for i in rng.choice(len(texts), 90, replace=False))
    for delete in (some, range(0, len(texts), 2), range(1, len(texts), 2)):
        a = check(texts, delete=delete, renumber=True, tokenizer=tokenizer, base=base)
        b = check(texts, delete=delete, renumber=False, tokenizer=tokenizer, base=base)
        assert a.terms == b.terms and np.array_equal(a.term_offsets, b.term_offsets) and np.array_equal(a.inst_pos, b.inst_pos)
        assert a.n_rows == b.n_rows == len(texts) - len(list(delete))
    # a table with holes goes on: n_rows names its id space, ids stay
    holes = check(texts, delete=some, renumber=False, tokenizer=tokenizer, base=base)
    row = next(i for i in range(len(texts)) if i not in some)
    got = holes.updated(["tail row"], delete=[row], renumber=False, n_rows=len(texts))
    rows = rows_after(texts, delete=some, renumber=False)
    del rows[row]
    rows[len(texts)] = "tail row"
    _same(got, sqlite_rows(rows, tokenizer))


# ---- replace -----------------------------------------------------------------------------------------------------------------
def test_replace():
    texts = [t.replace("\x00", " ") for t in R.random_ascii(73, 300, 40, nul=False)]
    base = TextIndexData.from_texts(texts)
    for renumber in (True, False):
        same = check(texts, replace={i: texts[i] for i in (0, 17, 150, 299)}, renumber=renumber, base=base)    # the same text
        _same(same, base)
        check(texts, replace={0: "", 17: "", 299: ""}, renumber=renumber, base=base)                            # an empty text
        got = check(texts, replace={5: "entirelynew words here", 6: "zzzlast 000first"}, delete=[7], renumber=renumber, base=base)
        assert "entirelynew" in got.vocab and "zzzlast" in got.vocab


# ---- composition -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokenizer", ["unicode61", "trigram"])
def test_appending_batches_equals_the_whole_corpus(tokenizer):
    texts = [t.replace("\x00", " ") for t in R.random_ascii(74, 900, 50, nul=False)]
    cur = TextIndexData.from_texts_device([], tokenizer)
    for lo in range(0, len(texts), 250):                       # a base that was itself built range by range
        cur = cur.updated(texts[lo: lo + 250])
    _same(cur, TextIndexData.from_texts(texts, tokenizer))
    _same(cur, TextIndexData.from_texts_device(texts, tokenizer))


def test_two_runs_give_the_same_bytes():
    texts = [t.replace("\x00", " ") for t in R.random_ascii(75, 600, 50, nul=False)]
    base = TextIndexData.from_texts(texts)
    kw = dict(delete=range(0, 600, 3), replace={1: "one", 301: "two"})
    a, b = base.updated(texts[:50], **kw), base.updated(texts[:50], **kw)
    assert a.terms == b.terms
    for k in ("term_offsets", "inst_doc", "inst_pos"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes()


# ---- fallback ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokenizer", ["unicode61", "trigram"])
def test_batches_with_fallback_documents(tokenizer):
    for renumber in (True, False):
        check(BASE, ["naïve café ok", "plain abc", "über abc"], delete=[1], replace={4: "é b c"}, renumber=renumber, tokenizer=tokenizer,
              fallback=[0, 1, 3])                                  # the batch: row 4's text, then the three new ones
        check(BASE, ["café", "ünï abc"], replace={0: "b ç"}, renumber=renumber, tokenizer=tokenizer, fallback=[0, 1, 2])   # all fallback
    check(["café b", "b"], ["b"], delete=[1], tokenizer=tokenizer)   # a base with non-ASCII terms takes an ASCII batch


# ---- handle level ------------------------------------------------------------------------------------------------------------
def test_update_text_then_keyword_and_hybrid_search():
    spec = synth.SynthSpec(num_docs=300, num_centroids=64, dim=64, nbits=4, doc_len_min=4, doc_len_max=12, seed=9)
    a = synth.generate_arrays(spec)
    words = ["alpha", "beta", "gamma", "delta", "parse", "request", "Handler", "stack", "x1", "x2"]
    rng = np.random.default_rng(8)
    old = [" ".join(rng.choice(words, int(rng.integers(1, 9)))) for _ in range(310)]
    delete = list(range(3, 310, 31))                            # ten rows go, 300 stay: the index has 300 documents
    replace = {10: "alpha beta parse request café", 200: "gamma"}
    rows = rows_after(old, [], delete, replace, True)
    assert len(rows) == 300
    qs, _ = synth.make_queries(spec, 3, n_tokens=8, cen=a["centroids"])
    flat = ["alpha beta", '"parse request"', "gamma OR delta"]
    tree = ["alpha NOT beta", "(parse OR stack) AND req*", "gamma"]
    out, grew = [], []
    for update in (True, False):
        ix = npa.MmapIndex.from_arrays(a["centroids"], a["bucket_weights"], a["ivf"], a["ivf_lengths"], a["doc_lengths"],
                                       a["codes"], a["residuals"], a["nbits"], device=0)
        before = ix.info.device_bytes
        if update:
            data = ix.update_text(delete=delete, replace=replace, base=TextIndexData.from_texts(old))
            assert ix.text is data and data.fallback_docs == [0]
            with pytest.raises(ValueError, match="in both delete and replace"):
                ix.update_text(delete=[1], replace={1: "x"})
            with pytest.raises(ValueError, match="outside the table"):
                ix.update_text(delete=[300])
            assert ix.text is data                              # a refused call leaves the keyword index as it was
        else:
            data = TextIndexData.from_texts([rows[i] for i in range(300)])
            ix.set_text(data)
        grew.append(ix.info.device_bytes - before)
        p = npa.SearchParameters(n_full_scores=64, top_k=10, n_ivf_probe=4)
        out.append(ix.text_search(flat, top_k=10) + ix.search_hybrid(qs, flat, p) + ix.text_search(tree, top_k=10, full_grammar=True) +
                   ix.search_hybrid(qs, tree, p, full_grammar=True))
    assert grew[0] == grew[1] > 0
    for x, y in zip(*out):
        assert np.array_equal(x.passage_ids, y.passage_ids)
        assert np.asarray(x.scores).tobytes() == np.asarray(y.scores).tobytes()


# ---- errors and the other binding --------------------------------------------------------------------------------------------
def _merge(base, remap, delta=None, delta_ids=(), n_rows_out=None, device=0, workspace=0, terms=None):
    L, h, rep = api.lib(), C.c_void_p(), api.np_text_merge_report()
    enc = [t.encode() for t in (base.terms if terms is None else terms)]
    tbo = np.concatenate([[0], np.cumsum([len(t) for t in enc])]).astype(np.int64)
    tb = np.frombuffer(b"".join(enc) or b"\0", np.uint8)
    off, doc, pos = (np.ascontiguousarray(x) for x in (base.term_offsets, base.inst_doc, base.inst_pos))
    t = api.np_text_index(len(enc), off.ctypes.data, doc.ctypes.data, pos.ctypes.data, int(base.n_rows))
    remap, ids = np.asarray(remap, np.int64), np.asarray(delta_ids, np.int64)
    o = api.np_text_merge_opts(workspace)
    rc = L.np_hip_text_build_merge(device, C.byref(t), api._ptr(tb), api._ptr(tbo), api._ptr(remap), remap.size, delta,
                                   api._ptr(ids) if ids.size else None, len(remap) if n_rows_out is None else n_rows_out, C.byref(o),
                                   C.byref(h), C.byref(rep))
    if rc == 0:
        L.np_hip_text_build_free(h)
    else:
        assert h.value is None
    return rc, api.last_error(), rep


def test_refusals_name_the_argument():
    L = api.lib()
    base = TextIndexData.from_texts(["a b", "b c", "c a a"])
    ok = [0, 1, 2]
    assert _merge(base, ok)[0] == 0
    bad = TextIndexData.from_texts(["a b", "b c", "c a a"])
    bad.inst_pos = bad.inst_pos[::-1].copy()
    for args, kw, rc, why in (((bad, ok), {}, 8, "base: instance"), ((base, ok), {"terms": ["b", "a", "c"]}, 8, "base_term_bytes: terms out of order"),
                              ((base, [0, 1]), {}, 8, "document 2 is outside the index (the index is n_remap = 2"),
                              ((base, [1, 0, 2]), {}, 8, "remap[1] is 0 after 1"), ((base, [0, 0, 2]), {}, 8, "the survivors' ids must ascend strictly"),
                              ((base, ok), {"n_rows_out": 2}, 8, "n_rows_out 2 is below the 3 documents"),
                              ((base, ok), {"workspace": -1}, 8, "workspace_bytes -1 is negative"),
                              ((base, ok), {"workspace": 4096}, 7, "workspace of 4096 bytes does not hold the call")):
        got, msg, _ = _merge(*args, **kw)
        assert got == rc and why in msg and "np_hip_text_build_merge" in msg, (kw, msg)
    # the batch: not finalised, ids that do not ascend or name a survivor, another device
    raw, off = np.frombuffer(b"a dd", np.uint8), np.asarray([0, 1, 4], np.int64)
    o, d = api.np_text_build_opts(0), C.c_void_p()
    assert L.np_hip_text_build(0, api._ptr(raw), api._ptr(off), 2, C.byref(o), C.byref(d), None) == 0
    try:
        got, msg, _ = _merge(base, ok, d, [3, 4], 5)
        assert got == 8 and "delta is not finalised" in msg
        assert L.np_hip_text_build_sizes(d, None, None, None, None) == 0
        for ids, why in (([4, 3], "delta_ids[1] is 3 after 4"), ([3, 3], "must ascend strictly"), ([2, 3], "delta_ids[0] is 2, the id that remap[2] keeps"),
                         ([-1, 3], "a negative id")):
            got, msg, _ = _merge(base, ok, d, ids, 5)
            assert got == 8 and why in msg, msg
        got, msg, _ = _merge(base, ok, d, [3, 4], 4)
        assert got == 8 and "n_rows_out 4 is below the 5 documents" in msg
        got, msg, _ = _merge(base, ok, d, [3, 4], 5, device=1 if api.device_count() > 1 else 99)
        assert got == 8 and "delta was built on device 0" in msg
        # the workspace: what the report names passes, one byte less does not -- before any launch
        got, msg, rep = _merge(base, ok, d, [3, 4], 5)
        assert got == 0 and rep.workspace_bytes > 0 and rep.n_instances == 9 and rep.n_terms == 4 and rep.delta_uploaded == 0
        assert _merge(base, ok, d, [3, 4], 5, workspace=rep.workspace_bytes)[0] == 0
        got, msg, _ = _merge(base, ok, d, [3, 4], 5, workspace=rep.workspace_bytes - 1)
        assert got == 7 and "does not hold the call" in msg
        # a merge's result takes no further instances, and lists no fallback documents
        h, n = C.c_void_p(), C.c_int64(7)
        t = api.np_text_index(0, None, None, None, 0)
        assert L.np_hip_text_build_merge(0, C.byref(t), None, None, None, 0, d, api._ptr(np.asarray([0, 1], np.int64)), 2, None, C.byref(h), None) == 0
        try:
            assert L.np_hip_text_build_fallback(h, None, C.byref(n)) == 0 and n.value == 0
            assert L.np_hip_text_build_add(h, None, None, 0, None, None, None, 0) == 8 and "the sizes were read" in api.last_error()
        finally:
            L.np_hip_text_build_free(h)
    finally:
        L.np_hip_text_build_free(d)
    with pytest.raises(ValueError, match="needs a dense table"):
        base.updated(delete=[0], n_rows=5)
    with pytest.raises(ValueError, match="a table with holes needs n_rows"):
        TextIndexData("unicode61", ["a"], np.asarray([0, 1]), np.asarray([4]), np.asarray([0], np.int32), 2, {"a": 0}).updated()


def test_cpp_mirror_updates_the_same_index(tmp_path):
    exe = str(tmp_path / "text_update")
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "cpp", "text_update.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    texts = [t.replace("\n", " ").replace("\r", " ") for t in R.random_ascii(76, 200, 40, nul=False)]
    src = tmp_path / "texts.txt"
    src.write_bytes("\n".join(texts).encode("utf-8") + b"\n")
    delete, replace, new = [0, 5, 6, 199], {7: "seven new words", 100: ""}, ["appended one", "", "zz appended two"]
    hx = lambda s: s.encode().hex() or "-"
    for tokenizer in ("unicode61", "trigram"):
        for renumber in (1, 0):
            ops = tmp_path / "ops.txt"
            ops.write_text(f"{renumber} {len(delete)} {' '.join(map(str, delete))}\n{len(replace)} " +
                           " ".join(f"{k} {hx(v)}" for k, v in replace.items()) + f"\n{len(new)} " + " ".join(hx(t) for t in new) + "\n")
            r = subprocess.run([exe, str(src), tokenizer, str(ops)], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            lines = r.stdout.splitlines()
            got = dict(terms=[bytes.fromhex(t) for t in lines[0].split()[1:]], term_offsets=np.asarray(lines[1].split()[1:], np.int64),
                       inst_doc=np.asarray(lines[2].split()[1:], np.int64), inst_pos=np.asarray(lines[3].split()[1:], np.int64).astype(np.int32),
                       n_rows=int(lines[4].split()[1]))
            want = sqlite_rows(rows_after(texts, new, delete, replace, bool(renumber)), tokenizer)
            assert R.same(got, R.of_data(want)), (tokenizer, renumber)
            assert lines[5] == "refusals ok"
