"""tests/textbuild_restate.py (the keyword-index build in plain Python) pinned to SQLite itself, shown to catch planted
defects, and the host logic of np_textbuild_plan.h (vocabulary sort, fallback merge, argument checks) held to it through a
stand-alone program.  CPU only; nothing here has a tolerance."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT

import textbuild_restate as R
from next_plaid_amd import api
from next_plaid_amd.text import TextIndexData


def _sqlite(texts, tokenizer):
    return R.of_data(TextIndexData.from_texts(texts, tokenizer))


def _raws(texts):
    return [t.encode("utf-8") for t in texts]


UNI = R.edge_corpus_unicode61() + R.random_ascii(11, 300, 60)
TRI = R.edge_corpus_trigram() + R.random_ascii(12, 300, 24, nul=False)


@pytest.fixture(scope="module")
def sqlite_unicode61():
    return _sqlite(UNI, "unicode61")


@pytest.fixture(scope="module")
def sqlite_trigram():
    return _sqlite(TRI, "trigram")


def test_unicode61_rules_equal_sqlite(sqlite_unicode61):
    got = R.build(_raws(UNI), "unicode61", max_token_bytes=32768)
    assert got["fallback_docs"] == []
    assert R.same(got, sqlite_unicode61)
    assert got["n_rows"] == len(UNI) and len(got["terms"]) > 50


def test_trigram_rules_equal_sqlite(sqlite_trigram):
    got = R.build(_raws(TRI), "trigram")
    assert got["fallback_docs"] == []
    assert R.same(got, sqlite_trigram)
    assert [len(R.trigram_tokens(b"x" * n)) for n in range(6)] == [0, 0, 0, 1, 2, 3]


def test_term_order_is_memcmp_shorter_first():
    got = R.build([b"ab a9 a10 a 0z 00"], "unicode61")
    assert got["terms"] == [b"00", b"0z", b"a", b"a10", b"a9", b"ab"]
    assert R.same(got, _sqlite(["ab a9 a10 a 0z 00"], "unicode61"))


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defects_are_caught(defect, sqlite_unicode61, sqlite_trigram):
    if defect == "trigram_past_end":
        assert not R.same(R.build(_raws(TRI), "trigram", defect=defect), sqlite_trigram)
    else:
        assert not R.same(R.build(_raws(UNI), "unicode61", max_token_bytes=32768, defect=defect), sqlite_unicode61), defect
    assert R.same(R.build(_raws(UNI), "unicode61", max_token_bytes=32768, defect=None), sqlite_unicode61)


def test_fallback_rule():
    assert R.is_fallback("café".encode(), "unicode61") and R.is_fallback("é".encode(), "trigram")
    assert not R.is_fallback(b"a\x00b", "unicode61") and R.is_fallback(b"a\x00b", "trigram")
    assert not R.is_fallback(b"x" * 8 + b" y", "unicode61", 8) and R.is_fallback(b"x" * 9 + b" y", "unicode61", 8)
    assert not R.is_fallback(b"x" * 256, "unicode61") and R.is_fallback(b"x" * 257, "unicode61")
    got = R.build([b"ok", "café ok".encode(), b"ok two"], "unicode61")
    assert got["fallback_docs"] == [1] and got["inst_doc"].tolist() == [0, 2, 2] and got["n_rows"] == 3


def _mixed():
    texts = R.random_ascii(13, 120, 40)
    for i in range(0, len(texts), 7):
        texts[i] = texts[i].replace("\x00", " ") + " naïve café ok über"
    return texts


def test_merge_of_fallback_documents_equals_sqlite():
    texts = _mixed()
    full = _sqlite(texts, "unicode61")
    dev = R.build(_raws(texts), "unicode61")
    assert dev["fallback_docs"] == list(range(0, len(texts), 7))
    added = R.restrict(full, dev["fallback_docs"])
    assert R.same(R.merge(dev, added), full)
    assert not R.same(dev, full)


# ---- np_textbuild_plan.h, stand-alone ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """tests/cpp/textbuild_plan_check.cpp built with the host compiler alone, plain and under ASan + UBSan; returns a
    function that runs one script through BOTH and returns the (identical) output lines."""
    d = tmp_path_factory.mktemp("tbplan")
    src = os.path.join(ROOT, "tests", "cpp", "textbuild_plan_check.cpp")
    exes = []
    for name, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = d / f"textbuild_plan_check_{name}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, src, "-o", str(exe)])
        exes.append(str(exe))

    def run(script: str):
        outs = []
        for exe in exes:
            r = subprocess.run([exe], input=script, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
            outs.append(r.stdout.splitlines())
        assert outs[0] == outs[1]
        return outs[0]
    return run


def _strs(terms):
    return " ".join(f"{len(t)} " + " ".join(str(c) for c in t) for t in terms)


def _parse_strs(tokens):
    out, i = [], 0
    while i < len(tokens):
        n = int(tokens[i])
        out.append(bytes(int(c) for c in tokens[i + 1: i + 1 + n]))
        i += 1 + n
    return out


def test_plan_vocabulary_sort_is_fts5vocab_order(plan_check):
    rng = np.random.default_rng(5)
    terms = {b"00", b"0z", b"a", b"a10", b"a9", b"ab", b"abc", b"abd", b"b", b"prefix1234", b"prefix12", b"z" * 40}
    while len(terms) < 400:
        terms.add(bytes(rng.choice(np.frombuffer(b"ab0z9", np.uint8), int(rng.integers(1, 9)))))
    terms = list(terms)
    rng.shuffle(terms)
    out = plan_check(f"SORT {len(terms)} {_strs(terms)}\nSORT 0\nSORT 1 1 97\n")
    ranks = [int(v) for v in out[0].split()[1:]]
    want = sorted(terms)
    assert [want[r] for r in ranks] == terms and sorted(ranks) == list(range(len(terms)))
    assert _parse_strs(out[1].split()[1:]) == want
    assert out[2].split() == ["ranks"] and out[4].split() == ["ranks", "0"]


def test_plan_sort_passes_and_table_size(plan_check):
    cases = [0, 1, 2, 255, 256, 257, 65535, 65536, 65537, 1 << 24, (1 << 24) + 1, (1 << 31) - 1]
    out = plan_check("".join(f"PASSES {n}\n" for n in cases))
    want = [0 if n <= 1 else (int(n - 1).bit_length() + 7) // 8 for n in cases]
    assert [int(l.split()[1]) for l in out] == want == [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 4]
    out = plan_check("BITS 0 0\nBITS 1 0\nBITS 1000 0\nBITS 1024 0\nBITS 100000000 0\nBITS 1000 2\n")
    assert [int(l.split()[1]) for l in out] == [10, 10, 11, 11, 26, 2]


def _args(tok=0, max_token=0, hash_bits=0, tile=0, ws=0, offs=(0, 3), have=1):
    return f"ARGS {tok} {max_token} {hash_bits} {tile} {ws} {len(offs) - 1} {' '.join(str(o) for o in offs)} {have}\n"


def test_plan_argument_checks(plan_check):
    cases = [(_args(), 0, ""), (_args(offs=(0,)), 0, ""), (_args(tok=1, max_token=32768, hash_bits=2, tile=16), 0, ""),
             (_args(tok=2), 8, "tokenizer 2"), (_args(tok=-1), 8, "tokenizer -1"),
             (_args(max_token=32769), 8, "max_token_bytes 32769"), (_args(max_token=-1), 8, "max_token_bytes -1"),
             (_args(hash_bits=32), 8, "hash_bits 32"), (_args(tile=24), 8, "tile_bytes 24"), (_args(tile=2048), 8, "tile_bytes 2048"),
             (_args(ws=-5), 8, "workspace_bytes"),
             (_args(offs=(1, 3)), 8, "offsets[0] is 1"), (_args(offs=(0, 5, 4)), 8, "offsets[2] = 4 after 5"),
             (_args(offs=(0, 3), have=0), 8, "bytes is NULL"), (_args(offs=(0, 0), have=0), 0, ""),
             (_args(offs=(0, (1 << 31) - 1)), 0, ""), (_args(offs=(0, 4, 4 + (1 << 31))), 3, "document 1 has 2147483648 bytes")]
    out = plan_check("".join(c[0] for c in cases))
    i = 0
    for script, rc, why in cases:
        assert out[i] == f"rc {rc}", (script, out[i], out[i + 1])
        assert why in out[i + 1], (script, out[i + 1])
        i += 3 if rc == 0 else 2
    assert plan_check(_args())[2] == "plan 256 1024 3"
    out = plan_check(f"INST {(1 << 31) - 1}\nINST {1 << 31}\n")
    assert out[0] == "rc 0" and out[2] == "rc 3" and "2147483648 instances" in out[3]


def _merge_script(a, b, fallback):
    ta, tb = a["terms"], b["terms"]
    b_term = np.repeat(np.arange(len(tb)), np.diff(b["term_offsets"]))
    j = lambda v: " ".join(str(int(x)) for x in v)
    return (f"MERGE {len(ta)} {_strs(ta)} {j(a['term_offsets'])} {a['inst_doc'].size} {j(a['inst_doc'])} {j(a['inst_pos'])} "
            f"{len(tb)} {_strs(tb)} {b['inst_doc'].size} {j(b_term)} {j(b['inst_doc'])} {j(b['inst_pos'])} "
            f"{len(fallback)} {j(fallback)}\n")


def _parse_merge(out):
    assert out[0] == "rc 0", out[:2]
    t = out[2].split()
    terms = _parse_strs(t[2:])
    assert len(terms) == int(t[1])
    ints = lambda l: np.asarray([int(v) for v in l.split()[1:]], np.int64)
    return dict(terms=terms, term_offsets=ints(out[3]), inst_doc=ints(out[4]), inst_pos=ints(out[5]).astype(np.int32))


def test_plan_merge_equals_restatement_and_sqlite(plan_check):
    texts = _mixed()
    full = _sqlite(texts, "unicode61")
    dev = R.build(_raws(texts), "unicode61")
    added = R.restrict(full, dev["fallback_docs"])
    got = _parse_merge(plan_check(_merge_script(dev, added, dev["fallback_docs"])))
    got["n_rows"] = len(texts)
    assert R.same(got, full) and R.same(got, R.merge(dev, added))
    # one side empty, either way
    empty = R.arrays([], len(texts))
    got = _parse_merge(plan_check(_merge_script(empty, added, dev["fallback_docs"])))
    got["n_rows"] = len(texts)
    assert R.same(got, added)
    got = _parse_merge(plan_check(_merge_script(dev, empty, [])))
    got["n_rows"] = len(texts)
    assert R.same(got, dev)


def test_plan_refuses_bad_added_instances(plan_check):
    dev = R.build([b"b d", "é".encode(), b"", "é".encode()], "unicode61")
    assert dev["fallback_docs"] == [1, 3]

    def added(inst):
        return R.arrays(inst, 4)

    good = added([(b"a", 1, 0), (b"a", 3, 2), (b"c", 1, 1)])
    assert plan_check(_merge_script(dev, good, [1, 3]))[0] == "rc 0"
    # a document that is not on the fallback list
    out = plan_check(_merge_script(dev, added([(b"a", 0, 0)]), [1, 3]))
    assert out[0] == "rc 8" and "document 0, which is not on the fallback list" in out[1]
    # (doc, pos) out of order inside a term, and a repeated instance
    for inst in ([(b"a", 3, 0), (b"a", 1, 0)], [(b"a", 1, 1), (b"a", 1, 0)], [(b"a", 1, 1), (b"a", 1, 1)]):
        a = added(sorted(inst))
        a["inst_doc"], a["inst_pos"] = (np.asarray([t[1] for t in inst], np.int64), np.asarray([t[2] for t in inst], np.int32))
        out = plan_check(_merge_script(dev, a, [1, 3]))
        assert out[0] == "rc 8" and "instances out of order" in out[1], out[:2]
    # terms out of memcmp order (the longer string first), and a term without an instance
    bad = added([(b"a", 1, 0), (b"ab", 1, 1)])
    bad["terms"] = [b"ab", b"a"]
    out = plan_check(_merge_script(dev, bad, [1, 3]))
    assert out[0] == "rc 8" and "terms out of order" in out[1]
    lone = added([(b"a", 1, 0)])
    lone["terms"], lone["term_offsets"] = [b"a", b"b"], np.asarray([0, 1, 1], np.int64)
    out = plan_check(_merge_script(dev, lone, [1, 3]))
    assert out[0] == "rc 8" and "term 1 has no instance" in out[1]


# ---- the ABI surface, as far as it goes without a device ---------------------------------------------------------------------
def test_entries_refuse_before_any_device_work():
    """The argument checks run before the device is touched: with or without a GPU they name the argument."""
    import ctypes as C
    L = api.lib()
    h = C.c_void_p()
    off = np.asarray([0, 3], np.int64)
    raw = np.frombuffer(b"abc", np.uint8)

    def call(o, offsets=off, data=raw):
        return L.np_hip_text_build(0, api._ptr(data), api._ptr(offsets), offsets.size - 1, C.byref(o), C.byref(h), None)

    assert call(api.np_text_build_opts(7)) == 8 and "tokenizer 7" in api.last_error()
    assert call(api.np_text_build_opts(0, 40000)) == 8 and "max_token_bytes 40000" in api.last_error()
    assert call(api.np_text_build_opts(0), np.asarray([0, 5, 3], np.int64)) == 8 and "offsets do not ascend" in api.last_error()
    assert call(api.np_text_build_opts(0), np.asarray([2, 3], np.int64)) == 8 and "offsets[0] is 2" in api.last_error()
    assert call(api.np_text_build_opts(0), np.asarray([0, 1 << 31], np.int64)) == 3 and "2^31 - 1" in api.last_error()
    tri = np.asarray([0, (1 << 31) - 1, (1 << 32) - 2], np.int64)    # 2 * (2^31 - 3) trigrams: refused before the text is read
    assert call(api.np_text_build_opts(1), tri) == 3 and "instances in one call" in api.last_error()
    assert h.value is None
    assert L.np_hip_text_build_fallback(None, None, None) == 8 and L.np_hip_text_build_sizes(None, None, None, None, None) == 8
    L.np_hip_text_build_free(None)


def test_text_module_imports_without_the_library():
    """text.py resolves the library lazily: it imports, and the SQLite path works, where no library can be loaded."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import next_plaid_amd.text as T\n"
            "assert hasattr(T.TextIndexData, 'from_texts_device')\n"
            "print(T.TextIndexData.from_texts(['a b'], 'unicode61').terms)\n") % os.path.join(ROOT, "next-plaid_amd")
    import sys
    env = dict(os.environ, NEXTPLAID_HIP_LIB="/nonexistent/libnextplaid_hip.so")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "['a', 'b']" in r.stdout, r.stdout + r.stderr
