"""text.unicode61_table and the three-class model built from it (tests/textbuild_utf8_restate.py) against SQLite itself, the
planted defects, and the table check of np_textbuild_plan.h as a stand-alone program under ASan + UBSan.  No device."""
import os
import subprocess

import numpy as np
import pytest

from next_plaid_amd import text as T

import textbuild_utf8_restate as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    return U.Model(2)


def test_table_shape_classes_and_ascii_rule(model):
    t = T.unicode61_table(2)
    assert t.dtype == np.uint32 and t.shape == (2 * 65536,) and not t.flags.writeable
    assert T.unicode61_table(2) is t                                   # cached per process
    assert np.array_equal(T.unicode61_table(1), t[:65536])
    cls, fold = t >> 30, t & T.UNICODE_FOLD_MASK
    assert int(cls.max()) == 2 and not (t & ~np.uint32(0xC01FFFFF)).any()
    assert t[0] == 0 and not t[0xD800:0xE000].any()                    # code point 0 and the surrogates separate
    for c in range(128):
        ch = chr(c)
        want = (1 << 30) | ord(ch.lower()) if (ch.isascii() and ch.isalnum()) else 0
        assert int(t[c]) == want, hex(c)
    tok = cls == 1
    assert (fold[tok] < 0x110000).all() and not ((fold[tok] >= 0xD800) & (fold[tok] < 0xE000)).any()
    assert not fold[cls == 0].any() and not fold[cls == 2].any()
    # a fold is never more than one byte longer than its source (2 -> 3 is the longest: U+023A -> U+2C65)
    blen = lambda a: 1 + (a >= 0x80) + (a >= 0x800) + (a >= 0x10000)
    cps = np.arange(t.size)
    assert (blen(fold[tok]) <= blen(cps[tok]) + 1).all()
    assert int(fold[0x23A]) == 0x2C65 and int(fold[0xC9]) == ord("e") and int(cls[0x301]) == 2
    assert set(T.unicode61_probe_seconds) >= {0, 1} and all(v > 0 for v in T.unicode61_probe_seconds.values())
    with pytest.raises(ValueError, match="planes 18"):
        T.unicode61_table(18)


@pytest.mark.parametrize("plane", [0, 1])
@pytest.mark.parametrize("form", ["x?y", "?y", "x?"])
def test_model_equals_sqlite_on_every_code_point(model, plane, form):
    cps = [cp for cp in range(plane * 65536, (plane + 1) * 65536) if cp != 0 and not 0xD800 <= cp < 0xE000]
    texts = [form.replace("?", chr(cp)) for cp in cps]
    got = U.sqlite_terms(texts)
    bad = [(hex(cp), s, model.terms(t)) for cp, t, s in zip(cps, texts, got) if model.terms(t) != s]
    assert not bad, bad[:10]


def test_model_equals_sqlite_on_random_strings(model):
    texts = U.random_strings(20000, 61, model)
    got = U.sqlite_terms(texts)
    bad = [(t, s, model.terms(t)) for t, s in zip(texts, got) if model.terms(t) != s]
    assert not bad, bad[:5]
    kinds = {model.cls[ord(ch)] for t in texts for ch in t}
    assert kinds == {0, 1, 2} and any(ord(ch) >= 0x10000 for t in texts for ch in t)
    assert any(len(model.tokens(t)) > 3 for t in texts)


# one document per defect on which the right model equals SQLite and the defective one does not
PLANTED = {
    "mark_starts_token": "́ a",
    "mark_after_separator_continues": "a, ́ b",
    "fold_not_applied": "Été",
    "continuation_byte_on_its_own": "café 中",
}


@pytest.mark.parametrize("defect", U.DEFECTS)
def test_each_planted_defect_changes_an_answer(model, defect):
    assert set(PLANTED) | {"cap_on_folded_bytes"} == set(U.DEFECTS) and len(U.DEFECTS) >= 5
    if defect == "cap_on_folded_bytes":
        doc = "ÀÀÀ b"                 # six raw bytes that fold to "aaa"
        assert model.terms(doc) == U.sqlite_terms([doc])[0] == ["aaa", "b"]
        assert model.overlong(doc, 5) and not model.overlong(doc, 6)
        assert not model.overlong(doc, 5, defect)  # the defect keeps on the device a document the kernel hands back
        assert U.predict_fallback([doc.encode()], 2, 5, model) == [0]
        return
    doc = PLANTED[defect]
    want = U.sqlite_terms([doc])[0]
    assert model.terms(doc) == want
    assert model.terms(doc, defect) != want
    for other, d in PLANTED.items():               # the defects are distinct: each leaves the others' documents alone or not,
        if other != defect:                        # but the right model is right on all of them
            assert model.terms(d) == U.sqlite_terms([d])[0]


def test_predicted_fallback_list(model):
    raws = [b"plain", "café".encode(), b"\x80x", b"\xc0\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"ab\xc3", b"\xf8\x88\x80\x80\x80",
            "\U00020000".encode(), "\U0001F600 ok".encode(), ("é" * 129).encode(), ("é" * 128).encode()]
    assert U.predict_fallback(raws, 2, 256, model) == [2, 3, 4, 5, 6, 7, 8, 10]
    assert U.predict_fallback(raws, 3, 256, U.Model(3)) == [2, 3, 4, 5, 6, 7, 10]


def test_table_check_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/textbuild_utf8_table_check.cpp: textbuild_check_table rejects every malformed table of the header's list,
    naming the argument; a program of its own with the host compiler, plain and under ASan + UBSan."""
    src = os.path.join(ROOT, "tests", "cpp", "textbuild_utf8_table_check.cpp")
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / f"table_check_{name}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, src, "-o", str(exe)])
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
