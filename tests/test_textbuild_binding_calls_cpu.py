"""What the two host bindings hand np_hip_text_build and the calls after it, and what they make of the answer -- without a
device and without the library.  A fake stands in for api._lib and records, per entry, the values behind every pointer; the
C++ mirror runs against recording stubs in tests/cpp/textbuild_binding_check.cpp.  Checked: the entries reached and their
order, the bytes and offsets, the options, that the fallback documents are tokenised by the host (SQLite here) and added
once, the arrays read back, and that the build is released on every path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from next_plaid_amd import api, text as T

import textbuild_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE, MESSAGE = 0xB11D, "Invalid argument: the fake said so"


def rd(ptr, dtype, n):
    if ptr is None:
        return None
    addr = ptr if isinstance(ptr, int) else ptr.value
    if int(n) == 0:
        return np.zeros(0, dtype)
    assert addr, "a NULL pointer where entries are read"
    return np.frombuffer((C.c_char * (int(n) * np.dtype(dtype).itemsize)).from_address(addr), dtype).copy()


def wr(ptr, values, dtype):
    values = np.asarray(values, dtype).reshape(-1)
    if values.size:
        C.memmove(ptr.value, values.ctypes.data, values.nbytes)


class FakeLib:
    """The device's answer is chosen by the test: `fallback` ids and the `result` arrays the fetch writes."""

    def __init__(self, fallback=(), result=None, rc=None):
        self.calls, self.fallback, self.rc = [], list(fallback), dict(rc or {})
        self.result = result or dict(terms=[b"ab", b"cd"], term_offsets=[0, 1, 3], inst_doc=[0, 0, 2], inst_pos=[0, 1, 0])
        self.n_rows = 0

    def _note(self, name, **kw):
        self.calls.append((name, kw))
        return self.rc.get(name, 0)

    def np_hip_last_error(self):
        return MESSAGE.encode()

    def np_hip_text_build(self, device, raw, offs, n_docs, opts, out, rep):
        o = opts._obj
        off = rd(offs, np.int64, n_docs + 1)
        self.n_rows = int(n_docs)
        rc = self._note("np_hip_text_build", device=device, offsets=off, bytes=rd(raw, np.uint8, off[-1]).tobytes(),
                        tokenizer=o.tokenizer, max_token_bytes=o.max_token_bytes, workspace_bytes=o.workspace_bytes,
                        hash_bits=o.hash_bits, tile_bytes=o.tile_bytes)
        if rc == 0:
            out._obj.value = HANDLE
            rep._obj.n_docs, rep._obj.n_fallback, rep._obj.n_instances = n_docs, len(self.fallback), 3
        return rc

    def np_hip_text_build_fallback(self, h, ids, count):
        assert h.value == HANDLE
        wr(ids, self.fallback, np.int64)
        return self._note("np_hip_text_build_fallback")

    def np_hip_text_build_add(self, h, tb, tbo, n_terms, it, idoc, ipos, n):
        assert h.value == HANDLE
        o = rd(tbo, np.int64, n_terms + 1)
        b = rd(tb, np.uint8, o[-1]).tobytes()
        return self._note("np_hip_text_build_add", terms=[b[o[i]: o[i + 1]] for i in range(n_terms)],
                          inst_term=rd(it, np.int32, n).tolist(), inst_doc=rd(idoc, np.int64, n).tolist(),
                          inst_pos=rd(ipos, np.int32, n).tolist())

    def np_hip_text_build_sizes(self, h, n_terms, n_bytes, n_inst, n_rows):
        assert h.value == HANDLE
        r = self.result
        n_terms._obj.value, n_bytes._obj.value = len(r["terms"]), sum(len(t) for t in r["terms"])
        n_inst._obj.value, n_rows._obj.value = len(r["inst_doc"]), self.n_rows
        return self._note("np_hip_text_build_sizes")

    def np_hip_text_build_fetch(self, h, tb, tbo, toff, idoc, ipos):
        assert h.value == HANDLE
        r = self.result
        wr(tb, np.frombuffer(b"".join(r["terms"]), np.uint8), np.uint8)
        wr(tbo, np.concatenate([[0], np.cumsum([len(t) for t in r["terms"]])]), np.int64)
        wr(toff, r["term_offsets"], np.int64)
        wr(idoc, r["inst_doc"], np.int64)
        wr(ipos, r["inst_pos"], np.int32)
        return self._note("np_hip_text_build_fetch")

    def np_hip_text_build_free(self, h):
        self._note("np_hip_text_build_free", handle=h.value)

    # MmapIndex.set_text
    def np_hip_index_set_text(self, h, t):
        t = t._obj
        return self._note("np_hip_index_set_text", n_terms=t.n_terms, n_rows=t.n_rows,
                          term_offsets=rd(t.term_offsets, np.int64, t.n_terms + 1).tolist())

    def np_hip_index_info(self, h, info):
        return 0


@pytest.fixture
def fake(monkeypatch):
    def install(**kw):
        f = FakeLib(**kw)
        monkeypatch.setattr(api, "_lib", f)
        return f
    return install


def names(f):
    return [c[0] for c in f.calls]


def test_python_build_without_fallback(fake):
    f = fake()
    texts = ["ab cd", "", "cd"]
    data = T.TextIndexData.from_texts_device(texts, "unicode61", device=2, max_token_bytes=99, hash_bits=5, tile_bytes=32)
    assert names(f) == ["np_hip_text_build", "np_hip_text_build_fallback", "np_hip_text_build_sizes", "np_hip_text_build_fetch",
                        "np_hip_text_build_free"]
    b = f.calls[0][1]
    assert b["bytes"] == b"ab cdcd" and b["offsets"].tolist() == [0, 5, 5, 7] and b["device"] == 2
    assert (b["tokenizer"], b["max_token_bytes"], b["hash_bits"], b["tile_bytes"], b["workspace_bytes"]) == (0, 99, 5, 32, 0)
    assert f.calls[-1][1]["handle"] == HANDLE
    assert data.terms == ["ab", "cd"] and data.vocab == {"ab": 0, "cd": 1} and data.n_rows == 3 and data.tokenizer == "unicode61"
    assert data.term_offsets.tolist() == [0, 1, 3] and data.inst_doc.tolist() == [0, 0, 2] and data.inst_pos.tolist() == [0, 1, 0]
    assert data.term_offsets.dtype == np.int64 and data.inst_pos.dtype == np.int32
    assert data.fallback_docs == [] and data.build_report["n_docs"] == 3 and data.build_report["n_instances"] == 3
    assert data.term_ids("cd ab zz") == [1, 0, -1]


def test_python_fallback_documents_are_tokenised_by_sqlite_and_added_once(fake):
    f = fake(fallback=[1, 3])
    texts = ["ab cd", "x É é", "cd", "é"]
    data = T.TextIndexData.from_texts_device(texts)
    assert names(f) == ["np_hip_text_build", "np_hip_text_build_fallback", "np_hip_text_build_add", "np_hip_text_build_sizes",
                        "np_hip_text_build_fetch", "np_hip_text_build_free"]
    assert f.calls[0][1]["bytes"] == "ab cdx É écdé".encode() and f.calls[0][1]["max_token_bytes"] == 0
    a = f.calls[2][1]
    want = R.restrict(R.of_data(T.TextIndexData.from_texts(texts)), [1, 3])      # SQLite's own tokens of those two rows
    assert a["terms"] == want["terms"] and len(want["terms"]) == 2 and a["terms"] == sorted(a["terms"])
    assert a["inst_term"] == np.repeat(np.arange(2), np.diff(want["term_offsets"])).tolist()
    assert a["inst_doc"] == want["inst_doc"].tolist() == [1, 1, 3, 1] and a["inst_pos"] == want["inst_pos"].tolist()
    assert data.fallback_docs == [1, 3]


@pytest.mark.parametrize("tokenizer,code,sent", [("trigram", 1, b"HandlerStack x"),
                                                 ("identifier_aware", 0, b"handlerstack handler stack handler_stack x")])
def test_python_tokenizer_codes_and_identifier_expansion(fake, tokenizer, code, sent):
    f = fake()
    data = T.TextIndexData.from_texts_device(["HandlerStack x"], tokenizer)
    assert f.calls[0][1]["tokenizer"] == code and f.calls[0][1]["bytes"] == sent and data.tokenizer == tokenizer


def test_python_errors_and_release(fake):
    f = fake(rc={"np_hip_text_build": 8})
    with pytest.raises(ValueError, match="the fake said so"):
        T.TextIndexData.from_texts_device(["a"])
    assert names(f) == ["np_hip_text_build"]                  # no build came back: nothing to release
    f = fake(fallback=[0], rc={"np_hip_text_build_add": 8})
    with pytest.raises(ValueError, match="the fake said so"):
        T.TextIndexData.from_texts_device(["é"])
    assert names(f)[-2:] == ["np_hip_text_build_add", "np_hip_text_build_free"]
    f = fake(rc={"np_hip_text_build_fetch": 7})
    with pytest.raises(MemoryError):
        T.TextIndexData.from_texts_device(["a"])
    assert names(f)[-1] == "np_hip_text_build_free"
    f = fake(fallback=[0])
    with pytest.raises(ValueError, match="no tokenize_fallback"):
        api.text_build(np.frombuffer(b"ab", np.uint8), [0, 2], 0)
    assert names(f)[-1] == "np_hip_text_build_free" and "np_hip_text_build_add" not in names(f)
    with pytest.raises(ValueError, match="unknown tokenizer"):
        T.TextIndexData.from_texts_device(["a"], "porter")


def test_python_build_text_sets_the_handles_index(fake):
    f = fake()
    ix = object.__new__(api.MmapIndex)
    ix._h, ix._info = C.c_void_p(1), api.np_info()
    ix._info.device = 3
    data = ix.build_text(["ab cd", "", "cd"], tokenizer="unicode61")
    assert names(f)[0] == "np_hip_text_build" and f.calls[0][1]["device"] == 3
    assert names(f)[-1] == "np_hip_index_set_text" and ix.text is data
    assert f.calls[-1][1] == dict(n_terms=2, n_rows=3, term_offsets=[0, 1, 3])


def test_cpp_mirror_reaches_the_same_entries(tmp_path):
    """tests/cpp/textbuild_binding_check.cpp: next_plaid.hpp against recording stubs, with the host compiler alone and under
    ASan + UBSan (an array the header sized too small is an error there)."""
    exe = tmp_path / "textbuild_binding_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "textbuild_binding_check.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
