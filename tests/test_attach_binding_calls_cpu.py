"""Both mirrors against recording stand-ins for the library: which entry keep_attachments= and rows= reach, the argument values,
the refusals that happen before the library or the directory is touched, and the order in which the keyword index is composed
around the keeping entries (update_text).  The C++ side: tests/cpp/attach_binding_check.cpp, under ASan + UBSan.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT

from next_plaid_amd import api, filters as F

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
GXX = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]


def test_entries_and_prototypes():
    L = api.lib()
    new = {"np_hip_index_remove_keep", "np_hip_index_append_rows", "np_hip_index_get_column", "np_hip_index_get_groups"}
    assert new <= set(api.EXPORTS) and all(hasattr(L, s) for s in new)
    assert L.np_hip_abi_version() == 6 == api.NP_ABI_VERSION   # new functions only: no struct changed
    assert L.np_hip_index_remove_keep.argtypes == L.np_hip_index_remove.argtypes
    hdr = open(os.path.join(ROOT, "include", "nextplaid_hip.h")).read()
    assert "int np_hip_index_remove_keep(np_index* index, const int64_t* doc_ids, int64_t n_ids, int64_t* out_removed);" in hdr
    assert "const int32_t* const* code_remap, const int32_t* new_groups, int64_t n_groups);" in hdr


def test_null_handles_are_refused_by_name():
    L = api.lib()
    out = C.c_int64(-5)
    assert L.np_hip_index_remove_keep(None, None, 0, C.byref(out)) == 8 and out.value == -5
    assert api.last_error() == "np_hip_index_remove_keep: index is NULL"
    assert L.np_hip_index_append_rows(None, None, 0, None, None, None, 0, None, None, 0) == 8
    assert api.last_error() == "np_hip_index_append_rows: index is NULL"
    assert L.np_hip_index_get_column(None, 0, None, None, None, None) == 8
    assert api.last_error() == "np_hip_index_get_column: index is NULL"
    assert L.np_hip_index_get_groups(None, None) == 8 and api.last_error() == "np_hip_index_get_groups: index is NULL"
    assert L.np_hip_index_remove(None, None, 0, None) == 8 and api.last_error() == "np_hip_index_remove: index is NULL"
    assert L.np_hip_index_append(None, None, 0, None, None) == 8 and api.last_error() == "np_hip_index_append: index is NULL"


class _Recorder:
    """stands in for the library: records the entries reached and their argument values"""

    def __init__(self, n_docs, groups=0, refuse=False):
        self.calls, self.n_docs, self.groups, self.refuse = [], n_docs, groups, refuse

    def np_hip_index_info(self, h, info):
        info._obj.num_documents = self.n_docs
        info._obj.shard_doc_end = self.n_docs
        info._obj.embedding_dim, info._obj.nbits = 8, 4
        return 0

    def np_hip_last_error(self):
        return b"Invalid argument: the stub said so"

    def np_hip_index_close(self, h):
        pass

    @staticmethod
    def _arr(ptr, n, ctype=C.c_int64):
        if ptr is None:
            return None
        ptr = ptr.value if isinstance(ptr, C.c_void_p) else ptr
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (n,)).tolist() if n else []

    def np_hip_index_remove(self, h, ids, n, out):
        self.calls.append(("remove", self._arr(ids, n), n, out is not None))
        return 0

    def np_hip_index_remove_keep(self, h, ids, n, out):
        self.calls.append(("remove_keep", self._arr(ids, n), n, out is not None))
        if self.refuse:
            return 8
        if out is not None:
            got = len({i for i in (self._arr(ids, n) or []) if 0 <= i < self.n_docs})
            out._obj.value = got
            self.n_docs -= got
        return 0

    def np_hip_index_delete(self, path, ids, n, out):
        self.calls.append(("delete", os.fsdecode(path), self._arr(ids, n), n))
        out._obj.value = len({i for i in self._arr(ids, n) if 0 <= i < 20})   # the directory holds 20 documents
        return 0

    def np_hip_index_group_count(self, h):
        self.calls.append(("group_count",))
        return self.groups

    def np_hip_index_append(self, h, lens, n, codes, res):
        self.calls.append(("append", self._arr(lens, n), n))
        return 0

    def np_hip_index_append_rows(self, h, lens, n, codes, res, cols, n_cols, remap, groups, n_groups):
        tables = None if remap is None else C.cast(remap, C.POINTER(C.c_void_p))
        seen = []
        for c in range(n_cols):
            t = cols[c].type
            ctype = {0: C.c_int64, 1: C.c_double, 2: C.c_int32}[t]
            seen.append((t, self._arr(cols[c].data, n, ctype), None if not cols[c].valid else self._arr(cols[c].valid, n, C.c_uint8),
                         None if tables is None or not tables[c] else self._arr(tables[c], self.remap_len, C.c_int32)))
        self.calls.append(("append_rows", self._arr(lens, n), n, seen, self._arr(groups, n, C.c_int32), n_groups))
        if self.refuse:
            return 8
        self.n_docs += n
        return 0

    def np_hip_index_set_column_text(self, h, column, text, off, n):
        self.calls.append(("set_column_text", column, n))
        return 0

    def np_hip_index_get_column(self, h, column, data, valid, typ, has):
        self.calls.append(("get_column", column))
        typ._obj.value, has._obj.value = self.col_type, self.col_has
        np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_int32)), (self.n_docs,))[:] = np.arange(self.n_docs)
        np.ctypeslib.as_array(C.cast(valid, C.POINTER(C.c_uint8)), (self.n_docs,))[:] = np.arange(self.n_docs) % 2
        return 0

    def np_hip_index_get_groups(self, h, out):
        self.calls.append(("get_groups",))
        np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int32)), (self.n_docs,))[:] = np.arange(self.n_docs) % 3
        return 0

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


OLD = {"year": [2001, 1999, None, 2010, 5], "lang": ["de", "fr", None, "de", "fr"], "tag": ["m", "m", "x", "q", "q"]}


class _Text:
    """stands in for a TextIndexData"""


def _handle(monkeypatch, rec, path="<arrays>", text=None, group_values=None):
    monkeypatch.setattr(api, "_lib", rec)
    hx = api.MmapIndex(C.c_void_p(1), path)
    hx.schema = F.make_schema(OLD, 5, text_on_device=["tag"])
    hx.text, hx.group_values = text, group_values
    composed = []
    monkeypatch.setattr(hx, "update_text", lambda **kw: (composed.append(kw), rec.calls.append(("update_text",)), setattr(hx, "text", "merged")))
    return hx, composed


# ---- remove ---------------------------------------------------------------------------------------------------------------------
def test_keep_attachments_reaches_the_keeping_entry(monkeypatch):
    rec = _Recorder(5, groups=3)
    base = _Text()
    hx, composed = _handle(monkeypatch, rec, text=base, group_values=["a", "b"])
    try:
        assert hx.remove_ids([3, 1, 3, -1, 9], keep_attachments=True) == 2 and hx.num_documents() == 3
        assert rec.calls == [("remove_keep", [3, 1, 3, -1, 9], 5, True), ("update_text",)]   # the entry first, then the keyword index
        assert len(composed) == 1 and composed[0]["base"] is base and composed[0]["renumber"] is True
        assert np.asarray(composed[0]["delete"]).tolist() == [1, 3]   # the ids the library acted on: in range, each once
        assert hx.text == "merged" and hx.group_values == ["a", "b"]
        sch = hx.schema   # the dictionaries stay, the row arrays shrink
        assert sch["lang"].dictionary == [b"de", b"fr"] and sch["tag"].dictionary == [b"m", b"q", b"x"] and sch["tag"].text_on_device
        assert sch["year"].data.tolist() == [2001, 0, 5] and sch["year"].valid.tolist() == [1, 0, 1]
        assert sch["lang"].data.tolist() == [0, 0, 1] and sch["tag"].data.tolist() == [0, 2, 1] and sch["tag"].valid is None
        # nothing in range: nothing changes, no keyword index is built
        rec.calls.clear()
        assert hx.remove_ids([77], keep_attachments=True) == 0 and hx.schema is sch and hx.text == "merged"
        assert rec.calls == [("remove_keep", [77], 1, True)]
        # the default is the dropping entry, as before
        rec.calls.clear()
        hx.remove_ids([0])
        assert rec.calls == [("remove", [0], 1, True)]
    finally:
        hx.close()


def test_keeping_remove_without_a_keyword_index_composes_nothing(monkeypatch):
    rec = _Recorder(5)
    hx, composed = _handle(monkeypatch, rec)
    try:
        assert hx.remove_ids([0], keep_attachments=True) == 1
        assert rec.calls == [("remove_keep", [0], 1, True)] and composed == [] and hx.text is None
    finally:
        hx.close()


def test_remove_on_a_directory_asks_the_keeping_entry_first(monkeypatch, tmp_path):
    (tmp_path / "metadata.json").write_text('{"num_documents": 20, "num_embeddings": 55}')
    rec = _Recorder(20)
    hx, _ = _handle(monkeypatch, rec, str(tmp_path))
    hx.schema = None
    try:
        assert hx.remove([4, 4, 19, 25], keep_attachments=True) == 2
        assert rec.calls == [("remove_keep", None, 0, False), ("delete", str(tmp_path), [4, 4, 19, 25], 4),
                             ("remove_keep", [4, 4, 19, 25], 4, True)]
        rec.calls.clear()   # the handle (18) against its directory's metadata (20, the stub rewrote nothing): refused, nothing called
        with pytest.raises(api.IndexLoadError, match="not current"):
            hx.remove([1], keep_attachments=True)
        assert rec.calls == []
    finally:
        hx.close()


# ---- append ---------------------------------------------------------------------------------------------------------------------
NEW = {"year": [None, 7], "lang": ["aa", "fr"], "tag": ["q", "m"]}
LENS, CODES, RES = [2, 1], [1, 2, 3], np.zeros((3, 4), np.uint8)


def test_rows_reach_the_entry_with_their_arrays(monkeypatch):
    rec = _Recorder(5, groups=3)
    rec.remap_len = 2
    base = _Text()
    hx, composed = _handle(monkeypatch, rec, text=base, group_values=["a", "b"])   # (the NULLs are the third group)
    try:
        ids = hx.append_arrays(LENS, CODES, RES, rows=api.AppendRows(columns=NEW, groups=["b", "zz"], texts=["one", "two"]))
        assert ids.tolist() == [5, 6] and hx.num_documents() == 7
        assert [c[0] for c in rec.calls] == ["group_count", "append_rows", "update_text"]   # 'lang' has no text on the device
        _, lens, n, cols, groups, n_groups = rec.calls[1]
        assert (lens, n) == (LENS, 2)
        assert cols[0] == (0, [0, 7], [0, 1], None)                      # year: the new rows alone, their validity bytes
        assert cols[1] == (2, [0, 2], None, [1, 2])                      # lang: coded against the merged dictionary, the remap
        assert cols[2] == (2, [1, 0], None, None)                        # tag: no string is new, no remap
        assert groups == [1, 3] and n_groups == 4                        # 'b' keeps its id, 'zz' takes the next one behind the NULLs
        assert hx.group_values == ["a", "b", None, "zz"]
        assert composed == [dict(new_texts=["one", "two"], base=base)]
        assert hx.schema["lang"].dictionary == [b"aa", b"de", b"fr"] and hx.schema["lang"].data.tolist() == [1, 2, 0, 1, 2, 0, 2]
        assert hx.schema["year"].valid.tolist() == [1, 1, 0, 1, 1, 0, 1]
    finally:
        hx.close()


def test_a_remap_of_a_device_text_column_sends_the_dictionary_again(monkeypatch):
    rec = _Recorder(5)
    rec.remap_len = 3
    hx, composed = _handle(monkeypatch, rec)
    try:
        hx.append_arrays(LENS, CODES, RES, rows=api.AppendRows(columns=dict(NEW, tag=["n", "x"])))
        assert [c[0] for c in rec.calls] == ["group_count", "append_rows", "set_column_text"]
        assert rec.calls[1][3][2] == (2, [1, 3], None, [0, 2, 3]) and rec.calls[1][4] is None and rec.calls[1][5] == 0
        assert rec.calls[2] == ("set_column_text", 2, 4) and composed == []
        # without rows the plain entry, the attachments dropped as before
        rec.calls.clear()
        hx.append_arrays(LENS, CODES, RES)
        assert rec.calls == [("append", LENS, 2)] and hx.schema is None
    finally:
        hx.close()


def test_refusals_before_the_library_is_touched(monkeypatch, tmp_path):
    rec = _Recorder(5, groups=2)
    hx, composed = _handle(monkeypatch, rec, text=_Text(), group_values=["a", "b"])
    sch = hx.schema
    rows = dict(columns=NEW, groups=["a", "a"], texts=["x", "y"])
    try:
        for bad, err, msg in [
            (dict(rows, texts=None), ValueError, "keyword index and rows.texts is None"),
            (dict(rows, texts=["x"]), api.ShapeError, "rows.texts has 1 entries for 2 new documents"),
            (dict(rows, columns=None), F.FilterError, "exactly the handle's columns"),
            (dict(rows, columns=dict(NEW, more=[1, 2])), F.FilterError, "not exactly the schema's"),
            (dict(rows, columns=dict(NEW, year=["x", "y"])), F.FilterError, "column 'year' has type 0, its new rows type 2"),
            (dict(rows, columns=dict(NEW, year=[1, 2, 3])), api.ShapeError, "entries"),
            (dict(rows, groups=None), ValueError, "the handle has groups and rows.groups is None"),
            (dict(rows, groups=["a"]), api.ShapeError, "rows.groups has 1 entries"),
            (dict(rows, groups=["a", 1.5]), ValueError, "a group key must be"),
            (dict(rows, groups=["a", 7]), ValueError, "all ints or all strings"),
        ]:
            rec.calls.clear()
            with pytest.raises(err, match=msg):
                hx.append_arrays(LENS, CODES, RES, rows=api.AppendRows(**bad))
            assert [c for c in rec.calls if c[0] != "group_count"] == [] and hx.schema is sch and composed == [], msg
        with pytest.raises(TypeError):
            hx.append_arrays(LENS, CODES, RES, rows=dict(rows))
        # the same checks run before append() touches its directory
        hx.path = str(tmp_path)
        (tmp_path / "metadata.json").write_text('{"num_documents": 5, "num_embeddings": 9}')
        rec.calls.clear()
        with pytest.raises(ValueError, match="rows.texts is None"):
            hx.append([np.zeros((2, 8), np.float32)] * 2, rows=api.AppendRows(columns=NEW, groups=["a", "a"]))
        assert rec.calls == []
        # the library's own refusal leaves the mirror's state alone
        rec.refuse = True
        rec.remap_len = 2
        with pytest.raises(ValueError, match="the stub said so"):
            hx.append_arrays(LENS, CODES, RES, rows=api.AppendRows(**rows))
        assert hx.schema is sch and hx.group_values == ["a", "b"] and composed == [] and hx.num_documents() == 5
    finally:
        hx.close()


def test_read_back_entries(monkeypatch):
    rec = _Recorder(5)
    rec.col_type, rec.col_has = 2, 1
    hx, _ = _handle(monkeypatch, rec)
    try:
        data, valid = hx.get_column("lang")
        assert rec.calls == [("get_column", 1)] and data.dtype == np.int32 and data.tolist() == [0, 1, 2, 3, 4] and valid.tolist() == [0, 1, 0, 1, 0]
        rec.col_has = 0
        assert hx.get_column("tag")[1] is None and rec.calls[-1] == ("get_column", 2)
        assert hx.get_groups().tolist() == [0, 1, 2, 0, 1]
        with pytest.raises(F.FilterError, match="unknown column 'nope'"):
            hx.get_column("nope")
        rec.col_type = 0
        with pytest.raises(api.NextPlaidError, match="has type 0 on the handle, 2 in the schema"):
            hx.get_column("lang")
    finally:
        hx.close()


def test_cpp_mirror_against_recording_stubs(tmp_path):
    """tests/cpp/attach_binding_check.cpp: next_plaid.hpp against recording stubs, with the host compiler alone, under ASan +
    UBSan"""
    exe, work = tmp_path / "attach_binding_check", tmp_path / "dir"
    work.mkdir()
    subprocess.check_call(GXX + SAN + [os.path.join(ROOT, "tests", "cpp", "attach_binding_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(work)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
