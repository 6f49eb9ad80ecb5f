"""What the two host bindings hand np_hip_text_build_merge for each of the crate's four operations, what they make of the
answer, and the refusals that happen before the library is touched -- without a device and without the library.  A fake
stands in for api._lib and records the values behind every pointer; the C++ mirror runs against recording stubs in
tests/cpp/textmerge_binding_check.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from next_plaid_amd import api, text as T

import textmerge_restate as M
from test_textbuild_binding_calls_cpu import FakeLib as BuildFake, rd, names, ROOT, MESSAGE

BATCH, RESULT = 0xB11D, 0xD0E5


class FakeLib(BuildFake):
    """test_textbuild_binding_calls_cpu's fake (its build is the batch) plus the merge, whose result is a second build."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.merged_rows = 0

    def np_hip_text_build_merge(self, device, base, tb, tbo, remap, n_remap, delta, ids, n_rows_out, opts, out, rep):
        b = base._obj
        o = rd(tbo, np.int64, b.n_terms + 1)
        s = rd(tb, np.uint8, o[-1]).tobytes()
        n = int(rd(b.term_offsets, np.int64, b.n_terms + 1)[-1])
        m = self.n_rows if delta else 0
        rc = self._note("np_hip_text_build_merge", device=device, terms=[s[o[i]: o[i + 1]] for i in range(b.n_terms)],
                        term_offsets=rd(b.term_offsets, np.int64, b.n_terms + 1).tolist(), inst_doc=rd(b.inst_doc, np.int64, n).tolist(),
                        inst_pos=rd(b.inst_pos, np.int32, n).tolist(), base_rows=b.n_rows, remap=rd(remap, np.int64, n_remap).tolist(),
                        delta=delta.value if delta else None, delta_ids=rd(ids, np.int64, m).tolist() if ids is not None else [], n_rows_out=n_rows_out,
                        workspace_bytes=opts._obj.workspace_bytes)
        if rc == 0:
            out._obj.value = RESULT
            rep._obj.n_instances, rep._obj.n_rows = 3, n_rows_out
            self.merged_rows = int(n_rows_out)
        return rc

    def np_hip_text_build_sizes(self, h, n_terms, n_bytes, n_inst, n_rows):
        if h.value == BATCH:
            assert n_terms is None and n_rows is None          # only finalised
            return self._note("np_hip_text_build_sizes(batch)")
        assert h.value == RESULT
        r = self.result
        n_terms._obj.value, n_bytes._obj.value = len(r["terms"]), sum(len(t) for t in r["terms"])
        n_inst._obj.value, n_rows._obj.value = len(r["inst_doc"]), self.merged_rows
        return self._note("np_hip_text_build_sizes")

    def np_hip_text_build_fetch(self, h, *a):
        assert h.value == RESULT
        h.value = BATCH
        try:
            return super().np_hip_text_build_fetch(h, *a)
        finally:
            h.value = RESULT


@pytest.fixture
def fake(monkeypatch):
    def install(**kw):
        f = FakeLib(**kw)
        monkeypatch.setattr(api, "_lib", f)
        return f
    return install


def base5():
    return T.TextIndexData.from_texts(["ab", "cd", "", "ab cd", "cd"])


WITH_BATCH = ["np_hip_text_build", "np_hip_text_build_fallback", "np_hip_text_build_sizes(batch)", "np_hip_text_build_merge",
              "np_hip_text_build_sizes", "np_hip_text_build_fetch", "np_hip_text_build_free", "np_hip_text_build_free"]
WITHOUT = ["np_hip_text_build_merge", "np_hip_text_build_sizes", "np_hip_text_build_fetch", "np_hip_text_build_free"]


def merge_call(f):
    return next(c[1] for c in f.calls if c[0] == "np_hip_text_build_merge")


def test_append(fake):
    f = fake()
    data = base5().updated(["zz", "", "zz ab"], device=2, max_token_bytes=99, hash_bits=5, merge_workspace_bytes=12345)
    assert names(f) == WITH_BATCH and [c[1]["handle"] for c in f.calls[-2:]] == [RESULT, BATCH]
    b, m = f.calls[0][1], merge_call(f)
    assert b["bytes"] == b"zzzz ab" and b["offsets"].tolist() == [0, 2, 2, 7] and (b["device"], b["max_token_bytes"], b["hash_bits"]) == (2, 99, 5)
    assert m["remap"] == [0, 1, 2, 3, 4] and m["delta_ids"] == [5, 6, 7] and m["n_rows_out"] == 8 and m["delta"] == BATCH
    assert m["terms"] == [b"ab", b"cd"] and m["term_offsets"] == [0, 2, 5] and m["inst_doc"] == [0, 3, 1, 3, 4] and m["inst_pos"] == [0, 0, 0, 1, 0]
    assert (m["device"], m["base_rows"], m["workspace_bytes"]) == (2, 5, 12345)
    assert data.terms == ["ab", "cd"] and data.n_rows == 8 and data.tokenizer == "unicode61" and data.fallback_docs == []
    assert data.term_offsets.tolist() == [0, 1, 3] and data.build_report["n_instances"] == 3 and data.vocab == {"ab": 0, "cd": 1}


def test_delete_with_and_without_renumbering(fake):
    f = fake()
    base5().updated(delete=[3, 1, 3], renumber=False)
    m = merge_call(f)
    assert names(f) == WITHOUT and m["delta"] is None and m["remap"] == [0, -1, 2, -1, 4] and m["delta_ids"] == [] and m["n_rows_out"] == 3
    f = fake()
    base5().updated(delete=[1, 3])
    assert names(f) == WITHOUT and merge_call(f)["remap"] == [0, -1, 1, -1, 2] and merge_call(f)["n_rows_out"] == 3


def test_replace_and_a_mix(fake):
    f = fake()
    base5().updated(replace={4: "four", 0: "zero"}, renumber=False)
    m = merge_call(f)
    assert names(f) == WITH_BATCH and f.calls[0][1]["bytes"] == b"zerofour"               # the replacements in id order
    assert m["remap"] == [-1, 1, 2, 3, -1] and m["delta_ids"] == [0, 4] and m["n_rows_out"] == 5
    f = fake()
    base5().updated(["tail"], delete=[1], replace=[(3, "three")])
    m = merge_call(f)
    assert f.calls[0][1]["bytes"] == b"threetail" and m["remap"] == [0, -1, 1, -1, 3] and m["delta_ids"] == [2, 4] and m["n_rows_out"] == 5
    for kw in (dict(delete=[1], replace={3: "x"}, n_new=1, renumber=True), dict(delete=[0, 4], replace={2: "x", 1: "y"}, n_new=2, renumber=False)):
        f = fake()
        base5().updated(["t"] * kw["n_new"], delete=kw["delete"], replace=kw["replace"], renumber=kw["renumber"])
        remap, ids, rows = M.plan_update(5, kw["delete"], kw["replace"], kw["n_new"], kw["renumber"])      # the restatement's plan
        m = merge_call(f)
        assert m["remap"] == remap.tolist() and m["delta_ids"] == ids.tolist() and m["n_rows_out"] == rows


def test_identifier_aware_and_trigram_batches(fake):
    f = fake()
    T.TextIndexData.from_texts(["x"], "identifier_aware").updated(["HandlerStack x"])
    assert f.calls[0][1]["bytes"] == b"handlerstack handler stack handler_stack x" and f.calls[0][1]["tokenizer"] == 0
    f = fake()
    T.TextIndexData.from_texts(["xyz"], "trigram").updated(["abc"])
    assert f.calls[0][1]["tokenizer"] == 1 and merge_call(f)["terms"] == [b"xyz"]


def test_fallback_documents_of_the_batch_are_added_once(fake):
    f = fake(fallback=[0, 2])
    data = base5().updated(["über ab", "cd"], replace={1: "café"})                     # the batch: café, über ab, cd
    assert names(f) == WITH_BATCH[:2] + ["np_hip_text_build_add"] + WITH_BATCH[2:]
    a = f.calls[2][1]
    assert a["terms"] == sorted(a["terms"]) == [b"cafe", b"cd"] and a["inst_doc"] == [0, 2]     # SQLite's own tokens (unicode61 strips the accent); ids index the batch
    assert data.fallback_docs == [0, 2]


def test_refused_before_the_library_is_touched(fake):
    f = fake()
    b = base5()
    for kw, why in ((dict(delete=[5]), "row 5 is outside the table's 5 row ids"), (dict(delete=[-1]), "row -1 is outside"),
                    (dict(replace={7: "x"}), "row 7 is outside"), (dict(delete=[2], replace={2: "x"}), "row 2 is in both delete and replace"),
                    (dict(replace=[(2, "x"), (2, "y")]), "replaced twice"), (dict(n_rows=4), "n_rows 4 is below the table's 5 rows"),
                    (dict(n_rows=9), "renumber=True needs a dense table")):
        with pytest.raises(ValueError, match=why):
            b.updated(**kw)
    sparse = T.TextIndexData("unicode61", ["a"], np.asarray([0, 1], np.int64), np.asarray([6], np.int64), np.asarray([0], np.int32), 2, {"a": 0})
    with pytest.raises(ValueError, match="a table with holes needs n_rows"):
        sparse.updated()
    assert f.calls == []
    sparse.updated(["t"], renumber=False, n_rows=8)                                    # holes: n_rows is the id space
    m = merge_call(f)
    assert m["remap"] == list(range(8)) and m["delta_ids"] == [8] and m["n_rows_out"] == 3 and m["base_rows"] == 2


def test_errors_release_both_builds(fake):
    f = fake(rc={"np_hip_text_build_merge": 8})
    with pytest.raises(ValueError, match="the fake said so"):
        base5().updated(["zz"])
    assert names(f)[-2:] == ["np_hip_text_build_merge", "np_hip_text_build_free"] and f.calls[-1][1]["handle"] == BATCH
    f = fake(rc={"np_hip_text_build_fetch": 7})
    with pytest.raises(MemoryError):
        base5().updated(["zz"])
    assert [c[1]["handle"] for c in f.calls[-2:]] == [RESULT, BATCH]
    f = fake(rc={"np_hip_text_build": 8})
    with pytest.raises(ValueError, match="the fake said so"):
        base5().updated(["zz"])
    assert names(f) == ["np_hip_text_build"]
    assert MESSAGE


def test_update_text_sets_the_handles_index(fake):
    f = fake()
    ix = object.__new__(api.MmapIndex)
    ix._h, ix._info = C.c_void_p(1), api.np_info()
    ix._info.device = 3
    ix.text = None
    with pytest.raises(ValueError, match="no keyword index and no base"):
        ix.update_text(["x"])
    kept = base5()
    data = ix.update_text(["zz"], delete=[0], base=kept)                               # the base kept from before update() / reload()
    assert merge_call(f)["device"] == 3 and f.calls[0][1]["device"] == 3
    assert names(f)[-1] == "np_hip_index_set_text" and ix.text is data
    assert f.calls[-1][1] == dict(n_terms=2, n_rows=5, term_offsets=[0, 1, 3])
    f.calls.clear()
    with pytest.raises(ValueError, match="in both"):
        ix.update_text(delete=[1], replace={1: "x"})                                   # base defaults to self.text
    assert f.calls == [] and ix.text is data
    ix.update_text(delete=[1])
    assert merge_call(f)["terms"] == [b"ab", b"cd"] and merge_call(f)["base_rows"] == 5


def test_cpp_mirror_reaches_the_same_entries(tmp_path):
    """tests/cpp/textmerge_binding_check.cpp: next_plaid.hpp against recording stubs, under ASan + UBSan."""
    exe = tmp_path / "textmerge_binding_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "textmerge_binding_check.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_entry_refuses_before_any_device_work():
    """The argument checks run before the device is touched: with or without a GPU they name the argument."""
    L = api.lib()
    h = C.c_void_p()
    off, doc, pos = np.asarray([0, 2], np.int64), np.asarray([0, 1], np.int64), np.asarray([0, 0], np.int32)
    tb, tbo = np.frombuffer(b"ab", np.uint8), np.asarray([0, 2], np.int64)

    def call(remap, n_rows_out=2, doc=doc, workspace=0):
        t = api.np_text_index(1, off.ctypes.data, doc.ctypes.data, pos.ctypes.data, 2)
        remap = np.asarray(remap, np.int64)
        o = api.np_text_merge_opts(workspace)
        return L.np_hip_text_build_merge(0, C.byref(t), api._ptr(tb), api._ptr(tbo), api._ptr(remap), remap.size, None, None, n_rows_out,
                                         C.byref(o), C.byref(h), None)

    assert call([1, 0]) == 8 and "remap[1] is 0 after 1" in api.last_error()
    assert call([0]) == 8 and "document 1 is outside the index (the index is n_remap = 1" in api.last_error()
    assert call([0, 1], 1) == 8 and "n_rows_out 1 is below the 2 documents" in api.last_error()
    assert call([0, 1], doc=np.asarray([1, 0], np.int64)) == 8 and "base: instance 1" in api.last_error()
    assert call([0, 1], workspace=100) == 7 and "workspace of 100 bytes does not hold the call" in api.last_error()
    assert h.value is None
    assert L.np_hip_text_build_merge(0, None, None, None, None, 0, None, None, 0, None, None, None) == 8 and "out_build is NULL" in api.last_error()
    assert L.np_hip_text_build_merge(0, None, None, None, None, 0, None, None, 0, None, C.byref(h), None) == 8 and "base is NULL" in api.last_error()
