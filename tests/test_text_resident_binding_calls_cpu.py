"""What the two host bindings hand the resident keyword-index entries (np_hip_index_set_text_build, np_hip_index_text_merge) and in
which order, against a recording stand-in for the library: resident=True reaches build -> sizes -> set_text_build, and
merge -> set_text_build, and fetches no instance array; the defaults record exactly the sequences they recorded before; append
and remove go merge, vector call, install, and a refused vector call frees the merge's result.  No device, no library."""
import ctypes as C

import numpy as np
import pytest

from next_plaid_amd import api, text as T

from test_textbuild_binding_calls_cpu import FakeLib as BuildFake, rd, names, wr
from test_textmerge_binding_calls_cpu import FakeLib as MergeFake, BATCH, RESULT, WITH_BATCH, WITHOUT, base5

INDEX = 0x1D


class FakeLib(MergeFake):
    """The merge tests' fake plus the resident entries.  The handle's keyword index is `held`: the terms it holds."""

    def __init__(self, held=(b"ab", b"cd"), **kw):
        super().__init__(**kw)
        self.held = list(held)
        self.built = False

    def np_hip_text_build(self, *a):
        rc = super().np_hip_text_build(*a)
        self.built = True
        return rc

    def np_hip_text_build_sizes(self, h, n_terms, n_bytes, n_inst, n_rows):
        if n_terms is None and h.value != BATCH:                   # a fresh build, finalised before it is installed
            return self._note("np_hip_text_build_sizes(finalise)")
        if h.value == BATCH and n_terms is not None:               # the sizes of a build that was installed
            h = C.c_void_p(RESULT)
            self.merged_rows = self.n_rows
        return super().np_hip_text_build_sizes(h, n_terms, n_bytes, n_inst, n_rows)

    def np_hip_text_build_fetch(self, h, tb, tbo, toff, idoc, ipos):
        if toff is not None or idoc is not None or ipos is not None:     # the host path: the instance arrays cross the bus
            if h.value == BATCH:                                         # (a plain build: the build tests' fake)
                return BuildFake.np_hip_text_build_fetch(self, h, tb, tbo, toff, idoc, ipos)
            return super().np_hip_text_build_fetch(h, tb, tbo, toff, idoc, ipos)
        r = self.result
        wr(tb, np.frombuffer(b"".join(r["terms"]), np.uint8), np.uint8)
        wr(tbo, np.concatenate([[0], np.cumsum([len(t) for t in r["terms"]])]), np.int64)
        return self._note("np_hip_text_build_fetch(vocabulary)")

    def np_hip_index_set_text_build(self, ix, h):
        rc = self._note("np_hip_index_set_text_build", index=ix.value, build=h.value)
        if rc == 0:
            self.held = list(self.result["terms"])
        return rc

    def np_hip_index_text_sizes(self, ix, n_terms, n_post, n_inst, n_rows, n_docs):
        if n_terms is not None:
            n_terms._obj.value = len(self.held)
        return self._note("np_hip_index_text_sizes")

    def np_hip_index_text_merge(self, ix, tb, tbo, remap, n_remap, delta, ids, n_rows_out, opts, out, rep):
        o = rd(tbo, np.int64, len(self.held) + 1)
        s = rd(tb, np.uint8, o[-1]).tobytes()
        m = self.n_rows if delta else 0
        rc = self._note("np_hip_index_text_merge", index=ix.value, terms=[s[o[i]: o[i + 1]] for i in range(len(self.held))],
                        remap=rd(remap, np.int64, n_remap).tolist(), delta=delta.value if delta else None,
                        delta_ids=rd(ids, np.int64, m).tolist() if ids is not None else [], n_rows_out=n_rows_out)
        if rc == 0:
            out._obj.value = RESULT
            rep._obj.n_instances, rep._obj.n_rows = 3, n_rows_out
            self.merged_rows = int(n_rows_out)
        return rc

    # the vector calls
    def np_hip_index_remove_keep(self, ix, ids, n, out):
        rc = self._note("np_hip_index_remove_keep", n=n)
        if rc == 0 and out is not None:
            out._obj.value = n
        return rc

    def np_hip_index_append_rows(self, ix, dl, n, *a):
        return self._note("np_hip_index_append_rows", n=n)

    def np_hip_index_expand_rows(self, ix, cen, k_new, n_replace, dl, n, *a):
        return self._note("np_hip_index_expand_rows", k_new=k_new, n_replace=n_replace, n=n)


@pytest.fixture
def fake(monkeypatch):
    def install(**kw):
        f = FakeLib(**kw)
        monkeypatch.setattr(api, "_lib", f)
        return f
    return install


def handle(text=None, n_docs=5):
    ix = object.__new__(api.MmapIndex)
    ix._h, ix._info = C.c_void_p(INDEX), api.np_info()
    ix._info.device = 3
    ix._info.num_documents = n_docs
    ix._info.dim, ix._info.nbits = 8, 4
    ix.text, ix.schema, ix.group_values = text, None, None
    return ix


def resident5(ix):
    ix.text = T.ResidentTextIndexData("unicode61", ["ab", "cd"], 5, ix._text_fetcher())
    return ix.text


BUILD_RESIDENT = ["np_hip_text_build", "np_hip_text_build_fallback", "np_hip_text_build_sizes(batch)", "np_hip_index_set_text_build",
                  "np_hip_text_build_sizes", "np_hip_text_build_fetch(vocabulary)", "np_hip_text_build_free"]
MERGE_RESIDENT = ["np_hip_index_text_sizes", "np_hip_index_text_merge"]
INSTALL = ["np_hip_text_build_sizes(finalise)", "np_hip_index_set_text_build", "np_hip_text_build_sizes", "np_hip_text_build_fetch(vocabulary)",
           "np_hip_text_build_free"]


def test_build_text_resident_reaches_build_sizes_install_and_fetches_only_the_vocabulary(fake):
    f = fake()
    ix = handle()
    data = ix.build_text(["ab cd", "", "cd"], max_token_bytes=77, resident=True)
    assert names(f) == BUILD_RESIDENT
    b = f.calls[0][1]
    assert b["bytes"] == b"ab cdcd" and b["offsets"].tolist() == [0, 5, 5, 7] and (b["device"], b["max_token_bytes"], b["tokenizer"]) == (3, 77, 0)
    assert f.calls[3][1] == dict(index=INDEX, build=0xB11D)
    assert data is ix.text and data.resident and data.terms == ["ab", "cd"] and data.n_rows == 3 and data.vocab == {"ab": 0, "cd": 1}
    assert data.tokenizer == "unicode61" and data.fallback_docs == []
    assert T.compile_text_query("cd ab", data).phrases() == [[1], [0]]               # compiles without an instance array


def test_build_text_resident_adds_the_fallback_documents_once(fake):
    f = fake(fallback=[1])
    data = handle().build_text(["ab", "café", "cd"], resident=True)
    assert names(f) == BUILD_RESIDENT[:2] + ["np_hip_text_build_add"] + BUILD_RESIDENT[2:] and data.fallback_docs == [1]


def test_update_text_resident_reaches_merge_and_install(fake):
    f = fake()
    ix = handle()
    old = resident5(ix)
    data = ix.update_text(["zz", "ab"], delete=[1], replace={3: "three"}, resident=True)
    assert names(f) == ["np_hip_index_text_sizes", "np_hip_text_build", "np_hip_text_build_fallback", "np_hip_text_build_sizes(batch)",
                        "np_hip_index_text_merge", "np_hip_text_build_free"] + INSTALL
    m = next(c[1] for c in f.calls if c[0] == "np_hip_index_text_merge")
    assert f.calls[1][1]["bytes"] == b"threezzab" and f.calls[1][1]["device"] == 3
    assert m == dict(index=INDEX, terms=[b"ab", b"cd"], remap=[0, -1, 1, -1, 3], delta=BATCH, delta_ids=[2, 4, 5], n_rows_out=6)
    assert [c[1]["handle"] for c in f.calls if c[0] == "np_hip_text_build_free"] == [BATCH, RESULT]
    assert f.calls[-4][1] == dict(index=INDEX, build=RESULT)
    assert data is ix.text and data is not old and data.resident and data.n_rows == 6 and data.build_report["n_instances"] == 3
    with pytest.raises(ValueError, match="replaced by a later resident update"):
        old.inst_doc
    f.calls.clear()
    ix.update_text(delete=[0], renumber=False, resident=True)                        # no batch
    assert names(f) == MERGE_RESIDENT + INSTALL
    m = f.calls[1][1]
    assert m["delta"] is None and m["remap"] == [-1, 1, 2, 3, 4, 5] and m["delta_ids"] == [] and m["n_rows_out"] == 5


def test_refused_before_the_library_is_touched(fake):
    f = fake()
    ix = handle()
    with pytest.raises(ValueError, match="the handle has no keyword index"):
        ix.update_text(["x"], resident=True)
    resident5(ix)
    with pytest.raises(ValueError, match="base= is refused"):
        ix.update_text(["x"], base=base5(), resident=True)
    with pytest.raises(ValueError, match="row 2 is in both delete and replace"):
        ix.update_text(delete=[2], replace={2: "x"}, resident=True)
    with pytest.raises(ValueError, match="row 5 is outside the table's 5 row ids"):
        ix.update_text(delete=[5], resident=True)
    assert f.calls == []
    f.held = [b"ab"]                                                                 # the handle holds another vocabulary
    with pytest.raises(ValueError, match="base_term_byte_offsets describes 2 terms, the handle's keyword index holds 1"):
        ix.update_text(["x"], resident=True)
    assert names(f) == ["np_hip_index_text_sizes"]


def test_the_defaults_record_the_sequences_they_recorded_before(fake):
    f = fake()
    ix = handle()
    data = ix.build_text(["ab cd", "", "cd"])
    assert names(f) == ["np_hip_text_build", "np_hip_text_build_fallback", "np_hip_text_build_sizes", "np_hip_text_build_fetch",
                        "np_hip_text_build_free", "np_hip_index_set_text"]
    assert not data.resident and data.inst_doc.tolist() == [0, 0, 2]


def test_defaults_of_update_text_go_through_the_host_merge(monkeypatch):
    f = MergeFake()
    monkeypatch.setattr(api, "_lib", f)
    ix = handle(base5())
    data = ix.update_text(["zz"], delete=[0])
    assert names(f) == WITH_BATCH + ["np_hip_index_set_text"] and not data.resident
    f.calls.clear()
    ix.update_text(delete=[1])
    assert names(f) == WITHOUT + ["np_hip_index_set_text"]


def test_remove_goes_merge_vector_call_install(fake):
    f = fake()
    ix = handle()
    old = resident5(ix)
    assert ix.remove_ids([1, 3, 99], keep_attachments=True) == 3
    assert names(f) == MERGE_RESIDENT + ["np_hip_index_remove_keep"] + INSTALL
    assert f.calls[1][1]["remap"] == [0, -1, 1, -1, 2] and f.calls[1][1]["n_rows_out"] == 3 and f.calls[1][1]["delta"] is None
    assert ix.text is not old and ix.text.resident
    # a refused vector call frees the merge's result and keeps the old object
    f = fake(rc={"np_hip_index_remove_keep": 8})
    ix = handle()
    old = resident5(ix)
    with pytest.raises(ValueError, match="the fake said so"):
        ix.remove_ids([1], keep_attachments=True)
    assert names(f) == MERGE_RESIDENT + ["np_hip_index_remove_keep", "np_hip_text_build_free"] and f.calls[-1][1]["handle"] == RESULT
    assert ix.text is old
    # nothing to remove: no merge at all
    f = fake()
    ix = handle()
    old = resident5(ix)
    f.np_hip_index_remove_keep = lambda ix_, ids, n, out: f._note("np_hip_index_remove_keep", n=n)
    assert ix.remove_ids([77], keep_attachments=True) == 0 and names(f) == ["np_hip_index_remove_keep"] and ix.text is old


def test_append_goes_merge_vector_call_install(fake):
    f = fake()
    ix = handle()
    old = resident5(ix)
    dl, codes, res = np.asarray([1, 2], np.int64), np.zeros(3, np.int64), np.zeros((3, 4), np.uint8)
    ix.group_count = int   # (no groups: int() is 0)
    ids = ix.append_arrays(dl, codes, res, rows=api.AppendRows(texts=["zz", "ab zz"]))
    assert ids.tolist() == [5, 6]
    assert names(f) == ["np_hip_index_text_sizes", "np_hip_text_build", "np_hip_text_build_fallback", "np_hip_text_build_sizes(batch)",
                        "np_hip_index_text_merge", "np_hip_text_build_free", "np_hip_index_append_rows"] + INSTALL
    m = next(c[1] for c in f.calls if c[0] == "np_hip_index_text_merge")
    assert m["remap"] == [0, 1, 2, 3, 4] and m["delta_ids"] == [5, 6] and m["n_rows_out"] == 7
    assert ix.text is not old and ix.text.resident
    f = fake(rc={"np_hip_index_append_rows": 8})
    ix = handle()
    old = resident5(ix)
    ix.group_count = int   # (no groups: int() is 0)
    with pytest.raises(ValueError, match="the fake said so"):
        ix.append_arrays(dl, codes, res, rows=api.AppendRows(texts=["zz", "ab zz"]))
    assert names(f)[-2:] == ["np_hip_index_append_rows", "np_hip_text_build_free"] and f.calls[-1][1]["handle"] == RESULT
    assert ix.text is old


def test_expand_goes_merge_vector_call_install(fake):
    """expand_arrays(rows=), which update_resident calls in expansion mode: the new documents' texts only, the replaced keep theirs"""
    dl, codes, res = np.asarray([1, 2, 1], np.int64), np.zeros(4, np.int64), np.zeros((4, 4), np.uint8)
    cen = np.zeros((2, 8), np.float32)

    def ready(f):
        ix = handle()
        ix._info.embedding_dim = 8
        ix.group_count = int
        return ix, resident5(ix)

    f = fake()
    ix, old = ready(f)
    ids = ix.expand_arrays(cen, dl, codes, res, n_replace=1, rows=api.AppendRows(texts=["zz", "ab zz"]))
    assert ids.tolist() == [4, 5, 6]
    assert names(f) == ["np_hip_index_text_sizes", "np_hip_text_build", "np_hip_text_build_fallback", "np_hip_text_build_sizes(batch)",
                        "np_hip_index_text_merge", "np_hip_text_build_free", "np_hip_index_expand_rows"] + INSTALL
    m = next(c[1] for c in f.calls if c[0] == "np_hip_index_text_merge")
    assert m["remap"] == [0, 1, 2, 3, 4] and m["delta_ids"] == [5, 6] and m["n_rows_out"] == 7
    assert next(c[1] for c in f.calls if c[0] == "np_hip_index_expand_rows") == dict(k_new=2, n_replace=1, n=3)
    assert ix.text is not old and ix.text.resident
    with pytest.raises(ValueError, match="replaced by a later resident update"):
        old.inst_doc
    # a refused vector call frees the merge's result and keeps the old object
    f = fake(rc={"np_hip_index_expand_rows": 8})
    ix, old = ready(f)
    with pytest.raises(ValueError, match="the fake said so"):
        ix.expand_arrays(cen, dl, codes, res, n_replace=1, rows=api.AppendRows(texts=["zz", "ab zz"]))
    assert names(f)[-2:] == ["np_hip_index_expand_rows", "np_hip_text_build_free"] and f.calls[-1][1]["handle"] == RESULT
    assert ix.text is old
    # only replacements (no new document): no merge, as with a host keyword index
    f = fake()
    ix, old = ready(f)
    ix.expand_arrays(cen, dl[:1], codes[:1], res[:1], n_replace=1, rows=api.AppendRows(texts=[]))
    assert names(f) == ["np_hip_index_expand_rows"] and ix.text is old


def test_cpp_mirror_reaches_the_same_entries(tmp_path):
    """tests/cpp/textres_binding_check.cpp: next_plaid.hpp's build_text_resident / update_text_resident / get_text against
    recording stubs, a program of its own under ASan + UBSan."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "textres_binding_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(root, "tests", "cpp", "textres_binding_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
