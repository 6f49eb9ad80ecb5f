"""What the two host bindings put into np_text_build_opts.unicode_table -- without a device and without the library.  The
fakes of the build, merge and resident binding tests stand in for api._lib and note the table of every np_hip_text_build;
the C++ mirror runs against recording stubs in tests/cpp/textbuild_utf8_binding_check.cpp.  utf8=False (the default) is a
NULL table through every entry, utf8=True the pointer and length of text.unicode61_table(planes); the ABI version and the
struct sizes are what they were."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from next_plaid_amd import api, text as T

from test_textbuild_binding_calls_cpu import FakeLib as BuildFake, ROOT, names
from test_textmerge_binding_calls_cpu import FakeLib as MergeFake, base5
from test_text_resident_binding_calls_cpu import FakeLib as ResidentFake, handle, resident5


class Tables:
    """Notes (pointer, length, the reserved word) of every np_hip_text_build, and that the table is readable then."""

    def np_hip_text_build(self, device, raw, offs, n_docs, opts, out, rep):
        o = opts._obj
        if o.unicode_table:
            head = np.frombuffer((C.c_char * 512).from_address(o.unicode_table), np.uint32)
            assert int(head[ord("A")]) == (1 << 30) | ord("a") and int(head[ord(" ")]) == 0
        SEEN.append((o.unicode_table, int(o.unicode_table_len), int(o.reserved[0])))
        return super().np_hip_text_build(device, raw, offs, n_docs, opts, out, rep)


SEEN = []   # across the fakes of one test


class PlainFake(Tables, BuildFake):      # a build that is read back
    pass


class HostFake(Tables, MergeFake):       # a batch that is merged on the host path
    pass


class HbmFake(Tables, ResidentFake):     # the resident entries
    pass


@pytest.fixture
def use(monkeypatch):
    SEEN.clear()

    def install(cls):
        f = cls()
        monkeypatch.setattr(api, "_lib", f)
        return f
    return install


NULL = (None, 0, 0)


def table(planes=2):
    t = T.unicode61_table(planes)
    return (t.ctypes.data, planes * 65536, 0)


RAW, OFF = np.frombuffer("café".encode(), np.uint8), [0, 5]


def test_abi_version_and_struct_sizes_are_unchanged():
    assert C.sizeof(api.np_text_build_opts) == 48 and C.sizeof(api.np_text_build_report) == 136
    assert C.sizeof(api.np_text_merge_opts) == 32
    o = api.np_text_build_opts
    assert (o.unicode_table.offset, o.unicode_table_len.offset, o.reserved.offset, o.reserved.size) == (24, 32, 40, 8)
    header = open(os.path.join(ROOT, "include", "nextplaid_hip.h")).read()
    assert re.search(r"#define\s+NP_ABI_VERSION\s+6\b", header)
    assert api.np_text_build_opts(0).unicode_table is None                     # the default options: a NULL table


def test_build_entries_pass_null_by_default_and_the_table_with_utf8(use):
    use(PlainFake)
    T.TextIndexData.from_texts_device(["café"])
    T.TextIndexData.from_texts_device(["café"], "identifier_aware")
    api.text_build(RAW, OFF, 0)
    assert SEEN == [NULL] * 3
    SEEN.clear()
    T.TextIndexData.from_texts_device(["café"], utf8=True)
    T.TextIndexData.from_texts_device(["café"], "identifier_aware", utf8=True, unicode_planes=1)
    T.TextIndexData.from_texts_device(["café"], "trigram", utf8=True)           # handed on; the library ignores it
    api.text_build(RAW, OFF, 0, utf8=True)
    api.text_build(RAW, OFF, 0, utf8=True, unicode_planes=3)
    assert SEEN == [table(), table(1), table(), table(), table(3)]


def test_merge_entries_pass_null_by_default_and_the_table_with_utf8(use):
    use(HostFake)
    b = base5()
    n = int(b.n_rows)
    merge = lambda **kw: api.text_merge([t.encode() for t in b.terms], b.term_offsets, b.inst_doc, b.inst_pos, n, np.arange(n), [n],
                                        n + 1, RAW, OFF, 0, **kw)
    b.updated(["zz"])
    merge()
    assert SEEN == [NULL] * 2
    SEEN.clear()
    b.updated(["zz"], utf8=True)
    b.updated(replace={1: "é"}, utf8=True, unicode_planes=3)
    merge(utf8=True, unicode_planes=1)
    assert SEEN == [table(), table(3), table(1)]
    SEEN.clear()
    b.updated(delete=[1], utf8=True)                                            # no batch: nothing is tokenised
    assert SEEN == []


def test_handle_entries_host_keyword_index(use):
    ix = handle()
    use(PlainFake)
    ix.build_text(["café"])
    ix.build_text(["café"], utf8=True)
    use(HostFake)
    ix.text = base5()
    ix.update_text(["zz"])
    ix.update_text(["zz"], utf8=True, unicode_planes=1)
    ix.update_text(["zz"])                                                       # an argument is the call's, not the handle's
    assert SEEN == [NULL, table(), NULL, table(1), NULL]
    SEEN.clear()
    ix.text_utf8, ix.text_unicode_planes = True, 3                               # the handle's own setting
    use(PlainFake)
    ix.build_text(["café"])
    use(HostFake)
    ix.text = base5()
    ix.update_text(["zz"])
    ix.update_text(["zz"], utf8=False)
    assert SEEN == [table(3), table(3), NULL]
    assert api.MmapIndex.text_utf8 is False and api.MmapIndex.text_unicode_planes == 2


def test_handle_entries_resident_keyword_index(use):
    use(HbmFake)
    ix = handle()
    ix.build_text(["café"], resident=True)
    resident5(ix)
    ix.update_text(["zz"], resident=True)
    assert SEEN == [NULL] * 2
    SEEN.clear()
    ix.build_text(["café"], resident=True, utf8=True)
    resident5(ix)
    ix.update_text(["zz"], replace={1: "é"}, resident=True, utf8=True, unicode_planes=1)
    assert SEEN == [table(), table(1)]


def test_append_expand_and_remove_take_the_handles_setting(use):
    hbm = use(HbmFake)
    dl, codes, res = np.asarray([1, 2], np.int64), np.zeros(3, np.int64), np.zeros((3, 4), np.uint8)
    rows = lambda: api.AppendRows(texts=["zz", "naïve zz"])

    def ready(utf8):
        ix = handle()
        ix._info.embedding_dim = 8
        ix.group_count = int
        resident5(ix)
        if utf8:
            ix.text_utf8 = True
        return ix

    ready(False).append_arrays(dl, codes, res, rows=rows())
    ready(False).expand_arrays(np.zeros((2, 8), np.float32), np.asarray([1, 2, 1], np.int64), np.zeros(4, np.int64),
                               np.zeros((4, 4), np.uint8), n_replace=1, rows=rows())
    assert SEEN == [NULL] * 2
    SEEN.clear()
    ready(True).append_arrays(dl, codes, res, rows=rows())
    ready(True).expand_arrays(np.zeros((2, 8), np.float32), np.asarray([1, 2, 1], np.int64), np.zeros(4, np.int64),
                              np.zeros((4, 4), np.uint8), n_replace=1, rows=rows())
    assert SEEN == [table()] * 2
    SEEN.clear()
    assert ready(True).remove_ids([1, 3], keep_attachments=True) == 2           # a delete alone tokenises nothing
    assert SEEN == [] and "np_hip_index_text_merge" in names(hbm)


def test_cpp_mirror_passes_the_callers_table(tmp_path):
    """tests/cpp/textbuild_utf8_binding_check.cpp: next_plaid.hpp against recording stubs, with the host compiler alone under
    ASan + UBSan, given the table file Python wrote with tofile."""
    path = tmp_path / "unicode61.u32"
    T.unicode61_table(2).tofile(str(path))
    exe = tmp_path / "textbuild_utf8_binding_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "textbuild_utf8_binding_check.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
