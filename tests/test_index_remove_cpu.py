"""The resident remove's surface without a device: the C entry and its prototype, the ABI version it leaves alone, the argument
checks that run before any device work; remove_restate.shrunk_arrays pinned to np_hip_index_delete (host only); the slab
schedule of the in-place token move replayed on byte arrays, with planted defects that named cases reject;
np_remove_plan.h stand-alone under ASan + UBSan (tests/cpp/remove_plan_check.cpp); and both mirrors against recording
stand-ins for the library (the C++ side: tests/cpp/index_remove_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import remove_restate as R
import update_restate as U
from helpers import make_arrays, synth
from oracle import npy_index

from next_plaid_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
GXX = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]


# ---- the entry --------------------------------------------------------------------------------------------------------------------
def test_entry_and_prototype():
    L = api.lib()
    assert "np_hip_index_remove" in api.EXPORTS
    assert L.np_hip_index_remove.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    assert L.np_hip_abi_version() == 6 == api.NP_ABI_VERSION   # a new function only: no struct changed
    with open(os.path.join(ROOT, "include", "nextplaid_hip.h")) as f:
        assert "int np_hip_index_remove(np_index* index, const int64_t* doc_ids, int64_t n_ids, int64_t* out_removed);" in f.read()


def test_null_handle_is_refused_by_name():
    L = api.lib()
    out, ids = C.c_int64(-5), np.array([1, 2], np.int64)
    assert L.np_hip_index_remove(None, ids.ctypes.data, 2, C.byref(out)) == 8
    assert api.last_error() == "np_hip_index_remove: index is NULL"
    assert L.np_hip_index_remove(None, None, -1, C.byref(out)) == 8   # the handle is looked at first
    assert api.last_error() == "np_hip_index_remove: index is NULL" and out.value == -5


# ---- shrunk_arrays is what np_hip_index_delete writes -------------------------------------------------------------------------------
def _base(n=300, seed=4, lens=None):
    spec, a = make_arrays(num_docs=n, num_centroids=64, dim=32, nbits=4, doc_len_min=0, doc_len_max=9, seed=seed)
    if lens is not None:   # the same tokens cut into documents of other lengths
        lens = np.asarray(lens, np.int64)
        T = int(lens.sum())
        a = dict(a, doc_lengths=lens, codes=a["codes"][:T], residuals=a["residuals"][:T])
        a["ivf"], a["ivf_lengths"] = synth.build_ivf(a["codes"], lens, 64)
    return spec, a


def _lists(a):
    off = np.concatenate([[0], np.cumsum(a["ivf_lengths"])])
    return [a["ivf"][x:y] for x, y in zip(off[:-1], off[1:])]


def _with_lists(a, lists):
    return dict(a, ivf=np.concatenate(lists).astype(np.int64), ivf_lengths=np.array([len(x) for x in lists], np.int32))


def _variant(a, which):
    lists = [x.copy() for x in _lists(a)]
    if which == "permuted":
        rng = np.random.default_rng(1)
        lists = [rng.permutation(x) for x in lists]
    elif which == "missing a pair":
        c = int(np.argmax([len(x) for x in lists]))
        lists[c] = np.delete(lists[c], len(lists[c]) // 2)
    elif which == "extra pairs":
        doc_of = np.repeat(np.arange(a["doc_lengths"].size), a["doc_lengths"])
        for d in (0, 7, a["doc_lengths"].size - 1):
            c = next(c for c in range(64) if c not in set(a["codes"][doc_of == d].tolist()))
            lists[c] = np.insert(lists[c], int(np.searchsorted(lists[c], d)), d)
    return _with_lists(a, lists)


CASES = {
    "a random tenth": lambda n: np.random.default_rng(2).choice(n, n // 10, replace=False),
    "out of range and twice": lambda n: np.array([5, -1, n, 5, 1 << 40, n - 1, 17, 17, -(1 << 40)]),
    "nothing in range": lambda n: np.array([-1, n]),
    "bitmap word edges": lambda n: np.array([63, 64, 65, 127, 128, 191]),
    "every document": lambda n: np.arange(n),
}


@pytest.mark.parametrize("lists", ["as written", "permuted", "missing a pair", "extra pairs"])
@pytest.mark.parametrize("case", list(CASES))
def test_shrunk_arrays_is_the_directory_delete(tmp_path, case, lists):
    spec, a = _base()
    a = _variant(a, lists)
    cut, wts = synth.bucket_tables(spec)
    d = str(tmp_path / "ix")
    api.write_index_dir(d, a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=120)
    if lists != "as written":   # the writer refuses lists that do not ascend; a directory may hold them all the same
        np.save(os.path.join(d, "ivf.npy"), a["ivf"].astype("<i8"))
        np.save(os.path.join(d, "ivf_lengths.npy"), a["ivf_lengths"].astype("<i4"))
    ids = CASES[case](300)
    want = R.shrunk_arrays(a, ids)
    assert api.delete_from_index_dir(d, ids) == 300 - want["doc_lengths"].size == R.removed_ids(ids, 300).size
    r = npy_index.read_index(d)
    for k in ("doc_lengths", "codes", "residuals", "ivf", "ivf_lengths"):
        assert np.array_equal(np.asarray(r[k]).reshape(np.asarray(want[k]).shape), want[k]), k
    n1, t1 = want["doc_lengths"].size, int(want["doc_lengths"].sum())
    assert api._dir_counts(d) == (n1, t1)
    assert U._j(os.path.join(d, "metadata.json"))["avg_doclen"] == (t1 / n1 if n1 else 0.0)


def test_an_empty_document_removed_at_id_0(tmp_path):
    """no token and no posting-list entry goes, every entry is renumbered"""
    lens = np.random.default_rng(3).integers(1, 9, 200)
    lens[0] = 0
    spec, a = _base(lens=lens)
    cut, wts = synth.bucket_tables(spec)
    d = str(tmp_path / "ix")
    api.write_index_dir(d, a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=120)
    want = R.shrunk_arrays(a, [0])
    assert want["ivf"].size == a["ivf"].size and np.array_equal(want["ivf"], a["ivf"] - 1) and np.array_equal(want["codes"], a["codes"])
    assert api.delete_from_index_dir(d, [0]) == 1
    r = npy_index.read_index(d)
    for k in ("doc_lengths", "codes", "residuals", "ivf", "ivf_lengths"):
        assert np.array_equal(np.asarray(r[k]).reshape(np.asarray(want[k]).shape), want[k]), k
    off = np.concatenate([[0], np.cumsum(lens)])
    assert R.plan(off, np.arange(200) != 0, 64)[0] == []   # ... and no token moves


# ---- the renumbering ------------------------------------------------------------------------------------------------------------------
def test_rank_by_words_is_the_renumbering():
    """the device's rank (a per-word prefix + a popcount inside the word) against searchsorted, around word edges"""
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 130, 1000):
        rem = np.flatnonzero(rng.random(n) < 0.3)
        keep = np.setdiff1d(np.arange(n), rem)
        assert np.array_equal(keep - R.rank_by_words(rem, n, keep), R.new_ids(keep, rem))
        assert np.array_equal(R.new_ids(keep, rem), np.arange(keep.size))


def test_defect_rank_off_by_one_at_a_word_edge():
    """ids 63, 64, 65: with 63 removed, 64 -- the first document of the next word -- is 63; a rank that loses the word before
    says 64"""
    rem = np.array([63])
    assert R.rank_by_words(rem, 200, [62, 64, 65, 128]).tolist() == [0, 1, 1, 1]
    assert R.rank_by_words(rem, 200, [62, 64, 65, 128], defect="word_edge").tolist() != [0, 1, 1, 1]
    rem = np.array([64])
    assert R.rank_by_words(rem, 200, [63, 65]).tolist() == [0, 1]
    rem = np.array([10, 65])
    assert R.rank_by_words(rem, 200, [63, 64, 66]).tolist() == [1, 1, 2]
    assert R.rank_by_words(rem, 200, [63, 64, 66], defect="word_edge").tolist() != [1, 1, 2]


def test_defect_upper_bound_for_lower_bound():
    """a survivor is never in the removed list, so the two bounds agree on survivors -- the defect shows where the library
    itself would meet an id that IS removed: the restatement renumbers only survivors, and delete([-1, 3]) equals delete([3])"""
    _, a = _base()
    rem = np.array([3, 64])
    assert R.new_ids([3, 4, 64, 65], rem).tolist() == [3, 3, 63, 63]
    assert R.new_ids([3, 4, 64, 65], rem, defect="upper_bound").tolist() == [2, 3, 62, 63]
    # the crate counts every listed id below an entry, negative ones included: with upper_bound semantics on the raw list the
    # result differs from the pinned one as soon as a duplicate is listed
    good = R.shrunk_arrays(a, [3, 3, 64])
    assert np.array_equal(good["ivf"], R.shrunk_arrays(a, [3, 64])["ivf"])
    dup = np.sort(np.array([3, 3, 64]))   # a renumbering over the list as given, duplicates left in
    stay = ~np.isin(a["ivf"], dup)
    assert not np.array_equal(a["ivf"][stay] - np.searchsorted(dup, a["ivf"][stay], side="right"), good["ivf"])


# ---- the slab schedule ---------------------------------------------------------------------------------------------------------------
def _geometry(name):
    rng = np.random.default_rng(len(name))
    if name == "random":
        lens = np.where(rng.random(80) < 0.2, 0, rng.integers(0, 40, 80))
        keep = rng.random(80) < 0.6
    elif name == "one token at the front":
        lens, keep = np.array([1, 4500, 3]), np.array([False, True, True])
    elif name == "only at the end":
        lens, keep = np.array([5, 6, 7, 8, 0]), np.array([True, True, False, False, False])
    elif name == "a slab without a survivor":
        lens, keep = np.array([4, 300, 4, 0, 0, 2]), np.array([True, False, True, False, True, True])
    elif name == "one short of direct":
        lens, keep = np.array([3, 4]), np.array([False, True])
    else:
        raise KeyError(name)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), keep


GEOMETRIES = ["random", "one token at the front", "only at the end", "a slab without a survivor", "one short of direct"]


def _run(name, slab, row, defect=None):
    off, keep = _geometry(name)
    data = np.random.default_rng(9).integers(0, 256, int(off[-1]) * row).astype(np.uint8)
    want = data.reshape(-1, row)[np.repeat(keep, np.diff(off))].reshape(-1)
    launches, first, new_tokens, staging = R.plan(off, keep, slab, defect)
    assert staging <= slab, "the staging buffer is larger than a slab"
    got = R.replay(launches, off, keep, row, staging, data)
    assert np.array_equal(got[:first * row], data[:first * row]), "tokens in front of the first removed one were touched"
    assert new_tokens * row == want.size and np.array_equal(got[:want.size], want), "the result is not the compaction"
    return launches


@pytest.mark.parametrize("row", [2, 12, 64])
@pytest.mark.parametrize("slab", [1, 7, 64, 2000, 1 << 21])
@pytest.mark.parametrize("name", GEOMETRIES)
def test_slab_schedule(name, slab, row):
    launches = _run(name, slab, row)
    if name == "only at the end":
        assert launches == []
    if name == "one token at the front" and slab == 2000:
        assert [l[0] for l in launches] == [R.GATHER, R.COPY] * 3
    if name == "a slab without a survivor" and slab == 64:
        assert [l[0] for l in launches] == [R.DIRECT]   # slabs [4, 68) .. [260, 304) hold nothing; the last one is direct
    if name == "one short of direct":
        assert [l[0] for l in launches] == ([R.GATHER, R.COPY] if slab >= 7 else [R.DIRECT] * len(launches))


def test_defect_le_for_lt_in_the_direct_condition():
    """a slab whose last destination token IS its first source token (d1 == f + 1) must go through the staging buffer"""
    _run("one short of direct", 8, 12)
    with pytest.raises(AssertionError, match="a direct launch writes"):
        _run("one short of direct", 8, 12, defect="le_for_lt")


def test_defect_destination_from_the_shift_at_the_slabs_end():
    """a slab with a removed document inside: its survivors in front of that document move by the shift at the slab's START"""
    with pytest.raises(AssertionError, match="not the compaction|a direct launch writes|outside the array"):
        _run("random", 64, 12, defect="shift_at_end")
    _run("random", 64, 12)


def test_plan_header_stand_alone(tmp_path):
    """tests/cpp/remove_plan_check.cpp: np_remove_plan.h with its own main, host compiler alone, under ASan + UBSan"""
    exe = str(tmp_path / "remove_plan_check")
    subprocess.check_call(GXX + SAN + ["-I", os.path.join(ROOT, "next-plaid_amd", "csrc"),
                                       os.path.join(ROOT, "tests", "cpp", "remove_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_python_plan_is_the_headers(tmp_path):
    """the restated plan and np_remove_plan.h give the same launches: a small program prints the header's"""
    src = tmp_path / "p.cpp"
    src.write_text('#include <cstdio>\n#include "np_remove_plan.h"\nint main() {\n'
                   '  const int64_t off[] = {0, 1, 4501, 4504, 4504, 7004, 7013};\n  const uint8_t keep[] = {0, 1, 1, 0, 0, 1};\n'
                   '  const np::RemovePlan p = np::remove_plan(off, keep, 6, 32, 2000);\n'
                   '  for (const np::RemoveLaunch& l : p.launches) std::printf("%d %lld %lld %lld %lld\\n", l.mode, (long long)l.src0, '
                   '(long long)l.src1, (long long)l.dst0, (long long)l.dst1);\n'
                   '  std::printf("%lld %lld %lld\\n", (long long)p.first_moved, (long long)p.new_tokens, (long long)p.staging_rows);\n}\n')
    exe = str(tmp_path / "p")
    subprocess.check_call(GXX + SAN + ["-I", os.path.join(ROOT, "next-plaid_amd", "csrc"), str(src), "-o", exe])
    lines = [tuple(map(int, x.split())) for x in subprocess.check_output([exe], text=True).splitlines()]
    launches, first, new_tokens, staging = R.plan([0, 1, 4501, 4504, 4504, 7004, 7013], [0, 1, 1, 0, 0, 1], 2000)
    assert lines[:-1] == launches and lines[-1] == (first, new_tokens, staging)
    assert {l[0] for l in launches} == {R.DIRECT, R.GATHER, R.COPY}


# ---- the mirrors ---------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the library: records the entries reached and their argument values"""

    def __init__(self, n_docs, refuse=False):
        self.calls, self.n_docs, self.refuse = [], n_docs, refuse

    def np_hip_index_info(self, h, info):
        info._obj.num_documents = self.n_docs
        return 0

    def np_hip_last_error(self):
        return b"Invalid argument: the stub said so"

    def np_hip_index_close(self, h):
        pass

    @staticmethod
    def _ids(ptr, n):
        return None if ptr is None else np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int64)), (n,)).tolist() if n else []

    def np_hip_index_remove(self, h, ids, n, out):
        self.calls.append(("remove", self._ids(ids, n), n, out is not None))
        if self.refuse:
            return 8
        if out is not None:
            got = R.removed_ids(self._ids(ids, n) or [], self.n_docs).size
            out._obj.value = got
            self.n_docs -= got
        return 0

    def np_hip_index_delete(self, path, ids, n, out):
        self.calls.append(("delete", os.fsdecode(path), self._ids(ids, n), n))
        out._obj.value = R.removed_ids(self._ids(ids, n) or [], 20).size   # the directory holds 20 documents
        return 0

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def _handle(monkeypatch, rec, path):
    monkeypatch.setattr(api, "_lib", rec)
    hx = api.MmapIndex(C.c_void_p(1), path)
    hx.schema, hx.text, hx.group_values = "schema", "text", "groups"
    return hx


def test_remove_ids_reaches_the_entry(monkeypatch):
    rec = _Recorder(20)
    hx = _handle(monkeypatch, rec, "<arrays>")
    try:
        assert hx.remove_ids([3, 17, 3, -1, 20]) == 2 and hx.num_documents() == 18
        assert rec.calls == [("remove", [3, 17, 3, -1, 20], 5, True)]
        assert (hx.schema, hx.text, hx.group_values) == (None, None, None)
        hx.schema = "again"
        assert hx.remove_ids([]) == 0 and hx.remove_ids(np.array([99])) == 0
        assert rec.calls[1:] == [("remove", None, 0, True), ("remove", [99], 1, True)] and hx.schema == "again"   # nothing removed: kept
        with pytest.raises(api.IndexLoadError, match=r"remove\(\) needs an index opened from a directory"):
            hx.remove([1])
    finally:
        hx.close()


def test_remove_deletes_then_removes(monkeypatch, tmp_path):
    (tmp_path / "metadata.json").write_text('{"num_documents": 20, "num_embeddings": 55}')
    rec = _Recorder(20)
    hx = _handle(monkeypatch, rec, str(tmp_path))
    try:
        assert hx.remove([4, 4, 19, 25]) == 2
        assert rec.calls == [("remove", None, 0, False), ("delete", str(tmp_path), [4, 4, 19, 25], 4), ("remove", [4, 4, 19, 25], 4, True)]
        assert hx.num_documents() == 18 and hx.schema is None
        # the handle (18) is now behind ... ahead of its directory's metadata (20, the stub rewrote nothing): refused, nothing called
        rec.calls.clear()
        with pytest.raises(api.IndexLoadError, match="not current"):
            hx.remove([1])
        assert rec.calls == []
        # the library's own refusal of the handle (a shard) comes before the directory is touched
        rec.n_docs, rec.refuse = 20, True
        hx._info.num_documents = 20
        with pytest.raises(ValueError, match="the stub said so"):
            hx.remove([1])
        assert rec.calls == [("remove", None, 0, False)]
    finally:
        hx.close()


def test_delete_keeps_its_behaviour(monkeypatch, tmp_path):
    rec = _Recorder(20)
    hx = _handle(monkeypatch, rec, str(tmp_path))
    try:
        assert hx.delete([1, 2]) == 2 and hx.num_documents() == 20 and hx.schema == "schema"
        assert rec.calls == [("delete", str(tmp_path), [1, 2], 2)]
        assert "remove()" in api.MmapIndex.delete.__doc__
    finally:
        hx.close()


def test_cpp_mirror_against_recording_stubs(tmp_path):
    """tests/cpp/index_remove_check.cpp: next_plaid.hpp against recording stubs, with the host compiler alone, under ASan +
    UBSan"""
    exe, work = tmp_path / "index_remove_check", tmp_path / "dir"
    work.mkdir()
    subprocess.check_call(GXX + SAN + [os.path.join(ROOT, "tests", "cpp", "index_remove_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(work)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
