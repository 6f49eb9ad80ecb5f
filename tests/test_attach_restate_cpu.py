"""The attachment compaction without a device: the replayed select rule equals np.flatnonzero(keep) at the document counts and
keep patterns the GPU test uses; each planted defect -- upper_bound for lower_bound in the word bisection, a k-th-bit select
off by one, a validity ballot split at the wrong half, a tail merge that overwrites the shared word -- is rejected by a named
case; np_attach_plan.h runs stand-alone under ASan + UBSan (tests/cpp/attach_plan_check.cpp); and filters.Schema.extended /
shrunk against a fresh make_schema."""
import os
import subprocess

import numpy as np
import pytest

import attach_restate as A
from helpers import ROOT

from next_plaid_amd import filters as F

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
GXX = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
SIZES = A.SIZES


@pytest.mark.parametrize("n", SIZES)
def test_select_is_flatnonzero(n):
    for name, keep in A.patterns(n).items():
        if n > 5000 and name not in ("random tenth", "every other", "a run longer than 256"):
            continue   # (the plain-Python replay is slow: the stand-alone program runs every pattern at every size)
        assert np.array_equal(A.select_sources(keep), np.flatnonzero(keep)), name


def test_defect_upper_bound_for_lower_bound():
    """the survivor that is the LAST kept document of its word has exactly as many kept documents up to the word's end as
    j + 1: an upper bound walks past the word"""
    keep = np.ones(130, bool)
    keep[[3, 70]] = False
    assert np.array_equal(A.select_sources(keep), np.flatnonzero(keep))
    bad = A.select_sources(keep, defect="upper_bound")
    assert not np.array_equal(bad, np.flatnonzero(keep))
    assert bad[62] != 63 and np.array_equal(bad[:62], np.flatnonzero(keep)[:62])   # new id 62 = old 63, the last of word 0


def test_defect_kth_bit_off_by_one():
    keep = np.array([True, False, True, True] * 8)
    assert np.array_equal(A.select_sources(keep), np.flatnonzero(keep))
    assert not np.array_equal(A.select_sources(keep, defect="kth_bit"), np.flatnonzero(keep))
    assert A.select_bit(0b1011, 2) == 3 and A.select_bit(0b1011, 2, defect="kth_bit") != 3
    assert [A.select_bit((1 << 64) - 1, k) for k in (0, 31, 32, 63)] == [0, 31, 32, 63]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200])
def test_ballot_words_are_the_bitmap(n):
    rng = np.random.default_rng(n)
    v = rng.random(n) < 0.6
    assert np.array_equal(A.ballot_words(v), A.bitmap_words(v))
    assert np.array_equal(A.ballot_words(np.zeros(n, bool)), np.zeros((n + 31) // 32, np.uint32))   # all NULL
    if n > 32:   # (one word only: the second half is never written)
        v = np.zeros(n, bool)
        v[0] = True   # bit 0 of the first word, whatever the other half holds
        assert not np.array_equal(A.ballot_words(v, defect="ballot_half"), A.bitmap_words(v))


@pytest.mark.parametrize("n_old", [32, 1, 18, 31, 33, 64, 95])   # the old last document at bit 31, 0, 17, 30, 0, 31, 30
@pytest.mark.parametrize("fresh", [False, True])
def test_tail_merge(n_old, fresh):
    rng = np.random.default_rng(n_old)
    for n_new in (1, 5, 40, 70):
        old = np.ones(n_old, bool) if fresh else rng.random(n_old) < 0.5
        new = rng.random(n_new) < 0.5
        want = A.bitmap_words(np.concatenate([old, new]))
        words = A.bitmap_words(old)
        assert np.array_equal(A.tail_merge(words, n_old, new, fresh), want)
        assert np.array_equal(A.tail_merge(words, n_old, new, fresh, garbage=0xFFFFFFFF), want)   # the old tail is not trusted


def test_defect_tail_merge_overwrites_the_shared_word():
    old = np.array([True, False, True] * 6)   # 18 old rows: the old last document is bit 17 of word 0
    new = np.array([True, True, False, True])
    want = A.bitmap_words(np.concatenate([old, new]))
    assert np.array_equal(A.tail_merge(A.bitmap_words(old), 18, new, False), want)
    bad = A.tail_merge(A.bitmap_words(old), 18, new, False, defect="overwrite")
    assert not np.array_equal(bad, want) and bad[0] & 0x3FFFF == 0   # the old rows' bits are gone


def test_restated_columns():
    data, valid = np.array([5, 6, 7, 8], np.int64), np.array([1, 0, 1, 1], np.uint8)
    d, v = A.shrunk_column(data, valid, np.array([True, False, True, False]))
    assert d.tolist() == [5, 7] and v is None   # the only NULL row left: no bitmap, as set_columns leaves it
    d, v = A.shrunk_column(data, valid, np.array([True, True, False, False]))
    assert d.tolist() == [5, 6] and v.tolist() == [1, 0]
    codes, cv = np.array([0, 2, 1, 0], np.int32), np.array([1, 1, 1, 0], np.uint8)
    d, v = A.appended_column(codes, cv, [1, 4], None, remap=[2, 3, 5])
    assert d.tolist() == [2, 5, 3, 0, 1, 4] and v.tolist() == [1, 1, 1, 0, 1, 1]   # the NULL row keeps its bytes
    d, v = A.appended_column(np.array([1.0]), None, [np.nan, 2.0], None)
    assert v.tolist() == [1, 0, 1] and np.isnan(d[1])
    assert A.code_range([3, 1]) == (0, 3) and A.code_range([]) == (0, -1) and A.code_range([-2, 0]) == (-2, 0)


def test_plan_header_stand_alone(tmp_path):
    """tests/cpp/attach_plan_check.cpp: np_attach_plan.h with the host compiler alone, under ASan + UBSan"""
    exe = tmp_path / "attach_plan_check"
    subprocess.check_call(GXX + SAN + [os.path.join(ROOT, "tests", "cpp", "attach_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- Schema.extended and Schema.shrunk ------------------------------------------------------------------------------------------
OLD = {"year": [2001, 1999, None, 2010], "score": [0.5, float("nan"), 2.0, 1.0], "lang": ["de", "fr", None, "de"],
       "tag": ["m", "m", "x", "q"]}


def _same(a: F.Schema, b: F.Schema):
    assert list(a.columns) == list(b.columns)
    for name in a.columns:
        x, y = a[name], b[name]
        assert (x.index, x.type, x.dictionary, x.text_on_device, x.first_non_ascii) == \
               (y.index, y.type, y.dictionary, y.text_on_device, y.first_non_ascii), name
        assert x.data.dtype == y.data.dtype and np.array_equal(x.data, y.data, equal_nan=x.type == F.NP_COL_F64), name
        assert (x.valid is None) == (y.valid is None) and (x.valid is None or np.array_equal(x.valid, y.valid)), name


@pytest.mark.parametrize("new_lang,new_tag,moved", [
    (["aa", "de"], ["m", "q"], True),      # a new string in front of the old ones
    (["es", None], ["x", "x"], True),      # ... between them
    (["zz", "fr"], ["m", "m"], True),      # ... behind them
    (["fr", "de"], ["q", "x"], False),     # none
    (["aa", "zz"], ["a", "z"], True),
])
def test_extended_is_a_fresh_schema_of_the_concatenation(new_lang, new_tag, moved):
    sch = F.make_schema(OLD, 4, text_on_device=["tag"])
    new = {"year": [None, 7], "score": [3.5, float("nan")], "lang": new_lang, "tag": new_tag}
    ext, rows, remaps = sch.extended(new)
    _same(ext, F.make_schema({k: OLD[k] + new[k] for k in OLD}, 6, text_on_device=["tag"]))
    assert (remaps["lang"] is not None) == moved and remaps["year"] is None and remaps["score"] is None
    for name in ("lang", "tag"):
        r = remaps[name]
        if r is None:
            assert ext[name].dictionary == sch[name].dictionary   # no string is new
        else:
            assert r.dtype == np.int32 and r.size == len(sch[name].dictionary) and r[0] >= 0 and (np.diff(r) > 0).all()
            assert [ext[name].dictionary[i] for i in r] == sch[name].dictionary
        assert np.array_equal(rows[name].data, ext[name].data[4:]) and rows[name].data.dtype == np.int32
    assert rows["score"].valid.tolist() == [1, 0] and rows["year"].valid.tolist() == [0, 1]


def test_extended_refusals_and_null_batches():
    sch = F.make_schema(OLD, 4)
    with pytest.raises(F.FilterError, match="not exactly the schema's"):
        sch.extended({"year": [1], "score": [1.0], "lang": ["de"]})
    with pytest.raises(F.FilterError, match="not exactly the schema's"):
        sch.extended({"year": [1], "score": [1.0], "lang": ["de"], "tag": ["m"], "more": [1]})
    with pytest.raises(F.FilterError, match="type"):
        sch.extended({"year": ["x"], "score": [1.0], "lang": ["de"], "tag": ["m"]})
    with pytest.raises(F.ShapeError):
        sch.extended({"year": [1, 2], "score": [1.0], "lang": ["de"], "tag": ["m"]})
    ext, rows, remaps = sch.extended({"year": [None], "score": [2], "lang": [None], "tag": [None]})   # all NULL; an int for a float
    assert rows["lang"].type == F.NP_COL_CODE and rows["lang"].data.tolist() == [0] and remaps["lang"] is None
    assert rows["score"].type == F.NP_COL_F64 and ext["score"].data[-1] == 2.0 and ext["year"].valid.tolist() == [1, 1, 0, 1, 0]


def test_shrunk_keeps_dictionaries():
    sch = F.make_schema(OLD, 4, text_on_device=["tag"])
    s = sch.shrunk(np.array([True, True, False, False]))
    assert s["lang"].dictionary == [b"de", b"fr"] and s["tag"].dictionary == [b"m", b"q", b"x"] and s["tag"].text_on_device
    assert s["year"].data.tolist() == [2001, 1999] and s["year"].valid is None and s["score"].valid.tolist() == [1, 0]
    assert s["lang"].data.tolist() == [0, 1] and s["tag"].data.tolist() == [0, 0]
