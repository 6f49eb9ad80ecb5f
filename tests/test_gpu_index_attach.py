"""np_hip_index_remove_keep / np_hip_index_append_rows and their mirrors (MmapIndex.remove / remove_ids with keep_attachments,
append / append_arrays with rows=): metadata columns and groups that stay attached through a resident remove and append.

The contract: after a keeping call, get_column / get_groups equal the restated arrays (tests/attach_restate.py) byte for byte,
and the handle equals, in filter_ids, search_batch(filters=), search_grouped and match_text, a fresh handle of the shrunk or
grown arrays with set_columns / set_groups of the restated rows.  Tiny indexes throughout.  Needs a real MI355X."""
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import append_restate as G
import attach_restate as A
import remove_restate as R
from helpers import ROOT, hip_index, make_arrays, synth

import next_plaid_amd as npa
from next_plaid_amd import api, filters as F, text as T

pytestmark = pytest.mark.gpu

GEOM = dict(num_centroids=64, dim=32, nbits=4, doc_len_min=1, doc_len_max=6)
LANGS = ["de", "en", "fr", "it", "pt"]
TAGS = ["alpha", "beta", "bravo", "gamma", "alps"]
FILTERS = [("i >= ?", (10,)), "im IS NULL", ("f < ? OR f IS NULL", (0.0,)), ("s = ?", ("fr",)), ("s IN (?, ?)", ("de", "pt")),
           ("t LIKE ?", ("al%",)), ("t REGEXP ?", ("^b.*a$",)), "nul IS NULL", ("NOT (im < ?)", (20,)), ("fv BETWEEN ? AND ?", (-0.5, 0.5))]
P = dict(n_full_scores=64, top_k=5, n_ivf_probe=4)


def _base(n, seed=5):
    return make_arrays(num_docs=n, seed=seed, **GEOM)[1]


def _values(n, seed=1):
    """every column kind over n documents: I64 without and with NULLs, F64 with NaN rows and without, a column that is all NULL,
    text with NULLs, text whose dictionary goes to the device; and group keys with NULLs"""
    rng = np.random.default_rng(seed)
    r = rng.random((4, n))
    r[2, 0] = 1.0   # (the first document's text is not NULL: a text column stays one at every cut)
    cols = {"i": rng.integers(-5, 50, n),
            "im": [None if r[0, d] < 0.3 else int(v) for d, v in enumerate(rng.integers(0, 40, n))],
            "f": np.where(r[1] < 0.25, np.nan, rng.standard_normal(n)),
            "fv": rng.standard_normal(n),
            "nul": [None] * n,
            "s": [None if r[2, d] < 0.2 else LANGS[j] for d, j in enumerate(rng.integers(0, len(LANGS), n))],
            "t": [TAGS[j] for j in rng.integers(0, len(TAGS), n)]}
    keys = [None if r[3, d] < 0.1 else int(g) for d, g in enumerate(rng.integers(0, max(1, n // 3), n))]
    return cols, keys


def _queries(a, n_queries=2, n_tokens=6, seed=11):
    lens, codes, res = a["doc_lengths"], a["codes"], a["residuals"]
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)])
    qs = []
    for d in np.argsort(-np.asarray(lens), kind="stable")[:n_queries]:
        pick = off[d] + rng.integers(0, max(int(lens[d]), 1), n_tokens)
        v = synth.reconstruct(codes[pick], res[pick], a["centroids"], a["bucket_weights"], a["nbits"])
        v = v + np.float32(0.05) * rng.standard_normal(v.shape).astype(np.float32)
        qs.append(np.ascontiguousarray(v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12), np.float32))
    return qs


def _attach_raw(hx, sch, gids, n_groups):
    """set_columns / set_column_text / set_groups of ready arrays: the rows reach the library exactly as restated"""
    cols = (api.np_column * max(len(sch), 1))()
    for c in sch.columns.values():
        cols[c.index] = api.np_column(c.type, 0, c.data.ctypes.data, None if c.valid is None else c.valid.ctypes.data)
    api._check(api.lib().np_hip_index_set_columns(hx._h, cols, len(sch)))
    for c in sch.columns.values():
        if c.text_on_device and c.dictionary:
            hx.set_column_text_raw(c.index, c.dictionary)
    hx.schema = sch if len(sch) else None
    if gids is not None and len(gids):
        hx.set_groups(np.asarray(gids, np.int32), n_groups=n_groups)


def _restated(sch, cols):
    """a Schema of restated (data, valid) pairs under the names, dictionaries and flags of `sch`"""
    out = F.Schema()
    for name, c in sch.columns.items():
        data, valid = cols[name]
        out.columns[name] = F.Column(name, c.index, c.type, np.ascontiguousarray(data), valid, c.dictionary, c.text_on_device,
                                     c.first_non_ascii)
    return out


def _assert_read_back(hx, sch, gids, what=""):
    """get_column / get_groups against the restated arrays, byte for byte, the presence of a bitmap included"""
    for name, c in sch.columns.items():
        data, valid = hx.get_column(name)
        assert data.dtype == c.data.dtype and data.tobytes() == c.data.tobytes(), f"{what}: column {name}"
        assert (valid is None) == (c.valid is None), f"{what}: column {name}: bitmap {'kept' if c.valid is None else 'lost'}"
        assert valid is None or np.array_equal(valid, c.valid), f"{what}: column {name}: validity"
    if gids is None or len(gids) == 0:
        assert hx.group_count() == 0, what
        with pytest.raises(ValueError, match="the handle has no groups"):
            hx.get_groups()
    else:
        assert np.array_equal(hx.get_groups(), gids), f"{what}: groups"


def _rows(results):
    return [(r.passage_ids.tobytes(), np.asarray(r.scores, np.float32).tobytes()) for r in results]


def _answers(hx, qs, filters=FILTERS, match="t"):
    out = {"filter_ids": [x.tobytes() for x in hx.filter_ids(filters)]}
    p = npa.SearchParameters(**P)
    out["filtered"] = _rows(hx.search_batch(qs, p, filters=[filters[(3 * i) % len(filters)] for i in range(len(qs))]))
    if hx.group_count():
        raw = hx.search_grouped(qs, p, group_size=2, raw=True)
        out["grouped"] = [None if x is None else np.ascontiguousarray(x).tobytes() for x in raw]
        raw = hx.search_grouped(qs, p, group_size=1, raw=True, filters=[filters[0]] * len(qs))
        out["grouped filtered"] = [None if x is None else np.ascontiguousarray(x).tobytes() for x in raw]
    if match:
        out["match"] = [m.tobytes() for m in hx.match_text(match, ["al.*", "b"])] + \
                       [m.tobytes() for m in hx.match_text(match, ["%a", "_l%"], like=True)]
    return out


def _assert_equal_to_fresh(hx, arrays, sch, gids, n_groups, what="", **kw):
    """the handle against a fresh one of `arrays` with the restated rows attached"""
    fresh = hip_index(arrays)
    try:
        _attach_raw(fresh, sch, gids, n_groups)
        assert hx.num_documents() == fresh.num_documents() and hx.group_count() == fresh.group_count(), what
        _assert_read_back(fresh, sch, gids, what + " (the fresh handle)")
        if hx.num_documents() == 0:
            return
        saved, hx.schema = hx.schema, sch   # both compile their filters against the same dictionaries
        try:
            qs = _queries(arrays)
            got, want = _answers(hx, qs, **kw), _answers(fresh, qs, **kw)
        finally:
            hx.schema = saved
        assert got.keys() == want.keys(), what
        for k in want:
            assert got[k] == want[k], f"{what}: {k}"
    finally:
        fresh.close()


def _remove_case(base, sch0, gids0, n_groups, ids, n_calls=1, what="", **kw):
    n0 = base["doc_lengths"].size
    keep = A.keep_mask(n0, ids)
    want_sch = _restated(sch0, {n: A.shrunk_column(c.data, c.valid, keep) for n, c in sch0.columns.items()})
    want_g = gids0[keep] if len(gids0) else gids0
    hx = hip_index(base)
    try:
        _attach_raw(hx, sch0, gids0, n_groups)
        cap = hx.capacity()
        rem = R.removed_ids(ids, n0)
        cuts = np.linspace(0, rem.size, n_calls + 1).astype(int)
        for a, b in zip(cuts[:-1], cuts[1:]):   # a later call names its documents by the ids the earlier ones left them
            assert hx.remove_ids(rem[a:b] - a, keep_attachments=True) == b - a
        assert hx.capacity() == cap and hx.text is None
        assert hx.group_count() == (n_groups if keep.any() else 0), what
        _assert_read_back(hx, want_sch, want_g, what)
        for name, c in (hx.schema.columns.items() if hx.schema is not None else ()):   # the mirror's own rows follow
            assert c.data.tobytes() == want_sch[name].data.tobytes() and c.dictionary == sch0[name].dictionary, what
        _assert_equal_to_fresh(hx, R.shrunk_arrays(base, ids), want_sch, want_g, n_groups, what, **kw)
    finally:
        hx.close()


@pytest.fixture(scope="module")
def corpus():
    """per document count: the index, the schema of every column kind and the groups -- computed once, left unchanged"""
    made = {}

    def get(n):
        if n not in made:
            cols, keys = _values(n)
            gids, _, n_groups = api.group_ids_of_keys(keys)
            made[n] = (_base(n), F.make_schema(cols, n, text_on_device=["t"]), gids, n_groups)
        return made[n]
    return get


# ---- remove: document counts and keep patterns ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", A.SIZES)
def test_remove_keep_counts_and_patterns(corpus, n):
    base, sch, gids, n_groups = corpus(n)
    for name, keep in A.patterns(n).items():
        _remove_case(base, sch, gids, n_groups, np.flatnonzero(~keep), what=f"n = {n}, {name}")


@pytest.mark.parametrize("n", [129, 4097])
def test_remove_keep_a_random_tenth_in_three_calls(corpus, n):
    base, sch, gids, n_groups = corpus(n)
    _remove_case(base, sch, gids, n_groups, np.flatnonzero(~A.patterns(n)["random tenth"]), n_calls=3, what="three calls")


def test_plain_remove_still_drops_the_attachments(corpus):
    """the unchanged default"""
    base, sch, gids, n_groups = corpus(65)
    hx = hip_index(base)
    try:
        _attach_raw(hx, sch, gids, n_groups)
        assert hx.remove_ids([3]) == 1
        assert hx.schema is None and hx.group_values is None and hx.group_count() == 0
        with pytest.raises(ValueError, match="outside the handle's 0 columns"):
            api._check(api.lib().np_hip_index_get_column(hx._h, 0, None, None, None, None))
    finally:
        hx.close()


# ---- remove: column kinds ----------------------------------------------------------------------------------------------------
def test_remove_keep_leaves_no_bitmap_without_a_null(corpus):
    """the only NULL rows leave: the column has no bitmap afterwards, as on a fresh handle; an all-NULL column keeps its own"""
    base = corpus(65)[0]
    vals = {"a": [None if d in (5, 64) else d for d in range(65)], "z": [None] * 65, "x": np.arange(65.0)}
    sch = F.make_schema(vals, 65)
    hx = hip_index(base)
    try:
        _attach_raw(hx, sch, None, 0)
        assert hx.get_column("a")[1] is not None and hx.get_column("x")[1] is None
        assert hx.remove_ids([5, 64], keep_attachments=True) == 2
        assert hx.get_column("a")[1] is None and hx.get_column("x")[1] is None
        assert np.array_equal(hx.get_column("z")[1], np.zeros(63, np.uint8))
        assert [x.size for x in hx.filter_ids(["a IS NULL", "z IS NULL", ("x >= ?", (0.0,))])] == [0, 63, 63]
    finally:
        hx.close()


def test_remove_keep_64_columns(corpus):
    base = corpus(129)[0]
    rng = np.random.default_rng(8)
    vals = {f"c{i:02d}": ([None if v % 7 == 0 else int(v) for v in rng.integers(0, 99, 129)] if i % 2 else rng.integers(0, 99, 129))
            for i in range(64)}
    _remove_case(base, F.make_schema(vals, 129), np.zeros(0, np.int32), 0, np.arange(1, 129, 3), what="64 columns",
                 filters=[("c00 > ?", (50,)), "c01 IS NULL", ("c63 < ? OR c63 IS NULL", (10,)), ("c32 = ?", (7,))], match=None)


def test_remove_keep_code_range_follows_the_survivors(corpus):
    """the only row that holds the largest code is removed: the shorter dictionary is then accepted as on a fresh handle, and
    refused before"""
    base = corpus(65)[0]
    words = ["a"] * 64 + ["zz"]
    sch = F.make_schema({"w": words}, 65, text_on_device=["w"])
    hx = hip_index(base)
    try:
        _attach_raw(hx, sch, None, 0)
        with pytest.raises(ValueError, match=r"holds codes 0\.\.1, which 1 strings do not cover"):
            hx.set_column_text_raw(0, [b"a"])
        assert hx.remove_ids([64], keep_attachments=True) == 1
        assert hx.match_text("w", ["a"])[0].tolist() == [True, False]   # the text stayed: it is per code
        hx.set_column_text_raw(0, [b"a"])
        fresh = hip_index(R.shrunk_arrays(base, [64]))
        try:
            _attach_raw(fresh, F.make_schema({"w": words[:64]}, 64), None, 0)
            fresh.set_column_text_raw(0, [b"a"])
        finally:
            fresh.close()
    finally:
        hx.close()


# ---- append ----------------------------------------------------------------------------------------------------------------
def _split(n0, n_new, seed=5):
    """an index of n0 + n_new documents cut into its first n0 (with their own lists) and the tokens of the rest"""
    whole = _base(n0 + n_new, seed)
    base = R.shrunk_arrays(whole, np.arange(n0, n0 + n_new))
    T0 = int(base["doc_lengths"].sum())
    return base, (whole["doc_lengths"][n0:], whole["codes"][T0:], whole["residuals"][T0:])


def _group_rule(old_keys, new_keys):
    """an existing key keeps its id, new keys take the next ids in the order they come; the NULLs are one group"""
    gids, values, n_groups = api.group_ids_of_keys(old_keys)
    where = {v: i for i, v in enumerate(values)}
    if n_groups == len(values) + 1:
        where[None] = len(values)
    new = []
    for k in new_keys:
        if k not in where:
            where[k] = len(where)
        new.append(where[k])
    return np.concatenate([gids, np.asarray(new, np.int32)]), len(where)


def _append_case(n0, n_new, old_vals, old_keys, new_vals, new_keys, reserve=None, what="", text_on_device=("t",)):
    base, new = _split(n0, n_new)
    sch0 = F.make_schema(old_vals, n0, text_on_device=text_on_device)
    _, rows, remaps = sch0.extended(new_vals)
    ext = sch0.extended(new_vals)[0]
    want_sch = _restated(ext, {n: A.appended_column(c.data, c.valid, rows[n].data, rows[n].valid, remaps[n]) for n, c in sch0.columns.items()})
    want_g, n_groups = _group_rule(old_keys, new_keys)
    hx = hip_index(base)
    try:
        if reserve:
            hx.reserve(*reserve)
        hx.set_columns(old_vals, text_on_device=text_on_device)
        hx.set_groups(old_keys)
        cap = hx.capacity()
        ids = hx.append_arrays(*new, rows=api.AppendRows(columns=new_vals, groups=new_keys))
        assert ids.tolist() == list(range(n0, n0 + n_new))
        if reserve and reserve[0] >= n_new and n_new:
            assert hx.capacity() == cap, "an append inside the reservation changed the capacity"
        assert hx.group_count() == n_groups
        _assert_read_back(hx, want_sch, want_g, what)
        for name, c in hx.schema.columns.items():
            assert c.dictionary == ext[name].dictionary and c.data.tobytes() == want_sch[name].data.tobytes(), f"{what}: schema {name}"
        _assert_equal_to_fresh(hx, G.grown_arrays(base, new), want_sch, want_g, n_groups, what, match=text_on_device[0] if text_on_device else None)
    finally:
        hx.close()


def _cut(vals, keys, n0):
    old = {k: (v[:n0] if isinstance(v, list) else v[:n0].copy()) for k, v in vals.items()}
    new = {k: (v[n0:] if isinstance(v, list) else v[n0:].copy()) for k, v in vals.items()}
    return old, keys[:n0], new, keys[n0:]


@pytest.mark.parametrize("n0,n_new", [(32, 1), (32, 70), (33, 40), (50, 5), (50, 100), (1, 64)])   # the old last document at bit 31, 0, 17
@pytest.mark.parametrize("reserve", [None, (200, 2000), (3, 10)])   # without, inside and beyond a reservation
def test_append_rows_counts_and_reservations(n0, n_new, reserve):
    vals, keys = _values(n0 + n_new, seed=n0)
    _append_case(n0, n_new, *_cut(vals, keys, n0), reserve=reserve, what=f"{n0} + {n_new}, reserve {reserve}")


def test_append_rows_first_null_of_a_column():
    """columns without a bitmap get one only where a new row is NULL, and all earlier rows are then valid"""
    n0, n_new = 50, 40
    vals, keys = _values(n0 + n_new, seed=2)
    old, ok, new, nk = _cut(vals, keys, n0)
    new["i"] = [None if d == 7 else int(v) for d, v in enumerate(new["i"])]     # the first NULL of an I64 column
    new["fv"] = np.where(np.arange(n_new) == 39, np.nan, new["fv"])             # ... of an F64 column, as a NaN, in the last row
    new["t"] = [None if d == 0 else v for d, v in enumerate(new["t"])]          # ... of a text column, in the first new row
    _append_case(n0, n_new, old, ok, new, nk, what="first NULL")


@pytest.mark.parametrize("extra", [["aa"], ["dz"], ["zz"], [], ["aa", "ea", "zz"]])   # a new string in front, between, behind, none
def test_append_rows_dictionary_growth(extra):
    n0, n_new = 50, 12
    vals, keys = _values(n0 + n_new, seed=3)
    old, ok, new, nk = _cut(vals, keys, n0)
    for j, s in enumerate(extra):
        new["s"][2 * j] = s
        new["t"][2 * j + 1] = s + "x"
    _append_case(n0, n_new, old, ok, new, nk, what=f"new strings {extra}")


def test_append_rows_group_keys_old_and_new():
    n0, n_new = 40, 6
    vals, keys = _values(n0 + n_new, seed=4)
    old, _, new, _ = _cut(vals, keys, n0)
    ok = [d % 5 for d in range(n0)]                    # no NULL group yet
    _append_case(n0, n_new, old, ok, new, [3, 99, None, 99, 0, -4], what="new keys, a first NULL key")
    ok[7] = None
    _append_case(n0, n_new, old, ok, new, [None, 5, 4, 6, 5, None], what="the NULLs' group keeps its id")


def test_append_rows_of_no_documents(corpus):
    base, sch, gids, n_groups = corpus(65)
    hx = hip_index(base)
    try:
        _attach_raw(hx, sch, gids, n_groups)
        empty = {n: ([] if c.type != F.NP_COL_F64 else np.zeros(0)) for n, c in sch.columns.items()}
        out = hx.append_arrays(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 16), np.uint8),
                               rows=api.AppendRows(columns=empty, groups=[]))
        assert out.size == 0 and hx.num_documents() == 65 and hx.group_count() == n_groups
        _assert_read_back(hx, sch, gids, "zero new documents")
    finally:
        hx.close()


# ---- sequences ----------------------------------------------------------------------------------------------------------------
def test_remove_append_remove_keeps_the_capacity():
    n0, n_new = 130, 30
    vals, keys = _values(n0 + n_new, seed=6)
    old, ok, new, nk = _cut(vals, keys, n0)
    base, tail = _split(n0, n_new)
    hx = hip_index(base)
    try:
        hx.set_columns(old, text_on_device=["t"])
        hx.set_groups(ok)
        sch0, (gids0, _, n_groups) = hx.schema, api.group_ids_of_keys(ok)
        cap = hx.capacity()
        first = np.arange(0, n0, 4)
        assert hx.remove_ids(first, keep_attachments=True) == first.size
        k1 = A.keep_mask(n0, first)
        s1 = _restated(sch0, {n: A.shrunk_column(c.data, c.valid, k1) for n, c in sch0.columns.items()})
        _assert_read_back(hx, s1, gids0[k1], "after the first remove")
        hx.append_arrays(*tail, rows=api.AppendRows(columns=new, groups=nk))
        assert hx.capacity()[0] == cap[0], "the freed documents are a reservation: the append's rows fit in it"
        cap = hx.capacity()
        _, rows, remaps = s1.extended(new)
        s2 = _restated(hx.schema, {n: A.appended_column(c.data, c.valid, rows[n].data, rows[n].valid, remaps[n]) for n, c in s1.columns.items()})
        g2 = np.concatenate([gids0[k1], _group_rule(ok, nk)[0][n0:]])
        _assert_read_back(hx, s2, g2, "after the append")
        n1 = int(k1.sum()) + n_new
        second = np.concatenate([np.arange(n1 - 10, n1), [0, 64]])
        assert hx.remove_ids(second, keep_attachments=True) == 12
        k2 = A.keep_mask(n1, second)
        s3 = _restated(s2, {n: A.shrunk_column(c.data, c.valid, k2) for n, c in s2.columns.items()})
        assert hx.capacity() == cap
        _assert_read_back(hx, s3, g2[k2], "after the second remove")
        arrays = R.shrunk_arrays(G.grown_arrays(R.shrunk_arrays(base, first), tail), second)
        _assert_equal_to_fresh(hx, arrays, s3, g2[k2], hx.group_count(), "remove, append, remove")
    finally:
        hx.close()


# ---- the keyword index, carried by the mirror ------------------------------------------------------------------------------------
WORDS = ["amber", "birch", "cedar", "delta", "ember", "fjord", "grove", "heath"]


def _texts(n, seed=9):
    rng = np.random.default_rng(seed)
    return [" ".join(WORDS[j] for j in rng.integers(0, len(WORDS), 4)) + (" lonely" if d == 3 else "") for d in range(n)]


def _text_answers(hx):
    return _rows(hx.text_search(["amber", "birch cedar", "lonely", "delta OR heath"], 8))


def test_keyword_index_follows_both_calls():
    n0, n_new = 60, 9
    base, tail = _split(n0, n_new)
    texts = _texts(n0 + n_new)
    hx = hip_index(base)
    try:
        hx.set_columns({"i": np.arange(n0)})
        hx.set_text(T.TextIndexData.from_texts(texts[:n0]))
        gone = [3, 10, 59]   # document 3 holds the only "lonely": the term dies and the rest is renumbered
        assert hx.remove_ids(gone, keep_attachments=True) == 3
        left = [t for d, t in enumerate(texts[:n0]) if d not in gone]
        fresh = hip_index(R.shrunk_arrays(base, gone))
        try:
            fresh.set_text(T.TextIndexData.from_texts(left))
            assert _text_answers(hx) == _text_answers(fresh)
        finally:
            fresh.close()
        with pytest.raises(ValueError, match="rows.texts is None"):
            hx.append_arrays(*tail, rows=api.AppendRows(columns={"i": np.arange(n_new)}))
        assert hx.num_documents() == n0 - 3 and hx.get_column("i")[0].size == n0 - 3
        hx.append_arrays(*tail, rows=api.AppendRows(columns={"i": np.arange(n_new)}, texts=texts[n0:]))
        fresh = hip_index(G.grown_arrays(R.shrunk_arrays(base, gone), tail))
        try:
            fresh.set_text(T.TextIndexData.from_texts(left + texts[n0:]))
            assert _text_answers(hx) == _text_answers(fresh)
        finally:
            fresh.close()
    finally:
        hx.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _append_rows_raw(hx, new, cols, n_cols, remap, groups, n_groups):
    lens, codes, res = np.ascontiguousarray(new[0], np.int64), np.ascontiguousarray(new[1], np.int64), np.ascontiguousarray(new[2], np.uint8)
    arr = (api.np_column * max(len(cols), 1))(*[api.np_column(t, 0, d.ctypes.data, None) for t, d in cols])
    tables = (C.c_void_p * max(len(cols), 1))(*[None if r is None else r.ctypes.data for r in remap]) if remap else None
    return api.lib().np_hip_index_append_rows(hx._h, lens.ctypes.data, lens.size, codes.ctypes.data, res.ctypes.data, arr,
                                              n_cols, None if tables is None else C.cast(tables, C.c_void_p),
                                              None if groups is None else groups.ctypes.data, n_groups)


def test_refusals_leave_the_handle_byte_identical():
    n0, n_new = 40, 4
    base, new = _split(n0, n_new)
    sch = F.make_schema({"i": np.arange(n0), "s": [LANGS[d % 3] for d in range(n0)], "f": np.arange(n0) * 0.5}, n0)
    gids = (np.arange(n0) % 4).astype(np.int32)
    i64, f64, i32, g = np.arange(4), np.zeros(4), np.zeros(4, np.int32), np.zeros(4, np.int32)
    good = [(0, i64), (2, i32), (1, f64)]
    hx = hip_index(base)
    try:
        _attach_raw(hx, sch, gids, 4)
        qs = _queries(base)
        before = _answers(hx, qs, filters=[("i > ?", (5,)), ("s = ?", ("en",)), ("f < ?", (3.0,))], match=None)
        for what, args, msg in [
            ("type mismatch", ([(0, i64), (1, f64), (1, f64)], 3, None, g, 4), r"new_cols\[1\] has type 1, column 1 of the handle type 2"),
            ("wrong n_cols", (good[:2], 2, None, g, 4), "n_cols is 2, the handle has 3 columns"),
            ("non-monotone remap", (good, 3, [None, np.array([0, 2, 2], np.int32), None], g, 4), r"code_remap\[1\]\[2\] = 2"),
            ("remap of a column that is no CODE column", (good, 3, [np.array([0], np.int32), None, None], g, 4), "no CODE column"),
            ("groups missing", (good, 3, None, None, 4), "new_groups is NULL, the handle has groups"),
            ("fewer groups", (good, 3, None, g, 3), "n_groups is 3, the handle has 4"),
            ("a group id out of range", (good, 3, None, np.array([0, 4, 0, 0], np.int32), 4), r"new_groups\[1\] = 4"),
        ]:
            assert _append_rows_raw(hx, new, *args) == 8, what
            assert re.search(msg, api.last_error()), (what, api.last_error())
            assert api.last_error().startswith("np_hip_index_append_rows: ")
            assert hx.num_documents() == n0
            _assert_read_back(hx, sch, gids, what)
        assert _answers(hx, qs, filters=[("i > ?", (5,)), ("s = ?", ("en",)), ("f < ?", (3.0,))], match=None) == before
        hx.set_groups(None)
        assert _append_rows_raw(hx, new, good, 3, None, g, 4) == 8 and "the handle has no groups" in api.last_error()
        _assert_read_back(hx, sch, None, "groups unexpected")
        with pytest.raises(F.FilterError, match="not exactly the schema's"):   # the mirror, before the library is reached
            hx.append_arrays(*new, rows=api.AppendRows(columns={"i": i64}))
        with pytest.raises(ValueError, match="rows.groups is given and the handle has no groups"):
            hx.append_arrays(*new, rows=api.AppendRows(columns={"i": i64, "s": ["de"] * 4, "f": f64}, groups=[1, 2, 3, 4]))
        _assert_read_back(hx, sch, None, "the mirror's refusals")
    finally:
        hx.close()


def test_a_sharded_handle_is_refused_by_both_entries():
    base, new = _split(40, 4)
    hx = hip_index(base, shard_rank=0, shard_count=2)
    try:
        hx.set_columns({"i": np.arange(40)})
        want = hx.get_column("i")
        with pytest.raises(ValueError, match=r"np_hip_index_remove_keep: index is a shard \(0 of 2\)"):
            hx.remove_ids([1], keep_attachments=True)
        with pytest.raises(ValueError, match=r"np_hip_index_append_rows: index is a shard \(0 of 2\)"):
            hx.append_arrays(*new, rows=api.AppendRows(columns={"i": np.arange(4)}))
        got = hx.get_column("i")
        assert got[0].tobytes() == want[0].tobytes() and got[1] is None and got[0].size == hx.info.shard_doc_end - hx.info.shard_doc_begin
    finally:
        hx.close()


# ---- concurrency and the C++ mirror ----------------------------------------------------------------------------------------------
def test_filtered_and_grouped_searches_beside_a_keeping_remove(corpus):
    """searches on a second thread see the old index with the old attachments or the new with the new, never a mixture"""
    base, sch, gids, n_groups = corpus(4097)
    qs = _queries(base)
    ids = np.concatenate([np.argsort(-base["doc_lengths"], kind="stable")[:2], np.arange(5, 4097, 2)])   # the queries' own documents leave
    keep = A.keep_mask(4097, ids)
    want_sch = _restated(sch, {n: A.shrunk_column(c.data, c.valid, keep) for n, c in sch.columns.items()})
    fresh = hip_index(R.shrunk_arrays(base, ids))
    try:
        _attach_raw(fresh, want_sch, gids[keep], n_groups)
        post = _answers(fresh, qs)
    finally:
        fresh.close()
    hx = hip_index(base, n_contexts=2)
    try:
        _attach_raw(hx, sch, gids, n_groups)
        pre = _answers(hx, qs)
        assert pre["filtered"] != post["filtered"] and pre["grouped"] != post["grouped"], "the queries do not tell the two states apart"
        removed, started, seen, errors = threading.Event(), threading.Event(), [], []

        def worker():
            try:
                after = 0
                while after < 2:
                    was_removed = removed.is_set()
                    seen.append((was_removed, _answers(hx, qs)))
                    started.set()
                    after += was_removed
            except Exception as e:   # noqa: BLE001
                errors.append(e)
                started.set()

        t = threading.Thread(target=worker, daemon=True)
        t.start()
        assert started.wait(60)
        api._check(api.lib().np_hip_index_remove_keep(hx._h, np.ascontiguousarray(ids, np.int64).ctypes.data, ids.size, None))
        removed.set()
        t.join(60)
        assert not errors and not t.is_alive(), errors
        for was_removed, got in seen:
            for k in post:
                assert got[k] == post[k] or (not was_removed and got[k] == pre[k]), k
        assert _answers(hx, qs) == post
    finally:
        hx.close()


def test_cpp_mirror_keeps_columns_and_groups(tmp_path):
    """tests/cpp/attach_index.cpp: next_plaid.hpp's remove_ids(keep_attachments) and append_arrays(rows) on a handle of a written
    directory, read back with get_column / get_groups"""
    spec, a = make_arrays(num_docs=70, seed=5, **GEOM)
    cut, wts = synth.bucket_tables(spec)
    d = tmp_path / "ix"
    npa.write_index_dir(str(d), a["centroids"], wts, a["doc_lengths"], a["codes"], a["residuals"], 4, bucket_cutoffs=cut,
                        cluster_threshold=0.3)
    T5 = int(a["doc_lengths"][:5].sum())   # the new documents: the tokens of the first five once more
    lens, codes, res = a["doc_lengths"][:5], a["codes"][:T5], a["residuals"][:T5]
    np.ascontiguousarray(lens, np.int64).tofile(tmp_path / "lens.bin")
    np.ascontiguousarray(codes, np.int64).tofile(tmp_path / "codes.bin")
    np.ascontiguousarray(res, np.uint8).tofile(tmp_path / "res.bin")
    exe = tmp_path / "attach_index"
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "attach_index.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    r = subprocess.run([str(exe), str(d), str(tmp_path), str(res.shape[1])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
