"""tests/append_limit_shapes.py bites: on the numpy restatement alone (no device) every case reaches the edge it names, the
route of ivf_cut_merge_kernel on an append's arguments, restated in tests/append_restate.py, gives the lists grown_arrays
states, and each planted defect of that route is rejected by a named case.tests/test_gpu_append_limits.py then holds the device to the same arrays.

Two of the planted defects cannot change the merged array, and the test says so instead of pretending: a fast-path bound that
is one entry too STRICT only sends a quad down the entry-by-entry path, and a tile whose first list is found from entry o0 - 1
starts its gallop one list early and arrives at the same list.  Both are rejected through the census, which is held against
array arithmetic that does not walk the route (expected_fast_quads, expected_tile_first_lists).
"""
import numpy as np
import pytest

import append_limit_shapes as S
import append_restate as A
import expand_restate as X
from test_gpu_index_append import _concat

MERGE = [c for c in S.all_cases() if c.merge]
TILE = A.NP_MERGE_TILE

# planted defect -> (the case that rejects it, how: "array" = the merged array differs, "census" = the array is the same and the
#                    census differs from the arithmetic, anything else = the kind of RouteFault the planted line must end in)
REJECTED_BY = {
    "gallop_lt": ("sparse lists", "pairs"),                       # off[hi] == o at every list behind empty lists
    "fast_plus": ("hot list across tiles", "array"),             # a quad ends one entry past an old part with new entries behind it
    "fast_minus": ("hot list across tiles", "census"),           # a quad ends exactly at the end of an old part
    "no_shift": ("hot list across tiles", "array"),              # lists above 7 take pairs far from pair 0
    "store_whole": ("residue total = 4097", "store"),            # a 16-byte store at the array's last entry
    "tile_prev": ("sparse lists", "census"),                     # tile 1 begins at list 16's first entry, behind list 8
    "keep_dups": ("raw list over a tile edge", "array"),         # 4500 tokens over five codes
}


def _route(case, defect=None):
    pairs = case.pairs(unique=defect != "keep_dups")[0]
    return A.merge_route(case.base["ivf"], A.offsets(case.base["ivf_lengths"]), pairs, case.K, defect=defect)


@pytest.fixture(scope="module")
def routed():
    return {c.name: _route(c) for c in MERGE}


def _arith(case):
    return A.offsets(case.base["ivf_lengths"]), case.pairs()[0], case.K


@pytest.mark.parametrize("case", MERGE, ids=lambda c: c.name)
def test_route_equals_the_stated_lists(case, routed):
    out, new_off, census = routed[case.name]
    g = case.grown()
    assert np.array_equal(out, g["ivf"]) and np.array_equal(np.diff(new_off), g["ivf_lengths"])
    assert census["fast"] == A.expected_fast_quads(*_arith(case))
    assert census["tile_first_list"] == A.expected_tile_first_lists(*_arith(case))
    assert census["fast"] + census["slow"] == census["whole_stores"] + census["partial_stores"] == -(-census["total"] // 4)
    assert census["partial_stores"] == (census["total"] % 4 != 0) and census["last_quad"] == (census["total"] - 1) % 4 + 1


@pytest.mark.parametrize("case", S.all_cases(), ids=lambda c: c.name)
def test_an_append_is_the_cut_merge_that_cuts_nothing(case, routed):
    """what folding the append's kernel into the expand's rests on: the cut-merge route with K0 = K1 = K, Nk = the old
    documents and the old offsets themselves as old_begin and kept_pfx writes, entry for entry, the array and the offsets of
    merge_route.  ivf_keep_kernel and its scan, which the append's call leaves out, would have given the same two arrays."""
    old_ivf, old_off, pairs = case.base["ivf"], A.offsets(case.base["ivf_lengths"]), case.pairs()[0]
    want = routed[case.name] if case.name in routed else _route(case)
    for uncut in (True, False):
        out, new_off, census = X.cut_merge_route(old_ivf, old_off, case.K, case.K, case.n_old, pairs, uncut=uncut)
        assert np.array_equal(out, want[0]) and np.array_equal(new_off, want[1])
        assert all(census[k] == want[2][k] for k in ("fast", "slow", "whole_stores", "partial_stores", "tile_first_list", "total", "P"))
        assert set(census["classes"]) <= {"keeps all", "empty"} and census["kept"] == old_off[-1]


@pytest.mark.parametrize("case", S.all_cases(), ids=lambda c: c.name)
def test_grown_arrays_equal_the_rebuilt_lists(case):
    """for a base whose lists state the codes, list c + the new ids is the list rebuilt from all codes"""
    g = case.grown()
    want = _concat(case.base, case.new)
    for k in ("doc_lengths", "codes", "residuals"):
        assert np.array_equal(g[k], want[k])
    same = np.array_equal(g["ivf"], want["ivf"]) and np.array_equal(g["ivf_lengths"], want["ivf_lengths"])
    assert same == case.states_codes
    il = A.offsets(g["ivf_lengths"])
    for c in np.nonzero(np.diff(il) > 1)[0][:4096]:     # every list ascends, the new entries included
        assert np.all(np.diff(g["ivf"][il[c]:il[c + 1]]) > 0)


def test_hot_list_premises(routed):
    _, _, census = routed["hot list across tiles"]
    hot = [t for t in census["tiles"] if t["list"] == S.HOT]
    assert hot[0]["n_old"] > TILE and hot[0]["n_new"] > TILE
    assert any(0 < t["r"] < t["n_old"] for t in hot), "no tile starts strictly inside the old part"
    assert any(t["r"] > t["n_old"] for t in hot), "no tile starts strictly inside the new part"
    assert any(t["r"] + TILE <= t["n_old"] for t in hot), "no whole tile in the old part"
    assert any(t["r"] >= t["n_old"] and t["r"] + TILE <= t["n_old"] + t["n_new"] for t in hot), "no whole tile in the new part"
    ends_at, ends_past = A.quad_ends(*_arith(S.case("hot list across tiles")))
    assert ends_at > 0 and ends_past > 0      # where the fast path's bound decides, in both directions


def test_residue_premises(routed):
    totals = {c.name: routed[c.name][2] for c in MERGE if c.name.startswith("residue")}
    assert len(totals) == 5
    t = sorted(v["total"] for v in totals.values())
    assert t[0] == 2 and t[1] % TILE == 0 and t[2] == t[1] + 1 and [x % 4 for x in t[1:]] == [0, 1, 2, 3]
    for name, v in totals.items():
        new = S.case(name).new[0]
        assert np.all(new == 1) and v["P"] == new.size, "every appended document adds exactly one pair"
        assert v["last_quad"] == (v["total"] - 1) % 4 + 1
    two = totals["residue total = 2"]
    assert two["fast"] == 0 and two["slow"] == 1 and two["partial_stores"] == 1 and two["whole_stores"] == 0
    assert len(routed["residue total = 4097"][2]["tiles"]) == 2      # a tile of a single entry
    assert len(routed["residue total = 4096"][2]["tiles"]) == 1


def test_sparse_list_premises(routed):
    case = S.case("sparse lists")
    _, new_off, census = routed["sparse lists"]
    assert case.K == 1024 and set(case.base["doc_lengths"].tolist()) == {1} and set(case.new[0].tolist()) == {1, 2}
    assert census["max_lists_in_quad"] >= 3 and census["alternates"]
    il = np.diff(new_off)
    assert np.all(il[np.arange(1024) % 8 != 0] == 0), "seven empty lists between any two used ones"
    t1 = census["tiles"][1]
    assert t1["r"] == 0 and t1["empty_lists_before"] >= 1 and t1["list"] == 16


def test_first_and_last_list_premises(routed):
    first, last, far = (S.case(n) for n in ("every new pair to list 0", "every new pair to list K - 1, K = 257",
                                            "only list K - 1 is used, K = 65600"))
    assert np.all(first.new[1] == 0)
    assert last.K == 257 and np.all(last.new[1] == 256) and int(np.ceil(np.log2(last.K))) == 9
    out, new_off, _ = routed[last.name]
    assert np.array_equal(out[-37:], np.arange(300, 337)), "the new entries are the array's tail"
    assert far.K == 65600 and np.all(far.base["ivf_lengths"][:-1] == 0)
    assert routed[far.name][2]["longest_gallop"] >= 16


def test_raw_list_premises(routed):
    case = S.case("raw list over a tile edge")
    lens = case.new[0]
    assert lens[0] > A.NP_UNIQ_MAX and np.all(lens[1:] <= 2)
    pairs, before = case.pairs()
    assert before != pairs.size and before - pairs.size == lens[0] - len(S.RAW_CODES)
    assert A.new_pairs(case.n_old, (lens[1:], case.new[1][lens[0]:], None))[0].size > TILE     # further pairs of short documents
    out, _, _ = routed[case.name]
    where = np.nonzero(out == case.n_old)[0]
    assert where.size == len(S.RAW_CODES) and len(set((where // TILE).tolist())) >= 2, "the document's entries lie in one tile"


def test_inexact_list_premises():
    miss, extra = S.case("lists that miss a pair"), S.case("lists with extra pairs")
    for c in (miss, extra):
        cell, doc = S.entries(c.base)
        same = cell[1:] == cell[:-1]
        assert np.all(doc[1:][same] > doc[:-1][same]), "the lists ascend"
    stated = _concat(miss.base, (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, S.PD), np.uint8)))
    assert miss.base["ivf"].size == stated["ivf"].size - 1 and extra.base["ivf"].size == stated["ivf"].size + extra.notes["n_extra"]
    assert extra.notes["n_extra"] > 100
    have = set(zip(*(x.tolist() for x in S.entries(extra.base))))
    assert set(zip(*(x.tolist() for x in S.entries(stated)))) <= have, "extra pairs only: every stated pair is there"


@pytest.mark.parametrize("defect", A.DEFECTS)
def test_planted_defects_are_rejected(defect):
    name, how = REJECTED_BY[defect]
    case = S.case(name)
    want = case.grown()["ivf"]
    if how not in ("array", "census"):      # the planted line's own fault, not any fault: the list it stops at has no such pair
        with pytest.raises(A.RouteFault) as e:
            _route(case, defect)
        assert e.value.kind == how, e.value
        return
    out, _, census = _route(case, defect)
    if how == "array":
        assert not np.array_equal(out, want), f"{defect} went unnoticed on {name}"
    else:
        assert np.array_equal(out, want), f"{defect} is expected to leave the array alone"
        arith = (census["fast"] == A.expected_fast_quads(*_arith(case)),
                 census["tile_first_list"] == A.expected_tile_first_lists(*_arith(case)))
        assert not all(arith), f"{defect} went unnoticed on {name}"


def test_every_partial_total_rejects_a_whole_store():
    for c in MERGE:
        if A.offsets(c.grown()["ivf_lengths"])[-1] % 4:
            with pytest.raises(A.RouteFault) as e:
                _route(c, "store_whole")
            assert e.value.kind == "store"


# ---- rebuilt layout --------------------------------------------------------------------------------------------------------
def test_stride_premises():
    for name in ("stride grows", "stride shrinks", "wide codes"):
        c = S.case(name)
        before, after = A.stride_bytes(c.base), A.stride_bytes(c.grown())
        assert (before[0], after[0]) == c.notes["strides"], (name, before, after)
    c = S.case("stride shrinks")
    assert A.stride_bytes(c.base)[1] == 0 and A.stride_bytes(c.grown())[1] == 10, "ten lists move to the overflow region"
    over = A.overflow_list_lengths(c.grown())
    assert sorted(over.tolist()) == sorted(S.LONG_ULEN) and {1, 2, 3} <= set((over % 4).tolist())    # NP_ULIST_ALIGN = 4
    assert S.case("wide codes").K > 65536 and A.code_bytes(S.case("wide codes").base) == 4


def test_range_premises():
    got = {}
    for c in S.all_cases():
        if c.name.startswith("range table"):
            assert c.base["doc_lengths"].min() >= 1 and c.base["doc_lengths"].max() <= 3
            got[(c.n_old, c.new[0].size)] = (A.n_ranges(c.n_old), A.n_ranges(c.n_old + c.new[0].size))
    assert got == {(32767, 1): (1, 1), (32768, 1): (1, 2), (32767, 2): (1, 2)}


def test_capacity_premises():
    cases = {c.name.split(": ")[1]: c for c in S.all_cases() if c.name.startswith("capacity")}
    n = {k: (c.new[0].size, int(c.new[0].sum())) for k, c in cases.items()}
    r = {k: c.reserve for k, c in cases.items()}
    k = "documents reserved, tokens not"
    assert r[k][0] >= n[k][0] and r[k][1] < n[k][1]
    k = "tokens reserved, documents not"
    assert r[k][0] < n[k][0] and r[k][1] >= n[k][1]
    k = "the reservation filled exactly"
    assert r[k] == n[k] and S.capacity_after(cases[k]) == (cases[k].n_old + r[k][0], int(cases[k].base["doc_lengths"].sum()) + r[k][1])
    k = "one document and one token beyond"
    assert (r[k][0] + 1, r[k][1] + 1) == n[k]


def test_inverse_norm_premises():
    seen = set()
    for c in S.all_cases():
        if c.name.startswith("inverse norms"):
            t0 = int(c.base["doc_lengths"].sum())
            assert t0 % 64 == c.notes["rem"] and int(c.new[0].sum()) == c.notes["n_tok"]
            seen.add((t0 % 64, int(c.new[0].sum())))
    assert seen == {(r, n) for r in (0, 63) for n in (1, 64, 65)}


def test_empty_base_premises():
    c = S.case("all-empty base")
    assert c.base["doc_lengths"].size > 0 and c.base["doc_lengths"].sum() == 0 and c.base["ivf"].size == 0
    assert c.new[0].sum() > 0
