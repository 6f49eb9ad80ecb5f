"""tests/expand_limit_shapes.py bites: on the numpy restatement alone (no device) every case reaches the edge it names, the
route of the expand's cut and merge kernels restated in tests/expand_restate.py gives the lists expanded_arrays states, the
route of widen_codes_kernel gives codes.astype(uint32) with every entry written once, and each planted defect of either route
is rejected by a named case.  tests/test_gpu_expand_limits.py then holds the device to the same arrays.

As in tests/test_append_limits_cpu.py two planted defects cannot change the merged array and are rejected through the census,
which is held against array arithmetic that does not walk the route: a fast-path bound one entry too strict (expected_fast_quads)
and a tile whose first list is found from entry o0 - 1 (expected_tiles).
"""
import numpy as np
import pytest

import append_restate as A
import expand_limit_shapes as S
import expand_restate as E
from helpers import synth

MERGE = [c for c in S.all_cases() if c.merge]
WIDEN = [c for c in S.all_cases() if c.widen]
TILE = A.NP_MERGE_TILE

# planted defect -> (the case that rejects it, how: "array" = the merged array differs, "census" = the array is the same and the
#                    census differs from the arithmetic, anything else = the kind of RouteFault the planted line must end in)
REJECTED_BY = {
    "keep_le": ("every bisection class", "dropped"),               # list 6 holds document Nk itself
    "no_cut": ("hot list cut across tiles", "dropped"),            # 3000 dropped entries directly behind the kept ones
    "begin_new": ("cut alignments", "dropped"),                    # old_begin and the new offset part at the first cut list
    "new_lists_keep": ("every given pair to list K1 - 1, K 250 -> 255", "old_off"),   # old_off has K0 + 1 entries
    "fast_plus": ("cut alignments", "dropped"),                    # a quad ends one entry past a cut: the first dropped entry
    "fast_minus": ("cut alignments", "census"),                    # a quad ends exactly at a cut
    "no_shift": ("hot list cut across tiles", "array"),            # lists above 7 take pairs far from pair 0
    "pfx_inclusive": ("cut alignments", "old_ivf"),                # every list takes its neighbour's kept length
    "store_whole": ("residue total = 4097", "store"),              # a 16-byte store at the array's last entry
    "tile_prev": ("lists cut to nothing", "census"),               # tile 1 begins at list 20's first entry, behind list 8
    "gallop_lt": ("lists cut to nothing", "pairs"),                # off[hi] == o at the list behind the run
    "tail_dropped": ("widen Tk = 2105", "unwritten"),
    "tail_any_block": ("widen Tk = 2105", "twice"),                # two blocks: threads 0-7 of block 1 write the tail again
    "stride_block": ("widen Tk = 2105", "twice"),                  # block 0's second turn is block 1's first
}


def _route(case, defect=None):
    return E.cut_merge_route(*case.arith(), defect=defect)


@pytest.fixture(scope="module")
def routed():
    return {c.name: _route(c) for c in MERGE}


def _kept_codes(case):
    return np.asarray(case.base["codes"][:case.Tk]).astype(np.uint16)


@pytest.mark.parametrize("case", MERGE, ids=lambda c: c.name)
def test_route_equals_the_stated_lists(case, routed):
    out, new_off, census = routed[case.name]
    f = case.final()
    assert np.array_equal(out, f["ivf"]) and np.array_equal(np.diff(new_off), f["ivf_lengths"])
    want_off, keep, length, gain = E.expected_cut(*case.arith())
    assert np.array_equal(new_off, want_off) and census["kept"] == keep.sum() and census["P"] == gain.sum()
    assert census["fast"] == E.expected_fast_quads(*case.arith())
    assert census["shifts"] == E.expected_shifts(*case.arith())
    assert (census["ends_at_cut"], census["ends_past_cut"]) == E.expected_cut_quad_ends(*case.arith())
    assert [(t["list"], t["part"], t["empty_lists_before"]) for t in census["tiles"]] == E.expected_tiles(*case.arith())
    assert census["tile_first_list"] == [t[0] for t in E.expected_tiles(*case.arith())]
    assert census["classes"] == E.expected_classes(*case.arith())
    assert census["fast"] + census["slow"] == census["whole_stores"] + census["partial_stores"] == -(-census["total"] // 4)
    assert census["partial_stores"] == (census["total"] % 4 != 0)
    assert census["total"] == 0 or census["last_quad"] == (census["total"] - 1) % 4 + 1


def test_route_equals_the_stated_lists_after_a_second_expand():
    cases = [c for c in S.all_cases() if c.then is not None]
    assert cases
    for case in cases:
        first, (cen, given, n_replace) = case.final(), case.then
        n_keep = first["doc_lengths"].size - n_replace
        assert n_replace > 0 and cen.shape[0] > 0
        out, new_off, _ = E.cut_merge_route(first["ivf"], A.offsets(first["ivf_lengths"]), case.K1, case.K1 + cen.shape[0], n_keep,
                                            E.given_pairs(n_keep, given)[0])
        f = case.final2()
        assert np.array_equal(out, f["ivf"]) and np.array_equal(np.diff(new_off), f["ivf_lengths"])


@pytest.mark.parametrize("case", S.all_cases(), ids=lambda c: c.name)
def test_expanded_arrays_equal_the_rebuilt_lists(case):
    """for lists that state the codes, the cut list + the given ids is the list rebuilt from the final codes; centroids,
    doc_lengths, codes and residuals are the kept documents followed by the given ones"""
    for f, start, (cen, given, n_replace) in [(case.final(), case.start, (case.new_centroids, case.given, case.n_replace))] + (
            [(case.final2(), case.final(), case.then)] if case.then else []):
        n_keep = start["doc_lengths"].size - n_replace
        t_keep = int(start["doc_lengths"][:n_keep].sum())
        assert np.array_equal(f["centroids"], np.concatenate([start["centroids"], cen]))
        assert np.array_equal(f["doc_lengths"], np.concatenate([start["doc_lengths"][:n_keep], given[0]]))
        assert np.array_equal(f["codes"], np.concatenate([start["codes"][:t_keep], given[1]]))
        assert np.array_equal(f["residuals"], np.concatenate([start["residuals"][:t_keep], given[2]]))
        assert f["codes"].size == 0 or 0 <= f["codes"].min() and f["codes"].max() < f["centroids"].shape[0]
        ivf, il = synth.build_ivf(f["codes"], f["doc_lengths"], f["centroids"].shape[0])
        same = np.array_equal(f["ivf"], ivf) and np.array_equal(f["ivf_lengths"], il)
        assert same == case.states_codes
        off = A.offsets(f["ivf_lengths"])
        for c in np.nonzero(np.diff(off) > 1)[0][:4096]:     # every list ascends, the given entries included
            assert np.all(np.diff(f["ivf"][off[c]:off[c + 1]]) > 0)
        assert f["ivf"].size == 0 or f["ivf"].max() < f["doc_lengths"].size


def test_hot_list_premises(routed):
    case = S.case("hot list cut across tiles")
    _, new_off, census = routed[case.name]
    assert (case.N0, case.Nk, len(case.given[0])) == (9000, 6000, 6500)
    hot = [t for t in census["tiles"] if t["list"] == S.HOT]
    assert new_off[S.HOT] == 0 and hot[0]["n_old"] == 6000 and hot[0]["n_new"] == 6500
    assert any(0 < t["r"] < t["n_old"] for t in hot), "no tile starts strictly inside the kept part"
    assert any(t["r"] > t["n_old"] for t in hot), "no tile starts strictly inside the new part"
    assert any(t["r"] + TILE <= t["n_old"] for t in hot), "no whole tile in the kept part"
    assert any(t["r"] >= t["n_old"] and t["r"] + TILE <= t["n_old"] + t["n_new"] for t in hot), "no whole tile in the new part"
    parts = [p for _, p, _ in E.expected_tiles(*case.arith())]
    assert "kept" in parts and "new" in parts
    old_off = A.offsets(case.base["ivf_lengths"])
    old = case.base["ivf"][old_off[S.HOT]:old_off[S.HOT + 1]]
    assert old.size == 9000 and np.all(old[6000:] >= case.Nk), "the dropped entries lie directly behind the kept ones"


def test_residue_premises(routed):
    totals = {c.name: routed[c.name][2] for c in MERGE if c.name.startswith("residue")}
    assert len(totals) == 5
    t = sorted(v["total"] for v in totals.values())
    assert t[0] == 2 and t[1] % TILE == 0 and t[2] == t[1] + 1 and [x % 4 for x in t[1:]] == [0, 1, 2, 3]
    for name, v in totals.items():
        case = S.case(name)
        assert case.n_replace > 0 and np.all(case.given[0] == 1) and v["P"] == case.given[0].size, "every given document adds exactly one pair"
        assert v["last_quad"] == (v["total"] - 1) % 4 + 1
    assert len({id(S.case(n).base) for n in totals if n != "residue total = 2"}) == 1, "one fixed base"
    two = totals["residue total = 2"]
    assert two["fast"] == 0 and two["slow"] == 1 and two["partial_stores"] == 1 and two["whole_stores"] == 0
    assert len(totals[f"residue total = {t[2]}"]["tiles"]) == len(totals[f"residue total = {t[1]}"]["tiles"]) + 1      # a tile of a single entry


def test_cut_alignment_premises(routed):
    case = S.case("cut alignments")
    census = routed[case.name][2]
    assert census["shifts"] == E.expected_shifts(*case.arith()) == {0, 1, 2, 3}
    at, past = E.expected_cut_quad_ends(*case.arith())
    assert at > 0 and past > 0 and (census["ends_at_cut"], census["ends_past_cut"]) == (at, past)
    assert census["fast"] > 0 and "cut inside" in census["classes"]


def test_lists_cut_to_nothing_premises(routed):
    for name in ("lists cut to nothing", "lists cut to nothing at the end"):
        case = S.case(name)
        _, new_off, census = routed[name]
        lo, hi = case.notes["run"]
        assert case.K0 == 1024 and hi - lo + 1 >= 8
        il0 = case.base["ivf_lengths"]
        assert np.all(il0[lo:hi + 1] > 0) and all(k == "keeps none" for k in census["classes"][lo:hi + 1]), "the replaced tail alone holds the run"
        assert np.all(np.diff(new_off)[lo:hi + 1] == 0), "the given documents avoid the run"
        assert new_off[9] == TILE and census["tiles"][1]["r"] == 0
    a = routed["lists cut to nothing"][2]
    assert a["tiles"][1]["list"] == 20 and a["tiles"][1]["empty_lists_before"] == 11 and a["tiles"][1]["n_old"] > 0
    assert E.expected_tiles(*S.case("lists cut to nothing").arith())[1] == (20, "kept", 11)
    case = S.case("lists cut to nothing at the end")
    il = np.diff(routed[case.name][1])
    assert case.K1 == 1029 and np.all(il[1010:] == 0) and il[1009] > 0, "the last old lists and every new list are empty"


def test_new_list_premises(routed):
    seen = {}
    for case in MERGE:
        if case.name.startswith("every given pair to list K1 - 1"):
            census = routed[case.name][2]
            assert np.all(case.given[1] == case.K1 - 1) and case.n_replace > 0
            out = routed[case.name][0]
            assert np.array_equal(out[-37:], np.arange(case.Nk, case.Nk + 37)), "the given entries are the array's tail"
            seen[(case.K0, case.K1)] = (census["keep_blocks"], census["keep_threads_in_last_block"])
            assert census["classes"][case.K0:] == ["new"] * (case.K1 - case.K0)
    assert seen == {(250, 255): (1, 256), (250, 256): (2, 1), (250, 257): (2, 2), (256, 257): (2, 2)}
    assert int(np.ceil(np.log2(257))) == 9 and int(np.ceil(np.log2(256))) == 8      # kbits of the pairs' sort
    far = S.case("only list K1 - 1 is used, K1 = 65600")
    out, new_off, census = routed[far.name]
    assert (far.K0, far.K1) == (65590, 65600) and np.all(np.diff(new_off)[:-1] == 0) and out.size > 0
    assert census["longest_gallop"] == 16


def test_bisection_class_premises(routed):
    case = S.case("every bisection class")
    census = routed[case.name][2]
    assert (case.N0, case.Nk) == (40, 30)
    for c, k in S.CLASS_OF.items():
        assert census["classes"][c] == k, (c, census["classes"][c])
    assert set(census["classes"]) == set(E.CLASSES)
    off = A.offsets(case.base["ivf_lengths"])
    six = case.base["ivf"][off[6]:off[7]].tolist()
    assert case.Nk - 1 in six and case.Nk in six, "the cut falls between Nk - 1 and Nk"
    assert case.base["ivf_lengths"][7] == 1 and case.base["ivf_lengths"][8] == 1, "one-entry lists on both sides of the cut"
    none = S.case("nothing replaced, new centroids")
    classes = routed[none.name][2]["classes"]
    assert none.n_replace == 0 and none.K1 > none.K0 and none.Nk == none.N0 > none.base["ivf"].max()
    assert set(classes[:none.K0]) <= {"keeps all", "empty"} and "keeps all" in classes


def test_raw_list_premises(routed):
    case = S.case("raw list through the cut")
    lens = case.given[0]
    assert lens[0] > A.NP_UNIQ_MAX and np.all(lens[1:] <= 2) and case.n_replace > 0
    pairs, before = case.pairs()
    assert before - pairs.size == lens[0] - len(case.notes["raw_codes"]) > 0
    out, _, _ = routed[case.name]
    where = np.nonzero(out == case.Nk)[0]
    assert where.size == len(case.notes["raw_codes"]) and len(set((where // TILE).tolist())) >= 2, "the document's entries lie in one tile"
    assert max(case.notes["raw_codes"]) >= case.K0, "one of its lists is new"


def test_inexact_list_premises():
    for where in ("kept", "replaced"):
        miss = S.case(f"lists that miss a pair of a {where} document")
        extra = S.case(f"lists with extra pairs of {where} documents")
        stated = synth.build_ivf(miss.base["codes"], miss.base["doc_lengths"], 256)[0]
        assert miss.base["ivf"].size == stated.size - 1 and extra.base["ivf"].size == stated.size + extra.notes["n_extra"]
        assert extra.notes["n_extra"] > 100
        for c in (miss, extra):
            cell, doc = S.entries(c.base)
            same = cell[1:] == cell[:-1]
            assert np.all(doc[1:][same] > doc[:-1][same]), "the lists ascend"
        assert (miss.notes["victim"] < miss.Nk) == (where == "kept")
        fin = extra.final()
        rebuilt = synth.build_ivf(fin["codes"], fin["doc_lengths"], extra.K1)[0]
        assert fin["ivf"].size - rebuilt.size == (extra.notes["n_extra"] if where == "kept" else 0)
        fin = miss.final()
        assert synth.build_ivf(fin["codes"], fin["doc_lengths"], miss.K1)[0].size - fin["ivf"].size == (where == "kept")


def test_empty_side_premises(routed):
    a, b, c, d = (S.case(n) for n in ("all-empty base", "emptied handle", "everything replaced by empty documents",
                                      "a replaced tail of empty documents"))
    assert a.N0 == 5 and a.T0 == 0 and a.base["ivf"].size == 0 and a.T1 > 0
    assert b.remove_all and b.N0 == 0 and b.n_replace == 0 and b.base["doc_lengths"].size > 0 and b.T1 > 0
    cc = routed[c.name][2]
    assert c.n_replace == c.N0 > 0 and (cc["P"], cc["total"], c.Tk, c.T1) == (0, 0, 0, 0) and cc["tiles"] == []
    assert d.n_replace > 0 and d.Tk == d.T0 and np.all(d.base["doc_lengths"][d.Nk:] == 0)


@pytest.mark.parametrize("defect", E.DEFECTS)
def test_planted_defects_are_rejected(defect):
    name, how = REJECTED_BY[defect]
    case = S.case(name)
    if defect in E.WIDEN_DEFECTS:
        with pytest.raises(A.RouteFault) as e:
            E.widen_route(_kept_codes(case), case.Tk, defect=defect)
        assert e.value.kind == how, e.value
        return
    want = case.final()["ivf"]
    if how not in ("array", "census"):      # the planted line's own fault, not any fault
        with pytest.raises(A.RouteFault) as e:
            _route(case, defect)
        assert e.value.kind == how, e.value
        return
    out, _, census = _route(case, defect)
    if how == "array":
        assert not np.array_equal(out, want), f"{defect} went unnoticed on {name}"
    else:
        assert np.array_equal(out, want), f"{defect} is expected to leave the array alone"
        tiles = [(t["list"], t["part"], t["empty_lists_before"]) for t in census["tiles"]]
        arith = (census["fast"] == E.expected_fast_quads(*case.arith()), tiles == E.expected_tiles(*case.arith()),
                 census["tile_first_list"] == [t[0] for t in E.expected_tiles(*case.arith())])
        assert not all(arith), f"{defect} went unnoticed on {name}"


def test_every_partial_total_rejects_a_whole_store():
    for c in MERGE:
        if c.final()["ivf"].size % 4:
            with pytest.raises(A.RouteFault) as e:
                _route(c, "store_whole")
            assert e.value.kind == "store"


# ---- widening ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WIDEN, ids=lambda c: c.name)
def test_widen_route_equals_the_codes(case):
    src = _kept_codes(case)
    assert case.Tk == case.notes["Tk"] and case.K0 <= 65536 < case.K1
    out, census = E.widen_route(src, case.Tk)
    assert out.dtype == np.uint32 and np.array_equal(out, src.astype(np.uint32))
    assert census == E.expected_widen(case.Tk)


@pytest.mark.parametrize("grid", [None, 1, 2])
def test_widen_route_for_every_small_n(grid):
    rng = np.random.default_rng(5)
    src = rng.integers(0, 65536, 6000).astype(np.uint16)
    for n in list(range(41)) + [2047, 2048, 2049, 4096 + 9, 6000]:      # with grid 1 and 2: several turns of the stride loop
        out, census = E.widen_route(src, n, grid=grid)
        assert np.array_equal(out, src[:n].astype(np.uint32)) and census == E.expected_widen(n, grid)
    assert E.widen_route(src, 6000, grid=1)[1]["max_turns"] == 3


def test_widening_premises():
    by_tk = {c.notes["Tk"]: c for c in WIDEN}
    assert {tk % 8 for tk in by_tk if 2000 <= tk < 2200} == set(range(8))
    assert {0, 7, 8} <= set(by_tk)
    for tk, c in by_tk.items():
        assert (c.K0, c.K1, c.base["nbits"]) == (S.WIDE_K0, S.WIDE_K1, 2)
        want = E.expected_widen(tk)
        assert want["grid"] == (2 if tk >= 2056 else 1) and want["max_turns"] == (tk >= 8)
        if tk >= 2000:
            assert want["groups"] > 64, "the groups span more than one wave"
        src = _kept_codes(c)
        n8 = tk >> 3
        if n8 and tk != 8:
            assert {0, S.WIDE_K0 - 1} <= set(src[8 * n8 - 8:8 * n8].tolist())
        if tk - 8 * n8 >= 2:
            assert {0, S.WIDE_K0 - 1} <= set(src[8 * n8:tk].tolist())
        elif tk - 8 * n8 == 1:
            assert src[tk - 1] == S.WIDE_K0 - 1
        assert c.given[1].max() == c.K1 - 1 and 65536 in c.given[1] or tk == 0
    assert by_tk[0].n_replace == by_tk[0].N0 and by_tk[7].n_replace > 0
    assert sum(c.env == dict(NP_TOK_SORT="1") for c in WIDEN) == 1 and sum(c.reserve is not None for c in WIDEN) == 1


def test_the_stride_loops_second_turn():
    """the large case's premise: at Tk = 8 * (8192 * 256 + 1) + 5 the grid is capped, thread 0 alone takes a second turn, and
    every entry is still written exactly once; one group fewer and no thread does"""
    n = S.BIG_TK
    assert n == 16_777_229 and E.widen_grid(n) == E.WIDEN_MAX_BLOCKS
    assert E.expected_widen(n)["max_turns"] == 2 and E.expected_widen(n - 8)["max_turns"] == 1
    src = S.big_widen_codes()
    out, census = E.widen_route(src, n)
    assert np.array_equal(out, src.astype(np.uint32)) and census == E.expected_widen(n)
    assert census == dict(grid=8192, groups=8192 * 256 + 1, tail=5, max_turns=2)
    assert {0, S.WIDE_K0 - 1} <= set(src[-5:].tolist()) and {0, S.WIDE_K0 - 1} <= set(src[-13:-5].tolist())


# ---- inverse norms and capacity ----------------------------------------------------------------------------------------------------
def test_inverse_norm_premises():
    seen = set()
    for c in S.all_cases():
        if c.name.startswith("inverse norms"):
            assert c.Tk % 64 == c.notes["rem"] and int(c.given[0].sum()) == c.notes["n_tok"] and c.n_replace > 0 and c.decompress_all
            assert c.given[1].min() >= c.K0, "the given tokens sit on new centroids"
            seen.add((c.Tk % 64, int(c.given[0].sum())))
    assert seen == {(r, n) for r in (0, 1, 63) for n in (1, 64, 65)}


def test_capacity_premises():
    cases = {c.name.split(": ")[1]: c for c in S.all_cases() if c.name.startswith("capacity")}
    need = {k: (c.N1 - c.N0, c.T1 - c.T0) for k, c in cases.items()}
    r = {k: c.reserve for k, c in cases.items()}
    assert all(c.n_replace > 0 for c in cases.values())
    k = "documents reserved, tokens not"
    assert r[k][0] >= need[k][0] and r[k][1] < need[k][1]
    k = "tokens reserved, documents not"
    assert r[k][0] < need[k][0] and r[k][1] >= need[k][1]
    k = "the reservation filled exactly"
    assert r[k] == need[k] and S.capacity_after(cases[k]) == (cases[k].N0 + r[k][0], cases[k].T0 + r[k][1])
    k = "one document and one token beyond"
    assert (r[k][0] + 1, r[k][1] + 1) == need[k] and S.capacity_after(cases[k]) == (cases[k].N1, cases[k].T1)
    c = S.case("fewer tokens than before")
    assert c.T1 < c.T0 and c.n_replace > 0 and S.capacity_after(c) == (c.N0, c.T0)
