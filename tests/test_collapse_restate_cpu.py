"""The reference of the grouped entry points can be trusted and its checker can fail: tests/collapse_restate.py's walk is
pinned to hand-written answers (collapse_by_file's behaviour among them), agrees with an independent numpy formulation and
with the kernel's own route (sorted (group, rank) keys, heads, a leader bitmap over ranks) restated on the host, and the
checker rejects planted defects.  Also builds and runs the stand-alone check of the entry points' host code
(np_group_plan.h), plainly and under ASan / UBSan, and pins set_groups' key mapping.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT

import collapse_restate as R
from next_plaid_amd import api


def bits(*xs):
    return np.asarray(xs, np.float32).view(np.uint32).tolist()


# ---- the walk, by hand ----------------------------------------------------------------------------------
def test_collapse_by_file_folds_later_units_and_stops_at_top_k_files():
    """colgrep/src/index/mod.rs:4394-4413 with group_size = 1: the first unit of a file leads, a later unit of an admitted
    file is folded into it, a new file after top_k files is skipped -- and a unit of an ADMITTED file after that point still
    folds."""
    file_of = np.array([0, 0, 1, 1, 2, 2, 3], np.int32)           # units 0..6 in files 0..3
    ranked = [2, 0, 3, 4, 1, 6, 5]                                 # files: 1 0 1 2 0 3 2
    sc = [9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0]
    got = R.walk(ranked, sc, file_of, top_k=2, group_size=1)
    assert got == [(1, [2], bits(9.0), 2), (0, [0], bits(8.0), 2)]
    got = R.walk(ranked, sc, file_of, top_k=3, group_size=1)
    assert got == [(1, [2], bits(9.0), 2), (0, [0], bits(8.0), 2), (2, [4], bits(6.0), 2)]   # file 3 came fourth: skipped


def test_member_limit_totals_duplicates_and_order():
    g = np.array([5, 5, 5, 7, 7, 9], np.int32)
    ranked = [3, 0, 1, 3, 2, 5, 4, 0]                              # 7 5 5 7 5 9 7 5; document 3 and 0 twice
    got = R.walk(ranked, None, g, top_k=2, group_size=2)
    assert got == [(7, [3, 3], None, 3), (5, [0, 1], None, 4)]     # duplicates are separate entries; 9 is skipped
    got = R.walk(ranked, None, g, top_k=5, group_size=9)
    assert got == [(7, [3, 3, 4], None, 3), (5, [0, 1, 2, 0], None, 4), (9, [5], None, 1)]
    assert R.walk([], None, g, 3, 2) == []
    assert R.walk([1, 99, -1, 0], None, g, 3, 2) == [(5, [1, 0], None, 2)]   # the device form: an id out of range is absent


def test_padded_layout():
    g = np.array([1, 0, 1], np.int32)
    nan = np.array([0x7FC00123], np.uint32).view(np.float32)[0]    # a NaN with a payload goes through bit for bit
    ids, sc, grp, mem, tot, cnt = R.walk_batch([2, 1, 0, 0] + [0] * 4, [1.0, nan, 0.5, 0.0] + [0.0] * 4, [3, 0], 4, g, 2, 2)
    assert ids.tolist() == [[[2, 0], [1, 0]], [[0, 0], [0, 0]]]
    assert sc[0].tolist() == [bits(1.0, 0.5), [0x7FC00123, 0]]
    assert grp.tolist() == [[1, 0], [0, 0]] and mem.tolist() == [[2, 1], [0, 0]] and tot.tolist() == [[2, 1], [0, 0]]
    assert cnt.tolist() == [2, 0]
    assert R.walk_batch([2, 1, 0, 0], None, [9], 4, g, 2, 2)[5].tolist() == [2]   # a count is clamped to the stride


# ---- other routes to the same answer ------------------------------------------------------------------------
def kernel_route(ids, scores, group_ids, top_k, group_size):
    """collapse_kernel's route on the host: keys (group << 32 | rank) sorted, heads, member index = position - head, leaders
    marked in a bitmap over RANKS, ordinal = leader bits below the leader's rank, the run's last entry writes the figures."""
    ids = np.asarray(ids, np.int64)
    sb = None if scores is None else np.asarray(scores, np.float32).view(np.uint32)
    valid = [r for r in range(ids.size) if 0 <= ids[r] < len(group_ids)]
    keys = sorted((int(group_ids[ids[r]]) << 32) | r for r in valid)
    lead = 0
    heads = []
    for p, k in enumerate(keys):
        if p == 0 or keys[p - 1] >> 32 != k >> 32:
            heads.append(p)
            lead |= 1 << (k & 0xFFFFFFFF)
    n_adm = min(bin(lead).count("1"), top_k)
    out = [[0, [], None if sb is None else [], 0] for _ in range(n_adm)]
    h = -1
    for p, k in enumerate(keys):
        if p == 0 or keys[p - 1] >> 32 != k >> 32:
            h = p
        lr = keys[h] & 0xFFFFFFFF
        ordinal = bin(lead & ((1 << lr) - 1)).count("1")
        if ordinal >= top_k:
            continue
        m, r = p - h, k & 0xFFFFFFFF
        if m < group_size:
            assert len(out[ordinal][1]) == m                       # slots fill in member order
            out[ordinal][1].append(int(ids[r]))
            if sb is not None:
                out[ordinal][2].append(int(sb[r]))
        if p + 1 == len(keys) or keys[p + 1] >> 32 != k >> 32:
            out[ordinal][0], out[ordinal][3] = k >> 32, m + 1
    return [tuple(o) for o in out]


def random_case(rng):
    n_docs = int(rng.integers(1, 60))
    n_groups = int(rng.integers(1, 12))
    g = rng.integers(0, n_groups, n_docs).astype(np.int32)
    if rng.random() < 0.2:
        g[:] = g[0]                                                # one group
    n = int(rng.integers(0, 90))
    ids = rng.integers(0, n_docs, n)                               # with duplicates
    sc = rng.standard_normal(n).astype(np.float32) if rng.random() < 0.7 else None
    return g, ids, sc, int(rng.integers(1, 9)), int(rng.integers(1, 6))


def test_three_formulations_agree_on_random_lists():
    rng = np.random.default_rng(20240)
    folded = skipped = 0
    for _ in range(400):
        g, ids, sc, top_k, group_size = random_case(rng)
        want = R.walk(ids, sc, g, top_k, group_size)
        assert R.walk_numpy(ids, sc, g, top_k, group_size) == want
        assert kernel_route(ids, sc, g, top_k, group_size) == want
        folded += any(t > len(m) for _, m, _, t in want)
        skipped += len(set(g[ids].tolist())) > top_k
    assert folded > 50 and skipped > 50                            # the cases are not vacuous


# ---- planted defects ------------------------------------------------------------------------------------------
def defect_members_of_unadmitted(ids, sc, g, top_k, gs):
    """every group of the list is kept, admitted or not"""
    return R.walk(ids, sc, g, 10 ** 9, gs)


def defect_total_capped(ids, sc, g, top_k, gs):
    return [(gr, m, s, min(t, gs)) for gr, m, s, t in R.walk(ids, sc, g, top_k, gs)]


def defect_groups_by_id(ids, sc, g, top_k, gs):
    return sorted(R.walk(ids, sc, g, top_k, gs), key=lambda x: x[0])


def defect_nulls_split(ids, sc, g, top_k, gs):
    """every document of the NULL group (the last id) is a group of its own"""
    null = int(g.max())
    g2 = g.astype(np.int64).copy()
    at = np.nonzero(g == null)[0]
    g2[at] = null + np.arange(at.size)
    return [(min(gr, null), m, s, t) for gr, m, s, t in R.walk(ids, sc, g2, top_k, gs)]


DEFECTS = {"members admitted for a non-admitted group": defect_members_of_unadmitted,
           "total capped at group_size": defect_total_capped,
           "groups ordered by id": defect_groups_by_id,
           "NULL documents split into singletons": defect_nulls_split}


def planted_case():
    keys = ["b", None, "a", None, "b", "c", None, "a", "c", "c"]   # documents 0..9; None -> group 3
    g, values, n_groups = api.group_ids_of_keys(keys)
    assert values == ["a", "b", "c"] and n_groups == 4 and g.tolist() == [1, 3, 0, 3, 1, 2, 3, 0, 2, 2]
    ids = np.array([5, 1, 0, 3, 8, 6, 4, 2, 9, 7, 0, 0], np.int64)  # c N b N c N b a c a | two entries past the count
    sc = np.linspace(5, 1, 12).astype(np.float32)
    return g, ids, sc


@pytest.mark.parametrize("name", list(DEFECTS))
def test_rejects(name):
    """Two lists, the second empty.  A group past top_k has no row of its own: a kernel that writes its members anyway lands in
    the next query's row, which the walk leaves all zeros."""
    g, ids, sc = planted_case()
    top_k, gs, count, stride = 3, 2, 10, 12
    ids2, sc2 = np.r_[ids, np.zeros(stride, np.int64)], np.r_[sc, np.zeros(stride, np.float32)]
    want = R.walk_batch(ids2, sc2, [count, 0], stride, g, top_k, gs)
    R.check(want, want, "the reference itself")
    wrong = DEFECTS[name](ids[:count], sc[:count], g, top_k, gs)
    assert len(wrong) <= 2 * top_k
    got = list(R.padded([wrong[:top_k], wrong[top_k:]], top_k, gs))
    got[5] = want[5].copy()                                        # (the counts stay right: only the rows are wrong)
    with pytest.raises(AssertionError):
        R.check(got, want, name)


def test_rejects_a_count_taken_from_the_stride():
    g, ids, sc = planted_case()
    want = R.walk_batch(ids, sc, [10], 12, g, 4, 3)
    got = R.walk_batch(ids, sc, [12], 12, g, 4, 3)                 # the two entries past the count were walked too
    with pytest.raises(AssertionError):
        R.check(got, want, "count from the stride")


def test_rejects_one_flipped_score_bit_and_dirty_padding():
    g, ids, sc = planted_case()
    want = R.walk_batch(ids, sc, [10], 12, g, 3, 2)
    for field, at in ((1, (0, 0, 1)), (0, (0, 2, 1)), (3, (0, 1))):
        got = [None if x is None else x.copy() for x in want]
        got[field][at] ^= 1
        with pytest.raises(AssertionError):
            R.check(got, want, "one bit")


# ---- the host code of the entry points --------------------------------------------------------------------------
def test_host_code_of_the_grouped_entries_stands_alone(tmp_path):
    """tests/cpp/group_plan_check.cpp: np_group_plan.h with the host compiler alone (no device, no library), then the same
    program built with -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "group_plan_check.cpp")
    inc = os.path.join(ROOT, "next-plaid_amd", "csrc")
    for name, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / f"group_plan_check_{name}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, src, "-o", str(exe)])
        out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "all checks passed" in out.stdout, name + ": " + out.stdout + out.stderr


def test_the_plan_constants_are_the_headers():
    with open(os.path.join(ROOT, "include", "nextplaid_hip.h")) as f:
        assert f"#define NP_GROUP_MAX_LIST {api.NP_GROUP_MAX_LIST}\n" in f.read()
    with open(os.path.join(ROOT, "next-plaid_amd", "csrc", "np_group_plan.h")) as f:
        assert f"NP_GROUP_LIST_CAP = {api.NP_GROUP_MAX_LIST};" in f.read()


# ---- set_groups' key mapping ------------------------------------------------------------------------------------
def test_group_keys_strings_ints_and_none():
    ids, values, n = api.group_ids_of_keys(["src/b.rs", "src/a.rs", None, "src/b.rs", "Z", None])
    assert values == ["Z", "src/a.rs", "src/b.rs"] and n == 4 and ids.tolist() == [2, 1, 3, 2, 0, 3] and ids.dtype == np.int32
    ids, values, n = api.group_ids_of_keys([30, -5, 30, None, 7])
    assert values == [-5, 7, 30] and n == 4 and ids.tolist() == [2, 0, 2, 3, 1]
    ids, values, n = api.group_ids_of_keys(np.array([4, 4, 9], np.int64))
    assert values == [4, 9] and n == 2 and ids.tolist() == [0, 0, 1]
    ids, values, n = api.group_ids_of_keys([None, None, None])      # all NULL: one group
    assert values == [] and n == 1 and ids.tolist() == [0, 0, 0]
    ids, values, n = api.group_ids_of_keys(["x", "y"])              # no NULL: no group for it
    assert n == 2
    ids, values, n = api.group_ids_of_keys([])
    assert n == 0 and ids.size == 0


def test_group_key_errors_need_no_device():
    with pytest.raises(ValueError, match="all ints or all strings"):
        api.group_ids_of_keys([1, "a"])
    with pytest.raises(ValueError, match="int, a string or None"):
        api.group_ids_of_keys([1.5, 2.0])
    with pytest.raises(ValueError, match="int, a string or None"):
        api.group_ids_of_keys([True, False])


def test_default_pool_is_colgreps():
    assert api.default_pool_k(10, 10 ** 6) == 200 and api.default_pool_k(50, 10 ** 6) == 1000
    assert api.default_pool_k(10, 120) == 120 and api.default_pool_k(10, 3) == 10
    assert api.default_pool_k(2000, 10 ** 6) == 16384 and api.default_pool_k(200, 10 ** 6, 2048) == 2048


def test_new_symbols_are_in_the_mirrors_list():
    for s in ("np_hip_index_set_groups", "np_hip_index_group_count", "np_hip_collapse", "np_hip_collapse_device",
              "np_hip_search_batch_grouped", "np_hip_search_hybrid_grouped"):
        assert s in api.EXPORTS
