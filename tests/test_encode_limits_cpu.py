"""The encode cases of tests/encode_limit_shapes.py on the CPU: the oracle gives the answers the cases state by
construction, the cases hold what they were built to hold, and every wrong rule changes an answer somewhere.

tests/test_gpu_encode_limits.py holds np_hip_encode_tokens to the same answers; nobody runs a deliberately wrong kernel
on a GPU, so that the cases would notice one is shown here, on the restatement's own wrong-rule variants.
"""
import re

import numpy as np
import pytest

import encode_limit_shapes as E
from helpers import O

CASES = E.all_cases()
ARGMAX = [c for c in CASES if not c.table]
PACK = [c for c in CASES if c.table]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_gives_the_answers_by_construction(case):
    cen, cut, nbits, x, want_codes, want_packed = case
    codes, packed = O.encode_tokens(x, cen, nbits, cut)
    bad = np.nonzero(codes != want_codes)[0]
    assert bad.size == 0, f"{case.name}: token {bad[0]}: oracle {codes[bad[0]]}, by construction {want_codes[bad[0]]}"
    bad = np.argwhere(packed != want_packed)
    assert bad.size == 0, f"{case.name}: token {bad[0][0]} byte {bad[0][1]}: oracle {packed[tuple(bad[0])]:#04x}, " \
                          f"by construction {want_packed[tuple(bad[0])]:#04x}"
    rc, rp = E.restate(cen, cut, nbits, x)
    assert np.array_equal(rc, want_codes) and np.array_equal(rp, want_packed)
    assert want_packed.shape == (x.shape[0], cen.shape[1] * nbits // 8)


def _planted(pattern):
    """(K, planted index tuple) of every note whose text matches."""
    out = []
    for c in ARGMAX:
        for t, text, planted in c.notes:
            m = re.search(pattern, text)
            if m:
                out.append((c.centroids.shape[0], tuple(int(v) for v in re.findall(r"\d+", m.group(0))), c, t))
    return out


def test_argmax_cases_hold_what_they_plant():
    assert {c.centroids.shape[0] for c in ARGMAX} == set(E.K_VALUES)
    dims = {c.centroids.shape[1] for c in ARGMAX}
    assert {8, 96, 128} <= dims and dims & {100, 104}
    dups = _planted(r"duplicates \([\d, ]+\)")
    groups = {d for _, d, _, _ in dups}
    assert any(len(d) == 2 and d[1] == d[0] + 1 and d[0] // 32 == d[1] // 32 for d in groups)        # (i, i + 1) in one group
    assert any(len(d) == 2 and d[0] % 32 == 0 and d[1] == d[0] + 31 for d in groups)                 # (i, i + 31) in one group
    assert (31, 32) in groups                                                                        # across a group border
    assert any(len(d) == 2 and d[1] == d[0] + 2048 for d in groups)                                  # same lane, next loop turn
    assert any(len(d) == 2 and d[1] == d[0] + 2048 and d[0] >= 32 for d in groups)                   # ... not in group 0
    assert any(len(d) == 3 and d[0] // 32 == d[2] // 32 for d in groups)                             # a triple in one group
    assert any(len(d) == 3 and len({i // 32 for i in d}) == 3 for d in groups)                       # ... and across three
    for K in E.K_VALUES:
        if K >= 2:
            assert any(k == K and d == (0, K - 1) for k, d, _, _ in dups), K
        assert any(c.centroids.shape[0] == K and "-same-" in c.name for c in ARGMAX)
    alone = _planted(r"winner alone at \d+")
    for K in E.K_VALUES:                         # index 0, K - 1 and the first row of the last (for most K partial) group
        got = {d[0] for k, d, _, _ in alone if k == K}
        assert {0, K - 1, 32 * ((K - 1) // 32)} <= got, (K, got)
    near = _planted(r"near tie: \d+ beats \d+")
    assert any(d[0] < d[1] for _, d, _, _ in near) and any(d[0] > d[1] for _, d, _, _ in near)
    assert any(abs(d[0] - d[1]) == 2048 for _, d, _, _ in near)
    for _, (win, lose), c, t in near:            # one step of the grid of score differences
        s = E.scores_f32(c.centroids, c.tokens[t:t + 1])[0].astype(np.float64)
        assert s[win] - s[lose] == 2.0 ** -12 and np.sort(s)[-1] == s[win] and (s == s[win]).sum() == 1
        assert c.want_codes[t] == win
    neg = [c for c in ARGMAX if "-neg-" in c.name]
    assert any(c.centroids.shape[0] < 32 for c in neg) and any(c.centroids.shape[0] % 32 for c in neg)
    for c in neg:
        assert np.all(E.scores_f32(c.centroids, c.tokens) < 0)
        if c.centroids.shape[0] < 32:
            assert any("minus the sum" in text for _, text, _ in c.notes), c.name
    for c in ARGMAX:
        K = c.centroids.shape[0]
        for t, text, _ in c.notes:
            if "every score +0" in text or "NaN component" in text:
                assert c.want_codes[t] == K - 1
    mixed = [c for c in ARGMAX if "-mixed" in c.name]
    for c in mixed:
        s = E.scores_f32(c.centroids, c.tokens)
        assert np.isposinf(s[0]).any() and np.isfinite(s[0]).any() and np.isfinite(s[0, c.want_codes[0]])
        if "-mixed0-" in c.name:
            assert c.want_codes[0] == 0 and np.isposinf(s[0, 1:]).all()
        else:
            assert (np.isneginf(s[0]).any() or s.shape[1] < 31) and not np.isfinite(s[0, -1])


@pytest.mark.parametrize("case", PACK, ids=lambda c: c.name)
def test_pack_cases_cover_the_cutoffs(case):
    E.check_pack_coverage(case)
    share, seen, seen_pos, res = E.pack_coverage(case)
    per = 8 // case.nbits
    if np.isfinite(case.cutoffs).any():
        assert share >= 0.25
    if case.table in ("ascending", "descending"):
        assert seen == set(range(1 << case.nbits))
        assert seen_pos == {(b, p) for b in range(1 << case.nbits) for p in range(per)}
    s = np.sort(E.scores_f32(case.centroids, case.tokens[:-6]).astype(np.float64), 1)
    if s.shape[1] > 1:
        assert np.all(s[:, -1] - s[:, -2] >= 2.0 ** -4)
    assert np.all(case.want_codes[-6:] == case.centroids.shape[0] - 1)


def test_pack_cases_cover_every_width_and_table():
    assert {c.nbits for c in PACK} == {1, 2, 4, 8}
    for nbits in (1, 2, 4, 8):
        assert {c.table for c in PACK if c.nbits == nbits} == set(E.TABLES), nbits
    assert {c.centroids.shape[1] for c in PACK} >= {8, 96, 100, 128}
    assert any(np.signbit(c.cutoffs[c.cutoffs == 0]).any() for c in PACK)       # a cutoff of -0.0


@pytest.mark.parametrize("rule", sorted(E.WRONG_RULES))
def test_every_wrong_rule_changes_an_answer(rule):
    changed = []
    for c in CASES:
        cen, cut, nbits, x, want_codes, want_packed = c
        codes, packed = E.restate(cen, cut, nbits, x, rule)
        if rule in ("ge", "msb"):
            assert np.array_equal(codes, want_codes)
            if not np.array_equal(packed, want_packed):
                changed.append(c.name)
        elif not np.array_equal(codes, want_codes):
            changed.append(c.name)
    assert changed, f"no case notices: {E.WRONG_RULES[rule]}"
    print(f"{rule}: {len(changed)} of {len(CASES)} cases change")
    if rule == "ge":          # every table with a finite cutoff separates > from >=
        assert {c.name for c in PACK if np.isfinite(c.cutoffs).any()} <= set(changed)
    if rule == "first":       # ... and the later duplicate loses in every table that plants one
        assert {c.name for c in ARGMAX if "-same-" in c.name and c.centroids.shape[0] > 1} <= set(changed)
    if rule == "pad":         # the padded rows win wherever every score is negative and K is no multiple of 64
        assert {c.name for c in ARGMAX if "-neg-" in c.name and c.centroids.shape[0] % 64} <= set(changed)
    if rule == "byvalue":
        assert {c.name for c in ARGMAX if "-mixed" in c.name} <= set(changed)
