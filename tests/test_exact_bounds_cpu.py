"""The S6 error bounds of tests/exact_restate.py are valid and sharp before any GPU runs.

Validity: the restated arithmetic of every precision stays inside its derived bound against float64, for every document
of every case of the list the GPU test (test_gpu_exact_bounds.py) uses.  Sharpness: the same restatement with one defect
(exact_restate.MUTANTS) leaves the bound on at least one document of a case built to catch it -- so substituting any
mutant for emulate() in the validity test makes it fail.  The residual unpacking of the restatement is checked against the
committed decompression fixtures first."""
import os

import numpy as np
import pytest

import exact_restate as X

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _distinct():
    """The case list without the kernel-form knobs, which do not change the arithmetic."""
    seen = {}
    for c in X.CASES:
        seen.setdefault((c.geo, c.lq, c.precision, c.s1_split), c)
    return list(seen.values())


@pytest.mark.parametrize("nbits", [2, 4])
def test_unpacking_matches_the_committed_decompress_fixtures(nbits):
    g = np.load(os.path.join(GOLDEN, f"decompress_nbits{nbits}.npz"))
    a = dict(centroids=g["centroids"], bucket_weights=g["weights"], codes=g["codes"], residuals=g["packed"],
             nbits=nbits, doc_lengths=np.array([g["codes"].size]))
    got = X.decompress64(a)
    assert got.shape == g["out"].shape
    # the fixture is an f32 computation of unit rows: a few f32 roundings of values below 1 (a wrong bucket moves a value
    # by a whole bucket step, 1e-2)
    assert np.max(np.abs(got - g["out"].astype(np.float64))) <= 3e-7


def test_bf16_bit_rounding():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e38, 0.0, 1e-20, np.inf, np.nan, 1.0 + 2.0 ** -8 + 2.0 ** -20], np.float32)
    got = X.bf16(x)
    want = np.array([1.0, 1.0, 1.015625, -2.9908e38, 0.0, 0, np.inf, np.nan, 1.0078125], np.float32)
    assert got[0] == 1.0 and got[1] == 1.0 and got[2] == want[2]        # ties go to the even mantissa
    assert got[8] == want[8] and got[4] == 0.0 and np.isinf(got[6]) and np.isnan(got[7])
    assert np.all((got[np.isfinite(got)].view(np.uint32) & 0xFFFF) == 0)
    hi, lo = X.split(x[:3])
    assert np.all(np.abs(x[:3].astype(np.float64) - hi - lo) <= 2.0 ** -16 * np.abs(x[:3]))


def test_case_list_covers_the_axes():
    """Every geometry, weight scale, query length and knob value meets every precision it applies to."""
    for prec in range(4):
        cs = [c for c in X.CASES if c.precision == prec]
        assert {c.geo for c in cs} == set(X.GEOMETRIES), prec
        assert {c.lq for c in cs} == set(X.QUERY_LENGTHS), prec
        assert {c.geo[2] for c in cs} == {0, -6, 2}, prec
    for prec in (1, 2):
        cs = [c for c in X.CASES if c.precision == prec]
        for knob, values in (("s6_lds", (0, 1, 2)), ("s6_tiles", (0, 1)), ("exact_rowmax", (0, 1)), ("s6_xcd", (0, 1))):
            assert {c.knob(knob) for c in cs} == set(values), (prec, knob)
        assert any(c.s1_split for c in cs)
    # the dispatch mirror: all kernel forms and NQT 1 / 2 / 8 are reached, and every query length meets every form that takes it
    reached = {c.form for c in X.CASES}
    assert {f for f, _ in reached} == set(X.FORMS) and {n for _, n in reached} == {1, 2, 8}
    for form in X.FORMS:
        can = {lq for lq in X.QUERY_LENGTHS for prec in range(4) for lds in (0, 1, 2) for tiles in (0, 1) for rm in (0, 1)
               if X.kernel_form(prec, 4, lq, dict(s6_lds=lds, s6_tiles=tiles, exact_rowmax=rm).get)[0] == form}
        assert {c.lq for c in X.CASES if c.form[0] == form} == can, form
    assert {g[:2] for g in X.GEOMETRIES} >= {(d, b) for d in (32, 64, 96, 128) for b in (2, 4)} | {(100, 4), (48, 4), (64, 1)}
    assert any(g[1] == 8 for g in X.GEOMETRIES)
    lens = np.asarray(X.make_corpus(X.GEOMETRIES[0])["doc_lengths"])
    assert set((0, 1, 31, 32, 33, 63, 64, 65, 200)) <= set(lens.tolist())
    assert len({c.name for c in X.CASES}) == len(X.CASES)
    names = {c.name for c in X.CASES}
    assert set(X.CATCHES) == set(X.MUTANTS) and all(n in names for ns in X.CATCHES.values() for n in ns)


@pytest.mark.parametrize("case", _distinct(), ids=lambda c: c.name)
def test_emulation_within_bound(case):
    a = X.make_corpus(case.geo)
    try:
        for qi, q in enumerate(X.case_queries(case)):
            ref = X.reference(a, q)
            emu = X.emulate(a, q, case.precision, case.s1_split)
            b = X.doc_bound(a, q, case.precision, case.s1_split)
            assert ref.shape == emu.shape == b.shape == (len(a["doc_lengths"]),)
            err = np.abs(emu - ref)
            bad = np.nonzero(~(err <= b))[0]
            assert bad.size == 0, f"{case.name} query {qi} ({X.QUERY_KINDS[qi]}): documents {bad[:5]}: " \
                                  f"error {err[bad[:5]]} over bound {b[bad[:5]]}"
    finally:
        X.drop_query_cache(a)


@pytest.mark.parametrize("mutant", sorted(X.MUTANTS))
def test_mutant_leaves_the_bound(mutant):
    by_name = {c.name: c for c in X.CASES}
    worst = 0.0
    for name in X.CATCHES[mutant]:
        case = by_name[name]
        a = X.make_corpus(case.geo)
        hit = 0
        try:
            for q in X.case_queries(case):
                ref = X.reference(a, q)
                b = X.doc_bound(a, q, case.precision, case.s1_split)
                err = np.abs(X.emulate(a, q, case.precision, case.s1_split, mutant=mutant) - ref)
                hit += int(np.sum(err > b))
                worst = max(worst, float(np.max(err / np.maximum(b, 1e-300) * (b > 0))))
        finally:
            X.drop_query_cache(a)
        # every named case must catch it: the list says which case is built for which mutant
        assert hit > 0, f"mutant ({mutant}) {X.MUTANTS[mutant]}: inside the bound on every document of {name} " \
                        f"(largest error / bound {worst:.3f})"
