"""Every S6 kernel form at every precision against float64, inside a bound derived from the arithmetic.

tests/exact_restate.py holds the float64 reference, the restated arithmetic and the derivation of the bound; its case list
is shared with tests/test_exact_bounds_cpu.py, which shows on the CPU that the bound holds for the restated arithmetic and
that eleven planted defects leave it.  Here every case probes every cell without a threshold and exact-scores every
document, through search_batch with 8 queries (the one-XCD-per-query grid) and with one query (debug_trace or search):

  A (accuracy)         |gpu - reference| <= bound, for every returned document, and every non-empty document is returned
  B (same arithmetic)  |gpu - emulate(acc="f64")| <= the accumulation part of the bound: the restatement rounds the same
                       operands, so only the order of the f32 sums may differ; this is what notices a decompression or
                       normalisation slip that the 2^-8 of the bf16 precisions would hide in A

The largest error / bound per (precision, kernel form) is collected; NP_S6_ERROR_TABLE=<file> writes the table that
profiles/s6_error_bounds.md records.
"""
import os

import numpy as np
import pytest

import exact_restate as X
from helpers import hip_index

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu

RATIOS = {}     # (precision, form, NQT, S1 form) -> [largest A ratio, largest B ratio, documents compared]
RAN = set()


@pytest.fixture(scope="module")
def indexes():
    """One index per (geometry, weight scale), opened on first use."""
    opened = {}

    def get(geo):
        if geo not in opened:
            opened[geo] = hip_index(X.make_corpus(geo), max_batch=16, max_query_tokens=256)
        return opened[geo]
    yield get
    for h in opened.values():
        h.close()
    _write_table()


def _write_table():
    lines = ["| precision | kernel form | NQT | S1 | documents | max error / bound (A) | max difference / accumulation part (B) |",
             "|---|---|---|---|---|---|---|"]
    for (prec, form, nqt, s1), (ra, rb, n) in sorted(RATIOS.items()):
        lines.append(f"| {prec} | `{form}` | {nqt} | {s1} | {n} | {ra:.4f} | {rb:.4f} |")
    text = "\n".join(lines) + "\n"
    print("\n" + text)
    out = os.environ.get("NP_S6_ERROR_TABLE")
    if out:
        with open(out, "w") as f:
            f.write(text)


def _check(case, what, a, q, ids, scores, s1_split):
    """Assertions A and B for one query's returned (document id, score) pairs."""
    ids = np.asarray(ids, np.int64)
    got = np.asarray(scores, np.float64)
    ref = X.reference(a, q)
    emu = X.emulate(a, q, case.precision, s1_split, acc="f64")
    b = X.doc_bound(a, q, case.precision, s1_split)
    bacc = X.doc_bound(a, q, case.precision, s1_split, part="acc")
    assert np.unique(ids).size == ids.size, f"{what}: a document is returned twice"
    lens = np.asarray(a["doc_lengths"])
    if np.all(np.isfinite(q), axis=1).any():    # some token probes: every non-empty document is a candidate
        assert np.array_equal(np.sort(ids), np.nonzero(lens > 0)[0]), f"{what}: not every non-empty document is returned"
    ea, eb = np.abs(got - ref[ids]), np.abs(got - emu[ids])
    ra = float(np.max(ea / np.maximum(b[ids], 1e-300) * (b[ids] > 0), initial=0.0))
    rb = float(np.max(eb / np.maximum(bacc[ids], 1e-300) * (bacc[ids] > 0), initial=0.0))
    print(f"{what}: {ids.size} documents, error / bound {ra:.4f}, difference / accumulation part {rb:.4f}")
    key = (case.precision,) + case.form + ("split bf16" if s1_split else "f32",)
    r = RATIOS.setdefault(key, [0.0, 0.0, 0])
    r[0], r[1], r[2] = max(r[0], ra), max(r[1], rb), r[2] + ids.size
    bad = np.nonzero(~(ea <= b[ids]))[0]
    assert bad.size == 0, f"{what}: A: documents {ids[bad[:5]]}: |gpu - reference| {ea[bad[:5]]} over {b[ids][bad[:5]]} " \
                          f"(gpu {got[bad[:5]]}, reference {ref[ids][bad[:5]]}, lengths {lens[ids][bad[:5]]})"
    bad = np.nonzero(~(eb <= bacc[ids]))[0]
    assert bad.size == 0, f"{what}: B: documents {ids[bad[:5]]}: |gpu - emulate| {eb[bad[:5]]} over {bacc[ids][bad[:5]]} " \
                          f"(gpu {got[bad[:5]]}, emulate {emu[ids][bad[:5]]}, lengths {lens[ids][bad[:5]]})"


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_scores_within_bound(indexes, case):
    a = X.make_corpus(case.geo)
    hx = indexes(case.geo)
    n = len(a["doc_lengths"])
    assert n <= 16384
    qs = X.case_queries(case)
    assert len(qs) >= 8 and all(q.shape == (case.lq, case.geo[0]) for q in qs)
    p = npa.SearchParameters(n_full_scores=n, top_k=n, n_ivf_probe=X.K, centroid_score_threshold=None,
                             precision=case.precision, centroid_batch_size=X.K // 2 if case.s1_split else 100_000)
    knobs = dict(X.DEFAULT_KNOBS, **dict(case.knobs), s1_split=int(case.s1_split))
    try:
        for k, v in knobs.items():
            hx.tune(k, v)
        res = hx.search_batch(qs, p)
        for qi, (q, r) in enumerate(zip(qs, res)):
            _check(case, f"{case.name} batch q{qi} ({X.QUERY_KINDS[qi]})", a, q, r.passage_ids, r.scores, case.s1_split)
        for qi, q in enumerate(qs):
            what = f"{case.name} single q{qi} ({X.QUERY_KINDS[qi]})"
            if case.s1_split or qi % 2:      # the stage trace switches the split S1 off: search() keeps it
                r = hx.search(q, p)
                _check(case, what, a, q, r.passage_ids, r.scores, case.s1_split)
            else:
                t = hx.debug_trace(q, p)
                _check(case, what + " trace", a, q, t["sel"], t["sel_exact"], False)
    finally:
        for k, v in dict(X.DEFAULT_KNOBS, s1_split=0).items():
            hx.tune(k, v)
        X.drop_query_cache(a)
    RAN.add(case)


def test_every_kernel_form_was_reached():
    """From launch_exact's rules (exact_restate.kernel_form mirrors them): the cases that ran reached all kernel
    templates -- exact_f32, exact_bf16, exact_qc, exact_qct with one and with two query tiles, exact_qcl at 3 and at 4
    waves per SIMD -- and NQT 1, 2 and 8; precisions 1 and 2 met each QC-reuse form."""
    assert RAN == set(X.CASES), f"{len(set(X.CASES) - RAN)} cases did not run to the end"
    reached = {c.form for c in RAN}
    assert {f for f, _ in reached} == set(X.FORMS), sorted(reached)
    assert {nq for _, nq in reached} == {1, 2, 8}
    for prec in (1, 2):
        assert {c.form[0] for c in RAN if c.precision == prec and c.geo[1] != 8} == set(X.FORMS[2:]), prec
    assert {c.form[0] for c in RAN if c.geo[1] == 8} == {X.FORMS[0]}      # 8 bits: the f32 kernel at every precision
    assert any(c.s1_split for c in RAN)
