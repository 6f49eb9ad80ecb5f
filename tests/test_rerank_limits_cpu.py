"""The rerank cases of tests/rerank_limit_shapes.py on the CPU: the oracle's handler loop and the module's float32
restatement agree bit for bit, both give the totals the constructed cases state from exact arithmetic, both refuse what
the handler refuses, and each wrong rule changes an answer.  tests/test_gpu_rerank_limits.py holds rerank_kernel to the same.
"""
import numpy as np
import pytest

import rerank_limit_shapes as R
from helpers import O

CASES = R.all_cases()


def _oracle(q, d):
    if q.shape[0] == 0:          # no query row: the loop body never runs (rerank.rs:61)
        return np.float32(0.0)
    try:
        return np.float32(O.rerank_maxsim(q, d))
    except ValueError:
        return None


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_and_restatement_agree(case):
    got = [R.restate(case.q, d) for d in case.docs]
    ref = [_oracle(case.q, d) for d in case.docs]
    for i, (a, b) in enumerate(zip(got, ref)):
        assert (a is None) == (b is None), f"{case.name} document {i}: restatement {a}, oracle {b}"
        if a is not None:
            assert np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32), f"{case.name} document {i}: {a!r} vs {b!r}"
    assert case.refused == any(a is None for a in got)
    if case.want is not None:
        w = np.asarray(case.want, np.float32)
        assert np.array_equal(np.asarray(got, np.float32).view(np.uint32), w.view(np.uint32)), f"{case.name}: {got} vs {w}"


def test_cases_cover_the_kernel_paths():
    rnd = [c for c in CASES if c.name.startswith("random")]
    assert {c.q.shape[1] for c in rnd} == set(R.DIMS) and {c.q.shape[0] for c in rnd} >= set(R.QUERY_LENGTHS)
    assert {d.shape[0] for c in rnd for d in c.docs} >= set(R.DOC_LENGTHS)
    assert any(len(c.docs) >= 1000 for c in rnd)
    by = {c.name: c for c in CASES}
    assert {p for n, c in by.items() if n.startswith("planted") for p in c.notes["places"]} >= {0, 255, 256, 299, 512}
    for n, c in by.items():
        if n.startswith("all-negative"):
            assert c.q.shape[0] == 5 and {d.shape[0] for d in c.docs} >= {1, 300} and np.all(c.want < 0)
            for d in c.docs:
                assert np.all(R.sims(c.q, d) < 0)
    eq = by["equal-scores"]
    assert R.order_of(eq.want).tolist().index(1) < R.order_of(eq.want).tolist().index(3) < R.order_of(eq.want).tolist().index(5)
    kinds = {n.rsplit("-", 1)[0] for n, c in by.items() if c.refused}
    assert kinds >= {"plus-inf-similarity", "minus-inf-similarity", "nan-in-document"}
    assert by["total-overflows"].refused and not by["total-of-one-row"].refused
    s = R.sims(by["total-overflows"].q, by["total-overflows"].docs[1])
    assert np.isfinite(s).all()                        # every maximum is finite; only the total overflows
    s = R.sims(by["minus-inf-similarity-last"].q, by["minus-inf-similarity-last"].docs[-1])
    assert np.isneginf(s).any() and np.isfinite(s.max(1)).all()      # the -inf is no row's maximum
    s = R.sims(by["plus-inf-similarity-last"].q, by["plus-inf-similarity-last"].docs[-1])
    assert np.isposinf(s[0]).any() and np.isfinite(s[1]).all()


def test_every_wrong_rule_changes_an_answer():
    by = {c.name: c for c in CASES}
    for n in ("all-negative-d4", "all-negative-d128"):      # idle lanes or padded rows contributing 0
        c = by[n]
        for d, w in zip(c.docs, c.want):
            z = R.restate(c.q, d, "zero")
            assert z == 0.0 and z != w and w < 0, (n, z, w)
    c = by["mul-then-add"]
    fused = [R.restate(c.q, d, "fused") for d in c.docs]
    assert fused[0] == np.float32(2.0 ** -24) and fused[1] == np.float32(2.0 ** -24) and c.want[0] == 0.0
    assert fused[2] == c.want[2]
    changed = sum(R.restate(cc.q, d, "fused") != R.restate(cc.q, d) for cc in CASES if cc.name.startswith("random")
                  for d in cc.docs[:4] if cc.q.shape[1] <= 129)
    assert changed > 0                                      # ... and random data separates the two as well
