"""np_hip_rerank_maxsim (rerank_kernel) held, with no tolerance, to the handler's loop: the oracle's scores bit for bit,
the totals tests/rerank_limit_shapes.py states from exact arithmetic, the stable descending order, and the handler's
BadRequest wherever a similarity or a running total is not finite.  tests/test_rerank_limits_cpu.py shows on the CPU that
the oracle and the module's restatement agree and that the cases separate the wrong rules.
"""
import numpy as np
import pytest

import next_plaid_amd as npa
import rerank_limit_shapes as R
from helpers import O

pytestmark = pytest.mark.gpu

CASES = R.all_cases()


@pytest.mark.parametrize("case", [c for c in CASES if not c.refused], ids=lambda c: c.name)
def test_scores_and_order(case):
    order, scores = npa.rerank_maxsim(case.q, case.docs)
    if case.q.shape[0]:
        ref = np.array([O.rerank_maxsim(case.q, d) for d in case.docs], np.float32)
    else:       # rerank.rs:61: without a query row the loop body never runs: 0.0 for every document, input order
        ref = np.zeros(len(case.docs), np.float32)
    bad = np.nonzero(scores.view(np.uint32) != ref.view(np.uint32))[0]
    assert bad.size == 0, f"{case.name}: document {bad[0]} ({case.docs[bad[0]].shape[0]} tokens): {scores[bad[0]]!r}, " \
                          f"handler {ref[bad[0]]!r} ({bad.size} of {ref.size} differ)"
    if case.want is not None:
        want = np.asarray(case.want, np.float32)
        assert np.array_equal(scores.view(np.uint32), want.view(np.uint32)), f"{case.name}: {scores} vs exact {want}"
    assert np.array_equal(order, R.order_of(ref)), f"{case.name}: order {order[:10]} vs {R.order_of(ref)[:10]}"


@pytest.mark.parametrize("case", [c for c in CASES if c.refused], ids=lambda c: c.name)
def test_non_finite_is_refused(case):
    with pytest.raises(ValueError, match="non-finite"):
        npa.rerank_maxsim(case.q, case.docs)


def test_wider_than_1024_is_a_shape_error():
    q = np.zeros((2, 1025), np.float32)
    with pytest.raises(npa.ShapeError):
        npa.rerank_maxsim(q, [np.zeros((3, 1025), np.float32)])
    order, scores = npa.rerank_maxsim(q[:, :1024], [np.zeros((3, 1024), np.float32)])
    assert scores.tolist() == [0.0] and order.tolist() == [0]
