"""The checker of the exhaustive exact search can fail: scan_restate.check_topk accepts the float64 truth and the restated
kernel arithmetic ranked by the entry point's rule, and rejects eight planted defects.  Also builds and runs the stand-alone
check of the scan's host code (argument checks, query grouping, pass planning).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import exact_restate as X
import scan_restate as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOS = [(128, 4, 0), (100, 4, 2), (64, 1, 0), (64, 8, 0)]
LENGTHS = (1, 33, 256)
G0 = (128, 4, 0)


@pytest.mark.parametrize("geo", GEOS, ids=X.geo_name)
@pytest.mark.parametrize("lq", LENGTHS)
def test_truth_and_restated_arithmetic_pass(geo, lq):
    a = X.make_corpus(geo)
    n = len(a["doc_lengths"])
    evens = np.arange(0, n, 2)
    try:
        for qi, q in enumerate(X.make_queries(a, lq, 700 + lq)):
            what = f"{X.geo_name(geo)} lq{lq} q{qi} ({X.QUERY_KINDS[qi]})"
            t = S.truth(a, q)
            for k in (1, 10, n + 5):
                S.check_topk(a, q, *S.rank(a, t, k), k, 0, what=what + " truth")
            for prec in (0, 3):
                e = X.emulate(a, q, prec)
                for k, scope in ((1, None), (10, None), (n + 5, None), (10, evens)):
                    S.check_topk(a, q, *S.rank(a, e, k, scope), k, prec, scope, what=f"{what} emulate({prec}) k{k}")
            if lq == 1 and X.QUERY_KINDS[qi] == "nan":   # every score is 0: the lowest non-empty ids
                ids, sc = S.rank(a, X.emulate(a, q, 0), 10)
                assert np.array_equal(ids, S.in_scope(a)[:10]) and not sc.any()
    finally:
        X.drop_query_cache(a)


@pytest.fixture(scope="module")
def base():
    a = X.make_corpus(G0)
    qs = X.make_queries(a, 33, 733)
    n = len(a["doc_lengths"])
    return a, qs, n


def rejected(a, q, ids, scores, k, precision=0, scope=None):
    with pytest.raises(AssertionError):
        S.check_topk(a, q, ids, scores, k, precision, scope)
    return True


def test_rejects_a_dropped_top_document(base):
    a, qs, n = base
    ids, sc = S.rank(a, X.emulate(a, qs[0], 0), 11)
    S.check_topk(a, qs[0], ids[:10], sc[:10], 10, 0)
    assert rejected(a, qs[0], ids[1:], sc[1:], 10)


def test_rejects_a_document_scored_with_its_neighbours_tokens(base):
    a, qs, n = base
    e = X.emulate(a, qs[0], 0).copy()
    top = S.rank(a, e, 1)[0][0]
    nb = top + 1 if a["doc_lengths"][top + 1] > 0 else top - 1
    e[top] = e[nb]
    assert rejected(a, qs[0], *S.rank(a, e, n + 5), n + 5)


@pytest.mark.parametrize("length", (33, 65))
def test_rejects_a_missing_last_token(length):
    a = X.make_corpus(G0)
    p = X.prepare(a)
    doc = X.N_RANDOM + X.PLANTED.index(length)
    assert p.off[doc + 1] - p.off[doc] == length
    D = X.decompress64(a)
    q = np.repeat(D[p.off[doc + 1] - 1][None, :], 4, 0).astype(np.float32)      # four copies of the document's LAST token
    try:
        e = X.emulate(a, q, 0).copy()
        S.check_topk(a, q, *S.rank(a, e, len(e) + 5), len(e) + 5, 0)
        short = (q.astype(np.float64) @ D[p.off[doc]:p.off[doc + 1] - 1].T).max(1).sum()
        assert short < e[doc] - 1e-3
        e[doc] = short
        assert rejected(a, q, *S.rank(a, e, len(e) + 5), len(e) + 5)
    finally:
        X.drop_query_cache(a)


def test_rejects_identical_documents_in_descending_id_order(base):
    a, qs, n = base
    copies = [3, n - 3, n - 2]
    assert all(np.array_equal(X.decompress64(a)[X.prepare(a).off[c]:X.prepare(a).off[c + 1]],
                              X.decompress64(a)[X.prepare(a).off[3]:X.prepare(a).off[4]]) for c in copies)
    ids, sc = S.rank(a, X.emulate(a, qs[2], 0), n + 5)
    pos = [int(np.nonzero(ids == c)[0][0]) for c in copies]
    assert pos == list(range(pos[0], pos[0] + 3)) and np.unique(sc[pos].view(np.uint32)).size == 1
    S.check_topk(a, qs[2], ids, sc, n + 5, 0)
    ids = ids.copy()
    ids[pos] = copies[::-1]
    assert rejected(a, qs[2], ids, sc, n + 5)


def test_rejects_an_empty_document(base):
    a, qs, n = base
    empty = int(np.nonzero(np.asarray(a["doc_lengths"]) == 0)[0][0])
    ids, sc = S.rank(a, X.emulate(a, qs[0], 0), 10)
    ids, sc = ids.copy(), sc.copy()
    ids[-1], sc[-1] = empty, 0.0
    assert rejected(a, qs[0], ids, sc, 10)


def test_rejects_a_document_outside_the_subset(base):
    a, qs, n = base
    evens = np.arange(0, n, 2)
    e = X.emulate(a, qs[0], 0)
    ids, sc = S.rank(a, e, 10, evens)
    S.check_topk(a, qs[0], ids, sc, 10, 0, evens)
    odd = next(d for d in S.rank(a, e, n)[0] if d % 2 == 1)
    ids, sc = ids.copy(), sc.copy()
    ids[-1], sc[-1] = odd, e[odd]
    order = np.lexsort((ids, -S.order_key(sc)))
    assert rejected(a, qs[0], ids[order], sc[order], 10, scope=evens)


def test_rejects_a_count_one_short(base):
    a, qs, n = base
    ids, sc = S.rank(a, X.emulate(a, qs[0], 0), 10)
    assert rejected(a, qs[0], ids[:-1], sc[:-1], 10)
    ids, sc = S.rank(a, X.emulate(a, qs[0], 0), n + 5)
    assert rejected(a, qs[0], ids[:-1], sc[:-1], n + 5)


def test_rejects_the_scores_of_the_next_query(base):
    a, qs, n = base
    for i in (0, 2, 6):
        assert rejected(a, qs[i], *S.rank(a, X.emulate(a, qs[i + 1], 0), 10), 10)


def test_host_code_of_the_scan_stands_alone(tmp_path):
    """tests/cpp/scan_plan_check.cpp: np_scan_plan.h with the host compiler alone (no device, no library)."""
    exe = tmp_path / "scan_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "next-plaid_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "scan_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
