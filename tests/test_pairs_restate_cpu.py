"""The checker of np_hip_score_pairs can fail: pairs_restate.check_pairs accepts the kernel's arithmetic restated in f32
numpy (lowest-index argmax, ordered f32 sum) and rejects eight planted defects.  Also builds and runs the stand-alone check
of the entry point's host code (offsets, slices, chunks, argument errors), plainly and under ASan / UBSan.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import exact_restate as X
import pairs_restate as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOS = [(128, 4, 0), (64, 2, 0), (100, 4, 0), (128, 8, 0), (64, 1, 0), (128, 4, 2)]
LENGTHS = (1, 33, 65)
G0 = (128, 4, 0)
F32 = np.float32


def candidate(a, q, doc_ids, defect=None):
    """(scores, sims, pos) as the kernel forms them, from P.sims32; `defect`: one of DEFECTS."""
    p = X.prepare(a)
    S = P.sims32(a, q)
    if defect == "un-normalised rows":
        S = X._mm(np.ascontiguousarray(q, F32), (p.C[p.codes] + p.w[p.bkt]).astype(F32), "f32").astype(F32)
    lq = S.shape[0]
    scores, sims, pos = [], [], []
    for d in np.asarray(doc_ids).tolist():
        o0, o1 = int(p.off[d]), int(p.off[d + 1])
        V = np.where(np.isfinite(S[:, o0:o1]), S[:, o0:o1], -np.inf).astype(F32)
        if defect == "only the rows of half 0" and o1 > o0:
            V = np.where(((np.arange(o1 - o0) & 4) == 0)[None, :], V, -np.inf).astype(F32)
        if o1 > o0:
            m = V.max(1)
            at = V.argmax(1)
            if defect == "highest index among equal sims":
                at = (o1 - o0 - 1) - V[:, ::-1].argmax(1)
            at = np.where(m > -np.inf, at, -1)
        else:
            m, at = np.full(lq, -np.inf, F32), np.full(lq, -1)
        if defect == "position off by one" and o1 - o0 > 1:
            at = np.where(at >= 0, (at + 1) % (o1 - o0), at)
        if defect == "position modulo 32":
            at = np.where(at >= 0, at % 32, at)
        if defect == "NaN query token at position 0":
            at = np.where(at < 0, 0, at) if o1 > o0 else at
        sc = P.ordered_sum(m)
        if defect == "score summed in float64":
            sc = F32(np.where(m > -np.inf, m, 0).astype(np.float64).sum())
        if defect == "row in reversed token order":
            m, at = m[::-1], at[::-1]
        scores.append(sc)
        sims.append(m)
        pos.append(at)
    return np.asarray(scores, F32), np.asarray(sims, F32).reshape(-1, lq), np.asarray(pos, np.int32).reshape(-1, lq)


DEFECTS = ("position off by one", "highest index among equal sims", "position modulo 32", "only the rows of half 0",
           "un-normalised rows", "row in reversed token order", "NaN query token at position 0", "score summed in float64")


@pytest.mark.parametrize("geo", GEOS, ids=X.geo_name)
def test_restated_arithmetic_passes(geo):
    a = X.make_corpus(geo)
    docs = np.arange(len(a["doc_lengths"]))
    tally = P.Tally()
    try:
        for lq in LENGTHS:
            for qi, q in enumerate(X.make_queries(a, lq, 700 + lq)):
                P.check_pairs(a, q, docs, *candidate(a, q, docs), what=f"{X.geo_name(geo)} lq{lq} q{qi} ({X.QUERY_KINDS[qi]})",
                              tally=tally)
    finally:
        X.drop_query_cache(a)
    assert tally.checked > 60000
    tally.assert_cap(X.geo_name(geo))


def test_duplicates_order_and_single_calls():
    """Pairs are independent: a permuted list with duplicates, and calls of one pair each (every one held to the cap alone)."""
    a = X.make_corpus(G0)
    n = len(a["doc_lengths"])
    q = X.make_queries(a, 33, 733)[0]
    docs = np.array([n - 1, 3, 3, 0, n - 1, 80, 5, n - 2, 93], np.int64)
    try:
        out = candidate(a, q, docs)
        P.check_pairs(a, q, docs, *out, tally=P.Tally())
        for j in (0, 1, 3):
            P.check_pairs(a, q, docs[j:j + 1], out[0][j:j + 1], out[1][j:j + 1], out[2][j:j + 1])
        assert P.repeated_token_doc(a) == n - 1 == X.repeated_doc(a)
    finally:
        X.drop_query_cache(a)


@pytest.mark.parametrize("defect", DEFECTS)
def test_rejects(defect):
    a = X.make_corpus(G0)
    docs = np.arange(len(a["doc_lengths"]))
    qs = X.make_queries(a, 33, 733)
    try:
        caught = 0
        for qi, q in enumerate(qs):
            P.check_pairs(a, q, docs, *candidate(a, q, docs), tally=P.Tally())
            try:
                P.check_pairs(a, q, docs, *candidate(a, q, docs, defect), tally=P.Tally())
            except AssertionError:
                caught += 1
        kinds = [k for k in X.QUERY_KINDS]
        if defect == "NaN query token at position 0":
            assert caught == kinds.count("nan"), "only the query with a NaN token shows it"
        else:
            assert caught >= 6, f"{defect}: rejected for {caught} of {len(qs)} queries"
    finally:
        X.drop_query_cache(a)


def test_rejects_too_many_ambiguous_entries():
    """The cap itself: a document of near-identical tokens makes every position ambiguous, and the checker says so."""
    t = P.Tally()
    t.add(1000, 5)
    t.assert_cap()
    t.add(0, 1)
    with pytest.raises(AssertionError):
        t.assert_cap()


def test_host_code_of_score_pairs_stands_alone(tmp_path):
    """tests/cpp/pairs_plan_check.cpp: np_pairs_plan.h with the host compiler alone (no device, no library), then the same
    program built with -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "pairs_plan_check.cpp")
    inc = os.path.join(ROOT, "next-plaid_amd", "csrc")
    for name, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / f"pairs_plan_check_{name}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, src, "-o", str(exe)])
        out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "all checks passed" in out.stdout, name + ": " + out.stdout + out.stderr
