"""/rerank MaxSim (next-plaid-api handlers/rerank.rs:57-94, 162-165) at rerank_kernel's own edges (test
infrastructure; numpy only: imports neither the package nor the oracle).

    restate(q, d)          the handler's loop in float32: sim = sequential sum of q*d products (multiply, THEN add), max
                           over the document's tokens, sum over the query's tokens; None where the handler answers
                           BadRequest (a non-finite similarity anywhere, or a non-finite running total)
    restate(..., rule)     the wrong rules of WRONG_RULES
    random_cases()         every dim, query length and document length at which the kernel takes another path
    constructed_cases()    grid values: exact similarities, totals stated from exact arithmetic
    nonfinite_cases()      calls the handler refuses, and their finite neighbours

The kernel: one block of 256 threads per document, thread i takes tokens i, i + 256, ...; query rows go through LDS eight
at a time, the last group zero-padded; an idle thread's maximum stays -inf.  Hence the lengths around 256 and 512, the
query lengths around 8 and 16, and documents whose every similarity is negative, where a 0 from an idle thread or from
a padded row would show.
"""
from dataclasses import dataclass, field

import numpy as np

F32, F64 = np.float32, np.float64
DIMS = (1, 4, 100, 128, 129, 1000, 1024)
QUERY_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 33)
DOC_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513)
WRONG_RULES = {
    "fused": "sim accumulated by fused multiply-add",
    "zero": "a running maximum starts at 0 (an idle lane or a padded query row contributes 0)",
}


@dataclass
class Case:
    name: str
    q: np.ndarray
    docs: list
    want: object = None            # expected scores from exact arithmetic (constructed cases), else None
    refused: bool = False          # the handler answers BadRequest
    notes: dict = field(default_factory=dict)


def sims(q, d, rule=None):
    """[lq, n] float32: k-ordered, one rounding per product and one per addition."""
    q, d = np.asarray(q, F32), np.asarray(d, F32)
    S = np.zeros((q.shape[0], d.shape[0]), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(q.shape[1]):
            if rule == "fused":     # the product of two f32 values is exact in float64; the sum is rounded to 53 bits, then 24
                S = (q[:, k, None].astype(F64) * d[None, :, k].astype(F64) + S.astype(F64)).astype(F32)
            else:
                S = S + q[:, k, None] * d[None, :, k]
    return S


def restate(q, d, rule=None):
    """The handler's score of one document as float32, or None for its BadRequest."""
    S = sims(q, d, rule)
    if not np.isfinite(S).all():
        return None
    total = F32(0.0)
    for r in range(S.shape[0]):
        m = F32(0.0) if rule == "zero" else F32(-np.inf)
        if S.shape[1]:
            m = max(m, S[r].max())
        if m > -np.inf:
            with np.errstate(over="ignore"):
                total = F32(total + m)
            if not np.isfinite(total):
                return None
    return total


def order_of(scores):
    """Stable descending order (results.sort_by(score_desc_cmp))."""
    return np.argsort(-np.asarray(scores, F64), kind="stable")


# ---- random data -------------------------------------------------------------------------------------------------------
def random_cases():
    out = []
    g = np.random.default_rng(9300)
    for i, lq in enumerate(QUERY_LENGTHS):
        dim = DIMS[i % len(DIMS)]
        q = g.standard_normal((lq, dim)).astype(F32)
        lens = list(DOC_LENGTHS) if dim <= 129 else [DOC_LENGTHS[(i + j) % len(DOC_LENGTHS)] for j in range(0, 11, 2)] + [257]
        docs = [g.standard_normal((n, dim)).astype(F32) for n in lens]
        docs.insert(3, docs[5].copy())                  # equal scores keep their input order
        out.append(Case(f"random-lq{lq}-d{dim}", q, docs))
    for dim, lq in ((1024, 33), (1000, 9), (129, 17), (1, 8)):       # the widest rows against the longest documents
        q = g.standard_normal((lq, dim)).astype(F32)
        docs = [g.standard_normal((n, dim)).astype(F32) for n in (513, 0, 256, 1)]
        out.append(Case(f"random-lq{lq}-d{dim}-long", q, docs))
    q = g.standard_normal((7, 100)).astype(F32)
    docs = [g.standard_normal((int(n), 100)).astype(F32) for n in g.integers(0, 4, 1000)]
    out.append(Case("random-1000-short-documents", q, docs))
    return out


# ---- by construction ---------------------------------------------------------------------------------------------------
def _exact_scores(q, docs):
    """Totals in float64 = exact arithmetic on the grid; asserts every similarity and total is exact in float32."""
    out = []
    for d in docs:
        S = q.astype(F64) @ d.astype(F64).T
        assert np.array_equal(S.astype(F32).astype(F64), S)
        t = S.max(1).sum() if d.shape[0] else 0.0
        assert F64(F32(t)) == t
        out.append(t)
    return np.asarray(out, F32)


def constructed_cases():
    out = []
    g = np.random.default_rng(9400)
    # the maximising token of query row 0 at position 0, 255, 256 and last: entries of q in {+-1, +-0.5}, of the
    # documents in {+-0.25, +-0.125}, the planted token 4 sign(q_0): q_0 . planted >= 2 dim, every other sim <= dim / 4
    for dim, lq in ((4, 3), (100, 9)):
        q = (g.choice([1.0, -1.0, 0.5, -0.5], (lq, dim))).astype(F32)
        docs, places = [], []
        for n, pos in ((300, 0), (300, 255), (300, 256), (300, 299), (513, 512), (257, 256), (1, 0)):
            d = g.choice([0.25, -0.25, 0.125, -0.125], (n, dim)).astype(F32)
            d[pos] = 4 * np.sign(q[0])
            S = q.astype(F64) @ d.astype(F64).T
            assert np.argmax(S[0]) == pos and (S[0] == S[0].max()).sum() == 1
            docs.append(d)
            places.append(pos)
        out.append(Case(f"planted-maximum-d{dim}", q, docs, _exact_scores(q, docs), notes=dict(places=places)))
    # every similarity negative, lq = 5 (three zero rows pad the group of eight), documents of 1 and 300 tokens
    for dim in (4, 128):
        q = g.choice([0.5, 1.0], (5, dim)).astype(F32)
        docs = [-g.choice([0.25, 0.125, 0.5], (n, dim)).astype(F32) for n in (1, 300, 1, 255, 257)]
        want = _exact_scores(q, docs)
        assert np.all(want < 0)
        out.append(Case(f"all-negative-d{dim}", q, docs, want))
    # multiply-then-add against a fused chain: q0 d0 = -(1 + 2^-11) exactly; q1 d1 = (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24
    # rounds to 1 + 2^-11 (a tie, to even), so the handler's sum is 0 where a fused chain keeps 2^-24
    e = F32(1 + 2.0 ** -12)
    q = np.array([[1.0, e], [0.0, 0.0]], F32)
    d = np.array([[-(1 + 2.0 ** -11), e], [-2.0, 0.0]], F32)
    out.append(Case("mul-then-add", q, [d, d[:1], d[1:]], np.array([0.0, 0.0, -2.0], F32)))
    # three documents with equal scores interleaved with others: the stable order keeps 1, 3, 5 in input order
    q = g.choice([1.0, -1.0, 0.5, -0.5], (4, 8)).astype(F32)
    same = g.choice([0.25, -0.25, 0.5], (70, 8)).astype(F32)
    docs = [g.choice([0.25, -0.25, 0.5], (n, 8)).astype(F32) for n in (3, 70, 9, 70, 300, 70, 2)]
    for i in (1, 3, 5):
        docs[i] = same.copy()
    docs[3] = same[::-1].copy()                         # the same tokens in another order: the same maxima
    want = _exact_scores(q, docs)
    assert want[1] == want[3] == want[5] and (want == want[1]).sum() == 3
    out.append(Case("equal-scores", q, docs, want))
    return out


# ---- non-finite --------------------------------------------------------------------------------------------------------
def nonfinite_cases():
    """(case, finite neighbour or None).  dim 2, huge = 3e38: huge * 2 overflows, huge * 1 does not."""
    huge = F32(3e38)
    fine = [np.array([[1.0, 0.0], [0.5, 1.0]], F32), np.array([[0.25, 1.0]], F32), np.zeros((0, 2), F32)]
    q2 = np.array([[huge, 0.0], [0.0, 1.0]], F32)
    over = np.array([[0.5, 7.0], [2.0, 0.0], [0.25, 1.0]], F32)        # row 0 of q: +inf at token 1; row 1's maximum at token 0
    under = np.array([[0.5, 7.0], [-2.0, 0.0], [0.25, 1.0]], F32)      # -inf at token 1: never a maximum
    nan = np.array([[0.5, 7.0], [0.25, np.nan]], F32)
    out = []
    for name, q, bad in (("plus-inf-similarity", q2, over), ("minus-inf-similarity", q2, under), ("nan-in-document", q2, nan)):
        for where in ("first", "middle", "last"):
            docs = {"first": [bad] + fine, "middle": fine[:2] + [bad] + fine[2:], "last": fine + [bad]}[where]
            out.append(Case(f"{name}-{where}", q, docs, refused=True))
        long = np.concatenate([np.tile(fine[0], (150, 1)), bad])        # the offending token past position 256
        out.append(Case(f"{name}-at-token-301", q, [fine[0], long], refused=True))
    # a total that overflows although every maximum is finite; the same document with one query token passes
    d = np.array([[1.0, 0.0], [0.5, 0.0]], F32)
    out.append(Case("total-overflows", np.array([[huge, 0.0], [huge, 0.0]], F32), fine[:1] + [d], refused=True))
    out.append(Case("total-of-one-row", np.array([[huge, 0.0]], F32), fine[:1] + [d], np.array([huge, huge], F32)))
    out.append(Case("nan-in-query", np.array([[np.nan, 0.0]], F32), fine, refused=True))
    return out


def lq0_case():
    """rerank.rs:61: no query row, the loop body never runs: every document scores 0.0 and the stable sort keeps the
    input order."""
    g = np.random.default_rng(9500)
    docs = [g.standard_normal((n, 4)).astype(F32) for n in (3, 0, 300)]
    return Case("no-query-tokens", np.zeros((0, 4), F32), docs, np.zeros(3, F32))


_cache = {}


def all_cases():
    if "all" not in _cache:
        _cache["all"] = random_cases() + constructed_cases() + nonfinite_cases() + [lq0_case()]
    return _cache["all"]
