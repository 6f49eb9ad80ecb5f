"""Checker of np_hip_search_exact, the exhaustive exact search (test infrastructure; no GPU).

    truth(a, q)            float64 MaxSim of every document: exact_restate.reference
    rank(a, scores, k)     the top k of per-document scores by the entry point's order rule
    check_topk(...)        the four conditions a returned top-k has to meet, every margin the derived bound of exact_restate

exact_restate is imported and not modified: the reference, the restated kernel arithmetic (emulate) and the per-document
error bound (doc_bound) are the ones the S6 kernels are already held to.  The scan runs the same arithmetic document-major.
"""
import numpy as np

import exact_restate as X

F32 = np.float32


def truth(a, q):
    return X.reference(a, q)


def order_key(scores):
    """The key the results are ordered by: f32 total order on finite values, every non-finite value below them all
    (finite first, as S7)."""
    b = np.ascontiguousarray(scores, F32).view(np.uint32).astype(np.int64)
    k = np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)
    return np.where((b & 0x7F800000) == 0x7F800000, 0, k)


def in_scope(a, scope=None):
    """Ids of the non-empty documents in scope, ascending.  scope = None: every document; otherwise an array of ids, where
    duplicates count once and ids outside [0, N) are ignored."""
    lens = np.asarray(a["doc_lengths"], np.int64)
    ok = lens > 0
    if scope is not None:
        s = np.asarray(scope, np.int64).reshape(-1)
        s = s[(s >= 0) & (s < lens.size)]
        m = np.zeros(lens.size, bool)
        m[s] = True
        ok &= m
    return np.nonzero(ok)[0]


def rank(a, scores, k, scope=None):
    """(ids, scores as f32) of the k best in-scope non-empty documents: score descending, bit-equal scores by ascending id."""
    d = in_scope(a, scope)
    s = np.asarray(scores)[d].astype(F32)
    o = np.lexsort((d, -order_key(s)))[:k]
    return d[o], s[o]


def check_topk(a, q, ids, scores, k, precision, scope=None, what="", truth_bd=None):
    """Asserts that (ids, scores) is an exact top-k of query q over `scope`.  truth_bd: (truth, bound) when the caller has
    them already (they depend on the query and the precision only)."""
    p = X.prepare(a)
    t, bd = truth_bd if truth_bd is not None else (truth(a, q), X.doc_bound(a, q, X.kernel_class(precision, p.nbits)))
    ids = np.asarray(ids, np.int64)
    s32 = np.asarray(scores).astype(F32)
    got = np.asarray(scores, np.float64)
    d = in_scope(a, scope)
    # 1. the count; ids distinct, in scope, non-empty
    want = min(int(k), d.size)
    assert ids.size == want and got.size == want, f"{what}: {ids.size} results, expected min({k}, {d.size})"
    assert np.unique(ids).size == ids.size, f"{what}: a document is returned twice"
    assert np.isin(ids, d).all(), f"{what}: returned outside the scope or empty: {ids[~np.isin(ids, d)][:5]}"
    if want == 0:
        return
    # 2. every returned score inside the derived bound
    err = np.abs(got - t[ids])
    bad = np.nonzero(~(err <= bd[ids]))[0]
    assert bad.size == 0, f"{what}: documents {ids[bad[:5]]}: |score - truth| {err[bad[:5]]} over {bd[ids][bad[:5]]}"
    # 3. never increasing; bit-equal scores by ascending id
    assert not np.isnan(s32).any(), f"{what}: NaN score"
    assert np.all(s32[1:] <= s32[:-1]), f"{what}: scores increase: {s32}"
    same = s32[1:].view(np.uint32) == s32[:-1].view(np.uint32)
    assert np.all(ids[1:][same] > ids[:-1][same]), f"{what}: equal scores not by ascending id: {ids}"
    # 4. complete up to the proven error
    rest = np.setdiff1d(d, ids)
    last = ids[-1]
    bad = rest[~(t[rest] <= t[last] + bd[rest] + bd[last])]
    assert bad.size == 0, f"{what}: documents {bad[:5]} (truth {t[bad[:5]]}) beat the last hit {last} (truth {t[last]}) " \
                          f"by more than the bounds {bd[bad[:5]]} + {bd[last]}"
