"""Brute-force float64 restatement of the search path's selection rules, written from search.rs (test infrastructure).

Only valid on the dyadic corpora of tie_corpus.py, where every value before the exact stage is exact in float64 AND
in f32, so that it can be compared with the C oracle bit for bit.  It states the tie rules literally, with none of
the oracle's data structures:
- dense probe (search.rs:388-414): per token the n_probe best by cmp_score_descending; ties at the cut take the LOWEST
  centroid ids (select_nth_unstable_by leaves them open; the library's documented choice);
- batched probe (search.rs:164-232): per slab and token a literal (Reverse(score), id) max-heap -- peek() is the lowest
  score, of equal scores the largest id -- entered when it has room or the score is strictly better
  (is_score_better); max_scores only over the pairs that entered; slab heaps merged in slab order, entries best first,
  ties lower id first (BinaryHeap's iteration order is unspecified: the documented choice);
- thresholds (search.rs:417-425 dense: max_by over all tokens, the LAST of equal maxima; :243-251 batched);
- the sorted, deduplicated posting-list union (index.rs:1142-1156); subset retain (search.rs:434-437);
- approximate scores: sum over tokens of the per-token max, tokens with no finite max skipped (search.rs:305-324);
- S5: stable sort by approximate score descending over ascending ids, cut to n_full_scores, then to
  max(n_full_scores / 4, top_k) (search.rs:460-469).
"""
from __future__ import annotations

import heapq

import numpy as np


def key(x):
    """cmp_score_ascending as a sortable integer: finite values by value (total order: -0.0 < +0.0), every
    non-finite value equal and below all finite ones."""
    x = np.asarray(x, np.float32)
    b = x.view(np.uint32).astype(np.int64)
    k = np.where(b >> 31 == 1, (~b) & 0xFFFFFFFF, b | 0x80000000) + 1
    return np.where(np.isfinite(x), k, 0)


def qc64(q, cen):
    """Query-centroid scores in float64; returns them as f32 after checking the f32 value is the same number."""
    s = np.asarray(q, np.float64) @ np.asarray(cen, np.float64).T
    s32 = s.astype(np.float32)
    fin = np.isfinite(s)
    assert np.array_equal(s32[fin].astype(np.float64), s[fin]), "corpus is not dyadic: QC is not exact in f32"
    return s32


def top_lowest_ids(scores, ids, n):
    order = np.lexsort((ids, -key(scores)))
    return ids[order[:n]]


def probe_dense(qc, n_probe, thr, pool=None):
    K = qc.shape[1]
    pool = np.arange(K) if pool is None else np.asarray(pool, np.int64)
    cells = set()
    for row in qc:
        cells.update(top_lowest_ids(row[pool], pool, min(n_probe, pool.size)).tolist())
    if thr is not None:
        keep = set()
        for c in cells:
            col = qc[:, c]
            ks = key(col)
            best = np.nonzero(ks == ks.max())[0][-1]          # max_by: the last of equal maxima
            if col[best] >= np.float32(thr):
                keep.add(c)
        cells = keep
    return np.array(sorted(cells), np.int64)


def probe_batched(qc, n_probe, cbs, thr):
    Lq, K = qc.shape
    kq = key(qc)
    final = [[] for _ in range(Lq)]                  # heapq min-heaps of (key, -id): heap[0] = peek()
    max_scores = {}                                  # c -> score of the pushed pairs, max_score(): first of equals

    def push(h, k, c):
        if len(h) < n_probe:
            heapq.heappush(h, (k, -c))
            return True
        if k > h[0][0]:                              # is_score_better: strict
            heapq.heapreplace(h, (k, -c))
            return True
        return False

    for b0 in range(0, K, cbs):
        for q in range(Lq):
            h = []
            for c in range(b0, min(b0 + cbs, K)):
                if push(h, kq[q, c], c):
                    v = qc[q, c]
                    if c not in max_scores or key(v) > key(max_scores[c]):
                        max_scores[c] = v
            for k, mc in sorted(h, key=lambda e: (-e[0], -e[1])):
                push(final[q], k, -mc)
    cells = {-mc for h in final for _, mc in h}
    if thr is not None:
        cells = {c for c in cells if c in max_scores and max_scores[c] >= np.float32(thr)}
    return np.array(sorted(cells), np.int64)


def candidates(a, cells, subset=None):
    off = np.concatenate([[0], np.cumsum(a["ivf_lengths"])])
    parts = [a["ivf"][off[c]: off[c + 1]] for c in cells]
    cand = np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.int64)
    if subset is not None:
        cand = cand[np.isin(cand, np.asarray(subset, np.int64))]
    return cand


def approx_scores(a, qc, cand):
    doff = np.concatenate([[0], np.cumsum(a["doc_lengths"])])
    out = np.zeros(cand.size, np.float64)
    for i, d in enumerate(cand):
        sub = qc[:, a["codes"][doff[d]: doff[d + 1]]].astype(np.float64)
        for row in sub:
            f = row[~np.isnan(row)]                     # `cs > max_score` from -inf: NaN never counts
            if f.size and f.max() > -np.inf:
                out[i] += f.max()
    s32 = out.astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), out), "approximate scores are not exact in f32"
    return s32


def select(cand, approx, n_full_scores, top_k):
    order = np.lexsort((np.arange(cand.size), -key(approx)))
    n_dec = min(max(n_full_scores // 4, top_k), min(cand.size, n_full_scores))
    return cand[order[:n_dec]]


def search(a, q, n_probe, nfs, top_k, thr, cbs=100_000, subset=None):
    """(cells, cand, approx, sel) of the reference path on a dyadic corpus."""
    K = a["centroids"].shape[0]
    qc = qc64(q, a["centroids"])
    if cbs > 0 and K > cbs:
        cells = probe_batched(qc, n_probe, cbs, thr)
    else:
        pool, eff = None, n_probe
        if subset is not None:
            doff = np.concatenate([[0], np.cumsum(a["doc_lengths"])])
            N = a["doc_lengths"].size
            el = set()
            for d in subset:
                if 0 <= d < N:
                    el.update(a["codes"][doff[d]: doff[d + 1]].tolist())
            if el:
                pool = np.array(sorted(el), np.int64)
                eff = min(max(n_probe * N // len(subset) if len(subset) else n_probe, n_probe), pool.size)
        cells = probe_dense(qc, eff, thr, pool)
    cand = candidates(a, cells, subset)
    approx = approx_scores(a, qc, cand)
    return cells, cand, approx, select(cand, approx, nfs, top_k)


def final_order(sel, exact, top_k):
    """S7 (search.rs:496-499): stable sort of the S5 selection by exact score descending -- equal exact scores keep
    their S5 (approximate-rank) order."""
    order = np.lexsort((np.arange(sel.size), -key(exact)))
    return sel[order[:top_k]]
