"""What the keyword search's limit tests share: the builders of tests/test_gpu_text_limits.py (an index straight from arrays, a
handle that only has a document count, the bit comparison, the plan's constants), np::text_plan restated, and the corpora and
trees with which tests/test_gpu_text_expr_limits.py drives the tree kernels to their own constants.

The generators take their size as an argument: tests/test_text_expr_limits_cpu.py runs the same functions at a reduced size
through SQLite's own FTS5, so that the restatement the device is compared with is pinned on the very shapes used there."""
import os
import re

import numpy as np

from helpers import ROOT, hip_index, make_arrays

from next_plaid_amd import text as T
import text_expr_restate as X

SLICE = 4096   # documents per slice of the scoring kernels (NP_TEXT_SLICE_DOCS, np_text_plan.h)
CAP = T.NP_TEXT_MAX_TOPK


def plan_constant(name):
    with open(os.path.join(ROOT, "next-plaid_amd", "csrc", "np_text_plan.h")) as f:
        return int(re.search(rf"constexpr int64_t {name} = (\d+);", f.read()).group(1))


def tiny_arrays(n_docs):
    return make_arrays(num_docs=n_docs, num_centroids=16, dim=32, nbits=2, doc_len_min=1, doc_len_max=1, seed=3)[1]


def tiny_index(n_docs, **opts):
    """An index of n_docs one-token documents: the keyword search only needs its document count."""
    a = tiny_arrays(n_docs)
    return a, hip_index(a, **opts)


def same(r, ids, sc):
    return (r.passage_ids.dtype == np.int64 and r.scores.dtype == np.float32 and np.array_equal(r.passage_ids, ids)
            and np.array_equal(r.scores.view(np.uint32), sc.view(np.uint32)))


def same_rows(a, b):
    return len(a) == len(b) and all(same(x, y.passage_ids, y.scores) for x, y in zip(a, b))


def index_data(terms, per_term, n_rows):
    """A TextIndexData from per-term (documents, positions) arrays in any order: sorted to (document, position) here."""
    docs, poss, off = [], [], [0]
    for d, p in per_term:
        d, p = np.asarray(d, np.int64), np.asarray(p, np.int64)
        o = np.argsort(d * (1 << 32) + p, kind="stable")
        docs.append(d[o])
        poss.append(p[o].astype(np.int32))
        off.append(off[-1] + d.size)
    assert list(terms) == sorted(terms)
    return T.TextIndexData("unicode61", list(terms), np.asarray(off, np.int64), np.concatenate(docs), np.concatenate(poss), int(n_rows),
                           {t: i for i, t in enumerate(terms)})


class Instances:
    """Token instances gathered a term at a time: put("w", documents, positions) any number of times, then data()."""

    def __init__(self):
        self.by_term = {}

    def put(self, term, docs, pos):
        docs = np.asarray(docs, np.int64).reshape(-1)
        pos = np.broadcast_to(np.asarray(pos, np.int64), docs.shape)
        if docs.size:
            self.by_term.setdefault(term, []).append((docs, pos))

    def data(self, n_rows):
        terms = sorted(self.by_term)
        return index_data(terms, [(np.concatenate([d for d, _ in self.by_term[t]]), np.concatenate([p for _, p in self.by_term[t]]))
                                  for t in terms], n_rows)


def data_of_token_lists(docs):
    """A TextIndexData from one list of words per document."""
    inst = Instances()
    where = {}
    for d, words in enumerate(docs):
        for p, w in enumerate(words):
            where.setdefault(w, ([], []))
            where[w][0].append(d)
            where[w][1].append(p)
    for w, (d, p) in where.items():
        inst.put(w, d, p)
    return inst.data(len(docs))


def texts_of(data):
    """The documents of a TextIndexData as text, one per row: what SQLite is handed for the same index."""
    term = np.repeat(np.arange(data.n_terms), np.diff(data.term_offsets))
    o = np.lexsort((data.inst_pos, data.inst_doc))
    words = [[] for _ in range(data.n_rows)]
    for t, d, p in zip(term[o].tolist(), data.inst_doc[o].tolist(), data.inst_pos[o].tolist()):
        assert p == len(words[d]), "positions without gaps"
        words[d].append(data.terms[t])
    return [" ".join(w) for w in words]


class CachedExpr(X.RestatedExpr):
    """tests/text_expr_restate.py's rule unchanged; a phrase's frequencies are computed once per corpus, whichever trees
    name it."""

    def __init__(self, data, n_docs=None):
        super().__init__(data, n_docs)
        self._memo = {}

    def expr_phrase_freqs(self, phrase, rng, defect=None):
        if defect is not None:
            return super().expr_phrase_freqs(phrase, rng, defect)
        key = (tuple(phrase), None if rng is None else tuple(rng))
        if key not in self._memo:
            self._memo[key] = super().expr_phrase_freqs(phrase, rng)
        return self._memo[key]


# ---- np::text_plan and the sizes around it (np_text_plan.h, np_text.hip), restated -------------------------------------------

def up256(x):
    return (int(x) + 255) // 256 * 256


def pair_bytes(top_k):
    return min(int(top_k), SLICE) * 12 + 4


def per_query_bytes(n_docs, top_k, subsets=False, slots=0):
    """text_per_query + TextProg::per_query_extra: the best-so-far list, the subset's bitmap, `slots` frequency arrays."""
    nw = max((n_docs + 31) // 32, 1)
    stride = (max(n_docs, 1) + 63) // 64 * 64
    return up256(top_k * 8) + up256(top_k * 4) + 8 + (up256(nw * 4) if subsets else 0) + slots * stride * 4


def result_bytes(B, top_k):
    """ResultStage::bytes (np_internal.h): a call's results in the arena, part of the plan's fixed bytes."""
    return up256(B * top_k * 8) + up256(B * top_k * 4) + up256(B * 4)


def subset_stage_bytes(B, n_subsets, total_ids):
    """HostScope::stage_bytes: a host CSR of subsets staged in the arena."""
    return up256(max(total_ids, 1) * 8) + up256((n_subsets + 1) * 8) + up256(B * 4)


def restated_plan(budget, fixed, per_query, n_slices, B, max_batch, top_k):
    """np::text_plan: (queries, slices) of a chunk, or None where one query over one slice does not fit."""
    n_slices = max(n_slices, 1)
    Q = max(B, 1)
    if max_batch >= 1 and Q > max_batch:
        Q = max_batch
    want = min(n_slices, 8)
    while True:
        left = budget - fixed - Q * per_query
        S = left // (Q * pair_bytes(top_k)) if left > 0 else 0
        if S >= want or Q == 1:
            return None if S < 1 else (Q, min(S, n_slices))
        Q = (Q + 1) // 2


def n_slices_of(n_docs):
    return max(1, (n_docs + SLICE - 1) // SLICE)


# ---- trees in text_expr_restate's form: ("p", words, star) | ("list", [p, ...]) | (op, left, right) --------------------------

def leaf(*words, star=False):
    return ("list", [("p", list(words), star)])


def chained(op, leaves):
    t = leaves[0]
    for x in leaves[1:]:
        t = (op, t, x)
    return t


def n_arrays(expr):
    """Frequency arrays a tree owns: its single-token phrases that end in a prefix (TextProg::build_expr)."""
    return sum(1 for p, hi in zip(expr.phrases(), expr.prefix_hi().tolist()) if hi != 0 and len(p) == 1)


# ---- A1: runs longer than the counting grid ---------------------------------------------------------------------------------

def long_run_size(grid):
    """Documents of the long-run corpus for a counting grid of `grid` postings: 2 / 5 of them hold three terms of the range
    (6 / 5 postings per document), every one holds the first token of the phrase."""
    return grid + grid // 16


def long_run_corpus(n):
    """n documents for runs longer than the counting grid.  Document d holds "h", then
         d % 5 < 2                "pa{d%7} pb{d%3} pc{d%11}"     three terms of the range p*
         else, d % 16 == 7        "pz"                           the LAST term of the range: these documents' only postings of
                                                                 the run lie at its end
         else                     "x{d%4}"
    then filler "fz" 4 + d % 29 times, or (d // 64) % 4 times where d % 64 == 3: 33 document lengths, the shortest ones rare, so
    that the head of a ranking is not one tie.  Four documents `rev` hold "pa0 h": the tokens of "h pa*" without the phrase;
    document `big` holds "h" and then 200 terms of the range.  Returns (data, rev, big)."""
    d = np.arange(n, dtype=np.int64)
    rev = np.array([5, n // 3, n // 2 + 1, n - 1], np.int64)
    big = (2 * n) // 3 + 1
    assert n >= 400 and big not in rev and np.unique(rev).size == 4
    kind = np.where(d % 5 < 2, 0, np.where(d % 16 == 7, 2, 1))
    kind[rev] = 3
    kind[big] = 4
    inst = Instances()
    for k in (0, 1, 2, 4):
        inst.put("h", d[kind == k], 0)
    inst.put("h", rev, 1)
    inst.put("pa0", rev, 0)
    p = d[kind == 0]
    for name, mod, pos in (("pa", 7, 1), ("pb", 3, 2), ("pc", 11, 3)):
        for r in range(mod):
            inst.put(f"{name}{r}", p[p % mod == r], pos)
    inst.put("pz", d[kind == 2], 1)
    x = d[kind == 1]
    for r in range(4):
        inst.put(f"x{r}", x[x % 4 == r], 1)
    i200 = np.arange(200)
    for r in range(7):
        inst.put(f"pa{r}", np.full(np.count_nonzero(i200 % 7 == r), big), 1 + i200[i200 % 7 == r])
    base = np.array([4, 2, 2, 2, 201])[kind]
    fill = np.where(d % 64 == 3, (d // 64) % 4, 4 + d % 29)
    start = np.cumsum(fill) - fill
    inst.put("fz", np.repeat(d, fill), np.arange(int(fill.sum())) - np.repeat(start, fill) + np.repeat(base, fill))
    return inst.data(n), rev, big


def long_run_trees():
    """[(name, tree)]: the bare prefix, the phrase of two tokens that ends in a prefix, each under OR, each on the left of a
    NOT whose right side is another prefix, and the AND of the two."""
    bare, multi = leaf("p", star=True), leaf("h", "pa", star=True)
    return [("p*", bare), ("h + pa*", multi),
            ("p* OR x1*", ("OR", bare, leaf("x1", star=True))), ("h + pa* OR pc1*", ("OR", multi, leaf("pc1", star=True))),
            ("p* NOT pc1*", ("NOT", bare, leaf("pc1", star=True))), ("h + pa* NOT pb2*", ("NOT", multi, leaf("pb2", star=True))),
            ("p* AND h + pa*", ("AND", bare, multi))]


def run_postings(data, lo, hi):
    """(postings of the terms [lo, hi) -- (term, document) pairs, the entries text_prefix_kernel walks --, the documents
    among them, the documents of the run's postings in the order of the walk)."""
    o = data.term_offsets
    term = np.repeat(np.arange(lo, hi), np.diff(o[lo: hi + 1]))
    doc = data.inst_doc[o[lo]: o[hi]]
    first = np.r_[True, (term[1:] != term[:-1]) | (doc[1:] != doc[:-1])] if doc.size else np.zeros(0, bool)
    return int(first.sum()), int(np.unique(doc).size), doc[first]


def check_long_run(data, rs, rev, big, grid):
    """The conditions the corpus was built for, on the restatement alone.  grid = None: the size-independent ones."""
    n = data.n_rows
    v = data.vocab
    lo, hi = T.prefix_range("p", data)
    assert (lo, hi) == (v["pa0"], v["pz"] + 1) and hi - lo == 22
    postings, holders, _ = run_postings(data, lo, hi)
    freqs, hit = rs.expr_phrase_freqs([lo], (lo, hi))
    # (a) fewer holders than half of the documents (the idf is not the clamp), fewer holders than postings
    assert hit == holders == len(freqs) and holders < n / 2 and holders < postings and rs.idf(hit) > 1e-6
    # (c) one entry of the frequency array is 200, and nHit counts its document once
    assert freqs[big] == 200 and sum(1 for f in freqs.values() if f == 200) == 1 and all(freqs[int(r)] == 1 for r in rev)
    # (b) the first token's list, and documents that hold the tokens without the phrase
    pa = T.prefix_range("pa", data)
    h_list = rs.post[v["h"]]
    phrase, phrase_hit = rs.expr_phrase_freqs([v["h"], pa[0]], pa)
    assert len(h_list) == n and all(int(r) not in phrase and v["pa0"] in [t for t in range(*pa) if int(r) in rs.post[t]] for r in rev)
    assert phrase[big] == 1 and 0 < phrase_hit < len(h_list) and pa[1] - pa[0] == 7 <= T.NP_TEXT_MAX_PREFIX_TERMS
    if grid is not None:
        assert postings > grid and len(h_list) > grid
        assert int(data.term_offsets[hi] - data.term_offsets[lo]) == postings + 200 - 7   # (the 200 instances are 7 postings)
    return postings, holders


def long_run_subsets(data, grid, n_queries):
    """One subset of at most 1024 ids per query, read off term_offsets: documents whose postings lie past position `grid`
    of the run of p* (those of "pz" among them: all their postings of the run lie there), documents before it, and documents
    past position `grid` of the list of "h"; shifted from query to query."""
    v = data.vocab
    lo, hi = T.prefix_range("p", data)
    _, _, walked = run_postings(data, lo, hi)
    o = data.term_offsets
    h_docs = np.unique(data.inst_doc[o[v["h"]]: o[v["h"] + 1]])
    pz = data.inst_doc[o[v["pz"]]: o[v["pz"] + 1]]
    assert walked.size > grid and h_docs.size > grid and pz.size > 64
    past, before, h_past = walked[grid:], walked[:grid], h_docs[grid:]
    out = []
    for q in range(n_queries):
        pick = lambda a, k: a[(np.arange(k) * (a.size // k) + 7 * q) % a.size]
        s = np.unique(np.concatenate([pick(past, 400), pick(pz, 64), pick(before, 200), pick(h_past, 300)]))
        assert s.size <= 1024 and np.isin(s, past).sum() >= 300 and np.isin(s, pz).sum() >= 32 and (s >= grid).sum() >= 300
        out.append(s)
    return out


# ---- A2: sixty-four frequency arrays ----------------------------------------------------------------------------------------

N_FAMILIES = 64


def families_corpus(n):
    """n documents over the word families w00 .. w63 of three terms each (w00a, w00b, w00c).  Document d holds 1 + d % 5
    words, word j of family (7 d + 13 j) % 64 in variant (d + j) % 3.  Document 17 holds every family twice (variant b) and
    the last document every family once (variant a): the only matches of an AND over all families."""
    assert n > 40
    docs = [[f"w{(7 * d + 13 * j) % N_FAMILIES:02d}{'abc'[(d + j) % 3]}" for j in range(1 + d % 5)] for d in range(n)]
    docs[17] = [f"w{f:02d}b" for f in range(N_FAMILIES) for _ in range(2)]
    docs[n - 1] = [f"w{f:02d}a" for f in range(N_FAMILIES)]
    return data_of_token_lists(docs)


def families_trees():
    """{name: tree}: the four shapes of 64 phrases, and the small trees that stand between them in an uneven batch."""
    fam = lambda f: leaf(f"w{f:02d}", star=True)
    word = lambda f: leaf(f"w{f:02d}{'abc'[f % 3]}")
    return {
        "OR of 64 prefixes": chained("OR", [fam(f) for f in range(64)]),
        "AND of 64 prefixes": chained("AND", [fam(f) for f in range(64)]),
        "32 prefixes and 32 words": chained("OR", [fam(f) if f % 2 == 0 else word(f) for f in range(64)]),
        "32 prefixes NOT a prefix": ("NOT", chained("OR", [fam(f) for f in range(32)]), fam(40)),
        "one prefix": fam(5),
        "three prefixes": ("NOT", ("OR", fam(1), fam(2)), fam(3)),
        "flat OR": chained("OR", [word(0), word(9), word(33)]),
        "flat AND": chained("AND", [word(7), word(20)]),
        "flat word": word(63),
        "flat phrase": leaf("w07b", "w20c"),
    }


UNEVEN = ["OR of 64 prefixes", "flat OR", "one prefix", "flat AND", "flat word", "flat phrase", "three prefixes", "AND of 64 prefixes"]
UNEVEN_ARRAYS = [64, 0, 1, 0, 0, 0, 3, 64]
SHAPES_64 = ["OR of 64 prefixes", "AND of 64 prefixes", "32 prefixes and 32 words", "32 prefixes NOT a prefix"]


# ---- A3: ties through the tree kernel ---------------------------------------------------------------------------------------

def ties_corpus(n, extra=()):
    """n documents of the one word w; the documents of `extra` hold a second term, wx, as well."""
    docs = [["w"] for _ in range(n)]
    for d in extra:
        docs[d].append("wx")
    return data_of_token_lists(docs)


def ties_trees():
    """[(name, tree)]; zq is in no document."""
    w, zq = leaf("w"), leaf("zq")
    return [("w*", leaf("w", star=True)), ("w OR w", ("OR", w, w)), ("w NOT zq", ("NOT", w, zq)),
            ("(w OR zq) AND w*", ("AND", ("OR", w, zq), leaf("w", star=True)))]
