"""The sharded keyword search over TREE queries (np_hip_text_search_sharded_expr) restated in numpy on top of
tests/text_expr_restate.py, and the corpus and queries its CPU and GPU tests share.

The protocol: the table is cut by the library's document ranges; every shard counts the nHit of every phrase over its own
documents -- exact, of several tokens, a single-token prefix (the documents that hold any term of the range), several tokens
ending in a prefix -- and the counts are summed; every shard then scores its documents by the tree rule with the WHOLE table's
nRow, average length and the summed counts, and the shards' lists are merged by (f64 score descending, global id ascending).
`defect=` plants one mistake an implementation can make; the CPU test shows that each changes a result on this corpus."""
import math
import random

import numpy as np

from next_plaid_amd import text as T
from text_expr_restate import RestatedExpr

N_CPU = 1501           # odd: the shards' ranges are unequal
N_GPU = 9001           # a 2-rank shard spans two 4096-document slices, and no shard boundary (4500; 3000, 6000) is a slice's
GS = (1, 2, 3)
DEFECTS = ("prefix_nhit_local", "prefix_nhit_df_sum", "multi_prefix_nhit_local", "nrow", "avgdl", "f32", "notie")


def shard_ranges(n, G):
    """The library's document ranges: shard r holds [n * r // G, n * (r + 1) // G)."""
    return [(n * r // G, n * (r + 1) // G) for r in range(G)]


def tie_pairs(n):
    """identical texts, one in the first shard, one in the last (at every G <= 3)"""
    return [(10 + i, n - 11 - i) for i in range(12)]


def corpus_texts(n, seed=5):
    """n short documents over a few dozen terms, built so that a shard's own figures differ from the table's:
      lengths     the first half holds short documents (1..6 words), the second half longer ones (14..26)
      lef*        "lefa" and "lefb" only below document n // 6 (one shard at G = 2 and 3); every 15th holds both
      mid*        "mida" ends every 4th document of the whole table, "midb" occurs in the last sixth only (a term of the range
                  that the first shard lacks); a document of the tail may hold both
      alpha mid*  "alpha" starts every 7th document of the first half and is never followed by a mid word there; from
                  n // 2 + 5 on every 11th document ends in "alpha mida" or "alpha midb": no hit on the first shard
      wo1 mid*    arises by itself all over the table ("mida" is appended behind a random word)
      nota, notb  "nota" in every 9th document; below n // 2 every such document holds "notb" too, above every other one:
                  `nota NOT notb` is empty on the first shard
      ties        tie_pairs(n): the same text in the first and in the last shard
      empty       documents 0 and n // 2 have no token (nRow counts them)"""
    rng = random.Random(seed)
    words = [f"wo{i}" for i in range(16)]
    weights = [1.0 / (i + 1) for i in range(16)]
    texts = []
    for d in range(n):
        k = rng.randint(1, 6) if d < n // 2 else rng.randint(14, 26)
        texts.append(rng.choices(words, weights, k=k))
    mid = lambda t: rng.randrange(1, len(t) + 1)       # never the front: "alpha" goes there
    for d in range(3, n // 6, 3):
        texts[d].insert(mid(texts[d]), "lefa")
    for d in range(5, n // 6, 5):
        texts[d].insert(mid(texts[d]), "lefb")
    for d in range(9, n, 9):
        texts[d].insert(mid(texts[d]), "nota")
        if d < n // 2 or (d // 9) % 2 == 0:
            texts[d].insert(mid(texts[d]), "notb")
    for d in range(n - n // 6, n, 3):
        texts[d].insert(mid(texts[d]), "midb")
    for d in range(0, n, 4):
        texts[d].append("mida")
    for d in range(7, n // 2, 7):
        texts[d].insert(0, "alpha")
    for i, d in enumerate(range(n // 2 + 5, n, 11)):
        texts[d] += ["alpha", "midb" if i % 3 == 2 else "mida"]
    for i, (a, b) in enumerate(tie_pairs(n)):
        texts[a] = texts[b] = ["tie", "wo1", f"wo{2 + i % 3}"] + ["wo0"] * (i % 4)
    texts[0] = []
    texts[n // 2] = []
    return [" ".join(t) for t in texts]


def special_trees(data):
    """(name, tree) for TextExpr.from_tree: every class of phrase and operator the sharded counts and merge must get right."""
    v = data.vocab
    nt = len(data.terms)
    P = lambda *ws: ("phrase", [v.get(w, -1) for w in ws])
    PX = lambda pre, *ws: ("phrase", [v.get(w, -1) for w in ws] + [0], T.prefix_range(pre, data))
    return [
        ("lef*", PX("lef")),                                            # a range whose documents lie on one shard
        ("mid*", PX("mid")),                                            # a term of the range is absent from a shard
        ("alpha mid*", PX("mid", "alpha")),                             # several tokens ending in a prefix: no hit on a shard
        ("wo1 mid*", PX("mid", "wo1")),                                 # ... and hits on every shard
        ("nota NOT notb", ("not", P("nota"), P("notb"))),               # a NOT that empties a shard
        ("(lef* OR mid*) AND wo0", ("and", ("or", PX("lef"), PX("mid")), P("wo0"))),
        ("(wo1 mid* OR alpha mid*) NOT wo2", ("not", ("or", PX("mid", "wo1"), PX("mid", "alpha")), P("wo2"))),
        ("wo3 wo1 OR lef* NOT lefb", ("or", P("wo3", "wo1"), ("not", PX("lef"), P("lefb")))),
        ("tie", P("tie")),                                              # exact f64 ties across the shards
        ("tie AND wo* NOT nota", ("not", ("and", P("tie"), PX("wo")), P("nota"))),
        ("zz*", ("or", PX("zz"), P("wo5"))),                            # a prefix of no term
        ("lefa*", PX("lefa")),                                          # ... of one term
        ("every term", ("phrase", [0], (0, nt))),                       # ... of every term
        ("nowhere OR wo4", ("or", P("nowhere"), P("wo4"))),             # an unknown token
        ("nowhere mid* OR mid*", ("or", PX("mid", "nowhere"), PX("mid"))),   # ... in a phrase that ends in a prefix: not counted
    ]


def special_exprs(data):
    return [T.TextExpr.from_tree(t) for _, t in special_trees(data)]


def counted_phrases(exprs):
    """The count vector of a batch, as the library lays it out from the queries alone: (the phrases of several known tokens,
    the single-token prefix phrases), each as (query, phrase) in query and phrase order."""
    multi, prefix = [], []
    for q, e in enumerate(exprs):
        hi = e.prefix_hi()
        for p, ids in enumerate(e.phrases()):
            if any(t < 0 for t in ids):
                continue
            if len(ids) > 1:
                multi.append((q, p))
            elif hi[p] != 0:
                prefix.append((q, p))
    return multi, prefix


class _Shard(RestatedExpr):
    """One shard's view of the table for RestatedExpr.expr_scores: its own documents' frequencies, and the figures it is told."""

    def __init__(self, rs, freqs_of, idf_rows, avg_tokens, avg_rows):
        self.doc_len = rs.doc_len
        self.freqs_of, self.idf_rows = freqs_of, idf_rows
        self.total_tokens, self.n_rows = avg_tokens, avg_rows      # (expr_scores takes avgdl from these two)

    def idf(self, n_hit):
        x = (self.idf_rows - n_hit + 0.5) / (n_hit + 0.5)
        v = math.log(x) if x > 0.0 else float("nan")               # (only a planted nRow can get here; C's log gives NaN too)
        return 1e-6 if v <= 0.0 else v

    def expr_phrase_freqs(self, phrase, rng, defect=None):
        return self.freqs_of(tuple(phrase), rng)


class ShardedExpr:
    """A table split over G shards, searched with tree queries by the protocol."""

    def __init__(self, rs, n_docs, G):
        self.rs, self.n, self.G = rs, n_docs, G
        self.ranges = shard_ranges(n_docs, G)
        self._whole = {}

    def _phrase(self, phrase, rng):
        """({document: frequency} over the whole table, the sum of the range's document frequencies)"""
        key = (tuple(phrase), rng)
        if key not in self._whole:
            f, _ = self.rs.expr_phrase_freqs(list(phrase), rng)
            over = 0 if rng is None else sum(len(self.rs.phrase_freqs(list(phrase[:-1]) + [t])) for t in range(rng[0], rng[1]))
            self._whole[key] = (f, over)
        return self._whole[key]

    def shard_hits(self, phrase, rng):
        """the shards' own nHit of one phrase: what each counts and sends"""
        f, _ = self._phrase(phrase, rng)
        return [sum(1 for d in f if lo <= d < hi) for lo, hi in self.ranges]

    def shard_scores(self, expr, r, defect=None):
        """{global id: f64 score} of shard r's matching documents; the figures are the table's unless `defect` says otherwise."""
        rs = self.rs
        lo, hi = self.ranges[r]

        def freqs_of(phrase, rng):
            f, over = self._phrase(phrase, rng)
            own = {d: c for d, c in f.items() if lo <= d < hi}
            per_shard = self.shard_hits(phrase, rng)
            n_hit = sum(per_shard)
            single = len(phrase) == 1
            if rng is not None and rng[1] > rng[0]:
                if (defect == "prefix_nhit_local" and single) or (defect == "multi_prefix_nhit_local" and not single):
                    n_hit = per_shard[r]
                if defect == "prefix_nhit_df_sum" and single:
                    n_hit = min(over, rs.n_rows)
            return own, n_hit

        n_rows = (hi - lo) if defect == "nrow" else rs.n_rows
        if defect == "avgdl":
            view = _Shard(rs, freqs_of, n_rows, int(rs.doc_len[lo:hi].sum()), hi - lo)
        else:
            view = _Shard(rs, freqs_of, n_rows, rs.total_tokens, rs.n_rows)
        return view.expr_scores(expr)

    def search(self, expr, top_k, subset=None, defect=None):
        """(ids int64, scores float32) of the merged lists."""
        keep = None if subset is None else set(int(x) for x in np.asarray(subset).reshape(-1))
        merged = []
        self.last_lengths = []
        for r in range(self.G):
            sc = self.shard_scores(expr, r, defect)
            if keep is not None:
                sc = {d: s for d, s in sc.items() if d in keep}
            order = sorted(sc, key=lambda d: (-sc[d], d))[:top_k]       # the shard's own list is always right
            self.last_lengths.append(len(order))
            merged += [(sc[d], d) for d in order]
        if defect == "f32":
            merged.sort(key=lambda e: (-float(np.float32(e[0])), e[1]))
        elif defect == "notie":
            merged.sort(key=lambda e: (-e[0], -e[1]))
        else:
            merged.sort(key=lambda e: (-e[0], e[1]))
        merged = merged[:top_k]
        return (np.asarray([e[1] for e in merged], np.int64),
                np.asarray([e[0] for e in merged], np.float64).astype(np.float32))
