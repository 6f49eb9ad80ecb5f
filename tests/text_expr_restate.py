"""Keyword search over a tree query (np_text_expr) restated in pure Python / numpy over a text.TextIndexData: the rule that
np_hip_text_search_expr implements, in f64, operation for operation as text_expr_kernel computes it.

  match   the boolean value of the tree over "phrase p occurs in the document"; NOT is binary, a AND NOT b
  score   bm25's sum in PHRASE order (the order of the query text) over the phrases that are LIVE in the document: the phrase
          occurs, every node on its path to the root is true, and the path enters no NOT from the right
  nHit    the phrase's own, whatever stands around it; a prefix phrase: the documents holding any term of its range, and its
          frequency adds the instances of all of them

tests/test_text_expr_restate_cpu.py pins the rule (and text.compile_text_expr) to SQLite itself; tests/test_gpu_text_expr.py
pins the device to this file bit for bit.  `defect` plants one wrong reading of the rule, for the CPU test that shows each
is caught."""
import random

import numpy as np

from next_plaid_amd import text as T
from text_restate import K1, B_, Restated

DEFECTS = ("not_right_counts", "false_and_counts", "tree_order", "subtree_sums", "nhit_from_matches", "prefix_counts_terms",
           "prefix_nhit_over_terms")


class RestatedExpr(Restated):
    def expr_phrase_freqs(self, phrase, rng, defect=None):
        """({document: frequency}, nHit) of one phrase; rng = None or the (lo, hi) its last token stands for."""
        if rng is None:
            f = self.phrase_freqs(phrase)
            return f, len(f)
        out, over_terms = {}, 0
        for t in range(rng[0], rng[1]):
            f = self.phrase_freqs(list(phrase[:-1]) + [t])
            over_terms += len(f)
            for d, c in f.items():
                out[d] = out.get(d, 0) + (1 if defect == "prefix_counts_terms" else c)
        if defect == "prefix_nhit_over_terms":   # (kept at nRow at most, where the idf is still defined)
            return out, min(over_terms, self.n_rows)
        return out, len(out)

    def expr_scores(self, expr, defect=None):
        """{document: f64 score} of every matching document of the whole table.  One numpy lane per document: the same IEEE
        operations in the same order as a scalar loop."""
        n = int(self.doc_len.size)
        phrases, nodes = expr.phrases(), expr.nodes.tolist()
        freqs, hits = [], []
        for p, r in zip(phrases, expr.prefix):
            f, h = self.expr_phrase_freqs(p, r, defect)
            arr = np.zeros(n, np.int64)
            if f:
                arr[np.fromiter(f.keys(), np.int64, len(f))] = np.fromiter(f.values(), np.int64, len(f))
            freqs.append(arr)
            hits.append(h)
        occurs = [f > 0 for f in freqs]
        truth = [None] * len(nodes)
        for x, (op, a, b) in enumerate(nodes):
            if op == T.NP_TEXT_NODE_PHRASE:
                truth[x] = occurs[a]
            elif op == T.NP_TEXT_NODE_AND:
                truth[x] = truth[a] & truth[b]
            elif op == T.NP_TEXT_NODE_OR:
                truth[x] = truth[a] | truth[b]
            else:
                truth[x] = truth[a] & ~truth[b]
        root = len(nodes) - 1
        match = truth[root]
        # liveness from the root down (children lie below their parent): a child is live if its parent is and the child is
        # true, never the right child of a NOT.  `free` = a planted defect lets everything below the node count
        none = np.zeros(n, bool)
        live_node, free, live = [none] * len(nodes), [False] * len(nodes), [none] * len(phrases)
        live_node[root] = match
        free[root] = defect == "false_and_counts"
        for x in range(root, -1, -1):
            op, a, b = nodes[x]
            if op == T.NP_TEXT_NODE_PHRASE:
                live[a] = live_node[x] & occurs[a]
                continue
            live_node[a] = live_node[x] & (truth[a] | free[x])
            live_node[b] = none if op == T.NP_TEXT_NODE_NOT else live_node[x] & (truth[b] | free[x])
            free[a] = free[b] = free[x]
            if defect == "not_right_counts" and op == T.NP_TEXT_NODE_NOT:
                live_node[b], free[b] = live_node[x], True
        if defect == "nhit_from_matches":
            hits = [int(np.count_nonzero(match & o)) for o in occurs]
        avgdl = float(self.total_tokens) / float(self.n_rows) if self.n_rows else 0.0
        D = self.doc_len.astype(np.float64)
        terms = []
        for p in range(len(phrases)):
            a = freqs[p].astype(np.float64)
            with np.errstate(all="ignore"):
                terms.append(self.idf(hits[p]) * ((a * (K1 + 1.0)) / (a + K1 * (1 - B_ + B_ * D / avgdl))))
        score = np.zeros(n, np.float64)
        if defect == "subtree_sums":   # the tree's own order: every node adds the sums of its two sides, (a + b) + (c + d)
            part = [None] * len(nodes)
            for x, (op, a, b) in enumerate(nodes):
                part[x] = np.where(live[a], terms[a], 0.0) if op == T.NP_TEXT_NODE_PHRASE else part[a] + part[b]
            score = score + part[root]
        else:
            order = range(len(phrases)) if defect != "tree_order" else reversed(range(len(phrases)))   # (tree_order: right to left)
            for p in order:
                score = np.where(live[p], score + terms[p], score)
        return {int(d): float(score[d]) for d in np.nonzero(match)[0]}

    def expr_search(self, expr, top_k, subset=None, defect=None):
        """(ids int64, scores float32): f64 score descending, ties by ascending id; `subset`: only these ids."""
        return self.rank(self.expr_scores(expr, defect), top_k, subset)


# ---- the generator of the probe: words that share prefixes, random trees up to depth 4 ---------------------------------------

WORDS = ["ab", "abc", "abd", "b", "ba", "bab", "c", "ca", "cab", "d", "da", "e"]
UNKNOWN = "zq"


def make_table(rng, n_rows):
    """n_rows documents of 0..13 tokens over WORDS."""
    return [" ".join(rng.choice(WORDS) for _ in range(rng.randint(0, 13))) for _ in range(n_rows)]


def random_tree(rng, depth, multi=True, nots=True, prefixes=True):
    """A random query tree as nested tuples: ("p", [words], star) | ("list", [p, ...]) | (op, l, r)."""
    def phrase():
        n = rng.choice([1, 1, 1, 2, 2, 3]) if multi else 1
        words = [rng.choice(WORDS + [UNKNOWN]) if rng.random() < 0.08 else rng.choice(WORDS) for _ in range(n)]
        return ("p", words, prefixes and rng.random() < 0.3)

    def node(d):
        if d == 0 or rng.random() < 0.3:
            return ("list", [phrase() for _ in range(rng.choice([1, 1, 1, 2, 3]))])
        op = rng.choice(["AND", "OR", "NOT"] if nots else ["AND", "OR"])
        return (op, node(d - 1), node(d - 1))

    return node(depth)


def tree_text(t, parens=True, rng=None):
    """FTS5 text of a tree.  parens=False: no parentheses at all (what the text then means is up to the precedence)."""
    if t[0] == "p":
        _, words, star = t
        style = rng.randrange(3) if rng else 0
        body = ('"' + " ".join(words) + '"') if style == 0 or (style == 2 and len(words) == 1) else \
            (" + ".join(words) if style == 1 else " + ".join('"' + w + '"' for w in words))
        return body + (" *" if star else "")
    if t[0] == "list":
        return " ".join(tree_text(p, parens, rng) for p in t[1])
    l, r = tree_text(t[1], parens, rng), tree_text(t[2], parens, rng)
    if parens:
        l = l if t[1][0] == "list" else "(" + l + ")"
        r = r if t[2][0] == "list" else "(" + r + ")"
    return f"{l} {t[0]} {r}"


def tree_class(t):
    """'A': no NOT, single-token phrases only; 'B': like A plus NOTs without an OR ancestor whose right side holds no NOT;
    'other' for the rest."""
    def single(t):
        if t[0] == "list":
            return all(len(p[1]) == 1 for p in t[1])
        return single(t[1]) and single(t[2])

    def has(t, op):
        return t[0] != "list" and (t[0] == op or has(t[1], op) or has(t[2], op))

    def nots_ok(t, under_or):
        if t[0] == "list":
            return True
        if t[0] == "NOT" and (under_or or has(t[2], "NOT")):
            return False
        u = under_or or t[0] == "OR"
        return nots_ok(t[1], u) and nots_ok(t[2], u)

    if not single(t):
        return "other"
    if not has(t, "NOT"):
        return "A"
    return "B" if nots_ok(t, False) else "other"


def tree_expr(t, data):
    """The TextExpr of a generated tree, built WITHOUT the compiler: the GPU tests' way from a tree to a query."""
    def conv(t):
        if t[0] == "p":
            ids = [data.vocab.get(w, -1) for w in t[1]]
            return ("phrase", ids, T.prefix_range(t[1][-1], data) if t[2] else None)
        if t[0] == "list":
            out = conv(t[1][0])
            for p in t[1][1:]:
                out = ("and", out, conv(p))
            return out
        return (t[0].lower(), conv(t[1]), conv(t[2]))
    return T.TextExpr.from_tree(conv(t))
