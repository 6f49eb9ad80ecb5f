"""The sharded keyword search of include/nextplaid_hip.h (np_hip_text_search_sharded) restated in numpy on top of
tests/text_restate.py, the corpus and the filter fixtures the CPU and the GPU tests share, and the probe scale of a filtered
query.

The protocol: the table is split by the library's document ranges, every shard ranks its own documents with the WHOLE table's
figures (nRow, average length, document frequencies, phrase hit counts), and the shards' lists are merged by (f64 score
descending, global id ascending).  `defect=` plants one of the mistakes an implementation can make; the CPU test shows that
every one of them changes a result on this corpus, so the GPU parity cannot pass with it in."""
import math
import random

import numpy as np

from next_plaid_amd import text as T
import text_restate as R

N_DOCS = 1501          # odd: the shards' ranges are unequal
GEOMETRY = dict(num_docs=N_DOCS, num_centroids=64, dim=32, nbits=2, doc_len_min=4, doc_len_max=12, seed=11)
DEFECTS = ("nrow", "avgdl", "df", "nhit", "f32", "notie", "short")
TIE_PAIRS = [(10 + i, N_DOCS - 11 - i) for i in range(12)]   # identical texts, one in the first shard, one in the last


def shard_ranges(n, G):
    """The library's document ranges: shard r holds [n * r // G, n * (r + 1) // G)."""
    return [(n * r // G, n * (r + 1) // G) for r in range(G)]


def corpus_texts(n=N_DOCS, seed=5):
    """About 1500 documents over a vocabulary of a few dozen terms, built so that a shard's own figures differ from the table's:
      lengths     the first half holds short documents (1..6 words), the second half long ones (12..40)
      one shard   "lefty" only below document 200, "righty" only in the last 150 (one shard only at every G <= 5)
      a phrase    "alpha beta" in 60 documents of the first fifth and in 6 of the rest; "beta alpha" and both words apart
                  elsewhere, so that the phrase's hit count is not a document frequency
      exact ties  TIE_PAIRS: the same text in the first and in the last shard
      empty       documents 0 and n // 2 have no token (nRow counts them)"""
    rng = random.Random(seed)
    words = [f"wo{i}" for i in range(24)]
    weights = [1.0 / (i + 1) for i in range(24)]
    texts = []
    for d in range(n):
        k = rng.randint(1, 6) if d < n // 2 else rng.randint(12, 40)
        texts.append(rng.choices(words, weights, k=k))
    for d in range(0, 200, 3):
        texts[d].insert(rng.randrange(len(texts[d]) + 1), "lefty")
    for d in range(n - 150, n, 2):
        texts[d].insert(rng.randrange(len(texts[d]) + 1), "righty")
    for d in range(5, 300, 5):                                   # 59 documents of the first fifth
        at = rng.randrange(len(texts[d]) + 1)
        texts[d][at:at] = ["alpha", "beta"]
    for d in (400, 700, 900, 1100, 1300, 1499):
        at = rng.randrange(len(texts[d]) + 1)
        texts[d][at:at] = ["alpha", "beta"] * (2 if d == 900 else 1)
    for d in range(310, n, 97):
        texts[d][0:0] = ["beta", "alpha"]
    for d in range(320, n, 89):
        texts[d] = ["alpha"] + texts[d] + ["beta"]
    for i, (a, b) in enumerate(TIE_PAIRS):
        texts[a] = texts[b] = ["tie", "wo1", f"wo{2 + i % 3}"] + ["wo0"] * (i % 4)
    texts[0] = []
    texts[n // 2] = []
    return [" ".join(t) for t in texts]


def special_queries(data):
    """The query forms of the parity tests: OR and AND, single-token and multi-token phrases (the counting exchange), an unknown
    term, terms on one shard only, a phrase with no match anywhere, the tie pairs."""
    v = data.vocab
    ids = lambda *ws: [v.get(w, -1) for w in ws]
    AND, OR = T.NP_TEXT_AND, T.NP_TEXT_OR
    return [T.TextQuery.from_phrases([ids("wo0")], AND),
            T.TextQuery.from_phrases([ids("wo3"), ids("wo5")], OR),
            T.TextQuery.from_phrases([ids("wo1"), ids("wo2")], AND),
            T.TextQuery.from_phrases([ids("alpha", "beta")], AND),                      # counted: 60 / 6 over the shards
            T.TextQuery.from_phrases([ids("alpha", "beta"), ids("wo4")], OR),
            T.TextQuery.from_phrases([ids("beta", "alpha"), ids("alpha", "beta")], OR),
            T.TextQuery.from_phrases([ids("nowhere")], OR),                             # an unknown term
            T.TextQuery.from_phrases([ids("wo2"), ids("nowhere")], OR),
            T.TextQuery.from_phrases([ids("lefty")], AND),                              # the first shard only
            T.TextQuery.from_phrases([ids("righty"), ids("wo1")], OR),                  # the last shard only, and everywhere
            T.TextQuery.from_phrases([ids("righty", "lefty")], AND),                    # a phrase with no match anywhere
            T.TextQuery.from_phrases([ids("tie")], AND),                                # exact f64 ties across the shards
            T.TextQuery.from_phrases([ids("tie"), ids("wo1")], AND)]


class Sharded:
    """A table split over G shards, searched by the protocol."""

    def __init__(self, rs, n_docs, G):
        self.rs, self.n, self.G = rs, n_docs, G
        self.ranges = shard_ranges(n_docs, G)
        self._freqs = {}

    def _phrase(self, phrase):
        key = tuple(phrase)
        if key not in self._freqs:
            self._freqs[key] = self.rs.phrase_freqs(list(phrase))
        return self._freqs[key]

    def shard_scores(self, query, r, defect=None):
        """{global id: f64 score} of shard r's matching documents; the figures are the table's unless `defect` says otherwise."""
        rs = self.rs
        lo, hi = self.ranges[r]
        phrases = query.phrases()
        whole = [self._phrase(p) for p in phrases]
        own = [{d: f for d, f in w.items() if lo <= d < hi} for w in whole]
        n_rows = (hi - lo) if defect == "nrow" else rs.n_rows
        idfs = []
        for p, w, o in zip(phrases, whole, own):
            multi = len(p) > 1
            local = (defect == "nhit" and multi) or (defect == "df" and not multi)
            n_hit = len(o) if local else len(w)
            x = (n_rows - n_hit + 0.5) / (n_hit + 0.5)
            v = math.log(x) if x > 0.0 else float("nan")   # (only a planted nRow can get here; C's log gives NaN too)
            idfs.append(1e-6 if v <= 0.0 else v)
        if defect == "avgdl":
            avgdl = float(int(rs.doc_len[lo:hi].sum())) / float(hi - lo)
        else:
            avgdl = float(rs.total_tokens) / float(rs.n_rows)
        if query.mode == T.NP_TEXT_AND:
            docs = set(own[0])
            for f in own[1:]:
                docs &= set(f)
        else:
            docs = set().union(*[set(f) for f in own])
        out = {}
        for d in docs:
            D = float(rs.doc_len[d])
            score = 0.0
            for f, idf in zip(own, idfs):
                a = float(f.get(d, 0))
                if a > 0.0:
                    score += idf * ((a * (R.K1 + 1.0)) / (a + R.K1 * (1 - R.B_ + R.B_ * D / avgdl)))
            out[d] = score
        return out

    def search(self, query, top_k, subset=None, defect=None):
        """(ids int64, scores float32) of the merged lists."""
        keep = None if subset is None else set(int(x) for x in np.asarray(subset).reshape(-1))
        lists = []
        for r in range(self.G):
            sc = self.shard_scores(query, r, defect)
            if keep is not None:
                sc = {d: s for d, s in sc.items() if d in keep}
            order = sorted(sc, key=lambda d: (-sc[d], d))[:top_k]       # the shard's own list is always right
            if defect == "short" and len(order) < top_k:
                continue
            lists.append([(sc[d], d) for d in order])
        merged = [e for l in lists for e in l]
        if defect == "f32":
            merged.sort(key=lambda e: (-float(np.float32(e[0])), e[1]))
        elif defect == "notie":
            merged.sort(key=lambda e: (-e[0], -e[1]))
        else:
            merged.sort(key=lambda e: (-e[0], e[1]))
        merged = merged[:top_k]
        return (np.asarray([e[1] for e in merged], np.int64),
                np.asarray([e[0] for e in merged], np.float64).astype(np.float32))


def find_f32_collision(rs, data, n_docs, Gs, tries=3000, seed=17):
    """A query and two documents of different shards (at some G of Gs) whose f64 scores differ but round to one f32, the larger
    id scoring higher -- so that a merge on f32 scores puts them the wrong way round.  Searches `tries` random OR queries;
    returns (query, hi_doc, lo_doc) or None."""
    rng = random.Random(seed)
    nt = len(data.terms)
    cuts = sorted({lo for G in Gs for lo, _ in shard_ranges(n_docs, G)} - {0})
    for _ in range(tries):
        q = T.TextQuery.from_phrases([[rng.randrange(nt)] for _ in range(rng.randint(2, 4))], T.NP_TEXT_OR)
        sc = rs.scores(q)
        by32 = {}
        for d, s in sc.items():
            by32.setdefault(np.float32(s).tobytes(), []).append(d)
        for ds in by32.values():
            if len(ds) < 2:
                continue
            ds.sort()
            for i, a in enumerate(ds):
                for b in ds[i + 1:]:
                    if sc[b] > sc[a] and any(a < c <= b for c in cuts):
                        return q, b, a
    return None


# ---- the filter fixtures and the probe scale --------------------------------------------------------------------------------

def filter_rows(n=N_DOCS):
    """Columns whose filters spread over every shard: z = d % 4 (even), u = 1 for 70 % of its rows in the first half of the
    index and 30 % in the second, s a text column for REGEXP."""
    d = np.arange(n, dtype=np.int64)
    u = np.where(d < n // 2, (d % 10 < 7), (d % 10 < 3)).astype(np.int64)
    s = [("alpha" if i % 3 == 0 else "Beta" if i % 3 == 1 else "ca_x") + str(i % 7) for i in range(n)]
    return {"z": d % 4, "u": u, "s": s}


SPREAD_FILTERS = [("z = ?", [1]), ("u = ?", [1])]     # evenly over the shards; roughly 70 / 30


def filter_ids(cond, rows):
    """The ids the fixtures' simple filters select (numpy; the GPU test compares the device's evaluation with it)."""
    z, u = np.asarray(rows["z"]), np.asarray(rows["u"])
    pick = {"z = ?": lambda p: z == p[0], "u = ?": lambda p: u == p[0], "z = ? AND u = ?": lambda p: (z == p[0]) & (u == p[1])}
    return np.nonzero(pick[cond[0]](cond[1]))[0].astype(np.int64)


def eligible_count(a, ids):
    """Centroids that occur in the documents `ids` (search.rs:350-364): n_elig of a subset."""
    off = np.concatenate([[0], np.cumsum(a["doc_lengths"])])
    codes = np.asarray(a["codes"])
    seen = set()
    for d in ids:
        seen.update(codes[off[d]:off[d + 1]].tolist())
    return len(seen)


def probe_scale(nprobe, n_total, length, n_elig):
    """clamp(nprobe * N / len, nprobe, n_elig) (search.rs:370-382), integer division; a subset without eligible centroids
    keeps nprobe."""
    if n_elig <= 0:
        return nprobe
    scaled = nprobe * n_total // length if length > 0 else nprobe
    return min(max(scaled, nprobe), n_elig)
