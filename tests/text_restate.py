"""The keyword search and the fusion of include/nextplaid_hip.h restated in pure Python / numpy: SQLite FTS5's bm25() in f64,
operation for operation, over the arrays of a text.TextIndexData, and the reference's two fusions in f32.

tests/test_text_restate_cpu.py pins the restatement to SQLite itself (bm25() bit-equal, matching sets equal);
tests/test_gpu_text.py pins the device to the restatement, ids equal and f32 scores bit for bit."""
import math
import random

import numpy as np

from next_plaid_amd import text as T

K1, B_ = 1.2, 0.75
F32 = np.float32


class Restated:
    """A keyword index as the library derives it from the instances: per term {document: ascending positions}, every
    document's token count, the total, nRow."""

    def __init__(self, data, n_docs=None):
        self.data = data
        self.n_rows = int(data.n_rows)
        self.post = []
        off, doc, pos = data.term_offsets, data.inst_doc, data.inst_pos
        n_docs = int(n_docs if n_docs is not None else (doc.max() + 1 if doc.size else 0))
        self.doc_len = np.zeros(max(n_docs, 1), np.int64)
        np.add.at(self.doc_len, doc, 1)
        for t in range(len(data.terms)):
            p = {}
            for i in range(int(off[t]), int(off[t + 1])):
                p.setdefault(int(doc[i]), []).append(int(pos[i]))
            self.post.append(p)
        self.total_tokens = int(doc.size)

    def phrase_freqs(self, phrase):
        """{document: frequency >= 1}: positions p of token 0 with token j at p + j for every j."""
        if any(t < 0 for t in phrase):
            return {}
        out = {}
        for d, plist in self.post[phrase[0]].items():
            f = 0
            for p in plist:
                if all(d in self.post[t] and (p + j) in self.post[t][d] for j, t in enumerate(phrase[1:], 1)):
                    f += 1
            if f:
                out[d] = f
        return out

    def idf(self, n_hit):
        v = math.log((self.n_rows - n_hit + 0.5) / (n_hit + 0.5))
        return 1e-6 if v <= 0.0 else v

    def scores(self, query):
        """{document: f64 score} of every matching document of the whole table."""
        phrases = query.phrases()
        freqs = [self.phrase_freqs(p) for p in phrases]
        idfs = [self.idf(len(f)) for f in freqs]
        if query.mode == T.NP_TEXT_AND:
            docs = set(freqs[0])
            for f in freqs[1:]:
                docs &= set(f)
        else:
            docs = set().union(*[set(f) for f in freqs])
        avgdl = float(self.total_tokens) / float(self.n_rows) if self.n_rows else 0.0
        out = {}
        for d in docs:
            D = float(self.doc_len[d])
            score = 0.0
            for f, idf in zip(freqs, idfs):
                a = float(f.get(d, 0))
                if a > 0.0:   # (a phrase that does not occur adds 0.0: the same bits)
                    score += idf * ((a * (K1 + 1.0)) / (a + K1 * (1 - B_ + B_ * D / avgdl)))
            out[d] = score
        return out

    def search(self, query, top_k, subset=None):
        """(ids int64, scores float32): f64 score descending, ties by ascending id; `subset`: only these ids."""
        return self.rank(self.scores(query), top_k, subset)

    @staticmethod
    def rank(sc, top_k, subset=None):
        """search() on the {document: f64 score} of scores(): one scoring serves several top_k and subsets."""
        if subset is not None:
            keep = set(int(x) for x in np.asarray(subset).reshape(-1))
            sc = {d: s for d, s in sc.items() if d in keep}
        order = sorted(sc, key=lambda d: (-sc[d], d))[:top_k]
        return np.asarray(order, np.int64), np.asarray([sc[d] for d in order], np.float64).astype(np.float32)


# ---- fusion (text_search.rs:1006-1075), f32 in the reference's order ------------------------------------------------------

def _order(fused, top_k):
    """fused score descending, NaN after every number, ties by ascending id."""
    ids = sorted(fused, key=lambda d: (1, 0.0, d) if math.isnan(float(fused[d])) else (0, -float(fused[d]), d))[:top_k]
    return np.asarray(ids, np.int64), np.asarray([fused[d] for d in ids], np.float32)


def fuse_rrf(sem_ids, kw_ids, alpha, top_k):
    alpha = F32(alpha)
    beta = F32(1.0) - alpha
    fused = {}
    for r, d in enumerate(sem_ids):
        fused[int(d)] = F32(0.0) + alpha / (F32(60.0) + F32(r) + F32(1.0))
    for r, d in enumerate(kw_ids):
        fused[int(d)] = fused.get(int(d), F32(0.0)) + beta / (F32(60.0) + F32(r) + F32(1.0))
    return _order(fused, top_k)


def _min_max_normalize(scores):
    s = np.asarray(scores, np.float32).reshape(-1)
    if s.size == 0:
        return s
    with np.errstate(all="ignore"):
        num = s[~np.isnan(s)]
        mn = num.min() if num.size else F32(np.inf)     # f32::min / max ignore NaN
        mx = num.max() if num.size else F32(-np.inf)
        if mx == mn:
            return np.ones(s.size, np.float32)
        return ((s - mn) / (mx - mn)).astype(np.float32)


def fuse_relative_score(sem_ids, sem_scores, kw_ids, kw_scores, alpha, top_k):
    alpha = F32(alpha)
    beta = F32(1.0) - alpha
    fused = {}
    with np.errstate(all="ignore"):
        for d, s in zip(sem_ids, _min_max_normalize(sem_scores)):
            fused[int(d)] = F32(0.0) + alpha * s
        for d, s in zip(kw_ids, _min_max_normalize(kw_scores)):
            fused[int(d)] = fused.get(int(d), F32(0.0)) + beta * s
    return _order(fused, top_k)


def fuse(mode, alpha, top_k, sem_ids, sem_scores, kw_ids, kw_scores):
    if mode == "rrf":
        return fuse_rrf(sem_ids, kw_ids, alpha, top_k)
    return fuse_relative_score(sem_ids, sem_scores, kw_ids, kw_scores, alpha, top_k)


# ---- corpora and queries the CPU and the GPU tests share -------------------------------------------------------------------

def make_texts(n_docs, vocab_size, seed, max_len=130, every=None, lens=(0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 130)):
    """n_docs documents of 0..max_len words over wo0..wo{vocab_size-1} (Zipf-like); `every` is a word put into every
    non-empty document (a term in almost all documents: the idf clamp).  Documents 0..2 have 0, 1 and max_len words, the
    others a length drawn from `lens`."""
    rng = random.Random(seed)
    words = [f"wo{i}" for i in range(vocab_size)]
    weights = [1.0 / (i + 1) for i in range(vocab_size)]
    texts = []
    for d in range(n_docs):
        n = (0, 1, max_len)[d] if d < 3 else rng.choice(lens)
        toks = rng.choices(words, weights, k=n)
        if every and toks:
            toks[rng.randrange(len(toks))] = every
        texts.append(" ".join(toks))
    return texts


def random_queries(data, n, seed, unknown=True):
    """n TextQuery objects: AND and OR of 1..5 phrases of 1..3 tokens drawn from the vocabulary (phrases mostly copied from
    adjacent term ids, so that some occur), with now and then an unknown token or a repeated phrase."""
    rng = random.Random(seed)
    nt = len(data.terms)
    out = []
    for _ in range(n):
        phrases = []
        for _ in range(rng.randint(1, 5)):
            ph = [rng.randrange(nt) for _ in range(rng.choice([1, 1, 1, 2, 2, 3]))]
            if unknown and rng.random() < 0.05:
                ph[rng.randrange(len(ph))] = -1
            phrases.append(ph)
        if rng.random() < 0.15:
            phrases.append(list(phrases[0]))
        out.append(T.TextQuery.from_phrases(phrases, rng.choice([T.NP_TEXT_AND, T.NP_TEXT_OR])))
    return out


LIMIT_WORDS = [f"lw{i:02d}" for i in range(64)]
LIMIT_BASE = 10   # documents limit_texts() puts first


def limit_texts(n):
    """n >= 16 documents for the limits of a query (NP_TEXT_MAX_PHRASES = 64 phrases, NP_TEXT_MAX_TOKENS = 256 tokens of a
    phrase).  The first LIMIT_BASE: 1 = "aa" 300 times, 2 = "aa" 5 times, 3 and 4 = "aa bb" / "bb aa" 150 times, 5 = the 64
    words of LIMIT_WORDS in order, 6 = the same reversed (every word, none of the phrases), 7 = the first 32, 8 = the 64 twice
    over, 9 = a short mix.  Then short filler documents, "aa" in every third; the last three hold copies: n - 3 = document 1,
    n - 2 = 5 then 3, n - 1 = 1 then 5 (with n = one slice + 1 these sit at the slice boundary and in the last document)."""
    words = " ".join(LIMIT_WORDS)
    rep, alt = " ".join(["aa"] * 300), " ".join(["aa bb"] * 150)
    base = ["", rep, " ".join(["aa"] * 5), alt, " ".join(["bb aa"] * 150), words, " ".join(reversed(LIMIT_WORDS)),
            " ".join(LIMIT_WORDS[:32]), words + " " + words, "aa aa bb aa aa aa bb"]
    assert len(base) == LIMIT_BASE and n >= LIMIT_BASE + 6
    fill = [f"zz fill{i % 37}" + (" aa" if i % 3 == 0 else "") for i in range(n - LIMIT_BASE - 3)]
    return base + fill + [rep, words + " " + alt, rep + " " + words]


def limit_queries(data):
    """[(name, TextQuery)] at the limits, over limit_texts(): the query shapes the CPU test pins to SQLite and the GPU test
    runs."""
    v = data.vocab
    AND, OR = T.NP_TEXT_AND, T.NP_TEXT_OR
    aa, bb = v["aa"], v["bb"]
    w = [v[x] for x in LIMIT_WORDS]
    return [("256 x aa", T.TextQuery.from_phrases([[aa] * 256], AND)),
            ("128 x aa bb", T.TextQuery.from_phrases([[aa, bb] * 128], AND)),
            ("aa aa aa", T.TextQuery.from_phrases([[aa] * 3], AND)),
            ("64 words AND", T.TextQuery.from_phrases([[x] for x in w], AND)),
            ("64 words OR", T.TextQuery.from_phrases([[x] for x in w], OR)),
            ("16 x 4 AND", T.TextQuery.from_phrases([w[4 * i: 4 * i + 4] for i in range(16)], AND)),
            ("63 words and an unknown AND", T.TextQuery.from_phrases([[x] for x in w[:40]] + [[-1]] + [[x] for x in w[40:63]], AND)),
            ("63 unknown OR aa", T.TextQuery.from_phrases([[-1]] * 63 + [[aa]], OR))]


def match_string(query, data):
    """The FTS5 MATCH text of a TextQuery whose tokens are plain words (an unknown token becomes a word no document has)."""
    ph = ['"' + " ".join(data.terms[t] if t >= 0 else "zzzunknown" for t in p) + '"' for p in query.phrases()]
    return (" AND " if query.mode == T.NP_TEXT_AND else " OR ").join(ph)
