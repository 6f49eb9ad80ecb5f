"""The cases of tests/test_expand_limits_cpu.py and tests/test_gpu_expand_limits.py: np_hip_index_expand at the edges of
ivf_keep_kernel, ivf_cut_offsets_kernel and ivf_cut_merge_kernel (a tile of 4096 entries, a quad of 4 per thread, a cut inside
every old list), of widen_codes_kernel (8 codes per lane, a tail of n % 8, a grid capped at 8192 blocks) and of the token
stages that now start at a cut inside the old tokens (test infrastructure; numpy and next_plaid_amd.synth only).

A case is a base index, the new centroids, the given documents, n_replace and one line that names the edge it is for.  Every
premise is asserted by the CPU test from expand_restate's census or rules, so that a generator change cannot move a case off
its edge.  Unless a case says otherwise: dim 32, nbits 4, K0 = 256.
"""
from dataclasses import dataclass, field

import numpy as np

import append_restate as A
import expand_restate as E
from append_limit_shapes import DIM, RAW_CODES, docs, entries, index_of, rand_docs, short_base, with_entries
from helpers import synth

HOT = 7
WIDE_K0, WIDE_K1 = 65530, 65542
WIDE_NBITS = 2
WIDE_PD = DIM * WIDE_NBITS // 8
BIG_TK = 8 * (E.WIDEN_MAX_BLOCKS * 256 + 1) + 5       # the stride loop's second turn, and a tail of 5


@dataclass
class Case:
    name: str
    edge: str                      # the edge the case is for
    base: dict
    new_centroids: np.ndarray
    given: tuple                   # (doc_lengths, codes, residuals)
    n_replace: int
    reserve: tuple = None          # (extra documents, extra tokens) reserved before the expand
    then: tuple = None             # a second expand on the result: (new_centroids, given, n_replace)
    remove_all: bool = False       # every document is removed (remove_ids) before the expand
    env: dict = None               # environment of the open (NP_TOK_SORT)
    states_codes: bool = True      # the expanded lists are exactly the (document, distinct code) pairs of the final codes
    level: object = None           # True: the zeroth level must run afterwards; False: it must stay off; None: not asserted
    decompress_all: bool = False   # every given document's rows against float64
    merge: bool = True             # a case of the cut and merge geometry: the CPU test routes it
    widen: bool = False            # the codes widen: the CPU test routes the kept codes through widen_route
    notes: dict = field(default_factory=dict)

    @property
    def start(self):
        """the index the expand meets"""
        if not self.remove_all:
            return self.base
        b = self.base
        return dict(b, doc_lengths=np.zeros(0, np.int64), codes=np.zeros(0, np.int64), residuals=b["residuals"][:0],
                    ivf=np.zeros(0, np.int64), ivf_lengths=np.zeros(b["centroids"].shape[0], np.int32))

    @property
    def K0(self):
        return int(self.base["centroids"].shape[0])

    @property
    def K1(self):
        return self.K0 + int(self.new_centroids.shape[0])

    @property
    def N0(self):
        return int(self.start["doc_lengths"].size)

    @property
    def Nk(self):
        return self.N0 - self.n_replace

    @property
    def T0(self):
        return int(self.start["doc_lengths"].sum())

    @property
    def Tk(self):
        return int(self.start["doc_lengths"][:self.Nk].sum())

    @property
    def T1(self):
        return self.Tk + int(np.sum(self.given[0]))

    @property
    def N1(self):
        return self.Nk + len(self.given[0])

    def pairs(self):
        return E.given_pairs(self.Nk, self.given)

    def final(self):
        return E.expanded_arrays(self.start, self.new_centroids, self.given, self.n_replace)

    def final2(self):
        return E.expanded_arrays(self.final(), *self.then)

    def arith(self):
        """the arguments of expand_restate's expected_* functions"""
        s = self.start
        return s["ivf"], A.offsets(s["ivf_lengths"]), self.K0, self.K1, self.Nk, self.pairs()[0]


def new_centroids(rng, k, dim=DIM):
    c = rng.standard_normal((k, dim)).astype(np.float32)
    return np.ascontiguousarray(c / np.linalg.norm(c, axis=1, keepdims=True), np.float32).reshape(k, dim)


# ---- cut and merge geometry ------------------------------------------------------------------------------------------------------
def hot_list():
    """9000 documents that all hold code 7, the last 3000 replaced, 6500 given that hold 7 (0-2 further codes above it each):
    list 7 is the array's first list, its kept part [0, 6000) holds tile 0 whole and tile 1 from inside, its new part
    [6000, 12500) holds tile 2 whole, and the 3000 dropped entries lie directly behind the kept ones in the old array"""
    rng = np.random.default_rng(8001)

    def make(n, K):
        lens = 1 + rng.integers(0, 3, n)
        codes = rng.integers(HOT + 1, K, int(lens.sum()))
        codes[A.offsets(lens)[:-1]] = HOT
        return lens, codes
    base = index_of(256, *make(9000, 256), rng)
    return Case("hot list cut across tiles", "list 7's kept part and its new part are each longer than a tile; 3000 dropped entries behind the cut",
                base, new_centroids(rng, 4), docs(rng, *make(6500, 260)), 3000)


def residues():
    rng = np.random.default_rng(8002)
    base = short_base(rng, 300)
    n_replace = 20
    kept = int(np.sum(base["ivf"] < 300 - n_replace))
    n0 = (-kept) % 4096
    n0 += 4096 if n0 < n_replace else 0
    cen = new_centroids(rng, 3)
    out = []
    for extra, what in ((0, "a multiple of 4096: the last tile is whole"), (1, "a multiple of 4096 plus 1: a tile of one entry"),
                        (2, "2 mod 4: a partial last quad of 2"), (3, "3 mod 4: a partial last quad of 3")):
        n = n0 + extra
        out.append(Case(f"residue total = {kept + n}", f"total is {what}", base, cen, rand_docs(rng, np.ones(n, np.int64), 259),
                        n_replace, notes=dict(residue=extra)))
    two = index_of(256, [1, 1], [9, 10], rng)
    out.append(Case("residue total = 2", "total < 4: the grid is a single partial quad", two, cen, docs(rng, [1], [257]), 1,
                    notes=dict(residue=2)))
    return out


def cut_alignments():
    """600 documents of 1-24 tokens, the last 80 replaced: the dropped entries in front of a list shift its kept part by any
    number of entries against the old array, so the 16-byte loads of the fast path start at every alignment"""
    rng = np.random.default_rng(8003)
    base = short_base(rng, 600)
    cen = new_centroids(rng, 6)
    given = rand_docs(rng, rng.integers(1, 25, 95), 262)
    then = (new_centroids(rng, 2), rand_docs(rng, rng.integers(1, 25, 30), 264), 25)
    return Case("cut alignments", "kept prefixes at all four shifts mod 4 on the fast path; quads that end at a cut and one past it",
                base, cen, given, 80, then=then)


def lists_cut_to_nothing():
    """K0 = 1024.  List 8 holds 4096 kept single-token documents and nothing new, so it is entries [0, 4096).  The lists of
    `run` are held by replaced documents alone and the given documents avoid them.  With the run at lists 9 .. 19, list 20
    (always kept and given to) begins at entry 4096: a tile whose first entry is a list's first entry behind eleven lists cut
    to nothing.  With the run at 1010 .. 1023 the last old lists and the new lists 1024 .. 1028 are all empty."""
    out = []
    for name, run, used in (("lists cut to nothing", np.arange(9, 20), (20, 1024)),
                            ("lists cut to nothing at the end", np.arange(1010, 1024), (9, 1010))):
        rng = np.random.default_rng(8004 + run[0])
        K0 = 1024
        mid = rng.integers(1, 4, 200)
        mid_codes = rng.integers(used[0], used[1], int(mid.sum()))
        mid_codes[0] = used[0]                                    # the list behind list 8 keeps an entry
        tail_run = np.repeat(run, 2)                              # two replaced single-token documents per list of the run
        tail_more = rng.integers(1, 4, 30)
        lens = np.concatenate([np.ones(4096, np.int64), mid, np.ones(tail_run.size, np.int64), tail_more])
        codes = np.concatenate([np.full(4096, 8), mid_codes, tail_run, rng.integers(used[0], used[1], int(tail_more.sum()))])
        base = index_of(K0, lens, codes, rng)
        n_replace = tail_run.size + tail_more.size
        gl = rng.integers(1, 4, n_replace + 15)
        gc = rng.integers(used[0], used[1] if run[0] > 1000 else K0 + 5, int(gl.sum()))
        gc[0] = used[0]
        out.append(Case(name, f"lists {run[0]} .. {run[-1]} keep nothing and gain nothing", base, new_centroids(rng, 5), docs(rng, gl, gc),
                        n_replace, notes=dict(run=(int(run[0]), int(run[-1])))))
    return out


def new_lists():
    out = []
    for K0, K1 in ((250, 255), (250, 256), (250, 257), (256, 257)):
        rng = np.random.default_rng(8100 + K1 + K0)
        base = short_base(rng, 300, K=K0)
        out.append(Case(f"every given pair to list K1 - 1, K {K0} -> {K1}",
                        f"ivf_keep_kernel writes {K1 + 1} entries: {(K1 + 256) // 256} block(s), {K1 + 1 - (K1 + 256) // 256 * 256 + 256} thread(s) of the last",
                        base, new_centroids(rng, K1 - K0), docs(rng, np.ones(37, np.int64), np.full(37, K1 - 1)), 10))
    rng = np.random.default_rng(8105)
    K0, K1 = 65590, 65600
    lens = np.concatenate([np.zeros(5, np.int64), rng.integers(1, 4, 50)])
    far = index_of(K0, lens, np.full(int(lens.sum()), K0 - 1), rng)
    gl = rng.integers(1, 4, 59)
    out.append(Case("only list K1 - 1 is used, K1 = 65600", "the tile's first list is 16 doublings from list 0; u32 codes before and after",
                    far, new_centroids(rng, K1 - K0), docs(rng, gl, np.full(int(gl.sum()), K1 - 1)), 50))
    return out


# (list, its document ids): N0 = 40, Nk = 30
CLASS_LISTS = {3: [0, 5, 12], 4: [30, 33], 5: [1, 8, 31, 35], 6: [2, 29, 30, 39], 7: [4], 8: [36], 10: [3, 6, 7, 9, 10, 11, 13, 14, 15, 37]}
CLASS_OF = {3: "keeps all", 4: "keeps none", 5: "cut inside", 6: "cut inside", 7: "keeps all", 8: "keeps none", 9: "empty", 10: "cut inside"}


def bisection_classes():
    rng = np.random.default_rng(8006)
    N0 = 40
    held = [[] for _ in range(N0)]
    for c, ids in sorted(CLASS_LISTS.items()):
        for d in ids:
            held[d].append(c)
    lens = np.array([len(h) for h in held], np.int64)
    base = index_of(256, lens, np.array([c for h in held for c in h], np.int64), rng)
    every = Case("every bisection class", "lists that keep all, none, are cut inside, are cut between Nk - 1 and Nk, hold one entry, are empty",
                 base, new_centroids(rng, 4), rand_docs(rng, rng.integers(0, 6, 12), 260), 10)
    b2 = short_base(rng, 300)
    none = Case("nothing replaced, new centroids", "n_replace = 0: Nk = N0 lies past every id, every list keeps all", b2, new_centroids(rng, 4),
                rand_docs(rng, rng.integers(1, 25, 20), 260), 0)
    return [every, none]


def raw_list():
    rng = np.random.default_rng(8007)
    base = short_base(rng, 300)
    raw_codes = RAW_CODES + (258,)
    long_codes = rng.choice(raw_codes, 4500)
    n_short = 2300
    short = np.stack([rng.integers(0, 128, n_short), rng.integers(128, 260, n_short)], 1).reshape(-1)
    lens = np.concatenate([[4500], np.full(n_short, 2)])
    return Case("raw list through the cut", "a given document past NP_UNIQ_MAX lists every token: Unique shrinks P, its entries lie in two tiles",
                base, new_centroids(rng, 4), docs(rng, lens, np.concatenate([long_codes, short])), 10, notes=dict(raw_codes=raw_codes))


def inexact_lists():
    """the append's two constructions, the odd pair once on a kept and once on a replaced document (300 documents, 40 replaced)"""
    rng = np.random.default_rng(8008)
    base = short_base(rng, 300)
    n_replace, Nk = 40, 260
    c, d = entries(base)
    cen = new_centroids(rng, 4)
    given = rand_docs(rng, rng.integers(1, 25, 55), 260)
    out = []
    for where, pool in (("kept", np.arange(0, Nk)), ("replaced", np.arange(Nk, 300))):
        victim = int(pool[np.argmax(base["doc_lengths"][pool])])
        drop = np.nonzero(d == victim)[0][1]
        missing = with_entries(base, np.delete(c, drop), np.delete(d, drop))
        kept = where == "kept"
        out.append(Case(f"lists that miss a pair of a {where} document",
                        "ivf_cover = 0 and the pair stays missing: the level stays off" if kept else
                        "ivf_cover = 0, but the expanded lists state every pair again: the coverage is looked at again",
                        missing, cen, given, n_replace, states_codes=not kept, level=not kept, notes=dict(victim=victim)))
        have = set((c * 300 + d).tolist())
        add = sorted({(cc, dd) for cc, dd in zip(rng.integers(0, 256, 400).tolist(), rng.choice(pool, 400).tolist())
                      if cc * 300 + dd not in have})
        extra = with_entries(base, np.append(c, [x for x, _ in add]), np.append(d, [y for _, y in add]))
        out.append(Case(f"lists with extra pairs of {where} documents",
                        "ivf_cover = 1; the extra entries stay" if kept else "ivf_cover = 1; the extra entries are cut away",
                        extra, cen, given, n_replace, states_codes=not kept, level=True, notes=dict(n_extra=len(add))))
    return out


def empty_sides():
    rng = np.random.default_rng(8009)
    cen = new_centroids(rng, 4)
    empty5 = index_of(256, np.zeros(5, np.int64), np.zeros(0, np.int64), rng)
    a = Case("all-empty base", "ivf_size = 0 and T = 0 before the expand: every entry of the new array is a pair", empty5, cen,
             rand_docs(rng, [5, 0, 12, 3], 260), 2, decompress_all=True)
    b = Case("emptied handle", "every document removed first: N0 = 0, n_replace = 0, lists of length 0 everywhere", short_base(rng, 50), cen,
             rand_docs(rng, [7, 0, 9, 2, 1], 260), 0, remove_all=True, decompress_all=True)
    small = short_base(rng, 30)
    c = Case("everything replaced by empty documents", "P = 0, total = 0, Tk = 0: no merge launch, an index without a token", small, cen,
             docs(rng, np.zeros(30, np.int64), np.zeros(0, np.int64)), 30, decompress_all=True)
    lens = np.concatenate([rng.integers(1, 25, 100), np.zeros(6, np.int64)])
    tail = index_of(256, lens, rng.integers(0, 256, int(lens.sum())), rng)
    d = Case("a replaced tail of empty documents", "Tk = T0: doc offsets are saved, tokens are not", tail, cen,
             rand_docs(rng, [3, 0, 8, 1, 1, 2, 6, 4], 260), 6, decompress_all=True)
    return [a, b, c, d]


# ---- widening ------------------------------------------------------------------------------------------------------------------------
_WIDE_CODEC = {}


def wide_index(K, lens, codes, rng):
    lens, codes = np.asarray(lens, np.int64), np.asarray(codes, np.int64)
    if K not in _WIDE_CODEC:
        spec = synth.SynthSpec(num_docs=1, num_centroids=K, dim=DIM, nbits=WIDE_NBITS, seed=4200 + K % 97)
        _WIDE_CODEC[K] = (synth.centroids(spec), synth.bucket_tables(spec)[1])
    cen, wts = _WIDE_CODEC[K]
    ivf, il = synth.build_ivf(codes, lens, K)
    return dict(nbits=WIDE_NBITS, centroids=cen, bucket_weights=wts, ivf=ivf, ivf_lengths=il, doc_lengths=lens, codes=codes,
                residuals=rng.integers(0, 256, (codes.size, WIDE_PD)).astype(np.uint8))


def wide_docs(rng, lens, lo, hi):
    lens = np.asarray(lens, np.int64)
    T = int(lens.sum())
    return lens, rng.integers(lo, hi, T).astype(np.int64), rng.integers(0, 256, (T, WIDE_PD)).astype(np.uint8)


def _widen_case(name, edge, Tk, seed, n_tail=3, **kw):
    """short documents whose kept tokens number exactly Tk (the last kept document's length is what fixes it), K 65530 -> 65542;
    the kept codes hold 0 and 65529 in the last group of 8 and in the tail"""
    rng = np.random.default_rng(seed)
    lens = []
    while Tk - sum(lens) > 12:
        lens.append(int(rng.integers(1, 13)))
    if Tk - sum(lens) > 0:
        lens.append(Tk - sum(lens))
    n_keep = len(lens)
    lens += rng.integers(1, 13, n_tail).tolist()
    T = sum(lens)
    codes = rng.integers(0, WIDE_K0, T)
    codes[::7] = WIDE_K0 - 1
    codes[3::11] = 0
    n8 = Tk >> 3
    if n8:
        codes[8 * n8 - 8], codes[8 * n8 - 1], codes[8 * n8 - 5] = 0, WIDE_K0 - 1, WIDE_K0 - 1
        codes[8 * n8 - 4] = 0
    edge_codes = [WIDE_K0 - 1, 0]
    for j, t in enumerate(range(8 * n8, Tk)):
        codes[t] = edge_codes[j % 2]
    base = wide_index(WIDE_K0, lens, codes, rng)
    gl = rng.integers(1, 13, n_tail + 11)
    given = wide_docs(rng, gl, 65000, WIDE_K1)
    given[1][::3] = WIDE_K1 - 1
    given[1][1::3] = 65536
    given[1][2::5] = 65535
    return Case(name, edge, base, new_centroids(rng, WIDE_K1 - WIDE_K0), given, n_tail if "n_replace" not in kw else kw.pop("n_replace"),
                merge=False, widen=True, notes=dict(Tk=Tk, n_keep=n_keep), **kw)


def widening():
    out = [_widen_case(f"widen Tk = {2104 + r}", f"Tk % 8 = {r}: two blocks of groups, a tail of {r}", 2104 + r, 8200 + r) for r in range(8)]
    out.append(_widen_case("widen Tk = 7", "no group of 8: the grid's minimum of one block, seven tail codes", 7, 8210))
    out.append(_widen_case("widen Tk = 8", "one group of 8 and no tail", 8, 8211))
    rng = np.random.default_rng(8212)
    lens = rng.integers(1, 13, 40)
    base = wide_index(WIDE_K0, lens, rng.integers(0, WIDE_K0, int(lens.sum())), rng)
    given = wide_docs(rng, rng.integers(1, 13, 44), 65000, WIDE_K1)
    given[1][::3] = WIDE_K1 - 1
    out.append(Case("widen Tk = 0", "every document replaced while the codes widen: nothing to convert", base,
                    new_centroids(rng, WIDE_K1 - WIDE_K0), given, 40, merge=False, widen=True, notes=dict(Tk=0, n_keep=0)))
    out.append(_widen_case("widen in the code-ordered token layout", "NP_TOK_SORT = 1, Tk % 8 = 3", 2107, 8213, env=dict(NP_TOK_SORT="1")))
    out.append(_widen_case("widen inside a reservation", "the wide array has room for cap_tokens entries, Tk % 8 = 5", 2109, 8214,
                           reserve=(50, 600)))
    return out


def big_widen_codes():
    """the kept codes of the large case alone (the CPU premise needs no index): BIG_TK u16 codes"""
    rng = np.random.default_rng(8215)
    codes = rng.integers(0, WIDE_K0, BIG_TK).astype(np.uint16)
    codes[-1], codes[-2], codes[-6], codes[-7] = 0, WIDE_K0 - 1, 0, WIDE_K0 - 1
    return codes


def big_widen():
    """Tk = 8 * (8192 * 256 + 1) + 5 tokens in 4096 documents of 4096 tokens and one of 13, each document on 8 codes (so the
    posting lists stay small), then three short documents that are replaced.  Built only where it is used: it takes seconds"""
    rng = np.random.default_rng(8216)
    n_full, rest = divmod(BIG_TK, 4096)
    lens = np.concatenate([np.full(n_full, 4096), [rest] if rest else [], [3, 5, 2]]).astype(np.int64)
    own = rng.integers(0, WIDE_K0, (lens.size, 8))
    own[:, 0], own[:, 1] = 0, WIDE_K0 - 1
    doc = A.doc_of_token(lens)
    codes = own[doc, rng.integers(0, 8, doc.size)]
    base = wide_index(WIDE_K0, lens, codes, rng)
    given = wide_docs(rng, rng.integers(1, 13, 9), 65000, WIDE_K1)
    given[1][::3] = WIDE_K1 - 1
    return Case("widen across the stride loop's second turn", f"Tk = {BIG_TK}: thread 0 takes a second turn, a tail of 5", base,
                new_centroids(rng, WIDE_K1 - WIDE_K0), given, 3, merge=False, widen=True, notes=dict(Tk=BIG_TK))


# ---- inverse norms and capacity ----------------------------------------------------------------------------------------------------
def inverse_norms():
    out = []
    for rem in (0, 1, 63):
        for n_tok in (1, 64, 65):
            rng = np.random.default_rng(8300 + rem + n_tok)
            lens = rng.integers(1, 25, 21)
            lens[-2] += (rem - int(lens[:-1].sum())) % 64          # the kept tokens; the last document is replaced
            base = index_of(256, lens, rng.integers(0, 256, int(lens.sum())), rng)
            out.append(Case(f"inverse norms {rem} mod 64 + {n_tok}", f"fill_inv_norm(Tk, T1) with Tk = {int(lens[:-1].sum())} and {n_tok} given tokens",
                            base, new_centroids(rng, 4), rand_docs(rng, [n_tok], 260, lo=256), 1, decompress_all=True, merge=False,
                            notes=dict(rem=rem, n_tok=n_tok)))
    return out


CAP_TAIL = (3, 4)          # the two replaced documents' lengths
CAP_GIVEN = (9, 30, 4, 11)


def capacity():
    """the append's four capacity cases with two documents replaced: 4 (5) given documents of 54 (55) tokens need 2 (3) more
    documents and 47 (48) more tokens than the handle holds"""
    rng = np.random.default_rng(8010)
    lens = np.concatenate([rng.integers(1, 25, 198), CAP_TAIL])
    base = index_of(256, lens, rng.integers(0, 256, int(lens.sum())), rng)
    need_t = sum(CAP_GIVEN) - sum(CAP_TAIL)
    out = []
    for name, nl, reserve in (("documents reserved, tokens not", CAP_GIVEN, (2, 10)),
                              ("tokens reserved, documents not", CAP_GIVEN, (1, need_t)),
                              ("the reservation filled exactly", CAP_GIVEN, (2, need_t)),
                              ("one document and one token beyond", CAP_GIVEN + (1,), (2, need_t))):
        out.append(Case(f"capacity: {name}", f"reserve{reserve}, 2 documents replaced, {len(nl)} given of {sum(nl)} tokens", base,
                        new_centroids(rng, 4), rand_docs(rng, list(nl), 260), 2, reserve=reserve, decompress_all=True, merge=False))
    lens = np.concatenate([rng.integers(1, 25, 100), [20, 24, 17]])
    shrink = index_of(256, lens, rng.integers(0, 256, int(lens.sum())), rng)
    out.append(Case("fewer tokens than before", "the given tokens are fewer than the replaced ones: T1 < T0, the capacity stays", shrink,
                    new_centroids(rng, 4), rand_docs(rng, [1, 1, 1], 260, lo=250), 3, decompress_all=True, merge=False))
    return out


def capacity_after(case):
    """grow_capacity: documents and tokens apart, each to exactly what is needed when what is allocated does not hold it"""
    rd, rt = case.reserve or (0, 0)
    return max(case.N0 + rd, case.N1), max(case.T0 + rt, case.T1)


def merge_cases():
    return ([hot_list()] + residues() + [cut_alignments()] + lists_cut_to_nothing() + new_lists() + bisection_classes() + [raw_list()]
            + inexact_lists() + empty_sides())


def layout_cases():
    return widening() + inverse_norms() + capacity()


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = merge_cases() + layout_cases()
        assert len({c.name for c in _ALL}) == len(_ALL)
    return _ALL


def case(name):
    return next(c for c in all_cases() if c.name == name)
