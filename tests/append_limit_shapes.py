"""The cases of tests/test_append_limits_cpu.py and tests/test_gpu_append_limits.py: np_hip_index_append at the edges of
ivf_cut_merge_kernel (a tile of 4096 entries, a quad of 4 per thread) and of the layouts it rebuilds (test infrastructure; numpy
and next_plaid_amd.synth only).

A case is a base index, the documents appended to it in one or more calls, and one line that names the edge it is for.  Every
premise is asserted by the CPU test from append_restate's census or rules, so that a generator change cannot move a case off
its edge.  Unless a case says otherwise: dim 32, nbits 4, K = 256.
"""
from dataclasses import dataclass, field

import numpy as np

import append_restate as A
from helpers import synth

DIM, NBITS = 32, 4
PD = DIM * NBITS // 8
_CODEC = {}


@dataclass
class Case:
    name: str
    edge: str                      # the edge the case is for
    base: dict
    steps: list                    # [(doc_lengths, codes, residuals)] one per append call
    reserve: tuple = None          # (extra documents, extra tokens) reserved before the first call
    states_codes: bool = True      # the base's lists are exactly the (document, distinct code) pairs
    level: object = None           # True: the zeroth level must run on the grown index; False: it must stay off; None: not asserted
    decompress_all: bool = False   # every new document's rows against float64
    merge: bool = True             # a case of the merge geometry: the CPU test routes it
    notes: dict = field(default_factory=dict)

    @property
    def K(self):
        return int(self.base["centroids"].shape[0])

    @property
    def n_old(self):
        return int(self.base["doc_lengths"].size)

    @property
    def new(self):
        return A.concat_new(self.steps, PD)

    def grown(self):
        return A.grown_arrays(self.base, self.new)

    def pairs(self, unique=True):
        return A.new_pairs(self.n_old, self.new, unique)


def _codec(K):
    if K not in _CODEC:
        spec = synth.SynthSpec(num_docs=1, num_centroids=K, dim=DIM, nbits=NBITS, seed=4100 + K % 97)
        _CODEC[K] = (synth.centroids(spec), synth.bucket_tables(spec)[1])
    return _CODEC[K]


def _residuals(rng, T):
    return rng.integers(0, 256, (int(T), PD)).astype(np.uint8)


def docs(rng, lens, codes):
    lens, codes = np.asarray(lens, np.int64), np.asarray(codes, np.int64)
    assert codes.size == lens.sum()
    return lens, codes, _residuals(rng, codes.size)


def index_of(K, lens, codes, rng):
    """an index whose lists state the codes (index.rs:479-499)"""
    lens, codes = np.asarray(lens, np.int64), np.asarray(codes, np.int64)
    cen, wts = _codec(K)
    ivf, il = synth.build_ivf(codes, lens, K)
    return dict(nbits=NBITS, centroids=cen, bucket_weights=wts, ivf=ivf, ivf_lengths=il, doc_lengths=lens, codes=codes,
                residuals=_residuals(rng, codes.size))


def rand_docs(rng, lens, K, lo=0, hi=None):
    lens = np.asarray(lens, np.int64)
    return docs(rng, lens, rng.integers(lo, K if hi is None else hi, int(lens.sum())))


def short_base(rng, n, K=256, lo=1, hi=24):
    lens = rng.integers(lo, hi + 1, n)
    return index_of(K, lens, rng.integers(0, K, int(lens.sum())), rng)


def with_entries(a, cells, ids):
    """a copy of `a` whose lists hold exactly the given (cell, document) entries, ascending"""
    cells, ids = np.asarray(cells, np.int64), np.asarray(ids, np.int64)
    o = np.lexsort((ids, cells))
    return dict(a, ivf=np.ascontiguousarray(ids[o]), ivf_lengths=np.bincount(cells, minlength=a["centroids"].shape[0]).astype(np.int32))


def entries(a):
    il = np.asarray(a["ivf_lengths"], np.int64)
    return np.repeat(np.arange(il.size, dtype=np.int64), il), np.asarray(a["ivf"], np.int64)


# ---- merge geometry ----------------------------------------------------------------------------------------------------
HOT = 7


def hot_list():
    """6000 + 6500 documents that all hold code 7, with 0-2 further codes above it: list 7 is the array's first list, its old
    part is entries [0, 6000) -- tile 0 whole, tile 1 from inside it -- and its new part [6000, 12500) holds tile 2 whole
    (a new part must be at least 2 * 4096 - 6000 % 4096 = 6288 entries long to hold a whole tile wherever it starts here)."""
    rng = np.random.default_rng(7001)

    def make(n):
        extra = rng.integers(0, 3, n)
        lens = 1 + extra
        codes = rng.integers(HOT + 1, 256, int(lens.sum()))
        codes[A.offsets(lens)[:-1]] = HOT          # every document's first token
        return lens, codes
    base = index_of(256, *make(6000), rng)
    return Case("hot list across tiles", "list 7's old part and its new part are each longer than a tile: tiles start inside both",
                base, [docs(rng, *make(6500))])


def residues():
    rng = np.random.default_rng(7002)
    base = short_base(rng, 300)
    e0 = int(base["ivf"].size)
    n0 = (-e0) % 4096
    out = []
    for extra, what in ((0, "a multiple of 4096: the last tile is whole"), (1, "a multiple of 4096 plus 1: a tile of one entry"),
                        (2, "2 mod 4: a partial last quad of 2"), (3, "3 mod 4: a partial last quad of 3")):
        n = n0 + extra
        out.append(Case(f"residue total = {e0 + n}", f"total is {what}", base, [rand_docs(rng, np.ones(n, np.int64), 256)],
                        notes=dict(residue=extra)))
    one = index_of(256, [1], [9], rng)
    out.append(Case("residue total = 2", "total < 4: the grid is a single partial quad", one, [docs(rng, [1], [200])], notes=dict(residue=2)))
    return out


def sparse_lists():
    """K = 1024, codes on multiples of 8.  The base gives every used list c >= 16 one document; new document j holds used
    list 2j (every fifth one the list behind it too), so the array reads old(c), new(c), old(c + 8), old(c + 16), ... across
    seven empty lists each time.  List 8 holds 4096 single-token documents and nothing new, so list 16 starts exactly at entry
    4096: a tile whose first entry is a list's first entry behind empty lists."""
    rng = np.random.default_rng(7003)
    K = 1024
    used = np.arange(16, K, 8)
    lens = [1] * used.size + [1] * 4096
    codes = used.tolist() + [8] * 4096
    new_lens, new_codes = [], []
    for j in range(50):
        mine = [used[2 * j], used[2 * j + 1]] if j % 5 == 4 else [used[2 * j]]
        new_lens.append(len(mine))
        new_codes += mine
    base = index_of(K, lens, codes, rng)
    return Case("sparse lists", "quads span three lists with empty lists between them; a tile begins at a list's first entry",
                base, [docs(rng, new_lens, new_codes)])


def first_and_last_list():
    rng = np.random.default_rng(7004)
    base = short_base(rng, 300)
    first = Case("every new pair to list 0", "the gain is all in front: every old entry moves by the same shift", base,
                 [docs(rng, np.ones(37, np.int64), np.zeros(37, np.int64))])
    b257 = short_base(rng, 300, K=257)
    last = Case("every new pair to list K - 1, K = 257", "kbits = 9 for one list past 256; the new entries are the array's tail",
                b257, [docs(rng, np.ones(37, np.int64), np.full(37, 256))])
    K = 65600
    lens = rng.integers(1, 4, 50)
    far = index_of(K, lens, np.full(int(lens.sum()), K - 1), rng)
    nl = rng.integers(1, 4, 9)
    gallop = Case("only list K - 1 is used, K = 65600", "the tile's first list is 16 doublings from list 0; u32 codes", far,
                  [docs(rng, nl, np.full(int(nl.sum()), K - 1))])
    return [first, last, gallop]


RAW_CODES = (3, 60, 120, 180, 250)


def raw_list():
    rng = np.random.default_rng(7005)
    base = short_base(rng, 300)
    long_codes = rng.choice(RAW_CODES, 4500)
    n_short = 2300
    short = np.stack([rng.integers(0, 128, n_short), rng.integers(128, 256, n_short)], 1).reshape(-1)   # two distinct codes each
    lens = np.concatenate([[4500], np.full(n_short, 2)])
    return Case("raw list over a tile edge", "a document past NP_UNIQ_MAX lists every token: Unique shrinks P, its entries lie in two tiles",
                base, [docs(rng, lens, np.concatenate([long_codes, short]))])


def inexact_lists():
    rng = np.random.default_rng(7006)
    base = short_base(rng, 300)
    c, d = entries(base)
    victim = int(np.argmax(base["doc_lengths"]))
    drop = np.nonzero(d == victim)[0][1]
    missing = with_entries(base, np.delete(c, drop), np.delete(d, drop))
    new = rand_docs(rng, rng.integers(1, 25, 20), 256)
    have = set((c * 300 + d).tolist())
    add = [(cc, dd) for cc, dd in zip(rng.integers(0, 256, 400).tolist(), rng.integers(0, 300, 400).tolist()) if cc * 300 + dd not in have]
    add = sorted(set(add))
    extra = with_entries(base, np.append(c, [x for x, _ in add]), np.append(d, [y for _, y in add]))
    return [Case("lists that miss a pair", "ivf_cover = 0: the coverage is looked at again and the level stays off", missing, [new],
                 states_codes=False, level=False, notes=dict(victim=victim)),
            Case("lists with extra pairs", "ivf_cover = 1 with entries the codes do not state: the re-check is skipped, the level runs",
                 extra, [new], states_codes=False, level=True, notes=dict(n_extra=len(add)))]


# ---- rebuilt layout ----------------------------------------------------------------------------------------------------
LONG_ULEN = (150, 150, 150, 150, 149, 147, 146, 145, 143, 141)   # distinct codes of the ten 200-token documents


def long_docs(rng, K=256):
    codes = []
    for u in LONG_ULEN:
        own = rng.choice(K, u, replace=False)
        codes.append(rng.permutation(np.concatenate([own, rng.choice(own, 200 - u)])))
    return docs(rng, np.full(len(LONG_ULEN), 200), np.concatenate(codes))


def strides():
    rng = np.random.default_rng(7007)
    base = short_base(rng, 300)
    long = long_docs(rng)
    grows = Case("stride grows", "ten 200-token documents take the block stride from 64 to 320 bytes: every block moves", base, [long],
                 merge=False, notes=dict(strides=(64, 320)))
    grown = A.grown_arrays(base, long)
    shrinks = Case("stride shrinks", "800 short documents take it from 320 back to 64 bytes: ten lists move to the overflow region",
                   grown, [rand_docs(rng, rng.integers(1, 25, 800), 256)], merge=False, notes=dict(strides=(320, 64)))
    K = 65600
    wbase = short_base(rng, 400, K=K)
    wl = np.full(10, 100)
    wide = Case("wide codes", "u32 codes: ten 100-token documents take the stride from 128 to 448 bytes", wbase,
                [rand_docs(rng, wl, K)], merge=False, notes=dict(strides=(128, 448)))
    return [grows, shrinks, wide]


def range_table():
    out = []
    for n_old, n_new in ((32767, 1), (32768, 1), (32767, 2)):
        rng = np.random.default_rng(7100 + n_old + n_new)
        base = short_base(rng, n_old, hi=3)
        out.append(Case(f"range table {n_old} + {n_new}", f"{A.n_ranges(n_old)} range(s) of 32768 documents become {A.n_ranges(n_old + n_new)}",
                        base, [rand_docs(rng, rng.integers(1, 4, n_new), 256)], level=True, merge=False,
                        notes=dict(ranges=(A.n_ranges(n_old), A.n_ranges(n_old + n_new)))))
    return out


def capacity():
    rng = np.random.default_rng(7008)
    base = short_base(rng, 200)
    out = []
    for name, nl, reserve in (("documents reserved, tokens not", [9, 30, 4, 11], (4, 10)),
                              ("tokens reserved, documents not", [9, 30, 4, 11], (2, 54)),
                              ("the reservation filled exactly", [9, 30, 4, 11], (4, 54)),
                              ("one document and one token beyond", [9, 30, 4, 11, 1], (4, 54))):
        out.append(Case(f"capacity: {name}", f"reserve{reserve} then {len(nl)} documents of {sum(nl)} tokens", base,
                        [rand_docs(rng, nl, 256)], reserve=reserve, decompress_all=True, merge=False))
    return out


def capacity_after(case):
    """grow_capacity: documents and tokens apart, each to exactly what is needed when the reservation does not hold it"""
    n0, t0 = case.n_old, int(case.base["doc_lengths"].sum())
    lens = case.new[0]
    return max(n0 + case.reserve[0], n0 + lens.size), max(t0 + case.reserve[1], t0 + int(lens.sum()))


def inverse_norms():
    out = []
    for rem in (0, 63):
        for n_tok in (1, 64, 65):
            rng = np.random.default_rng(7200 + rem + n_tok)
            lens = rng.integers(1, 25, 20)
            lens[-1] += (rem - int(lens.sum())) % 64
            base = index_of(256, lens, rng.integers(0, 256, int(lens.sum())), rng)
            out.append(Case(f"inverse norms {rem} mod 64 + {n_tok}", f"fill_inv_norm(T0, T1) with T0 = {int(lens.sum())} and {n_tok} new tokens",
                            base, [rand_docs(rng, [n_tok], 256)], decompress_all=True, merge=False, notes=dict(rem=rem, n_tok=n_tok)))
    return out


def empty_base():
    rng = np.random.default_rng(7009)
    base = index_of(256, np.zeros(5, np.int64), np.zeros(0, np.int64), rng)
    return Case("all-empty base", "ivf_size = 0 and T = 0 before the append: every entry of the new array is a pair", base,
                [rand_docs(rng, [5, 0, 12, 3], 256)], decompress_all=True)


def merge_cases():
    return [hot_list()] + residues() + [sparse_lists()] + first_and_last_list() + [raw_list()] + inexact_lists() + [empty_base()]


def layout_cases():
    return strides() + range_table() + capacity() + inverse_norms()


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = merge_cases() + layout_cases()
        assert len({c.name for c in _ALL}) == len(_ALL)
    return _ALL


def case(name):
    return next(c for c in all_cases() if c.name == name)


# ---- several appends on a directory ------------------------------------------------------------------------------------------
DIR_STEPS = (7, 30, 1)     # documents per MmapIndex.append call


def directory_documents(centroids, seed=7010):
    """three batches of float documents near the centroids (what MmapIndex.append encodes)"""
    rng = np.random.default_rng(seed)
    K, dim = centroids.shape
    out = []
    for n in DIR_STEPS:
        batch = []
        for _ in range(n):
            L = int(rng.integers(1, 20))
            x = centroids[rng.integers(0, K, L)] + 0.02 * rng.standard_normal((L, dim)).astype(np.float32)
            batch.append(x.astype(np.float32))
        out.append(batch)
    return out
