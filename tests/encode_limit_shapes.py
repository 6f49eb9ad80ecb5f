"""Index-time encode (codec.rs:297-411) at the kernels' own edges: cases with their answers by construction
(test infrastructure; numpy only: imports neither the package nor the oracle).

    argmax_cases()   centroids and tokens on a dyadic grid, so every dot product is exact in f32 in any summation order:
                     planted duplicates, near ties, all-negative scores, +0 and NaN rows, finite next to +-inf scores
    pack_cases()     well-separated centroids (the code does not depend on rounding); residuals ON the cutoffs, one ulp
                     above and below them, +-0, +-inf, NaN; five kinds of cutoff table at nbits 1, 2, 4, 8
    restate()        the rule written out plainly, and the wrong rules (WRONG_RULES) as variants of it
    codec_arrays()   the smallest valid index around a centroid table (one one-token document)

Every builder returns Case(centroids, cutoffs, nbits, tokens, want_codes, want_packed); what a case plants is asserted
where it is built (the set of exact maxima of a planted token IS the planted set), so want_codes does not rest on
restate() alone.

The argmax grid.  Centroid entries are +-2^-3, token entries are integer multiples of 2^-10 below 2^-2 in magnitude: a
product is a multiple of 2^-13, a score of dim <= 128 terms stays below 2^2, so every partial sum in every order needs
at most 15 bits.  sum_j s_j x_j has the parity of sum_j x_j whatever the signs s_j, so all scores of ONE token differ by
multiples of 2 * 2^-13: that is the grid of score differences, and a near tie is one step of it.
"""
from dataclasses import dataclass

import numpy as np

F32, F64 = np.float32, np.float64
CU, TU = 2.0 ** -3, 2.0 ** -10        # centroid entry, token grid unit
K_VALUES = (1, 2, 31, 32, 33, 63, 64, 65, 300, 2047, 2048, 2049, 2113)   # 2113: 67 groups of 32 (68 stored), more than a wave has lanes
# (dim, nbits) of the geometry fixtures' kind: the smallest dim; a kernel width; rows stored wider than the file's (100, 104)
GEOMETRIES = ((8, 4), (96, 2), (128, 4), (100, 2), (104, 1), (8, 1), (96, 8), (128, 1), (100, 8), (8, 2), (128, 8), (8, 8),
              (100, 4))
WRONG_RULES = {
    "ge": "a residual equal to a cutoff counts that cutoff (>= instead of >)",
    "first": "the first of equal maxima wins",
    "pad": "the zero rows that pad K up to a multiple of 64 take part with score 0",
    "byvalue": "non-finite scores are ordered by value (+inf above every finite score)",
    "msb": "a bucket's bits are written MSB-first",
}


@dataclass
class Case:
    name: str
    centroids: np.ndarray
    cutoffs: np.ndarray
    nbits: int
    tokens: np.ndarray
    want_codes: np.ndarray
    want_packed: np.ndarray
    notes: tuple = ()         # what each token plants: (token index, text, expected set of exact maxima or None)
    table: str = ""           # pack cases: the kind of cutoff table

    def __iter__(self):       # (centroids, cutoffs, nbits, tokens, want_codes, want_packed)
        return iter((self.centroids, self.cutoffs, self.nbits, self.tokens, self.want_codes, self.want_packed))


# ---- the rule ----------------------------------------------------------------------------------------------------------
def scores_f32(centroids, tokens):
    """[n, K] f32 scores from float64 dot products (exact on the cases' grids); overflow becomes +-inf as in f32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(tokens, F32).astype(F64) @ np.asarray(centroids, F32).astype(F64).T).astype(F32)


def codes_of(S, rule=None):
    """cmp_f32_for_max (codec.rs:23-30) + Iterator::max_by: non-finite scores are equal and below every finite one, the
    LAST of equal maxima wins."""
    S = np.asarray(S, F32)
    if rule == "pad":
        S = np.concatenate([S, np.zeros((S.shape[0], -S.shape[1] % 64), F32)], 1)
    with np.errstate(invalid="ignore"):
        if rule == "byvalue":
            V = np.where(np.isnan(S), -np.inf, S.astype(F64))
            V = np.where(np.isposinf(S), 1e300, np.where(np.isneginf(S), -1e300, V))
        else:
            V = np.where(np.isfinite(S), S.astype(F64), -np.inf)
    V = np.where(V == 0, 0.0, V)                       # total_cmp puts -0 below +0; no case has both (asserted by the builders)
    if rule == "first":
        return np.argmax(V, 1).astype(np.int64)
    return (V.shape[1] - 1 - np.argmax(V[:, ::-1], 1)).astype(np.int64)


def buckets_of(residuals, cutoffs, rule=None):
    """codec.rs:356-372: the number of cutoffs STRICTLY below the residual (a count, not a search; NaN is below nothing)."""
    r, c = np.asarray(residuals, F32)[:, :, None], np.asarray(cutoffs, F32)[None, None, :]
    with np.errstate(invalid="ignore"):
        return ((r >= c) if rule == "ge" else (r > c)).sum(2).astype(np.int64)


def pack_buckets(buckets, nbits, rule=None):
    """codec.rs:373-411: per dim the bucket's bits LSB-first into one bit stream, the stream into bytes MSB-first."""
    order = range(nbits - 1, -1, -1) if rule == "msb" else range(nbits)
    bits = np.stack([(buckets >> b) & 1 for b in order], 2).astype(np.uint8)
    return np.packbits(bits.reshape(buckets.shape[0], -1), axis=1, bitorder="big")


def restate(centroids, cutoffs, nbits, tokens, rule=None):
    """(codes, packed) of the encode; rule: None or a key of WRONG_RULES."""
    cen, x = np.asarray(centroids, F32), np.asarray(tokens, F32)
    codes = codes_of(scores_f32(cen, x), rule)
    with np.errstate(invalid="ignore", over="ignore"):
        res = x - cen[np.minimum(codes, cen.shape[0] - 1)]      # one f32 subtraction per component (index.rs:17-40)
    return codes, pack_buckets(buckets_of(res, cutoffs, rule), nbits, rule)


def codec_arrays(centroids, nbits):
    """Index arrays holding this codec and one one-token document (any valid posting data serves an encode)."""
    cen = np.ascontiguousarray(centroids, F32)
    K, dim = cen.shape
    il = np.zeros(K, np.int32)
    il[0] = 1
    return dict(nbits=nbits, centroids=cen, bucket_weights=np.zeros(1 << nbits, F32), ivf=np.zeros(1, np.int64),
                ivf_lengths=il, doc_lengths=np.ones(1, np.int64), codes=np.zeros(1, np.int64),
                residuals=np.zeros((1, dim * nbits // 8), np.uint8))


def ascending_cutoffs(nbits):
    """2^nbits - 1 ascending dyadic values, none of them 0, not symmetric: (2 i - ncut + 2) 2^-(nbits + 4)."""
    n = (1 << nbits) - 1
    return ((2 * np.arange(n) - n + 2) * 2.0 ** -(nbits + 4)).astype(F32)


# ---- argmax cases ------------------------------------------------------------------------------------------------------
def _signs(g, K, dim, p_plus=0.5):
    """K pairwise distinct rows of +-1 (dim 8: distinct by drawing distinct bit patterns)."""
    if dim <= 16 and p_plus == 0.5:
        pat = g.choice(1 << dim, K, replace=False)
        s = ((pat[:, None] >> np.arange(dim)) & 1) * 2 - 1
    elif dim <= 16:     # majority-plus rows: at least dim/2 + 1 pluses; 93 such patterns at dim 8
        pat = np.array([p for p in range(1 << dim) if bin(p).count("1") > dim // 2 + 1])     # 37 at dim 8: any two rows
        if K > pat.size:                                                                     # have a dot product >= 0
            pat = np.array([p for p in range(1 << dim) if bin(p).count("1") > dim // 2])
        s = ((g.choice(pat, K, replace=False)[:, None] >> np.arange(dim)) & 1) * 2 - 1
    else:
        s = np.where(g.random((K, dim)) < p_plus, 1, -1)
    assert np.unique(s, axis=0).shape[0] == K, "centroid rows are not distinct"
    return s.astype(np.int64)


def _near(g, s_row, n=1):
    """Tokens next to a centroid: 128 units of 2^-10 per entry plus up to 3 units of noise."""
    return s_row[None, :] * 128 + g.integers(-3, 4, (n, s_row.size))


def _finish(name, cen, nbits, X, notes, exact=True):
    """Case from f32 centroids and tokens: asserts exactness and what each token plants, derives the answers."""
    cen, X = np.ascontiguousarray(cen, F32), np.ascontiguousarray(X, F32)
    K = cen.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        S64 = X.astype(F64) @ cen.astype(F64).T
    S = scores_f32(cen, X)
    if exact:
        fin = np.isfinite(X).all(1)
        assert np.array_equal(S[fin].astype(F64), S64[fin]), f"{name}: a score is not exact in f32"
        assert np.abs(S64[fin]).max(initial=0) < 4 and np.all(S64[fin] * 2 ** 13 == np.round(S64[fin] * 2 ** 13)), name
    assert not np.any((S == 0) & np.signbit(S)), f"{name}: a -0 score"
    want = codes_of(S)
    with np.errstate(invalid="ignore"):
        V = np.where(np.isfinite(S), S.astype(F64), -np.inf)
    for t, text, planted in notes:
        if planted is not None:
            got = set(np.nonzero(V[t] == V[t].max())[0].tolist())
            assert got == set(planted), f"{name}: token {t} ({text}): maxima at {sorted(got)[:8]}, planted {sorted(planted)[:8]}"
            assert want[t] == max(planted), (name, t, text)
    assert np.all((want >= 0) & (want < K))
    cut = ascending_cutoffs(nbits)
    with np.errstate(invalid="ignore", over="ignore"):
        res = X - cen[want]
    return Case(name, cen, cut, nbits, X, want, pack_buckets(buckets_of(res, cut), nbits), tuple(notes))


def _plant_table(name, K, dim, nbits, seed, dups, nears):
    """Random sign centroids with planted duplicate groups and near pairs.  dups: tuples of indices that share one row.
    nears: (a, b): row b = row a with one sign flipped."""
    g = np.random.default_rng(seed)
    s = _signs(g, K, dim)
    used, flips = set(), {}
    dups = [d for d in dups if max(d) < K and min(d) >= 0 and len(set(d)) == len(d)]
    keep = []
    for d in dups:
        if used & set(d):
            continue
        used |= set(d)
        keep.append(d)
        for i in d[1:]:
            s[i] = s[d[0]]
    for a, b in nears:
        if max(a, b) >= K or used & {a, b}:
            continue
        others = {tuple(r) for i, r in enumerate(s.tolist()) if i not in (a, b)}
        for j0 in g.permutation(dim).tolist():      # row b = row a with sign j0 flipped, equal to no other row
            cand = s[a].copy()
            cand[j0] = -cand[j0]
            if tuple(cand.tolist()) not in others:
                s[b] = cand
                used |= {a, b}
                flips[(a, b)] = j0
                break
    assert np.unique(s, axis=0).shape[0] == K - sum(len(d) - 1 for d in keep), f"{name}: an unplanned duplicate"
    rows, notes = [], []

    def add(x, text, planted):
        notes.append((len(rows), text, planted))
        rows.append(np.asarray(x, np.int64).reshape(-1))
    alone = [i for i in dict.fromkeys((0, K - 1, 32 * ((K - 1) // 32), K // 2)) if i not in used]
    for i in alone:
        add(_near(g, s[i]), f"winner alone at {i}", {i})
    for d in keep:
        add(_near(g, s[d[0]]), f"duplicates {d}", set(d))
        add(s[d[0]] * 128, f"duplicates {d}, the row itself", set(d))
    for (a, b), j0 in flips.items():
        for win, lose in ((a, b), (b, a)):      # one step of the difference grid, in both index orders
            x = _near(g, s[win])[0]
            x[j0] = s[win, j0]
            add(x, f"near tie: {win} beats {lose} by 2^-12", {win})
    add(np.zeros(dim), "every score +0", set(range(K)))
    X = (np.stack(rows) * TU).astype(F32)
    nan_row = (_near(g, s[0])[0] * TU).astype(F32)
    nan_row[dim // 2] = np.nan
    notes.append((X.shape[0], "a NaN component: every score NaN", set(range(K))))
    return _finish(name, s * CU, nbits, np.concatenate([X, nan_row[None]]), notes)


def _identical_table(name, K, dim, nbits, seed):
    g = np.random.default_rng(seed)
    s = np.repeat(_signs(g, 1, dim), K, 0)
    X = np.concatenate([_near(g, s[0], 3), -_near(g, s[0], 1), np.zeros((1, dim), np.int64)])
    notes = [(t, "all K rows identical", set(range(K))) for t in range(X.shape[0])]
    return _finish(name, s * CU, nbits, X * TU, notes)


def _negative_table(name, K, dim, nbits, seed):
    """Rows with more pluses than minuses: -(1, ..., 1) and -(the sum of the centroid directions) score negative on every
    row, so the zero rows that pad K up to a multiple of 64 would win if they took part."""
    g = np.random.default_rng(seed)
    s = _signs(g, K, dim, p_plus=0.8)
    assert np.all(s.sum(1) > 0)
    tot = s.sum(0)
    scale = max(1, int(np.abs(tot).max()) // 200 + 1)
    X = np.stack([-np.ones(dim, np.int64) * 100, -(tot // scale), -np.ones(dim, np.int64), -(100 + g.integers(0, 2, dim)),
                  -(7 + g.integers(0, 2, dim))])
    cen = s * CU
    texts = ["-(1, ..., 1)", "minus the sum of the centroid directions", "-(1, ..., 1), small", "-(1, ..., 1) with noise",
             "-(1, ..., 1) with noise, small"]
    neg = np.all((X * TU) @ cen.T < 0, axis=1)
    assert neg[[0, 2, 3, 4]].all() and (neg[1] or K > 37), f"{name}: a score is not negative"
    notes = [(t, "every score negative: " + texts[i], None) for t, i in enumerate(np.nonzero(neg)[0])]
    return _finish(name, cen, nbits, X[neg] * TU, notes)


def _mixed_table(name, K, dim, nbits, seed, only_first_finite=False):
    """Token 3e38 e_j against a column j of 0.5, 0.25, 2 and -2: scores 1.5e38, 7.5e37, +inf, -inf.  The finite maximum
    wins; with only_first_finite the one finite score is at index 0 and +inf follows it everywhere."""
    g = np.random.default_rng(seed)
    cen = (_signs(g, K, dim) * CU).astype(F32)
    j = int(g.integers(0, dim))
    if only_first_finite:
        col = np.full(K, 2.0)
        col[0] = 0.5
    else:
        col = g.choice([0.5, 0.25, 2.0, -2.0], K)
        col[K - 1] = 2.0                                 # a non-finite score after the last finite maximum
        col[int(g.integers(0, K - 1))] = 0.5
    cen[:, j] = col
    X = np.zeros((3, dim), F32)
    X[0, j], X[1, j], X[2, j] = 3e38, -3e38, 3e38
    X[2, (j + 1) % dim] = 1.0 if dim > 1 else 0.0          # a second, finite term in every sum
    S = scores_f32(cen, X)
    assert np.isinf(S[0]).any() and np.isfinite(S[0]).any()
    fin0 = np.nonzero(col == 0.5)[0]
    notes = [(0, "finite maximum among +-inf scores", set(fin0.tolist()))]
    if not only_first_finite and np.any(col == 0.25):
        notes.append((1, "negated: 0.25 holds the finite maximum", None))
    return _finish(name, cen, nbits, X, notes, exact=False)


def _dups(K, which):
    """Disjoint duplicate groups; indices past K drop out.  (0, K - 1) and (31, 32) collide at K = 33, so table a holds
    the group border for K < 64 and the first and last lane of one group, (i, i + 31), otherwise."""
    if which == "a":
        lanes = (32, 63) if K >= 64 else ((0, 31) if K == 32 else (31, 32))
        return [(5, 6), lanes, (70, 2048 + 70), (32 + 7, 2080 + 7), (13, 13 + 32, 13 + 64), (2, 3)]
    return [(0, K - 1), (31, 32), (10, 11, 12), (63, 64), (2047, 2048), (3, 2048 + 35)]


def _geometry(K, ki, i):
    """dim 8 has 256 sign rows (93 with a plus majority): the K up to 65 take it every other time, the rest rotate the
    wider rows."""
    small = [gm for gm in GEOMETRIES if gm[0] == 8]
    wide = [gm for gm in GEOMETRIES if gm[0] != 8]
    if K <= 65 and (i + ki) % 2 == 0:
        return small[(i + ki) // 2 % len(small)]
    return wide[(3 * i + ki) % len(wide)]


def argmax_cases():
    out = []
    for ki, K in enumerate(K_VALUES):
        seed = 7000 + 17 * K
        tables = (("dupA", _plant_table, (seed + 1, _dups(K, "a"), [(20, 21), (0, 1)])),
                  ("dupB", _plant_table, (seed + 2, _dups(K, "b"), [(21, 20 + 32), (40, 40 + 2048), (1, 0)])),
                  ("alone", _plant_table, (seed + 7, [], [])),
                  ("same", _identical_table, (seed + 3,)),
                  ("neg", _negative_table, (seed + 4,)),
                  ("mixed", _mixed_table, (seed + 5,)),
                  ("mixed0", _mixed_table, (seed + 6, True)))
        for i, (kind, build, args) in enumerate(tables):
            if kind.startswith("mixed") and K < 2:      # one score cannot be finite AND not
                continue
            dim, nbits = _geometry(K, ki, i)
            out.append(build(f"K{K}-{kind}-d{dim}b{nbits}", K, dim, nbits, *args))
    return out


# ---- pack cases --------------------------------------------------------------------------------------------------------
PACK_GEOMETRIES = ((8, 1, 3), (8, 2, 40), (8, 4, 70), (8, 8, 5), (96, 2, 33), (100, 4, 65), (104, 1, 7), (128, 8, 300),
                   (100, 8, 2), (96, 4, 64))     # (dim, nbits, K)
TABLES = ("ascending", "zero", "repeated", "descending", "nan")


def cutoff_table(kind, nbits):
    a = ascending_cutoffs(nbits)
    n = a.size
    if kind == "ascending":
        return a
    if kind == "zero":                  # the codec of a corpus without held-out tokens
        return np.zeros(n, F32)
    if kind == "descending":            # the reference counts cutoffs, it does not search
        return a[::-1].copy()
    if kind == "repeated":              # a repeated value, and -0.0 next to +0.0
        r = a.copy()
        if n == 1:
            r[0] = -0.0
        else:
            r[n // 2] = r[n // 2 - 1]
            r[0], r[-1] = -0.0, 0.0
        return r
    if kind == "nan":
        r = a.copy()
        r[n // 2] = np.nan
        return r
    raise KeyError(kind)


def _pack_case(dim, nbits, K, kind, seed):
    """The smallest token count (doubling from 48) at which the coverage conditions hold."""
    n = 48
    while True:
        try:
            return _pack_case_n(dim, nbits, K, kind, seed, n)
        except AssertionError:
            if n >= 768:
                raise
            n *= 2


def _pack_case_n(dim, nbits, K, kind, seed, n):
    name = f"pack-d{dim}b{nbits}K{K}-{kind}"
    g = np.random.default_rng(seed)
    # entries +-2^-2, the last column 0: a token entry there IS the residual, so -0.0 meets +0.0 (x - c = -0 only for
    # x = -0, c = +0).  Rows differ in >= 1 of the other columns: margins of at least 2^-3 minus the residual terms.
    s = _signs(g, K, dim - 1)
    cen = np.concatenate([s * 0.25, np.zeros((K, 1))], 1).astype(F32)
    cut = cutoff_table(kind, nbits)
    per, ncut = 8 // nbits, cut.size
    fin = cut[np.isfinite(cut)]
    if fin.size == 0:                      # nbits 1, the one cutoff NaN: nothing can equal it
        fin = ascending_cutoffs(nbits)
    pool = np.concatenate([np.tile(fin, max(1, -(-14 // fin.size))), F32([0.0, -0.0])])    # the cutoffs themselves and +-0
    z = g.integers(0, K, n)
    r = pool[g.integers(0, pool.size, (n, dim))]
    move = g.integers(0, 3, (n, dim))                    # 0: on the cutoff, 1: one ulp up, 2: one ulp down
    x = (cen[z] + r).astype(F32)
    x = np.where((cen[z] == 0) & (r == 0), r, x)         # keep the sign of a zero
    # the ulp of the TOKEN's component: a neighbour of the cutoff itself is lost when it is added to the centroid
    x = np.where(move == 1, np.nextafter(x, F32(np.inf)), np.where(move == 2, np.nextafter(x, F32(-np.inf)), x)).astype(F32)
    x[0, dim - 1], x[1, dim - 1] = -0.0, 0.0            # residuals -0.0 and +0.0 (the centroids' last column is +0.0)
    with np.errstate(invalid="ignore"):
        S64 = x.astype(F64) @ cen.astype(F64).T
    top2 = np.sort(S64, 1)[:, -2:] if K > 1 else None
    if K > 1:
        assert np.all(top2[:, 1] - top2[:, 0] >= 2.0 ** -4), f"{name}: margin {np.min(top2[:, 1] - top2[:, 0])}"
    assert np.array_equal(np.argmax(S64, 1), z)
    # non-finite components: every score is non-finite, the code is K - 1 and the residual is taken against that row
    special = cen[np.full(6, K - 1)] + pool[g.integers(0, pool.size, (6, dim))]
    special = special.astype(F32)
    for t, (j, v) in enumerate(((0, np.inf), (dim - 1, -np.inf), (dim // 2, np.nan), (dim - 1, np.nan), (1 % dim, -np.inf),
                                (dim - 1, np.inf))):
        special[t, j] = v
    x = np.concatenate([x, special])
    want = np.concatenate([z, np.full(6, K - 1)]).astype(np.int64)
    assert np.array_equal(codes_of(scores_f32(cen, x)), want), name
    with np.errstate(invalid="ignore", over="ignore"):
        res = x - cen[want]
    bk = buckets_of(res, cut)
    c = Case(name, cen, cut, nbits, x, want, pack_buckets(bk, nbits), (), kind)
    check_pack_coverage(c)
    return c


def pack_coverage(c):
    """(share of residuals equal to a cutoff, buckets that occur, (bucket, position in the byte) pairs that occur)."""
    with np.errstate(invalid="ignore", over="ignore"):
        res = c.tokens - c.centroids[c.want_codes]
        on = (res[:, :, None] == c.cutoffs[None, None, :]).any(2)
    bk = buckets_of(res, c.cutoffs)
    per = 8 // c.nbits
    pos = np.broadcast_to(np.arange(bk.shape[1]) % per, bk.shape)
    return float(on.mean()), set(np.unique(bk).tolist()), set(zip(bk.ravel().tolist(), pos.ravel().tolist())), res


def attainable_buckets(cutoffs):
    """The counts some real residual can give: one per gap of the sorted finite cutoffs."""
    f = np.sort(cutoffs[np.isfinite(cutoffs)].astype(F64))
    probes = np.concatenate([[-np.inf], f, (f[:-1] + f[1:]) / 2, [np.inf]])
    return set(int((p > cutoffs.astype(F64)).sum()) for p in probes)


def check_pack_coverage(c):
    share, seen, seen_pos, res = pack_coverage(c)
    per = 8 // c.nbits
    assert share >= 0.25 or not np.isfinite(c.cutoffs).any(), f"{c.name}: only {share:.3f} of the residuals equal a cutoff"
    want = set(range(1 << c.nbits)) if c.table in ("ascending", "descending") else attainable_buckets(c.cutoffs)
    assert want <= seen, f"{c.name}: buckets {sorted(want - seen)} never occur"
    missing = {(b, p) for b in want for p in range(per)} - seen_pos
    assert not missing, f"{c.name}: (bucket, position in the byte) {sorted(missing)[:6]} never occur"
    z = (res == 0)
    assert np.any(z & np.signbit(res)) and np.any(z & ~np.signbit(res)), f"{c.name}: both zeros as residuals"
    assert np.isnan(res).any() and np.isposinf(res).any() and np.isneginf(res).any()


def pack_cases():
    out = []
    for gi, (dim, nbits, K) in enumerate(PACK_GEOMETRIES):
        for ti, kind in enumerate(TABLES):
            if gi >= 4 and (gi + ti) % 2:        # nbits 1, 2, 4, 8 meet every table at dim 8; the wider rows take half of them
                continue
            out.append(_pack_case(dim, nbits, K, kind, 8100 + 10 * gi + ti))
    return out


_cache = {}


def all_cases():
    if "all" not in _cache:
        _cache["all"] = argmax_cases() + pack_cases()
    return _cache["all"]
