"""numpy restatement of np_hip_index_expand's index-side rules (test infrastructure; numpy only: imports neither the package
nor the oracle).

    expanded_arrays   the arrays of the index after an expand, STARTING FROM THE BASE'S OWN LISTS: list c < K0 is old list c up
                      to its first id >= Nk = old documents - n_replace, followed by the ascending distinct ids of the given
                      documents that hold c; lists K0 .. K1 - 1 hold given ids only.  Centroids, doc_lengths, codes and residuals
                      as _final of tests/test_gpu_index_expand.py builds them
    given_pairs       append_restate.new_pairs with n_old = Nk: the NP_UNIQ_MAX raw-list rule is the append's
    widen_route       widen_codes_kernel thread by thread (the stride loop turn by turn in array arithmetic), with a census and
                      every destination entry counted: written twice or never is a RouteFault
    cut_merge_route   ivf_keep_kernel, the exclusive scan, ivf_code_starts_kernel, ivf_cut_offsets_kernel and
                      ivf_cut_merge_kernel in plain Python, thread by thread, with a census of the paths taken and the planted
                      defects of tests/test_expand_limits_cpu.py
    expected_*        the same facts from array arithmetic alone, without the route: what the census is held against
"""
import numpy as np

from append_restate import NP_MERGE_TILE, RouteFault, _list_of, new_pairs, offsets

WIDEN_MAX_BLOCKS = 8192
CUT_DEFECTS = ("keep_le", "no_cut", "begin_new", "new_lists_keep", "fast_plus", "fast_minus", "no_shift", "pfx_inclusive",
               "store_whole", "tile_prev", "gallop_lt")
WIDEN_DEFECTS = ("tail_dropped", "tail_any_block", "stride_block")
DEFECTS = CUT_DEFECTS + WIDEN_DEFECTS
CLASSES = ("keeps all", "keeps none", "cut inside", "empty", "new")


def given_pairs(n_keep, given, unique=True):
    return new_pairs(n_keep, given, unique)


def kept_mask(ivf, ivf_lengths, n_keep):
    """entries of each list in front of its FIRST id >= n_keep (the lists ascend, so these are its ids < n_keep)"""
    ivf = np.asarray(ivf, np.int64)
    il = np.asarray(ivf_lengths, np.int64)
    seen = np.concatenate([[0], np.cumsum(ivf >= n_keep)])        # dropped ids in front of entry i, over the whole array
    return seen[1:] - np.repeat(seen[offsets(il)[:-1]], il) == 0


def expanded_arrays(base, new_centroids, given, n_replace):
    """the index after the expand, from the base's own lists"""
    K0, dim = base["centroids"].shape
    pd = base["residuals"].shape[1]
    n_keep = int(np.asarray(base["doc_lengths"]).size) - int(n_replace)
    t_keep = int(np.asarray(base["doc_lengths"], np.int64)[:n_keep].sum())
    cen = np.ascontiguousarray(np.concatenate([base["centroids"], np.asarray(new_centroids, np.float32).reshape(-1, dim)]), np.float32)
    K1 = cen.shape[0]
    lens = np.concatenate([np.asarray(base["doc_lengths"], np.int64)[:n_keep], np.asarray(given[0], np.int64)])
    codes = np.concatenate([np.asarray(base["codes"], np.int64)[:t_keep], np.asarray(given[1], np.int64)])
    res = np.concatenate([base["residuals"][:t_keep], np.asarray(given[2], np.uint8).reshape(-1, pd)])
    il0 = np.asarray(base["ivf_lengths"], np.int64)
    keep = kept_mask(base["ivf"], il0, n_keep)
    old_cell = np.repeat(np.arange(K0, dtype=np.int64), il0)[keep]
    old_doc = np.asarray(base["ivf"], np.int64)[keep]
    pairs = np.unique(given_pairs(n_keep, given)[0])
    new_cell, new_doc = pairs >> 32, pairs & 0xFFFFFFFF
    cell = np.concatenate([old_cell, new_cell])
    order = np.argsort(cell, kind="stable")          # a list's kept entries stay in front, in their order
    ivf = np.concatenate([old_doc, new_doc])[order]
    il = np.bincount(cell, minlength=K1).astype(np.int32)
    return dict(base, centroids=cen, doc_lengths=lens, codes=codes, residuals=res, ivf=ivf, ivf_lengths=il)


# ---- widen_codes_kernel ----------------------------------------------------------------------------------------------------------
def widen_grid(n):
    """the grid expand_documents launches"""
    return max(1, min(((n >> 3) + 255) // 256, WIDEN_MAX_BLOCKS))


def widen_route(codes_u16, n, grid=None, defect=None):
    """widen_codes_kernel over `grid` blocks of 256 threads.  Returns (the u32 array of n entries, census).  Every destination
    entry must be written exactly once: RouteFault "twice" / "unwritten"; a 16-byte access over either array's end "store"."""
    assert defect is None or defect in WIDEN_DEFECTS
    src = np.asarray(codes_u16, np.uint16)
    n = int(n)
    assert src.size >= n
    G = widen_grid(n) if grid is None else int(grid)
    n8, threads = n >> 3, G * 256
    stride = 256 if defect == "stride_block" else threads
    dst = np.zeros(n, np.uint32)
    writes = np.zeros(n, np.uint8)
    census = dict(grid=G, groups=0, tail=0, max_turns=0)
    i = np.arange(threads, dtype=np.int64)          # tid
    eight = np.arange(8, dtype=np.int64)
    while True:
        i = i[i < n8]
        if i.size == 0:
            break
        census["max_turns"] += 1                     # thread 0 takes every turn any thread takes
        census["groups"] += int(i.size)
        for a in range(0, i.size, 1 << 20):
            at = (i[a:a + (1 << 20), None] * 8 + eight).reshape(-1)
            if at.size and at[-1] >= n:
                raise RouteFault("store", f"group {int(at[-1]) >> 3} of {n8}")
            dst[at] = src[at]                        # v.x & 0xFFFF, v.x >> 16, ...: the eight codes in their order
            if np.any(writes[at]):
                raise RouteFault("twice", f"a group of eight at turn {census['max_turns']}")
            writes[at] = 1
        i = i + stride
    tid = np.arange(threads, dtype=np.int64)
    first = (tid % 256 < 8) if defect == "tail_any_block" else (tid < 8)
    lane = tid % 256 if defect == "tail_any_block" else tid
    t = (n8 << 3) + lane[first]
    t = t[t < n]
    if defect != "tail_dropped":
        for x in t.tolist():
            if writes[x]:
                raise RouteFault("twice", f"tail entry {x}")
            dst[x] = src[x]
            writes[x] = 1
            census["tail"] += 1
    if not np.all(writes == 1):
        raise RouteFault("unwritten", f"entry {int(np.argmin(writes))} of {n}")
    return dst, census


def expected_widen(n, grid=None):
    G = widen_grid(n) if grid is None else grid
    return dict(grid=G, groups=n >> 3, tail=n & 7, max_turns=-(-(n >> 3) // (G * 256)))


# ---- the cut and the merge ---------------------------------------------------------------------------------------------------------
def cut_merge_route(old_ivf, old_off, K0, K1, Nk, pairs, tile=NP_MERGE_TILE, defect=None, uncut=False):
    """rewrite_posting_lists' kernels over the grids it launches.  Returns (new array, new offsets, census).  A read or a
    write outside an array raises RouteFault; so does a read of an old entry at or behind its list's cut ("dropped").
    uncut: the append's call, which cuts nothing and adds no list (K0 == K1, every old id < Nk) -- ivf_keep_kernel and its
    scan do not run, the old offsets themselves are old_begin and kept_pfx."""
    assert defect is None or defect in CUT_DEFECTS
    assert not uncut or (defect is None and K0 == K1)
    old_ivf = np.asarray(old_ivf, np.int64)
    old_off = [int(x) for x in old_off]
    pairs = np.asarray(pairs, np.int64)
    assert len(old_off) == K0 + 1 and K1 >= K0
    P, K = int(pairs.size), K1

    def off_at(c):
        if not 0 <= c <= K0:
            raise RouteFault("old_off", f"[{c}] of {K0 + 1}")
        return old_off[c]

    # where every old list is really cut (the lists ascend): what a read must stay in front of
    il0 = np.diff(np.asarray(old_off, np.int64))
    cell_of = np.repeat(np.arange(K0, dtype=np.int64), il0)
    true_keep = np.bincount(cell_of[old_ivf < Nk], minlength=K0)
    behind_cut = np.arange(old_ivf.size) >= (np.asarray(old_off[:-1], np.int64) + true_keep)[cell_of] if old_ivf.size else np.zeros(0, bool)

    # ivf_code_starts_kernel: start[c] = the first sorted pair whose code is >= c, by bisection
    start = [int(x) for x in np.searchsorted(pairs, np.arange(K + 1, dtype=np.int64) << 32, side="left")]
    # ivf_keep_kernel: (K + 256) / 256 blocks of 256
    old_begin, n_keep, klass = [None] * (K + 1), [None] * (K + 1), [None] * K
    keep_threads = 0 if uncut else (K + 256) // 256 * 256
    if uncut:
        old_begin, n_keep = list(old_off), il0.tolist() + [0]
        klass = ["keeps all" if n else "empty" for n in n_keep[:K]]
    for c in range(keep_threads):
        if c > K:
            continue
        if c >= K0 and defect != "new_lists_keep":
            old_begin[c], n_keep[c] = 0, 0
            if c < K:
                klass[c] = "new"
            continue
        s0 = off_at(c)
        a, z = 0, off_at(c + 1) - s0
        n = z
        while a < z:
            mid = (a + z) >> 1
            if not 0 <= s0 + mid < old_ivf.size:
                raise RouteFault("old_ivf", f"[{s0 + mid}] of {old_ivf.size}")
            v = int(old_ivf[s0 + mid])
            if (v <= Nk) if defect == "keep_le" else (v < Nk):
                a = mid + 1
            else:
                z = mid
        old_begin[c], n_keep[c] = s0, (n if defect == "no_cut" else a)
        klass[c] = "empty" if n == 0 else "keeps all" if a == n else "keeps none" if a == 0 else "cut inside"
    assert None not in old_begin and None not in n_keep, "the keep kernel's grid left a list out"
    # device_scan_exclusive over K + 1 entries
    kept_pfx = list(old_off) if uncut else (np.cumsum(n_keep) if defect == "pfx_inclusive" else offsets(n_keep)[:-1]).tolist()
    new_off = [a + b for a, b in zip(kept_pfx, start)]                 # ivf_cut_offsets_kernel
    total = kept_pfx[K] + P
    out = np.full(total, -1, np.int64)
    census = dict(fast=0, slow=0, whole_stores=0, partial_stores=0, max_lists_in_quad=0, longest_gallop=0, last_quad=0, tiles=[],
                  tile_first_list=[], total=total, P=P, kept=kept_pfx[K], classes=klass, shifts=set(), ends_at_cut=0,
                  ends_past_cut=0, keep_blocks=keep_threads // 256, keep_threads_in_last_block=K + 1 - (keep_threads - 256))
    quads_per_thread = tile // 1024
    assert tile % 1024 == 0

    def old_at(i):
        if not 0 <= i < old_ivf.size:
            raise RouteFault("old_ivf", f"[{i}] of {old_ivf.size}")
        if behind_cut[i]:
            raise RouteFault("dropped", f"[{i}] = {int(old_ivf[i])}, a document >= {Nk}")
        return int(old_ivf[i])

    def pair_at(j):
        if not 0 <= j < P:
            raise RouteFault("pairs", f"[{j}] of {P}")
        return int(pairs[j]) & 0xFFFFFFFF

    def of_list(c):
        return (new_off[c], new_off[c + 1], new_off[c] if defect == "begin_new" else old_begin[c], kept_pfx[c + 1] - kept_pfx[c],
                start[c])

    for blk in range((total + tile - 1) // tile):        # (no launch when total == 0)
        o0 = blk * tile
        c0 = _list_of(new_off, K, 0, o0 - 1 if defect == "tile_prev" else o0, defect, census)
        census["tile_first_list"].append(c0)
        for tid in range(256):
            c = c0
            for it in range(quads_per_thread):
                o = o0 + it * 1024 + tid * 4
                if o >= total:
                    continue
                n = min(4, total - o)
                c = _list_of(new_off, K, c, o, defect, census)
                b_new, e_new, b_old, n_old, b_pair = of_list(c)
                if tid == 0 and it == 0:
                    r = o - b_new
                    skipped = 0
                    while c - skipped > 0 and new_off[c - skipped - 1] == new_off[c - skipped]:
                        skipped += 1
                    census["tiles"].append(dict(list=c, r=r, n_old=n_old, n_new=e_new - b_new - n_old,
                                                part="kept" if r < n_old else "new", empty_lists_before=skipped))
                if n == 4 and c < K0 and true_keep[c] < il0[c] and o >= b_new:
                    census["ends_at_cut"] += o + 4 == b_new + n_old
                    census["ends_past_cut"] += o + 4 == b_new + n_old + 1
                q = [0, 0, 0, 0]
                bound = b_new + n_old + (1 if defect == "fast_plus" else -1 if defect == "fast_minus" else 0)
                if n == 4 and o + 4 <= bound:
                    census["fast"] += 1
                    census["shifts"].add((kept_pfx[c] - old_begin[c]) % 4)
                    q = [old_at(b_old + (o - b_new) + k) for k in range(4)]
                    lists = {c}
                else:
                    census["slow"] += 1
                    lists = set()
                    for k in range(n):
                        oo = o + k
                        if oo >= e_new:
                            c = _list_of(new_off, K, c, oo, defect, census)
                            b_new, e_new, b_old, n_old, b_pair = of_list(c)
                        r = oo - b_new
                        if r < 0:
                            raise RouteFault("list", f"entry {oo} before list {c}")
                        if r < n_old:
                            q[k] = old_at(b_old + r)
                        else:
                            q[k] = pair_at((0 if defect == "no_shift" else b_pair) + (r - n_old))
                        lists.add(c)
                census["max_lists_in_quad"] = max(census["max_lists_in_quad"], len(lists))
                if o + 4 <= total or defect == "store_whole":
                    census["whole_stores"] += 1
                    if o + 4 > total:
                        raise RouteFault("store", f"16 bytes at entry {o} of {total}")
                    out[o:o + 4] = q
                else:
                    census["partial_stores"] += 1
                    out[o:total] = q[:total - o]
                if o + 4 >= total:
                    census["last_quad"] = n
    return out, np.asarray(new_off, np.int64), census


# ---- what the census is held against: the same facts without the route -------------------------------------------------------------
def expected_cut(old_ivf, old_off, K0, K1, Nk, pairs):
    """(new offsets, kept length, old length, gain) per list of the K1"""
    old_ivf, old_off = np.asarray(old_ivf, np.int64), np.asarray(old_off, np.int64)
    il0 = np.diff(old_off)
    cell = np.repeat(np.arange(K0, dtype=np.int64), il0)
    keep = np.zeros(K1, np.int64)
    keep[:K0] = np.bincount(cell[old_ivf < Nk], minlength=K0)
    length = np.zeros(K1, np.int64)
    length[:K0] = il0
    gain = np.bincount(np.asarray(pairs, np.int64) >> 32, minlength=K1)
    return offsets(keep + gain), keep, length, gain


def _quads(new_off):
    o = np.arange(0, int(new_off[-1]) - 3, 4, dtype=np.int64)
    return o, np.searchsorted(new_off, o, side="right") - 1


def expected_fast_quads(*a):
    """quads of 4 entries that lie wholly inside the kept part of one list"""
    new_off, keep, _, _ = expected_cut(*a)
    o, c = _quads(new_off)
    return int(np.sum(o + 4 <= new_off[c] + keep[c]))


def expected_shifts(*a):
    """(place in the kept-only array - place in the old array) mod 4 of the lists that hold a fast quad"""
    new_off, keep, _, _ = expected_cut(*a)
    o, c = _quads(new_off)
    lists = np.unique(c[o + 4 <= new_off[c] + keep[c]])
    old_off = np.asarray(a[1], np.int64)
    return set(((offsets(keep)[lists] - old_off[lists]) % 4).tolist())


def expected_cut_quad_ends(*a):
    """(quads that end exactly at a cut with dropped entries behind it, quads that end one entry past such a cut)"""
    new_off, keep, length, _ = expected_cut(*a)
    o, c = _quads(new_off)
    end = new_off[c] + keep[c]
    cut = keep[c] < length[c]
    return int(np.sum((o + 4 == end) & cut)), int(np.sum((o + 4 == end + 1) & cut))


def expected_tiles(*a, tile=NP_MERGE_TILE):
    """per tile: (first list, "kept" / "new", empty lists directly in front of that list)"""
    new_off, keep, _, _ = expected_cut(*a)
    il = np.diff(new_off)
    out = []
    for o0 in range(0, int(new_off[-1]), tile):
        c = int(np.searchsorted(new_off, o0, side="right") - 1)
        filled = np.nonzero(il[:c] > 0)[0]
        out.append((c, "kept" if o0 - new_off[c] < keep[c] else "new", c - (int(filled[-1]) + 1 if filled.size else 0)))
    return out


def expected_classes(*a):
    _, keep, length, _ = expected_cut(*a)
    K0 = a[2]
    k = np.where(length == 0, 3, np.where(keep == length, 0, np.where(keep == 0, 1, 2)))
    k[K0:] = 4
    return [CLASSES[i] for i in k.tolist()]
