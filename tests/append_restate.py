"""numpy restatement of np_hip_index_append's index-side rules (test infrastructure; numpy only: imports neither the package
nor the oracle).

    grown_arrays   the arrays of the index after an append, STARTING FROM THE BASE'S GIVEN LISTS: list c is old list c followed
                   by the ascending ids of the new documents that hold c, each once (index.rs:479-499 for the new entries)
    new_pairs      the sorted (code << 32 | id) pairs rewrite_posting_lists makes of the new documents: a document of more than
                   NP_UNIQ_MAX tokens contributes every token (its distinct-code list is its codes as they are), and the
                   sorted pairs are then made unique
    merge_route    ivf_cut_merge_kernel's route on an append's arguments (nothing cut, no list added: the old offsets are
                   old_begin and kept_pfx at once) in plain Python, thread by thread, with a census of the paths it took and
                   the planted defects of tests/test_append_limits_cpu.py
    expected_*     the same facts from array arithmetic alone, without the route: what the census is held against
    stride_bytes   choose_ublock_stride's rule (host_stride_bytes)
    n_ranges       ceil(n_docs / NP_SPLIT_RANGE)
"""
import numpy as np

NP_UNIQ_MAX = 4096
NP_MERGE_TILE = 4096
NP_SPLIT_RANGE = 32768
DEFECTS = ("gallop_lt", "fast_plus", "fast_minus", "no_shift", "store_whole", "tile_prev", "keep_dups")


class RouteFault(Exception):
    """the route read or wrote outside an array: what the kernel would do out of bounds.  kind = "gallop" (past the last
    list), "old_ivf" / "pairs" (a read outside that array), "store" (a 16-byte store over the array's end), "list" (an entry in
    front of the list it was attributed to)"""

    def __init__(self, kind, what):
        super().__init__(f"{kind}: {what}")
        self.kind = kind


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int64)


def doc_of_token(lens):
    lens = np.asarray(lens, np.int64)
    return np.repeat(np.arange(lens.size, dtype=np.int64), lens)


def host_stride_bytes(a, code_bytes):
    """choose_ublock_stride: the block holds the 16-byte header and the smallest capacity that at most 1 % of the distinct-code
    lists exceed (list lengths are counted up to 256, longer ones in one bin), rounded up to a multiple of 64 bytes, at most
    512.  Returns (stride in bytes, lists that overflow it)."""
    lens = np.asarray(a["doc_lengths"], np.int64)
    codes = np.asarray(a["codes"], np.int64)
    n = lens.size
    K = int(a["centroids"].shape[0])
    doc = np.repeat(np.arange(n, dtype=np.int64), lens)
    ulen = np.bincount(np.unique(doc * K + codes) // K, minlength=n)
    hdr, per64, smax = 16 // code_bytes, 64 // code_bytes, 512 // code_bytes
    hist = np.bincount(np.minimum(ulen, 257), minlength=258)
    allow, over, q = n // 100, 0, 257
    while q > 0 and over + hist[q] <= allow:
        over += hist[q]
        q -= 1
    fit = min(smax - hdr, max(q, 1))
    stride = max(per64, min(smax, (hdr + fit + per64 - 1) // per64 * per64))
    return stride * code_bytes, int((ulen > stride - hdr).sum())


def code_bytes(a):
    return 4 if a["centroids"].shape[0] > 65536 else 2


def stride_bytes(a):
    return host_stride_bytes(a, code_bytes(a))


def overflow_list_lengths(a):
    """distinct-code counts of the documents whose list does not fit the block of stride_bytes(a)"""
    lens = np.asarray(a["doc_lengths"], np.int64)
    K = int(a["centroids"].shape[0])
    ulen = np.bincount(np.unique(doc_of_token(lens) * K + np.asarray(a["codes"], np.int64)) // K, minlength=lens.size)
    cb = code_bytes(a)
    return ulen[ulen > stride_bytes(a)[0] // cb - 16 // cb]


def n_ranges(n_docs):
    return -(-int(n_docs) // NP_SPLIT_RANGE)


def new_pairs(n_old, new, unique=True):
    """(sorted pairs code << 32 | id of the new documents, their count before the raw lists' duplicates are dropped)"""
    lens, codes = np.asarray(new[0], np.int64), np.asarray(new[1], np.int64)
    doc = doc_of_token(lens)
    key = (codes << 32) | (doc + n_old)
    raw = np.repeat(lens > NP_UNIQ_MAX, lens)
    # a document within NP_UNIQ_MAX has a sorted list of DISTINCT codes; a longer one lists every token
    pairs = np.sort(np.concatenate([np.unique(key[~raw]), key[raw]]))
    p_before = int(pairs.size)
    if unique and raw.any():   # (rewrite_posting_lists runs DeviceSelect::Unique only when some document is that long)
        pairs = np.unique(pairs)
    return pairs.astype(np.int64), p_before


def concat_new(new_steps, pd):
    lens = np.concatenate([np.asarray(s[0], np.int64).reshape(-1) for s in new_steps])
    codes = np.concatenate([np.asarray(s[1], np.int64).reshape(-1) for s in new_steps])
    res = np.concatenate([np.asarray(s[2], np.uint8).reshape(-1, pd) for s in new_steps])
    return lens, codes, res


def grown_arrays(base, new):
    """the index after the append, from the base's own lists"""
    K = int(base["centroids"].shape[0])
    n_old = int(np.asarray(base["doc_lengths"]).size)
    pd = base["residuals"].shape[1]
    lens = np.concatenate([np.asarray(base["doc_lengths"], np.int64), np.asarray(new[0], np.int64)])
    codes = np.concatenate([np.asarray(base["codes"], np.int64), np.asarray(new[1], np.int64)])
    res = np.concatenate([base["residuals"], np.asarray(new[2], np.uint8).reshape(-1, pd)])
    nl, nc = np.asarray(new[0], np.int64), np.asarray(new[1], np.int64)
    key = np.unique(nc * (nl.size + 1) + doc_of_token(nl))          # (code, new document) ascending, each once
    new_cell, new_doc = key // (nl.size + 1), key % (nl.size + 1) + n_old
    old_cell = np.repeat(np.arange(K, dtype=np.int64), np.asarray(base["ivf_lengths"], np.int64))
    cell = np.concatenate([old_cell, new_cell])
    order = np.argsort(cell, kind="stable")                          # old entries of a list stay in front, in their order
    ivf = np.concatenate([np.asarray(base["ivf"], np.int64), new_doc])[order]
    il = (np.asarray(base["ivf_lengths"], np.int64) + np.bincount(new_cell, minlength=K)).astype(np.int32)
    return dict(base, doc_lengths=lens, codes=codes, residuals=res, ivf=ivf, ivf_lengths=il)


# ---- the kernel's route ------------------------------------------------------------------------------------------------
def _list_of(off, K, c, o, defect, census):
    """ivf_list_of: the largest c' >= c with off[c'] <= o, galloping from c"""
    lo, step, hi = c, 1, min(K, c + 1)
    doublings = 0
    while (off[hi] < o) if defect == "gallop_lt" else (off[hi] <= o):
        lo = hi
        step <<= 1
        doublings += 1
        hi = min(K, lo + step)
        if lo == K:
            raise RouteFault("gallop", f"past list {K} for entry {o}")
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if off[mid] <= o:
            lo = mid
        else:
            hi = mid
    census["longest_gallop"] = max(census["longest_gallop"], doublings)
    return lo


def merge_route(old_ivf, old_off, pairs, K, tile=NP_MERGE_TILE, defect=None):
    """ivf_cut_merge_kernel over the grid rewrite_posting_lists launches for an append.  Returns (new array, new offsets, census).  A read or a
    write outside an array raises RouteFault."""
    assert defect is None or defect in DEFECTS
    old_ivf = np.asarray(old_ivf, np.int64)
    old_off = [int(x) for x in old_off]
    pairs = np.asarray(pairs, np.int64)
    P = int(pairs.size)
    # ivf_code_starts_kernel: start[c] = the first sorted pair whose code is >= c, by bisection
    start = [int(x) for x in np.searchsorted(pairs, np.arange(K + 1, dtype=np.int64) << 32, side="left")]
    new_off = [a + b for a, b in zip(old_off, start)]                  # ivf_cut_offsets_kernel on the old offsets
    total = old_off[K] + P
    out = np.full(total, -1, np.int64)
    census = dict(fast=0, slow=0, whole_stores=0, partial_stores=0, max_lists_in_quad=0, alternates=False, longest_gallop=0,
                  last_quad=0, tiles=[], tile_first_list=[], total=total, P=P)
    quads_per_thread = tile // 1024
    assert tile % 1024 == 0 and total > 0

    def old_at(i):
        if not 0 <= i < old_ivf.size:
            raise RouteFault("old_ivf", f"[{i}] of {old_ivf.size}")
        return int(old_ivf[i])

    def pair_at(j):
        if not 0 <= j < P:
            raise RouteFault("pairs", f"[{j}] of {P}")
        return int(pairs[j]) & 0xFFFFFFFF

    for blk in range((total + tile - 1) // tile):
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
                b_new, e_new, b_old, n_old, b_pair = new_off[c], new_off[c + 1], old_off[c], old_off[c + 1] - old_off[c], start[c]
                if tid == 0 and it == 0:
                    r = o - b_new
                    skipped = 0
                    while c - skipped > 0 and new_off[c - skipped - 1] == new_off[c - skipped]:
                        skipped += 1
                    census["tiles"].append(dict(list=c, r=r, n_old=n_old, n_new=e_new - b_new - n_old,
                                                part="old" if r < n_old else "new", empty_lists_before=skipped))
                q = [0, 0, 0, 0]
                bound = b_new + n_old + (1 if defect == "fast_plus" else -1 if defect == "fast_minus" else 0)
                if n == 4 and o + 4 <= bound:
                    census["fast"] += 1
                    q = [old_at(b_old + (o - b_new) + k) for k in range(4)]
                    lists, kinds = {c}, ["old"]
                else:
                    census["slow"] += 1
                    lists, kinds = set(), []
                    for k in range(n):
                        oo = o + k
                        if oo >= e_new:
                            c = _list_of(new_off, K, c, oo, defect, census)
                            b_new, e_new, b_old, n_old, b_pair = (new_off[c], new_off[c + 1], old_off[c],
                                                                  old_off[c + 1] - old_off[c], start[c])
                        r = oo - b_new
                        if r < 0:
                            raise RouteFault("list", f"entry {oo} before list {c}")
                        if r < n_old:
                            q[k] = old_at(b_old + r)
                            kinds.append(("old", c))
                        else:
                            q[k] = pair_at((0 if defect == "no_shift" else b_pair) + (r - n_old))
                            kinds.append(("new", c))
                        lists.add(c)
                    for i in range(len(kinds) - 2):
                        (k0, l0), (k1, l1), (k2, l2) = kinds[i:i + 3]
                        if (k0, k1, k2) == ("old", "new", "old") and l0 == l1 and l2 > l1:
                            census["alternates"] = True
                census["max_lists_in_quad"] = max(census["max_lists_in_quad"], len(lists))
                # the store
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


# ---- what the census is held against: the same facts without the route -----------------------------------------------------
def expected_layout(old_off, pairs, K):
    old_off = np.asarray(old_off, np.int64)
    gain = np.bincount(np.asarray(pairs, np.int64) >> 32, minlength=K)
    new_off = old_off + offsets(gain)
    return new_off, np.diff(old_off), gain


def expected_fast_quads(old_off, pairs, K):
    """quads of 4 entries that lie wholly inside the old part of one list"""
    new_off, n_old, _ = expected_layout(old_off, pairs, K)
    total = int(new_off[K])
    o = np.arange(0, total - 3, 4, dtype=np.int64)
    c = np.searchsorted(new_off, o, side="right") - 1
    return int(np.sum(o + 4 <= new_off[c] + n_old[c]))


def expected_tile_first_lists(old_off, pairs, K, tile=NP_MERGE_TILE):
    new_off, _, _ = expected_layout(old_off, pairs, K)
    o0 = np.arange(0, int(new_off[K]), tile, dtype=np.int64)
    return (np.searchsorted(new_off, o0, side="right") - 1).tolist()


def quad_ends(old_off, pairs, K):
    """(quads that end exactly at the end of an old part with new entries behind it, quads that end one entry past it):
    the two places where the fast path's bound decides"""
    new_off, n_old, gain = expected_layout(old_off, pairs, K)
    total = int(new_off[K])
    o = np.arange(0, total - 3, 4, dtype=np.int64)
    c = np.searchsorted(new_off, o, side="right") - 1
    end = new_off[c] + n_old[c]
    return int(np.sum((o + 4 == end) & (gain[c] > 0))), int(np.sum((o + 4 == end + 1) & (gain[c] > 0) & (o >= new_off[c])))
