"""np_hip_index_remove restated in numpy: the arrays of an index without some of its documents, and the slab schedule of the
in-place token move (next-plaid_amd/csrc/np_remove_plan.h) with a replay of its launches on a byte array.

shrunk_arrays filters and renumbers the base's OWN posting lists (delete.rs:43-268 as np_hip_index_delete applies it: ids out
of range ignored, duplicates once) -- it does not rebuild lists from the codes, so lists that are permuted, miss a pair or hold
an extra one keep their shape.  tests/test_index_remove_cpu.py pins it to np_hip_index_delete; the planted defects of
`defect=` are what that file's named cases reject."""
import numpy as np

DIRECT, GATHER, COPY = 0, 1, 2


def removed_ids(ids, n_docs):
    """the ids a remove acts on: in range, ascending, each once"""
    ids = np.asarray(ids, np.int64).reshape(-1)
    return np.unique(ids[(ids >= 0) & (ids < n_docs)])


def new_ids(old, removed, defect=None):
    """surviving ids renumbered: d minus the removed ids BELOW d"""
    side = "right" if defect == "upper_bound" else "left"
    return np.asarray(old, np.int64) - np.searchsorted(removed, old, side=side)


def rank_by_words(removed, n_docs, d, defect=None):
    """the device's rank(d): the removed documents in front of d's 64-document word plus a popcount inside the word"""
    keep = np.ones((n_docs + 63) // 64 * 64, bool)
    keep[removed] = False
    words = keep.reshape(-1, 64)
    gone = 64 - words.sum(1)
    wrank = np.concatenate([[0], np.cumsum(gone)[:-1]])
    d = np.asarray(d, np.int64)
    w, b = d >> 6, d & 63
    inside = np.array([int((~words[wi, :bi]).sum()) for wi, bi in zip(w, b)], np.int64)
    if defect == "word_edge":   # a word's first document read as bit 64 of the word before, whose mask is empty: that word is lost
        w = np.where((b == 0) & (w > 0), w - 1, w)
    return wrank[w] + inside


def shrunk_arrays(base, ids, defect=None):
    """the arrays of `base` (centroids, bucket_weights, nbits, doc_lengths, codes, residuals, ivf, ivf_lengths) without the
    documents `ids`"""
    lens = np.asarray(base["doc_lengths"], np.int64)
    n = lens.size
    rem = removed_ids(ids, n)
    keep = np.ones(n, bool)
    keep[rem] = False
    tok_keep = np.repeat(keep, lens)
    ivf = np.asarray(base["ivf"], np.int64)
    il = np.asarray(base["ivf_lengths"])
    list_of = np.repeat(np.arange(il.size), il)
    stay = keep[ivf]
    out = dict(base)
    out["doc_lengths"] = lens[keep]
    out["codes"] = np.asarray(base["codes"])[tok_keep]
    out["residuals"] = np.asarray(base["residuals"])[tok_keep]
    out["ivf"] = new_ids(ivf[stay], rem, defect)
    out["ivf_lengths"] = np.bincount(list_of[stay], minlength=il.size).astype(il.dtype)
    return out


# ---- the slab schedule ----------------------------------------------------------------------------------------------------------
def plan(off, keep, slab, defect=None):
    """np_remove_plan.h remove_plan: (launches, first_moved, new_tokens, staging_rows); a launch is (mode, src0, src1, dst0, dst1)
    in tokens.  The moved range [first removed token, T) is cut into slabs of `slab` SOURCE tokens; a slab's
    survivors go to [d0, d1), DIRECT when d1 <= f (their first source token), else through the staging buffer"""
    off = np.asarray(off, np.int64)
    keep = np.asarray(keep, bool)
    n, T = keep.size, int(off[-1])
    gone = np.flatnonzero(~keep & (np.diff(off) > 0))   # a removed document without tokens moves nothing
    first = int(off[gone[0]]) if gone.size else T
    tok_keep = np.repeat(keep, np.diff(off))
    kept_before = np.concatenate([[0], np.cumsum(tok_keep)])   # [T + 1]
    launches, staging = [], 0
    for s0 in range(first, T, slab):
        s1 = min(T, s0 + slab)
        src = s0 + np.flatnonzero(tok_keep[s0:s1])
        if src.size == 0:
            continue
        f, l = int(src[0]), int(src[-1]) + 1
        d0, d1 = int(kept_before[s0]), int(kept_before[s1])
        if defect == "shift_at_end":   # the destination from the shift at the slab's END: every survivor lands too low
            shift = s1 - int(kept_before[s1])
            d0, d1 = f - shift, f - shift + src.size
        direct = d1 <= f + 1 if defect == "le_for_lt" else d1 <= f   # i.e. last destination < first source
        if direct:
            launches.append((DIRECT, f, l, d0, d1))
        else:
            launches += [(GATHER, f, l, d0, d1), (COPY, f, l, d0, d1)]
            staging = max(staging, src.size)
    return launches, first, int(kept_before[T]), staging


def replay(launches, off, keep, row, staging_rows, data):
    """run the launches on `data` (u8 [T * row]) the way the device does -- a launch reads all it reads before it writes -- and
    check the schedule's promises: no launch reads an array byte that it writes itself, and the staging buffer is never
    exceeded.  Returns the array after the last launch"""
    off = np.asarray(off, np.int64)
    tok_keep = np.repeat(np.asarray(keep, bool), np.diff(off))
    a = np.array(data, np.uint8).reshape(-1, row)
    stage = np.zeros((max(staging_rows, 1), row), np.uint8)
    staged = 0
    for mode, s0, s1, d0, d1 in launches:
        src = s0 + np.flatnonzero(tok_keep[s0:s1])
        assert src.size == d1 - d0, "a launch's survivors are not its destination"
        assert 0 <= d0 <= d1 <= a.shape[0], f"a launch writes [{d0}, {d1}) of {a.shape[0]} tokens: outside the array"
        if mode == DIRECT:
            assert d1 <= src[0], f"a direct launch writes [{d0}, {d1}) and reads from {src[0]}"
            a[d0:d1] = a[src].copy()
        elif mode == GATHER:
            assert src.size <= staging_rows, "the staging buffer is exceeded"
            stage[:src.size] = a[src]
            staged = src.size
        else:
            assert staged == d1 - d0, "a copy without its gather"
            a[d0:d1] = stage[:staged]
    return a.reshape(-1)
