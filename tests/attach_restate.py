"""Columns and groups through a resident remove and append, restated (np_index.hip attach_compact_kernel and its kin,
np_attach_plan.h).

Two things live here.  The numpy restatement of what a keeping call leaves -- shrunk = arr[keep], validity likewise (no bitmap
where no survivor is NULL), a dictionary remap over the rows that are not NULL, the new rows appended, the code range as
np_hip_index_set_columns takes it -- which the GPU tests compare the read-back arrays with.  And a plain-Python replay of the
kernel's own rules -- the select of a survivor's source (a bisection of the words' kept-count prefix, then the k-th set bit),
the wave's validity ballot cut into two u32 words, the tail merge of an append's validity bits -- each with a planted defect
that a named case rejects.  Pure host code."""
import numpy as np

SIZES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4097, 32769]   # the document counts the remove is checked at


def patterns(n, seed=3):
    """name -> keep mask: the GPU test's patterns, where the count has room for them"""
    rng = np.random.default_rng(seed + n)
    idx = np.arange(n)
    p = {"none": np.ones(n, bool), "first": idx != 0, "last": idx != n - 1, "every other": idx % 2 == 1,
         "all but one": idx == n // 2, "all": np.zeros(n, bool), "last word only": idx >= (n - 1) // 64 * 64,
         "random tenth": rng.random(n) >= 0.1}
    if n > 128:
        p["one whole word"] = ~((idx >= 64) & (idx < 128))
    if n > 400:
        p["a run longer than 256"] = ~((idx >= 70) & (idx < 400))
    return p


# ---- the numpy restatement --------------------------------------------------------------------------------------------------
def keep_mask(n_docs, removed):
    keep = np.ones(int(n_docs), bool)
    ids = np.asarray(removed, np.int64).reshape(-1)
    keep[ids[(ids >= 0) & (ids < n_docs)]] = False
    return keep


def code_range(codes):
    """(min_code, max_code) as np_hip_index_set_columns folds every row into its start values 0 and -1"""
    c = np.asarray(codes, np.int64)
    return (min(0, int(c.min())), max(-1, int(c.max()))) if c.size else (0, -1)


def _no_bitmap_if_full(valid):
    return None if valid is None or valid.all() else np.ascontiguousarray(valid, np.uint8)


def shrunk_column(data, valid, keep):
    """(data, valid) of the survivors; valid is None where none of them is NULL"""
    return np.ascontiguousarray(data[keep]), _no_bitmap_if_full(None if valid is None else valid[keep])


def appended_column(data, valid, new_data, new_valid, remap=None):
    """(data, valid) after an append: the remap moves the old rows that are not NULL, the new rows follow; a NaN is NULL"""
    data = np.array(data, copy=True)
    if remap is not None:
        live = np.ones(data.size, bool) if valid is None else valid.astype(bool)
        data[live] = np.asarray(remap, data.dtype)[data[live]]
    new_data = np.asarray(new_data, data.dtype)
    nv = np.ones(new_data.size, np.uint8) if new_valid is None else np.asarray(new_valid, np.uint8).copy()
    if data.dtype == np.float64:
        nv &= ~np.isnan(new_data)
    ov = np.ones(data.size, np.uint8) if valid is None else valid
    return np.concatenate([data, new_data]), _no_bitmap_if_full(np.concatenate([ov, nv]))


# ---- the kernel's select, replayed ------------------------------------------------------------------------------------------
def keep_words(keep):
    """(bits, wrank): one u64 per 64 documents, bit = the document stays, the bits past n_docs SET; the removed documents in
    front of each word -- what keep_bitmap_kernel and the scan behind it leave"""
    n = len(keep)
    W = (n + 63) // 64
    bits, wrank, gone = [], [], 0
    for w in range(W):
        word = 0
        for b in range(64):
            d = 64 * w + b
            if d >= n or keep[d]:
                word |= 1 << b
        bits.append(word)
        wrank.append(gone)
        gone += 64 - bin(word).count("1")
    return bits, wrank


def select_word(wrank, n_words, j, defect=None):
    """the first w in [0, n_words - 1) with 64 (w + 1) - wrank[w + 1] >= j + 1, or the last word"""
    a, z = 0, n_words - 1
    while a < z:
        mid = (a + z) >> 1
        ends = 64 * (mid + 1) - wrank[mid + 1]
        if (ends <= j + 1) if defect == "upper_bound" else (ends < j + 1):
            a = mid + 1
        else:
            z = mid
    return a


def select_bit(word, k, defect=None):
    """the position of the k-th set bit (from 0), by halves"""
    pos, s = 0, 32
    while s > 0:
        c = bin(word & ((1 << s) - 1)).count("1")
        if (k > c) if defect == "kth_bit" else (k >= c):
            k -= c
            word >>= s
            pos += s
        s >>= 1
    return pos


def select_sources(keep, defect=None):
    """the old id of every survivor, by new id, as the kernel's lanes find it"""
    bits, wrank = keep_words(keep)
    out = []
    for j in range(int(np.count_nonzero(keep))):
        w = select_word(wrank, len(bits), j, defect)
        out.append(64 * w + select_bit(bits[w], j - (64 * w - wrank[w]), defect))
    return np.array(out, np.int64)


def ballot_words(valid_bits, defect=None):
    """the new bitmap's u32 words from the waves' ballots: a wave owns 64 new ids, lanes past the last survivor vote 0, the
    ballot leaves as two words of which only those that hold a document are written"""
    n = len(valid_bits)
    out = np.zeros((n + 31) // 32, np.uint32)
    for base in range(0, n, 64):
        ballot = 0
        for lane in range(64):
            if base + lane < n and valid_bits[base + lane]:
                ballot |= 1 << lane
        halves = (ballot & 0xFFFFFFFF, ballot >> 32)
        if defect == "ballot_half":
            halves = halves[::-1]
        for h in (0, 1):
            if base // 32 + h < out.size:
                out[base // 32 + h] = halves[h]
    return out


def bitmap_words(valid_bits):
    """the bitmap np_hip_index_set_columns uploads: bit d of word d / 32, nothing set past the last document"""
    v = np.asarray(valid_bits, bool)
    pad = np.zeros((-len(v)) % 32, bool)
    return np.packbits(np.concatenate([v, pad]), bitorder="little").view(np.uint32).copy()


def tail_merge(old_words, n_old, new_valid_bits, fresh, defect=None, garbage=0):
    """the bitmap after an append: the new rows' bits at their final positions, the word the old last document shares MERGED --
    the old rows' bits kept (all ones where the column had no bitmap), the new ones OR-ed in, whatever lay past the old count
    (`garbage`, for a test) not trusted"""
    n_new = len(new_valid_bits)
    n1 = n_old + n_new
    w0, shared = n_old >> 5, n_old & 31
    out = np.zeros((n1 + 31) // 32, np.uint32)
    out[:w0] = 0xFFFFFFFF if fresh else np.asarray(old_words[:w0], np.uint32)
    tail = np.zeros(out.size - w0, np.uint32)
    for i, ok in enumerate(new_valid_bits):
        if ok:
            d = n_old + i
            tail[(d >> 5) - w0] |= np.uint32(1 << (d & 31))
    if tail.size:
        low = (1 << shared) - 1
        old = 0xFFFFFFFF if fresh else (int(old_words[w0]) | (garbage & ~low & 0xFFFFFFFF) if shared else 0)
        first = int(tail[0]) if defect == "overwrite" else (old & low) | (int(tail[0]) & ~low & 0xFFFFFFFF)
        out[w0:] = tail
        out[w0] = first
    return out
