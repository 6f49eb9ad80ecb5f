"""numpy restatement of the crate's index update and delete (test infrastructure): delete_from_index (delete.rs:43-398, with
the documented rule that ids outside [0, num_documents) are ignored), update_index (update.rs:771-1120), the mode choice
of MmapIndex::update (index.rs:1431-1590) and find_outliers (update.rs:490-619) with its f64 distances, the device's
recheck window in f64 (outlier_window) and an f32 emulation of its first pass (min_dist_sq_f32).  It reads and
writes directories with numpy and json only (oracle.npy_index.read_index, oracle.encode_tokens) and none of the
product's code."""
import json
import math
import os

import numpy as np

import kmeans_restate as R
from oracle import oracle as O

MERGED = ["merged_codes.npy", "merged_codes.npy.tmp", "merged_codes.manifest.json", "merged_codes.manifest.json.tmp",
          "merged_residuals.npy", "merged_residuals.npy.tmp", "merged_residuals.manifest.json",
          "merged_residuals.manifest.json.tmp"]


def _j(path):
    with open(path) as f:
        return json.load(f)


def _w(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f)


def dir_state(path):
    """Every file of a directory by content: .npy -> (dtype, array bytes), .json -> parsed value, others -> bytes."""
    out = {}
    for f in sorted(os.listdir(path)):
        p = os.path.join(path, f)
        if f.endswith(".npy"):
            a = np.load(p)
            out[f] = (a.dtype.str, a.shape, a.tobytes())
        elif f.endswith(".json"):
            out[f] = _j(p)
        else:
            out[f] = open(p, "rb").read()
    return out


def _remove(path, names):
    for n in names:
        if os.path.exists(os.path.join(path, n)):
            os.remove(os.path.join(path, n))


def _load_flat(path, npy, lengths):
    """load_embeddings_npy / load_buffer (update.rs:127-165, 260-296): whole documents only."""
    if not os.path.exists(os.path.join(path, npy)):
        return []
    flat = np.load(os.path.join(path, npy))
    if not os.path.exists(os.path.join(path, lengths)):
        return [flat]
    docs, off = [], 0
    for n in _j(os.path.join(path, lengths)):
        if off + n > flat.shape[0]:
            break
        docs.append(flat[off:off + n])
        off += n
    return docs


def _save_flat(path, npy, lengths, docs, dim):
    flat = np.concatenate(docs, 0) if docs else np.zeros((0, dim), np.float32)
    np.save(os.path.join(path, npy), flat.astype(np.float32))
    _w(os.path.join(path, lengths), [int(d.shape[0]) for d in docs])


def delete(path, doc_ids, clean_buffer=True):
    meta = _j(os.path.join(path, "metadata.json"))
    n = int(meta["num_documents"])
    dele = sorted({int(i) for i in doc_ids if 0 <= int(i) < n})
    ds = set(dele)
    doc0, final_docs, total, gone = 0, 0, 0, 0
    for c in range(int(meta["num_chunks"])):
        dl = _j(os.path.join(path, f"doclens.{c}.json"))
        keep_doc = [doc0 + i not in ds for i in range(len(dl))]
        ndl = [l for l, k in zip(dl, keep_doc) if k]
        gone += len(dl) - len(ndl)
        if len(ndl) < len(dl):
            mask = np.repeat(np.array(keep_doc, bool), dl) if dl else np.zeros(0, bool)
            codes = np.load(os.path.join(path, f"{c}.codes.npy"))
            res = np.load(os.path.join(path, f"{c}.residuals.npy"))
            np.save(os.path.join(path, f"{c}.codes.npy"), codes[mask])
            np.save(os.path.join(path, f"{c}.residuals.npy"), res[mask])
            _w(os.path.join(path, f"doclens.{c}.json"), ndl)
            cm = _j(os.path.join(path, f"{c}.metadata.json"))
            cm["num_documents"], cm["num_embeddings"] = len(ndl), int(mask.sum())
            _w(os.path.join(path, f"{c}.metadata.json"), cm)
        final_docs += len(ndl)
        total += sum(ndl)
        doc0 += len(dl)
    ivf = np.load(os.path.join(path, "ivf.npy"))
    il = np.load(os.path.join(path, "ivf_lengths.npy")).astype(np.int32)
    darr = np.asarray(dele, np.int64)
    out, lens, off = [], [], 0
    for l in il:
        seg = ivf[off:off + l]
        off += l
        seg = seg[~np.isin(seg, darr)]
        out.append(seg - np.searchsorted(darr, seg, side="left"))
        lens.append(seg.size)
    np.save(os.path.join(path, "ivf.npy"), np.concatenate(out).astype(np.int64) if out else np.zeros(0, np.int64))
    np.save(os.path.join(path, "ivf_lengths.npy"), np.asarray(lens, np.int32))
    meta.update(num_embeddings=total, num_documents=final_docs, avg_doclen=total / final_docs if final_docs else 0.0)
    _w(os.path.join(path, "metadata.json"), meta)
    _remove(path, MERGED)
    if clean_buffer:
        for npy, lengths, info, base in (("embeddings.npy", "embeddings_lengths.json", None, 0),
                                         ("buffer.npy", "buffer_lengths.json", "buffer_info.json", None)):
            if not (os.path.exists(os.path.join(path, npy)) and os.path.exists(os.path.join(path, lengths))):
                continue
            docs = _load_flat(path, npy, lengths)
            b = n - len(_j(os.path.join(path, lengths))) if base is None else 0
            kept = [d for i, d in enumerate(docs) if b + i not in ds]
            if kept:
                _save_flat(path, npy, lengths, kept, docs[0].shape[1])
                if info:
                    _w(os.path.join(path, info), {"num_docs": len(kept)})
            else:
                _remove(path, [npy, lengths] + ([info] if info else []))
    return gone


def residual_norms(flat, centroids, codes):
    """|x - c[code]| with a sequential f32 sum of squares (the library's one rule for both thresholds)"""
    r = (flat - centroids[codes]).astype(np.float32)
    if r.shape[0] == 0:
        return np.zeros(0, np.float32)
    return np.sqrt(np.cumsum(r * r, axis=1, dtype=np.float32)[:, -1]).astype(np.float32)


def update_index(path, docs, batch_size, update_threshold):
    """update_index (update.rs:771-1120) with the directory's own codec; returns the new codes."""
    meta = _j(os.path.join(path, "metadata.json"))
    nbits, old_n, old_t = int(meta["nbits"]), int(meta["num_documents"]), int(meta["num_embeddings"])
    cen = np.load(os.path.join(path, "centroids.npy"))
    cut = np.load(os.path.join(path, "bucket_cutoffs.npy"))
    K, dim = cen.shape
    start, cur = int(meta["num_chunks"]), old_t
    append = False
    if start > 0 and os.path.exists(os.path.join(path, f"{start - 1}.metadata.json")):
        lm = _j(os.path.join(path, f"{start - 1}.metadata.json"))
        if lm["num_documents"] < 2000:
            start, append = start - 1, True
            cur = lm["embedding_offset"] if "embedding_offset" in lm else old_t - lm["num_embeddings"]
    lens = np.array([d.shape[0] for d in docs], np.int64)
    flat = np.concatenate(docs, 0) if len(docs) else np.zeros((0, dim), np.float32)
    codes, packed = O.encode_tokens(flat, cen, nbits, cut) if flat.shape[0] else (np.zeros(0, np.int64),
                                                                                   np.zeros((0, dim * nbits // 8), np.uint8))
    off = np.concatenate([[0], np.cumsum(lens)])
    nchunks = math.ceil(len(docs) / batch_size)
    for i in range(nchunks):
        c, d0, d1 = start + i, i * batch_size, min(len(docs), (i + 1) * batch_size)
        cl, cc, cr = lens[d0:d1].tolist(), codes[off[d0]:off[d1]], packed[off[d0]:off[d1]]
        if i == 0 and append:
            cl = _j(os.path.join(path, f"doclens.{c}.json")) + cl
            cc = np.concatenate([np.load(os.path.join(path, f"{c}.codes.npy")), cc])
            cr = np.concatenate([np.load(os.path.join(path, f"{c}.residuals.npy")), cr])
        np.save(os.path.join(path, f"{c}.codes.npy"), cc.astype(np.int64))
        np.save(os.path.join(path, f"{c}.residuals.npy"), cr.astype(np.uint8))
        _w(os.path.join(path, f"doclens.{c}.json"), [int(x) for x in cl])
        _w(os.path.join(path, f"{c}.metadata.json"),
           {"num_documents": len(cl), "num_embeddings": int(cc.size), "embedding_offset": int(cur)})
        cur += cc.size
    if update_threshold and codes.size:
        q = R.quantile(np.sort(residual_norms(flat, cen, codes)), 0.75)
        tp = os.path.join(path, "cluster_threshold.npy")
        if os.path.exists(tp):
            o = np.load(tp)[0]
            q = (o * np.float32(old_t) + q * np.float32(codes.size)) / np.float32(old_t + codes.size)
        np.save(tp, np.array([q], np.float32))
    ivf = np.load(os.path.join(path, "ivf.npy"))
    il = np.load(os.path.join(path, "ivf_lengths.npy")).astype(np.int64)
    oo = np.concatenate([[0], np.cumsum(il)])
    new = {}
    for d in range(len(docs)):
        for c in np.unique(codes[off[d]:off[d + 1]]):
            new.setdefault(int(c), []).append(old_n + d)
    out, nl = [], []
    for c in range(K):
        old = ivf[oo[c]:oo[c + 1]] if c < il.size else np.zeros(0, np.int64)
        lst = np.unique(np.concatenate([old, np.asarray(new.get(c, []), np.int64)]))
        out.append(lst)
        nl.append(lst.size)
    np.save(os.path.join(path, "ivf.npy"), np.concatenate(out).astype(np.int64))
    np.save(os.path.join(path, "ivf_lengths.npy"), np.asarray(nl, np.int32))
    total = old_n + len(docs)
    meta.update(num_chunks=start + nchunks, num_partitions=K, num_embeddings=old_t + int(lens.sum()),
                avg_doclen=(meta["avg_doclen"] * old_n + float(lens.sum())) / total if total else 0.0,
                num_documents=total, embedding_dim=dim, next_plaid_compatible=True)
    _w(os.path.join(path, "metadata.json"), meta)
    _remove(path, MERGED)
    return codes


def mode(path, n_new, start_from_scratch=999, buffer_size=100):
    """The crate's choice in MmapIndex::update: 'scratch', 'buffer' or 'expansion'."""
    n = int(_j(os.path.join(path, "metadata.json"))["num_documents"])
    if n <= start_from_scratch and len(_load_flat(path, "embeddings.npy", "embeddings_lengths.json")) == n:
        return "scratch"
    buffered = len(_load_flat(path, "buffer.npy", "buffer_lengths.json"))
    return "expansion" if n_new + buffered >= buffer_size else "buffer"


def min_dist_sq_precise(flat, centroids, block=256):
    """min_distance_sq_precise (update.rs:457-473): per centroid the f64 sum over dims in order, cast to f32, minimum"""
    c = centroids.astype(np.float64)
    out = np.empty(flat.shape[0], np.float32)
    for i in range(0, flat.shape[0], block):
        x = flat[i:i + block].astype(np.float64)
        diff = x[:, None, :] - c[None, :, :]
        s = np.cumsum(diff * diff, axis=2)[:, :, -1]
        out[i:i + block] = s.astype(np.float32).min(axis=1)
    return out


def find_outliers(flat, centroids, thr):
    """the outlier set this library computes: f32(min_c f64 |x - c|^2) > thr^2 (f32)"""
    thr2 = np.float32(thr) * np.float32(thr)
    return np.nonzero(min_dist_sq_precise(flat, centroids) > thr2)[0]


def storage_dim(dim):
    """the device's row width: dim rounded up to a multiple of 32 (zero padded)"""
    return (dim + 31) // 32 * 32


def min_dist_sq_f64(flat, centroids, block=256):
    """min_c |x - c|^2 in f64, not rounded to f32: the quantity the outlier window is measured around"""
    c = centroids.astype(np.float64)
    out = np.empty(flat.shape[0], np.float64)
    for i in range(0, flat.shape[0], block):
        diff = flat[i:i + block].astype(np.float64)[:, None, :] - c[None, :, :]
        out[i:i + block] = (diff * diff).sum(2).min(1)
    return out


def outlier_window(flat, centroids, thr):
    """The window of the device's first pass, restated in f64: a token whose f32 minimum d has |d - thr^2| <= w goes to
    the f64 recheck.  w = max(max(thr^2, 1) 1e-5, 4 (Dp + 2) 2^-24 (|x|^2 + 1.001 max |c|^2)), Dp the storage dim."""
    thr2 = float(np.float32(thr) * np.float32(thr))
    xn = (flat.astype(np.float64) ** 2).sum(1)
    cn = (centroids.astype(np.float64) ** 2).sum(1).max() * (1.0 + 1e-3)
    rel = 4.0 * (storage_dim(flat.shape[1]) + 2) * 2.0 ** -24
    return np.maximum(max(abs(thr2), 1.0) * 1e-5, rel * (xn + cn))


def _fma32(a, b, c):
    """fmaf on f32 arrays: the product of two f32 values is exact in f64, so one f64 addition and one rounding follow"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def min_dist_sq_f32(flat, centroids):
    """An f32 emulation of the first pass, min_c max(fma(-2, x.c, |x|^2 + |c|^2), 0), with |x|^2, |c|^2 and x.c as
    sequential FMA chains over the dims.  The kernel sums x.c in the MFMA's order, so this is the formula and the
    precision, not the kernel."""
    x, c = flat.astype(np.float32), centroids.astype(np.float32)
    xn, cn = np.zeros(x.shape[0], np.float32), np.zeros(c.shape[0], np.float32)
    dot = np.zeros((x.shape[0], c.shape[0]), np.float32)
    for j in range(x.shape[1]):
        xn = _fma32(x[:, j], x[:, j], xn)
        cn = _fma32(c[:, j], c[:, j], cn)
        dot = _fma32(x[:, j, None], c[None, :, j], dot)
    s = (xn[:, None] + cn[None, :]).astype(np.float32)
    return np.maximum(_fma32(np.float32(-2), dot, s), np.float32(0)).min(1)


def k_update(n_out, max_points_per_centroid):
    return min(max(1, math.ceil(n_out / max_points_per_centroid)) * 4, n_out)
