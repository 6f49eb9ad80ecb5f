"""numpy f64 restatement of the reference's token pooling, the checker of np_pool.hip.

It follows next-plaid-onnx/src/hierarchy.rs (pdist_cosine :599-653, linkage_ward :128-284 with its nearest-neighbour cache,
fcluster_maxclust :426-517) and src/lib.rs:2249-2317 (pool_embeddings_hierarchical) statement by statement, with the
reference's (2n-1)^2 storage.  Dot products are accumulated feature by feature over all pairs at once: every product of two
f32 values is exact in f64 and the additions happen in feature order, so the bits equal the reference's sequential loop.

Two switches leave the reference on purpose: cut_order = 1 applies the merges in stable order of merge distance (the
dendrogram cut of scipy / PyLate) instead of chain order, and use_cache = False recomputes every nearest neighbour afresh
(only to show that the cache is part of the semantics)."""
import numpy as np

INF = np.inf


def pooled_length(n, pool_factor, protected_tokens=1):
    """lib.rs:2254-2266; pool_factor <= 1 copies through (the C ABI's rule; the reference never calls with less than 2)."""
    if pool_factor <= 1 or n <= protected_tokens + 1:
        return n
    m = n - protected_tokens
    k = max(m // pool_factor, 1)
    return n if k >= m else protected_tokens + k


def pdist_cosine_square(x):
    """hierarchy.rs:599-653 as a full square matrix (entry [i, j] = the condensed entry of the pair)."""
    x64 = np.ascontiguousarray(x, np.float32).astype(np.float64)
    m, dim = x64.shape
    nsq = np.zeros(m, np.float64)
    dot = np.zeros((m, m), np.float64)
    for f in range(dim):
        c = x64[:, f]
        nsq += c * c
        dot += np.multiply.outer(c, c)
    nrm = np.sqrt(nsq)
    ok = (nrm[:, None] > 0.0) & (nrm[None, :] > 0.0)
    den = nrm[:, None] * nrm[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = np.where(ok, dot / den, 0.0)
    return np.clip(1.0 - cos, 0.0, 2.0)


def linkage_ward(dist, use_cache=True):
    """hierarchy.rs:128-284 on a square matrix of distances.  Returns the merges [m - 1, 4] in the order the chain finds them."""
    m = dist.shape[0]
    if m <= 1:
        return np.zeros((0, 4), np.float64)
    tot = 2 * m - 1
    D = np.full((tot, tot), INF, np.float64)
    D[:m, :m] = dist * dist
    D[np.arange(m), np.arange(m)] = 0.0
    sizes = np.ones(tot, np.int64)
    active = np.arange(m)
    nn = np.full(tot, -1, np.int64)
    nnd = np.full(tot, INF, np.float64)

    def find(i):
        others = active[active != i]
        if others.size == 0:
            return -1, INF
        row = D[i, others]
        j = int(np.argmin(row))        # the first minimum of the ascending list: the strict `<` of the reference
        if not row[j] < INF:
            return -1, INF
        return int(others[j]), float(row[j])

    for i in range(m):
        nn[i], nnd[i] = find(i)
    nxt = m
    chain = []
    Z = np.zeros((m - 1, 4), np.float64)
    for r in range(m - 1):
        if not chain:
            chain.append(int(active[0]))
        while True:
            cur = chain[-1]
            if use_cache and nn[cur] != -1:
                c, cd = int(nn[cur]), float(nnd[cur])
            else:
                c, cd = find(cur)
                nn[cur], nnd[cur] = c, cd
            assert c != -1, "no finite neighbour: the reference would index with usize::MAX"
            if len(chain) >= 2 and chain[-2] == c:
                a = chain.pop()
                b = chain.pop()
                na, nb = int(sizes[a]), int(sizes[b])
                Z[r] = (min(a, b), max(a, b), np.sqrt(np.float64(cd)), na + nb)
                active = active[(active != a) & (active != b)]
                sizes[nxt] = na + nb
                if active.size:
                    nk = sizes[active].astype(np.float64)
                    dak, dbk = D[a, active], D[b, active]
                    t1 = (np.float64(na) + nk) * dak
                    t2 = (np.float64(nb) + nk) * dbk
                    t3 = nk * np.float64(cd)
                    new = ((t1 + t2) - t3) / (np.float64(na + nb) + nk)
                    D[nxt, active] = new
                    D[active, nxt] = new
                    stale = (nn[active] == a) | (nn[active] == b)
                    nn[active[stale]] = -1
                active = np.append(active, nxt)
                nn[nxt], nnd[nxt] = find(nxt)
                nxt += 1
                break
            assert len(chain) <= m, "the chain does not terminate"
            chain.append(c)
    return Z


def _first_observation(Z, m, c):
    while c >= m:
        c = int(Z[c - m, 0])
    return c


def fcluster_maxclust(Z, m, k, cut_order=0):
    """hierarchy.rs:426-517: the first m - k rows of the list as it stands (cut_order 0) or of its stable sort by distance
    (cut_order 1); a cluster id is mapped to an observation through the unsorted list, as find_observation_in_cluster does."""
    if k >= m:
        return np.arange(1, m + 1)
    if k == 0:
        return np.ones(m, np.int64)
    rows = np.arange(m - 1) if cut_order == 0 else np.argsort(Z[:, 2], kind="stable")
    parent = list(range(m))

    def root(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for r in rows[: m - k]:
        a = root(_first_observation(Z, m, int(Z[r, 0])))
        b = root(_first_observation(Z, m, int(Z[r, 1])))
        if a != b:
            parent[max(a, b)] = min(a, b)
    labels = np.zeros(m, np.int64)
    seen = {}
    for i in range(m):
        labels[i] = seen.setdefault(root(i), len(seen) + 1)
    return labels


def pool_document(x, pool_factor, protected_tokens=1, cut_order=0, use_cache=True, linkage=None):
    """lib.rs:2249-2317.  Returns (pooled rows f32, labels i32 per input token with 0 = protected / unchanged, linkage or None).
    `linkage`: the document's merges from an earlier call (the other cut order), to save computing them again."""
    x = np.ascontiguousarray(x, np.float32)
    n = x.shape[0]
    if pooled_length(n, pool_factor, protected_tokens) == n:
        return x.copy(), np.zeros(n, np.int32), None
    p = protected_tokens
    m = n - p
    k = max(m // pool_factor, 1)
    tp = x[p:]
    Z = linkage if linkage is not None else linkage_ward(pdist_cosine_square(tp), use_cache)
    lab = fcluster_maxclust(Z, m, k, cut_order)
    out = np.zeros((p + k, x.shape[1]), np.float32)
    out[:p] = x[:p]
    for c in range(k):
        mem = np.nonzero(lab == c + 1)[0]
        s = np.zeros(x.shape[1], np.float32)
        for t in mem:
            s = s + tp[t]
        out[p + c] = s / np.float32(max(mem.size, 1))
    labels = np.zeros(n, np.int32)
    labels[p:] = lab
    return out, labels, Z


def partition_of(labels):
    """A labelling as a canonical partition (labels by first occurrence)."""
    seen = {}
    return np.array([seen.setdefault(int(l), len(seen)) for l in labels])


# ---- corpora ---------------------------------------------------------------------------------------------------------------

def clustered_document(rng, n, dim, n_topics=None, noise=0.35):
    """n unit rows around a few topic directions: token embeddings of a document that has something to pool."""
    if n == 0:
        return np.zeros((0, dim), np.float32)
    t = n_topics or max(1, n // 6)
    cen = rng.standard_normal((t, dim))
    x = cen[rng.integers(0, t, n)] + noise * rng.standard_normal((n, dim))
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    return x.astype(np.float32)


def tied_document(rng, n, dim):
    """A document with duplicated rows, zero rows and rows that differ in the last bit: exact ties and near ties."""
    x = clustered_document(rng, n, dim)
    for _ in range(max(1, n // 5)):
        i, j = rng.integers(0, n, 2)
        x[i] = x[j]
    if n >= 6:
        x[rng.integers(0, n)] = 0.0
        x[rng.integers(0, n)] = 0.0
        i, j = rng.integers(0, n, 2)
        x[i] = x[j]
        x[i].view(np.uint32)[rng.integers(0, dim)] ^= 1
    return x


def lattice_document(rng, n, dim):
    """Rows from a handful of one-hot directions and their pairwise sums: many exactly equal distances."""
    base = np.zeros((6, dim), np.float32)
    for i in range(6):
        base[i, i % dim] = 1.0
    rows = []
    for _ in range(n):
        i, j = rng.integers(0, 6, 2)
        rows.append(base[i] + (base[j] if rng.random() < 0.5 else 0))
    return np.asarray(rows, np.float32)


def cache_sensitive_document(seed=4):
    """A document on which the nearest-neighbour cache decides the result.  Rows are 0 / 3 patterns of equal norm, so equal
    overlaps give bit-equal distances.  The core is five rows w, x, a, b, k: k is equally far from x, a and b, and a and b are
    equally far from each other, so k's cached neighbour is x (the lowest id).  The chain starts at w, walks to a and merges
    (a, b) first.  In exact arithmetic the new cluster is exactly as far from k as x is; in f64 the Lance-Williams update
    (2 q + 2 q - q) / 3 rounds one ulp BELOW q for this q.  The reference keeps k's cached x and merges (x, k); a fresh search
    would take the new cluster.  A protected row in front and a few unrelated rows behind make the cut fall between the two."""
    r = np.random.default_rng(seed)
    j = int(r.integers(1, 8))
    ed = int(r.integers(2, 12))
    core = {"w": [6, 10, 11, 12], "x": [2, 4, 8, 9], "a": [1, 2, 5, 6], "b": [1, 3, 5, 7], "k": [1, 2, 3, 4]}
    dim = 23 + ed
    g = np.zeros((5, dim), np.float32)
    for i, nm in enumerate("wxabk"):
        g[i, core[nm]] = 3.0
        g[i, 13 + 2 * i: 13 + 2 * (i + 1)] = 3.0
    ex = np.zeros((j, dim), np.float32)
    for q in range(j):
        idx = r.choice(np.arange(23, 23 + ed), size=min(ed, int(r.integers(1, 4))), replace=False)
        ex[q, idx] = 3.0
        if r.random() < 0.3:
            ex[q, r.integers(0, 23)] = 3.0
    return np.concatenate([np.ones((1, dim), np.float32), g, ex])


def corpus_document(dim, n):
    """The test corpus' document of n tokens: seeded by (dim, n); some lengths carry ties."""
    rng = np.random.default_rng([dim, n])
    if n % 7 == 3:
        return tied_document(rng, n, dim)
    if n % 11 == 5:
        return lattice_document(rng, n, dim)
    return clustered_document(rng, n, dim)


def gpu_corpus(dim, stride=1, long_doc=True):
    """Lengths 0, stride, 2 stride, ... <= 300 and (long_doc) one ColPali-sized document of 1030 tokens."""
    docs = [corpus_document(dim, n) for n in range(0, 301, stride)]
    if long_doc:
        docs.append(corpus_document(dim, 1030))
    return docs
