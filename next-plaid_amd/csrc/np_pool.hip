// np_pool.hip -- token pooling of document embeddings on the GPU: pool_document_embeddings (next-plaid-onnx/src/lib.rs:1632-1643)
// -> pool_embeddings_hierarchical (lib.rs:2249-2317) -> hierarchy.rs pdist_cosine (:599-653), Ward linkage by nearest-neighbour
// chain (:128-284) and fcluster_maxclust (:426-517), restated bit for bit ("Token pooling").
//
// Three stages per chunk of documents, every f64 operation on the VALU:
//   pool_norms_kernel / pool_dist_kernel   f64 norms and dot products as sequential sums in feature order (each lane owns whole
//                                          pairs; the product of two f32 values is exact in f64, so the FMA equals mul-then-add),
//                                          d = clamp(1 - dot / (ni nj), 0, 2), the matrix of d * d into a per-document scratch
//   pool_linkage_kernel                    one workgroup per document: the chain and merge loop with the reference's
//                                          nearest-neighbour cache, the cut (chain order or stable order by distance), the labels
//   pool_means_kernel                      per cluster the f32 sum of its members in token order over the count
// The whole file is compiled without floating-point contraction (pragma below and -ffp-contract=off in the Makefile): outside
// the explicit fma() of the dot products no product and sum are fused, as the reference's scalar code does not fuse them.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "np_internal.h"

#pragma clang fp contract(off)

namespace np {

#define NP_POOL_MAX_TOKENS 2048   // tokens one document may hand to the clustering (its length minus the protected tokens)
#define NP_POOL_LDS_MAX 136       // ... up to which the distance matrix is held in LDS: (m | 1) m 8 B + 44 m B + 128 B <= 160 KB
#define NP_POOL_TILE 64           // rows per side of a distance tile
#define NP_POOL_FEAT 16           // features staged per step

struct PoolDoc {
  int64_t row0;      // first clustered row of the document in the chunk's embeddings (after the protected rows)
  int64_t d_off;     // its matrix in the scratch (doubles), m rows of ld
  int64_t link_off;  // its first merge row in the chunk's linkage (rows of 4 doubles)
  int64_t lab_off;   // its first label in the chunk's labels
  int64_t out_off;   // its first cluster row in the chunk's output
  int32_t m, k, ld, pad;
};

// ---- distances -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void pool_norms_kernel(const float* __restrict__ X, int dim, int64_t nrows,
                                                         double* __restrict__ norms) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nrows) return;
  const float* x = X + r * dim;
  double s = 0.0;
  for (int f = 0; f < dim; ++f) {
    const double v = (double)x[f];
    s = fma(v, v, s);   // v * v is exact: the same bits as norm_sq += v * v
  }
  norms[r] = sqrt(s);
}

// One 64 x 64 tile of one document's matrix per workgroup; a thread owns 4 x 4 pairs and walks the features in order.  The
// full square is computed: a * b and ni * nj commute exactly, so D[i][j] and D[j][i] carry the same bits without a transposed
// (scattered) store.
__global__ __launch_bounds__(256) void pool_dist_kernel(const float* __restrict__ X, int dim, const double* __restrict__ norms,
                                                        const PoolDoc* __restrict__ docs, const int4* __restrict__ tiles,
                                                        double* __restrict__ D) {
  __shared__ float A[NP_POOL_TILE][NP_POOL_FEAT + 1], B[NP_POOL_TILE][NP_POOL_FEAT + 1];
  const int4 t = tiles[blockIdx.x];
  const PoolDoc pd = docs[t.x];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = t.y * NP_POOL_TILE, j0 = t.z * NP_POOL_TILE, m = pd.m;
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
  for (int f0 = 0; f0 < dim; f0 += NP_POOL_FEAT) {
    const int nf = min(NP_POOL_FEAT, dim - f0);
    __syncthreads();
    for (int e = tid; e < NP_POOL_TILE * NP_POOL_FEAT; e += 256) {
      const int r = e / NP_POOL_FEAT, f = e % NP_POOL_FEAT;
      float va = 0.f, vb = 0.f;
      if (f < nf) {
        if (i0 + r < m) va = X[(pd.row0 + i0 + r) * dim + f0 + f];
        if (j0 + r < m) vb = X[(pd.row0 + j0 + r) * dim + f0 + f];
      }
      A[r][f] = va;
      B[r][f] = vb;
    }
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = (double)A[ty * 4 + u][f];
#pragma unroll
      for (int v = 0; v < 4; ++v) b[v] = (double)B[tx + 16 * v][f];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = i0 + ty * 4 + u;
    if (i >= m) continue;
    const double ni = norms[pd.row0 + i];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = j0 + tx + 16 * v;
      if (j >= m) continue;
      const double nj = norms[pd.row0 + j];
      double cs = 0.0;
      if (ni > 0.0 && nj > 0.0) {
        const double den = ni * nj;
        cs = acc[u][v] / den;
      }
      double d = 1.0 - cs;
      d = d < 0.0 ? 0.0 : (d > 2.0 ? 2.0 : d);
      D[pd.d_off + (int64_t)i * pd.ld + j] = d * d;
    }
  }
}

// ---- linkage ---------------------------------------------------------------------------------------------------------------

// The strict minimum of (d, id) over the block's candidates: equal distances go to the lowest cluster id, which is what the
// reference's `<` over its ascending active list gives.  Every thread returns the same (d, slot); slot -1 = no candidate.
__device__ __forceinline__ void pool_argmin(double& d, int& id, int& slot, double* redd, int* redi) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double od = __shfl_xor(d, o);
    const int oi = __shfl_xor(id, o), os = __shfl_xor(slot, o);
    if (od < d || (od == d && oi < id)) {
      d = od;
      id = oi;
      slot = os;
    }
  }
  const int nw = blockDim.x >> 6;
  if (nw > 1) {
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
      redd[w] = d;
      redi[2 * w] = id;
      redi[2 * w + 1] = slot;
    }
    __syncthreads();
    d = redd[0];
    id = redi[0];
    slot = redi[1];
    for (int x = 1; x < nw; ++x) {
      const double od = redd[x];
      const int oi = redi[2 * x], os = redi[2 * x + 1];
      if (od < d || (od == d && oi < id)) {
        d = od;
        id = oi;
        slot = os;
      }
    }
  }
}

#define NP_POOL_NOID 0x7fffffff

// One workgroup per document.  The matrix keeps m slots: a merged pair's new cluster takes the slot of the chain's top and
// the other slot goes idle, every slot carries its cluster id (the reference's (2n-1)^2 storage is not semantics).  The
// nearest-neighbour cache IS semantics (hierarchy.rs:153-247): an entry is recomputed only for the new cluster and for a
// cluster whose cached neighbour was one of the two just merged.
template <bool LDSMAT>
__global__ void pool_linkage_kernel(const PoolDoc* __restrict__ docs, const int32_t* __restrict__ order, double* Dg,
                                    double* __restrict__ link, int32_t* __restrict__ labels, int cut_order, int mcap,
                                    int32_t* __restrict__ err) {
  extern __shared__ double pool_smem[];
  const PoolDoc pd = docs[order[blockIdx.x]];
  const int m = pd.m, ld = pd.ld, T = blockDim.x, tid = threadIdx.x;
  double* nnd = pool_smem;          // [mcap] cached neighbour distance (squared)
  double* mdist = nnd + mcap;       // [mcap] merge distances
  double* redd = mdist + mcap;      // [8]
  int* id = (int*)(redd + 8);       // [mcap] cluster id of the slot, -1 = idle
  int* sz = id + mcap;              // [mcap]
  int* nns = sz + mcap;             // [mcap] cached neighbour SLOT, -1 = invalid
  int* chain = nns + mcap;          // [mcap]
  int* rep = chain + mcap;          // [mcap] the observation find_observation_in_cluster reaches from the slot's cluster
  int* mr1 = rep + mcap;            // [mcap] per merge: that observation for the lower id ...
  int* mr2 = mr1 + mcap;            // [mcap] ... and for the higher id
  int* redi = mr2 + mcap;           // [16]
  double* D = LDSMAT ? (double*)(redi + 16) : Dg + pd.d_off;
  if (LDSMAT) {
    const double* src = Dg + pd.d_off;
    for (int e = tid; e < m * ld; e += T) D[e] = src[e];
  }
  for (int s = tid; s < m; s += T) {
    id[s] = s;
    sz[s] = 1;
    rep[s] = s;
  }
  __syncthreads();
  for (int s = tid; s < m; s += T) {   // D[t][s] == D[s][t] bit for bit: the column read is the coalesced one
    double bd = INFINITY;
    int bs = -1;
    for (int t = 0; t < m; ++t) {
      if (t == s) continue;
      const double d = D[(int64_t)t * ld + s];
      if (d < bd) {
        bd = d;
        bs = t;
      }
    }
    nns[s] = bs;
    nnd[s] = bd;
  }
  __syncthreads();

  int next_id = m, len = 0, cur = -1, prev = -1, lo = 0;
  double* lrow = link + pd.link_off * 4;
  for (int r = 0; r < m - 1; ++r) {
    if (len == 0) {   // a chain starts at the lowest active id: an original sits in its own slot, new ids are all larger
      while (lo < m && id[lo] != lo) ++lo;
      if (lo < m) {
        cur = lo;
      } else {
        double d = 0.0;
        int bi = NP_POOL_NOID, bs = -1;
        for (int s = tid; s < m; s += T) {
          const int i = id[s];
          if (i >= 0 && i < bi) {
            bi = i;
            bs = s;
          }
        }
        pool_argmin(d, bi, bs, redd, redi);
        cur = bs;
        if (cur < 0) {
          if (tid == 0) *err = 1;
          return;
        }
      }
      if (tid == 0) chain[0] = cur;
      prev = -1;
      len = 1;
    }
    double nd;
    for (;;) {
      int nn = nns[cur];
      nd = nnd[cur];
      if (nn < 0) {
        double d = INFINITY;
        int bi = NP_POOL_NOID, bs = -1;
        for (int t = tid; t < m; t += T) {
          const int i = id[t];
          if (i < 0 || t == cur) continue;
          const double v = D[(int64_t)cur * ld + t];
          if (v < d || (v == d && i < bi)) {
            d = v;
            bi = i;
            bs = t;
          }
        }
        pool_argmin(d, bi, bs, redd, redi);
        nn = bs;
        nd = d;
        if (tid == 0) {
          nns[cur] = nn;
          nnd[cur] = nd;
        }
        __syncthreads();   // a later step of this walk may come back to `cur`
      }
      if (len >= 2 && prev == nn) break;
      if (len >= m || nn < 0) {   // a cycle of stale cache entries: the reference's chain grows without end on such a document
        if (tid == 0) *err = 1;
        return;
      }
      if (tid == 0) chain[len] = nn;
      prev = cur;
      cur = nn;
      ++len;
    }
    // merge the chain's top two
    const int a = cur, b = prev;
    const double dab = nd;
    __syncthreads();   // thread 0's cache and chain writes of this walk
    const int na = sz[a], nb = sz[b], ida = id[a], idb = id[b];
    const int newrep = ida < idb ? rep[a] : rep[b];
    if (tid == 0) {
      const double dist = sqrt(dab);
      lrow[4 * r + 0] = (double)min(ida, idb);
      lrow[4 * r + 1] = (double)max(ida, idb);
      lrow[4 * r + 2] = dist;
      lrow[4 * r + 3] = (double)(na + nb);
      mdist[r] = dist;
      mr1[r] = newrep;
      mr2[r] = ida < idb ? rep[b] : rep[a];
    }
    for (int k = tid; k < m; k += T) {
      if (k == a || k == b || id[k] < 0) continue;
      const int nk = sz[k];
      const double dak = D[(int64_t)a * ld + k], dbk = D[(int64_t)b * ld + k];
      const double t1 = (double)(na + nk) * dak;
      const double t2 = (double)(nb + nk) * dbk;
      const double t3 = (double)nk * dab;
      const double s12 = t1 + t2;
      const double num = s12 - t3;
      const double nw = num / (double)(na + nb + nk);
      D[(int64_t)a * ld + k] = nw;
      D[(int64_t)k * ld + a] = nw;
      const int c = nns[k];
      if (c == a || c == b) nns[k] = -1;
    }
    __syncthreads();
    if (tid == 0) {
      id[a] = next_id;
      sz[a] = na + nb;
      rep[a] = newrep;
      id[b] = -1;
    }
    ++next_id;
    __syncthreads();
    {   // the new cluster's neighbour, computed at creation
      double d = INFINITY;
      int bi = NP_POOL_NOID, bs = -1;
      for (int t = tid; t < m; t += T) {
        const int i = id[t];
        if (i < 0 || t == a) continue;
        const double v = D[(int64_t)a * ld + t];
        if (v < d || (v == d && i < bi)) {
          d = v;
          bi = i;
          bs = t;
        }
      }
      pool_argmin(d, bi, bs, redd, redi);
      if (tid == 0) {
        nns[a] = bs;
        nnd[a] = d;
      }
    }
    len -= 2;
    if (len > 0) {
      cur = chain[len - 1];
      prev = len >= 2 ? chain[len - 2] : -1;
    }
    __syncthreads();
  }

  // ---- the cut: the first m - k merges in chain order (fcluster_maxclust as the reference calls it) or in stable order by
  // merge distance (scipy / PyLate); a partition does not depend on the order its merges are applied in
  const int nsel = m - pd.k, nrows = m - 1;
  int* sel = nns;
  int* comp = chain;
  for (int r = tid; r < nrows; r += T) {
    int s = r < nsel;
    if (cut_order == 1) {
      const double dr = mdist[r];
      int rank = 0;
      for (int q = 0; q < nrows; ++q) {
        const double dq = mdist[q];
        rank += (dq < dr || (dq == dr && q < r)) ? 1 : 0;
      }
      s = rank < nsel;
    }
    sel[r] = s;
  }
  for (int t = tid; t < m; t += T) comp[t] = t;
  __syncthreads();
  for (int r = 0; r < nrows; ++r) {
    if (!sel[r]) continue;
    const int cx = comp[mr1[r]], cy = comp[mr2[r]];
    if (cx == cy) continue;
    const int keep = min(cx, cy), drop = max(cx, cy);
    __syncthreads();
    for (int t = tid; t < m; t += T)
      if (comp[t] == drop) comp[t] = keep;
    __syncthreads();
  }
  // comp[t] = the first token of t's cluster: labels count the clusters in the order of their first token
  const int per = (m + T - 1) / T, t0 = tid * per, t1 = min(m, t0 + per);
  int cnt = 0;
  for (int t = t0; t < t1; ++t) cnt += comp[t] == t;
  __syncthreads();
  sz[tid] = cnt;   // mcap >= T
  __syncthreads();
  int base = 0;
  for (int x = 0; x < tid; ++x) base += sz[x];
  for (int t = t0; t < t1; ++t)
    if (comp[t] == t) mr1[t] = base++;
  __syncthreads();
  for (int t = tid; t < m; t += T) labels[pd.lab_off + t] = 1 + mr1[comp[t]];
}

// ---- means -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void pool_means_kernel(const float* __restrict__ X, int dim, const PoolDoc* __restrict__ docs,
                                                         const int32_t* __restrict__ labels, float* __restrict__ out) {
  __shared__ int lab[NP_POOL_MAX_TOKENS];
  const PoolDoc pd = docs[blockIdx.x];
  const int m = pd.m;
  for (int t = threadIdx.x; t < m; t += 256) lab[t] = labels[pd.lab_off + t];
  __syncthreads();
  const int total = pd.k * dim;
  for (int e = threadIdx.x; e < total; e += 256) {
    const int c = e / dim, j = e - c * dim;
    float acc = 0.f;
    int cnt = 0;
    for (int t = 0; t < m; ++t) {
      if (lab[t] != c + 1) continue;
      acc += X[(pd.row0 + t) * dim + j];
      ++cnt;
    }
    out[(pd.out_off + c) * dim + j] = acc / (float)max(cnt, 1);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------

namespace {

struct PoolShape {
  int64_t n, m, k;   // tokens, clustered tokens, clusters; k == 0: the document is returned unchanged
  int64_t out() const { return k > 0 ? n - m + k : n; }
};

// lib.rs:2254-2266
PoolShape pool_shape(int64_t n, int64_t factor, int64_t prot) {
  PoolShape s{n, 0, 0};
  if (factor <= 1 || n <= prot + 1) return s;
  const int64_t m = n - prot;
  const int64_t k = std::max<int64_t>(m / factor, 1);
  if (k >= m) return s;
  s.m = m;
  s.k = k;
  return s;
}

int check_pool_args(const int64_t* doc_lengths, int64_t n_docs, const np_pool_opts* o, const char* who) {
  if (!o) {
    set_error("%s: opts is NULL", who);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (n_docs < 0 || (n_docs > 0 && !doc_lengths)) {
    set_error("%s: %lld documents without lengths", who, (long long)n_docs);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (o->protected_tokens < 0 || o->cut_order < 0 || o->cut_order > 1 || o->chunk_docs < 0) {
    set_error("%s: invalid options (protected_tokens=%d cut_order=%d chunk_docs=%lld)", who, o->protected_tokens,
              o->cut_order, (long long)o->chunk_docs);
    return NP_ERR_INVALID_ARGUMENT;
  }
  for (int64_t i = 0; i < n_docs; ++i)
    if (doc_lengths[i] < 0) {
      set_error("%s: document %lld has negative length %lld", who, (long long)i, (long long)doc_lengths[i]);
      return NP_ERR_INVALID_ARGUMENT;
    }
  return NP_OK;
}

struct PoolStream {
  hipStream_t st = nullptr;
  hipEvent_t ev[4] = {};
  ~PoolStream() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
  }
};

struct PoolClass {
  int mcap, threads;
  bool lds;
};
// LDS classes by the matrix they hold, scratch classes by the per-slot arrays; mcap >= threads (the label scan) and even
const PoolClass kPoolClasses[] = {{64, 64, true},    {96, 64, true},     {NP_POOL_LDS_MAX, 64, true}, {256, 256, false},
                                  {512, 256, false}, {1024, 256, false}, {NP_POOL_MAX_TOKENS, 256, false}};
constexpr int kPoolNClasses = (int)(sizeof(kPoolClasses) / sizeof(kPoolClasses[0]));

size_t pool_class_lds(const PoolClass& c) {
  return (size_t)c.mcap * 44 + 128 + (c.lds ? (size_t)(c.mcap | 1) * c.mcap * 8 : 0);
}

struct PoolChunk {
  int64_t doc0 = 0, doc1 = 0;       // documents [doc0, doc1)
  int64_t rows = 0, n_pooled = 0;   // their tokens; the documents among them that are clustered
  int64_t d_elems = 0, link_rows = 0, lab = 0, out_rows = 0, tiles = 0;
};

}  // namespace

static int pool_documents_impl(int device, const float* X, const int64_t* doc_lengths, int64_t n_docs, int dim,
                               const np_pool_opts& o, float* out, int64_t out_cap, int64_t* out_lengths, int32_t* out_labels,
                               double* out_linkage, np_pool_report* report) {
  const int64_t prot = o.protected_tokens, factor = o.pool_factor;
  std::vector<PoolShape> shp((size_t)n_docs);
  int64_t T_in = 0, T_out = 0, n_pooled = 0;
  for (int64_t i = 0; i < n_docs; ++i) {
    shp[(size_t)i] = pool_shape(doc_lengths[i], factor, prot);
    T_in += doc_lengths[i];
    T_out += shp[(size_t)i].out();
    if (shp[(size_t)i].k > 0) {
      ++n_pooled;
      if (shp[(size_t)i].m > NP_POOL_MAX_TOKENS) {
        set_error("Shape error: document %lld hands %lld tokens to the pooling (%lld tokens, %lld protected); the limit is %d",
                  (long long)i, (long long)shp[(size_t)i].m, (long long)doc_lengths[i], (long long)prot, NP_POOL_MAX_TOKENS);
        return NP_ERR_SHAPE;
      }
    }
  }
  if (report) {
    memset(report, 0, sizeof(*report));
    report->n_docs = n_docs;
    report->n_pooled = n_pooled;
    report->tokens_in = T_in;
    report->tokens_out = T_out;
  }
  if (T_in > 0 && !X) {
    set_error("np_hip_pool_documents: embeddings are NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (T_out > 0 && (!out || out_cap < T_out)) {
    set_error("np_hip_pool_documents: out_embeddings holds %lld rows, %lld needed", (long long)out_cap, (long long)T_out);
    return NP_ERR_INVALID_ARGUMENT;
  }
  {   // non-finite inputs: the reference's nearest-neighbour search would answer usize::MAX and index with it
    const uint32_t* u = reinterpret_cast<const uint32_t*>(X);
    const int64_t cnt = T_in * dim;
    for (int64_t i = 0; i < cnt; ++i)
      if ((u[i] & 0x7f800000u) == 0x7f800000u) {
        set_error("np_hip_pool_documents: non-finite value at token %lld, feature %lld", (long long)(i / dim),
                  (long long)(i % dim));
        return NP_ERR_INVALID_ARGUMENT;
      }
  }
  // protected rows and the documents that stay as they are: host copies
  {
    int64_t ri = 0, ro = 0;
    for (int64_t i = 0; i < n_docs; ++i) {
      const PoolShape& s = shp[(size_t)i];
      const int64_t keep = s.k > 0 ? s.n - s.m : s.n;
      if (keep > 0) memcpy(out + ro * dim, X + ri * dim, (size_t)keep * dim * 4);
      if (out_labels && s.n > 0) memset(out_labels + ri, 0, (size_t)s.n * 4);
      if (out_lengths) out_lengths[i] = s.out();
      ri += s.n;
      ro += s.out();
    }
  }
  if (n_pooled == 0) return NP_OK;

  NP_TRY(build_check_device(device));
  DeviceGuard g(device);
  int lds_max = NP_POOL_LDS_MAX;
  if (const char* e = getenv("NP_POOL_LDS_MAX")) lds_max = std::max(0, std::min(NP_POOL_LDS_MAX, atoi(e)));

  // chunks of consecutive documents whose device arrays fit the budget (results do not depend on the cut: documents are independent)
  size_t free_b = 0, total_b = 0;
  NP_HIP(hipMemGetInfo(&free_b, &total_b));
  const int64_t budget = std::max<int64_t>((int64_t)std::min<size_t>(free_b / 2, (size_t)8 << 30), (int64_t)64 << 20);
  std::vector<PoolChunk> chunks;
  {
    PoolChunk c;
    int64_t bytes = 0;
    for (int64_t i = 0; i < n_docs; ++i) {
      const PoolShape& s = shp[(size_t)i];
      int64_t need = s.n * ((int64_t)dim * 4 + 8);
      if (s.k > 0) {
        const int64_t nt = (s.m + NP_POOL_TILE - 1) / NP_POOL_TILE;
        need += s.m * (s.m | 1) * 8 + (s.m - 1) * 32 + s.m * 4 + s.k * (int64_t)dim * 4 + nt * nt * 16 + (int64_t)sizeof(PoolDoc) + 4;
      }
      const bool full = c.doc1 > c.doc0 && (bytes + need > budget || (o.chunk_docs > 0 && c.doc1 - c.doc0 >= o.chunk_docs));
      if (full) {
        chunks.push_back(c);
        c = PoolChunk();
        c.doc0 = c.doc1 = i;
        bytes = 0;
      }
      c.doc1 = i + 1;
      c.rows += s.n;
      bytes += need;
      if (s.k > 0) {
        const int64_t nt = (s.m + NP_POOL_TILE - 1) / NP_POOL_TILE;
        ++c.n_pooled;
        c.d_elems += s.m * (s.m | 1);
        c.link_rows += s.m - 1;
        c.lab += s.m;
        c.out_rows += s.k;
        c.tiles += nt * nt;
      }
    }
    if (c.doc1 > c.doc0) chunks.push_back(c);
  }
  PoolChunk mx;
  for (const PoolChunk& c : chunks) {
    mx.rows = std::max(mx.rows, c.rows);
    mx.n_pooled = std::max(mx.n_pooled, c.n_pooled);
    mx.d_elems = std::max(mx.d_elems, c.d_elems);
    mx.link_rows = std::max(mx.link_rows, c.link_rows);
    mx.lab = std::max(mx.lab, c.lab);
    mx.out_rows = std::max(mx.out_rows, c.out_rows);
    mx.tiles = std::max(mx.tiles, c.tiles);
  }
  DevPtr<float> dX, dOut;
  DevPtr<double> dNorm, dD, dLink;
  DevPtr<int32_t> dLab, dOrder, dErr;
  DevPtr<PoolDoc> dDocs;
  DevPtr<int4> dTiles;
  NP_TRY(dX.alloc((size_t)mx.rows * dim));
  NP_TRY(dNorm.alloc((size_t)mx.rows));
  NP_TRY(dD.alloc((size_t)mx.d_elems));
  NP_TRY(dLink.alloc((size_t)mx.link_rows * 4));
  NP_TRY(dLab.alloc((size_t)mx.lab));
  NP_TRY(dOrder.alloc((size_t)mx.n_pooled));
  NP_TRY(dOut.alloc((size_t)mx.out_rows * dim));
  NP_TRY(dDocs.alloc((size_t)mx.n_pooled));
  NP_TRY(dTiles.alloc((size_t)mx.tiles));
  NP_TRY(dErr.alloc(1));
  PoolStream ps;
  NP_HIP(hipStreamCreateWithFlags(&ps.st, hipStreamNonBlocking));
  for (hipEvent_t& e : ps.ev) NP_HIP(hipEventCreate(&e));
  hipStream_t st = ps.st;
  NP_HIP(hipMemsetAsync(dErr.get(), 0, 4, st));
  // the attribute is per kernel: leave each of the two at its largest class
  NP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pool_linkage_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)pool_class_lds(kPoolClasses[2])));
  NP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pool_linkage_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)pool_class_lds(kPoolClasses[kPoolNClasses - 1])));

  std::vector<PoolDoc> hdocs;
  std::vector<int4> htiles;
  std::vector<int32_t> horder, hlab;
  std::vector<int64_t> src_doc;
  std::vector<float> hout;
  std::vector<double> hlink;
  // positions of every document in the caller's arrays
  std::vector<int64_t> in_row((size_t)n_docs + 1, 0), out_row((size_t)n_docs + 1, 0), link_row((size_t)n_docs + 1, 0);
  for (int64_t i = 0; i < n_docs; ++i) {
    const PoolShape& s = shp[(size_t)i];
    in_row[(size_t)i + 1] = in_row[(size_t)i] + s.n;
    out_row[(size_t)i + 1] = out_row[(size_t)i] + s.out();
    link_row[(size_t)i + 1] = link_row[(size_t)i] + (s.k > 0 ? s.m - 1 : 0);
  }
  double ms_d = 0, ms_l = 0, ms_m = 0;
  for (const PoolChunk& c : chunks) {
    if (c.n_pooled == 0) continue;
    hdocs.clear();
    htiles.clear();
    src_doc.clear();
    int64_t d_off = 0, l_off = 0, lab_off = 0, o_off = 0;
    const int64_t R0 = in_row[(size_t)c.doc0];
    for (int64_t i = c.doc0; i < c.doc1; ++i) {
      const PoolShape& s = shp[(size_t)i];
      if (s.k <= 0) continue;
      PoolDoc pd{};
      pd.row0 = in_row[(size_t)i] - R0 + (s.n - s.m);
      pd.d_off = d_off;
      pd.link_off = l_off;
      pd.lab_off = lab_off;
      pd.out_off = o_off;
      pd.m = (int32_t)s.m;
      pd.k = (int32_t)s.k;
      pd.ld = (int32_t)(s.m | 1);
      const int nt = (int)((s.m + NP_POOL_TILE - 1) / NP_POOL_TILE);
      for (int a = 0; a < nt; ++a)
        for (int b = 0; b < nt; ++b) htiles.push_back(make_int4((int)hdocs.size(), a, b, 0));
      hdocs.push_back(pd);
      src_doc.push_back(i);
      d_off += s.m * (s.m | 1);
      l_off += s.m - 1;
      lab_off += s.m;
      o_off += s.k;
    }
    // documents by class, the classes launched one after the other
    horder.clear();
    int cls_begin[kPoolNClasses + 1];
    for (int ci = 0; ci < kPoolNClasses; ++ci) {
      cls_begin[ci] = (int)horder.size();
      const PoolClass& pc = kPoolClasses[ci];
      for (size_t d = 0; d < hdocs.size(); ++d) {
        const int m = hdocs[d].m;
        int want = -1;
        for (int cj = 0; cj < kPoolNClasses && want < 0; ++cj) {
          const PoolClass& q = kPoolClasses[cj];
          if (m <= q.mcap && (!q.lds || m <= lds_max)) want = cj;
        }
        if (want == ci) horder.push_back((int32_t)d);
      }
      (void)pc;
    }
    cls_begin[kPoolNClasses] = (int)horder.size();

    NP_HIP(hipMemcpyAsync(dX.get(), X + R0 * dim, (size_t)c.rows * dim * 4, hipMemcpyHostToDevice, st));
    NP_HIP(hipMemcpyAsync(dDocs.get(), hdocs.data(), hdocs.size() * sizeof(PoolDoc), hipMemcpyHostToDevice, st));
    NP_HIP(hipMemcpyAsync(dTiles.get(), htiles.data(), htiles.size() * sizeof(int4), hipMemcpyHostToDevice, st));
    NP_HIP(hipMemcpyAsync(dOrder.get(), horder.data(), horder.size() * 4, hipMemcpyHostToDevice, st));
    NP_HIP(hipEventRecord(ps.ev[0], st));
    pool_norms_kernel<<<(unsigned)((c.rows + 255) / 256), 256, 0, st>>>(dX.get(), dim, c.rows, dNorm.get());
    pool_dist_kernel<<<(unsigned)htiles.size(), 256, 0, st>>>(dX.get(), dim, dNorm.get(), dDocs.get(), dTiles.get(), dD.get());
    NP_HIP(hipEventRecord(ps.ev[1], st));
    for (int ci = 0; ci < kPoolNClasses; ++ci) {
      const int nd = cls_begin[ci + 1] - cls_begin[ci];
      if (nd == 0) continue;
      const PoolClass& pc = kPoolClasses[ci];
      const size_t lds = pool_class_lds(pc);
      if (pc.lds)
        pool_linkage_kernel<true><<<(unsigned)nd, pc.threads, lds, st>>>(dDocs.get(), dOrder.get() + cls_begin[ci], dD.get(),
                                                                        dLink.get(), dLab.get(), o.cut_order, pc.mcap, dErr.get());
      else
        pool_linkage_kernel<false><<<(unsigned)nd, pc.threads, lds, st>>>(dDocs.get(), dOrder.get() + cls_begin[ci], dD.get(),
                                                                         dLink.get(), dLab.get(), o.cut_order, pc.mcap, dErr.get());
    }
    NP_HIP(hipEventRecord(ps.ev[2], st));
    pool_means_kernel<<<(unsigned)hdocs.size(), 256, 0, st>>>(dX.get(), dim, dDocs.get(), dLab.get(), dOut.get());
    NP_HIP(hipEventRecord(ps.ev[3], st));
    NP_HIP(hipGetLastError());
    hout.resize((size_t)c.out_rows * dim);
    NP_HIP(hipMemcpyAsync(hout.data(), dOut.get(), hout.size() * 4, hipMemcpyDeviceToHost, st));
    if (out_labels) {
      hlab.resize((size_t)c.lab);
      NP_HIP(hipMemcpyAsync(hlab.data(), dLab.get(), hlab.size() * 4, hipMemcpyDeviceToHost, st));
    }
    if (out_linkage) {
      hlink.resize((size_t)c.link_rows * 4);
      NP_HIP(hipMemcpyAsync(hlink.data(), dLink.get(), hlink.size() * 8, hipMemcpyDeviceToHost, st));
    }
    int32_t herr = 0;
    NP_HIP(hipMemcpyAsync(&herr, dErr.get(), 4, hipMemcpyDeviceToHost, st));
    NP_HIP(hipStreamSynchronize(st));
    if (herr) {
      set_error("np_hip_pool_documents: the nearest-neighbour chain of a document in [%lld, %lld) does not terminate "
                "(the reference's does not either)", (long long)c.doc0, (long long)c.doc1);
      return NP_ERR_INVALID_ARGUMENT;
    }
    float ms = 0.f;
    NP_HIP(hipEventElapsedTime(&ms, ps.ev[0], ps.ev[1]));
    ms_d += ms;
    NP_HIP(hipEventElapsedTime(&ms, ps.ev[1], ps.ev[2]));
    ms_l += ms;
    NP_HIP(hipEventElapsedTime(&ms, ps.ev[2], ps.ev[3]));
    ms_m += ms;
    for (size_t d = 0; d < hdocs.size(); ++d) {
      const PoolDoc& pd = hdocs[d];
      const int64_t i = src_doc[d];
      const int64_t p = shp[(size_t)i].n - shp[(size_t)i].m;
      memcpy(out + (out_row[(size_t)i] + p) * dim, hout.data() + pd.out_off * dim, (size_t)pd.k * dim * 4);
      if (out_labels) memcpy(out_labels + in_row[(size_t)i] + p, hlab.data() + pd.lab_off, (size_t)pd.m * 4);
      if (out_linkage) memcpy(out_linkage + link_row[(size_t)i] * 4, hlink.data() + pd.link_off * 4, (size_t)(pd.m - 1) * 32);
    }
  }
  if (report) {
    report->ms_distances = ms_d;
    report->ms_linkage = ms_l;
    report->ms_means = ms_m;
    report->n_chunks = (int64_t)chunks.size();
  }
  return NP_OK;
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_pooled_lengths(const int64_t* doc_lengths, int64_t n_docs, const np_pool_opts* opts, int64_t* out_lengths) {
  clear_error();
  NP_TRY(check_pool_args(doc_lengths, n_docs, opts, "np_hip_pooled_lengths"));
  if (n_docs > 0 && !out_lengths) {
    set_error("np_hip_pooled_lengths: out_lengths is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  for (int64_t i = 0; i < n_docs; ++i) out_lengths[i] = pool_shape(doc_lengths[i], opts->pool_factor, opts->protected_tokens).out();
  return NP_OK;
}

int np_hip_pool_documents(int32_t device, const float* embeddings, const int64_t* doc_lengths, int64_t n_docs, int32_t dim,
                          const np_pool_opts* opts, float* out_embeddings, int64_t out_rows_capacity, int64_t* out_lengths,
                          int32_t* out_labels, double* out_linkage, np_pool_report* report) {
  clear_error();
  NP_TRY(check_pool_args(doc_lengths, n_docs, opts, "np_hip_pool_documents"));
  if (dim <= 0) {
    set_error("Shape error: pooling needs dim >= 1, got %d", dim);
    return NP_ERR_SHAPE;
  }
  return pool_documents_impl(device, embeddings, doc_lengths, n_docs, dim, *opts, out_embeddings, out_rows_capacity,
                             out_lengths, out_labels, out_linkage, report);
}

}  // extern "C"
