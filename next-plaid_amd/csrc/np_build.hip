// np_build.hip -- index creation on the GPU: k-means (Lloyd), codec training and the create path.
//
// The crate's create path (next-plaid/src/index.rs:927-967 create_index_with_kmeans_files) is
//   compute_kmeans (kmeans.rs:261-421) -> prepare_codec_artifacts (index.rs:182-287) -> encode + write (index.rs:551-...)
// and k-means is the only heavy computation in it: one Lloyd iteration is 2 n k d FLOP (1.8e16 at the crate's heuristic for
// 10 M documents x 300 tokens).  Rules of each piece: include/nextplaid_hip.h; the kernels (DESIGN.md "k-means kernels"):
//   km_norm_kernel        |x|^2 per point as a k-ordered f32 FMA chain, and max |x_j| (once per call)
//   km_tiles_kernel       centroids -> k-major 32-centroid tiles [d][32] + their |c|^2 (once per iteration)
//   km_assign_kernel      fused distance GEMM + argmin on exact-f32 MFMA 32x32x2: a wave holds 2 x 32 points as B fragments in
//                         registers and streams the centroid tiles through LDS as A fragments; the epilogue forms
//                         max(fma(-2, x.c, |x|^2 + |c|^2), 0) and keeps each point's minimum of (distance bits << 32 | index);
//                         centroid chunks of a point combine by a 64-bit atomicMin: the minimum distance, the lowest index on
//                         ties, in any order.  No n x k matrix is written.
//   km_count_kernel       assignment, cluster sizes and each cluster's max |x_j| (integer atomics: order-free)
//   km_scatter_kernel     counting sort of the point ids by cluster (the order inside a cluster is arbitrary ...)
//   km_mean_kernel        ... because each cluster sums its points in 64-bit fixed point (exact, so associative) on a scale
//                         set by its own max |x_j| and size: the means, the re-initialised empty clusters and |new - old|
//                         per cluster, one workgroup per cluster
//   km_shift_kernel       shift = the sum of |new - old| in f64 in a fixed order
// Held-out statistics, sorting and quantiles are host code (at most 50 000 tokens).
#include "np_internal.h"

#include <float.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace np {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ int mfma_row32(int r, int kk) { return (r & 3) + 8 * (r >> 2) + 4 * kk; }

// ---- random numbers: SplitMix64 (Steele, Lea, Flood 2014), unbiased bounded draws, Fisher-Yates ----------------------
struct SplitMix64 {
  uint64_t s;
  explicit SplitMix64(uint64_t seed) : s(seed) {}
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t b) {   // uniform in [0, b): reject the low (2^64 mod b) draws
    const uint64_t thr = (0 - b) % b;
    for (;;) {
      const uint64_t r = next();
      if (r >= thr) return r % b;
    }
  }
};

// the crate's document shuffle (rand's SliceRandom::shuffle order: i from n-1 down to 1, j uniform in [0, i])
std::vector<int64_t> shuffled_docs(int64_t n, uint64_t seed) {
  std::vector<int64_t> a((size_t)n);
  for (int64_t i = 0; i < n; ++i) a[(size_t)i] = i;
  SplitMix64 g(seed);
  for (int64_t i = n - 1; i > 0; --i) std::swap(a[(size_t)i], a[(size_t)g.below((uint64_t)i + 1)]);
  return a;
}

// first m entries of a partial Fisher-Yates over 0..n-1 (for i in 0..m: j = i + below(n - i), swap)
std::vector<uint32_t> partial_sample(SplitMix64& g, int64_t n, int64_t m) {
  std::vector<uint32_t> a((size_t)n);
  for (int64_t i = 0; i < n; ++i) a[(size_t)i] = (uint32_t)i;
  for (int64_t i = 0; i < m; ++i) std::swap(a[(size_t)i], a[(size_t)(i + (int64_t)g.below((uint64_t)(n - i)))]);
  a.resize((size_t)m);
  return a;
}

// utils.rs:94-149: sort, idx = q (n - 1) in f64, linear interpolation in f32 with the weight cast to f32
float quantile_sorted(const std::vector<float>& v, double q) {
#pragma clang fp contract(off)
  if (v.empty()) return 0.f;
  const double idx = q * (double)(v.size() - 1);
  const size_t lo = (size_t)floor(idx), hi = (size_t)ceil(idx);
  if (lo == hi) return v[lo];
  const float w = (float)(idx - (double)lo);
  return v[lo] * (1.0f - w) + v[hi] * w;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) km_norm_kernel(const float* __restrict__ X, int64_t n, int D, float* __restrict__ out,
                                                      float* __restrict__ amax) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* x = X + i * D;
  float s = 0.f, m = 0.f;
  for (int d = 0; d < D; ++d) {
    s = fmaf(x[d], x[d], s);
    m = fmaxf(m, fabsf(x[d]));
  }
  out[i] = s;
  amax[i] = m;
}

// tile t = centroids 32t .. 32t+31: [D][32] k-major values, then 32 squared norms (+inf for the padding rows past k:
// their distance is +inf with an index >= k, so a real centroid always wins)
__global__ void __launch_bounds__(256) km_tiles_kernel(const float* __restrict__ C, int64_t k, int D, int64_t ntiles,
                                                       float* __restrict__ Ct) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ntiles * 32) return;
  const int64_t t = i >> 5;
  const int j = (int)(i & 31);
  float* tile = Ct + t * ((int64_t)D * 32 + 32);
  float s = 0.f;
  if (i < k) {
    const float* c = C + i * D;
    for (int d = 0; d < D; ++d) {
      const float v = c[d];
      tile[d * 32 + j] = v;
      s = fmaf(v, v, s);
    }
  } else {
    for (int d = 0; d < D; ++d) tile[d * 32 + j] = 0.f;
    s = __int_as_float(0x7F800000);
  }
  tile[D * 32 + j] = s;
}

// One workgroup = 4 waves x 2 fragments x 32 points; blockIdx.y = a chunk of centroid tiles.  D[c][p] = sum_k A[c][k] B[k][p]
// with A = the centroid tile (lane: centroid li, dim 2s + kk, from LDS) and B = the points (lane: point li, dim 2s + kk, in
// registers for the whole kernel); a lane ends with point li against centroid rows mfma_row32(r, kk) of the tile.
// tile t (TW floats) -> LDS buffer by the DMA path (global_load_lds_dwordx4: no staging registers).  Wave w copies the 1-KiB
// pieces w, w + 4, ...; the last piece reads past the tile (the tile array carries 1 KiB of slack for the last tile)
template <int TW>
__device__ __forceinline__ void km_dma_tile(const float* __restrict__ Ct, int t, float* dst, int wave, int lane) {
  constexpr int NW = (TW / 4 + 63) / 64;
  const float* src = Ct + (int64_t)t * TW;
#pragma unroll
  for (int j = 0; j < NW; j += 4)
    if (j + wave < NW)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + ((j + wave) * 64 + lane) * 4),
                                       (__attribute__((address_space(3))) void*)(dst + (j + wave) * 256), 16, 0, 0);
}

// One workgroup = 4 waves x 2 fragments x 32 points; blockIdx.y = a chunk of centroid tiles.  D[c][p] = sum_k A[c][k] B[k][p]
// with A = the centroid tile (lane: centroid li, dim 2s + kk, from LDS) and B = the points (lane: point li, dim 2s + kk, in
// registers for the whole kernel); a lane ends with point li against centroid rows mfma_row32(r, kk) of the tile.
template <int D>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 128 ? 1 : 2))) km_assign_kernel(
    const float* __restrict__ X, const float* __restrict__ xn, int64_t n, const float* __restrict__ Ct, int ntiles,
    int tiles_per_chunk, unsigned long long* __restrict__ best) {
  constexpr int TW = D * 32 + 32;                   // floats per tile
  constexpr int TWL = (TW / 4 + 63) / 64 * 256;     // LDS floats per buffer (whole 1-KiB pieces)
  __shared__ __attribute__((aligned(16))) float sC[2][TWL];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, kk = lane >> 5, wave = tid >> 6;
  const int64_t p0 = (int64_t)blockIdx.x * 256 + wave * 64;
  float b[2][D / 2];
  float xv[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int64_t p = p0 + 32 * f + li;
    xv[f] = p < n ? xn[p] : 0.f;
#pragma unroll
    for (int m = 0; m < D / 4; ++m) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p < n) v = *reinterpret_cast<const float4*>(X + p * D + 4 * m);
      b[f][2 * m] = kk ? v.y : v.x;
      b[f][2 * m + 1] = kk ? v.w : v.z;
    }
  }
  unsigned long long bk0 = ~0ull, bk1 = ~0ull;
  const int t0 = blockIdx.y * tiles_per_chunk, t1 = min(ntiles, t0 + tiles_per_chunk);
  if (t0 < t1) km_dma_tile<TW>(Ct, t0, sC[0], wave, lane);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int cur = (t - t0) & 1;
    if (t + 1 < t1) km_dma_tile<TW>(Ct, t + 1, sC[cur ^ 1], wave, lane);   // in flight during this tile's MFMAs
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc0[r] = 0.f;
      acc1[r] = 0.f;
    }
    const float* a = &sC[cur][kk * 32 + li];   // [2s + kk][centroid li]
#pragma unroll
    for (int s = 0; s < D / 2; ++s) {
      const float av = a[s * 64];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[0][s], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[1][s], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mfma_row32(r, kk);
      const float cn = sC[cur][D * 32 + row];
      const unsigned long long idx = (unsigned long long)(uint32_t)(t * 32 + row);
      const float d0 = fmaxf(fmaf(-2.f, acc0[r], xv[0] + cn), 0.f);
      const float d1 = fmaxf(fmaf(-2.f, acc1[r], xv[1] + cn), 0.f);
      const unsigned long long k0 = ((unsigned long long)__float_as_uint(d0) << 32) | idx;
      const unsigned long long k1 = ((unsigned long long)__float_as_uint(d1) << 32) | idx;
      bk0 = k0 < bk0 ? k0 : bk0;
      bk1 = k1 < bk1 ? k1 : bk1;
    }
    __syncthreads();   // waits for the DMA too (vmcnt(0) before the barrier)
  }
  if (t0 >= t1) return;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const unsigned long long v = f ? bk1 : bk0;
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, 32);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), 32);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    const unsigned long long m = o < v ? o : v;
    const int64_t p = p0 + 32 * f + li;
    if (kk == 0 && p < n) atomicMin(best + p, m);
  }
}

// cmax[c] = the bits of max |x_j| over the cluster's points (non-negative floats order as their bit patterns)
__global__ void __launch_bounds__(256) km_count_kernel(const unsigned long long* __restrict__ best, const float* __restrict__ amax,
                                                       int64_t n, int32_t* __restrict__ assign, int32_t* __restrict__ counts,
                                                       uint32_t* __restrict__ cmax) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t c = (int32_t)(uint32_t)best[i];
  assign[i] = c;
  atomicAdd(counts + c, 1);
  atomicMax(cmax + c, __float_as_uint(amax[i]));
}

__global__ void __launch_bounds__(256) km_scatter_kernel(const int32_t* __restrict__ assign, int64_t n,
                                                         const int32_t* __restrict__ off, int32_t* __restrict__ cursor,
                                                         int32_t* __restrict__ order) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t c = assign[i];
  order[off[c] + atomicAdd(cursor + c, 1)] = (int32_t)i;
}

// One workgroup per cluster.  Sum of the points in fixed point q = rint(x 2^S) with the cluster's own scale
// S = 62 - e - ceil(log2 count), max |x_j| < 2^e: every |q| <= 2^(62 - ceil(log2 count)), so |sum| <= 2^62 and the sum is
// exact.  mean = (f64) sum 2^-S / count rounded to f32: within 1 ulp of the exact mean plus the quantisation
// 2^(-S-1) < 2 max|x_j| count 2^-62, which depends only on the cluster's own points.  An empty cluster takes row reinit[c] of X.  part[c] = |new - old| (f32,
// k-ordered FMA chain of the squared differences).
template <int D>
__global__ void __launch_bounds__(256) km_mean_kernel(const float* __restrict__ X, const int32_t* __restrict__ order,
                                                      const int32_t* __restrict__ off, const int32_t* __restrict__ reinit,
                                                      const uint32_t* __restrict__ cmax, const float* __restrict__ Cold,
                                                      float* __restrict__ Cnew, float* __restrict__ part) {
  constexpr int DL = (D + 63) / 64;   // dims per lane
  __shared__ long long s_sum[4][D];
  __shared__ float s_d2[D];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t b = off[c], e = off[c + 1];
  const float* old = Cold + (int64_t)c * D;
  float* nw = Cnew + (int64_t)c * D;
  if (e > b) {
    int ex = 0, lg = 0;
    (void)frexpf(__uint_as_float(cmax[c]), &ex);   // max |x_j| < 2^ex (ex = 0 for an all-zero cluster: any scale is exact)
    while (((int64_t)1 << lg) < (int64_t)(e - b)) ++lg;
    const double scale = ldexp(1.0, 62 - ex - lg), inv_scale = ldexp(1.0, ex + lg - 62);
    long long acc[DL];
#pragma unroll
    for (int j = 0; j < DL; ++j) acc[j] = 0;
    for (int32_t r = b + wave; r < e; r += 4) {
      const float* x = X + (int64_t)order[r] * D;
#pragma unroll
      for (int j = 0; j < DL; ++j)
        if (lane + 64 * j < D) acc[j] += __double2ll_rn((double)x[lane + 64 * j] * scale);
    }
#pragma unroll
    for (int j = 0; j < DL; ++j)
      if (lane + 64 * j < D) s_sum[wave][lane + 64 * j] = acc[j];
    __syncthreads();
    if (tid < D) {
      const long long s = s_sum[0][tid] + s_sum[1][tid] + s_sum[2][tid] + s_sum[3][tid];
      const float m = (float)((double)s * inv_scale / (double)(e - b));
      nw[tid] = m;
      const float df = m - old[tid];
      s_d2[tid] = df;
    }
  } else {
    const int32_t src = reinit[c];
    if (tid < D) {
      const float m = src >= 0 ? X[(int64_t)src * D + tid] : old[tid];
      nw[tid] = m;
      s_d2[tid] = m - old[tid];
    }
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int d = 0; d < D; ++d) s = fmaf(s_d2[d], s_d2[d], s);
    part[c] = sqrtf(s);
  }
}

__global__ void __launch_bounds__(1024) km_shift_kernel(const float* __restrict__ part, int64_t k, double* __restrict__ out) {
  __shared__ double s[1024];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < k; i += 1024) a += (double)part[i];
  s[threadIdx.x] = a;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = s[0];
}

// find_outliers (update.rs:490-619) after one nearest_step over all K centroids.  The f32 minimum d of a row is decided
// here when it lies outside the window |d - thr2| <= w; w covers the crate's own recheck window max(|thr2|, 1) 1e-5
// and this path's f32 error: |x|^2, |c|^2 and x.c are Dp-term f32 chains and the epilogue adds three roundings, so
// |d - |x - c|^2| <= 4 (Dp + 2) 2^-24 (|x|^2 + max |c|^2) for every centroid, hence for the minimum.  Rows inside the
// window go to a list for the f64 recheck.
__global__ void __launch_bounds__(256) ol_flag_kernel(const unsigned long long* __restrict__ best, const float* __restrict__ xn,
                                                      int64_t n, float thr2, float rel, float cn_max, uint8_t* __restrict__ flag,
                                                      int32_t* __restrict__ list, int32_t* __restrict__ n_list) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float d = __uint_as_float((uint32_t)(best[i] >> 32));
  const float w = fmaxf(fmaxf(fabsf(thr2), 1.f) * 1e-5f, rel * (xn[i] + cn_max));
  if (fabsf(d - thr2) <= w) {
    flag[i] = 0;
    list[atomicAdd(n_list, 1)] = (int32_t)i;
  } else {
    flag[i] = d > thr2 ? 1 : 0;
  }
}

// min_distance_sq_precise (update.rs:457-473) for one listed row per workgroup: per centroid the f64 sum of (x_j - c_j)^2 in
// dimension order (no contraction), cast to f32, minimum over all k centroids; the row is an outlier when it exceeds thr2.
// The zero padding of the storage rows adds exact zeros.
__global__ void __launch_bounds__(256) ol_recheck_kernel(const float* __restrict__ X, int Dp, const float* __restrict__ C,
                                                         int64_t k, const int32_t* __restrict__ list, float thr2,
                                                         uint8_t* __restrict__ flag) {
#pragma clang fp contract(off)
  __shared__ double sx[128];
  __shared__ float smin[256];
  const int tid = threadIdx.x;
  const int64_t row = list[blockIdx.x];
  if (tid < Dp) sx[tid] = (double)X[row * Dp + tid];
  __syncthreads();
  float mn = __int_as_float(0x7F800000);
  for (int64_t c = tid; c < k; c += 256) {
    const float* cr = C + c * Dp;
    double s = 0.0;
    for (int j = 0; j < Dp; ++j) {
      const double df = sx[j] - (double)cr[j];
      s += df * df;
    }
    mn = fminf(mn, (float)s);
  }
  smin[tid] = mn;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) smin[tid] = fminf(smin[tid], smin[tid + w]);
    __syncthreads();
  }
  if (tid == 0) flag[row] = smin[0] > thr2 ? 1 : 0;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct DevMem {   // every device buffer of one call, freed on every exit path
  std::vector<void*> ptrs;
  hipStream_t st = nullptr;
  hipEvent_t ev[4] = {};
  template <class T> int alloc(T** p, size_t n) {
    *p = nullptr;
    hipError_t e = hipMalloc((void**)p, std::max<size_t>(n * sizeof(T), 16));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      set_error("hipMalloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
      return e == hipErrorOutOfMemory ? NP_ERR_OUT_OF_MEMORY : NP_ERR_DEVICE_UNAVAILABLE;
    }
    ptrs.push_back((void*)*p);
    return NP_OK;
  }
  ~DevMem() {
    if (st) (void)hipStreamSynchronize(st);
    for (void* p : ptrs) (void)hipFree(p);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
  }
};

int check_build_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    set_error("no HIP device available: index creation runs on a gfx950 GPU (there is no CPU fallback)");
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  if (device < 0 || device >= n) {
    set_error("device %d out of range (%d devices)", device, n);
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess || strncmp(p.gcnArchName, "gfx950", 6) != 0) {
    (void)hipGetLastError();
    set_error("device %d is not a gfx950", device);
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  return NP_OK;
}

int check_dim(int dim) {
  if (dim <= 0 || dim > 128) {
    set_error("Shape error: index creation supports dim 1..128 (as search), got %d", dim);
    return NP_ERR_SHAPE;
  }
  return NP_OK;
}

// the largest |x_j| index creation takes at this dim: |x - c|^2 <= 4 dim B^2 stays below FLT_MAX (with 0.1 % left for
// the rounding of the f32 chains), so no distance is +inf; never above 1e18
double magnitude_bound(int dim) { return std::min(1.0e18, sqrt(0.999 * (double)FLT_MAX / (4.0 * (double)dim))); }

// non-finite values are refused: the crate would train on them and write an index of NaN centroids.  So are values
// above magnitude_bound(dim), whose f32 distances could overflow
int check_finite(const float* x, int64_t count, int dim) {
  float m = 0.f;
  for (int64_t i = 0; i < count; ++i) {
    const float a = fabsf(x[i]);
    if (!(a <= 3.0e38f)) {
      set_error("Index creation failed: embedding value %lld is not finite", (long long)i);
      return NP_ERR_INDEX_CREATION;
    }
    m = std::max(m, a);
  }
  if ((double)m > magnitude_bound(dim)) {
    set_error("Index creation failed: embedding values up to %g overflow the f32 distances at dim %d (bound %g)",
              (double)m, dim, magnitude_bound(dim));
    return NP_ERR_INDEX_CREATION;
  }
  return NP_OK;
}

template <int D>
void launch_assign(const float* X, const float* xn, int64_t n, const float* Ct, int ntiles, int chunks,
                   unsigned long long* best, hipStream_t st) {
  const int tpc = (ntiles + chunks - 1) / chunks;
  dim3 grid((unsigned)((n + 255) / 256), (unsigned)((ntiles + tpc - 1) / tpc));
  km_assign_kernel<D><<<grid, 256, 0, st>>>(X, xn, n, Ct, ntiles, tpc, best);
}

template <int D>
void launch_mean(const float* X, const int32_t* order, const int32_t* off, const int32_t* reinit, const uint32_t* cmax,
                 const float* Cold, float* Cnew, float* part, int64_t k, hipStream_t st) {
  km_mean_kernel<D><<<(unsigned)k, 256, 0, st>>>(X, order, off, reinit, cmax, Cold, Cnew, part);
}

// points [m][dim] (host; row j = points[subset[j]] with a subset) -> HBM in storage rows zero-padded to Dp, through a
// bounded staging buffer
int upload_rows(float* dX, const float* points, int64_t m, int dim, int Dp, const uint32_t* subset, hipStream_t st) {
  const int64_t rows = std::max<int64_t>(1, ((int64_t)64 << 20) / ((int64_t)Dp * 4));
  std::vector<float> stage((size_t)std::min(rows, m) * Dp, 0.f);
  for (int64_t r0 = 0; r0 < m; r0 += rows) {
    const int64_t nr = std::min(rows, m - r0);
    for (int64_t r = 0; r < nr; ++r) {
      const int64_t src = subset ? (int64_t)subset[r0 + r] : r0 + r;
      memcpy(&stage[(size_t)(r * Dp)], points + src * dim, (size_t)dim * 4);
    }
    NP_HIP(hipMemcpyAsync(dX + r0 * Dp, stage.data(), (size_t)nr * Dp * 4, hipMemcpyHostToDevice, st));
    NP_HIP(hipStreamSynchronize(st));   // the staging buffer is reused
  }
  return NP_OK;
}

// centroid chunks of the assign grid: enough workgroups for the device when the points alone do not fill it
int assign_chunks(int device, int64_t m, int64_t ntiles) {
  int n_cu = 256;
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) == hipSuccess && p.multiProcessorCount > 0) n_cu = p.multiProcessorCount;
  const int64_t pblocks = (m + 255) / 256;
  return (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, (2 * n_cu + pblocks - 1) / pblocks));
}

// best[i] = min over the k centroids of (distance bits << 32 | index) for the m points (tiles, then the fused assign)
int nearest_step(const float* dX, const float* dxn, int64_t m, int Dp, const float* dC, int64_t k, int64_t ntiles,
                 int chunks, float* dCt, unsigned long long* dbest, hipStream_t st) {
  km_tiles_kernel<<<(unsigned)((ntiles * 32 + 255) / 256), 256, 0, st>>>(dC, k, Dp, ntiles, dCt);
  NP_HIP(hipMemsetAsync(dbest, 0xFF, (size_t)m * 8, st));
  switch (Dp) {
    case 32: launch_assign<32>(dX, dxn, m, dCt, (int)ntiles, chunks, dbest, st); break;
    case 64: launch_assign<64>(dX, dxn, m, dCt, (int)ntiles, chunks, dbest, st); break;
    case 96: launch_assign<96>(dX, dxn, m, dCt, (int)ntiles, chunks, dbest, st); break;
    default: launch_assign<128>(dX, dxn, m, dCt, (int)ntiles, chunks, dbest, st); break;
  }
  NP_HIP(hipGetLastError());
  return NP_OK;
}

// FastKMeans::train.  points [n][dim] host; out_centroids [k][dim]; out_assign nullable [n]
int kmeans_run(int device, const float* points, int64_t n, int dim, const np_kmeans_opts& o, const float* init,
               float* out_centroids, int64_t* out_assign, np_kmeans_report* rep) {
  const int64_t k = o.k;
  if (n <= 0 || !points) {
    set_error("Index creation failed: No documents provided");
    return NP_ERR_INDEX_CREATION;
  }
  NP_TRY(check_dim(dim));
  if (k <= 0) {
    set_error("Index creation failed: Cannot compute 0 centroids");
    return NP_ERR_INDEX_CREATION;
  }
  if (k > n) {
    set_error("Index creation failed: cannot compute %lld centroids from %lld points", (long long)k, (long long)n);
    return NP_ERR_INDEX_CREATION;
  }
  if (n >= ((int64_t)1 << 31)) {
    set_error("Index creation failed: k-means takes fewer than 2^31 points, got %lld", (long long)n);
    return NP_ERR_INDEX_CREATION;
  }
  if (!out_centroids || o.max_iters < 0) {
    set_error("kmeans: invalid argument");
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(check_finite(points, n * dim, dim));
  if (init) NP_TRY(check_finite(init, k * dim, dim));
  NP_TRY(check_build_device(device));
  DeviceGuard g(device);

  // subsample, then init: one SplitMix64 stream
  SplitMix64 rng(o.seed);
  const bool sub = o.max_points_per_centroid > 0 && n > k * o.max_points_per_centroid;
  const int64_t m = sub ? k * o.max_points_per_centroid : n;
  std::vector<uint32_t> subset;
  if (sub) subset = partial_sample(rng, n, m);
  auto src_row = [&](int64_t j) -> int64_t { return sub ? (int64_t)subset[(size_t)j] : j; };
  const int Dp = storage_dim(dim);
  std::vector<float> c0((size_t)k * Dp, 0.f);
  if (init) {
    for (int64_t c = 0; c < k; ++c) memcpy(&c0[(size_t)(c * Dp)], init + c * dim, (size_t)dim * 4);
  } else {
    const std::vector<uint32_t> pick = partial_sample(rng, m, k);
    for (int64_t c = 0; c < k; ++c) memcpy(&c0[(size_t)(c * Dp)], points + src_row(pick[(size_t)c]) * dim, (size_t)dim * 4);
  }

  DevMem dm;
  NP_HIP(hipStreamCreateWithFlags(&dm.st, hipStreamNonBlocking));
  for (hipEvent_t& e : dm.ev) NP_HIP(hipEventCreate(&e));
  hipStream_t st = dm.st;
  const int64_t ntiles = (k + 31) / 32;
  float *dX, *dxn, *damax, *dC[2], *dCt, *dpart;
  unsigned long long* dbest;
  int32_t *dassign, *dcount, *doff, *dcursor, *dorder, *dreinit;
  uint32_t* dcmax;
  double* dshift;
  NP_TRY(dm.alloc(&dX, (size_t)m * Dp));
  NP_TRY(dm.alloc(&dxn, (size_t)m));
  NP_TRY(dm.alloc(&damax, (size_t)m));
  NP_TRY(dm.alloc(&dC[0], (size_t)k * Dp));
  NP_TRY(dm.alloc(&dC[1], (size_t)k * Dp));
  NP_TRY(dm.alloc(&dCt, (size_t)ntiles * (Dp * 32 + 32) + 256));   // + 1 KiB: the last DMA piece reads past the tile
  NP_TRY(dm.alloc(&dpart, (size_t)k));
  NP_TRY(dm.alloc(&dbest, (size_t)m));
  NP_TRY(dm.alloc(&dassign, (size_t)m));
  NP_TRY(dm.alloc(&dcount, (size_t)k));
  NP_TRY(dm.alloc(&dcmax, (size_t)k));
  NP_TRY(dm.alloc(&doff, (size_t)k + 1));
  NP_TRY(dm.alloc(&dcursor, (size_t)k));
  NP_TRY(dm.alloc(&dorder, (size_t)m));
  NP_TRY(dm.alloc(&dreinit, (size_t)k));
  NP_TRY(dm.alloc(&dshift, 1));

  NP_TRY(upload_rows(dX, points, m, dim, Dp, sub ? subset.data() : nullptr, st));
  NP_HIP(hipMemcpyAsync(dC[0], c0.data(), (size_t)k * Dp * 4, hipMemcpyHostToDevice, st));
  km_norm_kernel<<<(unsigned)((m + 255) / 256), 256, 0, st>>>(dX, m, Dp, dxn, damax);
  NP_HIP(hipGetLastError());

  const int chunks = assign_chunks(device, m, ntiles);

  std::vector<int32_t> counts((size_t)k), off((size_t)k + 1), reinit((size_t)k);
  int cur = 0, it = 0;
  double shift = 0.0, ms_assign = 0.0, ms_update = 0.0;
  int64_t n_reinit = 0;
  const unsigned nb = (unsigned)((m + 255) / 256);
  while (it < o.max_iters) {
    NP_HIP(hipEventRecord(dm.ev[0], st));
    NP_TRY(nearest_step(dX, dxn, m, Dp, dC[cur], k, ntiles, chunks, dCt, dbest, st));
    NP_HIP(hipEventRecord(dm.ev[1], st));
    NP_HIP(hipMemsetAsync(dcount, 0, (size_t)k * 4, st));
    NP_HIP(hipMemsetAsync(dcmax, 0, (size_t)k * 4, st));
    km_count_kernel<<<nb, 256, 0, st>>>(dbest, damax, m, dassign, dcount, dcmax);
    NP_HIP(hipGetLastError());
    NP_HIP(hipMemcpyAsync(counts.data(), dcount, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    NP_HIP(hipStreamSynchronize(st));
    // offsets, and the re-initialisation draws in ascending cluster order
    off[0] = 0;
    for (int64_t c = 0; c < k; ++c) {
      off[(size_t)c + 1] = off[(size_t)c] + counts[(size_t)c];
      reinit[(size_t)c] = -1;
      if (counts[(size_t)c] == 0) {
        reinit[(size_t)c] = (int32_t)rng.below((uint64_t)m);
        ++n_reinit;
      }
    }
    NP_HIP(hipMemcpyAsync(doff, off.data(), (size_t)(k + 1) * 4, hipMemcpyHostToDevice, st));
    NP_HIP(hipMemcpyAsync(dreinit, reinit.data(), (size_t)k * 4, hipMemcpyHostToDevice, st));
    NP_HIP(hipMemsetAsync(dcursor, 0, (size_t)k * 4, st));
    km_scatter_kernel<<<nb, 256, 0, st>>>(dassign, m, doff, dcursor, dorder);
    switch (Dp) {
      case 32: launch_mean<32>(dX, dorder, doff, dreinit, dcmax, dC[cur], dC[cur ^ 1], dpart, k, st); break;
      case 64: launch_mean<64>(dX, dorder, doff, dreinit, dcmax, dC[cur], dC[cur ^ 1], dpart, k, st); break;
      case 96: launch_mean<96>(dX, dorder, doff, dreinit, dcmax, dC[cur], dC[cur ^ 1], dpart, k, st); break;
      default: launch_mean<128>(dX, dorder, doff, dreinit, dcmax, dC[cur], dC[cur ^ 1], dpart, k, st); break;
    }
    km_shift_kernel<<<1, 1024, 0, st>>>(dpart, k, dshift);
    NP_HIP(hipGetLastError());
    NP_HIP(hipEventRecord(dm.ev[2], st));
    NP_HIP(hipMemcpyAsync(&shift, dshift, 8, hipMemcpyDeviceToHost, st));
    NP_HIP(hipStreamSynchronize(st));
    float t_a = 0.f, t_u = 0.f, t_h = 0.f;
    NP_HIP(hipEventElapsedTime(&t_a, dm.ev[0], dm.ev[1]));
    NP_HIP(hipEventElapsedTime(&t_u, dm.ev[1], dm.ev[2]));
    (void)t_h;
    ms_assign += t_a;
    ms_update += t_u;
    cur ^= 1;
    ++it;
    if (shift < o.tol) break;
  }
  std::vector<float> cout((size_t)k * Dp);
  NP_HIP(hipMemcpyAsync(cout.data(), dC[cur], (size_t)k * Dp * 4, hipMemcpyDeviceToHost, st));
  std::vector<int32_t> asg;
  if (out_assign && it > 0) {
    asg.resize((size_t)m);
    NP_HIP(hipMemcpyAsync(asg.data(), dassign, (size_t)m * 4, hipMemcpyDeviceToHost, st));
  }
  NP_HIP(hipStreamSynchronize(st));
  for (int64_t c = 0; c < k; ++c) memcpy(out_centroids + c * dim, &cout[(size_t)(c * Dp)], (size_t)dim * 4);
  if (out_assign) {
    for (int64_t i = 0; i < n; ++i) out_assign[i] = -1;
    if (it > 0)
      for (int64_t j = 0; j < m; ++j) out_assign[src_row(j)] = asg[(size_t)j];
  }
  if (rep) {
    memset(rep, 0, sizeof *rep);
    rep->iterations = it;
    rep->shift = shift;
    rep->n_points = m;
    rep->n_reinit = n_reinit;
    rep->ms_assign = ms_assign;
    rep->ms_update = ms_update;
  }
  return NP_OK;
}

np_index_config with_defaults(const np_index_config* c) {
  np_index_config o{};
  if (c) o = *c;
  if (o.nbits == 0) o.nbits = 4;
  if (o.kmeans_niters == 0) o.kmeans_niters = 4;
  if (o.batch_size == 0) o.batch_size = 50000;
  if (!c) o.seed = 42;
  if (o.max_points_per_centroid == 0) o.max_points_per_centroid = 256;
  if (o.start_from_scratch == 0) o.start_from_scratch = 999;
  return o;
}

int check_docs(const int64_t* doc_lengths, int64_t n_docs, int64_t* total) {
  if (n_docs <= 0 || !doc_lengths) {
    set_error("Index creation failed: No documents provided");
    return NP_ERR_INDEX_CREATION;
  }
  int64_t T = 0;
  for (int64_t d = 0; d < n_docs; ++d) {
    if (doc_lengths[d] < 0) {
      set_error("Index creation failed: negative document length at %lld", (long long)d);
      return NP_ERR_INVALID_ARGUMENT;
    }
    T += doc_lengths[d];
  }
  *total = T;
  return NP_OK;
}

int make_plan(const int64_t* doc_lengths, int64_t N, const np_index_config& cfg, np_kmeans_plan* p,
              std::vector<int64_t>* sample) {
  int64_t T = 0;
  NP_TRY(check_docs(doc_lengths, N, &T));
  memset(p, 0, sizeof *p);
  int64_t ns = cfg.n_samples_kmeans > 0 ? cfg.n_samples_kmeans
                                        : (int64_t)std::min(1.0 + 16.0 * sqrt(120.0 * (double)N), (double)N);   // kmeans.rs:273-276
  ns = std::min(ns, N);
  std::vector<int64_t> perm = shuffled_docs(N, cfg.seed);
  int64_t st = 0;
  for (int64_t i = 0; i < ns; ++i) st += doc_lengths[perm[(size_t)i]];
  int64_t K = cfg.num_partitions;
  if (K <= 0) {   // kmeans.rs:303-309; Rust's saturating f64 -> u32 cast makes anything below 1 give 2^0
    const double avg = ns > 0 ? (double)st / (double)ns : 0.0;
    const double v = floor(log2(16.0 * sqrt(avg * (double)N)));
    K = (int64_t)1 << (int)(v >= 1.0 ? std::min(v, 62.0) : 0.0);
  }
  p->n_samples = ns;
  p->sample_tokens = st;
  p->num_partitions = K;
  p->k = std::min(K, st);
  p->codec_samples = std::max<int64_t>(1, std::min<int64_t>(N, (int64_t)(16.0 * sqrt(120.0 * (double)N))));   // index.rs:199-201
  p->heldout_size = (int64_t)std::min(0.05 * (double)T, 50000.0);
  int64_t got = 0;
  for (int64_t i = p->codec_samples - 1; i >= 0 && got < p->heldout_size; --i)
    got += std::min(p->heldout_size - got, doc_lengths[perm[(size_t)i]]);
  p->heldout_tokens = got;
  if (sample) {
    perm.resize((size_t)std::max(ns, p->codec_samples));
    *sample = std::move(perm);
  }
  return NP_OK;
}

std::vector<int64_t> doc_offsets(const int64_t* doc_lengths, int64_t N) {
  std::vector<int64_t> off((size_t)N + 1, 0);
  for (int64_t d = 0; d < N; ++d) off[(size_t)d + 1] = off[(size_t)d] + doc_lengths[d];
  return off;
}

int compute_kmeans_impl(int device, const float* emb, const int64_t* doc_lengths, int64_t N, int dim,
                        const np_index_config& cfg, std::vector<float>* cen, int64_t* k_out, np_kmeans_report* rep) {
  np_kmeans_plan p;
  std::vector<int64_t> sample;
  NP_TRY(make_plan(doc_lengths, N, cfg, &p, &sample));
  NP_TRY(check_dim(dim));
  if (p.k == 0) {
    set_error("Index creation failed: Cannot compute 0 centroids");
    return NP_ERR_INDEX_CREATION;
  }
  if (!emb) {
    set_error("compute_kmeans: embeddings are NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const std::vector<int64_t> off = doc_offsets(doc_lengths, N);
  std::vector<float> pts((size_t)p.sample_tokens * dim);
  int64_t r = 0;
  for (int64_t i = 0; i < p.n_samples; ++i) {   // the sampled documents' tokens in shuffled order
    const int64_t d = sample[(size_t)i], l = doc_lengths[d];
    memcpy(&pts[(size_t)(r * dim)], emb + off[(size_t)d] * dim, (size_t)(l * dim) * 4);
    r += l;
  }
  np_kmeans_opts ko{};
  ko.k = p.k;
  ko.max_points_per_centroid = cfg.max_points_per_centroid;
  ko.seed = cfg.seed;
  ko.tol = 1e-8;
  ko.max_iters = cfg.kmeans_niters;
  cen->assign((size_t)p.k * dim, 0.f);
  NP_TRY(kmeans_run(device, pts.data(), p.sample_tokens, dim, ko, nullptr, cen->data(), nullptr, rep));
  for (int64_t c = 0; c < p.k; ++c) {   // F.normalize(centroids, dim=-1)
    float* row = cen->data() + c * dim;
    float ss = 0.f;
    for (int j = 0; j < dim; ++j) ss = fmaf(row[j], row[j], ss);
    const float nrm = std::max(sqrtf(ss), 1e-12f);
    for (int j = 0; j < dim; ++j) row[j] /= nrm;
  }
  *k_out = p.k;
  return NP_OK;
}

// a device handle that holds only the codec (one one-token document): np_hip_encode_tokens against these centroids
int codec_handle(int device, const float* centroids, int64_t k, int dim, int nbits, const float* weights, np_index** out) {
  std::vector<int32_t> il((size_t)k, 0);
  il[0] = 1;
  const int64_t ivf = 0, dl = 1, code = 0;
  std::vector<uint8_t> res((size_t)std::max(1, dim * nbits / 8), 0);
  std::vector<float> w((size_t)1 << nbits, 0.f);
  np_index_arrays a{};
  a.num_documents_total = 1;
  a.num_docs = 1;
  a.num_centroids = k;
  a.dim = dim;
  a.nbits = nbits;
  a.centroids = centroids;
  a.bucket_weights = weights ? weights : w.data();
  a.ivf = &ivf;
  a.ivf_lengths = il.data();
  a.doc_lengths = &dl;
  a.codes = &code;
  a.residuals = res.data();
  np_open_opts o{};
  o.device = device;
  o.n_contexts = 1;
  return np_hip_index_from_arrays(&a, &o, out);
}

struct HandleCloser {
  np_index* h = nullptr;
  ~HandleCloser() {
    if (h) np_hip_index_close(h);
  }
};

int codec_artifacts_impl(int device, const float* emb, const int64_t* doc_lengths, int64_t N, int dim,
                         const float* centroids, int64_t k, const np_index_config& cfg, std::vector<float>* cut,
                         std::vector<float>* wts, std::vector<float>* avg, float* thr) {
  np_kmeans_plan p;
  std::vector<int64_t> sample;
  NP_TRY(make_plan(doc_lengths, N, cfg, &p, &sample));
  NP_TRY(check_dim(dim));
  if (!emb || !centroids || k <= 0) {
    set_error("prepare_codec_artifacts: embeddings / centroids missing");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const int nbits = cfg.nbits;
  if (nbits <= 0 || 8 % nbits != 0 || (dim * nbits) % 8 != 0) {   // ResidualCodec::new (codec.rs:161-166)
    set_error("Codec error: nbits %d does not fit dim %d", nbits, dim);
    return NP_ERR_CODEC;
  }
  const std::vector<int64_t> off = doc_offsets(doc_lengths, N);
  // held-out tokens: the codec sample walked in reverse, the first rows of each document (index.rs:213-226)
  const int64_t H = p.heldout_tokens;
  std::vector<float> held((size_t)std::max<int64_t>(H, 1) * dim);
  int64_t got = 0;
  for (int64_t i = p.codec_samples - 1; i >= 0 && got < p.heldout_size; --i) {
    const int64_t d = sample[(size_t)i], take = std::min(p.heldout_size - got, doc_lengths[d]);
    memcpy(&held[(size_t)(got * dim)], emb + off[(size_t)d] * dim, (size_t)(take * dim) * 4);
    got += take;
  }
  NP_TRY(check_finite(held.data(), H * dim, dim));
  std::vector<int64_t> codes((size_t)std::max<int64_t>(H, 1));
  if (H > 0) {
    NP_TRY(check_build_device(device));
    HandleCloser hc;
    NP_TRY(codec_handle(device, centroids, k, dim, nbits, nullptr, &hc.h));
    std::vector<float> zc(((size_t)1 << nbits) - 1, 0.f);
    std::vector<uint8_t> packed((size_t)H * dim * nbits / 8);
    NP_TRY(np_hip_encode_tokens(hc.h, held.data(), H, dim, zc.data(), codes.data(), packed.data()));
  }
  std::vector<float> dist((size_t)H), flat((size_t)H * dim);
  std::vector<float> sabs((size_t)dim, 0.f);
  {
#pragma clang fp contract(off)
    for (int64_t i = 0; i < H; ++i) {
      const float* c = centroids + codes[(size_t)i] * dim;
      float ss = 0.f;
      for (int j = 0; j < dim; ++j) {
        const float r = held[(size_t)(i * dim + j)] - c[j];
        flat[(size_t)(i * dim + j)] = r;
        ss += r * r;
        sabs[(size_t)j] += fabsf(r);
      }
      dist[(size_t)i] = sqrtf(ss);
    }
  }
  std::sort(dist.begin(), dist.end());
  *thr = quantile_sorted(dist, 0.75);
  avg->resize((size_t)dim);
  for (int j = 0; j < dim; ++j) (*avg)[(size_t)j] = sabs[(size_t)j] / (float)H;   // 0 / 0 = NaN with no held-out rows, as the crate
  std::sort(flat.begin(), flat.end());
  const int nopt = 1 << nbits;
  cut->resize((size_t)nopt - 1);
  wts->resize((size_t)nopt);
  for (int i = 1; i < nopt; ++i) (*cut)[(size_t)i - 1] = quantile_sorted(flat, (double)i / (double)nopt);
  for (int i = 0; i < nopt; ++i) (*wts)[(size_t)i] = quantile_sorted(flat, ((double)i + 0.5) / (double)nopt);
  return NP_OK;
}

}  // namespace

// ---- the update path's device work (np_update.cpp) ----------------------------------------------------------------------
int build_check_device(int device) { return check_build_device(device); }
int build_check_dim(int dim) { return check_dim(dim); }
int build_check_finite(const float* x, int64_t count, int dim) { return check_finite(x, count, dim); }
float quantile_of_sorted(const std::vector<float>& v, double q) { return quantile_sorted(v, q); }

int find_outliers(int device, const float* X, int64_t n, int dim, const float* C, int64_t k, float thr,
                  std::vector<int64_t>* out, int64_t* n_rechecked) {
  out->clear();
  if (n_rechecked) *n_rechecked = 0;
  if (n <= 0 || k <= 0) return NP_OK;
  NP_TRY(check_dim(dim));
  if (n >= ((int64_t)1 << 31)) {
    set_error("Update failed: the outlier search takes fewer than 2^31 tokens, got %lld", (long long)n);
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(check_build_device(device));
  DeviceGuard g(device);
  const int Dp = storage_dim(dim);
  const int64_t ntiles = (k + 31) / 32;
  std::vector<float> cpad((size_t)k * Dp, 0.f);
  float cn_max = 0.f;
  for (int64_t c = 0; c < k; ++c) {
    float ss = 0.f;
    for (int j = 0; j < dim; ++j) {
      const float v = C[c * dim + j];
      cpad[(size_t)(c * Dp + j)] = v;
      ss = fmaf(v, v, ss);
    }
    cn_max = std::max(cn_max, ss);
  }
  cn_max *= 1.0f + 1e-3f;   // the host chain's own rounding
  DevMem dm;
  NP_HIP(hipStreamCreateWithFlags(&dm.st, hipStreamNonBlocking));
  hipStream_t st = dm.st;
  float *dX, *dxn, *damax, *dC, *dCt;
  unsigned long long* dbest;
  uint8_t* dflag;
  int32_t *dlist, *dnlist;
  NP_TRY(dm.alloc(&dX, (size_t)n * Dp));
  NP_TRY(dm.alloc(&dxn, (size_t)n));
  NP_TRY(dm.alloc(&damax, (size_t)n));
  NP_TRY(dm.alloc(&dC, (size_t)k * Dp));
  NP_TRY(dm.alloc(&dCt, (size_t)ntiles * (Dp * 32 + 32) + 256));   // + 1 KiB: the last DMA piece reads past the tile
  NP_TRY(dm.alloc(&dbest, (size_t)n));
  NP_TRY(dm.alloc(&dflag, (size_t)n));
  NP_TRY(dm.alloc(&dlist, (size_t)n));
  NP_TRY(dm.alloc(&dnlist, 1));
  NP_TRY(upload_rows(dX, X, n, dim, Dp, nullptr, st));
  NP_HIP(hipMemcpyAsync(dC, cpad.data(), cpad.size() * 4, hipMemcpyHostToDevice, st));
  NP_HIP(hipMemsetAsync(dnlist, 0, 4, st));
  const unsigned nb = (unsigned)((n + 255) / 256);
  km_norm_kernel<<<nb, 256, 0, st>>>(dX, n, Dp, dxn, damax);
  NP_HIP(hipGetLastError());
  NP_TRY(nearest_step(dX, dxn, n, Dp, dC, k, ntiles, assign_chunks(device, n, ntiles), dCt, dbest, st));
  const float thr2 = thr * thr;
  const float rel = 4.0f * (float)(Dp + 2) * 0x1p-24f;
  ol_flag_kernel<<<nb, 256, 0, st>>>(dbest, dxn, n, thr2, rel, cn_max, dflag, dlist, dnlist);
  NP_HIP(hipGetLastError());
  int32_t nl = 0;
  NP_HIP(hipMemcpyAsync(&nl, dnlist, 4, hipMemcpyDeviceToHost, st));
  NP_HIP(hipStreamSynchronize(st));
  if (nl > 0) {
    ol_recheck_kernel<<<(unsigned)nl, 256, 0, st>>>(dX, Dp, dC, k, dlist, thr2, dflag);
    NP_HIP(hipGetLastError());
  }
  std::vector<uint8_t> flag((size_t)n);
  NP_HIP(hipMemcpyAsync(flag.data(), dflag, (size_t)n, hipMemcpyDeviceToHost, st));
  NP_HIP(hipStreamSynchronize(st));
  for (int64_t i = 0; i < n; ++i)
    if (flag[(size_t)i]) out->push_back(i);
  if (n_rechecked) *n_rechecked = nl;
  return NP_OK;
}

int kmeans_points_as_docs(int device, const float* pts, int64_t n, int dim, const np_index_config& cfg, int64_t k,
                          std::vector<float>* cen) {
  np_index_config c = with_defaults(&cfg);
  c.num_partitions = k;
  const std::vector<int64_t> ones((size_t)n, 1);
  int64_t kk = 0;
  return compute_kmeans_impl(device, pts, ones.data(), n, dim, c, cen, &kk, nullptr);
}

int encode_with_codec(int device, const float* C, int64_t K, int dim, int nbits, const float* weights, const float* cutoffs,
                      const float* X, int64_t T, int64_t* codes, uint8_t* packed, float* norms) {
  if (T <= 0) return NP_OK;
  HandleCloser hc;
  NP_TRY(codec_handle(device, C, K, dim, nbits, weights, &hc.h));
  return encode_tokens_impl(hc.h, X, T, dim, cutoffs, codes, packed, norms);
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_kmeans_plan(const int64_t* doc_lengths, int64_t n_docs, const np_index_config* cfg, np_kmeans_plan* out,
                       int64_t* out_sample_ids) {
  clear_error();
  if (!out) {
    set_error("np_hip_kmeans_plan: out is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const np_index_config c = with_defaults(cfg);
  std::vector<int64_t> sample;
  NP_TRY(make_plan(doc_lengths, n_docs, c, out, out_sample_ids ? &sample : nullptr));
  if (out_sample_ids) memcpy(out_sample_ids, sample.data(), (size_t)out->n_samples * 8);
  return NP_OK;
}

int np_hip_kmeans(int32_t device, const float* points, int64_t n, int32_t dim, const np_kmeans_opts* opts,
                  const float* init, float* out_centroids, int64_t* out_assign, np_kmeans_report* report) {
  clear_error();
  if (!opts) {
    set_error("np_hip_kmeans: opts is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  return kmeans_run(device, points, n, dim, *opts, init, out_centroids, out_assign, report);
}

int np_hip_compute_kmeans(int32_t device, const float* embeddings, const int64_t* doc_lengths, int64_t n_docs,
                          int32_t dim, const np_index_config* cfg, float* out_centroids, int64_t capacity_k,
                          int64_t* out_k, np_kmeans_report* report) {
  clear_error();
  const np_index_config c = with_defaults(cfg);
  std::vector<float> cen;
  int64_t k = 0;
  NP_TRY(compute_kmeans_impl(device, embeddings, doc_lengths, n_docs, dim, c, &cen, &k, report));
  if (!out_centroids || capacity_k < k) {
    set_error("compute_kmeans: out_centroids holds %lld rows, %lld needed", (long long)capacity_k, (long long)k);
    return NP_ERR_INVALID_ARGUMENT;
  }
  memcpy(out_centroids, cen.data(), cen.size() * 4);
  if (out_k) *out_k = k;
  return NP_OK;
}

int np_hip_prepare_codec_artifacts(int32_t device, const float* embeddings, const int64_t* doc_lengths, int64_t n_docs,
                                   int32_t dim, const float* centroids, int64_t k, const np_index_config* cfg,
                                   float* out_bucket_cutoffs, float* out_bucket_weights, float* out_avg_residual,
                                   float* out_cluster_threshold) {
  clear_error();
  const np_index_config c = with_defaults(cfg);
  std::vector<float> cut, wts, avg;
  float thr = 0.f;
  NP_TRY(codec_artifacts_impl(device, embeddings, doc_lengths, n_docs, dim, centroids, k, c, &cut, &wts, &avg, &thr));
  if (out_bucket_cutoffs) memcpy(out_bucket_cutoffs, cut.data(), cut.size() * 4);
  if (out_bucket_weights) memcpy(out_bucket_weights, wts.data(), wts.size() * 4);
  if (out_avg_residual) memcpy(out_avg_residual, avg.data(), avg.size() * 4);
  if (out_cluster_threshold) *out_cluster_threshold = thr;
  return NP_OK;
}

int np_hip_index_create(const char* index_dir, const float* embeddings, const int64_t* doc_lengths, int64_t n_docs,
                        int32_t dim, const np_index_config* cfg, const np_open_opts* opts, np_index** out) {
  clear_error();
  if (out) *out = nullptr;
  if (!index_dir) {
    set_error("np_hip_index_create: index_dir is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const np_index_config c = with_defaults(cfg);
  const int device = opts ? opts->device : 0;
  int64_t T = 0;
  NP_TRY(check_docs(doc_lengths, n_docs, &T));
  NP_TRY(check_dim(dim));
  if (T > 0 && !embeddings) {
    set_error("np_hip_index_create: embeddings are NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(check_finite(embeddings, T * dim, dim));
  NP_TRY(check_build_device(device));
  std::vector<float> cen;
  int64_t k = 0;
  NP_TRY(compute_kmeans_impl(device, embeddings, doc_lengths, n_docs, dim, c, &cen, &k, nullptr));
  std::vector<float> cut, wts, avg;
  float thr = 0.f;
  NP_TRY(codec_artifacts_impl(device, embeddings, doc_lengths, n_docs, dim, cen.data(), k, c, &cut, &wts, &avg, &thr));
  const int pd = dim * c.nbits / 8;
  std::vector<int64_t> codes((size_t)std::max<int64_t>(T, 1));
  std::vector<uint8_t> packed((size_t)std::max<int64_t>(T, 1) * pd);
  if (T > 0) {   // every token through np_hip_encode_tokens (codec.rs:297-411)
    HandleCloser hc;
    NP_TRY(codec_handle(device, cen.data(), k, dim, c.nbits, wts.data(), &hc.h));
    NP_TRY(np_hip_encode_tokens(hc.h, embeddings, T, dim, cut.data(), codes.data(), packed.data()));
  }
  np_index_arrays a{};
  a.num_documents_total = n_docs;
  a.num_docs = n_docs;
  a.num_centroids = k;
  a.dim = dim;
  a.nbits = c.nbits;
  a.centroids = cen.data();
  a.bucket_weights = wts.data();
  a.doc_lengths = doc_lengths;
  a.codes = codes.data();
  a.residuals = packed.data();
  np_write_opts wo{};
  wo.chunk_docs = c.batch_size;
  wo.bucket_cutoffs = cut.data();
  wo.avg_residual = avg.data();
  wo.cluster_threshold = thr;
  NP_TRY(np_hip_index_write_dir(index_dir, &a, &wo));
  if (n_docs <= c.start_from_scratch) {   // update.rs:308-346 save_embeddings_npy
    const std::string dir = index_dir;
    const int64_t shape[2] = {T, dim};
    NP_TRY(write_npy_file(dir + "/embeddings.npy", "<f4", shape, 2, embeddings, (size_t)(T * dim) * 4));
    std::string js = "[";
    for (int64_t d = 0; d < n_docs; ++d) js += (d ? "," : "") + std::to_string((long long)doc_lengths[d]);
    js += "]";
    NP_TRY(write_text_file(dir + "/embeddings_lengths.json", js));
  }
  if (out) NP_TRY(np_hip_index_open(index_dir, opts, out));
  return NP_OK;
}

}  // extern "C"
