// np_index.hip -- makes a next-plaid index (or one document shard of it) resident in HBM.
//
// Replaces the in-memory half of MmapIndex::load (next-plaid/src/index.rs:1089-1139): ivf_offsets and
// doc_offsets prefix sums, the codec tables (codec.rs:154-225), and -- instead of mmap'ing
// merged_codes/merged_residuals -- device arrays laid out for the search kernels (np_internal.h).
// Also: the seeded synthetic corpus generator (bench / scale tests) and export back to host.
#include "np_internal.h"
#include "np_remove_plan.h"
#include "np_attach_plan.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <memory>
#include <thread>
#include <math.h>
#include <stdio.h>
#include <time.h>
#include <stdlib.h>
#include <string.h>

namespace np {

int DevBuf::reserve(size_t bytes) {
  if (bytes <= cap) return NP_OK;
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  size_t want = bytes + (bytes >> 3) + 256;
  hipError_t e = hipMalloc(&p, want);
  if (e != hipSuccess) {
    p = nullptr;
    set_error("hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
    return NP_ERR_OUT_OF_MEMORY;
  }
  cap = want;
  return NP_OK;
}
void DevBuf::release() {
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
}

void shard_range(int64_t n_total, int rank, int count, int64_t* b, int64_t* e) {
  if (count <= 1) {
    *b = 0;
    *e = n_total;
    return;
  }
  *b = (int64_t)((__int128)n_total * rank / count);
  *e = (int64_t)((__int128)n_total * (rank + 1) / count);
}

int normalise_opts(const np_open_opts* in, np_open_opts* o) {
  memset(o, 0, sizeof *o);
  if (in) *o = *in;
  if (o->shard_count <= 0) o->shard_count = 1;
  if (o->shard_rank < 0 || o->shard_rank >= o->shard_count) {
    set_error("Invalid configuration: shard_rank %d out of range for shard_count %d", o->shard_rank, o->shard_count);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (o->n_contexts <= 0) o->n_contexts = 2;
  if (o->n_contexts > 16) o->n_contexts = 16;
  if (o->max_batch <= 0) o->max_batch = 64;
  if (o->max_query_tokens <= 0) o->max_query_tokens = 64;
  // workspace_bytes <= 0: chosen when the index is resident (default_workspace: up to 16 GiB per context of what is free)
  return NP_OK;
}

// One clamp table for the environment (read once at open) and np_hip_index_tune().  Returns false for an unknown name.
bool set_tuning(Tuning* t, const std::string& n, int value) {
  auto clamp = [](int v, int lo, int hi) { return std::min(std::max(v, lo), hi); };
  if (n == "s4_mode") t->s4_mode = clamp(value, 0, 8);
  else if (n == "s4_minb") t->s4_minb = std::max(value, 1);
  else if (n == "s4_nbx") t->s4_nbx = clamp(value, 8, 512);
  else if (n == "s4_swz") t->s4_swz = value != 0;
  else if (n == "s4_filter") t->s4_filter = value != 0;
  else if (n == "s4_hot") t->s4_hot = clamp(value, 0, 500);
  else if (n == "s4_planes") t->s4_planes = value != 0;
  else if (n == "s4_pexp") t->s4_pexp = clamp(value, 5, 40);
  else if (n == "s4_lpd") t->s4_lpd = value == 2 ? 2 : 4;
  else if (n == "s4_qm") t->s4_qm = value != 0;
  else if (n == "s4_pnbx") t->s4_pnbx = clamp(value, 8, 512);
  else if (n == "s3_slices") t->s3_slices = value != 0;
  else if (n == "s4_warm") t->s4_warm = clamp(value, 0, 1000);
  else if (n == "ub_ncut") t->ub_ncut = clamp(value, 1, 512);
  else if (n == "s3_bisect") t->s3_bisect = clamp(value, 0, 1);
  else if (n == "s3_gain") t->s3_gain = clamp(value, 0, 2);
  else if (n == "s3_gain_mult") t->s3_gain_mult = clamp(value, 1, 16);
  else if (n == "s3_gain_direct") t->s3_gain_direct = clamp(value, 0, 64);
  else if (n == "s4_hot_auto") t->s4_hot_auto = clamp(value, 0, 0x7fffffff);
  else if (n == "ub_nt") t->ub_nt = value < 0 || value > 2 ? 0 : value;
  else if (n == "ub_steal") t->ub_steal = value < 1 ? 1 : value;
  else if (n == "ub_nbx") t->ub_nbx = clamp(value, 8, 256);
  else if (n == "ub_direct") t->ub_direct = clamp(value, 0, 16);
#ifdef NP_DIAGNOSTICS   // phase-skipping timing probe of the hot kernel: results are INVALID when != 0, so a production build has no way to set it
  else if (n == "s4_probe") t->s4_probe = clamp(value, 0, 7);
#endif
  else if (n == "ub_static") t->ub_static = value != 0;
  else if (n == "hot_static") t->hot_static = value != 0;
  else if (n == "s6_xcd") t->s6_xcd = value != 0;
  else if (n == "s6_tiles") t->s6_tiles = value != 0;
  else if (n == "s6_lds") t->s6_lds = clamp(value, 0, 2);
  else if (n == "gemm_cpw") t->gemm_cpw = value == 2 ? 2 : 1;
  else if (n == "s1_split") t->s1_split = value != 0;
  else if (n == "exact_rowmax") t->exact_rowmax = value != 0;
  else if (n == "scan_tiles") t->scan_tiles = clamp(value, 1, 8);
  else if (n == "scan_docs") t->scan_docs = std::max(value, 0);
  else if (n == "match_lds") t->match_lds = clamp(value, 0, 40);
  else if (n == "remove_slab") t->remove_slab = std::max(value, 0);
  else if (n == "expand_fail") t->expand_fail = clamp(value, 0, 4);
  else return false;
  return true;
}

void read_tuning_env(Tuning* t) {
  static const char* const knobs[][2] = {
      {"NP_S4_MODE", "s4_mode"}, {"NP_S4_MINB", "s4_minb"}, {"NP_S4_NBX", "s4_nbx"}, {"NP_S4_SWZ", "s4_swz"},
      {"NP_S4_FILTER", "s4_filter"}, {"NP_S4_HOT", "s4_hot"}, {"NP_S4_PLANES", "s4_planes"}, {"NP_S4_PEXP", "s4_pexp"}, {"NP_S4_LPD", "s4_lpd"}, {"NP_S4_QM", "s4_qm"}, {"NP_S4_PNBX", "s4_pnbx"}, {"NP_S4_WARM", "s4_warm"}, {"NP_UB_NCUT", "ub_ncut"}, {"NP_S3_BISECT", "s3_bisect"}, {"NP_S3_GAIN", "s3_gain"}, {"NP_S3_GAIN_MULT", "s3_gain_mult"}, {"NP_S3_GAIN_DIRECT", "s3_gain_direct"}, {"NP_S4_HOT_AUTO", "s4_hot_auto"}, {"NP_S3_SLICES", "s3_slices"}, {"NP_UB_NT", "ub_nt"},
      {"NP_UB_STEAL", "ub_steal"}, {"NP_UB_NBX", "ub_nbx"}, {"NP_UB_DIRECT", "ub_direct"}, {"NP_UB_STATIC", "ub_static"}, {"NP_HOT_STATIC", "hot_static"}, {"NP_S6_XCD", "s6_xcd"}, {"NP_S6_TILES", "s6_tiles"}, {"NP_S6_LDS", "s6_lds"}, {"NP_GEMM_CPW", "gemm_cpw"}, {"NP_S1_SPLIT", "s1_split"},
      {"NP_EXACT_ROWMAX", "exact_rowmax"}, {"NP_SCAN_TILES", "scan_tiles"}, {"NP_SCAN_DOCS", "scan_docs"}, {"NP_MATCH_LDS", "match_lds"}};
  for (const auto& k : knobs) {
    const char* e = getenv(k[0]);
    if (e && *e) (void)set_tuning(t, k[1], atoi(e));
  }
#ifdef NP_DIAGNOSTICS
  if (const char* e = getenv("NP_S4_PROBE")) (void)set_tuning(t, "s4_probe", atoi(e));
#endif
}

// Default per-context scratch budget: what the device has free once the index is resident, shared by the contexts, between
// 2 and 16 GiB.  The candidate pool is sized by it; the host enqueues the worst-case number of pool rounds of a batch
// (B x n_docs entries / pool) and the empty ones cost ~45 us of launches each: 16 GiB is 3 rounds at 10 M documents where
// 8 GiB was 6.  A 12.5 M x 300-token shard (268 GB) leaves 12 GiB per context with three contexts.
static void default_workspace(DeviceIndex* ix) {
  ix->ws_auto = ix->opts.workspace_bytes <= 0;
  ix->ws_budget = ix->opts.workspace_bytes;
  ix->ws_budget_open = ix->opts.workspace_bytes;
  if (!ix->ws_auto) return;
  size_t free_b = 0, total_b = 0;
  int64_t ws = (int64_t)8 << 30;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
    const int64_t share = ((int64_t)free_b - ((int64_t)4 << 30)) / std::max(ix->opts.n_contexts, 1);
    ws = std::min<int64_t>((int64_t)16 << 30, std::max<int64_t>((int64_t)2 << 30, share));
  }
  ix->opts.workspace_bytes = ws;
  ix->ws_budget = ws;
  ix->ws_budget_open = ws;
}

static int check_device(int dev) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    set_error("no HIP device available");
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  if (dev < 0 || dev >= n) {
    set_error("device %d out of range (%d devices)", dev, n);
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  return NP_OK;
}

void destroy_device_index(np_index* ix) {
  if (!ix) return;
  DeviceGuard g(ix->device);   // the arrays' owners free them on the current device
  for (Context* c : ix->contexts) destroy_context(c);
  delete ix;
}

// a handle being opened: closed on every early return, handed out with release() when the open succeeds
struct CloseIndex {
  void operator()(np_index* p) const { destroy_device_index(p); }
};
using IndexHandle = std::unique_ptr<np_index, CloseIndex>;

static uint32_t bitrev(uint32_t v, int nbits) {
  uint32_t r = 0;
  for (int k = 0; k < nbits; ++k)
    if (v & (1u << k)) r |= 1u << (nbits - 1 - k);
  return r;
}

static int check_geometry(int64_t K, int dim, int nbits, int64_t n_total) {
  if (nbits <= 0 || 8 % nbits != 0) {  // codec.rs:161-166
    set_error("Codec error: nbits must be a divisor of 8, got %d", nbits);
    return NP_ERR_CODEC;
  }
  if (K <= 0 || dim <= 0) {
    set_error("Shape error: centroids must be [K > 0, dim > 0], got [%lld, %d]", (long long)K, dim);
    return NP_ERR_SHAPE;
  }
  if ((dim * nbits) % 8 != 0) {
    set_error("Shape error: dim*nbits must be a multiple of 8 (dim=%d nbits=%d)", dim, nbits);
    return NP_ERR_SHAPE;
  }
  if (K >= ((int64_t)1 << 31) || n_total >= ((int64_t)1 << 32) - 1) {
    set_error("Index load failed: K=%lld / N=%lld exceed the 32-bit device id space", (long long)K, (long long)n_total);
    return NP_ERR_INDEX_LOAD;
  }
  return NP_OK;
}

// largest squared row norm of the centroid table (bit pattern of a non-negative float orders like the float) and a
// non-finite flag: |Q.c| <= ||q|| * cmax scales the u8 table of the S4 upper-bound filter (np_kernels.h)
__global__ void __launch_bounds__(256) centroid_bound_kernel(const float* __restrict__ C, int64_t K, int dim,
                                                             uint32_t* __restrict__ out /* [0] max bits, [1] non-finite */) {
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= K) return;
  float ss = 0.f;
  for (int j = lane; j < dim; j += 64) {
    const float x = C[c * dim + j];
    ss = fmaf(x, x, ss);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  if (lane == 0) {
    if ((__float_as_uint(ss) & 0x7F800000u) == 0x7F800000u) atomicOr(&out[1], 1u);
    else atomicMax(&out[0], __float_as_uint(ss));
  }
}

// k rows of the caller's centroids (file geometry) into storage rows at dst
static int upload_centroid_rows(const DeviceIndex* ix, const float* centroids, int64_t k, float* dst) {
  if (k <= 0) return NP_OK;
  if (ix->ldim == ix->dim) {
    NP_HIP(hipMemcpy(dst, centroids, (size_t)k * ix->dim * sizeof(float), hipMemcpyHostToDevice));
  } else {   // rows zero-padded to the storage width (np_internal.h storage_dim)
    NP_HIP(hipMemset(dst, 0, (size_t)k * ix->dim * sizeof(float)));
    NP_HIP(hipMemcpy2D(dst, (size_t)ix->dim * sizeof(float), centroids, (size_t)ix->ldim * sizeof(float),
                       (size_t)ix->ldim * sizeof(float), (size_t)k, hipMemcpyHostToDevice));
  }
  return NP_OK;
}

// cmax and filter_ok of a centroid table in storage rows (a maximum and an OR: the same for any order of the rows' visits)
static int centroid_bounds(const float* d_centroids, int64_t K, int dim, float* cmax, bool* filter_ok) {
  DevPtr<uint32_t> d_b;
  uint32_t h_b[2] = {0, 0};
  NP_TRY(d_b.alloc(2));
  NP_HIP(hipMemset(d_b.get(), 0, 8));
  centroid_bound_kernel<<<(unsigned)((K + 3) / 4), 256>>>(d_centroids, K, dim, d_b.get());
  NP_HIP(hipMemcpy(h_b, d_b.get(), 8, hipMemcpyDeviceToHost));
  float ss;
  memcpy(&ss, &h_b[0], 4);
  *cmax = sqrtf(ss) * 1.0001f;   // the f32 sum of squares is within ~dim * 2^-24 of the real one
  *filter_ok = h_b[1] == 0;
  return NP_OK;
}

static int upload_codec(DeviceIndex* ix, const float* centroids, const float* bucket_weights) {
  NP_TRY(ix->d_centroids.alloc((size_t)ix->K * ix->dim, &ix->device_bytes));
  NP_TRY(upload_centroid_rows(ix, centroids, ix->K, ix->d_centroids.get()));
  NP_TRY(centroid_bounds(ix->d_centroids.get(), ix->K, ix->dim, &ix->cmax, &ix->filter_ok));
  const int nb = 1 << ix->nbits, lnb = 1 << ix->lnbits;
  std::vector<float> wl(nb);
  for (int s = 0; s < nb; ++s) {   // 1-bit files stored as 2-bit: buckets 2 and 3 never occur
    const uint32_t b = bitrev((uint32_t)s, ix->nbits);
    wl[s] = b < (uint32_t)lnb ? bucket_weights[b] : 0.f;
  }
  bool wok = true;
  for (int s = 0; s < nb; ++s) wok = wok && std::isfinite(wl[s]) && std::fabs(wl[s]) < 1e6f;
  ix->s6_fast_ok = ix->filter_ok && ix->cmax < 1e6f && wok;
  ix->pad_ss = ix->dim > ix->ldim ? (float)(ix->dim - ix->ldim) * (wl[0] * wl[0]) : 0.f;
  NP_TRY(ix->d_wlut.alloc(nb, &ix->device_bytes));
  NP_HIP(hipMemcpy(ix->d_wlut.get(), wl.data(), nb * sizeof(float), hipMemcpyHostToDevice));
  return NP_OK;
}


// ---- derived: per-document distinct codes (one block per document, bitonic sort in LDS) ------------------
// Two passes over the same kernel: with ucodes == NULL it only counts (ulen[d]); the host then lays the lists out DENSELY
// (exclusive scan of the lengths, each list start rounded up to NP_ULIST_ALIGN entries so that list reads of 8 bytes stay
// aligned) and the second pass writes list d at uoff[d].  (Round 2 kept each list at its document's token offset: T
// entries of 4 bytes for ~T/4 useful ones, 4 B per token of HBM.)
#define NP_UNIQ_MAX 4096
#define NP_ULIST_ALIGN 4
__global__ void __launch_bounds__(256) unique_codes_kernel(const int64_t* __restrict__ doc_off, CodeArr codes,
                                                           void* __restrict__ ucodes, const int64_t* __restrict__ uoff,
                                                           int32_t* __restrict__ ulen) {
  __shared__ uint32_t s[NP_UNIQ_MAX];
  __shared__ int s_wave[4];
  const int64_t d = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t off = doc_off[d];
  const int len = (int)(doc_off[d + 1] - off);
  const int64_t uo = ucodes ? uoff[d] : 0;
  auto put = [&](int i, uint32_t c) {
    if (codes.wide) static_cast<uint32_t*>(ucodes)[uo + i] = c;
    else static_cast<uint16_t*>(ucodes)[uo + i] = (uint16_t)c;
  };
  if (len > NP_UNIQ_MAX) {  // very long document: keep the full list (still correct, just not shorter)
    if (ucodes)
      for (int i = tid; i < len; i += 256) put(i, codes[off + i]);
    else if (tid == 0) ulen[d] = len;
    return;
  }
  int n = 1;
  while (n < len) n <<= 1;
  for (int i = tid; i < n; i += 256) s[i] = (i < len) ? codes[off + i] : 0xFFFFFFFFu;
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < n; i += 256) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint32_t a = s[i], c = s[ixj];
          const bool asc = (i & k) == 0;
          if (asc ? (a > c) : (a < c)) { s[i] = c; s[ixj] = a; }
        }
      }
    }
  __syncthreads();
  int base = 0;
  for (int i0 = 0; i0 < len; i0 += 256) {
    const int i = i0 + tid;
    const bool head = i < len && (i == 0 || s[i] != s[i - 1]);
    const unsigned long long bal = __ballot(head);
    if (lane == 0) s_wave[wave] = (int)__popcll(bal);
    __syncthreads();
    int before = base;
    for (int k = 0; k < wave; ++k) before += s_wave[k];
    if (head && ucodes) put(before + (int)__popcll(bal & ((1ull << lane) - 1ull)), s[i]);
    base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  if (tid == 0 && !ucodes) ulen[d] = base;
}

// ---- list layout (round 3, second step): one fixed-stride BLOCK per document + an overflow region ---------------------
// d_ucodes = [ n_docs blocks of S entries | overflow lists ].  Block d = a 16-byte header {u32 #distinct codes, u32
// document length, u32 overflow index, u32 0} followed by the document's sorted distinct codes when they fit the block
// (#distinct <= S - HDR entries); a longer list lives in the overflow region (4-entry aligned, at overflow index * 4) and
// the block carries only the header.  S is chosen at open: a multiple of 64 bytes that holds 99 % of the lists (at most 256
// bytes: one 8-byte load per lane of half a wave).  With the block address computable from the document id, the hot level of the
// S4 filter needs NO per-candidate record: S3 hands it bare document ids and the 16-byte record gather of compact_kernel
// (one 128-byte line per candidate at 1.9 % density, 0.32 ms per batch at 10 M documents) disappears; the header arrives
// with the list.  Every other consumer keeps addressing lists through the 40-bit offset of doc_meta / the records.
#define NP_UBLOCK_MAX_U16 128   // entries (256 B: one 8-byte load per lane of half a wave): 8 header + 120 codes
#define NP_UBLOCK_MAX_U32 64    // entries (256 B): 4 header + 60 codes
// with the bit-plane hot level (approx_hotp_kernel, LPD = 4: a whole wave stages a block) blocks go up to 512 bytes, so that a
// corpus with 150-250 distinct codes per document (0.5-0.8 per token at 300 tokens) keeps its lists in the blocks
#define NP_UBLOCK_BIG_U16 256   // 8 header + 248 codes
#define NP_UBLOCK_BIG_U32 128   // 4 header + 124 codes
#define NP_ULEN_BINS 258        // list lengths 0..256, > 256

__global__ void ulen_hist_kernel(const int32_t* __restrict__ ulen, int64_t n, uint32_t* __restrict__ hist /* [NP_ULEN_BINS] */) {
  __shared__ uint32_t s_h[NP_ULEN_BINS];
  for (int i = threadIdx.x; i < NP_ULEN_BINS; i += blockDim.x) s_h[i] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&s_h[min(ulen[i], NP_ULEN_BINS - 1)], 1u);
  __syncthreads();
  for (int i = threadIdx.x; i < NP_ULEN_BINS; i += blockDim.x)
    if (s_h[i]) atomicAdd(&hist[i], s_h[i]);
}

// overflow entries of document i (its whole list, 4-entry aligned) or 0 when the list fits its block
__global__ void ulen_overflow_kernel(const int32_t* __restrict__ ulen, int64_t n, int fit, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = ulen[i] > fit ? ((int64_t)ulen[i] + NP_ULIST_ALIGN - 1) / NP_ULIST_ALIGN * NP_ULIST_ALIGN : 0;
}

// uoff[d] = entry offset of document d's list; the block header of d
__global__ void ublock_layout_kernel(int64_t n, const int64_t* __restrict__ doc_off, const int32_t* __restrict__ ulen,
                                     const int64_t* __restrict__ ovf_incl /* inclusive scan of the overflow sizes */,
                                     int S, int hdr, int fit, int64_t base_b, void* __restrict__ ucodes, int wide,
                                     int64_t* __restrict__ uoff) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n) return;
  const int32_t u = ulen[d];
  const bool ovf = u > fit;
  const int64_t ovf_size = ovf ? ((int64_t)u + NP_ULIST_ALIGN - 1) / NP_ULIST_ALIGN * NP_ULIST_ALIGN : 0;
  const int64_t ovf_excl = ovf_incl[d] - ovf_size;
  uoff[d] = ovf ? base_b + ovf_excl : d * (int64_t)S + hdr;
  uint4* h = reinterpret_cast<uint4*>(static_cast<char*>(ucodes) + d * (int64_t)S * (wide ? 4 : 2));
  *h = make_uint4((uint32_t)u, (uint32_t)(doc_off[d + 1] - doc_off[d]), ovf ? (uint32_t)(ovf_excl / NP_ULIST_ALIGN) : 0u, 0u);
}


// ---- derived layout: every document's tokens ordered by centroid code ------------------------------------------------
// S6 gathers one 128-B row of the query's score table per token (the MFMA C-in).  MaxSim is a max over the document's
// tokens, so their order is free: with the tokens of a document stored in code order, the 32 tokens of a tile name
// only a few distinct rows (the texture unit merges equal addresses of one instruction) and the gather traffic drops
// from one row per TOKEN to about one per DISTINCT code of the document.  codes / residuals are permuted in place at
// open (one workgroup per document, rows staged in LDS); tok_pos keeps the original position so that
// decompress_documents and np_hip_index_export return the on-disk order.  Documents longer than NP_SORT_MAX tokens
// stay as they are.  direction 1 = sort, 0 = restore the original order (export).
#define NP_SORT_MAX 512
template <typename CT>
__global__ void __launch_bounds__(256) sort_doc_tokens_kernel(const int64_t* __restrict__ doc_off, CT* __restrict__ codes,
                                                              uint8_t* __restrict__ residuals, uint16_t* __restrict__ tok_pos,
                                                              int pd, int to_sorted) {
  extern __shared__ uint64_t s_keys[];                        // [NP_SORT_MAX] (code << 32 | position)
  uint32_t* s_rows = reinterpret_cast<uint32_t*>(s_keys + NP_SORT_MAX);   // [len][pd / 4]
  const int tid = threadIdx.x;
  const int64_t off = doc_off[blockIdx.x];
  const int len = (int)(doc_off[blockIdx.x + 1] - off);
  if (len > NP_SORT_MAX) {
    if (to_sorted)
      for (int i = tid; i < len; i += 256) tok_pos[off + i] = (uint16_t)min(i, 65535);
    return;
  }
  if (len == 0) return;
  const int pw = pd / 4;                                       // dwords per residual row (pd is a multiple of 4 here)
  uint32_t* rows_g = reinterpret_cast<uint32_t*>(residuals + off * pd);
  for (int w = tid; w < len * pw; w += 256) s_rows[w] = rows_g[w];
  if (to_sorted) {
    int n = 1;
    while (n < len) n <<= 1;
    for (int i = tid; i < n; i += 256) s_keys[i] = (i < len) ? (((uint64_t)codes[off + i] << 32) | (uint64_t)i) : ~0ull;
    for (int k = 2; k <= n; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
          const int ixj = i ^ j;
          if (ixj > i) {
            const uint64_t a = s_keys[i], c = s_keys[ixj];
            const bool asc = (i & k) == 0;
            if (asc ? (a > c) : (a < c)) { s_keys[i] = c; s_keys[ixj] = a; }
          }
        }
      }
    __syncthreads();
    for (int i = tid; i < len; i += 256) {
      codes[off + i] = (CT)(s_keys[i] >> 32);
      tok_pos[off + i] = (uint16_t)(s_keys[i] & 0xFFFFu);
    }
    for (int w = tid; w < len * pw; w += 256) {
      const int i = w / pw, c = w - i * pw;
      rows_g[w] = s_rows[(int)(s_keys[i] & 0xFFFFFFFFull) * pw + c];
    }
  } else {
    for (int i = tid; i < len; i += 256) s_keys[i] = ((uint64_t)codes[off + i] << 32) | (uint64_t)tok_pos[off + i];
    __syncthreads();
    for (int i = tid; i < len; i += 256) codes[off + (int)(s_keys[i] & 0xFFFFull)] = (CT)(s_keys[i] >> 32);
    for (int w = tid; w < len * pw; w += 256) {
      const int i = w / pw, c = w - i * pw;
      rows_g[(int)(s_keys[i] & 0xFFFFull) * pw + c] = s_rows[w];
    }
  }
}

// documents [doc0, doc1) only: sorting a sorted document again would overwrite its tok_pos with the identity, so an append
// (np_hip_index_append) sorts the new documents and leaves the old ones alone
static int permute_tokens(const DeviceIndex* ix, int to_sorted, int64_t doc0, int64_t doc1) {
  if (doc1 <= doc0 || (ix->pd & 3)) return NP_OK;
  const size_t lds = (size_t)NP_SORT_MAX * 8 + (size_t)NP_SORT_MAX * ix->pd;
  if (lds > 48 * 1024) {
    NP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&sort_doc_tokens_kernel<uint16_t>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    NP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&sort_doc_tokens_kernel<uint32_t>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  for (int64_t d0 = doc0; d0 < doc1; d0 += (int64_t)1 << 30) {
    const int64_t n = std::min<int64_t>((int64_t)1 << 30, doc1 - d0);
    if (ix->code_wide)
      sort_doc_tokens_kernel<uint32_t><<<(unsigned)n, 256, lds>>>(ix->d_doc_offsets.get() + d0, (uint32_t*)ix->d_codes.get(),
                                                                  ix->d_residuals.get(), ix->d_tok_pos.get(), ix->pd, to_sorted);
    else
      sort_doc_tokens_kernel<uint16_t><<<(unsigned)n, 256, lds>>>(ix->d_doc_offsets.get() + d0, (uint16_t*)ix->d_codes.get(),
                                                                  ix->d_residuals.get(), ix->d_tok_pos.get(), ix->pd, to_sorted);
  }
  NP_HIP(hipGetLastError());
  NP_HIP(hipDeviceSynchronize());
  return NP_OK;
}

static int sort_tokens(DeviceIndex* ix) {
  const char* e = getenv("NP_TOK_SORT");
  // opt-in (NP_TOK_SORT=1): measured 1 % on S6 at 1M docs for 2 B/token of HBM, so the default keeps the on-disk order
  if (!(e && *e && atoi(e) != 0) || (ix->pd & 3)) return NP_OK;
  NP_TRY(ix->d_tok_pos.alloc((size_t)ix->T, &ix->device_bytes));
  NP_TRY(permute_tokens(ix, 1, 0, ix->n_docs));
  ix->tok_sorted = true;
  return NP_OK;
}

// ---- derived: 1 / ||centroid[code] + residual|| per token (codec.rs:443-467's normaliser) ------------------
// one wave per 64 consecutive tokens; lanes sweep the dims of one token at a time (coalesced rows)
__global__ void __launch_bounds__(256) inv_norm_kernel(int64_t T, int dim /* row stride */, int ldim /* dims that count */, int nbits, int pd,
                                                       const float* __restrict__ centroids,
                                                       const float* __restrict__ wlut,
                                                       CodeArr codes,
                                                       const uint8_t* __restrict__ residuals,
                                                       float* __restrict__ inv_norm) {
  const int lane = threadIdx.x & 63;
  const int64_t t0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
  const int per = 8 / nbits;
  const uint32_t mask = (1u << nbits) - 1u;
  float mine = 0.f;
  for (int i = 0; i < 64; ++i) {
    const int64_t tok = t0 + i;
    if (tok >= T) break;
    const uint32_t code = codes[tok];
    float ss = 0.f;
    for (int j = lane; j < ldim; j += 64) {
      const uint32_t byte = residuals[tok * pd + j / per];
      const int e = j % per;
      const float x = centroids[(int64_t)code * dim + j] + wlut[(byte >> (8 - nbits * (e + 1))) & mask];
      ss = fmaf(x, x, ss);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    if (lane == i) mine = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
  }
  if (t0 + lane < T) inv_norm[t0 + lane] = mine;
}

// ivf_split[c][r] = number of entries of posting list c with id < r * 32768 (r = 0 .. n_ranges): the zeroth filter level
// (gain_sweep_kernel, np_kernels.h) holds the accumulators of one 32768-document range per block and reads exactly its part of
// every probed list.  One thread per (list, boundary), a bisection each; ascending lists only.
#define NP_SPLIT_RANGE NP_IVF_SPLIT_RANGE
__global__ void __launch_bounds__(256) ivf_split_kernel(const uint32_t* __restrict__ ivf, const int64_t* __restrict__ ivf_off,
                                                        int64_t K, int R1, uint32_t* __restrict__ split) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= K * R1) return;
  const int64_t c = i / R1;
  const int r = (int)(i - c * R1);
  const int64_t s0 = ivf_off[c];
  const uint32_t len = (uint32_t)(ivf_off[c + 1] - s0);
  const uint64_t bound = (uint64_t)r * NP_SPLIT_RANGE;
  const uint32_t* L = ivf + s0;
  uint32_t a = 0, z = len;
  while (a < z) {
    const uint32_t mid = (a + z) >> 1;
    if ((uint64_t)L[mid] < bound) a = mid + 1;
    else z = mid;
  }
  split[i] = a;
}

// the planner's candidate bound (np_internal.h ivf_top_prefix), from the host copy of the list offsets
static void set_ivf_bound(DeviceIndex* ix, const int64_t* ioff) {
  const int64_t K = ix->K;
  std::vector<int64_t> len((size_t)K);
  for (int64_t c = 0; c < K; ++c) len[(size_t)c] = ioff[c + 1] - ioff[c];
  std::sort(len.begin(), len.end(), std::greater<int64_t>());
  ix->ivf_top_prefix.assign((size_t)K + 1, 0);
  for (int64_t c = 0; c < K; ++c) ix->ivf_top_prefix[(size_t)c + 1] = ix->ivf_top_prefix[(size_t)c] + len[(size_t)c];
}

// ---- derived: do the posting lists cover the codes? ------------------------------------------------------------------
// The zeroth filter level bounds a document's approximate score by the gains of the probed cells WHOSE LISTS HOLD IT, which
// is a bound only if every (document, distinct code c) pair is in list c.  The crate writes exactly these pairs
// (index.rs:479-504), but the reference only forms the candidate set from the lists (index.rs:1142-1156) and scores from the
// codes, so lists that miss a pair still make a defined index -- one the level would prune wrongly.  One wave per document
// bisects the document's id in the (ascending) list of each of its distinct codes and flags a pair that is not there.  The
// lists of documents longer than NP_UNIQ_MAX tokens are unsorted and keep duplicates: every entry is looked up all the same.
// Extra entries (a document in a list of a code it does not hold) only loosen the bound and are not flagged.
__global__ void __launch_bounds__(256) ivf_cover_kernel(int64_t n_docs, const uint4* __restrict__ meta, CodeArr ucodes,
                                                        const uint32_t* __restrict__ ivf, const int64_t* __restrict__ ivf_off,
                                                        int* __restrict__ missing) {
  const int64_t d = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= n_docs) return;
  const uint4 m = meta[d];
  const int64_t off = (int64_t)m.z | ((int64_t)(m.w & 0xFFu) << 32);
  bool miss = false;
  for (uint32_t j = threadIdx.x & 63; j < m.y; j += 64) {
    const uint32_t c = ucodes[off + j];
    const int64_t s0 = ivf_off[c], len = ivf_off[c + 1] - s0;
    int64_t a = 0, z = len;
    while (a < z) {
      const int64_t mid = (a + z) >> 1;
      if ((int64_t)ivf[s0 + mid] < d) a = mid + 1;
      else z = mid;
    }
    miss |= a == len || (int64_t)ivf[s0 + a] != d;
  }
  if (miss) *missing = 1;
}

// the documents, their distinct-code lists and the posting lists that the coverage check and the range table are about: the
// handle's own at open, the grown ones of an append before they are swapped in
struct ListsView {
  int64_t n_docs;
  int ublock_stride;
  const uint4* meta;
  CodeArr ucodes;
  const uint32_t* ivf;
  const int64_t* ivf_off;
};
static ListsView lists_of(const DeviceIndex* ix) {
  return ListsView{ix->n_docs, ix->ublock_stride, ix->d_doc_meta.get(), ix->ucodes(), ix->d_ivf.get(), ix->d_ivf_offsets.get()};
}

static int ivf_covers_codes(const ListsView& v, bool* covers) {
  *covers = false;
  DevPtr<int> d_missing;
  NP_TRY(d_missing.alloc(1));
  NP_HIP(hipMemset(d_missing.get(), 0, sizeof(int)));
  ivf_cover_kernel<<<(unsigned)((v.n_docs + 3) / 4), 256>>>(v.n_docs, v.meta, v.ucodes, v.ivf, v.ivf_off, d_missing.get());
  NP_HIP(hipGetLastError());
  int missing = 1;
  NP_HIP(hipMemcpy(&missing, d_missing.get(), sizeof(int), hipMemcpyDeviceToHost));
  *covers = missing == 0;
  return NP_OK;
}

// The range table of posting lists: *split and *R (no table: empty and 0), and *cover where the coverage was looked at.
// lists_cover: the caller knows that the lists hold every (document, distinct code) pair -- it built them from the distinct
// codes (build_ivf_from_ucodes), or appended such pairs to lists that did (np_hip_index_append)
static int make_ivf_split(const DeviceIndex* ix, const ListsView& v, bool lists_cover, DevPtr<uint32_t>* split, int* R, int* cover) {
  *R = 0;
  if (!ix->tune.s3_gain || !ix->tune.s4_planes || !ix->ivf_sorted || v.n_docs <= 0 || ix->K <= 0 || v.ublock_stride <= 0) return NP_OK;
  const int R_all = (int)((v.n_docs + NP_SPLIT_RANGE - 1) / NP_SPLIT_RANGE), R1 = R_all + 1;
  const size_t n = (size_t)ix->K * (size_t)R1;
  if (n * 4 > ((size_t)2 << 30)) return NP_OK;   // a table beyond 2 GiB (K x n_docs both huge) is not worth its HBM: the level stays off
  bool covers = lists_cover;
  if (!covers) NP_TRY(ivf_covers_codes(v, &covers));
  *cover = covers ? 1 : 0;
  if (!covers) return NP_OK;   // lists that miss a pair: no table, so the level stays off (np_search.hip gain_possible)
  NP_TRY(split->alloc(n));
  ivf_split_kernel<<<(unsigned)((n + 255) / 256), 256>>>(v.ivf, v.ivf_off, ix->K, R1, split->get());
  NP_HIP(hipGetLastError());
  NP_HIP(hipDeviceSynchronize());
  *R = R_all;
  return NP_OK;
}

static void install_ivf_split(DeviceIndex* ix, DevPtr<uint32_t>&& split, int R) {
  ix->device_bytes = ix->device_bytes - ix->d_ivf_split.bytes() + split.bytes();
  ix->d_ivf_split = std::move(split);
  ix->n_ranges = R;
}

static int build_ivf_split(DeviceIndex* ix, bool lists_cover) {
  DevPtr<uint32_t> split;
  int R = 0;
  NP_TRY(make_ivf_split(ix, lists_of(ix), lists_cover, &split, &R, &ix->ivf_cover));
  install_ivf_split(ix, std::move(split), R);
  return NP_OK;
}

// the inverse norms of tokens [t0, t1) into the (allocated) d_inv_norm: every token is computed on its own, so a range gives
// the same bits as the whole index does
static int fill_inv_norm(DeviceIndex* ix, int64_t t0, int64_t t1) {
  if (t1 > t0) {
    const int64_t n = t1 - t0, nblk = (n + 255) / 256;
    const CodeArr codes{ix->d_codes.get() + t0 * (int64_t)ix->code_bytes(), ix->code_wide};
    inv_norm_kernel<<<(unsigned)nblk, 256>>>(n, ix->dim, ix->ldim, ix->nbits, ix->pd, ix->d_centroids.get(), ix->d_wlut.get(), codes,
                                             ix->d_residuals.get() + t0 * ix->pd, ix->d_inv_norm.get() + t0);
  }
  NP_HIP(hipGetLastError());
  NP_HIP(hipDeviceSynchronize());
  return NP_OK;
}

static int build_inv_norm(DeviceIndex* ix) {
  if (ix->d_inv_norm.get()) {
    set_error("internal: inv_norm built twice");
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(ix->d_inv_norm.alloc((size_t)ix->T, &ix->device_bytes));
  return fill_inv_norm(ix, 0, ix->T);
}

// ---- derived: where each document's sorted distinct-code list crosses the eighths of the centroid range ----
// seg[d] = 8 x u16, seg[x] = number of distinct codes of d that are < (x+1)*ceil(K/8).  The sliced S4 kernel walks
// one eighth (or pair / quad of eighths) of every candidate at a time so that the slice of the query's score
// table it touches stays resident in one XCD's L2.
__global__ void __launch_bounds__(256) useg_kernel(int64_t n_docs, const int64_t* __restrict__ doc_off,
                                                   const int64_t* __restrict__ uoff, CodeArr ucodes,
                                                   const int32_t* __restrict__ ulen, uint32_t slice_w,
                                                   uint4* __restrict__ useg, int* __restrict__ bad) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= n_docs) return;
  const int64_t off = uoff[d];
  const int n = ulen[d];
  if (doc_off[d + 1] - doc_off[d] > NP_UNIQ_MAX || n > 65535) {   // list not sorted / counts do not fit
    *bad = 1;
    useg[d] = make_uint4(0, 0, 0, 0);
    return;
  }
  uint32_t e[8];
  int pos = 0;
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    const uint64_t hi = (uint64_t)(x + 1) * slice_w;
    while (pos < n && (uint64_t)ucodes[off + pos] < hi) ++pos;
    e[x] = (uint32_t)(x == 7 ? n : pos);
  }
  useg[d] = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
}

__global__ void doc_meta_kernel(int64_t n_docs, const int64_t* __restrict__ doc_off, const int64_t* __restrict__ uoff,
                                const int32_t* __restrict__ ulen, uint4* __restrict__ meta) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n_docs) return;
  const int64_t o = uoff[d];                                     // the document's list in d_ucodes
  const uint32_t dl = (uint32_t)(doc_off[d + 1] - doc_off[d]);   // w = offset bits 32..39 | doc length << 8
  meta[d] = make_uint4((uint32_t)d, (uint32_t)ulen[d], (uint32_t)(o & 0xFFFFFFFFll), (uint32_t)((o >> 32) & 0xFF) | (dl << 8));
}

// The distinct-code structures of a handle (np_internal.h: d_ucodes, d_ulen, d_useg, d_doc_meta and what describes them),
// built apart from it: an open installs them at once, an append (np_hip_index_append) builds those of the grown index beside
// the ones that are serving and swaps them in when nothing can fail any more.  `bytes` = their share of device_bytes.
struct Ucodes {
  DevPtr<uint8_t> d_ucodes;
  DevPtr<int32_t> d_ulen;
  DevPtr<uint4> d_useg, d_doc_meta;
  int64_t n_ucodes = 0;
  int ublock_stride = 0, ublock_hdr = 0;
  float ulen_mean = 0.f;
  bool sliced_ok = false;
  size_t bytes = 0;
};

static void install_ucodes(DeviceIndex* ix, Ucodes&& u) {
  ix->device_bytes -= ix->d_ucodes.bytes() + ix->d_ulen.bytes() + ix->d_useg.bytes() + ix->d_doc_meta.bytes();
  ix->device_bytes += u.bytes;
  ix->d_ucodes = std::move(u.d_ucodes);
  ix->d_ulen = std::move(u.d_ulen);
  ix->d_useg = std::move(u.d_useg);
  ix->d_doc_meta = std::move(u.d_doc_meta);
  ix->n_ucodes = u.n_ucodes;
  ix->ublock_stride = u.ublock_stride;
  ix->ublock_hdr = u.ublock_hdr;
  ix->ulen_mean = u.ulen_mean;
  ix->sliced_ok = u.sliced_ok;
}

// ---- what np_hip_index_append, _remove and _expand share: one exclusive section, one staged list state, one commit ----
// every context held and the handle's device current; begin() also waits for the device-side calls that returned but may
// still be running on their streams
struct UpdateSection {
  HoldContexts hold;
  DeviceGuard g;
  int device;
  explicit UpdateSection(DeviceIndex* ix) : hold(ix), g(ix->device), device(ix->device) {}
  int begin() {
    if (!g.ok) {
      set_error("hipSetDevice(%d) failed", device);
      return NP_ERR_DEVICE_UNAVAILABLE;
    }
    NP_HIP(hipDeviceSynchronize());
    return NP_OK;
  }
};

// The posting lists of the updated index and their range table, staged beside the ones that serve.  replaced == false: the
// handle's own lists stay (an append whose documents hold no token), and only the table and the coverage are new.
struct StagedLists {
  DevPtr<uint32_t> ivf;
  DevPtr<int64_t> ioff;
  std::vector<int64_t> h_ioff;
  int64_t ivf_size = 0;
  bool replaced = false;
  DevPtr<uint32_t> split;
  int R = 0, cover = 0;
};

// the range table of the staged lists over the N1 documents of u.  Lists that held every (document, code) pair still do: an
// update takes a document's entries away all at once, and the pairs it adds are all of the given documents'
static int stage_ivf_split(const DeviceIndex* ix, const Ucodes& u, int64_t N1, StagedLists* st) {
  const ListsView v{N1, u.ublock_stride, u.d_doc_meta.get(), CodeArr{u.d_ucodes.get(), ix->code_wide},
                    st->replaced ? st->ivf.get() : ix->d_ivf.get(), st->replaced ? st->ioff.get() : ix->d_ivf_offsets.get()};
  st->cover = N1 > 0 ? ix->ivf_cover : -1;
  return make_ivf_split(ix, v, ix->ivf_cover == 1, &st->split, &st->R, &st->cover);
}

static void install_lists(DeviceIndex* ix, StagedLists&& st) {
  if (st.replaced) {
    ix->device_bytes = ix->device_bytes - ix->d_ivf.bytes() - ix->d_ivf_offsets.bytes() + st.ivf.bytes() + st.ioff.bytes();
    ix->d_ivf = std::move(st.ivf);
    ix->d_ivf_offsets = std::move(st.ioff);
    ix->ivf_size = st.ivf_size;
    set_ivf_bound(ix, st.h_ioff.data());
  }
  install_ivf_split(ix, std::move(st.split), st.R);
  ix->ivf_cover = st.cover;
}

// the last step of an update, every context still held
static void finish_update(DeviceIndex* ix) {
  ix->gain_key.store(0, std::memory_order_relaxed);   // the zeroth level's run / skip policy starts over, as on a fresh handle
  ix->gain_run.store(0, std::memory_order_relaxed);
  ix->gain_skip.store(0, std::memory_order_relaxed);
  contexts_forget_index(ix);
}

// block stride of the lists (ublock_stride / ublock_hdr) from a histogram of their lengths, and ulen_mean
static int choose_ublock_stride(const DeviceIndex* ix, int64_t N, Ucodes* u) {
  // the smallest multiple of 16 bytes that holds the header and 99.9 % of the lists (at most the staging row)
  const int hdr = (int)(16 / ix->code_bytes());
  const int smax = ix->tune.s4_planes ? (ix->code_wide ? NP_UBLOCK_BIG_U32 : NP_UBLOCK_BIG_U16)
                                      : (ix->code_wide ? NP_UBLOCK_MAX_U32 : NP_UBLOCK_MAX_U16);
  int fit = smax - hdr;
  if (N > 0) {
    DevPtr<uint32_t> d_hist;
    uint32_t h_hist[NP_ULEN_BINS];
    NP_TRY(d_hist.alloc(NP_ULEN_BINS));
    NP_HIP(hipMemset(d_hist.get(), 0, sizeof h_hist));
    ulen_hist_kernel<<<(unsigned)std::min<int64_t>((N + 255) / 256, 1024), 256>>>(u->d_ulen.get(), N, d_hist.get());
    NP_HIP(hipMemcpy(h_hist, d_hist.get(), sizeof h_hist, hipMemcpyDeviceToHost));
    double usum = 0;
    for (int q2 = 0; q2 < NP_ULEN_BINS; ++q2) usum += (double)q2 * h_hist[q2];
    u->ulen_mean = (float)(usum / (double)N);
    const int64_t allow = N / 100;    // lists allowed to overflow (1 %: the filter re-reads only those)
    int64_t over = 0;
    int q = NP_ULEN_BINS - 1;
    while (q > 0 && over + h_hist[q] <= allow) over += h_hist[q--];   // q = the smallest capacity leaving <= 0.1 % outside
    fit = std::min(fit, std::max(q, 1));
  }
  // the stride is a multiple of 64 bytes, at most 256 bytes (512 with the bit-plane hot level).  What a block costs the hot
  // level is the 128-byte LINES it touches (every miss fetches a whole line: profiles/r05_fetch_probe.md), averaged over
  // even and odd documents -- blocks start on multiples of 64 bytes, so a stride that is an odd multiple of 64 straddles one
  // line more on every other document:
  //   stride (bytes)    64    128   192   256   320   384   512
  //   lines per block   1     1     2     2     3     3     4
  // approx_hotp_kernel stages exactly the block (the lane of an LDS row's 16 padding bytes issues no request; while it
  // fetched the next block's first 16 bytes the figures were 1.5, 2, 2.5, 3, 3.5, 4, 5: profiles/hot_block_lines.md).  The
  // metric corpus' 192-byte blocks sit at their two-line floor; a one-line block there needs coded lists.
  const int per64 = (int)(64 / ix->code_bytes());
  u->ublock_stride = std::max(per64, std::min(smax, (hdr + fit + per64 - 1) / per64 * per64));
  u->ublock_hdr = hdr;
  return NP_OK;
}

// inclusive scan of the overflow lists' sizes (lists longer than `fit`) into d_ovf [n_docs], and their total
static int scan_overflow(const int32_t* d_ulen, int64_t N, int fit, DevPtr<int64_t>* d_ovf, int64_t* ovf_total) {
  *ovf_total = 0;
  if (N == 0) return NP_OK;
  DevPtr<int64_t> d_pad;   // scan input; it and the scan's temp storage go before the lists are allocated
  DevPtr<uint8_t> d_temp;
  NP_TRY(d_pad.alloc((size_t)N));
  NP_TRY(d_ovf->alloc((size_t)N));
  ulen_overflow_kernel<<<(unsigned)((N + 255) / 256), 256>>>(d_ulen, N, fit, d_pad.get());
  size_t tb = 0;
  hipError_t e = hipcub::DeviceScan::InclusiveSum(nullptr, tb, d_pad.get(), d_ovf->get(), (int)N);
  if (e == hipSuccess) NP_TRY(d_temp.alloc(std::max<size_t>(tb, 16)));
  if (e == hipSuccess) e = hipcub::DeviceScan::InclusiveSum(d_temp.get(), tb, d_pad.get(), d_ovf->get(), (int)N);
  if (e == hipSuccess) e = hipMemcpy(ovf_total, d_ovf->get() + (N - 1), 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    set_error("distinct-code list scan failed: %s", hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? NP_ERR_OUT_OF_MEMORY : NP_ERR_DEVICE_UNAVAILABLE;
  }
  return NP_OK;
}

// the limits of a shard that the open path and an append share
static int check_shard_docs(int64_t n_docs) {
  if (n_docs >= ((int64_t)1 << 31)) {
    set_error("Index load failed: a shard holds < 2^31 documents (got %lld); use more shards", (long long)n_docs);
    return NP_ERR_INDEX_LOAD;
  }
  return NP_OK;
}
static int check_ucode_totals(int64_t total, int64_t ovf_total) {
  if (total >= ((int64_t)1 << 40)) {   // candidate records carry a 40-bit list offset
    set_error("Index load failed: %lld distinct-code list entries exceed the 40-bit list offset; use more shards",
              (long long)total);
    return NP_ERR_INDEX_LOAD;
  }
  if (ovf_total / NP_ULIST_ALIGN >= ((int64_t)1 << 32)) {   // a block header carries the overflow index in 32 bits
    set_error("Index load failed: %lld overflow list entries exceed the 32-bit overflow index of the list blocks; use more shards",
              (long long)ovf_total);
    return NP_ERR_INDEX_LOAD;
  }
  return NP_OK;
}

// the doc offsets and codes the distinct-code lists are built from: the handle's own (tokens_of), or -- np_hip_index_remove --
// the compacted ones while the old arrays still serve
struct TokensView {
  const int64_t* doc_off;
  CodeArr codes;
};
static TokensView tokens_of(const DeviceIndex* ix) { return TokensView{ix->d_doc_offsets.get(), ix->codes()}; }

// The distinct-code structures of the first N documents of tv (the handle's n_docs at open; the grown count in an append, whose
// doc offsets and codes are in place by then; the shrunk count and the compacted arrays in a remove) into *u.  d_uoff (list
// offsets, [N + 1]) goes back to the caller: the IVF build of the synthetic path and the posting-list merge of an append read
// the lists through it
static int build_unique_codes(const DeviceIndex* ix, const TokensView& tv, int64_t N, Ucodes* u, DevPtr<int64_t>* d_uoff) {
  NP_TRY(u->d_ulen.alloc((size_t)N, &u->bytes));
  NP_TRY(u->d_useg.alloc((size_t)N, &u->bytes));
  NP_TRY(u->d_doc_meta.alloc((size_t)N, &u->bytes));
  NP_TRY(d_uoff->alloc((size_t)N + 1));
  NP_HIP(hipMemset(d_uoff->get(), 0, 8));
  // pass 1: list lengths
  for (int64_t d0 = 0; d0 < N; d0 += (int64_t)1 << 30) {
    const int64_t n = std::min<int64_t>((int64_t)1 << 30, N - d0);
    unique_codes_kernel<<<(unsigned)n, 256>>>(tv.doc_off + d0, tv.codes, nullptr, nullptr, u->d_ulen.get() + d0);
  }
  NP_HIP(hipGetLastError());
  NP_TRY(choose_ublock_stride(ix, N, u));
  const int S = u->ublock_stride, hdr = u->ublock_hdr, fit = S - hdr;
  const int64_t base_b = N * (int64_t)S;   // first entry of the overflow region
  DevPtr<int64_t> d_ovf;                    // inclusive scan of the overflow sizes
  int64_t ovf_total = 0;
  NP_TRY(scan_overflow(u->d_ulen.get(), N, fit, &d_ovf, &ovf_total));
  const int64_t total = base_b + ovf_total;
  NP_TRY(check_ucode_totals(total, ovf_total));
  u->n_ucodes = total;
  // pass 2: headers, then the lists (+8 entries: list readers fetch up to 8 bytes past a list's last code)
  const size_t bytes = ((size_t)total + 8) * ix->code_bytes();
  NP_TRY(u->d_ucodes.alloc(bytes, &u->bytes));
  NP_HIP(hipMemset(u->d_ucodes.get(), 0, bytes));
  if (N > 0)
    ublock_layout_kernel<<<(unsigned)((N + 255) / 256), 256>>>(N, tv.doc_off, u->d_ulen.get(), d_ovf.get(), S, hdr,
                                                               fit, base_b, u->d_ucodes.get(), ix->code_wide, d_uoff->get());
  for (int64_t d0 = 0; d0 < N; d0 += (int64_t)1 << 30) {
    const int64_t n = std::min<int64_t>((int64_t)1 << 30, N - d0);
    unique_codes_kernel<<<(unsigned)n, 256>>>(tv.doc_off + d0, tv.codes, u->d_ucodes.get(), d_uoff->get() + d0,
                                              u->d_ulen.get() + d0);
  }
  if (N > 0)
    doc_meta_kernel<<<(unsigned)((N + 255) / 256), 256>>>(N, tv.doc_off, d_uoff->get(), u->d_ulen.get(),
                                                          u->d_doc_meta.get());
  NP_HIP(hipGetLastError());
  u->sliced_ok = false;
  if (N > 0) {
    DevPtr<int> d_bad;
    NP_TRY(d_bad.alloc(1));
    NP_HIP(hipMemset(d_bad.get(), 0, sizeof(int)));
    const uint32_t slice_w = (uint32_t)((ix->K + 7) / 8);
    useg_kernel<<<(unsigned)((N + 255) / 256), 256>>>(N, tv.doc_off, d_uoff->get(),
                                                      CodeArr{u->d_ucodes.get(), ix->code_wide}, u->d_ulen.get(), slice_w,
                                                      u->d_useg.get(), d_bad.get());
    int bad = 1;
    NP_HIP(hipMemcpy(&bad, d_bad.get(), sizeof(int), hipMemcpyDeviceToHost));
    u->sliced_ok = (bad == 0);
  }
  NP_HIP(hipDeviceSynchronize());
  return NP_OK;
}

// ---- from host arrays / files ----------------------------------------------------------------------
// ---- file geometry -> storage geometry (np_internal.h storage_dim / storage_nbits) --------------------------------
// one thread per storage byte.  widen: a 1-bit file byte (8 dims, first dim in bit 7) becomes two 2-bit storage bytes whose
// segment e holds bitrev2(bucket) = bucket << 1 (the bit layout of codec.rs:356-411 at nbits = 2).
__global__ void __launch_bounds__(256) repack_rows_kernel(const uint8_t* __restrict__ src, int64_t n, int lpd, int pd,
                                                          int widen, uint8_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * pd) return;
  const int64_t t = i / pd;
  const int jb = (int)(i - t * pd);
  uint32_t out = 0;
  if (widen) {
    const int sb = jb >> 1;
    if (sb < lpd) {
      const uint32_t nib = ((uint32_t)src[t * lpd + sb] >> ((jb & 1) ? 0 : 4)) & 15u;
      out = ((nib & 8u) << 4) | ((nib & 4u) << 3) | ((nib & 2u) << 2) | ((nib & 1u) << 1);
    }
  } else if (jb < lpd) {
    out = src[t * lpd + jb];
  }
  dst[i] = (uint8_t)out;
}

// the inverse, for np_hip_index_export
__global__ void __launch_bounds__(256) unpack_rows_kernel(const uint8_t* __restrict__ src, int64_t n, int lpd, int pd,
                                                          int widen, uint8_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * lpd) return;
  const int64_t t = i / lpd;
  const int jb = (int)(i - t * lpd);
  uint32_t out;
  if (widen) {
    const uint32_t hi = src[t * pd + 2 * jb], lo = src[t * pd + 2 * jb + 1];
    const uint32_t nh = ((hi >> 4) & 8u) | ((hi >> 3) & 4u) | ((hi >> 2) & 2u) | ((hi >> 1) & 1u);
    const uint32_t nl = ((lo >> 4) & 8u) | ((lo >> 3) & 4u) | ((lo >> 2) & 2u) | ((lo >> 1) & 1u);
    out = (nh << 4) | nl;
  } else {
    out = src[t * pd + jb];
  }
  dst[i] = (uint8_t)out;
}

// NP_OPEN_TRACE=1: seconds of each phase of an open to stderr (parse, token upload, posting lists, derived structures)
struct OpenTrace {
  const char* tag = "np open";
  bool on = getenv("NP_OPEN_TRACE") != nullptr;
  double t0 = now();
  OpenTrace() = default;
  OpenTrace(const char* env, const char* tag_) : tag(tag_), on(getenv(env) != nullptr) {}   // NP_APPEND_TRACE=1: an append's stages
  static double now() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
  }
  void mark(const char* what) {
    if (!on) return;
    (void)hipDeviceSynchronize();
    const double t = now();
    fprintf(stderr, "[%s] %-28s %8.6f s\n", tag, what, t - t0);
    t0 = t;
  }
};

// ---- host -> HBM at the link's rate ----------------------------------------------------------------------------------
// MmapIndex::load maps the chunk files and touches them lazily (index.rs:1096-1124); here the whole index has to cross
// PCIe once.  A plain hipMemcpy from the mapping is a single-threaded copy out of the page cache into the runtime's own
// staging buffer (3-6 GB/s: a 216 GB index would open in a minute).  Uploader keeps NP_UP_SLOTS pinned pieces in flight:
// NP_UP_THREADS host threads copy a piece out of the mapping in parallel (page faults and all), the DMA engine moves the
// previous piece meanwhile, and whatever the data needs (codes i64 -> u16 / u32 with the range check, residual rows to
// storage geometry) is done by a kernel on the staged bytes in HBM -- no scalar loop on the host touches a token.
#define NP_UP_SLOTS 3
#define NP_UP_PIECE ((size_t)128 << 20)
#define NP_UP_THREADS 12
struct Uploader {
  hipStream_t st = nullptr;
  char* pin[NP_UP_SLOTS] = {};
  hipEvent_t done[NP_UP_SLOTS] = {};
  int next = 0;
  size_t piece = NP_UP_PIECE;
  // piece_bytes: the largest piece the caller will fill (an append of a few documents pins kilobytes, not 3 x 128 MiB)
  int init(size_t piece_bytes = NP_UP_PIECE) {
    piece = std::min<size_t>(NP_UP_PIECE, (std::max<size_t>(piece_bytes, 1) + 4095) & ~(size_t)4095);
    NP_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (int i = 0; i < NP_UP_SLOTS; ++i) {
      NP_HIP(hipHostMalloc((void**)&pin[i], piece, hipHostMallocDefault));
      NP_HIP(hipEventCreateWithFlags(&done[i], hipEventDisableTiming));
    }
    return NP_OK;
  }
  ~Uploader() {
    if (st) (void)hipStreamSynchronize(st);
    for (int i = 0; i < NP_UP_SLOTS; ++i) {
      if (pin[i]) (void)hipHostFree(pin[i]);
      if (done[i]) (void)hipEventDestroy(done[i]);
    }
    if (st) (void)hipStreamDestroy(st);
  }
  // parallel copy of [src, src + bytes) into a pinned slot (bytes <= piece); returns the slot
  int fill(const void* src, size_t bytes, int* slot) {
    const int s = next;
    next = (next + 1) % NP_UP_SLOTS;
    NP_HIP(hipEventSynchronize(done[s]));   // the slot's previous piece has left (a fresh event is complete)
    const size_t per = ((bytes + NP_UP_THREADS - 1) / NP_UP_THREADS + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    for (int t = 1; t < NP_UP_THREADS; ++t) {
      const size_t a = (size_t)t * per;
      if (a >= bytes) break;
      th.emplace_back([=] { memcpy(pin[s] + a, (const char*)src + a, std::min(per, bytes - a)); });
    }
    memcpy(pin[s], src, std::min(per, bytes));
    for (auto& t : th) t.join();
    *slot = s;
    return NP_OK;
  }
  // the staged piece -> dst (device) ; `after` runs on the stream once the bytes are there
  template <class F>
  int send(int slot, size_t bytes, void* dst, F&& after) {
    NP_HIP(hipMemcpyAsync(dst, pin[slot], bytes, hipMemcpyHostToDevice, st));
    NP_TRY(after(st));
    NP_HIP(hipEventRecord(done[slot], st));
    return NP_OK;
  }
  int finish() {
    NP_HIP(hipStreamSynchronize(st));
    return NP_OK;
  }
};

// codes as stored (i64, N.codes.npy) -> u16 / u32 with the loader's range check: bad[0] = flag (0 = every code in range),
// bad[1] = one offending value (the thread that raises the flag stores it: any i64, -1 included, is reportable)
__global__ void __launch_bounds__(256) narrow_codes_kernel(const int64_t* __restrict__ src, int64_t n, int64_t K, void* __restrict__ dst,
                                                           int wide, long long* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t v = src[i];
  if (v < 0 || v >= K) {
    if (atomicExch((unsigned long long*)bad, 1ull) == 0ull) bad[1] = v;
    if (wide) static_cast<uint32_t*>(dst)[i] = 0u;   // never leave an unwritten (garbage) code behind
    else static_cast<uint16_t*>(dst)[i] = 0;
    return;
  }
  if (wide) static_cast<uint32_t*>(dst)[i] = (uint32_t)v;
  else static_cast<uint16_t*>(dst)[i] = (uint16_t)v;
}

// ---- the steps every open shares -------------------------------------------------------------------------------------
static int build_ivf_from_ucodes(DeviceIndex* ix, const int64_t* d_uoff);   // the synthetic corpus' posting lists (below)

// head: once the options and the device are checked (and the device made current by the caller's guard for the whole
// open), a fresh handle with the shard's document range of n_total documents and the tuning environment
static int start_index(const DeviceGuard& g, const np_open_opts& o, int64_t n_total, IndexHandle* out) {
  if (!g.ok) {
    set_error("hipSetDevice(%d) failed", o.device);
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  out->reset(new np_index());
  DeviceIndex* ix = out->get();
  ix->device = o.device;
  ix->opts = o;
  read_tuning_env(&ix->tune);
  ix->N_total = n_total;
  int64_t sb, se;
  shard_range(n_total, o.shard_rank, o.shard_count, &sb, &se);
  ix->doc_begin = sb;
  ix->n_docs = se - sb;
  return NP_OK;
}

// geometry and codec tables.  Files and caller arrays are stored in storage geometry (np_internal.h storage_dim /
// storage_nbits); as_stored: the rows are storage rows already (the synthetic generator: dim == ldim, nbits == lnbits)
static int set_geometry(DeviceIndex* ix, int64_t K, int dim, int nbits, bool as_stored, const float* centroids,
                        const float* bucket_weights) {
  ix->K = K;
  ix->KP = (K + 63) / 64 * 64;
  ix->code_wide = K > 65536 ? 1 : 0;   // u16 codes whenever every centroid id fits (2 B per token instead of 4)
  ix->ldim = dim;
  ix->lnbits = nbits;
  ix->lpd = dim * nbits / 8;
  ix->dim = as_stored ? dim : storage_dim(dim);
  ix->nbits = as_stored ? nbits : storage_nbits(dim, nbits);
  ix->pd = ix->dim * ix->nbits / 8;
  return upload_codec(ix, centroids, bucket_weights);
}

// the codes and residuals of the shard's ix->T tokens (the caller fills them)
static int alloc_tokens(DeviceIndex* ix) {
  NP_TRY(ix->d_codes.alloc((size_t)std::max<int64_t>(ix->T, 1) * ix->code_bytes(), &ix->device_bytes));
  return ix->d_residuals.alloc((size_t)ix->T * ix->pd, &ix->device_bytes);
}

// tail: the derived structures (np_internal.h) and the default workspace.  lists_from_codes: the index has no posting
// lists of its own (the synthetic corpus); they are built here from the distinct codes (index.rs:479-499)
static int build_derived(DeviceIndex* ix, bool lists_from_codes, OpenTrace& trace) {
  NP_TRY(sort_tokens(ix));
  {
    DevPtr<int64_t> d_uoff;
    Ucodes u;
    NP_TRY(build_unique_codes(ix, tokens_of(ix), ix->n_docs, &u, &d_uoff));
    install_ucodes(ix, std::move(u));
    trace.mark("distinct-code blocks");
    if (lists_from_codes) {
      NP_TRY(build_ivf_from_ucodes(ix, d_uoff.get()));
      trace.mark("posting lists from the codes");
    }
  }
  NP_TRY(build_ivf_split(ix, lists_from_codes));
  trace.mark("list coverage + range table");
  NP_TRY(build_inv_norm(ix));
  trace.mark("inverse norms");
  ix->cap_docs = ix->n_docs;
  ix->cap_tokens = ix->T;
  default_workspace(ix);
  return NP_OK;
}

// ---- from host arrays / files ----------------------------------------------------------------------------------------
// the shard's doc offsets (prefix sum of its lengths) -> HBM, T and max_doc_len; *tb = its first token in the host arrays
static int doc_offsets_from_lengths(const HostIndex& h, DeviceIndex* ix, int64_t* tb) {
  const int64_t hb = h.doc_begin, sb = ix->doc_begin;
  *tb = 0;
  for (int64_t d = hb; d < sb; ++d) *tb += h.doc_lengths[d - hb];
  std::vector<int64_t> off((size_t)ix->n_docs + 1);
  off[0] = 0;
  int64_t maxlen = 0;
  for (int64_t d = 0; d < ix->n_docs; ++d) {
    int64_t l = h.doc_lengths[sb - hb + d];
    if (l < 0) {
      set_error("Index load failed: negative doc length");
      return NP_ERR_INDEX_LOAD;
    }
    maxlen = std::max(maxlen, l);
    off[d + 1] = off[d] + l;
  }
  ix->T = off[ix->n_docs];
  ix->max_doc_len = maxlen;
  NP_TRY(ix->d_doc_offsets.alloc(off.size(), &ix->device_bytes));
  NP_HIP(hipMemcpy(ix->d_doc_offsets.get(), off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  return NP_OK;
}

// tokens [tb, tb + n_tok) of the host chunks -> d_codes (i64 -> u16 / u32, range-checked) and d_residuals from token dst0 on,
// pipelined through the Uploader.  An open sends the shard's T tokens to the arrays' start, an append the new ones behind them
static int upload_tokens(const HostIndex& h, DeviceIndex* ix, int64_t tb, int64_t n_tok, int64_t dst0) {
  const int64_t te = tb + n_tok;
  // device-side staging of raw pieces that need a kernel (i64 codes; residual rows in file geometry); declared before the
  // uploader, whose destructor waits for its stream, so that they outlive the work queued on them
  DevPtr<char> d_stage[NP_UP_SLOTS];
  DevPtr<long long> d_bad;
  Uploader up;
  NP_TRY(up.init((size_t)n_tok * (size_t)std::max(8, ix->lpd)));
  for (DevPtr<char>& st : d_stage) NP_TRY(st.alloc(up.piece));
  NP_TRY(d_bad.alloc(2));
  NP_HIP(hipMemset(d_bad.get(), 0, 16));
  const bool repack = ix->pd != ix->lpd;
  const int widen = ix->lnbits != ix->nbits;
  int64_t pos = 0;  // token position of the current chunk's first token in the host arrays
  for (const HostChunk& c : h.chunks) {
    const int64_t a = std::max(pos, tb), b = std::min(pos + c.n_tokens, te);
    // codes: raw i64 pieces, narrowed and range-checked on the device
    const int64_t CP = (int64_t)(up.piece / 8);
    for (int64_t t0 = a; t0 < b; t0 += CP) {
      const int64_t n = std::min(CP, b - t0);
      int slot;
      NP_TRY(up.fill((const char*)c.codes + (t0 - pos) * 8, (size_t)n * 8, &slot));
      NP_TRY(up.send(slot, (size_t)n * 8, d_stage[slot].get(), [&](hipStream_t st) -> int {
        narrow_codes_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(
            (const int64_t*)d_stage[slot].get(), n, ix->K, ix->d_codes.get() + (dst0 + t0 - tb) * (int64_t)ix->code_bytes(), ix->code_wide,
            d_bad.get());
        NP_HIP(hipGetLastError());
        return (int)NP_OK;
      }));
    }
    // residuals: straight into place, or through the staging area + repack (file rows -> storage rows: zero-padded,
    // 1-bit buckets widened to 2-bit segments)
    const int64_t RP = std::max<int64_t>(1, (int64_t)(up.piece / std::max(ix->lpd, 1)));
    for (int64_t t0 = a; t0 < b; t0 += RP) {
      const int64_t n = std::min(RP, b - t0);
      uint8_t* dst = ix->d_residuals.get() + (dst0 + t0 - tb) * ix->pd;
      int slot;
      NP_TRY(up.fill(c.residuals + (t0 - pos) * ix->lpd, (size_t)n * ix->lpd, &slot));
      if (!repack) {
        NP_TRY(up.send(slot, (size_t)n * ix->lpd, dst, [](hipStream_t) -> int { return NP_OK; }));
      } else {
        NP_TRY(up.send(slot, (size_t)n * ix->lpd, d_stage[slot].get(), [&](hipStream_t st) -> int {
          repack_rows_kernel<<<(unsigned)((n * ix->pd + 255) / 256), 256, 0, st>>>((const uint8_t*)d_stage[slot].get(), n, ix->lpd,
                                                                                  ix->pd, widen, dst);
          NP_HIP(hipGetLastError());
          return (int)NP_OK;
        }));
      }
    }
    pos += c.n_tokens;
  }
  NP_TRY(up.finish());
  if (pos < te) {
    set_error("Index load failed: chunks hold %lld tokens, doclens need %lld", (long long)pos, (long long)te);
    return NP_ERR_INDEX_LOAD;
  }
  long long bad[2] = {0, 0};
  NP_HIP(hipMemcpy(bad, d_bad.get(), 16, hipMemcpyDeviceToHost));
  if (bad[0] != 0) {
    set_error("Index load failed: code %lld out of range [0,%lld)", bad[1], (long long)ix->K);
    return NP_ERR_INDEX_LOAD;
  }
  return NP_OK;
}

// IVF restricted to the shard, re-based to shard-local u32 ids: two passes over the posting lists (count, then fill), the
// centroid range split over host threads (680 M i64 entries at 10 M x 300-token documents)
static int build_posting_lists(const HostIndex& h, DeviceIndex* ix) {
  const int64_t sb = ix->doc_begin, se = ix->doc_begin + ix->n_docs;
  std::vector<int64_t> ioff((size_t)ix->K + 1, 0), lstart((size_t)ix->K + 1, 0);
  for (int64_t c = 0; c < ix->K; ++c) {
    const int64_t l = h.ivf_lengths[c];
    if (l < 0 || lstart[c] + l > h.ivf_size) {
      set_error("Index load failed: ivf_lengths inconsistent with ivf.npy at centroid %lld", (long long)c);
      return NP_ERR_INDEX_LOAD;
    }
    lstart[c + 1] = lstart[c] + l;
  }
  const int NT = (int)std::max<int64_t>(1, std::min<int64_t>(NP_UP_THREADS, ix->K / 1024));
  const bool whole = sb == 0 && se == h.num_documents_total;
  std::vector<int64_t> bad_id((size_t)NT, -1);
  auto run = [&](auto&& body) {
    std::vector<std::thread> th;
    for (int t = 1; t < NT; ++t) th.emplace_back([&, t] { body(t); });
    body(0);
    for (auto& x : th) x.join();
  };
  auto range = [&](int t, int64_t* c0, int64_t* c1) {   // centroid ranges of about equal posting volume
    const int64_t tot = lstart[ix->K];
    *c0 = std::lower_bound(lstart.begin(), lstart.end(), tot * t / NT) - lstart.begin();
    *c1 = t + 1 == NT ? ix->K : std::lower_bound(lstart.begin(), lstart.end(), tot * (t + 1) / NT) - lstart.begin();
    *c0 = std::min<int64_t>(*c0, ix->K);
    *c1 = std::min<int64_t>(std::max(*c1, *c0), ix->K);
  };
  run([&](int t) {   // pass 1: entries of every list that fall into the shard, ids range-checked
    int64_t c0, c1;
    range(t, &c0, &c1);
    for (int64_t c = c0; c < c1; ++c) {
      int64_t cnt = 0;
      const char* src = (const char*)h.ivf + lstart[c] * 8;
      for (int64_t i = 0, l = lstart[c + 1] - lstart[c]; i < l; ++i) {
        int64_t id;
        memcpy(&id, src + i * 8, 8);
        if (id < 0 || id >= h.num_documents_total) {
          bad_id[t] = id;
          return;
        }
        cnt += whole || (id >= sb && id < se);
      }
      ioff[c + 1] = cnt;
    }
  });
  for (int t = 0; t < NT; ++t)
    if (bad_id[t] != -1) {
      set_error("Index load failed: ivf doc id %lld out of range", (long long)bad_id[t]);
      return NP_ERR_INDEX_LOAD;
    }
  for (int64_t c = 0; c < ix->K; ++c) ioff[c + 1] += ioff[c];
  std::vector<uint32_t> ivf((size_t)ioff[ix->K]);
  std::vector<int> unsorted((size_t)NT, 0);   // the crate writes ascending unique ids (index.rs:479-504); S3 relies on it only if true
  run([&](int t) {   // pass 2
    int64_t c0, c1;
    range(t, &c0, &c1);
    for (int64_t c = c0; c < c1; ++c) {
      uint32_t* out = ivf.data() + ioff[c];
      const char* src = (const char*)h.ivf + lstart[c] * 8;
      int64_t prev = -1;
      for (int64_t i = 0, l = lstart[c + 1] - lstart[c]; i < l; ++i) {
        int64_t id;
        memcpy(&id, src + i * 8, 8);
        if (id <= prev) unsorted[(size_t)t] = 1;
        prev = id;
        if (whole || (id >= sb && id < se)) *out++ = (uint32_t)(id - sb);
      }
    }
  });
  ix->ivf_sorted = true;
  for (int t = 0; t < NT; ++t)
    if (unsorted[(size_t)t]) ix->ivf_sorted = false;
  ix->ivf_size = (int64_t)ivf.size();
  NP_TRY(ix->d_ivf.alloc(ivf.size(), &ix->device_bytes));
  if (!ivf.empty()) NP_HIP(hipMemcpy(ix->d_ivf.get(), ivf.data(), ivf.size() * 4, hipMemcpyHostToDevice));
  NP_TRY(ix->d_ivf_offsets.alloc(ioff.size(), &ix->device_bytes));
  NP_HIP(hipMemcpy(ix->d_ivf_offsets.get(), ioff.data(), ioff.size() * 8, hipMemcpyHostToDevice));
  set_ivf_bound(ix, ioff.data());
  return NP_OK;
}

int build_device_index(const HostIndex& h, const np_open_opts* opts_in, DeviceIndex** out) {
  *out = nullptr;
  np_open_opts o;
  NP_TRY(normalise_opts(opts_in, &o));
  NP_TRY(check_device(o.device));
  NP_TRY(check_geometry(h.K, h.dim, h.nbits, h.num_documents_total));
  int64_t sb, se;
  shard_range(h.num_documents_total, o.shard_rank, o.shard_count, &sb, &se);
  const int64_t hb = h.doc_begin, he = h.doc_begin + (int64_t)h.doc_lengths.size();
  if (sb < hb || se > he) {
    set_error("Index load failed: host arrays cover docs [%lld,%lld) but shard %d/%d needs [%lld,%lld)", (long long)hb,
              (long long)he, o.shard_rank, o.shard_count, (long long)sb, (long long)se);
    return NP_ERR_INDEX_LOAD;
  }
  DeviceGuard g(o.device);
  IndexHandle ix;
  NP_TRY(start_index(g, o, h.num_documents_total, &ix));
  ix->n_emb_total = h.num_embeddings_total;
  ix->avg_doclen = h.avg_doclen;
  NP_TRY(check_shard_docs(ix->n_docs));
  OpenTrace trace;
  NP_TRY(set_geometry(ix.get(), h.K, h.dim, h.nbits, false, h.centroids, h.bucket_weights));
  trace.mark("codec");
  int64_t tb = 0;
  NP_TRY(doc_offsets_from_lengths(h, ix.get(), &tb));
  NP_TRY(alloc_tokens(ix.get()));
  NP_TRY(upload_tokens(h, ix.get(), tb, ix->T, 0));
  trace.mark("codes + residuals -> HBM");
  NP_TRY(build_posting_lists(h, ix.get()));
  trace.mark("posting lists");
  NP_TRY(build_derived(ix.get(), false, trace));
  *out = ix.release();
  return NP_OK;
}

// ---- synthetic corpus generated in HBM (spec: next_plaid_amd/synth.py) -----------------------------------
__host__ __device__ static inline uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
enum { S_LEN = 1, S_TOPIC = 2, S_TOK = 3, S_RES = 4 };

struct SynthP {
  uint64_t b_len, b_topic, b_tok, b_res;
  int64_t doc_begin, n_docs;
  uint32_t K;
  int32_t len_min, len_span, n_topics, rand256, pd, nw;
};

__global__ void synth_lens_kernel(SynthP p, const int32_t* __restrict__ len_table, int len_table_size, int64_t* lens) {
  int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= p.n_docs) return;
  const uint64_t r = mix64(p.b_len + (uint64_t)(p.doc_begin + d));
  lens[d] = len_table ? (int64_t)len_table[r % (uint64_t)len_table_size] : p.len_min + (int64_t)(r % (uint64_t)p.len_span);
}

// one wave per document
__global__ void __launch_bounds__(256) synth_tokens_kernel(SynthP p, const int64_t* __restrict__ doc_off,
                                                           void* __restrict__ codes, int wide, uint8_t* __restrict__ res) {
  const int lane = threadIdx.x & 63;
  int64_t d = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= p.n_docs) return;
  const uint64_t gdoc = (uint64_t)(p.doc_begin + d);
  const int64_t off = doc_off[d];
  const int len = (int)(doc_off[d + 1] - off);
  for (int t = lane; t < len; t += 64) {
    uint64_t r = mix64(p.b_tok + (gdoc * 65536ull + (uint64_t)t));
    uint32_t code;
    if ((r & 0xFF) < (uint64_t)p.rand256) {
      code = (uint32_t)(((r >> 8) & 0xFFFFFFFFull) % p.K);
    } else {
      uint64_t s = (r >> 40) % (uint64_t)p.n_topics;
      uint64_t rt = mix64(p.b_topic + (gdoc * (uint64_t)p.n_topics + s));
      code = (uint32_t)(((rt & 0xFFFFFFFFull) % p.K) >> ((rt >> 32) & 3));
    }
    if (wide) static_cast<uint32_t*>(codes)[off + t] = code;
    else static_cast<uint16_t*>(codes)[off + t] = (uint16_t)code;
  }
  const int nwords = len * p.nw;
  for (int w = lane; w < nwords; w += 64) {
    int t = w / p.nw, j = w - t * p.nw;
    uint64_t v = mix64(p.b_res + ((gdoc * 65536ull + (uint64_t)t) * 16ull + (uint64_t)j));
    uint8_t* dst = res + (off + t) * (int64_t)p.pd + j * 8;
    int nb = min(8, p.pd - j * 8);
    if (nb == 8 && (p.pd & 7) == 0) {
      *(uint64_t*)dst = v;  // little endian
    } else {
      for (int b = 0; b < nb; ++b) dst[b] = (uint8_t)(v >> (8 * b));
    }
  }
}

// ---- IVF from the per-document distinct-code lists (index.rs:479-499: per centroid the ascending unique doc ids) ----
// Pairs (code << 32 | shard-local doc) are emitted from ucodes/ulen for a contiguous document range, radix-sorted,
// and scattered into the posting lists.  Ranges hold at most NP_IVF_SEG pairs, so every hipcub call sees a count
// below 2^31 whatever the shard size (a 10M-document x 300-token shard has 3.0e9 tokens, ~0.7e9 pairs).
#define NP_IVF_SEG ((int64_t)1 << 29)

// one wave per document: pair position = (exclusive prefix of ulen) - seg_base
__global__ void __launch_bounds__(256) ivf_emit_pairs_kernel(int64_t d0, int64_t d1, const int64_t* __restrict__ uoff,
                                                             CodeArr ucodes,
                                                             const int32_t* __restrict__ ulen,
                                                             const int64_t* __restrict__ upfx /* inclusive, of documents pfx_d0 .. */,
                                                             int64_t pfx_d0, int64_t seg_base, uint64_t* __restrict__ keys) {
  const int64_t d = d0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (d >= d1) return;
  const int n = ulen[d];
  const int64_t pos = upfx[d - pfx_d0] - n - seg_base;
  const int64_t off = uoff[d];
  for (int i = lane; i < n; i += 64) keys[pos + i] = ((uint64_t)ucodes[off + i] << 32) | (uint64_t)d;
}

// start[c] = first sorted pair whose code is >= c  (c = 0..K; start[K] = n)
__global__ void ivf_code_starts_kernel(const uint64_t* __restrict__ sorted, int64_t n, int64_t K,
                                       int64_t* __restrict__ start) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > K) return;
  const uint64_t key = (uint64_t)c << 32;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  start[c] = lo;
}

// ivf[dst_base[code] + (i - start[code])] = doc
__global__ void ivf_scatter_kernel(const uint64_t* __restrict__ sorted, int64_t n, const int64_t* __restrict__ start,
                                   const int64_t* __restrict__ dst_base, uint32_t* __restrict__ ivf) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = sorted[i];
  const uint32_t c = (uint32_t)(k >> 32);
  ivf[dst_base[c] + (i - start[c])] = (uint32_t)(k & 0xFFFFFFFFull);
}

__global__ void ulen_to_i64_kernel(const int32_t* __restrict__ ulen, int64_t n, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = ulen[i];
}

// a pair of device events around a kernel, when a trace asks for the kernel's own time
struct KernelClock {
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool on = false;
  explicit KernelClock(bool want) { on = want && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess; }
  ~KernelClock() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  void start() {
    if (on) (void)hipEventRecord(ev[0], nullptr);
  }
  double stop() {   // seconds
    float ms = 0.f;
    if (!on) return 0.0;
    (void)hipEventRecord(ev[1], nullptr);
    if (hipEventSynchronize(ev[1]) != hipSuccess || hipEventElapsedTime(&ms, ev[0], ev[1]) != hipSuccess) return 0.0;
    return ms * 1e-3;
  }
};

template <class T>
static int device_scan_inclusive(const T* in, T* out, int64_t n) {
  DevPtr<uint8_t> d_temp;
  size_t tb = 0;
  NP_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, tb, in, out, (int)n));
  NP_TRY(d_temp.alloc(std::max<size_t>(tb, 16)));
  NP_HIP(hipcub::DeviceScan::InclusiveSum(d_temp.get(), tb, in, out, (int)n));
  return NP_OK;
}
template <class T>
static int device_scan_exclusive(const T* in, T* out, int64_t n) {
  DevPtr<uint8_t> d_temp;
  size_t tb = 0;
  NP_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)n));
  NP_TRY(d_temp.alloc(std::max<size_t>(tb, 16)));
  NP_HIP(hipcub::DeviceScan::ExclusiveSum(d_temp.get(), tb, in, out, (int)n));
  return NP_OK;
}
// n (code << 32 | document) keys by their low 32 + code_bits bits
static int device_sort_pairs(const uint64_t* in, uint64_t* out, int64_t n, int code_bits) {
  DevPtr<uint8_t> d_temp;
  size_t tb = 0;
  NP_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, in, out, (int)n, 0, 32 + code_bits));
  NP_TRY(d_temp.alloc(std::max<size_t>(tb, 16)));
  NP_HIP(hipcub::DeviceRadixSort::SortKeys(d_temp.get(), tb, in, out, (int)n, 0, 32 + code_bits));
  return NP_OK;
}
// sorted keys, each once: *n_out of them in out
static int device_unique(const uint64_t* in, uint64_t* out, int64_t n, int64_t* n_out) {
  DevPtr<uint8_t> d_temp;
  DevPtr<int64_t> d_n;
  size_t tb = 0;
  NP_TRY(d_n.alloc(1));
  NP_HIP(hipcub::DeviceSelect::Unique(nullptr, tb, in, out, d_n.get(), (int)n));
  NP_TRY(d_temp.alloc(std::max<size_t>(tb, 16)));
  NP_HIP(hipcub::DeviceSelect::Unique(d_temp.get(), tb, in, out, d_n.get(), (int)n));
  NP_HIP(hipMemcpy(n_out, d_n.get(), 8, hipMemcpyDeviceToHost));
  return NP_OK;
}

static int build_ivf_from_ucodes(DeviceIndex* ix, const int64_t* d_uoff) {
  const int64_t K = ix->K, N = ix->n_docs;
  std::vector<int64_t> ioff((size_t)K + 1, 0);
  ix->ivf_size = 0;
  DevPtr<int64_t> d_upfx, d_start, d_base;
  DevPtr<uint64_t> d_k1, d_k2;
  DevPtr<uint8_t> d_temp;
  std::vector<int64_t> upfx((size_t)N);
  if (N > 0) {
    NP_TRY(d_upfx.alloc((size_t)N));
    NP_TRY(d_start.alloc((size_t)N));   // scan input (released below; d_start is re-allocated per code later)
    ulen_to_i64_kernel<<<(unsigned)((N + 255) / 256), 256>>>(ix->d_ulen.get(), N, d_start.get());
    NP_TRY(device_scan_inclusive(d_start.get(), d_upfx.get(), N));
    NP_HIP(hipMemcpy(upfx.data(), d_upfx.get(), (size_t)N * 8, hipMemcpyDeviceToHost));
    d_start.reset();
  }
  const int64_t total = N > 0 ? upfx[(size_t)N - 1] : 0;
  // document ranges of at most NP_IVF_SEG pairs (a single document never exceeds 65535 distinct codes... any size fits)
  std::vector<int64_t> seg_d0;
  for (int64_t d = 0; d < N;) {
    seg_d0.push_back(d);
    const int64_t base = d > 0 ? upfx[(size_t)d - 1] : 0;
    const int64_t e = std::upper_bound(upfx.begin() + d, upfx.end(), base + NP_IVF_SEG) - upfx.begin();
    d = std::max<int64_t>(e, d + 1);
  }
  seg_d0.push_back(N);
  const int nseg = (int)seg_d0.size() - 1;
  int64_t max_pairs = 0;
  for (int s = 0; s < nseg; ++s) {
    const int64_t b = seg_d0[s] > 0 ? upfx[(size_t)seg_d0[s] - 1] : 0, e = seg_d0[s + 1] > 0 ? upfx[(size_t)seg_d0[s + 1] - 1] : 0;
    max_pairs = std::max(max_pairs, e - b);
  }
  if (max_pairs >= ((int64_t)1 << 31)) {
    set_error("Index load failed: one document range holds %lld (code, doc) pairs", (long long)max_pairs);
    return NP_ERR_INDEX_LOAD;
  }
  ix->ivf_size = total;
  NP_TRY(ix->d_ivf.alloc((size_t)total, &ix->device_bytes));
  if (total > 0) {
    int kbits = 1;
    while (((int64_t)1 << kbits) < K) ++kbits;
    NP_TRY(d_k1.alloc((size_t)max_pairs));
    NP_TRY(d_k2.alloc((size_t)max_pairs));
    NP_TRY(d_start.alloc((size_t)K + 1));
    NP_TRY(d_base.alloc((size_t)K + 1));
    size_t tb = 0;
    NP_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, d_k1.get(), d_k2.get(), (int)max_pairs, 0, 32 + kbits));
    NP_TRY(d_temp.alloc(std::max<size_t>(tb, 16)));
    std::vector<std::vector<int64_t>> seg_start((size_t)nseg, std::vector<int64_t>((size_t)K + 1));
    auto sort_segment = [&](int s, int64_t* n_out) -> int {
      const int64_t d0 = seg_d0[s], d1 = seg_d0[s + 1];
      const int64_t base = d0 > 0 ? upfx[(size_t)d0 - 1] : 0, n = upfx[(size_t)d1 - 1] - base;
      *n_out = n;
      if (n == 0) return NP_OK;
      ivf_emit_pairs_kernel<<<(unsigned)((d1 - d0 + 3) / 4), 256>>>(d0, d1, d_uoff, ix->ucodes(), ix->d_ulen.get(),
                                                                   d_upfx.get(), 0, base, d_k1.get());
      size_t tbs = tb;
      NP_HIP(hipcub::DeviceRadixSort::SortKeys(d_temp.get(), tbs, d_k1.get(), d_k2.get(), (int)n, 0, 32 + kbits));
      ivf_code_starts_kernel<<<(unsigned)((K + 256) / 256), 256>>>(d_k2.get(), n, K, d_start.get());
      NP_HIP(hipGetLastError());
      return NP_OK;
    };
    // pass 1: per-range code counts (a single range keeps its sorted pairs for the scatter below)
    for (int s = 0; s < nseg; ++s) {
      int64_t n = 0;
      NP_TRY(sort_segment(s, &n));
      if (n == 0) std::fill(seg_start[(size_t)s].begin(), seg_start[(size_t)s].end(), 0);
      else NP_HIP(hipMemcpy(seg_start[(size_t)s].data(), d_start.get(), ((size_t)K + 1) * 8, hipMemcpyDeviceToHost));
    }
    for (int64_t c = 0; c < K; ++c) {
      int64_t len = 0;
      for (int s = 0; s < nseg; ++s) len += seg_start[(size_t)s][(size_t)c + 1] - seg_start[(size_t)s][(size_t)c];
      ioff[(size_t)c + 1] = ioff[(size_t)c] + len;
    }
    // pass 2: scatter each range's lists behind the earlier ranges' (ranges are ascending in doc id)
    std::vector<int64_t> base_c(ioff.begin(), ioff.end());
    for (int s = 0; s < nseg; ++s) {
      int64_t n = 0;
      if (nseg > 1) NP_TRY(sort_segment(s, &n));
      else n = total;
      if (n > 0) {
        NP_HIP(hipMemcpy(d_base.get(), base_c.data(), ((size_t)K + 1) * 8, hipMemcpyHostToDevice));
        ivf_scatter_kernel<<<(unsigned)((n + 255) / 256), 256>>>(d_k2.get(), n, d_start.get(), d_base.get(), ix->d_ivf.get());
        NP_HIP(hipGetLastError());
        NP_HIP(hipDeviceSynchronize());
      }
      for (int64_t c = 0; c < K; ++c) base_c[(size_t)c] += seg_start[(size_t)s][(size_t)c + 1] - seg_start[(size_t)s][(size_t)c];
    }
  }
  NP_TRY(ix->d_ivf_offsets.alloc(ioff.size(), &ix->device_bytes));
  NP_HIP(hipMemcpy(ix->d_ivf_offsets.get(), ioff.data(), ioff.size() * 8, hipMemcpyHostToDevice));
  set_ivf_bound(ix, ioff.data());
  NP_HIP(hipDeviceSynchronize());
  ix->ivf_sorted = true;   // (code, document) pairs radix-sorted, ranges ascending: every list ascends
  return NP_OK;
}

// ---- append to and expand a resident index: the posting-list rewrite ----------------------------------------------------
// New documents take the largest ids, so every per-token and per-document array only grows at its end and, the lists
// ascending, posting list c only gains entries at its end.  The one array that is laid out again is d_ivf: K lists, each
// keeping a front part of what it held -- old_ivf[old_begin[c] .. + kept_pfx[c + 1] - kept_pfx[c]) -- and growing at its tail.
// With the given documents' (code, id) pairs sorted, start[c] = the pairs with a smaller code is at once the exclusive scan of
// the per-list gains, as kept_pfx is that of the kept lengths, so
//   new_off[c] = kept_pfx[c] + start[c];   kept entry i of list c -> new_off[c] + i;   pair j of code c -> new_off[c] + kept[c] + j
// and every entry of the new array has one source that scans alone decide: no atomics, no workgroup waits for another.
// An append (np_hip_index_append) keeps every list whole: the old offsets are old_begin and kept_pfx at once.  An expand
// (np_hip_index_expand, below) cuts every list at the first dropped document and may add lists: ivf_keep_kernel and a scan.
__global__ void ivf_cut_offsets_kernel(const int64_t* __restrict__ kept_pfx, const int64_t* __restrict__ start, int64_t K,
                                       int64_t* __restrict__ new_off) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c <= K) new_off[c] = kept_pfx[c] + start[c];
}

// the list that holds entry o of the new array: the largest c' >= c with off[c'] <= o.  Needs off[c] <= o < off[K]; gallops from
// c, since a thread's next entry lies in the same list or a near one (empty lists are stepped over: their offsets repeat)
__device__ __forceinline__ int64_t ivf_list_of(const int64_t* __restrict__ off, int64_t K, int64_t c, int64_t o) {
  int64_t lo = c, step = 1, hi = min(K, lo + step);
  while (off[hi] <= o) {
    lo = hi;
    step <<= 1;
    hi = min(K, lo + step);
  }
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= o) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The rewrite is a streaming move (4 bytes read and 4 written per entry; the offsets stay in the caches), balanced by ENTRIES:
// a workgroup owns NP_MERGE_TILE consecutive entries of the NEW array whatever lists they belong to (list lengths are
// Zipf-skewed: one thread per list would leave the longest to a single lane).  A thread owns 4 consecutive entries -- one
// aligned 16-byte store -- and the threads of a wave consecutive quads, so inside a list segment a wave reads 1 KiB of the
// old array (or 2 KiB of pairs) and writes 1 KiB, all contiguous.  A quad that lies inside the old part of one list -- nearly
// all of them on long lists -- is one 16-byte load (4-byte aligned: the shift between old and new position is any number of entries).  A thread
// finds and loads its NP_MERGE_QUADS quads first and stores them afterwards, so that many loads are in flight per lane.
#define NP_MERGE_TILE 4096
#define NP_MERGE_QUADS (NP_MERGE_TILE / 1024)
struct __attribute__((packed, aligned(4))) MergeQuad {
  uint32_t v[4];
};
__global__ void __launch_bounds__(256) ivf_cut_merge_kernel(const uint32_t* __restrict__ old_ivf, const int64_t* __restrict__ old_begin,
                                                            const int64_t* __restrict__ kept_pfx, const uint64_t* __restrict__ pairs,
                                                            const int64_t* __restrict__ start, const int64_t* __restrict__ new_off,
                                                            int64_t K, int64_t total, uint32_t* __restrict__ out) {
  __shared__ int64_t s_c0;
  const int64_t o0 = (int64_t)blockIdx.x * NP_MERGE_TILE;   // < total: the grid covers [0, total)
  if (threadIdx.x == 0) s_c0 = ivf_list_of(new_off, K, 0, o0);
  __syncthreads();
  int64_t c = s_c0;
  MergeQuad q[NP_MERGE_QUADS];
#pragma unroll
  for (int it = 0; it < NP_MERGE_QUADS; ++it) {
    const int64_t o = o0 + it * 1024 + (int64_t)threadIdx.x * 4;
    q[it] = MergeQuad{{0u, 0u, 0u, 0u}};
    if (o < total) {
      const int n = (int)min((int64_t)4, total - o);
      c = ivf_list_of(new_off, K, c, o);
      int64_t b_new = new_off[c], e_new = new_off[c + 1], b_old = old_begin[c], n_old = kept_pfx[c + 1] - kept_pfx[c], b_pair = start[c];
      if (n == 4 && o + 4 <= b_new + n_old) {   // (b_new + n_old <= e_new)
        q[it] = *reinterpret_cast<const MergeQuad*>(old_ivf + b_old + (o - b_new));
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < n) {
            const int64_t oo = o + k;
            if (oo >= e_new) {
              c = ivf_list_of(new_off, K, c, oo);
              b_new = new_off[c], e_new = new_off[c + 1], b_old = old_begin[c], n_old = kept_pfx[c + 1] - kept_pfx[c], b_pair = start[c];
            }
            const int64_t r = oo - b_new;
            q[it].v[k] = r < n_old ? old_ivf[b_old + r] : (uint32_t)(pairs[b_pair + (r - n_old)] & 0xFFFFFFFFull);
          }
        }
      }
    }
  }
#pragma unroll
  for (int it = 0; it < NP_MERGE_QUADS; ++it) {
    const int64_t o = o0 + it * 1024 + (int64_t)threadIdx.x * 4;
    if (o + 4 <= total) {
      *reinterpret_cast<uint4*>(out + o) = make_uint4(q[it].v[0], q[it].v[1], q[it].v[2], q[it].v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (o + k < total) out[o + k] = q[it].v[k];
    }
  }
}

template <class T>
static int grow_array(DeviceIndex* ix, DevPtr<T>& a, size_t used, size_t want) {
  DevPtr<T> f;
  NP_TRY(f.alloc(want));
  if (used > 0) NP_HIP(hipMemcpy(f.get(), a.get(), used * sizeof(T), hipMemcpyDeviceToDevice));
  ix->device_bytes = ix->device_bytes - a.bytes() + f.bytes();
  a = std::move(f);   // frees the old array: one array at a time is held twice
  return NP_OK;
}

// room for need_docs documents and need_tokens tokens in the arrays that only grow at their end.  A failed allocation leaves
// every array that did not grow yet, and the capacities, as they were.
static int grow_capacity(DeviceIndex* ix, int64_t need_docs, int64_t need_tokens) {
  if (need_tokens > ix->cap_tokens) {
    const size_t T = (size_t)ix->T, W = (size_t)need_tokens;
    NP_TRY(grow_array(ix, ix->d_residuals, T * ix->pd, W * ix->pd));
    NP_TRY(grow_array(ix, ix->d_codes, T * ix->code_bytes(), std::max<size_t>(W, 1) * ix->code_bytes()));
    NP_TRY(grow_array(ix, ix->d_inv_norm, T, W));
    if (ix->tok_sorted) NP_TRY(grow_array(ix, ix->d_tok_pos, T, W));
    ix->cap_tokens = need_tokens;
  }
  if (need_docs > ix->cap_docs) {
    NP_TRY(grow_array(ix, ix->d_doc_offsets, (size_t)ix->n_docs + 1, (size_t)need_docs + 1));
    ix->cap_docs = need_docs;
  }
  return NP_OK;
}

// columns, keyword index and groups cover the documents the handle had: gone, as after a reload
static void drop_attachments(DeviceIndex* ix) {
  ix->columns.clear();
  ix->d_coltab.reset();
  ix->text = DeviceText();
  ix->d_groups.reset();
  ix->n_groups = 0;
  ix->device_bytes -= ix->column_bytes + ix->coltext_bytes + ix->text_bytes + ix->group_bytes;
  ix->column_bytes = ix->coltext_bytes = ix->text_bytes = ix->group_bytes = 0;
}

// room for need_docs rows in the per-document attachment arrays (columns, validity, groups): grown to the handle's document
// capacity, like d_doc_offsets, so that an append inside a reservation moves none of them.  The filter kernels' table follows
// the arrays that moved, also where a later one failed to grow.
static int grow_attachments(DeviceIndex* ix, int64_t need_docs) {
  const size_t cap = (size_t)std::max(ix->cap_docs, need_docs), n = (size_t)ix->n_docs, need = (size_t)need_docs;
  int rc = NP_OK;
  bool moved = false;
  for (size_t c = 0; c < ix->columns.size() && rc == NP_OK; ++c) {
    DeviceColumn& col = ix->columns[c];
    const size_t esz = col.type == NP_COL_CODE ? 4 : 8, before = ix->device_bytes;
    if (col.data.bytes() < need * esz) {
      rc = grow_array(ix, col.data, n * esz, cap * esz);
      moved = moved || rc == NP_OK;
    }
    if (rc == NP_OK && col.has_valid && col.valid.bytes() < (need + 31) / 32 * 4) {
      rc = grow_array(ix, col.valid, (n + 31) / 32, (cap + 31) / 32);
      moved = moved || rc == NP_OK;
    }
    ix->column_bytes += ix->device_bytes - before;
  }
  if (moved) {
    std::vector<FilterCol> tab;
    for (const DeviceColumn& col : ix->columns)
      tab.push_back(FilterCol{col.data.get(), col.has_valid ? col.valid.get() : nullptr, col.type, 0});
    const hipError_t e = hipMemcpy(ix->d_coltab.get(), tab.data(), tab.size() * sizeof(FilterCol), hipMemcpyHostToDevice);
    if (e != hipSuccess && rc == NP_OK) {
      set_error("HIP error: %s", hipGetErrorString(e));
      rc = NP_ERR_DEVICE_UNAVAILABLE;
    }
  }
  if (rc == NP_OK && ix->n_groups > 0 && ix->d_groups.bytes() < need * 4) {
    const size_t before = ix->device_bytes;
    rc = grow_array(ix, ix->d_groups, n, cap);
    ix->group_bytes += ix->device_bytes - before;
  }
  return rc;
}

// the rows of the new documents that np_hip_index_append_rows takes, as its arguments give them
struct AppendRows {
  const np_column* cols;
  int32_t n_cols;
  const int32_t* const* remap;   // nullable, and so is every entry
  const int32_t* groups;
  int64_t n_groups;
};
// one workgroup's share of what np_hip_index_set_columns derives from a column's rows (attach_stats_kernel)
struct AttachStats {
  int32_t min_code, max_code;
  long long valid;
};
// ... and staged on the device, with everything that has to be allocated for them, before anything that serves is touched
struct StagedRows {
  struct Col {
    DevPtr<uint8_t> rows;          // the new rows' values
    DevPtr<uint32_t> tail;         // their validity bits at their final positions, from the word of document N0 on
    DevPtr<uint32_t> fresh_valid;  // the bitmap of a column that had none and gains its first NULL
    DevPtr<int32_t> remap;
    int64_t n_remap = 0;
    bool remapped = false;         // a remap is given, also one over no codes at all
    bool any_null = false;
  };
  std::vector<Col> cols;
  DevPtr<int32_t> groups;
  DevPtr<AttachStats> d_stats;
};
static int stage_appended_rows(const DeviceIndex* ix, const AppendRows& rows, int64_t N0, int64_t N1, StagedRows* st);
static int install_appended_rows(DeviceIndex* ix, const AppendRows& rows, StagedRows&& st, int64_t N0, int64_t N1);

// ---- remove from a resident index (np_hip_index_remove) ----------------------------------------------------------------
// Survivors keep their order, so document d becomes d - rank(d) with rank(d) = the removed ids below d, every per-token array
// is an order-preserving compaction towards lower addresses, and every posting list is a filter plus that renumbering.
//
// The survivors: one ballot word per 64 documents (bit = the document stays) and the removed documents in front of each word,
// so that rank(d) is one popcount and one add on 1.4 MB at 10 M documents -- they stay in the L2 under the posting-list pass.
struct KeepMap {
  const uint64_t* bits;     // [ceil(n_docs / 64)]; bits past n_docs are set
  const uint32_t* wrank;    // [same] removed documents with an id below 64 w
};
__device__ __forceinline__ bool doc_kept(const KeepMap& k, uint32_t d) { return (k.bits[d >> 6] >> (d & 63)) & 1ull; }
__device__ __forceinline__ uint32_t doc_rank(const KeepMap& k, uint32_t d) {
  return k.wrank[d >> 6] + (uint32_t)__popcll(~k.bits[d >> 6] & ((1ull << (d & 63)) - 1ull));
}

// removed: the ids to remove, ascending, each once (m > 0).  gone[w] = removed documents of word w
__global__ void __launch_bounds__(256) keep_bitmap_kernel(const int64_t* __restrict__ removed, int64_t m, int64_t n_docs,
                                                          int64_t n_words, uint64_t* __restrict__ bits, uint32_t* __restrict__ gone) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool keep = true;
  if (d < n_docs) {
    int64_t a = 0, z = m;
    while (a < z) {
      const int64_t mid = (a + z) >> 1;
      if (removed[mid] < d) a = mid + 1;
      else z = mid;
    }
    keep = !(a < m && removed[a] == d);
  }
  const unsigned long long word = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && (d >> 6) < n_words) {
    bits[d >> 6] = word;
    gone[d >> 6] = 64u - (uint32_t)__popcll(word);
  }
}

// per survivor, under its NEW id: its length (the scan's input, the max-reduction's too) and where its tokens lie in the old arrays
__global__ void __launch_bounds__(256) survivor_docs_kernel(int64_t n_docs, KeepMap km, const int64_t* __restrict__ old_off,
                                                            int64_t* __restrict__ klen, int64_t* __restrict__ src_start) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= n_docs || !doc_kept(km, (uint32_t)d)) return;
  const int64_t nd = d - doc_rank(km, (uint32_t)d);
  klen[nd] = old_off[d + 1] - old_off[d];
  src_start[nd] = old_off[d];
}

// The posting lists, balanced by ENTRIES like the merge of an append: a workgroup owns NP_FILTER_TILE consecutive entries of the
// OLD array whatever lists they belong to, a thread 4 consecutive ones per step (one aligned 16-byte load).  A count pass gives
// every tile's survivors, a scan over the tiles their first destination, and the placement pass -- the same kernel, the same
// ballots -- puts an entry at the tile's base + the survivors of the waves before its own + those of the lanes before its own +
// those before it in its quad.  The value written is id - rank(id).  No atomics, no workgroup waits for another, the same
// bytes from run to run.
#define NP_FILTER_TILE 4096
#define NP_FILTER_STEPS (NP_FILTER_TILE / 1024)
template <bool PLACE>
__global__ void __launch_bounds__(256) ivf_filter_kernel(const uint32_t* __restrict__ old_ivf, int64_t total, KeepMap km,
                                                         const int64_t* __restrict__ tile_base, int64_t* __restrict__ tile_count,
                                                         uint32_t* __restrict__ out) {
  __shared__ uint32_t s_wave[NP_FILTER_STEPS * 4];
  const int64_t o0 = (int64_t)blockIdx.x * NP_FILTER_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long before = (1ull << lane) - 1ull;
  uint32_t id[NP_FILTER_STEPS][4], mask[NP_FILTER_STEPS], pre[NP_FILTER_STEPS];
#pragma unroll
  for (int it = 0; it < NP_FILTER_STEPS; ++it) {
    const int64_t o = o0 + it * 1024 + (int64_t)threadIdx.x * 4;
    const int n = (int)max((int64_t)0, min((int64_t)4, total - o));
    if (n == 4) {
      const uint4 q = *reinterpret_cast<const uint4*>(old_ivf + o);   // o is a multiple of 4
      id[it][0] = q.x, id[it][1] = q.y, id[it][2] = q.z, id[it][3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) id[it][k] = k < n ? old_ivf[o + k] : 0u;
    }
    uint32_t mk = 0, p = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool keep = k < n && doc_kept(km, id[it][k]);
      const unsigned long long b = __ballot(keep);
      mk |= keep ? 1u << k : 0u;
      p += (uint32_t)__popcll(b & before);
      tot += (uint32_t)__popcll(b);
    }
    mask[it] = mk;
    pre[it] = p;
    if (lane == 0) s_wave[it * 4 + wave] = tot;
  }
  __syncthreads();
  if (!PLACE) {
    if (threadIdx.x == 0) {
      int64_t c = 0;
      for (int i = 0; i < NP_FILTER_STEPS * 4; ++i) c += s_wave[i];
      tile_count[blockIdx.x] = c;
    }
    return;
  }
  int64_t at = tile_base[blockIdx.x];
#pragma unroll
  for (int it = 0; it < NP_FILTER_STEPS; ++it) {
    int64_t w = at;
    for (int i = 0; i < 4; ++i) {
      if (i < wave) w += s_wave[it * 4 + i];
      at += s_wave[it * 4 + i];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (mask[it] & (1u << k))
        out[w + pre[it] + (uint32_t)__popc(mask[it] & ((1u << k) - 1u))] = id[it][k] - doc_rank(km, id[it][k]);
  }
}

// new_off[c] = the survivors in front of old_off[c]: the base of the tile that holds it + the survivors of that tile in front of
// it.  One wave per list boundary (c = 0 .. K), at most 64 coalesced steps.  tile_base has one entry past the last tile.
__global__ void __launch_bounds__(256) ivf_filter_offsets_kernel(const uint32_t* __restrict__ old_ivf, const int64_t* __restrict__ old_off,
                                                                 int64_t K, KeepMap km, const int64_t* __restrict__ tile_base,
                                                                 int64_t* __restrict__ new_off) {
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c > K) return;   // the whole wave
  const int lane = threadIdx.x & 63;
  const int64_t o = old_off[c], tile = o / NP_FILTER_TILE;
  int64_t cnt = 0;
  for (int64_t base = tile * NP_FILTER_TILE; base < o; base += 64) {
    const int64_t i = base + lane;
    cnt += __popcll(__ballot(i < o && doc_kept(km, old_ivf[i])));
  }
  if (lane == 0) new_off[c] = tile_base[tile] + cnt;
}

// The token move, balanced by destination BYTES (documents have 0 to 2049+ tokens): a workgroup owns NP_COMPACT_TILE bytes of the
// destination, cut at multiples of 16 bytes of the destination's address, a thread one 16-byte piece per step.  One thread
// bisects the new offsets for the tile's first document; lanes gallop from there (ivf_list_of).  Destination token n of new
// document j comes from old token src_start[j] + (n - new_off[j]).  A piece whose 16 source bytes are contiguous -- all of them
// but those that hold a removed document's edge -- is one load, as wide as the source ADDRESS allows (16-byte aligned: one
// 16-byte load; 4-byte aligned: the packed quad of the merge; else 2-byte loads: a shift of one 2-byte code allows no more);
// the others, and the ragged pieces at the ends of the range, go byte by byte.  A thread loads all its pieces
// before it stores any.  src and dst may be the same array: the caller's schedule (np_remove_plan.h) sees to it that no
// launch reads a byte it writes.
#define NP_COMPACT_TILE 16384
#define NP_COMPACT_STEPS (NP_COMPACT_TILE / 4096)
struct TokenMove {
  const int64_t* new_off;     // [n_new + 1]
  const int64_t* src_start;   // [n_new]
  int64_t n_new;
  int64_t b0, b1;             // the destination bytes, in the array's coordinates: [dst0 * row, dst1 * row), not empty
  int64_t dshift;             // destination byte b is written at dst + (b - dshift): 0 in place, b0 into the staging buffer
  int32_t row;                // bytes per token
};
__global__ void __launch_bounds__(256) token_compact_kernel(TokenMove m, const uint8_t* src, uint8_t* dst) {
  __shared__ int64_t s_j, s_tok;
  __shared__ uint32_t s_rem;
  const int64_t v_lo = m.b0 - m.dshift, v_hi = m.b1 - m.dshift;   // the destination relative to dst
  const int64_t tile0 = (v_lo & ~(int64_t)15) + (int64_t)blockIdx.x * NP_COMPACT_TILE;
  const int64_t vbase = max(tile0, v_lo);                          // < v_hi: the grid covers the range
  if (threadIdx.x == 0) {
    const int64_t b = vbase + m.dshift;
    s_tok = b / m.row;
    s_rem = (uint32_t)(b - s_tok * m.row);
    s_j = ivf_list_of(m.new_off, m.n_new, 0, s_tok);
  }
  __syncthreads();
  const int64_t tok0 = s_tok;
  const uint32_t rem0 = s_rem, row = (uint32_t)m.row;
  int64_t j = s_j;
  // the source byte of destination byte v (>= vbase); j only moves forward
  auto source = [&](int64_t v) -> int64_t {
    const uint32_t r = rem0 + (uint32_t)(v - vbase), q = r / row;
    const int64_t n = tok0 + q;
    j = ivf_list_of(m.new_off, m.n_new, j, n);
    return (m.src_start[j] + (n - m.new_off[j])) * (int64_t)row + (r - q * row);
  };
  uint32_t w[NP_COMPACT_STEPS][4];
#pragma unroll
  for (int it = 0; it < NP_COMPACT_STEPS; ++it) {
    const int64_t v = tile0 + it * 4096 + (int64_t)threadIdx.x * 16;
    const int64_t lo = max(v, v_lo), hi = min(v + 16, v_hi);
    w[it][0] = w[it][1] = w[it][2] = w[it][3] = 0u;
    if (hi <= lo) continue;
    bool whole = hi - lo == 16;
    if (whole) {
      const int64_t sa = source(v);
      const int64_t j_a = j;
      const int64_t sb = source(v + 15);
      j = j_a;   // the next piece of this thread lies behind, but keep the start for the byte path
      whole = sb - sa == 15;
      if (whole) {
        const uint8_t* p = src + sa;
        const uintptr_t al = reinterpret_cast<uintptr_t>(p);
        if ((al & 15) == 0) {
          const uint4 q = *reinterpret_cast<const uint4*>(p);
          w[it][0] = q.x, w[it][1] = q.y, w[it][2] = q.z, w[it][3] = q.w;
          continue;
        }
        if ((al & 3) == 0) {
          const MergeQuad q = *reinterpret_cast<const MergeQuad*>(p);
          w[it][0] = q.v[0], w[it][1] = q.v[1], w[it][2] = q.v[2], w[it][3] = q.v[3];
          continue;
        }
        if ((al & 1) == 0) {
          const uint16_t* p2 = reinterpret_cast<const uint16_t*>(p);
#pragma unroll
          for (int k = 0; k < 8; ++k) w[it][k >> 1] |= (uint32_t)p2[k] << ((k & 1) * 16);
          continue;
        }
      }   // (an odd address, which the handle's row sizes -- 2, 4 and multiples of 8 bytes -- never give: byte by byte, below)
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (v + k >= lo && v + k < hi) w[it][k >> 2] |= (uint32_t)src[source(v + k)] << ((k & 3) * 8);
  }
#pragma unroll
  for (int it = 0; it < NP_COMPACT_STEPS; ++it) {
    const int64_t v = tile0 + it * 4096 + (int64_t)threadIdx.x * 16;
    const int64_t lo = max(v, v_lo), hi = min(v + 16, v_hi);
    if (hi <= lo) continue;
    if (hi - lo == 16) {
      *reinterpret_cast<uint4*>(dst + v) = make_uint4(w[it][0], w[it][1], w[it][2], w[it][3]);
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (v + k >= lo && v + k < hi) dst[v + k] = (uint8_t)(w[it][k >> 2] >> ((k & 3) * 8));
    }
  }
}

// the survivors among the tokens behind destination token dst0 -> tokens [dst0, dst1) of dst (in place: dst == src), or -- to_staging --
// rows [0, dst1 - dst0) of dst
static void launch_token_compact(const int64_t* new_off, const int64_t* src_start, int64_t n_new, int64_t dst0, int64_t dst1, int row,
                                 bool to_staging, const void* src, void* dst) {
  if (dst1 <= dst0) return;
  TokenMove m{new_off, src_start, n_new, dst0 * row, dst1 * row, to_staging ? dst0 * row : 0, row};
  const int64_t v_lo = m.b0 - m.dshift, v_hi = m.b1 - m.dshift;
  const int64_t tiles = (v_hi - (v_lo & ~(int64_t)15) + NP_COMPACT_TILE - 1) / NP_COMPACT_TILE;
  token_compact_kernel<<<(unsigned)tiles, 256>>>(m, static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst));
}

// the handle's posting lists without the removed documents, the rest renumbered: *ivf [*ivf_size], *ioff / *h_ioff [K + 1]
static int filter_posting_lists(const DeviceIndex* ix, const KeepMap& km, DevPtr<uint32_t>* ivf, DevPtr<int64_t>* ioff,
                                std::vector<int64_t>* h_ioff, int64_t* ivf_size, const OpenTrace& trace) {
  const int64_t K = ix->K, total = ix->ivf_size, tiles = (total + NP_FILTER_TILE - 1) / NP_FILTER_TILE;
  if (tiles >= ((int64_t)1 << 31)) {
    set_error("np_hip_index_remove: %lld posting-list entries are more than one pass takes", (long long)total);
    return NP_ERR_INVALID_ARGUMENT;
  }
  DevPtr<int64_t> d_count, d_base;
  NP_TRY(d_count.alloc((size_t)tiles + 1));
  NP_TRY(d_base.alloc((size_t)tiles + 1));
  NP_HIP(hipMemset(d_count.get() + tiles, 0, 8));
  KernelClock clock(trace.on);
  clock.start();
  if (tiles > 0)
    ivf_filter_kernel<false><<<(unsigned)tiles, 256>>>(ix->d_ivf.get(), total, km, nullptr, d_count.get(), nullptr);
  NP_HIP(hipGetLastError());
  double sec = clock.stop();
  NP_TRY(device_scan_exclusive(d_count.get(), d_base.get(), tiles + 1));
  int64_t kept = 0;
  NP_HIP(hipMemcpy(&kept, d_base.get() + tiles, 8, hipMemcpyDeviceToHost));
  NP_TRY(ioff->alloc((size_t)K + 1));
  NP_TRY(ivf->alloc((size_t)kept));   // the new array beside the old one
  clock.start();
  if (tiles > 0)
    ivf_filter_kernel<true><<<(unsigned)tiles, 256>>>(ix->d_ivf.get(), total, km, d_base.get(), nullptr, ivf->get());
  ivf_filter_offsets_kernel<<<(unsigned)((K + 4) / 4), 256>>>(ix->d_ivf.get(), ix->d_ivf_offsets.get(), K, km, d_base.get(), ioff->get());
  NP_HIP(hipGetLastError());
  sec += clock.stop();
  if (trace.on)
    fprintf(stderr, "[%s] %-28s %8.6f s  %lld entries %lld kept\n", trace.tag, "filter kernel", sec, (long long)total, (long long)kept);
  h_ioff->resize((size_t)K + 1);
  NP_HIP(hipMemcpy(h_ioff->data(), ioff->get(), ((size_t)K + 1) * 8, hipMemcpyDeviceToHost));
  NP_HIP(hipDeviceSynchronize());
  *ivf_size = kept;
  return NP_OK;
}

// ---- the attachments through a remove (np_hip_index_remove_keep) ---------------------------------------------------------
// A column is one array over the documents plus validity bits, the groups one i32 per document: each is an order-preserving
// compaction by the same keep bitmap.  Output-driven: a wave owns 64 consecutive NEW ids, a lane finds its source document by
// select over the bitmap (np_attach_plan.h: a bisection of the words' kept-count prefix, then the k-th set bit of the word)
// -- once for all arrays, attach_select_kernel leaves the source ids in HBM --, loads the value and stores it coalesced; the
// source's validity bit is read in the same lane and the wave's 64 bits leave as one ballot = two words of the new bitmap.
// Lanes past the last survivor vote 0, so the bits past n_docs in the last word are zero, as np_hip_index_set_columns leaves
// them.  No atomics, no workgroup waits for another, the same bytes from run to run.
__global__ void __launch_bounds__(256) attach_select_kernel(KeepMap km, int64_t n_words, int64_t n_new, uint32_t* __restrict__ src_of) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n_new) src_of[j] = (uint32_t)attach_select(km.bits, km.wrank, n_words, j);
}

template <class T>
__global__ void __launch_bounds__(256) attach_compact_kernel(const uint32_t* __restrict__ src_of, int64_t n_old, int64_t n_new,
                                                             const T* __restrict__ src, const uint32_t* __restrict__ src_valid,
                                                             T* __restrict__ dst, uint32_t* __restrict__ dst_valid) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool ok = false;
  if (j < n_new) {
    const int64_t d = src_of[j];
    if (d < n_old) {   // always, with a bitmap and ranks that agree
      dst[j] = src[d];
      ok = !src_valid || ((src_valid[d >> 5] >> (d & 31)) & 1u);
    }
  }
  const unsigned long long word = __ballot(ok);
  if (dst_valid && (threadIdx.x & 63) == 0) {
    const int64_t v = j >> 5, nvw = (n_new + 31) >> 5;
    if (v < nvw) dst_valid[v] = attach_ballot_word(word, 0);
    if (v + 1 < nvw) dst_valid[v + 1] = attach_ballot_word(word, 1);
  }
}

// what np_hip_index_set_columns derives from a column's rows, for the surviving ones: the range of a CODE column's codes (from
// its start values 0 and -1) and the rows that are not NULL.  Every workgroup leaves one partial, the host folds them.
#define NP_ATTACH_STAT_BLOCKS 128
__global__ void __launch_bounds__(256) attach_stats_kernel(const int32_t* __restrict__ codes, const uint32_t* __restrict__ valid,
                                                           int64_t n, AttachStats* __restrict__ out) {
  __shared__ AttachStats part[4];
  const int64_t stride = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
  AttachStats s{0, -1, 0};
  if (codes)
    for (int64_t i = first; i < n; i += stride) {
      const int32_t c = codes[i];
      s.min_code = min(s.min_code, c);
      s.max_code = max(s.max_code, c);
    }
  if (valid)
    for (int64_t i = first, nvw = (n + 31) >> 5; i < nvw; i += stride) s.valid += __popc(valid[i]);   // the tail bits are zero
  for (int o = 32; o > 0; o >>= 1) {
    s.min_code = min(s.min_code, __shfl_down(s.min_code, o));
    s.max_code = max(s.max_code, __shfl_down(s.max_code, o));
    s.valid += __shfl_down(s.valid, o);
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      s.min_code = min(s.min_code, part[w].min_code);
      s.max_code = max(s.max_code, part[w].max_code);
      s.valid += part[w].valid;
    }
    out[blockIdx.x] = s;
  }
}

// the compacted attachments, built beside the ones that serve
struct KeptAttachments {
  std::vector<DeviceColumn> columns;   // data, validity and what is derived from the rows; the dictionary text stays where it is
  DevPtr<FilterCol> d_coltab;
  size_t column_bytes = 0;
  DevPtr<int32_t> d_groups;
  size_t group_bytes = 0;
};

static int compact_attachments(const DeviceIndex* ix, const KeepMap& km, int64_t W, int64_t N0, int64_t N1, KeptAttachments* k,
                               const OpenTrace& trace) {
  const size_t nc = ix->columns.size();
  const int64_t nvw = (N1 + 31) / 32;
  const size_t cap = (size_t)ix->cap_docs;   // the arrays keep the handle's document capacity: a later append moves none of them
  const unsigned grid = (unsigned)((N1 + 255) / 256);
  const int sblocks = (int)std::min<int64_t>(NP_ATTACH_STAT_BLOCKS, grid);
  DevPtr<AttachStats> d_stats;
  DevPtr<uint32_t> d_src;   // the old id of every survivor, by new id
  NP_TRY(d_src.alloc((size_t)N1));
  k->columns.resize(nc);
  for (size_t c = 0; c < nc; ++c) {   // every allocation first: nothing is launched when one fails
    const DeviceColumn& o = ix->columns[c];
    DeviceColumn& f = k->columns[c];
    f.type = o.type;
    f.has_valid = o.has_valid && N1 > 0;
    NP_TRY(f.data.alloc(cap * (o.type == NP_COL_CODE ? 4 : 8), &k->column_bytes));
    if (f.has_valid) NP_TRY(f.valid.alloc((cap + 31) / 32, &k->column_bytes));
  }
  if (nc > 0) {
    NP_TRY(k->d_coltab.alloc(nc, &k->column_bytes));
    NP_TRY(d_stats.alloc(nc * NP_ATTACH_STAT_BLOCKS));
  }
  if (ix->n_groups > 0 && N1 > 0) NP_TRY(k->d_groups.alloc(cap, &k->group_bytes));
  KernelClock clock(trace.on);
  clock.start();
  double bytes = 0;   // what the kernels read and write: the bitmap and the ranks, the source ids, rows and validity words
  if (N1 > 0 && (nc > 0 || k->d_groups.get())) {
    attach_select_kernel<<<grid, 256>>>(km, W, N1, d_src.get());
    bytes += 12.0 * (double)W + 4.0 * (double)N1;
  }
  for (size_t c = 0; c < nc && N1 > 0; ++c) {
    const DeviceColumn& o = ix->columns[c];
    DeviceColumn& f = k->columns[c];
    if (o.type == NP_COL_CODE)
      attach_compact_kernel<uint32_t><<<grid, 256>>>(d_src.get(), N0, N1, reinterpret_cast<const uint32_t*>(o.data.get()),
                                                     o.has_valid ? o.valid.get() : nullptr,
                                                     reinterpret_cast<uint32_t*>(f.data.get()), f.valid.get());
    else
      attach_compact_kernel<uint64_t><<<grid, 256>>>(d_src.get(), N0, N1, reinterpret_cast<const uint64_t*>(o.data.get()),
                                                     o.has_valid ? o.valid.get() : nullptr,
                                                     reinterpret_cast<uint64_t*>(f.data.get()), f.valid.get());
    bytes += (double)N1 * (4 + 2 * (o.type == NP_COL_CODE ? 4 : 8)) + (f.has_valid ? (double)nvw * 4 + (double)((N0 + 31) / 32) * 4 : 0);
  }
  if (k->d_groups.get()) {
    attach_compact_kernel<uint32_t><<<grid, 256>>>(d_src.get(), N0, N1, reinterpret_cast<const uint32_t*>(ix->d_groups.get()), nullptr,
                                                   reinterpret_cast<uint32_t*>(k->d_groups.get()), nullptr);
    bytes += 3.0 * (double)N1 * 4;
  }
  NP_HIP(hipGetLastError());
  const double sec = clock.stop();
  if (trace.on)
    fprintf(stderr, "[%s] %-28s %8.6f s  %.0f bytes %.1f GB/s\n", trace.tag, "attach kernel", sec, bytes,
            sec > 0 ? bytes / sec * 1e-9 : 0.0);
  // what set_columns derives from the rows: the code range, and no bitmap at all where no survivor is NULL
  std::vector<AttachStats> h_stats(nc * NP_ATTACH_STAT_BLOCKS);
  for (size_t c = 0; c < nc && N1 > 0; ++c) {
    const DeviceColumn& f = k->columns[c];
    if (f.type == NP_COL_CODE || f.has_valid)
      attach_stats_kernel<<<(unsigned)sblocks, 256>>>(f.type == NP_COL_CODE ? reinterpret_cast<const int32_t*>(f.data.get()) : nullptr,
                                                      f.valid.get(), N1, d_stats.get() + c * NP_ATTACH_STAT_BLOCKS);
  }
  NP_HIP(hipGetLastError());
  if (nc > 0 && N1 > 0) NP_HIP(hipMemcpy(h_stats.data(), d_stats.get(), h_stats.size() * sizeof(AttachStats), hipMemcpyDeviceToHost));
  std::vector<FilterCol> tab(nc);
  for (size_t c = 0; c < nc; ++c) {
    DeviceColumn& f = k->columns[c];
    long long valid = 0;
    for (int b = 0; b < sblocks && N1 > 0 && (f.type == NP_COL_CODE || f.has_valid); ++b) {
      const AttachStats& s = h_stats[c * NP_ATTACH_STAT_BLOCKS + (size_t)b];
      f.min_code = std::min(f.min_code, s.min_code);
      f.max_code = std::max(f.max_code, s.max_code);
      valid += s.valid;
    }
    if (f.has_valid && valid == N1) {
      k->column_bytes -= f.valid.bytes();
      f.valid.reset();
      f.has_valid = false;
    }
    tab[c] = FilterCol{f.data.get(), f.has_valid ? f.valid.get() : nullptr, f.type, 0};
  }
  if (nc > 0) NP_HIP(hipMemcpy(k->d_coltab.get(), tab.data(), nc * sizeof(FilterCol), hipMemcpyHostToDevice));
  NP_HIP(hipDeviceSynchronize());
  return NP_OK;
}

// the handle's attachments become the compacted ones; the keyword index, whose term numbering a removed row can change, goes
static void install_kept_attachments(DeviceIndex* ix, KeptAttachments&& k) {
  for (size_t c = 0; c < ix->columns.size(); ++c) {
    DeviceColumn& col = ix->columns[c];
    DeviceColumn& f = k.columns[c];
    col.data = std::move(f.data);
    col.valid = std::move(f.valid);
    col.has_valid = f.has_valid;
    col.min_code = f.min_code;
    col.max_code = f.max_code;
  }
  ix->d_coltab = std::move(k.d_coltab);
  if (!k.d_groups.get()) ix->n_groups = 0;   // no document left: what np_hip_index_set_groups makes of no ids
  ix->d_groups = std::move(k.d_groups);
  ix->text = DeviceText();
  ix->device_bytes = ix->device_bytes - ix->column_bytes - ix->group_bytes - ix->text_bytes + k.column_bytes + k.group_bytes;
  ix->column_bytes = k.column_bytes;
  ix->group_bytes = k.group_bytes;
  ix->text_bytes = 0;
}

// ---- the attachments through an append (np_hip_index_append_rows) ----------------------------------------------------------
// The new rows go behind the old ones in arrays that have the room (grow_attachments): outside what any kernel reads until
// the counts move.  What does touch serving rows -- a dictionary remap over the old codes, the validity word the old last
// document shares with the first new one -- happens once nothing can fail any more.

// old code -> new code over the rows that are not NULL (a NULL row's code means nothing and keeps its bytes)
__global__ void __launch_bounds__(256) attach_remap_kernel(int32_t* __restrict__ codes, const uint32_t* __restrict__ valid, int64_t n,
                                                           const int32_t* __restrict__ remap, int64_t n_remap) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= n || (valid && !((valid[d >> 5] >> (d & 31)) & 1u))) return;
  const int32_t c = codes[d];
  if (c >= 0 && c < n_remap) codes[d] = remap[c];
}

// valid[w0 + i] = tail[i], the first word merged with the old rows' bits (np_attach_plan.h attach_merge_word)
__global__ void __launch_bounds__(256) attach_tail_merge_kernel(uint32_t* __restrict__ valid, const uint32_t* __restrict__ tail,
                                                                int64_t w0, int64_t n_tail, int shared_bits, bool fresh) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_tail) return;
  valid[w0 + i] = i == 0 ? attach_merge_word(fresh ? 0u : valid[w0], tail[0], shared_bits, fresh) : tail[i];
}

static int stage_appended_rows(const DeviceIndex* ix, const AppendRows& rows, int64_t N0, int64_t N1, StagedRows* st) {
  const int64_t n = N1 - N0, w0 = N0 >> 5, n_tail = ((N1 + 31) >> 5) - w0;
  const size_t cap_words = ((size_t)std::max(ix->cap_docs, N1) + 31) / 32;
  st->cols.resize(ix->columns.size());
  std::vector<uint32_t> bits;
  for (size_t c = 0; c < ix->columns.size(); ++c) {
    const DeviceColumn& col = ix->columns[c];
    const np_column& in = rows.cols[c];
    StagedRows::Col& s = st->cols[c];
    const size_t esz = col.type == NP_COL_CODE ? 4 : 8;
    NP_TRY(s.rows.alloc((size_t)n * esz));
    NP_HIP(hipMemcpy(s.rows.get(), in.data, (size_t)n * esz, hipMemcpyHostToDevice));
    // validity as np_hip_index_set_columns reads it: the caller's bytes, and an f64 NaN is NULL whatever they say
    bits.assign((size_t)n_tail, 0u);
    const double* f64 = col.type == NP_COL_F64 ? (const double*)in.data : nullptr;
    for (int64_t i = 0; i < n; ++i) {
      const bool ok = (!in.valid || in.valid[i] != 0) && (!f64 || f64[i] == f64[i]);
      if (ok) bits[(size_t)(((N0 + i) >> 5) - w0)] |= 1u << ((N0 + i) & 31); else s.any_null = true;
    }
    if (col.has_valid || s.any_null) {
      NP_TRY(s.tail.alloc((size_t)n_tail));
      NP_HIP(hipMemcpy(s.tail.get(), bits.data(), (size_t)n_tail * 4, hipMemcpyHostToDevice));
    }
    if (!col.has_valid && s.any_null) NP_TRY(s.fresh_valid.alloc(cap_words));
    if (rows.remap && rows.remap[c]) {
      s.remapped = true;
      s.n_remap = (int64_t)col.max_code + 1;
      NP_TRY(s.remap.alloc((size_t)s.n_remap));
      if (s.n_remap > 0) NP_HIP(hipMemcpy(s.remap.get(), rows.remap[c], (size_t)s.n_remap * 4, hipMemcpyHostToDevice));
    }
  }
  if (ix->n_groups > 0) {
    NP_TRY(st->groups.alloc((size_t)n));
    NP_HIP(hipMemcpy(st->groups.get(), rows.groups, (size_t)n * 4, hipMemcpyHostToDevice));
  }
  if (!ix->columns.empty()) NP_TRY(st->d_stats.alloc(ix->columns.size() * NP_ATTACH_STAT_BLOCKS));
  return NP_OK;
}

// every context is held and every allocation is made: the rows join the handle's.  The keyword index, whose vocabulary the new
// rows' text changes, goes.  An error here is a device that stopped answering.
static int install_appended_rows(DeviceIndex* ix, const AppendRows& rows, StagedRows&& st, int64_t N0, int64_t N1) {
  const int64_t n = N1 - N0, w0 = N0 >> 5, n_tail = ((N1 + 31) >> 5) - w0;
  const size_t nc = ix->columns.size();
  const int sblocks = (int)std::min<int64_t>(NP_ATTACH_STAT_BLOCKS, (N1 + 255) / 256);
  bool table_changed = false;
  for (size_t c = 0; c < nc; ++c) {
    DeviceColumn& col = ix->columns[c];
    StagedRows::Col& s = st.cols[c];
    const size_t esz = col.type == NP_COL_CODE ? 4 : 8;
    if (s.remapped) {
      if (N0 > 0 && s.n_remap > 0)
        attach_remap_kernel<<<(unsigned)((N0 + 255) / 256), 256>>>(reinterpret_cast<int32_t*>(col.data.get()),
                                                                   col.has_valid ? col.valid.get() : nullptr, N0, s.remap.get(), s.n_remap);
      col.text.reset();   // the text was the old dictionary's: np_hip_index_set_column_text sets the grown one
      col.text_off.reset();
      ix->device_bytes -= col.text_acct;
      ix->coltext_bytes -= col.text_acct;
      col.text_acct = 0;
      col.n_strings = col.n_text_bytes = 0;
    }
    (void)hipMemcpyAsync(col.data.get() + (size_t)N0 * esz, s.rows.get(), (size_t)n * esz, hipMemcpyDeviceToDevice, nullptr);
    if (s.tail.get()) {
      const bool fresh = !col.has_valid;
      if (fresh) {
        (void)hipMemsetAsync(s.fresh_valid.get(), 0xff, (size_t)w0 * 4, nullptr);
        ix->device_bytes += s.fresh_valid.bytes();
        ix->column_bytes += s.fresh_valid.bytes();
        col.valid = std::move(s.fresh_valid);
        col.has_valid = true;
        table_changed = true;
      }
      attach_tail_merge_kernel<<<(unsigned)((n_tail + 255) / 256), 256>>>(col.valid.get(), s.tail.get(), w0, n_tail, (int)(N0 & 31), fresh);
    }
    if (col.type == NP_COL_CODE)   // the code range of all rows, as np_hip_index_set_columns takes it
      attach_stats_kernel<<<(unsigned)sblocks, 256>>>(reinterpret_cast<const int32_t*>(col.data.get()), nullptr, N1,
                                                      st.d_stats.get() + c * NP_ATTACH_STAT_BLOCKS);
  }
  if (ix->n_groups > 0) {
    (void)hipMemcpyAsync(ix->d_groups.get() + N0, st.groups.get(), (size_t)n * 4, hipMemcpyDeviceToDevice, nullptr);
    ix->n_groups = rows.n_groups;
  }
  ix->text = DeviceText();
  ix->device_bytes -= ix->text_bytes;
  ix->text_bytes = 0;
  std::vector<AttachStats> h_stats(nc * NP_ATTACH_STAT_BLOCKS);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && nc > 0)
    e = hipMemcpy(h_stats.data(), st.d_stats.get(), h_stats.size() * sizeof(AttachStats), hipMemcpyDeviceToHost);
  if (e == hipSuccess && table_changed) {
    std::vector<FilterCol> tab;
    for (const DeviceColumn& col : ix->columns)
      tab.push_back(FilterCol{col.data.get(), col.has_valid ? col.valid.get() : nullptr, col.type, 0});
    e = hipMemcpy(ix->d_coltab.get(), tab.data(), nc * sizeof(FilterCol), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();   // the staged rows are freed when this returns
  if (e != hipSuccess) {
    set_error("np_hip_index_append_rows: the rows' move failed: %s", hipGetErrorString(e));
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  for (size_t c = 0; c < nc; ++c) {
    DeviceColumn& col = ix->columns[c];
    if (col.type != NP_COL_CODE) continue;
    col.min_code = 0;
    col.max_code = -1;
    for (int b = 0; b < sblocks; ++b) {
      col.min_code = std::min(col.min_code, h_stats[c * NP_ATTACH_STAT_BLOCKS + (size_t)b].min_code);
      col.max_code = std::max(col.max_code, h_stats[c * NP_ATTACH_STAT_BLOCKS + (size_t)b].max_code);
    }
  }
  return NP_OK;
}

// removed: the ids to remove -- in range, ascending, each once, not empty.  keep: columns and groups are compacted with the
// documents (np_hip_index_remove_keep), where the plain remove drops them
static int remove_documents(DeviceIndex* ix, const std::vector<int64_t>& removed, bool keep, const char* entry) {
  UpdateSection section(ix);
  NP_TRY(section.begin());
  const int64_t N0 = ix->n_docs, m = (int64_t)removed.size(), N1 = N0 - m, T0 = ix->T, W = (N0 + 63) / 64;
  OpenTrace trace("NP_REMOVE_TRACE", "np remove");
  // 1. the survivors: bitmap, ranks, the new doc offsets (at the capacity the old ones have) and the longest survivor
  DevPtr<int64_t> d_removed, d_klen, d_src, d_newoff, d_max;
  DevPtr<uint64_t> d_bits;
  DevPtr<uint32_t> d_gone, d_wrank;
  NP_TRY(d_removed.alloc((size_t)m));
  NP_TRY(d_bits.alloc((size_t)W));
  NP_TRY(d_gone.alloc((size_t)W));
  NP_TRY(d_wrank.alloc((size_t)W));
  NP_TRY(d_klen.alloc((size_t)N1));
  NP_TRY(d_src.alloc((size_t)N1));
  NP_TRY(d_max.alloc(1));
  NP_TRY(d_newoff.alloc((size_t)ix->cap_docs + 1));
  NP_HIP(hipMemcpy(d_removed.get(), removed.data(), (size_t)m * 8, hipMemcpyHostToDevice));
  keep_bitmap_kernel<<<(unsigned)((N0 + 255) / 256), 256>>>(d_removed.get(), m, N0, W, d_bits.get(), d_gone.get());
  NP_HIP(hipGetLastError());
  NP_TRY(device_scan_exclusive(d_gone.get(), d_wrank.get(), W));
  const KeepMap km{d_bits.get(), d_wrank.get()};
  survivor_docs_kernel<<<(unsigned)((N0 + 255) / 256), 256>>>(N0, km, ix->d_doc_offsets.get(), d_klen.get(), d_src.get());
  NP_HIP(hipGetLastError());
  NP_HIP(hipMemset(d_newoff.get(), 0, 8));
  int64_t maxlen = 0, T1 = 0;
  if (N1 > 0) {
    NP_TRY(device_scan_inclusive(d_klen.get(), d_newoff.get() + 1, N1));
    DevPtr<uint8_t> d_temp;
    size_t tb = 0;
    NP_HIP(hipcub::DeviceReduce::Max(nullptr, tb, d_klen.get(), d_max.get(), (int)N1));
    NP_TRY(d_temp.alloc(std::max<size_t>(tb, 16)));
    NP_HIP(hipcub::DeviceReduce::Max(d_temp.get(), tb, d_klen.get(), d_max.get(), (int)N1));
    NP_HIP(hipMemcpy(&maxlen, d_max.get(), 8, hipMemcpyDeviceToHost));
    NP_HIP(hipMemcpy(&T1, d_newoff.get() + N1, 8, hipMemcpyDeviceToHost));
  }
  // the schedule of the in-place moves, from the host's copy of the old offsets
  std::vector<int64_t> h_off((size_t)N0 + 1);
  NP_HIP(hipMemcpy(h_off.data(), ix->d_doc_offsets.get(), h_off.size() * 8, hipMemcpyDeviceToHost));
  std::vector<uint8_t> h_keep((size_t)N0, 1);
  for (int64_t d : removed) h_keep[(size_t)d] = 0;
  const RemovePlan plan = remove_plan(h_off.data(), h_keep.data(), N0, ix->pd, ix->tune.remove_slab);
  if (plan.new_tokens != T1) {
    set_error("internal: the remove plan counts %lld tokens, the device %lld", (long long)plan.new_tokens, (long long)T1);
    return NP_ERR_INVALID_ARGUMENT;
  }
  const int64_t first = plan.first_moved;   // tokens in front of it stay where they are
  trace.mark("survivors");
  // 2. the codes, compacted BESIDE the old ones: the distinct-code structures are built from them while the old arrays serve
  const int cb = (int)ix->code_bytes();
  DevPtr<uint8_t> codes;
  NP_TRY(codes.alloc((size_t)std::max<int64_t>(ix->cap_tokens, 1) * cb));
  if (first > 0) NP_HIP(hipMemcpy(codes.get(), ix->d_codes.get(), (size_t)first * cb, hipMemcpyDeviceToDevice));
  launch_token_compact(d_newoff.get(), d_src.get(), N1, first, T1, cb, false, ix->d_codes.get(), codes.get());
  NP_HIP(hipGetLastError());
  trace.mark("codes beside");
  // 3. the distinct-code structures of the shrunk index
  Ucodes u;
  DevPtr<int64_t> d_uoff;
  NP_TRY(build_unique_codes(ix, TokensView{d_newoff.get(), CodeArr{codes.get(), ix->code_wide}}, N1, &u, &d_uoff));
  d_uoff.reset();
  trace.mark("distinct-code rebuild");
  // 4. the posting lists
  StagedLists lists;
  NP_TRY(filter_posting_lists(ix, km, &lists.ivf, &lists.ioff, &lists.h_ioff, &lists.ivf_size, trace));
  lists.replaced = true;
  trace.mark("posting-list filter");
  // 5. their range table
  NP_TRY(stage_ivf_split(ix, u, N1, &lists));
  trace.mark("range table");
  // 5b. columns and groups of the survivors, beside the ones that serve
  KeptAttachments kept;
  if (keep) {
    NP_TRY(compact_attachments(ix, km, W, N0, N1, &kept, trace));
    trace.mark("attachments");
  }
  // 6. the staging buffer of the in-place moves: the last thing that can fail
  DevPtr<uint8_t> staging;
  if (plan.staging_bytes > 0) NP_TRY(staging.alloc((size_t)plan.staging_bytes));
  // ---- nothing below can fail: the handle becomes the shrunk index ----
  struct Moved {
    void* p;
    int row;
  };
  const Moved arrays[3] = {{ix->d_residuals.get(), ix->pd}, {ix->d_inv_norm.get(), 4}, {ix->tok_sorted ? ix->d_tok_pos.get() : nullptr, 2}};
  KernelClock clock(trace.on);
  double sec_direct = 0, sec_staged = 0;
  for (const RemoveLaunch& l : plan.launches) {
    clock.start();
    for (const Moved& a : arrays) {
      if (!a.p) continue;
      if (l.mode == NP_REMOVE_DIRECT) launch_token_compact(d_newoff.get(), d_src.get(), N1, l.dst0, l.dst1, a.row, false, a.p, a.p);
      else if (l.mode == NP_REMOVE_GATHER) launch_token_compact(d_newoff.get(), d_src.get(), N1, l.dst0, l.dst1, a.row, true, a.p, staging.get());
      if (l.mode == NP_REMOVE_GATHER)   // ... and the copy out of it, behind the gather in stream order
        (void)hipMemcpyAsync(static_cast<uint8_t*>(a.p) + l.dst0 * a.row, staging.get(), (size_t)(l.dst1 - l.dst0) * a.row,
                             hipMemcpyDeviceToDevice, nullptr);
    }
    (l.mode == NP_REMOVE_DIRECT ? sec_direct : sec_staged) += clock.stop();
  }
  const hipError_t moved = hipDeviceSynchronize();
  if (trace.on) {
    const double per_token = (double)ix->pd + 4 + (ix->tok_sorted ? 2 : 0);
    fprintf(stderr, "[%s] %-28s %8.6f s  %lld tokens %.0f bytes each\n", trace.tag, "move kernel direct", sec_direct,
            (long long)plan.direct_tokens, per_token);
    fprintf(stderr, "[%s] %-28s %8.6f s  %lld tokens %.0f bytes each\n", trace.tag, "move kernel staged", sec_staged,
            (long long)plan.staged_tokens, per_token);
  }
  trace.mark("token move");
  staging.reset();
  ix->device_bytes = ix->device_bytes - ix->d_codes.bytes() - ix->d_doc_offsets.bytes() + codes.bytes() + d_newoff.bytes();
  ix->d_codes = std::move(codes);
  ix->d_doc_offsets = std::move(d_newoff);
  install_ucodes(ix, std::move(u));
  install_lists(ix, std::move(lists));
  // tokens / documents, what the directory delete writes (np_update.cpp delete_impl) and a handle made from arrays reports
  ix->avg_doclen = N1 > 0 ? (double)T1 / (double)N1 : 0.0;
  ix->n_docs = ix->N_total = N1;
  ix->T = T1;
  ix->n_emb_total -= T0 - T1;
  ix->max_doc_len = maxlen;
  if (keep) install_kept_attachments(ix, std::move(kept));
  else drop_attachments(ix);
  finish_update(ix);
  trace.mark("swap");
  if (moved != hipSuccess) {   // not an allocation: a device that stopped answering
    set_error("%s: the token move failed: %s", entry, hipGetErrorString(moved));
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  return NP_OK;
}

// ---- expand a resident index (np_hip_index_expand) --------------------------------------------------------------------
// The crate's usual update (index.rs:1515-1562, np_update.cpp update_impl): the buffered documents leave the tail, new centroids
// join the codec, and buffer ++ new documents are appended against the grown codec.  On the handle that is ONE exclusive
// section: the dropped tokens are the last ones, so nothing is compacted -- the new tokens land where the tail was (saved
// beside, and put back when anything fails before the swap); the distinct-code structures are built once over the final
// documents; and the posting lists are rewritten in one streaming pass that cuts every old list at the first dropped id and
// hangs the given documents' pairs behind it.  What depends on K follows K1 = K + k_new: the centroid table and its bounds, the
// code width, the eighths of the centroid range in d_useg, the list offsets, the range table and the planner's bound.

// u16 codes -> u32: a lane takes 8 codes with one 16-byte load and leaves them with two 16-byte stores; the last n % 8 codes go
// one by one.  Both arrays are hipMalloc'ed (256-byte aligned), dst holds at least n entries.
__global__ void __launch_bounds__(256) widen_codes_kernel(const uint16_t* __restrict__ src, int64_t n, uint32_t* __restrict__ dst) {
  const int64_t n8 = n >> 3, tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = tid; i < n8; i += stride) {
    const uint4 v = reinterpret_cast<const uint4*>(src)[i];
    reinterpret_cast<uint4*>(dst)[2 * i] = make_uint4(v.x & 0xFFFFu, v.x >> 16, v.y & 0xFFFFu, v.y >> 16);
    reinterpret_cast<uint4*>(dst)[2 * i + 1] = make_uint4(v.z & 0xFFFFu, v.z >> 16, v.w & 0xFFFFu, v.w >> 16);
  }
  const int64_t t = (n8 << 3) + tid;
  if (tid < 8 && t < n) dst[t] = src[t];
}

// what list c of the K1 lists keeps of the old array: old_begin[c] and n_keep[c] = its entries with id < n_keep_docs (the lists
// ascend: one bisection); lists K0 .. K1 - 1 are new and keep nothing.  Entry K1 is the scan's closing zero.
__global__ void __launch_bounds__(256) ivf_keep_kernel(const uint32_t* __restrict__ ivf, const int64_t* __restrict__ old_off, int64_t K0,
                                                       int64_t K1, int64_t n_keep_docs, int64_t* __restrict__ old_begin,
                                                       int64_t* __restrict__ n_keep) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c > K1) return;
  if (c >= K0) {
    old_begin[c] = 0;
    n_keep[c] = 0;
    return;
  }
  const int64_t s0 = old_off[c];
  const uint32_t* L = ivf + s0;
  int64_t a = 0, z = old_off[c + 1] - s0;
  while (a < z) {
    const int64_t mid = (a + z) >> 1;
    if ((int64_t)L[mid] < n_keep_docs) a = mid + 1;
    else z = mid;
  }
  old_begin[c] = s0;
  n_keep[c] = a;
}

static int as_expand_argument(const char* entry, int rc, const char* arg) {
  if (rc == NP_OK || rc == NP_ERR_OUT_OF_MEMORY || rc == NP_ERR_DEVICE_UNAVAILABLE) return rc;
  const std::string msg = last_error();
  set_error("%s: %s: %s", entry, arg, msg.c_str());
  return NP_ERR_INVALID_ARGUMENT;
}

// The K1 = ix->K posting lists (the handle's K-dependent scalars are the grown ones by now; its d_ivf / d_ivf_offsets still the
// K0 old lists): every old list cut at document Nk, then the pairs of documents [Nk, N1) from the distinct-code lists of the
// final index (u, d_uoff).  A call that cuts nothing and adds no list -- an append -- hands the kernel the handle's own offsets
// and, when the given documents hold no pair either, leaves the handle's lists where they are (st->replaced stays false).
// raw_lists: a given document is longer than NP_UNIQ_MAX tokens, so its list is its codes as they are, duplicates included --
// a posting list names a document once (index.rs:479-499), so equal pairs, adjacent once sorted, are dropped.
static int rewrite_posting_lists(const DeviceIndex* ix, int64_t K0, const Ucodes& u, const int64_t* d_uoff, int64_t Nk, int64_t N1,
                                   bool raw_lists, StagedLists* st, const char* entry, const OpenTrace& trace) {
  const int64_t K = ix->K, n_new = N1 - Nk;
  const bool cuts = K0 != K || Nk != ix->n_docs;
  DevPtr<int64_t> d_len64, d_upfx, d_start, d_begin, d_keep, d_kpfx;
  DevPtr<uint64_t> d_k1, d_k2;
  int64_t P = 0;   // (code, document) pairs of the given documents
  st->ivf_size = ix->ivf_size;
  if (n_new > 0) {
    NP_TRY(d_len64.alloc((size_t)n_new));
    NP_TRY(d_upfx.alloc((size_t)n_new));
    ulen_to_i64_kernel<<<(unsigned)((n_new + 255) / 256), 256>>>(u.d_ulen.get() + Nk, n_new, d_len64.get());
    NP_TRY(device_scan_inclusive(d_len64.get(), d_upfx.get(), n_new));
    NP_HIP(hipMemcpy(&P, d_upfx.get() + (n_new - 1), 8, hipMemcpyDeviceToHost));
    d_len64.reset();
  }
  if (P == 0 && !cuts) return NP_OK;
  if (P >= ((int64_t)1 << 31)) {   // one radix sort, as one document range of build_ivf_from_ucodes
    set_error("%s: n_docs: the %s documents hold %lld (code, doc) pairs, one call takes < 2^31", entry, cuts ? "given" : "new", (long long)P);
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(d_start.alloc((size_t)K + 1));
  NP_TRY(d_k1.alloc((size_t)P));
  NP_TRY(d_k2.alloc((size_t)P));
  if (P > 0) {
    int kbits = 1;
    while (((int64_t)1 << kbits) < K) ++kbits;
    ivf_emit_pairs_kernel<<<(unsigned)((n_new + 3) / 4), 256>>>(Nk, N1, d_uoff, CodeArr{u.d_ucodes.get(), ix->code_wide}, u.d_ulen.get(),
                                                              d_upfx.get(), Nk, 0, d_k1.get());
    NP_HIP(hipGetLastError());
    NP_TRY(device_sort_pairs(d_k1.get(), d_k2.get(), P, kbits));
    if (raw_lists) {
      NP_TRY(device_unique(d_k2.get(), d_k1.get(), P, &P));
      std::swap(d_k1, d_k2);   // d_k2 = the sorted pairs, each once
    }
  }
  ivf_code_starts_kernel<<<(unsigned)((K + 256) / 256), 256>>>(d_k2.get(), P, K, d_start.get());
  NP_HIP(hipGetLastError());
  // the cut: what every list keeps, and where the kept parts begin in an array of them alone
  const int64_t *old_begin = ix->d_ivf_offsets.get(), *kept_pfx = ix->d_ivf_offsets.get();
  int64_t kept = ix->ivf_size;
  if (cuts) {
    NP_TRY(d_begin.alloc((size_t)K + 1));
    NP_TRY(d_keep.alloc((size_t)K + 1));
    NP_TRY(d_kpfx.alloc((size_t)K + 1));
    ivf_keep_kernel<<<(unsigned)((K + 256) / 256), 256>>>(ix->d_ivf.get(), ix->d_ivf_offsets.get(), K0, K, Nk, d_begin.get(), d_keep.get());
    NP_HIP(hipGetLastError());
    NP_TRY(device_scan_exclusive(d_keep.get(), d_kpfx.get(), K + 1));
    NP_HIP(hipMemcpy(&kept, d_kpfx.get() + K, 8, hipMemcpyDeviceToHost));
    old_begin = d_begin.get(), kept_pfx = d_kpfx.get();
  }
  const int64_t total = kept + P;
  NP_TRY(st->ioff.alloc((size_t)K + 1));
  NP_TRY(st->ivf.alloc((size_t)total));   // the new array beside the old one: the pass reads the one and writes the other
  ivf_cut_offsets_kernel<<<(unsigned)((K + 256) / 256), 256>>>(kept_pfx, d_start.get(), K, st->ioff.get());
  NP_HIP(hipGetLastError());
  KernelClock clock(trace.on);   // NP_APPEND_TRACE: the kernel alone, for its bytes per second
  clock.start();
  if (total > 0)
    ivf_cut_merge_kernel<<<(unsigned)((total + NP_MERGE_TILE - 1) / NP_MERGE_TILE), 256>>>(
        ix->d_ivf.get(), old_begin, kept_pfx, d_k2.get(), d_start.get(), st->ioff.get(), K, total, st->ivf.get());
  NP_HIP(hipGetLastError());
  if (trace.on && cuts)
    fprintf(stderr, "[%s] %-28s %8.6f s  %lld entries %lld new %lld cut\n", trace.tag, "cut-merge kernel", clock.stop(), (long long)total,
            (long long)P, (long long)(ix->ivf_size - kept));
  else if (trace.on)
    fprintf(stderr, "[%s] %-28s %8.6f s  %lld entries %lld new\n", trace.tag, "merge kernel", clock.stop(), (long long)total, (long long)P);
  st->h_ioff.resize((size_t)K + 1);
  NP_HIP(hipMemcpy(st->h_ioff.data(), st->ioff.get(), ((size_t)K + 1) * 8, hipMemcpyDeviceToHost));
  NP_HIP(hipDeviceSynchronize());
  st->ivf_size = total;
  st->replaced = true;
  return NP_OK;
}

// What an expand flips or overwrites before its swap, and the way back: the K-dependent scalars and the two arrays that are
// replaced whole (centroids; the codes when they widen) are exchanged early so that the shared open stages run on the grown
// geometry, and the tail of the per-token arrays and of the doc offsets is overwritten by the given documents.  Every context
// is held meanwhile.  Unless commit() is reached the destructor puts all of it back: the handle answers as it did.
struct ExpandUndo {
  DeviceIndex* ix;
  bool armed = false, committed = false;
  int64_t K = 0, KP = 0;
  int code_wide = 0;
  float cmax = 0.f;
  bool filter_ok = false, s6_fast_ok = false;
  DevPtr<float> centroids;   // armed: the table that served (when one was built), else the grown one
  DevPtr<uint8_t> codes;     // armed: the narrow array that served (when the codes widen), else the wide one
  bool has_centroids = false, has_codes = false;
  int64_t Nk = 0, N0 = 0, Tk = 0, T0 = 0;   // the tail: documents [Nk, N0), tokens [Tk, T0)
  DevPtr<uint8_t> t_codes, t_res;
  DevPtr<float> t_inv;
  DevPtr<uint16_t> t_pos;
  DevPtr<int64_t> t_off;
  explicit ExpandUndo(DeviceIndex* i) : ix(i) {}
  int save_tail(int64_t Nk_, int64_t N0_, int64_t Tk_, int64_t T0_) {
    Nk = Nk_, N0 = N0_, Tk = Tk_, T0 = T0_;
    const size_t nt = (size_t)(T0 - Tk), nd = (size_t)(N0 - Nk), cb = ix->code_bytes();
    if (nd == 0) return NP_OK;
    NP_TRY(t_off.alloc(nd));
    NP_HIP(hipMemcpy(t_off.get(), ix->d_doc_offsets.get() + Nk + 1, nd * 8, hipMemcpyDeviceToDevice));
    if (nt == 0) return NP_OK;
    NP_TRY(t_codes.alloc(nt * cb));
    NP_TRY(t_res.alloc(nt * ix->pd));
    NP_TRY(t_inv.alloc(nt));
    if (ix->tok_sorted) NP_TRY(t_pos.alloc(nt));
    NP_HIP(hipMemcpy(t_codes.get(), ix->d_codes.get() + (size_t)Tk * cb, nt * cb, hipMemcpyDeviceToDevice));
    NP_HIP(hipMemcpy(t_res.get(), ix->d_residuals.get() + (size_t)Tk * ix->pd, nt * ix->pd, hipMemcpyDeviceToDevice));
    NP_HIP(hipMemcpy(t_inv.get(), ix->d_inv_norm.get() + Tk, nt * 4, hipMemcpyDeviceToDevice));
    if (ix->tok_sorted) NP_HIP(hipMemcpy(t_pos.get(), ix->d_tok_pos.get() + Tk, nt * 2, hipMemcpyDeviceToDevice));
    return NP_OK;
  }
  void exchange() {   // the handle's arrays <-> the ones held here, with their share of device_bytes
    if (has_centroids) {
      ix->device_bytes = ix->device_bytes - ix->d_centroids.bytes() + centroids.bytes();
      std::swap(ix->d_centroids, centroids);
    }
    if (has_codes) {
      ix->device_bytes = ix->device_bytes - ix->d_codes.bytes() + codes.bytes();
      std::swap(ix->d_codes, codes);
    }
  }
  // the grown geometry goes live for the stages (nobody else looks: every context is held)
  void flip(int64_t K1, float cmax1, bool filter_ok1, bool s6_fast_ok1) {
    K = ix->K, KP = ix->KP, code_wide = ix->code_wide, cmax = ix->cmax, filter_ok = ix->filter_ok, s6_fast_ok = ix->s6_fast_ok;
    exchange();
    ix->K = K1;
    ix->KP = (K1 + 63) / 64 * 64;
    ix->code_wide = K1 > 65536 ? 1 : 0;
    ix->cmax = cmax1, ix->filter_ok = filter_ok1, ix->s6_fast_ok = s6_fast_ok1;
    armed = true;
  }
  void commit() { committed = true; }
  ~ExpandUndo() {
    if (!armed || committed) return;
    (void)hipDeviceSynchronize();
    exchange();
    ix->K = K, ix->KP = KP, ix->code_wide = code_wide, ix->cmax = cmax, ix->filter_ok = filter_ok, ix->s6_fast_ok = s6_fast_ok;
    const size_t nt = (size_t)(T0 - Tk), nd = (size_t)(N0 - Nk), cb = ix->code_bytes();
    if (nd > 0 && t_off.get()) (void)hipMemcpy(ix->d_doc_offsets.get() + Nk + 1, t_off.get(), nd * 8, hipMemcpyDeviceToDevice);
    if (nt > 0 && t_codes.get()) {
      (void)hipMemcpy(ix->d_codes.get() + (size_t)Tk * cb, t_codes.get(), nt * cb, hipMemcpyDeviceToDevice);
      (void)hipMemcpy(ix->d_residuals.get() + (size_t)Tk * ix->pd, t_res.get(), nt * ix->pd, hipMemcpyDeviceToDevice);
      (void)hipMemcpy(ix->d_inv_norm.get() + Tk, t_inv.get(), nt * 4, hipMemcpyDeviceToDevice);
      if (ix->tok_sorted && t_pos.get()) (void)hipMemcpy(ix->d_tok_pos.get() + Tk, t_pos.get(), nt * 2, hipMemcpyDeviceToDevice);
    }
    (void)hipDeviceSynchronize();
  }
};

// the n given documents behind document Nk and token Tk -- outside what any kernel reads until the counts move, or saved by
// ExpandUndo -- and the per-token stages over them alone
static int place_given_documents(const char* entry, DeviceIndex* ix, const int64_t* lens, int64_t n, const int64_t* codes,
                                 const uint8_t* residuals, int64_t Tn, int64_t Nk, int64_t Tk) {
  if (n > 0) {
    std::vector<int64_t> off((size_t)n);
    int64_t t = Tk;
    for (int64_t d = 0; d < n; ++d) off[(size_t)d] = (t += lens[d]);
    NP_HIP(hipMemcpy(ix->d_doc_offsets.get() + Nk + 1, off.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  }
  if (Tn > 0) {
    HostIndex h;
    HostChunk c;
    c.codes = codes;
    c.residuals = residuals;
    c.n_tokens = Tn;
    h.chunks.push_back(c);
    NP_TRY(as_expand_argument(entry, upload_tokens(h, ix, 0, Tn, Tk), "codes"));
    if (ix->tok_sorted) NP_TRY(permute_tokens(ix, 1, Nk, Nk + n));
    NP_TRY(fill_inv_norm(ix, Tk, Tk + Tn));
  }
  return NP_OK;
}

// np_hip_index_append / _append_rows (k_new == 0 and n_replace == 0: nothing is cut, widened or saved, and ExpandUndo has
// nothing to put back) and np_hip_index_expand / _expand_rows, once the arguments are checked.  rows: the rows of the
// n - n_replace NEW documents (the replaced ones keep their ids and their rows), where the plain entry drops the attachments.
static int expand_documents(const char* entry, DeviceIndex* ix, const float* new_centroids, int64_t k_new, int64_t n_replace,
                            const int64_t* lens, int64_t n, const int64_t* codes, const uint8_t* residuals, int64_t Tn, int64_t maxlen,
                            const AppendRows* rows) {
  UpdateSection section(ix);
  NP_TRY(section.begin());
  const int64_t N0 = ix->n_docs, Nk = N0 - n_replace, N1 = Nk + n, K0 = ix->K, K1 = K0 + k_new, T0 = ix->T;
  const bool expands = k_new > 0 || n_replace > 0;   // else an append: its trace keeps its own tag and stage names
  if (n_replace > N0) {   // (checked by the entry; the handle may have shrunk since)
    set_error("%s: n_replace is %lld, the handle has %lld documents", entry, (long long)n_replace, (long long)N0);
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(as_expand_argument(entry, check_shard_docs(N1), "n_docs"));
  NP_TRY(as_expand_argument(entry, check_geometry(K1, ix->ldim, ix->lnbits, N1), "k_new"));
  OpenTrace trace("NP_APPEND_TRACE", expands ? "np expand" : "np append");
  // the tail that goes: its first token, its longest document
  std::vector<int64_t> h_tail((size_t)n_replace + 1, T0);
  if (n_replace > 0) NP_HIP(hipMemcpy(h_tail.data(), ix->d_doc_offsets.get() + Nk, h_tail.size() * 8, hipMemcpyDeviceToHost));
  const int64_t Tk = h_tail[0], T1 = Tk + Tn;
  int64_t kept_max = ix->max_doc_len, tail_max = 0;
  for (int64_t d = 0; d < n_replace; ++d) tail_max = std::max(tail_max, h_tail[(size_t)d + 1] - h_tail[(size_t)d]);
  if (n_replace > 0 && tail_max >= ix->max_doc_len) {   // the longest document may be leaving: the kept ones are looked at
    std::vector<int64_t> off((size_t)Nk + 1);
    NP_HIP(hipMemcpy(off.data(), ix->d_doc_offsets.get(), off.size() * 8, hipMemcpyDeviceToHost));
    kept_max = 0;
    for (int64_t d = 0; d < Nk; ++d) kept_max = std::max(kept_max, off[(size_t)d + 1] - off[(size_t)d]);
  }
  // 1. capacity first: commits nothing
  NP_TRY(grow_capacity(ix, N1, T1));
  const bool with_rows = rows && n > n_replace;
  if (with_rows) NP_TRY(grow_attachments(ix, N1));
  trace.mark("grow");
  // 2. the grown centroid table and its bounds over all K1 rows, the wide codes of the kept tokens: beside what serves
  ExpandUndo undo(ix);
  float cmax1 = ix->cmax;
  bool filter_ok1 = ix->filter_ok, s6_fast_ok1 = ix->s6_fast_ok;
  if (k_new > 0) {
    NP_TRY(undo.centroids.alloc((size_t)K1 * ix->dim));
    undo.has_centroids = true;
    NP_HIP(hipMemcpy(undo.centroids.get(), ix->d_centroids.get(), (size_t)K0 * ix->dim * sizeof(float), hipMemcpyDeviceToDevice));
    NP_TRY(upload_centroid_rows(ix, new_centroids, k_new, undo.centroids.get() + (size_t)K0 * ix->dim));
    NP_TRY(centroid_bounds(undo.centroids.get(), K1, ix->dim, &cmax1, &filter_ok1));
    const int nb = 1 << ix->nbits;
    std::vector<float> wl((size_t)nb);
    NP_HIP(hipMemcpy(wl.data(), ix->d_wlut.get(), (size_t)nb * sizeof(float), hipMemcpyDeviceToHost));
    bool wok = true;
    for (int s = 0; s < nb; ++s) wok = wok && std::isfinite(wl[(size_t)s]) && std::fabs(wl[(size_t)s]) < 1e6f;
    s6_fast_ok1 = filter_ok1 && cmax1 < 1e6f && wok;
    trace.mark("centroids + bounds");
  }
  if (!ix->code_wide && K1 > 65536) {
    NP_TRY(undo.codes.alloc((size_t)std::max<int64_t>(ix->cap_tokens, 1) * 4));
    undo.has_codes = true;
    KernelClock clock(trace.on);
    clock.start();
    widen_codes_kernel<<<(unsigned)std::max<int64_t>(1, std::min<int64_t>(((Tk >> 3) + 255) / 256, 8192)), 256>>>(
        reinterpret_cast<const uint16_t*>(ix->d_codes.get()), Tk, reinterpret_cast<uint32_t*>(undo.codes.get()));
    NP_HIP(hipGetLastError());
    if (trace.on) fprintf(stderr, "[%s] %-28s %8.6f s  %lld codes\n", trace.tag, "widen kernel", clock.stop(), (long long)Tk);
    NP_HIP(hipDeviceSynchronize());
    trace.mark("codes widened");
  }
  // 3. the tail's bytes beside, then the grown geometry goes live for the stages below; from here on a failure restores
  NP_TRY(undo.save_tail(Nk, N0, Tk, T0));
  undo.flip(K1, cmax1, filter_ok1, s6_fast_ok1);
  if (expands) trace.mark("tail saved");
  auto refused_after = [&](int stage) {   // Tuning::expand_fail: a test's stand-in for an allocation the device refuses here
    if (ix->tune.expand_fail != stage) return false;
    set_error("%s: out of memory after stage %d (np_hip_index_tune \"expand_fail\")", entry, stage);
    return true;
  };
  // 4. the given documents from the first dropped token on
  NP_TRY(place_given_documents(entry, ix, lens, n, codes, residuals, Tn, Nk, Tk));
  trace.mark("upload + token stages");
  if (refused_after(1)) return NP_ERR_OUT_OF_MEMORY;
  // 5. the distinct-code structures of the final documents, once: the eighths of the centroid range moved for all of them
  Ucodes u;
  DevPtr<int64_t> d_uoff;
  NP_TRY(as_expand_argument(entry, build_unique_codes(ix, tokens_of(ix), N1, &u, &d_uoff), "n_docs"));
  trace.mark("distinct-code rebuild");
  if (refused_after(2)) return NP_ERR_OUT_OF_MEMORY;
  // 6. the posting lists, one pass
  StagedLists lists;
  NP_TRY(rewrite_posting_lists(ix, K0, u, d_uoff.get(), Nk, N1, maxlen > NP_UNIQ_MAX, &lists, entry, trace));
  d_uoff.reset();
  trace.mark(expands ? "posting-list cut + merge" : "posting-list merge");
  if (refused_after(3)) return NP_ERR_OUT_OF_MEMORY;
  // 7. their range table
  NP_TRY(stage_ivf_split(ix, u, N1, &lists));
  trace.mark("range table");
  if (refused_after(4)) return NP_ERR_OUT_OF_MEMORY;
  // 8. the new documents' rows, staged beside the attachments that serve
  StagedRows staged;
  if (with_rows) {
    NP_TRY(stage_appended_rows(ix, *rows, N0, N1, &staged));
    trace.mark("rows staged");
  }
  // ---- nothing below can fail: the handle becomes the expanded index ----
  undo.commit();
  int rows_rc = NP_OK;
  if (with_rows) rows_rc = install_appended_rows(ix, *rows, std::move(staged), N0, N1);   // (not an allocation: a device that stopped answering)
  else if (!rows) drop_attachments(ix);
  install_ucodes(ix, std::move(u));
  install_lists(ix, std::move(lists));
  // the directory's arithmetic, delete and then append (np_update.cpp delete_impl, update_index_files): tokens / documents
  // after the tail drop, then (avg * n + new_tokens) / n1; a handle made from arrays reports tokens / documents
  const int64_t emb_k = ix->n_emb_total - (T0 - Tk);
  if (n > 0 || n_replace > 0) {
    if (ix->avg_from_counts) {
      ix->avg_doclen = N1 > 0 ? (double)(emb_k + Tn) / (double)N1 : 0.0;
    } else {
      const double a = n_replace > 0 ? (Nk > 0 ? (double)emb_k / (double)Nk : 0.0) : ix->avg_doclen;
      ix->avg_doclen = N1 > 0 ? (a * (double)Nk + (double)Tn) / (double)N1 : 0.0;
    }
  }
  ix->n_docs = ix->N_total = N1;
  ix->T = T1;
  ix->n_emb_total = emb_k + Tn;
  ix->max_doc_len = std::max(kept_max, maxlen);
  finish_update(ix);
  if (expands) trace.mark("swap");
  return rows_rc;
}

// doc lengths -> d_doc_offsets (an inclusive scan written one entry in)
static int synth_doc_offsets(const np_synth_spec* s, const SynthP& p, DeviceIndex* ix) {
  NP_TRY(ix->d_doc_offsets.alloc((size_t)ix->n_docs + 1, &ix->device_bytes));
  NP_HIP(hipMemset(ix->d_doc_offsets.get(), 0, sizeof(int64_t)));
  if (ix->n_docs == 0) return NP_OK;
  DevPtr<int64_t> d_lens;
  DevPtr<int32_t> d_tab;
  DevPtr<uint8_t> d_temp;
  NP_TRY(d_lens.alloc((size_t)ix->n_docs));
  if (s->len_table_size > 0) {
    NP_TRY(d_tab.alloc((size_t)s->len_table_size));
    const hipError_t e = hipMemcpy(d_tab.get(), s->len_table, (size_t)s->len_table_size * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      set_error("synth: length table upload failed: %s", hipGetErrorString(e));
      return NP_ERR_DEVICE_UNAVAILABLE;
    }
  }
  synth_lens_kernel<<<(unsigned)((ix->n_docs + 255) / 256), 256>>>(p, d_tab.get(), s->len_table_size, d_lens.get());
  int64_t* d_incl = ix->d_doc_offsets.get() + 1;
  size_t tb = 0;
  hipError_t e = hipcub::DeviceScan::InclusiveSum(nullptr, tb, d_lens.get(), d_incl, (int)ix->n_docs);
  if (e == hipSuccess) NP_TRY(d_temp.alloc(std::max<size_t>(tb, 16)));
  if (e == hipSuccess) e = hipcub::DeviceScan::InclusiveSum(d_temp.get(), tb, d_lens.get(), d_incl, (int)ix->n_docs);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    set_error("synth: doc offset scan failed: %s", hipGetErrorString(e));
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  return NP_OK;
}

static int synth_build(const np_synth_spec* s, const np_open_opts* opts_in, DeviceIndex** out) {
  *out = nullptr;
  np_open_opts o;
  NP_TRY(normalise_opts(opts_in, &o));
  NP_TRY(check_device(o.device));
  if (!s || !s->centroids || !s->bucket_weights) {
    set_error("Invalid configuration: synth spec needs centroids and bucket_weights");
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(check_geometry(s->num_centroids, s->dim, s->nbits, s->num_docs));
  if (s->doc_len_min < 0 || s->doc_len_max < s->doc_len_min || s->doc_len_max > NP_UNIQ_MAX || s->n_topics <= 0 ||
      s->dim * s->nbits / 8 > 128 || s->len_table_size < 0 || (s->len_table_size > 0 && !s->len_table)) {
    set_error("Invalid configuration: synth doc_len/n_topics/packed width out of range");
    return NP_ERR_INVALID_ARGUMENT;
  }
  int32_t table_max = 0;
  for (int i = 0; i < s->len_table_size; ++i) {
    if (s->len_table[i] < 0 || s->len_table[i] > NP_UNIQ_MAX) {
      set_error("Invalid configuration: synth len_table entry %d out of range", s->len_table[i]);
      return NP_ERR_INVALID_ARGUMENT;
    }
    table_max = std::max(table_max, s->len_table[i]);
  }
  DeviceGuard g(o.device);
  IndexHandle ix;
  NP_TRY(start_index(g, o, s->num_docs, &ix));
  if (ix->n_docs >= ((int64_t)1 << 31)) {
    set_error("synth: a shard holds < 2^31 documents (got %lld); use more shards", (long long)ix->n_docs);
    return NP_ERR_INVALID_ARGUMENT;
  }
  ix->max_doc_len = s->len_table_size > 0 ? table_max : s->doc_len_max;
  OpenTrace trace;
  // the generator writes storage geometry directly (spec checked above)
  NP_TRY(set_geometry(ix.get(), s->num_centroids, s->dim, s->nbits, true, s->centroids, s->bucket_weights));
  trace.mark("codec");

  SynthP p;
  p.b_len = mix64(s->seed + S_LEN);
  p.b_topic = mix64(s->seed + S_TOPIC);
  p.b_tok = mix64(s->seed + S_TOK);
  p.b_res = mix64(s->seed + S_RES);
  p.doc_begin = ix->doc_begin;
  p.n_docs = ix->n_docs;
  p.K = (uint32_t)ix->K;
  p.len_min = s->doc_len_min;
  p.len_span = s->doc_len_max - s->doc_len_min + 1;
  p.n_topics = s->n_topics;
  p.rand256 = s->rand256;
  p.pd = ix->pd;
  p.nw = (ix->pd + 7) / 8;
  NP_TRY(synth_doc_offsets(s, p, ix.get()));
  NP_HIP(hipMemcpy(&ix->T, ix->d_doc_offsets.get() + ix->n_docs, sizeof(int64_t), hipMemcpyDeviceToHost));
  if (ix->T >= ((int64_t)1 << 40)) {   // candidate records carry a 40-bit token offset
    set_error("synth: shard holds %lld tokens; a shard addresses < 2^40 tokens (use more shards)", (long long)ix->T);
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(alloc_tokens(ix.get()));
  if (ix->n_docs > 0)
    synth_tokens_kernel<<<(unsigned)((ix->n_docs + 3) / 4), 256>>>(p, ix->d_doc_offsets.get(), ix->d_codes.get(), ix->code_wide,
                                                                   ix->d_residuals.get());
  NP_HIP(hipGetLastError());
  NP_HIP(hipDeviceSynchronize());
  trace.mark("generated tokens");

  // whole-corpus token count: exact when unsharded or fixed-length, else extrapolated
  const bool fixed_len = s->len_table_size == 0 && s->doc_len_min == s->doc_len_max;
  if (o.shard_count == 1 || fixed_len)
    ix->n_emb_total = fixed_len ? s->num_docs * (int64_t)s->doc_len_min : ix->T;
  else
    ix->n_emb_total = ix->n_docs > 0 ? (int64_t)((double)ix->T / (double)ix->n_docs * (double)s->num_docs) : 0;
  ix->avg_doclen = s->num_docs > 0 ? (double)ix->n_emb_total / (double)s->num_docs : 0.0;
  NP_TRY(build_derived(ix.get(), true, trace));
  *out = ix.release();
  return NP_OK;
}

}  // namespace np

using namespace np;

// =================================== C ABI ====================================================
extern "C" {

int np_hip_abi_version(void) { return NP_ABI_VERSION; }

int64_t np_hip_struct_size(int32_t which) {
  switch (which) {
    case 0: return (int64_t)sizeof(np_info);
    case 1: return (int64_t)sizeof(np_stats);
    case 2: return (int64_t)sizeof(np_search_params);
    case 3: return (int64_t)sizeof(np_open_opts);
    case 4: return (int64_t)sizeof(np_kmeans_opts);
    case 5: return (int64_t)sizeof(np_kmeans_report);
    case 6: return (int64_t)sizeof(np_index_config);
    case 7: return (int64_t)sizeof(np_kmeans_plan);
    case 8: return (int64_t)sizeof(np_update_config);
    case 9: return (int64_t)sizeof(np_update_report);
    case 10: return (int64_t)sizeof(np_pool_opts);
    case 11: return (int64_t)sizeof(np_pool_report);
    case 12: return (int64_t)sizeof(np_text_expr);
    default: return -1;
  }
}

int np_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  int usable = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ++usable;
  }
  return usable;
}

const char* np_hip_last_error(void) { return np::last_error(); }

int np_hip_index_open(const char* index_dir, const np_open_opts* opts, np_index** out) {
  clear_error();
  if (!out) {
    set_error("np_hip_index_open: out is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  *out = nullptr;
  HostIndex h;
  OpenTrace trace;
  NP_TRY(load_index_dir(index_dir, &h));
  trace.mark("parse + map the directory");
  DeviceIndex* ix = nullptr;
  NP_TRY(build_device_index(h, opts, &ix));
  *out = static_cast<np_index*>(ix);
  return NP_OK;
}

int np_hip_index_from_arrays(const np_index_arrays* a, const np_open_opts* opts, np_index** out) {
  clear_error();
  if (!out || !a) {
    set_error("np_hip_index_from_arrays: NULL argument");
    return NP_ERR_INVALID_ARGUMENT;
  }
  *out = nullptr;
  if (!a->centroids || !a->ivf_lengths || (a->num_docs > 0 && !a->doc_lengths)) {
    set_error("np_hip_index_from_arrays: centroids / ivf_lengths / doc_lengths are required");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (!a->bucket_weights) {  // codec.rs:428-431
    set_error("Codec error: bucket_weights required for decompression");
    return NP_ERR_CODEC;
  }
  HostIndex h;
  h.num_documents_total = a->num_documents_total;
  h.doc_begin = a->doc_begin;
  h.K = a->num_centroids;
  h.dim = a->dim;
  h.nbits = a->nbits;
  h.centroids = a->centroids;
  h.bucket_weights = a->bucket_weights;
  h.ivf = a->ivf;
  h.ivf_lengths = a->ivf_lengths;
  h.ivf_size = 0;
  for (int64_t c = 0; c < a->num_centroids; ++c) h.ivf_size += a->ivf_lengths[c];
  h.doc_lengths.assign(a->doc_lengths, a->doc_lengths + a->num_docs);
  HostChunk c;
  c.codes = a->codes;
  c.residuals = a->residuals;
  c.n_tokens = 0;
  for (int64_t d = 0; d < a->num_docs; ++d) c.n_tokens += a->doc_lengths[d];
  if (c.n_tokens > 0 && (!a->codes || !a->residuals)) {
    set_error("np_hip_index_from_arrays: codes / residuals are required");
    return NP_ERR_INVALID_ARGUMENT;
  }
  h.chunks.push_back(c);
  h.num_embeddings_total = c.n_tokens;
  h.avg_doclen = a->num_docs > 0 ? (double)c.n_tokens / (double)a->num_docs : 0.0;
  DeviceIndex* ix = nullptr;
  NP_TRY(build_device_index(h, opts, &ix));
  ix->avg_from_counts = true;
  *out = static_cast<np_index*>(ix);
  return NP_OK;
}

int np_hip_index_synth(const np_synth_spec* spec, const np_open_opts* opts, np_index** out) {
  clear_error();
  if (!out) {
    set_error("np_hip_index_synth: out is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  DeviceIndex* ix = nullptr;
  NP_TRY(synth_build(spec, opts, &ix));
  ix->avg_from_counts = true;
  *out = static_cast<np_index*>(ix);
  return NP_OK;
}

int64_t np_hip_index_ivf_size(const np_index* index) { return index ? index->ivf_size : 0; }

int np_hip_index_tune(np_index* ix, const char* name, int32_t value) {
  clear_error();
  if (!ix || !name) {
    set_error("np_hip_index_tune: NULL argument");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (!set_tuning(&ix->tune, name, value)) {
    set_error("np_hip_index_tune: unknown knob '%s'", name);
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

int np_hip_index_export(const np_index* ix, int64_t* doc_lengths, int64_t* codes, uint8_t* residuals, int64_t* ivf,
                        int32_t* ivf_lengths) {
  clear_error();
  if (!ix) {
    set_error("np_hip_index_export: NULL index");
    return NP_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g(ix->device);
  if (doc_lengths) {
    std::vector<int64_t> off((size_t)ix->n_docs + 1);
    NP_HIP(hipMemcpy(off.data(), ix->d_doc_offsets.get(), off.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t d = 0; d < ix->n_docs; ++d) doc_lengths[d] = off[d + 1] - off[d];
  }
  // codes / residuals are kept in per-document code order (np_internal.h): put the on-disk order back for the copy
  // (not concurrent with searches on this handle: export is a test / bench utility)
  struct Resort {
    const np_index* ix;
    bool active;
    ~Resort() {
      if (active) (void)permute_tokens(ix, 1, 0, ix->n_docs);
    }
  } resort{ix, false};
  if ((codes || residuals) && ix->tok_sorted && ix->T > 0) {
    NP_TRY(permute_tokens(ix, 0, 0, ix->n_docs));
    resort.active = true;
  }
  if (codes && ix->T > 0) {
    const int64_t PIECE = (int64_t)8 << 20;
    std::vector<uint32_t> tmp((size_t)std::min(PIECE, ix->T));
    for (int64_t s = 0; s < ix->T; s += PIECE) {
      int64_t n = std::min(PIECE, ix->T - s);
      if (ix->code_wide) {
        NP_HIP(hipMemcpy(tmp.data(), (const uint32_t*)ix->d_codes.get() + s, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) codes[s + i] = (int64_t)tmp[i];
      } else {
        uint16_t* t16 = reinterpret_cast<uint16_t*>(tmp.data());
        NP_HIP(hipMemcpy(t16, (const uint16_t*)ix->d_codes.get() + s, (size_t)n * 2, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) codes[s + i] = (int64_t)t16[i];
      }
    }
  }
  if (residuals && ix->T > 0 && ix->pd == ix->lpd) {
    NP_HIP(hipMemcpy(residuals, ix->d_residuals.get(), (size_t)ix->T * ix->pd, hipMemcpyDeviceToHost));
  } else if (residuals && ix->T > 0) {   // storage rows -> file rows
    DevPtr<uint8_t> d_rows;
    NP_TRY(d_rows.alloc((size_t)ix->T * ix->lpd));
    unpack_rows_kernel<<<(unsigned)((ix->T * ix->lpd + 255) / 256), 256>>>(ix->d_residuals.get(), ix->T, ix->lpd, ix->pd,
                                                                          ix->lnbits != ix->nbits, d_rows.get());
    NP_HIP(hipMemcpy(residuals, d_rows.get(), (size_t)ix->T * ix->lpd, hipMemcpyDeviceToHost));
  }
  if (ivf && ix->ivf_size > 0) {
    std::vector<uint32_t> tmp((size_t)ix->ivf_size);
    NP_HIP(hipMemcpy(tmp.data(), ix->d_ivf.get(), tmp.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < ix->ivf_size; ++i) ivf[i] = (int64_t)tmp[i] + ix->doc_begin;
  }
  if (ivf_lengths) {
    std::vector<int64_t> off((size_t)ix->K + 1);
    NP_HIP(hipMemcpy(off.data(), ix->d_ivf_offsets.get(), off.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < ix->K; ++c) ivf_lengths[c] = (int32_t)(off[c + 1] - off[c]);
  }
  return NP_OK;
}

int np_hip_index_set_columns(np_index* ix, const np_column* cols, int32_t n_cols) {
  clear_error();
  if (!ix || n_cols < 0 || n_cols > NP_MAX_COLUMNS || (n_cols > 0 && !cols)) {
    set_error("set_columns: %s", !ix ? "NULL index" : !cols && n_cols > 0 ? "NULL columns" : "n_cols must be in 0..64");
    return NP_ERR_INVALID_ARGUMENT;
  }
  for (int32_t c = 0; c < n_cols; ++c) {
    if (cols[c].type != NP_COL_I64 && cols[c].type != NP_COL_F64 && cols[c].type != NP_COL_CODE) {
      set_error("set_columns: column %d has unknown type %d", c, cols[c].type);
      return NP_ERR_INVALID_ARGUMENT;
    }
    if (!cols[c].data) {
      set_error("set_columns: column %d has NULL data", c);
      return NP_ERR_INVALID_ARGUMENT;
    }
  }
  DeviceGuard g(ix->device);
  // the new set is built beside the old one and swapped in whole: a failed allocation leaves the handle as it was
  std::vector<DeviceColumn> fresh((size_t)n_cols);
  std::vector<FilterCol> tab((size_t)n_cols);
  DevPtr<FilterCol> d_tab;
  size_t bytes = 0;
  const int64_t b = ix->doc_begin, n = ix->n_docs, nvw = (n + 31) / 32;
  std::vector<uint32_t> bits;
  for (int32_t c = 0; c < n_cols; ++c) {
    DeviceColumn& dc = fresh[c];
    dc.type = cols[c].type;
    const size_t esz = dc.type == NP_COL_CODE ? 4 : 8;
    NP_TRY(dc.data.alloc((size_t)n * esz, &bytes));
    if (n > 0) NP_HIP(hipMemcpy(dc.data.get(), (const char*)cols[c].data + (size_t)b * esz, (size_t)n * esz, hipMemcpyHostToDevice));
    if (dc.type == NP_COL_CODE)
      for (int64_t d = 0; d < n; ++d) {
        const int32_t code = ((const int32_t*)cols[c].data)[b + d];
        dc.min_code = std::min(dc.min_code, code);
        dc.max_code = std::max(dc.max_code, code);
      }
    // validity: the caller's bytes, and an f64 NaN is NULL whatever they say; no array at all where nothing is NULL
    bits.assign((size_t)nvw, 0u);
    bool any_null = false;
    const double* f64 = dc.type == NP_COL_F64 ? (const double*)cols[c].data + b : nullptr;
    const uint8_t* valid = cols[c].valid ? cols[c].valid + b : nullptr;
    for (int64_t d = 0; d < n; ++d) {
      const bool ok = (!valid || valid[d] != 0) && (!f64 || f64[d] == f64[d]);
      if (ok) bits[d >> 5] |= 1u << (d & 31); else any_null = true;
    }
    dc.has_valid = any_null;
    if (any_null) {
      NP_TRY(dc.valid.alloc((size_t)nvw, &bytes));
      NP_HIP(hipMemcpy(dc.valid.get(), bits.data(), (size_t)nvw * 4, hipMemcpyHostToDevice));
    }
    tab[c] = FilterCol{dc.data.get(), any_null ? dc.valid.get() : nullptr, dc.type, 0};
  }
  if (n_cols > 0) {
    NP_TRY(d_tab.alloc((size_t)n_cols, &bytes));
    NP_HIP(hipMemcpy(d_tab.get(), tab.data(), (size_t)n_cols * sizeof(FilterCol), hipMemcpyHostToDevice));
  }
  ix->columns = std::move(fresh);
  ix->d_coltab = std::move(d_tab);
  ix->device_bytes = ix->device_bytes - ix->column_bytes - ix->coltext_bytes + bytes;   // the old columns' text goes with them
  ix->column_bytes = bytes;
  ix->coltext_bytes = 0;
  return NP_OK;
}

void np_hip_index_close(np_index* index) {
  destroy_device_index(index);
}

int np_hip_index_info(const np_index* ix, np_info* out) {
  clear_error();
  if (!ix || !out) {
    set_error("np_hip_index_info: NULL argument");
    return NP_ERR_INVALID_ARGUMENT;
  }
  memset(out, 0, sizeof *out);
  out->num_documents = ix->N_total;
  out->num_embeddings = ix->n_emb_total;
  out->num_partitions = ix->K;
  out->embedding_dim = ix->ldim;
  out->nbits = ix->lnbits;
  out->avg_doclen = ix->avg_doclen;
  out->shard_doc_begin = ix->doc_begin;
  out->shard_doc_end = ix->doc_begin + ix->n_docs;
  out->shard_embeddings = ix->T;
  out->device_bytes = (int64_t)ix->device_bytes;
  out->device = ix->device;
  out->abi_version = NP_ABI_VERSION;
  out->workspace_bytes = ix->ws_budget.load(std::memory_order_relaxed);
  return NP_OK;
}

// Host-only: parse and validate an index directory exactly like np_hip_index_open does (MmapIndex::load,
// index.rs:1026-1139; file formats mmap.rs:659-749) without touching a device.  Lets a service (or a CPU test)
// check an index before it claims a GPU.  out->device = -1, no shard fields.
int np_hip_index_probe_dir(const char* index_dir, np_info* out) {
  clear_error();
  if (!out) {
    set_error("np_hip_index_probe_dir: NULL argument");
    return NP_ERR_INVALID_ARGUMENT;
  }
  HostIndex h;
  NP_TRY(load_index_dir(index_dir, &h));
  NP_TRY(check_geometry(h.K, h.dim, h.nbits, h.num_documents_total));
  // every code must name a centroid and every posting a document (the same checks build_device_index makes)
  for (const HostChunk& c : h.chunks)
    for (int64_t t = 0; t < c.n_tokens; ++t)
      if (c.codes[t] < 0 || c.codes[t] >= h.K) {
        set_error("Index load failed: code %lld is outside [0, %lld)", (long long)c.codes[t], (long long)h.K);
        return NP_ERR_INDEX_LOAD;
      }
  int64_t ivf_sum = 0;
  for (int64_t i = 0; i < h.K; ++i) ivf_sum += h.ivf_lengths[i];
  for (int64_t i = 0; i < ivf_sum; ++i)
    if (h.ivf[i] < 0 || h.ivf[i] >= h.num_documents_total) {
      set_error("Index load failed: ivf entry %lld is outside [0, %lld)", (long long)h.ivf[i],
                (long long)h.num_documents_total);
      return NP_ERR_INDEX_LOAD;
    }
  memset(out, 0, sizeof *out);
  int64_t tokens = 0;
  for (const HostChunk& c : h.chunks) tokens += c.n_tokens;
  out->num_documents = h.num_documents_total;
  out->num_embeddings = h.num_embeddings_total;
  out->num_partitions = h.K;
  out->embedding_dim = h.dim;
  out->nbits = h.nbits;
  out->avg_doclen = h.avg_doclen;
  out->shard_doc_begin = 0;
  out->shard_doc_end = h.num_documents_total;
  out->shard_embeddings = tokens;
  out->device_bytes = 0;
  out->device = -1;
  out->abi_version = NP_ABI_VERSION;
  return NP_OK;
}

// the new documents' rows against the handle's attachments: refused by name, before any allocation
static int check_append_rows(const DeviceIndex* ix, const AppendRows& r, int64_t n_docs, const char* e) {
  const size_t nc = ix->columns.size();
  if (r.n_cols < 0 || (size_t)r.n_cols != nc) {
    set_error("%s: n_cols is %d, the handle has %zu columns", e, r.n_cols, nc);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (nc > 0 && n_docs > 0 && !r.cols) {
    set_error("%s: new_cols is NULL, the handle has %zu columns", e, nc);
    return NP_ERR_INVALID_ARGUMENT;
  }
  for (size_t c = 0; c < nc && r.cols; ++c) {
    const DeviceColumn& col = ix->columns[c];
    if (r.cols[c].type != col.type) {
      set_error("%s: new_cols[%zu] has type %d, column %zu of the handle type %d", e, c, r.cols[c].type, c, col.type);
      return NP_ERR_INVALID_ARGUMENT;
    }
    if (n_docs > 0 && !r.cols[c].data) {
      set_error("%s: new_cols[%zu] has NULL data", e, c);
      return NP_ERR_INVALID_ARGUMENT;
    }
  }
  for (size_t c = 0; c < nc && r.remap; ++c) {
    if (!r.remap[c]) continue;
    const DeviceColumn& col = ix->columns[c];
    if (col.type != NP_COL_CODE) {
      set_error("%s: code_remap[%zu] is given, column %zu is no CODE column", e, c, c);
      return NP_ERR_INVALID_ARGUMENT;
    }
    if (col.min_code < 0) {
      set_error("%s: code_remap[%zu]: column %zu holds the negative code %d, which no table maps", e, c, c, col.min_code);
      return NP_ERR_INVALID_ARGUMENT;
    }
    const int64_t bad = attach_remap_check(r.remap[c], (int64_t)col.max_code + 1);
    if (bad >= 0) {
      set_error("%s: code_remap[%zu][%lld] = %d: a remap is not negative and strictly increasing (the dictionary stays sorted)", e, c,
                (long long)bad, r.remap[c][bad]);
      return NP_ERR_INVALID_ARGUMENT;
    }
  }
  if (ix->n_groups > 0) {
    if (n_docs > 0 && !r.groups) {
      set_error("%s: new_groups is NULL, the handle has groups", e);
      return NP_ERR_INVALID_ARGUMENT;
    }
    if (r.n_groups < ix->n_groups || r.n_groups > (int64_t)0x7FFFFFFF) {
      set_error("%s: n_groups is %lld, the handle has %lld groups (and at most 2^31-1 fit)", e, (long long)r.n_groups, (long long)ix->n_groups);
      return NP_ERR_INVALID_ARGUMENT;
    }
    for (int64_t d = 0; d < n_docs; ++d)
      if (r.groups[d] < 0 || (int64_t)r.groups[d] >= r.n_groups) {
        set_error("%s: new_groups[%lld] = %d is outside [0, %lld)", e, (long long)d, r.groups[d], (long long)r.n_groups);
        return NP_ERR_INVALID_ARGUMENT;
      }
  } else if (r.groups) {
    set_error("%s: new_groups is given, the handle has no groups (np_hip_index_set_groups)", e);
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

// np_hip_index_append and np_hip_index_append_rows: the same checks under the entry's own name
static int append_entry(const char* entry, np_index* ix, const int64_t* doc_lengths, int64_t n_docs, const int64_t* codes,
                        const uint8_t* residuals, const AppendRows* rows) {
  clear_error();
  if (!ix) {
    set_error("%s: index is NULL", entry);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (ix->opts.shard_count > 1) {
    set_error("%s: index is a shard (%d of %d): a sharded index is reloaded", entry, ix->opts.shard_rank, ix->opts.shard_count);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (!ix->ivf_sorted) {
    set_error("%s: index has posting lists that do not ascend: only such lists grow at their end", entry);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (n_docs < 0 || (n_docs > 0 && !doc_lengths)) {
    set_error("%s: %s", entry, n_docs < 0 ? "n_docs is negative" : "doc_lengths is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (rows) NP_TRY(check_append_rows(ix, *rows, n_docs, entry));
  if (n_docs == 0) return NP_OK;
  int64_t Tn = 0, maxlen = 0;
  for (int64_t d = 0; d < n_docs; ++d) {
    if (doc_lengths[d] < 0) {
      set_error("%s: doc_lengths[%lld] is negative (%lld)", entry, (long long)d, (long long)doc_lengths[d]);
      return NP_ERR_SHAPE;
    }
    Tn += doc_lengths[d];
    maxlen = std::max(maxlen, doc_lengths[d]);
  }
  if (Tn > 0 && (!codes || !residuals)) {
    set_error("%s: %s is NULL", entry, !codes ? "codes" : "residuals");
    return NP_ERR_INVALID_ARGUMENT;
  }
  for (int64_t t = 0; t < Tn; ++t)
    if (codes[t] < 0 || codes[t] >= ix->K) {
      set_error("%s: codes[%lld] = %lld is outside [0, %lld)", entry, (long long)t, (long long)codes[t], (long long)ix->K);
      return NP_ERR_INVALID_ARGUMENT;
    }
  return expand_documents(entry, ix, nullptr, 0, 0, doc_lengths, n_docs, codes, residuals, Tn, maxlen, rows);
}

int np_hip_index_append(np_index* ix, const int64_t* doc_lengths, int64_t n_docs, const int64_t* codes, const uint8_t* residuals) {
  return append_entry("np_hip_index_append", ix, doc_lengths, n_docs, codes, residuals, nullptr);
}

int np_hip_index_append_rows(np_index* ix, const int64_t* doc_lengths, int64_t n_docs, const int64_t* codes, const uint8_t* residuals,
                             const np_column* new_cols, int32_t n_cols, const int32_t* const* code_remap, const int32_t* new_groups,
                             int64_t n_groups) {
  const AppendRows rows{new_cols, n_cols, code_remap, new_groups, n_groups};
  return append_entry("np_hip_index_append_rows", ix, doc_lengths, n_docs, codes, residuals, &rows);
}

// np_hip_index_expand and np_hip_index_expand_rows: the same checks under the entry's own name, all before any allocation
static int expand_entry(const char* entry, np_index* ix, const float* new_centroids, int64_t k_new, int64_t n_replace,
                        const int64_t* doc_lengths, int64_t n_docs, const int64_t* codes, const uint8_t* residuals, const AppendRows* rows) {
  clear_error();
  if (!ix) {
    set_error("%s: index is NULL", entry);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (ix->opts.shard_count > 1) {
    set_error("%s: index is a shard (%d of %d): a sharded index is reloaded", entry, ix->opts.shard_rank, ix->opts.shard_count);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (!ix->ivf_sorted) {
    set_error("%s: index has posting lists that do not ascend: only such lists are cut and grown at their end", entry);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (k_new < 0 || (k_new > 0 && !new_centroids)) {
    set_error("%s: %s", entry, k_new < 0 ? "k_new is negative" : "new_centroids is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (n_docs < 0 || (n_docs > 0 && !doc_lengths)) {
    set_error("%s: %s", entry, n_docs < 0 ? "n_docs is negative" : "doc_lengths is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (n_replace < 0 || n_replace > n_docs || n_replace > ix->n_docs) {
    set_error("%s: n_replace is %lld: it lies in [0, n_docs = %lld] and within the handle's %lld documents", entry, (long long)n_replace,
              (long long)n_docs, (long long)ix->n_docs);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (k_new == 0 && n_replace == 0) return append_entry(entry, ix, doc_lengths, n_docs, codes, residuals, rows);
  const int64_t K1 = ix->K + k_new, N1 = ix->n_docs - n_replace + n_docs;
  if (k_new >= ((int64_t)1 << 31) || K1 >= ((int64_t)1 << 31)) {   // check_geometry's limit on K
    set_error("%s: k_new: %lld centroids and the handle's %lld exceed the 32-bit device id space", entry, (long long)k_new, (long long)ix->K);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (check_shard_docs(N1) != NP_OK || N1 >= ((int64_t)1 << 32) - 1) {
    set_error("%s: n_docs: a shard holds < 2^31 documents (would be %lld)", entry, (long long)N1);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (rows) NP_TRY(check_append_rows(ix, *rows, n_docs - n_replace, entry));
  int64_t Tn = 0, maxlen = 0;
  for (int64_t d = 0; d < n_docs; ++d) {
    if (doc_lengths[d] < 0) {
      set_error("%s: doc_lengths[%lld] is negative (%lld)", entry, (long long)d, (long long)doc_lengths[d]);
      return NP_ERR_SHAPE;
    }
    Tn += doc_lengths[d];
    maxlen = std::max(maxlen, doc_lengths[d]);
  }
  if (Tn > 0 && (!codes || !residuals)) {
    set_error("%s: %s is NULL", entry, !codes ? "codes" : "residuals");
    return NP_ERR_INVALID_ARGUMENT;
  }
  for (int64_t t = 0; t < Tn; ++t)
    if (codes[t] < 0 || codes[t] >= K1) {
      set_error("%s: codes[%lld] = %lld is outside [0, %lld)", entry, (long long)t, (long long)codes[t], (long long)K1);
      return NP_ERR_INVALID_ARGUMENT;
    }
  return expand_documents(entry, ix, new_centroids, k_new, n_replace, doc_lengths, n_docs, codes, residuals, Tn, maxlen, rows);
}

int np_hip_index_expand(np_index* ix, const float* new_centroids, int64_t k_new, int64_t n_replace, const int64_t* doc_lengths,
                        int64_t n_docs, const int64_t* codes, const uint8_t* residuals) {
  return expand_entry("np_hip_index_expand", ix, new_centroids, k_new, n_replace, doc_lengths, n_docs, codes, residuals, nullptr);
}

int np_hip_index_expand_rows(np_index* ix, const float* new_centroids, int64_t k_new, int64_t n_replace, const int64_t* doc_lengths,
                             int64_t n_docs, const int64_t* codes, const uint8_t* residuals, const np_column* new_cols, int32_t n_cols,
                             const int32_t* const* code_remap, const int32_t* new_groups, int64_t n_groups) {
  const AppendRows rows{new_cols, n_cols, code_remap, new_groups, n_groups};
  return expand_entry("np_hip_index_expand_rows", ix, new_centroids, k_new, n_replace, doc_lengths, n_docs, codes, residuals, &rows);
}

// np_hip_index_remove and np_hip_index_remove_keep: the same checks under the entry's own name
static int remove_entry(const char* entry, np_index* ix, const int64_t* doc_ids, int64_t n_ids, int64_t* out_removed, bool keep) {
  clear_error();
  if (!ix) {
    set_error("%s: index is NULL", entry);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (n_ids < 0 || (n_ids > 0 && !doc_ids)) {
    set_error("%s: %s", entry, n_ids < 0 ? "n_ids is negative" : "doc_ids is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (ix->opts.shard_count > 1) {
    set_error("%s: index is a shard (%d of %d): a sharded index is reloaded", entry, ix->opts.shard_rank, ix->opts.shard_count);
    return NP_ERR_INVALID_ARGUMENT;
  }
  const std::vector<int64_t> removed = remove_ids_in_range(doc_ids, n_ids, ix->n_docs);
  if (!removed.empty()) NP_TRY(remove_documents(ix, removed, keep, entry));   // none in range: nothing changes, the attachments stay
  if (out_removed) *out_removed = (int64_t)removed.size();
  return NP_OK;
}

int np_hip_index_remove(np_index* ix, const int64_t* doc_ids, int64_t n_ids, int64_t* out_removed) {
  return remove_entry("np_hip_index_remove", ix, doc_ids, n_ids, out_removed, false);
}

int np_hip_index_remove_keep(np_index* ix, const int64_t* doc_ids, int64_t n_ids, int64_t* out_removed) {
  return remove_entry("np_hip_index_remove_keep", ix, doc_ids, n_ids, out_removed, true);
}

int np_hip_index_get_column(const np_index* ix, int32_t column, void* data, uint8_t* valid, int32_t* type, int32_t* has_valid) {
  clear_error();
  IndexRead reading(ix);   // an append or a remove waits for this call and holds later ones back (np_internal.h)
  if (!ix) {
    set_error("np_hip_index_get_column: index is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (column < 0 || (size_t)column >= ix->columns.size()) {
    set_error("np_hip_index_get_column: column %d is outside the handle's %zu columns", column, ix->columns.size());
    return NP_ERR_INVALID_ARGUMENT;
  }
  const DeviceColumn& col = ix->columns[(size_t)column];
  if (type) *type = col.type;
  if (has_valid) *has_valid = col.has_valid ? 1 : 0;
  const int64_t n = ix->n_docs;
  if (n == 0 || (!data && !valid)) return NP_OK;
  DeviceGuard g(ix->device);
  if (!g.ok) {
    set_error("hipSetDevice(%d) failed", ix->device);
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  if (data) NP_HIP(hipMemcpy(data, col.data.get(), (size_t)n * (col.type == NP_COL_CODE ? 4 : 8), hipMemcpyDeviceToHost));
  if (valid && !col.has_valid) memset(valid, 1, (size_t)n);
  if (valid && col.has_valid) {
    std::vector<uint32_t> bits((size_t)((n + 31) / 32));
    NP_HIP(hipMemcpy(bits.data(), col.valid.get(), bits.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t d = 0; d < n; ++d) valid[d] = (uint8_t)((bits[(size_t)(d >> 5)] >> (d & 31)) & 1u);
  }
  return NP_OK;
}

int np_hip_index_get_groups(const np_index* ix, int32_t* out) {
  clear_error();
  IndexRead reading(ix);
  if (!ix) {
    set_error("np_hip_index_get_groups: index is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (ix->n_groups <= 0) {
    set_error("np_hip_index_get_groups: the handle has no groups (np_hip_index_set_groups)");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (!out) {
    set_error("np_hip_index_get_groups: out is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g(ix->device);
  if (!g.ok) {
    set_error("hipSetDevice(%d) failed", ix->device);
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  NP_HIP(hipMemcpy(out, ix->d_groups.get(), (size_t)ix->n_docs * 4, hipMemcpyDeviceToHost));
  return NP_OK;
}

int np_hip_index_reserve(np_index* ix, int64_t extra_docs, int64_t extra_tokens) {
  clear_error();
  if (!ix || extra_docs < 0 || extra_tokens < 0) {
    set_error("np_hip_index_reserve: %s", !ix ? "index is NULL" : extra_docs < 0 ? "extra_docs is negative" : "extra_tokens is negative");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (ix->opts.shard_count > 1) {
    set_error("np_hip_index_reserve: index is a shard (%d of %d)", ix->opts.shard_rank, ix->opts.shard_count);
    return NP_ERR_INVALID_ARGUMENT;
  }
  HoldContexts hold(ix);
  DeviceGuard g(ix->device);
  if (!g.ok) {
    set_error("hipSetDevice(%d) failed", ix->device);
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  if (check_shard_docs(ix->n_docs + extra_docs) != NP_OK) {
    set_error("np_hip_index_reserve: extra_docs: a shard holds < 2^31 documents");
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_HIP(hipDeviceSynchronize());
  NP_TRY(grow_capacity(ix, ix->n_docs + extra_docs, ix->T + extra_tokens));
  return grow_attachments(ix, ix->cap_docs);   // the columns' and the groups' arrays follow d_doc_offsets
}

int np_hip_index_capacity(const np_index* ix, int64_t* docs, int64_t* tokens) {
  clear_error();
  if (!ix) {
    set_error("np_hip_index_capacity: index is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (docs) *docs = ix->cap_docs;
  if (tokens) *tokens = ix->cap_tokens;
  return NP_OK;
}

}  // extern "C"
