// np_scan.hip -- np_hip_search_exact: exhaustive exact MaxSim over every document of the handle (or of per-query subsets).
//
// S6 (np_kernels.h) is organised per (query, selected document): every query decompresses its documents for itself.  Here
// the same arithmetic (np_exact.h: one definition of the decompression, the row scales and the masked maxima) is organised
// BY DOCUMENT: a workgroup stages the 32-token tiles of a GROUP of queries in LDS once, a wave walks its documents in
// 32-token tiles, unpacks / gathers / normalises each tile once and multiplies it against every tile of the group.
//   grid          (document blocks, query groups); a wave takes NP_SCAN_DPW consecutive documents of a block
//   keys          [query][document of the pass] u64 = okey(score) << 32 | (0xFFFFFFFF - global id); 0 = out of scope
//   scan_topk     per query: the top_k largest keys of the pass and of the passes before it (radix select + bitonic sort in LDS)
// A (query, document) score depends on nothing but that query and that document -- one tile of one query per MFMA, the
// query's own token order in the sum -- so results do not depend on the batch, the grouping, the slices or the passes.
#include "np_internal.h"
#include "np_exact.h"
#include "np_scan_plan.h"

#include <string.h>

namespace np {

#define NP_SCAN_DPW 8   // documents per wave and block step

struct ScanP {
  const float* Qf;          // [groups][DIM][TW] f32, k-major (precision 0)
  const __bf16* Qb;         // [groups][TW][DIM] bf16 (precision 3)
  const int32_t* tile_info; // [groups][8] query | tile-of-query << 16, -1 = unused (scan_pack_groups)
  const int32_t* qoff;      // token offsets of the slice's queries
  int TW;                   // 32 * the most tiles a group of this launch holds
  const float* centroids;
  const float* wlut;
  CodeArr codes;
  const uint8_t* residuals;
  const int64_t* doc_off;
  float pad_ss;
  int64_t doc_begin;        // global id of the shard's document 0
  int64_t d0;               // first document (shard-local) of the pass
  int n;                    // documents of the pass
  int64_t P;                // row stride of keys
  const int32_t* qrow;      // [S] subset row of a query, -1 = none; NULL = no subsets at all
  const uint32_t* docbits;  // [rows][NW]
  int64_t NW;
  uint64_t* keys;           // [S][P]
  unsigned long long* ctr;  // {(query, document) pairs scored, tokens decompressed} or NULL
};

// tile table of the slice, built where the token offsets already are
__global__ void scan_groups_kernel(const int32_t* __restrict__ qoff, int S, int scan_tiles, int32_t* __restrict__ tile_info) {
  if (blockIdx.x == 0 && threadIdx.x == 0) (void)scan_pack_groups(qoff, S, scan_tiles, tile_info, nullptr);
}

// Qf / Qb of every group: the queries' rows (file dim `ldim`) zero-padded to DIM and to whole tiles
__global__ void __launch_bounds__(256) scan_prep_kernel(const float* __restrict__ q, const int32_t* __restrict__ qoff, int ldim,
                                                        int DIM, int TW, const int32_t* __restrict__ tile_info,
                                                        float* __restrict__ Qf, __bf16* __restrict__ Qb) {
  const int g = blockIdx.x;
  const int n = DIM * TW;
  auto value = [&](int k, int col) {
    const int info = tile_info[g * NP_SCAN_MAX_TILES + (col >> 5)];
    if (info < 0 || k >= ldim) return 0.0f;
    const int b = info & 0xFFFF, t = (info >> 16) * 32 + (col & 31);
    const int t0 = qoff[b], lq = qoff[b + 1] - t0;
    return t < lq ? q[(int64_t)(t0 + t) * ldim + k] : 0.0f;
  };
  for (int i = threadIdx.x; i < n; i += 256) {
    if (Qf) {
      const int k = i / TW, col = i - k * TW;
      Qf[(int64_t)g * n + i] = value(k, col);
    } else {
      const int col = i / DIM, k = i - col * DIM;
      Qb[(int64_t)g * n + i] = (__bf16)value(k, col);
    }
  }
}

template <int DIM, int NBITS, bool BF16>
__global__ void __launch_bounds__(256) scan_kernel(ScanP p) {
  constexpr int H = DIM / 2;              // f32: dims per lane
  constexpr int NS = DIM / 16;            // bf16: MFMA k-steps
  constexpr int RS = DIM + 8;             // bf16: LDS row stride in elements (16-byte rows, off the 256-byte bank period)
  constexpr int NT = NP_SCAN_MAX_TILES;
  static_assert(!BF16 || NBITS != 8, "8-bit residuals take the f32 arithmetic");
  extern __shared__ float smem[];
  __shared__ int s_info[NT];
  float* sW = smem;                       // [1 << NBITS]
  float* sQ = smem + (1 << NBITS);        // f32: [DIM][TW]; bf16: [TW][RS]
  __bf16* sQb = reinterpret_cast<__bf16*>(sQ);
  const int g = blockIdx.y, tid = threadIdx.x, TW = p.TW;
  if (tid < NT) s_info[tid] = p.tile_info[g * NT + tid];
  if (tid < (1 << NBITS)) sW[tid] = p.wlut[tid];
  if constexpr (BF16) {
    const __bf16* src = p.Qb + (int64_t)g * TW * DIM;
    for (int i = tid; i < TW * (DIM / 8); i += 256) {
      const int row = i / (DIM / 8), c8 = i - row * (DIM / 8);
      *reinterpret_cast<bf16x8*>(sQb + row * RS + 8 * c8) = *reinterpret_cast<const bf16x8*>(src + (int64_t)row * DIM + 8 * c8);
    }
  } else {
    const float4* src = reinterpret_cast<const float4*>(p.Qf + (int64_t)g * DIM * TW);
    for (int i = tid; i < DIM * TW / 4; i += 256) reinterpret_cast<float4*>(sQ)[i] = src[i];
  }
  __syncthreads();
  int info[NT];
  int ntiles = 0;
#pragma unroll
  for (int x = 0; x < NT; ++x) {
    info[x] = __builtin_amdgcn_readfirstlane(s_info[x]);   // wave-uniform: scalar registers, scalar branches
    if (info[x] >= 0) ntiles = x + 1;
  }
  const int lane = tid & 63, li = lane & 31, kk = lane >> 5, wave = tid >> 6;
  const int64_t nblk = ((int64_t)p.n + 4 * NP_SCAN_DPW - 1) / (4 * NP_SCAN_DPW);
  unsigned long long toks = 0, pairs = 0;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    for (int dd = 0; dd < NP_SCAN_DPW; ++dd) {
      const int64_t dl = (blk * 4 + wave) * NP_SCAN_DPW + dd;   // document of the pass
      if (dl >= p.n) break;
      const int64_t doc = p.d0 + dl;
      const int64_t off = p.doc_off[doc];
      const int len = (int)(p.doc_off[doc + 1] - off);
      // scope: bit x = tile x belongs to a query that has this document in its subset (or has no subset)
      uint32_t mask = 0;
      bool in = false;
#pragma unroll
      for (int x = 0; x < NT; ++x) {
        if (x < ntiles) {
          if ((info[x] >> 16) == 0) {
            const int row = p.qrow ? p.qrow[info[x] & 0xFFFF] : -1;
            in = len > 0 && (row < 0 || ((p.docbits[(int64_t)row * p.NW + (doc >> 5)] >> (doc & 31)) & 1u));
            pairs += in ? 1u : 0u;
          }
          mask |= in ? (1u << x) : 0u;
        }
      }
      mask = __builtin_amdgcn_readfirstlane(mask);
      float m[NT];
#pragma unroll
      for (int x = 0; x < NT; ++x) m[x] = NP_NEG_INF;
      if (mask) {   // (a document outside every subset of the group, or an empty one, is never decompressed)
        toks += (unsigned long long)len;
        for (int t0 = 0; t0 < len; t0 += 32) {
          const int tt = t0 + li;
          const bool valid = tt < len;
          const int64_t tok = off + (valid ? tt : len - 1);
          const uint32_t code = p.codes[tok];
          float rrow[16];
          if constexpr (BF16) {
            bf16x8 a[NS];
            const float ss = unpack_row_bf16<DIM, NBITS>(sW, p.centroids, p.residuals, code, tok, kk, a);
            row_scales(ss, p.pad_ss, valid, kk, rrow);
#pragma unroll
            for (int x = 0; x < NT; ++x) {
              if ((mask >> x) & 1u) {
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                const __bf16* qb = sQb + (x * 32 + li) * RS + 8 * kk;
#pragma unroll
                for (int s = 0; s < NS; ++s)
                  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], *reinterpret_cast<const bf16x8*>(qb + 16 * s), acc, 0, 0, 0);
                m[x] = tile_row_max(acc, rrow, t0, len, kk, m[x]);
              }
            }
          } else {
            float v[H];
            const float ss = unpack_row_f32<DIM, NBITS>(sW, p.centroids, p.residuals, code, tok, kk, v);
            row_scales(ss, p.pad_ss, valid, kk, rrow);
#pragma unroll
            for (int x = 0; x < NT; ++x) {
              if ((mask >> x) & 1u) {
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                const float* qb = sQ + (kk * H) * TW + x * 32 + li;
#pragma unroll
                for (int s = 0; s < H; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[s], qb[s * TW], acc, 0, 0, 0);
                m[x] = tile_row_max(acc, rrow, t0, len, kk, m[x]);
              }
            }
          }
        }
      }
      // per query: the q-ordered sum over its tiles, then the key
      float total = 0.f;
#pragma unroll
      for (int x = 0; x < NT; ++x) {
        if (x < ntiles) {
          const int b = info[x] & 0xFFFF, qt = info[x] >> 16;
          const bool scored = (mask >> x) & 1u;
          if (qt == 0) total = 0.f;
          if (scored) total = tile_sum(m[x], min(32, p.qoff[b + 1] - p.qoff[b] - qt * 32), total);
          const bool last = x + 1 == ntiles || (x + 1 < NT && (info[x + 1] >> 16) == 0);
          if (last && lane == 0)
            p.keys[(int64_t)b * p.P + dl] =
                scored ? ((uint64_t)okey(total) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)(p.doc_begin + doc)) : 0ull;
        }
      }
    }
  }
  if (p.ctr && lane == 0 && (pairs | toks)) {
    atomicAdd(&p.ctr[0], pairs);
    atomicAdd(&p.ctr[1], toks);
  }
}

// ---- top-k of a pass, merged with the passes before it ------------------------------------------------------------
struct ScanTopkP {
  const uint64_t* keys;   // [S][P]
  int64_t P;
  int n;                  // keys of this pass per query
  int n_prev;             // 0 on the first pass, else top_k: best[] holds the result so far (sorted, 0-padded)
  uint64_t* best;         // [S][top_k]
  int top_k, NSELP;       // pow2 >= top_k
  int64_t* out_ids;       // [S][top_k]
  float* out_scores;
  int32_t* out_counts;
};

// block bitonic sort, descending, n = power of two, in LDS (as np_kernels.h's)
__device__ __forceinline__ void scan_sort_desc(uint64_t* s, int n, int tid) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < n; i += 1024) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t a = s[i], c = s[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (a < c) : (a > c)) {
            s[i] = c;
            s[ixj] = a;
          }
        }
      }
    }
  }
  __syncthreads();
}

// One block per query.  Non-zero keys are distinct (distinct documents), so the top_k largest are one set whatever order the
// keys arrive in: a radix select of the top_k-th largest non-zero key, 8 bits per step from the top (select_kernel's), a
// gather of the keys at or above it, a sort.  Bit-equal scores leave the ids to decide: lowest id first, and a cut keeps
// the lowest ids.
__global__ void __launch_bounds__(1024) scan_topk_kernel(ScanTopkP p) {
  extern __shared__ uint64_t s_sel[];
  __shared__ uint32_t hist[256];
  __shared__ uint64_t s_prefix;
  __shared__ uint32_t s_rem, s_n, s_done, s_nz;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = p.n + p.n_prev;
  const uint64_t* kp = p.keys + (int64_t)b * p.P;
  const uint64_t* bp = p.best + (int64_t)b * p.top_k;
  auto key_of = [&](int i) { return i < p.n ? kp[i] : bp[i - p.n]; };
  for (int i = tid; i < p.NSELP; i += 1024) s_sel[i] = 0;
  if (tid == 0) {
    s_n = 0;
    s_nz = 0;
  }
  __syncthreads();
  uint32_t nz = 0;
  for (int i = tid; i < n; i += 1024) nz += key_of(i) != 0;
  if (nz) atomicAdd(&s_nz, nz);
  __syncthreads();
  const int nsel = min((uint32_t)p.top_k, s_nz);
  if (nsel > 0) {
    if ((int)s_nz <= nsel) {
      for (int i = tid; i < n; i += 1024) {
        const uint64_t key = key_of(i);
        if (key) s_sel[atomicAdd(&s_n, 1u)] = key;
      }
    } else {
      if (tid == 0) {
        s_prefix = 0;
        s_rem = (uint32_t)nsel;
        s_done = 0;
      }
      __syncthreads();
      for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        if (s_done) break;
        const uint64_t pre = s_prefix;
        for (int i = tid; i < n; i += 1024) {
          const uint64_t key = key_of(i);
          if (key && (pass == 0 || (key >> (shift + 8)) == pre)) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
          uint32_t rem = s_rem, cum = 0;
          int bin = 255;
          for (; bin > 0; --bin) {
            if (cum + hist[bin] >= rem) break;
            cum += hist[bin];
          }
          s_prefix = (pre << 8) | (uint64_t)bin;
          s_rem = rem - cum;
          if (hist[bin] == rem - cum) s_done = (uint32_t)(pass + 1);   // every key of the cut bin is taken
        }
        __syncthreads();
      }
      const int npass = s_done ? (int)s_done : 8;
      const uint64_t tau = s_prefix;                 // top 8 * npass bits of the cut
      const int sh = 64 - 8 * npass;
      for (int i = tid; i < n; i += 1024) {
        const uint64_t key = key_of(i);
        if (key && (sh == 0 ? key : (key >> sh)) >= tau) s_sel[atomicAdd(&s_n, 1u)] = key;
      }
    }
  }
  scan_sort_desc(s_sel, p.NSELP, tid);   // (its leading barrier also orders the reads of best[] before the writes below)
  for (int j = tid; j < p.top_k; j += 1024) {
    const uint64_t c = j < nsel ? s_sel[j] : 0ull;
    const int64_t o = (int64_t)b * p.top_k + j;
    p.best[o] = c;
    const uint32_t ks = (uint32_t)(c >> 32);
    p.out_ids[o] = j < nsel ? (int64_t)(0xFFFFFFFFu - (uint32_t)(c & 0xFFFFFFFFull)) : 0;
    p.out_scores[o] = j < nsel ? (ks ? unkey(ks) : __uint_as_float(0x7FC00000u)) : 0.f;   // a non-finite score comes back as NaN
  }
  if (tid == 0) p.out_counts[b] = nsel;
}

// ---- host ------------------------------------------------------------------------------------------------------------
static bool scan_geometry_ok(const DeviceIndex* ix) {
  return (ix->dim == 32 || ix->dim == 64 || ix->dim == 96 || ix->dim == 128) && (ix->nbits == 2 || ix->nbits == 4 || ix->nbits == 8);
}

template <int DIM, int NBITS, bool BF16>
static int launch_scan(hipStream_t st, const ScanP& p, unsigned gx, unsigned groups) {
  const size_t lds = (size_t)(1 << NBITS) * 4 + (BF16 ? (size_t)p.TW * (DIM + 8) * 2 : (size_t)DIM * p.TW * 4);
  if (lds > 48 * 1024)
    NP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&scan_kernel<DIM, NBITS, BF16>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  scan_kernel<DIM, NBITS, BF16><<<dim3(gx, groups), 256, lds, st>>>(p);
  return NP_OK;
}

template <int DIM>
static int launch_scan_dim(hipStream_t st, const ScanP& p, unsigned gx, unsigned groups, int nbits, bool bf16) {
  if (nbits == 8) return launch_scan<DIM, 8, false>(st, p, gx, groups);
  if (nbits == 2) return bf16 ? launch_scan<DIM, 2, true>(st, p, gx, groups) : launch_scan<DIM, 2, false>(st, p, gx, groups);
  return bf16 ? launch_scan<DIM, 4, true>(st, p, gx, groups) : launch_scan<DIM, 4, false>(st, p, gx, groups);
}

// bytes of the arena that scale with the slice (per query) -- one expression for the plan and for the carve-up
static int64_t scan_per_query(const DeviceIndex* ix, int top_k, bool subsets) {
  const int64_t NW = (ix->n_docs + 31) / 32;
  return (int64_t)up256((size_t)ix->dim * NP_SCAN_MAX_QUERY_TOKENS * 4)   // the group's staged tiles (f32 bounds bf16)
         + (int64_t)up256((size_t)top_k * 8) + (subsets ? (int64_t)up256((size_t)std::max<int64_t>(NW, 1) * 4) : 0)
         + NP_SCAN_MAX_TILES * 4 + 4 + 256;
}

// The whole batch on device buffers: slices of S queries, passes of P documents.  `base` .. `base + room`: the part of the
// arena this function may carve.  With `stats` the stream is synchronised per pass (timings), otherwise nothing waits.
static int scan_run(const DeviceIndex* ix, ContextUse& use, char* base, const ScanPlan& plan, const float* d_q,
                    const int32_t* d_qoff, const int32_t* h_qoff, int B, int top_k, int precision, const CallSubsets& sub,
                    int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, np_stats* stats) {
  hipStream_t st = use.stream;
  const int S = plan.S;
  const int64_t P = plan.P, NW = std::max<int64_t>((ix->n_docs + 31) / 32, 1);
  const bool bf16 = precision == 3 && ix->nbits != 8;
  const bool subsets = sub.n > 0;
  // carve-up (scan_per_query's terms, times S)
  Carver carve{base};
  unsigned long long* ctr = (unsigned long long*)carve.take(16);
  int32_t* tile_info = (int32_t*)carve.take((size_t)S * NP_SCAN_MAX_TILES * 4);
  int32_t* qrow = (int32_t*)carve.take((size_t)S * 4);
  char* Q = carve.take((size_t)S * up256((size_t)ix->dim * NP_SCAN_MAX_QUERY_TOKENS * 4));
  uint64_t* best = (uint64_t*)carve.take((size_t)S * up256((size_t)top_k * 8));
  uint32_t* docbits = subsets ? (uint32_t*)carve.take((size_t)S * up256((size_t)NW * 4)) : nullptr;
  uint64_t* keys = (uint64_t*)carve.take((size_t)S * P * 8);
  int nselp = 1;
  while (nselp < top_k) nselp <<= 1;
  const size_t topk_lds = (size_t)nselp * 8;
  if (topk_lds > 48 * 1024)
    NP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&scan_topk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)topk_lds));
  if (stats) NP_HIP(hipMemsetAsync(ctr, 0, 16, st));
  for (int s0 = 0; s0 < B; s0 += S) {
    const int Sn = std::min(S, B - s0);
    int max_tiles = 1;
    const int groups = scan_pack_groups(h_qoff + s0, Sn, ix->tune.scan_tiles, nullptr, &max_tiles);
    const int TW = 32 * max_tiles;
    scan_groups_kernel<<<1, 64, 0, st>>>(d_qoff + s0, Sn, ix->tune.scan_tiles, tile_info);
    scan_prep_kernel<<<groups, 256, 0, st>>>(d_q, d_qoff + s0, ix->ldim, ix->dim, TW, tile_info, bf16 ? nullptr : (float*)Q,
                                            bf16 ? (__bf16*)Q : nullptr);
    bool slice_subsets = subsets;
    if (subsets) {
      int64_t lo = 0, hi = sub.total;
      if (sub.h_off && sub.h_qsub) {   // only the ids this slice's queries reference
        lo = sub.total;
        hi = 0;
        slice_subsets = false;
        for (int b = 0; b < Sn; ++b) {
          const int32_t q = sub.h_qsub[s0 + b];
          if (q < 0) continue;
          slice_subsets = true;
          if (sub.h_off[q + 1] == sub.h_off[q]) continue;
          lo = std::min(lo, sub.h_off[q]);
          hi = std::max(hi, sub.h_off[q + 1]);
        }
        if (hi < lo) lo = hi = 0;
      }
      if (slice_subsets)
        NP_TRY(subset_doc_rows(ix, st, sub.d_ids, sub.d_off, sub.d_qsub + s0, sub.n, sub.total, lo, hi, Sn, NW, docbits, qrow));
    }
    for (int64_t d0 = 0, pass = 0; d0 < std::max<int64_t>(ix->n_docs, 1); d0 += P, ++pass) {
      const int n = (int)std::max<int64_t>(0, std::min<int64_t>(P, ix->n_docs - d0));
      if (stats) NP_HIP(hipEventRecord(use.ctx->ev[0], st));
      if (n > 0) {
        ScanP sp;
        sp.Qf = bf16 ? nullptr : (const float*)Q;
        sp.Qb = bf16 ? (const __bf16*)Q : nullptr;
        sp.tile_info = tile_info;
        sp.qoff = d_qoff + s0;
        sp.TW = TW;
        sp.centroids = ix->d_centroids.get();
        sp.wlut = ix->d_wlut.get();
        sp.codes = ix->codes();
        sp.residuals = ix->d_residuals.get();
        sp.doc_off = ix->d_doc_offsets.get();
        sp.pad_ss = ix->pad_ss;
        sp.doc_begin = ix->doc_begin;
        sp.d0 = d0;
        sp.n = n;
        sp.P = P;
        sp.qrow = slice_subsets ? qrow : nullptr;
        sp.docbits = docbits;
        sp.NW = NW;
        sp.keys = keys;
        sp.ctr = stats ? ctr : nullptr;
        const int64_t nblk = ((int64_t)n + 4 * NP_SCAN_DPW - 1) / (4 * NP_SCAN_DPW);
        const unsigned gx = (unsigned)std::min<int64_t>(nblk, std::max(1, 2048 / groups));
        int rc;
        switch (ix->dim) {
          case 32: rc = launch_scan_dim<32>(st, sp, gx, (unsigned)groups, ix->nbits, bf16); break;
          case 64: rc = launch_scan_dim<64>(st, sp, gx, (unsigned)groups, ix->nbits, bf16); break;
          case 96: rc = launch_scan_dim<96>(st, sp, gx, (unsigned)groups, ix->nbits, bf16); break;
          default: rc = launch_scan_dim<128>(st, sp, gx, (unsigned)groups, ix->nbits, bf16); break;
        }
        NP_TRY(rc);
      }
      if (stats) NP_HIP(hipEventRecord(use.ctx->ev[1], st));
      ScanTopkP tp;
      tp.keys = keys;
      tp.P = P;
      tp.n = n;
      tp.n_prev = pass > 0 ? top_k : 0;
      tp.best = best;
      tp.top_k = top_k;
      tp.NSELP = nselp;
      tp.out_ids = d_out_ids + (int64_t)s0 * top_k;
      tp.out_scores = d_out_scores + (int64_t)s0 * top_k;
      tp.out_counts = d_out_counts + s0;
      scan_topk_kernel<<<Sn, 1024, topk_lds, st>>>(tp);
      NP_HIP(hipGetLastError());
      if (stats) {
        NP_HIP(hipEventRecord(use.ctx->ev[2], st));
        NP_HIP(hipStreamSynchronize(st));
        float a = 0, b = 0;
        (void)hipEventElapsedTime(&a, use.ctx->ev[0], use.ctx->ev[1]);
        (void)hipEventElapsedTime(&b, use.ctx->ev[1], use.ctx->ev[2]);
        stats->ms_exact += a;
        stats->ms_topk += b;
        stats->ms_total += a + b;
      }
    }
  }
  if (stats) {
    unsigned long long h[2] = {0, 0};
    NP_HIP(hipMemcpyAsync(h, ctr, 16, hipMemcpyDeviceToHost, st));
    NP_HIP(hipStreamSynchronize(st));
    stats->n_exact_docs = (int64_t)h[0];
    stats->n_exact_tokens = (int64_t)h[1];
    stats->n_queries = B;
  }
  return NP_OK;
}

static int scan_validate(const np_index* ix, int32_t B, int32_t dim, int32_t top_k, int32_t precision, const int32_t* h_qoff) {
  if (!ix) {
    set_error("Search failed: NULL index");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const char* why = "";
  const int c = scan_check_args(B, dim, ix->ldim, scan_geometry_ok(ix), top_k, precision, h_qoff, &why);
  if (c == 1) {
    set_error("Shape error: %s (query dim %d, index dim %d nbits %d)", why, dim, ix->ldim, ix->lnbits);
    return NP_ERR_SHAPE;
  }
  if (c == 2) {
    set_error("Search failed: %s (top_k=%d precision=%d)", why, top_k, precision);
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

static int scan_plan_for(const DeviceIndex* ix, int64_t fixed, int B, int top_k, bool subsets, ScanPlan* plan) {
  const int64_t budget = ix->ws_budget.load(std::memory_order_relaxed);
  if (!scan_plan(budget, fixed + 4096, scan_per_query(ix, top_k, subsets), ix->n_docs, B, ix->opts.max_batch, ix->tune.scan_docs,
                 plan)) {
    set_error("Search failed: the exact scan's key table does not fit the workspace budget of %lld bytes", (long long)budget);
    return NP_ERR_OUT_OF_MEMORY;
  }
  return NP_OK;
}

static size_t scan_arena_bytes(const DeviceIndex* ix, const ScanPlan& plan, int top_k, bool subsets) {
  return 4096 + (size_t)plan.S * (size_t)scan_per_query(ix, top_k, subsets) + up256((size_t)plan.S * plan.P * 8);
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_search_exact_device(const np_index* ix, const float* d_queries, const int32_t* d_q_tok_offsets,
                               const int32_t* h_q_tok_offsets, int32_t B, int32_t dim, int32_t top_k, int32_t precision,
                               const int64_t* d_subset_ids, const int64_t* d_subset_offsets, const int64_t* h_subset_offsets,
                               int64_t n_subsets, const int32_t* d_query_subset, int64_t* d_out_ids, float* d_out_scores,
                               int32_t* d_out_counts, void* stream) {
  clear_error();
  if (B > 0 && !h_q_tok_offsets) {
    set_error("Search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(scan_validate(ix, B, dim, top_k, precision, B > 0 ? h_q_tok_offsets : nullptr));
  NP_TRY(check_device_subsets(d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset, B));
  if (B == 0) return NP_OK;
  if (!d_queries || !d_q_tok_offsets || !d_out_ids || !d_out_scores || !d_out_counts) {
    set_error("Search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const CallSubsets sub = CallSubsets::device(d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset);
  DeviceGuard g(ix->device);
  ScanPlan plan;
  NP_TRY(scan_plan_for(ix, 0, B, top_k, sub.n > 0, &plan));
  ContextUse use;
  NP_TRY(use.begin(ix, stream));
  NP_TRY(use.arena().reserve(scan_arena_bytes(ix, plan, top_k, sub.n > 0)));
  return scan_run(ix, use, use.arena().as<char>(), plan, d_queries, d_q_tok_offsets, h_q_tok_offsets, B, top_k, precision, sub,
                  d_out_ids, d_out_scores, d_out_counts, nullptr);
}

// np_hip_search_exact and np_hip_search_exact_filtered: the subsets come as a host CSR, or (filters != NULL) are evaluated
// on the call's context into a CSR that stays on the device; query_subset is the query map of either
static int scan_host(const np_index* ix, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                     int32_t top_k, int32_t precision, const int64_t* subset_ids, const int64_t* subset_offsets,
                     int64_t n_subsets, const int32_t* query_subset, const np_filter* filters, int64_t* out_ids,
                     float* out_scores, int32_t* out_counts, np_stats* stats) {
  clear_error();
  IndexRead reading(ix);   // an append waits for this call and holds later ones back (np_internal.h)
  if (stats) memset(stats, 0, sizeof *stats);
  if (B > 0 && !q_tok_offsets) {
    set_error("Search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(scan_validate(ix, B, dim, top_k, precision, B > 0 ? q_tok_offsets : nullptr));
  if (filters)
    NP_TRY(filter_check_call(ix, filters, (int32_t)n_subsets, query_subset, B, true));
  else
    NP_TRY(check_subsets(subset_ids, subset_offsets, n_subsets, query_subset, query_subset, B));
  if (B == 0) return NP_OK;
  if (!queries || !out_ids || !out_scores || !out_counts) {
    set_error("Search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g(ix->device);
  ContextUse use;
  NP_TRY(use.begin(ix, nullptr));
  hipStream_t st = use.stream;
  HostScope scope;
  NP_TRY(scope.resolve(ix, use, subset_ids, subset_offsets, n_subsets, query_subset, filters, B));
  const int64_t ntok = q_tok_offsets[B];
  // behind the scan's own regions: queries, offsets, the subsets, the batch's results
  const size_t b_q = up256((size_t)std::max<int64_t>(ntok, 1) * dim * 4), b_qoff = up256((size_t)(B + 1) * 4);
  ResultStage res(B, top_k);
  const size_t user = b_q + b_qoff + scope.stage_bytes() + res.bytes();
  ScanPlan plan;
  NP_TRY(scan_plan_for(ix, (int64_t)user + scope.budget_extra(), B, top_k, scope.any, &plan));
  NP_TRY(use.arena().reserve(user + scan_arena_bytes(ix, plan, top_k, scope.any)));
  void* pin = nullptr;
  NP_TRY(use.pin(res.bytes(), &pin));
  Carver carve{use.arena().as<char>()};
  float* d_q = (float*)carve.take(b_q);
  int32_t* d_qoff = (int32_t*)carve.take(b_qoff);
  CallSubsets sub;
  NP_TRY(scope.place(carve, st, &sub));
  res.carve(carve);
  if (ntok > 0) NP_HIP(hipMemcpyAsync(d_q, queries, (size_t)ntok * dim * 4, hipMemcpyHostToDevice, st));
  NP_HIP(hipMemcpyAsync(d_qoff, q_tok_offsets, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, st));
  NP_TRY(scan_run(ix, use, carve.at, plan, d_q, d_qoff, q_tok_offsets, B, top_k, precision, sub, res.d_ids, res.d_sc, res.d_cnt, stats));
  NP_TRY(res.fetch(pin, st));
  NP_TRY(use.end());
  NP_HIP(hipStreamSynchronize(st));
  res.deliver(out_ids, out_scores, out_counts);
  if (stats) stats->ms_total += scope.ms();
  return NP_OK;
}

int np_hip_search_exact(const np_index* ix, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                        int32_t top_k, int32_t precision, const int64_t* subset_ids, const int64_t* subset_offsets,
                        int64_t n_subsets, const int32_t* query_subset, int64_t* out_ids, float* out_scores,
                        int32_t* out_counts, np_stats* stats) {
  return scan_host(ix, queries, q_tok_offsets, B, dim, top_k, precision, subset_ids, subset_offsets, n_subsets, query_subset,
                   nullptr, out_ids, out_scores, out_counts, stats);
}

int np_hip_search_exact_filtered(const np_index* ix, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                                 int32_t top_k, int32_t precision, const np_filter* filters, int32_t n_filters,
                                 const int32_t* query_filter, int64_t* out_ids, float* out_scores, int32_t* out_counts,
                                 np_stats* stats) {
  static const np_filter none{};   // n_filters == 0: nothing to check or evaluate, but still the filtered call's checks
  return scan_host(ix, queries, q_tok_offsets, B, dim, top_k, precision, nullptr, nullptr, n_filters, query_filter,
                   filters ? filters : &none, out_ids, out_scores, out_counts, stats);
}

}  // extern "C"
