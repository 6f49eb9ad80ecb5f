// np_pairs.hip -- np_hip_score_pairs: the exact MaxSim of given (query, document) pairs, with the per-token matches.
//
// S6 (np_kernels.h) scores the documents a search selected and np_scan.hip scores all of them; both keep only the sum.
// Here the caller names the pairs, and besides the S6 score every query token gets its maximum and the document token
// that reached it.  The arithmetic is np_exact.h's (one definition of the decompression, the row scales, the masked
// maxima and the q-ordered sum), in exact_f32_kernel's shape: a workgroup stages one query in LDS, a wave walks a
// document in 32-token tiles.
//   grid          one-dimensional: query i of the slice takes ceil(n_i / 16) workgroups (its pairs are contiguous), so a
//                 query with many pairs and a query with none cost what they should; pairs_prefix_kernel builds the map
//   outputs       scores [pair], sims / positions [pair][Lq of its query], rows coalesced, either may be left out
// A pair's outputs depend on nothing but its query and its document: one tile of one query per MFMA, the query's own
// token order in the sum -- so they do not depend on the batch, the slices, the chunks or the pair's place in the list.
#include "np_internal.h"
#include "np_exact.h"
#include "np_pairs_plan.h"

#include <string.h>

namespace np {

#define NP_PAIRS_DPW 4   // documents per wave, as NP_EXACT_DPW
static_assert(NP_PAIRS_WG_DOCS == 4 * NP_PAIRS_DPW, "np_pairs_plan.h sizes the grid for 4 waves of NP_PAIRS_DPW documents");

struct PairsP {
  const float* Qt;          // [Sn][DIM][LQP] f32, k-major
  const int32_t* qoff;      // token offsets of the slice's queries [Sn + 1]
  const int64_t* poff;      // pair offsets of the slice's queries [Sn + 1]
  const int32_t* wgpre;     // [Sn + 1] workgroups before query i (pairs_prefix)
  const int64_t* rowbase;   // [Sn + 1] row entries before query i, from the slice's first
  int Sn, LQP;
  const float* centroids;
  const float* wlut;
  CodeArr codes;
  const uint8_t* residuals;
  const int64_t* doc_off;
  const uint16_t* tok_pos;  // NULL, or the on-disk position of every stored token (a handle that keeps its tokens by code)
  float pad_ss;
  int64_t doc_begin, n_docs;
  const int64_t* pair_docs; // global ids, indexed by poff's values
  float* scores;            // indexed by poff's values
  float* sims;              // [row entries of the call], or NULL
  int32_t* pos;             // ..., or NULL
  int64_t row0;             // row entries before the slice
  unsigned long long* ctr;  // {pairs scored, tokens decompressed} or NULL
};

__global__ void pairs_prefix_kernel(const int32_t* __restrict__ qoff, const int64_t* __restrict__ poff, int Sn,
                                    int32_t* __restrict__ wgpre, int64_t* __restrict__ rowbase) {
  if (blockIdx.x == 0 && threadIdx.x == 0) (void)pairs_prefix(qoff, poff, Sn, wgpre, rowbase);
}

// Qt of every query of the slice: its rows (file dim `ldim`) zero-padded to DIM and to LQP tokens, k-major
__global__ void __launch_bounds__(256) pairs_prep_kernel(const float* __restrict__ q, const int32_t* __restrict__ qoff, int ldim,
                                                         int DIM, int LQP, float* __restrict__ Qt) {
  const int b = blockIdx.x;
  const int t0 = qoff[b], lq = qoff[b + 1] - t0;
  const int n = DIM * LQP;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int k = i / LQP, col = i - k * LQP;
    Qt[(int64_t)b * n + i] = (k < ldim && col < lq) ? q[(int64_t)(t0 + col) * ldim + k] : 0.0f;
  }
}

template <int DIM, int NBITS, int NQT>
__global__ void __launch_bounds__(256) pairs_kernel(PairsP p) {
  constexpr int H = DIM / 2;              // dims per lane
  extern __shared__ float smem[];
  const int LQP = p.LQP;
  float* sQ = smem;                       // [DIM][LQP]: lane li reads column qt * 32 + li of row k -- consecutive banks
  float* sW = smem + DIM * LQP;           // [1 << NBITS]
  const int tid = threadIdx.x;
  const int b = pairs_query_of(p.wgpre, p.Sn, (int64_t)blockIdx.x);
  const int wg = (int)blockIdx.x - p.wgpre[b];
  {
    const float4* src = reinterpret_cast<const float4*>(p.Qt + (int64_t)b * DIM * LQP);
    for (int i = tid; i < DIM * LQP / 4; i += 256) reinterpret_cast<float4*>(sQ)[i] = src[i];
  }
  if (tid < (1 << NBITS)) sW[tid] = p.wlut[tid];
  __syncthreads();
  const int lane = tid & 63, li = lane & 31, kk = lane >> 5, wave = tid >> 6;
  const int Lq = p.qoff[b + 1] - p.qoff[b];
  const int nqt = (Lq + 31) >> 5;
  const int64_t pbeg = p.poff[b];
  const int64_t n = p.poff[b + 1] - pbeg;
  unsigned long long toks = 0, npairs = 0;
  for (int dd = 0; dd < NP_PAIRS_DPW; ++dd) {
    const int64_t j = ((int64_t)wg * 4 + wave) * NP_PAIRS_DPW + dd;
    if (j >= n) break;
    const int64_t doc = p.pair_docs[pbeg + j] - p.doc_begin;      // shard-local
    const bool here = doc >= 0 && doc < p.n_docs;
    int64_t off = 0;
    int len = 0;
    if (here) {
      off = p.doc_off[doc];
      len = (int)(p.doc_off[doc + 1] - off);
      toks += (unsigned long long)len;
      ++npairs;
    }
    float m[NQT];
    int ps[NQT];
#pragma unroll
    for (int x = 0; x < NQT; ++x) {
      m[x] = NP_NEG_INF;
      ps[x] = -1;
    }
    for (int t0 = 0; t0 < len; t0 += 32) {
      const int tt = t0 + li;
      const bool valid = tt < len;
      const int64_t tok = off + (valid ? tt : len - 1);
      const uint32_t code = p.codes[tok];
      float v[H];
      const float ss = unpack_row_f32<DIM, NBITS>(sW, p.centroids, p.residuals, code, tok, kk, v);
      float rrow[16];
      row_scales(ss, p.pad_ss, valid, kk, rrow);
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
        if (qt < nqt) {
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = 0.f;
          const float* qb = sQ + (kk * H) * LQP + qt * 32 + li;
#pragma unroll
          for (int s = 0; s < H; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[s], qb[s * LQP], acc, 0, 0, 0);
          tile_row_argmax(acc, rrow, t0, len, kk, m[qt], ps[qt]);
        }
      }
    }
    // the score, exactly as S6 forms it; then the two halves of every query token agree on (max, lowest position)
    float total = 0.f;
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      if (qt < nqt) total = tile_sum(m[qt], min(32, Lq - qt * 32), total);
    }
    if (lane == 0) p.scores[pbeg + j] = (here && finitef(total)) ? total : __uint_as_float(0x7FC00000u);
    if (p.sims || p.pos) {
      const int64_t row = p.row0 + p.rowbase[b] + j * (int64_t)Lq;
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
        if (qt < nqt) {
          const float om = __shfl_xor(m[qt], 32);
          const int op = __shfl_xor(ps[qt], 32);
          int best = ps[qt];
          if (om > m[qt] || (om == m[qt] && op < best)) best = op;
          const float mx = fmaxf(m[qt], om);
          const int tq = qt * 32 + li;
          if (kk == 0 && tq < Lq) {
            if (p.sims) p.sims[row + tq] = mx;
            if (p.pos) p.pos[row + tq] = (best >= 0 && p.tok_pos) ? (int32_t)p.tok_pos[off + best] : best;
          }
        }
      }
    }
  }
  if (p.ctr && lane == 0 && (npairs | toks)) {
    atomicAdd(&p.ctr[0], npairs);
    atomicAdd(&p.ctr[1], toks);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static bool pairs_geometry_ok(const DeviceIndex* ix) {
  return (ix->dim == 32 || ix->dim == 64 || ix->dim == 96 || ix->dim == 128) && (ix->nbits == 2 || ix->nbits == 4 || ix->nbits == 8);
}

template <int DIM, int NBITS, int NQT>
static int launch_pairs(hipStream_t st, const PairsP& p, unsigned gx) {
  const size_t lds = ((size_t)DIM * p.LQP + (1 << NBITS)) * sizeof(float);
  if (lds > 48 * 1024)
    NP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pairs_kernel<DIM, NBITS, NQT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  pairs_kernel<DIM, NBITS, NQT><<<gx, 256, lds, st>>>(p);
  return NP_OK;
}

template <int DIM, int NBITS>
static int launch_pairs_qt(hipStream_t st, const PairsP& p, unsigned gx) {
  if (p.LQP <= 32) return launch_pairs<DIM, NBITS, 1>(st, p, gx);
  if (p.LQP <= 64) return launch_pairs<DIM, NBITS, 2>(st, p, gx);
  return launch_pairs<DIM, NBITS, NP_MAX_QT>(st, p, gx);
}

template <int DIM>
static int launch_pairs_dim(hipStream_t st, const PairsP& p, unsigned gx, int nbits) {
  if (nbits == 8) return launch_pairs_qt<DIM, 8>(st, p, gx);
  if (nbits == 2) return launch_pairs_qt<DIM, 2>(st, p, gx);
  return launch_pairs_qt<DIM, 4>(st, p, gx);
}

// bytes of the arena that scale with the slice (per query): its staged Qt at the longest query, its two map entries
static int64_t pairs_per_query(const DeviceIndex* ix) {
  return (int64_t)up256((size_t)ix->dim * NP_PAIRS_MAX_QUERY_TOKENS * 4) + 16;
}
static const size_t kPairsFixed = 4096;   // the counters, the maps' last entries and the alignment of the regions
// what pairs_run carves for slices of S queries; its last 256 bytes are the caller's (the counters)
static size_t pairs_run_bytes(const DeviceIndex* ix, int S) { return up256(kPairsFixed + (size_t)S * (size_t)pairs_per_query(ix)); }

// Queries [0, B) on device buffers, in slices of at most S.  d_poff's values index d_pair_docs and d_scores; the row
// entries start at d_sims / d_pos.  `base`: pairs_run_bytes(S) of the arena.  With `stats` the kernels
// are timed between two events (the caller synchronises); nothing here waits.
static int pairs_run(const DeviceIndex* ix, ContextUse& use, char* base, int S, const float* d_q, const int32_t* d_qoff,
                     const int32_t* h_qoff, int B, const int64_t* d_pair_docs, const int64_t* d_poff, const int64_t* h_poff,
                     float* d_scores, float* d_sims, int32_t* d_pos, unsigned long long* ctr, np_stats* stats) {
  hipStream_t st = use.stream;
  Carver carve{base};
  int64_t* rowbase = (int64_t*)carve.take((size_t)(S + 1) * 8);
  int32_t* wgpre = (int32_t*)carve.take((size_t)(S + 1) * 4);
  float* Qt = (float*)carve.take((size_t)S * up256((size_t)ix->dim * NP_PAIRS_MAX_QUERY_TOKENS * 4));
  int64_t row0 = 0;
  for (int s0 = 0; s0 < B;) {
    int max_lq = 0;
    const int Sn = pairs_next_slice(h_qoff, h_poff, s0, B, S, &max_lq);
    const int64_t wgs = pairs_prefix(h_qoff + s0, h_poff + s0, Sn, nullptr, nullptr);
    if (wgs > 0) {
      const int LQP = std::max(32, (max_lq + 31) / 32 * 32);
      pairs_prefix_kernel<<<1, 64, 0, st>>>(d_qoff + s0, d_poff + s0, Sn, wgpre, rowbase);
      pairs_prep_kernel<<<Sn, 256, 0, st>>>(d_q, d_qoff + s0, ix->ldim, ix->dim, LQP, Qt);
      PairsP p;
      p.Qt = Qt;
      p.qoff = d_qoff + s0;
      p.poff = d_poff + s0;
      p.wgpre = wgpre;
      p.rowbase = rowbase;
      p.Sn = Sn;
      p.LQP = LQP;
      p.centroids = ix->d_centroids.get();
      p.wlut = ix->d_wlut.get();
      p.codes = ix->codes();
      p.residuals = ix->d_residuals.get();
      p.doc_off = ix->d_doc_offsets.get();
      p.tok_pos = ix->tok_sorted ? ix->d_tok_pos.get() : nullptr;
      p.pad_ss = ix->pad_ss;
      p.doc_begin = ix->doc_begin;
      p.n_docs = ix->n_docs;
      p.pair_docs = d_pair_docs;
      p.scores = d_scores;
      p.sims = d_sims;
      p.pos = d_pos;
      p.row0 = row0;
      p.ctr = ctr;
      if (stats) NP_HIP(hipEventRecord(use.ctx->ev[0], st));
      int rc;
      switch (ix->dim) {
        case 32: rc = launch_pairs_dim<32>(st, p, (unsigned)wgs, ix->nbits); break;
        case 64: rc = launch_pairs_dim<64>(st, p, (unsigned)wgs, ix->nbits); break;
        case 96: rc = launch_pairs_dim<96>(st, p, (unsigned)wgs, ix->nbits); break;
        default: rc = launch_pairs_dim<128>(st, p, (unsigned)wgs, ix->nbits); break;
      }
      NP_TRY(rc);
      NP_HIP(hipGetLastError());
      if (stats) {   // one slice at a time between the two events
        NP_HIP(hipEventRecord(use.ctx->ev[1], st));
        NP_HIP(hipStreamSynchronize(st));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, use.ctx->ev[0], use.ctx->ev[1]);
        stats->ms_exact += ms;
        stats->ms_total += ms;
      }
    }
    row0 += pairs_rows(h_qoff + s0, h_poff + s0, Sn);
    s0 += Sn;
  }
  return NP_OK;
}

static int pairs_validate(const np_index* ix, int32_t B, int32_t dim, int32_t precision, const int32_t* h_qoff,
                          const int64_t* h_poff) {
  if (!ix) {
    set_error("Search failed: NULL index");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const char* why = "";
  const int c = pairs_check_args(B, dim, ix->ldim, pairs_geometry_ok(ix), precision, h_qoff, h_poff, &why);
  if (c == 1) {
    set_error("Shape error: %s (query dim %d, index dim %d nbits %d)", why, dim, ix->ldim, ix->lnbits);
    return NP_ERR_SHAPE;
  }
  if (c == 2) {
    set_error("Search failed: %s (precision=%d)", why, precision);
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

static int pairs_plan_for(const DeviceIndex* ix, int64_t fixed, int B, int64_t worst_pair, PairsPlan* plan) {
  const int64_t budget = ix->ws_budget.load(std::memory_order_relaxed);
  if (!pairs_plan(budget, fixed + (int64_t)kPairsFixed + 256, pairs_per_query(ix), B, ix->opts.max_batch, worst_pair, plan)) {
    set_error("Search failed: one query and one pair of score_pairs do not fit the workspace budget of %lld bytes",
              (long long)budget);
    return NP_ERR_OUT_OF_MEMORY;
  }
  return NP_OK;
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_score_pairs_device(const np_index* ix, const float* d_queries, const int32_t* d_q_tok_offsets,
                              const int32_t* h_q_tok_offsets, int32_t B, int32_t dim, int32_t precision,
                              const int64_t* d_pair_docs, const int64_t* d_pair_offsets, const int64_t* h_pair_offsets,
                              float* d_out_scores, float* d_out_token_sims, int32_t* d_out_token_pos, void* stream) {
  clear_error();
  NP_TRY(pairs_validate(ix, B, dim, precision, h_q_tok_offsets, h_pair_offsets));
  if (B == 0 || h_pair_offsets[B] == 0) return NP_OK;
  if (!d_queries || !d_q_tok_offsets || !d_pair_docs || !d_pair_offsets || !d_out_scores) {
    set_error("Search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g(ix->device);
  PairsPlan plan;
  NP_TRY(pairs_plan_for(ix, 0, B, 0, &plan));
  ContextUse use;
  NP_TRY(use.begin(ix, stream));
  NP_TRY(use.arena().reserve(pairs_run_bytes(ix, plan.S)));
  return pairs_run(ix, use, use.arena().as<char>(), plan.S, d_queries, d_q_tok_offsets, h_q_tok_offsets, B, d_pair_docs,
                   d_pair_offsets, h_pair_offsets, d_out_scores, d_out_token_sims, d_out_token_pos, nullptr, nullptr);
}

int np_hip_score_pairs(const np_index* ix, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                       int32_t precision, const int64_t* pair_docs, const int64_t* pair_offsets, float* out_scores,
                       float* out_token_sims, int32_t* out_token_pos, np_stats* stats) {
  clear_error();
  if (stats) memset(stats, 0, sizeof *stats);
  NP_TRY(pairs_validate(ix, B, dim, precision, q_tok_offsets, pair_offsets));
  if (stats) stats->n_queries = B;
  if (B == 0) return NP_OK;
  const int64_t P = pair_offsets[B];
  if (P == 0) return NP_OK;
  if (!queries || !pair_docs || !out_scores) {
    set_error("Search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const int64_t bad = pairs_first_bad_id(pair_docs, P, ix->N_total);
  if (bad >= 0) {
    set_error("Search failed: pair %lld names document %lld, outside [0, %lld)", (long long)bad, (long long)pair_docs[bad],
              (long long)ix->N_total);
    return NP_ERR_INVALID_ARGUMENT;
  }
  const bool rows = out_token_sims || out_token_pos;
  int max_lq = 0;
  for (int b = 0; b < B; ++b) max_lq = std::max(max_lq, q_tok_offsets[b + 1] - q_tok_offsets[b]);
  const int64_t ntok = q_tok_offsets[B];
  // ahead of the run's own regions: the queries, their offsets, a chunk's pair offsets; behind them: the chunk's staging
  const size_t b_q = up256((size_t)std::max<int64_t>(ntok, 1) * dim * 4), b_qoff = up256((size_t)(B + 1) * 4);
  const size_t b_poff = up256((size_t)(B + 1) * 8);
  const size_t slop = 4 * 256;   // the four staged arrays start on 256-byte boundaries
  DeviceGuard g(ix->device);
  PairsPlan plan;
  NP_TRY(pairs_plan_for(ix, (int64_t)(b_q + b_qoff + b_poff + slop), B, pairs_pair_bytes(max_lq, rows), &plan));
  ContextUse use;
  NP_TRY(use.begin(ix, nullptr));
  hipStream_t st = use.stream;
  const size_t run_bytes = pairs_run_bytes(ix, plan.S);
  const size_t stage = (size_t)plan.chunk + slop;
  NP_TRY(use.arena().reserve(b_q + b_qoff + b_poff + run_bytes + stage));
  void* pinv = nullptr;
  NP_TRY(use.pin(b_poff + stage, &pinv));
  Carver carve{use.arena().as<char>()};
  float* d_q = (float*)carve.take(b_q);
  int32_t* d_qoff = (int32_t*)carve.take(b_qoff);
  int64_t* d_poff = (int64_t*)carve.take(b_poff);
  char* run_base = carve.take(run_bytes);
  unsigned long long* ctr = (unsigned long long*)(run_base + run_bytes - 256);   // inside kPairsFixed, past the run's regions
  char* d_stage = carve.take(stage);
  int64_t* h_poff = (int64_t*)pinv;
  char* h_stage = (char*)pinv + b_poff;
  if (ntok > 0) NP_HIP(hipMemcpyAsync(d_q, queries, (size_t)ntok * dim * 4, hipMemcpyHostToDevice, st));
  NP_HIP(hipMemcpyAsync(d_qoff, q_tok_offsets, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, st));
  if (stats) NP_HIP(hipMemsetAsync(ctr, 0, 16, st));
  PairsChunk c;
  int64_t p0 = 0, r0 = 0;
  int q_hint = 0;
  while (pairs_next_chunk(q_tok_offsets, pair_offsets, B, rows, plan.chunk, q_hint, p0, r0, &c)) {
    const int nq = c.q1 - c.q0;
    const int64_t np_ = c.p1 - c.p0, nr = c.r1 - c.r0;
    // the chunk as a batch of its own: queries [q0, q1) with their pair lists clipped to [p0, p1), offsets from 0
    for (int i = 0; i <= nq; ++i)
      h_poff[i] = std::min(std::max(pair_offsets[c.q0 + i], c.p0), c.p1) - c.p0;
    const size_t o_ids = 0, o_sc = up256((size_t)np_ * 8), o_sim = o_sc + up256((size_t)np_ * 4);
    const size_t o_pos = o_sim + up256((size_t)nr * 4);
    memcpy(h_stage + o_ids, pair_docs + c.p0, (size_t)np_ * 8);
    NP_HIP(hipMemcpyAsync(d_poff, h_poff, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
    NP_HIP(hipMemcpyAsync(d_stage + o_ids, h_stage + o_ids, (size_t)np_ * 8, hipMemcpyHostToDevice, st));
    NP_TRY(pairs_run(ix, use, run_base, plan.S, d_q, d_qoff + c.q0, q_tok_offsets + c.q0, nq, (const int64_t*)(d_stage + o_ids),
                     d_poff, h_poff, (float*)(d_stage + o_sc), out_token_sims ? (float*)(d_stage + o_sim) : nullptr,
                     out_token_pos ? (int32_t*)(d_stage + o_pos) : nullptr, stats ? ctr : nullptr, stats));
    NP_HIP(hipMemcpyAsync(h_stage + o_sc, d_stage + o_sc, (size_t)np_ * 4, hipMemcpyDeviceToHost, st));
    if (out_token_sims && nr > 0) NP_HIP(hipMemcpyAsync(h_stage + o_sim, d_stage + o_sim, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
    if (out_token_pos && nr > 0) NP_HIP(hipMemcpyAsync(h_stage + o_pos, d_stage + o_pos, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
    NP_HIP(hipStreamSynchronize(st));
    memcpy(out_scores + c.p0, h_stage + o_sc, (size_t)np_ * 4);
    if (out_token_sims && nr > 0) memcpy(out_token_sims + c.r0, h_stage + o_sim, (size_t)nr * 4);
    if (out_token_pos && nr > 0) memcpy(out_token_pos + c.r0, h_stage + o_pos, (size_t)nr * 4);
    p0 = c.p1;
    r0 = c.r1;
    q_hint = c.q1 - 1;
  }
  if (p0 != P) {   // (the plan holds one pair of the longest query, so a chunk always advances)
    set_error("Search failed: score_pairs could not stage pair %lld within the workspace budget", (long long)p0);
    return NP_ERR_OUT_OF_MEMORY;
  }
  if (stats) {
    unsigned long long h[2] = {0, 0};
    NP_HIP(hipMemcpyAsync(h, ctr, 16, hipMemcpyDeviceToHost, st));
    NP_HIP(hipStreamSynchronize(st));
    stats->n_exact_docs = (int64_t)h[0];
    stats->n_exact_tokens = (int64_t)h[1];
  }
  NP_TRY(use.end());
  return NP_OK;
}

}  // extern "C"
