// np_maxsim_long.hip -- np_hip_maxsim_batch_long: np_hip_maxsim_batch (np_maxsim.hip) for queries of any length, f32 or bf16
// rows, modes 0 to 2 of maxsim_kernel on the same MFMAs (v_mfma_f32_32x32x2f32, v_mfma_f32_32x32x16_bf16).
//
// maxsim_kernel holds one accumulator tile and one row of keys per 32-token query tile, eight at most: 256 tokens.  A query
// token's maximum needs every document tile but only its own query tile, and the score is an ordered sum over the query
// tokens, which can be carried.  So a query is walked in PASSES of at most NQT query tiles: the accumulators, the slots'
// LDS rows and the key table stay one pass wide whatever the query's length.
//
//   work split    blockIdx.y = one query in both forms (G = 1); blockIdx.x = WD <= 4 documents (all pairs) or WD consecutive
//                 pairs of the query's list.  The workgroup (4 waves) walks the query's passes in ascending token order.
//                 WD halves on the host while the grid is below two workgroups per compute unit (maxsim_long_plan).
//   passes        nqt = the query's tiles, passes = ceil(nqt / NQT), and the passes are even: the first nqt % passes take
//                 one tile more (np_maxsim_plan.h: 33 tiles are 7, 7, 7, 6, 6, never 8, 8, 8, 8, 1), so no pass pays a full
//                 round loop for one tile.  NQT <= 8 for the bf16 modes and <= 4 for mode 0, where 8 f32 accumulator tiles
//                 spill (profiles/maxsim_kernel_resources.md).
//   a pass        maxsim_kernel's round / chunk loop: the 32-token tiles of the workgroup's documents go round-robin to the
//                 waves; per chunk of KC dims all 256 threads stage the pass's query rows and each wave its document tile
//                 (MsLds' geometry: f32 k-major with the odd-multiple-of-32 pitch, bf16 row-major at 144 bytes), the next
//                 chunk's global loads are in registers before this chunk's MFMAs, steps in ascending dim order.  Row maxima
//                 merge by the LDS atomicMax on (okey(sim) << 32 | ~position).  A slot row's global row is computed from the
//                 pass's first token (one query per workgroup: no table of rows in LDS).
//   documents     are read again from L2 / HBM in every pass: a wave's tile is not kept in registers across passes.  With
//                 4 or 8 accumulator tiles the register file is full (the table in profiles/), and a document tile at dim
//                 128 would be 32 more registers a lane.
//   finishing     after a pass's last round wave e continues document e's running total through tile_sum over the pass's
//                 tiles, in token order, and writes the pass's match rows.  The total stays in that wave's registers
//                 from pass to pass; the score is written once, after the last pass.
//   key tables    two, in ping-pong: pass ps merges into table ps & 1.  ONE barrier a pass separates its atomics from its
//                 finishing; behind that barrier all threads clear the other table, which was last read by the finishing
//                 of pass ps - 1 (done before its waves reached this barrier) and is next written by the atomics of pass
//                 ps + 1 (behind the barriers of that pass's first chunk).
//   independence  one (query tile, document tile) accumulator adds the same products in the same order as maxsim_kernel's;
//                 the key maximum has no order; the sum runs over the query's tokens in their own order with tile_sum's
//                 additions, carried or not.  A pair's bits are maxsim_kernel's for a query that fits it, and do not depend
//                 on NQT, the passes, WD, the grid, the form or the entry.
#include "np_maxsim_dev.h"

#include <algorithm>

namespace np {

template <int MODE, int NQT> struct MsLongLds {
  using S = MsLds<MODE, NQT>;
  static constexpr size_t KEY_OFF = S::Q_BYTES + 4 * S::D_BYTES;
  static constexpr int TABLE = NP_MS_WG_DOCS * S::R;                // keys of one table: [NP_MS_WG_DOCS][R]
  static constexpr size_t META_OFF = KEY_OFF + 2 * (size_t)TABLE * 8;
  static constexpr size_t BYTES = META_OFF + NP_MS_META;
};

template <int MODE, int NQT>
__global__ void __launch_bounds__(256) maxsim_long_kernel(MaxsimP p) {
  static_assert(MODE >= 0 && MODE <= 2, "f32 and bf16 rows only");
  using S = MsLds<MODE, NQT>;
  using L = MsLongLds<MODE, NQT>;
  constexpr int KC = S::KC, R = S::R, SQ = S::SQ;
  constexpr int EPU = MODE == 0 ? 4 : 8;    // elements per staging unit; a chunk is 8 units per row either way
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, kk = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char* sQ = smem;
  unsigned char* sD = smem + S::Q_BYTES + (size_t)wave * S::D_BYTES;
  unsigned long long* sKey = reinterpret_cast<unsigned long long*>(smem + L::KEY_OFF);   // [2][NP_MS_WG_DOCS][R]
  unsigned long long* sRow = reinterpret_cast<unsigned long long*>(smem + L::META_OFF);  // row entries before this query's pairs
  int64_t* sDoff = reinterpret_cast<int64_t*>(smem + L::META_OFF + 8);                   // [4]
  int64_t* sDlen = sDoff + NP_MS_WG_DOCS;                                               // [4]
  int* sBad = reinterpret_cast<int*>(sDlen + NP_MS_WG_DOCS);                            // [4] id outside [0, n_docs)

  const bool listed = p.pair_docs != nullptr;
  const int query = p.y0 + (int)blockIdx.y;
  const int64_t pbeg = listed ? p.poff[query] : 0;
  const int64_t n = listed ? p.poff[query + 1] - pbeg : p.n_docs;
  const int64_t j0 = (int64_t)blockIdx.x * p.WD;
  if (j0 >= n) return;                      // the whole workgroup, before any barrier
  const int nd = (int)min((int64_t)p.WD, n - j0);
  const int qb = p.qoff[query], Lq = p.qoff[query + 1] - qb;
  const int nqt = (int)(((int64_t)Lq + 31) / 32);
  const int passes = maxsim_long_passes(nqt, NQT);

  if (tid < NP_MS_WG_DOCS) {
    int64_t off = 0, len = 0;
    int bad = 0;
    if (tid < nd) {
      const int64_t doc = listed ? p.pair_docs[pbeg + j0 + tid] : j0 + tid;
      if (doc >= 0 && doc < p.n_docs) {
        off = p.doff[doc];
        len = p.doff[doc + 1] - off;
      } else {
        bad = 1;
      }
    }
    sDoff[tid] = off;
    sDlen[tid] = len;
    sBad[tid] = bad;
  }
  if (tid == 0) *sRow = 0ull;
  for (int i = tid; i < 2 * L::TABLE; i += 256) sKey[i] = 0ull;
  __syncthreads();
  if (listed && (p.sims || p.pos)) {        // row entries of the queries before this one (read after a pass's barrier)
    unsigned long long part = 0;
    for (int i = tid; i < query; i += 256)
      part += (unsigned long long)(p.poff[i + 1] - p.poff[i]) * (unsigned long long)(p.qoff[i + 1] - p.qoff[i]);
    if (part) atomicAdd(sRow, part);
  }

  int64_t tpre[NP_MS_WG_DOCS + 1];          // tiles before document e of this workgroup
  tpre[0] = 0;
#pragma unroll
  for (int e = 0; e < NP_MS_WG_DOCS; ++e) tpre[e + 1] = tpre[e] + (sDlen[e] + 31) / 32;
  const int64_t T = tpre[NP_MS_WG_DOCS];
  const int64_t rounds = (T + 3) / 4;
  const int nchunks = (p.dim + KC - 1) / KC;

  float total = 0.f;                        // the finishing wave's: document `wave`'s sum over the passes so far
  for (int ps = 0; ps < passes; ++ps) {
    const int tile0 = maxsim_long_first(nqt, passes, ps);
    const int nslots = maxsim_long_first(nqt, passes, ps + 1) - tile0;   // <= NQT
    const int64_t tok0 = (int64_t)tile0 * 32;
    unsigned long long* key = sKey + (ps & 1) * L::TABLE;
    // global row of slot row `row` in this pass, -1 = none (past the pass's tiles or past the query's end)
    auto qrow = [&](int row) { return row < nslots * 32 && tok0 + row < Lq ? qb + tok0 + row : (int64_t)-1; };

    for (int64_t rd = 0; rd < rounds; ++rd) {
      const int64_t ti = rd * 4 + wave;     // this wave's tile of the round
      const bool has = ti < T;
      int e = 0;
#pragma unroll
      for (int x = 1; x < NP_MS_WG_DOCS; ++x)
        if (ti >= tpre[x]) e = x;
      int64_t tfirst = tpre[0];
#pragma unroll
      for (int x = 1; x < NP_MS_WG_DOCS; ++x)
        if (e == x) tfirst = tpre[x];
      const int64_t t0 = (ti - tfirst) * 32;
      const int64_t len = has ? sDlen[e] : 0;
      const int64_t drow0 = sDoff[e] + t0;

      f32x16 acc[NQT];
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[qt][r] = 0;

      MsRaw<MODE> rq[NQT], rdoc[4];
      auto load_chunk = [&](int c) {
        const int kc0 = c * KC;
#pragma unroll
        for (int i = 0; i < NQT; ++i) {
          int row, g;
          ms_unit<MODE>(tid + 256 * i, R, row, g);
          rq[i] = ms_load<MODE>(p.Q, qrow(row), p.dim, kc0 + g * EPU, p.vecq != 0);
        }
        if (has) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            int row, g;
            ms_unit<MODE>(lane + 64 * i, 32, row, g);
            rdoc[i] = ms_load<MODE>(p.D, t0 + row < len ? drow0 + row : (int64_t)-1, p.dim, kc0 + g * EPU, p.vecd != 0);
          }
        }
      };
      load_chunk(0);
      for (int c = 0; c < nchunks; ++c) {
        __syncthreads();                    // the previous chunk's fragments have been read (also the previous pass's)
#pragma unroll
        for (int i = 0; i < NQT; ++i) {
          int row, g;
          ms_unit<MODE>(tid + 256 * i, R, row, g);
          ms_store<MODE>(sQ, SQ, row, g, rq[i]);
        }
        if (has) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            int row, g;
            ms_unit<MODE>(lane + 64 * i, 32, row, g);
            ms_store<MODE>(sD, 32, row, g, rdoc[i]);
          }
        }
        __syncthreads();
        if (c + 1 < nchunks) load_chunk(c + 1);   // in flight during this chunk's MFMAs
        if (!has) continue;
        // the steps of this chunk in ascending dim order
        const float* df = reinterpret_cast<const float*>(sD) + kk * 32 + li;
        const float* qf = reinterpret_cast<const float*>(sQ) + kk * SQ + li;
        const unsigned char* dh = sD + ((size_t)li * NP_MS_BROW + 8 * kk) * 2;
        const unsigned char* qh = sQ + ((size_t)li * NP_MS_BROW + 8 * kk) * 2;
        auto step = [&](int s) {
          if constexpr (MODE == 0) {
            const float a = df[2 * s * 32];
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt)
              if (qt < nslots) acc[qt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, qf[2 * s * SQ + qt * 32], acc[qt], 0, 0, 0);
          } else {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(dh + 32 * s);
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt)
              if (qt < nslots)
                acc[qt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    a, *reinterpret_cast<const bf16x8*>(qh + (size_t)qt * 32 * NP_MS_BROW * 2 + 32 * s), acc[qt], 0, 0, 0);
          }
        };
        // four steps at a time; dims past `dim` are zeros on both sides, so the steps past dim's own last one add exact zeros
        constexpr int STEP = MODE == 0 ? 2 : 16;
        constexpr int GS = 4;   // steps per group
        const int ng = (min(KC, p.dim - c * KC) + GS * STEP - 1) / (GS * STEP);
#pragma unroll 1
        for (int s4 = 0; s4 < ng; ++s4) {
#pragma unroll
          for (int s = 0; s < GS; ++s) step(GS * s4 + s);
        }
      }
      if (has) {
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
          if (qt < nslots) {
            float m = NP_NEG_INF;
            int pos = -1;
            ms_row_argmax(acc[qt], t0, len, kk, m, pos);
            if (pos >= 0)
              atomicMax(&key[e * R + qt * 32 + li], ((unsigned long long)okey(m) << 32) | (0xFFFFFFFFu - (uint32_t)pos));
          }
          __builtin_amdgcn_sched_barrier(0);   // one accumulator tile out of the AGPRs at a time
        }
      }
    }
    __syncthreads();                        // the pass's one barrier between its atomics and its finishing
    if (ps + 1 < passes) {                  // the other table: read last before this barrier, merged into after the next pass's
      unsigned long long* other = sKey + ((ps + 1) & 1) * L::TABLE;
      for (int i = tid; i < L::TABLE; i += 256) other[i] = 0ull;
    }
    if (wave < nd) {
      // wave e continues document e's q-ordered sum of the maxima (tile_sum's rule) over this pass's tiles, and writes their matches
      const int e = wave;
      const int64_t rowb = (listed ? (int64_t)*sRow : p.n_docs * (int64_t)qb) + (j0 + e) * (int64_t)Lq;
      for (int t = 0; t < nslots; ++t) {
        const unsigned long long k = key[e * R + t * 32 + li];
        const float m = k ? unkey((uint32_t)(k >> 32)) : NP_NEG_INF;
        const int64_t tq = tok0 + t * 32 + li;
        total = tile_sum(m, (int)min((int64_t)32, Lq - (tok0 + t * 32)), total);
        if (kk == 0 && tq < Lq) {
          if (p.sims) p.sims[rowb + tq] = k ? m : 0.0f;
          if (p.pos) p.pos[rowb + tq] = k ? (int32_t)(0xFFFFFFFFu - (uint32_t)k) : -1;
        }
      }
    }
  }
  if (wave < nd && lane == 0) {
    const int64_t out = listed ? pbeg + j0 + wave : (int64_t)query * p.n_docs + j0 + wave;
    p.scores[out] = sBad[wave] != 0 ? __uint_as_float(0x7FC00000u) : total;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
template <int MODE, int NQT>
static int maxsim_long_launch_one(hipStream_t st, MaxsimP p, const MaxsimLongPlan& plan) {
  const size_t lds = MsLongLds<MODE, NQT>::BYTES;
  if (lds > 48 * 1024)
    NP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&maxsim_long_kernel<MODE, NQT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int64_t y0 = 0; y0 < plan.gy; y0 += NP_MS_MAX_GRID_Y) {
    p.y0 = (int)y0;
    const dim3 grid((unsigned)plan.gx, (unsigned)std::min<int64_t>(NP_MS_MAX_GRID_Y, plan.gy - y0));
    maxsim_long_kernel<MODE, NQT><<<grid, 256, lds, st>>>(p);
  }
  NP_HIP(hipGetLastError());
  return NP_OK;
}

template <int MODE>
static int maxsim_long_launch_mode(hipStream_t st, const MaxsimP& p, const MaxsimLongPlan& plan) {
  switch (plan.NQT) {
    case 1: return maxsim_long_launch_one<MODE, 1>(st, p, plan);
    case 2: return maxsim_long_launch_one<MODE, 2>(st, p, plan);
    case 4: return maxsim_long_launch_one<MODE, 4>(st, p, plan);
    default:
      if constexpr (MODE != 0) return maxsim_long_launch_one<MODE, 8>(st, p, plan);
      set_error("Search failed: maxsim_batch_long: no f32 kernel of %d slots", plan.NQT);   // maxsim_long_plan never asks for one
      return NP_ERR_INVALID_ARGUMENT;
  }
}

int maxsim_long_launch(hipStream_t st, MaxsimP p, const MaxsimLongPlan& plan, int mode) {
  if (mode == 0) return maxsim_long_launch_mode<0>(st, p, plan);
  if (mode == 1) return maxsim_long_launch_mode<1>(st, p, plan);
  return maxsim_long_launch_mode<2>(st, p, plan);
}

static int maxsim_validate_long(int32_t dtype, int32_t precision, int32_t dim, int32_t B, const int32_t* h_qoff, int64_t n_docs,
                                const int64_t* h_doff, bool listed, const int64_t* h_pair_docs, const int64_t* h_poff,
                                bool want_matches) {
  const char* why = "";
  int64_t bad = -1;
  const int c = maxsim_check_args_long(dtype, precision, dim, B, h_qoff, n_docs, h_doff, listed, h_pair_docs, h_poff,
                                       want_matches, &why, &bad);
  if (c == 0) return NP_OK;
  if (bad >= 0)
    set_error("maxsim_batch_long: %s (pair %lld names document %lld, n_docs %lld)", why, (long long)bad,
              (long long)h_pair_docs[bad], (long long)n_docs);
  else
    set_error("%s: maxsim_batch_long: %s (dtype=%d precision=%d dim=%d)", c == 1 ? "Shape error" : "Search failed", why, dtype,
              precision, dim);
  return c == 1 ? NP_ERR_SHAPE : NP_ERR_INVALID_ARGUMENT;
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_maxsim_batch_long_device(int32_t device, int32_t dtype, int32_t precision, int32_t dim, const void* d_queries,
                                    const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                                    const void* d_documents, const int64_t* d_doc_tok_offsets,
                                    const int64_t* h_doc_tok_offsets, int64_t n_docs, const int64_t* d_pair_docs,
                                    const int64_t* d_pair_offsets, const int64_t* h_pair_offsets, float* d_out_scores,
                                    float* d_out_match_sims, int32_t* d_out_match_pos, void* stream) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(d_pair_docs && d_pair_offsets && h_pair_offsets, d_pair_docs || d_pair_offsets || h_pair_offsets, true,
                          &listed));
  NP_TRY(maxsim_validate_long(dtype, precision, dim, B, h_q_tok_offsets, n_docs, h_doc_tok_offsets, listed, nullptr,
                              h_pair_offsets, d_out_match_sims || d_out_match_pos));
  return maxsim_device_call(device, dtype, precision, dim, d_queries, nullptr, d_q_tok_offsets, h_q_tok_offsets, B, d_documents,
                            nullptr, d_doc_tok_offsets, h_doc_tok_offsets, n_docs, d_pair_docs, d_pair_offsets, h_pair_offsets,
                            d_out_scores, d_out_match_sims, d_out_match_pos, stream, true);
}

int np_hip_maxsim_batch_long(int32_t device, int32_t dtype, int32_t precision, int32_t dim, const void* queries,
                             const int32_t* q_tok_offsets, int32_t B, const void* documents, const int64_t* doc_tok_offsets,
                             int64_t n_docs, const int64_t* pair_docs, const int64_t* pair_offsets, float* out_scores,
                             float* out_match_sims, int32_t* out_match_pos) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(pair_docs && pair_offsets, pair_docs || pair_offsets, false, &listed));
  NP_TRY(maxsim_validate_long(dtype, precision, dim, B, q_tok_offsets, n_docs, doc_tok_offsets, listed, pair_docs, pair_offsets,
                              out_match_sims || out_match_pos));
  return maxsim_host_call(device, dtype, precision, dim, queries, nullptr, q_tok_offsets, B, documents, nullptr, doc_tok_offsets,
                          n_docs, pair_docs, pair_offsets, out_scores, out_match_sims, out_match_pos, true);
}

}  // extern "C"
