// np_maxsim_long_i8.hip -- np_hip_maxsim_batch_long_i8: np_hip_maxsim_batch_i8 (np_maxsim.hip, MODE 3) for queries of any
// length.  Rows of int8 codes with one f32 scale per row on both sides, v_mfma_i32_32x32x32_i8, and the arithmetic of MODE 3 bit
// for bit (tests/maxsim_i8_restate.py pair(), which has no token limit): the exact i32 dot, f32(dot) * d_scale[t] with one
// rounding, the maximum in okey order with the lowest position, * q_scale[q] with one more rounding and a non-finite product
// dropped, the f32 sum in query-token order.
//
// A kernel of its own, not a mode of maxsim_long_kernel: an int8 row is a quarter of the f32 bytes, so a whole pass of query
// rows fits LDS at its full width and nothing has to stream through LDS in chunks.
//
//   work split    maxsim_long_kernel's: blockIdx.y = one query, blockIdx.x = WD <= 4 documents (all pairs) or WD consecutive
//                 pairs of the query's list; 4 waves; the documents' 32-token tiles go round-robin to the waves; the query is
//                 walked in even passes of at most NQT tiles (maxsim_long_passes / _first); two key tables in ping-pong; wave
//                 e carries document e's ordered total in registers from pass to pass.  The wave index lives in a scalar
//                 register from the first line.
//   query rows    a pass's rows are RESIDENT: staged once per pass by all 256 threads, `dim` bytes a row at a pitch of an odd
//                 number of 16-byte units that covers dim rounded up to 32 (maxsim_long_i8_pitch), bytes past dim zero; 16-byte
//                 global loads where base and dim allow, byte loads otherwise (ms_load16b).  The pass width follows from dim:
//                 SPmax(dim) = the widest of 8, 4, 2, 1 tiles whose rows, key tables and meta block fit NP_MS_LONG_I8_BUDGET
//                 (np_maxsim_plan.h: 80 KB, two workgroups per compute unit; dim 1024 keeps 2 tiles).
//   documents     never in LDS.  Lane (li, kk) owns row li of its wave's tile and loads the A fragments of a 128-dim chunk
//                 from global memory into 4 registers each: step s is the 16 bytes at byte 16 kk + 32 s of the chunk, MODE 3's
//                 split of a step, and the B fragment is the same 16 bytes of the slot row in LDS.  Nothing at or past dim is
//                 read; rows past a tile's end are zeros; steps wholly past dim are skipped.  The next chunk's -- or the next
//                 tile's first chunk's -- 16 registers are requested before the current chunk's MFMAs.  Which 16 of a step's
//                 32 dims a half-wave holds does not matter: both operands split alike and the i32 sum is exact.
//   scales        both half-waves load their row's document scale with the tile's first chunk; the epilogue brings the 16
//                 scales of a lane's accumulator rows mfma_row(r, kk) over by lane shuffles (np_exact.h row_scales' way).
//   barriers      none inside a pass's round loop: a wave reads the resident rows and its own registers.  A pass has two: one
//                 behind its staging, one between its atomicMax merges and its finishing -- which is also the one before the
//                 next pass's staging, as every wave has then read this pass's rows for the last time.  A 1030-token page
//                 against 1030-token pages at dim 128 is 5 passes: 11 barriers, the one behind the meta block included.
//   key tables    pass ps merges into table ps & 1; behind the pass's second barrier all threads clear the other table (last
//                 read by the finishing of pass ps - 1, next merged into behind the first barrier of pass ps + 1).
//   independence  one (query tile, document tile) accumulator is an exact integer whatever the split; the key maximum has no
//                 order; the sum runs over the query's tokens in their own order with tile_sum's additions, carried or not.  A
//                 pair's bits are maxsim_kernel<3, .>'s for a query that fits it and do not depend on NQT, the passes, WD, the
//                 grid, the form or the entry.
#include "np_maxsim_dev.h"

#include <algorithm>

namespace np {

static_assert(NP_MS_LONG_I8_META == NP_MS_META, "one meta block for every batched-MaxSim kernel");

struct I8Frag {
  uint4 v[4];   // a lane's 16 bytes of each of a chunk's four steps: the A fragments
};

struct I8Tile {
  int e;                    // document of the workgroup
  int64_t t0, len, drow0;   // first token of the tile, the document's length (0 = no tile), the tile's first global row
};

template <int NQT>
__global__ void __launch_bounds__(256) maxsim_long_i8_kernel(MaxsimP p) {
  constexpr int R = NQT * 32, TABLE = NP_MS_WG_DOCS * R;
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, kk = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pitch = maxsim_long_i8_pitch(p.dim);
  unsigned char* sQ = smem;                                                                                      // [R][pitch]
  unsigned long long* sKey = reinterpret_cast<unsigned long long*>(smem + maxsim_long_i8_key_off(p.dim, NQT));    // [2][NP_MS_WG_DOCS][R]
  unsigned char* meta = smem + maxsim_long_i8_meta_off(p.dim, NQT);
  unsigned long long* sRow = reinterpret_cast<unsigned long long*>(meta);   // row entries before this query's pairs
  int64_t* sDoff = reinterpret_cast<int64_t*>(meta + 8);                    // [4]
  int64_t* sDlen = sDoff + NP_MS_WG_DOCS;                                   // [4]
  int* sBad = reinterpret_cast<int*>(sDlen + NP_MS_WG_DOCS);                // [4] id outside [0, n_docs)

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
  for (int i = tid; i < 2 * TABLE; i += 256) sKey[i] = 0ull;
  __syncthreads();
  if (listed && (p.sims || p.pos)) {        // row entries of the queries before this one (read after a pass's second barrier)
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
  const int nchunks = (p.dim + NP_MS_KC_I8 - 1) / NP_MS_KC_I8;
  const uint8_t* Q = static_cast<const uint8_t*>(p.Q);
  const uint8_t* D = static_cast<const uint8_t*>(p.D);

  auto tile_of = [&](int64_t rd) {          // this wave's tile of round rd (past the last tile: len 0)
    const int64_t ti = rd * 4 + wave;
    I8Tile t;
    t.e = 0;
#pragma unroll
    for (int x = 1; x < NP_MS_WG_DOCS; ++x)
      if (ti >= tpre[x]) t.e = x;
    int64_t tfirst = tpre[0];
#pragma unroll
    for (int x = 1; x < NP_MS_WG_DOCS; ++x)
      if (t.e == x) tfirst = tpre[x];
    t.t0 = (ti - tfirst) * 32;
    t.len = ti < T ? sDlen[t.e] : 0;
    t.drow0 = sDoff[t.e] + t.t0;
    return t;
  };
  auto load_frag = [&](const I8Tile& t, int c) {   // this lane's bytes of row li's chunk c (zeros for a row past the end)
    const uint8_t* rowp = t.t0 + li < t.len ? D + (t.drow0 + li) * p.dim : nullptr;
    I8Frag f;
#pragma unroll
    for (int s = 0; s < 4; ++s) f.v[s] = ms_load16b(rowp, c * NP_MS_KC_I8 + 32 * s + 16 * kk, p.dim, p.vecd != 0);
    return f;
  };
  auto load_scale = [&](const I8Tile& t) { return t.t0 + li < t.len ? p.dscale[t.drow0 + li] : 0.f; };

  float total = 0.f;                        // the finishing wave's: document `wave`'s sum over the passes so far
  for (int ps = 0; ps < passes; ++ps) {
    const int tile0 = maxsim_long_first(nqt, passes, ps);
    const int nslots = maxsim_long_first(nqt, passes, ps + 1) - tile0;   // <= NQT
    const int64_t tok0 = (int64_t)tile0 * 32;
    unsigned long long* key = sKey + (ps & 1) * TABLE;

    // the wave's first tile is on its way while the pass's rows are staged
    I8Tile cur = tile_of(0);
    I8Frag fcur = load_frag(cur, 0);
    float scur = load_scale(cur);
    {
      // unit u = 16 bytes at byte 16 u of the rows' region: row u / upr, dims 16 (u % upr) ..; four units a thread in flight
      const int upr = pitch >> 4, units = nslots * 32 * upr;
      for (int u0 = tid; u0 < units; u0 += 4 * 256) {
        uint4 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int u = u0 + 256 * i, row = u / upr, g = u - row * upr;
          const bool in = u < units && tok0 + row < Lq;   // rows past the query's end are zeros
          v[i] = ms_load16b(in ? Q + (qb + tok0 + row) * p.dim : nullptr, 16 * g, p.dim, p.vecq != 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (u0 + 256 * i < units) *reinterpret_cast<uint4*>(sQ + (size_t)(u0 + 256 * i) * 16) = v[i];
      }
    }
    __syncthreads();                        // the pass's rows are there

    for (int64_t rd = 0; rd < rounds; ++rd) {
      const bool has = cur.len > 0;
      i32x16 acc[NQT];
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[qt][r] = 0;
      I8Tile nxt = cur;
      float snext = 0.f;
      for (int c = 0; c < nchunks; ++c) {
        const bool lastc = c + 1 == nchunks;
        if (lastc) nxt = tile_of(rd + 1);
        const I8Frag fnext = load_frag(nxt, lastc ? 0 : c + 1);   // in flight during this chunk's MFMAs
        if (lastc) snext = load_scale(nxt);
        if (has) {
          const unsigned char* qh = sQ + (size_t)li * pitch + c * NP_MS_KC_I8 + 16 * kk;
          const int nsteps = (min(NP_MS_KC_I8, p.dim - c * NP_MS_KC_I8) + 31) / 32;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            if (s < nsteps) {
              const i32x4 a = __builtin_bit_cast(i32x4, fcur.v[s]);
#pragma unroll
              for (int qt = 0; qt < NQT; ++qt)
                if (qt < nslots)
                  acc[qt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(
                      a, *reinterpret_cast<const i32x4*>(qh + (size_t)qt * 32 * pitch + 32 * s), acc[qt], 0, 0, 0);
            }
          }
        }
        fcur = fnext;
      }
      if (has) {                            // the same for the whole wave
        float sc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = __shfl(scur, mfma_row(r, kk));
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
          if (qt < nslots) {
            uint32_t best = 0u;
            int pos = -1;
            ms_row_argmax_i8(acc[qt], sc, cur.t0, cur.len, kk, best, pos);
            if (best) atomicMax(&key[cur.e * R + qt * 32 + li], ((unsigned long long)best << 32) | (0xFFFFFFFFu - (uint32_t)pos));
          }
          __builtin_amdgcn_sched_barrier(0);   // one accumulator tile out of the AGPRs at a time
        }
      }
      cur = nxt;
      scur = snext;
    }
    __syncthreads();                        // between the pass's atomics and its finishing; its rows have been read
    if (ps + 1 < passes) {                  // the other table: read last before this barrier, merged into after the next pass's first
      unsigned long long* other = sKey + ((ps + 1) & 1) * TABLE;
      for (int i = tid; i < TABLE; i += 256) other[i] = 0ull;
    }
    if (wave < nd) {
      // wave e continues document e's q-ordered sum of the maxima (tile_sum's rule) over this pass's tiles, and writes their matches
      const int e = wave;
      const int64_t rowb = (listed ? (int64_t)*sRow : p.n_docs * (int64_t)qb) + (j0 + e) * (int64_t)Lq;
      for (int t = 0; t < nslots; ++t) {
        unsigned long long k = key[e * R + t * 32 + li];
        float m = k ? unkey((uint32_t)(k >> 32)) : NP_NEG_INF;
        const int64_t tq = tok0 + t * 32 + li;
        if (k) {                            // the query token's scale, one multiplication; not finite = no match
          m *= p.qscale[qb + min(tq, (int64_t)Lq - 1)];
          if (!finitef(m)) k = 0ull, m = NP_NEG_INF;
        }
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
template <int NQT>
static int maxsim_long_i8_launch_one(hipStream_t st, MaxsimP p, const MaxsimLongPlan& plan) {
  const size_t lds = maxsim_long_i8_lds(p.dim, NQT);   // <= NP_MS_LONG_I8_BUDGET: NQT <= SPmax(dim)
  if (lds > 48 * 1024)
    NP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&maxsim_long_i8_kernel<NQT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int64_t y0 = 0; y0 < plan.gy; y0 += NP_MS_MAX_GRID_Y) {
    p.y0 = (int)y0;
    const dim3 grid((unsigned)plan.gx, (unsigned)std::min<int64_t>(NP_MS_MAX_GRID_Y, plan.gy - y0));
    maxsim_long_i8_kernel<NQT><<<grid, 256, lds, st>>>(p);
  }
  NP_HIP(hipGetLastError());
  return NP_OK;
}

int maxsim_long_i8_launch(hipStream_t st, MaxsimP p, const MaxsimLongPlan& plan) {
  if (plan.NQT > maxsim_long_i8_spmax(p.dim)) {   // maxsim_long_i8_plan never asks for one
    set_error("Search failed: maxsim_batch_long_i8: no kernel of %d slots at dim %d", plan.NQT, p.dim);
    return NP_ERR_INVALID_ARGUMENT;
  }
  switch (plan.NQT) {
    case 1: return maxsim_long_i8_launch_one<1>(st, p, plan);
    case 2: return maxsim_long_i8_launch_one<2>(st, p, plan);
    case 4: return maxsim_long_i8_launch_one<4>(st, p, plan);
    default: return maxsim_long_i8_launch_one<8>(st, p, plan);
  }
}

static int maxsim_validate_long_i8(int32_t dim, const void* q_scales, int32_t B, const int32_t* h_qoff, const void* d_scales,
                                   int64_t n_docs, const int64_t* h_doff, bool listed, const int64_t* h_pair_docs,
                                   const int64_t* h_poff) {
  const char* why = "";
  int64_t bad = -1;
  const int c = maxsim_check_args_long_i8(dim, q_scales, B, h_qoff, d_scales, n_docs, h_doff, listed, h_pair_docs, h_poff, &why,
                                          &bad);
  if (c == 0) return NP_OK;
  if (bad >= 0)
    set_error("maxsim_batch_long_i8: %s (pair %lld names document %lld, n_docs %lld)", why, (long long)bad,
              (long long)h_pair_docs[bad], (long long)n_docs);
  else
    set_error("%s: maxsim_batch_long_i8: %s (dim=%d)", c == 1 ? "Shape error" : "Search failed", why, dim);
  return c == 1 ? NP_ERR_SHAPE : NP_ERR_INVALID_ARGUMENT;
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_maxsim_batch_long_i8_device(int32_t device, int32_t dim, const int8_t* d_queries, const float* d_q_scales,
                                       const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                                       const int8_t* d_documents, const float* d_d_scales, const int64_t* d_doc_tok_offsets,
                                       const int64_t* h_doc_tok_offsets, int64_t n_docs, const int64_t* d_pair_docs,
                                       const int64_t* d_pair_offsets, const int64_t* h_pair_offsets, float* d_out_scores,
                                       float* d_out_match_sims, int32_t* d_out_match_pos, void* stream) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(d_pair_docs && d_pair_offsets && h_pair_offsets, d_pair_docs || d_pair_offsets || h_pair_offsets, true,
                          &listed));
  NP_TRY(maxsim_validate_long_i8(dim, d_q_scales, B, h_q_tok_offsets, d_d_scales, n_docs, h_doc_tok_offsets, listed, nullptr,
                                 h_pair_offsets));
  return maxsim_device_call(device, NP_MS_DT_I8, 0, dim, d_queries, d_q_scales, d_q_tok_offsets, h_q_tok_offsets, B, d_documents,
                            d_d_scales, d_doc_tok_offsets, h_doc_tok_offsets, n_docs, d_pair_docs, d_pair_offsets, h_pair_offsets,
                            d_out_scores, d_out_match_sims, d_out_match_pos, stream, true);
}

int np_hip_maxsim_batch_long_i8(int32_t device, int32_t dim, const int8_t* queries, const float* q_scales,
                                const int32_t* q_tok_offsets, int32_t B, const int8_t* documents, const float* d_scales,
                                const int64_t* doc_tok_offsets, int64_t n_docs, const int64_t* pair_docs,
                                const int64_t* pair_offsets, float* out_scores, float* out_match_sims, int32_t* out_match_pos) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(pair_docs && pair_offsets, pair_docs || pair_offsets, false, &listed));
  NP_TRY(maxsim_validate_long_i8(dim, q_scales, B, q_tok_offsets, d_scales, n_docs, doc_tok_offsets, listed, pair_docs,
                                 pair_offsets));
  return maxsim_host_call(device, NP_MS_DT_I8, 0, dim, queries, q_scales, q_tok_offsets, B, documents, d_scales, doc_tok_offsets,
                          n_docs, pair_docs, pair_offsets, out_scores, out_match_sims, out_match_pos, true);
}

}  // extern "C"
