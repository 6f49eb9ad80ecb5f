// np_maxsim_i4.hip -- np_hip_maxsim_batch_i4: MaxSim of int8 query rows against INT4 document rows, eight two's-complement
// nibbles per 32-bit word with one f32 scale per row, on v_mfma_i32_32x32x32_i8.  A document row of dim 128 is 64 bytes:
// it never touches LDS.  Every step is exact or one f32 rounding: tests/maxsim_i8_restate.py pair() on the unpacked nibbles.
//
//   work split    maxsim_b1_kernel's (np_maxsim_b1.hip): 4 waves, up to 8 query slots of 32 tokens and up to WD <= 4 documents
//                 per workgroup by maxsim_plan; the 32-token tiles of the documents go round-robin to the waves; row maxima
//                 merge by an LDS atomicMax on (okey << 32 | ~position); wave e forms document e's q-ordered sum and
//                 multiplies by the query scale.  The wave index lives in a scalar register from the first line.
//   documents     lane (li, kk) owns row li of its wave's tile and HALF of the row's chunk: words 8 kk .. 8 kk + 7 of the
//                 chunk's 16, dims 64 kk .. 64 kk + 63, from global memory into registers -- two 16-byte loads where every
//                 row allows it (W % 4 == 0 and an aligned base), dword loads otherwise; words at or past W are not read.
//                 The next chunk's (or next round's) words are requested before the current MFMAs.  Step s takes the lane's
//                 words 2 s and 2 s + 1, dims 64 kk + 16 s .. + 15: an integer sum does not care which 16 of a step's 32 dims
//                 a half-wave holds as long as the query fragment splits alike.
//   expansion     per word  hi = w & 0xF0F0F0F0  (dims 1, 3, 5, 7)  and  lo = (w << 4) & 0xF0F0F0F0  (dims 0, 2, 4, 6): each
//                 code sits in the high nibble of its byte, which as a signed byte is 16 * code, no sign extension.  The A
//                 fragment of a step is {lo(w0), hi(w0), lo(w1), hi(w1)}: 6 VALU operations for 16 dims, shared by all
//                 slots.  The accumulator holds 16 * dot, |16 * dot| <= 1024 * 128 * 128 = 2^24, exact; the epilogue shifts
//                 it right by 4 (exact: a multiple of 16) before the f32 conversion, so the scale multiplies f32(dot).
//   query slots   int8 rows in LDS in MODE 3's geometry (128-dim chunk, rows 144 bytes apart), but DEINTERLEAVED to the
//                 fragment's byte order when a chunk is staged: within each 8 bytes dims 0, 2, 4, 6, 1, 3, 5, 7, two v_perm_b32
//                 per 8 bytes at staging and nothing per tile.  A lane's B fragment is the 16 bytes at row li, byte
//                 64 kk + 16 s.  Dims past `dim` are staged as zeros (pad nibbles multiply them); steps past dim are skipped.
//                 dim <= 128: staged once, the rounds have no barrier.  dim > 128: the slot chunk is double buffered for up
//                 to 4 slots with ONE barrier per chunk, exactly as maxsim_b1_kernel; 8 slots keep one buffer.
//   scales        lane li reads its row's scale from global memory when the round starts; the epilogue fetches the 16
//                 scales of rows mfma_row(r, kk) by wave shuffles and walks ms_row_argmax_i8.
#include "np_maxsim_dev.h"

namespace np {

template <int NQT> struct MsI4Lds {
  static constexpr int R = NQT * 32;                                // slot rows
  static constexpr bool DBL = NQT < 8;                              // two slot buffers when dim > 128
  static constexpr size_t Q_BYTES = (size_t)R * NP_MS_BROW * 2;     // one buffer
  static constexpr size_t KEY_OFF = (DBL ? 2 : 1) * Q_BYTES;
  static constexpr size_t QROW_OFF = KEY_OFF + (size_t)NP_MS_WG_DOCS * R * 8;
  static constexpr size_t META_OFF = QROW_OFF + (size_t)R * 8;
  static constexpr size_t BYTES = META_OFF + NP_MS_META;
};

constexpr int NP_MS_I4_CW = NP_MS_KC_I8 / 8;   // words of a row per chunk

struct I4Words {
  uint4 a, b;   // a lane's eight words of a chunk: 64 dims
};

// words w0 .. w0 + 7 of a nibble row (NULL = a row past the end), zeros at and past W
__device__ __forceinline__ I4Words i4_load_words(const uint32_t* rowp, int w0, int W, bool vec) {
  I4Words r;
  r.a = r.b = make_uint4(0u, 0u, 0u, 0u);
  if (!rowp || w0 >= W) return r;
  if (vec) {                                   // W % 4 == 0: w0 + 4 <= W, and w0 + 8 <= W when w0 + 4 < W
    r.a = *reinterpret_cast<const uint4*>(rowp + w0);
    if (w0 + 4 < W) r.b = *reinterpret_cast<const uint4*>(rowp + w0 + 4);
    return r;
  }
  uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (w0 + i < W) w[i] = rowp[w0 + i];
  r.a = make_uint4(w[0], w[1], w[2], w[3]);
  r.b = make_uint4(w[4], w[5], w[6], w[7]);
  return r;
}

// sixteen nibbles of two words as sixteen int8 of 16 * code, in the order 0 2 4 6 1 3 5 7 within each word
__device__ __forceinline__ i32x4 i4_expand(uint32_t w0, uint32_t w1) {
  i32x4 a;
  a[0] = (int)((w0 << 4) & 0xF0F0F0F0u);
  a[1] = (int)(w0 & 0xF0F0F0F0u);
  a[2] = (int)((w1 << 4) & 0xF0F0F0F0u);
  a[3] = (int)(w1 & 0xF0F0F0F0u);
  return a;
}

// sixteen query bytes into i4_expand's order: per 8 bytes the even dims, then the odd ones
__device__ __forceinline__ uint4 i4_deinterleave(uint4 v) {
  return make_uint4(__builtin_amdgcn_perm(v.y, v.x, 0x06040200u), __builtin_amdgcn_perm(v.y, v.x, 0x07050301u),
                    __builtin_amdgcn_perm(v.w, v.z, 0x06040200u), __builtin_amdgcn_perm(v.w, v.z, 0x07050301u));
}

struct I4Tile {
  int e;                    // document of the workgroup
  int64_t t0, len, drow0;   // first token of the tile, the document's length (0 = no tile), the tile's first global row
};

template <int NQT>
__global__ void __launch_bounds__(256) maxsim_i4_kernel(MaxsimP p) {
  using L = MsI4Lds<NQT>;
  constexpr int R = L::R;
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, kk = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char* sQ = smem;
  unsigned long long* sKey = reinterpret_cast<unsigned long long*>(smem + L::KEY_OFF);   // [NP_MS_WG_DOCS][R]
  int64_t* sQrow = reinterpret_cast<int64_t*>(smem + L::QROW_OFF);                      // [R] global row of a slot row, -1 = none
  unsigned long long* sRow = reinterpret_cast<unsigned long long*>(smem + L::META_OFF);  // row entries before this query's pairs
  int64_t* sDoff = reinterpret_cast<int64_t*>(smem + L::META_OFF + 8);                   // [4]
  int64_t* sDlen = sDoff + NP_MS_WG_DOCS;                                               // [4]
  int* sBad = reinterpret_cast<int*>(sDlen + NP_MS_WG_DOCS);                            // [4] id outside [0, n_docs)

  const bool listed = p.pair_docs != nullptr;
  const int by = p.y0 + (int)blockIdx.y;
  const int qg0 = listed ? by : by * p.G;
  const int nq = listed ? 1 : min(p.G, p.B - qg0);
  const int64_t pbeg = listed ? p.poff[qg0] : 0;
  const int64_t n = listed ? p.poff[qg0 + 1] - pbeg : p.n_docs;
  const int64_t j0 = (int64_t)blockIdx.x * p.WD;
  if (j0 >= n) return;                      // the whole workgroup, before any barrier
  const int nd = (int)min((int64_t)p.WD, n - j0);
  const int nslots = p.G * p.nqt;           // <= NQT

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
  for (int r = tid; r < R; r += 256) {
    const int slot = r >> 5, s = slot / p.nqt, t = slot - s * p.nqt;
    int64_t grow = -1;
    if (s < nq && slot < nslots) {
      const int qb = p.qoff[qg0 + s], lq = p.qoff[qg0 + s + 1] - qb;
      const int tok = t * 32 + (r & 31);
      if (tok < lq) grow = qb + tok;
    }
    sQrow[r] = grow;
  }
  for (int i = tid; i < NP_MS_WG_DOCS * R; i += 256) sKey[i] = 0ull;
  __syncthreads();
  if (listed && (p.sims || p.pos)) {        // row entries of the queries before this one (read after the last barrier)
    unsigned long long part = 0;
    for (int i = tid; i < qg0; i += 256)
      part += (unsigned long long)(p.poff[i + 1] - p.poff[i]) * (unsigned long long)(p.qoff[i + 1] - p.qoff[i]);
    if (part) atomicAdd(sRow, part);
  }

  int64_t tpre[NP_MS_WG_DOCS + 1];          // tiles before document e of this workgroup
  tpre[0] = 0;
#pragma unroll
  for (int e = 0; e < NP_MS_WG_DOCS; ++e) tpre[e + 1] = tpre[e] + (sDlen[e] + 31) / 32;
  const int64_t T = tpre[NP_MS_WG_DOCS];
  const int64_t rounds = (T + 3) / 4;
  const int W = (p.dim + 7) / 8;
  const int nchunks = (p.dim + NP_MS_KC_I8 - 1) / NP_MS_KC_I8;
  const bool resident = nchunks == 1;       // the slots are staged once; the rounds then touch no shared memory but the keys

  auto tile_of = [&](int64_t rd) {          // this wave's tile of round rd
    const int64_t ti = rd * 4 + wave;
    I4Tile t;
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
  auto load_words = [&](const I4Tile& t, int c) {   // this lane's half of row li's chunk c (zeros for a row past the end)
    const bool row = t.t0 + li < t.len;
    return i4_load_words(row ? static_cast<const uint32_t*>(p.D) + (t.drow0 + li) * W : nullptr, NP_MS_I4_CW * c + 8 * kk, W,
                         p.vecd != 0);
  };
  uint4 rq[NQT];                            // a slot chunk on its way from HBM to LDS: unit (row u >> 3, 16 bytes at 16 (u & 7))
  auto load_q = [&](int c) {
#pragma unroll
    for (int i = 0; i < NQT; ++i) {
      const int u = tid + 256 * i;
      const int64_t grow = sQrow[u >> 3];
      rq[i] = ms_load16b(grow < 0 ? nullptr : static_cast<const uint8_t*>(p.Q) + grow * p.dim, c * NP_MS_KC_I8 + 16 * (u & 7), p.dim,
                         p.vecq != 0);
    }
  };
  auto store_q = [&](unsigned char* buf) {  // the permutation stays inside a unit: the unit keeps its place
#pragma unroll
    for (int i = 0; i < NQT; ++i) {
      const int u = tid + 256 * i;
      *reinterpret_cast<uint4*>(buf + (size_t)(u >> 3) * NP_MS_BROW * 2 + 16 * (u & 7)) = i4_deinterleave(rq[i]);
    }
  };

  I4Tile cur = tile_of(0);
  I4Words wcur = load_words(cur, 0);
  load_q(0);
  store_q(sQ);
  __syncthreads();
  int buf = 0;                              // the slot buffer that holds the current chunk
  for (int64_t rd = 0; rd < rounds; ++rd) {
    const bool has = cur.len > 0;
    i32x16 acc[NQT];
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[qt][r] = 0;
    const float dsc = cur.t0 + li < cur.len ? p.dscale[cur.drow0 + li] : 0.f;   // read back by shuffles in the epilogue
    I4Tile nxt = cur;
    for (int c = 0; c < nchunks; ++c) {
      const bool lastc = c + 1 == nchunks;
      const bool more = !lastc || rd + 1 < rounds;   // the same for every wave
      const int cn = lastc ? 0 : c + 1;
      if (lastc) nxt = tile_of(rd + 1);              // past the last round: no tile
      const I4Words wnext = load_words(nxt, cn);     // in flight during this chunk's MFMAs, as the next slot chunk is
      if (!resident && more) load_q(cn);
      if (has) {
        const unsigned char* qh = sQ + (size_t)buf * L::Q_BYTES + (size_t)li * NP_MS_BROW * 2 + 64 * kk;
        const uint32_t w[8] = {wcur.a.x, wcur.a.y, wcur.a.z, wcur.a.w, wcur.b.x, wcur.b.y, wcur.b.z, wcur.b.w};
        // half-wave 0 holds the chunk's dims 0 .. 63: a step whose 16 dims lie past dim there lies past it in half-wave 1 too
        const int nsteps = (min(64, p.dim - c * NP_MS_KC_I8) + 15) / 16;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          if (s < nsteps) {
            const i32x4 a = i4_expand(w[2 * s], w[2 * s + 1]);
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt)
              if (qt < nslots)
                acc[qt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(
                    a, *reinterpret_cast<const i32x4*>(qh + (size_t)qt * 32 * NP_MS_BROW * 2 + 16 * s), acc[qt], 0, 0, 0);
          }
        }
      }
      if (!resident) {
        if (!L::DBL) __syncthreads();       // one buffer: its fragments have been read
        if (L::DBL) buf ^= 1;
        if (more) store_q(sQ + (size_t)buf * L::Q_BYTES);
        __syncthreads();                    // two buffers: the one written now was last read before the previous barrier
      }
      wcur = wnext;
    }
    if (has) {
      float sc[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = __shfl(dsc, mfma_row(r, kk));
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
        if (qt < nslots) {
          uint32_t best = 0u;
          int ps = -1;
          i32x16 dot;
#pragma unroll
          for (int r = 0; r < 16; ++r) dot[r] = acc[qt][r] >> 4;   // 16 * dot -> dot, exact
          ms_row_argmax_i8(dot, sc, cur.t0, cur.len, kk, best, ps);
          if (best) atomicMax(&sKey[cur.e * R + qt * 32 + li], ((unsigned long long)best << 32) | (0xFFFFFFFFu - (uint32_t)ps));
        }
        __builtin_amdgcn_sched_barrier(0);  // one accumulator tile out of the AGPRs at a time
      }
    }
    cur = nxt;
  }
  __syncthreads();
  if (wave >= nd) return;
  // wave e finishes document e: per query the q-ordered sum of the scaled maxima (tile_sum's rule), and the matches
  const int e = wave;
  const bool bad = sBad[e] != 0;
  for (int s = 0; s < nq; ++s) {
    const int query = qg0 + s;
    const int qb = p.qoff[query], Lq = p.qoff[query + 1] - qb;
    const int64_t out = listed ? pbeg + j0 + e : (int64_t)query * p.n_docs + j0 + e;
    const int64_t rowb = (listed ? (int64_t)*sRow : p.n_docs * (int64_t)qb) + (j0 + e) * (int64_t)Lq;
    float total = 0.f;
    for (int t = 0; t * 32 < Lq; ++t) {
      unsigned long long key = sKey[e * R + (s * p.nqt + t) * 32 + li];
      float m = NP_NEG_INF;
      const int tq = t * 32 + li;
      if (key) {                            // the query token's scale, one multiplication; not finite = no match
        m = unkey((uint32_t)(key >> 32)) * p.qscale[qb + min(tq, Lq - 1)];
        if (!finitef(m)) key = 0ull, m = NP_NEG_INF;
      }
      total = tile_sum(m, min(32, Lq - t * 32), total);
      if (kk == 0 && tq < Lq) {
        if (p.sims) p.sims[rowb + tq] = key ? m : 0.0f;
        if (p.pos) p.pos[rowb + tq] = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
      }
    }
    if (lane == 0) p.scores[out] = bad ? __uint_as_float(0x7FC00000u) : total;
  }
}

template <int NQT>
static int maxsim_i4_launch_one(hipStream_t st, MaxsimP p, const MaxsimPlan& plan) {
  static_assert(MsI4Lds<NQT>::BYTES <= 48 * 1024, "the launch asks for no more LDS than every kernel may have");
  for (int64_t y0 = 0; y0 < plan.gy; y0 += NP_MS_MAX_GRID_Y) {
    p.y0 = (int)y0;
    const dim3 grid((unsigned)plan.gx, (unsigned)std::min<int64_t>(NP_MS_MAX_GRID_Y, plan.gy - y0));
    maxsim_i4_kernel<NQT><<<grid, 256, MsI4Lds<NQT>::BYTES, st>>>(p);
  }
  NP_HIP(hipGetLastError());
  return NP_OK;
}

int maxsim_i4_launch(hipStream_t st, MaxsimP p, const MaxsimPlan& plan) {
  switch (plan.NQT) {
    case 1: return maxsim_i4_launch_one<1>(st, p, plan);
    case 2: return maxsim_i4_launch_one<2>(st, p, plan);
    case 4: return maxsim_i4_launch_one<4>(st, p, plan);
    default: return maxsim_i4_launch_one<8>(st, p, plan);
  }
}

static int maxsim_validate_i4(int32_t dim, const void* q_scales, int32_t B, const int32_t* h_qoff, const void* doc_words,
                              const void* d_scales, int64_t n_docs, const int64_t* h_doff, bool listed,
                              const int64_t* h_pair_docs, const int64_t* h_poff) {
  const char* why = "";
  int64_t bad = -1;
  const int c = maxsim_check_args_i4(dim, q_scales, B, h_qoff, doc_words, d_scales, n_docs, h_doff, listed, h_pair_docs, h_poff, &why,
                                     &bad);
  if (c == 0) return NP_OK;
  if (bad >= 0)
    set_error("maxsim_batch_i4: %s (pair %lld names document %lld, n_docs %lld)", why, (long long)bad,
              (long long)h_pair_docs[bad], (long long)n_docs);
  else
    set_error("%s: maxsim_batch_i4: %s (dim=%d)", c == 1 ? "Shape error" : "Search failed", why, dim);
  return c == 1 ? NP_ERR_SHAPE : NP_ERR_INVALID_ARGUMENT;
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_maxsim_batch_i4_device(int32_t device, int32_t dim, const int8_t* d_queries, const float* d_q_scales,
                                  const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                                  const uint32_t* d_doc_words, const float* d_d_scales, const int64_t* d_doc_tok_offsets,
                                  const int64_t* h_doc_tok_offsets, int64_t n_docs, const int64_t* d_pair_docs,
                                  const int64_t* d_pair_offsets, const int64_t* h_pair_offsets, float* d_out_scores,
                                  float* d_out_match_sims, int32_t* d_out_match_pos, void* stream) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(d_pair_docs && d_pair_offsets && h_pair_offsets, d_pair_docs || d_pair_offsets || h_pair_offsets, true,
                          &listed));
  NP_TRY(maxsim_validate_i4(dim, d_q_scales, B, h_q_tok_offsets, d_doc_words, d_d_scales, n_docs, h_doc_tok_offsets, listed, nullptr,
                            h_pair_offsets));
  return maxsim_device_call(device, NP_MS_DT_I4, 0, dim, d_queries, d_q_scales, d_q_tok_offsets, h_q_tok_offsets, B, d_doc_words,
                            d_d_scales, d_doc_tok_offsets, h_doc_tok_offsets, n_docs, d_pair_docs, d_pair_offsets, h_pair_offsets,
                            d_out_scores, d_out_match_sims, d_out_match_pos, stream);
}

int np_hip_maxsim_batch_i4(int32_t device, int32_t dim, const int8_t* queries, const float* q_scales,
                           const int32_t* q_tok_offsets, int32_t B, const uint32_t* doc_words, const float* d_scales,
                           const int64_t* doc_tok_offsets, int64_t n_docs, const int64_t* pair_docs, const int64_t* pair_offsets,
                           float* out_scores, float* out_match_sims, int32_t* out_match_pos) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(pair_docs && pair_offsets, pair_docs || pair_offsets, false, &listed));
  NP_TRY(maxsim_validate_i4(dim, q_scales, B, q_tok_offsets, doc_words, d_scales, n_docs, doc_tok_offsets, listed, pair_docs,
                            pair_offsets));
  return maxsim_host_call(device, NP_MS_DT_I4, 0, dim, queries, q_scales, q_tok_offsets, B, doc_words, d_scales, doc_tok_offsets,
                          n_docs, pair_docs, pair_offsets, out_scores, out_match_sims, out_match_pos);
}

}  // extern "C"
