// np_maxsim_b1.hip -- np_hip_maxsim_batch_b1: MaxSim of int8 query rows against BINARY document rows, one bit per dim
// (set = +1, clear = -1) with one f32 scale per row, on v_mfma_i32_32x32x32_i8.  A document row of dim 128 is 16 bytes:
// it never touches LDS.  Every step is exact or one f32 rounding: tests/maxsim_i8_restate.py pair() on the unpacked bits.
//
//   work split    maxsim_kernel's (np_maxsim.hip): 4 waves, up to 8 query slots of 32 tokens and up to WD <= 4 documents per
//                 workgroup by maxsim_plan; the 32-token tiles of the documents go round-robin to the waves; row maxima
//                 merge by an LDS atomicMax on (okey << 32 | ~position); wave e forms document e's q-ordered sum and
//                 multiplies by the query scale.  The wave index lives in a scalar register from the first line.
//   query slots   int8 rows in LDS in MODE 3's geometry: a chunk is 128 dims, a row 144 bytes apart, a lane's B fragment the
//                 16 bytes at row li, byte 16 kk + 32 s.  Dims past `dim` are staged as zeros.
//                 dim <= 128: staged once, before the rounds; the rounds have no barrier.
//                 dim > 128: the slots are the ONLY thing in LDS that changes, so with up to 4 slots the chunk is double
//                 buffered: chunk c + 1 (of the next round after the last one) is loaded into registers before the MFMAs
//                 of chunk c, written to the other buffer after them, and ONE barrier ends the chunk.  8 slots (36 KB a
//                 buffer, and one workgroup per CU by registers anyway) keep one buffer and two barriers.
//   documents     lane (li, kk) owns row li of its wave's tile: the row's bit words of a chunk (4 words = 128 dims) come
//                 from global memory into registers, one 16-byte load where every row allows it (W % 4 == 0 and an aligned
//                 base), dword loads otherwise; words at or past W are not read.  The next chunk's (or next round's) words
//                 are requested before the current MFMAs.  Step s takes 16 bits, (word[s] >> 16 kk) & 0xFFFF, and expands
//                 them to the 16-byte A fragment of +-1 bytes: per dword v_bfe (4 bits), v_mul_u32_u24 by 0x204081 (bit i
//                 to bit 8 i, no two partial products meet), v_and 0x01010101, v_perm picking 0x01 or 0xFF.  Pad bits
//                 multiply staged zeros; rows past the tile's end are masked in the epilogue.
//   scales        lane li reads its row's scale from global memory when the round starts; the epilogue fetches the 16
//                 scales of rows mfma_row(r, kk) by wave shuffles and walks ms_row_argmax_i8.
#include "np_maxsim_dev.h"

namespace np {

template <int NQT> struct MsB1Lds {
  static constexpr int R = NQT * 32;                                // slot rows
  static constexpr bool DBL = NQT < 8;                              // two slot buffers when dim > 128
  static constexpr size_t Q_BYTES = (size_t)R * NP_MS_BROW * 2;     // one buffer
  static constexpr size_t KEY_OFF = (DBL ? 2 : 1) * Q_BYTES;
  static constexpr size_t QROW_OFF = KEY_OFF + (size_t)NP_MS_WG_DOCS * R * 8;
  static constexpr size_t META_OFF = QROW_OFF + (size_t)R * 8;
  static constexpr size_t BYTES = META_OFF + NP_MS_META;
};

// words w0 .. w0 + 3 of a bit row (NULL = a row past the end), zeros at and past W
__device__ __forceinline__ uint4 b1_load_words(const uint32_t* rowp, int w0, int W, bool vec) {
  uint4 r = make_uint4(0u, 0u, 0u, 0u);
  if (!rowp || w0 >= W) return r;
  if (vec) return *reinterpret_cast<const uint4*>(rowp + w0);   // W % 4 == 0: w0 + 4 <= W
  r.x = rowp[w0];
  if (w0 + 1 < W) r.y = rowp[w0 + 1];
  if (w0 + 2 < W) r.z = rowp[w0 + 2];
  if (w0 + 3 < W) r.w = rowp[w0 + 3];
  return r;
}

// bits sh .. sh + 15 of `word` as sixteen int8: set = +1, clear = -1, bit sh first
__device__ __forceinline__ i32x4 b1_expand(uint32_t word, int sh) {
  i32x4 a;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t nib = (word >> (sh + 4 * j)) & 0xFu;
    const uint32_t sel = __umul24(nib, 0x204081u) & 0x01010101u;   // bit i of nib at bit 8 i: a byte selector 0 or 1
    a[j] = (int)__builtin_amdgcn_perm(0u, 0x000001FFu, sel);       // selector 0 = byte 0xFF, 1 = byte 0x01
  }
  return a;
}

struct B1Tile {
  int e;                    // document of the workgroup
  int64_t t0, len, drow0;   // first token of the tile, the document's length (0 = no tile), the tile's first global row
};

template <int NQT>
__global__ void __launch_bounds__(256) maxsim_b1_kernel(MaxsimP p) {
  using L = MsB1Lds<NQT>;
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
  const int W = (p.dim + 31) / 32;
  const int nchunks = (p.dim + NP_MS_KC_I8 - 1) / NP_MS_KC_I8;
  const bool resident = nchunks == 1;       // the slots are staged once; the rounds then touch no shared memory but the keys

  auto tile_of = [&](int64_t rd) {          // this wave's tile of round rd
    const int64_t ti = rd * 4 + wave;
    B1Tile t;
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
  auto load_words = [&](const B1Tile& t, int c) {   // row li's four words of chunk c (zeros for a row past the end)
    const bool row = t.t0 + li < t.len;
    return b1_load_words(row ? static_cast<const uint32_t*>(p.D) + (t.drow0 + li) * W : nullptr, 4 * c, W, p.vecd != 0);
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
  auto store_q = [&](unsigned char* buf) {
#pragma unroll
    for (int i = 0; i < NQT; ++i) {
      const int u = tid + 256 * i;
      *reinterpret_cast<uint4*>(buf + (size_t)(u >> 3) * NP_MS_BROW * 2 + 16 * (u & 7)) = rq[i];
    }
  };

  B1Tile cur = tile_of(0);
  uint4 wcur = load_words(cur, 0);
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
    B1Tile nxt = cur;
    for (int c = 0; c < nchunks; ++c) {
      const bool lastc = c + 1 == nchunks;
      const bool more = !lastc || rd + 1 < rounds;   // the same for every wave
      const int cn = lastc ? 0 : c + 1;
      if (lastc) nxt = tile_of(rd + 1);              // past the last round: no tile
      const uint4 wnext = load_words(nxt, cn);       // in flight during this chunk's MFMAs, as the next slot chunk is
      if (!resident && more) load_q(cn);
      if (has) {
        const unsigned char* qh = sQ + (size_t)buf * L::Q_BYTES + ((size_t)li * NP_MS_BROW + 8 * kk) * 2;
        const uint32_t w[4] = {wcur.x, wcur.y, wcur.z, wcur.w};
        const int nsteps = (min(NP_MS_KC_I8, p.dim - c * NP_MS_KC_I8) + 31) / 32;   // the steps past dim would add exact zeros
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          if (s < nsteps) {
            const i32x4 a = b1_expand(w[s], 16 * kk);
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt)
              if (qt < nslots)
                acc[qt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(
                    a, *reinterpret_cast<const i32x4*>(qh + (size_t)qt * 32 * NP_MS_BROW * 2 + 32 * s), acc[qt], 0, 0, 0);
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
          ms_row_argmax_i8(acc[qt], sc, cur.t0, cur.len, kk, best, ps);
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
static int maxsim_b1_launch_one(hipStream_t st, MaxsimP p, const MaxsimPlan& plan) {
  static_assert(MsB1Lds<NQT>::BYTES <= 48 * 1024, "the launch asks for no more LDS than every kernel may have");
  for (int64_t y0 = 0; y0 < plan.gy; y0 += NP_MS_MAX_GRID_Y) {
    p.y0 = (int)y0;
    const dim3 grid((unsigned)plan.gx, (unsigned)std::min<int64_t>(NP_MS_MAX_GRID_Y, plan.gy - y0));
    maxsim_b1_kernel<NQT><<<grid, 256, MsB1Lds<NQT>::BYTES, st>>>(p);
  }
  NP_HIP(hipGetLastError());
  return NP_OK;
}

int maxsim_b1_launch(hipStream_t st, MaxsimP p, const MaxsimPlan& plan) {
  switch (plan.NQT) {
    case 1: return maxsim_b1_launch_one<1>(st, p, plan);
    case 2: return maxsim_b1_launch_one<2>(st, p, plan);
    case 4: return maxsim_b1_launch_one<4>(st, p, plan);
    default: return maxsim_b1_launch_one<8>(st, p, plan);
  }
}

static int maxsim_validate_b1(int32_t dim, const void* q_scales, int32_t B, const int32_t* h_qoff, const void* doc_bits,
                              const void* d_scales, int64_t n_docs, const int64_t* h_doff, bool listed,
                              const int64_t* h_pair_docs, const int64_t* h_poff) {
  const char* why = "";
  int64_t bad = -1;
  const int c = maxsim_check_args_b1(dim, q_scales, B, h_qoff, doc_bits, d_scales, n_docs, h_doff, listed, h_pair_docs, h_poff, &why,
                                     &bad);
  if (c == 0) return NP_OK;
  if (bad >= 0)
    set_error("maxsim_batch_b1: %s (pair %lld names document %lld, n_docs %lld)", why, (long long)bad,
              (long long)h_pair_docs[bad], (long long)n_docs);
  else
    set_error("%s: maxsim_batch_b1: %s (dim=%d)", c == 1 ? "Shape error" : "Search failed", why, dim);
  return c == 1 ? NP_ERR_SHAPE : NP_ERR_INVALID_ARGUMENT;
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_maxsim_batch_b1_device(int32_t device, int32_t dim, const int8_t* d_queries, const float* d_q_scales,
                                  const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                                  const uint32_t* d_doc_bits, const float* d_d_scales, const int64_t* d_doc_tok_offsets,
                                  const int64_t* h_doc_tok_offsets, int64_t n_docs, const int64_t* d_pair_docs,
                                  const int64_t* d_pair_offsets, const int64_t* h_pair_offsets, float* d_out_scores,
                                  float* d_out_match_sims, int32_t* d_out_match_pos, void* stream) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(d_pair_docs && d_pair_offsets && h_pair_offsets, d_pair_docs || d_pair_offsets || h_pair_offsets, true,
                          &listed));
  NP_TRY(maxsim_validate_b1(dim, d_q_scales, B, h_q_tok_offsets, d_doc_bits, d_d_scales, n_docs, h_doc_tok_offsets, listed, nullptr,
                            h_pair_offsets));
  return maxsim_device_call(device, NP_MS_DT_B1, 0, dim, d_queries, d_q_scales, d_q_tok_offsets, h_q_tok_offsets, B, d_doc_bits,
                            d_d_scales, d_doc_tok_offsets, h_doc_tok_offsets, n_docs, d_pair_docs, d_pair_offsets, h_pair_offsets,
                            d_out_scores, d_out_match_sims, d_out_match_pos, stream);
}

int np_hip_maxsim_batch_b1(int32_t device, int32_t dim, const int8_t* queries, const float* q_scales,
                           const int32_t* q_tok_offsets, int32_t B, const uint32_t* doc_bits, const float* d_scales,
                           const int64_t* doc_tok_offsets, int64_t n_docs, const int64_t* pair_docs, const int64_t* pair_offsets,
                           float* out_scores, float* out_match_sims, int32_t* out_match_pos) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(pair_docs && pair_offsets, pair_docs || pair_offsets, false, &listed));
  NP_TRY(maxsim_validate_b1(dim, q_scales, B, q_tok_offsets, doc_bits, d_scales, n_docs, doc_tok_offsets, listed, pair_docs,
                            pair_offsets));
  return maxsim_host_call(device, NP_MS_DT_B1, 0, dim, queries, q_scales, q_tok_offsets, B, doc_bits, d_scales, doc_tok_offsets,
                          n_docs, pair_docs, pair_offsets, out_scores, out_match_sims, out_match_pos);
}

}  // extern "C"
