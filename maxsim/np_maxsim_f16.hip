// np_maxsim_f16.hip -- np_hip_maxsim_batch_f16: MaxSim of IEEE binary16 rows, queries and documents alike, `dim` halves apart
// and unpadded, on v_mfma_f32_32x32x16_f16.  A product of two f16 values has a 22-bit significand: it is exact in f32, so the
// only roundings are the f32 accumulator's, and tests/maxsim_restate.py pair(.., "bf16_rows") on the widened values is the
// reference and the bound.  Rows are used as given: nothing is rounded, so matches are allowed as at precision 0.
//
//   work split    maxsim_i4_kernel's (np_maxsim_i4.hip): 4 waves, up to 8 query slots of 32 tokens and up to WD <= 4 documents
//                 per workgroup by maxsim_plan; the 32-token tiles of the documents go round-robin to the waves; row maxima
//                 merge by an LDS atomicMax on (okey << 32 | ~position); wave e forms document e's q-ordered sum.  The wave
//                 index lives in a scalar register from the first line.
//   chunk         64 dims = 128 bytes a row, four MFMA steps of 16 dims.
//   documents     never in LDS.  Lane (li, kk) owns row li of its wave's tile and HALF of the row's chunk: bytes 64 kk ..
//                 64 kk + 63, dims 32 kk .. 32 kk + 31 of the chunk, from global memory into 16 registers -- four 16-byte
//                 loads where every row allows it (dim % 8 == 0 and an aligned base), element loads otherwise; nothing at
//                 or past dim is read, pad dims and rows past the tile are zeros.  The two half-waves load different halves,
//                 so a wave requests each byte once.  The next chunk's (or next round's) 16 registers are requested before
//                 the current MFMAs.  Step s takes the lane's s-th 16 bytes as its A fragment: half-wave 0 brings the
//                 chunk's dims 8 s .. 8 s + 7, half-wave 1 dims 32 + 8 s .. 32 + 8 s + 7.  That assignment is fixed -- it
//                 does not depend on WD, G, the grid or the list -- so one (slot, tile) accumulator adds the same products
//                 in the same order wherever the pair stands: a pair's bits depend on its two matrices only.
//   query slots   f16 rows in LDS in the bf16 modes' geometry (rows 144 bytes apart, eight 16-byte units a row); the B
//                 fragment of step s is the 16 bytes at row li, byte 64 kk + 16 s: the document's split.  Dims past `dim`
//                 are staged as zeros; steps wholly past dim are skipped.
//                 up to 4 slots: two slot buffers.  dim <= 128 is at most two chunks: each buffer holds one, staged once
//                 before the round loop, and the rounds run without a barrier.  Above 128 the two buffers double-buffer the
//                 flat (round, chunk) sequence with ONE barrier per chunk.
//                 8 slots: one buffer (two would pass the 48 KB every launch may ask for without an attribute call):
//                 resident at dim <= 64, two barriers per chunk above, as maxsim_b1_kernel<8>.
//   epilogue      precision 0's: no scales; per tile and slot the masked row maximum with the lowest position over ascending
//                 rows, non-finite sims ignored, then the key atomicMax; the finishing wave sums by tile_sum.
#include "np_maxsim_dev.h"

namespace np {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int NQT> struct MsF16Lds {
  static constexpr int R = NQT * 32;                                // slot rows
  static constexpr bool DBL = NQT < 8;                              // two slot buffers
  static constexpr size_t Q_BYTES = (size_t)R * NP_MS_BROW * 2;     // one buffer: a 64-dim chunk of every slot row
  static constexpr size_t KEY_OFF = (DBL ? 2 : 1) * Q_BYTES;
  static constexpr size_t QROW_OFF = KEY_OFF + (size_t)NP_MS_WG_DOCS * R * 8;
  static constexpr size_t META_OFF = QROW_OFF + (size_t)R * 8;
  static constexpr size_t BYTES = META_OFF + NP_MS_META;
};

constexpr int NP_MS_KC_F16 = NP_MS_KC_BF16;   // dims per chunk

// eight f16 dims k0 .. k0 + 7 of a row (NULL = a row past the end), zeros at and past dim; k0 is a multiple of 8
__device__ __forceinline__ uint4 f16_load8(const uint16_t* rowp, int k0, int dim, bool vec) {
  uint4 r = make_uint4(0u, 0u, 0u, 0u);
  if (!rowp || k0 >= dim) return r;
  if (vec) return *reinterpret_cast<const uint4*>(rowp + k0);   // dim % 8 == 0: k0 + 8 <= dim
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (k0 + i < dim) w[i >> 1] |= (uint32_t)rowp[k0 + i] << (16 * (i & 1));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

struct F16Half {
  uint4 v[4];   // a lane's 32 dims of a chunk: the A fragments of the four steps
};

struct F16Tile {
  int e;                    // document of the workgroup
  int64_t t0, len, drow0;   // first token of the tile, the document's length (0 = no tile), the tile's first global row
};

// rows t0 + mfma_row(r, kk) of one accumulator: entries of rows past `len` and non-finite entries ignored; ascending rows
// and the strict `>` keep the lowest position of this lane's rows (ms_row_argmax of np_maxsim.hip, the same walk)
__device__ __forceinline__ void f16_row_argmax(const f32x16& acc, int64_t t0, int64_t len, int kk, float& mm, int& pos) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t trow = t0 + mfma_row(r, kk);
    const float x = acc[r];
    if (trow < len && finitef(x)) {
      pos = x > mm ? (int)trow : pos;
      mm = fmaxf(mm, x);
    }
  }
}

template <int NQT>
__global__ void __launch_bounds__(256) maxsim_f16_kernel(MaxsimP p) {
  using L = MsF16Lds<NQT>;
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
  const int nchunks = (p.dim + NP_MS_KC_F16 - 1) / NP_MS_KC_F16;
  // every chunk of the slots has a buffer of its own: staged once, and the rounds touch no shared memory but the keys
  const bool resident = nchunks <= (L::DBL ? 2 : 1);

  auto tile_of = [&](int64_t rd) {          // this wave's tile of round rd
    const int64_t ti = rd * 4 + wave;
    F16Tile t;
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
  auto load_half = [&](const F16Tile& t, int c) {   // this lane's half of row li's chunk c (zeros for a row past the end)
    const uint16_t* rowp = t.t0 + li < t.len ? static_cast<const uint16_t*>(p.D) + (t.drow0 + li) * p.dim : nullptr;
    F16Half h;
#pragma unroll
    for (int s = 0; s < 4; ++s) h.v[s] = f16_load8(rowp, c * NP_MS_KC_F16 + 32 * kk + 8 * s, p.dim, p.vecd != 0);
    return h;
  };
  uint4 rq[NQT];                            // a slot chunk on its way from HBM to LDS: unit (row u >> 3, 16 bytes at 16 (u & 7))
  auto load_q = [&](int c) {
#pragma unroll
    for (int i = 0; i < NQT; ++i) {
      const int u = tid + 256 * i;
      const int64_t grow = sQrow[u >> 3];
      rq[i] = f16_load8(grow < 0 ? nullptr : static_cast<const uint16_t*>(p.Q) + grow * p.dim, c * NP_MS_KC_F16 + 8 * (u & 7), p.dim,
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

  F16Tile cur = tile_of(0);
  F16Half hcur = load_half(cur, 0);
  load_q(0);
  store_q(sQ);
  if (L::DBL && resident && nchunks == 2) {
    load_q(1);
    store_q(sQ + L::Q_BYTES);
  }
  __syncthreads();
  int buf = 0;                              // streaming: the slot buffer that holds the current chunk
  for (int64_t rd = 0; rd < rounds; ++rd) {
    const bool has = cur.len > 0;
    f32x16 acc[NQT];
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[qt][r] = 0.f;
    F16Tile nxt = cur;
    for (int c = 0; c < nchunks; ++c) {
      const bool lastc = c + 1 == nchunks;
      const bool more = !lastc || rd + 1 < rounds;   // the same for every wave
      const int cn = lastc ? 0 : c + 1;
      if (lastc) nxt = tile_of(rd + 1);              // past the last round: no tile
      const F16Half hnext = load_half(nxt, cn);      // in flight during this chunk's MFMAs, as the next slot chunk is
      if (!resident && more) load_q(cn);
      if (has) {
        const unsigned char* qh = sQ + (size_t)(resident ? c : buf) * L::Q_BYTES + (size_t)li * NP_MS_BROW * 2 + 64 * kk;
        // half-wave 0 holds the chunk's dims 0 .. 31: a step whose 8 dims lie past dim there lies past it in half-wave 1 too
        const int nsteps = (min(32, p.dim - c * NP_MS_KC_F16) + 7) / 8;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          if (s < nsteps) {
            const f16x8 a = __builtin_bit_cast(f16x8, hcur.v[s]);
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt)
              if (qt < nslots)
                acc[qt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                    a, *reinterpret_cast<const f16x8*>(qh + (size_t)qt * 32 * NP_MS_BROW * 2 + 16 * s), acc[qt], 0, 0, 0);
          }
        }
      }
      if (!resident) {
        if (!L::DBL) __syncthreads();       // one buffer: its fragments have been read
        if (L::DBL) buf ^= 1;
        if (more) store_q(sQ + (size_t)buf * L::Q_BYTES);
        __syncthreads();                    // two buffers: the one written now was last read before the previous barrier
      }
      hcur = hnext;
    }
    if (has) {
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
        if (qt < nslots) {
          float m = NP_NEG_INF;
          int ps = -1;
          f16_row_argmax(acc[qt], cur.t0, cur.len, kk, m, ps);
          if (ps >= 0)
            atomicMax(&sKey[cur.e * R + qt * 32 + li], ((unsigned long long)okey(m) << 32) | (0xFFFFFFFFu - (uint32_t)ps));
        }
        __builtin_amdgcn_sched_barrier(0);  // one accumulator tile out of the AGPRs at a time
      }
    }
    cur = nxt;
  }
  __syncthreads();
  if (wave >= nd) return;
  // wave e finishes document e: per query the q-ordered sum of the maxima (tile_sum's rule), and the matches
  const int e = wave;
  const bool bad = sBad[e] != 0;
  for (int s = 0; s < nq; ++s) {
    const int query = qg0 + s;
    const int qb = p.qoff[query], Lq = p.qoff[query + 1] - qb;
    const int64_t out = listed ? pbeg + j0 + e : (int64_t)query * p.n_docs + j0 + e;
    const int64_t rowb = (listed ? (int64_t)*sRow : p.n_docs * (int64_t)qb) + (j0 + e) * (int64_t)Lq;
    float total = 0.f;
    for (int t = 0; t * 32 < Lq; ++t) {
      const unsigned long long key = sKey[e * R + (s * p.nqt + t) * 32 + li];
      const float m = key ? unkey((uint32_t)(key >> 32)) : NP_NEG_INF;
      const int tq = t * 32 + li;
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
static int maxsim_f16_launch_one(hipStream_t st, MaxsimP p, const MaxsimPlan& plan) {
  static_assert(MsF16Lds<NQT>::BYTES <= 48 * 1024, "the launch asks for no more LDS than every kernel may have");
  for (int64_t y0 = 0; y0 < plan.gy; y0 += NP_MS_MAX_GRID_Y) {
    p.y0 = (int)y0;
    const dim3 grid((unsigned)plan.gx, (unsigned)std::min<int64_t>(NP_MS_MAX_GRID_Y, plan.gy - y0));
    maxsim_f16_kernel<NQT><<<grid, 256, MsF16Lds<NQT>::BYTES, st>>>(p);
  }
  NP_HIP(hipGetLastError());
  return NP_OK;
}

int maxsim_f16_launch(hipStream_t st, MaxsimP p, const MaxsimPlan& plan) {
  switch (plan.NQT) {
    case 1: return maxsim_f16_launch_one<1>(st, p, plan);
    case 2: return maxsim_f16_launch_one<2>(st, p, plan);
    case 4: return maxsim_f16_launch_one<4>(st, p, plan);
    default: return maxsim_f16_launch_one<8>(st, p, plan);
  }
}

static int maxsim_validate_f16(int32_t dim, int32_t B, const int32_t* h_qoff, int64_t n_docs, const int64_t* h_doff, bool listed,
                               const int64_t* h_pair_docs, const int64_t* h_poff) {
  const char* why = "";
  int64_t bad = -1;
  const int c = maxsim_check_args_f16(dim, B, h_qoff, n_docs, h_doff, listed, h_pair_docs, h_poff, &why, &bad);
  if (c == 0) return NP_OK;
  if (bad >= 0)
    set_error("maxsim_batch_f16: %s (pair %lld names document %lld, n_docs %lld)", why, (long long)bad,
              (long long)h_pair_docs[bad], (long long)n_docs);
  else
    set_error("%s: maxsim_batch_f16: %s (dim=%d)", c == 1 ? "Shape error" : "Search failed", why, dim);
  return c == 1 ? NP_ERR_SHAPE : NP_ERR_INVALID_ARGUMENT;
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_maxsim_batch_f16_device(int32_t device, int32_t dim, const uint16_t* d_queries, const int32_t* d_q_tok_offsets,
                                   const int32_t* h_q_tok_offsets, int32_t B, const uint16_t* d_documents,
                                   const int64_t* d_doc_tok_offsets, const int64_t* h_doc_tok_offsets, int64_t n_docs,
                                   const int64_t* d_pair_docs, const int64_t* d_pair_offsets, const int64_t* h_pair_offsets,
                                   float* d_out_scores, float* d_out_match_sims, int32_t* d_out_match_pos, void* stream) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(d_pair_docs && d_pair_offsets && h_pair_offsets, d_pair_docs || d_pair_offsets || h_pair_offsets, true,
                          &listed));
  NP_TRY(maxsim_validate_f16(dim, B, h_q_tok_offsets, n_docs, h_doc_tok_offsets, listed, nullptr, h_pair_offsets));
  return maxsim_device_call(device, NP_MS_DT_F16, 0, dim, d_queries, nullptr, d_q_tok_offsets, h_q_tok_offsets, B, d_documents,
                            nullptr, d_doc_tok_offsets, h_doc_tok_offsets, n_docs, d_pair_docs, d_pair_offsets, h_pair_offsets,
                            d_out_scores, d_out_match_sims, d_out_match_pos, stream);
}

int np_hip_maxsim_batch_f16(int32_t device, int32_t dim, const uint16_t* queries, const int32_t* q_tok_offsets, int32_t B,
                            const uint16_t* documents, const int64_t* doc_tok_offsets, int64_t n_docs, const int64_t* pair_docs,
                            const int64_t* pair_offsets, float* out_scores, float* out_match_sims, int32_t* out_match_pos) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(pair_docs && pair_offsets, pair_docs || pair_offsets, false, &listed));
  NP_TRY(maxsim_validate_f16(dim, B, q_tok_offsets, n_docs, doc_tok_offsets, listed, pair_docs, pair_offsets));
  return maxsim_host_call(device, NP_MS_DT_F16, 0, dim, queries, nullptr, q_tok_offsets, B, documents, nullptr, doc_tok_offsets,
                          n_docs, pair_docs, pair_offsets, out_scores, out_match_sims, out_match_pos);
}

}  // extern "C"
