// np_maxsim.hip -- np_hip_maxsim_batch: MaxSim (maxsim.rs:270-294) of caller-supplied embeddings, many queries against
// listed documents or against all of them, on matrix instructions, for any dim up to 1024.
//
// Every other MFMA path of the library reads compressed rows of at most 128 dims and keeps a whole row in registers.  Here
// the operands are plain rows, f32 or bf16, `dim` elements apart, and the reduction dimension does not fit: both operands
// stream through LDS in chunks along dim while the 32x32 accumulators stay in registers across the chunk loop.
//
//   work split    A workgroup (4 waves) holds up to 8 query tiles of 32 tokens ("slots") and up to WD <= 4 documents.
//                 listed form: blockIdx.y = the query, blockIdx.x = a group of WD consecutive pairs of its list; the slots
//                 are the query's own tiles.  all-pairs form: blockIdx.y = a group of G consecutive queries (G * nqt <= 8
//                 slots, nqt = tiles of the call's longest query), blockIdx.x = WD consecutive documents: a document
//                 chunk is staged once and multiplied against every slot, so its bytes are read once per query group.
//                 The 32-token tiles of the workgroup's documents form one list that the waves take round-robin: four
//                 short documents occupy four waves, a 1000-token document spreads its 32 tiles over all of them.
//                 WD and G shrink on the host while the grid would leave compute units idle (np_maxsim_plan.h).
//   chunk loop    per round (one tile per wave) and per chunk of KC dims: all 256 threads stage the slots' query rows,
//                 each wave stages its own document tile, barrier, MFMA steps in ascending dim order.  The global loads
//                 of chunk c + 1 are issued into registers before the MFMAs of chunk c and written to LDS after them.
//                 KC = 32 (f32) / 64 (bf16): 8 slots x 32 rows x KC plus 4 document tiles is 52-54 KB, so the 160 KB of a
//                 CU hold two workgroups wherever the registers do (1 and 2 slots: profiles/maxsim_kernel_resources.md)
//                 and one's barriers hide behind the other's MFMAs; a chunk is 16 (f32) or 4 (bf16) MFMA steps per
//                 slot, up to 128 / 32 MFMAs between two barriers.
//   LDS layout    f32: k-major, [k][row], a row of k values `S` floats apart, S = 32 for a document tile and an ODD
//                 multiple of 32 for the slots (rows padded by 32 when the slot count is even).  The fragment read of
//                 v_mfma_f32_32x32x2f32 is one float per lane at (2s + kk) * S + li: lanes 0..31 read consecutive banks,
//                 lanes 32..63 the next k row, 32 (mod 64) banks on: no conflict on 32 or 64 banks.  Staging transposes: a
//                 lane loads four consecutive dims of one row and writes them to four k rows, lanes along the tokens
//                 (consecutive banks); the half-waves write their four values in opposite order so they never meet.
//                 bf16: row-major, a row 72 elements (144 B = 9 x 16 B) apart for 64 used: the fragment read of
//                 v_mfma_f32_32x32x16_bf16 is 16 B per lane at row li, and an odd count of 16-byte units per row puts
//                 consecutive rows into different bank groups.  f32 input is rounded (nearest even) when it is staged.
//   rows          global rows are unpadded and `dim` may be odd: a lane's 16-byte load is taken only where the call allows
//                 it everywhere (base pointer and row pitch multiples of 16 bytes), otherwise element loads; dims past
//                 `dim` and rows past the tile's end are staged as zeros, so every pad product is exactly 0.
//   maxima        per tile and slot the masked row maximum with its lowest position (the shape of tile_row_argmax), then
//                 an LDS atomic max on the key (okey(sim) << 32 | ~position): order-free, so the waves need no order.
//                 After the last round wave e forms, per query, tile_sum's q-ordered sum for document e from the keys.
//   independence  one (slot, document tile) accumulator sees the dims in ascending order whatever surrounds it; the key
//                 maximum does not depend on which wave brought what; the sum runs in the query's own order.  A pair's
//                 bits therefore depend on its two matrices only -- not on WD, G, the grid, the list or the entry.
//
// np_hip_maxsim_batch_i8 (MODE 3): rows of int8 codes with one f32 scale per row, v_mfma_i32_32x32x32_i8.
//   chunk         128 dims = 128 bytes a row: byte for byte the bf16 geometry above (144-byte pitch, eight 16-byte staging
//                 units a row, a fragment = 16 bytes per lane at row li, byte 16 kk + 32 s; four MFMA steps a chunk and slot).
//                 Which 16 of a step's 32 dims a half-wave holds does not matter: both operands split alike and the i32
//                 sum is exact (|dot| <= 1024 * 128 * 128 = 2^24, which f32 also holds exactly).
//   scales        a wave writes the scales of its tile's 32 document tokens into the 16 pad bytes of its own LDS rows; the
//                 epilogue forms f32(acc) * scale[row], one multiplication, and compares the okey of the products (strict >
//                 over ascending rows, then the same key atomicMax).  The finishing wave multiplies each maximum by the
//                 query token's scale, once; a product that is not finite reports no match.
//   resident      dim <= 128 is a single chunk: the slots' query rows are then staged ONCE, before the round loop, and since
//                 a document tile is its wave's own, the rounds need no barrier at all -- the four waves stream their tiles
//                 independently (a 1030-token page: 9 rounds, 1 staging of the slots instead of 9, 1 barrier instead of 18).
//                 MODE 3 only; the other modes keep their loop.
#include "np_internal.h"
#include "np_exact.h"
#include "np_maxsim_plan.h"
#include "np_maxsim_dev.h"

#include <string.h>
#include <type_traits>
#include <vector>

namespace np {


// MODE 0: f32 rows, f32 MFMA.  1: f32 rows rounded to bf16, bf16 MFMA.  2: bf16 rows, bf16 MFMA.  3: int8 rows, i8 MFMA, in
// the bf16 modes' LDS geometry (a row's 128 bytes are 128 dims instead of 64).
constexpr int NP_MS_SCALE_AT = 128;                    // MODE 3: a document row's scale, in the pad bytes of its LDS row
// MsRaw, MsLds and the staging helpers (ms_load, ms_store, ms_unit, ms_row_argmax): np_maxsim_dev.h, shared with
// maxsim_long_kernel (np_maxsim_long.hip).

template <int MODE, int NQT>
__global__ void __launch_bounds__(256) maxsim_kernel(MaxsimP p) {
  using L = MsLds<MODE, NQT>;
  constexpr int KC = L::KC, R = L::R, SQ = L::SQ;
  constexpr int EPU = MODE == 0 ? 4 : MODE == 3 ? 16 : 8;   // elements per staging unit; a chunk is 8 units per row either way
  using Acc = typename std::conditional<MODE == 3, i32x16, f32x16>::type;
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, kk = lane >> 5;
  // MODE 3 keeps the wave index in a scalar register (the other modes keep the code they had)
  const int wave = MODE == 3 ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
  unsigned char* sQ = smem;
  unsigned char* sD = smem + L::Q_BYTES + (size_t)wave * L::D_BYTES;
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
  const int nchunks = (p.dim + KC - 1) / KC;
  // MODE 3 with a single chunk: the slots are staged here, once; the rounds then touch only each wave's own tile
  const bool resident = MODE == 3 && nchunks == 1;
  if (resident) {
#pragma unroll
    for (int i = 0; i < NQT; ++i) {
      int row, g;
      ms_unit<MODE>(tid + 256 * i, R, row, g);
      ms_store<MODE>(sQ, SQ, row, g, ms_load<MODE>(p.Q, sQrow[row], p.dim, g * EPU, p.vecq != 0));
    }
    __syncthreads();
  }

  for (int64_t rd = 0; rd < rounds; ++rd) {
    const int64_t ti = rd * 4 + wave;       // this wave's tile of the round
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

    Acc acc[NQT];
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[qt][r] = 0;
    if (MODE == 3 && has && lane < 32)      // this tile's scales, read back in the epilogue (rows past the end are masked there)
      *reinterpret_cast<float*>(sD + lane * NP_MS_BROW * 2 + NP_MS_SCALE_AT) = t0 + lane < len ? p.dscale[drow0 + lane] : 0.f;

    MsRaw<MODE> rq[NQT], rdoc[4];
    auto load_chunk = [&](int c) {
      const int kc0 = c * KC;
      if (!resident) {
#pragma unroll
        for (int i = 0; i < NQT; ++i) {
          int row, g;
          ms_unit<MODE>(tid + 256 * i, R, row, g);
          rq[i] = ms_load<MODE>(p.Q, sQrow[row], p.dim, kc0 + g * EPU, p.vecq != 0);
        }
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
      if (!resident) {
        __syncthreads();                    // the previous chunk's fragments have been read
#pragma unroll
        for (int i = 0; i < NQT; ++i) {
          int row, g;
          ms_unit<MODE>(tid + 256 * i, R, row, g);
          ms_store<MODE>(sQ, SQ, row, g, rq[i]);
        }
      }
      if (has) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          int row, g;
          ms_unit<MODE>(lane + 64 * i, 32, row, g);
          ms_store<MODE>(sD, 32, row, g, rdoc[i]);
        }
      }
      if (!resident) __syncthreads();       // (resident: a wave reads the tile it wrote itself, and slots nobody writes)
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
        } else if constexpr (MODE == 3) {
          const i32x4 a = *reinterpret_cast<const i32x4*>(dh + 32 * s);
#pragma unroll
          for (int qt = 0; qt < NQT; ++qt)
            if (qt < nslots)
              acc[qt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(
                  a, *reinterpret_cast<const i32x4*>(qh + (size_t)qt * 32 * NP_MS_BROW * 2 + 32 * s), acc[qt], 0, 0, 0);
        } else {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(dh + 32 * s);
#pragma unroll
          for (int qt = 0; qt < NQT; ++qt)
            if (qt < nslots)
              acc[qt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                  a, *reinterpret_cast<const bf16x8*>(qh + (size_t)qt * 32 * NP_MS_BROW * 2 + 32 * s), acc[qt], 0, 0, 0);
        }
      };
      // four steps at a time (more fragments in flight than that only cost registers); dims past `dim` are zeros on both
      // sides, so the steps past dim's own last one add exact zeros
      constexpr int STEP = MODE == 0 ? 2 : MODE == 3 ? 32 : 16;
      constexpr int GS = 4;   // steps per group
      const int ng = (min(KC, p.dim - c * KC) + GS * STEP - 1) / (GS * STEP);
#pragma unroll 1
      for (int s4 = 0; s4 < ng; ++s4) {
#pragma unroll
        for (int s = 0; s < GS; ++s) step(GS * s4 + s);
      }
    }
    if constexpr (MODE == 3) {
      if (has) {
        float sc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r)
          sc[r] = *reinterpret_cast<const float*>(sD + mfma_row(r, kk) * NP_MS_BROW * 2 + NP_MS_SCALE_AT);
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
          if (qt < nslots) {
            uint32_t best = 0u;
            int ps = -1;
            ms_row_argmax_i8(acc[qt], sc, t0, len, kk, best, ps);
            if (best) atomicMax(&sKey[e * R + qt * 32 + li], ((unsigned long long)best << 32) | (0xFFFFFFFFu - (uint32_t)ps));
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    } else if (has) {
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
        if (qt < nslots) {
          float m = NP_NEG_INF;
          int ps = -1;
          ms_row_argmax(acc[qt], t0, len, kk, m, ps);
          if (ps >= 0)
            atomicMax(&sKey[e * R + qt * 32 + li], ((unsigned long long)okey(m) << 32) | (0xFFFFFFFFu - (uint32_t)ps));
        }
        __builtin_amdgcn_sched_barrier(0);   // one accumulator tile out of the AGPRs at a time
      }
    }
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
      unsigned long long key = sKey[e * R + (s * p.nqt + t) * 32 + li];
      float m = key ? unkey((uint32_t)(key >> 32)) : NP_NEG_INF;
      const int tq = t * 32 + li;
      if (MODE == 3 && key) {               // the query token's scale, one multiplication; not finite = no match
        m *= p.qscale[qb + min(tq, Lq - 1)];
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

// ---- host ------------------------------------------------------------------------------------------------------------
template <int MODE, int NQT>
static int maxsim_launch_one(hipStream_t st, MaxsimP p, const MaxsimPlan& plan) {
  const size_t lds = MsLds<MODE, NQT>::BYTES;
  if (lds > 48 * 1024)
    NP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&maxsim_kernel<MODE, NQT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int64_t y0 = 0; y0 < plan.gy; y0 += NP_MS_MAX_GRID_Y) {
    p.y0 = (int)y0;
    const dim3 grid((unsigned)plan.gx, (unsigned)std::min<int64_t>(NP_MS_MAX_GRID_Y, plan.gy - y0));
    maxsim_kernel<MODE, NQT><<<grid, 256, lds, st>>>(p);
  }
  NP_HIP(hipGetLastError());
  return NP_OK;
}

template <int MODE>
static int maxsim_launch_mode(hipStream_t st, const MaxsimP& p, const MaxsimPlan& plan) {
  switch (plan.NQT) {
    case 1: return maxsim_launch_one<MODE, 1>(st, p, plan);
    case 2: return maxsim_launch_one<MODE, 2>(st, p, plan);
    case 4: return maxsim_launch_one<MODE, 4>(st, p, plan);
    default: return maxsim_launch_one<MODE, 8>(st, p, plan);
  }
}

static int maxsim_validate(int32_t dtype, int32_t precision, int32_t dim, int32_t B, const int32_t* h_qoff, int64_t n_docs,
                           const int64_t* h_doff, bool listed, const int64_t* h_pair_docs, const int64_t* h_poff,
                           bool want_matches) {
  const char* why = "";
  int64_t bad = -1;
  const int c = maxsim_check_args(dtype, precision, dim, B, h_qoff, n_docs, h_doff, listed, h_pair_docs, h_poff, want_matches,
                                  &why, &bad);
  if (c == 0) return NP_OK;
  if (bad >= 0)
    set_error("maxsim_batch: %s (pair %lld names document %lld, n_docs %lld)", why, (long long)bad,
              (long long)h_pair_docs[bad], (long long)n_docs);
  else
    set_error("%s: maxsim_batch: %s (dtype=%d precision=%d dim=%d)", c == 1 ? "Shape error" : "Search failed", why, dtype,
              precision, dim);
  return c == 1 ? NP_ERR_SHAPE : NP_ERR_INVALID_ARGUMENT;
}

int maxsim_device_ok(int32_t device, int* compute_units) {   // np_quant.hip and np_maxsim_b1.hip call it too
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    (void)hipGetLastError();
    set_error("no usable gfx950 device %d", device);
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  if (hipDeviceGetAttribute(compute_units, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
    (void)hipGetLastError();
    *compute_units = 256;
  }
  return NP_OK;
}

// every array on the device, the offsets also on the host; enqueues and returns
static int maxsim_run(hipStream_t st, int compute_units, int32_t dtype, int32_t precision, int32_t dim, const void* d_q,
                      const int32_t* d_qoff, const int32_t* h_qoff, int32_t B, const void* d_d, const int64_t* d_doff,
                      int64_t n_docs, const int64_t* d_pair_docs, const int64_t* d_poff, const int64_t* h_poff, float* d_scores,
                      float* d_sims, int32_t* d_pos, const float* d_qscale = nullptr, const float* d_dscale = nullptr,
                      bool long_queries = false) {
  const bool listed = d_pair_docs != nullptr;
  const int mode = precision == 0 ? 0 : dtype == NP_MS_DT_F32 ? 1 : 2;   // the _long entries take f32 / bf16 rows, or int8 rows
  const bool long_i8 = long_queries && dtype == NP_MS_DT_I8;
  const MaxsimLongPlan lplan = long_i8        ? maxsim_long_i8_plan(dim, listed, h_qoff, B, n_docs, h_poff, compute_units)
                               : long_queries ? maxsim_long_plan(mode, listed, h_qoff, B, n_docs, h_poff, compute_units)
                                              : MaxsimLongPlan();
  const MaxsimPlan plan = long_queries ? MaxsimPlan(lplan) : maxsim_plan(listed, h_qoff, B, n_docs, h_poff, compute_units);
  if (plan.gx <= 0 || plan.gy <= 0) return NP_OK;
  const size_t pitch = maxsim_row_bytes(dtype, dim, false), dpitch = maxsim_row_bytes(dtype, dim, true);
  MaxsimP p;
  p.Q = d_q;
  p.qoff = d_qoff;
  p.D = d_d;
  p.doff = d_doff;
  p.pair_docs = d_pair_docs;
  p.poff = d_poff;
  p.scores = d_scores;
  p.sims = d_sims;
  p.pos = d_pos;
  p.n_docs = n_docs;
  p.B = B;
  p.dim = dim;
  p.G = plan.G;
  p.nqt = plan.nqt;
  p.WD = plan.WD;
  p.y0 = 0;
  p.vecq = pitch % 16 == 0 && (uintptr_t)d_q % 16 == 0;
  p.vecd = dpitch % 16 == 0 && (uintptr_t)d_d % 16 == 0;
  p.qscale = d_qscale;
  p.dscale = d_dscale;
  if (long_i8) return maxsim_long_i8_launch(st, p, lplan);
  if (long_queries) return maxsim_long_launch(st, p, lplan, mode);
  if (dtype == NP_MS_DT_B1) return maxsim_b1_launch(st, p, plan);
  if (dtype == NP_MS_DT_I4) return maxsim_i4_launch(st, p, plan);
  if (dtype == NP_MS_DT_F16) return maxsim_f16_launch(st, p, plan);
  if (dtype == NP_MS_DT_I8) return maxsim_launch_mode<3>(st, p, plan);
  if (precision == 0) return maxsim_launch_mode<0>(st, p, plan);
  if (dtype == NP_MS_DT_F32) return maxsim_launch_mode<1>(st, p, plan);
  return maxsim_launch_mode<2>(st, p, plan);
}

// the int8 entries' checks (q_scales / d_scales non-NULL = the call is one of them)
static int maxsim_validate_i8(int32_t dim, const void* q_scales, int32_t B, const int32_t* h_qoff, const void* d_scales,
                              int64_t n_docs, const int64_t* h_doff, bool listed, const int64_t* h_pair_docs,
                              const int64_t* h_poff) {
  const char* why = "";
  int64_t bad = -1;
  const int c = maxsim_check_args_i8(dim, q_scales, B, h_qoff, d_scales, n_docs, h_doff, listed, h_pair_docs, h_poff, &why, &bad);
  if (c == 0) return NP_OK;
  if (bad >= 0)
    set_error("maxsim_batch_i8: %s (pair %lld names document %lld, n_docs %lld)", why, (long long)bad,
              (long long)h_pair_docs[bad], (long long)n_docs);
  else
    set_error("%s: maxsim_batch_i8: %s (dim=%d)", c == 1 ? "Shape error" : "Search failed", why, dim);
  return c == 1 ? NP_ERR_SHAPE : NP_ERR_INVALID_ARGUMENT;
}

// The device entries after their checks: every array in HBM.  d_q_scales / d_d_scales: the int8 and binary entries', NULL otherwise.
int maxsim_device_call(int32_t device, int32_t dtype, int32_t precision, int32_t dim, const void* d_queries,
                              const float* d_q_scales, const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                              const void* d_documents, const float* d_d_scales, const int64_t* d_doc_tok_offsets,
                              const int64_t* h_doc_tok_offsets, int64_t n_docs, const int64_t* d_pair_docs,
                              const int64_t* d_pair_offsets, const int64_t* h_pair_offsets, float* d_out_scores,
                              float* d_out_match_sims, int32_t* d_out_match_pos, void* stream, bool long_queries) {
  const bool listed = d_pair_docs != nullptr;
  const int64_t P = B <= 0 ? 0 : (listed ? h_pair_offsets[B] : (int64_t)B * n_docs);
  if (P == 0) return NP_OK;
  if (!d_q_tok_offsets || !d_doc_tok_offsets || !d_out_scores || (h_q_tok_offsets[B] > 0 && !d_queries) ||
      (h_doc_tok_offsets[n_docs] > 0 && !d_documents)) {
    set_error("Search failed: maxsim_batch: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  int cus = 0;
  NP_TRY(maxsim_device_ok(device, &cus));
  DeviceGuard g(device);
  return maxsim_run((hipStream_t)stream, cus, dtype, precision, dim, d_queries, d_q_tok_offsets, h_q_tok_offsets, B,
                    d_documents, d_doc_tok_offsets, n_docs, d_pair_docs, d_pair_offsets, h_pair_offsets, d_out_scores,
                    d_out_match_sims, d_out_match_pos, d_q_scales, d_d_scales, long_queries);
}

// The host entries after their checks: the call staged through one allocation.
int maxsim_host_call(int32_t device, int32_t dtype, int32_t precision, int32_t dim, const void* queries,
                            const float* q_scales, const int32_t* q_tok_offsets, int32_t B, const void* documents,
                            const float* d_scales, const int64_t* doc_tok_offsets, int64_t n_docs, const int64_t* pair_docs,
                            const int64_t* pair_offsets, float* out_scores, float* out_match_sims, int32_t* out_match_pos,
                            bool long_queries) {
  const bool listed = pair_docs != nullptr;
  const bool rows = out_match_sims || out_match_pos;
  const int64_t P = B <= 0 ? 0 : (listed ? pair_offsets[B] : (int64_t)B * n_docs);
  if (P == 0) return NP_OK;
  const int64_t qtok = q_tok_offsets[B], dtok = doc_tok_offsets[n_docs];
  if (!out_scores || (qtok > 0 && !queries) || (dtok > 0 && !documents)) {
    set_error("Search failed: maxsim_batch: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  int64_t R = 0;   // row entries
  if (rows)
    for (int b = 0; b < B; ++b)
      R += (listed ? pair_offsets[b + 1] - pair_offsets[b] : n_docs) * (int64_t)(q_tok_offsets[b + 1] - q_tok_offsets[b]);
  int cus = 0;
  NP_TRY(maxsim_device_ok(device, &cus));
  DeviceGuard g(device);
  // one allocation for the call: inputs (int8: and their scales), offsets, outputs, each on a 256-byte boundary
  const size_t n_q = (size_t)qtok * maxsim_row_bytes(dtype, dim, false), n_d = (size_t)dtok * maxsim_row_bytes(dtype, dim, true);
  const size_t b_q = up256(n_q), b_d = up256(n_d);
  const size_t b_qs = q_scales ? up256((size_t)qtok * 4) : 0, b_ds = d_scales ? up256((size_t)dtok * 4) : 0;
  const size_t b_qoff = up256((size_t)(B + 1) * 4), b_doff = up256((size_t)(n_docs + 1) * 8);
  const size_t b_ids = listed ? up256((size_t)P * 8) : 0, b_poff = listed ? up256((size_t)(B + 1) * 8) : 0;
  const size_t b_sc = up256((size_t)P * 4), b_sim = out_match_sims ? up256((size_t)R * 4) : 0;
  const size_t b_pos = out_match_pos ? up256((size_t)R * 4) : 0;
  DevPtr<char> buf;
  NP_TRY(buf.alloc(b_q + b_d + b_qs + b_ds + b_qoff + b_doff + b_ids + b_poff + b_sc + b_sim + b_pos));
  Carver carve{buf.get()};
  char* d_q = carve.take(b_q);
  char* d_d = carve.take(b_d);
  float* d_qs = q_scales ? (float*)carve.take(b_qs) : nullptr;
  float* d_ds = d_scales ? (float*)carve.take(b_ds) : nullptr;
  int32_t* d_qoff = (int32_t*)carve.take(b_qoff);
  int64_t* d_doff = (int64_t*)carve.take(b_doff);
  int64_t* d_ids = listed ? (int64_t*)carve.take(b_ids) : nullptr;
  int64_t* d_poff = listed ? (int64_t*)carve.take(b_poff) : nullptr;
  float* d_sc = (float*)carve.take(b_sc);
  float* d_sim = out_match_sims ? (float*)carve.take(b_sim) : nullptr;
  int32_t* d_pos = out_match_pos ? (int32_t*)carve.take(b_pos) : nullptr;
  if (qtok > 0) NP_HIP(hipMemcpy(d_q, queries, n_q, hipMemcpyHostToDevice));
  if (dtok > 0) NP_HIP(hipMemcpy(d_d, documents, n_d, hipMemcpyHostToDevice));
  if (d_qs && qtok > 0) NP_HIP(hipMemcpy(d_qs, q_scales, (size_t)qtok * 4, hipMemcpyHostToDevice));
  if (d_ds && dtok > 0) NP_HIP(hipMemcpy(d_ds, d_scales, (size_t)dtok * 4, hipMemcpyHostToDevice));
  NP_HIP(hipMemcpy(d_qoff, q_tok_offsets, (size_t)(B + 1) * 4, hipMemcpyHostToDevice));
  NP_HIP(hipMemcpy(d_doff, doc_tok_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice));
  if (listed) {
    NP_HIP(hipMemcpy(d_ids, pair_docs, (size_t)P * 8, hipMemcpyHostToDevice));
    NP_HIP(hipMemcpy(d_poff, pair_offsets, (size_t)(B + 1) * 8, hipMemcpyHostToDevice));
  }
  NP_TRY(maxsim_run(nullptr, cus, dtype, precision, dim, d_q, d_qoff, q_tok_offsets, B, d_d, d_doff, n_docs, d_ids, d_poff,
                    pair_offsets, d_sc, d_sim, d_pos, d_qs, d_ds, long_queries));
  NP_HIP(hipMemcpy(out_scores, d_sc, (size_t)P * 4, hipMemcpyDeviceToHost));
  if (d_sim && R > 0) NP_HIP(hipMemcpy(out_match_sims, d_sim, (size_t)R * 4, hipMemcpyDeviceToHost));
  if (d_pos && R > 0) NP_HIP(hipMemcpy(out_match_pos, d_pos, (size_t)R * 4, hipMemcpyDeviceToHost));
  return NP_OK;
}

// pair_docs and pair_offsets (the device entries: and the host copy) go together; *listed = they are there
int maxsim_pair_args(bool all, bool any, bool device_entry, bool* listed) {
  *listed = any;
  if (any && !all) {
    set_error(device_entry ? "Search failed: maxsim_batch: pair_docs and pair_offsets (device and host copy) go together, or all NULL"
                           : "Search failed: maxsim_batch: pair_docs and pair_offsets go together, or both NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_maxsim_batch_device(int32_t device, int32_t dtype, int32_t precision, int32_t dim, const void* d_queries,
                               const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                               const void* d_documents, const int64_t* d_doc_tok_offsets, const int64_t* h_doc_tok_offsets,
                               int64_t n_docs, const int64_t* d_pair_docs, const int64_t* d_pair_offsets,
                               const int64_t* h_pair_offsets, float* d_out_scores, float* d_out_match_sims,
                               int32_t* d_out_match_pos, void* stream) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(d_pair_docs && d_pair_offsets && h_pair_offsets, d_pair_docs || d_pair_offsets || h_pair_offsets, true,
                          &listed));
  NP_TRY(maxsim_validate(dtype, precision, dim, B, h_q_tok_offsets, n_docs, h_doc_tok_offsets, listed, nullptr, h_pair_offsets,
                         d_out_match_sims || d_out_match_pos));
  return maxsim_device_call(device, dtype, precision, dim, d_queries, nullptr, d_q_tok_offsets, h_q_tok_offsets, B, d_documents,
                            nullptr, d_doc_tok_offsets, h_doc_tok_offsets, n_docs, d_pair_docs, d_pair_offsets, h_pair_offsets,
                            d_out_scores, d_out_match_sims, d_out_match_pos, stream);
}

int np_hip_maxsim_batch(int32_t device, int32_t dtype, int32_t precision, int32_t dim, const void* queries,
                        const int32_t* q_tok_offsets, int32_t B, const void* documents, const int64_t* doc_tok_offsets,
                        int64_t n_docs, const int64_t* pair_docs, const int64_t* pair_offsets, float* out_scores,
                        float* out_match_sims, int32_t* out_match_pos) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(pair_docs && pair_offsets, pair_docs || pair_offsets, false, &listed));
  NP_TRY(maxsim_validate(dtype, precision, dim, B, q_tok_offsets, n_docs, doc_tok_offsets, listed, pair_docs, pair_offsets,
                         out_match_sims || out_match_pos));
  return maxsim_host_call(device, dtype, precision, dim, queries, nullptr, q_tok_offsets, B, documents, nullptr, doc_tok_offsets,
                          n_docs, pair_docs, pair_offsets, out_scores, out_match_sims, out_match_pos);
}

int np_hip_maxsim_batch_i8_device(int32_t device, int32_t dim, const int8_t* d_queries, const float* d_q_scales,
                                  const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                                  const int8_t* d_documents, const float* d_d_scales, const int64_t* d_doc_tok_offsets,
                                  const int64_t* h_doc_tok_offsets, int64_t n_docs, const int64_t* d_pair_docs,
                                  const int64_t* d_pair_offsets, const int64_t* h_pair_offsets, float* d_out_scores,
                                  float* d_out_match_sims, int32_t* d_out_match_pos, void* stream) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(d_pair_docs && d_pair_offsets && h_pair_offsets, d_pair_docs || d_pair_offsets || h_pair_offsets, true,
                          &listed));
  NP_TRY(maxsim_validate_i8(dim, d_q_scales, B, h_q_tok_offsets, d_d_scales, n_docs, h_doc_tok_offsets, listed, nullptr,
                            h_pair_offsets));
  return maxsim_device_call(device, NP_MS_DT_I8, 0, dim, d_queries, d_q_scales, d_q_tok_offsets, h_q_tok_offsets, B, d_documents,
                            d_d_scales, d_doc_tok_offsets, h_doc_tok_offsets, n_docs, d_pair_docs, d_pair_offsets, h_pair_offsets,
                            d_out_scores, d_out_match_sims, d_out_match_pos, stream);
}

int np_hip_maxsim_batch_i8(int32_t device, int32_t dim, const int8_t* queries, const float* q_scales,
                           const int32_t* q_tok_offsets, int32_t B, const int8_t* documents, const float* d_scales,
                           const int64_t* doc_tok_offsets, int64_t n_docs, const int64_t* pair_docs, const int64_t* pair_offsets,
                           float* out_scores, float* out_match_sims, int32_t* out_match_pos) {
  clear_error();
  bool listed;
  NP_TRY(maxsim_pair_args(pair_docs && pair_offsets, pair_docs || pair_offsets, false, &listed));
  NP_TRY(maxsim_validate_i8(dim, q_scales, B, q_tok_offsets, d_scales, n_docs, doc_tok_offsets, listed, pair_docs, pair_offsets));
  return maxsim_host_call(device, NP_MS_DT_I8, 0, dim, queries, q_scales, q_tok_offsets, B, documents, d_scales, doc_tok_offsets,
                          n_docs, pair_docs, pair_offsets, out_scores, out_match_sims, out_match_pos);
}

}  // extern "C"
