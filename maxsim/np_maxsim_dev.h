// np_maxsim_dev.h -- what the batched-MaxSim kernels share: maxsim_kernel (np_maxsim.hip), maxsim_b1_kernel
// (np_maxsim_b1.hip), maxsim_i4_kernel (np_maxsim_i4.hip) and maxsim_f16_kernel (np_maxsim_f16.hip) take the same launch arguments, the int8 LDS geometry and the scaled argmax walk; the entries of both
// files go through the same staging (np_maxsim.hip defines it).  maxsim_long_kernel (np_maxsim_long.hip) also takes the
// staging helpers of modes 0 to 2 from here.
#pragma once
#include "np_internal.h"
#include "np_exact.h"
#include "np_maxsim_plan.h"

namespace np {

struct MaxsimP {
  const void* Q;             // [q tokens][dim]
  const int32_t* qoff;       // [B + 1]
  const void* D;             // [d tokens][dim]; binary / int4 rows: [d tokens][ceil(dim / 32 or 8)] words
  const int64_t* doff;       // [n_docs + 1]
  const int64_t* pair_docs;  // NULL = all pairs
  const int64_t* poff;       // [B + 1] (listed form)
  float* scores;
  float* sims;               // NULL, or a row entry per (pair, query token)
  int32_t* pos;              // ...
  int64_t n_docs;
  int B, dim, G, nqt, WD;
  int y0;                    // blockIdx.y of this launch starts here (launches are slices of NP_MS_MAX_GRID_Y)
  int vecq, vecd;            // 16-byte loads are legal for every row of Q / D
  const float* qscale;       // int8, binary and int4 rows: [q tokens], [d tokens]
  const float* dscale;
};

constexpr int NP_MS_BROW = 72;                         // bf16 LDS row pitch in elements
constexpr int NP_MS_META = 128;                        // bytes: the row base, the documents' offsets, lengths and flags
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// sixteen int8 dims k0 .. k0 + 15 of a row
__device__ __forceinline__ uint4 ms_load16b(const uint8_t* rowp, int k0, int dim, bool vec) {
  uint4 r = make_uint4(0u, 0u, 0u, 0u);
  if (!rowp || k0 >= dim) return r;
  if (vec) return *reinterpret_cast<const uint4*>(rowp + k0);   // dim % 16 == 0: k0 + 16 <= dim
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (k0 + i < dim) w[i >> 2] |= (uint32_t)rowp[k0 + i] << (8 * (i & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// tile_row_argmax's walk over f32(acc[r]) * sc[r] (sc = the scales of rows mfma_row(r, kk)), compared as keys: okey is 0 for
// a non-finite product and grows with a finite one, so `best` ends as the key the workgroup's atomicMax takes.
__device__ __forceinline__ void ms_row_argmax_i8(const i32x16& acc, const float (&sc)[16], int64_t t0, int64_t len, int kk,
                                                 uint32_t& best, int& pos) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t trow = t0 + mfma_row(r, kk);
    const uint32_t k = okey((float)acc[r] * sc[r]);
    if (trow < len && k > best) {
      best = k;
      pos = (int)trow;
    }
  }
}

// ---- the staging of modes 0 to 3, shared by maxsim_kernel (np_maxsim.hip) and maxsim_long_kernel (np_maxsim_long.hip) ------
template <int MODE> struct MsRaw { uint4 v[MODE == 1 ? 2 : 1]; };   // one staging unit on its way from HBM to LDS

template <int MODE, int NQT> struct MsLds {
  static constexpr int KC = MODE == 0 ? NP_MS_KC_F32 : MODE == 3 ? NP_MS_KC_I8 : NP_MS_KC_BF16;
  static constexpr int R = NQT * 32;                               // slot rows
  static constexpr int SQ = (NQT & 1) ? R : R + 32;                // f32: floats between two k rows of the slots
  static constexpr size_t Q_BYTES = MODE == 0 ? (size_t)KC * SQ * 4 : (size_t)R * NP_MS_BROW * 2;
  static constexpr size_t D_BYTES = MODE == 0 ? (size_t)KC * 32 * 4 : (size_t)32 * NP_MS_BROW * 2;
  static constexpr size_t KEY_OFF = Q_BYTES + 4 * D_BYTES;
  static constexpr size_t QROW_OFF = KEY_OFF + (size_t)NP_MS_WG_DOCS * R * 8;
  static constexpr size_t META_OFF = QROW_OFF + (size_t)R * 8;
  static constexpr size_t BYTES = META_OFF + NP_MS_META;
};

// four f32 dims k0 .. k0 + 3 of a row (NULL = a row past the end), zeros past `dim`
__device__ __forceinline__ uint4 ms_load4f(const float* rowp, int k0, int dim, bool vec) {
  uint4 r = make_uint4(0u, 0u, 0u, 0u);
  if (!rowp || k0 >= dim) return r;
  if (vec) return *reinterpret_cast<const uint4*>(rowp + k0);   // dim % 4 == 0: k0 + 4 <= dim
  r.x = __float_as_uint(rowp[k0]);
  if (k0 + 1 < dim) r.y = __float_as_uint(rowp[k0 + 1]);
  if (k0 + 2 < dim) r.z = __float_as_uint(rowp[k0 + 2]);
  if (k0 + 3 < dim) r.w = __float_as_uint(rowp[k0 + 3]);
  return r;
}
// eight bf16 dims k0 .. k0 + 7 of a row
__device__ __forceinline__ uint4 ms_load8h(const uint16_t* rowp, int k0, int dim, bool vec) {
  uint4 r = make_uint4(0u, 0u, 0u, 0u);
  if (!rowp || k0 >= dim) return r;
  if (vec) return *reinterpret_cast<const uint4*>(rowp + k0);   // dim % 8 == 0: k0 + 8 <= dim
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (k0 + i < dim) w[i >> 1] |= (uint32_t)rowp[k0 + i] << (16 * (i & 1));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int MODE>
__device__ __forceinline__ MsRaw<MODE> ms_load(const void* base, int64_t row, int dim, int k0, bool vec) {
  MsRaw<MODE> r;
  if (MODE == 3) {
    r.v[0] = ms_load16b(row < 0 ? nullptr : static_cast<const uint8_t*>(base) + row * dim, k0, dim, vec);
  } else if (MODE == 2) {
    r.v[0] = ms_load8h(row < 0 ? nullptr : static_cast<const uint16_t*>(base) + row * dim, k0, dim, vec);
  } else {
    const float* rp = row < 0 ? nullptr : static_cast<const float*>(base) + row * dim;
    r.v[0] = ms_load4f(rp, k0, dim, vec);
    if (MODE == 1) r.v[MODE == 1 ? 1 : 0] = ms_load4f(rp, k0 + 4, dim, vec);
  }
  return r;
}

__device__ __forceinline__ uint32_t ms_bf16_pair(uint32_t lo_f32, uint32_t hi_f32) {   // nearest, ties to even
  const uint16_t a = __builtin_bit_cast(uint16_t, (__bf16)__uint_as_float(lo_f32));
  const uint16_t b = __builtin_bit_cast(uint16_t, (__bf16)__uint_as_float(hi_f32));
  return (uint32_t)a | ((uint32_t)b << 16);
}

// unit (row, g) of a region to LDS (int8 units are 16 bytes at 16 g like bf16 ones).  f32: `S` floats between k rows, the unit's dims are k rows 4g .. 4g + 3, written in
// opposite order by even and odd g (the two halves of a wave differ in g's parity or in the bank of `row`).
template <int MODE>
__device__ __forceinline__ void ms_store(unsigned char* region, int S, int row, int g, const MsRaw<MODE>& r) {
  if (MODE == 0) {
    float* s = reinterpret_cast<float*>(region);
    const uint32_t v[4] = {r.v[0].x, r.v[0].y, r.v[0].z, r.v[0].w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int a = (4 * g + i) * S + row, b = (4 * g + (i ^ 1)) * S + row;
      s[(g & 1) ? b : a] = __uint_as_float((g & 1) ? v[i ^ 1] : v[i]);
    }
  } else {
    uint4 w = r.v[0];
    if (MODE == 1) {
      const uint4 hi = r.v[MODE == 1 ? 1 : 0];
      w = make_uint4(ms_bf16_pair(r.v[0].x, r.v[0].y), ms_bf16_pair(r.v[0].z, r.v[0].w), ms_bf16_pair(hi.x, hi.y),
                     ms_bf16_pair(hi.z, hi.w));
    }
    *reinterpret_cast<uint4*>(region + ((size_t)row * NP_MS_BROW + 8 * g) * 2) = w;
  }
}

// unit u of a region of `rows` rows (a power of two >= 32): f32 walks the rows first (consecutive banks on the transposed
// write), bf16 the eight 16-byte units of a row first (a row's 128 bytes per eight lanes, on the load and on the write)
template <int MODE>
__device__ __forceinline__ void ms_unit(int u, int rows, int& row, int& g) {
  if (MODE == 0) {
    row = u & (rows - 1);
    g = u / rows;
  } else {
    g = u & 7;
    row = u >> 3;
  }
}

// tile_row_argmax's shape without row scales: rows t0 + mfma_row(r, kk) of one accumulator, entries of rows past `len`
// and non-finite entries ignored; ascending rows and the strict `>` keep the lowest position of this lane's rows.
__device__ __forceinline__ void ms_row_argmax(const f32x16& acc, int64_t t0, int64_t len, int kk, float& mm, int& pos) {
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

// ---- host (np_maxsim.hip) --------------------------------------------------------------------------------------------
int maxsim_device_ok(int32_t device, int* compute_units);
// pair_docs and pair_offsets (the device entries: and the host copy) go together; *listed = they are there
int maxsim_pair_args(bool all, bool any, bool device_entry, bool* listed);
// The entries after their checks.  dtype NP_MS_DT_B1 / NP_MS_DT_I4: queries are int8 rows, documents rows of bit / nibble words.
// long_queries: the _long entries: maxsim_long_plan and maxsim_long_kernel (f32 / bf16 rows) or maxsim_long_i8_plan and
// maxsim_long_i8_kernel (NP_MS_DT_I8) instead of maxsim_plan's kernels.
int maxsim_device_call(int32_t device, int32_t dtype, int32_t precision, int32_t dim, const void* d_queries,
                       const float* d_q_scales, const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                       const void* d_documents, const float* d_d_scales, const int64_t* d_doc_tok_offsets,
                       const int64_t* h_doc_tok_offsets, int64_t n_docs, const int64_t* d_pair_docs, const int64_t* d_pair_offsets,
                       const int64_t* h_pair_offsets, float* d_out_scores, float* d_out_match_sims, int32_t* d_out_match_pos,
                       void* stream, bool long_queries = false);
int maxsim_host_call(int32_t device, int32_t dtype, int32_t precision, int32_t dim, const void* queries, const float* q_scales,
                     const int32_t* q_tok_offsets, int32_t B, const void* documents, const float* d_scales,
                     const int64_t* doc_tok_offsets, int64_t n_docs, const int64_t* pair_docs, const int64_t* pair_offsets,
                     float* out_scores, float* out_match_sims, int32_t* out_match_pos, bool long_queries = false);
// np_maxsim_long.hip: the launches of maxsim_long_kernel<mode, plan.NQT> (mode 0, 1 or 2 of np_maxsim.hip)
int maxsim_long_launch(hipStream_t st, MaxsimP p, const MaxsimLongPlan& plan, int mode);
// np_maxsim_long_i8.hip: the launches of maxsim_long_i8_kernel<plan.NQT> (long_queries with NP_MS_DT_I8; maxsim_long_i8_plan)
int maxsim_long_i8_launch(hipStream_t st, MaxsimP p, const MaxsimLongPlan& plan);
// np_maxsim_b1.hip: the launches of maxsim_b1_kernel for a filled MaxsimP
int maxsim_b1_launch(hipStream_t st, MaxsimP p, const MaxsimPlan& plan);
// np_maxsim_i4.hip: the launches of maxsim_i4_kernel
int maxsim_i4_launch(hipStream_t st, MaxsimP p, const MaxsimPlan& plan);
// np_maxsim_f16.hip: the launches of maxsim_f16_kernel (Q and D are f16 rows; no scales)
int maxsim_f16_launch(hipStream_t st, MaxsimP p, const MaxsimPlan& plan);

}  // namespace np
