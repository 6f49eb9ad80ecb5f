// np_maxsim_dev.h -- what the batched-MaxSim kernels share: maxsim_kernel (np_maxsim.hip), maxsim_b1_kernel
// (np_maxsim_b1.hip), maxsim_i4_kernel (np_maxsim_i4.hip) and maxsim_f16_kernel (np_maxsim_f16.hip) take the same launch arguments, the int8 LDS geometry and the scaled argmax walk; the entries of both
// files go through the same staging (np_maxsim.hip defines it).
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

// ---- host (np_maxsim.hip) --------------------------------------------------------------------------------------------
int maxsim_device_ok(int32_t device, int* compute_units);
// pair_docs and pair_offsets (the device entries: and the host copy) go together; *listed = they are there
int maxsim_pair_args(bool all, bool any, bool device_entry, bool* listed);
// The entries after their checks.  dtype NP_MS_DT_B1 / NP_MS_DT_I4: queries are int8 rows, documents rows of bit / nibble words.
int maxsim_device_call(int32_t device, int32_t dtype, int32_t precision, int32_t dim, const void* d_queries,
                       const float* d_q_scales, const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                       const void* d_documents, const float* d_d_scales, const int64_t* d_doc_tok_offsets,
                       const int64_t* h_doc_tok_offsets, int64_t n_docs, const int64_t* d_pair_docs, const int64_t* d_pair_offsets,
                       const int64_t* h_pair_offsets, float* d_out_scores, float* d_out_match_sims, int32_t* d_out_match_pos,
                       void* stream);
int maxsim_host_call(int32_t device, int32_t dtype, int32_t precision, int32_t dim, const void* queries, const float* q_scales,
                     const int32_t* q_tok_offsets, int32_t B, const void* documents, const float* d_scales,
                     const int64_t* doc_tok_offsets, int64_t n_docs, const int64_t* pair_docs, const int64_t* pair_offsets,
                     float* out_scores, float* out_match_sims, int32_t* out_match_pos);
// np_maxsim_b1.hip: the launches of maxsim_b1_kernel for a filled MaxsimP
int maxsim_b1_launch(hipStream_t st, MaxsimP p, const MaxsimPlan& plan);
// np_maxsim_i4.hip: the launches of maxsim_i4_kernel
int maxsim_i4_launch(hipStream_t st, MaxsimP p, const MaxsimPlan& plan);
// np_maxsim_f16.hip: the launches of maxsim_f16_kernel (Q and D are f16 rows; no scales)
int maxsim_f16_launch(hipStream_t st, MaxsimP p, const MaxsimPlan& plan);

}  // namespace np
