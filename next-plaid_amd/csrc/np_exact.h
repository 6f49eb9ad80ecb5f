// np_exact.h -- the device pieces of exact MaxSim that more than one kernel file uses: the orderable score key, the
// decompression of one 32-token tile straight into MFMA A fragments, the row scales and the masked row maximum.
// exact_f32_kernel / exact_bf16_kernel (np_kernels.h, S6: one query, its selected documents) and scan_kernel (np_scan.hip:
// every document, many queries) call these same definitions, so a (query, document) pair gets the same bits from both.
// Included after np_internal.h (CodeArr).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace np {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define NP_NEG_INF (-__builtin_huge_valf())
#define NP_MAX_QT 8      // query tiles of 32 tokens (LQP <= 256); exact kernels are instantiated for 1, 2 and 8

// Orderable key of search.rs:110-117's comparator: finite values keep f32::total_cmp order in
// [0x00800000, 0xFF7FFFFF]; every non-finite value maps to 0 (all Equal, below any finite).
__device__ __forceinline__ uint32_t okey(float x) {
  uint32_t b = __float_as_uint(x);
  uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((b & 0x7F800000u) == 0x7F800000u) ? 0u : k;
}
__device__ __forceinline__ float unkey(uint32_t k) {  // inverse for k != 0
  uint32_t b = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
  return __uint_as_float(b);
}
__device__ __forceinline__ bool finitef(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ float readlane_f(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ int mfma_row(int r, int kk) { return (r & 3) + 8 * (r >> 2) + 4 * kk; }

template <int NBITS>
__device__ __forceinline__ float seg_weight(const float* sW, uint32_t byte, int e) {
  constexpr uint32_t MASK = (1u << NBITS) - 1u;
  return sW[(byte >> (8 - NBITS * (e + 1))) & MASK];  // segment e: 0 = highest bits = first dim
}

// ---- decompress (codec.rs:443-467), one token per lane pair ---------------------------------------------------------
// f32 form: lane (tok, kk) unpacks dims [kk * DIM/2, +DIM/2) of token `tok` into v[] (centroid + bucket weight, not yet
// normalised: v[s] is the A operand of the s-th 32x32x2 MFMA) and returns its sum of squares.  sW: the bucket weights in LDS.
template <int DIM, int NBITS>
__device__ __forceinline__ float unpack_row_f32(const float* sW, const float* __restrict__ centroids,
                                                const uint8_t* __restrict__ residuals, uint32_t code, int64_t tok, int kk,
                                                float (&v)[DIM / 2]) {
  constexpr int H = DIM / 2;              // dims per lane
  constexpr int PD = DIM * NBITS / 8;     // bytes per token
  constexpr int PH = PD / 2;              // bytes per lane
  constexpr int PER = 8 / NBITS;          // dims per byte
  static_assert(PH % 4 == 0 && H % 4 == 0, "unsupported DIM/NBITS");
  const uint32_t* rp = reinterpret_cast<const uint32_t*>(residuals + tok * PD + kk * PH);
  const float4* cp = reinterpret_cast<const float4*>(centroids + (int64_t)code * DIM + kk * H);
  float ss = 0.f;
#pragma unroll
  for (int w = 0; w < PH / 4; ++w) {
    const uint32_t word = rp[w];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t byte = (word >> (8 * i)) & 0xFFu;
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const int jdim = (w * 4 + i) * PER + e;
        const float c = reinterpret_cast<const float*>(cp)[jdim];
        const float x = c + seg_weight<NBITS>(sW, byte, e);
        v[jdim] = x;
        ss = fmaf(x, x, ss);
      }
    }
  }
  return ss;
}

// bf16 form: A fragment s of lane (tok, kk) = dims [16s + 8kk, +8), rounded to bf16 un-normalised (rows are scaled after the
// MFMA); the returned sum of squares is taken over the f32 values.
template <int DIM, int NBITS>
__device__ __forceinline__ float unpack_row_bf16(const float* sW, const float* __restrict__ centroids,
                                                 const uint8_t* __restrict__ residuals, uint32_t code, int64_t tok, int kk,
                                                 bf16x8 (&a)[DIM / 16]) {
  constexpr int NS = DIM / 16;            // MFMA k-steps
  constexpr int PD = DIM * NBITS / 8;
  constexpr int PER = 8 / NBITS;
  static_assert(DIM % 16 == 0 && (NBITS == 2 || NBITS == 4), "unsupported DIM/NBITS");
  const uint8_t* rp = residuals + tok * PD;
  const float* cp = centroids + (int64_t)code * DIM;
  float ss = 0.f;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int d0 = 16 * s + 8 * kk;
    const float4 c0 = *reinterpret_cast<const float4*>(cp + d0);
    const float4 c1 = *reinterpret_cast<const float4*>(cp + d0 + 4);
    const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    uint32_t word;
    if (NBITS == 4) word = *reinterpret_cast<const uint32_t*>(rp + d0 / 2);
    else word = *reinterpret_cast<const uint16_t*>(rp + d0 / 4);
#pragma unroll
    for (int i = 0; i < 8 / PER; ++i) {
      const uint32_t byte = (word >> (8 * i)) & 0xFFu;
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const float x = cc[i * PER + e] + seg_weight<NBITS>(sW, byte, e);
        a[s][i * PER + e] = (__bf16)x;
        ss = fmaf(x, x, ss);
      }
    }
  }
  return ss;
}

// 1/||row|| is applied to the MFMA output rows (S[t][q] = rn[t] * <raw_t, q>) instead of to the fragment values: the two
// halves of a token exchange their sums of squares, lane li then holds rn of token t0 + li, and row r of this lane needs
// token t0 + mfma_row(r, kk).  pad_ss: see ExactP::pad_ss.  An invalid (past-the-end) token scales by 0.
__device__ __forceinline__ void row_scales(float ss, float pad_ss, bool valid, int kk, float (&rrow)[16]) {
  const float tot = ss + __shfl_xor(ss, 32) - pad_ss;
  const float rn = valid ? 1.0f / fmaxf(sqrtf(tot), 1e-12f) : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) rrow[r] = __shfl(rn, mfma_row(r, kk));
}

// maxsim.rs:281-291 for one (document tile, query tile): mm = max(mm, scaled similarities of the tile's valid tokens),
// non-finite entries ignored; this lane holds query token lane & 31 and the rows mfma_row(r, kk).
__device__ __forceinline__ float tile_row_max(const f32x16& acc, const float (&rrow)[16], int t0, int len, int kk, float mm) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int trow = t0 + mfma_row(r, kk);
    const float x = acc[r] * rrow[r];
    if (trow < len && finitef(x)) mm = fmaxf(mm, x);
  }
  return mm;
}

// The same with the position of the maximum (np_pairs.hip): mm takes tile_row_max's very updates, so it holds the same
// bits; pos = the document token that first reached it.  mfma_row(r, kk) ascends in r and tiles ascend, so with the strict
// `>` the lowest index of this lane's rows wins, within a tile and across tiles.  pos stays as given (-1) while no entry is finite.
__device__ __forceinline__ void tile_row_argmax(const f32x16& acc, const float (&rrow)[16], int t0, int len, int kk, float& mm,
                                                int& pos) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int trow = t0 + mfma_row(r, kk);
    const float x = acc[r] * rrow[r];
    if (trow < len && finitef(x)) {
      pos = x > mm ? trow : pos;
      mm = fmaxf(mm, x);
    }
  }
}

// ... and its q-ordered sum over the nq tokens of one query tile, continued from `total`: mm = the tile's running maxima
// (both halves still apart); a token without a finite similarity adds nothing.
__device__ __forceinline__ float tile_sum(float m, int nq, float total) {
  const float mm = fmaxf(m, __shfl_xor(m, 32));
  for (int qi = 0; qi < nq; ++qi) {
    const float x = readlane_f(mm, qi);
    if (x > NP_NEG_INF) total += x;
  }
  return total;
}

}  // namespace np
