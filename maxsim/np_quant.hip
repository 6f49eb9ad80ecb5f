// np_quant.hip -- np_hip_quantize_rows_i8: f32 or bf16 rows to int8 codes with one f32 scale per row, the operands of
// np_hip_maxsim_batch_i8 (np_maxsim.hip, MODE 3); np_hip_pack_rows_b1 (further down): the same rows to one bit per dim; and
// np_hip_quantize_rows_i4 (after it): the same rows to one nibble per dim.
//
//   rule          per row: a = max_d |x_d|, scale = a / 127, inv = 127 / a (both correctly rounded f32 divisions),
//                 code_d = clamp(rintf(x_d * inv), -127, 127) (one f32 product, nearest with ties to even).  a == 0: scale 0,
//                 codes 0.  A row with a non-finite element: scale NaN, codes 0 (MODE 3 ignores every product of such a row).
//                 bf16 input is widened to f32 exactly.  tests/maxsim_i8_restate.py is the same rule in numpy, bit for bit.
//   work split    one wave per row, four rows per workgroup.  A unit is 16 bytes of input: 4 f32 or 8 bf16 elements.  Lane l
//                 takes units l, l + 64, ...: a wave's load instruction reads 1 KB of consecutive bytes, and dim <= 1024 is
//                 at most 4 (f32) or 2 (bf16) units a lane, which stay in registers between the two passes -- a row is read
//                 from HBM once.  The absolute maximum and the non-finite flag cross the wave by shuffles; no LDS, no atomics.
//   stores        a unit's codes leave as one packed 4-byte (f32 input) or 8-byte (bf16 input) store, consecutive across
//                 the lanes.  16-byte loads and packed stores are used where the call allows them for every row (base
//                 pointers and row pitches multiples of the access), otherwise element loads and byte stores.
#include "np_internal.h"
#include "np_maxsim_plan.h"

namespace np {

struct QuantP {
  const void* rows;   // [n_rows][dim] f32 or bf16
  int8_t* codes;      // [n_rows][dim]
  float* scales;      // [n_rows]
  int64_t n_rows;
  int dim;
  int vec_in, vec_out;   // 16-byte loads / packed stores are legal for every row
};

// BF = bf16 input.  EL elements per unit, NU units per lane cover dim <= 1024.
template <bool BF>
__global__ void __launch_bounds__(256) quantize_rows_kernel(QuantP p) {
  constexpr int EL = BF ? 8 : 4, NU = NP_MS_MAX_DIM / (64 * EL);
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.n_rows) return;   // a whole wave; the kernel has no barrier
  const int dim = p.dim;
  float x[NU][EL];
  uint32_t amax = 0u, bad = 0u;   // |x| as bits: for finite values the integer order is the f32 order
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int k0 = (u * 64 + lane) * EL;
    uint32_t w[4] = {0u, 0u, 0u, 0u};   // the unit's 16 bytes, zeros past dim
    if (k0 < dim) {
      if (p.vec_in) {
        const uint4 v = *reinterpret_cast<const uint4*>(static_cast<const char*>(p.rows) + ((size_t)row * dim + k0) * (BF ? 2 : 4));
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      } else if (BF) {
        const uint16_t* rp = static_cast<const uint16_t*>(p.rows) + (size_t)row * dim;
#pragma unroll
        for (int i = 0; i < EL; ++i)
          if (k0 + i < dim) w[i >> 1] |= (uint32_t)rp[k0 + i] << (16 * (i & 1));
      } else {
        const uint32_t* rp = static_cast<const uint32_t*>(p.rows) + (size_t)row * dim;
#pragma unroll
        for (int i = 0; i < EL; ++i)
          if (k0 + i < dim) w[i] = rp[k0 + i];
      }
    }
#pragma unroll
    for (int i = 0; i < EL; ++i) {
      const uint32_t b = BF ? (w[i >> 1] >> (16 * (i & 1))) << 16 : w[i];
      x[u][i] = __uint_as_float(b);
      const uint32_t mag = b & 0x7FFFFFFFu;
      bad |= mag >= 0x7F800000u ? 1u : 0u;
      amax = mag > amax ? mag : amax;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)amax, d);
    amax = o > amax ? o : amax;
    bad |= (uint32_t)__shfl_xor((int)bad, d);
  }
  const float a = __uint_as_float(amax);
  const bool zero = bad || amax == 0u;            // every code is 0
  const float inv = zero ? 0.f : __fdiv_rn(127.0f, a);
  if (lane == 0) p.scales[row] = bad ? __uint_as_float(0x7FC00000u) : __fdiv_rn(a, 127.0f);
  int8_t* out = p.codes + (size_t)row * dim;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int k0 = (u * 64 + lane) * EL;
    if (k0 >= dim) continue;
    uint32_t c[EL / 4] = {};
#pragma unroll
    for (int i = 0; i < EL; ++i) {
      const float r = zero ? 0.f : fminf(fmaxf(rintf(x[u][i] * inv), -127.0f), 127.0f);
      c[i >> 2] |= ((uint32_t)(int)r & 0xFFu) << (8 * (i & 3));
    }
    if (p.vec_out) {
      if (BF) *reinterpret_cast<uint2*>(out + k0) = make_uint2(c[0], c[EL / 4 - 1]);
      else *reinterpret_cast<uint32_t*>(out + k0) = c[0];
    } else {
#pragma unroll
      for (int i = 0; i < EL; ++i)
        if (k0 + i < dim) out[k0 + i] = (int8_t)(c[i >> 2] >> (8 * (i & 3)));
    }
  }
}

static int quantize_validate(int32_t dtype, int32_t dim, int64_t n_rows, const void* rows, const void* codes, const void* scales) {
  const char* why = "";
  const int c = quantize_check_args(dtype, dim, n_rows, rows, codes, scales, &why);
  if (c == 0) return NP_OK;
  set_error("%s: quantize_rows_i8: %s (dtype=%d dim=%d)", c == 1 ? "Shape error" : "Search failed", why, dtype, dim);
  return c == 1 ? NP_ERR_SHAPE : NP_ERR_INVALID_ARGUMENT;
}

// every array on the device; enqueues and returns
static int quantize_run(hipStream_t st, int32_t dtype, int32_t dim, const void* d_rows, int64_t n_rows, int8_t* d_codes,
                        float* d_scales) {
  const bool bf = dtype == NP_MS_DT_BF16;
  const size_t pitch = (size_t)dim * (bf ? 2 : 4), unit = bf ? 8 : 4;   // bytes of an input row, codes of a packed store
  QuantP p;
  p.rows = d_rows;
  p.codes = d_codes;
  p.scales = d_scales;
  p.n_rows = n_rows;
  p.dim = dim;
  p.vec_in = pitch % 16 == 0 && (uintptr_t)d_rows % 16 == 0;
  p.vec_out = dim % unit == 0 && (uintptr_t)d_codes % unit == 0;
  const unsigned grid = (unsigned)((n_rows + 3) / 4);
  if (bf) quantize_rows_kernel<true><<<grid, 256, 0, st>>>(p);
  else quantize_rows_kernel<false><<<grid, 256, 0, st>>>(p);
  NP_HIP(hipGetLastError());
  return NP_OK;
}

// ---- np_hip_pack_rows_b1: rows to one bit per dim and one f32 scale per row (np_maxsim_b1.hip's documents) --------------
//   rule          bit_d = x_d >= 0 (so +-0.0 gives a set bit, a NaN a clear one); bit j of word w is dim 32 w + j and the pad
//                 bits of the last word are 0.  scale = (sum_d |x_d|) / dim, the least-squares s of s * sign(x): f32 sums in
//                 the order below, then one correctly rounded division by f32(dim).  A row with a non-finite element: NaN.
//   work split    the quantiser's: one wave per row, lane l takes the 16-byte units l, l + 64, ..., a row is read once.  A
//                 lane's 4 (f32) or 8 (bf16) bits are shifted to their place in the word and OR-ed across the 8 or 4 lanes
//                 that share a word (xor shuffles); the group's first lane stores the word, consecutive words across the wave.
//   sum order     a lane adds its own |x| in ascending dim order to 0.0f; then s = s + s[lane ^ d] for d = 32, 16, .., 1.
struct PackP {
  const void* rows;   // [n_rows][dim] f32 or bf16
  uint32_t* bits;     // [n_rows][ceil(dim / 32)]
  float* scales;      // [n_rows]
  int64_t n_rows;
  int dim;
  int vec_in;         // 16-byte loads are legal for every row
};

template <bool BF>
__global__ void __launch_bounds__(256) pack_rows_b1_kernel(PackP p) {
  constexpr int EL = BF ? 8 : 4, NU = NP_MS_MAX_DIM / (64 * EL), LW = 32 / EL;   // LW lanes share a word
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.n_rows) return;   // a whole wave; the kernel has no barrier
  const int dim = p.dim;
  uint32_t* out = p.bits + (size_t)row * ((dim + 31) / 32);
  float sum = 0.f;
  uint32_t bad = 0u;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    if (u * 64 * EL >= dim) break;   // the whole wave
    const int k0 = (u * 64 + lane) * EL;
    uint32_t w[4] = {0u, 0u, 0u, 0u};   // the unit's 16 bytes, zeros past dim
    if (k0 < dim) {
      if (p.vec_in) {
        const uint4 v = *reinterpret_cast<const uint4*>(static_cast<const char*>(p.rows) + ((size_t)row * dim + k0) * (BF ? 2 : 4));
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      } else if (BF) {
        const uint16_t* rp = static_cast<const uint16_t*>(p.rows) + (size_t)row * dim;
#pragma unroll
        for (int i = 0; i < EL; ++i)
          if (k0 + i < dim) w[i >> 1] |= (uint32_t)rp[k0 + i] << (16 * (i & 1));
      } else {
        const uint32_t* rp = static_cast<const uint32_t*>(p.rows) + (size_t)row * dim;
#pragma unroll
        for (int i = 0; i < EL; ++i)
          if (k0 + i < dim) w[i] = rp[k0 + i];
      }
    }
    uint32_t m = 0u;
#pragma unroll
    for (int i = 0; i < EL; ++i) {
      const uint32_t b = BF ? (w[i >> 1] >> (16 * (i & 1))) << 16 : w[i];
      const uint32_t mag = b & 0x7FFFFFFFu;
      bad |= mag >= 0x7F800000u ? 1u : 0u;
      sum += __uint_as_float(mag);   // a dim past the end adds +0.0
      m |= (k0 + i < dim && __uint_as_float(b) >= 0.f ? 1u : 0u) << i;
    }
    uint32_t word = m << (EL * (lane & (LW - 1)));
#pragma unroll
    for (int d = 1; d < LW; d <<= 1) word |= (uint32_t)__shfl_xor((int)word, d);
    if ((lane & (LW - 1)) == 0 && k0 < dim) out[k0 >> 5] = word;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    sum = sum + __shfl_xor(sum, d);
    bad |= (uint32_t)__shfl_xor((int)bad, d);
  }
  if (lane == 0) p.scales[row] = bad ? __uint_as_float(0x7FC00000u) : __fdiv_rn(sum, (float)dim);
}

static int pack_validate(int32_t dtype, int32_t dim, int64_t n_rows, const void* rows, const void* bits, const void* scales) {
  const char* why = "";
  const int c = quantize_check_args(dtype, dim, n_rows, rows, bits, scales, &why);
  if (c == 0) return NP_OK;
  set_error("%s: pack_rows_b1: %s (dtype=%d dim=%d)", c == 1 ? "Shape error" : "Search failed", why, dtype, dim);
  return c == 1 ? NP_ERR_SHAPE : NP_ERR_INVALID_ARGUMENT;
}

// every array on the device; enqueues and returns
static int pack_run(hipStream_t st, int32_t dtype, int32_t dim, const void* d_rows, int64_t n_rows, uint32_t* d_bits,
                    float* d_scales) {
  const bool bf = dtype == NP_MS_DT_BF16;
  PackP p;
  p.rows = d_rows;
  p.bits = d_bits;
  p.scales = d_scales;
  p.n_rows = n_rows;
  p.dim = dim;
  p.vec_in = ((size_t)dim * (bf ? 2 : 4)) % 16 == 0 && (uintptr_t)d_rows % 16 == 0;
  const unsigned grid = (unsigned)((n_rows + 3) / 4);
  if (bf) pack_rows_b1_kernel<true><<<grid, 256, 0, st>>>(p);
  else pack_rows_b1_kernel<false><<<grid, 256, 0, st>>>(p);
  NP_HIP(hipGetLastError());
  return NP_OK;
}

// ---- np_hip_quantize_rows_i4: rows to one two's-complement nibble per dim and one f32 scale per row (np_maxsim_i4.hip's
// documents) ------------------------------------------------------------------------------------------------------------
//   rule          the int8 quantiser's with 7 for 127: a = max_d |x_d|, scale = a / 7, inv = 7 / a (correctly rounded),
//                 code_d = clamp(rintf(x_d * inv), -7, 7); nibble j of word w is dim 8 w + j and the pad nibbles are 0.
//                 a == 0: scale 0, codes 0.  A row with a non-finite element: scale NaN, codes 0.
//   work split    the int8 quantiser's: one wave per row, lane l takes the 16-byte units l, l + 64, ..., which stay in
//                 registers between the absmax pass and the rounding pass.  A bf16 unit is 8 dims, a whole word, which its
//                 lane stores; an f32 unit is 4 dims, half a word, shifted into place and OR-ed with the neighbour lane's
//                 half by one xor shuffle, and the even lane stores.  Consecutive words across the wave; no LDS, no atomics.
struct Quant4P {
  const void* rows;   // [n_rows][dim] f32 or bf16
  uint32_t* words;    // [n_rows][ceil(dim / 8)]
  float* scales;      // [n_rows]
  int64_t n_rows;
  int dim;
  int vec_in;         // 16-byte loads are legal for every row
};

template <bool BF>
__global__ void __launch_bounds__(256) quantize_rows_i4_kernel(Quant4P p) {
  constexpr int EL = BF ? 8 : 4, NU = NP_MS_MAX_DIM / (64 * EL);
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.n_rows) return;   // a whole wave; the kernel has no barrier
  const int dim = p.dim;
  float x[NU][EL];
  uint32_t amax = 0u, bad = 0u;   // |x| as bits: for finite values the integer order is the f32 order
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int k0 = (u * 64 + lane) * EL;
    uint32_t w[4] = {0u, 0u, 0u, 0u};   // the unit's 16 bytes, zeros past dim
    if (k0 < dim) {
      if (p.vec_in) {
        const uint4 v = *reinterpret_cast<const uint4*>(static_cast<const char*>(p.rows) + ((size_t)row * dim + k0) * (BF ? 2 : 4));
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      } else if (BF) {
        const uint16_t* rp = static_cast<const uint16_t*>(p.rows) + (size_t)row * dim;
#pragma unroll
        for (int i = 0; i < EL; ++i)
          if (k0 + i < dim) w[i >> 1] |= (uint32_t)rp[k0 + i] << (16 * (i & 1));
      } else {
        const uint32_t* rp = static_cast<const uint32_t*>(p.rows) + (size_t)row * dim;
#pragma unroll
        for (int i = 0; i < EL; ++i)
          if (k0 + i < dim) w[i] = rp[k0 + i];
      }
    }
#pragma unroll
    for (int i = 0; i < EL; ++i) {
      const uint32_t b = BF ? (w[i >> 1] >> (16 * (i & 1))) << 16 : w[i];
      x[u][i] = __uint_as_float(b);
      const uint32_t mag = b & 0x7FFFFFFFu;
      bad |= mag >= 0x7F800000u ? 1u : 0u;
      amax = mag > amax ? mag : amax;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)amax, d);
    amax = o > amax ? o : amax;
    bad |= (uint32_t)__shfl_xor((int)bad, d);
  }
  const float a = __uint_as_float(amax);
  const bool zero = bad || amax == 0u;            // every code is 0
  const float inv = zero ? 0.f : __fdiv_rn(7.0f, a);
  if (lane == 0) p.scales[row] = bad ? __uint_as_float(0x7FC00000u) : __fdiv_rn(a, 7.0f);
  uint32_t* out = p.words + (size_t)row * ((dim + 7) / 8);
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    if (u * 64 * EL >= dim) break;                // the whole wave: the shuffle below has every lane
    const int k0 = (u * 64 + lane) * EL;
    uint32_t nib = 0u;
#pragma unroll
    for (int i = 0; i < EL; ++i) {
      const float r = zero || k0 + i >= dim ? 0.f : fminf(fmaxf(rintf(x[u][i] * inv), -7.0f), 7.0f);
      nib |= ((uint32_t)(int)r & 0xFu) << (4 * i);
    }
    if (BF) {
      if (k0 < dim) out[k0 >> 3] = nib;
    } else {
      uint32_t word = nib << (16 * (lane & 1));
      word |= (uint32_t)__shfl_xor((int)word, 1);
      if ((lane & 1) == 0 && k0 < dim) out[k0 >> 3] = word;
    }
  }
}

static int quantize4_validate(int32_t dtype, int32_t dim, int64_t n_rows, const void* rows, const void* words, const void* scales) {
  const char* why = "";
  const int c = quantize_check_args(dtype, dim, n_rows, rows, words, scales, &why);
  if (c == 0) return NP_OK;
  set_error("%s: quantize_rows_i4: %s (dtype=%d dim=%d)", c == 1 ? "Shape error" : "Search failed", why, dtype, dim);
  return c == 1 ? NP_ERR_SHAPE : NP_ERR_INVALID_ARGUMENT;
}

// every array on the device; enqueues and returns
static int quantize4_run(hipStream_t st, int32_t dtype, int32_t dim, const void* d_rows, int64_t n_rows, uint32_t* d_words,
                         float* d_scales) {
  const bool bf = dtype == NP_MS_DT_BF16;
  Quant4P p;
  p.rows = d_rows;
  p.words = d_words;
  p.scales = d_scales;
  p.n_rows = n_rows;
  p.dim = dim;
  p.vec_in = ((size_t)dim * (bf ? 2 : 4)) % 16 == 0 && (uintptr_t)d_rows % 16 == 0;
  const unsigned grid = (unsigned)((n_rows + 3) / 4);
  if (bf) quantize_rows_i4_kernel<true><<<grid, 256, 0, st>>>(p);
  else quantize_rows_i4_kernel<false><<<grid, 256, 0, st>>>(p);
  NP_HIP(hipGetLastError());
  return NP_OK;
}

int maxsim_device_ok(int32_t device, int* compute_units);   // np_maxsim.hip

}  // namespace np

using namespace np;

extern "C" {

int np_hip_quantize_rows_i8_device(int32_t device, int32_t dtype, int32_t dim, const void* d_rows, int64_t n_rows,
                                   int8_t* d_out_codes, float* d_out_scales, void* stream) {
  clear_error();
  NP_TRY(quantize_validate(dtype, dim, n_rows, d_rows, d_out_codes, d_out_scales));
  if (n_rows == 0) return NP_OK;
  int cus = 0;
  NP_TRY(maxsim_device_ok(device, &cus));
  DeviceGuard g(device);
  return quantize_run((hipStream_t)stream, dtype, dim, d_rows, n_rows, d_out_codes, d_out_scales);
}

int np_hip_quantize_rows_i8(int32_t device, int32_t dtype, int32_t dim, const void* rows, int64_t n_rows, int8_t* out_codes,
                            float* out_scales) {
  clear_error();
  NP_TRY(quantize_validate(dtype, dim, n_rows, rows, out_codes, out_scales));
  if (n_rows == 0) return NP_OK;
  int cus = 0;
  NP_TRY(maxsim_device_ok(device, &cus));
  DeviceGuard g(device);
  // one allocation for the call: rows, codes, scales, each on a 256-byte boundary
  const size_t n = (size_t)n_rows * dim, b_in = up256(n * (dtype == NP_MS_DT_BF16 ? 2 : 4)), b_codes = up256(n);
  DevPtr<char> buf;
  NP_TRY(buf.alloc(b_in + b_codes + up256((size_t)n_rows * 4)));
  Carver carve{buf.get()};
  char* d_in = carve.take(b_in);
  int8_t* d_codes = (int8_t*)carve.take(b_codes);
  float* d_scales = (float*)carve.take((size_t)n_rows * 4);
  NP_HIP(hipMemcpy(d_in, rows, n * (dtype == NP_MS_DT_BF16 ? 2 : 4), hipMemcpyHostToDevice));
  NP_TRY(quantize_run(nullptr, dtype, dim, d_in, n_rows, d_codes, d_scales));
  NP_HIP(hipMemcpy(out_codes, d_codes, n, hipMemcpyDeviceToHost));
  NP_HIP(hipMemcpy(out_scales, d_scales, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
  return NP_OK;
}

int np_hip_pack_rows_b1_device(int32_t device, int32_t dtype, int32_t dim, const void* d_rows, int64_t n_rows,
                               uint32_t* d_out_bits, float* d_out_scales, void* stream) {
  clear_error();
  NP_TRY(pack_validate(dtype, dim, n_rows, d_rows, d_out_bits, d_out_scales));
  if (n_rows == 0) return NP_OK;
  int cus = 0;
  NP_TRY(maxsim_device_ok(device, &cus));
  DeviceGuard g(device);
  return pack_run((hipStream_t)stream, dtype, dim, d_rows, n_rows, d_out_bits, d_out_scales);
}

int np_hip_pack_rows_b1(int32_t device, int32_t dtype, int32_t dim, const void* rows, int64_t n_rows, uint32_t* out_bits,
                        float* out_scales) {
  clear_error();
  NP_TRY(pack_validate(dtype, dim, n_rows, rows, out_bits, out_scales));
  if (n_rows == 0) return NP_OK;
  int cus = 0;
  NP_TRY(maxsim_device_ok(device, &cus));
  DeviceGuard g(device);
  // one allocation for the call: rows, bit words, scales, each on a 256-byte boundary
  const size_t n_in = (size_t)n_rows * dim * (dtype == NP_MS_DT_BF16 ? 2 : 4), n_bits = (size_t)n_rows * ((dim + 31) / 32) * 4;
  DevPtr<char> buf;
  NP_TRY(buf.alloc(up256(n_in) + up256(n_bits) + up256((size_t)n_rows * 4)));
  Carver carve{buf.get()};
  char* d_in = carve.take(up256(n_in));
  uint32_t* d_bits = (uint32_t*)carve.take(up256(n_bits));
  float* d_scales = (float*)carve.take((size_t)n_rows * 4);
  NP_HIP(hipMemcpy(d_in, rows, n_in, hipMemcpyHostToDevice));
  NP_TRY(pack_run(nullptr, dtype, dim, d_in, n_rows, d_bits, d_scales));
  NP_HIP(hipMemcpy(out_bits, d_bits, n_bits, hipMemcpyDeviceToHost));
  NP_HIP(hipMemcpy(out_scales, d_scales, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
  return NP_OK;
}

int np_hip_quantize_rows_i4_device(int32_t device, int32_t dtype, int32_t dim, const void* d_rows, int64_t n_rows,
                                   uint32_t* d_out_words, float* d_out_scales, void* stream) {
  clear_error();
  NP_TRY(quantize4_validate(dtype, dim, n_rows, d_rows, d_out_words, d_out_scales));
  if (n_rows == 0) return NP_OK;
  int cus = 0;
  NP_TRY(maxsim_device_ok(device, &cus));
  DeviceGuard g(device);
  return quantize4_run((hipStream_t)stream, dtype, dim, d_rows, n_rows, d_out_words, d_out_scales);
}

int np_hip_quantize_rows_i4(int32_t device, int32_t dtype, int32_t dim, const void* rows, int64_t n_rows, uint32_t* out_words,
                            float* out_scales) {
  clear_error();
  NP_TRY(quantize4_validate(dtype, dim, n_rows, rows, out_words, out_scales));
  if (n_rows == 0) return NP_OK;
  int cus = 0;
  NP_TRY(maxsim_device_ok(device, &cus));
  DeviceGuard g(device);
  // one allocation for the call: rows, nibble words, scales, each on a 256-byte boundary
  const size_t n_in = (size_t)n_rows * dim * (dtype == NP_MS_DT_BF16 ? 2 : 4), n_words = (size_t)n_rows * ((dim + 7) / 8) * 4;
  DevPtr<char> buf;
  NP_TRY(buf.alloc(up256(n_in) + up256(n_words) + up256((size_t)n_rows * 4)));
  Carver carve{buf.get()};
  char* d_in = carve.take(up256(n_in));
  uint32_t* d_words = (uint32_t*)carve.take(up256(n_words));
  float* d_scales = (float*)carve.take((size_t)n_rows * 4);
  NP_HIP(hipMemcpy(d_in, rows, n_in, hipMemcpyHostToDevice));
  NP_TRY(quantize4_run(nullptr, dtype, dim, d_in, n_rows, d_words, d_scales));
  NP_HIP(hipMemcpy(out_words, d_words, n_words, hipMemcpyDeviceToHost));
  NP_HIP(hipMemcpy(out_scales, d_scales, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
  return NP_OK;
}

}  // extern "C"
