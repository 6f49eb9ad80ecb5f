// np_textbuild_dev.h -- what the keyword-index build (np_textbuild.hip) and the keyword-index merge (np_textmerge.hip) share
// on the device side: the build object both return, the exclusive scan of u32 counts, the stream of a call.  Every
// translation unit that includes it gets its own copy of the kernels (they have internal linkage).
#pragma once
#include <chrono>
#include "np_internal.h"
#include "np_textbuild_plan.h"

struct np_text_build {
  int device = 0;
  int32_t tokenizer = 0;
  int64_t n_docs = 0, n_inst = 0, n_terms = 0;
  std::vector<int64_t> fallback;
  // the device's result: the strings on the host, the arrays in HBM until they are fetched or merged
  std::vector<uint8_t> term_bytes;
  std::vector<int64_t> term_byte_offsets;
  np::DevPtr<int64_t> d_toff, d_inst_doc;
  np::DevPtr<int32_t> d_inst_pos;
  // the fallback documents' instances (np_hip_text_build_add)
  bool added = false, finalised = false, merged = false;
  // np_hip_index_set_text_build installed it: inst_pos belongs to the handle, inst_doc and term_offsets are freed; the sizes
  // and the vocabulary stay
  bool consumed = false;
  std::vector<uint8_t> b_bytes;
  std::vector<int64_t> b_tbo, b_doc;
  std::vector<int32_t> b_term, b_pos;
  np::TextArrays out;   // the merged result
};

namespace np {

// The base of a merge that lies in a handle (np_hip_index_text_merge, np_textres.hip): term_offsets and inst_doc regenerated
// from the postings into the call's workspace, pos read where it lies.  Without one the base comes from the host.
struct TextMergeResident {
  const DeviceIndex* ix = nullptr;
  int64_t n_docs = 0;       // the handle's documents: doc_len's entries
};
// np_textmerge.hip: np_hip_text_build_merge, and with `res` np_hip_index_text_merge (`base` is then NULL)
int text_merge_impl(const char* entry, int device, const np_text_index* base, const TextMergeResident* res, const uint8_t* a_bytes,
                    const int64_t* a_tbo, const int64_t* remap, int64_t n_remap, const np_text_build* delta, const int64_t* delta_ids,
                    int64_t n_rows_out, const np_text_merge_opts* opts, np_text_build* R, np_text_merge_report* rep);
// np_textres.hip: term_offsets [n_terms + 1] and inst_doc [n_inst] of a handle's keyword index, from its postings
int textres_expand(hipStream_t st, const DeviceText& t, int64_t* toff, int64_t* inst_doc);
// np_textres.hip: entries d < n of doc_len with doc_len[d] > 0 and (remap given) remap[d] >= 0; flags and scan hold n + 1 each
int textres_count_docs(hipStream_t st, const int32_t* doc_len, int64_t n, const int64_t* d_remap, uint32_t* flags, uint32_t* scan,
                       uint64_t* sums, int64_t* out);

namespace {

// ---- exclusive scan of u32 counts: reduce per block, scan the block sums in one block, apply ----------------------------
__device__ __forceinline__ uint64_t tb_block_excl_scan(uint64_t v, uint64_t* lds, uint64_t* total) {
  const int tid = threadIdx.x;
  lds[tid] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const uint64_t t = tid >= d ? lds[tid - d] : 0;
    __syncthreads();
    lds[tid] += t;
    __syncthreads();
  }
  const uint64_t incl = lds[tid];
  *total = lds[255];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(256) void tb_scan_reduce(const uint32_t* __restrict__ in, int64_t n, uint64_t* sums) {
  __shared__ uint64_t lds[256];
  const int64_t i0 = (int64_t)blockIdx.x * NP_TB_SCAN_CHUNK + threadIdx.x * 8;
  uint64_t s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (i0 + j < n) s += in[i0 + j];
  uint64_t total;
  (void)tb_block_excl_scan(s, lds, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void tb_scan_sums(uint64_t* sums, int64_t nb) {
  __shared__ uint64_t lds[256];
  uint64_t carry = 0;
  for (int64_t c0 = 0; c0 < nb; c0 += 256) {
    const int64_t i = c0 + threadIdx.x;
    const uint64_t v = i < nb ? sums[i] : 0;
    uint64_t total;
    const uint64_t ex = tb_block_excl_scan(v, lds, &total);
    if (i < nb) sums[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) sums[nb] = carry;
}

// out[i] = sum of in[0..i), out[n] = the total; out may be in (each block reads its items before it writes them)
template <class T>
__global__ __launch_bounds__(256) void tb_scan_apply(const uint32_t* in, int64_t n, const uint64_t* __restrict__ sums, int64_t nb,
                                                      T* out) {
  __shared__ uint64_t lds[256];
  const int64_t i0 = (int64_t)blockIdx.x * NP_TB_SCAN_CHUNK + threadIdx.x * 8;
  uint32_t v[8];
  uint64_t s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = i0 + j < n ? in[i0 + j] : 0u;
    s += v[j];
  }
  uint64_t total;
  uint64_t run = tb_block_excl_scan(s, lds, &total) + sums[blockIdx.x];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (i0 + j < n) out[i0 + j] = (T)run;
    run += v[j];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = (T)sums[nb];
}

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

inline unsigned grid_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

struct TbStream {
  hipStream_t st = nullptr;
  ~TbStream() {
    if (st) (void)hipStreamDestroy(st);
  }
};

template <class T>
int tb_scan(hipStream_t st, const uint32_t* in, int64_t n, T* out, uint64_t* sums) {
  const int64_t nb = (n + NP_TB_SCAN_CHUNK - 1) / NP_TB_SCAN_CHUNK;
  if (nb > 0) hipLaunchKernelGGL(tb_scan_reduce, dim3((unsigned)nb), dim3(256), 0, st, in, n, sums);
  hipLaunchKernelGGL(tb_scan_sums, dim3(1), dim3(256), 0, st, sums, nb);
  if (nb > 0)
    hipLaunchKernelGGL(tb_scan_apply<T>, dim3((unsigned)nb), dim3(256), 0, st, in, n, (const uint64_t*)sums, nb, out);
  else
    NP_HIP(hipMemsetAsync(out, 0, sizeof(T), st));
  NP_HIP(hipGetLastError());
  return NP_OK;
}

}  // namespace
}  // namespace np
