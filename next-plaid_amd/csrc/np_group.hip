// np_group.hip -- grouped search: the group of every document in HBM (np_hip_index_set_groups), the collapse of ranked lists
// to "top_k distinct groups, the best group_size members of each" (np_hip_collapse, np_hip_collapse_device) and the search
// pass with the collapse behind it on the same stream (np_hip_search_batch_grouped; np_hip_search_hybrid_grouped lives with
// the hybrid request in np_text.hip and launches through collapse_launch here).
//
// The semantics are ColGREP's collapse_by_file (colgrep/src/index/mod.rs:4394-4413) with a member limit: walk the ranked
// list, admit a group at its first entry while fewer than top_k are admitted, fold every later entry of an admitted group
// into it (the first group_size are kept, all are counted), skip the rest.  No score is read: the list's order is the order.
//
//   collapse_kernel   one workgroup of 1024 threads per list.  key = group << 32 | rank, padded with all-ones, bitonic sort
//                     ascending in LDS: a group's entries are now adjacent and in rank order.  A position is a head where the
//                     group changes; a block-wide max-scan of head positions (wave shuffles + one LDS level) gives every
//                     position its head, hence its member index.  Heads set the bit of their RANK in a bitmap: a group's
//                     ordinal in order of admission is the number of leader bits below its leader's rank, and it is admitted
//                     iff that is < top_k.  Entries with a member index < group_size of an admitted group write their slot,
//                     the last entry of a run -- which knows the head, so the run's length: the next head's position minus
//                     this head's -- writes the group's three figures.  No output atomics: the result is deterministic.
#include "np_internal.h"
#include "np_group_plan.h"

#include <chrono>
#include <string.h>

namespace np {

struct CollapseP {
  const int64_t* ids;       // [B][stride]
  const uint32_t* scores;   // [B][stride] f32 bits, or NULL
  const int32_t* counts;    // [B]
  int stride, P2, C;        // C = sorted positions per thread
  const int32_t* group_ids; // [n_docs]
  int64_t n_docs;
  int top_k, group_size;
  int64_t* out_ids;         // [B][top_k][group_size]
  uint32_t* out_scores;     // likewise, or NULL
  int32_t *out_group, *out_members, *out_total;   // [B][top_k]
  int32_t* out_counts;      // [B]
};

static_assert(NP_GROUP_LIST_CAP == NP_GROUP_MAX_LIST, "np_group_plan.h sizes the sort for the header's limit");
constexpr uint64_t GROUP_PAD = ~0ull;

__device__ __forceinline__ void bitonic_sort_asc(uint64_t* s, int n, int tid, int nthreads) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < n; i += nthreads) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t a = s[i], c = s[ixj];
          const bool asc = (i & k) == 0;
          if (asc ? (a > c) : (a < c)) {
            s[i] = c;
            s[ixj] = a;
          }
        }
      }
    }
  }
  __syncthreads();
}

// Exclusive scan over the block's 1024 threads in thread order: shuffles inside a wave, the 16 wave totals through s_w and
// one more shuffle scan.  ADD: sum, identity 0; otherwise max, identity -1.  *total = the scan over all threads.  Every thread
// of the block calls it; s_w is free again on return.
template <bool ADD>
__device__ __forceinline__ int block_scan_excl(int v, int* s_w, int tid, int* total) {
  const int ident = ADD ? 0 : -1;
  const int lane = tid & 63, wave = tid >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v = ADD ? v + o : max(v, o);
  }
  int ex = __shfl_up(v, 1);
  if (lane == 0) ex = ident;
  if (lane == 63) s_w[wave] = v;
  __syncthreads();
  if (wave == 0) {
    int w = lane < NP_GROUP_TPB / 64 ? s_w[lane] : ident;
    for (int d = 1; d < NP_GROUP_TPB / 64; d <<= 1) {
      const int o = __shfl_up(w, d);
      if (lane >= d) w = ADD ? w + o : max(w, o);
    }
    if (lane < NP_GROUP_TPB / 64) s_w[lane] = w;
  }
  __syncthreads();
  if (wave > 0) ex = ADD ? ex + s_w[wave - 1] : max(ex, s_w[wave - 1]);
  *total = s_w[NP_GROUP_TPB / 64 - 1];
  __syncthreads();
  return ex;
}

__global__ void __launch_bounds__(NP_GROUP_TPB) collapse_kernel(CollapseP p) {
  extern __shared__ __align__(16) unsigned char g_lds[];
  uint64_t* keys = (uint64_t*)g_lds;                       // [P2]
  unsigned long long* lead = (unsigned long long*)(keys + p.P2);   // [P2 / 64] leaders by rank
  int* wpre = (int*)(lead + p.P2 / 64);                    // [P2 / 64] leader bits in the words before
  int* s_w = wpre + p.P2 / 64;                             // [NP_GROUP_SCAN_WORDS]
  const int b = blockIdx.x, tid = threadIdx.x;
  const int P2 = p.P2, NW = P2 / 64;
  const int count = min(max(p.counts[b], 0), p.stride);
  const int64_t* ids = p.ids + (int64_t)b * p.stride;
  const int slots = p.top_k * p.group_size;
  int64_t* o_ids = p.out_ids + (int64_t)b * slots;
  uint32_t* o_sc = p.out_scores ? p.out_scores + (int64_t)b * slots : nullptr;
  int32_t* o_group = p.out_group + (int64_t)b * p.top_k;
  int32_t* o_members = p.out_members + (int64_t)b * p.top_k;
  int32_t* o_total = p.out_total + (int64_t)b * p.top_k;

  // the row's padding first: whatever is not written below stays id 0 / score 0 / figures 0 (the sort's barriers order these
  // stores before the ones that overwrite them)
  for (int i = tid; i < slots; i += NP_GROUP_TPB) {
    o_ids[i] = 0;
    if (o_sc) o_sc[i] = 0u;
  }
  for (int i = tid; i < p.top_k; i += NP_GROUP_TPB) {
    o_group[i] = 0;
    o_members[i] = 0;
    o_total[i] = 0;
  }
  for (int r = tid; r < P2; r += NP_GROUP_TPB) {
    uint64_t k = GROUP_PAD;
    if (r < count) {
      const int64_t id = ids[r];
      if (id >= 0 && id < p.n_docs) k = (uint64_t)(uint32_t)p.group_ids[id] << 32 | (uint32_t)r;   // an id out of range is absent
    }
    keys[r] = k;
  }
  for (int w = tid; w < NW; w += NP_GROUP_TPB) lead[w] = 0ull;
  bitonic_sort_asc(keys, P2, tid, NP_GROUP_TPB);   // (its first barrier covers the stores above)

  // first walk of the thread's positions [p0, p0 + C): the last head among them, and every head's leader bit
  const int p0 = tid * p.C;
  int last_head = -1;
  if (p0 < P2) {
    uint64_t prev = p0 > 0 ? keys[p0 - 1] : GROUP_PAD;
    for (int i = 0; i < p.C; ++i) {
      const uint64_t k = keys[p0 + i];
      if (k == GROUP_PAD) break;   // pads sort last
      if (p0 + i == 0 || (uint32_t)(k >> 32) != (uint32_t)(prev >> 32)) {
        last_head = p0 + i;
        const uint32_t rank = (uint32_t)k;
        atomicOr(&lead[rank >> 6], 1ull << (rank & 63));   // distinct bits of one word come from different lanes
      }
      prev = k;
    }
  }
  int unused;
  int head = block_scan_excl<false>(last_head, s_w, tid, &unused);   // the head the thread's first position continues
  // leader bits in the words before each word (the scan's barriers have completed the bitmap)
  int n_groups = 0;
  {
    const int c = tid < NW ? __popcll(lead[tid]) : 0;
    const int ex = block_scan_excl<true>(c, s_w, tid, &n_groups);
    if (tid < NW) wpre[tid] = ex;
  }
  __syncthreads();
  if (tid == 0) p.out_counts[b] = min(n_groups, p.top_k);

  // second walk: member index, ordinal of the group, the stores
  if (p0 < P2) {
    int ord = -1, ord_of = -2;   // ordinal of the group whose head is ord_of
    for (int i = 0; i < p.C; ++i) {
      const int pos = p0 + i;
      const uint64_t k = keys[pos];
      if (k == GROUP_PAD) break;
      const uint32_t gid = (uint32_t)(k >> 32);
      if (pos == 0 || (uint32_t)(keys[pos - 1] >> 32) != gid) head = pos;
      if (head != ord_of) {
        const uint32_t lr = (uint32_t)keys[head];   // the leader's rank: the lowest of the run
        ord = wpre[lr >> 6] + __popcll(lead[lr >> 6] & ((1ull << (lr & 63)) - 1ull));
        ord_of = head;
      }
      if (ord >= p.top_k) continue;
      const int m = pos - head;
      if (m < p.group_size) {
        const uint32_t r = (uint32_t)k;
        o_ids[ord * p.group_size + m] = ids[r];
        if (o_sc) o_sc[ord * p.group_size + m] = p.scores[(int64_t)b * p.stride + r];
      }
      const bool tail = pos + 1 == P2 || keys[pos + 1] == GROUP_PAD || (uint32_t)(keys[pos + 1] >> 32) != gid;
      if (tail) {
        o_group[ord] = (int32_t)gid;
        o_total[ord] = m + 1;
        o_members[ord] = min(m + 1, p.group_size);
      }
    }
  }
}

int GroupStage::fetch(void* pinned, hipStream_t st, bool with_scores) {
  pin = (char*)pinned;
  scores = with_scores;
  char* at = pin;
  NP_HIP(hipMemcpyAsync(at, d_ids, n * 8, hipMemcpyDeviceToHost, st));
  at += o_ids;
  if (scores) NP_HIP(hipMemcpyAsync(at, d_sc, n * 4, hipMemcpyDeviceToHost, st));
  at += o_sc;
  NP_HIP(hipMemcpyAsync(at, d_group, g * 4, hipMemcpyDeviceToHost, st));
  NP_HIP(hipMemcpyAsync(at + o_g, d_members, g * 4, hipMemcpyDeviceToHost, st));
  NP_HIP(hipMemcpyAsync(at + 2 * o_g, d_total, g * 4, hipMemcpyDeviceToHost, st));
  NP_HIP(hipMemcpyAsync(at + 3 * o_g, d_cnt, B * 4, hipMemcpyDeviceToHost, st));
  return NP_OK;
}

void GroupStage::deliver(int64_t* out_ids, float* out_scores, int32_t* out_group, int32_t* out_members, int32_t* out_total,
                         int32_t* out_counts) const {
  const char* at = pin;
  memcpy(out_ids, at, n * 8);
  at += o_ids;
  if (scores && out_scores) memcpy(out_scores, at, n * 4);
  at += o_sc;
  memcpy(out_group, at, g * 4);
  memcpy(out_members, at + o_g, g * 4);
  memcpy(out_total, at + 2 * o_g, g * 4);
  memcpy(out_counts, at + 3 * o_g, B * 4);
}

int collapse_check(const DeviceIndex* ix, int32_t top_k, int32_t group_size, int32_t B, int32_t stride) {
  if (!ix) {
    set_error("Collapse failed: NULL index");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const char* why = "";
  if (group_check_args(ix->n_groups > 0, top_k, group_size, B, stride, &why) != 0) {
    set_error("Collapse failed: %s (top_k=%d group_size=%d stride=%d)", why, top_k, group_size, stride);
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

int collapse_launch(const DeviceIndex* ix, hipStream_t st, int32_t top_k, int32_t group_size, int32_t B, const int64_t* d_ids,
                    const float* d_scores, const int32_t* d_counts, int32_t stride, int64_t* d_out_ids, float* d_out_scores,
                    int32_t* d_out_group, int32_t* d_out_members, int32_t* d_out_total, int32_t* d_out_counts) {
  NP_TRY(collapse_check(ix, top_k, group_size, B, stride));
  if (B == 0) return NP_OK;
  CollapseP p;
  p.ids = d_ids;
  p.scores = (const uint32_t*)d_scores;
  p.counts = d_counts;
  p.stride = stride;
  p.P2 = group_p2(stride);
  p.C = group_chunk(stride);
  p.group_ids = ix->d_groups.get();
  p.n_docs = ix->n_docs;
  p.top_k = top_k;
  p.group_size = group_size;
  p.out_ids = d_out_ids;
  p.out_scores = d_scores ? (uint32_t*)d_out_scores : nullptr;
  p.out_group = d_out_group;
  p.out_members = d_out_members;
  p.out_total = d_out_total;
  p.out_counts = d_out_counts;
  const size_t lds = (size_t)group_lds_bytes(stride);
  if (lds > 48 * 1024)
    NP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&collapse_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
  collapse_kernel<<<(unsigned)B, NP_GROUP_TPB, lds, st>>>(p);
  NP_HIP(hipGetLastError());
  return NP_OK;
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_index_set_groups(np_index* ix, const int32_t* group_ids, int64_t n, int64_t n_groups) {
  clear_error();
  if (!ix) {
    set_error("set_groups: NULL index");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const char* why = "";
  int64_t bad = -1;
  const int rc = group_check_ids(group_ids, n, n_groups, ix->N_total, ix->opts.shard_count, &why, &bad);
  if (rc != 0) {
    if (bad >= 0)
      set_error("set_groups: %s (document %lld has group %d, n_groups = %lld)", why, (long long)bad, group_ids[bad],
                (long long)n_groups);
    else
      set_error("set_groups: %s (n = %lld, num_documents = %lld, n_groups = %lld)", why, (long long)n, (long long)ix->N_total,
                (long long)n_groups);
    return rc == 1 ? NP_ERR_SHAPE : NP_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g(ix->device);
  DevPtr<int32_t> fresh;   // built beside the old array and swapped in: a failed allocation leaves the handle as it was
  size_t bytes = 0;
  if (n > 0) {
    NP_TRY(fresh.alloc((size_t)n, &bytes));
    NP_HIP(hipMemcpy(fresh.get(), group_ids, (size_t)n * 4, hipMemcpyHostToDevice));
  }
  ix->d_groups = std::move(fresh);
  ix->n_groups = n > 0 ? n_groups : 0;
  ix->device_bytes = ix->device_bytes - ix->group_bytes + bytes;
  ix->group_bytes = bytes;
  return NP_OK;
}

int64_t np_hip_index_group_count(const np_index* ix) { return ix ? ix->n_groups : 0; }

int np_hip_collapse_device(const np_index* ix, int32_t top_k, int32_t group_size, int32_t B, const int64_t* d_ids,
                           const float* d_scores, const int32_t* d_counts, int32_t stride, int64_t* d_out_ids,
                           float* d_out_scores, int32_t* d_out_group, int32_t* d_out_members, int32_t* d_out_total,
                           int32_t* d_out_counts, void* stream) {
  clear_error();
  IndexRead reading(ix);   // an append waits for this call and holds later ones back (np_internal.h)
  NP_TRY(collapse_check(ix, top_k, group_size, B, stride));
  if (B == 0) return NP_OK;
  if (!d_ids || !d_counts || !d_out_ids || (d_scores && !d_out_scores) || !d_out_group || !d_out_members || !d_out_total ||
      !d_out_counts) {
    set_error("Collapse failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g(ix->device);
  ContextUse use;   // (a context's stream where `stream` is NULL)
  NP_TRY(use.begin(ix, stream));
  return collapse_launch(ix, use.stream, top_k, group_size, B, d_ids, d_scores, d_counts, stride, d_out_ids, d_out_scores,
                         d_out_group, d_out_members, d_out_total, d_out_counts);
}

int np_hip_collapse(const np_index* ix, int32_t top_k, int32_t group_size, int32_t B, const int64_t* ids, const float* scores,
                    const int32_t* counts, int32_t stride, int64_t* out_ids, float* out_scores, int32_t* out_group,
                    int32_t* out_members, int32_t* out_total, int32_t* out_counts) {
  clear_error();
  IndexRead reading(ix);   // an append waits for this call and holds later ones back (np_internal.h)
  NP_TRY(collapse_check(ix, top_k, group_size, B, stride));
  if (B == 0) return NP_OK;
  if (!ids || !counts || !out_ids || (scores && !out_scores) || !out_group || !out_members || !out_total || !out_counts) {
    set_error("Collapse failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const int bc = group_first_bad_count(counts, B, stride);
  if (bc >= 0) {
    set_error("Collapse failed: the count of query %d (%d) is outside its stride (%d)", bc, counts[bc], stride);
    return NP_ERR_INVALID_ARGUMENT;
  }
  const int64_t bi = group_first_bad_id(ids, counts, B, stride, ix->N_total);
  if (bi >= 0) {
    set_error("Collapse failed: id %lld (query %lld, rank %lld) is outside [0, %lld)", (long long)ids[bi], (long long)(bi / stride),
              (long long)(bi % stride), (long long)ix->N_total);
    return NP_ERR_INVALID_ARGUMENT;
  }
  const size_t n_l = (size_t)B * stride;
  const size_t b_i = up256(n_l * 8), b_s = up256(n_l * 4), b_c = up256((size_t)B * 4);
  GroupStage res(B, top_k, group_size);
  DeviceGuard g(ix->device);
  ContextUse use;
  NP_TRY(use.begin(ix, nullptr));
  hipStream_t st = use.stream;
  NP_TRY(use.arena().reserve(b_i + b_s + b_c + res.bytes()));
  void* pin = nullptr;
  NP_TRY(use.pin(res.bytes(), &pin));
  Carver carve{use.arena().as<char>()};
  int64_t* d_i = (int64_t*)carve.take(b_i);
  float* d_s = (float*)carve.take(b_s);
  int32_t* d_c = (int32_t*)carve.take(b_c);
  res.carve(carve);
  // pageable sources: the copies complete before the call returns (it synchronises below)
  NP_HIP(hipMemcpyAsync(d_i, ids, n_l * 8, hipMemcpyHostToDevice, st));
  if (scores) NP_HIP(hipMemcpyAsync(d_s, scores, n_l * 4, hipMemcpyHostToDevice, st));
  NP_HIP(hipMemcpyAsync(d_c, counts, (size_t)B * 4, hipMemcpyHostToDevice, st));
  NP_TRY(collapse_launch(ix, st, top_k, group_size, B, d_i, scores ? d_s : nullptr, d_c, stride, res.d_ids, res.d_sc, res.d_group,
                         res.d_members, res.d_total, res.d_cnt));
  NP_TRY(res.fetch(pin, st, scores != nullptr));
  NP_TRY(use.end());
  NP_HIP(hipStreamSynchronize(st));
  res.deliver(out_ids, out_scores, out_group, out_members, out_total, out_counts);
  return NP_OK;
}

int np_hip_search_batch_grouped(const np_index* ix, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                                const np_search_params* params, const int64_t* subset_ids, const int64_t* subset_offsets,
                                int64_t n_subsets, const int32_t* query_subset, const np_filter* filters, int32_t n_filters,
                                int32_t pool_k, int32_t group_size, int64_t* out_ids, float* out_scores, int32_t* out_group,
                                int32_t* out_members, int32_t* out_total, int32_t* out_counts, np_stats* stats) {
  clear_error();
  IndexRead reading(ix);   // an append waits for this call and holds later ones back (np_internal.h)
  if (stats) memset(stats, 0, sizeof *stats);
  if (!ix || !params) {
    set_error("Search failed: NULL index or params");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (pool_k < 1 || pool_k > NP_GROUP_LIST_CAP) {
    set_error("Collapse failed: pool_k = %d must be in 1 .. %d", pool_k, NP_GROUP_LIST_CAP);
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(collapse_check(ix, params->top_k, group_size, B, pool_k));
  if (filters) n_subsets = n_filters;
  if (filters)
    NP_TRY(filter_check_call(ix, filters, n_filters, query_subset, B, true));
  else
    NP_TRY(check_subsets(subset_ids, subset_offsets, n_subsets, query_subset, query_subset, B));
  if (B > 0 && (!queries || !q_tok_offsets || !out_ids || !out_scores || !out_group || !out_members || !out_total || !out_counts)) {
    set_error("Search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (B > 0 && q_tok_offsets[0] != 0) {
    set_error("Shape error: q_tok_offsets[0] must be 0");
    return NP_ERR_SHAPE;
  }
  for (int b = 0; b < B; ++b)
    if (q_tok_offsets[b + 1] < q_tok_offsets[b]) {
      set_error("Shape error: q_tok_offsets must be non-decreasing");
      return NP_ERR_SHAPE;
    }
  np_search_params pool = *params;
  pool.top_k = pool_k;
  const int top_k = params->top_k;
  const auto t0 = std::chrono::steady_clock::now();
  DeviceGuard g(ix->device);
  ContextUse use;
  NP_TRY(use.begin(ix, nullptr));
  hipStream_t st = use.stream;
  if (B == 0)   // (the pass's own checks)
    return search_batch_in_use(ix, use, nullptr, nullptr, nullptr, 0, dim, &pool, CallSubsets(), nullptr, nullptr, nullptr);
  HostScope scope;
  NP_TRY(scope.resolve(ix, use, subset_ids, subset_offsets, n_subsets, query_subset, filters, B));
  const int64_t ntok = q_tok_offsets[B];
  const size_t b_q = up256((size_t)std::max<int64_t>(ntok, 1) * dim * 4), b_qoff = up256((size_t)(B + 1) * 4);
  ResultStage list(B, pool_k);   // the pool stays on the device
  GroupStage res(B, top_k, group_size);
  NP_TRY(use.arena().reserve(b_q + b_qoff + scope.stage_bytes() + list.bytes() + res.bytes()));
  void* pin = nullptr;
  NP_TRY(use.pin(res.bytes(), &pin));
  Carver carve{use.arena().as<char>()};
  float* d_q = (float*)carve.take(b_q);
  int32_t* d_qoff = (int32_t*)carve.take(b_qoff);
  CallSubsets sub;
  NP_TRY(scope.place(carve, st, &sub));
  list.carve(carve);
  res.carve(carve);
  if (ntok > 0) NP_HIP(hipMemcpyAsync(d_q, queries, (size_t)ntok * dim * 4, hipMemcpyHostToDevice, st));
  NP_HIP(hipMemcpyAsync(d_qoff, q_tok_offsets, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, st));
  NP_TRY(search_batch_in_use(ix, use, d_q, d_qoff, q_tok_offsets, B, dim, &pool, sub, list.d_ids, list.d_sc, list.d_cnt));
  NP_TRY(collapse_launch(ix, st, top_k, group_size, B, list.d_ids, list.d_sc, list.d_cnt, pool_k, res.d_ids, res.d_sc, res.d_group,
                         res.d_members, res.d_total, res.d_cnt));
  NP_TRY(res.fetch(pin, st, true));
  NP_TRY(use.end());
  NP_HIP(hipStreamSynchronize(st));
  res.deliver(out_ids, out_scores, out_group, out_members, out_total, out_counts);
  if (stats) {
    stats->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    stats->n_queries = B;
  }
  return NP_OK;
}

}  // extern "C"
