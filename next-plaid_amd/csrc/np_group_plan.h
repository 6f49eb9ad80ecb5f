// np_group_plan.h -- the host side of the grouped entry points (np_group.hip) that needs no device: the checks of
// np_hip_index_set_groups and of a collapse, the sort width and the LDS bytes of collapse_kernel, the output sizes.  Plain
// C++; tests/cpp/group_plan_check.cpp runs all of it stand-alone.
#pragma once
#include <stdint.h>

namespace np {

constexpr int NP_GROUP_LIST_CAP = 16384;    // NP_GROUP_MAX_LIST: entries of one ranked list, and slots of one output row
constexpr int NP_GROUP_TPB = 1024;          // threads of collapse_kernel's one workgroup per query
constexpr int NP_GROUP_MIN_P2 = 64;         // the sort is at least one wave wide: the leader bitmap has whole u64 words
constexpr int64_t NP_GROUP_MAX_GROUPS = 0x7FFFFFFF;   // ids are below it, so (id << 32 | rank) never equals the all-ones pad
constexpr int NP_GROUP_SCAN_WORDS = 32;     // i32 of scan scratch: one per wave, and a little room

// The arguments of np_hip_index_set_groups that need only the host's arrays.  0 = fine, 1 = shape error, 2 = invalid
// argument; *why names the reason, *bad the first offending entry (-1: none).  n == 0 drops the groups and checks nothing else.
inline int group_check_ids(const int32_t* group_ids, int64_t n, int64_t n_groups, int64_t num_documents, int shard_count,
                           const char** why, int64_t* bad) {
  *why = "";
  *bad = -1;
  if (n < 0) return *why = "negative length", 2;
  if (shard_count > 1)
    return *why = "a sharded handle is refused: a group's members can lie on several shards, so per-shard grouped lists do not "
                  "merge exactly",
           2;
  if (n == 0) return 0;
  if (n != num_documents) return *why = "one group id per document of the whole index is needed", 1;
  if (n_groups < 1 || n_groups > NP_GROUP_MAX_GROUPS) return *why = "n_groups must be in 1 .. 2^31-1", 2;
  if (!group_ids) return *why = "NULL group_ids", 2;
  for (int64_t d = 0; d < n; ++d)
    if (group_ids[d] < 0 || (int64_t)group_ids[d] >= n_groups) return *bad = d, *why = "a group id is outside [0, n_groups)", 2;
  return 0;
}

// The scalar arguments of a collapse.  0 = fine, 2 = invalid argument.
inline int group_check_args(bool has_groups, int32_t top_k, int32_t group_size, int32_t B, int32_t stride, const char** why) {
  *why = "";
  if (!has_groups) return *why = "the handle has no groups (np_hip_index_set_groups)", 2;
  if (B < 0) return *why = "negative batch size", 2;
  if (top_k < 1) return *why = "top_k must be at least 1", 2;
  if (group_size < 1) return *why = "group_size must be at least 1", 2;
  if ((int64_t)top_k * group_size > NP_GROUP_LIST_CAP) return *why = "top_k * group_size exceeds 16384", 2;
  if (stride < 1 || stride > NP_GROUP_LIST_CAP) return *why = "stride must be in 1 .. 16384", 2;
  return 0;
}

// host form only: the first query whose count lies outside 0 .. stride, or -1
inline int group_first_bad_count(const int32_t* counts, int B, int32_t stride) {
  for (int b = 0; b < B; ++b)
    if (counts[b] < 0 || counts[b] > stride) return b;
  return -1;
}

// host form only: the first entry (b * stride + r, r < counts[b]) whose id lies outside [0, num_documents), or -1
inline int64_t group_first_bad_id(const int64_t* ids, const int32_t* counts, int B, int32_t stride, int64_t num_documents) {
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < counts[b]; ++r) {
      const int64_t id = ids[(int64_t)b * stride + r];
      if (id < 0 || id >= num_documents) return (int64_t)b * stride + r;
    }
  return -1;
}

// the sort width: the power of two >= stride, at least one wave
inline int group_p2(int32_t stride) {
  int p = NP_GROUP_MIN_P2;
  while (p < stride) p <<= 1;
  return p;
}

// dynamic LDS of collapse_kernel: the keys, the leader bitmap over ranks, the bitmap words' popcount prefix, the scan scratch
inline int64_t group_lds_bytes(int32_t stride) {
  const int64_t p2 = group_p2(stride);
  return p2 * 8 + p2 / 8 + p2 / 64 * 4 + NP_GROUP_SCAN_WORDS * 4;
}

// entries of sorted position one thread walks (a contiguous run of them)
inline int group_chunk(int32_t stride) {
  const int p2 = group_p2(stride);
  return p2 > NP_GROUP_TPB ? p2 / NP_GROUP_TPB : 1;
}

// ColGREP's pool for top_k groups (index/mod.rs: max(20 top_k, 200)), inside what the index holds and the entry's limit
inline int64_t group_default_pool(int64_t top_k, int64_t num_documents, int64_t limit) {
  int64_t want = 20 * top_k > 200 ? 20 * top_k : 200;
  const int64_t have = num_documents > top_k ? num_documents : top_k;
  if (want > have) want = have;
  if (want > limit) want = limit;
  return want < 1 ? 1 : want;
}

}  // namespace np
