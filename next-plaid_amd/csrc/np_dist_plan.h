// np_dist_plan.h -- the host side of the sharded keyword and filtered searches that needs no device: the layouts of the records a
// rank sends (offsets, sizes, the status trailer the keyword records end in), the rule that cuts a batch into exchanges (a function of
// the call's arguments alone: every rank must run the same number of collectives of the same size, whatever its workspace
// budget), and the summation and cross-check of the gathered hit counts.  Plain C++; tests/cpp/dist_plan_check.cpp runs all of
// it stand-alone.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/nextplaid_hip.h"

namespace np {

// ---- the status word: 0 = healthy, else np_status | (rank + 1) << 32 ------------------------------------------------------
inline uint64_t dist_status_word(int rank, int rc) { return rc == NP_OK ? 0ull : ((uint64_t)(rank + 1) << 32) | (uint32_t)rc; }
inline int dist_status_rank(uint64_t w) { return w ? (int)(w >> 32) - 1 : -1; }
inline int dist_status_code(uint64_t w) { return (int)(w & 0xffffffffu); }

// first non-zero status word among G gathered records of rec_bytes each (host memory), or 0
inline uint64_t dist_first_failure(const char* h_all, size_t rec_bytes, size_t off_status, int G) {
  for (int g = 0; g < G; ++g) {
    uint64_t w;
    memcpy(&w, h_all + (size_t)g * rec_bytes + off_status, 8);
    if (w) return w;
  }
  return 0;
}

// ---- the eligible-centroid exchange of a sharded semantic pass with subsets (dense probe only) -------------------------------
//   bitmaps [rows][words] u32 | [filters only] local lengths [rows] i64
// `words` = K padded to 64, over 32: even, so the lengths start on an 8-byte boundary.  There is no status word here: the record
// is OR-ed and summed on the device, and a failed rank sends zeros (its status travels in the next record).
struct DistEligRec {
  size_t o_lens = 0, bytes = 0;
  bool lens = false;
};
inline DistEligRec dist_elig_record(int64_t rows, int64_t words, bool with_lens) {
  DistEligRec r;
  r.o_lens = (size_t)rows * (size_t)words * 4;
  r.lens = with_lens;
  r.bytes = r.o_lens + (with_lens ? (size_t)rows * 8 : 0);
  return r;
}

// ---- exchange 1, only in a batch with a phrase of several known tokens: the shard's nHit of those phrases -------------------
//   nhit [n_items] u64 | n_rows i64 | status u64
struct DistCountRec {
  int64_t n_items = 0;
  size_t o_rows = 0, o_status = 0, bytes = 0;
};
inline DistCountRec dist_count_record(int64_t n_items) {
  DistCountRec r;
  r.n_items = n_items < 0 ? 0 : n_items;
  r.o_rows = (size_t)r.n_items * 8;
  r.o_status = r.o_rows + 8;
  r.bytes = r.o_status + 8;
  return r;
}

// The gathered records summed: sums[i] = the phrase's nHit over the healthy ranks, *failed = the first non-zero status word,
// *n_rows = the healthy ranks' nRow (0 if none is healthy).  Returns 0, or 1 when two healthy ranks report different nRow
// (they were handed different tables; *rank_a and *rank_b name the first such pair): every rank reads the same bytes, so
// every rank decides alike.
inline int dist_sum_counts(const char* h_all, const DistCountRec& r, int G, uint64_t* sums, uint64_t* failed, int64_t* n_rows,
                           int* rank_a, int* rank_b) {
  for (int64_t i = 0; i < r.n_items; ++i) sums[i] = 0;
  *failed = dist_first_failure(h_all, r.bytes, r.o_status, G);
  *n_rows = 0;
  int first = -1, mismatch = 0;
  for (int g = 0; g < G; ++g) {
    const char* rec = h_all + (size_t)g * r.bytes;
    uint64_t w;
    memcpy(&w, rec + r.o_status, 8);
    if (w) continue;   // a failed rank sends no counts
    int64_t rows;
    memcpy(&rows, rec + r.o_rows, 8);
    if (first < 0) {
      first = g;
      *n_rows = rows;
    } else if (rows != *n_rows && !mismatch) {
      mismatch = 1;
      if (rank_a) *rank_a = first;
      if (rank_b) *rank_b = g;
    }
    for (int64_t i = 0; i < r.n_items; ++i) {
      uint64_t v;
      memcpy(&v, rec + (size_t)i * 8, 8);
      sums[i] += v;
    }
  }
  return mismatch;
}

// ---- exchange 2: the shard's top-k of a run of queries ----------------------------------------------------------------------
//   keys [B * top_k] u64 (bits of the f64 score) | ids [B * top_k] i64 (global) | counts [B] i32, padded to 8 bytes | status u64
struct DistTextRec {
  int32_t B = 0, top_k = 0;
  size_t o_keys = 0, o_ids = 0, o_counts = 0, o_status = 0, bytes = 0;
};
inline DistTextRec dist_text_record(int32_t B, int32_t top_k) {
  DistTextRec r;
  r.B = B;
  r.top_k = top_k;
  const size_t n = (size_t)B * (size_t)top_k;
  r.o_ids = n * 8;
  r.o_counts = r.o_ids + n * 8;
  r.o_status = (r.o_counts + (size_t)B * 4 + 7) / 8 * 8;
  r.bytes = r.o_status + 8;
  return r;
}

// Queries per exchange: as many as keep one rank's record at NP_DIST_EXCHANGE_BYTES or less, at least one; a batch takes
// ceil(B / that) exchanges.  B and top_k only.
constexpr int64_t NP_DIST_EXCHANGE_BYTES = 4ll << 20;
inline int32_t dist_text_exchange_queries(int32_t B, int32_t top_k) {
  const int64_t per_query = (int64_t)(top_k < 1 ? 1 : top_k) * 16 + 4;
  int64_t q = (NP_DIST_EXCHANGE_BYTES - 16) / per_query;
  if (q < 1) q = 1;
  if (q > B) q = B;
  return (int32_t)(q < 1 ? 1 : q);
}
inline int32_t dist_text_exchanges(int32_t B, int32_t top_k) {
  if (B <= 0) return 0;
  const int32_t q = dist_text_exchange_queries(B, top_k);
  return (B + q - 1) / q;
}

}  // namespace np
