// np_scan_plan.h -- the host side of np_hip_search_exact that needs no device: argument checks, the packing of queries into
// groups of 32-token tiles, and the plan of query slices and document passes under a byte budget.  Plain C++ (the packing
// also compiles as device code: the scan builds its group table on the device from the token offsets it already has there);
// tests/cpp/scan_plan_check.cpp runs all of it stand-alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NP_SCAN_HD __host__ __device__
#else
#define NP_SCAN_HD
#endif

namespace np {

constexpr int NP_SCAN_MAX_TILES = 8;       // 32-token query tiles a workgroup can hold (256 query tokens)
constexpr int NP_SCAN_MAX_TOPK = 16384;    // the exact window the search path has too: 8 bytes per key in 128 KB of LDS
constexpr int NP_SCAN_MAX_QUERY_TOKENS = 32 * NP_SCAN_MAX_TILES;

// tiles a query of lq tokens takes: whole tiles, at least one (a query without tokens scores every document 0)
NP_SCAN_HD inline int scan_query_tiles(int lq) { return lq <= 0 ? 1 : (lq + 31) / 32; }

// Greedy packing in query order: a group takes whole queries while their tiles stay within `scan_tiles`; a query with more
// tiles than that gets a group of its own (a (document, query) sum always finishes inside one workgroup).  Tiles of a query
// are adjacent and in order.  tile_info[g * 8 + x] = query | tile-of-query << 16, or -1 for an unused slot (may be NULL: count
// only).  Returns the number of groups (<= B); *max_tiles = the most tiles any group holds.  Every query must have at most
// NP_SCAN_MAX_QUERY_TOKENS tokens and B must be below 65536.
NP_SCAN_HD inline int scan_pack_groups(const int32_t* qoff, int B, int scan_tiles, int32_t* tile_info, int* max_tiles) {
  int g = -1, used = NP_SCAN_MAX_TILES + 1, mt = 0;
  if (scan_tiles < 1) scan_tiles = 1;
  if (scan_tiles > NP_SCAN_MAX_TILES) scan_tiles = NP_SCAN_MAX_TILES;
  for (int b = 0; b < B; ++b) {
    const int nt = scan_query_tiles(qoff[b + 1] - qoff[b]);
    if (g < 0 || used + nt > scan_tiles) {   // open a group
      ++g;
      used = 0;
      if (tile_info)
        for (int x = 0; x < NP_SCAN_MAX_TILES; ++x) tile_info[g * NP_SCAN_MAX_TILES + x] = -1;
    }
    for (int t = 0; t < nt; ++t)
      if (tile_info) tile_info[g * NP_SCAN_MAX_TILES + used + t] = b | (t << 16);
    used += nt;
    if (used > mt) mt = used;
  }
  if (max_tiles) *max_tiles = mt;
  return g + 1;
}

// The checks of np_hip_search_exact that need only the host's arguments.  0 = fine, 1 = shape error, 2 = invalid argument;
// *why names the reason (a string literal).
inline int scan_check_args(int32_t B, int32_t dim, int32_t index_dim, bool geometry_supported, int32_t top_k,
                           int32_t precision, const int32_t* q_tok_offsets, const char** why) {
  *why = "";
  if (B < 0) return *why = "negative batch size", 2;
  if (dim != index_dim) return *why = "query dim does not match index dim", 1;
  if (!geometry_supported) return *why = "the exact scan supports dim <= 128", 1;
  if (top_k < 1 || top_k > NP_SCAN_MAX_TOPK) return *why = "top_k must be in 1..16384", 2;
  if (precision != 0 && precision != 3) return *why = "precision must be 0 (f32) or 3 (bf16)", 2;
  if (B >= 65536) return *why = "more than 65535 queries in one call", 2;
  if (q_tok_offsets) {
    if (q_tok_offsets[0] != 0) return *why = "q_tok_offsets[0] must be 0", 1;
    for (int b = 0; b < B; ++b) {
      const int64_t lq = (int64_t)q_tok_offsets[b + 1] - q_tok_offsets[b];
      if (lq < 0) return *why = "q_tok_offsets must be non-decreasing", 1;
      if (lq > NP_SCAN_MAX_QUERY_TOKENS) return *why = "a query has more than 256 tokens", 1;
    }
  }
  return 0;
}

// Slices and passes: S queries at a time, P documents per pass, so that
//     S * per_query + S * P * 8 (the key table) + fixed  <=  budget.
// S starts at min(B, max_batch) and halves while a pass could not hold min(n_docs, 1024) documents; P is then what the rest of
// the budget holds, capped by n_docs and by `scan_docs` when that is positive.  false: even one query and one document do
// not fit.
struct ScanPlan {
  int S = 1;
  int64_t P = 1;
};
inline bool scan_plan(int64_t budget, int64_t fixed, int64_t per_query, int64_t n_docs, int B, int max_batch,
                      int64_t scan_docs, ScanPlan* out) {
  if (n_docs < 1) n_docs = 1;
  int S = B < 1 ? 1 : B;
  if (max_batch >= 1 && S > max_batch) S = max_batch;
  const int64_t want = n_docs < 1024 ? n_docs : 1024;
  for (;;) {
    const int64_t left = budget - fixed - (int64_t)S * per_query;
    const int64_t P = left > 0 ? left / ((int64_t)S * 8) : 0;
    if (P >= want || S == 1) {
      if (P < 1) return false;
      out->S = S;
      out->P = P < n_docs ? P : n_docs;
      if (scan_docs > 0 && out->P > scan_docs) out->P = scan_docs;
      return true;
    }
    S = (S + 1) / 2;
  }
}

}  // namespace np
