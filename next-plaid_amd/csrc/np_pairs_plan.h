// np_pairs_plan.h -- the host side of np_hip_score_pairs that needs no device: argument checks, the offsets of the
// per-token rows, the map from workgroups to queries, the query slices and the staging chunks of the host entry.  Plain
// C++ (the workgroup map also compiles as device code: a launch builds it on the device from the offsets it already has
// there, with the very function the host sizes the grid by); tests/cpp/pairs_plan_check.cpp runs all of it stand-alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NP_PAIRS_HD __host__ __device__
#else
#define NP_PAIRS_HD
#endif

namespace np {

constexpr int NP_PAIRS_MAX_QUERY_TOKENS = 256;   // eight 32-token query tiles, as S6
constexpr int NP_PAIRS_WG_DOCS = 16;             // pairs per workgroup: 4 waves x NP_EXACT_DPW documents
constexpr int64_t NP_PAIRS_MAX_GRID = 0x7FFFFFFF;
constexpr int64_t NP_PAIRS_MAX_CHUNK = (int64_t)64 << 20;   // bytes of pinned staging the host entry takes at most

// workgroups query i takes: its pairs are contiguous, one wave scores NP_EXACT_DPW of them
NP_PAIRS_HD inline int64_t pairs_query_wgs(int64_t n) { return (n + NP_PAIRS_WG_DOCS - 1) / NP_PAIRS_WG_DOCS; }

// The checks that need only the host's arguments.  0 = fine, 1 = shape error, 2 = invalid argument; *why names the
// reason (a string literal).  q_tok_offsets / pair_offsets: [B + 1], may be NULL only when B == 0.
inline int pairs_check_args(int32_t B, int32_t dim, int32_t index_dim, bool geometry_supported, int32_t precision,
                            const int32_t* q_tok_offsets, const int64_t* pair_offsets, const char** why) {
  *why = "";
  if (B < 0) return *why = "negative batch size", 2;
  if (dim != index_dim) return *why = "query dim does not match index dim", 1;
  if (!geometry_supported) return *why = "score_pairs supports dim <= 128", 1;
  if (precision != 0)
    return *why = "precision must be 0 (exact f32): a token position has no meaning under bf16 rounding", 2;
  if (B > 0 && (!q_tok_offsets || !pair_offsets)) return *why = "NULL offsets", 2;
  if (B == 0) return 0;
  if (q_tok_offsets[0] != 0) return *why = "q_tok_offsets[0] must be 0", 1;
  for (int b = 0; b < B; ++b) {
    const int64_t lq = (int64_t)q_tok_offsets[b + 1] - q_tok_offsets[b];
    if (lq < 0) return *why = "q_tok_offsets must be non-decreasing", 1;
    if (lq > NP_PAIRS_MAX_QUERY_TOKENS) return *why = "a query has more than 256 tokens", 1;
  }
  if (pair_offsets[0] != 0) return *why = "pair_offsets[0] must be 0", 2;
  for (int b = 0; b < B; ++b) {
    if (pair_offsets[b + 1] < pair_offsets[b]) return *why = "pair_offsets must be non-decreasing", 2;
    if (pairs_query_wgs(pair_offsets[b + 1] - pair_offsets[b]) > NP_PAIRS_MAX_GRID)
      return *why = "a query has more pairs than one launch can take", 2;
  }
  return 0;
}

// index of the first id outside [0, num_documents), or -1
inline int64_t pairs_first_bad_id(const int64_t* pair_docs, int64_t P, int64_t num_documents) {
  for (int64_t i = 0; i < P; ++i)
    if (pair_docs[i] < 0 || pair_docs[i] >= num_documents) return i;
  return -1;
}

// R = sum_i n_i * Lq_i over queries [0, B): the entries of out_token_sims / out_token_pos
inline int64_t pairs_rows(const int32_t* qoff, const int64_t* poff, int B) {
  int64_t r = 0;
  for (int b = 0; b < B; ++b) r += (poff[b + 1] - poff[b]) * (int64_t)(qoff[b + 1] - qoff[b]);
  return r;
}

// The workgroup map of a slice of Sn queries (qoff / poff point at the slice's first query): wgpre[i] = workgroups of the
// queries before i, rowbase[i] = row entries of the queries before i; both [Sn + 1] (either may be NULL: count only).
// Returns the workgroups of the slice.
NP_PAIRS_HD inline int64_t pairs_prefix(const int32_t* qoff, const int64_t* poff, int Sn, int32_t* wgpre, int64_t* rowbase) {
  int64_t w = 0, r = 0;
  for (int i = 0; i < Sn; ++i) {
    if (wgpre) wgpre[i] = (int32_t)w;
    if (rowbase) rowbase[i] = r;
    const int64_t n = poff[i + 1] - poff[i];
    w += pairs_query_wgs(n);
    r += n * (int64_t)(qoff[i + 1] - qoff[i]);
  }
  if (wgpre) wgpre[Sn] = (int32_t)w;
  if (rowbase) rowbase[Sn] = r;
  return w;
}

// the query a workgroup serves: the i with wgpre[i] <= wg < wgpre[i + 1] (wg < wgpre[Sn]); queries without pairs own none
NP_PAIRS_HD inline int pairs_query_of(const int32_t* wgpre, int Sn, int64_t wg) {
  int lo = 0, hi = Sn - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)wgpre[mid + 1] <= wg) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Queries [q0, q0 + return value) form the next slice: at most S of them, and no more workgroups than a one-dimensional
// grid holds (a single query never exceeds it: pairs_check_args).  *max_lq = the longest query of the slice.
inline int pairs_next_slice(const int32_t* qoff, const int64_t* poff, int q0, int B, int S, int* max_lq) {
  int64_t w = 0;
  int n = 0, ml = 0;
  while (q0 + n < B && n < S) {
    const int64_t add = pairs_query_wgs(poff[q0 + n + 1] - poff[q0 + n]);
    if (n > 0 && w + add > NP_PAIRS_MAX_GRID) break;
    w += add;
    const int lq = qoff[q0 + n + 1] - qoff[q0 + n];
    if (lq > ml) ml = lq;
    ++n;
  }
  if (max_lq) *max_lq = ml;
  return n;
}

// bytes of staging one pair of a query of lq tokens takes: its id, its score and (with rows) a sim and a position per token
inline int64_t pairs_pair_bytes(int lq, bool rows) { return 8 + 4 + (rows ? (int64_t)lq * 8 : 0); }

// A chunk of the host entry: pairs [p0, p1) of the call's list -- whole queries or a part of one, pairs are independent --
// which touch queries [q0, q1) and own the row entries [r0, r1).
struct PairsChunk {
  int q0 = 0, q1 = 0;
  int64_t p0 = 0, p1 = 0, r0 = 0, r1 = 0;
};
// The chunk that starts at pair `p0` (row entry `r0`; q_hint: a query at or before the one that owns p0): as many pairs as
// `cap` bytes of staging hold, at least one.  false: no pair is left, or one pair does not fit.
inline bool pairs_next_chunk(const int32_t* qoff, const int64_t* poff, int B, bool rows, int64_t cap, int q_hint, int64_t p0,
                             int64_t r0, PairsChunk* out) {
  if (B <= 0 || p0 >= poff[B]) return false;
  int q = q_hint < 0 ? 0 : q_hint;
  while (q < B && poff[q + 1] <= p0) ++q;   // the owner of p0 (queries without pairs are passed over)
  if (q >= B) return false;
  PairsChunk c;
  c.q0 = q;
  c.p0 = c.p1 = p0;
  c.r0 = c.r1 = r0;
  int64_t left = cap;
  for (; q < B; ++q) {
    const int lq = qoff[q + 1] - qoff[q];
    const int64_t each = pairs_pair_bytes(lq, rows);
    const int64_t from = c.p1 > poff[q] ? c.p1 : poff[q];
    const int64_t have = poff[q + 1] - from;
    if (have <= 0) continue;
    int64_t take = left / each;
    if (take > have) take = have;
    if (take <= 0) break;
    c.p1 = from + take;
    c.r1 += rows ? take * (int64_t)lq : 0;
    c.q1 = q + 1;
    left -= take * each;
    if (take < have) break;
  }
  if (c.p1 == c.p0) return false;
  *out = c;
  return true;
}

// Slices and staging under the budget:  fixed + S * per_query + chunk  <=  budget.  S starts at min(B, max_batch) and
// halves while the chunk could not hold one pair of the longest query (`worst_pair` bytes); the chunk is the rest, at most
// NP_PAIRS_MAX_CHUNK.  chunk = 0 for the device entry (worst_pair = 0: nothing is staged).  false: one query and one pair
// do not fit.
struct PairsPlan {
  int S = 1;
  int64_t chunk = 0;
};
inline bool pairs_plan(int64_t budget, int64_t fixed, int64_t per_query, int B, int max_batch, int64_t worst_pair,
                       PairsPlan* out) {
  int S = B < 1 ? 1 : B;
  if (max_batch >= 1 && S > max_batch) S = max_batch;
  for (;;) {
    const int64_t left = budget - fixed - (int64_t)S * per_query;
    if (left >= worst_pair && left >= 0) {
      out->S = S;
      out->chunk = worst_pair == 0 ? 0 : (left < NP_PAIRS_MAX_CHUNK ? left : NP_PAIRS_MAX_CHUNK);
      return true;
    }
    if (S == 1) return false;
    S = (S + 1) / 2;
  }
}

}  // namespace np
