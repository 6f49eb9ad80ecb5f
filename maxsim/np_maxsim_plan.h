// np_maxsim_plan.h -- the host side of np_hip_maxsim_batch that needs no device: the constants of the kernel's tiling, the
// argument checks and the split of a call into workgroups.  Plain C++; np_maxsim.hip includes it for the same constants.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace np {

constexpr int NP_MS_DT_F32 = 0, NP_MS_DT_BF16 = 1;   // NP_DT_F32 / NP_DT_BF16 of the public header
constexpr int NP_MS_DT_I8 = 2;                // NP_DT_I8: int8 codes with one f32 scale per row (the _i8 entries only)
constexpr int NP_MS_DT_B1 = 3;                // inside the library only: int8 query rows against document rows of one bit per dim (the _b1 entries)
constexpr int NP_MS_DT_I4 = 4;                // inside the library only: int8 query rows against document rows of one nibble per dim (the _i4 entries)
constexpr int NP_MS_DT_F16 = 5;               // NP_DT_F16: rows as raw IEEE binary16 words on both sides (the _f16 entries only)
constexpr int NP_MS_MAX_DIM = 1024;
constexpr int NP_MS_MAX_QUERY_TOKENS = 256;   // eight 32-token query tiles, as S6
constexpr int NP_MS_KC_F32 = 32;              // dims per LDS chunk, f32 MFMA (16 steps of 32x32x2)
constexpr int NP_MS_KC_BF16 = 64;             // dims per LDS chunk, bf16 MFMA (4 steps of 32x32x16)
constexpr int NP_MS_KC_I8 = 128;              // dims per LDS chunk, i8 MFMA (4 steps of 32x32x32): the bf16 chunk's bytes
constexpr int NP_MS_WG_DOCS = 4;              // documents a workgroup scores at most (one per wave when they are short)
constexpr int NP_MS_MAX_SLOTS = 8;            // 32-token query tiles a workgroup holds accumulators for
constexpr int64_t NP_MS_MAX_GRID_X = 0x7FFFFFFF;
constexpr int NP_MS_MAX_GRID_Y = 65535;

// The checks that need only host arrays.  0 = fine, 1 = shape error, 2 = invalid argument; *why names the argument (a
// string literal).  pair_docs may be NULL with a list (the device entry cannot see the ids); *bad_pair = the first pair
// whose id lies outside [0, n_docs), when the return value is 2 because of one (-1 otherwise).
// max_query_tokens: NP_MS_MAX_QUERY_TOKENS for every entry but the _long ones, which have no limit (maxsim_check_args_long).
inline int maxsim_check_args_upto(int64_t max_query_tokens, int32_t dtype, int32_t precision, int32_t dim, int32_t B,
                                  const int32_t* q_tok_offsets, int64_t n_docs, const int64_t* doc_tok_offsets, bool listed,
                                  const int64_t* pair_docs, const int64_t* pair_offsets, bool want_matches, const char** why,
                                  int64_t* bad_pair) {
  *why = "";
  *bad_pair = -1;
  if (dim < 1 || dim > NP_MS_MAX_DIM) return *why = "dim must lie in 1 .. 1024", 1;
  if (dtype != NP_MS_DT_F32 && dtype != NP_MS_DT_BF16) return *why = "dtype must be NP_DT_F32 (0) or NP_DT_BF16 (1)", 2;
  if (precision != 0 && precision != 3) return *why = "precision must be 0 (f32 MFMA) or 3 (bf16 MFMA)", 2;
  if (precision == 0 && dtype != NP_MS_DT_F32) return *why = "dtype NP_DT_BF16 needs precision 3", 2;
  if (want_matches && precision != 0)
    return *why = "out_match_sims / out_match_pos need precision 0: a position has no meaning under bf16 rounding", 2;
  if (B < 0) return *why = "B is negative", 2;
  if (n_docs < 0) return *why = "n_docs is negative", 2;
  if (B > 0 && !q_tok_offsets) return *why = "q_tok_offsets is NULL", 2;
  if (n_docs > 0 && !doc_tok_offsets) return *why = "doc_tok_offsets is NULL", 2;
  if (B > 0 && q_tok_offsets[0] != 0) return *why = "q_tok_offsets must start at 0", 2;
  for (int b = 0; b < B; ++b) {
    const int64_t lq = (int64_t)q_tok_offsets[b + 1] - q_tok_offsets[b];
    if (lq < 0) return *why = "q_tok_offsets must not decrease", 2;
    if (lq > max_query_tokens) return *why = "q_tok_offsets: a query has more than 256 tokens", 1;
  }
  if (n_docs > 0 && doc_tok_offsets[0] != 0) return *why = "doc_tok_offsets must start at 0", 2;
  for (int64_t i = 0; i < n_docs; ++i)
    if (doc_tok_offsets[i + 1] < doc_tok_offsets[i]) return *why = "doc_tok_offsets must not decrease", 2;
  if (!listed) {
    if ((n_docs + NP_MS_WG_DOCS - 1) / NP_MS_WG_DOCS > NP_MS_MAX_GRID_X) return *why = "n_docs exceeds one launch", 2;
    return 0;
  }
  if (B > 0 && !pair_offsets) return *why = "pair_offsets is NULL", 2;
  if (B > 0 && pair_offsets[0] != 0) return *why = "pair_offsets must start at 0", 2;
  for (int b = 0; b < B; ++b) {
    if (pair_offsets[b + 1] < pair_offsets[b]) return *why = "pair_offsets must not decrease", 2;
    if (pair_offsets[b + 1] - pair_offsets[b] > NP_MS_MAX_GRID_X) return *why = "pair_offsets: a query has more pairs than one launch takes", 2;
  }
  if (B > 0 && pair_offsets[B] > 0 && n_docs == 0) return *why = "pair_docs names documents but n_docs is 0", 2;
  if (pair_docs && B > 0)
    for (int64_t i = 0; i < pair_offsets[B]; ++i)
      if (pair_docs[i] < 0 || pair_docs[i] >= n_docs) return *bad_pair = i, *why = "pair_docs names a document outside [0, n_docs)", 2;
  return 0;
}
inline int maxsim_check_args(int32_t dtype, int32_t precision, int32_t dim, int32_t B, const int32_t* q_tok_offsets,
                             int64_t n_docs, const int64_t* doc_tok_offsets, bool listed, const int64_t* pair_docs,
                             const int64_t* pair_offsets, bool want_matches, const char** why, int64_t* bad_pair) {
  return maxsim_check_args_upto(NP_MS_MAX_QUERY_TOKENS, dtype, precision, dim, B, q_tok_offsets, n_docs, doc_tok_offsets, listed,
                                pair_docs, pair_offsets, want_matches, why, bad_pair);
}
// np_hip_maxsim_batch_long: the same tests without the one on a query's tokens (the int32 q_tok_offsets are the only bound)
inline int maxsim_check_args_long(int32_t dtype, int32_t precision, int32_t dim, int32_t B, const int32_t* q_tok_offsets,
                                  int64_t n_docs, const int64_t* doc_tok_offsets, bool listed, const int64_t* pair_docs,
                                  const int64_t* pair_offsets, bool want_matches, const char** why, int64_t* bad_pair) {
  return maxsim_check_args_upto(INT64_MAX, dtype, precision, dim, B, q_tok_offsets, n_docs, doc_tok_offsets, listed, pair_docs,
                                pair_offsets, want_matches, why, bad_pair);
}

// np_hip_maxsim_batch_i8: the same limits (rows of int8 codes multiply exactly, so matches are allowed as at precision 0),
// and both scale vectors must be there.
inline int maxsim_check_args_i8(int32_t dim, const void* q_scales, int32_t B, const int32_t* q_tok_offsets, const void* d_scales,
                                int64_t n_docs, const int64_t* doc_tok_offsets, bool listed, const int64_t* pair_docs,
                                const int64_t* pair_offsets, const char** why, int64_t* bad_pair) {
  *bad_pair = -1;
  if (!q_scales) return *why = "q_scales is NULL", 2;
  if (!d_scales) return *why = "d_scales is NULL", 2;
  return maxsim_check_args(NP_MS_DT_F32, 0, dim, B, q_tok_offsets, n_docs, doc_tok_offsets, listed, pair_docs, pair_offsets, true,
                           why, bad_pair);
}

// np_hip_maxsim_batch_b1: the int8 entry's checks, and the bit rows must be there when a document has a token.
inline int maxsim_check_args_b1(int32_t dim, const void* q_scales, int32_t B, const int32_t* q_tok_offsets, const void* doc_bits,
                                const void* d_scales, int64_t n_docs, const int64_t* doc_tok_offsets, bool listed,
                                const int64_t* pair_docs, const int64_t* pair_offsets, const char** why, int64_t* bad_pair) {
  const int c = maxsim_check_args_i8(dim, q_scales, B, q_tok_offsets, d_scales, n_docs, doc_tok_offsets, listed, pair_docs,
                                     pair_offsets, why, bad_pair);
  if (c == 0 && n_docs > 0 && doc_tok_offsets[n_docs] > 0 && !doc_bits) return *why = "doc_bits is NULL", 2;
  return c;
}

// np_hip_maxsim_batch_i4: the binary entry's checks; doc_words are the nibble rows.
inline int maxsim_check_args_i4(int32_t dim, const void* q_scales, int32_t B, const int32_t* q_tok_offsets, const void* doc_words,
                                const void* d_scales, int64_t n_docs, const int64_t* doc_tok_offsets, bool listed,
                                const int64_t* pair_docs, const int64_t* pair_offsets, const char** why, int64_t* bad_pair) {
  const int c = maxsim_check_args_i8(dim, q_scales, B, q_tok_offsets, d_scales, n_docs, doc_tok_offsets, listed, pair_docs,
                                     pair_offsets, why, bad_pair);
  if (c == 0 && n_docs > 0 && doc_tok_offsets[n_docs] > 0 && !doc_words) return *why = "doc_words is NULL", 2;
  return c;
}

// np_hip_maxsim_batch_f16: np_hip_maxsim_batch's limits (f16 products are exact in f32 and the rows are not rounded, so
// matches are allowed as at precision 0)
inline int maxsim_check_args_f16(int32_t dim, int32_t B, const int32_t* q_tok_offsets, int64_t n_docs, const int64_t* doc_tok_offsets,
                                 bool listed, const int64_t* pair_docs, const int64_t* pair_offsets, const char** why,
                                 int64_t* bad_pair) {
  return maxsim_check_args(NP_MS_DT_F32, 0, dim, B, q_tok_offsets, n_docs, doc_tok_offsets, listed, pair_docs, pair_offsets, true,
                           why, bad_pair);
}

// bytes of one row: f32 / bf16 / f16 / int8 rows are `dim` elements; a binary document row is ceil(dim / 32) 32-bit words, an
// int4 document row ceil(dim / 8) words, and the queries of both are int8 rows
inline size_t maxsim_row_bytes(int32_t dtype, int32_t dim, bool document) {
  if (dtype == NP_MS_DT_B1) return document ? (size_t)((dim + 31) / 32) * 4 : (size_t)dim;
  if (dtype == NP_MS_DT_I4) return document ? (size_t)((dim + 7) / 8) * 4 : (size_t)dim;
  if (dtype == NP_MS_DT_F16) return (size_t)dim * 2;
  return (size_t)dim * (dtype == NP_MS_DT_I8 ? 1 : dtype == NP_MS_DT_BF16 ? 2 : 4);
}

// np_hip_quantize_rows_i8: one wave takes a whole row, 16 elements a lane, so dim has maxsim's limit.  0 / 1 / 2 as above.
// np_hip_pack_rows_b1 and np_hip_quantize_rows_i4 have the same limits (out_codes = their words).
inline int quantize_check_args(int32_t dtype, int32_t dim, int64_t n_rows, const void* rows, const void* out_codes,
                               const void* out_scales, const char** why) {
  *why = "";
  if (dim < 1 || dim > NP_MS_MAX_DIM) return *why = "dim must lie in 1 .. 1024", 1;
  if (dtype != NP_MS_DT_F32 && dtype != NP_MS_DT_BF16) return *why = "dtype must be NP_DT_F32 (0) or NP_DT_BF16 (1)", 2;
  if (n_rows < 0) return *why = "n_rows is negative", 2;
  if (n_rows > 4 * NP_MS_MAX_GRID_X) return *why = "n_rows exceeds one launch", 2;
  if (n_rows > 0 && !rows) return *why = "rows is NULL", 2;
  if (n_rows > 0 && !out_codes) return *why = "out_codes is NULL", 2;
  if (n_rows > 0 && !out_scales) return *why = "out_scales is NULL", 2;
  return 0;
}

// How a call maps to workgroups.  A workgroup holds `slots` = G * nqt query tiles (nqt = tiles of the call's longest query;
// G queries of a group in all-pairs form, 1 in listed form) and walks the 32-token tiles of WD documents with its 4 waves.
// Both shrink while the grid would leave compute units idle: a pair's bits do not depend on either (np_maxsim.hip).
// NQT = the kernel instantiation (1, 2, 4 or 8 accumulator tiles) that holds the slots.
struct MaxsimPlan {
  int nqt = 1, G = 1, WD = NP_MS_WG_DOCS, NQT = 1;
  int64_t gx = 0;   // workgroups along x: document groups (all pairs) or the longest list's groups (listed)
  int64_t gy = 0;   // along y: query groups (all pairs) or queries (listed); launched in slices of NP_MS_MAX_GRID_Y
};
inline MaxsimPlan maxsim_plan(bool listed, const int32_t* q_tok_offsets, int32_t B, int64_t n_docs,
                              const int64_t* pair_offsets, int compute_units) {
  MaxsimPlan p;
  int max_lq = 1;
  int64_t max_n = listed ? 0 : n_docs;
  for (int b = 0; b < B; ++b) {
    if (q_tok_offsets[b + 1] - q_tok_offsets[b] > max_lq) max_lq = q_tok_offsets[b + 1] - q_tok_offsets[b];
    if (listed && pair_offsets[b + 1] - pair_offsets[b] > max_n) max_n = pair_offsets[b + 1] - pair_offsets[b];
  }
  p.nqt = (max_lq + 31) / 32;
  p.G = listed ? 1 : (NP_MS_MAX_SLOTS / p.nqt < B ? NP_MS_MAX_SLOTS / p.nqt : B);
  if (p.G < 1) p.G = 1;
  const int64_t want = 2 * (int64_t)(compute_units > 0 ? compute_units : 256);
  auto wgs = [&]() { return ((B + p.G - 1) / p.G) * ((max_n + p.WD - 1) / p.WD); };
  while (p.WD > 1 && wgs() < want) p.WD /= 2;
  while (p.G > 1 && wgs() < want) p.G = (p.G + 1) / 2;
  const int slots = p.G * p.nqt;
  p.NQT = slots <= 1 ? 1 : slots <= 2 ? 2 : slots <= 4 ? 4 : 8;
  p.gx = (max_n + p.WD - 1) / p.WD;
  p.gy = (B + p.G - 1) / p.G;
  return p;
}

// np_hip_maxsim_batch_long (np_maxsim_long.hip): a query of nqt 32-token tiles is walked in `passes` passes of at most SP tiles,
// so that the accumulators and the key table are one pass wide whatever the query's length.  The passes are even: the first
// nqt % passes of them take one tile more than the others (33 tiles at 8 a pass: 7, 7, 7, 6, 6).  SPmax: 8 for the bf16 MFMA
// modes; 4 for mode 0, where 8 accumulator tiles beside the f32 staging registers do not fit the register file without
// spills (profiles/maxsim_kernel_resources.md).  constexpr: the kernel evaluates the same three formulas per query.
constexpr int NP_MS_LONG_SPMAX_F32 = 4, NP_MS_LONG_SPMAX_BF16 = 8;
constexpr int maxsim_long_passes(int nqt, int spmax) { return (nqt + spmax - 1) / spmax; }
constexpr int maxsim_long_sp(int nqt, int passes) { return passes > 0 ? (nqt + passes - 1) / passes : 0; }
// first tile of pass ps (ps = passes: nqt); passes > 0
constexpr int maxsim_long_first(int nqt, int passes, int ps) {
  return ps * (nqt / passes) + (ps < nqt % passes ? ps : nqt % passes);
}

// blockIdx.y = one query in both forms (G = 1), blockIdx.x = WD documents or WD consecutive pairs of the query's list; WD
// halves while the grid would leave compute units idle.  nqt, passes and SP are those of the call's longest query; NQT = the
// instantiation (1, 2, 4 or 8 slots >= SP).  In the kernel a query's own passes = ceil(its tiles / NQT): for the longest
// query that is `passes` (SP <= NQT <= SPmax), and a pair's bits do not depend on the split anyway.
struct MaxsimLongPlan : MaxsimPlan {
  int passes = 0, SP = 0;
};
// the plan for passes of at most `spmax` tiles (1, 2, 4 or 8)
inline MaxsimLongPlan maxsim_long_plan_upto(int spmax, bool listed, const int32_t* q_tok_offsets, int32_t B, int64_t n_docs,
                                            const int64_t* pair_offsets, int compute_units) {
  MaxsimLongPlan p;
  int max_lq = 0;
  int64_t max_n = listed ? 0 : n_docs;
  for (int b = 0; b < B; ++b) {
    if (q_tok_offsets[b + 1] - q_tok_offsets[b] > max_lq) max_lq = q_tok_offsets[b + 1] - q_tok_offsets[b];
    if (listed && pair_offsets[b + 1] - pair_offsets[b] > max_n) max_n = pair_offsets[b + 1] - pair_offsets[b];
  }
  p.nqt = (int)(((int64_t)max_lq + 31) / 32);
  p.passes = maxsim_long_passes(p.nqt, spmax);
  p.SP = maxsim_long_sp(p.nqt, p.passes);
  p.NQT = p.SP <= 1 ? 1 : p.SP <= 2 ? 2 : p.SP <= 4 ? 4 : 8;
  p.G = 1;
  const int64_t want = 2 * (int64_t)(compute_units > 0 ? compute_units : 256);
  while (p.WD > 1 && (int64_t)B * ((max_n + p.WD - 1) / p.WD) < want) p.WD /= 2;
  p.gx = (max_n + p.WD - 1) / p.WD;
  p.gy = B;
  return p;
}
inline MaxsimLongPlan maxsim_long_plan(int mode, bool listed, const int32_t* q_tok_offsets, int32_t B, int64_t n_docs,
                                       const int64_t* pair_offsets, int compute_units) {
  return maxsim_long_plan_upto(mode == 0 ? NP_MS_LONG_SPMAX_F32 : NP_MS_LONG_SPMAX_BF16, listed, q_tok_offsets, B, n_docs,
                               pair_offsets, compute_units);
}

// np_hip_maxsim_batch_long_i8 (np_maxsim_long_i8.hip): int8 rows for the _long entries.  The int8 entry's checks without the
// one on a query's tokens.
inline int maxsim_check_args_long_i8(int32_t dim, const void* q_scales, int32_t B, const int32_t* q_tok_offsets,
                                     const void* d_scales, int64_t n_docs, const int64_t* doc_tok_offsets, bool listed,
                                     const int64_t* pair_docs, const int64_t* pair_offsets, const char** why, int64_t* bad_pair) {
  *bad_pair = -1;
  if (!q_scales) return *why = "q_scales is NULL", 2;
  if (!d_scales) return *why = "d_scales is NULL", 2;
  return maxsim_check_args_upto(INT64_MAX, NP_MS_DT_F32, 0, dim, B, q_tok_offsets, n_docs, doc_tok_offsets, listed, pair_docs,
                                pair_offsets, true, why, bad_pair);
}
// A pass's query rows stay in LDS at their whole width: a row is `dim` bytes, rows maxsim_long_i8_pitch(dim) bytes apart -- an
// ODD number of 16-byte units (consecutive rows start in different bank groups) that covers dim rounded up to the 32 dims of an
// MFMA step, so a step's fragment never leaves its row.  Beside the rows: the two key tables and the meta block.  SPmax(dim) is
// the widest pass (8, 4, 2 or 1 tiles) that fits NP_MS_LONG_I8_BUDGET: half of a compute unit's 160 KB, so that two workgroups
// share one and one's staging hides behind the other's MFMAs.  dim 128: 8 tiles in 52.1 KB; dim 512: 4 tiles in 74.1 KB;
// dim 1024 (pitch 1040): 2 tiles in 69.1 KB.  constexpr: the kernel evaluates the pitch and the offsets from the same formulas.
constexpr int NP_MS_LONG_I8_BUDGET = 80 * 1024;
constexpr int NP_MS_LONG_I8_META = 128;       // NP_MS_META of np_maxsim_dev.h
constexpr int maxsim_long_i8_pitch(int dim) { return 16 * (2 * ((dim + 31) / 32) + 1); }
constexpr size_t maxsim_long_i8_key_off(int dim, int nqt) { return (size_t)nqt * 32 * maxsim_long_i8_pitch(dim); }
constexpr size_t maxsim_long_i8_meta_off(int dim, int nqt) {
  return maxsim_long_i8_key_off(dim, nqt) + 2 * (size_t)NP_MS_WG_DOCS * nqt * 32 * 8;
}
constexpr size_t maxsim_long_i8_lds(int dim, int nqt) { return maxsim_long_i8_meta_off(dim, nqt) + NP_MS_LONG_I8_META; }
constexpr int maxsim_long_i8_spmax(int dim) {
  return maxsim_long_i8_lds(dim, 8) <= NP_MS_LONG_I8_BUDGET ? 8 : maxsim_long_i8_lds(dim, 4) <= NP_MS_LONG_I8_BUDGET ? 4
       : maxsim_long_i8_lds(dim, 2) <= NP_MS_LONG_I8_BUDGET ? 2 : 1;
}
inline MaxsimLongPlan maxsim_long_i8_plan(int dim, bool listed, const int32_t* q_tok_offsets, int32_t B, int64_t n_docs,
                                          const int64_t* pair_offsets, int compute_units) {
  return maxsim_long_plan_upto(maxsim_long_i8_spmax(dim), listed, q_tok_offsets, B, n_docs, pair_offsets, compute_units);
}

}  // namespace np
