// next_plaid_maxsim_long.hpp -- the C++ host mirror of batched MaxSim for queries of any length: maxsim_scores_long
// (np_hip_maxsim_batch_long) and maxsim_scores_long_i8 (np_hip_maxsim_batch_long_i8), beside maxsim_scores_f16 of
// next_plaid_maxsim_f16.hpp and maxsim_scores_i8 of next_plaid_maxsim_i8.hpp, whose argument conventions they keep.
// Host-only; the library refuses what it does not take and `check` throws.
#pragma once
#include "next_plaid_maxsim_i8.hpp"

namespace next_plaid {

// What the two mirrors below share: the pair lists flattened, the outputs sized, and `entry(B, n_docs, pair ids or NULL, pair
// offsets or NULL, scores, sims or NULL, positions or NULL)` -- the call of the C entry -- checked.
template <class Entry>
inline MaxsimScores maxsim_long_call(const char* who, const std::vector<int32_t>& q_tok_offsets,
                                     const std::vector<int64_t>& doc_tok_offsets, const std::vector<std::vector<int64_t>>& pairs,
                                     bool want_matches, Entry entry) {
  const size_t B = q_tok_offsets.empty() ? 0 : q_tok_offsets.size() - 1;
  const size_t n = doc_tok_offsets.empty() ? 0 : doc_tok_offsets.size() - 1;
  const bool listed = !pairs.empty();
  if (listed && pairs.size() != B)
    throw Error(NP_ERR_INVALID_ARGUMENT, (std::string(who) + ": one list of document ids per query").c_str());
  std::vector<int64_t> ids, poff(B + 1, 0);
  size_t rows = 0;
  for (size_t b = 0; b < B; ++b) {
    const size_t nb = listed ? pairs[b].size() : n;
    if (listed) ids.insert(ids.end(), pairs[b].begin(), pairs[b].end());
    poff[b + 1] = poff[b] + (int64_t)nb;
    rows += nb * (size_t)std::max(q_tok_offsets[b + 1] - q_tok_offsets[b], 0);
  }
  MaxsimScores out;
  out.scores.assign(std::max<size_t>((size_t)poff[B], 1), 0.f);
  if (want_matches) {
    out.sims.assign(std::max<size_t>(rows, 1), 0.f);
    out.positions.assign(std::max<size_t>(rows, 1), -1);
  }
  if (listed && ids.empty()) ids.push_back(0);
  check(entry((int32_t)B, (int64_t)n, listed ? ids.data() : nullptr, listed ? poff.data() : nullptr, out.scores.data(),
              want_matches ? out.sims.data() : nullptr, want_matches ? out.positions.data() : nullptr));
  out.scores.resize((size_t)poff[B]);
  if (want_matches) {
    out.sims.resize(rows);
    out.positions.resize(rows);
  }
  return out;
}

// MaxSim of f32 rows (dtype NP_DT_F32, precision 0 = f32 MFMA or 3 = rounded to bf16) or of bf16 rows as raw 16-bit words
// (NP_DT_BF16, precision 3), with no limit on a query's tokens.  queries / docs: flat [tokens][dim] rows with their token
// offsets; `pairs` and want_matches (precision 0 only) as maxsim_scores_i8.
inline MaxsimScores maxsim_scores_long(const void* queries, const std::vector<int32_t>& q_tok_offsets, const void* docs,
                                       const std::vector<int64_t>& doc_tok_offsets, size_t dim, int dtype = NP_DT_F32,
                                       int precision = 0, const std::vector<std::vector<int64_t>>& pairs = {},
                                       bool want_matches = false, int device = 0) {
  return maxsim_long_call("maxsim_scores_long", q_tok_offsets, doc_tok_offsets, pairs, want_matches,
                          [&](int32_t B, int64_t n, const int64_t* ids, const int64_t* poff, float* sc, float* sims, int32_t* pos) {
                            return np_hip_maxsim_batch_long(device, dtype, precision, (int32_t)dim, queries, q_tok_offsets.data(), B,
                                                            docs, doc_tok_offsets.data(), n, ids, poff, sc, sims, pos);
                          });
}

// maxsim_scores_i8 with no limit on a query's tokens (np_hip_maxsim_batch_long_i8): the same arguments, the same bits for a
// query of at most 256 tokens.
inline MaxsimScores maxsim_scores_long_i8(const int8_t* queries, const float* q_scales, const std::vector<int32_t>& q_tok_offsets,
                                          const int8_t* docs, const float* d_scales, const std::vector<int64_t>& doc_tok_offsets,
                                          size_t dim, const std::vector<std::vector<int64_t>>& pairs = {}, bool want_matches = false,
                                          int device = 0) {
  return maxsim_long_call("maxsim_scores_long_i8", q_tok_offsets, doc_tok_offsets, pairs, want_matches,
                          [&](int32_t B, int64_t n, const int64_t* ids, const int64_t* poff, float* sc, float* sims, int32_t* pos) {
                            return np_hip_maxsim_batch_long_i8(device, (int32_t)dim, queries, q_scales, q_tok_offsets.data(), B, docs,
                                                               d_scales, doc_tok_offsets.data(), n, ids, poff, sc, sims, pos);
                          });
}

}  // namespace next_plaid
