// next_plaid_maxsim_long.hpp -- the C++ host mirror of batched MaxSim for queries of any length: maxsim_scores_long
// (np_hip_maxsim_batch_long), beside maxsim_scores_f16 of next_plaid_maxsim_f16.hpp, whose argument conventions it keeps.
// Host-only; the library refuses what it does not take and `check` throws.
#pragma once
#include "next_plaid_maxsim_i8.hpp"

namespace next_plaid {

// MaxSim of f32 rows (dtype NP_DT_F32, precision 0 = f32 MFMA or 3 = rounded to bf16) or of bf16 rows as raw 16-bit words
// (NP_DT_BF16, precision 3), with no limit on a query's tokens.  queries / docs: flat [tokens][dim] rows with their token
// offsets; `pairs` and want_matches (precision 0 only) as maxsim_scores_i8.
inline MaxsimScores maxsim_scores_long(const void* queries, const std::vector<int32_t>& q_tok_offsets, const void* docs,
                                       const std::vector<int64_t>& doc_tok_offsets, size_t dim, int dtype = NP_DT_F32,
                                       int precision = 0, const std::vector<std::vector<int64_t>>& pairs = {},
                                       bool want_matches = false, int device = 0) {
  const size_t B = q_tok_offsets.empty() ? 0 : q_tok_offsets.size() - 1;
  const size_t n = doc_tok_offsets.empty() ? 0 : doc_tok_offsets.size() - 1;
  const bool listed = !pairs.empty();
  if (listed && pairs.size() != B) throw Error(NP_ERR_INVALID_ARGUMENT, "maxsim_scores_long: one list of document ids per query");
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
  check(np_hip_maxsim_batch_long(device, dtype, precision, (int32_t)dim, queries, q_tok_offsets.data(), (int32_t)B, docs,
                                 doc_tok_offsets.data(), (int64_t)n, listed ? ids.data() : nullptr,
                                 listed ? poff.data() : nullptr, out.scores.data(), want_matches ? out.sims.data() : nullptr,
                                 want_matches ? out.positions.data() : nullptr));
  out.scores.resize((size_t)poff[B]);
  if (want_matches) {
    out.sims.resize(rows);
    out.positions.resize(rows);
  }
  return out;
}

}  // namespace next_plaid
