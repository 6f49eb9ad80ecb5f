// next_plaid_maxsim_i8.hpp -- the C++ host mirror of the int8 form of batched MaxSim: quantize_rows (np_hip_quantize_rows_i8)
// and maxsim_scores_i8 (np_hip_maxsim_batch_i8), beside maxsim_scores of next_plaid.hpp, whose argument conventions they
// keep.  Host-only; the library refuses what it does not take and `check` throws.
#pragma once
#include "../next-plaid_amd/cpp/next_plaid.hpp"

namespace next_plaid {

// rows [n_rows][dim] f32 -> one int8 code per element and one f32 scale per row: scale = max|x| / 127, code =
// rint(x * (127 / max|x|)); a row with a non-finite element gets scale NaN and codes 0.
struct QuantizedRows {
  std::vector<int8_t> codes;   // [n_rows][dim]
  std::vector<float> scales;   // [n_rows]
};
inline QuantizedRows quantize_rows(const float* rows, size_t n_rows, size_t dim, int device = 0) {
  QuantizedRows out;
  out.codes.assign(std::max<size_t>(n_rows * dim, 1), 0);
  out.scales.assign(std::max<size_t>(n_rows, 1), 0.f);
  check(np_hip_quantize_rows_i8(device, NP_DT_F32, (int32_t)dim, rows, (int64_t)n_rows, out.codes.data(), out.scales.data()));
  out.codes.resize(n_rows * dim);
  out.scales.resize(n_rows);
  return out;
}

// MaxSim of int8 rows with their row scales on the i8 MFMA kernel: sim = (integer dot product) * document scale * query
// scale, exact but for those two f32 multiplications.  queries / docs are flat [tokens][dim] codes with one scale per token
// and their token offsets; `pairs` holds one id list per query, or is empty for all pairs (scores [B][n_docs], query-major).
// With want_matches every (pair, query token) also gets its best document token, as maxsim_scores at precision 0.
inline MaxsimScores maxsim_scores_i8(const int8_t* queries, const float* q_scales, const std::vector<int32_t>& q_tok_offsets,
                                     const int8_t* docs, const float* d_scales, const std::vector<int64_t>& doc_tok_offsets,
                                     size_t dim, const std::vector<std::vector<int64_t>>& pairs = {}, bool want_matches = false,
                                     int device = 0) {
  const size_t B = q_tok_offsets.empty() ? 0 : q_tok_offsets.size() - 1;
  const size_t n = doc_tok_offsets.empty() ? 0 : doc_tok_offsets.size() - 1;
  const bool listed = !pairs.empty();
  if (listed && pairs.size() != B) throw Error(NP_ERR_INVALID_ARGUMENT, "maxsim_scores_i8: one list of document ids per query");
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
  check(np_hip_maxsim_batch_i8(device, (int32_t)dim, queries, q_scales, q_tok_offsets.data(), (int32_t)B, docs, d_scales,
                               doc_tok_offsets.data(), (int64_t)n, listed ? ids.data() : nullptr, listed ? poff.data() : nullptr,
                               out.scores.data(), want_matches ? out.sims.data() : nullptr,
                               want_matches ? out.positions.data() : nullptr));
  out.scores.resize((size_t)poff[B]);
  if (want_matches) {
    out.sims.resize(rows);
    out.positions.resize(rows);
  }
  return out;
}

}  // namespace next_plaid
