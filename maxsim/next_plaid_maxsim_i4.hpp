// next_plaid_maxsim_i4.hpp -- the C++ host mirror of the int4 form of batched MaxSim: quantize_rows_i4
// (np_hip_quantize_rows_i4) and maxsim_scores_i4 (np_hip_maxsim_batch_i4), beside maxsim_scores_i8 of
// next_plaid_maxsim_i8.hpp, whose argument conventions they keep.  Host-only; the library refuses what it does not take and
// `check` throws.
#pragma once
#include "next_plaid_maxsim_i8.hpp"

namespace next_plaid {

// rows [n_rows][dim] f32 -> ceil(dim / 8) words of two's-complement nibbles per row (nibble j of word w: the code of
// x[8 w + j], clamp(rint(x * (7 / max|x|)), -7, 7); pad nibbles 0) and one f32 scale per row, max|x| / 7; a row with a
// non-finite element gets scale NaN and codes 0.
struct Int4Rows {
  std::vector<uint32_t> words;   // [n_rows][ceil(dim / 8)]
  std::vector<float> scales;     // [n_rows]
};
inline Int4Rows quantize_rows_i4(const float* rows, size_t n_rows, size_t dim, int device = 0) {
  const size_t W = (dim + 7) / 8;
  Int4Rows out;
  out.words.assign(std::max<size_t>(n_rows * W, 1), 0u);
  out.scales.assign(std::max<size_t>(n_rows, 1), 0.f);
  check(np_hip_quantize_rows_i4(device, NP_DT_F32, (int32_t)dim, rows, (int64_t)n_rows, out.words.data(), out.scales.data()));
  out.words.resize(n_rows * W);
  out.scales.resize(n_rows);
  return out;
}

// MaxSim of int8 query rows against int4 document rows, one f32 scale per row on both sides.  queries: flat [tokens][dim]
// codes; doc_words: flat [tokens][ceil(dim / 8)] words; `pairs` and want_matches as maxsim_scores_i8.
inline MaxsimScores maxsim_scores_i4(const int8_t* queries, const float* q_scales, const std::vector<int32_t>& q_tok_offsets,
                                     const uint32_t* doc_words, const float* d_scales, const std::vector<int64_t>& doc_tok_offsets,
                                     size_t dim, const std::vector<std::vector<int64_t>>& pairs = {}, bool want_matches = false,
                                     int device = 0) {
  const size_t B = q_tok_offsets.empty() ? 0 : q_tok_offsets.size() - 1;
  const size_t n = doc_tok_offsets.empty() ? 0 : doc_tok_offsets.size() - 1;
  const bool listed = !pairs.empty();
  if (listed && pairs.size() != B) throw Error(NP_ERR_INVALID_ARGUMENT, "maxsim_scores_i4: one list of document ids per query");
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
  check(np_hip_maxsim_batch_i4(device, (int32_t)dim, queries, q_scales, q_tok_offsets.data(), (int32_t)B, doc_words, d_scales,
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
