// np_textmerge_plan.h -- the host side of the keyword-index merge (np_textmerge.hip) that needs no device: every check of
// np_hip_text_build_merge, the union of the two sorted vocabularies, `bound` (where a batch document falls among the old
// ids), the compaction of the strings of the terms that stay alive, and the workspace plan.  Plain C++;
// tests/cpp/textmerge_plan_check.cpp runs all of it stand-alone.
#pragma once
#include "np_text_plan.h"
#include "np_textbuild_plan.h"

namespace np {

// The batch as the checks see it: its vocabulary, its run starts and sizes.  An empty batch is all zeros / NULL.
struct TextMergeDelta {
  const uint8_t* term_bytes = nullptr;
  const int64_t* term_byte_offsets = nullptr;   // [n_terms + 1]
  int64_t n_terms = 0, n_inst = 0, n_docs = 0;
  const int64_t* inst_doc = nullptr;            // [n_inst], host copy: only the distinct documents are counted from it
};

struct TextMergePlan {
  int64_t n_remap = 0, n_a_terms = 0, n_b_terms = 0, n_union = 0, n_a = 0, n_b = 0, n_delta_docs = 0;
  int64_t n_survivors = 0;                // old documents that stay
  std::vector<uint32_t> ua, ub;           // union id of every A term / B term
  std::vector<int32_t> a_of, b_of;        // [n_union] the A term / B term of a union id, -1 = absent
  std::vector<int64_t> bound;             // [n_delta_docs] smallest old id whose survivor id is >= delta_ids[j]; n_remap = none
  int64_t workspace_bytes = 0;            // device bytes the call holds at its peak (textmerge_bytes)
};

// Device bytes of a call at its peak.  Inputs: A's three arrays and remap; keep and S per A instance; the union's four maps,
// cnt, alive, off and the alive rank per union term; delta_ids and bound; the scan's block sums; the batch's arrays where
// they have to be uploaded (upload_b).  Outputs: term_offsets (at most n_union + 1), inst_doc and inst_pos of at most
// n_a + n_b instances.  An upper bound that depends on the sizes alone, so that a call can be refused before any launch.
inline int64_t textmerge_bytes(int64_t n_a_terms, int64_t n_a, int64_t n_remap, int64_t n_b_terms, int64_t n_b, int64_t n_delta_docs,
                               int64_t n_union, bool upload_b) {
  auto up = textbuild_up256;
  int64_t t = up((n_a_terms + 1) * 8) + up(n_a * 8 + 8) + up(n_a * 4 + 4) + up(n_remap * 8 + 8);   // toff_A, doc_A, pos_A, remap
  t += 2 * up((n_a + 1) * 4);                                                                      // keep, S
  t += up(n_a_terms * 4 + 4) + up(n_b_terms * 4 + 4) + 2 * up(n_union * 4 + 4);                    // ua, ub, a_of, b_of
  t += 2 * up(n_union * 4 + 4) + up((n_union + 1) * 8) + up((n_union + 1) * 4);                    // cnt, alive, off, rank
  t += 2 * up(n_delta_docs * 8 + 8);                                                               // delta_ids, bound
  t += up(textbuild_scan_sums(std::max(n_a, n_union) + 1) * 8);                                    // block sums
  if (upload_b) t += up((n_b_terms + 1) * 8) + up(n_b * 8 + 8) + up(n_b * 4 + 4);
  t += up((n_union + 1) * 8) + up((n_a + n_b) * 8 + 8) + up((n_a + n_b) * 4 + 4);                  // the result
  return t;
}

// The vocabulary checks shared by both sides: strings that ascend strictly in term order.
inline int textmerge_check_terms(const char* side, const uint8_t* bytes, const int64_t* tbo, int64_t n_terms, char* why, size_t why_len) {
  if (n_terms == 0) return NP_OK;
  if (!tbo) return snprintf(why, why_len, "%s_term_byte_offsets is NULL", side), (int)NP_ERR_INVALID_ARGUMENT;
  if (tbo[0] != 0)
    return snprintf(why, why_len, "%s_term_byte_offsets[0] is %lld, not 0", side, (long long)tbo[0]), (int)NP_ERR_INVALID_ARGUMENT;
  for (int64_t t = 0; t < n_terms; ++t) {
    if (tbo[t + 1] <= tbo[t])
      return snprintf(why, why_len, "%s_term_byte_offsets: term %lld is empty or the offsets descend", side, (long long)t),
             (int)NP_ERR_INVALID_ARGUMENT;
    if (!bytes) return snprintf(why, why_len, "%s_term_bytes is NULL", side), (int)NP_ERR_INVALID_ARGUMENT;
    if (t > 0 && textbuild_term_cmp(bytes + tbo[t - 1], tbo[t] - tbo[t - 1], bytes + tbo[t], tbo[t + 1] - tbo[t]) >= 0)
      return snprintf(why, why_len, "%s_term_bytes: terms out of order: term %lld does not sort after term %lld", side, (long long)t,
                      (long long)(t - 1)),
             (int)NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

// Every check of np_hip_text_build_merge that needs no device, then the plan.  `why` (at least 256 bytes) names the
// argument.  NP_ERR_INVALID_ARGUMENT / NP_ERR_SHAPE / NP_ERR_OUT_OF_MEMORY (workspace_limit > 0 that does not hold the call).
inline int textmerge_plan(const np_text_index* base, const uint8_t* base_term_bytes, const int64_t* base_tbo, const int64_t* remap,
                          int64_t n_remap, const TextMergeDelta& delta, const int64_t* delta_ids, int64_t n_rows_out, bool upload_b,
                          int64_t workspace_limit, TextMergePlan* plan, char* why, size_t why_len) {
  auto bad = [](int rc) { return rc; };   // the comma expressions below end in an int
  if (n_remap < 0) return snprintf(why, why_len, "n_remap %lld is negative", (long long)n_remap), bad(NP_ERR_INVALID_ARGUMENT);
  if (n_remap > 0 && !remap) return snprintf(why, why_len, "remap is NULL"), bad(NP_ERR_INVALID_ARGUMENT);
  if (n_rows_out < 0) return snprintf(why, why_len, "n_rows_out %lld is negative", (long long)n_rows_out), bad(NP_ERR_INVALID_ARGUMENT);
  if (workspace_limit < 0)
    return snprintf(why, why_len, "opts: workspace_bytes %lld is negative", (long long)workspace_limit), bad(NP_ERR_INVALID_ARGUMENT);
  // ---- the base: np_hip_index_set_text's checks against an id space of n_remap documents, and its vocabulary
  if (!base) return snprintf(why, why_len, "base is NULL"), bad(NP_ERR_INVALID_ARGUMENT);
  if (base->n_terms >= 0 && base->n_terms <= 0x7FFFFFFF && base->n_terms > 0 && base->term_offsets && base->term_offsets[0] == 0) {
    bool asc = true;
    for (int64_t k = 0; k < base->n_terms && asc; ++k) asc = base->term_offsets[k + 1] >= base->term_offsets[k];
    if (asc && base->term_offsets[base->n_terms] > NP_TB_MAX_INSTANCES)
      return snprintf(why, why_len, "Shape error: base holds %lld instances; the limit is 2^31 - 1",
                      (long long)base->term_offsets[base->n_terms]),
             bad(NP_ERR_SHAPE);
  }
  {
    char inner[200];
    if (text_check_index(base, n_remap, inner, sizeof(inner)) != 0)
      return snprintf(why, why_len, "base: %s (the index is n_remap = %lld old documents)", inner, (long long)n_remap),
             bad(NP_ERR_INVALID_ARGUMENT);
  }
  if (const int rc = textmerge_check_terms("base", base_term_bytes, base_tbo, base->n_terms, why, why_len)) return rc;
  const int64_t n_a = base->n_terms > 0 ? base->term_offsets[base->n_terms] : 0;
  // ---- the batch
  if (delta.n_terms < 0 || delta.n_inst < 0 || delta.n_docs < 0)
    return snprintf(why, why_len, "delta: a negative count"), bad(NP_ERR_INVALID_ARGUMENT);
  if (delta.n_inst > NP_TB_MAX_INSTANCES)
    return snprintf(why, why_len, "Shape error: delta holds %lld instances; the limit is 2^31 - 1", (long long)delta.n_inst),
           bad(NP_ERR_SHAPE);
  if (const int rc = textmerge_check_terms("delta", delta.term_bytes, delta.term_byte_offsets, delta.n_terms, why, why_len)) return rc;
  if (delta.n_docs > 0 && !delta_ids) return snprintf(why, why_len, "delta_ids is NULL"), bad(NP_ERR_INVALID_ARGUMENT);
  if (delta.n_inst > 0 && !delta.inst_doc) return snprintf(why, why_len, "delta: inst_doc is NULL"), bad(NP_ERR_INVALID_ARGUMENT);
  // ---- remap: -1 or the new id; the survivors' ids ascend strictly
  int64_t last = -1, n_surv = 0;
  for (int64_t d = 0; d < n_remap; ++d) {
    const int64_t v = remap[d];
    if (v == -1) continue;
    if (v < -1) return snprintf(why, why_len, "remap[%lld] is %lld: -1 removes, an id >= 0 keeps", (long long)d, (long long)v), bad(NP_ERR_INVALID_ARGUMENT);
    if (v <= last)
      return snprintf(why, why_len, "remap[%lld] is %lld after %lld: the survivors' ids must ascend strictly", (long long)d, (long long)v,
                      (long long)last),
             bad(NP_ERR_INVALID_ARGUMENT);
    last = v;
    ++n_surv;
  }
  // ---- delta_ids: ascending strictly, none a survivor's id; bound[j] out of one linear walk over the survivors
  plan->bound.assign((size_t)delta.n_docs, n_remap);
  {
    int64_t d = 0;   // the first old document at or after the walk whose survivor id is >= the current delta id
    for (int64_t j = 0; j < delta.n_docs; ++j) {
      const int64_t id = delta_ids[j];
      if (id < 0) return snprintf(why, why_len, "delta_ids[%lld] is %lld, a negative id", (long long)j, (long long)id), bad(NP_ERR_INVALID_ARGUMENT);
      if (j > 0 && id <= delta_ids[j - 1])
        return snprintf(why, why_len, "delta_ids[%lld] is %lld after %lld: the ids must ascend strictly", (long long)j, (long long)id,
                        (long long)delta_ids[j - 1]),
               bad(NP_ERR_INVALID_ARGUMENT);
      while (d < n_remap && remap[d] < id) ++d;   // -1 < id too: holes are skipped
      if (d < n_remap && remap[d] == id)
        return snprintf(why, why_len, "delta_ids[%lld] is %lld, the id that remap[%lld] keeps", (long long)j, (long long)id, (long long)d),
               bad(NP_ERR_INVALID_ARGUMENT);
      plan->bound[(size_t)j] = d;
    }
  }
  // ---- sizes
  if (n_a + delta.n_inst > NP_TB_MAX_INSTANCES)
    return snprintf(why, why_len, "Shape error: the result may hold %lld instances; the limit is 2^31 - 1", (long long)(n_a + delta.n_inst)),
           bad(NP_ERR_SHAPE);
  // ---- n_rows_out against the documents of the result that hold a token.  The batch's documents are walked in any case
  // (the device indexes delta_ids with them); the base's only where n_rows_out is below the survivors plus the batch,
  // which no table with one row per document is
  {
    std::vector<bool> seen_b((size_t)delta.n_docs, false);
    int64_t distinct = 0;
    for (int64_t k = 0; k < delta.n_inst; ++k) {
      const int64_t d = delta.inst_doc[k];
      if (d < 0 || d >= delta.n_docs)
        return snprintf(why, why_len, "delta: instance %lld names document %lld of %lld", (long long)k, (long long)d, (long long)delta.n_docs),
               bad(NP_ERR_INVALID_ARGUMENT);
      if (!seen_b[(size_t)d]) seen_b[(size_t)d] = true, ++distinct;
    }
    if (n_rows_out < n_surv + delta.n_docs) {
      std::vector<bool> seen((size_t)n_remap, false);
      for (int64_t i = 0; i < n_a; ++i) {
        const int64_t d = base->inst_doc[i];
        if (remap[d] >= 0 && !seen[(size_t)d]) seen[(size_t)d] = true, ++distinct;
      }
      if (n_rows_out < distinct)
        return snprintf(why, why_len, "n_rows_out %lld is below the %lld documents of the result that hold a token", (long long)n_rows_out,
                        (long long)distinct),
               bad(NP_ERR_INVALID_ARGUMENT);
    }
  }
  // ---- the union of the two vocabularies, one linear walk
  plan->ua.assign((size_t)base->n_terms, 0);
  plan->ub.assign((size_t)delta.n_terms, 0);
  plan->a_of.clear();
  plan->b_of.clear();
  int64_t i = 0, j = 0;
  while (i < base->n_terms || j < delta.n_terms) {
    int c;
    if (i >= base->n_terms) c = 1;
    else if (j >= delta.n_terms) c = -1;
    else
      c = textbuild_term_cmp(base_term_bytes + base_tbo[i], base_tbo[i + 1] - base_tbo[i], delta.term_bytes + delta.term_byte_offsets[j],
                             delta.term_byte_offsets[j + 1] - delta.term_byte_offsets[j]);
    const uint32_t u = (uint32_t)plan->a_of.size();
    plan->a_of.push_back(c <= 0 ? (int32_t)i : -1);
    plan->b_of.push_back(c >= 0 ? (int32_t)j : -1);
    if (c <= 0) plan->ua[(size_t)i++] = u;
    if (c >= 0) plan->ub[(size_t)j++] = u;
  }
  plan->n_remap = n_remap;
  plan->n_a_terms = base->n_terms;
  plan->n_b_terms = delta.n_terms;
  plan->n_union = (int64_t)plan->a_of.size();
  plan->n_a = n_a;
  plan->n_b = delta.n_inst;
  plan->n_delta_docs = delta.n_docs;
  plan->n_survivors = n_surv;
  plan->workspace_bytes =
      textmerge_bytes(plan->n_a_terms, n_a, n_remap, plan->n_b_terms, plan->n_b, plan->n_delta_docs, plan->n_union, upload_b);
  if (workspace_limit > 0 && plan->workspace_bytes > workspace_limit)
    return snprintf(why, why_len, "opts: the workspace of %lld bytes does not hold the call: it needs %lld", (long long)workspace_limit,
                    (long long)plan->workspace_bytes),
           bad(NP_ERR_OUT_OF_MEMORY);
  return NP_OK;
}

// The strings of the union's alive terms, in order: from A where the term is A's, otherwise from B.
inline void textmerge_compact_terms(const TextMergePlan& plan, const uint32_t* alive, const uint8_t* a_bytes, const int64_t* a_tbo,
                                    const uint8_t* b_bytes, const int64_t* b_tbo, std::vector<uint8_t>* out_bytes,
                                    std::vector<int64_t>* out_tbo) {
  out_bytes->clear();
  out_tbo->assign(1, 0);
  for (int64_t u = 0; u < plan.n_union; ++u) {
    if (!alive[u]) continue;
    const int32_t a = plan.a_of[(size_t)u], b = plan.b_of[(size_t)u];
    if (a >= 0) out_bytes->insert(out_bytes->end(), a_bytes + a_tbo[a], a_bytes + a_tbo[a + 1]);
    else out_bytes->insert(out_bytes->end(), b_bytes + b_tbo[b], b_bytes + b_tbo[b + 1]);
    out_tbo->push_back((int64_t)out_bytes->size());
  }
}

}  // namespace np
