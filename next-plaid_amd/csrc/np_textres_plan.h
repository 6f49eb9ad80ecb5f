// np_textres_plan.h -- the host side of the resident keyword index (np_textres.hip) that needs no device: the sizes and the
// peak device bytes of np_hip_index_set_text_build (a build installed as the handle's keyword index) and of
// np_hip_index_text_merge (np_hip_text_build_merge whose base is the handle's keyword index), their refusals, and the message
// of the device check's first offender.  Plain C++; tests/cpp/textres_plan_check.cpp runs all of it stand-alone.
#pragma once
#include "np_textmerge_plan.h"

#if defined(__HIPCC__)
#define NP_TEXTRES_HD __host__ __device__
#else
#define NP_TEXTRES_HD
#endif

namespace np {

// instances a block of the check / heads launch covers: the scan's chunk, so that one grid serves both
constexpr int64_t NP_TR_CHUNK = NP_TB_SCAN_CHUNK;
inline int64_t textres_blocks(int64_t n_inst) { return (n_inst + NP_TR_CHUNK - 1) / NP_TR_CHUNK; }

// ---- np_hip_index_set_text_build ------------------------------------------------------------------------------------------
// Device bytes the install holds at its peak, a function of the sizes alone.  The build's three arrays (uploaded: allocated by
// the call, otherwise the build's own, which the call is handed); the flags (term starts, then heads, then "document holds a
// token") and their exclusive scan, each over max(n_inst, n_docs) + 1 entries; the scan's block sums; the lowest offender per
// block; the new index with as many postings as instances, which no table exceeds.
inline int64_t textres_install_bytes(int64_t n_terms, int64_t n_inst, int64_t n_docs) {
  auto up = textbuild_up256;
  const int64_t m = std::max(n_inst, n_docs) + 1;
  int64_t t = up((n_terms + 1) * 8) + up(n_inst * 8 + 8) + up(n_inst * 4 + 4);   // term_offsets, inst_doc, inst_pos
  t += 2 * up(m * 4);                                                            // flags, their scan
  t += up(textbuild_scan_sums(m) * 8);                                           // block sums
  t += up((textres_blocks(n_inst) + 1) * 8);                                     // lowest offender per block
  t += up((n_terms + 1) * 8) + 2 * up(n_inst * 4 + 4) + up(n_inst * 8 + 8);      // post_off, post_doc, post_tf, post_first
  t += up(std::max<int64_t>(n_docs, 1) * 4);                                     // doc_len (pos is inst_pos, counted above)
  return t;
}

// What the install knows of a build and a handle before any launch.
struct TextResInstall {
  bool build_null = false, index_null = false;
  bool finalised = false, consumed = false;
  int build_device = 0, index_device = 0;
  int shard_count = 1;
  int64_t n_terms = 0, n_inst = 0, n_rows = 0, n_docs = 0;
};

// The refusals of np_hip_index_set_text_build that need no device, each naming its argument.
inline int textres_check_install(const TextResInstall& a, char* why, size_t why_len) {
  auto bad = [](int rc) { return rc; };
  if (a.index_null) return snprintf(why, why_len, "index is NULL"), bad(NP_ERR_INVALID_ARGUMENT);
  if (a.build_null) return snprintf(why, why_len, "build is NULL"), bad(NP_ERR_INVALID_ARGUMENT);
  if (a.shard_count > 1)
    return snprintf(why, why_len,
                    "index is a shard (opened with shard_count = %d): a slice needs the whole table's document frequencies "
                    "(np_hip_index_set_text_shard)",
                    a.shard_count),
           bad(NP_ERR_INVALID_ARGUMENT);
  if (a.consumed)
    return snprintf(why, why_len, "build is consumed: it was installed before and its instance arrays belong to that handle"),
           bad(NP_ERR_INVALID_ARGUMENT);
  if (!a.finalised)
    return snprintf(why, why_len, "build is not finalised: call np_hip_text_build_sizes on it first"), bad(NP_ERR_INVALID_ARGUMENT);
  if (a.build_device != a.index_device)
    return snprintf(why, why_len, "build was built on device %d, the index lies on device %d", a.build_device, a.index_device),
           bad(NP_ERR_INVALID_ARGUMENT);
  if (a.n_terms < 0 || a.n_inst < 0 || a.n_rows < 0 || a.n_docs < 0)
    return snprintf(why, why_len, "build: a negative count"), bad(NP_ERR_INVALID_ARGUMENT);
  if (a.n_terms > 0x7FFFFFFF)
    return snprintf(why, why_len, "build: n_terms = %lld does not fit an i32 term id", (long long)a.n_terms), bad(NP_ERR_INVALID_ARGUMENT);
  if (a.n_inst > NP_TB_MAX_INSTANCES)
    return snprintf(why, why_len, "Shape error: build holds %lld instances; the limit is 2^31 - 1", (long long)a.n_inst), bad(NP_ERR_SHAPE);
  return NP_OK;
}

// The rules of the device check, in text_check_index's order; 0 = the instance passes.
enum { NP_TR_RULE_DOC = 1, NP_TR_RULE_POS = 2, NP_TR_RULE_ORDER = 3 };

// The verdict on instance i, as the kernel and the host both compute it: first = i starts its term; (pd, pp) is its
// predecessor where it has one.
NP_TEXTRES_HD static inline int textres_rule(int64_t d, int32_t p, bool first, int64_t pd, int32_t pp, int64_t n_docs) {
  if (d < 0 || d >= n_docs) return NP_TR_RULE_DOC;
  if (p < 0) return NP_TR_RULE_POS;
  if (!first && (pd > d || (pd == d && pp >= p))) return NP_TR_RULE_ORDER;
  return 0;
}

// The message for the lowest offending instance, in np_hip_index_set_text's words.
inline void textres_offender_message(int rule, int64_t inst, int64_t term, int64_t doc, int32_t pos, char* why, size_t why_len) {
  if (rule == NP_TR_RULE_DOC)
    snprintf(why, why_len, "build: instance %lld: document %lld is outside the index", (long long)inst, (long long)doc);
  else if (rule == NP_TR_RULE_POS)
    snprintf(why, why_len, "build: instance %lld: position %lld is negative", (long long)inst, (long long)pos);
  else
    snprintf(why, why_len, "build: instance %lld of term %lld is not after its predecessor in (document, position) order",
             (long long)inst, (long long)term);
}

// ---- np_hip_index_text_merge ----------------------------------------------------------------------------------------------
// The base's term_offsets and inst_doc are MATERIALISED from the postings by one expanding launch and the merge's kernels run
// unchanged; pos_A is the handle's pos, read where it lies.  Against kernels that read the postings through an accessor this
// holds 8 bytes per base instance more for the length of the call -- what the host merge holds for its uploaded inst_doc, and
// 4 bytes per instance LESS than that merge, which uploads pos_A too -- and keeps the placing kernels' binary searches over a
// run of A at one read per step instead of a bisection of post_first per step.
//
// Device bytes at the peak: np_hip_text_build_merge's (textmerge_bytes) without pos_A, plus the flags "survivor that holds a
// token" and their scan over the handle's documents (only where n_rows_out is below survivors plus batch; planned always).
inline int64_t textres_merge_bytes(int64_t n_a_terms, int64_t n_a, int64_t n_remap, int64_t n_b_terms, int64_t n_b, int64_t n_delta_docs,
                                   int64_t n_union, bool upload_b, int64_t n_docs) {
  auto up = textbuild_up256;
  int64_t t = textmerge_bytes(n_a_terms, n_a, n_remap, n_b_terms, n_b, n_delta_docs, n_union, upload_b) - up(n_a * 4 + 4);
  t += 2 * up((n_docs + 1) * 4) + up(textbuild_scan_sums(n_docs + 1) * 8);
  return t;
}

// What the merge knows of the handle's keyword index before any launch.
struct TextResBase {
  bool index_null = false, present = false;
  int shard_count = 1;
  int64_t n_terms = 0, n_inst = 0, n_docs = 0;
};

// Every check of np_hip_index_text_merge that needs no device, then the plan: np_hip_text_build_merge's own (textmerge_plan,
// over a base of the handle's n_terms terms whose instances stay where they are -- they were checked when they were
// installed), the handle's, and the sizes with the handle's instances counted in.  *need_distinct = n_rows_out is below the
// survivors plus the batch, so the survivors that hold a token have to be counted on the device.  base_tbo must describe
// exactly the handle's n_terms strings: a pointer has no length, so that check is the host mirrors', which hold the array.
// Where n_remap is below the handle's documents, the documents behind it must hold no token: counted on the device too.
inline int textres_merge_plan(const TextResBase& base, const uint8_t* base_term_bytes, const int64_t* base_tbo,
                              const int64_t* remap, int64_t n_remap, const TextMergeDelta& delta, const int64_t* delta_ids,
                              int64_t n_rows_out, bool upload_b, int64_t workspace_limit, TextMergePlan* plan, bool* need_distinct,
                              char* why, size_t why_len) {
  auto bad = [](int rc) { return rc; };
  if (base.index_null) return snprintf(why, why_len, "index is NULL"), bad(NP_ERR_INVALID_ARGUMENT);
  if (base.shard_count > 1)
    return snprintf(why, why_len, "index is a shard (opened with shard_count = %d): a slice does not hold the whole table", base.shard_count),
           bad(NP_ERR_INVALID_ARGUMENT);
  if (!base.present)
    return snprintf(why, why_len, "index has no keyword index (np_hip_index_set_text, np_hip_index_set_text_build)"),
           bad(NP_ERR_INVALID_ARGUMENT);
  if (base.n_inst > NP_TB_MAX_INSTANCES)
    return snprintf(why, why_len, "Shape error: base holds %lld instances; the limit is 2^31 - 1", (long long)base.n_inst), bad(NP_ERR_SHAPE);
  // the vocabulary, remap, delta_ids, bound, the batch and the union: the existing plan over a base without instances
  std::vector<int64_t> zeros((size_t)base.n_terms + 1, 0);
  np_text_index hollow;
  memset(&hollow, 0, sizeof(hollow));
  hollow.n_terms = base.n_terms;
  hollow.term_offsets = zeros.data();
  hollow.n_rows = 0;
  if (const int rc = textmerge_plan(&hollow, base_term_bytes, base_tbo, remap, n_remap, delta, delta_ids, n_rows_out, upload_b, 0, plan, why,
                                    why_len))
    return rc;
  if (workspace_limit < 0)
    return snprintf(why, why_len, "opts: workspace_bytes %lld is negative", (long long)workspace_limit), bad(NP_ERR_INVALID_ARGUMENT);
  if (base.n_inst + delta.n_inst > NP_TB_MAX_INSTANCES)
    return snprintf(why, why_len, "Shape error: the result may hold %lld instances; the limit is 2^31 - 1",
                    (long long)(base.n_inst + delta.n_inst)),
           bad(NP_ERR_SHAPE);
  plan->n_a = base.n_inst;
  plan->workspace_bytes = textres_merge_bytes(plan->n_a_terms, plan->n_a, n_remap, plan->n_b_terms, plan->n_b, plan->n_delta_docs,
                                              plan->n_union, upload_b, base.n_docs);
  *need_distinct = n_rows_out < plan->n_survivors + delta.n_docs;
  if (workspace_limit > 0 && plan->workspace_bytes > workspace_limit)
    return snprintf(why, why_len, "opts: the workspace of %lld bytes does not hold the call: it needs %lld", (long long)workspace_limit,
                    (long long)plan->workspace_bytes),
           bad(NP_ERR_OUT_OF_MEMORY);
  return NP_OK;
}

}  // namespace np
