// np_text_plan.h -- the host side of the keyword index and the keyword search that needs no device: the checks of a keyword
// index (np_hip_index_set_text refuses a malformed one before any allocation), of a query and of a call (refused before any
// launch), the idf, and the plan of query chunks and document-slice chunks under a byte budget.  Plain C++;
// tests/cpp/text_plan_check.cpp runs all of it stand-alone.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../include/nextplaid_hip.h"

namespace np {

// documents per slice of the scoring kernel: one f64 accumulator (32 KB), one match count (4 KB) and one sort index (8 KB)
// per document of the slice in LDS -- 45 KB with the phrase ranges, three workgroups per CU of 160 KB
constexpr int64_t NP_TEXT_SLICE_DOCS = 4096;

// workgroups (of 256 lanes) per phrase of the counting pass at most: a first posting list longer than 256 times this many
// entries is walked in several grid strides
constexpr int64_t NP_TEXT_HIT_BLOCKS = 512;

// entries a slice hands to the merge: no slice holds more than its documents
inline int64_t text_slice_keep(int32_t top_k) { return top_k < NP_TEXT_SLICE_DOCS ? top_k : NP_TEXT_SLICE_DOCS; }

// The index against a handle of n_docs documents.  0 = well-formed; otherwise NP_ERR_INVALID_ARGUMENT with `why` naming the
// first offender.  *n_distinct (nullable) = documents that hold a token.
inline int text_check_index(const np_text_index* t, int64_t n_docs, char* why, size_t why_len, int64_t* n_distinct = nullptr) {
  auto fail = [&](const char* what, long long a, long long b) {
    snprintf(why, why_len, what, a, b);
    return (int)NP_ERR_INVALID_ARGUMENT;
  };
  if (!t) return fail("NULL text index", 0, 0);
  if (t->n_terms < 0) return fail("n_terms = %lld is negative", t->n_terms, 0);
  if (t->n_rows < 0) return fail("n_rows = %lld is negative", t->n_rows, 0);
  if (t->n_terms > 0x7FFFFFFF) return fail("n_terms = %lld does not fit an i32 term id", t->n_terms, 0);
  if (t->n_terms > 0 && !t->term_offsets) return fail("n_terms = %lld but term_offsets is NULL", t->n_terms, 0);
  if (t->n_terms == 0) {
    if (n_distinct) *n_distinct = 0;
    return 0;
  }
  if (t->term_offsets[0] != 0) return fail("term_offsets[0] = %lld must be 0", t->term_offsets[0], 0);
  for (int64_t k = 0; k < t->n_terms; ++k)
    if (t->term_offsets[k + 1] < t->term_offsets[k]) return fail("term_offsets decrease at term %lld", k, 0);
  const int64_t n_inst = t->term_offsets[t->n_terms];
  if (n_inst > 0 && (!t->inst_doc || !t->inst_pos)) return fail("%lld instances but inst_doc or inst_pos is NULL", n_inst, 0);
  std::vector<bool> seen((size_t)(n_docs > 0 ? n_docs : 0), false);
  int64_t distinct = 0;
  for (int64_t k = 0; k < t->n_terms; ++k)
    for (int64_t i = t->term_offsets[k]; i < t->term_offsets[k + 1]; ++i) {
      const int64_t d = t->inst_doc[i];
      if (d < 0 || d >= n_docs) return fail("instance %lld: document %lld is outside the index", i, d);
      if (t->inst_pos[i] < 0) return fail("instance %lld: position %lld is negative", i, t->inst_pos[i]);
      if (i > t->term_offsets[k]) {
        const int64_t pd = t->inst_doc[i - 1];
        if (pd > d || (pd == d && t->inst_pos[i - 1] >= t->inst_pos[i]))
          return fail("instance %lld of term %lld is not after its predecessor in (document, position) order", i, k);
      }
      if (!seen[(size_t)d]) {
        seen[(size_t)d] = true;
        ++distinct;
      }
    }
  if (t->n_rows < distinct) return fail("n_rows = %lld is below the %lld documents that hold a token", t->n_rows, distinct);
  if (n_distinct) *n_distinct = distinct;
  return 0;
}

// One query against a vocabulary of n_terms.  `q` only labels the message.
inline int text_check_query(const np_text_query* tq, int32_t q, int64_t n_terms, char* why, size_t why_len) {
  auto fail = [&](const char* what, long long a) {
    char msg[160];
    snprintf(msg, sizeof msg, what, a);
    snprintf(why, why_len, "text query %d: %s", q, msg);
    return (int)NP_ERR_INVALID_ARGUMENT;
  };
  if (!tq) return fail("NULL query", 0);
  if (tq->n_phrases < 1 || tq->n_phrases > NP_TEXT_MAX_PHRASES) return fail("n_phrases = %lld must be in 1..64", tq->n_phrases);
  if (tq->mode != NP_TEXT_AND && tq->mode != NP_TEXT_OR) return fail("unknown mode %lld", tq->mode);
  if (!tq->phrase_offsets || !tq->terms) return fail("NULL phrase_offsets or terms", 0);
  if (tq->phrase_offsets[0] != 0) return fail("phrase_offsets[0] = %lld must be 0", tq->phrase_offsets[0]);
  for (int32_t p = 0; p < tq->n_phrases; ++p) {
    if (tq->phrase_offsets[p + 1] <= tq->phrase_offsets[p]) return fail("phrase %lld has no token", p);
    if (tq->phrase_offsets[p + 1] > NP_TEXT_MAX_TOKENS) return fail("more than 256 tokens (at phrase %lld)", p);
  }
  for (int32_t i = 0; i < tq->phrase_offsets[tq->n_phrases]; ++i)
    if (tq->terms[i] < -1 || (int64_t)tq->terms[i] >= n_terms) return fail("token %lld names no term of the vocabulary", i);
  return 0;
}

// One tree query (np_text_expr) against a vocabulary of n_terms: the phrases as text_check_query checks them, the prefix
// ranges, and the postfix node list -- stack discipline, children below their parent, every phrase named exactly once, one
// node left at the end.  `q` only labels the message.
inline int text_check_expr(const np_text_expr* te, int32_t q, int64_t n_terms, char* why, size_t why_len) {
  auto fail = [&](const char* what, long long a, long long b = 0) {
    char msg[200];
    snprintf(msg, sizeof msg, what, a, b);
    snprintf(why, why_len, "text query %d: %s", q, msg);
    return (int)NP_ERR_INVALID_ARGUMENT;
  };
  if (!te) return fail("NULL query", 0);
  if (te->n_phrases < 1 || te->n_phrases > NP_TEXT_MAX_PHRASES) return fail("n_phrases = %lld must be in 1..64", te->n_phrases);
  if (te->n_nodes < 1 || te->n_nodes > NP_TEXT_MAX_NODES) return fail("n_nodes = %lld must be in 1..127", te->n_nodes);
  if (!te->phrase_offsets || !te->terms || !te->prefix_hi || !te->nodes) return fail("NULL phrase_offsets, terms, prefix_hi or nodes", 0);
  if (te->phrase_offsets[0] != 0) return fail("phrase_offsets[0] = %lld must be 0", te->phrase_offsets[0]);
  for (int32_t p = 0; p < te->n_phrases; ++p) {
    if (te->phrase_offsets[p + 1] <= te->phrase_offsets[p]) return fail("phrase %lld has no token", p);
    if (te->phrase_offsets[p + 1] > NP_TEXT_MAX_TOKENS) return fail("more than 256 tokens (at phrase %lld)", p);
  }
  for (int32_t i = 0; i < te->phrase_offsets[te->n_phrases]; ++i)
    if (te->terms[i] < -1 || (int64_t)te->terms[i] >= n_terms) return fail("token %lld names no term of the vocabulary", i);
  for (int32_t p = 0; p < te->n_phrases; ++p) {
    const int64_t hi = te->prefix_hi[p];
    if (hi == 0) continue;
    const int32_t nt = te->phrase_offsets[p + 1] - te->phrase_offsets[p];
    const int64_t lo = te->terms[te->phrase_offsets[p + 1] - 1];
    if (lo < 0) return fail("phrase %lld: a prefix range needs a known last token to start at", p);
    if (hi <= lo || hi > n_terms) return fail("phrase %lld: the prefix range ends at %lld, outside the vocabulary or not after its start", p, hi);
    if (nt > 1 && hi - lo > NP_TEXT_MAX_PREFIX_TERMS)
      return fail("phrase %lld of several tokens ends in a prefix of %lld terms, more than NP_TEXT_MAX_PREFIX_TERMS = 1024", p, hi - lo);
  }
  uint64_t used = 0;
  int32_t stack[NP_TEXT_MAX_NODES];
  int32_t depth = 0;
  for (int32_t n = 0; n < te->n_nodes; ++n) {
    const np_text_node& nd = te->nodes[n];
    if (nd.op == NP_TEXT_NODE_PHRASE) {
      if (nd.a < 0 || nd.a >= te->n_phrases) return fail("node %lld names phrase %lld, which the query does not have", n, nd.a);
      if ((used >> nd.a) & 1) return fail("node %lld names phrase %lld a second time", n, nd.a);
      used |= (uint64_t)1 << nd.a;
    } else if (nd.op == NP_TEXT_NODE_AND || nd.op == NP_TEXT_NODE_OR || nd.op == NP_TEXT_NODE_NOT) {
      if (depth < 2) return fail("node %lld: the stack holds %lld nodes, an operator needs two", n, depth);
      if (nd.a < 0 || nd.a >= n || nd.b < 0 || nd.b >= n) return fail("node %lld: a child index is not below the node's own", n);
      if (stack[depth - 1] != nd.b || stack[depth - 2] != nd.a)
        return fail("node %lld: its children are not the two nodes on top of the stack (%lld below the top)", n, stack[depth - 2]);
      depth -= 2;
    } else {
      return fail("node %lld: unknown op %lld", n, nd.op);
    }
    stack[depth++] = n;
  }
  if (depth != 1) return fail("%lld nodes are left on the stack at the end, not one", depth);
  for (int32_t p = 0; p < te->n_phrases; ++p)
    if (!((used >> p) & 1)) return fail("phrase %lld is named by no node", p);
  return 0;
}

// The phrases of a batch of tree queries whose nHit crosses the ranks of a sharded call, in the order of the count vector: first
// the phrases of several tokens, all known (their last token may be a prefix range), in query and phrase order, then the
// single-token prefix phrases, likewise.  Follows from the queries alone (which have passed text_check_expr: a prefix range
// starts at a known term and is not empty), so every rank runs the same counting exchange of the same size.  An exact single
// token is not counted: its document frequency is the table's on every shard.  *n_multi, *n_prefix: nullable.
inline int64_t text_counted_expr_phrases(const np_text_expr* queries, int32_t B, int64_t* n_multi = nullptr, int64_t* n_prefix = nullptr) {
  int64_t multi = 0, prefix = 0;
  for (int32_t q = 0; q < B; ++q)
    for (int32_t i = 0; i < queries[q].n_phrases; ++i) {
      const int32_t tb = queries[q].phrase_offsets[i], te = queries[q].phrase_offsets[i + 1];
      bool known = true;
      for (int32_t k = tb; k < te; ++k) known = known && queries[q].terms[k] >= 0;
      if (!known) continue;
      if (te - tb > 1) ++multi;
      else if (queries[q].prefix_hi[i] != 0) ++prefix;
    }
  if (n_multi) *n_multi = multi;
  if (n_prefix) *n_prefix = prefix;
  return multi + prefix;
}

// The counting pre-pass of a sharded tree batch marks a prefix phrase's documents in a bitmap of one bit per document, padded
// to whole 256-byte lines; the phrases are counted in groups of as many bitmaps as `scratch` bytes hold, at most 65535 (the
// group is a grid dimension).  How a rank groups is its own business: only the complete count vector leaves the pre-pass.
inline int64_t text_prefix_bitmap_bytes(int64_t n_docs) {
  const int64_t bits = n_docs < 1 ? 1 : n_docs;
  return (bits + 2047) / 2048 * 256;
}
// phrases per group: 0 = not even one bitmap fits
inline int64_t text_prefix_group(int64_t scratch, int64_t n_docs, int64_t n_prefix) {
  int64_t g = scratch > 0 ? scratch / text_prefix_bitmap_bytes(n_docs) : 0;
  if (g > 65535) g = 65535;
  if (g > n_prefix) g = n_prefix;
  return g < 0 ? 0 : g;
}

// B and top_k of a keyword search.  *why = a string literal.
inline int text_check_call(int32_t B, int32_t top_k, const char** why) {
  *why = "";
  if (B < 0) return *why = "negative batch size", (int)NP_ERR_INVALID_ARGUMENT;
  if (B >= 65536) return *why = "more than 65535 queries in one call", (int)NP_ERR_INVALID_ARGUMENT;
  if (top_k < 1 || top_k > NP_TEXT_MAX_TOPK) return *why = "top_k must be in 1..1024", (int)NP_ERR_INVALID_ARGUMENT;
  return 0;
}

// the arguments of a fusion that the host can see
inline int fuse_check_call(int32_t mode, float alpha, int32_t top_k, int32_t B, int32_t sem_stride, int32_t kw_stride,
                           const char** why) {
  *why = "";
  if (mode != NP_FUSE_RRF && mode != NP_FUSE_RELATIVE_SCORE) return *why = "unknown fusion mode", (int)NP_ERR_INVALID_ARGUMENT;
  if (!(alpha >= 0.0f && alpha <= 1.0f)) return *why = "alpha must be in [0, 1]", (int)NP_ERR_INVALID_ARGUMENT;
  if (B < 0) return *why = "negative batch size", (int)NP_ERR_INVALID_ARGUMENT;
  if (top_k < 1 || top_k > 2 * NP_TEXT_MAX_TOPK) return *why = "top_k must be in 1..2048", (int)NP_ERR_INVALID_ARGUMENT;
  if (sem_stride < 0 || sem_stride > NP_TEXT_MAX_TOPK || kw_stride < 0 || kw_stride > NP_TEXT_MAX_TOPK)
    return *why = "a list stride must be in 0..1024", (int)NP_ERR_INVALID_ARGUMENT;
  return 0;
}

// bm25's idf as SQLite computes it (fts5_aux.c): libm's log in f64, clamped to 1e-6 where it is not positive
inline double text_idf(int64_t n_rows, int64_t n_hit) {
  const double idf = log(((double)(n_rows - n_hit) + 0.5) / ((double)n_hit + 0.5));
  return idf <= 0.0 ? 1e-6 : idf;
}

// Chunks: `queries` queries over `slices` document slices at a time, so that
//     queries * per_query + queries * slices * (keep * 12 + 4) + fixed  <=  budget        (keep = text_slice_keep(top_k)).
// queries starts at min(B, max_batch) and halves while a chunk could not hold min(n_slices, 8) slices; slices is then what
// the rest of the budget holds, at most n_slices.  false: one query over one slice does not fit.
struct TextPlan {
  int32_t queries = 1;
  int64_t slices = 1;
};
inline int64_t text_pair_bytes(int32_t top_k) { return text_slice_keep(top_k) * 12 + 4; }
inline bool text_plan(int64_t budget, int64_t fixed, int64_t per_query, int64_t n_slices, int32_t B, int32_t max_batch,
                      int32_t top_k, TextPlan* out) {
  if (n_slices < 1) n_slices = 1;
  int64_t Q = B < 1 ? 1 : B;
  if (max_batch >= 1 && Q > max_batch) Q = max_batch;
  const int64_t want = n_slices < 8 ? n_slices : 8;
  for (;;) {
    const int64_t left = budget - fixed - Q * per_query;
    const int64_t S = left > 0 ? left / (Q * text_pair_bytes(top_k)) : 0;
    if (S >= want || Q == 1) {
      if (S < 1) return false;
      out->queries = (int32_t)Q;
      out->slices = S < n_slices ? S : n_slices;
      return true;
    }
    Q = (Q + 1) / 2;
  }
}

}  // namespace np
