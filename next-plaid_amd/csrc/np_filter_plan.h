// np_filter_plan.h -- the host side of the metadata filters that needs no device: the checks of a postfix program
// (np_hip_filter_eval and the filtered searches refuse a malformed one before any launch) and the plan of document and filter
// chunks under a byte budget.  Plain C++; tests/cpp/filter_plan_check.cpp runs all of it stand-alone.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/nextplaid_hip.h"
#include "np_match_plan.h"

namespace np {

// documents per compaction block: 256 lanes, one 64-document ballot word each.  Chunks of documents start at multiples of it.
constexpr int64_t NP_FILTER_BLOCK_DOCS = 256 * 64;

static inline double filter_f64_of(int64_t bits) {
  double d;
  memcpy(&d, &bits, 8);
  return d;
}

// One program against the column types of a handle (n_cols of them).  0 = well-formed; otherwise NP_ERR_INVALID_ARGUMENT with
// `why` (at least 160 bytes) naming the op.  `filter` only labels the message.
inline int filter_check_program(const np_filter* f, int32_t filter, const int32_t* col_types, int32_t n_cols, char* why,
                                size_t why_len) {
  auto fail = [&](int op, const char* what) {
    if (op >= 0)
      snprintf(why, why_len, "filter %d, op %d: %s", filter, op, what);
    else
      snprintf(why, why_len, "filter %d: %s", filter, what);
    return (int)NP_ERR_INVALID_ARGUMENT;
  };
  if (!f) return fail(-1, "NULL filter");
  if (f->n_ops < 1 || f->n_ops > NP_FILTER_MAX_OPS) return fail(-1, "n_ops must be in 1..256");
  if (!f->ops) return fail(-1, "NULL ops");
  if (f->n_values < 0 || f->n_values > NP_FILTER_MAX_VALUES) return fail(-1, "n_values must be in 0..2^20");
  if (f->n_values > 0 && !f->values) return fail(-1, "NULL values");
  int depth = 0;
  for (int i = 0; i < f->n_ops; ++i) {
    const np_filter_op& o = f->ops[i];
    const bool leaf = o.op == NP_F_CMP || o.op == NP_F_BETWEEN || o.op == NP_F_IN || o.op == NP_F_IS_NULL;
    if (leaf) {
      if (o.column < 0 || o.column >= n_cols) return fail(i, "column index out of range");
      const int want = o.op == NP_F_CMP ? 1 : o.op == NP_F_BETWEEN ? 2 : o.op == NP_F_IS_NULL ? 0 : -1;
      if (want >= 0 && o.n_values != want) return fail(i, "wrong n_values for the op");
      if (o.n_values < 0) return fail(i, "negative n_values");
      if (o.n_values > 0 && (o.first_value < 0 || o.first_value > f->n_values || o.n_values > f->n_values - o.first_value))
        return fail(i, "value range outside values[]");
      if (o.op == NP_F_CMP && (o.arg < 0 || o.arg > 5)) return fail(i, "unknown comparison");
      if (o.op == NP_F_IN && (o.arg & ~1)) return fail(i, "unknown IN flags");
      if ((o.op == NP_F_BETWEEN || o.op == NP_F_IS_NULL) && o.arg != 0) return fail(i, "arg must be 0");
      const int type = col_types[o.column];
      const int64_t* v = o.n_values > 0 ? f->values + o.first_value : nullptr;
      if (type == NP_COL_F64)
        for (int k = 0; k < o.n_values; ++k)
          if (filter_f64_of(v[k]) != filter_f64_of(v[k])) return fail(i, "NaN constant");
      if (o.op == NP_F_IN)
        for (int k = 1; k < o.n_values; ++k) {
          const bool asc = type == NP_COL_F64 ? filter_f64_of(v[k - 1]) < filter_f64_of(v[k]) : v[k - 1] < v[k];
          if (!asc) return fail(i, "IN list is not ascending and distinct");
        }
      ++depth;
    } else if (o.op == NP_F_MATCH) {
      // the packed DFA is checked here; that the column has text on the device is the handle's to say (match_collect)
      if (o.column < 0 || o.column >= n_cols) return fail(i, "column index out of range");
      if (col_types[o.column] != NP_COL_CODE) return fail(i, "MATCH needs a CODE column");
      if (o.arg != 0) return fail(i, "arg must be 0");
      if (o.n_values < 1 || o.first_value < 0 || o.first_value > f->n_values || o.n_values > f->n_values - o.first_value)
        return fail(i, "value range outside values[]");
      char dfa_why[160];
      if (match_check_dfa(f->values + o.first_value, (int64_t)o.n_values, 0, dfa_why, sizeof dfa_why, nullptr) != 0) {
        snprintf(why, why_len, "filter %d, op %d: %s", filter, i, dfa_why);
        return (int)NP_ERR_INVALID_ARGUMENT;
      }
      ++depth;
    } else if (o.op == NP_F_CONST) {
      if (o.arg < 0 || o.arg > 2) return fail(i, "unknown constant");
      ++depth;
    } else if (o.op == NP_F_AND || o.op == NP_F_OR) {
      if (depth < 2) return fail(i, "stack underflow");
      --depth;
    } else if (o.op == NP_F_NOT) {
      if (depth < 1) return fail(i, "stack underflow");
    } else {
      return fail(i, "unknown op");
    }
    if (depth > NP_FILTER_MAX_DEPTH) return fail(i, "stack deeper than 32");
  }
  if (depth != 1) return fail(-1, "the program does not leave exactly one value");
  return 0;
}

// Chunks: `filters` filters over `docs` documents at a time (docs a multiple of NP_FILTER_BLOCK_DOCS unless it is all of
// them), so that per chunk
//     filters * blocks * (2048 mask + 4 count + 8 base [+ 8 * NP_FILTER_BLOCK_DOCS staged ids]) + fixed  <=  budget.
// All filters first, then fewer; false: one filter over one block does not fit.
struct FilterPlan {
  int32_t filters = 1;
  int64_t docs = NP_FILTER_BLOCK_DOCS;
  int64_t blocks() const { return (docs + NP_FILTER_BLOCK_DOCS - 1) / NP_FILTER_BLOCK_DOCS; }
};
inline int64_t filter_block_bytes(bool stage_ids) {
  return NP_FILTER_BLOCK_DOCS / 8 + 4 + 8 + (stage_ids ? 8 * NP_FILTER_BLOCK_DOCS : 0);
}
inline bool filter_plan(int64_t budget, int64_t fixed, int64_t n_docs, int32_t n_filters, bool stage_ids, FilterPlan* out) {
  if (n_docs < 1) n_docs = 1;
  if (n_filters < 1) n_filters = 1;
  const int64_t all_blocks = (n_docs + NP_FILTER_BLOCK_DOCS - 1) / NP_FILTER_BLOCK_DOCS;
  const int64_t units = budget > fixed ? (budget - fixed) / filter_block_bytes(stage_ids) : 0;   // (filter, block) pairs
  if (units < 1) return false;
  if (units >= n_filters) {
    const int64_t b = units / n_filters;
    out->filters = n_filters;
    out->docs = b >= all_blocks ? n_docs : b * NP_FILTER_BLOCK_DOCS;
  } else {
    out->filters = (int32_t)units;
    out->docs = all_blocks == 1 ? n_docs : NP_FILTER_BLOCK_DOCS;
  }
  return true;
}

}  // namespace np
