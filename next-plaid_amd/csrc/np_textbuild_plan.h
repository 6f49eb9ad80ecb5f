// np_textbuild_plan.h -- the host side of the keyword-index build (np_textbuild.hip) that needs no device: the argument
// checks of np_hip_text_build and np_hip_text_build_add, the sizes of the term table, the sort and the workspace, the sort of
// the vocabulary (fts5vocab's term order) and the merge of the fallback documents' instances into the device's arrays.
// Plain C++; tests/cpp/textbuild_plan_check.cpp runs all of it stand-alone.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/nextplaid_hip.h"

namespace np {

constexpr int32_t NP_TB_DEFAULT_MAX_TOKEN = 256;
constexpr int32_t NP_TB_TILE_MAX = 1024;           // 64 lanes of 16 bytes: what a wave loads per step
constexpr int64_t NP_TB_TEXT_PAD = 64;             // zero bytes behind the text: a 16-byte load may start at its last byte
constexpr int64_t NP_TB_MAX_INSTANCES = ((int64_t)1 << 31) - 1;
constexpr int64_t NP_TB_MAX_DOC_BYTES = ((int64_t)1 << 31) - 1;
constexpr int32_t NP_TB_TRIGRAM_KEYS = 1 << 21;    // three 7-bit bytes
constexpr int32_t NP_TB_HASH_BITS_MIN = 10, NP_TB_HASH_BITS_PLANNED_MAX = 26, NP_TB_HASH_BITS_MAX = 31;
constexpr int32_t NP_TB_SORT_CHUNK = 2048;         // keys per block of a radix pass (one wave, 32 rounds)
constexpr int32_t NP_TB_SCAN_CHUNK = 2048;         // items per block of a scan launch

constexpr int64_t NP_TB_PLANE = 65536;              // code points per plane of the unicode61 table; 1..17 planes
constexpr int32_t NP_TB_UTF8_MAX_TOKEN = 21845;     // UTF-8 mode: 3/2 of it is SQLite's own cut at 32768
constexpr uint32_t NP_TB_CLASS_SEP = 0, NP_TB_CLASS_TOKEN = 1, NP_TB_CLASS_MARK = 2;   // bits 30-31 of a table entry
constexpr uint32_t NP_TB_FOLD_MASK = 0x1FFFFFu;     // bits 0-20: the folded code point

struct TextBuildPlan {
  int32_t tokenizer = 0, max_token = 0, tile_bytes = 0, hash_bits_forced = 0;
  int64_t text_bytes = 0, workspace_bytes = 0;
  const uint32_t* unicode_table = nullptr;   // UTF-8 mode when set (unicode61 only)
  int64_t unicode_table_len = 0;
};

// A-Z -> a-z; every other byte as it is
static inline uint8_t textbuild_fold(uint8_t c) { return (c >= 'A' && c <= 'Z') ? (uint8_t)(c + 32) : c; }
static inline bool textbuild_token_char(uint8_t c) {
  return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z');
}

static inline int textbuild_utf8_len(uint32_t cp) { return cp < 0x80u ? 1 : cp < 0x800u ? 2 : cp < 0x10000u ? 3 : 4; }

// The checks of np_text_build_opts.unicode_table, before any launch: what the kernels rely on (they index the table with
// any code point below its length and take the ASCII rule for bytes below 0x80 without reading it).  One pass over the
// whole table on EVERY call, 131 072 entries for two planes and 1.1 M for seventeen: a fixed cost per call that a small
// batch pays in full.  It has not been measured on its own.
inline int textbuild_check_table(const uint32_t* table, int64_t len, char* why, size_t why_len) {
  if (len < NP_TB_PLANE || len > 17 * NP_TB_PLANE || len % NP_TB_PLANE != 0)
    return snprintf(why, why_len, "unicode_table_len %lld is not a multiple of 65536 in 65536..%lld", (long long)len,
                    (long long)(17 * NP_TB_PLANE)),
           (int)NP_ERR_INVALID_ARGUMENT;
  for (int64_t cp = 0; cp < len; ++cp) {
    const uint32_t e = table[cp], cls = e >> 30, fold = e & NP_TB_FOLD_MASK;
    if (cls > NP_TB_CLASS_MARK)
      return snprintf(why, why_len, "unicode_table[0x%llX] has class %u; the classes are 0, 1 and 2", (long long)cp, cls),
             (int)NP_ERR_INVALID_ARGUMENT;
    if (fold >= 0x110000u || (fold >= 0xD800u && fold < 0xE000u))
      return snprintf(why, why_len, "unicode_table[0x%llX] folds to 0x%X, which is no code point", (long long)cp, fold),
             (int)NP_ERR_INVALID_ARGUMENT;
    if (cp < 128) {
      const uint32_t want = textbuild_token_char((uint8_t)cp) ? (NP_TB_CLASS_TOKEN << 30) | textbuild_fold((uint8_t)cp) : 0u;
      if (e != want)
        return snprintf(why, why_len, "unicode_table[0x%llX] is 0x%08X; the ASCII rule is 0x%08X", (long long)cp, e, want),
               (int)NP_ERR_INVALID_ARGUMENT;
    }
    if (cls == NP_TB_CLASS_TOKEN && textbuild_utf8_len(fold) > textbuild_utf8_len((uint32_t)cp) + 1)
      return snprintf(why, why_len, "unicode_table[0x%llX] folds to 0x%X, more than one byte longer in UTF-8", (long long)cp, fold),
             (int)NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

// The term of a token in UTF-8 mode: the folds of its code points, marks skipped, as UTF-8.  The token passed the walk, so
// every sequence is well formed and inside the table.  At most 3/2 of the raw length comes out.
inline void textbuild_fold_utf8(const uint8_t* p, int64_t len, const uint32_t* table, std::vector<uint8_t>* out) {
  for (int64_t i = 0; i < len;) {
    const uint32_t c = p[i];
    uint32_t cp;
    if (c < 0x80u) cp = c, i += 1;
    else if (c < 0xE0u) cp = ((c & 0x1Fu) << 6) | (p[i + 1] & 0x3Fu), i += 2;
    else if (c < 0xF0u) cp = ((c & 0x0Fu) << 12) | ((p[i + 1] & 0x3Fu) << 6) | (p[i + 2] & 0x3Fu), i += 3;
    else cp = ((c & 0x07u) << 18) | ((p[i + 1] & 0x3Fu) << 12) | ((p[i + 2] & 0x3Fu) << 6) | (p[i + 3] & 0x3Fu), i += 4;
    const uint32_t e = table[cp];
    if ((e >> 30) != NP_TB_CLASS_TOKEN) continue;
    const uint32_t f = e & NP_TB_FOLD_MASK;
    if (f < 0x80u) {
      out->push_back((uint8_t)f);
    } else if (f < 0x800u) {
      out->push_back((uint8_t)(0xC0u | (f >> 6)));
      out->push_back((uint8_t)(0x80u | (f & 0x3Fu)));
    } else if (f < 0x10000u) {
      out->push_back((uint8_t)(0xE0u | (f >> 12)));
      out->push_back((uint8_t)(0x80u | ((f >> 6) & 0x3Fu)));
      out->push_back((uint8_t)(0x80u | (f & 0x3Fu)));
    } else {
      out->push_back((uint8_t)(0xF0u | (f >> 18)));
      out->push_back((uint8_t)(0x80u | ((f >> 12) & 0x3Fu)));
      out->push_back((uint8_t)(0x80u | ((f >> 6) & 0x3Fu)));
      out->push_back((uint8_t)(0x80u | (f & 0x3Fu)));
    }
  }
}

// The checks of np_hip_text_build, before any launch.  `why` (at least 200 bytes) names the argument.
inline int textbuild_check_args(const int64_t* offsets, int64_t n_docs, const np_text_build_opts* opts, bool have_bytes,
                                TextBuildPlan* plan, char* why, size_t why_len) {
  if (!opts) return snprintf(why, why_len, "opts is NULL"), (int)NP_ERR_INVALID_ARGUMENT;
  if (opts->tokenizer != NP_TOK_UNICODE61 && opts->tokenizer != NP_TOK_TRIGRAM)
    return snprintf(why, why_len, "tokenizer %d is neither NP_TOK_UNICODE61 nor NP_TOK_TRIGRAM", opts->tokenizer),
           (int)NP_ERR_INVALID_ARGUMENT;
  if (opts->max_token_bytes < 0 || opts->max_token_bytes > NP_TEXT_BUILD_MAX_TOKEN_BYTES)
    return snprintf(why, why_len, "max_token_bytes %d outside 1..%d (0 = %d)", opts->max_token_bytes,
                    NP_TEXT_BUILD_MAX_TOKEN_BYTES, NP_TB_DEFAULT_MAX_TOKEN),
           (int)NP_ERR_INVALID_ARGUMENT;
  if (opts->hash_bits < 0 || opts->hash_bits > NP_TB_HASH_BITS_MAX)
    return snprintf(why, why_len, "hash_bits %d outside 1..%d (0 = planned)", opts->hash_bits, NP_TB_HASH_BITS_MAX),
           (int)NP_ERR_INVALID_ARGUMENT;
  if (opts->tile_bytes < 0 || opts->tile_bytes > NP_TB_TILE_MAX || opts->tile_bytes % 16 != 0)
    return snprintf(why, why_len, "tile_bytes %d is not a multiple of 16 in 16..%d (0 = %d)", opts->tile_bytes, NP_TB_TILE_MAX,
                    NP_TB_TILE_MAX),
           (int)NP_ERR_INVALID_ARGUMENT;
  if (opts->workspace_bytes < 0)
    return snprintf(why, why_len, "workspace_bytes %lld is negative", (long long)opts->workspace_bytes),
           (int)NP_ERR_INVALID_ARGUMENT;
  const bool utf8 = opts->tokenizer == NP_TOK_UNICODE61 && opts->unicode_table != nullptr;   // trigram ignores the table
  if (utf8) {
    const int rc = textbuild_check_table(opts->unicode_table, opts->unicode_table_len, why, why_len);
    if (rc != NP_OK) return rc;
    if (opts->max_token_bytes > NP_TB_UTF8_MAX_TOKEN)
      return snprintf(why, why_len, "max_token_bytes %d outside 1..%d with a unicode_table (0 = %d): a longer token could fold "
                                    "past SQLite's cut at %d", opts->max_token_bytes, NP_TB_UTF8_MAX_TOKEN, NP_TB_DEFAULT_MAX_TOKEN,
                      NP_TEXT_BUILD_MAX_TOKEN_BYTES),
             (int)NP_ERR_INVALID_ARGUMENT;
  }
  if (n_docs < 0) return snprintf(why, why_len, "n_docs %lld is negative", (long long)n_docs), (int)NP_ERR_INVALID_ARGUMENT;
  if (n_docs > NP_TB_MAX_INSTANCES)
    return snprintf(why, why_len, "Shape error: n_docs %lld; the limit is 2^31 - 1", (long long)n_docs), (int)NP_ERR_SHAPE;
  if (!offsets) return snprintf(why, why_len, "offsets is NULL"), (int)NP_ERR_INVALID_ARGUMENT;
  if (offsets[0] != 0)
    return snprintf(why, why_len, "offsets[0] is %lld, not 0", (long long)offsets[0]), (int)NP_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < n_docs; ++i) {
    if (offsets[i + 1] < offsets[i])
      return snprintf(why, why_len, "offsets do not ascend: offsets[%lld] = %lld after %lld", (long long)(i + 1),
                      (long long)offsets[i + 1], (long long)offsets[i]),
             (int)NP_ERR_INVALID_ARGUMENT;
    if (offsets[i + 1] - offsets[i] > NP_TB_MAX_DOC_BYTES)
      return snprintf(why, why_len, "Shape error: document %lld has %lld bytes; the limit is 2^31 - 1", (long long)i,
                      (long long)(offsets[i + 1] - offsets[i])),
             (int)NP_ERR_SHAPE;
  }
  if (offsets[n_docs] > 0 && !have_bytes) return snprintf(why, why_len, "bytes is NULL"), (int)NP_ERR_INVALID_ARGUMENT;
  if (plan) {
    plan->tokenizer = opts->tokenizer;
    plan->max_token = opts->max_token_bytes ? opts->max_token_bytes : NP_TB_DEFAULT_MAX_TOKEN;
    plan->tile_bytes = opts->tile_bytes ? opts->tile_bytes : NP_TB_TILE_MAX;
    plan->hash_bits_forced = opts->hash_bits;
    plan->text_bytes = offsets[n_docs];
    plan->workspace_bytes = opts->workspace_bytes;
    plan->unicode_table = utf8 ? opts->unicode_table : nullptr;
    plan->unicode_table_len = utf8 ? opts->unicode_table_len : 0;
  }
  return NP_OK;
}

// trigram: the instance count is known on the host (unicode61's only after the counting launch)
inline int64_t textbuild_trigram_upper(const int64_t* offsets, int64_t n_docs) {
  int64_t t = 0;
  for (int64_t i = 0; i < n_docs; ++i) t += std::max<int64_t>(offsets[i + 1] - offsets[i] - 2, 0);
  return t;
}

inline int textbuild_check_instances(int64_t n_instances, char* why, size_t why_len) {
  if (n_instances > NP_TB_MAX_INSTANCES)
    return snprintf(why, why_len, "Shape error: %lld instances in one call; the limit is 2^31 - 1", (long long)n_instances),
           (int)NP_ERR_SHAPE;
  return NP_OK;
}

static inline int32_t textbuild_bit_length(uint64_t v) {
  int32_t b = 0;
  while (v) ++b, v >>= 1;
  return b;
}

// passes of 8 bits that order term ids 0 .. n_terms - 1
static inline int32_t textbuild_sort_passes(int64_t n_terms) {
  return n_terms <= 1 ? 0 : (textbuild_bit_length((uint64_t)(n_terms - 1)) + 7) / 8;
}

// the first term table: at least two slots per instance up to 2^26 slots (a vocabulary is far smaller than its corpus; a
// table that fills up is doubled)
static inline int32_t textbuild_hash_bits(int64_t n_instances, int32_t forced) {
  if (forced > 0) return forced;
  const int32_t b = textbuild_bit_length((uint64_t)std::max<int64_t>(2 * n_instances - 1, 1));
  return std::min(std::max(b, NP_TB_HASH_BITS_MIN), NP_TB_HASH_BITS_PLANNED_MAX);
}

static inline int64_t textbuild_up256(int64_t v) { return (v + 255) & ~(int64_t)255; }
static inline int64_t textbuild_scan_sums(int64_t n) { return (n + NP_TB_SCAN_CHUNK - 1) / NP_TB_SCAN_CHUNK + 1; }

// device bytes of the first phase (text, offsets, per-document arrays; UTF-8 mode: the table's device copy) ...
static inline int64_t textbuild_bytes_docs(int64_t text_bytes, int64_t n_docs, int64_t table_len = 0) {
  return textbuild_up256(text_bytes + NP_TB_TEXT_PAD) + 2 * textbuild_up256((n_docs + 1) * 8) + 2 * textbuild_up256((n_docs + 1) * 4) +
         textbuild_up256(textbuild_scan_sums(n_docs + 1) * 8) + 256 + (table_len > 0 ? textbuild_up256(table_len * 4) : 0);
}
// ... and of everything a call holds at its peak: per instance doc, offset, length, two key and two value arrays, then
// inst_doc and inst_pos; the term table with its flags and ranks (trigram: bitmap, counts and prefix); the histograms
static inline int64_t textbuild_bytes_total(int64_t text_bytes, int64_t n_docs, int64_t n_inst, int32_t tokenizer, int32_t hash_bits,
                                            int64_t table_len = 0) {
  const int64_t per_inst = 7 * textbuild_up256(n_inst * 4 + 4) + textbuild_up256(n_inst * 8 + 8) + textbuild_up256(n_inst * 4 + 4);
  const int64_t slots = tokenizer == NP_TOK_TRIGRAM ? NP_TB_TRIGRAM_KEYS / 32 : (int64_t)1 << hash_bits;
  const int64_t table = 3 * textbuild_up256(slots * 4 + 4) + textbuild_up256(textbuild_scan_sums(slots + 1) * 8);
  const int64_t blocks = (n_inst + NP_TB_SORT_CHUNK - 1) / NP_TB_SORT_CHUNK;
  const int64_t hist = textbuild_up256((256 * blocks + 1) * 4) + textbuild_up256(textbuild_scan_sums(256 * blocks + 1) * 8);
  const int64_t max_terms = std::min<int64_t>(n_inst, tokenizer == NP_TOK_TRIGRAM ? (int64_t)NP_TB_TRIGRAM_KEYS : slots);
  const int64_t terms = 5 * textbuild_up256(max_terms * 4 + 4) + textbuild_up256((max_terms + 1) * 8);   // their places, ranks, term_offsets
  return textbuild_bytes_docs(text_bytes, n_docs, table_len) + per_inst + table + hist + terms;
}

// ---- the vocabulary ------------------------------------------------------------------------------------------------------
// fts5vocab's order: memcmp over the common length, the shorter string first on a tie
static inline int textbuild_term_cmp(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb) {
  const int c = memcmp(a, b, (size_t)std::min(la, lb));
  return c ? c : (la < lb ? -1 : (la > lb ? 1 : 0));
}

// n distinct strings (bytes + offsets[n + 1]) -> rank[i] = position of string i in term order, and the strings in that order
inline void textbuild_sort_terms(const uint8_t* bytes, const int64_t* offs, int64_t n, std::vector<uint32_t>* rank,
                                 std::vector<uint8_t>* sorted_bytes, std::vector<int64_t>* sorted_offs) {
  std::vector<uint32_t> order((size_t)n);
  for (int64_t i = 0; i < n; ++i) order[(size_t)i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    return textbuild_term_cmp(bytes + offs[x], offs[x + 1] - offs[x], bytes + offs[y], offs[y + 1] - offs[y]) < 0;
  });
  rank->assign((size_t)n, 0);
  sorted_bytes->clear();
  sorted_bytes->reserve((size_t)(n ? offs[n] : 0));
  sorted_offs->assign((size_t)n + 1, 0);
  for (int64_t r = 0; r < n; ++r) {
    const uint32_t i = order[(size_t)r];
    (*rank)[i] = (uint32_t)r;
    sorted_bytes->insert(sorted_bytes->end(), bytes + offs[i], bytes + offs[i + 1]);
    (*sorted_offs)[(size_t)r + 1] = (int64_t)sorted_bytes->size();
  }
}

// ---- the fallback documents' instances -----------------------------------------------------------------------------------
struct TextArrays {
  std::vector<uint8_t> term_bytes;
  std::vector<int64_t> term_byte_offsets;   // [n_terms + 1]
  std::vector<int64_t> term_offsets;        // [n_terms + 1]
  std::vector<int64_t> inst_doc;
  std::vector<int32_t> inst_pos;
  int64_t n_terms() const { return term_byte_offsets.empty() ? 0 : (int64_t)term_byte_offsets.size() - 1; }
};

// The checks of np_hip_text_build_add.  fallback [n_fallback] ascending.
inline int textbuild_check_added(const uint8_t* term_bytes, const int64_t* tbo, int64_t n_terms, const int32_t* inst_term,
                                 const int64_t* inst_doc, const int32_t* inst_pos, int64_t n, const int64_t* fallback,
                                 int64_t n_fallback, char* why, size_t why_len) {
  if (n_terms < 0 || n < 0) return snprintf(why, why_len, "a negative count"), (int)NP_ERR_INVALID_ARGUMENT;
  if (n_terms > 0 && !tbo) return snprintf(why, why_len, "term_byte_offsets is NULL"), (int)NP_ERR_INVALID_ARGUMENT;
  if (n > 0 && (!inst_term || !inst_doc || !inst_pos))
    return snprintf(why, why_len, "an instance array is NULL"), (int)NP_ERR_INVALID_ARGUMENT;
  if (n_terms > 0 && tbo[0] != 0)
    return snprintf(why, why_len, "term_byte_offsets[0] is %lld, not 0", (long long)tbo[0]), (int)NP_ERR_INVALID_ARGUMENT;
  for (int64_t t = 0; t < n_terms; ++t) {
    if (tbo[t + 1] <= tbo[t])
      return snprintf(why, why_len, "term %lld is empty or term_byte_offsets descend", (long long)t), (int)NP_ERR_INVALID_ARGUMENT;
    if (!term_bytes) return snprintf(why, why_len, "term_bytes is NULL"), (int)NP_ERR_INVALID_ARGUMENT;
    if (t > 0 && textbuild_term_cmp(term_bytes + tbo[t - 1], tbo[t] - tbo[t - 1], term_bytes + tbo[t], tbo[t + 1] - tbo[t]) >= 0)
      return snprintf(why, why_len, "terms out of order: term %lld does not sort after term %lld", (long long)t, (long long)(t - 1)),
             (int)NP_ERR_INVALID_ARGUMENT;
  }
  int64_t expect = 0;   // the next term that must appear: every term has an instance
  for (int64_t i = 0; i < n; ++i) {
    const int64_t t = inst_term[i];
    if (t < 0 || t >= n_terms)
      return snprintf(why, why_len, "instance %lld names term %lld of %lld", (long long)i, (long long)t, (long long)n_terms),
             (int)NP_ERR_INVALID_ARGUMENT;
    if (inst_pos[i] < 0)
      return snprintf(why, why_len, "instance %lld has the negative position %d", (long long)i, inst_pos[i]),
             (int)NP_ERR_INVALID_ARGUMENT;
    if (i == 0 || t != inst_term[i - 1]) {
      if (t != expect)
        return snprintf(why, why_len, t < expect ? "instances out of order: instance %lld (term %lld) after term %lld"
                                                 : "instance %lld names term %lld, but term %lld has no instance",
                        (long long)i, (long long)t, (long long)(t < expect ? expect - 1 : expect)),
               (int)NP_ERR_INVALID_ARGUMENT;
      ++expect;
    } else if (inst_doc[i] < inst_doc[i - 1] || (inst_doc[i] == inst_doc[i - 1] && inst_pos[i] <= inst_pos[i - 1])) {
      return snprintf(why, why_len, "instances out of order: instance %lld (term %lld, document %lld, position %d) after (%lld, %d)",
                      (long long)i, (long long)t, (long long)inst_doc[i], inst_pos[i], (long long)inst_doc[i - 1], inst_pos[i - 1]),
             (int)NP_ERR_INVALID_ARGUMENT;
    }
    if (!std::binary_search(fallback, fallback + n_fallback, inst_doc[i]))
      return snprintf(why, why_len, "instance %lld names document %lld, which is not on the fallback list", (long long)i,
                      (long long)inst_doc[i]),
             (int)NP_ERR_INVALID_ARGUMENT;
  }
  if (expect != n_terms)
    return snprintf(why, why_len, "term %lld has no instance", (long long)expect), (int)NP_ERR_INVALID_ARGUMENT;
  return NP_OK;
}

// One linear merge: the vocabularies are united in term order; a term of both sides gets the two runs merged by (document,
// position).  The two sides never share a document, so no two instances compare equal.
inline void textbuild_merge(const TextArrays& a, const uint8_t* b_bytes, const int64_t* b_tbo, int64_t b_terms,
                            const int32_t* b_term, const int64_t* b_doc, const int32_t* b_pos, int64_t b_n, TextArrays* out) {
  std::vector<int64_t> b_off((size_t)b_terms + 1, 0);   // term_offsets of the added side
  for (int64_t i = 0; i < b_n; ++i) ++b_off[(size_t)b_term[i] + 1];
  for (int64_t t = 0; t < b_terms; ++t) b_off[(size_t)t + 1] += b_off[(size_t)t];
  const int64_t a_terms = a.n_terms();
  out->term_bytes.clear();
  out->term_byte_offsets.assign(1, 0);
  out->term_offsets.assign(1, 0);
  out->inst_doc.clear();
  out->inst_pos.clear();
  out->inst_doc.reserve(a.inst_doc.size() + (size_t)b_n);
  out->inst_pos.reserve(a.inst_pos.size() + (size_t)b_n);
  int64_t i = 0, j = 0;
  while (i < a_terms || j < b_terms) {
    int c;
    if (i >= a_terms) c = 1;
    else if (j >= b_terms) c = -1;
    else
      c = textbuild_term_cmp(a.term_bytes.data() + a.term_byte_offsets[(size_t)i], a.term_byte_offsets[(size_t)i + 1] - a.term_byte_offsets[(size_t)i],
                             b_bytes + b_tbo[j], b_tbo[j + 1] - b_tbo[j]);
    if (c <= 0)
      out->term_bytes.insert(out->term_bytes.end(), a.term_bytes.begin() + a.term_byte_offsets[(size_t)i],
                             a.term_bytes.begin() + a.term_byte_offsets[(size_t)i + 1]);
    else
      out->term_bytes.insert(out->term_bytes.end(), b_bytes + b_tbo[j], b_bytes + b_tbo[j + 1]);
    int64_t p = c <= 0 ? a.term_offsets[(size_t)i] : 0, pe = c <= 0 ? a.term_offsets[(size_t)i + 1] : 0;
    int64_t q = c >= 0 ? b_off[(size_t)j] : 0, qe = c >= 0 ? b_off[(size_t)j + 1] : 0;
    while (p < pe || q < qe) {
      const bool take_a = q >= qe || (p < pe && (a.inst_doc[(size_t)p] < b_doc[q] ||
                                                 (a.inst_doc[(size_t)p] == b_doc[q] && a.inst_pos[(size_t)p] < b_pos[q])));
      if (take_a) {
        out->inst_doc.push_back(a.inst_doc[(size_t)p]);
        out->inst_pos.push_back(a.inst_pos[(size_t)p]);
        ++p;
      } else {
        out->inst_doc.push_back(b_doc[q]);
        out->inst_pos.push_back(b_pos[q]);
        ++q;
      }
    }
    out->term_byte_offsets.push_back((int64_t)out->term_bytes.size());
    out->term_offsets.push_back((int64_t)out->inst_doc.size());
    if (c <= 0) ++i;
    if (c >= 0) ++j;
  }
}

}  // namespace np
