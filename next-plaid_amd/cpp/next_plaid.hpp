// next_plaid.hpp -- C++ host-side mirror of the next-plaid crate's search API over the C ABI.
//
// The reference host code is Rust (next-plaid/src/index.rs, search.rs, error.rs); this image has no
// Rust toolchain, so the host side above include/nextplaid_hip.h is written in C++ with the SAME
// names, argument meaning and error behaviour.  The Rust shim a maintainer would add is shown in
// INTEGRATION.md; it is a line-for-line analogue of this header.
//
//   next_plaid::MmapIndex::load(path)                      index.rs:1026
//   index.search(query, n_tokens, params, subset)          index.rs:1258  -> QueryResult, query_id = 0
//   index.search_batch(queries, params, parallel, subset)  index.rs:1279  -> query_id = batch position
//   index.search_batch_subsets(queries, n, params, parallel, subsets)   one subset per query (a server's batch of requests)
//   index.search_exact(queries, n, top_k, precision, subset) / search_exact_subsets(...)   every document scored: the exact top-k
//   index.set_text(...) / text_search(...) / fuse(...) / search_hybrid(...)   the keyword half of a hybrid search (text_search.rs);
//                                                          TextQuery = flat AND / OR, TextExpr = FTS5's NOT, parentheses, prefixes
//   index.set_groups(...) / collapse(...) / search_grouped(...) / search_hybrid_grouped(...)   top-k groups with their best documents
//   SearchParameters (defaults search.rs:58-69), QueryResult (search.rs:71-80), Error (error.rs:9-66)
//
// Accelerator policy (the crate's precedent for its CUDA feature, lib.rs:71-84 and cuda.rs:52-182):
//   NEXT_PLAID_FORCE_GPU=1|true   a device failure is an Error, never a fallback            (is_force_gpu)
//   NEXT_PLAID_FORCE_CPU=1|true   the HIP library is not touched at all (unless FORCE_GPU)  (is_force_cpu)
//   is_hip_broken / mark_hip_broken / clear_hip_broken: once DeviceUnavailable is seen the flag makes every later call
//   skip the device until it is cleared (CUDA_BROKEN, get_global_context's fast path).  OutOfMemory hands THAT call (or
//   that index) to the CPU hook without raising the process-wide flag: one oversized index must not take the device away
//   from every other index of the process.
// The CPU implementation itself is the crate's existing Rust path; here it is a hook (set_cpu_fallback) that the
// DeviceUnavailable hand-off calls -- this header ships NO CPU search of its own, and with no hook installed a
// device failure stays an Error (nothing is papered over).
//
// Header-only; link with -lnextplaid_hip.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <optional>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/nextplaid_hip.h"

namespace next_plaid {

struct Error : std::runtime_error {  // error.rs:9-66
  enum Kind { IndexLoad = 1, Search = 2, Shape = 3, Codec = 4, Io = 5, DeviceUnavailable = 6, OutOfMemory = 7, Config = 8,
              IndexCreation = 9 };
  Kind kind;
  Error(int code, const char* msg) : std::runtime_error(msg && *msg ? msg : "next-plaid error"), kind((Kind)code) {}
};

inline void check(int rc) {
  if (rc != NP_OK) throw Error(rc, np_hip_last_error());
}

// ---- accelerator policy: lib.rs:71-84 -----------------------------------------------------------------------
inline bool env_flag(const char* name) {
  const char* v = std::getenv(name);
  if (!v) return false;
  if (std::strcmp(v, "1") == 0) return true;
  std::string s(v);
  std::transform(s.begin(), s.end(), s.begin(), [](unsigned char c) { return (char)std::tolower(c); });
  return s == "true";
}
inline bool is_force_gpu() { return env_flag("NEXT_PLAID_FORCE_GPU"); }
inline bool is_force_cpu() { return !is_force_gpu() && env_flag("NEXT_PLAID_FORCE_CPU"); }

// ---- broken flag: cuda.rs:52-182 ----------------------------------------------------------------------------------
inline std::atomic<bool>& hip_broken_flag() {
  static std::atomic<bool> f{false};
  return f;
}
inline bool is_hip_broken() { return hip_broken_flag().load(std::memory_order_relaxed); }
inline void mark_hip_broken() { hip_broken_flag().store(true, std::memory_order_relaxed); }
inline void clear_hip_broken() { hip_broken_flag().store(false, std::memory_order_relaxed); }
inline bool is_device_failure(int rc) { return rc == NP_ERR_DEVICE_UNAVAILABLE || rc == NP_ERR_OUT_OF_MEMORY; }

struct SearchParameters {  // search.rs:26-69
  size_t batch_size = 2000;
  size_t n_full_scores = 4096;
  size_t top_k = 10;
  size_t n_ivf_probe = 8;
  size_t centroid_batch_size = 100000;
  std::optional<float> centroid_score_threshold = 0.4f;
  int precision = 2;  // exact-MaxSim arithmetic (np_search_params.precision): 2 = split-bf16 QC-reuse, f32-class (default)
  np_search_params c() const {
    np_search_params p{};
    p.top_k = (int32_t)top_k;
    p.n_full_scores = (int32_t)n_full_scores;
    p.n_ivf_probe = (int32_t)n_ivf_probe;
    p.centroid_batch_size = (int32_t)centroid_batch_size;
    p.centroid_score_threshold = centroid_score_threshold.value_or(0.f);
    p.has_threshold = centroid_score_threshold.has_value() ? 1 : 0;
    p.precision = precision;
    return p;
  }
};

struct QueryResult {  // search.rs:71-80
  size_t query_id = 0;
  std::vector<int64_t> passage_ids;
  std::vector<float> scores;
};
using SearchResult = QueryResult;  // search.rs:678

// A row-major [n_tokens, dim] f32 query (ndarray::Array2<f32> in the crate).
struct Query {
  const float* data;
  size_t n_tokens;
};

// The CPU path a device failure hands off to (in the crate: search::search_many_mmap on the mmap'ed index).
using CpuSearchFn = std::function<std::vector<QueryResult>(const std::string& index_path, const Query* queries, size_t n,
                                                           size_t dim, const SearchParameters& params, bool parallel,
                                                           const std::vector<int64_t>* subset)>;
inline CpuSearchFn& cpu_fallback() {
  static CpuSearchFn f;
  return f;
}
inline void set_cpu_fallback(CpuSearchFn f) { cpu_fallback() = std::move(f); }

// IndexConfig (index.rs:60-112): the fields index creation reads, same defaults.  start_from_scratch < 0: never write
// embeddings.npy.
struct IndexConfig {
  int nbits = 4;
  int64_t batch_size = 50000;
  uint64_t seed = 42;
  int kmeans_niters = 4;
  int64_t max_points_per_centroid = 256;
  std::optional<int64_t> n_samples_kmeans;
  int64_t start_from_scratch = 999;
  np_index_config c(int64_t num_partitions = 0) const {
    np_index_config o{};
    o.nbits = nbits;
    o.kmeans_niters = kmeans_niters;
    o.batch_size = batch_size;
    o.seed = seed;
    o.max_points_per_centroid = max_points_per_centroid;
    o.n_samples_kmeans = n_samples_kmeans.value_or(0);
    o.num_partitions = num_partitions;
    o.start_from_scratch = start_from_scratch == 0 ? -1 : start_from_scratch;
    return o;
  }
};

// Documents for index creation: every document's token rows concatenated ([sum doc_lengths][dim], row-major).
struct Documents {
  const float* embeddings = nullptr;
  std::vector<int64_t> doc_lengths;
  size_t dim = 0;
};

// kmeans.rs:423-...: the number of centroids compute_kmeans computes (host only)
inline int64_t estimate_num_partitions(const std::vector<int64_t>& doc_lengths, const IndexConfig& cfg = {}) {
  np_index_config c = cfg.c();
  np_kmeans_plan p{};
  check(np_hip_kmeans_plan(doc_lengths.data(), (int64_t)doc_lengths.size(), &c, &p, nullptr));
  return p.k;
}

// FastKMeans::train on the GPU: centroids [k][dim] (not normalised); assign (optional) = the last iteration's assignment,
// -1 outside the subsample
inline std::vector<float> kmeans(const float* points, int64_t n, size_t dim, const np_kmeans_opts& opts,
                                 const float* init = nullptr, std::vector<int64_t>* assign = nullptr,
                                 np_kmeans_report* report = nullptr, int device = 0) {
  std::vector<float> out((size_t)std::max<int64_t>(opts.k, 1) * dim);
  if (assign) assign->assign((size_t)std::max<int64_t>(n, 1), -1);
  check(np_hip_kmeans(device, points, n, (int32_t)dim, &opts, init, out.data(), assign ? assign->data() : nullptr, report));
  out.resize((size_t)std::max<int64_t>(opts.k, 0) * dim);
  if (assign) assign->resize((size_t)n);
  return out;
}

// compute_kmeans (kmeans.rs:261-421): L2-normalised centroids [K][dim]
inline std::vector<float> compute_kmeans(const Documents& docs, const IndexConfig& cfg = {}, int64_t num_partitions = 0,
                                         int device = 0) {
  np_index_config c = cfg.c(num_partitions);
  np_kmeans_plan p{};
  check(np_hip_kmeans_plan(docs.doc_lengths.data(), (int64_t)docs.doc_lengths.size(), &c, &p, nullptr));
  std::vector<float> out((size_t)std::max<int64_t>(p.k, 1) * docs.dim);
  int64_t k = 0;
  check(np_hip_compute_kmeans(device, docs.embeddings, docs.doc_lengths.data(), (int64_t)docs.doc_lengths.size(),
                              (int32_t)docs.dim, &c, out.data(), p.k, &k, nullptr));
  out.resize((size_t)k * docs.dim);
  return out;
}

// prepare_codec_artifacts (index.rs:182-287)
struct CodecArtifacts {
  std::vector<float> bucket_cutoffs, bucket_weights, avg_residual;
  float cluster_threshold = 0.f;
};
inline CodecArtifacts prepare_codec_artifacts(const Documents& docs, const std::vector<float>& centroids,
                                              const IndexConfig& cfg = {}, int device = 0) {
  np_index_config c = cfg.c();
  CodecArtifacts a;
  a.bucket_cutoffs.resize(((size_t)1 << cfg.nbits) - 1);
  a.bucket_weights.resize((size_t)1 << cfg.nbits);
  a.avg_residual.resize(docs.dim);
  check(np_hip_prepare_codec_artifacts(device, docs.embeddings, docs.doc_lengths.data(), (int64_t)docs.doc_lengths.size(),
                                       (int32_t)docs.dim, centroids.data(), (int64_t)(centroids.size() / std::max<size_t>(docs.dim, 1)),
                                       &c, a.bucket_cutoffs.data(), a.bucket_weights.data(), a.avg_residual.data(),
                                       &a.cluster_threshold));
  return a;
}

// UpdateConfig (update.rs:75-107), same defaults.  start_from_scratch = 0 / buffer_size = 0 keep the crate's meaning (only an
// empty index starts from scratch; every update expands).
struct UpdateConfig {
  int64_t batch_size = 50000;
  int kmeans_niters = 4;
  int64_t max_points_per_centroid = 256;
  std::optional<int64_t> n_samples_kmeans;
  uint64_t seed = 42;
  int64_t start_from_scratch = 999;
  int64_t buffer_size = 100;
  np_update_config c() const {
    np_update_config o{};
    o.batch_size = batch_size;
    o.kmeans_niters = kmeans_niters;
    o.max_points_per_centroid = max_points_per_centroid;
    o.n_samples_kmeans = n_samples_kmeans.value_or(0);
    o.seed = seed;
    o.start_from_scratch = start_from_scratch == 0 ? -1 : start_from_scratch;
    o.buffer_size = buffer_size == 0 ? -1 : buffer_size;
    return o;
  }
};

inline std::vector<int64_t> update_ids(const np_update_report& r, size_t n) {
  std::vector<int64_t> ids(n);
  for (size_t i = 0; i < n; ++i) ids[i] = r.first_doc_id + (int64_t)i;
  return ids;
}

// A packed byte DFA (include/nextplaid_hip.h, "text predicates"): what a REGEXP or LIKE pattern crosses the ABI as.  There is
// no pattern compiler here, as there is no WHERE parser: a Rust host builds the table with regex-automata, the Python package
// with next_plaid_amd/regexes.py.  The library checks every table before a launch.
struct Dfa {
  std::vector<uint32_t> words;
  Dfa() = default;
  explicit Dfa(std::vector<uint32_t> w) : words(std::move(w)) {}
  // from its parts: class_of[256], flags[n_states] (NP_DFA_*), table[n_states * n_classes]
  Dfa(uint32_t start, const std::vector<uint8_t>& class_of, const std::vector<uint8_t>& flags, const std::vector<uint16_t>& table) {
    const size_t ns = flags.size(), nc = ns ? table.size() / ns : 0, f0 = NP_DFA_HEADER_WORDS, t0 = f0 + (ns + 3) / 4;
    if (class_of.size() != 256 || ns == 0 || nc * ns != table.size())
      throw Error(NP_ERR_INVALID_ARGUMENT, "Dfa: class_of needs 256 entries and table n_states * n_classes");
    words.assign(t0 + (ns * nc + 1) / 2, 0u);
    words[0] = NP_DFA_MAGIC;
    words[1] = (uint32_t)ns;
    words[2] = (uint32_t)nc;
    words[3] = start;
    for (size_t b = 0; b < 256; ++b) words[4 + b / 4] |= (uint32_t)class_of[b] << (8 * (b & 3));
    for (size_t s = 0; s < ns; ++s) words[f0 + s / 4] |= (uint32_t)flags[s] << (8 * (s & 3));
    for (size_t e = 0; e < table.size(); ++e) words[t0 + e / 2] |= (uint32_t)table[e] << (16 * (e & 1));
  }
  np_dfa c() const { return np_dfa{words.data(), (int64_t)words.size()}; }
};

// A metadata filter as the postfix program of np_hip_filter_eval (include/nextplaid_hip.h): leaves push a value, not_()
// replaces the top, and_() / or_() replace the top two; every value is TRUE, FALSE or UNKNOWN (SQLite's three-valued logic)
// and a document is selected where the program leaves TRUE.  `x NOT IN (...)` is in(...) followed by not_().  There is no
// WHERE parser here: a Rust caller keeps the crate's validator (filtering.rs:571-583), resolves text against its dictionary
// and emits the program.  The library checks the program (stack, columns, value ranges, sorted IN lists).
class FilterProgram {
 public:
  enum Cmp { EQ = 0, NE = 1, LT = 2, LE = 3, GT = 4, GE = 5 };
  enum Const { FALSE_ = 0, TRUE_ = 1, UNKNOWN = 2 };
  static int64_t bits(double v) {
    int64_t b;
    std::memcpy(&b, &v, 8);
    return b;
  }
  // constants: i64 as they are, codes sign-extended, doubles through bits()
  FilterProgram& cmp(int column, Cmp op, int64_t value) { return leaf(NP_F_CMP, column, op, {value}); }
  FilterProgram& cmp(int column, Cmp op, double value) { return leaf(NP_F_CMP, column, op, {bits(value)}); }
  FilterProgram& between(int column, int64_t lo, int64_t hi) { return leaf(NP_F_BETWEEN, column, 0, {lo, hi}); }
  FilterProgram& between(int column, double lo, double hi) { return leaf(NP_F_BETWEEN, column, 0, {bits(lo), bits(hi)}); }
  // `values` ascending and distinct (in the column's order); has_null: the list also held a NULL
  FilterProgram& in(int column, std::vector<int64_t> values, bool has_null = false) {
    return leaf(NP_F_IN, column, has_null ? 1 : 0, std::move(values));
  }
  FilterProgram& in(int column, const std::vector<double>& values, bool has_null = false) {
    std::vector<int64_t> b;
    for (double v : values) b.push_back(bits(v));
    return leaf(NP_F_IN, column, has_null ? 1 : 0, std::move(b));
  }
  FilterProgram& is_null(int column) { return leaf(NP_F_IS_NULL, column, 0, {}); }
  // `column` (CODE, with text on the device: MmapIndex::set_column_text) matches the DFA; UNKNOWN on a NULL cell
  FilterProgram& match(int column, const Dfa& dfa) {
    return leaf(NP_F_MATCH, column, 0, std::vector<int64_t>(dfa.words.begin(), dfa.words.end()));
  }
  FilterProgram& constant(Const c) { return node(NP_F_CONST, c); }
  FilterProgram& and_() { return node(NP_F_AND, 0); }
  FilterProgram& or_() { return node(NP_F_OR, 0); }
  FilterProgram& not_() { return node(NP_F_NOT, 0); }
  np_filter c() const {
    return np_filter{ops_.data(), (int32_t)ops_.size(), values_.empty() ? nullptr : values_.data(), (int64_t)values_.size()};
  }

 private:
  FilterProgram& leaf(int op, int column, int arg, std::vector<int64_t> v) {
    ops_.push_back(np_filter_op{op, column, arg, (int32_t)v.size(), v.empty() ? 0 : (int64_t)values_.size()});
    values_.insert(values_.end(), v.begin(), v.end());
    return *this;
  }
  FilterProgram& node(int op, int arg) {
    ops_.push_back(np_filter_op{op, -1, arg, 0, 0});
    return *this;
  }
  std::vector<np_filter_op> ops_;
  std::vector<int64_t> values_;
};

// One metadata column over the WHOLE index for MmapIndex::set_columns: a typed span and an optional validity span
// (one byte per document, 0 = NULL; nullptr = no NULLs; an f64 NaN is NULL either way).
struct ColumnSpan {
  int32_t type;
  const void* data;
  const uint8_t* valid;
  size_t size;
  static ColumnSpan i64(const int64_t* d, size_t n, const uint8_t* valid = nullptr) { return {NP_COL_I64, d, valid, n}; }
  static ColumnSpan f64(const double* d, size_t n, const uint8_t* valid = nullptr) { return {NP_COL_F64, d, valid, n}; }
  static ColumnSpan codes(const int32_t* d, size_t n, const uint8_t* valid = nullptr) { return {NP_COL_CODE, d, valid, n}; }
};

// A compiled keyword query (np_text_query), as FilterProgram is a compiled filter: phrases of term ids (-1 = a token the
// vocabulary does not hold), all joined by AND or all by OR.  Compiling FTS5 query text into term ids needs SQLite's own
// tokenizer and stays in the Python front end (next_plaid_amd/text.py); a Rust host would do it with rusqlite.
class TextQuery {
 public:
  explicit TextQuery(int mode = NP_TEXT_AND) : mode_(mode), off_{0} {}
  TextQuery& phrase(const std::vector<int32_t>& term_ids) {
    terms_.insert(terms_.end(), term_ids.begin(), term_ids.end());
    off_.push_back((int32_t)terms_.size());
    return *this;
  }
  np_text_query c() const { return np_text_query{terms_.data(), off_.data(), (int32_t)off_.size() - 1, mode_}; }

 private:
  int mode_;
  std::vector<int32_t> terms_, off_;
};

// A compiled keyword query with FTS5's boolean operators and prefixes (np_text_expr): phrases in the order of the query text
// and a postfix list of nodes over them.  phrase() and the operators append a node and return its index; operands are the
// indexes of the two nodes appended last that no operator has taken yet (the stack discipline np_hip_text_search_expr
// checks).  prefix_hi != 0: the phrase's last token stands for the terms [its id, prefix_hi).
// Append the phrases in the order of the query text, one statement each (C++ leaves the order of arguments open):
//   TextExpr e;  int a = e.phrase({parse}), b = e.phrase({lex}), l = e.or_(a, b);
//   int t = e.phrase({tok}, tok_hi);  e.not_(l, t);                                                 // (parse OR lex) NOT tok*
class TextExpr {
 public:
  TextExpr() : off_{0} {}
  int phrase(const std::vector<int32_t>& term_ids, int32_t prefix_hi = 0) {
    terms_.insert(terms_.end(), term_ids.begin(), term_ids.end());
    off_.push_back((int32_t)terms_.size());
    hi_.push_back(prefix_hi);
    return node(NP_TEXT_NODE_PHRASE, (int32_t)hi_.size() - 1, 0);
  }
  int and_(int a, int b) { return node(NP_TEXT_NODE_AND, a, b); }
  int or_(int a, int b) { return node(NP_TEXT_NODE_OR, a, b); }
  int not_(int a, int b) { return node(NP_TEXT_NODE_NOT, a, b); }   // a AND NOT b
  np_text_expr c() const {
    return np_text_expr{terms_.data(), off_.data(), hi_.data(), nodes_.data(), (int32_t)hi_.size(), (int32_t)nodes_.size()};
  }

 private:
  int node(int32_t op, int32_t a, int32_t b) {
    nodes_.push_back(np_text_node{op, a, b});
    return (int)nodes_.size() - 1;
  }
  std::vector<int32_t> terms_, off_, hi_;
  std::vector<np_text_node> nodes_;
};

// The keyword index for MmapIndex::set_text: the FTS5 table's (term, document, position) instances, sorted, term t owning
// [term_offsets[t], term_offsets[t + 1]), and the table's row count.
struct TextIndexSpan {
  const int64_t* term_offsets;
  size_t n_terms;
  const int64_t* inst_doc;
  const int32_t* inst_pos;
  int64_t n_rows;
};

// ---- what MmapIndex::append reads back from the directory an update_append wrote -----------------------------------------
namespace detail {
inline std::string read_file(const std::string& path) {
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw Error(NP_ERR_IO, ("IO error: cannot open " + path).c_str());
  std::string out;
  char buf[1 << 16];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
  std::fclose(f);
  return out;
}
// "key": <integer> of a JSON object the library wrote (metadata.json)
inline int64_t json_int(const std::string& j, const char* key, const std::string& path) {
  const std::string k = std::string("\"") + key + "\"";
  size_t at = j.find(k);
  if (at != std::string::npos) at = j.find(':', at + k.size());
  if (at == std::string::npos) throw Error(NP_ERR_INDEX_LOAD, ("Index load failed: no \"" + std::string(key) + "\" in " + path).c_str());
  return std::strtoll(j.c_str() + at + 1, nullptr, 10);
}
// a JSON list of integers (doclens.N.json)
inline std::vector<int64_t> json_ints(const std::string& j) {
  std::vector<int64_t> out;
  const char* p = j.c_str();
  while (*p) {
    if (*p == '-' || (*p >= '0' && *p <= '9')) {
      char* e = nullptr;
      out.push_back(std::strtoll(p, &e, 10));
      p = e;
    } else {
      ++p;
    }
  }
  return out;
}
// the last n_rows rows of an NPY v1 / v2 array of the given dtype (C order); *cols = entries per row (1 for rank 1)
inline std::string npy_tail(const std::string& path, const char* descr, size_t item, int64_t n_rows, int64_t* cols) {
  // only the header and the tail are read: a chunk of 50 000 documents holds gigabytes of residuals
  struct File {
    std::FILE* f;
    ~File() {
      if (f) std::fclose(f);
    }
  } file{std::fopen(path.c_str(), "rb")};
  if (!file.f) throw Error(NP_ERR_IO, ("IO error: cannot open " + path).c_str());
  unsigned char b[12] = {};
  if (std::fread(b, 1, 12, file.f) != 12 || std::memcmp(b, "\x93NUMPY", 6) != 0)
    throw Error(NP_ERR_INDEX_LOAD, ("Index load failed: " + path + " is not an NPY file").c_str());
  const bool v2 = b[6] >= 2;
  const size_t hl = v2 ? (size_t)b[8] | (size_t)b[9] << 8 | (size_t)b[10] << 16 | (size_t)b[11] << 24 : (size_t)b[8] | (size_t)b[9] << 8;
  const size_t h0 = v2 ? 12 : 10;
  std::string h(hl, '\0');
  if (hl > ((size_t)1 << 24) || std::fseek(file.f, (long)h0, SEEK_SET) != 0 || std::fread(&h[0], 1, hl, file.f) != hl)
    throw Error(NP_ERR_INDEX_LOAD, ("Index load failed: " + path + " has a truncated header").c_str());
  size_t sh = h.find("'shape'");
  if (h.find(descr) == std::string::npos || h.find("'fortran_order': False") == std::string::npos || sh == std::string::npos)
    throw Error(NP_ERR_INDEX_LOAD, ("Index load failed: " + path + " is not a C-order " + descr + " array").c_str());
  const std::vector<int64_t> shape = json_ints(h.substr(h.find('(', sh), h.find(')', sh) - h.find('(', sh)));
  const int64_t rows = shape.empty() ? 0 : shape[0];
  *cols = shape.size() > 1 ? shape[1] : 1;
  const size_t row = (size_t)*cols * item;
  std::string tail((size_t)std::max<int64_t>(n_rows, 0) * row, '\0');
  if (n_rows > rows || std::fseek(file.f, (long)(h0 + hl + (size_t)(rows - n_rows) * row), SEEK_SET) != 0 ||
      (!tail.empty() && std::fread(&tail[0], 1, tail.size(), file.f) != tail.size()))
    throw Error(NP_ERR_INDEX_LOAD, ("Index load failed: " + path + " holds fewer rows than its directory counts").c_str());
  return tail;
}
struct DirCounts {
  int64_t documents = 0, embeddings = 0, chunks = 0;
};
inline DirCounts dir_counts(const std::string& dir) {
  const std::string p = dir + "/metadata.json", j = read_file(p);
  return DirCounts{json_int(j, "num_documents", p), json_int(j, "num_embeddings", p), json_int(j, "num_chunks", p)};
}
// The documents a directory holds beyond `before`, as update_index wrote them: the tail of its last chunks (it appends to the
// last chunk or adds chunks, update.rs:771-1120)
struct AppendedTokens {
  std::vector<int64_t> doc_lengths, codes;
  std::vector<uint8_t> residuals;
};
inline AppendedTokens appended_tokens(const std::string& dir, const DirCounts& before) {
  const DirCounts now = dir_counts(dir);
  const int64_t n_new = now.documents - before.documents, t_new = now.embeddings - before.embeddings;
  AppendedTokens out;
  std::vector<std::vector<int64_t>> dl_parts;   // per chunk, the last chunk first: joined once below
  std::vector<std::string> cd_parts, rs_parts;
  int64_t have_d = 0, have_t = 0;
  for (int64_t c = now.chunks - 1; c >= 0 && have_d < n_new; --c) {
    const std::string stem = dir + "/" + std::to_string((long long)c);
    const std::vector<int64_t> dl = json_ints(read_file(dir + "/doclens." + std::to_string((long long)c) + ".json"));
    const int64_t take_d = std::min<int64_t>(n_new - have_d, (int64_t)dl.size());
    int64_t take_t = 0, cols = 0;
    for (int64_t d = (int64_t)dl.size() - take_d; d < (int64_t)dl.size(); ++d) take_t += dl[(size_t)d];
    dl_parts.emplace_back(dl.end() - take_d, dl.end());
    cd_parts.push_back(npy_tail(stem + ".codes.npy", "<i8", 8, take_t, &cols));
    rs_parts.push_back(npy_tail(stem + ".residuals.npy", "|u1", 1, take_t, &cols));
    have_d += take_d;
    have_t += take_t;
  }
  out.codes.resize((size_t)have_t);
  size_t at_c = 0;
  for (size_t i = dl_parts.size(); i-- > 0;) {
    out.doc_lengths.insert(out.doc_lengths.end(), dl_parts[i].begin(), dl_parts[i].end());
    if (!cd_parts[i].empty()) std::memcpy((char*)out.codes.data() + at_c, cd_parts[i].data(), cd_parts[i].size());
    at_c += cd_parts[i].size();
    out.residuals.insert(out.residuals.end(), rs_parts[i].begin(), rs_parts[i].end());
  }
  if (have_d != n_new || have_t != t_new)
    throw Error(NP_ERR_INDEX_LOAD, ("Index load failed: the chunk files of " + dir + " hold " + std::to_string(have_d) + " new documents / " +
                                    std::to_string(have_t) + " tokens, metadata.json counts " + std::to_string(n_new) + " / " + std::to_string(t_new)).c_str());
  return out;
}
// appended_tokens' reading for a given count: the directory's LAST n_tail documents, what an update in expansion mode wrote
// behind the documents it kept
inline AppendedTokens tail_documents(const std::string& dir, int64_t n_tail) {
  const DirCounts now = dir_counts(dir);
  AppendedTokens out;
  std::vector<std::vector<int64_t>> dl_parts;   // per chunk, the last chunk first: joined once below
  std::vector<std::string> cd_parts, rs_parts;
  int64_t have_d = 0, have_t = 0;
  for (int64_t c = now.chunks - 1; c >= 0 && have_d < n_tail; --c) {
    const std::string stem = dir + "/" + std::to_string((long long)c);
    const std::vector<int64_t> dl = json_ints(read_file(dir + "/doclens." + std::to_string((long long)c) + ".json"));
    const int64_t take_d = std::min<int64_t>(n_tail - have_d, (int64_t)dl.size());
    int64_t take_t = 0, cols = 0;
    for (int64_t d = (int64_t)dl.size() - take_d; d < (int64_t)dl.size(); ++d) take_t += dl[(size_t)d];
    dl_parts.emplace_back(dl.end() - take_d, dl.end());
    cd_parts.push_back(npy_tail(stem + ".codes.npy", "<i8", 8, take_t, &cols));
    rs_parts.push_back(npy_tail(stem + ".residuals.npy", "|u1", 1, take_t, &cols));
    have_d += take_d;
    have_t += take_t;
  }
  out.codes.resize((size_t)have_t);
  size_t at_c = 0;
  for (size_t i = dl_parts.size(); i-- > 0;) {
    out.doc_lengths.insert(out.doc_lengths.end(), dl_parts[i].begin(), dl_parts[i].end());
    if (!cd_parts[i].empty()) std::memcpy((char*)out.codes.data() + at_c, cd_parts[i].data(), cd_parts[i].size());
    at_c += cd_parts[i].size();
    out.residuals.insert(out.residuals.end(), rs_parts[i].begin(), rs_parts[i].end());
  }
  if (have_d != n_tail)
    throw Error(NP_ERR_INDEX_LOAD, ("Index load failed: the chunk files of " + dir + " hold " + std::to_string(have_d) + " documents, " +
                                    std::to_string(n_tail) + " were written").c_str());
  return out;
}
}  // namespace detail

class MmapIndex {
 public:
  // MmapIndex::create_with_kmeans (index.rs:927-967): k-means and codec training on the GPU, the crate's file set written
  // under index_path, then the index opened with `opts`.  Index creation has no CPU fallback here: a device failure is
  // the caller's to route to the crate's CPU path.
  static MmapIndex create_with_kmeans(const Documents& docs, const std::string& index_path, const IndexConfig& cfg = {},
                                      const np_open_opts* opts = nullptr) {
    check_abi();
    np_index_config c = cfg.c();
    np_index* h = nullptr;
    check(np_hip_index_create(index_path.c_str(), docs.embeddings, docs.doc_lengths.data(), (int64_t)docs.doc_lengths.size(),
                              (int32_t)docs.dim, &c, opts, &h));
    return MmapIndex(h, index_path);
  }

  // MmapIndex::load (index.rs:1026).  `opts` selects the device / document shard.
  // Policy: FORCE_CPU or a raised broken flag never touch the device (the handle stays empty and searches go to the
  // CPU hook); a device failure raises the flag and falls back unless FORCE_GPU; every other error is the caller's.
  static MmapIndex load(const std::string& index_path, const np_open_opts* opts = nullptr) {
    if ((is_force_cpu() || (is_hip_broken() && !is_force_gpu())) && cpu_fallback()) return MmapIndex(nullptr, index_path);
    check_abi();
    np_index* h = nullptr;
    const int rc = np_hip_index_open(index_path.c_str(), opts, &h);
    if (is_device_failure(rc)) {
      if (rc == NP_ERR_DEVICE_UNAVAILABLE) mark_hip_broken();   // OutOfMemory concerns this index only
      if (!is_force_gpu() && cpu_fallback()) {
        std::fprintf(stderr, "[next-plaid] HIP device unavailable: %s. Falling back to CPU. Set NEXT_PLAID_FORCE_CPU=1 to "
                             "skip the GPU and silence this warning.\n", np_hip_last_error());
        return MmapIndex(nullptr, index_path);
      }
    }
    check(rc);
    return MmapIndex(h, index_path);
  }
  // The library this binary RUNS against must speak the header it was COMPILED against: np_info / np_stats are allocated here and
  // have grown between ABI versions (np_hip_abi_version exists since v6; an older library fails at link / load time already).
  static void check_abi() {
    if (np_hip_abi_version() != NP_ABI_VERSION || np_hip_struct_size(0) != (int64_t)sizeof(np_info) ||
        np_hip_struct_size(1) != (int64_t)sizeof(np_stats))
      throw std::runtime_error("libnextplaid_hip speaks ABI v" + std::to_string(np_hip_abi_version()) + ", this host was built against v" +
                               std::to_string(NP_ABI_VERSION));
  }
  // MmapIndex::reload (index.rs:1767-1775): after delete / update rewrote the directory.  The crate releases its maps before
  // it loads again; here the device copy is dropped first for the same reason (two copies of a 200 GB index do not fit).
  // Exclusive access like `&mut self`; a service swaps handles.  Same device policy as load().
  void reload(const np_open_opts* opts = nullptr) {
    MmapIndex fresh = (close(), load(path, opts));
    *this = std::move(fresh);
  }
  // MmapIndex::update (index.rs:1431-1590): the new documents' ids; the handle is reloaded from the rewritten directory
  std::vector<int64_t> update(const Documents& docs, const UpdateConfig& cfg = {}, const np_open_opts* opts = nullptr,
                              np_update_report* report = nullptr) {
    check_abi();
    const np_update_config c = cfg.c();
    np_update_report r{};
    check(np_hip_index_update(path.c_str(), docs.embeddings, docs.doc_lengths.data(), (int64_t)docs.doc_lengths.size(),
                              (int32_t)docs.dim, &c, opts ? opts->device : 0, &r));
    if (report) *report = r;
    reload(opts);
    return update_ids(r, docs.doc_lengths.size());
  }
  // MmapIndex::update_append (index.rs:1675-1700): no mode choice, no reload
  static std::vector<int64_t> update_append(const Documents& docs, const std::string& index_path, const UpdateConfig& cfg = {},
                                            int device = 0) {
    check_abi();
    const np_update_config c = cfg.c();
    np_update_report r{};
    check(np_hip_index_update_append(index_path.c_str(), docs.embeddings, docs.doc_lengths.data(),
                                     (int64_t)docs.doc_lengths.size(), (int32_t)docs.dim, &c, device, &r));
    return update_ids(r, docs.doc_lengths.size());
  }
  // ---- append to the RESIDENT index (np_hip_index_append) -- where update() reloads the whole index, these cost the new
  // documents plus one pass over the posting lists, and searches on other threads go on meanwhile (the running ones finish on
  // the old index).  The handle then equals one freshly opened on the grown index; columns, keyword index and groups are
  // dropped, as reload() leaves a handle.  Unsharded handles with ascending posting lists (what this library and the crate
  // write); an update that may add centroids: update_resident() below; for delete see remove() below.
  // Documents already encoded (codes in [0, K), residuals [tokens][dim * nbits / 8] as np_hip_encode_tokens returns them):
  std::vector<int64_t> append_arrays(const std::vector<int64_t>& doc_lengths, const int64_t* codes, const uint8_t* residuals) {
    require_device("append_arrays");
    const int64_t first = info_.num_documents;
    check(np_hip_index_append(h_, doc_lengths.data(), (int64_t)doc_lengths.size(), codes, residuals));
    check(np_hip_index_info(h_, &info_));
    std::vector<int64_t> ids(doc_lengths.size());
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = first + (int64_t)i;
    return ids;
  }
  // ... with the new documents' rows (np_hip_index_append_rows): columns and groups stay attached and grow with the index.
  // `columns` holds one span per column of the handle over the NEW documents; `code_remap` is empty or has one entry per
  // column, each nullptr or the table old code -> new code of a dictionary that grew (its text on the device is then dropped:
  // set_column_text sets the grown dictionary); `groups` one id per new document in [0, n_groups), empty where the handle has
  // no groups.  The keyword index is dropped by the library: update_text_index(base, {add = the new texts}) and set_text
  // bring it along.
  struct AppendedRows {
    std::vector<ColumnSpan> columns;
    std::vector<const int32_t*> code_remap;
    std::vector<int32_t> groups;
    int64_t n_groups = 0;
  };
  std::vector<int64_t> append_arrays(const std::vector<int64_t>& doc_lengths, const int64_t* codes, const uint8_t* residuals,
                                     const AppendedRows& rows) {
    require_device("append_arrays");
    std::vector<np_column> c;
    for (const ColumnSpan& s : rows.columns) {
      if (s.size != doc_lengths.size()) throw Error(NP_ERR_SHAPE, "Shape error: a column needs one new entry per new document");
      c.push_back(np_column{s.type, 0, s.data, s.valid});
    }
    if (!rows.code_remap.empty() && rows.code_remap.size() != rows.columns.size())
      throw Error(NP_ERR_SHAPE, "Shape error: code_remap needs one entry per column, or none");
    if (!rows.groups.empty() && rows.groups.size() != doc_lengths.size())
      throw Error(NP_ERR_SHAPE, "Shape error: groups needs one id per new document");
    const int64_t first = info_.num_documents;
    check(np_hip_index_append_rows(h_, doc_lengths.data(), (int64_t)doc_lengths.size(), codes, residuals, c.data(), (int32_t)c.size(),
                                   rows.code_remap.empty() ? nullptr : rows.code_remap.data(),
                                   rows.groups.empty() ? nullptr : rows.groups.data(), rows.n_groups));
    check(np_hip_index_info(h_, &info_));
    std::vector<int64_t> ids(doc_lengths.size());
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = first + (int64_t)i;
    return ids;
  }
  // update_append on the handle's directory AND on the handle: the documents are encoded once, by np_hip_index_update_append,
  // and the codes and residuals it wrote to the chunk files are what np_hip_index_append gets
  std::vector<int64_t> append(const Documents& docs, const UpdateConfig& cfg = {}, int device = 0, np_update_report* report = nullptr) {
    return append_by(
        docs, cfg, device, report, [&] { check(np_hip_index_append(h_, nullptr, 0, nullptr, nullptr)); },
        [&](const detail::AppendedTokens& t) { (void)append_arrays(t.doc_lengths, t.codes.data(), t.residuals.data()); });
  }
  // ... with the new documents' rows (its own name: append(docs, {}) keeps meaning a default UpdateConfig).  What the library
  // refuses of the rows is found before the directory is touched
  std::vector<int64_t> append_with_rows(const Documents& docs, const AppendedRows& rows, const UpdateConfig& cfg = {}, int device = 0,
                                        np_update_report* report = nullptr) {
    if (!rows.code_remap.empty() && rows.code_remap.size() != rows.columns.size())
      throw Error(NP_ERR_SHAPE, "Shape error: code_remap needs one entry per column, or none");
    for (const ColumnSpan& s : rows.columns)
      if (s.size != docs.doc_lengths.size()) throw Error(NP_ERR_SHAPE, "Shape error: a column needs one new entry per new document");
    if (!rows.groups.empty() && rows.groups.size() != docs.doc_lengths.size())
      throw Error(NP_ERR_SHAPE, "Shape error: groups needs one id per new document");
    return append_by(
        docs, cfg, device, report,
        [&] {   // an append of no documents runs the library's checks of the rows too: column count, types, remaps, group presence
          if (!docs.doc_lengths.empty() && (np_hip_index_group_count(h_) > 0) != !rows.groups.empty())
            throw Error(NP_ERR_INVALID_ARGUMENT, "Invalid argument: append: groups are needed of a handle with groups, and of no other");
          std::vector<np_column> c;
          for (const ColumnSpan& s : rows.columns) c.push_back(np_column{s.type, 0, s.data, s.valid});
          check(np_hip_index_append_rows(h_, nullptr, 0, nullptr, nullptr, c.data(), (int32_t)c.size(),
                                         rows.code_remap.empty() ? nullptr : rows.code_remap.data(),
                                         rows.groups.empty() ? nullptr : rows.groups.data(), rows.n_groups));
        },
        [&](const detail::AppendedTokens& t) { (void)append_arrays(t.doc_lengths, t.codes.data(), t.residuals.data(), rows); });
  }

 private:
  // the two appends differ in the check of the handle before the directory is touched and in the entry the tokens go to (a
  // program that never appends rows never names the entry that takes them)
  template <class Check, class Put>
  std::vector<int64_t> append_by(const Documents& docs, const UpdateConfig& cfg, int device, np_update_report* report, Check&& check_handle,
                                 Put&& put) {
    require_device("append");
    // whatever would refuse the handle's half is found BEFORE the directory is touched: a handle that is not current with its
    // directory, and (an append of no documents runs the library's checks of the handle: shards, list order)
    const detail::DirCounts before = detail::dir_counts(path);
    if (before.documents != info_.num_documents)
      throw Error(NP_ERR_INDEX_LOAD, "Index load failed: the handle is not current with its directory: reload()");
    check_handle();
    const np_update_config c = cfg.c();
    np_update_report r{};
    check(np_hip_index_update_append(path.c_str(), docs.embeddings, docs.doc_lengths.data(), (int64_t)docs.doc_lengths.size(),
                                     (int32_t)docs.dim, &c, device, &r));
    if (report) *report = r;
    const detail::AppendedTokens t = detail::appended_tokens(path, before);
    put(t);
    return update_ids(r, docs.doc_lengths.size());
  }

 public:
  // ---- expand the RESIDENT index (np_hip_index_expand): new_centroids [k_new][dim] join the codec as centroids K .., the first
  // n_replace of the given documents REPLACE the handle's last n_replace documents (same ids) and the others take the ids
  // num_documents() .. -- the crate's update in expansion mode, on the handle, in one exclusive section.  codes lie in
  // [0, K + k_new).  The handle then equals one freshly opened on the resulting index; columns, keyword index and groups are
  // dropped.  Returns the given documents' ids, the replaced ones first.
  std::vector<int64_t> expand_arrays(const float* new_centroids, int64_t k_new, const std::vector<int64_t>& doc_lengths, const int64_t* codes,
                                     const uint8_t* residuals, int64_t n_replace = 0) {
    require_device("expand_arrays");
    const int64_t first = info_.num_documents - std::max<int64_t>(n_replace, 0);
    check(np_hip_index_expand(h_, new_centroids, k_new, n_replace, doc_lengths.data(), (int64_t)doc_lengths.size(), codes, residuals));
    check(np_hip_index_info(h_, &info_));
    std::vector<int64_t> ids(doc_lengths.size());
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = first + (int64_t)i;
    return ids;
  }
  // ... with the rows of the doc_lengths.size() - n_replace NEW documents (np_hip_index_expand_rows): the replaced documents keep
  // their rows, columns and groups stay attached; everything else as append_arrays with rows
  std::vector<int64_t> expand_arrays(const float* new_centroids, int64_t k_new, const std::vector<int64_t>& doc_lengths, const int64_t* codes,
                                     const uint8_t* residuals, int64_t n_replace, const AppendedRows& rows) {
    require_device("expand_arrays");
    const size_t n_new = doc_lengths.size() - (size_t)std::min<int64_t>(std::max<int64_t>(n_replace, 0), (int64_t)doc_lengths.size());
    std::vector<np_column> c;
    for (const ColumnSpan& s : rows.columns) {
      if (s.size != n_new) throw Error(NP_ERR_SHAPE, "Shape error: a column needs one new entry per new document");
      c.push_back(np_column{s.type, 0, s.data, s.valid});
    }
    if (!rows.code_remap.empty() && rows.code_remap.size() != rows.columns.size())
      throw Error(NP_ERR_SHAPE, "Shape error: code_remap needs one entry per column, or none");
    if (!rows.groups.empty() && rows.groups.size() != n_new) throw Error(NP_ERR_SHAPE, "Shape error: groups needs one id per new document");
    const int64_t first = info_.num_documents - std::max<int64_t>(n_replace, 0);
    check(np_hip_index_expand_rows(h_, new_centroids, k_new, n_replace, doc_lengths.data(), (int64_t)doc_lengths.size(), codes, residuals,
                                   c.data(), (int32_t)c.size(), rows.code_remap.empty() ? nullptr : rows.code_remap.data(),
                                   rows.groups.empty() ? nullptr : rows.groups.data(), rows.n_groups));
    check(np_hip_index_info(h_, &info_));
    std::vector<int64_t> ids(doc_lengths.size());
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = first + (int64_t)i;
    return ids;
  }
  // update() on the handle's directory AND on the handle, without the reload: np_hip_index_update chooses the mode as the crate
  // does and the handle follows the report -- buffer mode: append_arrays of what the directory gained; expansion mode:
  // expand_arrays with the centroids.npy rows the update added, n_replace = the buffered documents it deleted from the tail and
  // the tokens the chunk files hold beyond the kept documents; start-from-scratch mode: reload().  The handle equals load() of
  // the directory afterwards.  update() itself still reloads.
  std::vector<int64_t> update_resident(const Documents& docs, const UpdateConfig& cfg = {}, const np_open_opts* opts = nullptr,
                                       np_update_report* report = nullptr) {
    require_device("update_resident");
    const detail::DirCounts before = detail::dir_counts(path);
    if (before.documents != info_.num_documents)
      throw Error(NP_ERR_INDEX_LOAD, "Index load failed: the handle is not current with its directory: reload()");
    check(np_hip_index_expand(h_, nullptr, 0, 0, nullptr, 0, nullptr, nullptr));   // the library's checks of the handle
    const np_update_config c = cfg.c();
    np_update_report r{};
    const int64_t n = (int64_t)docs.doc_lengths.size();
    check(np_hip_index_update(path.c_str(), docs.embeddings, docs.doc_lengths.data(), n, (int32_t)docs.dim, &c, opts ? opts->device : 0, &r));
    if (report) *report = r;
    if (r.mode == NP_UPDATE_NONE) return update_ids(r, docs.doc_lengths.size());
    if (r.mode == NP_UPDATE_SCRATCH) {
      reload(opts);
      return update_ids(r, docs.doc_lengths.size());
    }
    const detail::DirCounts after = detail::dir_counts(path);
    if (r.mode == NP_UPDATE_EXPAND) {
      const int64_t n_given = r.n_reindexed + n, n_replace = before.documents - (after.documents - n_given);
      if (n_replace < 0 || n_replace > n_given)
        throw Error(NP_ERR_INDEX_LOAD, "Index load failed: the directory gained another number of documents than the update wrote: reload()");
      const detail::AppendedTokens t = detail::tail_documents(path, n_given);
      int64_t cols = 0;
      const std::string cen = detail::npy_tail(path + "/centroids.npy", "<f4", 4, r.n_new_centroids, &cols);
      if (r.n_new_centroids > 0 && cols != info_.embedding_dim)
        throw Error(NP_ERR_INDEX_LOAD, "Index load failed: centroids.npy has another dim than the handle: reload()");
      (void)expand_arrays(reinterpret_cast<const float*>(cen.data()), r.n_new_centroids, t.doc_lengths, t.codes.data(), t.residuals.data(),
                          n_replace);
    } else {
      const detail::AppendedTokens t = detail::appended_tokens(path, before);
      (void)append_arrays(t.doc_lengths, t.codes.data(), t.residuals.data());
    }
    if (info_.num_documents != after.documents)
      throw Error(NP_ERR_INDEX_LOAD, "Index load failed: the directory gained another number of documents than the handle: reload()");
    return update_ids(r, docs.doc_lengths.size());
  }
  // room for this many MORE documents / tokens, so that later appends move no per-token array (without it every array grows
  // by allocate, copy, free: a peak of the largest array twice).  A service reserves right after load()
  void reserve(int64_t extra_docs, int64_t extra_tokens) {
    require_device("reserve");
    check(np_hip_index_reserve(h_, extra_docs, extra_tokens));
  }
  // (documents, tokens) the handle's arrays are allocated for
  std::pair<int64_t, int64_t> capacity() const {
    require_device("capacity");
    std::pair<int64_t, int64_t> c{0, 0};
    check(np_hip_index_capacity(h_, &c.first, &c.second));
    return c;
  }
  // MmapIndex::update_or_create (index.rs:1644-1673): created when metadata.json is absent, ids 0..n then
  static MmapIndex update_or_create(const Documents& docs, const std::string& index_path, std::vector<int64_t>* ids,
                                    const IndexConfig& icfg = {}, const UpdateConfig& ucfg = {},
                                    const np_open_opts* opts = nullptr) {
    if (std::FILE* f = std::fopen((index_path + "/metadata.json").c_str(), "rb")) {
      std::fclose(f);
      MmapIndex ix = load(index_path, opts);
      std::vector<int64_t> got = ix.update(docs, ucfg, opts);
      if (ids) *ids = std::move(got);
      return ix;
    }
    MmapIndex ix = create_with_kmeans(docs, index_path, icfg, opts);
    if (ids) *ids = update_ids(np_update_report{}, docs.doc_lengths.size());
    return ix;
  }
  // ---- remove from the RESIDENT index (np_hip_index_remove) -- where delete_documents() + reload() read the whole index
  // again, these cost one pass over the posting lists and one move of the tokens behind the first removed document.  The
  // semantics are delete_documents': ids outside the index are ignored, duplicates count once, the survivors are renumbered.
  // The handle then equals one freshly opened on the shrunk index; columns, keyword index and groups are dropped, as reload()
  // leaves a handle; capacity() does not shrink.  Unsharded handles.  keep_attachments goes through np_hip_index_remove_keep:
  // columns (with their dictionary text) and groups are compacted with the documents on the device and stay attached; the
  // keyword index is dropped by the library all the same -- update_text_index(base, {delete = the removed ids}) and set_text
  // bring it along.  The handle alone:
  int64_t remove_ids(const std::vector<int64_t>& doc_ids) { return remove_ids_by(np_hip_index_remove, doc_ids); }
  int64_t remove_ids(const std::vector<int64_t>& doc_ids, bool keep_attachments) {
    return keep_attachments ? remove_ids_by(np_hip_index_remove_keep, doc_ids) : remove_ids(doc_ids);
  }
  // A column / the groups as the handle holds them, read back from HBM (np_hip_index_get_column / _get_groups).  `data` takes
  // the rows' bytes (8 per row for I64 and F64, 4 for CODE), `valid` one byte per row (all 1 where the column has no bitmap)
  struct ColumnRows {
    int32_t type = 0;
    bool has_valid = false;
    std::vector<uint8_t> data, valid;
  };
  ColumnRows get_column(int column) const {
    require_device("get_column");
    ColumnRows r;
    int32_t has = 0;
    check(np_hip_index_get_column(h_, column, nullptr, nullptr, &r.type, &has));
    const size_t n = (size_t)(info_.shard_doc_end - info_.shard_doc_begin);
    r.data.resize(n * (r.type == NP_COL_CODE ? 4 : 8));
    r.valid.resize(n);
    check(np_hip_index_get_column(h_, column, r.data.data(), r.valid.data(), &r.type, &has));
    r.has_valid = has != 0;
    return r;
  }
  std::vector<int32_t> get_groups() const {
    require_device("get_groups");
    std::vector<int32_t> g((size_t)num_documents());
    check(np_hip_index_get_groups(h_, g.data()));
    return g;
  }
  // delete_documents() on the handle's directory AND np_hip_index_remove on the handle: it equals load() of the directory then
  int64_t remove(const std::vector<int64_t>& doc_ids) { return remove_by(np_hip_index_remove, doc_ids); }
  int64_t remove(const std::vector<int64_t>& doc_ids, bool keep_attachments) {
    return keep_attachments ? remove_by(np_hip_index_remove_keep, doc_ids) : remove(doc_ids);
  }

 private:
  // the two removes differ in the entry alone (a program that never keeps attachments never names the keeping entry)
  using RemoveEntry = int (*)(np_index*, const int64_t*, int64_t, int64_t*);
  int64_t remove_ids_by(RemoveEntry entry, const std::vector<int64_t>& doc_ids) {
    require_device("remove_ids");
    int64_t n = 0;
    check(entry(h_, doc_ids.data(), (int64_t)doc_ids.size(), &n));
    check(np_hip_index_info(h_, &info_));
    return n;
  }
  int64_t remove_by(RemoveEntry entry, const std::vector<int64_t>& doc_ids) {
    require_device("remove");
    // whatever would refuse the handle's half is found BEFORE the directory is touched: a handle that is not current with its
    // directory, and (a remove of no ids runs the library's checks of the handle: shards)
    const detail::DirCounts before = detail::dir_counts(path);
    if (before.documents != info_.num_documents)
      throw Error(NP_ERR_INDEX_LOAD, "Index load failed: the handle is not current with its directory: reload()");
    check(entry(h_, nullptr, 0, nullptr));
    int64_t n = 0;
    check(np_hip_index_delete(path.c_str(), doc_ids.data(), (int64_t)doc_ids.size(), &n));
    const int64_t m = remove_ids_by(entry, doc_ids);
    if (m != n) throw Error(NP_ERR_INDEX_LOAD, "Index load failed: the directory lost another number of documents than the handle: reload()");
    return n;
  }

 public:
  // MmapIndex::delete (delete.rs:43-268): the count removed; no reload, as the crate (ids outside the index are ignored).
  // remove() does the same and brings the handle along
  int64_t delete_documents(const std::vector<int64_t>& doc_ids) {
    check_abi();
    int64_t n = 0;
    check(np_hip_index_delete(path.c_str(), doc_ids.data(), (int64_t)doc_ids.size(), &n));
    return n;
  }
  bool on_device() const { return h_ != nullptr; }
  MmapIndex(MmapIndex&& o) noexcept : path(std::move(o.path)), h_(o.h_), info_(o.info_) { o.h_ = nullptr; }
  MmapIndex& operator=(MmapIndex&& o) noexcept {
    if (this != &o) {
      close();
      h_ = o.h_;
      o.h_ = nullptr;
      path = std::move(o.path);
      info_ = o.info_;
    }
    return *this;
  }
  MmapIndex(const MmapIndex&) = delete;
  MmapIndex& operator=(const MmapIndex&) = delete;
  ~MmapIndex() { close(); }

  // index.rs:1258-1265
  QueryResult search(const float* query, size_t n_tokens, const SearchParameters& params,
                     const std::vector<int64_t>* subset = nullptr) const {
    Query q{query, n_tokens};
    auto r = search_batch(&q, 1, params, /*parallel=*/false, subset);
    r[0].query_id = 0;
    return std::move(r[0]);
  }

  // index.rs:1279-1287 -> search.rs:643-675.  `parallel` keeps the reference's error policy: with
  // parallel = true a failing search yields empty results instead of an error (search.rs:656-660).
  std::vector<QueryResult> search_batch(const Query* queries, size_t n, const SearchParameters& params, bool parallel,
                                        const std::vector<int64_t>* subset = nullptr) const {
    return run_batch(
        queries, n, params, parallel,
        [&](const float* flat, const int32_t* off, const np_search_params* p, int64_t* ids, float* sc, int32_t* cnt) {
          return np_hip_search_batch(h_, flat, off, (int32_t)n, (int32_t)embedding_dim(), p, subset ? subset->data() : nullptr,
                                     subset ? (int64_t)subset->size() : -1, ids, sc, cnt, &last_stats);
        },
        [&] { return cpu_search(queries, n, params, parallel, subset); });
  }

  // One subset per query (np_hip_search_batch_subsets): subsets[i] is query i's, or nullptr for none; query i gets what
  // search(queries[i], params, subsets[i]) returns.  Entries that point to the SAME vector share one subset (its bitmaps are
  // built once); contents are never compared.  The CPU fallback takes one subset per call: it is called once per query.
  std::vector<QueryResult> search_batch_subsets(const Query* queries, size_t n, const SearchParameters& params, bool parallel,
                                                const std::vector<const std::vector<int64_t>*>& subsets) const {
    const SubsetArgs s(subsets, n, "search_batch_subsets", /*empty_is_none=*/false);
    return run_batch(
        queries, n, params, parallel,
        [&](const float* flat, const int32_t* off, const np_search_params* p, int64_t* ids, float* sc, int32_t* cnt) {
          return np_hip_search_batch_subsets(h_, flat, off, (int32_t)n, (int32_t)embedding_dim(), p, s.sids.data(), s.soff.data(),
                                             (int64_t)s.n_distinct, s.qsub.data(), ids, sc, cnt, &last_stats);
        },
        [&] {
          std::vector<QueryResult> out;
          for (size_t i = 0; i < n; ++i) {
            auto r = cpu_search(queries + i, 1, params, parallel, subsets[i]);
            QueryResult one;   // a hook that answers a failed query with nothing: an empty result (search.rs:656-660)
            if (!r.empty()) one = std::move(r[0]);
            one.query_id = i;
            out.push_back(std::move(one));
          }
          return out;
        });
  }

  // The exact answer (np_hip_search_exact; the crate has no counterpart, so there is no CPU hand-off): for every query the
  // true top_k of its scope by exact MaxSim, every document scored.  precision 0 = exact f32, 3 = bf16 MFMA.  Scores that are
  // bit-equal come back by ascending id.  `subset`: one scope for the whole batch (nullptr: every document).
  std::vector<QueryResult> search_exact(const Query* queries, size_t n, size_t top_k, int precision = 0,
                                        const std::vector<int64_t>* subset = nullptr) const {
    return search_exact_subsets(queries, n, top_k, precision, std::vector<const std::vector<int64_t>*>(n, subset));
  }
  // ... with one scope per query, as search_batch_subsets takes them
  std::vector<QueryResult> search_exact_subsets(const Query* queries, size_t n, size_t top_k, int precision,
                                                const std::vector<const std::vector<int64_t>*>& subsets) const {
    require_device("search_exact");
    const SubsetArgs s(subsets, n, "search_exact_subsets", /*empty_is_none=*/false);
    const PackedQueries q = pack_queries(queries, n);
    RowBuffers b(n, std::max<size_t>(top_k, 1));
    check(np_hip_search_exact(h_, q.flat.data(), q.off.data(), (int32_t)n, (int32_t)embedding_dim(), (int32_t)top_k, (int32_t)precision,
                              s.sids.data(), s.soff.data(), (int64_t)s.n_distinct, s.qsub.data(), b.ids.data(), b.sc.data(),
                              b.cnt.data(), &last_stats));
    return b.rows(n);
  }

  // Metadata columns (np_hip_index_set_columns): replaces any earlier set, an empty vector drops them.  Every span covers
  // the whole index.  Needs exclusive access to the handle.  reload() / update() leave a handle without columns.
  void set_columns(const std::vector<ColumnSpan>& columns) {
    require_device("set_columns");
    std::vector<np_column> c;
    for (const ColumnSpan& s : columns) {
      if (s.size != num_documents()) throw Error(NP_ERR_SHAPE, "Shape error: a column needs one entry per document");
      c.push_back(np_column{s.type, 0, s.data, s.valid});
    }
    check(np_hip_index_set_columns(h_, c.data(), (int32_t)c.size()));
    check(np_hip_index_info(h_, &info_));
  }

  // The dictionary strings of a CODE column in HBM (np_hip_index_set_column_text): string c is the text of code c.  An empty
  // vector drops the text; set_columns() drops it with the columns.  Needs exclusive access to the handle.
  void set_column_text(int column, const std::vector<std::string>& dictionary) {
    require_device("set_column_text");
    std::vector<int64_t> off(dictionary.size() + 1, 0);
    std::string bytes;
    for (size_t i = 0; i < dictionary.size(); ++i) {
      bytes += dictionary[i];
      off[i + 1] = (int64_t)bytes.size();
    }
    check(np_hip_index_set_column_text(h_, column, (const uint8_t*)bytes.data(), off.data(), (int64_t)dictionary.size()));
    check(np_hip_index_info(h_, &info_));
  }

  // Which of a column's n_strings dictionary strings every DFA accepts (np_hip_text_match): out[d][c] for DFA d and code c.
  std::vector<std::vector<bool>> text_match(int column, const std::vector<Dfa>& dfas, size_t n_strings,
                                            np_match_report* report = nullptr) const {
    require_device("text_match");
    std::vector<np_dfa> d;
    for (const Dfa& x : dfas) d.push_back(x.c());
    const size_t nw = (n_strings + 31) / 32;
    std::vector<uint32_t> bits(std::max<size_t>(dfas.size() * nw, 1), 0u);
    check(np_hip_text_match(h_, column, d.data(), (int32_t)d.size(), bits.data(), report));
    std::vector<std::vector<bool>> out(dfas.size(), std::vector<bool>(n_strings));
    for (size_t j = 0; j < dfas.size(); ++j)
      for (size_t c = 0; c < n_strings; ++c) out[j][c] = (bits[j * nw + c / 32] >> (c & 31)) & 1u;
    return out;
  }

  // The global ids every filter selects among this handle's documents, ascending (np_hip_filter_eval).
  std::vector<std::vector<int64_t>> filter_ids(const std::vector<FilterProgram>& filters) const {
    require_device("filter_ids");
    const std::vector<np_filter> f = c_filters(filters);
    std::vector<int64_t> off(filters.size() + 1, 0);
    check(np_hip_filter_eval(h_, f.data(), (int32_t)f.size(), nullptr, 0, off.data()));
    std::vector<int64_t> ids(std::max<size_t>((size_t)off.back(), 1));
    check(np_hip_filter_eval(h_, f.data(), (int32_t)f.size(), ids.data(), (int64_t)ids.size(), off.data()));
    std::vector<std::vector<int64_t>> out(filters.size());
    for (size_t j = 0; j < filters.size(); ++j) out[j].assign(ids.begin() + off[j], ids.begin() + off[j + 1]);
    return out;
  }

  // search_batch_subsets with the subsets computed on the device (np_hip_search_batch_filtered): query i takes
  // filters[query_filter[i]], -1 = none, and gets what the subsets call returns for the ids that filter selects, ascending.
  // Filters have no CPU hand-off: a missing device is an Error.
  std::vector<QueryResult> search_batch_filtered(const Query* queries, size_t n, const SearchParameters& params, bool parallel,
                                                 const std::vector<FilterProgram>& filters,
                                                 const std::vector<int32_t>& query_filter) const {
    require_device("search_batch_filtered");
    if (query_filter.size() != n) throw Error(NP_ERR_INVALID_ARGUMENT, "search_batch_filtered: one query_filter entry per query");
    const std::vector<np_filter> f = c_filters(filters);
    return run_batch(
        queries, n, params, parallel,
        [&](const float* flat, const int32_t* off, const np_search_params* p, int64_t* ids, float* sc, int32_t* cnt) {
          return np_hip_search_batch_filtered(h_, flat, off, (int32_t)n, (int32_t)embedding_dim(), p, f.data(), (int32_t)f.size(),
                                              query_filter.data(), ids, sc, cnt, &last_stats);
        },
        [&]() -> std::vector<QueryResult> {
          throw Error(NP_ERR_DEVICE_UNAVAILABLE, "search_batch_filtered: filters are evaluated on the device; no CPU hand-off");
        });
  }

  // ... and the exact scan over each query's filter (np_hip_search_exact_filtered)
  std::vector<QueryResult> search_exact_filtered(const Query* queries, size_t n, size_t top_k, int precision,
                                                 const std::vector<FilterProgram>& filters,
                                                 const std::vector<int32_t>& query_filter) const {
    require_device("search_exact_filtered");
    if (query_filter.size() != n) throw Error(NP_ERR_INVALID_ARGUMENT, "search_exact_filtered: one query_filter entry per query");
    const std::vector<np_filter> f = c_filters(filters);
    const PackedQueries q = pack_queries(queries, n);
    RowBuffers b(n, std::max<size_t>(top_k, 1));
    check(np_hip_search_exact_filtered(h_, q.flat.data(), q.off.data(), (int32_t)n, (int32_t)embedding_dim(), (int32_t)top_k,
                                       (int32_t)precision, f.data(), (int32_t)f.size(), query_filter.data(), b.ids.data(),
                                       b.sc.data(), b.cnt.data(), &last_stats));
    return b.rows(n);
  }

  // The keyword index (np_hip_index_set_text): replaces any earlier one, nullptr drops it.  Needs exclusive access to the
  // handle.  reload() / update() leave a handle without one.
  void set_text(const TextIndexSpan* t) {
    require_device("set_text");
    if (t) {
      const np_text_index c{(int64_t)t->n_terms, t->term_offsets, t->inst_doc, t->inst_pos, t->n_rows};
      check(np_hip_index_set_text(h_, &c));
    } else {
      check(np_hip_index_set_text(h_, nullptr));
    }
    check(np_hip_index_info(h_, &info_));
  }

  // BM25 keyword search with SQLite FTS5's results (np_hip_text_search; text_search.rs:1246-1342): per query the top_k
  // documents by -bm25(), ties by ascending id.  One scope per query as search_exact_subsets takes them (an empty vector of
  // subsets: none).  No CPU hand-off: the crate's CPU path is SQLite itself.
  std::vector<QueryResult> text_search(const std::vector<TextQuery>& queries, size_t top_k,
                                       const std::vector<const std::vector<int64_t>*>& subsets = {}) const {
    require_device("text_search");
    const size_t n = queries.size();
    const SubsetArgs s(subsets, n, "text_search");
    const std::vector<np_text_query> tq = c_text_queries(queries);
    RowBuffers b(n, std::max<size_t>(top_k, 1));
    check(np_hip_text_search(h_, tq.data(), (int32_t)n, (int32_t)top_k, s.sids.data(), s.soff.data(), (int64_t)s.n_distinct,
                             s.qsub.data(), b.ids.data(), b.sc.data(), b.cnt.data(), &last_stats));
    return b.rows(n);
  }

  // ... with tree queries (np_hip_text_search_expr): NOT, AND, OR, parentheses and prefixes as FTS5 reads them.
  std::vector<QueryResult> text_search(const std::vector<TextExpr>& queries, size_t top_k,
                                       const std::vector<const std::vector<int64_t>*>& subsets = {}) const {
    require_device("text_search");
    const size_t n = queries.size();
    const SubsetArgs s(subsets, n, "text_search");
    const std::vector<np_text_expr> tq = c_text_exprs(queries);
    RowBuffers b(n, std::max<size_t>(top_k, 1));
    check(np_hip_text_search_expr(h_, tq.data(), (int32_t)n, (int32_t)top_k, s.sids.data(), s.soff.data(), (int64_t)s.n_distinct,
                                  s.qsub.data(), b.ids.data(), b.sc.data(), b.cnt.data(), &last_stats));
    return b.rows(n);
  }

  // Fusion of per-query semantic and keyword lists (np_hip_fuse; text_search.rs:1006-1075): mode NP_FUSE_RRF or
  // NP_FUSE_RELATIVE_SCORE, f32 in the reference's order; fused score descending, ties by ascending id.
  std::vector<QueryResult> fuse(int mode, float alpha, size_t top_k, const std::vector<QueryResult>& sem,
                                const std::vector<QueryResult>& kw) const {
    require_device("fuse");
    const size_t n = sem.size();
    if (kw.size() != n) throw Error(NP_ERR_INVALID_ARGUMENT, "fuse: one keyword list per semantic list");
    const PaddedLists s(sem), w(kw);
    RowBuffers b(n, std::max<size_t>(top_k, 1));
    check(np_hip_fuse(h_, mode, alpha, (int32_t)top_k, (int32_t)n, s.ids.data(), s.sc.data(), s.cnt.data(), (int32_t)s.stride,
                      w.ids.data(), w.sc.data(), w.cnt.data(), (int32_t)w.stride, b.ids.data(), b.sc.data(), b.cnt.data()));
    return b.rows(n);
  }

  // The /search handler's hybrid request in one call (np_hip_search_hybrid): the semantic and the keyword pass with
  // top_k = fetch_k (0: the handler's 3 * params.top_k) and their fusion to params.top_k, all on the device.
  std::vector<QueryResult> search_hybrid(const Query* queries, const std::vector<TextQuery>& text_queries, const SearchParameters& params,
                                         float alpha = 0.75f, int fusion = NP_FUSE_RELATIVE_SCORE, size_t fetch_k = 0,
                                         const std::vector<const std::vector<int64_t>*>& subsets = {}) const {
    require_device("search_hybrid");
    const size_t n = text_queries.size();
    const SubsetArgs s(subsets, n, "search_hybrid");
    const std::vector<np_text_query> tq = c_text_queries(text_queries);
    const PackedQueries q = pack_queries(queries, n);
    const np_search_params p = params.c();
    RowBuffers b(n, std::max<size_t>(params.top_k, 1));
    check(np_hip_search_hybrid(h_, q.flat.data(), q.off.data(), (int32_t)n, (int32_t)embedding_dim(), &p, tq.data(),
                               (int32_t)(fetch_k ? fetch_k : 3 * params.top_k), alpha, fusion, s.sids.data(), s.soff.data(),
                               (int64_t)s.n_distinct, s.qsub.data(), nullptr, 0, b.ids.data(), b.sc.data(), b.cnt.data(),
                               &last_stats));
    return b.rows(n);
  }

  // ... with tree queries (np_hip_search_hybrid_expr)
  std::vector<QueryResult> search_hybrid(const Query* queries, const std::vector<TextExpr>& text_queries, const SearchParameters& params,
                                         float alpha = 0.75f, int fusion = NP_FUSE_RELATIVE_SCORE, size_t fetch_k = 0,
                                         const std::vector<const std::vector<int64_t>*>& subsets = {}) const {
    require_device("search_hybrid");
    const size_t n = text_queries.size();
    const SubsetArgs s(subsets, n, "search_hybrid");
    const std::vector<np_text_expr> tq = c_text_exprs(text_queries);
    const PackedQueries q = pack_queries(queries, n);
    const np_search_params p = params.c();
    RowBuffers b(n, std::max<size_t>(params.top_k, 1));
    check(np_hip_search_hybrid_expr(h_, q.flat.data(), q.off.data(), (int32_t)n, (int32_t)embedding_dim(), &p, tq.data(),
                                    (int32_t)(fetch_k ? fetch_k : 3 * params.top_k), alpha, fusion, s.sids.data(), s.soff.data(),
                                    (int64_t)s.n_distinct, s.qsub.data(), nullptr, 0, b.ids.data(), b.sc.data(), b.cnt.data(),
                                    &last_stats));
    return b.rows(n);
  }

  // ---- grouped search (np_hip_index_set_groups and its kin; ColGREP's collapse_by_file on the device) -----------------------
  // One group of a grouped result: its id, its first documents in list order (at most group_size) with their scores, and the
  // number of the list's entries that belong to it (total - passage_ids.size() were folded).
  struct Group {
    int32_t group_id = 0;
    std::vector<int64_t> passage_ids;
    std::vector<float> scores;   // empty where the collapsed list had none
    int32_t total = 0;
  };
  using GroupedResult = std::vector<Group>;   // of one query, in order of admission

  // The group of every document of the WHOLE index: dense ids in [0, n_groups), kept in HBM.  An empty vector drops them.
  // Needs exclusive access to the handle; a sharded handle is refused.  reload() / update() leave a handle without groups, as
  // they leave it without columns.
  void set_groups(const std::vector<int32_t>& group_ids, int64_t n_groups) {
    require_device("set_groups");
    check(np_hip_index_set_groups(h_, group_ids.empty() ? nullptr : group_ids.data(), (int64_t)group_ids.size(), n_groups));
    check(np_hip_index_info(h_, &info_));
  }
  int64_t group_count() const { return h_ ? np_hip_index_group_count(h_) : 0; }

  // np_hip_collapse: each ranked list walked to top_k groups of at most group_size documents.  with_scores = false passes no
  // scores (the walk never reads one).
  std::vector<GroupedResult> collapse(const std::vector<QueryResult>& lists, size_t top_k, size_t group_size,
                                      bool with_scores = true) const {
    require_device("collapse");
    const size_t n = lists.size();
    const PaddedLists l(lists);
    GroupBuffers b(n, top_k, group_size);
    check(np_hip_collapse(h_, (int32_t)top_k, (int32_t)group_size, (int32_t)n, l.ids.data(), with_scores ? l.sc.data() : nullptr,
                          l.cnt.data(), (int32_t)l.stride, b.ids.data(), with_scores ? b.sc.data() : nullptr, b.group.data(),
                          b.members.data(), b.total.data(), b.cnt.data()));
    return b.groups(n, with_scores);
  }

  // np_hip_search_batch_grouped: the top params.top_k GROUPS with their best group_size documents -- the search pass with
  // top_k = pool_k (0: ColGREP's max(20 top_k, 200), inside the index and the limit of 16384) and the collapse of its lists,
  // on the device.  Query i gets collapse(search_batch(top_k = pool_k)).  One scope per query as search_hybrid takes them.
  std::vector<GroupedResult> search_grouped(const Query* queries, size_t n, const SearchParameters& params, size_t group_size = 1,
                                            size_t pool_k = 0,
                                            const std::vector<const std::vector<int64_t>*>& subsets = {}) const {
    require_device("search_grouped");
    const SubsetArgs s(subsets, n, "search_grouped");
    const PackedQueries q = pack_queries(queries, n);
    const np_search_params p = params.c();
    GroupBuffers b(n, params.top_k, group_size);
    check(np_hip_search_batch_grouped(h_, q.flat.data(), q.off.data(), (int32_t)n, (int32_t)embedding_dim(), &p, s.sids.data(),
                                      s.soff.data(), (int64_t)s.n_distinct, s.qsub.data(), nullptr, 0,
                                      (int32_t)(pool_k ? pool_k : default_pool_k(params.top_k, NP_GROUP_MAX_LIST)), (int32_t)group_size,
                                      b.ids.data(), b.sc.data(), b.group.data(), b.members.data(), b.total.data(), b.cnt.data(),
                                      &last_stats));
    return b.groups(n, true);
  }

  // np_hip_search_hybrid_grouped: ColGREP's request -- search_hybrid fused into a pool of pool_k (0: the default above, inside
  // the fusion's limit of 2 * NP_TEXT_MAX_TOPK), then collapsed to params.top_k groups.  fetch_k 0: min(3 * pool_k, 1024).
  std::vector<GroupedResult> search_hybrid_grouped(const Query* queries, const std::vector<TextQuery>& text_queries,
                                                   const SearchParameters& params, size_t group_size = 1, size_t pool_k = 0,
                                                   float alpha = 0.75f, int fusion = NP_FUSE_RELATIVE_SCORE, size_t fetch_k = 0,
                                                   const std::vector<const std::vector<int64_t>*>& subsets = {}) const {
    require_device("search_hybrid_grouped");
    const size_t n = text_queries.size();
    const SubsetArgs s(subsets, n, "search_hybrid_grouped");
    const std::vector<np_text_query> tq = c_text_queries(text_queries);
    const PackedQueries q = pack_queries(queries, n);
    const np_search_params p = params.c();
    const size_t pk = pool_k ? pool_k : default_pool_k(params.top_k, 2 * NP_TEXT_MAX_TOPK);
    const size_t fk = fetch_k ? fetch_k : std::min<size_t>(3 * pk, NP_TEXT_MAX_TOPK);
    GroupBuffers b(n, params.top_k, group_size);
    check(np_hip_search_hybrid_grouped(h_, q.flat.data(), q.off.data(), (int32_t)n, (int32_t)embedding_dim(), &p, tq.data(), (int32_t)fk,
                                       alpha, fusion, s.sids.data(), s.soff.data(), (int64_t)s.n_distinct, s.qsub.data(), nullptr, 0,
                                       (int32_t)pk, (int32_t)group_size, b.ids.data(), b.sc.data(), b.group.data(), b.members.data(),
                                       b.total.data(), b.cnt.data(), &last_stats));
    return b.groups(n, true);
  }

  // Given pairs with the per-token matches (np_hip_score_pairs; no crate counterpart, no CPU hand-off): query i against the
  // documents doc_ids[i] (global ids; duplicates allowed).  scores[p] is the S6 score of the pair -- the bits search_batch and
  // search_exact give it at precision 0 -- and, with return_matches, token_sims / token_pos hold one row of n_tokens entries
  // per pair: each query token's best similarity (-inf: none finite) and the lowest document-token index that reaches it (-1).
  struct PairScores {
    std::vector<float> scores;        // [n_i]
    std::vector<float> token_sims;    // [n_i][n_tokens of query i], or empty
    std::vector<int32_t> token_pos;   // ...
  };
  std::vector<PairScores> score_pairs(const Query* queries, size_t n, const std::vector<std::vector<int64_t>>& doc_ids,
                                      bool return_matches = true, int precision = 0) const {
    require_device("score_pairs");
    if (doc_ids.size() != n) throw Error(NP_ERR_INVALID_ARGUMENT, "score_pairs: one list of document ids per query");
    const PackedQueries q = pack_queries(queries, n);
    std::vector<int64_t> poff(n + 1, 0), roff(n + 1, 0), ids;
    for (size_t i = 0; i < n; ++i) {
      poff[i + 1] = poff[i] + (int64_t)doc_ids[i].size();
      roff[i + 1] = roff[i] + (int64_t)(doc_ids[i].size() * queries[i].n_tokens);
      ids.insert(ids.end(), doc_ids[i].begin(), doc_ids[i].end());
    }
    std::vector<float> sc(std::max<size_t>((size_t)poff[n], 1)), sims(return_matches ? std::max<size_t>((size_t)roff[n], 1) : 0);
    std::vector<int32_t> pos(sims.size());
    ids.resize(std::max<size_t>(ids.size(), 1));
    check(np_hip_score_pairs(h_, q.flat.data(), q.off.data(), (int32_t)n, (int32_t)embedding_dim(), (int32_t)precision, ids.data(),
                             poff.data(), sc.data(), return_matches ? sims.data() : nullptr, return_matches ? pos.data() : nullptr,
                             &last_stats));
    std::vector<PairScores> out(n);
    for (size_t i = 0; i < n; ++i) {
      out[i].scores.assign(sc.begin() + poff[i], sc.begin() + poff[i + 1]);
      if (return_matches) {
        out[i].token_sims.assign(sims.begin() + roff[i], sims.begin() + roff[i + 1]);
        out[i].token_pos.assign(pos.begin() + roff[i], pos.begin() + roff[i + 1]);
      }
    }
    return out;
  }

 private:
  // One subset entry per query -> the CSR arguments of the per-query-subset entry points.  Entries that point to the SAME
  // vector share one subset; contents are never compared.  Returns the number of distinct subsets.
  static size_t pack_subsets(const std::vector<const std::vector<int64_t>*>& subsets, std::vector<int32_t>& qsub,
                             std::vector<int64_t>& soff, std::vector<int64_t>& sids) {
    std::vector<const std::vector<int64_t>*> distinct;
    qsub.assign(subsets.size(), -1);
    for (size_t i = 0; i < subsets.size(); ++i) {
      if (!subsets[i]) continue;
      size_t j = 0;
      while (j < distinct.size() && distinct[j] != subsets[i]) ++j;
      if (j == distinct.size()) distinct.push_back(subsets[i]);
      qsub[i] = (int32_t)j;
    }
    soff.assign(distinct.size() + 1, 0);
    sids.clear();
    for (size_t j = 0; j < distinct.size(); ++j) {
      sids.insert(sids.end(), distinct[j]->begin(), distinct[j]->end());
      soff[j + 1] = (int64_t)sids.size();
    }
    return distinct.size();
  }

  // One scope per query as the entries take it (CallSubsets on the C side): the CSR of the distinct subsets and the
  // queries' map into them.  An empty vector of subsets means none (where the method allows it: empty_is_none); otherwise
  // there is one entry per query, or the error names the method.
  struct SubsetArgs {
    std::vector<int32_t> qsub;
    std::vector<int64_t> soff, sids;
    size_t n_distinct = 0;
    SubsetArgs(const std::vector<const std::vector<int64_t>*>& subsets, size_t n, const char* what, bool empty_is_none = true) {
      if (empty_is_none && subsets.empty()) return;
      if (subsets.size() != n) throw Error(NP_ERR_INVALID_ARGUMENT, (std::string(what) + ": one subset entry per query").c_str());
      n_distinct = pack_subsets(subsets, qsub, soff, sids);
    }
  };

  static std::vector<np_filter> c_filters(const std::vector<FilterProgram>& filters) {
    std::vector<np_filter> f;
    for (const FilterProgram& p : filters) f.push_back(p.c());
    return f;
  }
  static std::vector<np_text_query> c_text_queries(const std::vector<TextQuery>& queries) {
    std::vector<np_text_query> q;
    for (const TextQuery& t : queries) q.push_back(t.c());
    return q;
  }

  static std::vector<np_text_expr> c_text_exprs(const std::vector<TextExpr>& queries) {
    std::vector<np_text_expr> q;
    for (const TextExpr& t : queries) q.push_back(t.c());
    return q;
  }

  // Ranked lists (the inputs of fuse and collapse) as [n][stride] ids and scores and [n] counts, zero-padded
  struct PaddedLists {
    size_t stride = 1;
    std::vector<int64_t> ids;
    std::vector<float> sc;
    std::vector<int32_t> cnt;
    explicit PaddedLists(const std::vector<QueryResult>& l) {
      const size_t n = l.size();
      for (const QueryResult& r : l) stride = std::max(stride, r.passage_ids.size());
      ids.assign(std::max<size_t>(n, 1) * stride, 0);
      sc.assign(std::max<size_t>(n, 1) * stride, 0.f);
      cnt.assign(std::max<size_t>(n, 1), 0);
      for (size_t i = 0; i < n; ++i) {
        std::copy(l[i].passage_ids.begin(), l[i].passage_ids.end(), ids.begin() + i * stride);
        std::copy(l[i].scores.begin(), l[i].scores.end(), sc.begin() + i * stride);
        cnt[i] = (int32_t)l[i].passage_ids.size();
      }
    }
  };

  // The flat [sum n_tokens][dim] queries and their [n + 1] token offsets (never empty: padded to one float)
  struct PackedQueries {
    std::vector<int32_t> off;
    std::vector<float> flat;
  };
  PackedQueries pack_queries(const Query* queries, size_t n) const {
    const size_t dim = embedding_dim();
    PackedQueries q;
    q.off.assign(n + 1, 0);
    for (size_t i = 0; i < n; ++i) q.off[i + 1] = q.off[i] + (int32_t)queries[i].n_tokens;
    q.flat.assign(std::max<size_t>((size_t)q.off[n] * dim, 1), 0.f);
    for (size_t i = 0; i < n; ++i)
      std::copy(queries[i].data, queries[i].data + queries[i].n_tokens * dim, q.flat.begin() + (size_t)q.off[i] * dim);
    return q;
  }

  // The [n][k] ids and scores and the [n] counts a search entry fills (ResultStage on the C side), never empty, and their
  // unpacking.  k is the caller's: max(top_k, 1) everywhere but in run_batch.
  struct RowBuffers {
    size_t k;
    std::vector<int64_t> ids;
    std::vector<float> sc;
    std::vector<int32_t> cnt;
    RowBuffers(size_t n, size_t k_) : k(k_), ids(std::max<size_t>(n * k, 1)), sc(std::max<size_t>(n * k, 1)), cnt(std::max<size_t>(n, 1)) {}
    std::vector<QueryResult> rows(size_t n) const {
      std::vector<QueryResult> out(n);
      for (size_t i = 0; i < n; ++i) {
        out[i].query_id = i;
        out[i].passage_ids.assign(ids.begin() + i * k, ids.begin() + i * k + cnt[i]);
        out[i].scores.assign(sc.begin() + i * k, sc.begin() + i * k + cnt[i]);
      }
      return out;
    }
  };

  // ColGREP's over-fetch for top_k groups, inside what the index holds and the entry's limit
  size_t default_pool_k(size_t top_k, size_t limit) const {
    const size_t want = std::max<size_t>(20 * top_k, 200), have = std::max<size_t>(num_documents(), top_k);
    return std::max<size_t>(1, std::min(std::min(want, have), limit));
  }

  // the padded outputs of a grouped call, and their unpacking
  struct GroupBuffers {
    size_t k, g;
    std::vector<int64_t> ids;
    std::vector<float> sc;
    std::vector<int32_t> group, members, total, cnt;
    GroupBuffers(size_t n, size_t top_k, size_t group_size)
        : k(std::max<size_t>(top_k, 1)), g(std::max<size_t>(group_size, 1)), ids(std::max<size_t>(n * k * g, 1)),
          sc(std::max<size_t>(n * k * g, 1)), group(std::max<size_t>(n * k, 1)), members(std::max<size_t>(n * k, 1)),
          total(std::max<size_t>(n * k, 1)), cnt(std::max<size_t>(n, 1)) {}
    std::vector<GroupedResult> groups(size_t n, bool with_scores) const {
      std::vector<GroupedResult> out(n);
      for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < (size_t)cnt[i]; ++j) {
          Group gr;
          gr.group_id = group[i * k + j];
          gr.total = total[i * k + j];
          const size_t at = (i * k + j) * g, m = (size_t)members[i * k + j];
          gr.passage_ids.assign(ids.begin() + at, ids.begin() + at + m);
          if (with_scores) gr.scores.assign(sc.begin() + at, sc.begin() + at + m);
          out[i].push_back(std::move(gr));
        }
      return out;
    }
  };

  // The body of every batch call: pack the queries, `call` the library, apply the error and fallback policy (`cpu`: this
  // batch on the CPU hand-off), unpack.
  template <class Call, class Cpu>
  std::vector<QueryResult> run_batch(const Query* queries, size_t n, const SearchParameters& params, bool parallel, Call&& call,
                                     Cpu&& cpu) const {
    if (!h_) return cpu();
    const PackedQueries q = pack_queries(queries, n);
    RowBuffers b(n, params.top_k);   // the crate's top_k as it is: top_k = 0 is a batch of empty results
    np_search_params p = params.c();
    int rc = call(q.flat.data(), q.off.data(), &p, b.ids.data(), b.sc.data(), b.cnt.data());
    if (rc != NP_OK) {
      if (is_device_failure(rc)) {   // mid-flight device loss: flag it, hand this call to the CPU unless FORCE_GPU
        if (rc == NP_ERR_DEVICE_UNAVAILABLE) mark_hip_broken();   // an OutOfMemory of one call leaves the device usable
        if (!is_force_gpu() && cpu_fallback()) return cpu();
      }
      if (parallel && rc == NP_ERR_SEARCH) return RowBuffers(n, 0).rows(n);   // n empty results (search.rs:656-660)
      check(rc);
    }
    for (size_t i = 0; i < n; ++i)
      // ABI v5: a negative count (NP_COUNT_ABANDONED) marks a batch a sharded peer abandoned -- never a length
      if (b.cnt[i] < 0) throw Error(NP_ERR_SEARCH, "Search failed: the batch was abandoned (a peer shard failed)");
    return b.rows(n);
  }

 public:
  // index.rs:1197-1245 decompress_documents: (embeddings [sum len, dim], lengths)
  std::pair<std::vector<float>, std::vector<int64_t>> decompress_documents(const std::vector<int64_t>& doc_ids) const {
    require_device("decompress_documents");
    std::vector<int64_t> lens(std::max<size_t>(doc_ids.size(), 1));
    check(np_hip_decompress_documents(h_, doc_ids.data(), (int64_t)doc_ids.size(), nullptr, 0, lens.data()));
    lens.resize(doc_ids.size());
    int64_t total = 0;
    for (int64_t l : lens) total += l;
    std::vector<float> emb((size_t)std::max<int64_t>(total, 1) * embedding_dim());
    check(np_hip_decompress_documents(h_, doc_ids.data(), (int64_t)doc_ids.size(), emb.data(), total, lens.data()));
    emb.resize((size_t)total * embedding_dim());
    return {std::move(emb), std::move(lens)};
  }

  // index.rs:289-371 encode_index_chunk for a flat [n, dim] batch: (codes, packed residuals [n, dim*nbits/8])
  std::pair<std::vector<int64_t>, std::vector<uint8_t>> encode_tokens(const float* embeddings, size_t n,
                                                                      const std::vector<float>& bucket_cutoffs) const {
    require_device("encode_tokens");
    const size_t pd = embedding_dim() * (size_t)info_.nbits / 8;
    std::vector<int64_t> codes(std::max<size_t>(n, 1));
    std::vector<uint8_t> packed(std::max<size_t>(n * pd, 1));
    if (bucket_cutoffs.size() + 1 != ((size_t)1 << info_.nbits)) throw Error(NP_ERR_CODEC, "Codec error: bucket_cutoffs size");
    check(np_hip_encode_tokens(h_, embeddings, (int64_t)n, (int32_t)embedding_dim(), bucket_cutoffs.data(), codes.data(),
                               packed.data()));
    codes.resize(n);
    packed.resize(n * pd);
    return {std::move(codes), std::move(packed)};
  }

  // index.rs:1290-1312
  size_t num_documents() const { return (size_t)info_.num_documents; }
  size_t num_embeddings() const { return (size_t)info_.num_embeddings; }
  size_t num_partitions() const { return (size_t)info_.num_partitions; }
  double avg_doclen() const { return info_.avg_doclen; }
  size_t embedding_dim() const { return (size_t)info_.embedding_dim; }
  const np_info& info() const { return info_; }
  np_index* handle() const { return h_; }
  // info() again from the library: after a call on handle() that changed what the handle holds (the resident keyword index)
  void refresh_info() {
    require_device("refresh_info");
    check(np_hip_index_info(h_, &info_));
  }

  std::string path;
  mutable np_stats last_stats{};
  size_t cpu_dim = 0;   // overrides the embedding dim handed to the CPU hook (0 = the index's own, from metadata)

 private:
  MmapIndex(np_index* h, std::string p) : path(std::move(p)), h_(h) {
    if (h_) check(np_hip_index_info(h_, &info_));
    // CPU hand-off mode: the geometry accessors (index.rs:1290-1312) stay valid -- host-only parse of the same directory
    else check(np_hip_index_probe_dir(path.c_str(), &info_));
  }
  void require_device(const char* what) const {
    if (!h_)
      throw Error(NP_ERR_DEVICE_UNAVAILABLE, (std::string(what) + ": this index runs on the CPU hand-off (no device handle)").c_str());
  }
  std::vector<QueryResult> cpu_search(const Query* queries, size_t n, const SearchParameters& params, bool parallel,
                                      const std::vector<int64_t>* subset) const {
    if (!cpu_fallback()) throw Error(NP_ERR_DEVICE_UNAVAILABLE, "HIP device unavailable and no CPU fallback installed");
    return cpu_fallback()(path, queries, n, cpu_dim ? cpu_dim : embedding_dim(), params, parallel, subset);
  }
  void close() {
    if (h_) np_hip_index_close(h_);
    h_ = nullptr;
  }
  np_index* h_ = nullptr;
  np_info info_{};
};

// index.rs:373-528 write_index_from_encoded_chunks: encoded chunks (flat here) -> an index directory in the crate's
// on-disk format.  Host only.  Posting lists are built from the codes (index.rs:479-504).
struct IndexFiles {
  size_t num_centroids = 0, dim = 0;
  int nbits = 4;
  const float* centroids = nullptr;            // [K, dim]
  std::vector<float> bucket_weights;           // [2^nbits]
  std::vector<float> bucket_cutoffs;           // [2^nbits - 1] or empty
  std::vector<float> avg_residual;             // [dim] or empty (zeros)
  float cluster_threshold = 0.f;
  std::vector<int64_t> doc_lengths;            // [N]
  const int64_t* codes = nullptr;              // [sum doc_lengths]
  const uint8_t* residuals = nullptr;          // [sum doc_lengths, dim * nbits / 8]
  size_t chunk_docs = 50000;                   // IndexConfig.batch_size (index.rs:92)
};
inline void write_index(const std::string& path, const IndexFiles& f) {
  if (f.bucket_weights.size() != ((size_t)1 << f.nbits)) throw Error(NP_ERR_CODEC, "Codec error: bucket_weights size");
  if (!f.bucket_cutoffs.empty() && f.bucket_cutoffs.size() + 1 != ((size_t)1 << f.nbits))
    throw Error(NP_ERR_CODEC, "Codec error: bucket_cutoffs size");
  if (!f.avg_residual.empty() && f.avg_residual.size() != f.dim) throw Error(NP_ERR_SHAPE, "Shape error: avg_residual size");
  np_index_arrays a{};
  a.num_documents_total = a.num_docs = (int64_t)f.doc_lengths.size();
  a.num_centroids = (int64_t)f.num_centroids;
  a.dim = (int32_t)f.dim;
  a.nbits = f.nbits;
  a.centroids = f.centroids;
  a.bucket_weights = f.bucket_weights.data();
  a.doc_lengths = f.doc_lengths.data();
  a.codes = f.codes;
  a.residuals = f.residuals;
  np_write_opts o{};
  o.chunk_docs = (int64_t)f.chunk_docs;
  o.bucket_cutoffs = f.bucket_cutoffs.empty() ? nullptr : f.bucket_cutoffs.data();
  o.avg_residual = f.avg_residual.empty() ? nullptr : f.avg_residual.data();
  o.cluster_threshold = f.cluster_threshold;
  check(np_hip_index_write_dir(path.c_str(), &a, &o));
}

// next-plaid-api handlers/rerank.rs:57-170: MaxSim of one query against caller-supplied document embeddings
// (document i = rows doc_tok_offsets[i] .. doc_tok_offsets[i+1] of `docs`).  Returns (order, scores).
inline std::pair<std::vector<int64_t>, std::vector<float>> rerank_maxsim(const float* query, size_t n_query_tokens,
                                                                         size_t dim, const float* docs,
                                                                         const std::vector<int64_t>& doc_tok_offsets,
                                                                         int device = 0) {
  const size_t n = doc_tok_offsets.empty() ? 0 : doc_tok_offsets.size() - 1;
  std::vector<float> scores(std::max<size_t>(n, 1));
  std::vector<int64_t> order(std::max<size_t>(n, 1));
  check(np_hip_rerank_maxsim(device, query, (int32_t)n_query_tokens, (int32_t)dim, docs, doc_tok_offsets.data(), (int64_t)n,
                             scores.data(), order.data()));
  scores.resize(n);
  order.resize(n);
  return {std::move(order), std::move(scores)};
}

// ---- token pooling: next-plaid-onnx src/lib.rs:1632-1643 pool_document_embeddings, :2249-2317, hierarchy.rs ------------
enum class PoolCut { Reference = 0, Distance = 1 };   // chain order (the crate) / stable order by merge distance (scipy, PyLate)

inline np_pool_opts pool_opts(size_t pool_factor, size_t protected_tokens, PoolCut cut, int64_t chunk_docs = 0) {
  np_pool_opts o{};
  o.pool_factor = (int32_t)pool_factor;
  o.protected_tokens = (int32_t)protected_tokens;
  o.cut_order = (int32_t)cut;
  o.chunk_docs = chunk_docs;
  return o;
}

// every document's token count after pooling (host only)
inline std::vector<int64_t> pooled_lengths(const std::vector<int64_t>& doc_lengths, size_t pool_factor,
                                           size_t protected_tokens = 1) {
  const np_pool_opts o = pool_opts(pool_factor, protected_tokens, PoolCut::Reference);
  std::vector<int64_t> out(doc_lengths.size());
  check(np_hip_pooled_lengths(doc_lengths.data(), (int64_t)doc_lengths.size(), &o, out.data()));
  return out;
}

struct PooledDocuments {
  std::vector<float> embeddings;       // every pooled document's rows concatenated
  std::vector<int64_t> doc_lengths;
  std::vector<int32_t> labels;         // per INPUT token (only with want_labels): 0 = protected / unchanged, 1.. = cluster
  np_pool_report report{};
};

inline PooledDocuments pool_document_embeddings(const Documents& docs, size_t pool_factor, size_t protected_tokens = 1,
                                                PoolCut cut = PoolCut::Reference, int device = 0, bool want_labels = false,
                                                int64_t chunk_docs = 0) {
  const np_pool_opts o = pool_opts(pool_factor, protected_tokens, cut, chunk_docs);
  const int64_t n = (int64_t)docs.doc_lengths.size();
  PooledDocuments r;
  r.doc_lengths = pooled_lengths(docs.doc_lengths, pool_factor, protected_tokens);
  int64_t rows = 0, tokens = 0;
  for (int64_t v : r.doc_lengths) rows += v;
  for (int64_t v : docs.doc_lengths) tokens += v;
  r.embeddings.resize((size_t)std::max<int64_t>(rows, 1) * docs.dim);
  if (want_labels) r.labels.resize((size_t)std::max<int64_t>(tokens, 1));
  check(np_hip_pool_documents(device, docs.embeddings, docs.doc_lengths.data(), n, (int32_t)docs.dim, &o, r.embeddings.data(),
                              rows, r.doc_lengths.data(), want_labels ? r.labels.data() : nullptr, nullptr, &r.report));
  r.embeddings.resize((size_t)rows * docs.dim);
  if (want_labels) r.labels.resize((size_t)tokens);
  return r;
}

// ---- the keyword index built on the device (np_hip_text_build): the arrays np_hip_index_set_text takes, from raw text ----
enum class Tokenizer { Unicode61 = NP_TOK_UNICODE61, Trigram = NP_TOK_TRIGRAM };

// Instances tokenised by the caller (this mirror has no SQLite): the terms in memcmp order, the shorter string first, and
// the instances sorted by (term, doc, pos), inst_term indexing `terms`.
struct TextInstances {
  std::vector<std::string> terms;
  std::vector<int32_t> inst_term;
  std::vector<int64_t> inst_doc;
  std::vector<int32_t> inst_pos;
};

struct BuiltTextIndex {
  std::vector<std::string> terms;          // term id -> term, in fts5vocab's order
  std::vector<int64_t> term_offsets;       // [n_terms + 1]
  std::vector<int64_t> inst_doc;
  std::vector<int32_t> inst_pos;
  int64_t n_rows = 0;
  std::vector<int64_t> fallback_docs;      // documents the device does not reproduce (non-ASCII, ...), ascending
  np_text_build_report report{};
};

namespace detail {
struct TextBuildHandle {
  np_text_build* h = nullptr;
  ~TextBuildHandle() { np_hip_text_build_free(h); }
};

inline void text_build_start(TextBuildHandle& b, const std::vector<std::string>& texts, const np_text_build_opts& o, int device,
                             BuiltTextIndex* r) {
  std::vector<int64_t> off(texts.size() + 1, 0);
  for (size_t i = 0; i < texts.size(); ++i) off[i + 1] = off[i] + (int64_t)texts[i].size();
  std::vector<uint8_t> raw((size_t)off.back());
  for (size_t i = 0; i < texts.size(); ++i) std::copy(texts[i].begin(), texts[i].end(), raw.begin() + off[i]);
  check(np_hip_text_build(device, raw.empty() ? nullptr : raw.data(), off.data(), (int64_t)texts.size(), &o, &b.h, &r->report));
  r->fallback_docs.resize((size_t)r->report.n_fallback);
  check(np_hip_text_build_fallback(b.h, r->fallback_docs.data(), nullptr));
}

inline void text_build_finish(TextBuildHandle& b, BuiltTextIndex* r) {
  int64_t n_terms = 0, n_bytes = 0, n_inst = 0;
  check(np_hip_text_build_sizes(b.h, &n_terms, &n_bytes, &n_inst, &r->n_rows));
  std::vector<uint8_t> tb((size_t)std::max<int64_t>(n_bytes, 1));
  std::vector<int64_t> tbo((size_t)n_terms + 1);
  r->term_offsets.resize((size_t)n_terms + 1);
  r->inst_doc.resize((size_t)n_inst);
  r->inst_pos.resize((size_t)n_inst);
  check(np_hip_text_build_fetch(b.h, tb.data(), tbo.data(), r->term_offsets.data(), r->inst_doc.data(), r->inst_pos.data()));
  r->terms.resize((size_t)n_terms);
  for (int64_t t = 0; t < n_terms; ++t) r->terms[(size_t)t].assign((const char*)tb.data() + tbo[(size_t)t], (size_t)(tbo[(size_t)t + 1] - tbo[(size_t)t]));
}
}  // namespace detail

inline np_text_build_opts text_build_opts(Tokenizer tokenizer, int32_t max_token_bytes = 0) {
  np_text_build_opts o{};
  o.tokenizer = (int32_t)tokenizer;
  o.max_token_bytes = max_token_bytes;
  return o;
}

// UTF-8 mode: the overloads below that take a `unicode_table` hand it to the library (np_text_build_opts.unicode_table:
// SQLite's unicode61 rule, one uint32 per code point of 1..17 planes), which then reproduces unicode61 for well-formed
// UTF-8 inside the table instead of ASCII alone.  This mirror has no SQLite, so the caller supplies the table -- for
// example the file next_plaid_amd.text.unicode61_table(planes).tofile(path) wrote, read by load_unicode_table.  The
// vector must live until the call returns.
inline np_text_build_opts text_build_opts(Tokenizer tokenizer, int32_t max_token_bytes, const std::vector<uint32_t>& unicode_table) {
  np_text_build_opts o = text_build_opts(tokenizer, max_token_bytes);
  o.unicode_table = unicode_table.data();
  o.unicode_table_len = (int64_t)unicode_table.size();
  return o;
}

inline std::vector<uint32_t> load_unicode_table(const std::string& path) {
  std::vector<uint32_t> t;
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw Error(NP_ERR_INVALID_ARGUMENT, ("load_unicode_table: cannot open " + path).c_str());
  uint32_t buf[4096];
  size_t n;
  while ((n = std::fread(buf, sizeof(uint32_t), 4096, f)) > 0) t.insert(t.end(), buf, buf + n);
  std::fclose(f);
  return t;
}

// The index of the documents the device reproduces.  A non-empty fallback_docs means the arrays lack those documents: the
// caller tokenises them and calls the overload below (nothing is dropped silently: the list is part of the result).
inline BuiltTextIndex build_text_index(const std::vector<std::string>& texts, Tokenizer tokenizer = Tokenizer::Unicode61,
                                       int device = 0, int32_t max_token_bytes = 0) {
  BuiltTextIndex r;
  detail::TextBuildHandle b;
  detail::text_build_start(b, texts, text_build_opts(tokenizer, max_token_bytes), device, &r);
  detail::text_build_finish(b, &r);
  return r;
}

// ... with the caller's instances for the fallback documents: tokenize(fallback_docs) is called once, when the list is not empty.
namespace detail {
template <class Tokenize>
inline BuiltTextIndex build_text_index_with(const std::vector<std::string>& texts, const np_text_build_opts& o, Tokenize&& tokenize,
                                            int device);
}
template <class Tokenize>
inline BuiltTextIndex build_text_index(const std::vector<std::string>& texts, Tokenizer tokenizer, Tokenize&& tokenize,
                                       int device = 0, int32_t max_token_bytes = 0) {
  return detail::build_text_index_with(texts, text_build_opts(tokenizer, max_token_bytes), tokenize, device);
}

// ... in UTF-8 mode (see text_build_opts): fallback_docs then lists only malformed text, code points beyond the table and
// overlong tokens.
inline BuiltTextIndex build_text_index(const std::vector<std::string>& texts, const std::vector<uint32_t>& unicode_table,
                                       Tokenizer tokenizer = Tokenizer::Unicode61, int device = 0, int32_t max_token_bytes = 0) {
  BuiltTextIndex r;
  detail::TextBuildHandle b;
  detail::text_build_start(b, texts, text_build_opts(tokenizer, max_token_bytes, unicode_table), device, &r);
  detail::text_build_finish(b, &r);
  return r;
}
template <class Tokenize>
inline BuiltTextIndex build_text_index(const std::vector<std::string>& texts, const std::vector<uint32_t>& unicode_table,
                                       Tokenizer tokenizer, Tokenize&& tokenize, int device = 0, int32_t max_token_bytes = 0) {
  return detail::build_text_index_with(texts, text_build_opts(tokenizer, max_token_bytes, unicode_table), tokenize, device);
}

template <class Tokenize>
inline BuiltTextIndex detail::build_text_index_with(const std::vector<std::string>& texts, const np_text_build_opts& o,
                                                    Tokenize&& tokenize, int device) {
  BuiltTextIndex r;
  detail::TextBuildHandle b;
  detail::text_build_start(b, texts, o, device, &r);
  if (!r.fallback_docs.empty()) {
    const TextInstances inst = tokenize(r.fallback_docs);
    std::vector<int64_t> tbo(inst.terms.size() + 1, 0);
    for (size_t i = 0; i < inst.terms.size(); ++i) tbo[i + 1] = tbo[i] + (int64_t)inst.terms[i].size();
    std::vector<uint8_t> tb((size_t)tbo.back());
    for (size_t i = 0; i < inst.terms.size(); ++i) std::copy(inst.terms[i].begin(), inst.terms[i].end(), tb.begin() + tbo[i]);
    if (inst.inst_term.size() != inst.inst_doc.size() || inst.inst_term.size() != inst.inst_pos.size())
      throw Error(NP_ERR_INVALID_ARGUMENT, "build_text_index: the instance arrays differ in length");
    check(np_hip_text_build_add(b.h, tb.empty() ? nullptr : tb.data(), tbo.data(), (int64_t)inst.terms.size(), inst.inst_term.data(),
                                inst.inst_doc.data(), inst.inst_pos.data(), (int64_t)inst.inst_term.size()));
  }
  detail::text_build_finish(b, &r);
  return r;
}

// ---- the keyword index kept current (np_hip_text_build_merge): append, delete and replace rows of a built index ----
// What the crate's index / delete / update_rows (and rebuild) leave, without building the table again.  `replace` maps row
// ids to their new text; the batch is the replacements in id order, then new_texts, which follow the last id.  renumber
// numbers the surviving rows 0, 1, ... in order (delete + rebuild); otherwise every id stays.  The base is a dense table
// (rows 0 .. base.n_rows - 1).  merge_report is the merge's report, report the batch's build.
struct TextUpdate {
  std::vector<std::string> new_texts;
  std::vector<int64_t> delete_ids;
  std::vector<std::pair<int64_t, std::string>> replace;
  bool renumber = true;
};

struct UpdatedTextIndex : BuiltTextIndex {
  np_text_merge_report merge_report{};
};

namespace detail {
// remap, delta_ids, the batch's texts and the result's row count; throws on an id outside the table or named twice
inline void text_update_plan(int64_t n_old, const TextUpdate& u, std::vector<int64_t>* remap, std::vector<int64_t>* delta_ids,
                             std::vector<std::string>* texts, int64_t* n_rows_out) {
  std::vector<int64_t> gone(u.delete_ids);
  std::sort(gone.begin(), gone.end());
  gone.erase(std::unique(gone.begin(), gone.end()), gone.end());
  std::vector<std::pair<int64_t, std::string>> rep(u.replace);
  std::sort(rep.begin(), rep.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
  auto inside = [&](int64_t d) {
    if (d < 0 || d >= n_old)
      throw Error(NP_ERR_INVALID_ARGUMENT,
                  ("update_text_index: row " + std::to_string(d) + " is outside the table's " + std::to_string(n_old) + " row ids").c_str());
  };
  for (int64_t d : gone) inside(d);
  for (size_t i = 0; i < rep.size(); ++i) {
    inside(rep[i].first);
    if (i > 0 && rep[i].first == rep[i - 1].first)
      throw Error(NP_ERR_INVALID_ARGUMENT, ("update_text_index: row " + std::to_string(rep[i].first) + " is replaced twice").c_str());
    if (std::binary_search(gone.begin(), gone.end(), rep[i].first))
      throw Error(NP_ERR_INVALID_ARGUMENT, ("update_text_index: row " + std::to_string(rep[i].first) + " is in both delete and replace").c_str());
  }
  remap->assign((size_t)n_old, 0);
  for (int64_t d = 0; d < n_old; ++d) (*remap)[(size_t)d] = d;
  for (int64_t d : gone) (*remap)[(size_t)d] = -1;
  int64_t top = n_old;
  if (u.renumber) {
    top = 0;
    for (int64_t& v : *remap)
      if (v >= 0) v = top++;
  }
  delta_ids->clear();
  texts->clear();
  for (const auto& r : rep) {
    delta_ids->push_back((*remap)[(size_t)r.first]);
    (*remap)[(size_t)r.first] = -1;
    texts->push_back(r.second);
  }
  for (size_t i = 0; i < u.new_texts.size(); ++i) {
    delta_ids->push_back(top + (int64_t)i);
    texts->push_back(u.new_texts[i]);
  }
  *n_rows_out = n_old - (int64_t)gone.size() + (int64_t)u.new_texts.size();
}

template <class AddFallback>
inline UpdatedTextIndex text_update_run(const BuiltTextIndex& base, const TextUpdate& u, const np_text_build_opts& opts, int device,
                                        AddFallback&& add_fallback) {
  if (base.term_offsets.size() != base.terms.size() + 1)
    throw Error(NP_ERR_INVALID_ARGUMENT, "update_text_index: base.term_offsets does not have one entry per term and one more");
  std::vector<int64_t> remap, delta_ids;
  std::vector<std::string> texts;
  int64_t n_rows_out = 0;
  text_update_plan(base.n_rows, u, &remap, &delta_ids, &texts, &n_rows_out);
  std::vector<int64_t> tbo(base.terms.size() + 1, 0);
  for (size_t i = 0; i < base.terms.size(); ++i) tbo[i + 1] = tbo[i] + (int64_t)base.terms[i].size();
  std::vector<uint8_t> tb((size_t)tbo.back());
  for (size_t i = 0; i < base.terms.size(); ++i) std::copy(base.terms[i].begin(), base.terms[i].end(), tb.begin() + tbo[i]);
  np_text_index t{};
  t.n_terms = (int64_t)base.terms.size();
  t.term_offsets = base.term_offsets.data();
  t.inst_doc = base.inst_doc.empty() ? nullptr : base.inst_doc.data();
  t.inst_pos = base.inst_pos.empty() ? nullptr : base.inst_pos.data();
  t.n_rows = base.n_rows;
  UpdatedTextIndex r;
  TextBuildHandle batch, merged;
  if (!texts.empty()) {
    text_build_start(batch, texts, opts, device, &r);
    add_fallback(batch, r);
    check(np_hip_text_build_sizes(batch.h, nullptr, nullptr, nullptr, nullptr));
  }
  np_text_merge_opts o{};
  check(np_hip_text_build_merge(device, &t, tb.empty() ? nullptr : tb.data(), tbo.data(), remap.empty() ? nullptr : remap.data(),
                                (int64_t)remap.size(), batch.h, delta_ids.empty() ? nullptr : delta_ids.data(), n_rows_out, &o,
                                &merged.h, &r.merge_report));
  text_build_finish(merged, &r);
  return r;
}

template <class Tokenize>
inline void text_build_add_fallback(TextBuildHandle& b, const BuiltTextIndex& r, Tokenize&& tokenize) {
  if (r.fallback_docs.empty()) return;
  const TextInstances inst = tokenize(r.fallback_docs);
  std::vector<int64_t> tbo(inst.terms.size() + 1, 0);
  for (size_t i = 0; i < inst.terms.size(); ++i) tbo[i + 1] = tbo[i] + (int64_t)inst.terms[i].size();
  std::vector<uint8_t> tb((size_t)tbo.back());
  for (size_t i = 0; i < inst.terms.size(); ++i) std::copy(inst.terms[i].begin(), inst.terms[i].end(), tb.begin() + tbo[i]);
  if (inst.inst_term.size() != inst.inst_doc.size() || inst.inst_term.size() != inst.inst_pos.size())
    throw Error(NP_ERR_INVALID_ARGUMENT, "update_text_index: the instance arrays differ in length");
  check(np_hip_text_build_add(b.h, tb.empty() ? nullptr : tb.data(), tbo.data(), (int64_t)inst.terms.size(), inst.inst_term.data(),
                              inst.inst_doc.data(), inst.inst_pos.data(), (int64_t)inst.inst_term.size()));
}
}  // namespace detail

// The batch must be text the device reproduces: a fallback document in it is an error here (nothing is dropped silently);
// the overload below takes the caller's instances for them.
namespace detail {
inline void text_update_no_fallback(TextBuildHandle&, const BuiltTextIndex& r) {
  if (!r.fallback_docs.empty())
    throw Error(NP_ERR_INVALID_ARGUMENT, ("update_text_index: batch document " + std::to_string(r.fallback_docs[0]) +
                                          " is not reproduced on the device and no tokenize was given").c_str());
}
}  // namespace detail
inline UpdatedTextIndex update_text_index(const BuiltTextIndex& base, const TextUpdate& update, Tokenizer tokenizer = Tokenizer::Unicode61,
                                          int device = 0, int32_t max_token_bytes = 0) {
  return detail::text_update_run(base, update, text_build_opts(tokenizer, max_token_bytes), device, detail::text_update_no_fallback);
}
// ... the batch tokenised in UTF-8 mode (see text_build_opts)
inline UpdatedTextIndex update_text_index(const BuiltTextIndex& base, const TextUpdate& update, const std::vector<uint32_t>& unicode_table,
                                          Tokenizer tokenizer = Tokenizer::Unicode61, int device = 0, int32_t max_token_bytes = 0) {
  return detail::text_update_run(base, update, text_build_opts(tokenizer, max_token_bytes, unicode_table), device,
                                 detail::text_update_no_fallback);
}

// ... tokenize(fallback_docs) is called once when the batch has fallback documents; the ids index the batch (the
// replacements in id order, then new_texts).
template <class Tokenize>
inline UpdatedTextIndex update_text_index(const BuiltTextIndex& base, const TextUpdate& update, Tokenizer tokenizer, Tokenize&& tokenize,
                                          int device = 0, int32_t max_token_bytes = 0) {
  return detail::text_update_run(base, update, text_build_opts(tokenizer, max_token_bytes), device,
                                 [&](detail::TextBuildHandle& b, const BuiltTextIndex& r) { detail::text_build_add_fallback(b, r, tokenize); });
}
template <class Tokenize>
inline UpdatedTextIndex update_text_index(const BuiltTextIndex& base, const TextUpdate& update, const std::vector<uint32_t>& unicode_table,
                                          Tokenizer tokenizer, Tokenize&& tokenize, int device = 0, int32_t max_token_bytes = 0) {
  return detail::text_update_run(base, update, text_build_opts(tokenizer, max_token_bytes, unicode_table), device,
                                 [&](detail::TextBuildHandle& b, const BuiltTextIndex& r) { detail::text_build_add_fallback(b, r, tokenize); });
}

// ---- the resident keyword index (np_hip_index_set_text_build, np_hip_index_text_merge): built and updated in HBM ----
// What a handle's keyword index is to the host when its arrays stay on the device: the vocabulary and the counts.  The
// arrays come back with get_text (np_hip_index_get_text) when they are wanted.
struct ResidentTextIndex {
  std::vector<std::string> terms;          // term id -> term, in fts5vocab's order
  int64_t n_rows = 0;
  int64_t n_instances = 0;
  std::vector<int64_t> fallback_docs;      // of the build, or of the update's batch
  np_text_build_report report{};           // the build's, or the batch's
  np_text_merge_report merge_report{};     // the merge's (update_text_resident)
};

namespace detail {
// np_hip_text_build_sizes, np_hip_index_set_text_build and the vocabulary half of np_hip_text_build_fetch
inline void text_install(MmapIndex& ix, TextBuildHandle& b, ResidentTextIndex* r) {
  check(np_hip_text_build_sizes(b.h, nullptr, nullptr, nullptr, nullptr));
  check(np_hip_index_set_text_build(ix.handle(), b.h));
  int64_t n_terms = 0, n_bytes = 0;
  check(np_hip_text_build_sizes(b.h, &n_terms, &n_bytes, &r->n_instances, &r->n_rows));
  std::vector<uint8_t> tb((size_t)std::max<int64_t>(n_bytes, 1));
  std::vector<int64_t> tbo((size_t)n_terms + 1);
  check(np_hip_text_build_fetch(b.h, tb.data(), tbo.data(), nullptr, nullptr, nullptr));
  r->terms.resize((size_t)n_terms);
  for (int64_t t = 0; t < n_terms; ++t) r->terms[(size_t)t].assign((const char*)tb.data() + tbo[(size_t)t], (size_t)(tbo[(size_t)t + 1] - tbo[(size_t)t]));
  ix.refresh_info();
}

// np_hip_index_text_merge of the handle's keyword index (whose vocabulary is cur.terms) with the update's batch
template <class AddFallback>
inline void text_merge_resident(const MmapIndex& ix, const ResidentTextIndex& cur, const TextUpdate& u, const np_text_build_opts& opts,
                                AddFallback&& add_fallback, TextBuildHandle* merged, ResidentTextIndex* r) {
  int64_t have = 0;
  check(np_hip_index_text_sizes(ix.handle(), &have, nullptr, nullptr, nullptr, nullptr));
  if (have != (int64_t)cur.terms.size())
    throw Error(NP_ERR_INVALID_ARGUMENT, ("base_term_byte_offsets describes " + std::to_string(cur.terms.size()) +
                                          " terms, the handle's keyword index holds " + std::to_string(have)).c_str());
  std::vector<int64_t> remap, delta_ids;
  std::vector<std::string> texts;
  int64_t n_rows_out = 0;
  text_update_plan(cur.n_rows, u, &remap, &delta_ids, &texts, &n_rows_out);
  std::vector<int64_t> tbo(cur.terms.size() + 1, 0);
  for (size_t i = 0; i < cur.terms.size(); ++i) tbo[i + 1] = tbo[i] + (int64_t)cur.terms[i].size();
  std::vector<uint8_t> tb((size_t)tbo.back());
  for (size_t i = 0; i < cur.terms.size(); ++i) std::copy(cur.terms[i].begin(), cur.terms[i].end(), tb.begin() + tbo[i]);
  TextBuildHandle batch;
  if (!texts.empty()) {
    BuiltTextIndex built;
    text_build_start(batch, texts, opts, ix.info().device, &built);
    add_fallback(batch, built);
    check(np_hip_text_build_sizes(batch.h, nullptr, nullptr, nullptr, nullptr));
    r->fallback_docs = built.fallback_docs;
    r->report = built.report;
  }
  np_text_merge_opts o{};
  check(np_hip_index_text_merge(ix.handle(), tb.empty() ? nullptr : tb.data(), tbo.data(), remap.empty() ? nullptr : remap.data(),
                                (int64_t)remap.size(), batch.h, delta_ids.empty() ? nullptr : delta_ids.data(), n_rows_out, &o,
                                &merged->h, &r->merge_report));
}

inline void text_no_fallback(TextBuildHandle&, const BuiltTextIndex& r) {
  if (!r.fallback_docs.empty())
    throw Error(NP_ERR_INVALID_ARGUMENT, ("update_text_resident: batch document " + std::to_string(r.fallback_docs[0]) +
                                          " is not reproduced on the device and no tokenize was given").c_str());
}
}  // namespace detail

// build_text_index whose result stays in HBM and becomes the handle's keyword index: build -> (fallback -> add) -> sizes ->
// np_hip_index_set_text_build.  Only the vocabulary is fetched.  Searches beside the call go on; no lock is needed.
namespace detail {
inline ResidentTextIndex build_text_resident_with(MmapIndex& ix, const std::vector<std::string>& texts, const np_text_build_opts& o);
template <class Tokenize>
inline ResidentTextIndex build_text_resident_with(MmapIndex& ix, const std::vector<std::string>& texts, const np_text_build_opts& o,
                                                  Tokenize&& tokenize) {
  ResidentTextIndex r;
  BuiltTextIndex built;
  TextBuildHandle b;
  text_build_start(b, texts, o, ix.info().device, &built);
  text_build_add_fallback(b, built, tokenize);
  r.report = built.report;
  r.fallback_docs = built.fallback_docs;
  text_install(ix, b, &r);
  return r;
}
// true for what may stand where update_text_resident takes its `step`: anything but a unicode_table, so that a table the
// caller holds as a plain (non-const) vector selects the table overloads and is never deduced as the step
template <class T>
using is_step = std::integral_constant<bool, !std::is_same<typename std::decay<T>::type, std::vector<uint32_t>>::value>;
}
inline ResidentTextIndex build_text_resident(MmapIndex& ix, const std::vector<std::string>& texts, Tokenizer tokenizer = Tokenizer::Unicode61,
                                             int32_t max_token_bytes = 0) {
  return detail::build_text_resident_with(ix, texts, text_build_opts(tokenizer, max_token_bytes));
}
// ... in UTF-8 mode (see text_build_opts)
inline ResidentTextIndex build_text_resident(MmapIndex& ix, const std::vector<std::string>& texts, const std::vector<uint32_t>& unicode_table,
                                             Tokenizer tokenizer = Tokenizer::Unicode61, int32_t max_token_bytes = 0) {
  return detail::build_text_resident_with(ix, texts, text_build_opts(tokenizer, max_token_bytes, unicode_table));
}
inline ResidentTextIndex detail::build_text_resident_with(MmapIndex& ix, const std::vector<std::string>& texts, const np_text_build_opts& o) {
  ResidentTextIndex r;
  BuiltTextIndex built;
  detail::TextBuildHandle b;
  detail::text_build_start(b, texts, o, ix.info().device, &built);
  if (!built.fallback_docs.empty())
    throw Error(NP_ERR_INVALID_ARGUMENT, ("build_text_resident: document " + std::to_string(built.fallback_docs[0]) +
                                          " is not reproduced on the device and no tokenize was given").c_str());
  r.report = built.report;
  detail::text_install(ix, b, &r);
  return r;
}
template <class Tokenize>
inline ResidentTextIndex build_text_resident(MmapIndex& ix, const std::vector<std::string>& texts, Tokenizer tokenizer, Tokenize&& tokenize,
                                             int32_t max_token_bytes = 0) {
  return detail::build_text_resident_with(ix, texts, text_build_opts(tokenizer, max_token_bytes), tokenize);
}
// ... in UTF-8 mode with the caller's tokenizer for what still falls back (code points beyond the table, overlong tokens)
template <class Tokenize>
inline ResidentTextIndex build_text_resident(MmapIndex& ix, const std::vector<std::string>& texts, const std::vector<uint32_t>& unicode_table,
                                             Tokenizer tokenizer, Tokenize&& tokenize, int32_t max_token_bytes = 0) {
  return detail::build_text_resident_with(ix, texts, text_build_opts(tokenizer, max_token_bytes, unicode_table), tokenize);
}

// The handle's keyword index updated from itself: the batch is built on the device, np_hip_index_text_merge reads the base
// where it lies and np_hip_index_set_text_build installs the result.  `cur` is what the last resident call returned (its
// vocabulary and row count are the base's).  `step` runs between the merge and the install: the vector-index call that
// drops the handle's keyword index (append_arrays with rows, remove_ids with keep_attachments, expand_arrays with rows), so
// that the order is merge, vector call, install.  If it throws, the handle keeps its old keyword index and the result is freed.
template <class Step, class = typename std::enable_if<detail::is_step<Step>::value>::type>
inline ResidentTextIndex update_text_resident(MmapIndex& ix, const ResidentTextIndex& cur, const TextUpdate& update, Step&& step,
                                              Tokenizer tokenizer = Tokenizer::Unicode61, int32_t max_token_bytes = 0) {
  ResidentTextIndex r;
  detail::TextBuildHandle merged;
  detail::text_merge_resident(ix, cur, update, text_build_opts(tokenizer, max_token_bytes), detail::text_no_fallback, &merged, &r);
  step();
  detail::text_install(ix, merged, &r);
  return r;
}
inline ResidentTextIndex update_text_resident(MmapIndex& ix, const ResidentTextIndex& cur, const TextUpdate& update,
                                              Tokenizer tokenizer = Tokenizer::Unicode61, int32_t max_token_bytes = 0) {
  return update_text_resident(ix, cur, update, [] {}, tokenizer, max_token_bytes);
}
// ... the batch tokenised in UTF-8 mode (see text_build_opts)
template <class Step>
inline ResidentTextIndex update_text_resident(MmapIndex& ix, const ResidentTextIndex& cur, const TextUpdate& update,
                                              const std::vector<uint32_t>& unicode_table, Step&& step,
                                              Tokenizer tokenizer = Tokenizer::Unicode61, int32_t max_token_bytes = 0) {
  ResidentTextIndex r;
  detail::TextBuildHandle merged;
  detail::text_merge_resident(ix, cur, update, text_build_opts(tokenizer, max_token_bytes, unicode_table), detail::text_no_fallback,
                              &merged, &r);
  step();
  detail::text_install(ix, merged, &r);
  return r;
}
inline ResidentTextIndex update_text_resident(MmapIndex& ix, const ResidentTextIndex& cur, const TextUpdate& update,
                                              const std::vector<uint32_t>& unicode_table, Tokenizer tokenizer = Tokenizer::Unicode61,
                                              int32_t max_token_bytes = 0) {
  return update_text_resident(ix, cur, update, unicode_table, [] {}, tokenizer, max_token_bytes);
}
// ... tokenize(fallback_docs) is called once when the batch has fallback documents (a byte >= 0x80, ...); the ids index the
// batch (the replacements in id order, then new_texts), as in update_text_index.
template <class Step, class Tokenize,
          class = typename std::enable_if<detail::is_step<Step>::value && !std::is_integral<typename std::decay<Tokenize>::type>::value>::type>
inline ResidentTextIndex update_text_resident(MmapIndex& ix, const ResidentTextIndex& cur, const TextUpdate& update, Step&& step,
                                              Tokenizer tokenizer, Tokenize&& tokenize, int32_t max_token_bytes = 0) {
  ResidentTextIndex r;
  detail::TextBuildHandle merged;
  detail::text_merge_resident(ix, cur, update, text_build_opts(tokenizer, max_token_bytes),
                              [&](detail::TextBuildHandle& b, const BuiltTextIndex& built) { detail::text_build_add_fallback(b, built, tokenize); },
                              &merged, &r);
  step();
  detail::text_install(ix, merged, &r);
  return r;
}
// ... in UTF-8 mode with the caller's tokenizer for what still falls back
template <class Step, class Tokenize, class = typename std::enable_if<!std::is_integral<typename std::decay<Tokenize>::type>::value>::type>
inline ResidentTextIndex update_text_resident(MmapIndex& ix, const ResidentTextIndex& cur, const TextUpdate& update,
                                              const std::vector<uint32_t>& unicode_table, Step&& step, Tokenizer tokenizer,
                                              Tokenize&& tokenize, int32_t max_token_bytes = 0) {
  ResidentTextIndex r;
  detail::TextBuildHandle merged;
  detail::text_merge_resident(ix, cur, update, text_build_opts(tokenizer, max_token_bytes, unicode_table),
                              [&](detail::TextBuildHandle& b, const BuiltTextIndex& built) { detail::text_build_add_fallback(b, built, tokenize); },
                              &merged, &r);
  step();
  detail::text_install(ix, merged, &r);
  return r;
}

// The handle's keyword index read back from HBM (np_hip_index_get_text) with the vocabulary the host kept.
inline BuiltTextIndex get_text(const MmapIndex& ix, const std::vector<std::string>& terms) {
  BuiltTextIndex r;
  int64_t n_terms = 0, n_inst = 0;
  check(np_hip_index_text_sizes(ix.handle(), &n_terms, nullptr, &n_inst, &r.n_rows, nullptr));
  if (n_terms != (int64_t)terms.size())
    throw Error(NP_ERR_INVALID_ARGUMENT, ("get_text: the handle's keyword index holds " + std::to_string(n_terms) + " terms, the vocabulary " +
                                          std::to_string(terms.size())).c_str());
  r.terms = terms;
  r.term_offsets.resize((size_t)n_terms + 1);
  r.inst_doc.resize((size_t)n_inst);
  r.inst_pos.resize((size_t)n_inst);
  check(np_hip_index_get_text(ix.handle(), r.term_offsets.data(), r.inst_doc.data(), r.inst_pos.data()));
  return r;
}

// ... and as it lies (np_hip_index_get_text_layout)
struct TextLayout {
  std::vector<int64_t> post_off, post_first;
  std::vector<int32_t> post_doc, post_tf, doc_len;
};
inline TextLayout get_text_layout(const MmapIndex& ix) {
  TextLayout l;
  int64_t n_terms = 0, n_post = 0, n_docs = 0;
  check(np_hip_index_text_sizes(ix.handle(), &n_terms, &n_post, nullptr, nullptr, &n_docs));
  l.post_off.resize((size_t)n_terms + 1);
  l.post_doc.resize((size_t)n_post);
  l.post_tf.resize((size_t)n_post);
  l.post_first.resize((size_t)n_post);
  l.doc_len.resize((size_t)n_docs);
  check(np_hip_index_get_text_layout(ix.handle(), l.post_off.data(), l.post_doc.data(), l.post_tf.data(), l.post_first.data(), l.doc_len.data()));
  return l;
}

}  // namespace next_plaid
