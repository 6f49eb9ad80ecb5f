// np_internal.h -- shared declarations of libnextplaid_hip.so (not part of the C ABI).
//
// Data layout in HBM.  One np_index = one document shard:
//   centroids   f32 [K][dim]            replicated on every shard   (centroids.npy)
//   wlut        f32 [2^nbits]           permuted bucket weights: wlut[s] = bucket_weights[bitrev_nbits(s)]
//                                       (folds codec.rs:168-214's two LUTs into one)
//   codes       u16 [T] (K <= 65536) or u32 [T]   centroid id per token   (N.codes.npy, i64 on disk, range-checked at load)
//   residuals   u8  [T][pd]             packed buckets, unchanged   (N.residuals.npy)
//   ucodes      u16 / u32 [U]           derived at open: the documents' sorted DISTINCT-code lists: one fixed-stride block per
//                                       document (16-byte header + codes; the stride holds 99.9 % of the lists) followed by an
//                                       overflow region for longer lists; the doc_meta record carries the list's offset either
//                                       way.  S4 reads these.  ulen i32 [n_docs] = list lengths
//   inv_norm    f32 [T]                 derived at open: 1/||centroid + residual|| per token (S6 QC-reuse form)
//   tok_pos     u16 [T]                 derived at open: codes / residuals / inv_norm keep each document's tokens ORDERED BY
//                                       CODE (MaxSim is a max over tokens: order-free), tok_pos = the original position
//                                       (decompress_documents / export restore the on-disk order)
//   doc_offsets i64 [n_docs+1]          prefix sum of doclens       (index.rs:1106-1110)
//   ivf         u32 [ivf_size]          shard-local doc ids         (ivf.npy re-based)
//   ivf_offsets i64 [K+1]                                           (index.rs:1089-1094)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <condition_variable>
#include <string>
#include <vector>
#include "../../include/nextplaid_hip.h"

namespace np {

// A code array of the index (token codes, or the documents' distinct-code lists): u16 entries when every centroid id
// fits 16 bits (K <= 65536), u32 otherwise.  `wide` is a kernel argument, so the branch is wave-uniform.
struct CodeArr {
  const void* p;
  int wide;
  __device__ __forceinline__ uint32_t operator[](int64_t i) const {
    return wide ? static_cast<const uint32_t*>(p)[i] : (uint32_t)static_cast<const uint16_t*>(p)[i];
  }
};

// ---- errors --------------------------------------------------------------------------------
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
const char* last_error();
void clear_error();

struct Status {
  int code;
  Status(int c = NP_OK) : code(c) {}
  bool ok() const { return code == NP_OK; }
};

#define NP_HIP(expr)                                                                         \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess) {                                                                 \
      np::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
      return (e__ == hipErrorOutOfMemory) ? NP_ERR_OUT_OF_MEMORY : NP_ERR_DEVICE_UNAVAILABLE; \
    }                                                                                        \
  } while (0)

#define NP_TRY(expr)            \
  do {                          \
    int rc__ = (expr);          \
    if (rc__ != NP_OK) return rc__; \
  } while (0)

// ---- host view of an index (on-disk dtypes), produced by the loader or handed in by the caller
struct HostChunk {
  const int64_t* codes = nullptr;     // [n_tokens]
  const uint8_t* residuals = nullptr; // [n_tokens][pd]
  int64_t n_tokens = 0;
};

struct HostIndex {
  int64_t num_documents_total = 0, num_embeddings_total = 0;
  double avg_doclen = 0.0;
  int64_t doc_begin = 0;               // global id of doc_lengths[0]
  int64_t K = 0;
  int32_t dim = 0, nbits = 0;
  const float* centroids = nullptr;
  const float* bucket_weights = nullptr;
  const int64_t* ivf = nullptr;        // global doc ids
  int64_t ivf_size = 0;
  const int32_t* ivf_lengths = nullptr;
  std::vector<int64_t> doc_lengths;    // docs [doc_begin, doc_begin + size)
  std::vector<HostChunk> chunks;       // token data of those docs, in order
  // keeps mmaps / owned buffers alive
  std::vector<std::pair<void*, size_t>> maps;
  std::vector<std::vector<char>> owned;
  ~HostIndex();
};

// np_loader.cpp: MmapIndex::load's file parsing (index.rs:1026-1139, mmap.rs:659-749)
int load_index_dir(const char* dir, HostIndex* out);

// np_loader.cpp: the loader's parsers for the update path (np_update.cpp), over files read whole
int read_text_file(const std::string& path, std::string* out);
bool json_number_field(const std::string& j, const char* key, double* out);
int json_int_list(const std::string& path, const std::string& j, std::vector<int64_t>* out);
// NPY v1 / v2: *data points into *bytes; descr and shape as in the header (fortran order refused)
int read_npy_file(const std::string& path, std::vector<uint8_t>* bytes, std::string* descr, std::vector<int64_t>* shape,
                  const uint8_t** data);

// np_writer.cpp: the writer's temporary-name + fsync + rename files, and serde's f64 text
int write_npy_file(const std::string& path, const char* descr, const int64_t* shape, int ndim, const void* data,
                   size_t bytes);
int write_text_file(const std::string& path, const std::string& text);
std::string format_f64(double v);

// np_build.hip: the device work of the update path (np_update.cpp), with the create path's rules and input checks
int build_check_device(int device);
int build_check_dim(int dim);
int build_check_finite(const float* x, int64_t count, int dim);
// rows of X [n][dim] whose f32(min_c f64 |x - c|^2) > thr * thr (f32), ascending; *n_rechecked = rows the f64 pass decided
int find_outliers(int device, const float* X, int64_t n, int dim, const float* C, int64_t k, float thr,
                  std::vector<int64_t>* out, int64_t* n_rechecked);
// compute_kmeans on the points as one-token documents with num_partitions = k (update.rs:700-730)
int kmeans_points_as_docs(int device, const float* pts, int64_t n, int dim, const np_index_config& cfg, int64_t k,
                          std::vector<float>* cen);
// every token encoded against a codec (np_hip_encode_tokens' rules); norms (nullable) = |x - c[code]| per token
int encode_with_codec(int device, const float* C, int64_t K, int dim, int nbits, const float* weights, const float* cutoffs,
                      const float* X, int64_t T, int64_t* codes, uint8_t* packed, float* norms);
float quantile_of_sorted(const std::vector<float>& v, double q);   // utils.rs:94-149

// ---- device buffers ------------------------------------------------------------------------
// One device allocation and its only owner: move-only, freed on destruction or reset().  alloc(n) takes max(n, 1)
// elements (an empty array still has an address) and adds the bytes to *acct when given (DeviceIndex::device_bytes).
// hipFree acts on the current device: the arrays of a DeviceIndex go under destroy_device_index's DeviceGuard.
template <class T>
class DevPtr {
 public:
  DevPtr() = default;
  DevPtr(DevPtr&& o) noexcept : p_(o.p_), bytes_(o.bytes_) {
    o.p_ = nullptr;
    o.bytes_ = 0;
  }
  DevPtr& operator=(DevPtr&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      bytes_ = o.bytes_;
      o.p_ = nullptr;
      o.bytes_ = 0;
    }
    return *this;
  }
  ~DevPtr() { reset(); }
  int alloc(size_t n, size_t* acct = nullptr) {
    reset();
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    hipError_t e = hipMalloc((void**)&p_, bytes);
    if (e != hipSuccess) {
      p_ = nullptr;
      set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
      return NP_ERR_OUT_OF_MEMORY;
    }
    bytes_ = bytes;
    if (acct) *acct += bytes;
    return NP_OK;
  }
  T* get() const { return p_; }
  size_t bytes() const { return bytes_; }   // of the allocation (0 when empty): what alloc() added to *acct
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
  }

 private:
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes);  // grows (never shrinks); contents are NOT preserved
  void release();
  template <class T> T* as() const { return (T*)p; }
};

struct Workspace;  // np_search.hip

struct Context {
  hipStream_t stream = nullptr;
  hipEvent_t ev[10] = {};
  Workspace* ws = nullptr;
  bool busy = false;
  uint64_t last_use = 0;   // acquisition stamp: idle contexts are handed out least-recently-used first
};

// Kernel-selection knobs.  Read from the environment ONCE, at index open (NP_<NAME>, e.g. NP_S4_MODE); np_hip_index_tune()
// changes them on a live handle for sweep tools and the kernel-variant parity tests; both go through set_tuning()'s one
// clamp table.  Every setting produces identical results.
struct Tuning {
  int s4_mode = 4;       // 0 approx_kernel; 1..4 approx_xcd_kernel with 8/4/2/1 phases; 5..8 approx_stream_kernel (the survivor lists
                         // of the filter are short: one phase measured best; 2 was best on unfiltered 18 k-document lists)
  int s4_minb = 8;       // smallest batch that takes the per-XCD kernels
  int s4_nbx = 128;      // workgroups per XCD
  int s4_swz = 1;        // ds_swizzle vs ds_bpermute code broadcast
  int s3_bisect = 1;     // S3: a bitmap range reads only its part of every (ascending) posting list instead of sweeping all of it
  int s3_slices = 1;     // S3: document-bitmap ranges built in LDS (mark_slices_kernel) instead of atomicOr in memory
  int s3_gain = 1;       // zeroth filter level (gain_sweep_kernel): per-document sums of the probed cells' gains prune the candidates
                         // before any list block is read -- where no centroid_score_threshold is set (with one, the removed cells
                         // lift the bound's floor above the cut: tools/sim/s3_gain_sim.py).  0 off (read at OPEN too: the range
                         // table of the posting lists is not built), 2 whenever it applies, 1 (default) = 2 with a run / skip policy:
                         // the level costs ~2 ms per batch at 10 M documents whatever it prunes, so while the candidates it removed
                         // in the handle's recent batches would not have cost the filter that much (K = 2^19: the bound's floor
                         // reaches the cut, 85 % of the candidates stay) it is skipped for 31 batches and tried again
  int s3_gain_mult = 3;  // ... S0 = the s3_gain_mult x n_sel candidates with the largest bound take the exact bound first (tau0)
  int s3_gain_direct = 16;   // ... workgroups per query of that launch (0 = one query per XCD at a time, like the S2 list)
  int s4_filter = 1;     // u8 upper-bound filter ahead of the exact f32 approximate scores
  int s4_hot = 60;       // per-mille of the centroids that are "hot" for a query in the first filter level (0 = single-level
                         // filter).  More hot centroids: fewer documents left to the exact bound (S1 + S2: 2.79 M / 2.20 M / 1.81 M of
                         // 11.9 M at 60 / 100 / 150) but more plane rows and walk steps per document in the hot kernel.  With the
                         // floored exact level (s4_warm) behind it, 10 M documents: 40 / 60 / 80 / 100 / 150 -> 18.3 / 18.6 / 18.4 /
                         // 17.8 / 16.6 k queries/s (round 3, byte maxima and every row at the exact level: 100 was best)
  int s4_hot_auto = 200000;   // candidates per query up to which s4_hot applies as given; beyond, the share falls with the
                         // candidate count^(-1/3), never below 8 per mille (hot_levels_kernel; 0 = s4_hot always).  The REST
                         // API's default regime (t_cs = None, nprobe 8: 2 M candidates per query at 10 M documents) wants ~30
  int s4_planes = 1;     // first filter level in bit-plane form (approx_hotp_kernel: 8 planes per hot centroid, OR + weighted popcount
                         // instead of 32 byte maxima per table row); 0 = approx_hot_kernel.  Read at OPEN too: with it the list blocks
                         // may be up to 512 bytes (corpora with long distinct-code lists), which approx_hot_kernel cannot stage
  int s4_lpd = 2;        // approx_hotp_kernel: lanes per document -- 4: claims of 16 documents (half the LDS rows per wave: more waves per
                         // CU hide the latency of the block loads), 2: claims of 32.  512-byte blocks always take 4
  int s4_pnbx = 96;      // ... workgroups per XCD (3 per CU at 42 KB of LDS each with 2 lanes per document; 160 = 5 per CU with 4)
  int s4_qm = 1;         // ... a lane's hot codes as a position mask in registers (1) or compacted in place by LDS writes (0)
  int s4_pexp = 15;      // plane levels: t_j = Lambda + span * (j / 8)^(s4_pexp / 10); 10 = uniform (hot_levels_kernel)
  int s4_warm = 0;       // ... per-mille of the centroids whose rows the exact level still gathers for the S2 list (the rest: floored
                         // at Lambda2; approx_ub_kernel FLOOR); 1000 = every row; 0 = by query length and list length (np_search.hip)
  int ub_ncut = 96;      // workgroups per query of the cut kernels (each appends 2048 records per step: latency-bound per step)
  int ub_direct = 8;     // workgroups per query of the short-list (S1) exact-bound launch; 0 = the per-XCD hand-out
  int hot_static = 1;    // hot kernel: waves take a query's claims round-robin (no cursor atomic: a device-scope atomic per claim
                         // on a line all XCDs share costs ~50 ns, serialised): 2.06 -> 1.68 ms at 10 M documents
  int ub_static = 0;     // the same for the exact-bound kernel: measured WORSE there (single-level S4 4.43 -> 5.17 ms: workgroups
                         // that run ahead pull the next query's table into the L2), so it keeps the cursor
  int s4_probe = 0;      // DIAGNOSTIC (results invalid when != 0): phases of the hot kernel to skip, for timing them
  int ub_nbx = 96;       // filter workgroups per XCD: 3 per CU (48 KB of LDS each).  64 makes the stage itself 3 % faster (0.70 vs 0.73 ms at
                         // 1 M, 4.43 vs 4.57 ms at 10 M documents) but the sustained 3-stream rate at 10 M drops 10.8 k -> 10.3 k queries/s
  int ub_steal = 16384;  // filter: an idle XCD joins a running query that has at least this many unclaimed documents (0x7fffffff = never)
  int ub_nt = 2;         // filter loads: 0 plain, 1 non-temporal records / code lists, 2 bounds-checked buffer loads of the table
  int s6_xcd = 1;        // one XCD per query in S6
  int s6_lds = 1;        // QC-reuse S6: query fragments in LDS + C-in rows prefetched one tile ahead (exact_qcl_kernel); 0 = exact_qct_kernel
  int s6_tiles = 1;      // QC-reuse S6: one launch of the one-tile kernel per 32-token query tile (0: the multi-tile kernels)
  int s1_split = 0;      // OPT-IN (np_hip_index_tune / NP_S1_SPLIT): split-bf16 S1 (qc_gemm_b3_kernel) when precision >= 1 and K >
                         // centroid_batch_size -- S1-S5 are then no longer bit-equal to the f32 chain (near-ties < ~1e-5 can reorder)
  int gemm_cpw = 1;      // centroid fragments per wave in S1
  int exact_rowmax = 0;  // force the row-max form of the QC-reuse S6 kernel
  int scan_tiles = 8;    // np_hip_search_exact: 32-token query tiles a workgroup of the scan stages in LDS (whole queries are packed
                         // up to this many tiles; a longer query takes a group of its own)
  int match_lds = 32;    // np_hip_text_match / NP_F_MATCH: KiB of LDS a DFA table may take; a larger table is read from global
                         // memory through the caches (0 = every table; at most 40: tile + classes + table stay within 64 KiB)
  int scan_docs = 0;     // ... documents per pass over the index; 0 = as many as the key table's share of the workspace budget holds
  int remove_slab = 0;   // np_hip_index_remove: source tokens per slab of the in-place token move (np_remove_plan.h) = rows of its
                         // staging buffer; 0 = NP_REMOVE_SLAB_DEFAULT.  np_hip_index_tune only: tests cross slab edges with a few thousand tokens
  int expand_fail = 0;   // np_hip_index_expand and, sharing its body, np_hip_index_append (both with their _rows entries): the stage
                         // after which the call returns NP_ERR_OUT_OF_MEMORY as a refused allocation there would (1 token
                         // stages, 2 distinct-code rebuild, 3 posting lists, 4 range table; 0 = never).  No device
                         // error is involved: the call ends early and its undo runs.  np_hip_index_tune only: tests check that the
                         // handle is put back -- a real refusal needs a full device
};

// documents per range of the posting lists' range table (d_ivf_split) = per block of the zeroth filter level's sweep (np_kernels.h)
#define NP_IVF_SPLIT_RANGE 32768

// what a filter kernel needs of one metadata column (np_filter.hip)
struct FilterCol {
  const void* data;        // i64 / f64 / i32 [n_docs]
  const uint32_t* valid;   // bit d = document d is not NULL; nullptr = no NULLs
  int32_t type, pad;
};
struct DeviceColumn {
  int32_t type = 0;
  DevPtr<uint8_t> data;
  DevPtr<uint32_t> valid;
  bool has_valid = false;
  int32_t min_code = 0, max_code = -1;   // CODE columns: the range of the handle's rows (np_hip_index_set_column_text checks it)
  // the dictionary text of a CODE column (np_hip_index_set_column_text, np_match.hip): string s = text[text_off[s] .. text_off[s + 1])
  DevPtr<uint8_t> text;                  // the bytes, padded with zeros to a multiple of 16 (tiles are staged with 16-byte loads)
  DevPtr<int64_t> text_off;              // [n_strings + 1]
  int64_t n_strings = 0, n_text_bytes = 0;
  size_t text_acct = 0;                  // this text's share of device_bytes
};

// the keyword index of a handle (np_hip_index_set_text, np_text.hip): per-term posting lists, the positions behind them and
// every document's token count in HBM; what only the host needs (document frequencies, totals) stays there
struct DeviceText {
  int64_t n_terms = 0, n_post = 0, n_inst = 0, n_rows = 0, total_tokens = 0;
  DevPtr<int64_t> post_off;     // [n_terms + 1] a term's postings
  DevPtr<int32_t> post_doc;     // [n_post] document, ascending inside a term
  DevPtr<int32_t> post_tf;      // [n_post] term frequency
  DevPtr<int64_t> post_first;   // [n_post] index of the posting's first position in pos
  DevPtr<int32_t> pos;          // [n_inst] positions, ascending inside a posting
  DevPtr<int32_t> doc_len;      // [n_docs] tokens of a document (its instances)
  std::vector<int64_t> h_post_off;   // host copy: a term's document frequency is the length of its list
  // a shard's slice of the whole table (np_hip_index_set_text_shard): the arrays above hold the shard's documents under their
  // shard-local ids; n_rows and total_tokens stay the WHOLE table's, and so does every term's document frequency
  std::vector<int64_t> h_df;         // [n_terms] documents of the whole table that hold the term (slices only)
  bool slice = false;
  bool present = false;
  int64_t df(int64_t term) const { return slice ? h_df[(size_t)term] : h_post_off[(size_t)term + 1] - h_post_off[(size_t)term]; }
};

struct DeviceIndex {
  int device = 0;
  int64_t N_total = 0, n_emb_total = 0;
  double avg_doclen = 0.0;
  int64_t doc_begin = 0, n_docs = 0;
  int64_t K = 0, KP = 0;  // KP = K rounded up to 64
  int32_t dim = 0, nbits = 0, pd = 0;     // STORAGE geometry: what every kernel is instantiated on (see storage_dim below)
  int32_t ldim = 0, lnbits = 0, lpd = 0;  // geometry of the index files and of the caller's queries / embeddings
  float pad_ss = 0.f;                     // (dim - ldim) * wlut[0]^2, see ExactP::pad_ss
  int64_t T = 0;
  int64_t max_doc_len = 0;
  // what the per-document (d_doc_offsets) and the per-token arrays (d_codes, d_residuals, d_inv_norm, d_tok_pos) are
  // ALLOCATED for: n_docs / T at open, more after np_hip_index_reserve -- an append within them moves none of these arrays
  int64_t cap_docs = 0, cap_tokens = 0;
  bool avg_from_counts = false;   // avg_doclen is num_embeddings / num_documents (arrays, synth), not a directory's stored figure
  // device arrays: owned, freed when destroy_device_index deletes the handle
  DevPtr<float> d_centroids;
  DevPtr<float> d_wlut;
  DevPtr<uint8_t> d_codes;        // [T] u16 when code_wide == 0 (K <= 65536), else u32
  int code_wide = 0;
  DevPtr<uint8_t> d_ucodes;       // [n_ucodes] dense per-document sorted distinct-code lists, same element type (derived)
  int64_t n_ucodes = 0;           // entries of d_ucodes without the tail padding
  int ublock_stride = 0;          // entries per document block of d_ucodes (header + codes; lists that do not fit: overflow region)
  int ublock_hdr = 0;             // entries of a block's 16-byte header {#distinct, doc length, overflow index, 0}
  DevPtr<int32_t> d_ulen;         // [n_docs] number of distinct codes per document (derived)
  DevPtr<uint4> d_useg;           // [n_docs] 8 x u16: distinct codes below each eighth of the centroid range (derived)
  DevPtr<uint4> d_doc_meta;       // [n_docs] the 16-B candidate record of every document {doc, n distinct codes, offset of its
                                  // distinct-code list in d_ucodes: low 32 bits, bits 32..39 | doc length << 8} (derived)
  float ulen_mean = 0.f;          // mean number of distinct codes per document (derived; scales the exact level's floor)
  bool sliced_ok = false;         // every document's distinct-code list is sorted and < 65536 long
  float cmax = 0.f;               // upper bound of the centroid row norms (derived; scales the S4 u8 score table)
  bool filter_ok = false;         // every centroid value is finite: the S4 upper-bound filter may run
  bool s6_fast_ok = false;        // centroids and bucket weights finite and < 1e6 in magnitude: with an unflagged query no S6
                                  // product can overflow, so the QC-reuse kernel drops its non-finite guard
  DevPtr<float> d_inv_norm;       // [T] 1 / max(||centroid[code] + residual||, 1e-12) per token (derived)
  DevPtr<uint16_t> d_tok_pos;     // [T] original position (inside its document) of the token stored here (derived; see below)
  bool tok_sorted = false;        // codes / residuals / inv_norm hold every document's tokens ORDERED BY CODE
  DevPtr<uint8_t> d_residuals;
  DevPtr<int64_t> d_doc_offsets;
  DevPtr<uint32_t> d_ivf;
  DevPtr<int64_t> d_ivf_offsets;
  int64_t ivf_size = 0;
  bool ivf_sorted = false;        // every posting list ascends (what the crate writes): S3 may bisect a list for a document range
  DevPtr<uint32_t> d_ivf_split;   // [K][n_ranges + 1] (derived, ascending lists only): entries of list c with id < 32768 r -- the
                                  // zeroth filter level's blocks read their range's part of a posting list without a bisection
  int n_ranges = 0;               // ceil(n_docs / 32768)
  int ivf_cover = -1;             // the lists hold every (document, distinct code) pair: 1 yes, 0 no, -1 never looked at
  // ivf_top_prefix[i] = entries of the i longest posting lists together (host side, i <= K): a query that probes c cells cannot
  // have more candidates than ivf_top_prefix[c] (search.rs:427-452 unions the probed cells' lists), which is what the workspace
  // planner sizes the candidate pool and the number of pool rounds for -- n_docs per query only when the lists do not say less
  std::vector<int64_t> ivf_top_prefix;
  // metadata columns (np_hip_index_set_columns, np_filter.hip): one SoA array per column over the shard's documents, validity
  // packed to bits (absent: no NULLs), and the table the filter kernels read them through
  std::vector<DeviceColumn> columns;
  DevPtr<FilterCol> d_coltab;     // [columns.size()]
  size_t column_bytes = 0;        // the columns' share of device_bytes
  size_t coltext_bytes = 0;       // ... and that of the columns' dictionary text
  DeviceText text;                // the keyword index (np_hip_index_set_text)
  size_t text_bytes = 0;          // ... and its share of device_bytes
  DevPtr<int32_t> d_groups;       // [n_docs] the group of every document (np_hip_index_set_groups, np_group.hip); unsharded only
  int64_t n_groups = 0;           // 0 = no groups set
  size_t group_bytes = 0;         // ... and their share of device_bytes
  size_t device_bytes = 0;
  np_open_opts opts{};
  // per-context scratch budget the planner uses.  A caller-given workspace_bytes is kept as it is; the default (what the device
  // had free at open, np_index.hip default_workspace) is re-clamped against what is free NOW whenever a candidate pool has to
  // grow, and halved when a reservation still fails: a second index opened on the device (the "swap handles" reload pattern),
  // or an encoder allocating later, shrinks the pool (more rounds) instead of failing the search with OutOfMemory.
  mutable std::atomic<int64_t> ws_budget{0};
  int64_t ws_budget_open = 0;   // the budget at open: the live one grows back towards it when the device has headroom again
  bool ws_auto = false;
  Tuning tune;
  // zeroth filter level, run / skip policy (s3_gain = 1): batches left to skip, and the parameters the count belongs to
  mutable std::atomic<int> gain_skip{0};
  mutable std::atomic<int> gain_run{0};    // 1: the last report of these parameters said the level pays (no guard between batches)
  mutable std::atomic<uint64_t> gain_key{0};
  CodeArr codes() const { return CodeArr{d_codes.get(), code_wide}; }
  CodeArr ucodes() const { return CodeArr{d_ucodes.get(), code_wide}; }
  size_t code_bytes() const { return code_wide ? 4 : 2; }
  // context pool
  mutable std::mutex mu;
  mutable std::condition_variable cv;
  mutable std::vector<Context*> contexts;
  mutable uint64_t use_clock = 0;
  mutable bool exclusive = false;   // np_hip_index_append / _remove / _reserve hold every context: acquire_context waits (under mu)
  mutable int readers = 0;          // calls registered with IndexRead (under mu): an append waits for them too
};

// Any index the crate can write is searchable up to dim 128: rows are stored zero-padded to the next instantiated width
// (queries are padded with zeros too, so the padded dims add exact zeros to every dot product; norms and outputs stop at
// ldim), and 1-bit residuals are stored as 2-bit ones (bucket b -> segment b << 1, weights {w0, w1, 0, 0}: the same values).
// 8-bit residuals keep their layout and take the all-f32 S6 kernel at every precision.  codec.rs:161-166 accepts nbits
// in {1, 2, 4, 8} and any dim with dim * nbits % 8 == 0.
static inline int storage_dim(int dim) { return dim <= 0 || dim > 128 ? dim : (dim + 31) / 32 * 32; }
static inline int storage_nbits(int dim, int nbits) { return (nbits == 1 && dim <= 128) ? 2 : nbits; }

// np_index.hip
int build_device_index(const HostIndex& h, const np_open_opts* opts, DeviceIndex** out);
void destroy_device_index(np_index* ix);   // the contexts, then the handle and its arrays, on the index's device
int normalise_opts(const np_open_opts* in, np_open_opts* out);
void read_tuning_env(Tuning* t);
bool set_tuning(Tuning* t, const std::string& name, int value);   // shared clamp table (environment + np_hip_index_tune)
void shard_range(int64_t n_total, int rank, int count, int64_t* b, int64_t* e);

// np_search.hip
// A call that reads the handle OUTSIDE a context -- the checks of its columns, keyword index and groups before it takes one,
// the keyword index's host tables, the token arrays np_hip_decompress_documents reads -- registered from its first line to its
// last: np_hip_index_append / _reserve wait until no such call runs and, once they hold the handle, later ones wait here.  So
// a call sees the attachments it checked, or none; never a handle that changed under it.  Re-entrant per thread; a registered
// thread's acquire_context does not wait for the append that is waiting for it.
struct IndexRead {
  const DeviceIndex* ix = nullptr;
  explicit IndexRead(const DeviceIndex* index);
  ~IndexRead();
  IndexRead(const IndexRead&) = delete;
  IndexRead& operator=(const IndexRead&) = delete;
};
// every context of the handle's pool checked out (DeviceIndex::exclusive; np_hip_index_append / _remove / _expand / _reserve and
// np_hip_index_set_text_build): running calls finish on the index as it was, calls that arrive wait in acquire_context, and
// nobody sees a half-changed handle
struct HoldContexts {
  const DeviceIndex* ix;
  explicit HoldContexts(const DeviceIndex* i) : ix(i) {
    std::unique_lock<std::mutex> lk(ix->mu);
    ix->cv.wait(lk, [&] { return !ix->exclusive; });
    ix->exclusive = true;
    ix->cv.wait(lk, [&] {   // the calls registered outside a context (IndexRead) end, then the contexts fall idle
      if (ix->readers > 0) return false;
      for (const Context* c : ix->contexts)
        if (c->busy) return false;
      return true;
    });
    for (Context* c : ix->contexts) c->busy = true;
  }
  ~HoldContexts() {
    {
      std::lock_guard<std::mutex> lk(ix->mu);
      for (Context* c : ix->contexts) c->busy = false;
      ix->exclusive = false;
    }
    ix->cv.notify_all();
  }
};
void destroy_context(Context* c);
// after np_hip_index_append (every context held): the contexts forget what they learnt about the index they served
void contexts_forget_index(const DeviceIndex* ix);
// np_hip_encode_tokens with an optional third output: norms[t] = |x_t - c[code_t]| (sequential f32 sum, no contraction)
int encode_tokens_impl(const np_index* index, const float* embeddings, int64_t n_tokens, int32_t dim,
                       const float* bucket_cutoffs, int64_t* out_codes, uint8_t* out_packed, float* out_norms);
// document-sharded exchange on records with a per-rank status trailer (np_dist.hip); the C ABI's np_hip_select_cut /
// np_hip_merge_packed are the status-free cases
int select_cut_strided(const DeviceIndex* ix, const uint64_t* d_all_keys, int64_t rank_stride, int64_t status_off, int G,
                       int B, int n_sel, uint64_t* d_cut, hipStream_t st);
bool select_cut_fits(int G, int n_sel);
// the CSR arguments of the per-query-subset entry points (np_search.hip), checked before any launch or collective
int check_subsets(const void* ids, const int64_t* h_off, int64_t n_subsets, const void* qsub, const int32_t* h_qsub, int B);
int check_device_subsets(const void* d_ids, const int64_t* d_off, const int64_t* h_off, int64_t n_subsets, const void* d_qsub,
                         int B);
int merge_packed_status(const DeviceIndex* ix, const void* d_records, int64_t record_bytes, int64_t off_keys,
                        int64_t off_scores, int64_t off_counts, int64_t off_status, uint64_t* h_status, int G, int B,
                        int top_k, int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, hipStream_t st);
int set_status_word(const DeviceIndex* ix, uint64_t* d_word, uint64_t value, hipStream_t st);

// np_search.hip, for the host entry points outside the search pass (exact scan, pair scoring, filters, keyword and hybrid
// search): a context of the handle's pool checked out for one call -- begin() waits for the workspace's previous use on the
// call's stream, the destructor records the end of this one and hands the context back.  arena() is the context's one device
// allocation for such a call (grown on demand, never shrunk, counted in the workspace like every other buffer); pin() its
// pinned host staging area.
struct ContextUse {
  const DeviceIndex* ix = nullptr;
  Context* ctx = nullptr;
  hipStream_t stream = nullptr;
  bool began = false;
  int begin(const DeviceIndex* index, void* user_stream);
  DevBuf& arena() const;
  DevBuf& filter_scratch() const;   // masks, counts and programs of a filter evaluation (np_filter.hip)
  DevBuf& filter_csr() const;       // the CSR a filtered search evaluates its filters into
  int pin(size_t bytes, void** out) const;
  int end();   // records the end of the use now (the destructor then only releases)
  ~ContextUse();
};

// ---- what the host entry points share: the carve-up of a reserved region, a call's scope, its result staging ---------------
static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
// a reserved region handed out in 256-byte aligned pieces
struct Carver {
  char* at;
  char* take(size_t bytes) {
    char* r = at;
    at += up256(bytes);
    return r;
  }
};
// a batch none of whose queries has a subset (or a filter) is a batch without subsets
static inline bool any_scoped(const int32_t* query_subset, int64_t n, int B) {
  bool any = false;
  for (int b = 0; n > 0 && b < B; ++b) any = any || query_subset[b] >= 0;
  return any;
}
// A call's scope -- the documents each query may see -- as every pass takes it: a CSR of subsets on the device with one
// subset (or -1) per query, plus the host's copies of the offsets and -- where the caller has it, NULL otherwise -- of the
// query map: with both a pass builds only the id range its own queries reference.  n == 0: no scope.
struct CallSubsets {
  const int64_t* d_ids = nullptr;
  const int64_t* d_off = nullptr;
  const int32_t* d_qsub = nullptr;
  int64_t n = 0, total = 0;
  const int64_t* h_off = nullptr;
  const int32_t* h_qsub = nullptr;
  bool any() const { return n > 0; }
  // the checked CSR arguments of a device-side entry point; h_qsub: the host's copy of the query map, where there is one
  static CallSubsets device(const int64_t* d_ids, const int64_t* d_off, const int64_t* h_off, int64_t n_subsets,
                            const int32_t* d_qsub, const int32_t* h_qsub = nullptr) {
    CallSubsets s;
    if (n_subsets <= 0) return s;
    s.d_ids = d_ids;
    s.d_off = d_off;
    s.d_qsub = d_qsub;
    s.n = n_subsets;
    s.total = h_off[n_subsets];
    s.h_off = h_off;
    s.h_qsub = h_qsub;
    return s;
  }
};
// the document bitmaps of a pass's subsets (subset_rows_kernel + subset_kernel without the eligible-centroid side):
// qrow[B] = the row of query b (-1: no subset), docbits[row][NW] over the shard's documents.  CSR arguments on the device,
// ids [lo, hi) are the ones the pass's queries reference.
int subset_doc_rows(const DeviceIndex* ix, hipStream_t st, const int64_t* d_ids, const int64_t* d_off, const int32_t* d_qsub,
                    int64_t n_subsets, int64_t total, int64_t lo, int64_t hi, int B, int64_t NW, uint32_t* docbits,
                    int32_t* qrow);

// np_filter.hip: a call's filters evaluated on `st` into a CSR that stays on the device.  `out` receives ids [total] i64 |
// offsets [n_filters + 1] i64 | query map [B] i32 (the arguments of the per-query-subset pass), `scratch` the masks and
// counts; both are reserved here.  h_off gets the offsets; synchronises `st` once.  *ms = wall time of the evaluation.
struct FilterCsr {
  const int64_t* d_ids = nullptr;
  const int64_t* d_off = nullptr;
  const int32_t* d_qsub = nullptr;
  std::vector<int64_t> h_off;
  float ms = 0.f;
};
// the checks of the filtered entry points that need no device: the programs, the query map, the handle (columns, no shards).
// for_search: 0 = np_hip_filter_eval, 1 = a search without a communicator (a sharded handle is refused), 2 = a sharded search
int filter_check_call(const DeviceIndex* ix, const np_filter* filters, int32_t n_filters, const int32_t* query_filter, int B,
                      int for_search);
// np_match.hip: the NP_F_MATCH leaves of a call's filters, whose programs filter_check_program has passed (columns, value ranges,
// well-formed DFAs: the tables are checked there, once).  match_check_text refuses a leaf over a column without text;
// match_collect lists the distinct (column, DFA) jobs; bit_words = what their bitmaps over codes take together, work_bytes
// the images of the largest one.  match_run_jobs writes the bitmaps to d_bits (job j at d_bits + jobs[j].bit_word0), one DFA at a
// time through d_work; enqueues on st and synchronises it.
struct MatchJob {
  int32_t column;
  const int64_t* words;   // host, inside the filter's values
  int64_t n_words, image_bytes;
  int64_t bit_word0;      // the job's bitmap: u32 words at this offset, one bit per code
};
int match_check_text(const DeviceIndex* ix, const np_filter* filters, int32_t n_filters);
int match_collect(const DeviceIndex* ix, const np_filter* filters, int32_t n_filters, std::vector<MatchJob>* jobs,
                  std::vector<int64_t>* op_bit_word0, int64_t* bit_words, int64_t* work_bytes);
int match_run_jobs(const DeviceIndex* ix, hipStream_t st, const std::vector<MatchJob>& jobs, uint32_t* d_bits, char* d_work);

int filter_eval_resident(const DeviceIndex* ix, hipStream_t st, DevBuf& scratch, DevBuf& out, const np_filter* filters,
                         int32_t n_filters, const int32_t* h_query_filter, int B, FilterCsr* csr);

// The scope of a host entry point (np_search.hip), in two steps because the arena is reserved between them.  The scope comes as
// a host CSR, or (filters != NULL) as n_subsets filters that resolve() evaluates on the call's context into a CSR that stays on
// the device; query_subset is the query map of either.  The object owns that evaluation's FilterCsr -- the host offsets of the
// CallSubsets point into it -- so it lives as long as the call and is not copied.
struct HostScope {
  bool any = false;        // some query has a subset
  bool resident = false;   // ... and the CSR is on the device already (filters)
  int64_t total = 0;       // ids of all subsets together
  int resolve(const DeviceIndex* ix, ContextUse& use, const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
              const int32_t* query_subset, const np_filter* filters, int B);
  bool staged() const { return any && !resident; }   // the CSR is copied into the arena
  size_t stage_bytes() const {
    return staged() ? up256((size_t)std::max<int64_t>(total, 1) * 8) + up256((size_t)(n + 1) * 8) + up256((size_t)B * 4) : 0;
  }
  int64_t budget_extra() const { return resident ? total * 8 : 0; }   // a filter's CSR lives outside the arena but inside the budget
  float ms() const { return csr.ms; }   // wall time of the filters' evaluation
  // carves stage_bytes() and enqueues the CSR's upload on st (staged), or points at the evaluated one
  int place(Carver& carve, hipStream_t st, CallSubsets* sub) const;
  HostScope() = default;
  HostScope(const HostScope&) = delete;
  HostScope& operator=(const HostScope&) = delete;

 private:
  FilterCsr csr;
  const int64_t *ids = nullptr, *off = nullptr;
  const int32_t* qsub = nullptr;
  int64_t n = 0;
  int B = 0;
};

// The results of a host entry point, [B][top_k] ids and scores and [B] counts: carved out of the arena, copied back through the
// head of the pinned area (whatever else a call pins lies behind bytes()), handed to the caller once the stream is synchronised.
struct ResultStage {
  size_t n, B;                  // B * top_k, B
  size_t o_ids, o_sc, o_cnt;    // the three regions' sizes
  int64_t* d_ids = nullptr;
  float* d_sc = nullptr;
  int32_t* d_cnt = nullptr;
  char* pin = nullptr;
  ResultStage(int B_, int top_k)
      : n((size_t)B_ * top_k), B((size_t)B_), o_ids(up256(n * 8)), o_sc(up256(n * 4)), o_cnt(up256(B * 4)) {}
  size_t bytes() const { return o_ids + o_sc + o_cnt; }   // of the arena, and of the pinned area
  void carve(Carver& c) {
    d_ids = (int64_t*)c.take(o_ids);
    d_sc = (float*)c.take(o_sc);
    d_cnt = (int32_t*)c.take(o_cnt);
  }
  int fetch(void* pinned, hipStream_t st);   // the three copies to the host, enqueued
  void deliver(int64_t* out_ids, float* out_scores, int32_t* out_counts) const;
};

// np_search.hip: the pass of np_hip_search_batch_subsets_device on a context the caller already holds (np_hip_search_hybrid
// runs the semantic and the keyword pass on one context and one stream).
int search_batch_in_use(const DeviceIndex* ix, ContextUse& use, const float* d_q, const int32_t* d_qoff, const int32_t* h_qoff,
                        int B, int dim, const np_search_params* prm, const CallSubsets& scope, int64_t* d_out_ids,
                        float* d_out_scores, int32_t* d_out_counts);

// np_group.hip: the outputs of a grouped host entry point -- [B][top_k][group_size] ids and scores, [B][top_k] group, members
// and total, [B] counts -- staged as ResultStage stages its three: carved out of the arena, copied back through the head of
// the pinned area, handed to the caller once the stream is synchronised.  The score regions exist even where nobody asks for
// them (a list without scores): the layout does not depend on it.
struct GroupStage {
  size_t n, g, B;                             // B * top_k * group_size, B * top_k, B
  size_t o_ids, o_sc, o_g, o_cnt;             // the regions' sizes (group, members and total share o_g)
  int64_t* d_ids = nullptr;
  float* d_sc = nullptr;
  int32_t *d_group = nullptr, *d_members = nullptr, *d_total = nullptr, *d_cnt = nullptr;
  char* pin = nullptr;
  bool scores = true;
  GroupStage(int B_, int top_k, int group_size)
      : n((size_t)B_ * top_k * group_size), g((size_t)B_ * top_k), B((size_t)B_), o_ids(up256(n * 8)), o_sc(up256(n * 4)),
        o_g(up256(g * 4)), o_cnt(up256(B * 4)) {}
  size_t bytes() const { return o_ids + o_sc + 3 * o_g + o_cnt; }
  void carve(Carver& c) {
    d_ids = (int64_t*)c.take(o_ids);
    d_sc = (float*)c.take(o_sc);
    d_group = (int32_t*)c.take(o_g);
    d_members = (int32_t*)c.take(o_g);
    d_total = (int32_t*)c.take(o_g);
    d_cnt = (int32_t*)c.take(o_cnt);
  }
  int fetch(void* pinned, hipStream_t st, bool with_scores);
  void deliver(int64_t* out_ids, float* out_scores, int32_t* out_group, int32_t* out_members, int32_t* out_total,
               int32_t* out_counts) const;
};
// the scalar checks of a collapse (np_group_plan.h) against the handle, with the error set; then collapse_kernel on `st`:
// B lists [B][stride] (d_scores may be NULL, and then d_out_scores is not written) to top_k groups of at most group_size
int collapse_check(const DeviceIndex* ix, int32_t top_k, int32_t group_size, int32_t B, int32_t stride);
int collapse_launch(const DeviceIndex* ix, hipStream_t st, int32_t top_k, int32_t group_size, int32_t B, const int64_t* d_ids,
                    const float* d_scores, const int32_t* d_counts, int32_t stride, int64_t* d_out_ids, float* d_out_scores,
                    int32_t* d_out_group, int32_t* d_out_members, int32_t* d_out_total, int32_t* d_out_counts);
// the grouped part of np_hip_search_hybrid_grouped's arguments (np_text.hip runs the hybrid request, fused to pool_k)
struct GroupCall {
  int32_t pool_k, group_size;
  int32_t *out_group, *out_members, *out_total;
};

// np_search.hip: np_hip_search_phase_a_subsets with the subsets' GLOBAL lengths on the device (d_global_lens[n_subsets], NULL =
// the CSR's own): what the probe scaling reads when the CSR holds only a shard's part of every subset
int search_phase_a_subsets_lens(const np_index* ix, const float* d_queries, const int32_t* d_q_tok_offsets,
                                const int32_t* h_q_tok_offsets, int32_t B, int32_t dim, const np_search_params* params,
                                const int64_t* d_subset_ids, const int64_t* d_subset_offsets, const int64_t* h_subset_offsets,
                                int64_t n_subsets, const int32_t* d_query_subset, const int64_t* d_global_lens,
                                const uint32_t* d_elig_global, uint64_t* d_sel_keys, void* stream, void** call_state);

struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

}  // namespace np

struct np_index : np::DeviceIndex {};

// The communicator of the sharded entry points (np_dist.hip; the keyword and hybrid calls of np_text.hip use it too).  Opaque
// to the ABI.  Every buffer is grow-only and belongs to the one protocol pass the mutex admits at a time.
struct np_comm {
  void* comm = nullptr;                      // ncclComm_t, or NULL
  np_all_gather_host_fn host_fn = nullptr;   // hosted transport (np_hip_comm_create_hosted): the host moves the bytes
  void* host_ctx = nullptr;
  int host_flags = 0;
  int rank = 0, nranks = 1, device = 0;
  np::DevBuf keys_local, keys_all, cut, pack_local, pack_all, elig_local, elig_all, elig_global;
  // filters of a sharded call: the evaluation's scratch, the shard's CSR, the subsets' global lengths
  np::DevBuf filt, filt_csr, glen;
  // keyword search: the counting record and the result record of a rank, the gathered ones, the whole batch's local lists where
  // it takes several exchanges; hybrid: the two global lists
  np::DevBuf tx_cnt_local, tx_cnt_all, tx_local, tx_all, tx_src, lists;
  char* h_stage = nullptr;       // pinned staging of the hosted transport: [send | recv x nranks]
  size_t h_stage_cap = 0;
  char* h_small = nullptr;       // pinned: a call's small host-side figures on their way to or from the device
  size_t h_small_cap = 0;
  uint64_t* h_status = nullptr;  // pinned, device-visible: the merge kernel leaves a failed rank's status word here
  std::mutex mu;   // one protocol pass at a time per communicator (RCCL orders a communicator's collectives)
  bool host_check() const { return host_fn && !(host_flags & NP_COMM_DEFERRED_STATUS); }
};

namespace np {

// np_dist.hip, for the calls that run more than one protocol pass under the communicator's mutex
// send -> recv[nranks][bytes] on st; *h_recv (hosted transport only, else NULL) = the gathered bytes in host memory
int comm_all_gather(np_comm* c, const void* send, void* recv, size_t bytes, hipStream_t st, const char** h_recv = nullptr);
int comm_small_pin(np_comm* c, size_t bytes, char** out);   // the pinned area, grown; reuse only after the stream was synchronised

// The subsets of a sharded call: the single-subset form (off == NULL: d_ids[len], len < 0 = None) or the CSR form with one
// subset per query.  Either way the shards' eligible bitmaps -- one row per subset -- cross the ranks in ONE all-gather.
// h_local_lens (filters): the CSR holds only this shard's part of every subset; the local lengths ride in that all-gather and
// the probe scaling reads their sums.
struct ShardSubsets {
  const int64_t* d_ids = nullptr;
  int64_t len = -1;
  const int64_t *d_off = nullptr, *h_off = nullptr;
  int64_t n = 0;
  const int32_t* d_qsub = nullptr;
  const int64_t* h_local_lens = nullptr;
  int64_t rows() const { return h_off ? n : (len > 0 ? 1 : 0); }   // eligible bitmaps to exchange
  static ShardSubsets none() { return ShardSubsets(); }
  static ShardSubsets single(const int64_t* d_ids, int64_t len) {
    ShardSubsets s;
    s.d_ids = d_ids;
    s.len = len;
    return s;
  }
  static ShardSubsets csr(const CallSubsets& c) {   // (a scope without subsets is none())
    ShardSubsets s;
    if (!c.any()) return s;
    s.d_ids = c.d_ids;
    s.len = 0;
    s.d_off = c.d_off;
    s.h_off = c.h_off;
    s.n = c.n;
    s.d_qsub = c.d_qsub;
    return s;
  }
  ShardSubsets with_local_lens(const int64_t* lens) const {
    ShardSubsets s = *this;
    s.h_local_lens = lens;
    return s;
  }
};
// np_hip_search_batch_sharded's pass; the caller holds c->mu.  rc0 / rc0_msg: a local failure the caller already met (its
// filters did not evaluate): the rank then takes part in every exchange with empty data and returns that error.
int search_batch_sharded_locked(const np_index* ix, np_comm* c, const float* d_queries, const int32_t* d_q_tok_offsets,
                                const int32_t* h_q_tok_offsets, int32_t B, int32_t dim, const np_search_params* params,
                                const ShardSubsets& ss, int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts,
                                void* stream, int rc0 = NP_OK, const char* rc0_msg = nullptr);

// the arguments of a sharded call's filters that need no handle; `who` starts the message
int check_sharded_filters(const char* who, const np_filter* filters, int32_t n_filters, const int32_t* query_filter, int B);

// The filters of a sharded call as its scope (np_dist.hip).  eval() -- the caller holds c->mu -- evaluates them over this
// shard's columns into the communicator's own buffers (np_filter.hip's checks first; a context of the handle stays free for
// the pass) and synchronises the stream.  A failure stays in rc0 / msg0 for the pass to carry through its exchanges: the rank
// then takes part with subsets that are all empty (shard()) and hands its own passes no scope (call()).  A batch none of
// whose queries has a filter evaluates nothing and has no scope.
struct ShardFilterScope {
  bool any = false;
  int rc0 = NP_OK;
  std::string msg0;
  void eval(const np_index* ix, np_comm* c, hipStream_t st, const np_filter* filters, int32_t n_filters,
            const int32_t* query_filter, int B);
  const CallSubsets& call() const { return sub; }
  ShardSubsets shard() const;   // with every filter's local length, for the probe scaling
  ShardFilterScope() = default;
  ShardFilterScope(const ShardFilterScope&) = delete;
  ShardFilterScope& operator=(const ShardFilterScope&) = delete;

 private:
  FilterCsr csr;
  CallSubsets sub;                  // empty after a failure
  std::vector<int64_t> zero, lens;  // offsets of a failed evaluation; the local lengths
  int32_t n = 0;
};

}  // namespace np
