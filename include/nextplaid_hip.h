/*
 * nextplaid_hip.h -- C ABI of the MI355X-native PLAID search path for next-plaid.
 *
 * This is the drop-in boundary: the entry points a `hip` cargo feature of the next-plaid crate
 * would bind (extern "C") to serve MmapIndex::{load, search, search_batch} from a gfx950 GPU
 * instead of the crate's CPU path.  Plain pointers and sizes only; no C++/torch types.
 * Each entry cites the reference interface it replaces (paths under /root/reference/next-plaid/src).
 *
 * Conventions
 *  - Every function returning int returns an np_status; 0 = ok.  Codes map onto the crate's
 *    error enum (error.rs:9-66): 1 IndexLoad, 2 Search, 3 Shape, 4 Codec, 5 Io, 6 DeviceUnavailable
 *    (the Rust wrapper falls back to its CPU path unless NEXT_PLAID_FORCE_GPU, mirroring
 *    cuda.rs:105-144), 7 OutOfMemory, 8 InvalidArgument.  Nothing aborts or throws across the ABI.
 *  - np_hip_last_error() is thread-local and valid until the next call on that thread.
 *  - An np_index is immutable after open; all search entry points are re-entrant and may be
 *    called concurrently on one shared handle from many threads (the crate shares &MmapIndex
 *    across tokio workers, next-plaid-api/src/state.rs:413-416).  Each call checks a private
 *    stream + workspace out of a small pool.
 *  - The caller allocates every output buffer; no allocation crosses the boundary.
 *  - Doc ids are GLOBAL i64 ids (position in the concatenation of doclens.*.json) even when the
 *    handle holds one document shard.
 */
#ifndef NEXTPLAID_HIP_H
#define NEXTPLAID_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NP_ABI_VERSION 6

typedef enum np_status {
  NP_OK = 0,
  NP_ERR_INDEX_LOAD = 1,         /* Error::IndexLoad  (error.rs:37) */
  NP_ERR_SEARCH = 2,             /* Error::Search     (error.rs:17) */
  NP_ERR_SHAPE = 3,              /* Error::Shape      (error.rs:29) */
  NP_ERR_CODEC = 4,              /* Error::Codec      (error.rs:41) */
  NP_ERR_IO = 5,                 /* Error::Io / Json  (error.rs:21,25) */
  NP_ERR_DEVICE_UNAVAILABLE = 6, /* no usable gfx950 device / HIP runtime failure */
  NP_ERR_OUT_OF_MEMORY = 7,
  NP_ERR_INVALID_ARGUMENT = 8,
  NP_ERR_INDEX_CREATION = 9      /* Error::IndexCreation (error.rs:13) */
} np_status;

typedef struct np_index np_index; /* opaque: device-resident index (or one document shard of it) */

/* Options for opening an index.  Zero-initialise, then set what you need. */
typedef struct np_open_opts {
  int32_t device;       /* HIP device ordinal (one process per GPU: pass LOCAL_RANK) */
  int32_t shard_rank;   /* this handle holds documents [N*rank/count, N*(rank+1)/count) */
  int32_t shard_count;  /* 0 or 1 = whole index */
  int32_t n_contexts;   /* concurrent search calls served without blocking (default 2) */
  int32_t max_batch;    /* workspace is sized for this many queries per call (default 64);
                           larger batches are processed in slices */
  int32_t max_query_tokens; /* per-query token cap used to size workspaces (default 64;
                           grows automatically, this is only the initial reservation) */
  int64_t workspace_bytes;  /* soft cap for per-context scratch (0 = default: the HBM left free by the resident index,
                               shared by the contexts, between 2 and 16 GiB) */
} np_open_opts;

/* Mirrors SearchParameters (search.rs:26-69).  batch_size is unused by search and omitted. */
typedef struct np_search_params {
  int32_t top_k;                  /* search.rs:34 */
  int32_t n_full_scores;          /* search.rs:32 */
  int32_t n_ivf_probe;            /* search.rs:36 */
  int32_t centroid_batch_size;    /* search.rs:41: K > this (and > 0) selects the batched-probe
                                     semantics of search.rs:140-254 */
  float centroid_score_threshold; /* search.rs:47 */
  int32_t has_threshold;          /* 0 = None */
  int32_t precision;              /* exact MaxSim stage (S1-S5 are always exact f32):
                                     0 = exact-f32 MFMA on decompressed rows (strict parity mode)
                                     1 = QC-reuse form, bf16 MFMA on the residual term
                                     2 = QC-reuse form, split-bf16 (hi/lo) MFMA: f32-class accuracy
                                     3 = bf16 MFMA on decompressed rows (plain bf16 MaxSim) */
} np_search_params;

typedef struct np_info {            /* accessors of index.rs:1290-1312 */
  int64_t num_documents;            /* whole index */
  int64_t num_embeddings;           /* whole index (metadata.json) */
  int64_t num_partitions;           /* K */
  int32_t embedding_dim;
  int32_t nbits;
  double avg_doclen;
  int64_t shard_doc_begin, shard_doc_end; /* documents held by this handle */
  int64_t shard_embeddings;         /* tokens held by this handle */
  int64_t device_bytes;             /* HBM held by the index (without workspaces) */
  int32_t device;
  int32_t abi_version;
  int64_t workspace_bytes;          /* ABI v5: the LIVE per-context scratch budget (np_open_opts.workspace_bytes, or the
                                       default, which shrinks under memory pressure and grows back; 0 from probe_dir) */
} np_info;

/* Per-call stage timings (HIP events on the call's stream) and work counters.  Optional. */
typedef struct np_stats {
  float ms_total;        /* first launch -> results ready */
  float ms_centroid;     /* S1  Q.C^T (MFMA) + group maxima */
  float ms_probe;        /* S2  top-nprobe per token, threshold, cell list */
  float ms_candidates;   /* S3  posting-list union (bitmap) + compaction; since round 5 also the hot level's thresholds and plane
                            rows (they follow the candidate count), since round 6 the zeroth filter level (three sweeps of the
                            posting lists + the exact bound of its S0 list) */
  float ms_approx;       /* S4  approximate scores (codes x QC gather) */
  float ms_select;       /* S5  top n_full_scores/4 by approximate score */
  float ms_exact;        /* S6  decompress + MaxSim (MFMA) */
  float ms_topk;         /* S7  final top-k */
  int64_t n_cells;       /* probed cells after threshold, summed over the batch */
  int64_t n_ivf_ids;     /* posting-list entries read */
  int64_t n_candidates;  /* unique candidate documents */
  int64_t n_cand_tokens; /* sum of candidate doc lengths (codes read by S4) */
  int64_t n_exact_docs;  /* documents exact-scored */
  int64_t n_exact_tokens;/* tokens decompressed by S6 */
  int64_t n_cand_codes;  /* u8 table rows gathered by the S4 filter (both levels); without the filter: f32 rows */
  int32_t n_queries;
  int32_t n_rounds;      /* candidate-pool rounds (1 unless the batch's candidates overflowed workspace_bytes) */
  int64_t n_survivors;   /* candidates that passed the S4 upper-bound filter and got an exact approximate score */
  int64_t n_cand_dcodes; /* distinct (document, code) pairs of the candidates (<= n_cand_tokens) */
  int64_t n_level2;      /* two-level filter: documents that took the exact u8 bound after the hot bound */
  float ms_hot_level;    /* ABI v5: the first filter level's launch alone (approx_hotp_kernel / approx_hot_kernel of round 0;
                            part of ms_approx; 0 when the two-level filter does not apply) */
  int32_t reserved0;
  int64_t n_level0;      /* ABI v6: candidates the zeroth filter level (per-document sums of the probed cells' gains, S3) handed to
                            the filter; n_candidates stays the size of the posting-list union; 0 when the level did not run */
} np_stats;

/* ---- runtime ------------------------------------------------------------------------------ */

/* Number of usable gfx950 devices (0 if none / no HIP runtime).  Replaces the role of
 * cuda::get_global_context().is_some() (cuda.rs:105-144) for the search path. */
int np_hip_device_count(void);

/* Thread-local description of the last error on this thread ("" if none). */
const char* np_hip_last_error(void);

/* ABI v6: the library's NP_ABI_VERSION, readable BEFORE any struct crosses the boundary.  np_info and np_stats are
 * caller-allocated and have grown (v5: np_info.workspace_bytes, np_stats.ms_hot_level): a host compiled against an older
 * header would have bytes written past its structs before it could read np_info.abi_version.  A host binds this first and
 * refuses a library whose version differs from the header it was built with; np_hip_struct_size lets it check the two
 * layouts it allocates (which: 0 = np_info, 1 = np_stats, 2 = np_search_params, 3 = np_open_opts, 4 = np_kmeans_opts,
 * 5 = np_kmeans_report, 6 = np_index_config, 7 = np_kmeans_plan, 8 = np_update_config, 9 = np_update_report,
 * 10 = np_pool_opts, 11 = np_pool_report, 12 = np_text_expr; -1 for an unknown id). */
int np_hip_abi_version(void);
int64_t np_hip_struct_size(int32_t which);

/* ---- index lifecycle ------------------------------------------------------------------------ */

/* MmapIndex::load (index.rs:1026-1139): reads the crate's on-disk index directory unchanged
 * (metadata.json, centroids.npy, bucket_weights.npy, ivf.npy, ivf_lengths.npy, doclens.N.json,
 * N.codes.npy, N.residuals.npy; NPY v1/v2) and makes it resident in HBM.  The merged_*.npy caches
 * are not needed: chunks are concatenated in the same order. */
int np_hip_index_open(const char* index_dir, const np_open_opts* opts, np_index** out);

/* Same index, built from host arrays in the on-disk dtypes instead of files (what
 * MmapIndex holds after load: index.rs:995-1016).  doc ids in `ivf` are global; with sharding
 * the arrays may cover only the shard's documents (doc_begin = first global id) or the whole
 * index (doc_begin = 0, the shard range is cut out here).  bucket_cutoffs may be NULL. */
typedef struct np_index_arrays {
  int64_t num_documents_total;  /* N of the whole index */
  int64_t doc_begin;            /* global id of doc_lengths[0] */
  int64_t num_docs;             /* entries in doc_lengths */
  int64_t num_centroids;        /* K */
  int32_t dim, nbits;
  const float* centroids;       /* [K, dim] */
  const float* bucket_weights;  /* [2^nbits] */
  const int64_t* ivf;           /* concatenated posting lists of global doc ids: any entries give the reference's
                                   answer (candidates = union of the probed lists, scores from the codes).  The crate
                                   writes list c = the ascending ids of the documents holding code c; only lists that
                                   strictly ascend AND hold every (document, code) pair of the shard enable the zeroth
                                   filter level (checked at open), other lists are served without it */
  const int32_t* ivf_lengths;   /* [K] */
  const int64_t* doc_lengths;   /* [num_docs] */
  const int64_t* codes;         /* [sum doc_lengths] */
  const uint8_t* residuals;     /* [sum doc_lengths, dim*nbits/8] */
} np_index_arrays;
int np_hip_index_from_arrays(const np_index_arrays* arrays, const np_open_opts* opts, np_index** out);

/* Seeded synthetic corpus generated directly in HBM (bench / large-scale tests; the generator
 * spec is next-plaid_amd/next_plaid_amd/synth.py, bit-identical).  centroids / bucket_weights
 * are host arrays.  Sharding as in np_open_opts. */
typedef struct np_synth_spec {
  int64_t num_docs;             /* whole corpus */
  int64_t num_centroids;
  int32_t dim, nbits;
  int32_t doc_len_min, doc_len_max;
  int32_t n_topics, rand256;
  uint64_t seed;
  const float* centroids;       /* [K, dim] */
  const float* bucket_weights;  /* [2^nbits] */
  const int32_t* len_table;     /* optional: document length = len_table[hash(doc) % len_table_size] (a quantile table,
                                   e.g. the clipped LogNormal of MS MARCO passages) instead of uniform [doc_len_min, doc_len_max] */
  int32_t len_table_size;       /* 0 = none */
} np_synth_spec;
int np_hip_index_synth(const np_synth_spec* spec, const np_open_opts* opts, np_index** out);

/* Copies the shard held by a handle back to host arrays in the on-disk dtypes (ivf ids global).
 * Pass NULL for any array not wanted.  Sizes come from np_hip_index_info / np_hip_index_ivf_size. */
int np_hip_index_export(const np_index* index, int64_t* doc_lengths, int64_t* codes, uint8_t* residuals,
                        int64_t* ivf, int32_t* ivf_lengths);
int64_t np_hip_index_ivf_size(const np_index* index);

/* Host only (no device): writes host arrays as an index DIRECTORY in the crate's on-disk format -- the canonical file
 * set of write_index_from_encoded_chunks (index.rs:373-528): centroids / bucket_cutoffs / bucket_weights / avg_residual /
 * cluster_threshold .npy, plan.json, per chunk of <= chunk_docs documents {i}.metadata.json, doclens.{i}.json,
 * {i}.codes.npy, {i}.residuals.npy, then ivf.npy, ivf_lengths.npy and metadata.json.  NPY 1.0 headers padded to 64 bytes
 * (mmap.rs:1176-1250), every file via temporary name + fsync + rename (utils.rs:16-60).  arrays->ivf / ivf_lengths may
 * be NULL: the posting lists (ascending unique document ids per centroid, index.rs:479-504) are then built from the
 * codes.  arrays must hold the whole index (doc_begin = 0).  With np_hip_encode_tokens this is the index-build path:
 * encode on the GPU, write here, and MmapIndex::load (the crate's or np_hip_index_open) reads the result. */
typedef struct np_write_opts {
  int64_t chunk_docs;           /* documents per chunk; 0 = 50 000 (IndexConfig.batch_size, index.rs:92) */
  const float* bucket_cutoffs;  /* [2^nbits - 1] or NULL (file not written; search does not read it) */
  const float* avg_residual;    /* [dim] or NULL = zeros (not used by search arithmetic) */
  float cluster_threshold;      /* update path only (update.rs:372) */
} np_write_opts;
int np_hip_index_write_dir(const char* index_dir, const np_index_arrays* arrays, const np_write_opts* opts);

/* Kernel-selection knobs (no reference counterpart).  Each knob is read from the environment once, at open, as
 * NP_<UPPER-CASE NAME>, and can be changed on a live handle with this call (sweep tools, kernel-variant parity tests);
 * both paths clamp through one table.  Knobs: "s4_mode" 0..8, "s4_minb" >= 1, "s4_nbx" 8..512, "s4_swz" 0/1,
 * "s4_filter" 0/1, "s4_hot" 0..500 (per-mille of hot centroids in the first filter level; 0 = single-level filter),
 * "s4_planes" 0/1 (first level in bit planes; read at open too: it sets the list-block cap), "s4_pexp" 5..40, "s4_lpd" 2/4,
 * "s4_qm" 0/1, "s4_pnbx" 8..512, "s4_warm" 0..1000 (per-mille of centroids whose rows the exact filter level still gathers
 * for the S2 lists; 1000 = every row; 0 = the default: by query length and mean distinct-code count), "s4_hot_auto" >= 0 (candidates
 * per query up to which "s4_hot" applies as given; beyond it the share falls with the count^(-1/3); 0 = always as given),
 * "ub_ncut" 1..512, "s3_bisect" 0/1, "s3_gain" 0/1/2 (zeroth filter level in S3: 0 = off -- read at open too: its range table is not built --, 2 = whenever it
 * applies, 1 = the default: 2 with a run / skip policy fed by the previous batches' pruning; with a centroid_score_threshold it starts skipped),
 * "s3_gain_mult" 1..16, "s3_gain_direct" 0..64, "s1_split" 0/1 (the only knob that changes values: see INTEGRATION.md),
 * "s3_slices" 0/1, "ub_nt" 0..2, "ub_steal" >= 1, "ub_nbx" 8..256, "ub_direct" 0..16, "ub_static" 0/1, "hot_static" 0/1, "s6_xcd" 0/1, "s6_tiles" 0/1, "s6_lds" 0..2, "gemm_cpw" 1/2, "exact_rowmax" 0/1,
 * "scan_tiles" 1..8 (np_hip_search_exact: 32-token query tiles per workgroup), "scan_docs" >= 0 (documents per pass; 0 = what the budget holds).
 * Results are identical for every setting except "s1_split"; not synchronised with concurrent searches.  Unknown name:
 * NP_ERR_INVALID_ARGUMENT.  (A library built with -DNP_DIAGNOSTICS also accepts "s4_probe" 0..7, a phase-skipping timing
 * probe whose results are invalid; production builds reject the name and never read it from the environment.) */
int np_hip_index_tune(np_index* index, const char* name, int32_t value);

void np_hip_index_close(np_index* index);               /* Drop for MmapIndex */
int np_hip_index_info(const np_index* index, np_info* out); /* index.rs:1290-1312 */

/* ---- search ------------------------------------------------------------------------------------ */

/* MmapIndex::search_batch (index.rs:1279-1287 -> search.rs:643-675); MmapIndex::search
 * (index.rs:1258-1265) is the B = 1 case.
 *   queries        row-major f32, all queries' token rows concatenated: [q_tok_offsets[B], dim]
 *   q_tok_offsets  B+1 prefix offsets (query i owns rows [off[i], off[i+1]))
 *   subset         optional pre-filter doc ids (search.rs:350-382,434-437); subset_len < 0 = None,
 *                  subset_len == 0 = empty subset (every result empty)
 *   out_ids/out_scores  [B * top_k], query i at [i*top_k, i*top_k + out_counts[i]); scores descending
 *   out_counts     [B]
 * Host pointers; H2D/D2H copies are inside the call.
 * Geometry: every index the crate writes with embedding_dim <= 128 is searchable -- nbits 1, 2, 4, 8 (codec.rs:161-166),
 * any dim with dim * nbits % 8 == 0.  `dim` here, np_info.embedding_dim / nbits, decompressed rows, exported and encoded
 * residual rows are always in the geometry of the index FILES; inside, rows are stored at the next of the four kernel
 * widths (32 / 64 / 96 / 128, zero-padded) and 1-bit buckets as 2-bit segments.  A wider index opens (info, decompress,
 * export work) and search returns NP_ERR_SHAPE: the wrapper's signal to take the CPU path. */
int np_hip_search_batch(const np_index* index, const float* queries, const int32_t* q_tok_offsets,
                        int32_t B, int32_t dim, const np_search_params* params,
                        const int64_t* subset, int64_t subset_len,
                        int64_t* out_ids, float* out_scores, int32_t* out_counts, np_stats* stats);

/* Same call with every buffer already resident in HBM on `index`'s device and the work enqueued on
 * `stream` (a hipStream_t; NULL = the context's own stream).  Returns after enqueueing; the caller
 * synchronises the stream.  `stats` (host) is filled only by np_hip_search_batch.  This is what a
 * multi-GPU host and bench.py use (queries resident, results consumed on device by the merge). */
int np_hip_search_batch_device(const np_index* index, const float* d_queries,
                               const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets,
                               int32_t B, int32_t dim, const np_search_params* params,
                               const int64_t* d_subset, int64_t subset_len,
                               int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts,
                               void* stream);

/* ---- one subset per query (per-request filters) -------------------------------------------------
 * The crate's search_batch takes ONE subset because it batches inside one request; a GPU service batches ACROSS requests, and
 * each request brings its own filter.  These entry points take, per batch,
 *   subset_ids / subset_offsets   n_subsets distinct subsets in CSR form: subset s owns subset_ids[subset_offsets[s] ..
 *                                 subset_offsets[s + 1]); subset_offsets has n_subsets + 1 entries, starts at 0 and never
 *                                 decreases
 *   query_subset                  [B]: the subset of query i, or -1 for none
 * and give query i exactly what the single-subset call returns for query i and its subset alone (search.rs:350-382 and
 * :434-437 on the dense path, :542-545 -- candidate retain only -- where K > centroid_batch_size): duplicate ids, ids outside
 * [0, num_documents) and the subset's length as given count as they do there, an empty subset empties that query's result and
 * no other, and a query with -1 is searched as in a batch without subsets.  Queries that share a filter should share one
 * subset: its bitmaps are built once per pass, not once per query.  n_subsets == 0 is a batch without subsets.  The
 * single-subset calls above are the case n_subsets = 1 with every query mapped to subset 0; all of them run the same pass.
 * A pass in which any query has a subset plans its candidate pool for num_documents per query and runs without the
 * zeroth filter level, as a single-subset pass does -- also for its queries without one.
 * Errors, before any launch (NP_ERR_INVALID_ARGUMENT): subset_offsets[0] != 0 or decreasing offsets; a NULL array with a
 * positive count (n_subsets > 0 without offsets or query_subset, ids counted without subset_ids); a query_subset entry
 * < -1 or >= n_subsets.  The last is checked only where query_subset is a host array: on the device-side entry points an
 * entry outside [0, n_subsets) reads as -1. */
int np_hip_search_batch_subsets(const np_index* index, const float* queries, const int32_t* q_tok_offsets,
                                int32_t B, int32_t dim, const np_search_params* params,
                                const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
                                const int32_t* query_subset,
                                int64_t* out_ids, float* out_scores, int32_t* out_counts, np_stats* stats);
/* The same with every buffer in HBM; the offsets are passed twice, on the device and as a host copy (as the queries' token
 * offsets are).  Enqueues on `stream` and returns. */
int np_hip_search_batch_subsets_device(const np_index* index, const float* d_queries,
                                       const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets,
                                       int32_t B, int32_t dim, const np_search_params* params,
                                       const int64_t* d_subset_ids, const int64_t* d_subset_offsets,
                                       const int64_t* h_subset_offsets, int64_t n_subsets,
                                       const int32_t* d_query_subset,
                                       int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts,
                                       void* stream);

/* ---- exhaustive exact search ----------------------------------------------------------------------
 * The exact answer (no reference counterpart: the crate only reaches documents through posting lists): for query i, the
 * top_k documents IN ITS SCOPE by exact ColBERT MaxSim on the decompressed index -- the S6 score unchanged (codec.rs:423-470
 * decompress, maxsim.rs:281-291: non-finite similarities are ignored, a query token without a finite maximum adds 0).
 *   scope       without subsets (n_subsets == 0, or query_subset[i] == -1): every document the handle holds; with a subset:
 *               those of them the subset names.  Duplicate ids count once, ids outside [0, num_documents) are ignored, an
 *               empty subset empties that query's result and no other.  The CSR arguments, their checks and their errors
 *               are those of np_hip_search_batch_subsets.
 *   empty docs  a document without tokens is never returned (search cannot reach one either)
 *   count       out_counts[i] = min(top_k, non-empty documents in scope)
 *   order       score descending, finite first (as S7; a non-finite score comes back as NaN); bit-equal scores by ascending
 *               global id; a cut keeps the lowest ids
 *   independent query i's result is the same, bit for bit, alone, in any batch, in any number of query slices or
 *               document passes ("scan_tiles", "scan_docs", max_batch, workspace_bytes), and from run to run
 *   precision   0 = exact-f32 MFMA (the ground truth; bit-equal to what np_hip_search_batch(precision = 0) gives the same
 *               (query, document) pair); 3 = bf16 MFMA on the decompressed rows (8-bit indexes take the f32 arithmetic at
 *               either).  1 and 2 are not offered: their QC-reuse form gathers one table value per (token, query).
 *   limits      1 <= top_k <= 16384; at most 256 tokens per query (NP_ERR_SHAPE); dim must match the index and the index
 *               be at most 128 wide (NP_ERR_SHAPE); another precision or top_k: NP_ERR_INVALID_ARGUMENT.  All of it is checked
 *               before any launch.
 *   memory      the (query, document) key table, 8 bytes per pair, comes out of the context's workspace budget: the batch
 *               runs in slices of at most max_batch queries and in passes over the documents, merged per query on the
 *               device; nothing is allocated outside the context's arena, and a budget that does not hold one query
 *               and one document is NP_ERR_OUT_OF_MEMORY, not a failed launch.
 *   stats       ms_total, ms_exact (the scan), ms_topk (selection and merge), n_exact_docs ((query, document) pairs scored),
 *               n_exact_tokens (tokens decompressed, once per query group), n_queries; everything else 0.  With stats the
 *               call synchronises once per pass.
 * A sharded handle scans its own documents and returns global ids; the caller merges shards by (score descending, id
 * ascending).  Re-entrant on a shared handle (the context checkout of np_hip_search_batch). */
int np_hip_search_exact(const np_index* index, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                        int32_t top_k, int32_t precision,
                        const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
                        const int32_t* query_subset,
                        int64_t* out_ids, float* out_scores, int32_t* out_counts, np_stats* stats);
/* The same with every buffer in HBM and the two offset arrays also as host copies; enqueues on `stream` and returns.  A
 * query_subset entry outside [0, n_subsets) reads as -1 here (it cannot be checked on the host). */
int np_hip_search_exact_device(const np_index* index, const float* d_queries, const int32_t* d_q_tok_offsets,
                               const int32_t* h_q_tok_offsets, int32_t B, int32_t dim, int32_t top_k, int32_t precision,
                               const int64_t* d_subset_ids, const int64_t* d_subset_offsets,
                               const int64_t* h_subset_offsets, int64_t n_subsets, const int32_t* d_query_subset,
                               int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);

/* ---- given pairs, with the per-token matches ---------------------------------------------------------
 * "Why did this document match?" (no reference counterpart): query i is scored against the documents
 * pair_docs[pair_offsets[i] .. pair_offsets[i+1]) (global ids), exactly, and every query token reports its best document
 * token.  P = pair_offsets[B] pairs, R = sum_i n_i * Lq_i row entries.  Rows are pair-major in the order given: the row of
 * pair p of query i starts at sum_{j<i} n_j * Lq_j + (p - pair_offsets[i]) * Lq_i and holds Lq_i entries in query-token order.
 * out_token_sims and out_token_pos may each be NULL (the launch then skips those stores).
 *   score       out_scores[p]: the S6 score unchanged (codec.rs:423-470 decompress, maxsim.rs:281-291).  A finite score is
 *               bit-equal to what np_hip_search_batch(precision = 0) and np_hip_search_exact(precision = 0) give the same
 *               pair; a non-finite total comes back as NaN, as in S7.
 *   token sim   max over the document's tokens of the scaled similarities of that query token, non-finite entries ignored
 *               (maxsim.rs:281-291); -inf when no document token gives a finite one.  The score equals the f32 sum of the
 *               row's entries greater than -inf, taken in token order starting from 0.0f, bit for bit.
 *   token pos   (i32) the lowest document-token index whose device similarity equals (==) that maximum; -1 when the sim
 *               is -inf.  Indexes are the document's on-disk token order.  (A handle opened with NP_TOK_SORT=1 keeps each
 *               document's tokens by centroid id: it reports on-disk indexes too, but among equal similarities the token
 *               that comes first in its stored order.)
 *   empty doc   a document without tokens: score 0.0, sims -inf, positions -1
 *   shards      an id inside [0, num_documents) that the handle's shard does not hold: score NaN, sims -inf, positions -1.
 *               The caller takes each pair from the shard that owns it.
 *   bad ids     an id outside [0, num_documents): NP_ERR_INVALID_ARGUMENT from the host entry before any launch, naming
 *               the first one.  The device entry cannot see them: there they read as "outside the shard".
 *   independent pairs are independent, duplicates allowed: a pair's three outputs are the same bits alone, in any batch, at
 *               any position of the list, in any slicing or chunking (max_batch, workspace_bytes), and from run to run
 *   precision   0 only; another value is NP_ERR_INVALID_ARGUMENT.  A position has no meaning under bf16 rounding: by the
 *               derived bound of tests/exact_restate.py the winner is ambiguous for 21-27 % of (pair, token) entries at
 *               precision 3, for fewer than 0.06 % at precision 0.
 *   limits      at most 256 tokens per query; dim must match the index and the index be at most 128 wide (both
 *               NP_ERR_SHAPE).  pair_offsets must start at 0 and be non-decreasing (NP_ERR_INVALID_ARGUMENT).  All of it is
 *               checked before any launch.
 *   memory      everything comes from the context's arena, nothing else is allocated: queries run in slices of at most
 *               max_batch, and the host entry stages ids and outputs in chunks of pairs that fit the workspace budget (a
 *               chunk may end inside a query's list).  A budget that cannot hold one query and one pair is
 *               NP_ERR_OUT_OF_MEMORY, not a failed launch.
 *   stats       ms_total, ms_exact (the kernel), n_exact_docs (pairs scored: those the shard holds), n_exact_tokens
 *               (document tokens decompressed), n_queries; everything else 0.  With stats the call synchronises per slice.
 * Re-entrant on a shared handle (the context checkout of np_hip_search_batch). */
int np_hip_score_pairs(const np_index* index, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                       int32_t precision, const int64_t* pair_docs, const int64_t* pair_offsets /* [B+1] */,
                       float* out_scores /* [P] */, float* out_token_sims /* [R] or NULL */,
                       int32_t* out_token_pos /* [R] or NULL */, np_stats* stats);
/* The same with every buffer in HBM and the two offset arrays also as host copies (which must agree with the device
 * copies); enqueues on `stream` and returns. */
int np_hip_score_pairs_device(const np_index* index, const float* d_queries, const int32_t* d_q_tok_offsets,
                              const int32_t* h_q_tok_offsets, int32_t B, int32_t dim, int32_t precision,
                              const int64_t* d_pair_docs, const int64_t* d_pair_offsets, const int64_t* h_pair_offsets,
                              float* d_out_scores, float* d_out_token_sims, int32_t* d_out_token_pos, void* stream);

/* ---- metadata filters: columns in HBM, WHERE evaluated to a subset on the device ---------------------
 * The crate computes a request's subset with filtering::where_condition (filtering.rs:1880: a SQLite query over metadata.db)
 * and hands the id list to search.  Here a few typed attributes per document live next to the index, a filter crosses the
 * ABI as a postfix program over them (pattern strings never do: the host resolves text against a dictionary into i32 codes,
 * and a REGEXP / LIKE pattern crosses as a DFA table -- "text predicates" below), and
 * the ids it selects are produced on the device, with SQLite's semantics including its three-valued logic for NULL.
 *
 * np_hip_index_set_columns replaces the handle's columns (n_cols = 0 drops them; at most NP_MAX_COLUMNS).  `data` and `valid`
 * are host arrays over the WHOLE index; a sharded handle keeps its slice [shard_doc_begin, shard_doc_end).  An f64 NaN is NULL
 * whatever `valid` says (what SQLite does with a bound NaN).  The bytes are added to np_info.device_bytes and freed at close.
 * Needs exclusive access to the handle: no call may run on it meanwhile.  NP_ERR_INVALID_ARGUMENT (unknown type, NULL data,
 * n_cols out of range) is reported before any allocation; NP_ERR_OUT_OF_MEMORY leaves the previous columns in place. */
#define NP_COL_I64 0
#define NP_COL_F64 1
#define NP_COL_CODE 2   /* i32 dictionary codes */
#define NP_MAX_COLUMNS 64
typedef struct np_column {
  int32_t type;            /* NP_COL_I64, NP_COL_F64, NP_COL_CODE */
  int32_t reserved;
  const void* data;        /* host, num_documents entries of the WHOLE index (i64 / f64 / i32) */
  const uint8_t* valid;    /* host, num_documents bytes, 0 = NULL; NULL pointer = no NULLs */
} np_column;
int np_hip_index_set_columns(np_index* index, const np_column* cols, int32_t n_cols);

/* A filter is a postfix program: leaves push a value, NOT replaces the top, AND / OR replace the top two.  Every value is
 * TRUE, FALSE or UNKNOWN and a document is selected only where the program leaves TRUE:
 *   CMP, BETWEEN   UNKNOWN on a NULL cell
 *   IN             TRUE on a match; otherwise UNKNOWN if the cell is NULL or the list held a NULL (arg bit 0); otherwise FALSE
 *   IS_NULL        always known
 *   NOT            keeps UNKNOWN;  AND / OR are Kleene's (FALSE AND UNKNOWN = FALSE, TRUE OR UNKNOWN = TRUE)
 * `x NOT IN`, `NOT BETWEEN` and `IS NOT NULL` are the leaf followed by NOT.  I64 and CODE columns compare as integers, exactly
 * over the whole range; F64 columns compare as IEEE doubles (-0.0 == 0.0, infinities order as numbers; a cell is never NaN,
 * and a NaN constant is refused).
 * Limits (NP_ERR_INVALID_ARGUMENT before any launch, the message names the filter and the op): 1..NP_FILTER_MAX_OPS ops, stack
 * depth at most NP_FILTER_MAX_DEPTH, exactly one value left at the end, column indexes inside the handle's columns, value
 * ranges inside values[], IN lists ascending and distinct (in the column's order), known ops and args, at most
 * NP_FILTER_MAX_VALUES values in one filter, and a handle that has columns. */
#define NP_F_CMP 0
#define NP_F_BETWEEN 1
#define NP_F_IN 2
#define NP_F_IS_NULL 3
#define NP_F_CONST 4
#define NP_F_AND 5
#define NP_F_OR 6
#define NP_F_NOT 7
#define NP_F_MATCH 16   /* text predicates below; 8..15 stay unknown ops */
#define NP_FILTER_MAX_OPS 256
#define NP_FILTER_MAX_DEPTH 32
#define NP_FILTER_MAX_VALUES (1 << 20)
typedef struct np_filter_op {
  int32_t op;          /* NP_F_* */
  int32_t column;      /* leaves: column index; otherwise -1 */
  int32_t arg;         /* CMP: 0 ==, 1 !=, 2 <, 3 <=, 4 >, 5 >=;  CONST: 0 false, 1 true, 2 unknown;
                          IN: bit 0 set = the list also held a NULL */
  int32_t n_values;    /* CMP 1, BETWEEN 2 (lo, hi), IN n >= 0 (ascending, distinct) */
  int64_t first_value; /* index into values[] */
} np_filter_op;
typedef struct np_filter {
  const np_filter_op* ops;
  int32_t n_ops;
  const int64_t* values;   /* i64 as is, f64 as its bit pattern, codes sign-extended */
  int64_t n_values;
} np_filter;

/* The documents each filter selects, as GLOBAL ids, ascending, each once: filter f's ids are
 * out_ids[out_offsets[f] .. out_offsets[f + 1]).  A sharded handle returns the ids of its own documents.  out_ids may be NULL
 * (counts only).  If ids_capacity is smaller than out_offsets[n_filters], out_offsets is still filled in full and the call
 * returns NP_ERR_INVALID_ARGUMENT with the needed size in the message.  The result is the same bits from run to run and in any
 * chunking: positions come from popcounts and an exclusive scan, never from atomics.  Scratch comes out of a context's arena
 * (the checkout of np_hip_search_batch: re-entrant on a shared handle); the call runs in chunks of documents and filters that
 * fit the workspace budget, and a budget that holds no chunk is NP_ERR_OUT_OF_MEMORY, not a failed launch. */
int np_hip_filter_eval(const np_index* index, const np_filter* filters, int32_t n_filters,
                       int64_t* out_ids /* may be NULL: counts only */, int64_t ids_capacity,
                       int64_t* out_offsets /* [n_filters + 1] */);

/* np_hip_search_batch_subsets and np_hip_search_exact with (filters, n_filters, query_filter[B]) in place of the subsets'
 * CSR: the filters are evaluated into a CSR that stays in HBM (the host reads back only its n_filters + 1 offsets) and the
 * existing pass runs on it.  Query i gets, bit for bit, what the subsets call returns for the same ids, ascending, as subset
 * query_filter[i]: -1 = no filter; a filter that selects nothing empties that query's result and no other; one that selects
 * everything is a subset of all documents, not "no subset".  A query_filter entry < -1 or >= n_filters is
 * NP_ERR_INVALID_ARGUMENT, and so is a handle opened with shard_count > 1: the crate's probe scaling needs the global subset
 * length, a collective these calls do not run (np_hip_filter_eval does work on a shard; np_hip_search_batch_sharded_filtered
 * and its kin in the sharded section run it over a communicator).  stats are those of the underlying
 * call with the filter's time added to ms_total. */
int np_hip_search_batch_filtered(const np_index* index, const float* queries, const int32_t* q_tok_offsets,
                                 int32_t B, int32_t dim, const np_search_params* params,
                                 const np_filter* filters, int32_t n_filters, const int32_t* query_filter,
                                 int64_t* out_ids, float* out_scores, int32_t* out_counts, np_stats* stats);
int np_hip_search_exact_filtered(const np_index* index, const float* queries, const int32_t* q_tok_offsets, int32_t B,
                                 int32_t dim, int32_t top_k, int32_t precision,
                                 const np_filter* filters, int32_t n_filters, const int32_t* query_filter,
                                 int64_t* out_ids, float* out_scores, int32_t* out_counts, np_stats* stats);

/* ---- text predicates: the dictionary text of a CODE column in HBM, REGEXP and LIKE as byte DFAs ------
 * The crate's grep side is filtering::where_condition_regexp (filtering.rs:1969): `col REGEXP ?` with the Rust regex crate's
 * is_match behind it.  Here a pattern crosses the ABI as a dense DFA over bytes, not as a string: a Rust binding builds it
 * exactly with regex-automata, the Python package compiles a stated dialect (next_plaid_amd/regexes.py) and refuses the rest.
 *
 * np_hip_index_set_column_text keeps the dictionary strings of one NP_COL_CODE column on the device, indexed by code: the
 * strings' UTF-8 bytes concatenated and offsets[n_strings + 1] into them.  NP_ERR_INVALID_ARGUMENT before any allocation: the
 * column is not a CODE column, n_strings does not exceed the largest code of the handle's rows (or a code is negative), the
 * offsets do not ascend from 0, a string is longer than NP_MATCH_MAX_STRING_BYTES (4 MiB: one lane walks one string, so a longer
 * one would hold its block of the launch without bound).  n_strings = 0 drops the text; np_hip_index_set_columns drops it with the columns.  The bytes
 * count in np_info.device_bytes; NP_ERR_OUT_OF_MEMORY leaves the previous text in place.  A sharded handle keeps the whole
 * dictionary (codes are global).  Needs exclusive access to the handle, as np_hip_index_set_columns does.
 *
 * A packed DFA is n_words 32-bit words:
 *   [0] NP_DFA_MAGIC   [1] n_states (1..NP_DFA_MAX_STATES)   [2] n_classes (1..NP_DFA_MAX_CLASSES)   [3] start state
 *   [4 .. 68)          class_of[256], one byte each, byte b in bits 8 (b & 3) of word 4 + b / 4
 *   [68 .. 68 + F)     per-state flags, one byte each in the same way, F = ceil(n_states / 4)
 *   [68 + F .. )       table[n_states][n_classes] of u16 next states, entry e in bits 16 (e & 1) of word e / 2; ceil(n_states * n_classes / 2) words
 * A string matches if the walk from the start state over its bytes (state = table[state][class_of[byte]]) ends in a state with
 * NP_DFA_ACCEPT_AT_END.  NP_DFA_MATCHED and NP_DFA_DEAD mark absorbing states (every / no continuation matches) at which a
 * lane may stop.  Checked before any launch (the message names the DFA and the state): sizes consistent, every transition
 * < n_states, every class < n_classes, MATCHED and DEAD rows point to themselves, MATCHED implies ACCEPT_AT_END, DEAD excludes
 * it.  In a filter the same words are values[first_value .. first_value + n_values), one word per i64.
 *
 * np_hip_text_match: bit s of out_bits[d * ceil(n_strings / 32) + s / 32] = DFA d accepts dictionary string s (bits past the
 * last string are zero).  The same bits from run to run and for any tiling: verdicts leave as ballot words, no atomics.
 * Scratch comes out of a context's arena (re-entrant on a shared handle); the call runs in chunks that fit the workspace
 * budget and a budget that holds no chunk is NP_ERR_OUT_OF_MEMORY.  A table within the plan's LDS budget is walked out of LDS,
 * a larger one out of global memory (np_hip_index_tune "match_lds" = that budget in KiB, 0 = always global).
 *
 * NP_F_MATCH (op 16) is the filter leaf: column = a CODE column that has text, arg = 0, values = the packed DFA.  TRUE / FALSE
 * by the cell's dictionary string, UNKNOWN on a NULL cell as LIKE gives, so NOT over a NULL cell selects nothing.  (The crate
 * differs: its regexp function reads the argument as String, so a NULL cell fails the whole query.)  One match pass per
 * distinct (column, DFA) of a call writes a bitmap over codes and the per-document leaf reads bit[code[d]].  A column without
 * text or an invalid DFA is NP_ERR_INVALID_ARGUMENT before any launch. */
#define NP_DFA_MAGIC 0x4146444Eu
#define NP_DFA_HEADER_WORDS 68
#define NP_DFA_MAX_STATES 4096
#define NP_DFA_MAX_CLASSES 256
#define NP_DFA_ACCEPT_AT_END 1
#define NP_DFA_MATCHED 2
#define NP_DFA_DEAD 4
#define NP_MATCH_MAX_STRING_BYTES (4 << 20)
typedef struct np_dfa {
  const uint32_t* words;
  int64_t n_words;
} np_dfa;
typedef struct np_match_report {
  int32_t tile_bytes;        /* bytes of text a block stages at a time */
  int32_t table_lds_bytes;   /* the plan's LDS budget for a table */
  int32_t n_lds, n_global;   /* DFAs whose table was walked out of LDS / out of global memory */
  int32_t n_chunks;          /* (DFA group, string chunk) passes */
  int32_t reserved;
  int64_t bytes_scanned;     /* text bytes x DFAs (lanes stop early at MATCHED and DEAD, so an upper bound of the lookups) */
  float ms;                  /* wall time of the call */
  int32_t reserved2;
} np_match_report;
int np_hip_index_set_column_text(np_index* index, int32_t column, const uint8_t* bytes, const int64_t* offsets /* [n_strings + 1] */,
                                 int64_t n_strings);
int np_hip_text_match(const np_index* index, int32_t column, const np_dfa* dfas, int32_t n_dfas,
                      uint32_t* out_bits /* [n_dfas][ceil(n_strings / 32)] */, np_match_report* report /* may be NULL */);

/* ---- hybrid search: the keyword index in HBM, FTS5-exact BM25, fusion ---------------------------------
 * The crate's /search handler runs, next to index.search, an SQLite FTS5 query (text_search.rs:1246-1342: MATCH ordered by
 * -bm25()) and fuses the two lists (text_search.rs:1006-1075).  Here the FTS5 index lives next to the ColBERT index and
 * the keyword search, the fusion and the whole hybrid request run on the device, with SQLite's results bit for bit.
 *
 * np_hip_index_set_text replaces the handle's keyword index (NULL, or an index without instances and rows, drops it).  The
 * arrays are host arrays over the WHOLE index: the (term, document, position) instances of the FTS5 table as fts5vocab's
 * 'instance' rows give them, sorted by (term, document, position), term t owning [term_offsets[t], term_offsets[t + 1]);
 * n_rows is the row count of the FTS5 table (its nRow: rows without a token count, so it need not equal num_documents).
 * Document ids are global ids in [0, num_documents).  Derived on the host and kept in HBM: per-term posting lists of
 * (document, term frequency, first position), every document's token count (its instances), and on the host the total
 * token count and every term's document frequency.  The bytes are added to np_info.device_bytes and freed at close.
 * Needs exclusive access to the handle.  Checked on the host before any allocation (NP_ERR_INVALID_ARGUMENT, the message
 * names the first offending term / instance): offsets that do not start at 0 or decrease, instances out of (document,
 * position) order or repeated, a document outside [0, num_documents), a negative position, n_rows below the number of
 * distinct documents, NULL arrays with a positive count.  NP_ERR_OUT_OF_MEMORY leaves the previous index in place.
 * A handle opened with shard_count > 1 is refused (NP_ERR_INVALID_ARGUMENT), here and in every call below: nRow, the
 * average length and a phrase's hit count are global figures and need a collective that these calls do not run.  The calls
 * that run it take a communicator: np_hip_index_set_text_shard, np_hip_text_search_sharded and np_hip_search_hybrid_sharded
 * in the sharded section below. */
typedef struct np_text_index {
  int64_t n_terms;
  const int64_t* term_offsets;   /* [n_terms + 1] */
  const int64_t* inst_doc;       /* [term_offsets[n_terms]] global document ids */
  const int32_t* inst_pos;       /* [term_offsets[n_terms]] token positions inside the document */
  int64_t n_rows;                /* FTS5's nRow */
} np_text_index;
int np_hip_index_set_text(np_index* index, const np_text_index* text);

/* A keyword query: phrases of term ids (-1 = a token the vocabulary does not hold), all joined by AND or all by OR.  Phrase
 * p owns terms[phrase_offsets[p] .. phrase_offsets[p + 1]).  The tokenising front end (FTS5 query text -> term ids) is host
 * work (next_plaid_amd/text.py).
 *   result    what SQLite returns for SELECT rowid, CAST(-bm25(t) AS REAL) ... WHERE t MATCH ? [AND rowid IN subset] ORDER BY
 *             score DESC LIMIT top_k, read as f32
 *   frequency of a phrase in a document: the number of positions p with token j of the phrase at p + j for every j
 *   match     AND: every phrase has frequency >= 1; OR: any has.  A phrase holding a -1 has frequency 0 everywhere
 *   score     nHit_i = documents of the WHOLE table holding phrase i (never the subset's);
 *             idf_i = log((nRow - nHit_i + 0.5) / (nHit_i + 0.5)), 1e-6 where that is <= 0, on the host in f64 with libm's log;
 *             avgdl = (double)total_tokens / (double)nRow; k1 = 1.2, b = 0.75, D = the document's token count, a = the
 *             frequency; score = 0.0, then in phrase order score += idf_i * ((a * (k1 + 1.0)) / (a + k1 * (1 - b + b * D / avgdl)));
 *             every operation IEEE f64, in this order, none fused; repeated phrases score repeatedly; the result is (float)score
 *   order     f64 score descending, ties by ascending id (SQLite leaves ties unspecified); out_counts[i] = min(top_k,
 *             matches); the rest of a row is padded as np_hip_search_exact pads it (id 0, score 0)
 *   independent  query i's result is the same bits alone, in any batch, at any position, in any chunking (max_batch,
 *             workspace_bytes) and from run to run: no float atomic, integer atomics only for counters and for slots
 *             whose order a total-order sort then decides
 *   subsets   the CSR arguments, their checks and their meaning are those of np_hip_search_exact: -1 = none, an empty subset
 *             empties that query's result and no other, duplicate ids count once, ids outside [0, num_documents) are ignored
 *   limits    1..NP_TEXT_MAX_PHRASES phrases, at least one token per phrase, at most NP_TEXT_MAX_TOKENS tokens per query, term
 *             ids in [-1, n_terms), a known mode, 1 <= top_k <= NP_TEXT_MAX_TOPK, B < 65536, a handle with a keyword index
 *             and without shards: NP_ERR_INVALID_ARGUMENT before any launch, the message names the query
 *   memory    scratch comes out of the context's arena; the call runs in chunks of queries and of document slices that fit
 *             the workspace budget, merged per query on the device.  A budget that holds no chunk is NP_ERR_OUT_OF_MEMORY
 *   stats     ms_total, n_queries, n_ivf_ids = postings visited by the scoring pass; everything else 0
 * A batch with a phrase of several tokens runs a counting pass first (nHit) and synchronises once to compute the idf on the
 * host; a batch of single-token phrases takes the document frequencies it already has.  Re-entrant on a shared handle. */
#define NP_TEXT_AND 0
#define NP_TEXT_OR 1
#define NP_TEXT_MAX_PHRASES 64
#define NP_TEXT_MAX_TOKENS 256
#define NP_TEXT_MAX_TOPK 1024
typedef struct np_text_query {
  const int32_t* terms;            /* [phrase_offsets[n_phrases]] */
  const int32_t* phrase_offsets;   /* [n_phrases + 1], starts at 0, strictly increasing */
  int32_t n_phrases;
  int32_t mode;                    /* NP_TEXT_AND, NP_TEXT_OR */
} np_text_query;
int np_hip_text_search(const np_index* index, const np_text_query* queries, int32_t B, int32_t top_k,
                       const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
                       const int32_t* query_subset,
                       int64_t* out_ids, float* out_scores, int32_t* out_counts, np_stats* stats);
/* The same with the subsets' CSR and the outputs in HBM (the queries stay host structs: they are programs, as filters are);
 * enqueues on `stream`.  A batch with a multi-token phrase synchronises the stream once (the counting pass). */
int np_hip_text_search_device(const np_index* index, const np_text_query* queries, int32_t B, int32_t top_k,
                              const int64_t* d_subset_ids, const int64_t* d_subset_offsets,
                              const int64_t* h_subset_offsets, int64_t n_subsets, const int32_t* d_query_subset,
                              int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);
/* ... and with filters in place of the subsets, as np_hip_search_exact_filtered is to np_hip_search_exact. */
int np_hip_text_search_filtered(const np_index* index, const np_text_query* queries, int32_t B, int32_t top_k,
                                const np_filter* filters, int32_t n_filters, const int32_t* query_filter,
                                int64_t* out_ids, float* out_scores, int32_t* out_counts, np_stats* stats);

/* Fusion of a semantic and a keyword list per query (text_search.rs:1006-1075), f32 in the reference's order, unfused.  List
 * i of either side is ids / scores [i * stride .. i * stride + counts[i]); out rows have top_k entries, padded with id 0 and
 * score 0; out_counts[i] = min(top_k, distinct ids of the two lists).
 *   NP_FUSE_RRF             entry r (0-based) of the semantic list adds alpha / (60.0f + (float)r + 1.0f), entry r of the
 *                           keyword list (1.0f - alpha) / (60.0f + (float)r + 1.0f); a document starts at 0.0f and the
 *                           semantic term is added first.  Scores are not read (they may be NULL)
 *   NP_FUSE_RELATIVE_SCORE  each list is min-max normalised over its own entries, (s - min) / (max - min), 1.0f for every
 *                           entry when max == min, nothing from an empty list, min / max ignoring NaN as f32::min / max do;
 *                           then 0.0f + alpha * s_sem, then + (1.0f - alpha) * s_kw
 *   order                   fused score descending, ties by ascending id, a NaN score after every number (the reference's
 *                           tie order is a HashMap's)
 * An id occurs at most once per list (not checked).  NP_ERR_INVALID_ARGUMENT: alpha outside [0, 1] or NaN (the handler's
 * BadRequest), an unknown mode, top_k outside 1 .. 2 * NP_TEXT_MAX_TOPK, a stride or (host form) a count outside
 * 0 .. NP_TEXT_MAX_TOPK; the device form clamps a count to its stride.  `index` names the device and lends a context; NULL =
 * the current device (the host form then allocates and frees its own scratch). */
#define NP_FUSE_RRF 0
#define NP_FUSE_RELATIVE_SCORE 1
int np_hip_fuse(const np_index* index, int32_t mode, float alpha, int32_t top_k, int32_t B,
                const int64_t* sem_ids, const float* sem_scores, const int32_t* sem_counts, int32_t sem_stride,
                const int64_t* kw_ids, const float* kw_scores, const int32_t* kw_counts, int32_t kw_stride,
                int64_t* out_ids, float* out_scores, int32_t* out_counts);
int np_hip_fuse_device(const np_index* index, int32_t mode, float alpha, int32_t top_k, int32_t B,
                       const int64_t* d_sem_ids, const float* d_sem_scores, const int32_t* d_sem_counts, int32_t sem_stride,
                       const int64_t* d_kw_ids, const float* d_kw_scores, const int32_t* d_kw_counts, int32_t kw_stride,
                       int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);

/* The hybrid request in one call: the semantic pass (np_hip_search_batch_subsets_device's pass with top_k = fetch_k), the
 * keyword pass with top_k = fetch_k and the fusion to params->top_k, on one stream; neither list leaves HBM.  Query i gets,
 * byte for byte, what np_hip_fuse returns for the outputs of np_hip_search_batch_subsets (or _filtered) and
 * np_hip_text_search (or _filtered) called separately with the same arguments and top_k = fetch_k.  The scope is the
 * subsets' CSR, or -- filters != NULL -- n_filters filters with query_subset as the query map (then subset_ids and
 * subset_offsets are ignored and n_subsets is not read).  1 <= fetch_k <= NP_TEXT_MAX_TOPK (the handler takes 3 * top_k);
 * 1 <= params->top_k <= 2 * NP_TEXT_MAX_TOPK.  stats: ms_total and n_queries of the whole call, n_ivf_ids of the keyword
 * pass; everything else 0. */
int np_hip_search_hybrid(const np_index* index, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                         const np_search_params* params, const np_text_query* text_queries, int32_t fetch_k, float alpha,
                         int32_t fusion,
                         const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
                         const int32_t* query_subset, const np_filter* filters, int32_t n_filters,
                         int64_t* out_ids, float* out_scores, int32_t* out_counts, np_stats* stats);

/* ---- keyword search with the FTS5 boolean grammar and prefix queries ----------------------------------
 * A keyword query as a TREE: phrases as np_text_query has them, every phrase optionally ending in a PREFIX, and a postfix
 * list of nodes over them -- what FTS5 makes of `error NOT test`, `(parse OR lex) AND token`, `interceptor*`,
 * `"http req" *` and `foo + bar` (the compiler from query text is next_plaid_amd/text.py, compile_text_expr).
 *   phrases   terms / phrase_offsets as in np_text_query.  prefix_hi[p] = 0: the phrase's last token is the term it names;
 *             otherwise the last token stands for every term of [last term id, prefix_hi[p]) -- fts5vocab numbers the terms
 *             in byte order, so the terms that start with a prefix are one range.  (An empty range is written as the
 *             unknown token -1 with prefix_hi = 0: the phrase never occurs.)  A phrase of ONE token may name any range:
 *             its postings are one run of the instance arrays.  A phrase of several tokens that ends in a prefix may name
 *             at most NP_TEXT_MAX_PREFIX_TERMS terms (its last position is looked up in every one of them)
 *   nodes     postfix: NP_TEXT_NODE_PHRASE pushes phrase `a`; AND / OR / NOT pop the nodes `b` (top) and `a` (below it) --
 *             indexes into the list, both below the node's own -- and push the result; NOT is binary, a AND NOT b.  One
 *             node is left at the end: the last.  Every phrase is named by exactly one PHRASE node
 *   match     the boolean value of the tree over "phrase p has frequency >= 1 in the document"
 *   score     np_text_query's sum, IN PHRASE ORDER, over the phrases that are LIVE in the document: the phrase occurs,
 *             every node on its path to the root is true, and the path enters no NOT from the right.  nHit and idf of a
 *             phrase are the phrase's own, whatever stands around it; a prefix phrase's nHit counts the documents that hold
 *             any term of the range and its frequency adds the instances of all of them.  SQLite's own bm25() differs on
 *             a few rows of trees with a NOT below an OR or inside a NOT's right side, and with an OR below an AND next
 *             to phrases of several tokens (leftovers of its cursors); everywhere else the bits are
 *             SQLite's.  A flat tree (a chain of ANDs or of ORs without prefixes) returns np_hip_text_search's bytes
 *   everything else (order, independence, subsets, filters, memory, stats, errors) is np_hip_text_search's; n_ivf_ids counts
 *   the postings a prefix's pre-pass walks too, and every query of a chunk owns 4 bytes x num_documents of scratch per
 *   single-token prefix phrase (of the query that has most).  A malformed tree is NP_ERR_INVALID_ARGUMENT before any launch;
 *   the message names the query and the node or phrase.
 * The device-pointer form is np_hip_text_search_expr_device below, the sharded forms np_hip_text_search_sharded_expr,
 * _sharded_expr_filtered and np_hip_search_hybrid_sharded_expr (with the sharded entries).  The grouped entries have no _expr
 * form yet. */
#define NP_TEXT_NODE_PHRASE 0
#define NP_TEXT_NODE_AND 1
#define NP_TEXT_NODE_OR 2
#define NP_TEXT_NODE_NOT 3
#define NP_TEXT_MAX_NODES 127
#define NP_TEXT_MAX_PREFIX_TERMS 1024
typedef struct np_text_node {
  int32_t op;   /* NP_TEXT_NODE_* */
  int32_t a;    /* PHRASE: the phrase; otherwise the left child */
  int32_t b;    /* the right child (PHRASE: 0) */
} np_text_node;
typedef struct np_text_expr {
  const int32_t* terms;            /* [phrase_offsets[n_phrases]] */
  const int32_t* phrase_offsets;   /* [n_phrases + 1], starts at 0, strictly increasing */
  const int32_t* prefix_hi;        /* [n_phrases] 0 = an exact last token */
  const np_text_node* nodes;       /* [n_nodes] postfix */
  int32_t n_phrases;
  int32_t n_nodes;
} np_text_expr;   /* np_hip_struct_size(12) */
int np_hip_text_search_expr(const np_index* index, const np_text_expr* queries, int32_t B, int32_t top_k,
                            const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
                            const int32_t* query_subset,
                            int64_t* out_ids, float* out_scores, int32_t* out_counts, np_stats* stats);
int np_hip_text_search_expr_filtered(const np_index* index, const np_text_expr* queries, int32_t B, int32_t top_k,
                                     const np_filter* filters, int32_t n_filters, const int32_t* query_filter,
                                     int64_t* out_ids, float* out_scores, int32_t* out_counts, np_stats* stats);
/* np_hip_text_search_device with tree queries: np_hip_text_search_expr's bytes in device buffers, enqueued on `stream`.  It
 * synchronises the stream where np_hip_text_search_device does (once, for the idf, in a batch with a phrase of several
 * tokens) and once more per chunk of queries that holds a single-token prefix phrase (that chunk's prefix counts). */
int np_hip_text_search_expr_device(const np_index* index, const np_text_expr* queries, int32_t B, int32_t top_k,
                                   const int64_t* d_subset_ids, const int64_t* d_subset_offsets,
                                   const int64_t* h_subset_offsets, int64_t n_subsets, const int32_t* d_query_subset,
                                   int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);
/* np_hip_search_hybrid with tree queries: its arguments, scope forms and result, the keyword list being
 * np_hip_text_search_expr's. */
int np_hip_search_hybrid_expr(const np_index* index, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                              const np_search_params* params, const np_text_expr* text_queries, int32_t fetch_k, float alpha,
                              int32_t fusion,
                              const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
                              const int32_t* query_subset, const np_filter* filters, int32_t n_filters,
                              int64_t* out_ids, float* out_scores, int32_t* out_counts, np_stats* stats);

/* ---- grouped search: top_k groups with their best documents ------------------------------------------
 * Both applications of the crate index UNITS and answer in GROUPS: code units of a file, passages of a document.  ColGREP does
 * it on the host (colgrep/src/index/mod.rs:4093-4292, collapse_by_file at :4394-4413): it over-fetches max(20 top_k, 200)
 * results, walks them keeping the first unit of every file as its leader, folds later units of that file into it and stops at
 * top_k distinct files.  Here the group of every document lives in HBM and the ranked list never leaves it.
 *
 * np_hip_index_set_groups gives every document of the WHOLE index a dense group id in [0, n_groups): a host array of n =
 * num_documents i32, kept in HBM (its n * 4 bytes count in np_info.device_bytes; freed at close).  n = 0 drops the groups.
 * NP_ERR_SHAPE: n != num_documents.  NP_ERR_INVALID_ARGUMENT, before any allocation: an id outside [0, n_groups), n_groups
 * outside 1 .. 2^31-1, or a handle opened with shard_count > 1 (see "out of scope").  NP_ERR_OUT_OF_MEMORY leaves the previous
 * groups in place.  Needs exclusive access to the handle, as np_hip_index_set_columns does.  A handle is immutable otherwise:
 * a reload, an update or a delete opens a new handle, which has no groups (as it has no columns) until they are set again, so
 * an array whose length differs from num_documents is never read.  np_hip_index_group_count: n_groups, 0 without groups.
 *
 * np_hip_collapse takes B ranked lists in np_hip_fuse's layout -- list b is ids / scores [b * stride .. b * stride +
 * counts[b]), scores may be NULL, 1 <= stride <= NP_GROUP_MAX_LIST -- and walks each one:
 *     for r in 0 .. counts[b]-1:   g = group of ids[b][r]
 *         g admitted:                 total[g] += 1; if members[g] < group_size: append (id, score) to g
 *         fewer than top_k admitted:  admit g with (id, score) as its leader; total[g] = members[g] = 1
 *         otherwise:                  skip
 * No score is read: the order of the list is the order.  Duplicate ids are separate entries.  Groups come in order of
 * admission (their leaders' ranks), a group's members in list order:
 *   out_ids      [B][top_k][group_size], padded with id 0 as np_hip_fuse pads
 *   out_scores   likewise, the input's bits (a NaN keeps its payload), padded with 0; NULL when scores is NULL
 *   out_group    [B][top_k] i32 the group id        out_members  [B][top_k] i32 members written, <= group_size
 *   out_total    [B][top_k] i32 entries of the group in the whole list (what was folded = total - members)
 *   out_counts   [B] groups admitted
 * NP_ERR_INVALID_ARGUMENT before any launch: no groups set, top_k < 1, group_size < 1, top_k * group_size > 16384, a stride
 * out of range; host form only: a count outside 0 .. stride, an id outside [0, num_documents).  The device form clamps a
 * count to its stride and treats an id out of range as absent: skipped, and counted in no total.  The same bits from run to
 * run, alone or in any batch: one workgroup per list sorts (group, rank) keys, positions come from scans and popcounts, no
 * output atomics.
 *
 * np_hip_search_batch_grouped: np_hip_search_hybrid's arguments without the text part, plus pool_k and group_size.  Runs the
 * search pass with top_k = pool_k (1 <= pool_k <= 16384) into scratch and collapses it to params->top_k groups on the same
 * stream; neither the pool nor the lists leave HBM.  Query i gets, byte for byte, np_hip_collapse of what
 * np_hip_search_batch_subsets (or _filtered) returns with top_k = pool_k.  stats: ms_total and n_queries.
 * np_hip_search_hybrid_grouped: np_hip_search_hybrid fused to pool_k (1 <= pool_k <= 2 * NP_TEXT_MAX_TOPK), then collapsed:
 * byte for byte the two calls composed.  This is ColGREP's request: fuse into the pool, collapse to top_k files.
 *
 * Out of scope:
 *   sharded handles   a group's members can lie on several shards, and a member's shard-local group can fall outside that
 *                     shard's local top_k groups while the group is in the global top_k: per-shard grouped lists do not merge
 *                     exactly for group_size > 1.  The handle is refused, not approximated.
 *   grouped search_exact beyond the pool   the true grouped top-k over all documents needs a per-query, per-group maximum table
 *                     across scan passes and a second pass for members.  np_hip_collapse of np_hip_search_exact(top_k = pool_k)
 *                     is available.
 *   ColGREP's score adjustments   the path penalty, the boosts and the line-span merge are application code on at most 200
 *                     rows; out_total and a large group_size give the host what it needs for the span. */
#define NP_GROUP_MAX_LIST 16384
int np_hip_index_set_groups(np_index* index, const int32_t* group_ids, int64_t n, int64_t n_groups);
int64_t np_hip_index_group_count(const np_index* index);
int np_hip_collapse(const np_index* index, int32_t top_k, int32_t group_size, int32_t B,
                    const int64_t* ids, const float* scores, const int32_t* counts, int32_t stride,
                    int64_t* out_ids, float* out_scores, int32_t* out_group, int32_t* out_members, int32_t* out_total,
                    int32_t* out_counts);
int np_hip_collapse_device(const np_index* index, int32_t top_k, int32_t group_size, int32_t B,
                           const int64_t* d_ids, const float* d_scores, const int32_t* d_counts, int32_t stride,
                           int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_group, int32_t* d_out_members,
                           int32_t* d_out_total, int32_t* d_out_counts, void* stream);
int np_hip_search_batch_grouped(const np_index* index, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                                const np_search_params* params,
                                const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
                                const int32_t* query_subset, const np_filter* filters, int32_t n_filters,
                                int32_t pool_k, int32_t group_size,
                                int64_t* out_ids, float* out_scores, int32_t* out_group, int32_t* out_members,
                                int32_t* out_total, int32_t* out_counts, np_stats* stats);
int np_hip_search_hybrid_grouped(const np_index* index, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                                 const np_search_params* params, const np_text_query* text_queries, int32_t fetch_k, float alpha,
                                 int32_t fusion,
                                 const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
                                 const int32_t* query_subset, const np_filter* filters, int32_t n_filters,
                                 int32_t pool_k, int32_t group_size,
                                 int64_t* out_ids, float* out_scores, int32_t* out_group, int32_t* out_members,
                                 int32_t* out_total, int32_t* out_counts, np_stats* stats);

/* ---- document-sharded search (one process per GPU) -------------------------
 * Phase A runs S1-S5 on the local shard and leaves, per query, the shard's best
 * n_sel = min(n_full_scores, max(n_full_scores/4, top_k)) candidates as 64-bit rank keys in
 * d_sel_keys[B * n_sel] (descending; key = orderable(approx score) << 32 | ~global_doc_id; 0 pads).
 * The host all-gathers the keys over RCCL, takes each query's global n_sel-th key as the cut, and
 * phase B exact-scores only the local candidates with key >= d_cut[b], returning the local top-k
 * as (score, id, key) triples.  np_hip_merge_topk then merges the G shards' triples into the
 * final top-k with the reference's tie rules (exact score desc, then approx rank).  With
 * shard_count == 1 and d_cut == NULL the result equals np_hip_search_batch. */
int np_hip_search_phase_a(const np_index* index, const float* d_queries, const int32_t* d_q_tok_offsets,
                          const int32_t* h_q_tok_offsets, int32_t B, int32_t dim,
                          const np_search_params* params, const int64_t* d_subset, int64_t subset_len,
                          const uint32_t* d_elig_global, uint64_t* d_sel_keys, void* stream, void** call_state);
/* With a `subset` the dense path restricts the probe to the centroids that occur in the subset's documents and
 * scales n_ivf_probe by their number (search.rs:350-382).  A document shard only sees its own documents, so for a
 * result identical to the unsharded search the host ORs the shards' bitmaps: np_hip_subset_eligible writes this
 * shard's bitmap (np_hip_elig_words() u32 words), the host all-gathers them, np_hip_or_bitmaps combines
 * d_all[G][words] and the result goes into phase A as d_elig_global (NULL = use the local bitmap: unsharded). */
int64_t np_hip_elig_words(const np_index* index);
int np_hip_subset_eligible(const np_index* index, const int64_t* d_subset, int64_t subset_len, uint32_t* d_elig_bits,
                           void* stream);
int np_hip_or_bitmaps(const np_index* index, const uint32_t* d_all, int32_t G, int64_t words, uint32_t* d_out,
                      void* stream);
/* One subset per query, for hosts that run the phases themselves: np_hip_subsets_eligible writes this shard's bitmaps of
 * all n_subsets subsets, d_elig_bits[n_subsets][np_hip_elig_words()], in one launch; the host all-gathers them (one
 * all-gather, n_subsets times wider), np_hip_or_bitmaps combines d_all[G][n_subsets * words] (it ORs any word count) and the
 * result goes into np_hip_search_phase_a_subsets as d_elig_global (NULL = the local bitmaps).  Phase B, np_hip_search_end and
 * the merge are the ones below. */
int np_hip_subsets_eligible(const np_index* index, const int64_t* d_subset_ids, const int64_t* d_subset_offsets,
                            const int64_t* h_subset_offsets, int64_t n_subsets, uint32_t* d_elig_bits, void* stream);
int np_hip_search_phase_a_subsets(const np_index* index, const float* d_queries, const int32_t* d_q_tok_offsets,
                                  const int32_t* h_q_tok_offsets, int32_t B, int32_t dim,
                                  const np_search_params* params, const int64_t* d_subset_ids,
                                  const int64_t* d_subset_offsets, const int64_t* h_subset_offsets, int64_t n_subsets,
                                  const int32_t* d_query_subset, const uint32_t* d_elig_global, uint64_t* d_sel_keys,
                                  void* stream, void** call_state);
int np_hip_search_phase_b(const np_index* index, void* call_state, const uint64_t* d_cut,
                          int64_t* d_out_ids, float* d_out_scores, uint64_t* d_out_keys,
                          int32_t* d_out_counts, void* stream);
/* Ends a phase-A/phase-B call and returns its context to the pool (always call it). */
void np_hip_search_end(const np_index* index, void* call_state);
/* n_sel for given params (size of one query's slice of d_sel_keys). */
int32_t np_hip_n_sel(const np_search_params* params);
/* Global cut from G gathered key lists: d_all_keys[G][B][n_sel] -> d_cut[B]. */
int np_hip_select_cut(const np_index* index, const uint64_t* d_all_keys, int32_t G, int32_t B,
                      int32_t n_sel, uint64_t* d_cut, void* stream);
/* Merge G shards' local top-k triples ([G][B][top_k], counts [G][B]) into out [B][top_k]. */
int np_hip_merge_topk(const np_index* index, const int64_t* d_ids, const float* d_scores,
                      const uint64_t* d_keys, const int32_t* d_counts, int32_t G, int32_t B,
                      int32_t top_k, int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts,
                      void* stream);

/* The same merge over one packed record per rank: rank g's record starts at d_records + g * record_bytes and holds
 * ids [B*top_k] i64 at 0, keys [B*top_k] u64 at off_keys, scores [B*top_k] f32 at off_scores, counts [B] i32 at
 * off_counts (one all-gather instead of four). */
int np_hip_merge_packed(const np_index* index, const void* d_records, int64_t record_bytes, int64_t off_keys,
                        int64_t off_scores, int64_t off_counts, int32_t G, int32_t B, int32_t top_k,
                        int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);

/* ---- the whole sharded protocol in one call, RCCL below the ABI (np_dist.hip) -----------------------------------
 * One process per GPU.  Every rank opens its document shard (np_open_opts.shard_rank / shard_count = rank / nranks),
 * rank 0 draws a 128-byte id (np_hip_comm_unique_id = ncclGetUniqueId) and hands it to the others by whatever
 * channel the host has (the crate: its own RPC / a file; bench.py: a torch.distributed broadcast), every rank calls
 * np_hip_comm_create (= ncclCommInitRank; collective).  np_hip_search_batch_sharded then runs phase A ->
 * ncclAllGather(keys) -> cut -> phase B -> ncclAllGather(packed top-k) -> merge on `stream` and leaves the GLOBAL
 * top-k (identical to the unsharded search, subsets included) in the output buffers of EVERY rank.  All ranks must
 * call it with the same queries / params / subset in the same order.  librccl is loaded at first use
 * (dlopen "librccl.so.1"; NEXTPLAID_RCCL_LIB overrides); nranks == 1 with id128 == NULL needs no RCCL at all.
 * A communicator serialises its calls; use one per concurrent stream.
 *
 * Failure of ONE rank never blocks the others: every exchange record carries a status word, a rank whose local work
 * fails (its workspace does not fit, a launch error) still takes part in both all-gathers with empty data and returns its
 * own error at once; on the other ranks the batch comes back ABANDONED -- every out_counts[i] = -1 (NP_COUNT_ABANDONED), a
 * count no healthy batch produces: a host MUST treat a negative count as a failed batch, whether or not it polls
 * np_hip_comm_status -- and np_hip_comm_status, valid once `stream` is synchronised, names the failed rank and its np_status.  With the hosted transport below the
 * gathered bytes pass through the host, so every rank returns NP_ERR_SEARCH from the call itself (after gather 1). */
typedef struct np_comm np_comm;
#define NP_COUNT_ABANDONED (-1)
int np_hip_comm_unique_id(void* id128);
int np_hip_comm_create(const np_index* index, const void* id128, int32_t rank, int32_t nranks, np_comm** out);
void np_hip_comm_destroy(np_comm* comm);
/* Reads and clears the failure word of the communicator's last batches: *failed_rank = -1 and *code = 0 if every batch
 * since the last call was healthy, else the first failed rank and its np_status.  Call after synchronising the stream. */
int np_hip_comm_status(np_comm* comm, int32_t* failed_rank, int32_t* code);
/* ABI v6: what a communicator really is, for a bench line or a health endpoint.  *transport = NP_COMM_LOCAL (one rank, no
 * collective library at all), NP_COMM_RCCL (ncclCommInitRank succeeded) or NP_COMM_HOSTED; *nranks = the size the
 * communicator was created with; *rccl_ranks = ncclCommCount of the RCCL communicator (the number of ranks RCCL itself
 * sees: equals nranks on a healthy communicator), 0 for the other transports or a librccl without ncclCommCount.  Any
 * pointer may be NULL. */
#define NP_COMM_LOCAL 0
#define NP_COMM_RCCL 1
#define NP_COMM_HOSTED 2
int np_hip_comm_info(np_comm* comm, int32_t* transport, int32_t* nranks, int32_t* rccl_ranks);
/* The same protocol over a transport the HOST brings (MPI, gloo, shared memory, the crate's own RPC) instead of RCCL:
 * for hosts without librccl, for ranks that share one GPU (RCCL refuses two ranks on a device), and for the tests that
 * run the shipped multi-rank code path on a one-GPU box.  `all_gather(ctx, send, recv, bytes)` is called on the calling
 * thread with HOST pointers: it must place rank r's `bytes` bytes at recv + r * bytes for every rank and return 0.  The
 * library stages the (<= 0.6 MB) records through pinned memory and synchronises the stream around the callback, so a
 * hosted communicator costs two stream synchronisations per batch; results are identical to the RCCL transport.
 * flags: NP_COMM_DEFERRED_STATUS = do not inspect the gathered status words on the host (propagate a failure on the
 * device like the RCCL transport does; np_hip_comm_status reports it). */
typedef int (*np_all_gather_host_fn)(void* ctx, const void* send, void* recv, int64_t bytes);
#define NP_COMM_DEFERRED_STATUS 1
int np_hip_comm_create_hosted(const np_index* index, int32_t rank, int32_t nranks, np_all_gather_host_fn all_gather,
                              void* ctx, int32_t flags, np_comm** out);
int np_hip_search_batch_sharded(const np_index* index, np_comm* comm, const float* d_queries,
                                const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B, int32_t dim,
                                const np_search_params* params, const int64_t* d_subset, int64_t subset_len,
                                int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);

/* np_hip_search_batch_sharded with one subset per query (see np_hip_search_batch_subsets): the eligible bitmaps of all
 * n_subsets subsets are OR-ed over the ranks in the one all-gather the single-subset call has, n_subsets times wider.  All
 * ranks pass the same subsets and the same map. */
int np_hip_search_batch_sharded_subsets(const np_index* index, np_comm* comm, const float* d_queries,
                                        const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                                        int32_t dim, const np_search_params* params, const int64_t* d_subset_ids,
                                        const int64_t* d_subset_offsets, const int64_t* h_subset_offsets,
                                        int64_t n_subsets, const int32_t* d_query_subset, int64_t* d_out_ids,
                                        float* d_out_scores, int32_t* d_out_counts, void* stream);

/* ---- keyword, filtered and hybrid search over document shards (np_text.hip, np_dist.hip) ------------------------
 * The request features of the unsharded handle -- filters evaluated on the device, FTS5-exact BM25, the hybrid request --
 * through the communicator above, with the unsharded results bit for bit on every rank.  All ranks pass the same
 * queries, scopes and parameters in the same order; `stream` is required; a communicator serialises its calls.  The
 * failure rules are those of np_hip_search_batch_sharded: arguments every rank sees alike are checked before the first
 * collective; every exchange record ends in a status word; a rank whose local work fails (no keyword index or no columns
 * on its handle, a workspace too small) takes part in every exchange with empty data and returns its own error; its peers
 * return NP_ERR_SEARCH naming the shard (hosted transport with the host-side check) or get every count =
 * NP_COUNT_ABANDONED and the rank from np_hip_comm_status (RCCL, NP_COMM_DEFERRED_STATUS); the communicator serves the
 * next batch.  The RCCL transport of these calls is the same code around ncclAllGather; only the hosted transport and the
 * one-rank communicator can run on a box with one GPU (RCCL refuses two ranks on a device).
 *
 * np_hip_index_set_text_shard: np_hip_index_set_text for a handle opened with shard_count > 1, by np_hip_index_set_columns'
 * convention -- the arrays describe the WHOLE table (global document ids in [0, num_documents of the whole index)) and
 * the handle keeps its slice: the posting lists, positions and document lengths of the documents of its shard in HBM,
 * under shard-local ids, and on the host the whole table's n_rows, token count and every term's document frequency.
 * Checks, error codes and the out-of-memory rule are np_hip_index_set_text's; on an unsharded handle it IS that call.
 * (A form that hands every rank only its own instances would have to exchange those figures at set time: not offered.)
 *
 * np_hip_text_search_sharded: np_hip_text_search_device over the shards; the GLOBAL result -- ids, f32 scores, counts and
 * padding equal to the unsharded call's, bit for bit -- is left in the output buffers of every rank.  Subset ids are
 * global; a rank ignores those of other shards.
 *   counts   a single-token phrase takes the global document frequency kept at set time.  Only a batch with a phrase of
 *            several known tokens (the condition under which the unsharded call synchronises; it follows from the
 *            queries alone) counts on the shard and exchanges one record per rank: nhit [counted phrases] u64 | n_rows
 *            i64 | status.  The sums are taken on the host (the idf needs libm's log): every rank reads the same bytes
 *            and computes the same idf bits, the unsharded ones.  Ranks that report different n_rows were handed
 *            different tables: NP_ERR_INVALID_ARGUMENT on every rank
 *   scoring  the unsharded kernels on the shard with the global idf and avgdl = (double)total_tokens / (double)n_rows
 *   merge    one all-gather of keys [B * top_k] u64 (the f64 score's bits: two scores that differ in f64 can round to one
 *            f32, and the order is f64 score descending, ties by ascending global id) | ids [B * top_k] i64 | counts [B]
 *            i32 | status, then one block per query places every entry by binary searches in the other ranks' sorted
 *            lists.  No limit on nranks * top_k.  A batch whose record would exceed 4 MiB per rank is cut into runs of
 *            floor((4 MiB - 16) / (16 * top_k + 4)) queries, one exchange each: a function of B and top_k alone, never of
 *            a rank's workspace (how a rank chunks its local scoring stays its own business)
 * _filtered: the scope as filters, evaluated by every rank over its own column slice into a CSR that stays in HBM (the
 * programs are compiled against the whole-index schema, so they are the same on every rank); query_filter is a host array.
 *
 * np_hip_search_batch_sharded_filtered: np_hip_search_batch_filtered over the shards.  The probe of a filtered query is
 * scaled by the GLOBAL length of its filter's id list, so every filter's local length (n_filters i64) rides behind the
 * eligible bitmaps in the all-gather np_hip_search_batch_sharded_subsets already runs, and the pass reads the sums.  The
 * batched probe (centroid_batch_size < K) scales nothing and exchanges neither.  A filter that selects nothing on one
 * shard but something elsewhere empties nothing; one that selects nothing anywhere empties its queries' results only.
 *
 * np_hip_search_hybrid_sharded: np_hip_search_hybrid over the shards, byte for byte: the sharded semantic pass and the
 * sharded keyword pass with top_k = fetch_k and the fusion, on one stream; every rank holds both global lists after the
 * merges, so every rank fuses.  The scope is the subsets' CSR on the device, or -- filters != NULL -- n_filters filters
 * with the host array query_filter as the query map (then the CSR arguments are not read).
 *
 * np_hip_text_search_sharded_expr, np_hip_text_search_sharded_expr_filtered, np_hip_search_hybrid_sharded_expr: the three
 * calls above with tree queries (np_text_expr) in place of the flat ones; every rank holds, bit for bit, what
 * np_hip_text_search_expr / np_hip_search_hybrid_expr return on the unsharded handle for the same scope, and a flat query
 * lifted to a tree keeps the flat sharded entry's bytes.  The argument-only checks are the tree's own against a vocabulary
 * of 2^31 terms, before the first collective; the check against the handle's vocabulary is a local failure.  Limits are
 * np_text_expr's.  Failure rules, exchanges of lists and scopes are the flat calls'.
 *   counts   the counting exchange carries, in query and phrase order, first the phrases of several known tokens (their
 *            last token may be a prefix range), then the single-token prefix phrases: the shard's documents that hold any
 *            term of the range, counted for the WHOLE batch ahead of the local chunks by a pass over one bitmap of a bit
 *            per document and phrase (in groups that fit the rank's workspace).  The record's size follows from the
 *            queries alone; a batch without such a phrase exchanges no counts.  The chunks then fill their frequency
 *            arrays as the unsharded call does, without its synchronisation per chunk */
int np_hip_index_set_text_shard(np_index* index, const np_text_index* text);
int np_hip_text_search_sharded(const np_index* index, np_comm* comm, const np_text_query* queries, int32_t B, int32_t top_k,
                               const int64_t* d_subset_ids, const int64_t* d_subset_offsets,
                               const int64_t* h_subset_offsets, int64_t n_subsets, const int32_t* d_query_subset,
                               int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);
int np_hip_text_search_sharded_filtered(const np_index* index, np_comm* comm, const np_text_query* queries, int32_t B,
                                        int32_t top_k, const np_filter* filters, int32_t n_filters,
                                        const int32_t* query_filter /* host, [B] */,
                                        int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);
int np_hip_text_search_sharded_expr(const np_index* index, np_comm* comm, const np_text_expr* queries, int32_t B, int32_t top_k,
                                    const int64_t* d_subset_ids, const int64_t* d_subset_offsets,
                                    const int64_t* h_subset_offsets, int64_t n_subsets, const int32_t* d_query_subset,
                                    int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);
int np_hip_text_search_sharded_expr_filtered(const np_index* index, np_comm* comm, const np_text_expr* queries, int32_t B,
                                             int32_t top_k, const np_filter* filters, int32_t n_filters,
                                             const int32_t* query_filter /* host, [B] */,
                                             int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);
int np_hip_search_batch_sharded_filtered(const np_index* index, np_comm* comm, const float* d_queries,
                                         const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                                         int32_t dim, const np_search_params* params, const np_filter* filters,
                                         int32_t n_filters, const int32_t* query_filter /* host, [B] */,
                                         int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);
int np_hip_search_hybrid_sharded(const np_index* index, np_comm* comm, const float* d_queries,
                                 const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B, int32_t dim,
                                 const np_search_params* params, const np_text_query* text_queries, int32_t fetch_k,
                                 float alpha, int32_t fusion,
                                 const int64_t* d_subset_ids, const int64_t* d_subset_offsets,
                                 const int64_t* h_subset_offsets, int64_t n_subsets, const int32_t* d_query_subset,
                                 const np_filter* filters, int32_t n_filters, const int32_t* query_filter /* host, [B] */,
                                 int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);
int np_hip_search_hybrid_sharded_expr(const np_index* index, np_comm* comm, const float* d_queries,
                                      const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B, int32_t dim,
                                      const np_search_params* params, const np_text_expr* text_queries, int32_t fetch_k,
                                      float alpha, int32_t fusion,
                                      const int64_t* d_subset_ids, const int64_t* d_subset_offsets,
                                      const int64_t* h_subset_offsets, int64_t n_subsets, const int32_t* d_query_subset,
                                      const np_filter* filters, int32_t n_filters, const int32_t* query_filter /* host, [B] */,
                                      int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream);

/* Host-only validation of an index directory: parses and checks every file exactly as np_hip_index_open
 * does (MmapIndex::load, index.rs:1026-1139; NPY headers mmap.rs:659-749; fast-plaid dtypes mmap.rs:1780-1808)
 * without touching a device, and reports the index geometry (out->device = -1).  Same error codes/messages as
 * np_hip_index_open. */
int np_hip_index_probe_dir(const char* index_dir, np_info* out);

/* ---- adjacent rows ----------------------------------------------------- */

/* N2: MmapIndex::get_document_embeddings / decompress_documents (index.rs:1159-1245): decompressed,
 * L2-normalised f32 embeddings of the given global doc ids, concatenated; out_lengths[i] = tokens of
 * doc i (0 for ids outside this shard).  out_embeddings may be NULL to query lengths only. */
int np_hip_decompress_documents(const np_index* index, const int64_t* doc_ids, int64_t n_docs,
                                float* out_embeddings, int64_t out_capacity_rows, int64_t* out_lengths);

/* N3: index-time encode of a flat batch of token embeddings against this index's codec -- replaces
 * ResidualCodec::compress_into_codes + compress_and_residuals + quantize_residuals (codec.rs:297-411,
 * index.rs:17-40,289-371 encode_index_chunk; the reference's CUDA path cuda.rs:185-237,353-653).
 * out_codes[t] = nearest centroid by dot product (last index among equal maxima, non-finite scores below
 * every finite one: Iterator::max_by(cmp_f32_for_max)); out_packed[t][dim*nbits/8] = residual buckets in the
 * on-disk bit layout.  bucket_cutoffs holds 2^nbits - 1 floats (bucket_cutoffs.npy).  Host pointers. */
int np_hip_encode_tokens(const np_index* index, const float* embeddings, int64_t n_tokens, int32_t dim,
                         const float* bucket_cutoffs, int64_t* out_codes, uint8_t* out_packed);

/* N4: /rerank MaxSim on caller-supplied embeddings (next-plaid-api/src/handlers/rerank.rs:57-94 compute_maxsim,
 * :139-170 scoring + sort).  query [n_query_tokens][dim]; documents concatenated, document i owns rows
 * doc_tok_offsets[i] .. doc_tok_offsets[i+1].  out_scores[n_docs] in input order; out_order (nullable) =
 * document indices sorted by descending score, stable.  NP_ERR_INVALID_ARGUMENT with the handler's message for
 * "No documents provided" and "Rerank score contains non-finite value".  Needs no index; host pointers. */
int np_hip_rerank_maxsim(int32_t device, const float* query, int32_t n_query_tokens, int32_t dim,
                         const float* doc_embeddings, const int64_t* doc_tok_offsets, int64_t n_docs,
                         float* out_scores, int64_t* out_order);

/* ---- index creation: k-means and codec training (np_build.hip) --------------------------------------------------
 * The crate's create path (index.rs:927-967 create_index_with_kmeans_files -> kmeans.rs:261-421 compute_kmeans ->
 * index.rs:182-287 prepare_codec_artifacts / index.rs:551-... create_index_files), with Lloyd's iterations on the GPU.
 *
 * k-means is fastkmeans' Lloyd (FastKMeans::train; fastkmeans-rs is not vendored, so the rules are restated here):
 *  - subsample: n > k * max_points_per_centroid keeps m = k * max_points_per_centroid points, drawn by a partial
 *    Fisher-Yates (for i in 0..m: j = i + below(n - i), swap) over 0..n-1; the subset is a[0..m) in draw order;
 *  - init: without an explicit init, centroid c = subset[p[c]] where p is the same partial Fisher-Yates of k over 0..m-1;
 *  - assign: dist = max(fma(-2, x.c, |x|^2 + |c|^2), 0) in f32 (x.c and the norms as k-ordered f32 FMA chains), argmin
 *    with the LOWEST centroid index winning equal distances (np_hip_encode_tokens is the opposite: a dot-product argmax,
 *    last index wins);
 *  - update: a non-empty cluster takes the mean of its points: a 64-bit fixed-point sum on the cluster's own scale
 *    2^S, S = 62 - e - ceil(log2 count) with max |x_j| < 2^e over the cluster's points (exact, so the bytes never depend
 *    on the order the GPU visits points in), divided by the count in f64 and rounded to f32.  The mean is within 1 f32
 *    ulp of the exact mean plus 2^(-S-1) < 2 max|x_j| count 2^-62, which depends only on the cluster's own points; an
 *    empty cluster takes subset[below(m)], drawn in ascending cluster order;
 *  - shift = sum_k |new_k - old_k| (f32 per cluster, summed in f64 in a fixed order); stop once shift < tol or after
 *    max_iters iterations.
 * Random numbers: ONE SplitMix64 stream seeded with `seed` (state += 0x9E3779B97F4A7C15, the standard output mix),
 * below(b) = the first draw r with r >= (2^64 - b) % b, taken mod b (unbiased).  Draw order: subsample, init,
 * re-initialisations.  This is NOT the crate's ChaCha8Rng + rand 0.8.5 shuffle stream: for the same seed the document
 * sample, the point subsample and the init differ from the crate's (the resulting index is equally valid).
 * Inputs: dim 1..128 (NP_ERR_SHAPE above, as search); non-finite values are refused with NP_ERR_INDEX_CREATION (the
 * crate would train on them and write garbage), and so are values above min(1e18, sqrt(0.999 FLT_MAX / (4 dim))): below
 * that bound no f32 distance can overflow to +inf. */
typedef struct np_kmeans_opts {
  int64_t k;                        /* centroids (> 0, <= points) */
  int64_t max_points_per_centroid;  /* subsample cap (fastkmeans default 256); 0 = no subsample */
  uint64_t seed;
  double tol;                       /* stop once shift < tol (compute_kmeans: 1e-8) */
  int32_t max_iters;                /* Lloyd iterations at most (compute_kmeans: kmeans_niters) */
  int32_t reserved0;
} np_kmeans_opts;

typedef struct np_kmeans_report {
  int32_t iterations;       /* Lloyd iterations run */
  int32_t reserved0;
  double shift;             /* shift of the last iteration */
  int64_t n_points;         /* points k-means ran on (after the subsample) */
  int64_t n_reinit;         /* empty clusters re-initialised, summed over the iterations */
  double ms_assign;         /* device time of the assign step (distance GEMM + argmin), summed over the iterations */
  double ms_update;         /* device time of the update step (count, scatter, means, re-init, shift) */
} np_kmeans_report;

/* The IndexConfig fields that apply (index.rs:60-112; defaults in parentheses; 0 selects the default). */
typedef struct np_index_config {
  int32_t nbits;                    /* 4 */
  int32_t kmeans_niters;            /* 4 */
  int64_t batch_size;               /* 50 000: documents per chunk */
  uint64_t seed;                    /* 42 (a seed is required: there is no entropy-seeded mode) */
  int64_t max_points_per_centroid;  /* 256 */
  int64_t n_samples_kmeans;         /* 0 = the heuristic */
  int64_t num_partitions;           /* 0 = the heuristic (ComputeKmeansConfig.num_partitions) */
  int64_t start_from_scratch;       /* 999; < 0 = never write embeddings.npy */
} np_index_config;

/* What compute_kmeans / prepare_codec_artifacts will do for these document lengths (host only, no device). */
typedef struct np_kmeans_plan {
  int64_t n_samples;        /* documents sampled for k-means: min(floor(1 + 16 sqrt(120 N)), N) or n_samples_kmeans */
  int64_t sample_tokens;    /* tokens of those documents */
  int64_t num_partitions;   /* 2^floor(log2(16 sqrt(avg_tokens_per_sampled_doc * N))) or cfg->num_partitions */
  int64_t k;                /* min(num_partitions, sample_tokens): the centroids k-means computes */
  int64_t codec_samples;    /* max(1, min(N, floor(16 sqrt(120 N)))) (prepare_codec_artifacts) */
  int64_t heldout_size;     /* floor(min(0.05 T, 50000)) */
  int64_t heldout_tokens;   /* tokens the held-out walk collects (<= heldout_size) */
} np_kmeans_plan;

/* kmeans.rs:261-311 + index.rs:199-226 formulas.  out_sample_ids (nullable, capacity n_docs): the k-means document
 * sample, the first n_samples entries of the seeded document shuffle (prepare_codec_artifacts takes the first
 * codec_samples entries of the same shuffle). */
int np_hip_kmeans_plan(const int64_t* doc_lengths, int64_t n_docs, const np_index_config* cfg, np_kmeans_plan* out,
                       int64_t* out_sample_ids);

/* FastKMeans::train on flat points [n][dim] (host pointers).  init (nullable): [k][dim] initial centroids.
 * out_centroids [k][dim] (NOT normalised).  out_assign (nullable) [n]: the last iteration's assignment of every input
 * point, -1 for points outside the subsample.  report nullable. */
int np_hip_kmeans(int32_t device, const float* points, int64_t n, int32_t dim, const np_kmeans_opts* opts,
                  const float* init, float* out_centroids, int64_t* out_assign, np_kmeans_report* report);

/* compute_kmeans (kmeans.rs:261-421): document sample, K heuristic, k-means (tol 1e-8), rows L2-normalised by
 * max(|row|, 1e-12).  embeddings = every document's tokens concatenated ([sum doc_lengths][dim]).  out_centroids has
 * room for capacity_k rows (np_hip_kmeans_plan's k); *out_k = the rows written. */
int np_hip_compute_kmeans(int32_t device, const float* embeddings, const int64_t* doc_lengths, int64_t n_docs,
                          int32_t dim, const np_index_config* cfg, float* out_centroids, int64_t capacity_k,
                          int64_t* out_k, np_kmeans_report* report);

/* prepare_codec_artifacts (index.rs:182-287): held-out tokens of the codec sample walked in reverse, codes by
 * np_hip_encode_tokens' rule, f32 residuals x - c, cluster_threshold = quantile(|r|, 0.75), avg_residual[j] = sequential
 * f32 sum of |r_j| / rows, bucket_cutoffs [2^nbits - 1] at i / 2^nbits, bucket_weights [2^nbits] at (i + 0.5) / 2^nbits
 * (quantile rule of utils.rs:94-149).  Any output pointer may be NULL. */
int np_hip_prepare_codec_artifacts(int32_t device, const float* embeddings, const int64_t* doc_lengths, int64_t n_docs,
                                   int32_t dim, const float* centroids, int64_t k, const np_index_config* cfg,
                                   float* out_bucket_cutoffs, float* out_bucket_weights, float* out_avg_residual,
                                   float* out_cluster_threshold);

/* MmapIndex::create_with_kmeans (index.rs:927-967, 551-...): compute_kmeans, prepare_codec_artifacts, every token
 * encoded on the GPU (np_hip_encode_tokens), the directory written by np_hip_index_write_dir in chunks of batch_size
 * documents, embeddings.npy + embeddings_lengths.json when n_docs <= start_from_scratch (update.rs:308-346).
 * opts->device selects the GPU (opts nullable: device 0).  out (nullable): the created index, opened with opts. */
int np_hip_index_create(const char* index_dir, const float* embeddings, const int64_t* doc_lengths, int64_t n_docs,
                        int32_t dim, const np_index_config* cfg, const np_open_opts* opts, np_index** out);

/* ---- index update and delete: MmapIndex::update / update_append / delete (np_update.cpp, np_build.hip) ----------------
 * Directory-level calls like np_hip_index_create: they read the crate's file set under index_dir and rewrite it in place;
 * a handle open on the directory keeps serving the old index until it is reopened (MmapIndex.reload in the mirrors).
 *
 * np_hip_index_update (index.rs:1431-1590) takes the crate's three modes, chosen as the crate chooses them:
 *  - start from scratch: num_documents <= start_from_scratch and embeddings.npy holds exactly num_documents documents:
 *    np_hip_index_create on old ++ new (nbits of the index, the other fields from cfg); embeddings.npy is removed when
 *    the total passes start_from_scratch.  Otherwise:
 *  - buffer: buffered + new < buffer_size: buffer.npy / buffer_lengths.json / buffer_info.json hold buffer ++ new, and
 *    the new documents are appended (update_index, update.rs:771-1120) without a threshold update;
 *  - expansion: the buffer_info.num_docs buffered documents are deleted from the tail (the buffer files stay), the
 *    outliers of buffer ++ new (tokens whose f32(min_c f64 |x - c|^2) > cluster_threshold^2 in f32) are clustered by
 *    compute_kmeans as one-token documents with num_partitions = min(max(1, ceil(n_out / max_points_per_centroid)) * 4,
 *    n_out), the new centroids are appended to centroids.npy, the buffer is cleared and buffer ++ new are appended with
 *    the threshold update (update.rs:385-416: the 0.75 quantile of the new residual norms, averaged in f32 with the old
 *    threshold by count).  Without cluster_threshold.npy there is no expansion, as in the crate.
 * All device work (outliers, k-means, encoding with the expanded codec, residual norms) is done before the first file is
 * written, so a refused input or a missing device leaves the directory unchanged.  The k-means draws come from the
 * SplitMix64 stream of np_hip_kmeans, not the crate's ChaCha8: the new centroids equal np_hip_compute_kmeans on the same
 * outliers, not the crate's bytes.  Residual norms are |x - c[code]| with the sum of squares as a sequential f32 sum
 * without contraction, the rule np_hip_prepare_codec_artifacts uses for cluster_threshold (the crate's ndarray dot may
 * sum in another order).
 * update_index: when the last chunk holds fewer than 2000 documents the first batch_size new documents join it, the rest
 * go to new chunks of batch_size; each chunk's metadata carries embedding_offset; posting list c gains the ids of the
 * new documents holding code c (a list that ascends below the first new id is appended to, any other is sorted and
 * deduplicated with its new entries, as the crate does); avg_doclen = (old_avg * old_n + new_tokens) / n in f64; the
 * merged_* caches are removed.  Inputs are checked as np_hip_index_create checks them (dim mismatch with the index:
 * NP_ERR_SHAPE; non-finite or oversized values: NP_ERR_INDEX_CREATION); n_docs == 0 changes nothing.  The new documents'
 * ids are report->first_doc_id + i. */
typedef struct np_update_config {   /* UpdateConfig (update.rs:75-107); 0 selects the default */
  int64_t batch_size;               /* 50 000: documents per new chunk */
  int32_t kmeans_niters;            /* 4 */
  int32_t reserved0;
  int64_t max_points_per_centroid;  /* 256 */
  int64_t n_samples_kmeans;         /* 0 = the heuristic */
  uint64_t seed;                    /* 42 (taken as given; only a NULL cfg selects 42) */
  int64_t start_from_scratch;       /* 999; < 0 = never */
  int64_t buffer_size;              /* 100; < 0 = 0 (every update expands) */
  int64_t reserved[4];
} np_update_config;

#define NP_UPDATE_NONE 0      /* no documents: nothing changed */
#define NP_UPDATE_SCRATCH 1
#define NP_UPDATE_BUFFER 2
#define NP_UPDATE_EXPAND 3
#define NP_UPDATE_APPEND 4    /* np_hip_index_update_append */

typedef struct np_update_report {
  int32_t mode;                 /* NP_UPDATE_* */
  int32_t reserved0;
  int64_t first_doc_id;         /* id of the first new document */
  int64_t n_outliers;           /* expansion: outlier tokens found */
  int64_t n_rechecked;          /* expansion: tokens the f64 recheck decided */
  int64_t n_new_centroids;      /* expansion: centroids appended */
  int64_t n_reindexed;          /* expansion: buffered documents deleted and appended again */
  double ms_encode;             /* host wall time of each stage */
  double ms_outliers;
  double ms_kmeans;
  double ms_files;              /* reading and rewriting the directory (start from scratch: the whole create) */
  int64_t reserved[4];
} np_update_report;

/* MmapIndex::update (index.rs:1431-1590).  embeddings = the new documents' tokens concatenated ([sum doc_lengths][dim]);
 * device = the GPU; cfg and report nullable. */
int np_hip_index_update(const char* index_dir, const float* embeddings, const int64_t* doc_lengths, int64_t n_docs,
                        int32_t dim, const np_update_config* cfg, int32_t device, np_update_report* report);

/* MmapIndex::update_append (index.rs:1675-1700): update_index only (no mode choice, no buffer, no threshold update). */
int np_hip_index_update_append(const char* index_dir, const float* embeddings, const int64_t* doc_lengths, int64_t n_docs,
                               int32_t dim, const np_update_config* cfg, int32_t device, np_update_report* report);

/* MmapIndex::delete (delete.rs:43-398), host only: every chunk that loses documents gets its doclens, codes, residuals
 * and {i}.metadata.json rewritten (embedding_offset unchanged; a chunk may become empty and stays), posting lists drop
 * the ids and renumber the rest, metadata.json gets the new counts and avg_doclen = tokens / documents, the merged_*
 * caches are removed, and embeddings.npy / buffer.npy lose the deleted documents' rows (clean_embeddings_files).
 * *out_deleted (nullable) = distinct ids removed.  Divergence from the crate: ids < 0 or >= num_documents are ignored.
 * The crate's renumbering counts every listed id below a posting-list entry, negative ones included, so a negative
 * id shifts every entry by one and its posting lists no longer match its codes; here delete([-1, 3]) equals delete([3]). */
int np_hip_index_delete(const char* index_dir, const int64_t* doc_ids, int64_t n_ids, int64_t* out_deleted);

/* ---- append to a RESIDENT index (np_index.hip) ------------------------------------------------------------------------
 * np_hip_index_update / _update_append rewrite the directory; np_hip_index_append brings a handle that is already in HBM up to
 * date without reading the index again: its cost follows the appended tokens plus one pass over the posting lists and the
 * codes, not the residuals.
 *
 * Append n_docs documents (ids num_documents .. num_documents + n_docs - 1) to a resident, unsharded handle.
 * doc_lengths [n_docs]; codes i64 [sum lengths] in [0, K); residuals u8 [sum lengths, dim*nbits/8] in FILE geometry
 * (what np_hip_encode_tokens returns and {i}.residuals.npy holds).  Posting list c gains, ascending, the new documents
 * that hold code c (update_index, update.rs:771-1120, for lists that ascend).
 *
 * Afterwards the handle equals one freshly opened on the resulting index (np_hip_index_from_arrays on the concatenated
 * arrays, np_hip_index_open on the directory np_hip_index_update_append wrote): np_hip_index_export, np_hip_index_info
 * (but device_bytes / workspace_bytes) and every search entry return the same bytes.  avg_doclen becomes (old_avg * old_n +
 * new_tokens) / n in f64, the expression the directory update writes; a handle made from arrays, which has no stored figure,
 * keeps reporting tokens / documents.  n_docs == 0 changes nothing.
 *
 * Refused with NP_ERR_INVALID_ARGUMENT or NP_ERR_SHAPE, the argument named, before any allocation or launch, the handle
 * answering as it did: a sharded handle; a handle whose posting lists do not ascend (only such lists grow at their end); a
 * negative length; a code outside [0, K); totals beyond the open path's limits (2^31 documents -- and, found once the new
 * documents' distinct codes are counted, the 40-bit list offset and the 32-bit overflow index: refused then, the handle
 * unchanged all the same).  Centroid expansion (K changes): np_hip_index_expand (below).  Delete: np_hip_index_remove (below).
 *
 * Attachments: metadata columns, the keyword index and the groups are DROPPED, as a reload leaves a handle: their rows no
 * longer cover the documents.  np_hip_index_set_columns / _set_text / _set_groups attach the grown ones, or
 * np_hip_index_append_rows (below) takes the new documents' rows and keeps columns and groups.
 *
 * Memory: capacity grows first and commits nothing.  Without a reservation every per-token array (codes, residuals, inverse
 * norms) grows by allocate, copy device to device, free -- one array at a time, so the peak is the LARGEST ARRAY TWICE (the
 * residuals: 128 bytes of the ~145 per token at dim 128, 4 bits).  On a device that full, reserve at open time
 * (np_hip_index_reserve right after the open: later appends within the reservation move no per-token array) or reload.  The
 * derived arrays that are laid out again -- distinct-code blocks, posting lists, range table -- are allocated BESIDE the old
 * ones and swapped in when nothing can fail any more: NP_ERR_OUT_OF_MEMORY leaves the handle unchanged (its capacity may
 * have grown).
 *
 * Concurrency: append, remove and reserve check out EVERY context of the handle's pool: calls that run finish on the index as it
 * was, calls that arrive wait, nobody observes a half-grown handle.  The entries that read the handle outside a context are
 * registered from their first line to their last and waited for in the same way: np_hip_decompress_documents (it reads the
 * token arrays an unreserved append frees) and every entry that checks columns, keyword index or groups before it takes a
 * context (np_hip_filter_eval, np_hip_text_match, the _filtered, text, hybrid, grouped and collapse entries) -- beside an append
 * such a call answers from the attachments it checked, or gets the error of a handle without them, never a handle that
 * changed under it.  What may NOT run beside append or reserve, as before this call existed: np_hip_index_export,
 * np_hip_index_set_columns, _set_column_text, _set_text and _set_groups (they change the handle themselves and need
 * exclusive access), np_hip_index_close, and the sharded entries (a sharded handle is refused anyway).  A context between np_hip_search_phase_a and
 * np_hip_search_end counts as running: end such calls first -- an append from the thread that holds one waits for itself.
 * np_hip_index_remove is exactly the same: it waits for the same calls, and the same entries may not run beside it.
 * NP_APPEND_TRACE=1 prints the stages' seconds to stderr (tools/append_time.py reads them). */
int np_hip_index_append(np_index* index, const int64_t* doc_lengths, int64_t n_docs,
                        const int64_t* codes, const uint8_t* residuals);
/* Room for this many MORE documents / tokens, so that later appends move no per-token array. */
int np_hip_index_reserve(np_index* index, int64_t extra_docs, int64_t extra_tokens);
int np_hip_index_capacity(const np_index* index, int64_t* docs, int64_t* tokens);   /* allocated, not used */

/* ---- remove from a RESIDENT index (np_index.hip) -----------------------------------------------------------------------
 * np_hip_index_delete rewrites the directory; np_hip_index_remove takes the same documents out of a handle that is already
 * in HBM without reading the index again: one pass over the posting lists, one move of the tokens behind the first removed
 * document.
 *
 * The semantics are np_hip_index_delete's (delete.rs:43-268), applied to the handle: ids outside [0, num_documents) are
 * ignored, duplicates count once, *out_removed (nullable) = the distinct documents removed.  Surviving document d gets the id
 * d - |{removed ids < d}|; each posting list keeps its surviving entries in its own order, renumbered.
 *
 * Afterwards the handle equals one freshly opened on the resulting index (np_hip_index_from_arrays on the shrunk arrays,
 * np_hip_index_open on the directory np_hip_index_delete wrote): np_hip_index_export, np_hip_index_info (but device_bytes /
 * workspace_bytes) and every search entry return the same bytes.  avg_doclen becomes tokens / documents in f64 (0.0 without
 * documents), what the directory delete writes; num_embeddings follows; max_doc_len is that of the survivors.  If no listed
 * id is in range nothing changes and the attachments stay.  Removing EVERY document leaves the handle that
 * np_hip_index_from_arrays makes of the empty arrays (it opens: an index without documents answers every search with no rows).
 *
 * Refused with NP_ERR_INVALID_ARGUMENT, by name, before any allocation or launch, the handle answering as it did: a NULL
 * handle, n_ids < 0, NULL doc_ids with n_ids > 0, a sharded handle.  Posting lists that do not ascend are NOT refused (the
 * filter keeps a list's own order, as the directory delete does): they stay flagged as not ascending -- even where the
 * removal leaves them ascending -- and the zeroth filter level stays off.
 *
 * Capacity (np_hip_index_capacity) does not shrink: the freed room is a reservation, an append that fits in it moves no
 * per-token array.  Attachments -- metadata columns, the keyword index, the groups -- are DROPPED, as a reload leaves a
 * handle: attach the survivors' rows again, or call np_hip_index_remove_keep (below), which compacts columns and groups.
 *
 * Memory: everything that allocates happens before anything that serves is overwritten -- the survivor bitmap and the new
 * doc offsets, the codes compacted BESIDE the old ones (2 to 4 of the ~145 bytes per token), the distinct-code blocks built
 * from them, the filtered posting lists and their offsets, the range table, and one staging buffer of fixed size
 * (np_hip_index_tune "remove_slab" tokens, 0 = the default 2^21, times the residual row).  NP_ERR_OUT_OF_MEMORY up to there
 * leaves the handle unchanged.  Residuals, inverse norms and token positions are then compacted IN PLACE, slab by slab in
 * ascending order (np_remove_plan.h): no second copy of the residuals exists at any time.
 *
 * Concurrency: as np_hip_index_append (above).  NP_REMOVE_TRACE=1 prints the stages' seconds and the two kernels' own times
 * to stderr (tools/remove_time.py reads them). */
int np_hip_index_remove(np_index* index, const int64_t* doc_ids, int64_t n_ids, int64_t* out_removed);

/* ---- remove from a RESIDENT index and KEEP its columns and groups (np_index.hip) -----------------------------------------
 * np_hip_index_remove_keep is np_hip_index_remove with one difference: the metadata columns (with their dictionary text) and
 * the groups are compacted and renumbered with the documents, on the device, and stay attached.  Afterwards the handle equals
 * a fresh one of the shrunk arrays with np_hip_index_set_columns / _set_column_text / _set_groups of the surviving rows:
 *  - a column keeps its type; the survivor with new id j has the value and the validity of its old row; a column whose
 *    surviving rows hold no NULL has no validity bitmap (as set_columns leaves it), one without a bitmap stays without;
 *  - the code range of a CODE column that np_hip_index_set_column_text checks is that of the surviving rows, so a shorter
 *    dictionary is accepted exactly as on a fresh handle; the text on the device is per code, not per document, and stays;
 *  - the groups keep n_groups: an emptied group is a group without members;
 *  - np_info.device_bytes follows the new sizes.
 * The keyword index is DROPPED: its term numbering follows the vocabulary, and a term whose last row is removed renumbers the
 * rest.  np_hip_text_build_merge computes the index of the surviving rows; the host mirrors compose the two calls.
 *
 * Removing nothing changes nothing.  Removing EVERY document leaves what the setters make of an empty handle: columns without
 * rows (no bitmap, the empty code range), and NO groups -- np_hip_index_set_groups takes no ids as "drop the groups".
 *
 * Memory: the new column, validity and group arrays (at most 8 bytes per document and column) are allocated and filled BESIDE
 * the old ones before anything that serves is overwritten, in the remove's own order: NP_ERR_OUT_OF_MEMORY up to there leaves
 * the index and its attachments unchanged.  Refusals and concurrency are np_hip_index_remove's: a filtered or grouped call that
 * runs beside it sees the old index with the old attachments or the new with the new, never a mixture.  NP_REMOVE_TRACE=1
 * also prints the compaction kernels' own time and rate. */
int np_hip_index_remove_keep(np_index* index, const int64_t* doc_ids, int64_t n_ids, int64_t* out_removed);

/* ---- append to a RESIDENT index WITH the new documents' rows (np_index.hip) --------------------------------------------------
 * np_hip_index_append_rows is np_hip_index_append (its first five arguments, its checks, its memory and failure order, its
 * concurrency) with the new documents' rows: the columns and the groups stay attached and grow with the index.  Afterwards the
 * handle equals a fresh one of the grown arrays with np_hip_index_set_columns / _set_groups of all rows.
 *  - new_cols[i] holds the n_docs NEW entries of column i (data, valid: bytes over the new documents alone).  n_cols must equal
 *    the handle's column count and every type its column's type.  A column without a validity bitmap gets one only if a new
 *    row is NULL (all earlier rows are then valid); an f64 NaN is NULL, as in set_columns.
 *  - code_remap (nullable) has one entry per column, each NULL or, for a CODE column, an i32 table old code -> new code over
 *    the codes 0 .. the largest code the handle's rows hold: the case of a dictionary that grew -- it is sorted by bytes, so
 *    new strings shift codes.  It must be strictly increasing and not negative.  It is applied on the device to the old rows
 *    that are not NULL (a NULL row's code means nothing and keeps its bytes); the new rows come in new codes.  The column's
 *    text on the device, if any, is DROPPED with a remap: np_hip_index_set_column_text sets the grown dictionary.
 *  - new_groups: n_docs ids in [0, n_groups), n_groups >= the handle's.  Required when the handle has groups, refused when it
 *    has none; in the same way n_cols = 0 is required of a handle without columns.
 *  - The keyword index is DROPPED, as by np_hip_index_remove_keep: the host mirrors compose np_hip_text_build_merge.
 * Every violation is NP_ERR_INVALID_ARGUMENT, by name, before any allocation, the handle answering as it did with the
 * attachments it had.  n_docs == 0 runs the checks and changes nothing (no remap either).
 *
 * Memory: the per-document attachment arrays grow to the handle's document capacity with d_doc_offsets -- in this call and in
 * np_hip_index_reserve -- so an append inside a reservation moves none of them (np_hip_index_set_columns itself allocates
 * for the documents the handle has: reserve after it).  The new rows are staged on the device, and a first validity bitmap
 * allocated, before anything that serves is touched: NP_ERR_OUT_OF_MEMORY up to there leaves index and attachments as they
 * were.  The validity bits of the new rows are merged at the word that holds the old last document.  What comes after --
 * the remap, the rows' move, the merge, the code range read back -- allocates nothing; if the device stops answering there the
 * call returns NP_ERR_DEVICE_UNAVAILABLE with the handle already grown, as np_hip_index_remove does for its token move. */
int np_hip_index_append_rows(np_index* index, const int64_t* doc_lengths, int64_t n_docs, const int64_t* codes,
                             const uint8_t* residuals, const np_column* new_cols, int32_t n_cols,
                             const int32_t* const* code_remap, const int32_t* new_groups, int64_t n_groups);

/* ---- expand a RESIDENT index: new centroids, the buffered tail re-encoded, new documents (np_index.hip) --------------------
 * The crate's usual update (MmapIndex::update above its buffer size, np_hip_index_update in expansion mode) deletes the
 * buffered documents from the tail, appends new centroids to centroids.npy and appends buffer ++ new documents encoded
 * against the grown codec.  np_hip_index_expand brings a handle that is already in HBM along, without reading the index again.
 *
 *  - new_centroids f32 [k_new][dim], FILE geometry (rows are padded to the storage width as the open path pads them): they
 *    become centroids K .. K + k_new - 1; K1 = K + k_new.
 *  - the first n_replace of the n_docs documents REPLACE the handle's last n_replace documents: the same ids, new lengths,
 *    codes and residuals.  The other n_docs - n_replace take the ids num_documents .. as an append's do.
 *  - codes i64 in [0, K1); residuals in file geometry, as for np_hip_index_append.
 *
 * Afterwards the handle equals one freshly opened on the resulting index (np_hip_index_from_arrays on old centroids ++ new and
 * the old documents without their last n_replace ++ the given ones; np_hip_index_open on the directory np_hip_index_update wrote
 * in expansion mode): np_hip_index_export, np_hip_index_info (but device_bytes / workspace_bytes) and every search entry return
 * the same bytes.  avg_doclen follows the directory's arithmetic, delete and then append: tokens / documents in f64 after the
 * tail drop (n_replace > 0), then (avg * n + new_tokens) / n1; a handle made from arrays keeps reporting tokens / documents.
 * k_new == 0 && n_replace == 0 is np_hip_index_append; n_docs == 0 && k_new > 0 adds centroids with empty posting lists; all
 * three zero changes nothing.
 *
 * What follows K1: the centroid table, cmax / filter_ok / s6_fast_ok over ALL K1 rows (non-finite values are accepted as the
 * open path accepts them), the code width (K <= 65536 < K1: the u16 codes are widened to u32 by one streaming kernel into an
 * array beside the narrow one), the eighths of the centroid range in every document's distinct-code record, the list offsets,
 * the range table (whose range count follows the NEW document count, down as well as up) and the planner's candidate bound.
 * The distinct-code blocks are built once over the final documents; the posting lists are rewritten in one streaming pass:
 * list c keeps its entries below the first replaced id (the lists ascend: one bisection) and gains, ascending, the given
 * documents that hold code c; lists K .. K1 - 1 start empty.
 *
 * One exclusive section (Concurrency: as np_hip_index_append): a search beside it sees the old index or the new one, never the
 * index without its tail and never K1 centroids without their documents.
 *
 * Memory and failure order: capacity grows first and commits nothing.  The grown centroid table, the wide codes, the
 * distinct-code blocks, the posting lists and the range table are allocated BESIDE what serves.  The given documents' tokens
 * land where the replaced tail was: the tail's per-token bytes and doc offsets are saved in a side buffer first and put back,
 * with K, the code width and the bounds, on any failure before the swap.  NP_ERR_OUT_OF_MEMORY leaves the handle answering as
 * it did (its capacity may have grown).
 *
 * Refused with NP_ERR_INVALID_ARGUMENT or NP_ERR_SHAPE, the argument named, before any allocation or launch, the handle
 * answering as it did: a NULL or sharded handle; posting lists that do not ascend; k_new < 0, or NULL new_centroids with
 * k_new > 0; n_replace < 0, > n_docs or > the handle's documents; a negative length (NP_ERR_SHAPE); a code outside [0, K1);
 * totals beyond the open path's limits (2^31 documents, K1 >= 2^31 -- and, found once the distinct codes are counted, the
 * 40-bit list offset and the 32-bit overflow index: refused then, the handle restored).
 *
 * Attachments: np_hip_index_expand DROPS columns, keyword index and groups, as np_hip_index_append does.
 * np_hip_index_expand_rows keeps columns and groups: the replaced documents keep their ids, so their rows STAY, and new_cols /
 * new_groups cover only the n_docs - n_replace NEW documents.  Apart from that it has the arguments, checks, remap, memory order
 * and keyword-index rule of np_hip_index_append_rows; with no new document the attachments stay as they are.
 * NP_APPEND_TRACE=1 prints this call's stages too (tag "np expand"; tools/expand_time.py reads them). */
int np_hip_index_expand(np_index* index, const float* new_centroids, int64_t k_new, int64_t n_replace,
                        const int64_t* doc_lengths, int64_t n_docs, const int64_t* codes, const uint8_t* residuals);
int np_hip_index_expand_rows(np_index* index, const float* new_centroids, int64_t k_new, int64_t n_replace,
                             const int64_t* doc_lengths, int64_t n_docs, const int64_t* codes, const uint8_t* residuals,
                             const np_column* new_cols, int32_t n_cols, const int32_t* const* code_remap,
                             const int32_t* new_groups, int64_t n_groups);

/* Read the handle's attachments back to the host, array for array.  np_hip_index_get_column: `data` (nullable) takes the
 * column's rows over the documents this handle holds (i64 / f64 / i32 by *type), `valid` (nullable) one byte per document, 0 =
 * NULL (all 1 where the column has no bitmap); *type and *has_valid (nullable) report the column's type and whether it holds
 * a validity bitmap.  np_hip_index_get_groups: `out` takes the group of every document.  NP_ERR_INVALID_ARGUMENT, by name: a
 * NULL handle, a column outside the handle's, a handle without groups.  Both are registered like the entries that check the
 * attachments before they take a context: an append or a remove waits for them. */
int np_hip_index_get_column(const np_index* index, int32_t column, void* data, uint8_t* valid, int32_t* type,
                            int32_t* has_valid);
int np_hip_index_get_groups(const np_index* index, int32_t* out);

/* ---- token pooling: pool_document_embeddings (np_pool.hip) --------------------------------------------------------------
 * next-plaid-onnx pools every document before it reaches the index (src/lib.rs:1632-1643 pool_document_embeddings ->
 * :2249-2317 pool_embeddings_hierarchical -> hierarchy.rs:599-653 pdist_cosine, :128-284 Ward linkage by nearest-neighbour
 * chain, :426-517 fcluster_maxclust).  Per document of n tokens, with p = protected_tokens and f = pool_factor:
 *  - n <= p + 1, or k = max((n - p) / f, 1) >= n - p, or f <= 1: the document is returned unchanged;
 *  - otherwise the first p rows are copied and the other m = n - p rows are clustered into k clusters; a cluster's row is the
 *    f32 sum of its members in token order divided by the count as f32 (not renormalised); clusters are ordered by the first
 *    token that belongs to them.
 * Distances: norms and dot products are f64 sums over the features in feature order of the f32 inputs widened to f64,
 * cos = dot / (ni nj) (0 when a norm is 0), d = clamp(1 - cos, 0, 2); Ward's Lance-Williams update runs on d * d in f64 without
 * contraction.  Linkage: a chain starts at the lowest active id, a nearest neighbour is the strict minimum (ties to the lowest
 * id), and the reference's nearest-neighbour CACHE is kept: an entry is recomputed only for the new cluster and for a cluster
 * whose cached neighbour was one of the two just merged.  Merges are recorded as [min id, max id, sqrt(d^2), size] in the
 * order the chain finds them.  The results equal the reference's bit for bit and never depend on the chunking or on the
 * other documents of the call.
 * cut_order: 0 (the reference, and what an index built by the crate holds) applies the first m - k merges IN CHAIN ORDER
 * (fcluster_maxclust reads the unsorted list); 1 applies the first m - k merges of a stable sort by merge distance: the
 * dendrogram cut of scipy's fcluster(linkage(., 'ward'), k, 'maxclust') and of PyLate.  The two partitions differ on most
 * documents ("Token pooling"). */
typedef struct np_pool_opts {
  int32_t pool_factor;       /* <= 1: every document is copied through */
  int32_t protected_tokens;  /* leading rows kept as they are (the reference fixes 1) */
  int32_t cut_order;         /* 0 = chain order (the reference), 1 = stable order by merge distance (scipy / PyLate) */
  int32_t reserved0;
  int64_t chunk_docs;        /* documents per device chunk at most; 0 = as many as the free device memory takes */
  int64_t reserved[3];
} np_pool_opts;

typedef struct np_pool_report {
  int64_t n_docs;            /* documents in */
  int64_t n_pooled;          /* documents that were clustered (the others were copied through) */
  int64_t tokens_in;
  int64_t tokens_out;
  double ms_distances;       /* device time of the three stages, summed over the chunks */
  double ms_linkage;
  double ms_means;
  int64_t n_chunks;
  int64_t reserved[3];
} np_pool_report;

/* Host only: out_lengths[i] = tokens of document i after pooling. */
int np_hip_pooled_lengths(const int64_t* doc_lengths, int64_t n_docs, const np_pool_opts* opts, int64_t* out_lengths);

/* embeddings = every document's tokens concatenated ([sum doc_lengths][dim]); out_embeddings has room for
 * out_rows_capacity rows (sum of np_hip_pooled_lengths); out_lengths [n_docs].  out_labels (nullable) [sum doc_lengths]:
 * 0 for a protected token or a token of an unchanged document, 1.. for the clusters in output order.  out_linkage
 * (nullable): [m - 1][4] f64 per CLUSTERED document, concatenated in document order.  report nullable.  Host pointers; needs
 * no index.  Non-finite inputs: NP_ERR_INVALID_ARGUMENT (the reference would index with usize::MAX).  A document that hands
 * more than 2048 tokens to the clustering: NP_ERR_SHAPE. */
int np_hip_pool_documents(int32_t device, const float* embeddings, const int64_t* doc_lengths, int64_t n_docs, int32_t dim,
                          const np_pool_opts* opts, float* out_embeddings, int64_t out_rows_capacity, int64_t* out_lengths,
                          int32_t* out_labels, double* out_linkage, np_pool_report* report);

/* ---- Building the keyword index on the device (np_textbuild.hip; DESIGN.md section 4, "Building the keyword index") ----
 * From raw document text to the arrays np_hip_index_set_text takes, equal array for array to what SQLite's FTS5 gives for
 * the same rows (fts5vocab 'instance': every (term, document, position), terms in memcmp order, the shorter string first).
 * Input: the documents' UTF-8 bytes concatenated and offsets[n_docs + 1] into them (host pointers, uploaded by the call);
 * document i is the FTS5 row with rowid i.  Needs no index.
 *
 * By default the device reproduces SQLite for ASCII text only:
 *   NP_TOK_UNICODE61  token characters are [0-9A-Za-z]; every other byte 0x00..0x7F separates (NUL too); A-Z fold to a-z;
 *                     positions count tokens from 0
 *   NP_TOK_TRIGRAM    every byte offset i <= len - 3 is a token: the three bytes, A-Z folded, at position i
 * UTF-8 mode (opt-in: NP_TOK_UNICODE61 with opts->unicode_table set; NP_TOK_TRIGRAM ignores the table) reproduces unicode61
 * (remove_diacritics=1) for every code point the caller's table covers.  The table has one uint32 per code point of its
 * planes (unicode_table_len = planes * 65536, 1..17 planes): bits 0-20 the folded code point, bits 30-31 the class -- 0 a
 * separator, 1 a token character (the term gets its fold, always one code point), 2 a mark: it continues a token that is
 * open and contributes nothing to the term, and separates otherwise.  The rule is SQLite's, so the table is probed from
 * SQLite by the caller (text.unicode61_table); none of it is compiled in.  Checked before any launch (np_textbuild_plan.h,
 * textbuild_check_table): the length, classes <= 2, folds below 0x110000 and no surrogates, entries 0..127 exactly the
 * ASCII rule above (a separator's entry is 0), no fold whose UTF-8 form is more than one byte longer than its source.
 * Instances still name raw byte ranges of the text; two tokens are one term when their folded code points, marks skipped,
 * are equal, whatever their raw lengths, and the vocabulary holds the folded strings.
 * A document it cannot reproduce is a FALLBACK document: it contributes no instance, its id is listed by
 * np_hip_text_build_fallback, and the caller tokenises it (with SQLite) and hands its instances to np_hip_text_build_add.
 * Fallback rules: any byte >= 0x80; trigram: a NUL byte (it ends the text for SQLite); unicode61: a token longer than
 * max_token_bytes (1..32768, 0 = 256; SQLite cuts a token at 32768).  The cap only moves documents to the list: it never
 * changes the result.  UTF-8 mode replaces the first rule: a malformed sequence (a stray continuation byte, an overlong
 * form, a surrogate, a value above U+10FFFF, F8..FF, a lead whose continuation bytes are missing at the document's end --
 * the next document's bytes never complete it), a code point at or beyond the table's length.  There the cap counts the
 * token's raw bytes, marks included, and max_token_bytes above 21845 is refused (a fold grows a token by at most 3/2).
 *
 * Stages (each a sequence of launches; no workgroup waits for another inside a launch, only integer atomics are used and
 * no result depends on the order in which they arrive):
 *   classify  one wave per document over 16-byte loads: the fallback verdict and the document's token count; an exclusive
 *             scan of the counts places every document's first instance
 *   emit      the same walk writes instance n = (document, byte offset in the document, length): (document, position) order
 *             by construction
 *   terms     unicode61: an open-addressing table of instance indexes claimed by atomicCAS; a lane that finds a slot taken
 *             compares its token's folded bytes with the bytes of the instance in the slot (both in the immutable text), so
 *             a hash collision never merges two terms; a table that fills up is counted, detected on the host and the stage
 *             repeated with twice the slots (report->table_retries).  The occupied slots are compacted, the host sorts
 *             their strings and a slot's rank is its term id.  trigram: a presence bitmap over the 21-bit folded keys and a
 *             popcount scan give the rank directly
 *   order     a stable LSD radix sort of (term id, instance index) by term id, 8 bits a pass (histogram, scan, scatter),
 *             ceil(bits(n_terms - 1) / 8) passes; then a gather writes inst_doc / inst_pos and the run starts term_offsets
 *
 * np_hip_text_build runs the stages and returns a build.  Then, in this order: np_hip_text_build_fallback (any time before
 * free), at most one np_hip_text_build_add, np_hip_text_build_sizes (finalises: with nothing added the device arrays are
 * the result as they are; otherwise one linear host merge unites the vocabularies and merges, per term, the two runs by
 * document -- their document sets are disjoint), np_hip_text_build_fetch, np_hip_text_build_free.  n_rows of the result is
 * n_docs (FTS5's nRow counts empty rows).  A build is not shared between threads.
 *
 * Refused before any launch, the message naming the argument.  NP_ERR_INVALID_ARGUMENT: offsets that do not ascend from 0,
 * an unknown tokenizer, max_token_bytes outside 0..32768 (UTF-8 mode: 0..21845), a unicode_table that fails its checks, a
 * hash_bits or tile_bytes knob out of range; for
 * np_hip_text_build_add: instances out of (term, document, position) order, terms out of memcmp order, a document that is
 * not on the fallback list, a second add or an add after np_hip_text_build_sizes.  NP_ERR_SHAPE: a document longer than
 * 2^31 - 1 bytes, 2^31 documents or more, 2^31 instances or more in one call (known for unicode61 only after the counting
 * launch: refused then, before anything is emitted).  NP_ERR_OUT_OF_MEMORY: a workspace (workspace_bytes, or the device's
 * free memory) that does not hold the call.  One call is a whole-corpus sort; a corpus that does not fit one call is built
 * in document ranges that np_hip_text_build_merge (below) appends to one another. */
#define NP_TOK_UNICODE61 0
#define NP_TOK_TRIGRAM 1
#define NP_TEXT_BUILD_MAX_TOKEN_BYTES 32768

typedef struct np_text_build_opts {
  int32_t tokenizer;         /* NP_TOK_UNICODE61 / NP_TOK_TRIGRAM */
  int32_t max_token_bytes;   /* unicode61: a longer token sends its document to the fallback list; 0 = 256 */
  int64_t workspace_bytes;   /* device bytes the call may hold at once; 0 = what the device has free */
  int32_t hash_bits;         /* test knob: log2 of the first term table, 1..31; 0 = planned from the instance count */
  int32_t tile_bytes;        /* test knob: bytes a wave walks per step, a multiple of 16 in 16..1024; 0 = 1024 */
  const uint32_t* unicode_table;   /* host pointer; non-NULL with NP_TOK_UNICODE61 = UTF-8 mode (see above); NULL = ASCII */
  int64_t unicode_table_len;       /* entries: a multiple of 65536 in 65536 .. 17 * 65536 */
  int64_t reserved[1];
} np_text_build_opts;

typedef struct np_text_build_report {
  int64_t n_docs;
  int64_t n_fallback;        /* documents on the fallback list */
  int64_t n_instances;       /* instances the device emitted (the fallback documents' are not among them) */
  int64_t n_terms;           /* distinct terms of those instances */
  int64_t term_bytes;        /* bytes of their strings */
  int32_t table_retries;     /* times the term table filled up and was doubled */
  int32_t sort_passes;
  int32_t hash_bits;         /* of the table that held the vocabulary (0 for trigram) */
  int32_t tile_bytes;
  double ms_upload;          /* host to device copy of the text */
  double ms_classify;        /* classify, count and the scan */
  double ms_emit;
  double ms_terms;           /* table or bitmap, compaction, the host's sort of the vocabulary, term ids */
  double ms_sort;            /* radix passes, gather, term_offsets */
  double ms_total;           /* wall time of the call */
  int64_t workspace_bytes;   /* device bytes held at the peak */
  int64_t reserved[3];
} np_text_build_report;

typedef struct np_text_build np_text_build;

int np_hip_text_build(int32_t device, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs,
                      const np_text_build_opts* opts, np_text_build** out_build, np_text_build_report* report /* nullable */);
/* The fallback documents' ids, ascending: out_doc_ids [report->n_fallback] (NULL: count only).  *out_count nullable. */
int np_hip_text_build_fallback(const np_text_build* build, int64_t* out_doc_ids, int64_t* out_count);
/* The fallback documents' instances, tokenised by the host: n_terms strings (bytes + offsets[n_terms + 1]) in ascending
 * memcmp order, each with at least one instance, and n instances sorted by (term, doc, pos), inst_term indexing the strings. */
int np_hip_text_build_add(np_text_build* build, const uint8_t* term_bytes, const int64_t* term_byte_offsets, int64_t n_terms,
                          const int32_t* inst_term, const int64_t* inst_doc, const int32_t* inst_pos, int64_t n);
int np_hip_text_build_sizes(np_text_build* build, int64_t* n_terms, int64_t* term_bytes, int64_t* n_instances, int64_t* n_rows);
/* term_bytes [term_bytes], term_byte_offsets [n_terms + 1], term_offsets [n_terms + 1], inst_doc / inst_pos [n_instances];
 * any pointer may be NULL.  After np_hip_text_build_sizes. */
int np_hip_text_build_fetch(const np_text_build* build, uint8_t* term_bytes, int64_t* term_byte_offsets, int64_t* term_offsets,
                            int64_t* inst_doc, int32_t* inst_pos);
void np_hip_text_build_free(np_text_build* build);

/* ---- Merging keyword indexes: append, delete and replace rows (np_textmerge.hip; DESIGN.md section 4, "Keeping the keyword
 * index current") ----
 * The crate keeps its FTS5 table incremental: index() appends rows, delete() removes them, update_rows() replaces their text
 * and rebuild() renumbers the survivors.  np_hip_text_build_merge is the one operation behind all four: from
 *   the base index A   the arrays of np_text_index (host pointers) and its vocabulary: n_terms strings, bytes + offsets
 *                      [n_terms + 1], in ascending term order (memcmp, the shorter string first)
 *   remap [n_remap]    a verdict per old document id: -1 = removed, otherwise the id it has in the result.  The survivors'
 *                      ids ascend strictly (renumbering keeps the order)
 *   the batch B        the build of the new texts, as np_hip_text_build returns it, finalised by np_hip_text_build_sizes
 *                      (so the fallback documents' instances are in it); NULL = no new text.  Its arrays are read where they
 *                      lie in HBM; a build that np_hip_text_build_sizes merged on the host is uploaded
 *   delta_ids [batch n_docs]   the id every batch document gets: ascending strictly, none of them a survivor's id
 *   n_rows_out         FTS5's nRow of the result
 * it returns the keyword index of the resulting table, equal array for array (terms, term_offsets, inst_doc, inst_pos,
 * n_rows) to building that table from scratch with SQLite.  A term whose last instance went is not listed any more.
 *   append (index)        remap[d] = d, delta_ids = n, n + 1, ...
 *   delete                remap[d] = -1 for the deleted rows, d for the others (ids keep their holes); no batch
 *   delete + rebuild      the survivors numbered 0, 1, ... in order; no batch
 *   replace (update_rows) remap[d] = -1 for the replaced rows and the batch holds their new texts with delta_ids = those ids
 * or any mix of them in one call.  The result is a finalised np_text_build: np_hip_text_build_sizes, _fetch and _free serve
 * it, np_hip_text_build_fallback lists nothing and np_hip_text_build_add is refused.  No handle is involved.
 *
 * The host unites the two sorted vocabularies and computes bound[j], the smallest old id whose survivor id is >=
 * delta_ids[j] (both linear).  On the device (each step a launch; no workgroup waits for another, no atomics, integers only,
 * so the bytes are a function of the inputs alone):
 *   keep    keep[i] = remap[doc_A[i]] >= 0, and S = its exclusive scan
 *   count   per union term: kept instances of A's run (two reads of S) + the length of B's run; an exclusive scan places
 *           the terms' runs, a scan of "any left" numbers the terms that stay; the flags go to the host, which compacts the strings
 *   place   a kept A instance: its run's start + the kept instances of its run before it + the instances of B's run with a
 *           lower new id (a binary search); a B instance: its run's start + its index in B's run + the kept instances of A's
 *           run whose OLD id is below bound[its document] (a binary search over A's run, then S).  term_offsets are the
 *           run starts of the terms that stay
 *
 * Refused before any launch, the message naming the argument.  NP_ERR_INVALID_ARGUMENT: base arrays that fail
 * np_hip_index_set_text's checks (against n_remap documents: a base document >= n_remap is one of them), base or batch
 * terms out of order, survivor ids that do not ascend strictly, delta_ids that do not ascend strictly or name a survivor's
 * id, a batch that is not finalised or lives on another device, n_rows_out below the result's distinct documents.  (That the
 * two sides were tokenised alike cannot be known here: it is the caller's check.)  NP_ERR_SHAPE: 2^31 instances or more in
 * the base, the batch or both together.  NP_ERR_OUT_OF_MEMORY: a workspace that does not hold the call -- the need depends
 * on the sizes alone and is report->workspace_bytes. */
typedef struct np_text_merge_opts {
  int64_t workspace_bytes;   /* device bytes the call may hold at once; 0 = what the device has free */
  int64_t reserved[3];
} np_text_merge_opts;

typedef struct np_text_merge_report {
  int64_t n_base_terms;
  int64_t n_base_instances;
  int64_t n_old_docs;            /* n_remap */
  int64_t n_survivors;           /* old documents that stay */
  int64_t n_delta_docs;
  int64_t n_delta_terms;
  int64_t n_delta_instances;
  int64_t n_terms;               /* of the result */
  int64_t n_instances;
  int64_t n_rows;
  int64_t n_terms_dropped;       /* terms of the union without an instance left */
  int64_t n_instances_dropped;   /* instances of removed documents */
  int32_t delta_uploaded;        /* 1: the batch's arrays came from the host (it held fallback documents, or was empty) */
  int32_t reserved0;
  double ms_check;               /* the checks, the vocabulary union and bound, on the host */
  double ms_upload;              /* the base's arrays and the maps, host to device */
  double ms_count;               /* keep, the scans, the terms' counts; the flags back */
  double ms_terms;               /* the host's compaction of the strings */
  double ms_place;               /* the two placing launches and term_offsets */
  double ms_total;               /* wall time of the call */
  int64_t workspace_bytes;       /* device bytes the call needs (planned from the sizes, an upper bound of what it held) */
  int64_t reserved[3];
} np_text_merge_report;

int np_hip_text_build_merge(int32_t device, const np_text_index* base, const uint8_t* base_term_bytes,
                            const int64_t* base_term_byte_offsets, const int64_t* remap, int64_t n_remap,
                            const np_text_build* delta /* finalised; NULL = empty batch */, const int64_t* delta_ids /* [delta's n_docs] */,
                            int64_t n_rows_out, const np_text_merge_opts* opts /* nullable */, np_text_build** out_build,
                            np_text_merge_report* report /* nullable */);

/* ---- The resident keyword index: built and updated without leaving HBM (np_textres.hip; DESIGN.md section 4, "The resident
 * keyword index") ----
 * np_hip_text_build and np_hip_text_build_merge leave their result in HBM; these entries keep it there.  Only the vocabulary
 * strings and a few counts cross the bus.
 *
 * np_hip_index_set_text_build installs a finalised build (np_hip_text_build + _add + _sizes, or a merge's result) as the
 * handle's keyword index.  The result equals, array for array, np_hip_index_set_text given the arrays
 * np_hip_text_build_fetch would return.  On the device (each step a launch; no workgroup waits for another; integers only;
 * the one atomic is the integer add into a document's length, whose sum does not depend on the order of arrival):
 *   check     np_hip_index_set_text's checks per instance -- the document inside [0, n_docs), the position >= 0, (document,
 *             position) ascending strictly inside a term; every block reports its lowest offender, the host takes the minimum
 *             and names that instance and its rule
 *   heads     instance i starts a posting when it is the first of its term (the term starts come from term_offsets) or names
 *             another document than instance i - 1: two neighbouring terms that end and begin with one document stay apart
 *   postings  an exclusive scan of the heads numbers the postings; a head writes its document and its own index (the
 *             posting's first position); the term frequency is the distance to the next head; a term's list starts at the
 *             rank of its first instance (a term without instances has an empty list)
 *   doc_len   every posting adds its term frequency to its document; n_rows must not be below the nonzero entries
 * The positions are inst_pos verbatim: the handle takes the build's array instead of copying it, and inst_doc is freed once
 * the postings exist.  The build is then CONSUMED: np_hip_text_build_sizes and the vocabulary half of np_hip_text_build_fetch
 * (term_bytes, term_byte_offsets) still serve it and np_hip_text_build_free frees it; the instance half of _fetch, a second
 * install and a merge that takes it as its batch are refused by name.  A build that np_hip_text_build_sizes merged on the host
 * (fallback documents) is uploaded first.  The new index is built beside the old one and swapped in whole: a refused call, and
 * NP_ERR_OUT_OF_MEMORY, leave the handle AND the build as they were.  The peak device bytes depend on the sizes alone:
 * np_hip_index_set_text_build_bytes(n_terms, n_instances, n_docs of the handle), the build's own arrays included.  A build
 * without instances and rows drops the handle's keyword index, as np_hip_index_set_text does.
 * The call takes the handle as np_hip_index_append does: searches that run finish on the old keyword index, later ones see
 * the new one, and the caller needs no lock of its own (np_hip_index_set_text does).
 * NP_ERR_INVALID_ARGUMENT, by name: a NULL index or build, a build that is not finalised, lies on another device or is
 * consumed, a handle opened with shard_count > 1 (a slice needs the whole table's document frequencies:
 * np_hip_index_set_text_shard), an instance that fails the checks, n_rows below the documents that hold a token (a backstop: no build the library
 * makes can meet it -- np_hip_text_build's n_rows is its document count and the merges check n_rows_out first -- so no test
 * reaches it).  The call also compares what it held with np_hip_index_set_text_build_bytes and fails if the plan was exceeded.
 *
 * np_hip_index_text_merge is np_hip_text_build_merge whose base A is the handle's keyword index, read where it lies: the
 * result is a finalised device build, byte-equal to that call's on the fetched base, and every rule of remap, delta_ids and
 * n_rows_out holds.  The handle is not modified (the call registers like a search: an append or an install waits for it).
 * The base is not uploaded and not checked instance by instance again -- it was when it was installed.  Its term_offsets and
 * inst_doc are regenerated from the postings into the call's workspace by one launch (term_offsets[k] = the first position
 * of term k's first posting; an instance's document = that of the last posting that starts at or before it), pos_A is the
 * handle's array, and the merge's kernels run unchanged.  Where n_rows_out is below survivors plus batch, the survivors that
 * hold a token are counted from the documents' lengths and remap by one reduction on the device.  base_term_bytes /
 * base_term_byte_offsets are the handle's vocabulary: exactly its n_terms strings (the host mirrors, which hold the arrays,
 * refuse another length).  Documents of the handle at or behind n_remap must hold no token.  report->ms_upload covers the
 * maps, the regenerating launch and the two counts over the handle's documents where they run; report->workspace_bytes is the planned need, np_hip_text_build_merge's without pos_A
 * plus the reduction's flags.  Refusals: np_hip_text_build_merge's, a handle without a keyword index, a sharded handle.
 *
 * np_hip_index_text_sizes, np_hip_index_get_text and np_hip_index_get_text_layout read the handle's keyword index back, as
 * np_hip_index_get_column does a column: the sizes; the table regenerated from HBM (term_offsets [n_terms + 1], inst_doc /
 * inst_pos [n_instances]); the layout as it lies (post_off [n_terms + 1], post_doc / post_tf / post_first [n_postings],
 * doc_len [n_docs]).  Any pointer may be NULL.  Unsharded handles with a keyword index only. */
int np_hip_index_set_text_build(np_index* index, np_text_build* build);
int64_t np_hip_index_set_text_build_bytes(int64_t n_terms, int64_t n_instances, int64_t n_docs);
int np_hip_index_text_merge(const np_index* index, const uint8_t* base_term_bytes, const int64_t* base_term_byte_offsets,
                            const int64_t* remap, int64_t n_remap, const np_text_build* delta /* finalised; NULL = empty batch */,
                            const int64_t* delta_ids, int64_t n_rows_out, const np_text_merge_opts* opts /* nullable */,
                            np_text_build** out_build, np_text_merge_report* report /* nullable */);
int np_hip_index_text_sizes(const np_index* index, int64_t* n_terms, int64_t* n_postings, int64_t* n_instances, int64_t* n_rows,
                            int64_t* n_docs);
int np_hip_index_get_text(const np_index* index, int64_t* term_offsets, int64_t* inst_doc, int32_t* inst_pos);
int np_hip_index_get_text_layout(const np_index* index, int64_t* post_off, int32_t* post_doc, int32_t* post_tf,
                                 int64_t* post_first, int32_t* doc_len);

/* Stage-level debug access for parity tests: runs S1-S5 for ONE query and copies out the probed
 * cells (ascending), candidate doc ids (ascending, global), their approximate scores, and the
 * selected docs in approx-rank order with their exact scores.  Capacities are in elements;
 * counts are returned in n_*.  Any pointer may be NULL. */
int np_hip_debug_trace(const np_index* index, const float* query, int32_t n_tokens, int32_t dim,
                       const np_search_params* params, const int64_t* subset, int64_t subset_len,
                       int64_t* cells, int64_t cap_cells, int64_t* n_cells,
                       int64_t* cand, float* approx, int64_t cap_cand, int64_t* n_cand,
                       int64_t* sel, float* sel_exact, int64_t cap_sel, int64_t* n_sel);

#ifdef __cplusplus
}
#endif
#endif /* NEXTPLAID_HIP_H */
