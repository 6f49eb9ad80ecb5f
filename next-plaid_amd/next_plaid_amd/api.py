"""Host-side mirror of the next-plaid crate's search API over the C ABI (include/nextplaid_hip.h).

Names, argument meaning and error behaviour follow the reference:
  MmapIndex.load / search / search_batch / accessors  -> next-plaid/src/index.rs:1026-1312
  SearchParameters / QueryResult                       -> next-plaid/src/search.rs:26-80
  error classes                                        -> next-plaid/src/error.rs:9-66
There is NO CPU fallback here: a missing library or GPU raises (DeviceUnavailableError); the
Rust wrapper is where a CPU fallback would live.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(os.path.dirname(_PKG), "csrc", "libnextplaid_hip.so")


def library_path() -> str:
    return os.environ.get("NEXTPLAID_HIP_LIB", _LIB)


# ---- errors (error.rs) ------------------------------------------------------------------------

class NextPlaidError(RuntimeError):
    pass


class IndexLoadError(NextPlaidError):
    """Error::IndexLoad"""


class SearchError(NextPlaidError):
    """Error::Search"""


class ShapeError(NextPlaidError):
    """Error::Shape"""


class CodecError(NextPlaidError):
    """Error::Codec"""


class IoError(NextPlaidError):
    """Error::Io / Error::Json"""


class DeviceUnavailableError(NextPlaidError):
    """No usable gfx950 device or the HIP library is missing."""


class IndexCreationError(NextPlaidError):
    """Error::IndexCreation"""


_ERR = {1: IndexLoadError, 2: SearchError, 3: ShapeError, 4: CodecError, 5: IoError,
        6: DeviceUnavailableError, 7: MemoryError, 8: ValueError, 9: IndexCreationError}


# ---- C structs -----------------------------------------------------------------------------------

class np_open_opts(C.Structure):
    _fields_ = [("device", C.c_int32), ("shard_rank", C.c_int32), ("shard_count", C.c_int32),
                ("n_contexts", C.c_int32), ("max_batch", C.c_int32), ("max_query_tokens", C.c_int32),
                ("workspace_bytes", C.c_int64)]


class np_search_params(C.Structure):
    _fields_ = [("top_k", C.c_int32), ("n_full_scores", C.c_int32), ("n_ivf_probe", C.c_int32),
                ("centroid_batch_size", C.c_int32), ("centroid_score_threshold", C.c_float),
                ("has_threshold", C.c_int32), ("precision", C.c_int32)]


class np_info(C.Structure):
    _fields_ = [("num_documents", C.c_int64), ("num_embeddings", C.c_int64), ("num_partitions", C.c_int64),
                ("embedding_dim", C.c_int32), ("nbits", C.c_int32), ("avg_doclen", C.c_double),
                ("shard_doc_begin", C.c_int64), ("shard_doc_end", C.c_int64), ("shard_embeddings", C.c_int64),
                ("device_bytes", C.c_int64), ("device", C.c_int32), ("abi_version", C.c_int32),
                ("workspace_bytes", C.c_int64)]


class np_stats(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_centroid", C.c_float), ("ms_probe", C.c_float),
                ("ms_candidates", C.c_float), ("ms_approx", C.c_float), ("ms_select", C.c_float),
                ("ms_exact", C.c_float), ("ms_topk", C.c_float),
                ("n_cells", C.c_int64), ("n_ivf_ids", C.c_int64), ("n_candidates", C.c_int64),
                ("n_cand_tokens", C.c_int64), ("n_exact_docs", C.c_int64), ("n_exact_tokens", C.c_int64),
                ("n_cand_codes", C.c_int64), ("n_queries", C.c_int32), ("n_rounds", C.c_int32),
                ("n_survivors", C.c_int64), ("n_cand_dcodes", C.c_int64), ("n_level2", C.c_int64),
                ("ms_hot_level", C.c_float), ("reserved0", C.c_int32), ("n_level0", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class np_index_arrays(C.Structure):
    _fields_ = [("num_documents_total", C.c_int64), ("doc_begin", C.c_int64), ("num_docs", C.c_int64),
                ("num_centroids", C.c_int64), ("dim", C.c_int32), ("nbits", C.c_int32),
                ("centroids", C.c_void_p), ("bucket_weights", C.c_void_p), ("ivf", C.c_void_p),
                ("ivf_lengths", C.c_void_p), ("doc_lengths", C.c_void_p), ("codes", C.c_void_p),
                ("residuals", C.c_void_p)]


class np_write_opts(C.Structure):
    _fields_ = [("chunk_docs", C.c_int64), ("bucket_cutoffs", C.c_void_p), ("avg_residual", C.c_void_p),
                ("cluster_threshold", C.c_float)]


class np_synth_spec(C.Structure):
    _fields_ = [("num_docs", C.c_int64), ("num_centroids", C.c_int64), ("dim", C.c_int32), ("nbits", C.c_int32),
                ("doc_len_min", C.c_int32), ("doc_len_max", C.c_int32), ("n_topics", C.c_int32),
                ("rand256", C.c_int32), ("seed", C.c_uint64), ("centroids", C.c_void_p),
                ("bucket_weights", C.c_void_p), ("len_table", C.c_void_p), ("len_table_size", C.c_int32)]


class np_kmeans_opts(C.Structure):
    _fields_ = [("k", C.c_int64), ("max_points_per_centroid", C.c_int64), ("seed", C.c_uint64), ("tol", C.c_double),
                ("max_iters", C.c_int32), ("reserved0", C.c_int32)]


class np_kmeans_report(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("reserved0", C.c_int32), ("shift", C.c_double), ("n_points", C.c_int64),
                ("n_reinit", C.c_int64), ("ms_assign", C.c_double), ("ms_update", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class np_index_config(C.Structure):
    _fields_ = [("nbits", C.c_int32), ("kmeans_niters", C.c_int32), ("batch_size", C.c_int64), ("seed", C.c_uint64),
                ("max_points_per_centroid", C.c_int64), ("n_samples_kmeans", C.c_int64), ("num_partitions", C.c_int64),
                ("start_from_scratch", C.c_int64)]


class np_kmeans_plan(C.Structure):
    _fields_ = [("n_samples", C.c_int64), ("sample_tokens", C.c_int64), ("num_partitions", C.c_int64), ("k", C.c_int64),
                ("codec_samples", C.c_int64), ("heldout_size", C.c_int64), ("heldout_tokens", C.c_int64)]


class np_update_config(C.Structure):
    _fields_ = [("batch_size", C.c_int64), ("kmeans_niters", C.c_int32), ("reserved0", C.c_int32),
                ("max_points_per_centroid", C.c_int64), ("n_samples_kmeans", C.c_int64), ("seed", C.c_uint64),
                ("start_from_scratch", C.c_int64), ("buffer_size", C.c_int64), ("reserved", C.c_int64 * 4)]


class np_update_report(C.Structure):
    _fields_ = [("mode", C.c_int32), ("reserved0", C.c_int32), ("first_doc_id", C.c_int64), ("n_outliers", C.c_int64),
                ("n_rechecked", C.c_int64), ("n_new_centroids", C.c_int64), ("n_reindexed", C.c_int64),
                ("ms_encode", C.c_double), ("ms_outliers", C.c_double), ("ms_kmeans", C.c_double), ("ms_files", C.c_double),
                ("reserved", C.c_int64 * 4)]

    MODES = {0: "none", 1: "start_from_scratch", 2: "buffer", 3: "expansion", 4: "append"}

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}
        d["mode"] = self.MODES.get(self.mode, str(self.mode))
        return d


class np_pool_opts(C.Structure):
    _fields_ = [("pool_factor", C.c_int32), ("protected_tokens", C.c_int32), ("cut_order", C.c_int32), ("reserved0", C.c_int32),
                ("chunk_docs", C.c_int64), ("reserved", C.c_int64 * 3)]


class np_pool_report(C.Structure):
    _fields_ = [("n_docs", C.c_int64), ("n_pooled", C.c_int64), ("tokens_in", C.c_int64), ("tokens_out", C.c_int64),
                ("ms_distances", C.c_double), ("ms_linkage", C.c_double), ("ms_means", C.c_double), ("n_chunks", C.c_int64),
                ("reserved", C.c_int64 * 3)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class np_column(C.Structure):
    _fields_ = [("type", C.c_int32), ("reserved", C.c_int32), ("data", C.c_void_p), ("valid", C.c_void_p)]


class np_filter_op(C.Structure):
    _fields_ = [("op", C.c_int32), ("column", C.c_int32), ("arg", C.c_int32), ("n_values", C.c_int32),
                ("first_value", C.c_int64)]


class np_filter(C.Structure):
    _fields_ = [("ops", C.POINTER(np_filter_op)), ("n_ops", C.c_int32), ("values", C.c_void_p), ("n_values", C.c_int64)]


class np_dfa(C.Structure):
    _fields_ = [("words", C.c_void_p), ("n_words", C.c_int64)]


class np_match_report(C.Structure):
    _fields_ = [("tile_bytes", C.c_int32), ("table_lds_bytes", C.c_int32), ("n_lds", C.c_int32), ("n_global", C.c_int32),
                ("n_chunks", C.c_int32), ("reserved", C.c_int32), ("bytes_scanned", C.c_int64), ("ms", C.c_float),
                ("reserved2", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class np_text_index(C.Structure):
    _fields_ = [("n_terms", C.c_int64), ("term_offsets", C.c_void_p), ("inst_doc", C.c_void_p), ("inst_pos", C.c_void_p),
                ("n_rows", C.c_int64)]


class np_text_build_opts(C.Structure):
    _fields_ = [("tokenizer", C.c_int32), ("max_token_bytes", C.c_int32), ("workspace_bytes", C.c_int64),
                ("hash_bits", C.c_int32), ("tile_bytes", C.c_int32), ("unicode_table", C.c_void_p),
                ("unicode_table_len", C.c_int64), ("reserved", C.c_int64 * 1)]


class np_text_build_report(C.Structure):
    _fields_ = [("n_docs", C.c_int64), ("n_fallback", C.c_int64), ("n_instances", C.c_int64), ("n_terms", C.c_int64),
                ("term_bytes", C.c_int64), ("table_retries", C.c_int32), ("sort_passes", C.c_int32), ("hash_bits", C.c_int32),
                ("tile_bytes", C.c_int32), ("ms_upload", C.c_double), ("ms_classify", C.c_double), ("ms_emit", C.c_double),
                ("ms_terms", C.c_double), ("ms_sort", C.c_double), ("ms_total", C.c_double), ("workspace_bytes", C.c_int64),
                ("reserved", C.c_int64 * 3)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class np_text_merge_opts(C.Structure):
    _fields_ = [("workspace_bytes", C.c_int64), ("reserved", C.c_int64 * 3)]


class np_text_merge_report(C.Structure):
    _fields_ = [("n_base_terms", C.c_int64), ("n_base_instances", C.c_int64), ("n_old_docs", C.c_int64),
                ("n_survivors", C.c_int64), ("n_delta_docs", C.c_int64), ("n_delta_terms", C.c_int64),
                ("n_delta_instances", C.c_int64), ("n_terms", C.c_int64), ("n_instances", C.c_int64), ("n_rows", C.c_int64),
                ("n_terms_dropped", C.c_int64), ("n_instances_dropped", C.c_int64), ("delta_uploaded", C.c_int32),
                ("reserved0", C.c_int32), ("ms_check", C.c_double), ("ms_upload", C.c_double), ("ms_count", C.c_double),
                ("ms_terms", C.c_double), ("ms_place", C.c_double), ("ms_total", C.c_double), ("workspace_bytes", C.c_int64),
                ("reserved", C.c_int64 * 3)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


NP_TOK_UNICODE61, NP_TOK_TRIGRAM = 0, 1


class np_text_query(C.Structure):
    _fields_ = [("terms", C.c_void_p), ("phrase_offsets", C.c_void_p), ("n_phrases", C.c_int32), ("mode", C.c_int32)]


class np_text_node(C.Structure):
    _fields_ = [("op", C.c_int32), ("a", C.c_int32), ("b", C.c_int32)]


class np_text_expr(C.Structure):
    _fields_ = [("terms", C.c_void_p), ("phrase_offsets", C.c_void_p), ("prefix_hi", C.c_void_p), ("nodes", C.c_void_p),
                ("n_phrases", C.c_int32), ("n_nodes", C.c_int32)]


# np_all_gather_host_fn: int (*)(void* ctx, const void* send, void* recv, int64_t bytes)
ALL_GATHER_HOST_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)
NP_COMM_DEFERRED_STATUS = 1

NP_ABI_VERSION = 6     # include/nextplaid_hip.h this mirror was written against

EXPORTS = [
    "np_hip_abi_version", "np_hip_struct_size", "np_hip_comm_info",
    "np_hip_device_count", "np_hip_last_error", "np_hip_index_open", "np_hip_index_from_arrays",
    "np_hip_index_synth", "np_hip_index_export", "np_hip_index_ivf_size", "np_hip_index_tune", "np_hip_index_close",
    "np_hip_index_info", "np_hip_index_probe_dir", "np_hip_index_write_dir", "np_hip_search_batch", "np_hip_search_batch_device", "np_hip_search_phase_a",
    "np_hip_search_phase_b", "np_hip_search_end", "np_hip_n_sel", "np_hip_select_cut", "np_hip_merge_topk",
    "np_hip_merge_packed", "np_hip_elig_words", "np_hip_subset_eligible", "np_hip_or_bitmaps",
    "np_hip_comm_unique_id", "np_hip_comm_create", "np_hip_comm_create_hosted", "np_hip_comm_status", "np_hip_comm_destroy",
    "np_hip_search_batch_sharded",
    "np_hip_search_batch_subsets", "np_hip_search_batch_subsets_device", "np_hip_search_phase_a_subsets",
    "np_hip_subsets_eligible", "np_hip_search_batch_sharded_subsets",
    "np_hip_decompress_documents", "np_hip_encode_tokens", "np_hip_rerank_maxsim", "np_hip_debug_trace",
    "np_hip_kmeans_plan", "np_hip_kmeans", "np_hip_compute_kmeans", "np_hip_prepare_codec_artifacts", "np_hip_index_create",
    "np_hip_index_update", "np_hip_index_update_append", "np_hip_index_delete",
    "np_hip_pooled_lengths", "np_hip_pool_documents",
    "np_hip_search_exact", "np_hip_search_exact_device",
    "np_hip_score_pairs", "np_hip_score_pairs_device",
    "np_hip_index_set_columns", "np_hip_filter_eval", "np_hip_search_batch_filtered", "np_hip_search_exact_filtered",
    "np_hip_index_set_text", "np_hip_text_search", "np_hip_text_search_device", "np_hip_text_search_filtered",
    "np_hip_fuse", "np_hip_fuse_device", "np_hip_search_hybrid",
    "np_hip_text_search_expr", "np_hip_text_search_expr_filtered", "np_hip_search_hybrid_expr",
    "np_hip_index_set_column_text", "np_hip_text_match",
    "np_hip_index_set_text_shard", "np_hip_text_search_sharded", "np_hip_text_search_sharded_filtered",
    "np_hip_search_batch_sharded_filtered", "np_hip_search_hybrid_sharded",
    "np_hip_text_search_expr_device", "np_hip_text_search_sharded_expr", "np_hip_text_search_sharded_expr_filtered",
    "np_hip_search_hybrid_sharded_expr",
    "np_hip_index_set_groups", "np_hip_index_group_count", "np_hip_collapse", "np_hip_collapse_device",
    "np_hip_search_batch_grouped", "np_hip_search_hybrid_grouped",
    "np_hip_text_build", "np_hip_text_build_fallback", "np_hip_text_build_add", "np_hip_text_build_sizes",
    "np_hip_text_build_fetch", "np_hip_text_build_free", "np_hip_text_build_merge",
    "np_hip_index_set_text_build", "np_hip_index_set_text_build_bytes", "np_hip_index_text_merge", "np_hip_index_text_sizes",
    "np_hip_index_get_text", "np_hip_index_get_text_layout",
    "np_hip_index_append", "np_hip_index_reserve", "np_hip_index_capacity", "np_hip_index_remove",
    "np_hip_index_remove_keep", "np_hip_index_append_rows", "np_hip_index_get_column", "np_hip_index_get_groups",
    "np_hip_index_expand", "np_hip_index_expand_rows",
]

_lib = None


def _preload_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  Two HIP runtimes cannot share a
    process: if libnextplaid_hip.so pulls in /opt/rocm's copy first, a later `import torch` loads the bundled one
    next to it and torch's device init fails ("no ROCm-capable device is detected").  So when torch is installed
    its runtime is loaded first (without importing torch); our NEEDED libamdhip64.so.7 then binds to that copy and
    torch reuses it.  Without torch (C++/Rust hosts, plain ctypes users) the system runtime is used."""
    if os.environ.get("NEXTPLAID_HIP_NO_TORCH_RUNTIME"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    hip = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(hip):
        try:
            C.CDLL(hip, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load libnextplaid_hip.so.  Raises DeviceUnavailableError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise DeviceUnavailableError(f"{path} not built (run python -c 'import __graft_entry__ as g; g.build()')")
    _preload_hip_runtime()
    try:
        L = C.CDLL(path)
    except OSError as e:  # e.g. libamdhip64 missing
        raise DeviceUnavailableError(f"cannot load {path}: {e}") from e
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    # ABI check before any caller-allocated struct crosses the boundary (np_info / np_stats have grown between versions)
    if not hasattr(L, "np_hip_abi_version"):
        raise DeviceUnavailableError(f"{path} predates ABI v6 (no np_hip_abi_version); this mirror needs v{NP_ABI_VERSION}: rebuild it")
    L.np_hip_abi_version.restype = C.c_int
    L.np_hip_struct_size.argtypes = [i32]
    L.np_hip_struct_size.restype = i64
    ver = int(L.np_hip_abi_version())
    if ver != NP_ABI_VERSION:
        raise DeviceUnavailableError(f"{path} speaks ABI v{ver}, this mirror v{NP_ABI_VERSION}: rebuild the library")
    for which, st in ((0, np_info), (1, np_stats), (2, np_search_params), (3, np_open_opts), (4, np_kmeans_opts),
                      (5, np_kmeans_report), (6, np_index_config), (7, np_kmeans_plan), (8, np_update_config),
                      (9, np_update_report), (10, np_pool_opts), (11, np_pool_report), (12, np_text_expr)):
        if int(L.np_hip_struct_size(which)) != C.sizeof(st):
            raise DeviceUnavailableError(f"{path}: sizeof({st.__name__}) is {int(L.np_hip_struct_size(which))} in the library, "
                                         f"{C.sizeof(st)} in this mirror")
    L.np_hip_device_count.restype = C.c_int
    L.np_hip_last_error.restype = C.c_char_p
    L.np_hip_index_open.argtypes = [C.c_char_p, C.POINTER(np_open_opts), C.POINTER(vp)]
    L.np_hip_index_from_arrays.argtypes = [C.POINTER(np_index_arrays), C.POINTER(np_open_opts), C.POINTER(vp)]
    L.np_hip_index_synth.argtypes = [C.POINTER(np_synth_spec), C.POINTER(np_open_opts), C.POINTER(vp)]
    L.np_hip_index_export.argtypes = [vp] * 6
    L.np_hip_index_ivf_size.argtypes = [vp]
    L.np_hip_index_ivf_size.restype = i64
    L.np_hip_index_tune.argtypes = [vp, C.c_char_p, i32]
    L.np_hip_index_close.argtypes = [vp]
    L.np_hip_index_close.restype = None
    L.np_hip_index_info.argtypes = [vp, C.POINTER(np_info)]
    L.np_hip_index_probe_dir.argtypes = [C.c_char_p, C.POINTER(np_info)]
    L.np_hip_index_write_dir.argtypes = [C.c_char_p, C.POINTER(np_index_arrays), C.POINTER(np_write_opts)]
    L.np_hip_search_batch.argtypes = [vp, vp, vp, i32, i32, C.POINTER(np_search_params), vp, i64, vp, vp, vp,
                                      C.POINTER(np_stats)]
    L.np_hip_search_batch_device.argtypes = [vp, vp, vp, vp, i32, i32, C.POINTER(np_search_params), vp, i64,
                                             vp, vp, vp, vp]
    L.np_hip_search_phase_a.argtypes = [vp, vp, vp, vp, i32, i32, C.POINTER(np_search_params), vp, i64, vp, vp, vp,
                                        C.POINTER(vp)]
    L.np_hip_elig_words.argtypes = [vp]
    L.np_hip_elig_words.restype = i64
    L.np_hip_subset_eligible.argtypes = [vp, vp, i64, vp, vp]
    L.np_hip_or_bitmaps.argtypes = [vp, vp, i32, i64, vp, vp]
    L.np_hip_merge_packed.argtypes = [vp, vp, i64, i64, i64, i64, i32, i32, i32, vp, vp, vp, vp]
    L.np_hip_comm_unique_id.argtypes = [vp]
    L.np_hip_comm_create.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
    L.np_hip_comm_create_hosted.argtypes = [vp, i32, i32, ALL_GATHER_HOST_FN, vp, i32, C.POINTER(vp)]
    L.np_hip_comm_status.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.np_hip_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.np_hip_comm_destroy.argtypes = [vp]
    L.np_hip_comm_destroy.restype = None
    L.np_hip_search_batch_sharded.argtypes = [vp, vp, vp, vp, vp, i32, i32, C.POINTER(np_search_params), vp, i64,
                                              vp, vp, vp, vp]
    L.np_hip_search_batch_subsets.argtypes = [vp, vp, vp, i32, i32, C.POINTER(np_search_params), vp, vp, i64, vp, vp, vp, vp,
                                              C.POINTER(np_stats)]
    L.np_hip_search_batch_subsets_device.argtypes = [vp, vp, vp, vp, i32, i32, C.POINTER(np_search_params), vp, vp, vp, i64,
                                                     vp, vp, vp, vp, vp]
    L.np_hip_search_phase_a_subsets.argtypes = [vp, vp, vp, vp, i32, i32, C.POINTER(np_search_params), vp, vp, vp, i64, vp,
                                                vp, vp, vp, C.POINTER(vp)]
    L.np_hip_subsets_eligible.argtypes = [vp, vp, vp, vp, i64, vp, vp]
    L.np_hip_search_batch_sharded_subsets.argtypes = [vp, vp, vp, vp, vp, i32, i32, C.POINTER(np_search_params), vp, vp, vp,
                                                      i64, vp, vp, vp, vp, vp]
    L.np_hip_search_exact.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, C.POINTER(np_stats)]
    L.np_hip_search_exact_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    L.np_hip_score_pairs.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, C.POINTER(np_stats)]
    L.np_hip_score_pairs_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.np_hip_index_set_columns.argtypes = [vp, C.POINTER(np_column), i32]
    L.np_hip_filter_eval.argtypes = [vp, C.POINTER(np_filter), i32, vp, i64, vp]
    L.np_hip_search_batch_filtered.argtypes = [vp, vp, vp, i32, i32, C.POINTER(np_search_params), C.POINTER(np_filter), i32, vp,
                                               vp, vp, vp, C.POINTER(np_stats)]
    L.np_hip_search_exact_filtered.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.POINTER(np_filter), i32, vp, vp, vp, vp,
                                               C.POINTER(np_stats)]
    L.np_hip_index_set_column_text.argtypes = [vp, i32, vp, vp, i64]
    L.np_hip_text_match.argtypes = [vp, i32, C.POINTER(np_dfa), i32, vp, C.POINTER(np_match_report)]
    L.np_hip_index_set_text.argtypes = [vp, C.POINTER(np_text_index)]
    L.np_hip_text_search.argtypes = [vp, C.POINTER(np_text_query), i32, i32, vp, vp, i64, vp, vp, vp, vp, C.POINTER(np_stats)]
    L.np_hip_text_search_device.argtypes = [vp, C.POINTER(np_text_query), i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    L.np_hip_text_search_filtered.argtypes = [vp, C.POINTER(np_text_query), i32, i32, C.POINTER(np_filter), i32, vp, vp, vp, vp,
                                              C.POINTER(np_stats)]
    L.np_hip_fuse.argtypes = [vp, i32, C.c_float, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp]
    L.np_hip_fuse_device.argtypes = [vp, i32, C.c_float, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    L.np_hip_search_hybrid.argtypes = [vp, vp, vp, i32, i32, C.POINTER(np_search_params), C.POINTER(np_text_query), i32,
                                       C.c_float, i32, vp, vp, i64, vp, C.POINTER(np_filter), i32, vp, vp, vp,
                                       C.POINTER(np_stats)]
    L.np_hip_text_search_expr.argtypes = [vp, C.POINTER(np_text_expr), i32, i32, vp, vp, i64, vp, vp, vp, vp, C.POINTER(np_stats)]
    L.np_hip_text_search_expr_filtered.argtypes = [vp, C.POINTER(np_text_expr), i32, i32, C.POINTER(np_filter), i32, vp, vp, vp,
                                                   vp, C.POINTER(np_stats)]
    L.np_hip_search_hybrid_expr.argtypes = [vp, vp, vp, i32, i32, C.POINTER(np_search_params), C.POINTER(np_text_expr), i32,
                                            C.c_float, i32, vp, vp, i64, vp, C.POINTER(np_filter), i32, vp, vp, vp,
                                            C.POINTER(np_stats)]
    L.np_hip_index_set_text_shard.argtypes = [vp, C.POINTER(np_text_index)]
    L.np_hip_text_search_sharded.argtypes = [vp, vp, C.POINTER(np_text_query), i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    L.np_hip_text_search_sharded_filtered.argtypes = [vp, vp, C.POINTER(np_text_query), i32, i32, C.POINTER(np_filter), i32, vp,
                                                      vp, vp, vp, vp]
    L.np_hip_search_batch_sharded_filtered.argtypes = [vp, vp, vp, vp, vp, i32, i32, C.POINTER(np_search_params),
                                                       C.POINTER(np_filter), i32, vp, vp, vp, vp, vp]
    L.np_hip_search_hybrid_sharded.argtypes = [vp, vp, vp, vp, vp, i32, i32, C.POINTER(np_search_params),
                                               C.POINTER(np_text_query), i32, C.c_float, i32, vp, vp, vp, i64, vp,
                                               C.POINTER(np_filter), i32, vp, vp, vp, vp, vp]
    L.np_hip_text_search_expr_device.argtypes = [vp, C.POINTER(np_text_expr), i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    L.np_hip_text_search_sharded_expr.argtypes = [vp, vp, C.POINTER(np_text_expr), i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    L.np_hip_text_search_sharded_expr_filtered.argtypes = [vp, vp, C.POINTER(np_text_expr), i32, i32, C.POINTER(np_filter), i32,
                                                           vp, vp, vp, vp, vp]
    L.np_hip_search_hybrid_sharded_expr.argtypes = [vp, vp, vp, vp, vp, i32, i32, C.POINTER(np_search_params),
                                                    C.POINTER(np_text_expr), i32, C.c_float, i32, vp, vp, vp, i64, vp,
                                                    C.POINTER(np_filter), i32, vp, vp, vp, vp, vp]
    L.np_hip_index_set_groups.argtypes = [vp, vp, i64, i64]
    L.np_hip_index_group_count.argtypes = [vp]
    L.np_hip_index_group_count.restype = i64
    L.np_hip_collapse.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.np_hip_collapse_device.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.np_hip_search_batch_grouped.argtypes = [vp, vp, vp, i32, i32, C.POINTER(np_search_params), vp, vp, i64, vp,
                                              C.POINTER(np_filter), i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(np_stats)]
    L.np_hip_search_hybrid_grouped.argtypes = [vp, vp, vp, i32, i32, C.POINTER(np_search_params), C.POINTER(np_text_query), i32,
                                               C.c_float, i32, vp, vp, i64, vp, C.POINTER(np_filter), i32, i32, i32,
                                               vp, vp, vp, vp, vp, vp, C.POINTER(np_stats)]
    L.np_hip_search_phase_b.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.np_hip_search_end.argtypes = [vp, vp]
    L.np_hip_search_end.restype = None
    L.np_hip_n_sel.argtypes = [C.POINTER(np_search_params)]
    L.np_hip_n_sel.restype = i32
    L.np_hip_select_cut.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    L.np_hip_merge_topk.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.np_hip_decompress_documents.argtypes = [vp, vp, i64, vp, i64, vp]
    L.np_hip_encode_tokens.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    L.np_hip_rerank_maxsim.argtypes = [i32, vp, i32, i32, vp, vp, i64, vp, vp]
    L.np_hip_debug_trace.argtypes = [vp, vp, i32, i32, C.POINTER(np_search_params), vp, i64,
                                     vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp]
    L.np_hip_kmeans_plan.argtypes = [vp, i64, C.POINTER(np_index_config), C.POINTER(np_kmeans_plan), vp]
    L.np_hip_kmeans.argtypes = [i32, vp, i64, i32, C.POINTER(np_kmeans_opts), vp, vp, vp, C.POINTER(np_kmeans_report)]
    L.np_hip_compute_kmeans.argtypes = [i32, vp, vp, i64, i32, C.POINTER(np_index_config), vp, i64, C.POINTER(i64),
                                        C.POINTER(np_kmeans_report)]
    L.np_hip_prepare_codec_artifacts.argtypes = [i32, vp, vp, i64, i32, vp, i64, C.POINTER(np_index_config), vp, vp, vp, vp]
    L.np_hip_index_create.argtypes = [C.c_char_p, vp, vp, i64, i32, C.POINTER(np_index_config), C.POINTER(np_open_opts),
                                      C.POINTER(vp)]
    for f in (L.np_hip_index_update, L.np_hip_index_update_append):
        f.argtypes = [C.c_char_p, vp, vp, i64, i32, C.POINTER(np_update_config), i32, C.POINTER(np_update_report)]
    L.np_hip_index_delete.argtypes = [C.c_char_p, vp, i64, C.POINTER(i64)]
    L.np_hip_index_append.argtypes = [vp, vp, i64, vp, vp]
    L.np_hip_index_remove.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.np_hip_index_remove_keep.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.np_hip_index_append_rows.argtypes = [vp, vp, i64, vp, vp, C.POINTER(np_column), i32, vp, vp, i64]
    L.np_hip_index_expand.argtypes = [vp, vp, i64, i64, vp, i64, vp, vp]
    L.np_hip_index_expand_rows.argtypes = [vp, vp, i64, i64, vp, i64, vp, vp, C.POINTER(np_column), i32, vp, vp, i64]
    L.np_hip_index_get_column.argtypes =[vp, i32, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    L.np_hip_index_get_groups.argtypes = [vp, vp]
    L.np_hip_index_reserve.argtypes = [vp, i64, i64]
    L.np_hip_index_capacity.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.np_hip_pooled_lengths.argtypes = [vp, i64, C.POINTER(np_pool_opts), vp]
    L.np_hip_pool_documents.argtypes = [i32, vp, vp, i64, i32, C.POINTER(np_pool_opts), vp, i64, vp, vp, vp,
                                        C.POINTER(np_pool_report)]
    L.np_hip_text_build.argtypes = [i32, vp, vp, i64, C.POINTER(np_text_build_opts), C.POINTER(vp),
                                    C.POINTER(np_text_build_report)]
    L.np_hip_text_build_fallback.argtypes = [vp, vp, C.POINTER(i64)]
    L.np_hip_text_build_add.argtypes = [vp, vp, vp, i64, vp, vp, vp, i64]
    L.np_hip_text_build_sizes.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.np_hip_text_build_fetch.argtypes = [vp, vp, vp, vp, vp, vp]
    L.np_hip_text_build_free.argtypes = [vp]
    L.np_hip_text_build_free.restype = None
    L.np_hip_text_build_merge.argtypes = [i32, C.POINTER(np_text_index), vp, vp, vp, i64, vp, vp, i64,
                                          C.POINTER(np_text_merge_opts), C.POINTER(vp), C.POINTER(np_text_merge_report)]
    L.np_hip_index_set_text_build.argtypes = [vp, vp]
    L.np_hip_index_set_text_build_bytes.argtypes = [i64, i64, i64]
    L.np_hip_index_set_text_build_bytes.restype = i64
    L.np_hip_index_text_merge.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64, C.POINTER(np_text_merge_opts), C.POINTER(vp),
                                          C.POINTER(np_text_merge_report)]
    L.np_hip_index_text_sizes.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.np_hip_index_get_text.argtypes = [vp, vp, vp, vp]
    L.np_hip_index_get_text_layout.argtypes = [vp, vp, vp, vp, vp, vp]
    _lib = L
    return L


def last_error() -> str:
    return lib().np_hip_last_error().decode("utf-8", "replace")


def _check(rc: int, msg: str | None = None):
    if rc:
        msg = last_error() if msg is None else msg
        raise _ERR.get(rc, NextPlaidError)(msg or f"np_status {rc}")


def probe_index_dir(path: str) -> np_info:
    """Host-only parse + validation of an index directory (same checks and errors as MmapIndex.load; no GPU)."""
    info = np_info()
    _check(lib().np_hip_index_probe_dir(os.fsencode(path), C.byref(info)))
    return info


def write_index_dir(path: str, centroids, bucket_weights, doc_lengths, codes, residuals, nbits, ivf=None, ivf_lengths=None,
                    bucket_cutoffs=None, avg_residual=None, cluster_threshold: float = 0.0, chunk_docs: int = 50000):
    """write_index_from_encoded_chunks (index.rs:373-528): host arrays -> an index directory in the crate's on-disk
    format (host only).  Without ivf / ivf_lengths the posting lists are built from the codes (index.rs:479-504)."""
    cen = np.ascontiguousarray(centroids, np.float32)
    if cen.ndim != 2:
        raise ShapeError("centroids must be [K, dim]")
    w = np.ascontiguousarray(bucket_weights, np.float32)
    dl = np.ascontiguousarray(doc_lengths, np.int64)
    cd = np.ascontiguousarray(codes, np.int64)
    rs = np.ascontiguousarray(residuals, np.uint8)
    pd = cen.shape[1] * int(nbits) // 8
    if w.size != (1 << int(nbits)):
        raise CodecError(f"Codec error: bucket_weights has {w.size} entries, nbits={nbits} needs {1 << int(nbits)}")
    if cd.size != int(dl.sum()) or rs.size != cd.size * pd:
        raise ShapeError(f"Shape error: {cd.size} codes / {rs.size} residual bytes for {int(dl.sum())} tokens of {pd} bytes")
    iv = None if ivf is None else np.ascontiguousarray(ivf, np.int64)
    il = None if ivf_lengths is None else np.ascontiguousarray(ivf_lengths, np.int32)
    cut = None if bucket_cutoffs is None else np.ascontiguousarray(bucket_cutoffs, np.float32)
    avg = None if avg_residual is None else np.ascontiguousarray(avg_residual, np.float32)
    if cut is not None and cut.size != (1 << int(nbits)) - 1:
        raise CodecError(f"Codec error: bucket_cutoffs has {cut.size} entries, nbits={nbits} needs {(1 << int(nbits)) - 1}")
    if avg is not None and avg.size != cen.shape[1]:
        raise ShapeError("avg_residual must have dim entries")
    a = np_index_arrays(dl.size, 0, dl.size, cen.shape[0], cen.shape[1], int(nbits), _ptr(cen), _ptr(w),
                        None if iv is None else _ptr(iv), None if il is None else _ptr(il), _ptr(dl), _ptr(cd), _ptr(rs))
    o = np_write_opts(int(chunk_docs), None if cut is None else _ptr(cut), None if avg is None else _ptr(avg),
                      float(cluster_threshold))
    _check(lib().np_hip_index_write_dir(path.encode(), C.byref(a), C.byref(o)))


def rerank_maxsim(query, documents, device: int = 0):
    """/rerank (next-plaid-api handlers/rerank.rs:57-170): MaxSim of one query against caller-supplied document
    embeddings.  Returns (order, scores): document indices by descending score (stable) and the scores in INPUT
    order.  ValueError carries the handler's BadRequest messages."""
    q = np.ascontiguousarray(query, np.float32)
    docs = [np.ascontiguousarray(d, np.float32) for d in documents]
    if q.ndim != 2:
        raise ShapeError(f"Shape error: query has shape {q.shape}")
    for d in docs:
        if d.ndim != 2 or d.shape[1] != q.shape[1]:   # ApiError::DimensionMismatch (rerank.rs:141-146)
            raise ShapeError(f"Shape error: expected dim {q.shape[1]}, got {d.shape}")
    off = np.zeros(len(docs) + 1, np.int64)
    if docs:
        off[1:] = np.cumsum([d.shape[0] for d in docs])
    flat = np.concatenate(docs, 0) if docs and off[-1] > 0 else np.zeros((1, max(q.shape[1], 1)), np.float32)
    scores = np.zeros(max(len(docs), 1), np.float32)
    order = np.zeros(max(len(docs), 1), np.int64)
    _check(lib().np_hip_rerank_maxsim(int(device), _ptr(q), q.shape[0], q.shape[1], _ptr(flat), _ptr(off), len(docs),
                                      _ptr(scores), _ptr(order)))
    return order[: len(docs)], scores[: len(docs)]


def device_count() -> int:
    try:
        return int(lib().np_hip_device_count())
    except DeviceUnavailableError:
        return 0


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pack_subsets(subsets, n_queries: int):
    """One subset per query -> the CSR arguments of np_hip_search_batch_subsets: (subset_ids i64, subset_offsets i64
    [n_subsets + 1], query_subset i32 [n_queries], -1 = none).  `subsets` has n_queries entries, each None or an array of
    document ids.  Entries that are the SAME OBJECT share one subset (by identity; contents are never compared or hashed),
    so a server passes one array object per distinct filter and the device builds that filter's bitmaps once.  Pure host
    code: no device, no library."""
    subsets = list(subsets)
    if len(subsets) != n_queries:
        raise ValueError(f"subsets has {len(subsets)} entries for {n_queries} queries")
    slot, arrays = {}, []
    qsub = np.full(n_queries, -1, np.int32)
    for i, sub in enumerate(subsets):   # (every entry stays alive in `subsets`: an id() names one object throughout)
        if sub is None:
            continue
        j = slot.get(id(sub))
        if j is None:
            j = slot[id(sub)] = len(arrays)
            arrays.append(np.ascontiguousarray(sub, np.int64).reshape(-1))
        qsub[i] = j
    off = np.zeros(len(arrays) + 1, np.int64)
    if arrays:
        off[1:] = np.cumsum([a.size for a in arrays])
    ids = np.concatenate(arrays) if arrays else np.zeros(0, np.int64)
    return np.ascontiguousarray(ids, np.int64), off, qsub


def _compiled(f, schema):
    """A filter as callers give it -- a (condition, params) pair, a bare condition string or a CompiledFilter -- compiled."""
    from . import filters as F
    if isinstance(f, F.CompiledFilter):
        return f
    cond, params = (f, ()) if isinstance(f, str) else f
    return F.compile_filter(cond, params, schema)


def pack_filters(filters, n_queries: int, schema):
    """One filter per query -> (compiled distinct filters, query_filter i32 [n_queries], -1 = none).  `filters` has n_queries
    entries, each None, a (condition, params) pair, a bare condition string or a CompiledFilter.  Entries that compile to the
    same program share one filter: it is evaluated once.  Pure host code."""
    filters = list(filters)
    if len(filters) != n_queries:
        raise ValueError(f"filters has {len(filters)} entries for {n_queries} queries")
    slot, progs = {}, []
    qf = np.full(n_queries, -1, np.int32)
    for i, f in enumerate(filters):
        if f is None:
            continue
        f = _compiled(f, schema)
        j = slot.get(f.key())
        if j is None:
            j = slot[f.key()] = len(progs)
            progs.append(f)
        qf[i] = j
    return progs, qf


class _CFilters:
    """The ctypes form of compiled filters; keeps every array it points to alive."""

    def __init__(self, progs):
        self.n = len(progs)
        self.arr = (np_filter * max(self.n, 1))()
        self.keep = []
        for j, p in enumerate(progs):
            ops = (np_filter_op * max(len(p.ops), 1))(*[np_filter_op(*o) for o in p.ops])
            vals = np.ascontiguousarray(p.values, np.int64)
            self.keep += [ops, vals]
            self.arr[j] = np_filter(C.cast(ops, C.POINTER(np_filter_op)), len(p.ops), vals.ctypes.data if vals.size else None,
                                    vals.size)


class _CTextQueries:
    """The ctypes form of compiled keyword queries (text.TextQuery); keeps every array it points to alive."""

    def __init__(self, queries):
        self.n = len(queries)
        self.arr = (np_text_query * max(self.n, 1))()
        self.keep = []
        for j, q in enumerate(queries):
            if not hasattr(q, "mode"):
                raise ValueError("a tree query (text.TextExpr) where only flat keyword queries are taken: the grouped searches "
                                 "have no _expr form yet")
            terms = np.ascontiguousarray(q.terms, np.int32).reshape(-1)
            off = np.ascontiguousarray(q.phrase_offsets, np.int32).reshape(-1)
            self.keep += [terms, off]
            self.arr[j] = np_text_query(terms.ctypes.data if terms.size else None, off.ctypes.data if off.size else None,
                                        max(off.size - 1, 0), int(q.mode))


class _CTextExprs:
    """The ctypes form of tree queries (text.TextExpr; a flat text.TextQuery is lifted to a chain of ANDs or ORs); keeps
    every array it points to alive."""

    def __init__(self, queries):
        from . import text as T
        self.n = len(queries)
        self.arr = (np_text_expr * max(self.n, 1))()
        self.keep = []
        for j, q in enumerate(queries):
            if not isinstance(q, T.TextExpr):
                q = T.TextExpr.from_query(q)
            terms = np.ascontiguousarray(q.terms, np.int32).reshape(-1)
            off = np.ascontiguousarray(q.phrase_offsets, np.int32).reshape(-1)
            hi = np.ascontiguousarray(q.prefix_hi(), np.int32).reshape(-1)
            nodes = np.ascontiguousarray(q.nodes, np.int32).reshape(-1)
            self.keep += [terms, off, hi, nodes]
            self.arr[j] = np_text_expr(*(a.ctypes.data if a.size else None for a in (terms, off, hi, nodes)),
                                       max(off.size - 1, 0), nodes.size // 3)


def _c_text_queries(queries):
    """(the ctypes queries, "_expr" or ""): a batch that holds a text.TextExpr goes to the _expr entries as a whole."""
    from . import text as T
    if any(isinstance(q, T.TextExpr) for q in queries):
        return _CTextExprs(queries), "_expr"
    return _CTextQueries(queries), ""


def _pad_lists(lists, dtype, width=None):
    """Ragged per-query lists -> (flat [B * width] array, counts i32 [B], width)."""
    arrs = [np.asarray(a, dtype).reshape(-1) for a in lists]
    width = max([a.size for a in arrs] + [1]) if width is None else width
    flat = np.zeros((max(len(arrs), 1), width), dtype)
    for i, a in enumerate(arrs):
        flat[i, :a.size] = a
    return flat.reshape(-1), np.asarray([a.size for a in arrs], np.int32), width


def _fusion_mode(fusion) -> int:
    """"rrf" / "relative_score" (or the NP_FUSE_* value itself) -> the fusion argument of the entries"""
    from . import text as T
    return T.FUSION_MODES[fusion] if isinstance(fusion, str) else int(fusion)


def fuse(mode, alpha: float, top_k: int, sem_ids, sem_scores, kw_ids, kw_scores, index=None):
    """np_hip_fuse over a batch: per query a semantic and a keyword list (sequences of id / score arrays; the scores may be
    None for "rrf").  mode is "rrf" or "relative_score".  Returns per query (ids int64, scores float32).  `index` names the
    device (an MmapIndex; None = the current device)."""
    B = len(sem_ids)
    if len(kw_ids) != B:
        raise ValueError(f"{B} semantic lists and {len(kw_ids)} keyword lists")
    si, sc, sw = _pad_lists(sem_ids, np.int64)
    ki, kc, kw = _pad_lists(kw_ids, np.int64)
    ss = None if sem_scores is None else _pad_lists(sem_scores, np.float32, sw)[0]
    ks = None if kw_scores is None else _pad_lists(kw_scores, np.float32, kw)[0]
    rows = _ResultRows(B, max(int(top_k), 1))
    _check(lib().np_hip_fuse(None if index is None else index._h, _fusion_mode(mode), float(alpha), int(top_k), B, _ptr(si), _ptr(ss),
                             _ptr(sc), sw, _ptr(ki), _ptr(ks), _ptr(kc), kw, *rows.ptrs()))
    return [(r.passage_ids, r.scores) for r in rows.results()]


def fuse_rrf(sem_ids, kw_ids, alpha: float, top_k: int, index=None):
    """fuse_rrf (text_search.rs:1013-1033) with its argument order, batched: one list of ids per query on either side."""
    return fuse("rrf", alpha, top_k, sem_ids, None, kw_ids, None, index=index)


def fuse_relative_score(sem_ids, sem_scores, kw_ids, kw_scores, alpha: float, top_k: int, index=None):
    """fuse_relative_score (text_search.rs:1040-1075) with its argument order, batched."""
    return fuse("relative_score", alpha, top_k, sem_ids, sem_scores, kw_ids, kw_scores, index=index)


# ---- grouped search ------------------------------------------------------------------------------------
NP_GROUP_MAX_LIST = 16384


def group_ids_of_keys(keys):
    """One key per document (ints, strings or None) -> (dense group ids int32, the distinct non-null values sorted, n_groups).
    Group g < len(values) holds the documents whose key is values[g]; every None entry goes to ONE group with the last id
    (SQLite's GROUP BY puts all NULLs together).  Pure host code."""
    keys = keys.tolist() if isinstance(keys, np.ndarray) else list(keys)
    live = [k for k in keys if k is not None]
    for k in live:
        if isinstance(k, bool) or not isinstance(k, (int, str, np.integer)):
            raise ValueError(f"a group key must be an int, a string or None, not {type(k).__name__}")
    if len({isinstance(k, str) for k in live}) > 1:
        raise ValueError("group keys must be all ints or all strings (None aside)")
    values = sorted(set(live))
    n_groups = len(values) + (1 if len(live) < len(keys) else 0)
    if n_groups > 2 ** 31 - 1:
        raise ValueError("more than 2^31-1 groups")
    where = {v: i for i, v in enumerate(values)}
    ids = np.fromiter((len(values) if k is None else where[k] for k in keys), np.int32, len(keys))
    return ids, values, n_groups


def default_pool_k(top_k: int, num_documents: int, limit: int = NP_GROUP_MAX_LIST) -> int:
    """ColGREP's over-fetch for top_k groups (colgrep/src/index/mod.rs: max(20 top_k, 200)), inside what the index holds
    and inside the entry's limit."""
    return max(1, min(max(20 * int(top_k), 200), max(int(num_documents), int(top_k)), int(limit)))


def _groups_of_rows(B, k, g, ids, sc, grp, mem, tot, cnt):
    """The padded outputs of a grouped call -> per query a list of (group_id, passage_ids, scores or None, total)."""
    if B == 0:
        return []
    ids = ids.reshape(B, k, g)
    sc = None if sc is None else sc.reshape(B, k, g)
    grp, mem, tot = (x.reshape(B, k) for x in (grp, mem, tot))
    return [[(int(grp[i, j]), ids[i, j, : mem[i, j]].copy(), None if sc is None else sc[i, j, : mem[i, j]].copy(), int(tot[i, j]))
             for j in range(int(cnt[i]))] for i in range(B)]


def _group_outputs(B, k, g, scores=True):
    n = max(B * k * g, 1)
    return (np.zeros(n, np.int64), np.zeros(n, np.float32) if scores else None, np.zeros(max(B * k, 1), np.int32),
            np.zeros(max(B * k, 1), np.int32), np.zeros(max(B * k, 1), np.int32), np.zeros(max(B, 1), np.int32))


def collapse(ids, scores, top_k: int, group_size: int, index):
    """np_hip_collapse over a batch of ranked lists (sequences of id arrays; `scores` likewise or None): walk each list, admit
    a group -- index.set_groups -- at its first entry while fewer than top_k are admitted, keep the first group_size entries of
    every admitted group and count them all.  Returns per query a list of groups (group_id, passage_ids, scores, total) in
    order of admission; scores is None when none were given."""
    B = len(ids)
    if scores is not None and len(scores) != B:
        raise ValueError(f"{B} id lists and {len(scores)} score lists")
    fi, cnt, w = _pad_lists(ids, np.int64)
    fs = None if scores is None else _pad_lists(scores, np.float32, w)[0]
    return _groups_of_rows(B, max(int(top_k), 1), max(int(group_size), 1),
                           *index.collapse_raw(fi, fs, cnt, w, top_k, group_size))


# ---- crate mirror ------------------------------------------------------------------------------------

@dataclass
class SearchParameters:
    """search.rs:26-69 (same field names and defaults) + `precision`, the arithmetic of the exact MaxSim stage
    (S1-S5 are always exact f32): 2 (default) = QC-reuse form with split-bf16 MFMA on the residual term (error bound
    against float64 derived in tests/exact_restate.py, measured in profiles/s6_error_bounds.md); 0 = exact-f32 MFMA on decompressed rows;
    1 = QC-reuse with plain bf16 on the residual term (<= 1e-3 relative); 3 = bf16 MFMA on decompressed rows."""
    batch_size: int = 2000
    n_full_scores: int = 4096
    top_k: int = 10
    n_ivf_probe: int = 8
    centroid_batch_size: int = 100_000
    centroid_score_threshold: float | None = 0.4
    precision: int = 2

    # serde (search.rs:26-48): the four counts are required fields, `centroid_batch_size` and `centroid_score_threshold`
    # carry #[serde(default = ...)] (100 000 / Some(0.4)); an explicit null threshold is None; unknown fields are ignored
    @classmethod
    def from_json(cls, text) -> "SearchParameters":
        import json
        d = json.loads(text) if isinstance(text, (str, bytes)) else dict(text)
        for k in ("batch_size", "n_full_scores", "top_k", "n_ivf_probe"):
            if k not in d:
                raise ValueError(f"missing field `{k}`")
            if isinstance(d[k], bool) or not isinstance(d[k], int) or d[k] < 0:
                raise ValueError(f"invalid type for `{k}`: expected usize")
        t = d.get("centroid_score_threshold", 0.4)
        return cls(batch_size=d["batch_size"], n_full_scores=d["n_full_scores"], top_k=d["top_k"], n_ivf_probe=d["n_ivf_probe"],
                   centroid_batch_size=int(d.get("centroid_batch_size", 100_000)),
                   centroid_score_threshold=None if t is None else float(t), precision=int(d.get("precision", 2)))

    def to_json(self) -> str:
        import json
        return json.dumps(dict(batch_size=self.batch_size, n_full_scores=self.n_full_scores, top_k=self.top_k,
                               n_ivf_probe=self.n_ivf_probe, centroid_batch_size=self.centroid_batch_size,
                               centroid_score_threshold=self.centroid_score_threshold))

    def _c(self) -> np_search_params:
        t = self.centroid_score_threshold
        return np_search_params(self.top_k, self.n_full_scores, self.n_ivf_probe, self.centroid_batch_size,
                                0.0 if t is None else float(t), 0 if t is None else 1, self.precision)


@dataclass
class IndexConfig:
    """IndexConfig (index.rs:60-112): the fields that apply to index creation, same names and defaults.  `seed` is
    required here (the crate's None = an entropy seed has no counterpart); start_from_scratch < 0 never writes
    embeddings.npy."""
    nbits: int = 4
    batch_size: int = 50_000
    seed: int = 42
    kmeans_niters: int = 4
    max_points_per_centroid: int = 256
    n_samples_kmeans: int | None = None
    start_from_scratch: int = 999

    # serde (index.rs:60-112): every field but nbits has a default; unknown fields (force_cpu, fts_tokenizer) are ignored
    @classmethod
    def from_json(cls, text) -> "IndexConfig":
        import json
        d = json.loads(text) if isinstance(text, (str, bytes)) else dict(text)
        if "nbits" not in d:
            raise ValueError("missing field `nbits`")
        for k in ("nbits", "batch_size", "kmeans_niters", "max_points_per_centroid", "start_from_scratch"):
            if k in d and (isinstance(d[k], bool) or not isinstance(d[k], int) or d[k] < 0):
                raise ValueError(f"invalid type for `{k}`: expected usize")
        seed = d.get("seed", 42)
        ns = d.get("n_samples_kmeans")
        return cls(nbits=d["nbits"], batch_size=d.get("batch_size", 50_000), seed=42 if seed is None else int(seed),
                   kmeans_niters=d.get("kmeans_niters", 4), max_points_per_centroid=d.get("max_points_per_centroid", 256),
                   n_samples_kmeans=None if ns is None else int(ns), start_from_scratch=d.get("start_from_scratch", 999))

    def to_json(self) -> str:
        import json
        return json.dumps(dict(nbits=self.nbits, batch_size=self.batch_size, seed=self.seed, kmeans_niters=self.kmeans_niters,
                               max_points_per_centroid=self.max_points_per_centroid, n_samples_kmeans=self.n_samples_kmeans,
                               start_from_scratch=self.start_from_scratch))

    def _c(self, num_partitions: int | None = None) -> np_index_config:
        for k in ("nbits", "batch_size", "kmeans_niters", "max_points_per_centroid"):
            if int(getattr(self, k)) <= 0:
                raise ValueError(f"IndexConfig.{k} must be > 0")
        return np_index_config(int(self.nbits), int(self.kmeans_niters), int(self.batch_size), int(self.seed) & (2**64 - 1),
                               int(self.max_points_per_centroid), int(self.n_samples_kmeans or 0), int(num_partitions or 0),
                               -1 if int(self.start_from_scratch) == 0 else int(self.start_from_scratch))


@dataclass
class UpdateConfig:
    """UpdateConfig (update.rs:75-107): same field names and defaults.  start_from_scratch = 0 and buffer_size = 0 keep the
    crate's meaning (only an empty index starts from scratch; every update expands)."""
    batch_size: int = 50_000
    kmeans_niters: int = 4
    max_points_per_centroid: int = 256
    n_samples_kmeans: int | None = None
    seed: int = 42
    start_from_scratch: int = 999
    buffer_size: int = 100

    _USIZE = ("batch_size", "kmeans_niters", "max_points_per_centroid", "seed", "start_from_scratch", "buffer_size")

    # serde (update.rs:75-93): no #[serde(default)] on the struct, so every field but the Option and force_cpu is required;
    # force_cpu (and any other unknown field) is ignored
    @classmethod
    def from_json(cls, text) -> "UpdateConfig":
        import json
        d = json.loads(text) if isinstance(text, (str, bytes)) else dict(text)
        for k in cls._USIZE:
            if k not in d:
                raise ValueError(f"missing field `{k}`")
        for k in cls._USIZE:
            if isinstance(d[k], bool) or not isinstance(d[k], int) or d[k] < 0:
                raise ValueError(f"invalid type for `{k}`: expected usize")
        ns = d.get("n_samples_kmeans")
        if ns is not None and (isinstance(ns, bool) or not isinstance(ns, int) or ns < 0):
            raise ValueError("invalid type for `n_samples_kmeans`: expected usize")
        return cls(**{k: d[k] for k in cls._USIZE}, n_samples_kmeans=ns)

    def to_json(self) -> str:
        import json
        return json.dumps(dict(batch_size=self.batch_size, kmeans_niters=self.kmeans_niters,
                               max_points_per_centroid=self.max_points_per_centroid, n_samples_kmeans=self.n_samples_kmeans,
                               seed=self.seed, start_from_scratch=self.start_from_scratch, buffer_size=self.buffer_size,
                               force_cpu=False))

    def _c(self) -> np_update_config:
        for k in ("batch_size", "kmeans_niters", "max_points_per_centroid"):
            if int(getattr(self, k)) <= 0:
                raise ValueError(f"UpdateConfig.{k} must be > 0")
        return np_update_config(int(self.batch_size), int(self.kmeans_niters), 0, int(self.max_points_per_centroid),
                                int(self.n_samples_kmeans or 0), int(self.seed) & (2**64 - 1),
                                -1 if int(self.start_from_scratch) == 0 else int(self.start_from_scratch),
                                -1 if int(self.buffer_size) == 0 else int(self.buffer_size))


@dataclass
class AppendRows:
    """What MmapIndex.append / append_arrays take with rows=: the new documents' attachment rows.  `columns`: name -> the new
    entries, under exactly the names of the handle's columns (None where it has none); `groups`: one key per new document, as
    set_groups takes them (ready int32 ids where the handle's groups were set with n_groups=, then with `n_groups`; None
    where the handle has no groups); `texts`: the new documents' text for the keyword index (None where it has none),
    tokenised as the handle's text_utf8 / text_unicode_planes say (MmapIndex)."""
    columns: dict | None = None
    groups: object = None
    texts: object = None
    n_groups: int | None = None


def _update_docs(documents):
    """Like _docs, but an empty list is allowed (an update with no documents changes nothing)."""
    if len(documents) == 0:
        return np.zeros((1, 1), np.float32), np.zeros(0, np.int64), None
    return _docs(documents)


def _update_call(fn, index_path: str, documents, config, device: int):
    flat, lens, dim = _update_docs(documents)
    rep = np_update_report()
    cfg = (config or UpdateConfig())._c()
    if lens.size == 0:
        dim = 0
    _check(fn(os.fsencode(index_path), _ptr(flat), _ptr(lens), lens.size, int(dim or 0), C.byref(cfg), int(device),
              C.byref(rep)))
    ids = np.arange(rep.first_doc_id, rep.first_doc_id + lens.size, dtype=np.int64)
    return ids, rep.as_dict()


def update_index_dir(index_path: str, documents, config: UpdateConfig | None = None, device: int = 0):
    """MmapIndex::update on a directory (index.rs:1431-1590): returns (new document ids, report dict)."""
    return _update_call(lib().np_hip_index_update, index_path, documents, config, device)


def update_append_dir(index_path: str, documents, config: UpdateConfig | None = None, device: int = 0):
    """MmapIndex::update_append (index.rs:1675-1700): returns (new document ids, report dict)."""
    return _update_call(lib().np_hip_index_update_append, index_path, documents, config, device)


def _dir_counts(index_path: str):
    """(num_documents, num_embeddings) of an index directory's metadata.json"""
    with open(os.path.join(index_path, "metadata.json"), "rb") as f:
        m = json.loads(f.read())
    return int(m["num_documents"]), int(m["num_embeddings"])


def _appended_tokens(index_path: str, before):
    """What an update_append wrote for its documents, read back from the chunk files: (doc_lengths, codes, residuals) of the
    documents the directory holds beyond the counts `before` -- the tail of its last chunks (update_index appends to the last
    chunk or adds chunks, update.rs:771-1120)."""
    with open(os.path.join(index_path, "metadata.json"), "rb") as f:
        m = json.loads(f.read())
    n_new, t_new = int(m["num_documents"]) - before[0], int(m["num_embeddings"]) - before[1]
    lens, codes, res = [], [], []
    have_d = have_t = 0
    c = int(m["num_chunks"]) - 1
    while have_d < n_new and c >= 0:
        with open(os.path.join(index_path, f"doclens.{c}.json"), "rb") as f:
            dl = np.asarray(json.loads(f.read()), np.int64).reshape(-1)
        take_d = min(n_new - have_d, dl.size)
        tail = dl[dl.size - take_d:]
        take_t = int(tail.sum())
        cd = np.load(os.path.join(index_path, f"{c}.codes.npy"), mmap_mode="r")
        rs = np.load(os.path.join(index_path, f"{c}.residuals.npy"), mmap_mode="r")
        lens.insert(0, tail)
        codes.insert(0, np.asarray(cd[cd.shape[0] - take_t:], np.int64))
        res.insert(0, np.asarray(rs[rs.shape[0] - take_t:], np.uint8))
        have_d += take_d
        have_t += take_t
        c -= 1
    if have_d != n_new or have_t != t_new:
        raise IndexLoadError(f"Index load failed: the chunk files hold {have_d} new documents / {have_t} tokens, "
                             f"metadata.json counts {n_new} / {t_new}")
    pd = res[0].shape[1] if res else 0
    return (np.concatenate(lens) if lens else np.zeros(0, np.int64),
            np.concatenate(codes) if codes else np.zeros(0, np.int64),
            np.concatenate(res) if res else np.zeros((0, pd), np.uint8))


def _tail_documents(index_path: str, n_tail: int):
    """_appended_tokens' reading for a given count: (doc_lengths, codes, residuals) of the directory's LAST n_tail documents,
    from the tail of its last chunks -- what an update in expansion mode wrote behind the documents it kept."""
    with open(os.path.join(index_path, "metadata.json"), "rb") as f:
        m = json.loads(f.read())
    lens, codes, res = [], [], []
    have_d = 0
    c = int(m["num_chunks"]) - 1
    while have_d < n_tail and c >= 0:
        with open(os.path.join(index_path, f"doclens.{c}.json"), "rb") as f:
            dl = np.asarray(json.loads(f.read()), np.int64).reshape(-1)
        take_d = min(n_tail - have_d, dl.size)
        tail = dl[dl.size - take_d:]
        take_t = int(tail.sum())
        cd = np.load(os.path.join(index_path, f"{c}.codes.npy"), mmap_mode="r")
        rs = np.load(os.path.join(index_path, f"{c}.residuals.npy"), mmap_mode="r")
        lens.insert(0, tail)
        codes.insert(0, np.asarray(cd[cd.shape[0] - take_t:], np.int64))
        res.insert(0, np.asarray(rs[rs.shape[0] - take_t:], np.uint8))
        have_d += take_d
        c -= 1
    if have_d != n_tail:
        raise IndexLoadError(f"Index load failed: the chunk files hold {have_d} documents, {n_tail} were written")
    pd = res[0].shape[1] if res else 0
    return (np.concatenate(lens) if lens else np.zeros(0, np.int64),
            np.concatenate(codes) if codes else np.zeros(0, np.int64),
            np.concatenate(res) if res else np.zeros((0, pd), np.uint8))


def delete_from_index_dir(index_path: str, doc_ids) -> int:
    """MmapIndex::delete (delete.rs:43-268), host only: the number of distinct ids removed.  Ids outside
    [0, num_documents) are ignored (include/nextplaid_hip.h)."""
    ids = np.ascontiguousarray(np.asarray(doc_ids, np.int64).reshape(-1))
    out = C.c_int64(0)
    _check(lib().np_hip_index_delete(os.fsencode(index_path), _ptr(ids) if ids.size else None, ids.size, C.byref(out)))
    return int(out.value)


def _docs(documents):
    """List of [n_i, dim] arrays -> (flat f32 [sum n_i, dim], lengths i64, dim)."""
    docs = [np.ascontiguousarray(d, np.float32) for d in documents]
    if not docs:
        raise IndexCreationError("Index creation failed: No documents provided")
    dim = docs[0].shape[1] if docs[0].ndim == 2 else -1
    for d in docs:
        if d.ndim != 2 or d.shape[1] != dim:
            raise ShapeError(f"Shape error: document has shape {d.shape}, expected [n, {dim}]")
    lens = np.array([d.shape[0] for d in docs], np.int64)
    flat = np.concatenate(docs, 0) if lens.sum() > 0 else np.zeros((1, max(dim, 1)), np.float32)
    return np.ascontiguousarray(flat, np.float32), lens, dim


def _text_build_open(L, doc_bytes, offsets, tokenizer, tokenize_fallback, device, max_token_bytes, workspace_bytes, hash_bits,
                     tile_bytes, utf8=False, unicode_planes=2):
    """np_hip_text_build and np_hip_text_build_add: (the build, the fallback ids, the report).  The caller frees the build.
    utf8: opts->unicode_table is text.unicode61_table(unicode_planes), SQLite's rule probed from SQLite (the library reads
    it during the call only); otherwise the table is NULL and the device reproduces ASCII text alone."""
    raw = np.ascontiguousarray(doc_bytes, np.uint8).reshape(-1)
    off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
    if off.size < 1:
        raise ValueError("offsets needs n_docs + 1 entries")
    o = np_text_build_opts(int(tokenizer), int(max_token_bytes), int(workspace_bytes), int(hash_bits), int(tile_bytes))
    table = None
    if utf8:
        from . import text as T
        table = T.unicode61_table(unicode_planes)
        o.unicode_table, o.unicode_table_len = table.ctypes.data, table.size
    rep, h = np_text_build_report(), C.c_void_p()
    _check(L.np_hip_text_build(int(device), _ptr(raw) if raw.size else None, _ptr(off), off.size - 1, C.byref(o), C.byref(h),
                               C.byref(rep)))
    try:
        fb = np.zeros(max(int(rep.n_fallback), 1), np.int64)
        _check(L.np_hip_text_build_fallback(h, _ptr(fb), None))
        fb = fb[: int(rep.n_fallback)]
        if fb.size:
            if tokenize_fallback is None:
                raise ValueError(f"{fb.size} documents (the first: {int(fb[0])}) are not reproduced on the device and "
                                           f"no tokenize_fallback was given")
            tb, tbo, it, idoc, ipos = tokenize_fallback(fb)
            tb = np.ascontiguousarray(tb, np.uint8)
            tbo = np.ascontiguousarray(tbo, np.int64)
            it = np.ascontiguousarray(it, np.int32)
            idoc = np.ascontiguousarray(idoc, np.int64)
            ipos = np.ascontiguousarray(ipos, np.int32)
            _check(L.np_hip_text_build_add(h, _ptr(tb) if tb.size else None, _ptr(tbo), tbo.size - 1, _ptr(it), _ptr(idoc),
                                           _ptr(ipos), it.size))
    except BaseException:
        L.np_hip_text_build_free(h)
        raise
    return h, fb, rep


def _text_build_read(L, h):
    """np_hip_text_build_sizes and np_hip_text_build_fetch: the arrays of a build (sizes finalises it)."""
    nt, nb, ni, nr = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _check(L.np_hip_text_build_sizes(h, C.byref(nt), C.byref(nb), C.byref(ni), C.byref(nr)))
    out = dict(term_bytes=np.zeros(max(nb.value, 1), np.uint8), term_byte_offsets=np.zeros(nt.value + 1, np.int64),
               term_offsets=np.zeros(nt.value + 1, np.int64), inst_doc=np.zeros(max(ni.value, 1), np.int64),
               inst_pos=np.zeros(max(ni.value, 1), np.int32))
    _check(L.np_hip_text_build_fetch(h, *(_ptr(out[k]) for k in ("term_bytes", "term_byte_offsets", "term_offsets",
                                                                  "inst_doc", "inst_pos"))))
    out["term_bytes"] = out["term_bytes"][: nb.value]
    out["inst_doc"] = out["inst_doc"][: ni.value]
    out["inst_pos"] = out["inst_pos"][: ni.value]
    out["n_rows"] = int(nr.value)
    return out


def text_build(doc_bytes, offsets, tokenizer: int, tokenize_fallback=None, device: int = 0, max_token_bytes: int = 0,
               workspace_bytes: int = 0, hash_bits: int = 0, tile_bytes: int = 0, utf8: bool = False, unicode_planes: int = 2):
    """np_hip_text_build and the calls that follow it: the documents' UTF-8 bytes concatenated (u8 array) and offsets i64
    [n_docs + 1] -> a dict with term_bytes u8, term_byte_offsets / term_offsets i64 [n_terms + 1], inst_doc i64, inst_pos
    i32, n_rows, fallback_docs i64 (ascending) and the stage report.  tokenize_fallback(ids) is called once when the device
    hands documents back, and returns their instances as (term_bytes u8, term_byte_offsets i64, inst_term i32, inst_doc i64,
    inst_pos i32) sorted by (term, doc, pos) with the terms in memcmp order; without it a non-empty fallback list is an
    error, never a silently smaller index.  utf8=True is the library's UTF-8 mode with text.unicode61_table(unicode_planes)
    (unicode61 only; trigram ignores it)."""
    L = lib()
    h, fb, rep = _text_build_open(L, doc_bytes, offsets, tokenizer, tokenize_fallback, device, max_token_bytes, workspace_bytes,
                                  hash_bits, tile_bytes, utf8, unicode_planes)
    try:
        out = _text_build_read(L, h)
        out.update(fallback_docs=fb, report=rep.as_dict())
        return out
    finally:
        L.np_hip_text_build_free(h)


def text_merge(base_terms, base_term_offsets, base_inst_doc, base_inst_pos, base_n_rows, remap, delta_ids, n_rows_out,
               doc_bytes=None, offsets=None, tokenizer: int = 0, tokenize_fallback=None, device: int = 0, max_token_bytes: int = 0,
               workspace_bytes: int = 0, merge_workspace_bytes: int = 0, hash_bits: int = 0, tile_bytes: int = 0,
               utf8: bool = False, unicode_planes: int = 2):
    """np_hip_text_build_merge, the one caller of the entry: the keyword index of the table that results from a base index
    (its terms as byte strings in term order, and the np_text_index arrays), a verdict per old document (remap i64: -1 =
    removed, otherwise the new id) and a batch of new texts (doc_bytes / offsets as text_build takes them; offsets None = no
    batch) whose documents get delta_ids.  The batch is built on the device first (np_hip_text_build, the fallback documents
    added as in text_build) and merged where it lies.  Returns text_build's dict; `report` is the merge's, `build_report` the
    batch's (None without a batch), fallback_docs index the batch.  utf8 / unicode_planes: text_build's, for the batch."""
    L = lib()
    enc = [bytes(t) for t in base_terms]
    a_tbo = np.zeros(len(enc) + 1, np.int64)
    if enc:
        a_tbo[1:] = np.cumsum([len(t) for t in enc])
    a_tb = np.frombuffer(b"".join(enc), np.uint8)
    a_off = np.ascontiguousarray(base_term_offsets, np.int64).reshape(-1)
    a_doc = np.ascontiguousarray(base_inst_doc, np.int64).reshape(-1)
    a_pos = np.ascontiguousarray(base_inst_pos, np.int32).reshape(-1)
    if a_off.size != len(enc) + 1:
        raise ValueError(f"base_term_offsets has {a_off.size} entries for {len(enc)} terms")
    remap = np.ascontiguousarray(remap, np.int64).reshape(-1)
    ids = np.ascontiguousarray(delta_ids, np.int64).reshape(-1)
    n_delta = 0 if offsets is None else int(np.asarray(offsets).size) - 1
    if ids.size != n_delta:
        raise ValueError(f"delta_ids has {ids.size} entries for a batch of {n_delta} documents")
    t = np_text_index(len(enc), a_off.ctypes.data, a_doc.ctypes.data if a_doc.size else None,
                      a_pos.ctypes.data if a_pos.size else None, int(base_n_rows))
    d, fb, brep = C.c_void_p(), np.zeros(0, np.int64), None
    if offsets is not None:
        d, fb, brep = _text_build_open(L, doc_bytes if doc_bytes is not None else np.zeros(0, np.uint8), offsets, tokenizer,
                                       tokenize_fallback, device, max_token_bytes, workspace_bytes, hash_bits, tile_bytes,
                                       utf8, unicode_planes)
    h = C.c_void_p()
    try:
        if d:
            _check(L.np_hip_text_build_sizes(d, None, None, None, None))
        o, rep = np_text_merge_opts(int(merge_workspace_bytes)), np_text_merge_report()
        _check(L.np_hip_text_build_merge(int(device), C.byref(t), _ptr(a_tb) if a_tb.size else None, _ptr(a_tbo),
                                         _ptr(remap) if remap.size else None, remap.size, d, _ptr(ids) if ids.size else None,
                                         int(n_rows_out), C.byref(o), C.byref(h), C.byref(rep)))
        out = _text_build_read(L, h)
        out.update(fallback_docs=fb, report=rep.as_dict(), build_report=brep.as_dict() if brep is not None else None)
        return out
    finally:
        if h:
            L.np_hip_text_build_free(h)
        if d:
            L.np_hip_text_build_free(d)


def _text_build_vocab(L, h):
    """np_hip_text_build_sizes and the vocabulary half of np_hip_text_build_fetch: (the terms as strings, n_rows, the
    instance count).  No instance array crosses the bus; a consumed build still answers."""
    nt, nb, ni, nr = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _check(L.np_hip_text_build_sizes(h, C.byref(nt), C.byref(nb), C.byref(ni), C.byref(nr)))
    tb, tbo = np.zeros(max(nb.value, 1), np.uint8), np.zeros(nt.value + 1, np.int64)
    _check(L.np_hip_text_build_fetch(h, _ptr(tb), _ptr(tbo), None, None, None))
    raw = tb[: nb.value].tobytes()
    return [raw[tbo[i]: tbo[i + 1]].decode("utf-8") for i in range(nt.value)], int(nr.value), int(ni.value)


def text_merge_resident(index_handle, base_terms, remap, delta_ids, n_rows_out, doc_bytes=None, offsets=None, tokenizer: int = 0,
                        tokenize_fallback=None, device: int = 0, max_token_bytes: int = 0, workspace_bytes: int = 0,
                        merge_workspace_bytes: int = 0, hash_bits: int = 0, tile_bytes: int = 0, utf8: bool = False,
                        unicode_planes: int = 2):
    """np_hip_index_text_merge, the one caller of the entry: text_merge whose base is the keyword index of the handle
    `index_handle`, read where it lies.  base_terms are the handle's terms as byte strings, in term order.  Returns (the
    result, a finalised device build that the caller installs with np_hip_index_set_text_build or frees; the merge's report
    as a dict, the batch's under "batch"; the batch's fallback ids)."""
    L = lib()
    enc = [bytes(t) for t in base_terms]
    nt = C.c_int64()
    _check(L.np_hip_index_text_sizes(index_handle, C.byref(nt), None, None, None, None))
    if len(enc) != nt.value:
        raise ValueError(f"base_term_byte_offsets describes {len(enc)} terms, the handle's keyword index holds {nt.value}")
    a_tbo = np.zeros(len(enc) + 1, np.int64)
    if enc:
        a_tbo[1:] = np.cumsum([len(t) for t in enc])
    a_tb = np.frombuffer(b"".join(enc), np.uint8)
    remap = np.ascontiguousarray(remap, np.int64).reshape(-1)
    ids = np.ascontiguousarray(delta_ids, np.int64).reshape(-1)
    n_delta = 0 if offsets is None else int(np.asarray(offsets).size) - 1
    if ids.size != n_delta:
        raise ValueError(f"delta_ids has {ids.size} entries for a batch of {n_delta} documents")
    d, fb, brep = C.c_void_p(), np.zeros(0, np.int64), None
    if offsets is not None:
        d, fb, brep = _text_build_open(L, doc_bytes if doc_bytes is not None else np.zeros(0, np.uint8), offsets, tokenizer,
                                       tokenize_fallback, device, max_token_bytes, workspace_bytes, hash_bits, tile_bytes,
                                       utf8, unicode_planes)
    h = C.c_void_p()
    try:
        if d:
            _check(L.np_hip_text_build_sizes(d, None, None, None, None))
        o, rep = np_text_merge_opts(int(merge_workspace_bytes)), np_text_merge_report()
        _check(L.np_hip_index_text_merge(index_handle, _ptr(a_tb) if a_tb.size else None, _ptr(a_tbo),
                                         _ptr(remap) if remap.size else None, remap.size, d, _ptr(ids) if ids.size else None,
                                         int(n_rows_out), C.byref(o), C.byref(h), C.byref(rep)))
    finally:
        if d:
            L.np_hip_text_build_free(d)
    return h, dict(rep.as_dict(), batch=brep.as_dict() if brep is not None else None), fb


_POOL_CUTS = {"reference": 0, "distance": 1}


def _pool_opts(pool_factor, protected_tokens, cut, chunk_docs=0):
    if cut not in _POOL_CUTS:
        raise ValueError(f"cut must be 'reference' or 'distance', got {cut!r}")
    return np_pool_opts(int(pool_factor), int(protected_tokens), _POOL_CUTS[cut], 0, int(chunk_docs))


def pooled_lengths(doc_lengths, pool_factor: int, protected_tokens: int = 1):
    """Host only: every document's token count after pool_document_embeddings (lib.rs:2254-2266)."""
    dl = np.ascontiguousarray(doc_lengths, np.int64)
    out = np.zeros(max(dl.size, 1), np.int64)
    o = _pool_opts(pool_factor, protected_tokens, "reference")
    _check(lib().np_hip_pooled_lengths(_ptr(dl), dl.size, C.byref(o), _ptr(out)))
    return out[: dl.size]


def pool_document_embeddings(documents, pool_factor: int, protected_tokens: int = 1, cut: str = "reference", device: int = 0,
                             return_labels: bool = False, chunk_docs: int = 0, return_details: bool = False):
    """pool_document_embeddings (next-plaid-onnx lib.rs:1632-1643, :2249-2317; hierarchy.rs) on the GPU, bit for bit: Ward
    clustering of every document's tokens after the first `protected_tokens` into (n - protected) / pool_factor clusters,
    each replaced by the mean of its members.  cut="reference" applies the merges in the order the crate's chain finds them
    (an index built from the result equals one built by the crate); cut="distance" is the dendrogram cut of scipy / PyLate.
    Returns the pooled documents (a list of [n_i', dim] f32 arrays); with return_labels also the per-token labels of every
    document (0 = protected or unchanged, 1.. = cluster in output order); with return_details a dict with the linkage rows
    of the clustered documents (f64 [m - 1, 4] each, None for the others) and the stage report."""
    docs = [np.ascontiguousarray(d, np.float32) for d in documents]
    if not docs:
        return ([], []) if return_labels else []
    dim = docs[0].shape[1] if docs[0].ndim == 2 else -1
    for d in docs:
        if d.ndim != 2 or d.shape[1] != dim:
            raise ShapeError(f"Shape error: document has shape {d.shape}, expected [n, {dim}]")
    lens = np.array([d.shape[0] for d in docs], np.int64)
    flat = np.ascontiguousarray(np.concatenate(docs, 0), np.float32) if lens.sum() > 0 else np.zeros((1, max(dim, 1)), np.float32)
    o = _pool_opts(pool_factor, protected_tokens, cut, chunk_docs)
    plen = np.zeros(lens.size, np.int64)
    _check(lib().np_hip_pooled_lengths(_ptr(lens), lens.size, C.byref(o), _ptr(plen)))
    out = np.zeros((max(int(plen.sum()), 1), max(dim, 1)), np.float32)
    olen = np.zeros(lens.size, np.int64)
    labels = np.zeros(max(int(lens.sum()), 1), np.int32) if return_labels else None
    clustered = plen != lens
    nlink = int((lens[clustered] - int(protected_tokens) - 1).sum())
    link = np.zeros((max(nlink, 1), 4), np.float64) if return_details else None
    rep = np_pool_report()
    _check(lib().np_hip_pool_documents(int(device), _ptr(flat), _ptr(lens), lens.size, dim, C.byref(o), _ptr(out),
                                       int(plen.sum()), _ptr(olen), _ptr(labels), _ptr(link), C.byref(rep)))
    oo = np.concatenate([[0], np.cumsum(olen)])
    pooled = [out[oo[i]: oo[i + 1]].copy() for i in range(lens.size)]
    res = [pooled]
    if return_labels:
        io = np.concatenate([[0], np.cumsum(lens)])
        res.append([labels[io[i]: io[i + 1]].copy() for i in range(lens.size)])
    if return_details:
        links, r = [], 0
        for i in range(lens.size):
            if clustered[i]:
                nr = int(lens[i]) - int(protected_tokens) - 1
                links.append(link[r: r + nr].copy())
                r += nr
            else:
                links.append(None)
        res.append({"linkage": links, "report": rep.as_dict()})
    return res[0] if len(res) == 1 else tuple(res)


def kmeans_plan(doc_lengths, config: IndexConfig | None = None, num_partitions: int | None = None):
    """Host only: what compute_kmeans / prepare_codec_artifacts do for these document lengths (kmeans.rs:261-311,
    index.rs:199-226).  Returns (np_kmeans_plan as a dict, sampled document ids in shuffled order)."""
    cfg = (config or IndexConfig())._c(num_partitions)
    dl = np.ascontiguousarray(doc_lengths, np.int64)
    p = np_kmeans_plan()
    ids = np.zeros(max(dl.size, 1), np.int64)
    _check(lib().np_hip_kmeans_plan(_ptr(dl), dl.size, C.byref(cfg), C.byref(p), _ptr(ids)))
    return {k: int(getattr(p, k)) for k, _ in p._fields_}, ids[: p.n_samples].copy()


def estimate_num_partitions(documents, config: IndexConfig | None = None) -> int:
    """The number of centroids compute_kmeans computes for these documents (kmeans.rs:423-...)."""
    lens = np.array([np.shape(d)[0] for d in documents], np.int64)
    if lens.size == 0:
        raise IndexCreationError("Index creation failed: No documents provided")
    return kmeans_plan(lens, config)[0]["k"]


def kmeans(points, k: int, max_iters: int = 4, tol: float = 1e-8, seed: int = 0, max_points_per_centroid: int = 256,
           init=None, device: int = 0, return_assign: bool = False):
    """FastKMeans::train on the GPU (rules: include/nextplaid_hip.h).  Returns (centroids [k, dim], report dict) or,
    with return_assign, (centroids, assignment i64 [n] with -1 outside the subsample, report)."""
    x = np.ascontiguousarray(points, np.float32)
    if x.ndim != 2:
        raise ShapeError(f"Shape error: points have shape {x.shape}")
    n, dim = x.shape
    o = np_kmeans_opts(int(k), int(max_points_per_centroid), int(seed) & (2**64 - 1), float(tol), int(max_iters), 0)
    ini = None
    if init is not None:
        ini = np.ascontiguousarray(init, np.float32)
        if ini.shape != (int(k), dim):
            raise ShapeError(f"Shape error: init has shape {ini.shape}, expected {(int(k), dim)}")
    out = np.zeros((max(int(k), 1), max(dim, 1)), np.float32)
    asg = np.zeros(max(n, 1), np.int64) if return_assign else None
    rep = np_kmeans_report()
    _check(lib().np_hip_kmeans(int(device), _ptr(x) if n else None, n, dim, C.byref(o), _ptr(ini), _ptr(out), _ptr(asg),
                               C.byref(rep)))
    cen = out[: int(k), :dim]
    if return_assign:
        return cen, asg[:n], rep.as_dict()
    return cen, rep.as_dict()


def compute_kmeans(documents, config: IndexConfig | None = None, num_partitions: int | None = None, device: int = 0,
                   return_report: bool = False):
    """compute_kmeans (kmeans.rs:261-421) on the GPU: L2-normalised centroids [K, dim]."""
    flat, lens, dim = _docs(documents)
    cfg = (config or IndexConfig())._c(num_partitions)
    p, _ = kmeans_plan(lens, config, num_partitions)
    out = np.zeros((max(p["k"], 1), max(dim, 1)), np.float32)
    k = C.c_int64(0)
    rep = np_kmeans_report()
    _check(lib().np_hip_compute_kmeans(int(device), _ptr(flat), _ptr(lens), lens.size, dim, C.byref(cfg), _ptr(out),
                                       out.shape[0], C.byref(k), C.byref(rep)))
    cen = out[: k.value]
    return (cen, rep.as_dict()) if return_report else cen


def prepare_codec_artifacts(documents, centroids, config: IndexConfig | None = None, device: int = 0) -> dict:
    """prepare_codec_artifacts (index.rs:182-287): bucket_cutoffs, bucket_weights, avg_residual, cluster_threshold."""
    flat, lens, dim = _docs(documents)
    cfg = (config or IndexConfig())._c()
    cen = np.ascontiguousarray(centroids, np.float32)
    if cen.ndim != 2 or cen.shape[1] != dim:
        raise ShapeError(f"Shape error: centroids have shape {cen.shape}, documents dim {dim}")
    nb = 1 << int(cfg.nbits)
    cut = np.zeros(nb - 1, np.float32)
    w = np.zeros(nb, np.float32)
    avg = np.zeros(max(dim, 1), np.float32)
    thr = C.c_float(0.0)
    _check(lib().np_hip_prepare_codec_artifacts(int(device), _ptr(flat), _ptr(lens), lens.size, dim, _ptr(cen), cen.shape[0],
                                                C.byref(cfg), _ptr(cut), _ptr(w), _ptr(avg), C.byref(thr)))
    return dict(bucket_cutoffs=cut, bucket_weights=w, avg_residual=avg[:dim], cluster_threshold=np.float32(thr.value))


@dataclass
class QueryResult:
    """search.rs:71-80"""
    query_id: int
    passage_ids: np.ndarray  # i64
    scores: np.ndarray       # f32


def _empty_results(B):
    return [QueryResult(i, np.zeros(0, np.int64), np.zeros(0, np.float32)) for i in range(B)]


class _ResultRows:
    """The [B][k] ids and scores and the [B] counts a search entry fills (ResultStage on the C side): no output array is ever
    empty (the max(..., 1) padding), row j lies at stride k and holds counts[j] entries.  k is the caller's, so that
    max(top_k, 0) of the search_batch forms and max(top_k, 1) everywhere else stay visible where they are chosen."""

    def __init__(self, B: int, k: int, arrays=None):
        self.B, self.k = B, k
        if arrays is None:
            arrays = np.zeros(max(B * k, 1), np.int64), np.zeros(max(B * k, 1), np.float32), np.zeros(max(B, 1), np.int32)
        self.ids, self.sc, self.cnt = arrays

    def ptrs(self):
        """The (out_ids, out_scores, out_counts) arguments"""
        return _ptr(self.ids), _ptr(self.sc), _ptr(self.cnt)

    def results(self, live=None, n_queries=None):
        """One QueryResult per query, its ids and scores copied out of the padded arrays.  Row j is query j, or --
        text_search skips its empty queries -- query live[j] of n_queries; a query without a row has an empty result."""
        ids, sc, k = self.ids, self.sc, self.k
        rows = [QueryResult(j, ids[j * k: j * k + c].copy(), sc[j * k: j * k + c].copy())
                for j, c in enumerate(self.cnt[: self.B].tolist())]
        if live is None:
            return rows
        out = _empty_results(n_queries)
        for row, i in zip(rows, live):
            row.query_id = i
            out[i] = row
        return out


def _failed_batch(rc, parallel, B):
    """The error policy of the search_batch forms (search.rs:650-674): None when the call succeeded; under `parallel` a
    failed search (rc == 2) is B empty results (search.rs:656-660: a failed query yields an empty result); any other
    failure raises the mapped error."""
    if rc == 0:
        return None
    if parallel and rc == 2:
        return _empty_results(B)
    _check(rc)


class _Scope(NamedTuple):
    """The per-query scope of a call as the entries take it (CallSubsets / HostScope on the C side): the CSR of the batch's
    distinct subsets (sid, soff, n_sub) with the queries' map into them (qmap, -1 = none), or the compiled filters `cf`
    with the same map -- then there is no CSR and n_sub counts the filters.  `form` is what the caller gave: None, "subset",
    "subsets" or "filters"."""
    form: str | None
    sid: np.ndarray | None
    soff: np.ndarray | None
    n_sub: int
    qmap: np.ndarray | None
    cf: "_CFilters | None"

    @property
    def csr(self):
        """The (subset_ids, subset_offsets, n_subsets, query_subset) arguments"""
        return _ptr(self.sid), _ptr(self.soff), self.n_sub, _ptr(self.qmap)

    @property
    def filter_args(self):
        """The (filters, n_filters) arguments"""
        cf = self.cf
        return (None, 0) if cf is None else (cf.arr, cf.n)

    def of_rows(self, live):
        """The scope of the queries `live` alone: their entries of the map (one padding entry when none is left)"""
        if self.qmap is None:
            return self
        return self._replace(qmap=np.ascontiguousarray(self.qmap[live], np.int32) if live else np.zeros(1, np.int32))


def _csr_as_given(subset_ids, subset_offsets, query_subset, B):
    """The CSR arrays of the *_csr methods as a _Scope: they reach the library as given (None = NULL, n_subsets =
    len(subset_offsets) - 1) after the two checks that keep the library from reading past them."""
    sid = None if subset_ids is None else np.ascontiguousarray(subset_ids, np.int64)
    soff = None if subset_offsets is None else np.ascontiguousarray(subset_offsets, np.int64)
    qsub = None if query_subset is None else np.ascontiguousarray(query_subset, np.int32)
    if qsub is not None and qsub.size != B:
        raise ValueError(f"query_subset has {qsub.size} entries for {B} queries")
    if sid is not None and soff is not None and soff.size and int(soff[-1]) > sid.size:
        raise ValueError(f"subset_offsets count {int(soff[-1])} ids, subset_ids has {sid.size}")
    return _Scope("subsets", sid, soff, 0 if soff is None else soff.size - 1, qsub, None)


def _filters_as_given(compiled, query_filter, B):
    """The CompiledFilters (or a ready _CFilters) and the queries' map of the *_filtered methods as a _Scope."""
    cf = compiled if isinstance(compiled, _CFilters) else _CFilters(list(compiled))
    qf = np.ascontiguousarray(query_filter, np.int32)
    if qf.size != B:
        raise ValueError(f"query_filter has {qf.size} entries for {B} queries")
    return _Scope("filters", None, None, cf.n, qf, cf)


def _opts(device=0, shard_rank=0, shard_count=1, n_contexts=2, max_batch=64, max_query_tokens=64,
          workspace_bytes=0):
    return np_open_opts(device, shard_rank, shard_count, n_contexts, max_batch, max_query_tokens, workspace_bytes)


class MmapIndex:
    """Device-resident PLAID index; mirror of next_plaid::MmapIndex (index.rs:995-1312)."""

    # How this handle tokenises text for its keyword index where a call has no argument of its own -- build_text /
    # update_text with utf8=None, and the rows.texts of append / append_arrays / update_resident: True = UTF-8 on the
    # device with text.unicode61_table(text_unicode_planes); False = ASCII on the device, the rest through SQLite.
    text_utf8 = False
    text_unicode_planes = 2

    def __init__(self, handle, path="", open_opts=None):
        self._h = handle
        self.path = path
        self._open_opts = dict(open_opts or {})
        self._info = np_info()
        _check(lib().np_hip_index_info(self._h, C.byref(self._info)))
        self.last_stats: dict | None = None
        self.last_update: dict | None = None
        self.schema = None   # set_columns: the columns' names, types and dictionaries (filters.Schema)
        self.last_match_report = None   # match_text / text_match_raw: np_match_report of the last call
        self.text = None     # set_text: the keyword index's arrays and vocabulary (text.TextIndexData)
        self.group_values = None   # set_groups: the distinct non-null keys, sorted (group g < len: its key; the last: the NULLs)

    # -- constructors ---------------------------------------------------------------------------------
    @classmethod
    def load(cls, index_path: str, **opts) -> "MmapIndex":
        """MmapIndex::load (index.rs:1026).  opts: device, shard_rank, shard_count, n_contexts, max_batch."""
        h = C.c_void_p()
        o = _opts(**opts)
        _check(lib().np_hip_index_open(os.fsencode(index_path), C.byref(o), C.byref(h)))
        return cls(h, index_path, opts)

    @classmethod
    def create_with_kmeans(cls, documents, index_path: str, config: IndexConfig | None = None, **opts) -> "MmapIndex":
        """MmapIndex::create_with_kmeans (index.rs:927-967): k-means and codec training on the GPU, every token encoded by
        np_hip_encode_tokens, the crate's file set written under index_path, then the index opened with opts (as load)."""
        flat, lens, dim = _docs(documents)
        cfg = (config or IndexConfig())._c()
        o = _opts(**opts)
        h = C.c_void_p()
        _check(lib().np_hip_index_create(os.fsencode(index_path), _ptr(flat), _ptr(lens), lens.size, dim, C.byref(cfg),
                                         C.byref(o), C.byref(h)))
        return cls(h, index_path, opts)

    def reload(self):
        """MmapIndex::reload (index.rs:1767-1775): refresh the resident index from its directory after the files changed
        (delete / update write new chunk files).  Like the crate -- which releases its maps first -- the old device copy is
        dropped BEFORE the new one is read: two 200 GB copies do not fit one GPU.  Exclusive access, as `&mut self` there;
        a service swaps handles instead.  If the directory no longer loads, the error is raised
        and the handle stays closed.  The reloaded handle has NO metadata columns: updates and deletes re-sequence the
        document ids, so set_columns() has to be called again with the new rows."""
        if not self.path or self.path.startswith("<"):
            raise IndexLoadError("Index load failed: reload() needs an index opened from a directory")
        self.close()
        h = C.c_void_p()
        o = _opts(**self._open_opts)
        _check(lib().np_hip_index_open(os.fsencode(self.path), C.byref(o), C.byref(h)))
        self._h = h
        self.schema = None
        self.text = None     # (and no keyword index, for the same reason: set_text / load_text again)
        self.group_values = None   # (and no groups: set_groups again)
        _check(lib().np_hip_index_info(self._h, C.byref(self._info)))
        self.last_stats = None

    # -- update / delete (index.rs:1431-1775) ----------------------------------------------------------------
    def _dir(self, what: str) -> str:
        if not self.path or self.path.startswith("<"):
            raise IndexLoadError(f"Index load failed: {what}() needs an index opened from a directory")
        return self.path

    def update(self, documents, config: UpdateConfig | None = None) -> np.ndarray:
        """MmapIndex::update (index.rs:1431-1590): the new documents' ids; the handle is reloaded from the rewritten
        directory (without metadata columns: ids are re-sequenced, call set_columns() again).  The report of the call is
        kept in self.last_update."""
        path = self._dir("update")
        ids, self.last_update = update_index_dir(path, documents, config, self._open_opts.get("device", 0))
        self.reload()
        return ids

    @staticmethod
    def update_append(documents, index_path: str, config: UpdateConfig | None = None, device: int = 0) -> np.ndarray:
        """MmapIndex::update_append (index.rs:1675-1700): appends without a mode choice and without loading the index."""
        return update_append_dir(index_path, documents, config, device)[0]

    @classmethod
    def update_or_create(cls, documents, index_path: str, index_config: IndexConfig | None = None,
                         update_config: UpdateConfig | None = None, **opts):
        """MmapIndex::update_or_create (index.rs:1644-1673): (index, ids); created when metadata.json is absent."""
        if os.path.exists(os.path.join(index_path, "metadata.json")):
            index = cls.load(index_path, **opts)
            return index, index.update(documents, update_config)
        index = cls.create_with_kmeans(documents, index_path, index_config, **opts)
        return index, np.arange(len(documents), dtype=np.int64)

    def delete(self, doc_ids) -> int:
        """MmapIndex::delete (index.rs:1731-1765): rewrites the directory and returns the count removed; like the crate
        it does not reload (call reload(); that drops the metadata columns, whose rows no longer match the new ids).
        remove() does the same and brings the resident handle along, without the reload."""
        return delete_from_index_dir(self._dir("delete"), doc_ids)

    # -- remove from the resident index (np_hip_index_remove) ----------------------------------------------
    def remove_ids(self, doc_ids, keep_attachments: bool = False) -> int:
        """np_hip_index_remove on any unsharded handle: the listed documents leave the handle without the index being read
        again.  delete()'s semantics: ids outside [0, num_documents()) are ignored, duplicates count once, surviving document
        d becomes d minus the removed ids below it.  The handle then equals one freshly opened on the shrunk index.  Metadata
        columns, the keyword index and the groups are dropped when something was removed, as reload() leaves a handle;
        capacity() does not shrink.  Searches on other threads go on: the running ones finish on the old index, the next ones
        see the new.  Returns the number of documents removed.

        keep_attachments=True goes through np_hip_index_remove_keep: columns and groups are compacted on the device and stay
        attached -- self.schema keeps its dictionaries and has its row arrays shrunk, self.group_values stays -- and the
        keyword index, which the library drops, is brought along by update_text(delete=<the removed ids>) from the one the
        handle had."""
        ids = np.ascontiguousarray(np.asarray(doc_ids, np.int64).reshape(-1))
        out = C.c_int64(0)
        if keep_attachments:
            n0, saved = self.num_documents(), self.text
            removed = np.unique(ids[(ids >= 0) & (ids < n0)])
            merged = None   # a resident keyword index: merged while the handle still has it, installed after the vector call
            if getattr(saved, "resident", False) and removed.size:
                merged = self._merge_text_resident(delete=removed, renumber=True)
            try:
                _check(lib().np_hip_index_remove_keep(self._h, _ptr(ids) if ids.size else None, ids.size, C.byref(out)))
            except BaseException:
                if merged is not None:
                    lib().np_hip_text_build_free(merged[0])   # refused: the handle keeps its old keyword index
                raise
            _check(lib().np_hip_index_info(self._h, C.byref(self._info)))
            if out.value:
                if self.schema is not None:
                    keep = np.ones(n0, bool)
                    keep[removed] = False
                    self.schema = self.schema.shrunk(keep)
                if self.num_documents() == 0:
                    self.group_values = None   # no document, no groups: what set_groups makes of no keys
                self.text = None
                if merged is not None:
                    saved.invalidate()
                    self._install_text_build(merged[0], saved.tokenizer, merged[1], merged[2])
                elif saved is not None:
                    self.update_text(delete=removed, renumber=True, base=saved)
            elif merged is not None:
                lib().np_hip_text_build_free(merged[0])
            return int(out.value)
        _check(lib().np_hip_index_remove(self._h, _ptr(ids) if ids.size else None, ids.size, C.byref(out)))
        if out.value:
            self.schema = None
            self.text = None
            self.group_values = None
        _check(lib().np_hip_index_info(self._h, C.byref(self._info)))
        return int(out.value)

    def remove(self, doc_ids, keep_attachments: bool = False) -> int:
        """delete() on the handle's directory AND np_hip_index_remove on the handle: where delete() + reload() read the whole
        index again, this costs one pass over the posting lists and one move of the tokens behind the first removed
        document.  The handle equals MmapIndex.load of the directory afterwards (no columns, keyword index or groups: attach
        them again -- or pass keep_attachments=True, see remove_ids).  Returns the number of documents removed."""
        path = self._dir("remove")
        # whatever would refuse the handle's half is found BEFORE the directory is touched: a handle that is not current with
        # its directory, and (a remove of no ids runs the library's checks of the handle: shards)
        n_before = _dir_counts(path)
        if n_before[0] != self.num_documents():
            raise IndexLoadError(f"Index load failed: the directory holds {n_before[0]} documents, the handle "
                                 f"{self.num_documents()}: the handle is not current, reload()")
        _check((lib().np_hip_index_remove_keep if keep_attachments else lib().np_hip_index_remove)(self._h, None, 0, None))
        n = delete_from_index_dir(path, doc_ids)
        m = self.remove_ids(doc_ids, keep_attachments)
        if m != n:
            raise IndexLoadError(f"Index load failed: the directory lost {n} documents, the handle {m}: reload()")
        return n

    # -- append to the resident index (np_hip_index_append) ------------------------------------------------
    def _plan_rows(self, rows: "AppendRows", n_new: int):
        """The checks of an append with rows that need no library call but the group count, and the arrays the entry takes:
        (schema, new columns, remaps, group ids, n_groups, group_values).  Raises before anything is touched."""
        from . import filters as F
        if not isinstance(rows, AppendRows):
            raise TypeError("rows must be an AppendRows")
        if self.text is not None and rows.texts is None:
            raise ValueError("append: the handle has a keyword index and rows.texts is None: pass the new documents' text")
        if self.text is None and rows.texts is not None:
            raise ValueError("append: rows.texts is given and the handle has no keyword index (set_text / build_text)")
        if rows.texts is not None and len(rows.texts) != n_new:
            raise ShapeError(f"Shape error: rows.texts has {len(rows.texts)} entries for {n_new} new documents")
        if (self.schema is None) != (not rows.columns):
            raise F.FilterError("append: rows.columns must hold the new rows of exactly the handle's columns"
                                if self.schema is not None else "append: rows.columns is given and the handle has no columns")
        sch = new = remaps = None
        if self.schema is not None:
            sch, new, remaps = self.schema.extended(dict(rows.columns))
            for c in new.values():
                if c.data.shape[0] != n_new:
                    raise ShapeError(f"Shape error: column '{c.name}' has {c.data.shape[0]} new entries for {n_new} new documents")
        have = self.group_count()
        if (have > 0) != (rows.groups is not None):
            raise ValueError("append: the handle has groups and rows.groups is None" if have > 0 else
                             "append: rows.groups is given and the handle has no groups (set_groups)")
        gids, n_groups, values = None, 0, self.group_values
        if have > 0:
            if len(rows.groups) != n_new:
                raise ShapeError(f"Shape error: rows.groups has {len(rows.groups)} entries for {n_new} new documents")
            if values is None:   # ready ids
                gids = np.ascontiguousarray(rows.groups, np.int32).reshape(-1)
                n_groups = max(have, int(rows.n_groups or 0), int(gids.max()) + 1 if gids.size else 0)
            else:                # keys: an existing key keeps its id, new keys take the next ids in the order they come
                keys = rows.groups.tolist() if isinstance(rows.groups, np.ndarray) else list(rows.groups)
                values = list(values) + ([None] if have == len(values) + 1 else [])   # (the NULLs' group, by its id)
                where = {v: i for i, v in enumerate(values)}
                for k in keys:
                    if k is not None and (isinstance(k, bool) or not isinstance(k, (int, str, np.integer))):
                        raise ValueError(f"a group key must be an int, a string or None, not {type(k).__name__}")
                if len({isinstance(k, str) for k in list(values) + keys if k is not None}) > 1:   # set_groups' own rule
                    raise ValueError("group keys must be all ints or all strings (None aside), the handle's and the new ones together")
                for k in keys:
                    if k not in where:
                        where[k] = len(values)
                        values.append(k)
                gids, n_groups = np.fromiter((where[k] for k in keys), np.int32, len(keys)), len(values)
        return sch, new, remaps, gids, n_groups, values

    def append_arrays(self, doc_lengths, codes, residuals, rows: "AppendRows | None" = None):
        """np_hip_index_append on any unsharded handle: documents already encoded (codes i64 in [0, K), residuals u8
        [tokens, dim * nbits / 8] as np_hip_encode_tokens returns them) take the ids num_documents() .. and are served from
        the next call on, without reading the index again.  The handle then equals one freshly opened on the grown index.
        Metadata columns, the keyword index and the groups are dropped, as reload() leaves a handle (set_columns / set_text /
        set_groups attach the grown ones).  Searches on other threads go on: the running ones finish on the old index, the
        next ones see the new.  Returns the new documents' ids.

        rows=AppendRows(...) goes through np_hip_index_append_rows instead: columns and groups stay attached and take the
        new documents' rows.  self.schema becomes Schema.extended's (a text column's new strings join its sorted dictionary,
        the old rows' codes move on the device, the dictionary text of text_on_device columns is sent again); new group keys
        extend self.group_values at its end, existing ids never move (the NULLs' group, if any, is then the entry None); the
        keyword index is brought along by update_text(new_texts=rows.texts) from the one the handle had.  A handle with a
        keyword index and rows.texts=None is refused before anything is touched."""
        dl = np.ascontiguousarray(np.asarray(doc_lengths, np.int64).reshape(-1))
        if rows is not None:
            return self._append_arrays_rows(dl, codes, residuals, rows)
        cd = np.ascontiguousarray(np.asarray(codes, np.int64).reshape(-1))
        rs = np.ascontiguousarray(residuals, np.uint8)
        tokens = int(dl.sum()) if dl.size and (dl >= 0).all() else 0
        pd = self.embedding_dim() * int(self._info.nbits) // 8
        if cd.size < tokens or rs.size < tokens * pd:
            raise ShapeError(f"Shape error: {tokens} tokens need {tokens} codes and {tokens * pd} residual bytes, got "
                             f"{cd.size} and {rs.size}")
        first = self.num_documents()
        _check(lib().np_hip_index_append(self._h, _ptr(dl) if dl.size else None, dl.size, _ptr(cd) if cd.size else None,
                                         _ptr(rs) if rs.size else None))
        if dl.size:
            self.schema = None
            self.text = None
            self.group_values = None
        _check(lib().np_hip_index_info(self._h, C.byref(self._info)))
        return np.arange(first, first + dl.size, dtype=np.int64)

    def _append_arrays_rows(self, dl, codes, residuals, rows, plan=None):
        sch, new, remaps, gids, n_groups, values = plan if plan is not None else self._plan_rows(rows, dl.size)
        cd = np.ascontiguousarray(np.asarray(codes, np.int64).reshape(-1))
        rs = np.ascontiguousarray(residuals, np.uint8)
        tokens = int(dl.sum()) if dl.size and (dl >= 0).all() else 0
        pd = self.embedding_dim() * int(self._info.nbits) // 8
        if cd.size < tokens or rs.size < tokens * pd:
            raise ShapeError(f"Shape error: {tokens} tokens need {tokens} codes and {tokens * pd} residual bytes, got "
                             f"{cd.size} and {rs.size}")
        n_cols = len(sch) if sch is not None else 0
        cols = (np_column * max(n_cols, 1))()
        tables = (C.c_void_p * max(n_cols, 1))()
        for c in (new or {}).values():
            cols[c.index] = np_column(c.type, 0, c.data.ctypes.data, None if c.valid is None else c.valid.ctypes.data)
            tables[c.index] = None if remaps[c.name] is None else remaps[c.name].ctypes.data
        first, saved = self.num_documents(), self.text
        merged = None   # a resident keyword index: merged while the handle still has it, installed after the vector call
        if getattr(saved, "resident", False) and dl.size:
            merged = self._merge_text_resident(new_texts=list(rows.texts))
        try:
            _check(lib().np_hip_index_append_rows(self._h, _ptr(dl) if dl.size else None, dl.size, _ptr(cd) if cd.size else None,
                                                  _ptr(rs) if rs.size else None, cols, n_cols,
                                                  C.cast(tables, C.c_void_p) if n_cols else None,
                                                  _ptr(gids) if gids is not None and gids.size else None, n_groups))
        except BaseException:
            if merged is not None:
                lib().np_hip_text_build_free(merged[0])   # refused: the handle keeps its old keyword index
            raise
        _check(lib().np_hip_index_info(self._h, C.byref(self._info)))
        if dl.size:
            self.schema, self.group_values, self.text = sch, values, None
            for c in (sch.columns.values() if sch is not None else ()):
                if c.text_on_device and remaps[c.name] is not None:   # the library dropped the old dictionary's text
                    text, off = c.text_arrays()
                    _check(lib().np_hip_index_set_column_text(self._h, c.index, text.ctypes.data if text.size else None,
                                                              _ptr(off), len(c.dictionary)))
            if merged is not None:
                saved.invalidate()
                self._install_text_build(merged[0], saved.tokenizer, merged[1], merged[2])
            elif saved is not None:
                self.update_text(new_texts=list(rows.texts), base=saved)
            _check(lib().np_hip_index_info(self._h, C.byref(self._info)))
        return np.arange(first, first + dl.size, dtype=np.int64)

    def append(self, documents, config: UpdateConfig | None = None, rows: "AppendRows | None" = None) -> np.ndarray:
        """update_append on the handle's directory AND on the handle: the documents are encoded once, by update_append_dir,
        and the codes and residuals it wrote to the chunk files go to np_hip_index_append -- where update() reloads the whole
        index, this costs the new documents plus one pass over the posting lists.  The handle equals MmapIndex.load of the
        directory afterwards (no columns, keyword index or groups: attach them again -- or pass rows=AppendRows(...), see
        append_arrays: they stay and take the new rows).  For an update that may add centroids see update_resident();
        for delete see remove().  Returns the new ids."""
        path = self._dir("append")
        plan = None if rows is None else self._plan_rows(rows, len(documents))   # refused before the directory is touched
        # whatever would refuse the handle's half is found BEFORE the directory is touched: a handle that is not current with
        # its directory, and (an append of no documents runs the library's checks of the handle: shards, list order)
        n_before = _dir_counts(path)
        if n_before[0] != self.num_documents():
            raise IndexLoadError(f"Index load failed: the directory holds {n_before[0]} documents, the handle "
                                 f"{self.num_documents()}: the handle is not current, reload()")
        _check(lib().np_hip_index_append(self._h, None, 0, None, None))
        ids, self.last_update = update_append_dir(path, documents, config, self._open_opts.get("device", 0))
        lens, codes, residuals = _appended_tokens(path, n_before)
        if rows is None:
            self.append_arrays(lens, codes, residuals)
        else:
            self._append_arrays_rows(np.ascontiguousarray(np.asarray(lens, np.int64).reshape(-1)), codes, residuals, rows, plan)
        return ids

    # -- expand the resident index (np_hip_index_expand) ----------------------------------------------------
    def expand_arrays(self, new_centroids, doc_lengths, codes, residuals, n_replace: int = 0,
                      rows: "AppendRows | None" = None, _plan=None):
        """np_hip_index_expand on any unsharded handle: new_centroids [k_new, dim] join the codec as centroids K .., the
        first n_replace of the given documents REPLACE the handle's last n_replace documents (same ids; new lengths, codes
        and residuals) and the others take the ids num_documents() .. -- the crate's update in expansion mode, on the
        handle, in one exclusive section and without reading the index again.  codes lie in [0, K + k_new).  The handle then
        equals one freshly opened on the resulting index.  Columns, keyword index and groups are dropped as append_arrays
        drops them; rows=AppendRows(...) (np_hip_index_expand_rows) keeps them: the replaced documents keep their rows, the
        rows given cover the len(doc_lengths) - n_replace NEW documents, everything else as in append_arrays.  Returns the
        given documents' ids, the replaced ones first."""
        dim = self.embedding_dim()
        cen = np.ascontiguousarray(np.asarray(new_centroids, np.float32))
        if cen.size == 0:
            cen = np.zeros((0, dim), np.float32)
        if cen.ndim != 2 or cen.shape[1] != dim:
            raise ShapeError(f"Shape error: new_centroids has shape {cen.shape}, expected [k_new, {dim}]")
        dl = np.ascontiguousarray(np.asarray(doc_lengths, np.int64).reshape(-1))
        cd = np.ascontiguousarray(np.asarray(codes, np.int64).reshape(-1))
        rs = np.ascontiguousarray(residuals, np.uint8)
        n_replace = int(n_replace)
        tokens = int(dl.sum()) if dl.size and (dl >= 0).all() else 0
        pd = dim * int(self._info.nbits) // 8
        if cd.size < tokens or rs.size < tokens * pd:
            raise ShapeError(f"Shape error: {tokens} tokens need {tokens} codes and {tokens * pd} residual bytes, got "
                             f"{cd.size} and {rs.size}")
        first = self.num_documents() - max(n_replace, 0)
        head = (self._h, _ptr(cen) if cen.size else None, cen.shape[0], n_replace, _ptr(dl) if dl.size else None, dl.size,
                _ptr(cd) if cd.size else None, _ptr(rs) if rs.size else None)
        if rows is None:
            _check(lib().np_hip_index_expand(*head))
            if dl.size or cen.shape[0]:
                self.schema = None
                self.text = None
                self.group_values = None
            _check(lib().np_hip_index_info(self._h, C.byref(self._info)))
            return np.arange(first, first + dl.size, dtype=np.int64)
        n_new = max(dl.size - max(n_replace, 0), 0)
        sch, new, remaps, gids, n_groups, values = _plan if _plan is not None else self._plan_rows(rows, n_new)
        n_cols = len(sch) if sch is not None else 0
        cols = (np_column * max(n_cols, 1))()
        tables = (C.c_void_p * max(n_cols, 1))()
        for c in (new or {}).values():
            cols[c.index] = np_column(c.type, 0, c.data.ctypes.data, None if c.valid is None else c.valid.ctypes.data)
            tables[c.index] = None if remaps[c.name] is None else remaps[c.name].ctypes.data
        saved = self.text
        merged = None   # a resident keyword index: merged while the handle still has it, installed after the vector call
        if getattr(saved, "resident", False) and n_new:
            merged = self._merge_text_resident(new_texts=list(rows.texts))
        try:
            _check(lib().np_hip_index_expand_rows(*head, cols, n_cols, C.cast(tables, C.c_void_p) if n_cols else None,
                                                  _ptr(gids) if gids is not None and gids.size else None, n_groups))
        except BaseException:
            if merged is not None:
                lib().np_hip_text_build_free(merged[0])   # refused: the handle keeps its old keyword index
            raise
        _check(lib().np_hip_index_info(self._h, C.byref(self._info)))
        if n_new:
            self.schema, self.group_values, self.text = sch, values, None
            for c in (sch.columns.values() if sch is not None else ()):
                if c.text_on_device and remaps[c.name] is not None:   # the library dropped the old dictionary's text
                    text, off = c.text_arrays()
                    _check(lib().np_hip_index_set_column_text(self._h, c.index, text.ctypes.data if text.size else None,
                                                              _ptr(off), len(c.dictionary)))
            if merged is not None:
                saved.invalidate()
                self._install_text_build(merged[0], saved.tokenizer, merged[1], merged[2])
            elif saved is not None:
                self.update_text(new_texts=list(rows.texts), base=saved)
            _check(lib().np_hip_index_info(self._h, C.byref(self._info)))
        return np.arange(first, first + dl.size, dtype=np.int64)

    def update_resident(self, documents, config: UpdateConfig | None = None, rows: "AppendRows | None" = None) -> np.ndarray:
        """update() on the handle's directory AND on the handle, without the reload: update_index_dir chooses the mode as the
        crate does, and the handle follows the report -- buffer mode: append_arrays of what the directory gained; expansion
        mode: expand_arrays with the centroids.npy rows the update added, n_replace = the buffered documents it re-indexed and
        the tokens the chunk files hold beyond the kept documents; start-from-scratch mode (a small index is rebuilt whole):
        reload(), which drops the attachments.  The handle equals MmapIndex.load of the directory afterwards.  rows: the
        attachment rows of `documents`, as in append().  Returns the new ids; update() itself still reloads."""
        path = self._dir("update_resident")
        plan = None if rows is None else self._plan_rows(rows, len(documents))   # refused before the directory is touched
        n_before = _dir_counts(path)
        if n_before[0] != self.num_documents():
            raise IndexLoadError(f"Index load failed: the directory holds {n_before[0]} documents, the handle "
                                 f"{self.num_documents()}: the handle is not current, reload()")
        _check(lib().np_hip_index_expand(self._h, None, 0, 0, None, 0, None, None))   # the library's checks of the handle
        ids, self.last_update = update_index_dir(path, documents, config, self._open_opts.get("device", 0))
        mode = self.last_update["mode"]
        if mode == "none":
            return ids
        if mode == "start_from_scratch":
            self.reload()
            return ids
        n_after = _dir_counts(path)
        if mode == "expansion":
            k_new = int(self.last_update["n_new_centroids"])
            n_given = int(self.last_update["n_reindexed"]) + len(documents)
            n_replace = n_before[0] - (n_after[0] - n_given)   # the buffered documents the update deleted from the tail
            if n_replace < 0 or n_replace > n_given:
                raise IndexLoadError(f"Index load failed: the directory gained {n_after[0] - n_before[0]} documents, the update "
                                     f"wrote {n_given}: reload()")
            lens, codes, residuals = _tail_documents(path, n_given)
            cen = np.load(os.path.join(path, "centroids.npy"), mmap_mode="r")
            if cen.shape[0] != self.num_partitions() + k_new:
                raise IndexLoadError(f"Index load failed: the directory holds {cen.shape[0]} centroids, the handle "
                                     f"{self.num_partitions()} and {k_new} new ones: the handle is not current, reload()")
            self.expand_arrays(np.asarray(cen[cen.shape[0] - k_new:], np.float32), lens, codes, residuals, n_replace, rows, plan)
        else:
            lens, codes, residuals = _appended_tokens(path, n_before)
            if rows is None:
                self.append_arrays(lens, codes, residuals)
            else:
                self._append_arrays_rows(np.ascontiguousarray(np.asarray(lens, np.int64).reshape(-1)), codes, residuals, rows, plan)
        if self.num_documents() != n_after[0]:
            raise IndexLoadError(f"Index load failed: the directory gained {n_after[0] - n_before[0]} documents, the handle "
                                 f"{self.num_documents() - n_before[0]}: reload()")
        return ids

    def reserve(self, extra_docs: int, extra_tokens: int):
        """np_hip_index_reserve: room for this many MORE documents / tokens, so that later appends move no per-token array
        (without it every array grows by allocate, copy, free: a peak of the largest array twice).  A service reserves
        right after the open."""
        _check(lib().np_hip_index_reserve(self._h, int(extra_docs), int(extra_tokens)))

    def capacity(self):
        """np_hip_index_capacity: (documents, tokens) the handle's arrays are allocated for."""
        d, t = C.c_int64(0), C.c_int64(0)
        _check(lib().np_hip_index_capacity(self._h, C.byref(d), C.byref(t)))
        return int(d.value), int(t.value)

    @classmethod
    def from_arrays(cls, centroids, bucket_weights, ivf, ivf_lengths, doc_lengths, codes, residuals, nbits,
                    num_documents_total=None, doc_begin=0, **opts) -> "MmapIndex":
        cen = np.ascontiguousarray(centroids, np.float32)
        w = np.ascontiguousarray(bucket_weights, np.float32)
        ivf = np.ascontiguousarray(ivf, np.int64)
        il = np.ascontiguousarray(ivf_lengths, np.int32)
        dl = np.ascontiguousarray(doc_lengths, np.int64)
        cd = np.ascontiguousarray(codes, np.int64)
        rs = np.ascontiguousarray(residuals, np.uint8)
        if cen.ndim != 2:
            raise ShapeError("centroids must be [K, dim]")
        a = np_index_arrays(dl.size if num_documents_total is None else num_documents_total, doc_begin, dl.size,
                            cen.shape[0], cen.shape[1], int(nbits), _ptr(cen), _ptr(w), _ptr(ivf), _ptr(il),
                            _ptr(dl), _ptr(cd), _ptr(rs))
        h = C.c_void_p()
        o = _opts(**opts)
        _check(lib().np_hip_index_from_arrays(C.byref(a), C.byref(o), C.byref(h)))
        return cls(h, "<arrays>")

    @classmethod
    def synth(cls, spec, centroids=None, **opts) -> "MmapIndex":
        """Seeded synthetic corpus generated in HBM (spec: next_plaid_amd.synth.SynthSpec)."""
        from . import synth as S
        cen = np.ascontiguousarray(S.centroids(spec) if centroids is None else centroids, np.float32)
        _, w = S.bucket_tables(spec)
        w = np.ascontiguousarray(w, np.float32)
        lt = None if spec.len_table is None else np.ascontiguousarray(spec.len_table, np.int32)
        s = np_synth_spec(spec.num_docs, spec.num_centroids, spec.dim, spec.nbits, spec.doc_len_min,
                          spec.doc_len_max, spec.n_topics, spec.rand256, spec.seed, _ptr(cen), _ptr(w),
                          None if lt is None else _ptr(lt), 0 if lt is None else int(lt.size))
        h = C.c_void_p()
        o = _opts(**opts)
        _check(lib().np_hip_index_synth(C.byref(s), C.byref(o), C.byref(h)))
        return cls(h, "<synth>")

    def tune(self, name: str, value: int):
        """Kernel-selection knob on a live handle (np_hip_index_tune): sweep tools / variant parity tests."""
        _check(lib().np_hip_index_tune(self._h, name.encode(), int(value)))

    def close(self):
        h, self._h = self._h, None
        if h:
            lib().np_hip_index_close(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- accessors (index.rs:1290-1312) ---------------------------------------------------------------
    def num_documents(self):
        return int(self._info.num_documents)

    def num_embeddings(self):
        return int(self._info.num_embeddings)

    def num_partitions(self):
        return int(self._info.num_partitions)

    def avg_doclen(self):
        return float(self._info.avg_doclen)

    def embedding_dim(self):
        return int(self._info.embedding_dim)

    @property
    def info(self) -> np_info:
        return self._info

    def workspace_bytes(self) -> int:
        """The LIVE per-context scratch budget (np_info.workspace_bytes, ABI v5): the default one shrinks when another
        tenant of the device leaves less room than at open and grows back towards its open value afterwards."""
        live = np_info()
        _check(lib().np_hip_index_info(self._h, C.byref(live)))
        return int(live.workspace_bytes)

    # -- metadata columns and filters ---------------------------------------------------------------------
    def set_columns(self, columns: dict, text_on_device=()):
        """np_hip_index_set_columns: the handle's metadata columns, name -> one entry per document of the WHOLE index (a
        sharded handle keeps its slice).  Integer and bool arrays become I64, float arrays F64, string sequences
        dictionary codes (the dictionary, the distinct non-null strings sorted by their UTF-8 bytes, stays on this object in
        self.schema).  None entries, numpy masked entries and NaN are NULL.  Replaces any earlier set; {} drops them.  A
        length other than num_documents() is a ShapeError.  Needs exclusive access to the handle, as reload() does.

        text_on_device names text columns whose dictionary strings are kept in HBM too (np_hip_index_set_column_text): over
        those, `col REGEXP ?`, `col NOT REGEXP ?` and `col LIKE ?` run on the device as byte DFAs (regexes.py) and
        match_text() answers for the dictionary directly.  Their strings must be UTF-8."""
        from . import filters as F
        sch = F.make_schema(dict(columns), self.num_documents(), text_on_device)
        cols = (np_column * max(len(sch), 1))()
        for c in sch.columns.values():
            cols[c.index] = np_column(c.type, 0, c.data.ctypes.data, None if c.valid is None else c.valid.ctypes.data)
        _check(lib().np_hip_index_set_columns(self._h, cols, len(sch)))
        try:
            for c in sch.columns.values():
                if c.text_on_device and c.dictionary:   # (an empty dictionary has no text: the compiler emits no MATCH over it)
                    text, off = c.text_arrays()
                    _check(lib().np_hip_index_set_column_text(self._h, c.index, text.ctypes.data if text.size else None,
                                                              _ptr(off), len(c.dictionary)))
        except Exception:
            # the columns without their text would disagree with the schema: the handle is left without columns
            lib().np_hip_index_set_columns(self._h, None, 0)
            self.schema = None
            lib().np_hip_index_info(self._h, C.byref(self._info))
            raise
        self.schema = sch if len(sch) else None
        _check(lib().np_hip_index_info(self._h, C.byref(self._info)))

    def get_column(self, name: str):
        """np_hip_index_get_column: the rows of column `name` as the handle holds them, read back from HBM: (data, valid) with
        data int64 / float64 / int32 codes by the column's type and valid a uint8 array, 0 = NULL, or None where the column
        has no validity bitmap."""
        from . import filters as F
        if self.schema is None or name not in self.schema:
            raise F.FilterError(f"unknown column '{name}'")
        col = self.schema[name]
        dtype = {F.NP_COL_I64: np.int64, F.NP_COL_F64: np.float64, F.NP_COL_CODE: np.int32}[col.type]
        n = int(self._info.shard_doc_end - self._info.shard_doc_begin)
        data, valid = np.zeros(n, dtype), np.zeros(n, np.uint8)
        typ, has = C.c_int32(-1), C.c_int32(0)
        _check(lib().np_hip_index_get_column(self._h, col.index, _ptr(data) if n else None, _ptr(valid) if n else None,
                                             C.byref(typ), C.byref(has)))
        if typ.value != col.type:
            raise NextPlaidError(f"column '{name}' has type {typ.value} on the handle, {col.type} in the schema")
        return data, (valid if has.value else None)

    def get_groups(self) -> np.ndarray:
        """np_hip_index_get_groups: the group id of every document, int32, read back from HBM."""
        out = np.zeros(self.num_documents(), np.int32)
        _check(lib().np_hip_index_get_groups(self._h, _ptr(out) if out.size else None))
        return out

    def match_text(self, column: str, patterns, like: bool = False):
        """np_hip_text_match: for every pattern (a REGEXP pattern of regexes.py's dialect, a LIKE pattern with like=True, or a
        regexes.Dfa) a boolean array over the dictionary of `column` (set_columns(..., text_on_device=[column])): entry c =
        the string with code c matches.  The report of the call is in self.last_match_report."""
        from . import filters as F, regexes as R
        if self.schema is None or column not in self.schema:
            raise F.FilterError(f"unknown column '{column}'")
        col = self.schema[column]
        if not col.text_on_device:
            raise F.FilterError(f"column '{column}' has no text on the device (set_columns(..., text_on_device=['{column}']))")
        dfas = [p if isinstance(p, R.Dfa) else R.compile_like(p) if like else
                R.compile_regex(p, col.first_non_ascii is None, first_non_ascii=col.first_non_ascii) for p in patterns]
        n = len(col.dictionary)
        if n == 0:
            return [np.zeros(0, bool) for _ in dfas]
        bits = self.text_match_raw(col.index, [d.pack() for d in dfas], n)
        return [np.unpackbits(row.view(np.uint8), bitorder="little")[:n].astype(bool) for row in bits]

    def set_column_text_raw(self, column_index: int, strings):
        """np_hip_index_set_column_text as it is: byte strings by code for column `column_index` ([] drops the text)."""
        strings = [bytes(s) for s in strings]
        off = np.zeros(len(strings) + 1, np.int64)
        np.cumsum([len(s) for s in strings], out=off[1:])
        text = np.frombuffer(b"".join(strings), np.uint8)
        _check(lib().np_hip_index_set_column_text(self._h, int(column_index), text.ctypes.data if text.size else None, _ptr(off),
                                                  len(strings)))
        _check(lib().np_hip_index_info(self._h, C.byref(self._info)))

    def text_match_raw(self, column_index: int, packed, n_strings: int):
        """np_hip_text_match as it is: packed DFAs (u32 word arrays) -> u32 [n_dfas][ceil(n_strings / 32)]."""
        words = [np.ascontiguousarray(w, np.uint32) for w in packed]
        arr = (np_dfa * max(len(words), 1))(*[np_dfa(w.ctypes.data, w.size) for w in words])
        bits = np.zeros((len(words), (int(n_strings) + 31) // 32), np.uint32)
        rep = np_match_report()
        _check(lib().np_hip_text_match(self._h, int(column_index), arr, len(words), _ptr(bits) if bits.size else None,
                                       C.byref(rep)))
        self.last_match_report = rep.as_dict()
        return bits

    def _schema(self):
        """The columns filters compile against: the handle's, or none (every column name is then unknown)"""
        from . import filters as F
        return self.schema if self.schema is not None else F.Schema()

    def _filters(self, filters, n_queries):
        progs, qf = pack_filters(filters, n_queries, self._schema())
        return _CFilters(progs), qf

    def filter_ids(self, filters, counts_only: bool = False):
        """np_hip_filter_eval: for every filter -- a (condition, params) pair, a condition string or a CompiledFilter -- the
        global ids of the documents it selects (those this handle holds), ascending, as one int64 array each.  With
        counts_only the arrays are not fetched and the counts come back instead."""
        sch = self._schema()
        progs = [_compiled(f, sch) for f in filters]
        cf = _CFilters(progs)
        off = np.zeros(len(progs) + 1, np.int64)
        _check(lib().np_hip_filter_eval(self._h, cf.arr, cf.n, None, 0, _ptr(off)))
        if counts_only:
            return np.diff(off)
        ids = np.zeros(max(int(off[-1]), 1), np.int64)
        _check(lib().np_hip_filter_eval(self._h, cf.arr, cf.n, _ptr(ids), ids.size, _ptr(off)))
        return [ids[off[j]: off[j + 1]].copy() for j in range(len(progs))]

    def filter_eval_raw(self, compiled, ids_capacity: int, want_ids: bool = True):
        """np_hip_filter_eval as it is: (rc, offsets, ids) for CompiledFilters and a caller-chosen ids_capacity."""
        cf = _CFilters(list(compiled))
        off = np.full(cf.n + 1, -1, np.int64)
        ids = np.zeros(max(int(ids_capacity), 1), np.int64)
        rc = lib().np_hip_filter_eval(self._h, cf.arr, cf.n, _ptr(ids) if want_ids else None, int(ids_capacity), _ptr(off))
        return rc, off, ids

    def search_batch_filtered(self, queries, params: "SearchParameters", compiled, query_filter, parallel: bool = True):
        """np_hip_search_batch_filtered as it is: CompiledFilters and the queries' map (-1 = none) reach the library as given."""
        flat, off = self._pack(queries)
        B = len(queries)
        rows = _ResultRows(B, max(int(params.top_k), 0))
        p = params._c()
        scope = _filters_as_given(compiled, query_filter, B)
        st = np_stats()
        rc = lib().np_hip_search_batch_filtered(self._h, _ptr(flat), _ptr(off), B, self.embedding_dim(), C.byref(p),
                                                *scope.filter_args, _ptr(scope.qmap), *rows.ptrs(), C.byref(st))
        failed = _failed_batch(rc, parallel, B)
        if failed is not None:
            return failed
        self.last_stats = st.as_dict()
        return rows.results()

    def search_exact_filtered(self, queries, top_k: int, precision: int, compiled, query_filter):
        """np_hip_search_exact_filtered as it is."""
        flat, off = self._pack(queries)
        B = len(queries)
        rows = _ResultRows(B, max(int(top_k), 1))
        scope = _filters_as_given(compiled, query_filter, B)
        st = np_stats()
        _check(lib().np_hip_search_exact_filtered(self._h, _ptr(flat), _ptr(off), B, self.embedding_dim(), int(top_k),
                                                  int(precision), *scope.filter_args, _ptr(scope.qmap), *rows.ptrs(),
                                                  C.byref(st)))
        self.last_stats = st.as_dict()
        return rows.results()

    # -- keyword and hybrid search ------------------------------------------------------------------------
    def set_text(self, data, _entry="np_hip_index_set_text"):
        """np_hip_index_set_text: the handle's keyword index from a text.TextIndexData (its vocabulary stays on this object
        in self.text); None drops it.  Document i of the FTS5 table is document i of the index.  Needs exclusive access to
        the handle, as set_columns does."""
        fn = getattr(lib(), _entry)
        if data is None:
            _check(fn(self._h, None))
        else:
            off = np.ascontiguousarray(data.term_offsets, np.int64)
            doc = np.ascontiguousarray(data.inst_doc, np.int64)
            pos = np.ascontiguousarray(data.inst_pos, np.int32)
            t = np_text_index(len(data.terms), off.ctypes.data, doc.ctypes.data if doc.size else None,
                              pos.ctypes.data if pos.size else None, int(data.n_rows))
            _check(fn(self._h, C.byref(t)))
        old = getattr(self, "text", None)
        if getattr(old, "resident", False) and old is not data:
            old.invalidate()
        self.text = data
        _check(lib().np_hip_index_info(self._h, C.byref(self._info)))

    def build_text(self, texts, tokenizer: str = "unicode61", max_token_bytes: int | None = None, resident: bool = False,
                   utf8: bool | None = None, unicode_planes: int | None = None):
        """set_text from the documents' raw text, tokenised, numbered and sorted on this handle's device
        (text.TextIndexData.from_texts_device); returns the TextIndexData, which set_text_shard takes unchanged.

        resident=True keeps the build in HBM: np_hip_text_build (the fallback documents through SQLite, as ever),
        np_hip_text_build_sizes and np_hip_index_set_text_build, which derives the postings by kernels and takes the
        positions as they lie.  Only the vocabulary is fetched.  Returns (and leaves in self.text) a
        text.ResidentTextIndexData: terms, vocab, n_rows and tokenizer as before, term_offsets / inst_doc / inst_pos
        fetched from the handle on first access.  Searches on other threads go on; the caller needs no lock.

        utf8=True tokenises UTF-8 text on the device (text.unicode61_table(unicode_planes), see from_texts_device); None
        takes the handle's text_utf8 / text_unicode_planes, which every update of the keyword index that has no argument
        of its own uses too (append / append_arrays / update_resident with rows.texts)."""
        from . import text as T
        utf8 = self.text_utf8 if utf8 is None else bool(utf8)
        unicode_planes = self.text_unicode_planes if unicode_planes is None else int(unicode_planes)
        if not resident:
            data = T.TextIndexData.from_texts_device(texts, tokenizer, device=int(self._info.device),
                                                     max_token_bytes=max_token_bytes, utf8=utf8, unicode_planes=unicode_planes)
            self.set_text(data)
            return data
        if tokenizer not in T.TOKENIZERS:
            raise ValueError(f"unknown tokenizer {tokenizer!r}")
        L = lib()
        texts = list(texts)
        raws = [T.prepare_document_text(t, tokenizer).encode("utf-8") for t in texts]
        off = np.zeros(len(raws) + 1, np.int64)
        if raws:
            off[1:] = np.cumsum([len(r) for r in raws])
        raw = np.frombuffer(b"".join(raws), np.uint8)

        def tokenize_fallback(ids):
            return T._tokenize_rows(T.TextIndexData, [texts[int(i)] for i in ids], [int(i) for i in ids], tokenizer)

        code = NP_TOK_TRIGRAM if T.TOKENIZERS[tokenizer] == "trigram" else NP_TOK_UNICODE61
        h, fb, rep = _text_build_open(L, raw, off, code, tokenize_fallback, int(self._info.device), int(max_token_bytes or 0), 0, 0, 0,
                                      utf8, unicode_planes)
        return self._install_text_build(h, tokenizer, rep.as_dict(), fb)

    def _install_text_build(self, h, tokenizer, report, fallback):
        """np_hip_text_build_sizes, np_hip_index_set_text_build and the vocabulary of a build; frees it either way."""
        from . import text as T
        L = lib()
        try:
            _check(L.np_hip_text_build_sizes(h, None, None, None, None))
            _check(L.np_hip_index_set_text_build(self._h, h))
            terms, n_rows, n_inst = _text_build_vocab(L, h)
        finally:
            L.np_hip_text_build_free(h)
        old = getattr(self, "text", None)
        if getattr(old, "resident", False):
            old.invalidate()
        if n_inst == 0 and n_rows == 0:   # (no instances and no rows drop the keyword index, as set_text does)
            self.text = None
        else:
            self.text = T.ResidentTextIndexData(tokenizer, terms, n_rows, self._text_fetcher(), report,
                                                [int(i) for i in fallback])
        _check(L.np_hip_index_info(self._h, C.byref(self._info)))
        return self.text

    def text_sizes(self) -> dict:
        """np_hip_index_text_sizes: n_terms, n_postings, n_instances, n_rows and n_docs of the handle's keyword index."""
        v = [C.c_int64() for _ in range(5)]
        _check(lib().np_hip_index_text_sizes(self._h, *(C.byref(x) for x in v)))
        return dict(zip(("n_terms", "n_postings", "n_instances", "n_rows", "n_docs"), (int(x.value) for x in v)))

    def _fetch_text_arrays(self):
        """np_hip_index_get_text: (term_offsets, inst_doc, inst_pos) regenerated from the handle's keyword index."""
        z = self.text_sizes()
        off = np.zeros(z["n_terms"] + 1, np.int64)
        doc, pos = np.zeros(max(z["n_instances"], 1), np.int64), np.zeros(max(z["n_instances"], 1), np.int32)
        _check(lib().np_hip_index_get_text(self._h, _ptr(off), _ptr(doc), _ptr(pos)))
        return off, doc[: z["n_instances"]], pos[: z["n_instances"]]

    def _text_fetcher(self):
        """_fetch_text_arrays for a ResidentTextIndexData to keep: it holds the handle weakly, so that self.text and the
        handle form no cycle and the handle closes when its last owner lets go."""
        import weakref
        ref = weakref.ref(self)

        def fetch():
            ix = ref()
            if ix is None or not ix._h:
                raise ValueError("the handle of this keyword index is closed: its arrays cannot be fetched any more")
            return ix._fetch_text_arrays()
        return fetch

    def get_text(self):
        """The handle's keyword index read back from HBM (np_hip_index_get_text) as a plain text.TextIndexData with the
        handle's vocabulary (self.text's)."""
        from . import text as T
        if self.text is None:
            raise ValueError("get_text: the handle has no keyword index")
        z = self.text_sizes()
        if z["n_terms"] != len(self.text.terms):
            raise ValueError(f"get_text: the handle's keyword index holds {z['n_terms']} terms, self.text {len(self.text.terms)}")
        off, doc, pos = self._fetch_text_arrays()
        return T.TextIndexData(self.text.tokenizer, list(self.text.terms), off, doc, pos, z["n_rows"], dict(self.text.vocab))

    def get_text_layout(self) -> dict:
        """np_hip_index_get_text_layout: the keyword index as it lies in HBM -- post_off i64 [n_terms + 1], post_doc /
        post_tf i32 and post_first i64 [n_postings], doc_len i32 [n_docs]."""
        z = self.text_sizes()
        P, N = z["n_postings"], z["n_docs"]
        out = dict(post_off=np.zeros(z["n_terms"] + 1, np.int64), post_doc=np.zeros(max(P, 1), np.int32),
                   post_tf=np.zeros(max(P, 1), np.int32), post_first=np.zeros(max(P, 1), np.int64),
                   doc_len=np.zeros(max(N, 1), np.int32))
        _check(lib().np_hip_index_get_text_layout(self._h, *(_ptr(out[k]) for k in ("post_off", "post_doc", "post_tf",
                                                                                    "post_first", "doc_len"))))
        for k in ("post_doc", "post_tf", "post_first"):
            out[k] = out[k][:P]
        out["doc_len"] = out["doc_len"][:N]
        return out

    def _merge_text_resident(self, new_texts=(), delete=(), replace=None, renumber: bool = True, utf8=None, unicode_planes=None):
        """The first half of a resident update: np_hip_index_text_merge of the handle's keyword index with the batch.
        Returns (the result build, the report, the fallback ids); the handle is untouched.  The caller installs or frees."""
        base = self.text
        remap, delta_ids, n_rows_out, raw, off, code, tokenize_fallback = base._update_plan(new_texts, delete, replace, renumber, None)
        return text_merge_resident(self._h, [t.encode("utf-8") for t in base.terms], remap, delta_ids, n_rows_out, raw, off, code,
                                   tokenize_fallback, device=int(self._info.device),
                                   utf8=self.text_utf8 if utf8 is None else bool(utf8),
                                   unicode_planes=self.text_unicode_planes if unicode_planes is None else int(unicode_planes))

    def update_text(self, new_texts=(), delete=(), replace=None, renumber: bool = True, base=None, resident: bool = False,
                    utf8: bool | None = None, unicode_planes: int | None = None):
        """The keyword index kept current (text.TextIndexData.updated, on this handle's device): `new_texts` appended,
        the rows `delete` removed, the rows of `replace` ({id: text}) given new text; renumber=True numbers the survivors
        densely, as the document ids are after delete() / update().  `base` defaults to self.text; update() and reload()
        drop it, so pass the TextIndexData kept from before them.  Calls set_text with the result and returns it
        (set_text_shard takes it unchanged).  A refused call leaves the previous keyword index in place.

        resident=True updates the handle's keyword index from itself: the batch is built on the device,
        np_hip_index_text_merge reads the base where it lies and np_hip_index_set_text_build installs the result; no
        instance array crosses the bus.  The base IS the handle, so `base=` is refused.  Returns a
        text.ResidentTextIndexData (see build_text); the arrays of the object it replaces are INVALIDATED unless they were
        fetched before.

        utf8 / unicode_planes: build_text's, for the batch (None = the handle's text_utf8 / text_unicode_planes)."""
        if resident:
            if base is not None:
                raise ValueError("update_text: base= is refused with resident=True: the base is the handle's keyword index")
            if self.text is None:
                raise ValueError("update_text: the handle has no keyword index")
            h, rep, fb = self._merge_text_resident(new_texts, delete, replace, renumber, utf8, unicode_planes)
            return self._install_text_build(h, self.text.tokenizer, rep, fb)
        base = self.text if base is None else base
        if base is None:
            raise ValueError("update_text: the handle has no keyword index and no base was given")
        data = base.updated(new_texts, delete=delete, replace=replace, renumber=renumber, device=int(self._info.device),
                            utf8=self.text_utf8 if utf8 is None else bool(utf8),
                            unicode_planes=self.text_unicode_planes if unicode_planes is None else int(unicode_planes))
        self.set_text(data)
        return data

    def _load_text(self, index_path, what, set_text):
        from . import text as T
        data = T.TextIndexData.from_sqlite(os.path.join(index_path or self._dir(what), "metadata.db"))
        set_text(data)
        return data

    def load_text(self, index_path: str | None = None):
        """set_text from the metadata.db of an index directory (the crate's METADATA_FTS table); returns the TextIndexData."""
        return self._load_text(index_path, "load_text", self.set_text)

    def set_text_shard(self, data):
        """np_hip_index_set_text_shard: set_text for a handle that holds a document shard.  `data` is the WHOLE table's
        TextIndexData, the same on every rank (global document ids); the handle keeps the postings of its own documents and
        the whole table's row count, token count and document frequencies.  On an unsharded handle it is set_text.  The
        searches over it are dist.CShardedSearcher's text_search and search_hybrid."""
        self.set_text(data, _entry="np_hip_index_set_text_shard")

    def load_text_shard(self, index_path: str | None = None):
        """set_text_shard from the metadata.db of an index directory; returns the (whole table's) TextIndexData."""
        return self._load_text(index_path, "load_text_shard", self.set_text_shard)

    def _text_queries(self, text_queries, empty_matches_nothing: bool, full_grammar: bool = False):
        """Strings are compiled against self.text (full_grammar: by text.compile_text_expr, into TextExpr trees), TextQuery
        and TextExpr objects pass; '' (text_search.rs:1247: an empty query has an empty result) -> None, or the query that
        matches nothing."""
        from . import text as T
        out = []
        for q in text_queries:
            if isinstance(q, str):
                if q == "":
                    q = T.TextQuery.from_phrases(T.MATCH_NOTHING) if empty_matches_nothing else None
                else:
                    if getattr(self, "text", None) is None:
                        raise ValueError("the handle has no keyword index (set_text / load_text)")
                    q = T.compile_text_expr(q, self.text) if full_grammar else T.compile_text_query(q, self.text)
            out.append(q)
        return out

    def _scope(self, B, subset, subsets, filters, what) -> _Scope:
        """The per-query scope arguments of the method `what` as a _Scope: the one place where filters= / subsets= /
        subset= are told apart and refused together."""
        if filters is not None:
            if subset is not None or subsets is not None:
                raise ValueError(f"{what} takes filters= or subset= / subsets=, not both")
            cf, qf = self._filters(filters, B)
            return _Scope("filters", None, None, cf.n, qf, cf)
        if subsets is not None:
            if subset is not None:
                raise ValueError(f"{what} takes subset= (one for the batch) or subsets= (one per query), not both")
            sid, soff, qsub = pack_subsets(subsets, B)
            return _Scope("subsets", sid, soff, soff.size - 1, qsub, None)
        if subset is not None:
            sid = np.ascontiguousarray(subset, np.int64).reshape(-1)
            return _Scope("subset", sid, np.array([0, sid.size], np.int64), 1, np.zeros(max(B, 1), np.int32), None)
        return _Scope(None, None, None, 0, None, None)

    def _live_text_queries(self, text_queries, subset, subsets, filters, full_grammar: bool = False):
        """The prologue of text_search, here and over the shards: (B, live, their compiled queries, the scope of those).  An
        empty query is not searched: `live` lists the positions of the others, which are all the library sees."""
        if isinstance(text_queries, str):
            text_queries = [text_queries]
        qs = self._text_queries(list(text_queries), False, full_grammar)
        live = [i for i, q in enumerate(qs) if q is not None]
        scope = self._scope(len(qs), subset, subsets, filters, "text_search").of_rows(live)
        return len(qs), live, [qs[i] for i in live], scope

    def _hybrid_compiled(self, B, text_queries, full_grammar: bool = False):
        """The text half of the hybrid-shaped calls, compiled, one per query: an empty one matches nothing (its keyword list
        is empty)."""
        qs = self._text_queries(list(text_queries), True, full_grammar)
        if len(qs) != B:
            raise ValueError(f"{B} queries and {len(qs)} text queries")
        return qs

    def _hybrid_text_queries(self, B, text_queries):
        """... in ctypes form, for the calls that take flat queries only: the grouped ones (a text.TextExpr is refused by
        name)."""
        return _CTextQueries(self._hybrid_compiled(B, text_queries))

    def text_search(self, text_queries, top_k: int, subset=None, subsets=None, filters=None, full_grammar: bool = False):
        """np_hip_text_search: BM25 keyword search with SQLite FTS5's results (text_search.rs:1246-1342) -- for every query
        the top_k documents by -bm25(), f64 score descending, ties by ascending id.  A query is FTS5 text (compiled by
        text.compile_text_query against the handle's keyword index) or a text.TextQuery; '' returns an empty result.  Scope:
        `subset`, `subsets` or `filters` as search_exact takes them.  Returns QueryResults.

        A text.TextExpr -- a tree with FTS5's NOT, AND, OR, parentheses and prefixes -- among the queries sends the whole
        batch to np_hip_text_search_expr (flat queries are lifted to trees and keep their bytes); full_grammar=True compiles
        strings with text.compile_text_expr into such trees.  The default refuses what compile_text_query refuses."""
        B, live, qs, scope = self._live_text_queries(text_queries, subset, subsets, filters, full_grammar)
        n = len(live)
        tq, form = _c_text_queries(qs)
        rows = _ResultRows(n, max(int(top_k), 1))
        st = np_stats()
        if scope.cf is not None:
            _check(getattr(lib(), f"np_hip_text_search{form}_filtered")(self._h, tq.arr, n, int(top_k), *scope.filter_args,
                                                                        _ptr(scope.qmap), *rows.ptrs(), C.byref(st)))
        else:
            _check(getattr(lib(), f"np_hip_text_search{form}")(self._h, tq.arr, n, int(top_k), *scope.csr, *rows.ptrs(),
                                                               C.byref(st)))
        self.last_stats = st.as_dict()
        return rows.results(live, B)

    def search_hybrid(self, queries, text_queries, params: "SearchParameters", alpha: float = 0.75,
                      fusion: str = "relative_score", fetch_k: int | None = None, subset=None, subsets=None, filters=None,
                      full_grammar: bool = False):
        """np_hip_search_hybrid: the /search handler's hybrid request (search.rs:134-375) in one call -- the semantic pass and
        the keyword pass with top_k = fetch_k (default: the handler's 3 * params.top_k) and their fusion ("relative_score",
        the default, or "rrf") to params.top_k, on the device.  Query i gets what fuse(...) returns for search_batch and
        text_search with top_k = fetch_k.  An empty text query contributes an empty keyword list.  Returns QueryResults.
        Tree queries (a text.TextExpr among them, or strings under full_grammar=True) go to np_hip_search_hybrid_expr, as
        text_search routes them."""
        queries = list(queries)
        flat, off = self._pack(queries)
        B = len(queries)
        tq, form = _c_text_queries(self._hybrid_compiled(B, text_queries, full_grammar))
        fk = 3 * int(params.top_k) if fetch_k is None else int(fetch_k)
        scope = self._scope(B, subset, subsets, filters, "search_hybrid")
        rows = _ResultRows(B, max(int(params.top_k), 1))
        p = params._c()
        st = np_stats()
        _check(getattr(lib(), f"np_hip_search_hybrid{form}")(self._h, _ptr(flat), _ptr(off), B, self.embedding_dim(), C.byref(p),
                                                             tq.arr, fk, float(alpha), _fusion_mode(fusion), *scope.csr,
                                                             *scope.filter_args, *rows.ptrs(), C.byref(st)))
        self.last_stats = st.as_dict()
        return rows.results()

    # -- grouped search -----------------------------------------------------------------------------------
    def set_groups(self, keys, n_groups: int | None = None):
        """np_hip_index_set_groups: the group of every document of the WHOLE index, kept in HBM.  `keys` has one entry per
        document -- ints, strings or None: dense ids follow the sorted distinct non-null values, which stay on this object as
        self.group_values, and all None entries form one group with the last id (SQLite's GROUP BY rule) -- or, with
        n_groups=, it is a ready int32 array of ids in [0, n_groups).  None or an empty sequence drops the groups.  A length
        other than num_documents() is a ShapeError.  A sharded handle is refused.  reload() (and so update()) leaves the
        handle without groups, as it leaves it without columns.  Needs exclusive access to the handle, as set_columns does."""
        if keys is None or len(keys) == 0:
            _check(lib().np_hip_index_set_groups(self._h, None, 0, 0))
            self.group_values = None
        else:
            if n_groups is not None:
                ids, values, n = np.ascontiguousarray(keys, np.int32).reshape(-1), None, int(n_groups)
            else:
                ids, values, n = group_ids_of_keys(keys)
            _check(lib().np_hip_index_set_groups(self._h, _ptr(ids), ids.size, n))
            self.group_values = values
        _check(lib().np_hip_index_info(self._h, C.byref(self._info)))

    def group_count(self) -> int:
        """np_hip_index_group_count: n_groups, 0 when no groups are set."""
        return int(lib().np_hip_index_group_count(self._h))

    def collapse_raw(self, ids, scores, counts, stride: int, top_k: int, group_size: int):
        """np_hip_collapse as it is: ids i64 [B * stride], scores f32 likewise or None, counts i32 [B] reach the library as
        given, so its checks answer.  Returns the padded outputs (ids, scores or None, group, members, total, counts)."""
        cnt = np.ascontiguousarray(counts, np.int32).reshape(-1)
        B = cnt.size
        fi = np.ascontiguousarray(ids, np.int64).reshape(-1)
        fs = None if scores is None else np.ascontiguousarray(scores, np.float32).reshape(-1)
        if fi.size < B * max(int(stride), 0) or (fs is not None and fs.size < fi.size):
            raise ValueError(f"{B} lists of stride {stride} need {B * stride} entries")
        out = _group_outputs(B, max(int(top_k), 1), max(int(group_size), 1), fs is not None)
        _check(lib().np_hip_collapse(self._h, int(top_k), int(group_size), B, _ptr(fi), _ptr(fs), _ptr(cnt), int(stride),
                                     *[_ptr(o) for o in out]))
        return out

    def search_grouped(self, queries, params: "SearchParameters", group_size: int = 1, pool_k: int | None = None, subset=None,
                       subsets=None, filters=None, raw: bool = False):
        """np_hip_search_batch_grouped: the top params.top_k GROUPS (set_groups) with their best group_size documents each --
        the search pass with top_k = pool_k and the collapse of its ranked lists, on the device; neither leaves HBM.  Query i
        gets collapse(search_batch(top_k = pool_k)).  pool_k defaults to ColGREP's max(20 top_k, 200), inside the index and
        the entry's limit of 16384.  Scope: `subset`, `subsets` or `filters` as search_batch takes them.  Returns per query a
        list of groups (group_id, passage_ids, scores, total); raw=True returns the padded output arrays instead."""
        queries = list(queries)
        flat, off = self._pack(queries)
        B = len(queries)
        pk = default_pool_k(params.top_k, self.num_documents()) if pool_k is None else int(pool_k)
        scope = self._scope(B, subset, subsets, filters, "search_grouped")
        k, g = max(int(params.top_k), 1), max(int(group_size), 1)
        out = _group_outputs(B, k, g)
        p = params._c()
        st = np_stats()
        _check(lib().np_hip_search_batch_grouped(self._h, _ptr(flat), _ptr(off), B, self.embedding_dim(), C.byref(p), *scope.csr,
                                                 *scope.filter_args, pk, int(group_size), *[_ptr(o) for o in out], C.byref(st)))
        self.last_stats = st.as_dict()
        return out if raw else _groups_of_rows(B, k, g, *out)

    def search_hybrid_grouped(self, queries, text_queries, params: "SearchParameters", group_size: int = 1,
                              pool_k: int | None = None, alpha: float = 0.75, fusion: str = "relative_score",
                              fetch_k: int | None = None, subset=None, subsets=None, filters=None):
        """np_hip_search_hybrid_grouped: ColGREP's request -- search_hybrid fused into a pool of pool_k, then collapsed to
        params.top_k groups of at most group_size documents, on the device.  Query i gets collapse(search_hybrid(top_k =
        pool_k)).  fetch_k defaults to min(3 * pool_k, 1024), pool_k to ColGREP's max(20 top_k, 200) inside the index and the
        fusion's limit of 2048.  Returns what search_grouped returns."""
        from . import text as T
        queries = list(queries)
        flat, off = self._pack(queries)
        B = len(queries)
        tq = self._hybrid_text_queries(B, text_queries)
        pk = default_pool_k(params.top_k, self.num_documents(), 2 * T.NP_TEXT_MAX_TOPK) if pool_k is None else int(pool_k)
        fk = min(3 * pk, T.NP_TEXT_MAX_TOPK) if fetch_k is None else int(fetch_k)
        scope = self._scope(B, subset, subsets, filters, "search_hybrid_grouped")
        k, g = max(int(params.top_k), 1), max(int(group_size), 1)
        out = _group_outputs(B, k, g)
        p = params._c()
        st = np_stats()
        _check(lib().np_hip_search_hybrid_grouped(self._h, _ptr(flat), _ptr(off), B, self.embedding_dim(), C.byref(p), tq.arr, fk,
                                                  float(alpha), _fusion_mode(fusion), *scope.csr, *scope.filter_args, pk,
                                                  int(group_size), *[_ptr(o) for o in out], C.byref(st)))
        self.last_stats = st.as_dict()
        return _groups_of_rows(B, k, g, *out)

    # -- search ------------------------------------------------------------------------------------------
    def _pack(self, queries):
        qs = [np.ascontiguousarray(q, np.float32) for q in queries]
        d = self.embedding_dim()
        for q in qs:
            if q.ndim != 2 or q.shape[1] != d:
                raise ShapeError(f"Shape error: query has shape {q.shape}, index dim is {d}")
        off = np.zeros(len(qs) + 1, np.int32)
        if qs:
            off[1:] = np.cumsum([q.shape[0] for q in qs])
        flat = np.concatenate(qs, 0) if qs else np.zeros((0, d), np.float32)
        return np.ascontiguousarray(flat, np.float32), off

    def search(self, query, params: SearchParameters, subset=None, filter=None) -> QueryResult:
        """MmapIndex::search (index.rs:1258-1265); query_id is 0 (search.rs:511-515).  `filter` = (condition, params) over
        the handle's columns in place of a subset (not both)."""
        if filter is not None and subset is not None:
            raise ValueError("search takes subset= or filter=, not both")
        r = self.search_batch([query], params, parallel=False, subset=subset, filters=None if filter is None else [filter])[0]
        r.query_id = 0
        return r

    def search_batch(self, queries, params: SearchParameters, parallel: bool = True, subset=None, subsets=None, filters=None):
        """MmapIndex::search_batch (index.rs:1279-1287).  `parallel` only selects the reference's
        error policy (search.rs:650-674): the GPU path always runs the batch as one pipeline pass.

        `subset` is the crate's argument: one subset for the whole batch.  `subsets` gives every query its own: a sequence
        of len(queries) entries, each None or an array of document ids; query i gets what search(queries[i], params,
        subsets[i]) returns.  Entries that are the same object share one subset (see pack_subsets).

        `filters` gives every query a WHERE condition over the handle's columns instead (set_columns): one entry per query,
        None or (condition, params); the ids are computed on the device and query i gets what subsets=[ids the filter
        selects, ascending] returns.  Equal entries are compiled and evaluated once.  Not together with subset / subsets."""
        queries = list(queries)
        B = len(queries)
        scope = self._scope(B, subset, subsets, filters, "search_batch")
        if scope.form == "filters":
            return self.search_batch_filtered(queries, params, scope.cf, scope.qmap, parallel=parallel)
        if scope.form == "subsets":
            return self.search_batch_csr(queries, params, scope.sid, scope.soff, scope.qmap, parallel=parallel)
        # the crate's own argument, one subset for the batch, stays on the crate's entry: its ids alone, a length of -1 = none
        flat, off = self._pack(queries)
        rows = _ResultRows(B, max(int(params.top_k), 0))
        p = params._c()
        sub = scope.sid
        st = np_stats()
        rc = lib().np_hip_search_batch(self._h, _ptr(flat), _ptr(off), B, self.embedding_dim(), C.byref(p),
                                       _ptr(sub), -1 if sub is None else sub.size, *rows.ptrs(), C.byref(st))
        failed = _failed_batch(rc, parallel, B)
        if failed is not None:
            return failed
        self.last_stats = st.as_dict()
        return rows.results()

    def search_batch_csr(self, queries, params: SearchParameters, subset_ids, subset_offsets, query_subset,
                         parallel: bool = True):
        """np_hip_search_batch_subsets as it is: the batch's distinct subsets in CSR form and the queries' map (-1 = none).
        The arrays reach the library as given (None = NULL; n_subsets = len(subset_offsets) - 1), so its argument checks
        are the ones that answer."""
        flat, off = self._pack(queries)
        B = len(queries)
        rows = _ResultRows(B, max(int(params.top_k), 0))
        p = params._c()
        scope = _csr_as_given(subset_ids, subset_offsets, query_subset, B)
        st = np_stats()
        rc = lib().np_hip_search_batch_subsets(self._h, _ptr(flat), _ptr(off), B, self.embedding_dim(), C.byref(p),
                                               *scope.csr, *rows.ptrs(), C.byref(st))
        failed = _failed_batch(rc, parallel, B)
        if failed is not None:
            return failed
        self.last_stats = st.as_dict()
        return rows.results()

    def search_exact(self, queries, top_k: int, precision: int = 0, subset=None, subsets=None, filters=None):
        """np_hip_search_exact: for every query the true top_k of its scope by exact MaxSim over the decompressed index,
        every document scored (no probe, no candidates).  Scope: the whole handle, `subset` (one for the batch) or
        `subsets` (one entry per query, None or an array of ids, as search_batch takes them through pack_subsets).
        precision 0 = exact f32 (the ground truth), 3 = bf16 MFMA.  Ties in score come back by ascending id.  A single
        [tokens, dim] matrix is the batch of one.  Returns QueryResults."""
        if isinstance(queries, np.ndarray) and queries.ndim == 2:
            queries = [queries]
        queries = list(queries)
        B = len(queries)
        scope = self._scope(B, subset, subsets, filters, "search_exact")
        if scope.form == "filters":   # one WHERE condition per query (None or (condition, params)), as search_batch takes them
            return self.search_exact_filtered(queries, top_k, precision, scope.cf, scope.qmap)
        # search_exact_csr wants exactly one map entry per query: the one-subset map, padded to one entry for an empty
        # batch, goes without its padding
        qsub = None if scope.qmap is None else scope.qmap[:B]
        return self.search_exact_csr(queries, top_k, precision, scope.sid, scope.soff, qsub)

    def search_exact_csr(self, queries, top_k: int, precision: int, subset_ids, subset_offsets, query_subset):
        """np_hip_search_exact as it is: the CSR arrays reach the library as given (None = NULL), so its checks answer."""
        flat, off = self._pack(queries)
        B = len(queries)
        rows = _ResultRows(B, max(int(top_k), 1))
        scope = _csr_as_given(subset_ids, subset_offsets, query_subset, B)
        st = np_stats()
        _check(lib().np_hip_search_exact(self._h, _ptr(flat), _ptr(off), B, self.embedding_dim(), int(top_k), int(precision),
                                         *scope.csr, *rows.ptrs(), C.byref(st)))
        self.last_stats = st.as_dict()
        return rows.results()

    def score_pairs(self, queries, doc_ids, return_matches: bool = True, precision: int = 0):
        """np_hip_score_pairs: the exact MaxSim of given (query, document) pairs and, per query token, its best document
        token.  `doc_ids` has one array of global document ids per query (duplicates allowed, any order).  Returns per query
        (scores f32 [n_i], token_sims f32 [n_i, Lq_i], token_pos i32 [n_i, Lq_i]), or only the scores with
        return_matches=False.  A score is the very bits search_batch / search_exact give the pair at precision 0 and the
        ordered f32 sum of its row of sims; a position is the lowest document-token index that reaches the sim (-1 and -inf
        where no similarity is finite).  A single [tokens, dim] matrix is the batch of one (doc_ids then one array)."""
        if isinstance(queries, np.ndarray) and queries.ndim == 2:
            queries, doc_ids = [queries], [doc_ids]
        queries, doc_ids = list(queries), list(doc_ids)
        if len(doc_ids) != len(queries):
            raise ValueError(f"doc_ids has {len(doc_ids)} entries for {len(queries)} queries")
        lists = [np.ascontiguousarray(d, np.int64).reshape(-1) for d in doc_ids]
        off = np.zeros(len(lists) + 1, np.int64)
        if lists:
            off[1:] = np.cumsum([d.size for d in lists])
        flat_ids = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        return self.score_pairs_csr(queries, flat_ids, off, return_matches, precision)

    def score_pairs_csr(self, queries, pair_docs, pair_offsets, return_matches: bool = True, precision: int = 0):
        """np_hip_score_pairs as it is: query i against pair_docs[pair_offsets[i]:pair_offsets[i + 1]].  The arrays reach the
        library as given (None = NULL), so its checks answer.  Returns what score_pairs returns."""
        flat, qoff = self._pack(queries)
        B = len(queries)
        ids = None if pair_docs is None else np.ascontiguousarray(pair_docs, np.int64).reshape(-1)
        poff = None if pair_offsets is None else np.ascontiguousarray(pair_offsets, np.int64).reshape(-1)
        if poff is not None and poff.size != B + 1:
            raise ValueError(f"pair_offsets has {poff.size} entries for {B} queries")
        n = np.zeros(B, np.int64) if poff is None else np.maximum(np.diff(poff), 0)
        if ids is not None and poff is not None and poff.size and int(poff.max()) > ids.size:
            raise ValueError(f"pair_offsets count {int(poff.max())} pairs, pair_docs has {ids.size}")
        lq = np.diff(qoff).astype(np.int64)
        P, R = int(n.sum()), int((n * lq).sum())
        sc = np.zeros(max(P, 1), np.float32)
        sims = np.zeros(max(R, 1), np.float32) if return_matches else None
        pos = np.zeros(max(R, 1), np.int32) if return_matches else None
        st = np_stats()
        _check(lib().np_hip_score_pairs(self._h, _ptr(flat), _ptr(qoff), B, self.embedding_dim(), int(precision), _ptr(ids),
                                        _ptr(poff), _ptr(sc), _ptr(sims), _ptr(pos), C.byref(st)))
        self.last_stats = st.as_dict()
        out, p0, r0 = [], 0, 0
        for i in range(B):
            ni, li = int(n[i]), int(lq[i])
            s = sc[p0:p0 + ni].copy()
            if return_matches:
                out.append((s, sims[r0:r0 + ni * li].reshape(ni, li).copy(), pos[r0:r0 + ni * li].reshape(ni, li).copy()))
            else:
                out.append(s)
            p0, r0 = p0 + ni, r0 + ni * li
        return out

    # -- adjacent rows ---------------------------------------------------------------------------------------
    def get_document_embeddings(self, doc_id: int) -> np.ndarray:
        """index.rs:1159-1179"""
        embs, lens = self.decompress_documents([doc_id])
        if doc_id < 0 or doc_id >= self.num_documents():
            raise SearchError(f"Search failed: Invalid document ID: {doc_id}")
        return embs

    def decompress_documents(self, doc_ids):
        """index.rs:1197-1245: (embeddings [sum len, dim], lengths)."""
        ids = np.ascontiguousarray(doc_ids, np.int64)
        lens = np.zeros(max(ids.size, 1), np.int64)
        _check(lib().np_hip_decompress_documents(self._h, _ptr(ids), ids.size, None, 0, _ptr(lens)))
        lens = lens[: ids.size]
        total = int(lens.sum())
        out = np.zeros((max(total, 1), self.embedding_dim()), np.float32)
        _check(lib().np_hip_decompress_documents(self._h, _ptr(ids), ids.size, _ptr(out), total, _ptr(lens)))
        return out[:total], lens

    def encode_tokens(self, embeddings, bucket_cutoffs):
        """Index-time encode of a flat [n, dim] batch against this index's codec (codec.rs:297-411,
        index.rs:289-371): (codes i64 [n], packed residuals u8 [n, dim*nbits/8])."""
        x = np.ascontiguousarray(embeddings, np.float32)
        if x.ndim != 2 or x.shape[1] != self.embedding_dim():
            raise ShapeError(f"Shape error: embeddings have shape {x.shape}, index dim is {self.embedding_dim()}")
        nbits = int(self.info.nbits)
        cut = np.ascontiguousarray(bucket_cutoffs, np.float32)
        if cut.size != (1 << nbits) - 1:
            raise CodecError(f"Codec error: bucket_cutoffs has {cut.size} entries, nbits={nbits} needs {(1 << nbits) - 1}")
        n = x.shape[0]
        codes = np.zeros(max(n, 1), np.int64)
        packed = np.zeros((max(n, 1), x.shape[1] * nbits // 8), np.uint8)
        _check(lib().np_hip_encode_tokens(self._h, _ptr(x), n, x.shape[1], _ptr(cut), _ptr(codes), _ptr(packed)))
        return codes[:n], packed[:n]

    def debug_trace(self, query, params: SearchParameters, subset=None) -> dict:
        q = np.ascontiguousarray(query, np.float32)
        if q.ndim != 2 or q.shape[1] != self.embedding_dim():
            raise ShapeError(f"Shape error: query has shape {q.shape}")
        K = self.num_partitions()
        n_loc = int(self._info.shard_doc_end - self._info.shard_doc_begin)
        nsel = max(int(lib().np_hip_n_sel(C.byref(params._c()))), 1)
        cells = np.zeros(max(K, 1), np.int64)
        cand = np.zeros(max(n_loc, 1), np.int64)
        approx = np.zeros(max(n_loc, 1), np.float32)
        sel = np.zeros(nsel, np.int64)
        sel_exact = np.zeros(nsel, np.float32)
        nc, nd, ns = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        p = params._c()
        sub = None if subset is None else np.ascontiguousarray(subset, np.int64)
        _check(lib().np_hip_debug_trace(self._h, _ptr(q), q.shape[0], q.shape[1], C.byref(p), _ptr(sub),
                                        -1 if sub is None else sub.size, _ptr(cells), cells.size, C.byref(nc),
                                        _ptr(cand), _ptr(approx), cand.size, C.byref(nd),
                                        _ptr(sel), _ptr(sel_exact), sel.size, C.byref(ns)))
        return dict(cells=cells[: nc.value].copy(), cand=cand[: nd.value].copy(), approx=approx[: nd.value].copy(),
                    sel=sel[: ns.value].copy(), sel_exact=sel_exact[: ns.value].copy())

    def export(self) -> dict:
        """Shard arrays back on the host in the on-disk dtypes (bench cpu_baseline, generator tests)."""
        n_loc = int(self._info.shard_doc_end - self._info.shard_doc_begin)
        T = int(self._info.shard_embeddings)
        pd = self.embedding_dim() * int(self._info.nbits) // 8
        K = self.num_partitions()
        dl = np.zeros(max(n_loc, 1), np.int64)
        cd = np.zeros(max(T, 1), np.int64)
        rs = np.zeros((max(T, 1), pd), np.uint8)
        ivf = np.zeros(max(int(lib().np_hip_index_ivf_size(self._h)), 1), np.int64)
        il = np.zeros(max(K, 1), np.int32)
        _check(lib().np_hip_index_export(self._h, _ptr(dl), _ptr(cd), _ptr(rs), _ptr(ivf), _ptr(il)))
        return dict(doc_lengths=dl[:n_loc], codes=cd[:T], residuals=rs[:T], ivf=ivf[: int(il[:K].sum())],
                    ivf_lengths=il[:K], nbits=int(self._info.nbits))
