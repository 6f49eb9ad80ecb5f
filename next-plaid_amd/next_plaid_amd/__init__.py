"""MI355X-native PLAID search path for next-plaid: Python host mirror of the crate API.

`MmapIndex.load / search / search_batch`, `SearchParameters`, `QueryResult` keep the names,
argument meaning and error behaviour of next-plaid/src/{index,search,error}.rs and forward to
the C ABI in include/nextplaid_hip.h (libnextplaid_hip.so, hand-written HIP for gfx950).
There is no CPU fallback in this package: if the HIP library or a GPU is missing, calls raise.
"""
from .api import (  # noqa: F401
    MmapIndex, SearchParameters, QueryResult, NextPlaidError, IndexLoadError, SearchError,
    ShapeError, CodecError, DeviceUnavailableError, device_count, library_path, rerank_maxsim, probe_index_dir, write_index_dir,
    IndexConfig, IndexCreationError, kmeans, kmeans_plan, compute_kmeans, estimate_num_partitions, prepare_codec_artifacts,
    UpdateConfig, update_index_dir, update_append_dir, delete_from_index_dir, pool_document_embeddings, pooled_lengths,
    pack_filters, fuse, fuse_rrf, fuse_relative_score, collapse, group_ids_of_keys, default_pool_k,
)
from .filters import compile_filter, make_schema, CompiledFilter, FilterError, Schema  # noqa: F401
from .regexes import compile_regex, compile_like, Dfa  # noqa: F401
from .text import (  # noqa: F401
    TextIndexData, TextQuery, TextQueryError, compile_text_query, sanitize_fts5_query, sanitize_fts5_query_or,
    tokenize_identifiers,
)
