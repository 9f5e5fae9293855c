"""ctypes binding of librag_hip.so (include/rag_hip.h). Plain pointers and sizes only.

numpy arrays are passed as host pointers (`*_host` entry points); torch CUDA tensors as device pointers
(`*_dev` entry points, asynchronous on the current torch stream). PyTorch is used for device memory and
streams only — never for the arithmetic.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class RagError(RuntimeError):
    pass


def lib_path():
    # RAG_HIP_LIB: diagnostic builds of the library (tools/ce_probe_build.sh); the product path is the in-tree .so
    return os.environ.get("RAG_HIP_LIB") or os.path.join(_HERE, "librag_hip.so")


class DenseStats(C.Structure):
    _fields_ = [("n_queries", C.c_int32), ("proven_fast", C.c_int32), ("proven_wide", C.c_int32),
                ("exact_scan", C.c_int32), ("overflowed", C.c_int32), ("shortlist", C.c_int32),
                ("stages", C.c_int32), ("second_pass", C.c_int32), ("eps", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RowBlock(C.Structure):
    _fields_ = [("n", C.c_int64), ("emb", C.c_void_p), ("ids", C.c_void_p), ("tenants", C.c_void_p), ("temporal", C.c_void_p),
                ("tokens", C.c_void_p), ("token_lens", C.c_void_p)]


class IdMapInfo(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("ids_ascending", C.c_int32)] + \
               [(k, C.c_int64) for k in ("slots", "entries", "tombstones", "longest_probe", "hbm_bytes", "rebuilds")]


class Bm25Segments(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("base_docs", "tail_docs", "base_nnz", "tail_nnz", "n_terms", "tail_bytes", "appends", "folds")]


class Bm25RefreshInfo(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_docs_live", "nnz_live", "n_terms", "terms_without_postings", "negative_idf_terms")] + \
               [(k, C.c_double) for k in ("avgdl_before", "avgdl_after", "idf_max_abs_change")]


class CeConfig(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32),
                ("ffn", C.c_int32), ("max_pos", C.c_int32), ("type_vocab", C.c_int32), ("reserved", C.c_int32),
                ("ln_eps", C.c_double)]


# flag bits of rag_embed_load_host (include/rag_hip.h)
EMBED_NORMALIZE = 1
EMBED_POOL_CLS = 2
# pair layouts of rag_ce_set_pair_format
PAIR_BERT = 0
PAIR_ROBERTA = 1

_P = C.c_void_p
_SIGS = {
    "rag_version": ([], C.c_int),
    "rag_device_count": ([C.POINTER(C.c_int)], C.c_int),
    "rag_create": ([C.c_int, C.c_int, C.POINTER(_P)], C.c_int),
    "rag_destroy": ([_P], C.c_int),
    "rag_last_error": ([_P], C.c_char_p),
    "rag_synchronize": ([_P], C.c_int),
    "rag_set_profiling": ([_P, C.c_int], C.c_int),
    "rag_set_option": ([_P, C.c_char_p, C.c_int], C.c_int),
    "rag_bm25_index_bytes": ([_P, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)], C.c_int),
    "rag_bm25_grid_plan": ([C.c_int, C.c_int, C.c_int, _P], C.c_int),
    "rag_index_load_host": ([_P, _P, _P, C.c_int64, C.c_int64], C.c_int),
    "rag_index_load_dev": ([_P, _P, _P, C.c_int64, C.c_int64, _P], C.c_int),
    "rag_index_reserve": ([_P, C.c_int64, C.c_int64], C.c_int),
    "rag_index_append_host": ([_P, _P, C.c_int64], C.c_int),
    "rag_index_append_dev": ([_P, _P, C.c_int64, _P], C.c_int),
    "rag_index_set_tenants_host": ([_P, _P, C.c_int64], C.c_int),
    "rag_index_set_ids_host": ([_P, _P, C.c_int64], C.c_int),
    "rag_index_rows": ([_P, C.POINTER(C.c_int64)], C.c_int),
    "rag_index_fetch_rows_host": ([_P, _P, C.c_int, _P], C.c_int),
    "rag_index_insert_host": ([_P, C.POINTER(RowBlock), C.POINTER(C.c_int64)], C.c_int),
    "rag_index_delete_host": ([_P, _P, C.c_int64, C.c_int, C.POINTER(C.c_int64)], C.c_int),
    "rag_index_compact": ([_P, _P, C.POINTER(C.c_int64)], C.c_int),
    "rag_index_compact_bm25": ([_P, _P, C.POINTER(C.c_int64)], C.c_int),
    "rag_index_compact_live": ([_P, _P, C.POINTER(C.c_int64)], C.c_int),
    "rag_index_deleted_rows": ([_P, C.POINTER(C.c_int64)], C.c_int),
    "rag_index_id_map": ([_P, C.c_int], C.c_int),
    "rag_index_rows_of_ids_dev": ([_P, _P, C.c_int64, _P, _P], C.c_int),
    "rag_index_rows_of_ids_host": ([_P, _P, C.c_int64, _P], C.c_int),
    "rag_index_id_map_info": ([_P, C.POINTER(IdMapInfo)], C.c_int),
    "rag_dense_topk_host": ([_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P], C.c_int),
    "rag_dense_topk_dev": ([_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P], C.c_int),
    "rag_dense_last_stats": ([_P, C.POINTER(DenseStats)], C.c_int),
    "rag_dense_kernel_ms": ([_P, C.POINTER(C.c_float), C.POINTER(C.c_int)], C.c_int),
    "rag_stage_kernel_ms": ([_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)], C.c_int),
    "rag_merge_topk_dev": ([_P, _P, _P, C.c_int, C.c_int64, C.c_int, C.c_int, _P, _P, _P], C.c_int),
    "rag_comm_unique_id": ([_P], C.c_int),
    "rag_comm_init": ([_P, C.c_int, C.c_int, _P], C.c_int),
    "rag_comm_allgather_dev": ([_P, _P, _P, C.c_size_t, _P], C.c_int),
    "rag_comm_count": ([_P, _P], C.c_int),
    "rag_comm_destroy": ([_P], C.c_int),
    "rag_pairwise_cosine_host": ([_P, _P, C.c_int, _P, C.c_int, C.c_int, _P], C.c_int),
    "rag_pairwise_cosine_f64_host": ([_P, _P, C.c_int, _P, C.c_int, C.c_int, _P], C.c_int),
    "rag_rrf_fuse_host": ([_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P], C.c_int),
    "rag_bm25_load_host": ([_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double], C.c_int),
    "rag_bm25_append_host": ([_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64], C.c_int),
    "rag_bm25_fold": ([_P], C.c_int),
    "rag_bm25_segment_stats": ([_P, C.POINTER(Bm25Segments)], C.c_int),
    "rag_bm25_live_counts_host": ([_P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)], C.c_int),
    "rag_bm25_set_statistics_host": ([_P, _P, C.c_double], C.c_int),
    "rag_bm25_refresh": ([_P, C.c_double, _P, C.POINTER(Bm25RefreshInfo)], C.c_int),
    "rag_bm25_topk_host": ([_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P], C.c_int),
    "rag_bm25_scores_host": ([_P, _P, _P, C.c_int, _P], C.c_int),
    "rag_bm25_scores_adhoc_host": ([_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double, _P, _P,
                                   C.c_int, _P], C.c_int),
    "rag_bm25_set_normalize": ([_P, C.c_int], C.c_int),
    "rag_chunk_chain_host": ([_P, _P, _P, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _P], C.c_int),
    "rag_mmr_select_host": ([_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _P, _P], C.c_int),
    "rag_mmr_select_dev": ([_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _P, _P, _P], C.c_int),
    "rag_rrf_fuse_dev": ([_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P], C.c_int),
    "rag_bm25_topk_dev": ([_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P], C.c_int),
    "rag_hybrid_rrf_dev": ([_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P], C.c_int),
    "rag_sparse_load_host": ([_P, _P, _P, _P, C.c_int64, C.c_int64], C.c_int),
    "rag_sparse_append_host": ([_P, _P, _P, _P, C.c_int64, C.c_int64], C.c_int),
    "rag_sparse_append_dev": ([_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int64, _P], C.c_int),
    "rag_sparse_append_docs_host": ([_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int64], C.c_int),
    "rag_sparse_clear": ([_P], C.c_int),
    "rag_sparse_export_host": ([_P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)], C.c_int),
    "rag_sparse_fold": ([_P], C.c_int),
    "rag_sparse_segment_stats": ([_P, C.POINTER(Bm25Segments)], C.c_int),
    "rag_sparse_info": ([_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)], C.c_int),
    "rag_sparse_topk_host": ([_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P], C.c_int),
    "rag_sparse_topk_dev": ([_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P], C.c_int),
    "rag_sparse_scores_host": ([_P, _P, _P, _P, C.c_int, _P], C.c_int),
    "rag_hybrid_sparse_rrf_dev": ([_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P], C.c_int),
    "rag_index_set_temporal_host": ([_P, _P, C.c_int64], C.c_int),
    "rag_hybrid_linear_dev": ([_P, _P, _P, _P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, _P, _P, _P, _P, _P, _P,
                               _P], C.c_int),
    "rag_hybrid_linear_batch": ([_P, C.POINTER(C.c_int)], C.c_int),
    "rag_hybrid_linear_begin_dev": ([_P, _P, _P, C.c_int, C.c_int, _P, _P], C.c_int),
    "rag_hybrid_linear_finish_dev": ([_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, _P, _P], C.c_int),
    "rag_hybrid_linear_merge_gathered_dev": ([_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P], C.c_int),
    "rag_linear_fuse_topk_host": ([_P, _P, _P, _P, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, _P, _P], C.c_int),
    "rag_ce_load_host": ([_P, C.POINTER(CeConfig), C.POINTER(_P), C.c_int], C.c_int),
    "rag_ce_score_host": ([_P, _P, _P, _P, C.c_int, C.c_int, _P], C.c_int),
    "rag_tokens_load_host": ([_P, _P, _P, C.c_int64, C.c_int], C.c_int),
    "rag_tokens_reserve": ([_P, C.c_int64, C.c_int], C.c_int),
    "rag_tokens_append_dev": ([_P, _P, _P, C.c_int64, _P], C.c_int),
    "rag_tokens_load_wide_host": ([_P, _P, _P, C.c_int64, C.c_int, C.c_int], C.c_int),
    "rag_tokens_reserve_wide": ([_P, C.c_int64, C.c_int, C.c_int], C.c_int),
    "rag_tokens_info": ([_P, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
    "rag_ce_set_pair_format": ([_P, C.c_int], C.c_int),
    "rag_hybrid_fuse_gathered_dev": ([_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P], C.c_int),
    "rag_retrieve_rerank_dev": ([_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_int, _P, _P, _P, _P, _P], C.c_int),
    "rag_ce_build_pairs_dev": ([_P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P], C.c_int),
    "rag_rerank_topk_dev": ([_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P], C.c_int),
    "rag_ce_score_dev": ([_P, _P, _P, _P, C.c_int, C.c_int, _P, _P], C.c_int),
    "rag_embed_load_host": ([_P, C.POINTER(CeConfig), C.POINTER(_P), C.c_int, C.c_int], C.c_int),
    "rag_embed_host": ([_P, _P, _P, _P, C.c_int, C.c_int, _P], C.c_int),
    "rag_embed_dev": ([_P, _P, _P, _P, C.c_int, C.c_int, _P, _P], C.c_int),
    "rag_embed_dim": ([_P, C.POINTER(C.c_int)], C.c_int),
    "rag_embed_heads_load_host": ([_P, _P, _P, C.c_int, _P, C.c_float], C.c_int),
    "rag_embed_multi_host": ([_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int64, _P], C.c_int),
    "rag_embed_multi_dev": ([_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int64, _P, _P], C.c_int),
    "rag_maxsim_host": ([_P, _P, _P, C.c_int, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P], C.c_int),
    "rag_maxsim_dev": ([_P, _P, _P, C.c_int, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P], C.c_int),
    "rag_lexical_match_host": ([_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_int, _P], C.c_int),
    "rag_lexical_match_dev": ([_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_int, _P, _P], C.c_int),
    "rag_lexical_compact_host": ([_P, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int64], C.c_int),
    "rag_lexical_compact_dev": ([_P, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int64, _P], C.c_int),
    "rag_tokvec_reserve": ([_P, C.c_int64, C.c_int64, C.c_int], C.c_int),
    "rag_tokvec_reserve_form": ([_P, C.c_int64, C.c_int64, C.c_int, C.c_int], C.c_int),
    "rag_tokvec_load_form_host": ([_P, _P, _P, C.c_int64, C.c_int, C.c_int], C.c_int),
    "rag_tokvec_form": ([_P, C.POINTER(C.c_int)], C.c_int),
    "rag_tokvec_append_dev": ([_P, _P, _P, C.c_int64, _P], C.c_int),
    "rag_tokvec_append_host": ([_P, _P, _P, C.c_int64], C.c_int),
    "rag_tokvec_load_host": ([_P, _P, _P, C.c_int64, C.c_int], C.c_int),
    "rag_tokvec_info": ([_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int64)], C.c_int),
    "rag_tokvec_fetch_host": ([_P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64)], C.c_int),
    "rag_tokvec_rerank_dev": ([_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P], C.c_int),
    "rag_tokvec_rerank_host": ([_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P], C.c_int),
    "rag_retrieve_maxsim_dev": ([_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P], C.c_int),
    "rag_sparse_score_rows_dev": ([_P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P], C.c_int),
    "rag_sparse_score_rows_host": ([_P, _P, _P, _P, _P, C.c_int, C.c_int, _P], C.c_int),
    "rag_m3_score_rows_dev": ([_P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P,
                               _P], C.c_int),
    "rag_retrieve_m3_dev": ([_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                             C.c_double, _P, _P, _P, _P, _P], C.c_int),
    "rag_m3_candidates_gathered_dev": ([_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P], C.c_int),
    "rag_m3_score_ids_dev": ([_P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, _P, _P], C.c_int),
    "rag_m3_combine_gathered_dev": ([_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P],
                                    C.c_int),
    "rag_search_m3_tokens_dev": ([_P, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                  C.c_double, C.c_double, _P, _P, _P, _P, _P], C.c_int),
    "rag_ce_length_class": ([C.c_int, C.c_int, C.POINTER(C.c_int)], C.c_int),
    "rag_model_seq_limit": ([_P, C.c_int, C.POINTER(C.c_int)], C.c_int),
}
# The per-query-tenant entries: the arguments of their namesakes with `const int32_t* tenants_host` where those have `int tenant`
# (argument position of the tenant in the namesake's list).
for _name, _pos in (("rag_dense_topk_host", 4), ("rag_dense_topk_dev", 4), ("rag_bm25_topk_host", 5), ("rag_bm25_topk_dev", 5),
                    ("rag_hybrid_rrf_dev", 8), ("rag_hybrid_linear_dev", 9), ("rag_retrieve_rerank_dev", 11),
                    ("rag_sparse_topk_host", 6), ("rag_sparse_topk_dev", 6), ("rag_hybrid_sparse_rrf_dev", 9),
                    ("rag_retrieve_maxsim_dev", 11), ("rag_retrieve_m3_dev", 11), ("rag_search_m3_tokens_dev", 11),
                    ("rag_hybrid_linear_begin_dev", 4), ("rag_hybrid_linear_finish_dev", 9)):
    _args, _res = _SIGS[_name]
    assert _args[_pos] is C.c_int
    _SIGS[_name.replace("_host", "_tenants_host").replace("_dev", "_tenants_dev")] = (_args[:_pos] + [_P] + _args[_pos + 1:], _res)


def exported_symbols():
    """Every entry point include/rag_hip.h declares (tests check the .so exports each of them)."""
    return sorted(_SIGS)


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (soname libamdhip64.so.7). Two HIP runtimes in one
    process cannot both own the GPU, and device pointers are only shareable inside one runtime, so when torch is
    installed its runtime is loaded FIRST: librag_hip.so's DT_NEEDED libamdhip64.so.7 then binds to it."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load_library(path=None):
    """Load librag_hip.so. Fails loudly when it has not been built (`python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or lib_path()
    if not os.path.exists(p):
        raise RagError(f"{p} is missing: build the HIP extension first (__graft_entry__.build()); "
                       "there is no CPU fallback")
    _preload_torch_hip_runtime()
    lib = C.CDLL(p)
    for name, (args, res) in _SIGS.items():
        fn = getattr(lib, name)          # AttributeError = missing export: loud
        fn.argtypes = args
        fn.restype = res
    if path is None:
        _LIB = lib
    return lib


def bm25_index_bytes(indptr, n_docs):
    """(postings, metadata, bracket-table) bytes of HBM a CSR with these offsets takes once loaded; host-only, no GPU."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    rc = load_library().rag_bm25_index_bytes(C.c_void_p(indptr.ctypes.data), int(n_docs), int(indptr.shape[0] - 1), C.byref(a), C.byref(b), C.byref(c))
    if rc != 0:
        raise RagError(f"rag_bm25_index_bytes failed ({rc})")
    return int(a.value), int(b.value), int(c.value)


def bm25_grid_plan(n_ranges_in_launch, n_queries, linear=False):
    """(workgroups, ranges, queries, query groups per range, queries per group) of one BM25 scoring launch; host-only, no GPU."""
    out = (C.c_int64 * 5)()
    rc = load_library().rag_bm25_grid_plan(int(n_ranges_in_launch), int(n_queries), int(bool(linear)), C.cast(out, C.c_void_p))
    if rc != 0:
        raise RagError(f"rag_bm25_grid_plan failed ({rc})")
    return tuple(int(v) for v in out)


def _np(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _tenant_arg(tenant, n_queries):
    """The `tenant` of a search -> (per_query, C argument). An int is the one filter of the whole batch (the scalar entries); a
    sequence or int32 array of length n_queries gives every query its own tenant (< 0: not filtered) and selects the
    rag_*_tenants_* entries. The array is host memory and is consumed before the call returns."""
    if isinstance(tenant, (int, np.integer)):
        return False, int(tenant)
    if _is_torch(tenant):
        tenant = tenant.cpu().numpy()
    if np.ndim(tenant) == 0:                                  # a 0-d array or tensor is one number, as int(tenant) always took it
        return False, int(tenant)
    t = np.ascontiguousarray(tenant, dtype=np.int32)
    if t.shape != (n_queries,):
        raise RagError(f"tenant: expected an int or {n_queries} tenant numbers, got shape {t.shape}")
    return True, t


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class RagEngine:
    """One handle = one GPU (one process rank). Thin object wrapper over the C-ABI."""

    def __init__(self, dim, device=0):
        self.lib = load_library()
        self.dim = int(dim)
        self.device = int(device)
        h = _P()
        rc = self.lib.rag_create(self.device, self.dim, C.byref(h))
        if rc != 0:
            raise RagError(f"rag_create(device={device}, dim={dim}) failed with {rc} (no usable MI355X / bad dim)")
        self.h = h
        self._keep = []
        self.n_rows = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.rag_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.rag_last_error(self.h)
            raise RagError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def synchronize(self):
        self._check(self.lib.rag_synchronize(self.h), "rag_synchronize")

    def set_option(self, name, value):
        """Diagnostic / tuning switch of this handle (include/rag_hip.h rag_set_option); defaults come from RAG_<NAME> at creation."""
        self._check(self.lib.rag_set_option(self.h, name.encode(), int(value)), f"rag_set_option({name})")

    def set_profiling(self, on):
        self._check(self.lib.rag_set_profiling(self.h, 1 if on else 0), "rag_set_profiling")

    # ---- dense index ---------------------------------------------------------------------------
    def index_load(self, emb, ids=None, id_base=0):
        """emb: [N, dim] float32 numpy array (host) or torch CUDA tensor (device)."""
        if _is_torch(emb):
            import torch
            assert emb.is_cuda and emb.dtype == torch.float32 and emb.is_contiguous() and emb.shape[1] == self.dim
            idp = None
            if ids is not None:
                assert ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous()
                idp = C.c_void_p(ids.data_ptr())
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            self._check(self.lib.rag_index_load_dev(self.h, C.c_void_p(emb.data_ptr()), idp, int(id_base),
                                                    emb.shape[0], st), "rag_index_load_dev")
            torch.cuda.current_stream().synchronize()
            self.n_rows = int(emb.shape[0])
            return
        emb = _np(emb, np.float32)
        if emb.ndim != 2 or emb.shape[1] != self.dim:
            raise RagError(f"index_load: expected [N,{self.dim}] got {emb.shape}")
        ida = None if ids is None else _np(ids, np.int64)
        self._check(self.lib.rag_index_load_host(self.h, _ptr(emb), _ptr(ida), int(id_base), emb.shape[0]),
                    "rag_index_load_host")
        self.n_rows = int(emb.shape[0])

    def index_reserve(self, n_rows_total, id_base=0):
        self._check(self.lib.rag_index_reserve(self.h, int(n_rows_total), int(id_base)), "rag_index_reserve")
        self.n_rows = 0

    def index_append(self, emb):
        """Append a block of rows (numpy host array or torch CUDA tensor) to a reserved index."""
        if _is_torch(emb):
            import torch
            assert emb.is_cuda and emb.dtype == torch.float32 and emb.is_contiguous() and emb.shape[1] == self.dim
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            self._check(self.lib.rag_index_append_dev(self.h, C.c_void_p(emb.data_ptr()), emb.shape[0], st), "rag_index_append_dev")
            torch.cuda.current_stream().synchronize()
        else:
            emb = _np(emb, np.float32)
            self._check(self.lib.rag_index_append_host(self.h, _ptr(emb), emb.shape[0]), "rag_index_append_host")
        self.n_rows += int(emb.shape[0])

    def set_tenants(self, tenant_of_row):
        t = None if tenant_of_row is None else _np(tenant_of_row, np.int32)
        self._check(self.lib.rag_index_set_tenants_host(self.h, _ptr(t), 0 if t is None else t.shape[0]),
                    "rag_index_set_tenants_host")

    def set_ids(self, ids):
        ids = _np(ids, np.int64)
        self._check(self.lib.rag_index_set_ids_host(self.h, _ptr(ids), ids.shape[0]), "rag_index_set_ids_host")

    def fetch_rows(self, rows):
        rows = _np(rows, np.int64)
        out = np.empty((rows.shape[0], self.dim), dtype=np.float32)
        self._check(self.lib.rag_index_fetch_rows_host(self.h, _ptr(rows), rows.shape[0], _ptr(out)),
                    "rag_index_fetch_rows_host")
        return out

    # ---- live writes (include/rag_hip.h rag_index_insert_host / _delete_host / _compact) ---------------------------------
    def index_insert(self, emb, ids=None, tenants=None, temporal=None, tokens=None, token_lens=None):
        """Insert rows (host arrays); searchable on return. Returns the first new row number."""
        emb = _np(emb, np.float32)
        if emb.ndim == 1:
            emb = emb[None]
        if emb.ndim != 2 or emb.shape[1] != self.dim:
            raise RagError(f"index_insert: expected [N,{self.dim}] got {emb.shape}")
        n = emb.shape[0]
        planes = {}
        for name, a, dt in (("ids", ids, np.int64), ("tenants", tenants, np.int32), ("temporal", temporal, np.float64),
                            ("tokens", tokens, np.int32), ("token_lens", token_lens, np.int32)):
            if a is not None:
                a = _np(a, dt)
                if a.shape[0] != n:
                    raise RagError(f"index_insert: {name} has {a.shape[0]} rows, emb has {n}")
            planes[name] = a
        tok_L = getattr(self, "_tok_L", None)
        if planes["tokens"] is not None:           # the C side reads n * tok_L ids and n lengths from these pointers
            if tok_L is None or planes["tokens"].ndim != 2 or planes["tokens"].shape[1] != tok_L:
                raise RagError(f"index_insert: tokens must be [{n}, {tok_L}] (the loaded token store's passage length)")
            if planes["token_lens"] is None or planes["token_lens"].shape != (n,):
                raise RagError(f"index_insert: token_lens must be [{n}]")
        rb = RowBlock(n, emb.ctypes.data, *[None if planes[k] is None else planes[k].ctypes.data
                                            for k in ("ids", "tenants", "temporal", "tokens", "token_lens")])
        first = C.c_int64()
        self._check(self.lib.rag_index_insert_host(self.h, C.byref(rb), C.byref(first)), "rag_index_insert_host")
        self.n_rows = int(first.value) + n
        return int(first.value)

    def index_delete(self, ids, tenant=-1):
        """Delete the live rows with these doc ids (and tenant, when >= 0). Returns the number of rows removed."""
        ids = _np(np.atleast_1d(ids), np.int64)
        out = C.c_int64()
        self._check(self.lib.rag_index_delete_host(self.h, _ptr(ids), ids.shape[0], int(tenant), C.byref(out)), "rag_index_delete_host")
        return int(out.value)

    def index_compact(self, keep_postings=False, keep_resident=False):
        """Remove deleted rows from every plane. Returns row_map (int64 [rows before]: new row or -1). keep_postings
        (rag_index_compact_bm25): loaded BM25 postings are renumbered on the device and stay live; by default they end stale.
        keep_resident (rag_index_compact_live): the same, and the learned-sparse postings are renumbered and the token-vector
        store's documents move with their rows; neither ends stale."""
        n = C.c_int64()
        self._check(self.lib.rag_index_rows(self.h, C.byref(n)), "rag_index_rows")
        row_map = np.empty(int(n.value), dtype=np.int64)
        after = C.c_int64()
        name = "rag_index_compact_live" if keep_resident else ("rag_index_compact_bm25" if keep_postings else "rag_index_compact")
        keep_postings = keep_postings or keep_resident
        self._check(getattr(self.lib, name)(self.h, _ptr(row_map), C.byref(after)), name)
        self.n_rows = int(after.value)
        if keep_postings and hasattr(self, "bm25_docs"):             # the remap dropped documents: bm25_scores' width follows
            s = self.bm25_segment_stats()
            self.bm25_docs = s["base_docs"] + s["tail_docs"]
        return row_map

    def index_deleted_rows(self):
        out = C.c_int64()
        self._check(self.lib.rag_index_deleted_rows(self.h, C.byref(out)), "rag_index_deleted_rows")
        return int(out.value)

    # ---- id-to-row map (include/rag_hip.h rag_index_id_map) ----------------------------------------------------------------
    def index_id_map(self, enable=True):
        """Build the device id-to-row map of an index with explicit ids and keep it maintained through the writes (False frees it)."""
        self._check(self.lib.rag_index_id_map(self.h, 1 if enable else 0), "rag_index_id_map")

    def index_id_map_info(self):
        s = IdMapInfo()
        self._check(self.lib.rag_index_id_map_info(self.h, C.byref(s)), "rag_index_id_map_info")
        return {k: int(getattr(s, k)) for k, _ in s._fields_}

    def rows_of_ids(self, ids):
        """The live row of each doc id (int32, -1 = unknown, deleted or negative id); host arrays."""
        ids = _np(np.atleast_1d(ids), np.int64)
        out = np.empty(ids.shape, dtype=np.int32)
        self._check(self.lib.rag_index_rows_of_ids_host(self.h, _ptr(ids), ids.size, _ptr(out)), "rag_index_rows_of_ids_host")
        return out

    def rows_of_ids_dev(self, ids, rows_out, stream=None):
        """torch CUDA tensors (int64 in, int32 out, same number of elements); asynchronous on `stream` (default: torch's current stream)."""
        import torch
        assert ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous()
        assert rows_out.is_cuda and rows_out.dtype == torch.int32 and rows_out.is_contiguous() and rows_out.numel() == ids.numel()
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_index_rows_of_ids_dev(self.h, C.c_void_p(ids.data_ptr()), ids.numel(), C.c_void_p(rows_out.data_ptr()), st),
                    "rag_index_rows_of_ids_dev")

    def dense_topk(self, queries, k, tenant=-1):
        """queries [Q, dim] float32 (numpy). Returns (ids int64 [Q,k], rows int32 [Q,k], scores float64 [Q,k])."""
        q = _np(queries, np.float32)
        if q.ndim == 1:
            q = q[None]
        if q.shape[1] != self.dim:
            raise RagError(f"dense_topk: expected [Q,{self.dim}] got {q.shape}")
        Q = q.shape[0]
        ids = np.empty((Q, k), dtype=np.int64)
        rows = np.empty((Q, k), dtype=np.int32)
        sc = np.empty((Q, k), dtype=np.float64)
        per_query, t = _tenant_arg(tenant, Q)
        if per_query:
            self._check(self.lib.rag_dense_topk_tenants_host(self.h, _ptr(q), Q, int(k), _ptr(t), _ptr(ids), _ptr(rows), _ptr(sc)),
                        "rag_dense_topk_tenants_host")
            return ids, rows, sc
        self._check(self.lib.rag_dense_topk_host(self.h, _ptr(q), Q, int(k), t, _ptr(ids), _ptr(rows), _ptr(sc)),
                    "rag_dense_topk_host")
        return ids, rows, sc

    def dense_topk_dev(self, q, k, ids_out, rows_out, scores_out, tenant=-1, stream=None):
        """torch CUDA tensors in/out; asynchronous on `stream` (default: torch's current stream)."""
        import torch
        assert q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() and q.shape[1] == self.dim
        assert ids_out.dtype == torch.int64 and scores_out.dtype == torch.float64
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        rp = None if rows_out is None else C.c_void_p(rows_out.data_ptr())
        per_query, t = _tenant_arg(tenant, q.shape[0])
        fn, name = (self.lib.rag_dense_topk_tenants_dev, "rag_dense_topk_tenants_dev") if per_query else (self.lib.rag_dense_topk_dev, "rag_dense_topk_dev")
        self._check(fn(self.h, C.c_void_p(q.data_ptr()), q.shape[0], int(k), _ptr(t) if per_query else t,
                       C.c_void_p(ids_out.data_ptr()), rp, C.c_void_p(scores_out.data_ptr()), st), name)

    def dense_stats(self):
        s = DenseStats()
        self._check(self.lib.rag_dense_last_stats(self.h, C.byref(s)), "rag_dense_last_stats")
        return s.as_dict()

    def dense_kernel_ms(self):
        ms, n = C.c_float(), C.c_int()
        self._check(self.lib.rag_dense_kernel_ms(self.h, C.byref(ms), C.byref(n)), "rag_dense_kernel_ms")
        return float(ms.value), int(n.value)

    def stage_kernel_ms(self, stage):
        """(summed device ms, spans) of profiling stage 0 dense emit / 1 BM25 top-k / 2 cross-encoder forward."""
        ms, n = C.c_float(), C.c_int()
        self._check(self.lib.rag_stage_kernel_ms(self.h, int(stage), C.byref(ms), C.byref(n)), "rag_stage_kernel_ms")
        return float(ms.value), int(n.value)

    def merge_topk_dev(self, ids, scores, ids_out, scores_out, n_lists=None, list_stride=None, stream=None):
        """ids/scores: torch CUDA tensors holding n_lists lists of [Q, k] (int64 / float64), list l at element
        offset l*list_stride (default: contiguous [L, Q, k]). Output [Q, k], score desc then id asc."""
        import torch
        Q, k = ids_out.shape
        if n_lists is None:
            n_lists = ids.shape[0]
        if list_stride is None:
            list_stride = Q * k
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_merge_topk_dev(self.h, C.c_void_p(ids.data_ptr()), C.c_void_p(scores.data_ptr()),
                                                int(n_lists), int(list_stride), Q, k, C.c_void_p(ids_out.data_ptr()),
                                                C.c_void_p(scores_out.data_ptr()), st), "rag_merge_topk_dev")

    # ---- RCCL exchange behind the C-ABI (multi-GPU, one process per GPU) -----------------------------
    def comm_unique_id(self):
        """128-byte RCCL id (bytes): create on ONE rank, hand to the others out of band, pass to comm_init on every rank."""
        buf = C.create_string_buffer(128)
        rc = self.lib.rag_comm_unique_id(buf)
        if rc != 0:
            raise RagError(f"rag_comm_unique_id failed ({rc}): librccl not available")
        return buf.raw

    def comm_init(self, rank, world, unique_id):
        """Collective over `world` ranks (one per GPU). Afterwards the sharded classes gather through the library."""
        if len(unique_id) != 128:
            raise RagError("comm_init: unique_id must be 128 bytes")
        self._check(self.lib.rag_comm_init(self.h, int(rank), int(world), C.c_char_p(unique_id)), "rag_comm_init")
        self.comm_world = int(world)

    def comm_allgather_dev(self, send, recv, stream=None):
        """recv[world, ...] <- every rank's send (torch CUDA tensors, contiguous); asynchronous on `stream`."""
        import torch
        nbytes = send.numel() * send.element_size()
        if not (send.is_contiguous() and recv.is_contiguous()) or recv.numel() * recv.element_size() != nbytes * getattr(self, "comm_world", 1):
            raise RagError("comm_allgather_dev: recv must be contiguous and hold world x send")
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_comm_allgather_dev(self.h, C.c_void_p(send.data_ptr()), C.c_void_p(recv.data_ptr()), nbytes, st),
                    "rag_comm_allgather_dev")

    def comm_count(self):
        """Ranks of the RCCL communicator behind rag_comm_allgather_dev (ncclCommCount)."""
        n = C.c_int(0)
        self._check(self.lib.rag_comm_count(self.h, C.byref(n)), "rag_comm_count")
        return int(n.value)

    def comm_destroy(self):
        self._check(self.lib.rag_comm_destroy(self.h), "rag_comm_destroy")
        self.comm_world = 0

    # ---- small ops --------------------------------------------------------------------------------
    def pairwise_cosine(self, a, b=None):
        """float64 cosine matrix. float64 inputs (what engine.as_matrix builds from the agent's List[float]) go to the device
        unrounded (rag_pairwise_cosine_f64_host); anything else is taken as float32."""
        f64 = getattr(a, "dtype", None) == np.float64 and (b is None or getattr(b, "dtype", None) == np.float64)
        dt = np.float64 if f64 else np.float32
        a = _np(a, dt)
        b = a if b is None else _np(b, dt)
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
            raise RagError(f"pairwise_cosine: shapes {a.shape} {b.shape}")
        out = np.zeros((a.shape[0], b.shape[0]), dtype=np.float64)
        if out.size:
            fn = self.lib.rag_pairwise_cosine_f64_host if f64 else self.lib.rag_pairwise_cosine_host
            self._check(fn(self.h, _ptr(a), a.shape[0], _ptr(b), b.shape[0], a.shape[1], _ptr(out)), "rag_pairwise_cosine_host")
        return out

    def chunk_chain(self, embs, sent_len, threshold, max_chunk, min_chunk):
        """SemanticChunker's sentence loop on the device: embs [n, dim] float32, sent_len [n] -> chunk number per sentence."""
        embs = _np(embs, np.float32)
        sent_len = _np(sent_len, np.int32)
        n, dim = embs.shape
        out = np.empty((n,), dtype=np.int32)
        self._check(self.lib.rag_chunk_chain_host(self.h, _ptr(embs), _ptr(sent_len), n, dim, float(threshold), int(max_chunk),
                                                  int(min_chunk), _ptr(out)), "rag_chunk_chain_host")
        return out

    MMR_MAX_CANDIDATES = 256

    def mmr_select(self, query, embs, top_k, lam, variant):
        """Greedy MMR over explicit candidates: query [dim], embs [n, dim] float32 -> (positions [<=top_k], scores).
        variant 0 = MMRDiversifier.diversify, 1 = apply_mmr (see include/rag_hip.h)."""
        query = _np(query, np.float32).reshape(-1)
        embs = _np(embs, np.float32)
        n, dim = embs.shape
        kk = int(min(top_k, n))
        sel = np.empty((kk,), dtype=np.int32)
        sc = np.empty((kk,), dtype=np.float64)
        self._check(self.lib.rag_mmr_select_host(self.h, _ptr(query), _ptr(embs), n, dim, kk, float(lam), int(variant),
                                                 _ptr(sel), _ptr(sc)), "rag_mmr_select_host")
        keep = sel >= 0
        return sel[keep], sc[keep]

    def mmr_select_dev(self, q, rows, top_k, lam, variant, sel_out, score_out, stream=None):
        """Batched MMR over rows of the resident index: q [Q, dim] float32, rows [Q, pool] int32 (CUDA tensors)."""
        import torch
        Q, pool = rows.shape
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_mmr_select_dev(self.h, C.c_void_p(q.data_ptr()), C.c_void_p(rows.data_ptr()), Q, pool,
                                                int(top_k), float(lam), int(variant), C.c_void_p(sel_out.data_ptr()),
                                                C.c_void_p(score_out.data_ptr()), st), "rag_mmr_select_dev")

    def rrf_fuse(self, lists, rrf_k=60, top_k=10):
        """lists: int64 [Q, L, len] (-1 padded at tails). Returns (keys [Q,top_k], scores, ranks [Q,top_k,L])."""
        lists = _np(lists, np.int64)
        Q, L, ln = lists.shape
        keys = np.empty((Q, top_k), dtype=np.int64)
        sc = np.empty((Q, top_k), dtype=np.float64)
        ranks = np.empty((Q, top_k, L), dtype=np.int32)
        self._check(self.lib.rag_rrf_fuse_host(self.h, _ptr(lists), Q, L, ln, int(rrf_k), int(top_k), _ptr(keys), _ptr(sc),
                                               _ptr(ranks)), "rag_rrf_fuse_host")
        return keys, sc, ranks

    def linear_fuse_topk(self, semantic, keyword, temporal, alpha, beta, gamma, top_k):
        s = _np(semantic, np.float64)
        kw = _np(keyword, np.float64)
        t = None if temporal is None else _np(temporal, np.float64)
        n = s.shape[0]
        kk = min(int(top_k), n) if n else 0
        idx = np.empty((max(kk, 1),), dtype=np.int32)
        hyb = np.empty((max(n, 1),), dtype=np.float64)
        if n == 0 or kk <= 0:
            return idx[:0], hyb[:0]
        self._check(self.lib.rag_linear_fuse_topk_host(self.h, _ptr(s), _ptr(kw), _ptr(t), n, float(alpha), float(beta),
                                                       float(gamma), kk, _ptr(idx), _ptr(hyb)), "rag_linear_fuse_topk_host")
        return idx[:kk], hyb[:n]

    # ---- BM25 -------------------------------------------------------------------------------------
    def bm25_load(self, indptr, doc, tf, doc_len, idf, avgdl, k1=1.5, b=0.75):
        indptr = _np(indptr, np.int64)
        doc = _np(doc, np.int32)
        tf = _np(tf, np.int32)
        doc_len = _np(doc_len, np.int32)
        idf = _np(idf, np.float64)
        self._check(self.lib.rag_bm25_load_host(self.h, _ptr(indptr), _ptr(doc), _ptr(tf), _ptr(doc_len), _ptr(idf),
                                                doc_len.shape[0], idf.shape[0], float(avgdl), float(k1), float(b)),
                    "rag_bm25_load_host")
        self.bm25_docs = int(doc_len.shape[0])

    # ---- appendable postings (include/rag_hip.h rag_bm25_append_host / rag_bm25_fold / rag_bm25_segment_stats) -------------
    def bm25_append(self, indptr, doc, tf, doc_len, idf_new, n_terms_total=None):
        """Postings of the next len(doc_len) rows after the rows the resident postings cover: CSR over the handle's vocabulary
        (doc relative to the block's first row), idf_new for the terms numbered past the known ones. Statistics stay frozen."""
        indptr = _np(indptr, np.int64)
        doc = _np(doc, np.int32)
        tf = _np(tf, np.int32)
        doc_len = _np(doc_len, np.int32)
        idf_new = _np(idf_new, np.float64)
        V = int(indptr.shape[0] - 1 if n_terms_total is None else n_terms_total)
        if indptr.shape[0] != V + 1 or doc.shape[0] != tf.shape[0] or (V >= 0 and doc.shape[0] != int(indptr[-1])):
            raise RagError("bm25_append: indptr must have n_terms_total + 1 entries and end at len(doc) == len(tf)")
        self._check(self.lib.rag_bm25_append_host(self.h, _ptr(indptr), _ptr(doc), _ptr(tf), _ptr(doc_len), _ptr(idf_new),
                                                  doc_len.shape[0], V), "rag_bm25_append_host")
        self.bm25_docs = getattr(self, "bm25_docs", 0) + int(doc_len.shape[0])

    def bm25_fold(self):
        """Merge the appended tail into the base postings on the device (results do not change)."""
        self._check(self.lib.rag_bm25_fold(self.h), "rag_bm25_fold")

    def bm25_segment_stats(self):
        out = Bm25Segments()
        self._check(self.lib.rag_bm25_segment_stats(self.h, C.byref(out)), "rag_bm25_segment_stats")
        return {k: int(getattr(out, k)) for k, _ in out._fields_}

    # ---- statistics refresh (include/rag_hip.h rag_bm25_refresh; needs set_option("bm25_keep_tf", 1) before bm25_load) ------
    def bm25_live_counts(self):
        """(df int32 [n_terms], live documents, sum of their lengths) over the covered documents that are not deleted."""
        V = self.bm25_segment_stats()["n_terms"]
        df = np.zeros(V, dtype=np.int32)
        n, s = C.c_int64(), C.c_int64()
        self._check(self.lib.rag_bm25_live_counts_host(self.h, _ptr(df), C.byref(n), C.byref(s)), "rag_bm25_live_counts_host")
        return df, int(n.value), int(s.value)

    def bm25_set_statistics(self, idf, avgdl):
        """Install idf [n_terms] / avgdl: every impact of the resident postings is recomputed on the device."""
        idf = _np(idf, np.float64)
        V = self.bm25_segment_stats()["n_terms"]
        if idf.shape != (V,):
            raise RagError(f"bm25_set_statistics: idf must have one entry per known term ({V}), got shape {idf.shape}")
        self._check(self.lib.rag_bm25_set_statistics_host(self.h, _ptr(idf), float(avgdl)), "rag_bm25_set_statistics_host")

    def bm25_refresh(self, epsilon=0.25):
        """Recompute idf / avgdl over the live documents (rank-bm25's rule) and rewrite the impacts in place -> (idf, info)."""
        V = self.bm25_segment_stats()["n_terms"]
        idf = np.zeros(V, dtype=np.float64)
        info = Bm25RefreshInfo()
        self._check(self.lib.rag_bm25_refresh(self.h, float(epsilon), _ptr(idf), C.byref(info)), "rag_bm25_refresh")
        return idf, {k: getattr(info, k) for k, _ in info._fields_}

    def bm25_topk(self, term_ptr, terms, k, tenant=-1):
        term_ptr = _np(term_ptr, np.int32)
        terms = _np(terms, np.int32)
        Q = term_ptr.shape[0] - 1
        ids = np.empty((Q, k), dtype=np.int64)
        rows = np.empty((Q, k), dtype=np.int32)
        sc = np.empty((Q, k), dtype=np.float64)
        mx = np.empty((Q,), dtype=np.float64)
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = (self.lib.rag_bm25_topk_tenants_host, "rag_bm25_topk_tenants_host") if per_query else (self.lib.rag_bm25_topk_host, "rag_bm25_topk_host")
        self._check(fn(self.h, _ptr(term_ptr), _ptr(terms), Q, int(k), _ptr(t) if per_query else t, _ptr(ids),
                       _ptr(rows), _ptr(sc), _ptr(mx)), name)
        return ids, rows, sc, mx

    def bm25_set_normalize(self, on):
        """on=False: bm25_topk* return RAW scores (a row-sharded index divides by the global max after its merge)."""
        self._check(self.lib.rag_bm25_set_normalize(self.h, 1 if on else 0), "rag_bm25_set_normalize")

    def bm25_topk_dev(self, term_ptr, terms, k, ids_out, rows_out, scores_out, raw_max_out=None, stream=None, tenant=-1):
        """Device tensors in / out (int32 term arrays; int64 ids, float64 scores [Q, k]); asynchronous on `stream`."""
        import torch
        Q = term_ptr.shape[0] - 1
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = (self.lib.rag_bm25_topk_tenants_dev, "rag_bm25_topk_tenants_dev") if per_query else (self.lib.rag_bm25_topk_dev, "rag_bm25_topk_dev")
        self._check(fn(self.h, C.c_void_p(term_ptr.data_ptr()), C.c_void_p(terms.data_ptr()), Q, int(k),
                       _ptr(t) if per_query else t, C.c_void_p(ids_out.data_ptr()),
                       C.c_void_p(rows_out.data_ptr() if rows_out is not None else 0),
                       C.c_void_p(scores_out.data_ptr()),
                       C.c_void_p(raw_max_out.data_ptr() if raw_max_out is not None else 0), st), name)

    def rrf_fuse_dev(self, lists, keys_out, scores_out, ranks_out, rrf_k=60, stream=None):
        """lists: [Q, n_lists, list_len] int64 doc ids (-1 padded) on the device -> keys/scores [Q, top_k], ranks [Q, top_k, n_lists]."""
        import torch
        Q, n_lists, list_len = lists.shape
        top_k = keys_out.shape[1]
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_rrf_fuse_dev(self.h, C.c_void_p(lists.data_ptr()), Q, n_lists, list_len, int(rrf_k), int(top_k),
                                              C.c_void_p(keys_out.data_ptr()), C.c_void_p(scores_out.data_ptr()),
                                              C.c_void_p(ranks_out.data_ptr()), st), "rag_rrf_fuse_dev")

    def hybrid_rrf_dev(self, q, term_ptr, terms, pool, k, rrf_k=60, tenant=-1, stream=None):
        """All-device hybrid (torch CUDA tensors): dense top-pool + BM25 top-pool -> RRF -> (keys [Q,k] int64, rrf scores
        [Q,k] float64, ranks [Q,k,2] int32). term_ptr / terms are int32 CUDA tensors."""
        import torch
        Q = q.shape[0]
        dev = q.device
        key = ("hyb", Q, pool, k)
        if getattr(self, "_hyb_key", None) != key:
            self._hyb = (torch.empty((2, Q, pool), dtype=torch.int64, device=dev),
                         torch.empty((Q, pool), dtype=torch.float64, device=dev),
                         torch.empty((Q, k), dtype=torch.int64, device=dev),
                         torch.empty((Q, k), dtype=torch.float64, device=dev),
                         torch.empty((Q, k, 2), dtype=torch.int32, device=dev))
            self._hyb_key = key
        lists, sc, keys, rrf, ranks = self._hyb
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = (self.lib.rag_hybrid_rrf_tenants_dev, "rag_hybrid_rrf_tenants_dev") if per_query else (self.lib.rag_hybrid_rrf_dev, "rag_hybrid_rrf_dev")
        self._check(fn(self.h, C.c_void_p(q.data_ptr()), C.c_void_p(term_ptr.data_ptr()),
                       C.c_void_p(terms.data_ptr()), Q, int(pool), int(k), int(rrf_k), _ptr(t) if per_query else t,
                       C.c_void_p(lists.data_ptr()), C.c_void_p(sc.data_ptr()),
                       C.c_void_p(keys.data_ptr()), C.c_void_p(rrf.data_ptr()),
                       C.c_void_p(ranks.data_ptr()), st), name)
        return keys, rrf, ranks

    # ---- learned-sparse inverted index (include/rag_hip.h rag_sparse_*; sparse.LexicalPostings builds the arrays) ----------
    def sparse_load(self, indptr, doc, weight, n_docs):
        """Term-major CSR of (doc int32, weight float32) postings: indptr [n_terms + 1], docs of a term strictly ascending,
        weights finite and > 0. Replaces the resident sparse index; the BM25 postings are not touched."""
        indptr = _np(indptr, np.int64)
        doc = _np(doc, np.int32)
        weight = _np(weight, np.float32)
        if indptr.ndim != 1 or indptr.shape[0] < 2 or doc.shape != weight.shape or doc.shape[0] != int(indptr[-1]):
            raise RagError("sparse_load: indptr must have n_terms + 1 entries and end at len(doc) == len(weight)")
        self._check(self.lib.rag_sparse_load_host(self.h, _ptr(indptr), _ptr(doc), _ptr(weight), int(n_docs), indptr.shape[0] - 1),
                    "rag_sparse_load_host")

    # ---- appendable sparse postings (include/rag_hip.h rag_sparse_append_host / rag_sparse_fold / rag_sparse_segment_stats) --
    def sparse_append(self, indptr, doc, weight, n_docs_new, n_terms_total=None):
        """Postings of the next n_docs_new rows after the rows the resident sparse postings cover: CSR over the handle's
        vocabulary (doc relative to the block's first row), weights finite and > 0. n_terms_total may grow, never shrink."""
        indptr = _np(indptr, np.int64)
        doc = _np(doc, np.int32)
        weight = _np(weight, np.float32)
        V = int(indptr.shape[0] - 1 if n_terms_total is None else n_terms_total)
        if indptr.ndim != 1 or indptr.shape[0] != V + 1 or V < 0 or doc.shape != weight.shape or doc.shape[0] != int(indptr[-1]):
            raise RagError("sparse_append: indptr must have n_terms_total + 1 entries and end at len(doc) == len(weight)")
        self._check(self.lib.rag_sparse_append_host(self.h, _ptr(indptr), _ptr(doc), _ptr(weight), int(n_docs_new), V),
                    "rag_sparse_append_host")

    # ---- the same from a doc-major block (rag_sparse_append_dev / rag_sparse_append_docs_host), rag_sparse_clear / _export_host --
    def sparse_append_dev(self, doc_ptr, terms, weights, n_terms_total, n_docs_new=None, stream=None):
        """The next rows from a doc-major block in CUDA tensors - the term_ptr / terms / qweights outputs of lexical_compact_dev as
        they are: int32 doc_ptr [n + 1] from 0, int32 terms ascending per document, float32 weights > 0 (terms and weights of one
        capacity). Transposed and appended on the device; waits for `stream` and returns once the postings are resident and
        checked. Without resident sparse postings the block becomes the base."""
        import torch
        assert doc_ptr.is_cuda and doc_ptr.dtype == torch.int32 and doc_ptr.is_contiguous()
        assert terms.is_cuda and terms.dtype == torch.int32 and terms.is_contiguous()
        assert weights.is_cuda and weights.dtype == torch.float32 and weights.is_contiguous()
        if terms.shape[0] != weights.shape[0]:
            raise RagError("sparse_append_dev: terms and weights must have one capacity")
        n = doc_ptr.shape[0] - 1 if n_docs_new is None else int(n_docs_new)
        if n + 1 > doc_ptr.shape[0]:
            raise RagError("sparse_append_dev: doc_ptr must hold n_docs_new + 1 offsets")
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_sparse_append_dev(self.h, C.c_void_p(doc_ptr.data_ptr()), C.c_void_p(terms.data_ptr()),
                                                   C.c_void_p(weights.data_ptr()), n, int(terms.shape[0]), int(n_terms_total), st),
                    "rag_sparse_append_dev")

    def sparse_append_docs(self, doc_ptr, terms, weights, n_terms_total):
        """The same block from host arrays (LexicalPostings.doc_major builds them), staged and run through the device path."""
        doc_ptr, terms, weights = _np(doc_ptr, np.int32), _np(terms, np.int32), _np(weights, np.float32)
        if doc_ptr.ndim != 1 or doc_ptr.shape[0] < 2 or terms.ndim != 1 or terms.shape != weights.shape:
            raise RagError("sparse_append_docs: expected doc_ptr [n + 1] and terms / weights of one length")
        self._check(self.lib.rag_sparse_append_docs_host(self.h, _ptr(doc_ptr), _ptr(terms), _ptr(weights), doc_ptr.shape[0] - 1,
                                                         terms.shape[0], int(n_terms_total)), "rag_sparse_append_docs_host")

    def sparse_clear(self):
        """Drop the resident sparse postings (nothing happens without any)."""
        self._check(self.lib.rag_sparse_clear(self.h), "rag_sparse_clear")

    def sparse_export(self):
        """The resident sparse postings, base and tail merged, as one term-major CSR with global document numbers:
        {"indptr" int64 [n_terms + 1], "doc" int32, "weight" float32, "n_docs"}."""
        v = [C.c_int64() for _ in range(3)]
        self._check(self.lib.rag_sparse_export_host(self.h, None, None, None, *[C.byref(x) for x in v]), "rag_sparse_export_host")
        n_docs, n_terms, nnz = (int(x.value) for x in v)
        indptr = np.zeros((n_terms + 1,), dtype=np.int64)
        doc, weight = np.empty((nnz,), dtype=np.int32), np.empty((nnz,), dtype=np.float32)
        self._check(self.lib.rag_sparse_export_host(self.h, _ptr(indptr), _ptr(doc), _ptr(weight), None, None, None), "rag_sparse_export_host")
        return {"indptr": indptr, "doc": doc, "weight": weight, "n_docs": n_docs}

    def sparse_fold(self):
        """Merge the appended tail into the base sparse postings on the device (results do not change)."""
        self._check(self.lib.rag_sparse_fold(self.h), "rag_sparse_fold")

    def sparse_segment_stats(self):
        out = Bm25Segments()
        self._check(self.lib.rag_sparse_segment_stats(self.h, C.byref(out)), "rag_sparse_segment_stats")
        return {k: int(getattr(out, k)) for k, _ in out._fields_}

    def sparse_info(self):
        v = [C.c_int64() for _ in range(4)]
        self._check(self.lib.rag_sparse_info(self.h, *[C.byref(x) for x in v]), "rag_sparse_info")
        return dict(zip(("n_docs", "n_terms", "nnz", "hbm_bytes"), (int(x.value) for x in v)))

    def sparse_topk(self, term_ptr, terms, weights, k, tenant=-1):
        """Weighted queries (CSR: term_ptr [Q + 1], terms, float32 weights) -> (ids, rows, scores) [Q, k]: the documents with a
        score > 0 by score descending, lower row first on ties; -1 / -1 / 0.0 behind them."""
        term_ptr = _np(term_ptr, np.int32)
        terms = _np(terms, np.int32)
        weights = _np(weights, np.float32)
        Q = term_ptr.shape[0] - 1
        ids = np.empty((Q, k), dtype=np.int64)
        rows = np.empty((Q, k), dtype=np.int32)
        sc = np.empty((Q, k), dtype=np.float64)
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = (self.lib.rag_sparse_topk_tenants_host, "rag_sparse_topk_tenants_host") if per_query else (self.lib.rag_sparse_topk_host, "rag_sparse_topk_host")
        self._check(fn(self.h, _ptr(term_ptr), _ptr(terms), _ptr(weights), Q, int(k), _ptr(t) if per_query else t, _ptr(ids),
                       _ptr(rows), _ptr(sc)), name)
        return ids, rows, sc

    def sparse_scores(self, term_ptr, terms, weights):
        """Float64 score of EVERY document [Q, n_docs] (0.0: no match, or a hidden row); for small corpora and tests."""
        term_ptr = _np(term_ptr, np.int32)
        terms = _np(terms, np.int32)
        weights = _np(weights, np.float32)
        Q = term_ptr.shape[0] - 1
        out = np.empty((Q, self.sparse_info()["n_docs"]), dtype=np.float64)
        self._check(self.lib.rag_sparse_scores_host(self.h, _ptr(term_ptr), _ptr(terms), _ptr(weights), Q, _ptr(out)), "rag_sparse_scores_host")
        return out

    def sparse_topk_dev(self, term_ptr, terms, weights, k, ids_out, rows_out, scores_out, stream=None, tenant=-1):
        """Device tensors in / out (int32 term arrays, float32 weights; int64 ids, float64 scores [Q, k]); asynchronous on `stream`."""
        import torch
        Q = term_ptr.shape[0] - 1
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = (self.lib.rag_sparse_topk_tenants_dev, "rag_sparse_topk_tenants_dev") if per_query else (self.lib.rag_sparse_topk_dev, "rag_sparse_topk_dev")
        self._check(fn(self.h, C.c_void_p(term_ptr.data_ptr()), C.c_void_p(terms.data_ptr()),
                       C.c_void_p(weights.data_ptr()), Q, int(k), _ptr(t) if per_query else t, C.c_void_p(ids_out.data_ptr()),
                       C.c_void_p(rows_out.data_ptr() if rows_out is not None else 0),
                       C.c_void_p(scores_out.data_ptr()), st), name)

    def hybrid_sparse_rrf_dev(self, q, term_ptr, terms, weights, pool, k, rrf_k=60, tenant=-1, stream=None):
        """hybrid_rrf_dev with the learned-sparse list in place of the BM25 list: dense top-pool + sparse top-pool -> RRF ->
        (keys [Q,k] int64, rrf scores [Q,k] float64, ranks [Q,k,2] int32); every input a CUDA tensor."""
        import torch
        Q = q.shape[0]
        dev = q.device
        key = ("hybs", Q, pool, k)
        if getattr(self, "_hybs_key", None) != key:
            self._hybs = (torch.empty((2, Q, pool), dtype=torch.int64, device=dev),
                          torch.empty((Q, pool), dtype=torch.float64, device=dev),
                          torch.empty((Q, k), dtype=torch.int64, device=dev),
                          torch.empty((Q, k), dtype=torch.float64, device=dev),
                          torch.empty((Q, k, 2), dtype=torch.int32, device=dev))
            self._hybs_key = key
        lists, sc, keys, rrf, ranks = self._hybs
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = ((self.lib.rag_hybrid_sparse_rrf_tenants_dev, "rag_hybrid_sparse_rrf_tenants_dev") if per_query
                    else (self.lib.rag_hybrid_sparse_rrf_dev, "rag_hybrid_sparse_rrf_dev"))
        self._check(fn(self.h, C.c_void_p(q.data_ptr()), C.c_void_p(term_ptr.data_ptr()),
                       C.c_void_p(terms.data_ptr()), C.c_void_p(weights.data_ptr()), Q, int(pool), int(k),
                       int(rrf_k), _ptr(t) if per_query else t, C.c_void_p(lists.data_ptr()), C.c_void_p(sc.data_ptr()),
                       C.c_void_p(keys.data_ptr()), C.c_void_p(rrf.data_ptr()),
                       C.c_void_p(ranks.data_ptr()), st), name)
        return keys, rrf, ranks

    def set_temporal(self, temporal):
        """Per-row temporal scores (float64 [n_rows], e.g. shard_format.temporal_scores) for hybrid_linear_dev; None clears."""
        t = None if temporal is None else _np(temporal, np.float64)
        self._check(self.lib.rag_index_set_temporal_host(self.h, _ptr(t), 0 if t is None else t.shape[0]), "rag_index_set_temporal_host")

    def hybrid_linear_dev(self, q, term_ptr, terms, k, alpha, beta, gamma, tenant=-1, stream=None):
        """hybrid_search over the whole resident index (CUDA tensors in): returns dict of CUDA tensors ids [Q,k] int64, rows
        [Q,k] int32, hybrid / semantic / keyword / temporal [Q,k] float64."""
        import torch
        Q, dev = q.shape[0], q.device
        key = ("lin", Q, k)
        if getattr(self, "_lin_key", None) != key:
            f64 = torch.float64
            self._lin = dict(ids=torch.empty((Q, k), dtype=torch.int64, device=dev), rows=torch.empty((Q, k), dtype=torch.int32, device=dev),
                             hybrid=torch.empty((Q, k), dtype=f64, device=dev), semantic=torch.empty((Q, k), dtype=f64, device=dev),
                             keyword=torch.empty((Q, k), dtype=f64, device=dev), temporal=torch.empty((Q, k), dtype=f64, device=dev))
            self._lin_key = key
        o = self._lin
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = (self.lib.rag_hybrid_linear_tenants_dev, "rag_hybrid_linear_tenants_dev") if per_query else (self.lib.rag_hybrid_linear_dev, "rag_hybrid_linear_dev")
        self._check(fn(
            self.h, C.c_void_p(q.data_ptr()), C.c_void_p(term_ptr.data_ptr()), C.c_void_p(terms.data_ptr()), Q, int(k), float(alpha),
            float(beta), float(gamma), _ptr(t) if per_query else t, C.c_void_p(o["ids"].data_ptr()), C.c_void_p(o["rows"].data_ptr()),
            C.c_void_p(o["hybrid"].data_ptr()), C.c_void_p(o["semantic"].data_ptr()), C.c_void_p(o["keyword"].data_ptr()),
            C.c_void_p(o["temporal"].data_ptr()), st), name)
        return o

    # ---- hybrid_linear_dev over row shards: begin -> gather of the maxima -> finish -> gather of the blocks -> merge -----------
    def hybrid_linear_batch(self):
        """Queries one hybrid_linear_begin_dev / _finish_dev pair takes on the index as it stands (the sub-batch of hybrid_linear_dev)."""
        n = C.c_int(0)
        self._check(self.lib.rag_hybrid_linear_batch(self.h, C.byref(n)), "rag_hybrid_linear_batch")
        return int(n.value)

    def hybrid_linear_begin_dev(self, term_ptr, terms, local_max_out, tenant=-1, stream=None):
        """First half of hybrid_linear_dev: local_max_out [Q] float64 <- this handle's largest raw BM25 score per query (-inf: no
        visible document of the query's tenant). tenant: an int or one number per query, the same for the finish."""
        import torch
        Q = term_ptr.shape[0] - 1
        if local_max_out.dtype != torch.float64 or local_max_out.numel() < Q or not local_max_out.is_contiguous():
            raise RagError("hybrid_linear_begin_dev: local_max_out must be a contiguous float64 tensor of n_queries elements")
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = ((self.lib.rag_hybrid_linear_begin_tenants_dev, "rag_hybrid_linear_begin_tenants_dev") if per_query
                    else (self.lib.rag_hybrid_linear_begin_dev, "rag_hybrid_linear_begin_dev"))
        self._check(fn(self.h, C.c_void_p(term_ptr.data_ptr()), C.c_void_p(terms.data_ptr()), int(Q), _ptr(t) if per_query else t,
                       C.c_void_p(local_max_out.data_ptr()), st), name)
        return local_max_out

    def hybrid_linear_finish_dev(self, q, gathered_max, k, alpha, beta, gamma, partial_out, tenant=-1, stream=None):
        """Second half: gathered_max [world, Q] float64 (every rank's local maxima) -> partial_out [5, Q, k] int64 = ids | hybrid |
        semantic | keyword | temporal (float64 bits), this handle's top-k under the GLOBAL maximum."""
        import torch
        Q = q.shape[0]
        if gathered_max.dtype != torch.float64 or gathered_max.dim() != 2 or gathered_max.shape[1] != Q or not gathered_max.is_contiguous():
            raise RagError("hybrid_linear_finish_dev: gathered_max must be a contiguous float64 [world, n_queries] tensor")
        if partial_out.dtype != torch.int64 or tuple(partial_out.shape) != (5, Q, int(k)) or not partial_out.is_contiguous():
            raise RagError("hybrid_linear_finish_dev: partial_out must be a contiguous int64 [5, n_queries, k] tensor")
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = ((self.lib.rag_hybrid_linear_finish_tenants_dev, "rag_hybrid_linear_finish_tenants_dev") if per_query
                    else (self.lib.rag_hybrid_linear_finish_dev, "rag_hybrid_linear_finish_dev"))
        self._check(fn(self.h, C.c_void_p(q.data_ptr()), C.c_void_p(gathered_max.data_ptr()), int(gathered_max.shape[0]), int(Q), int(k),
                       float(alpha), float(beta), float(gamma), _ptr(t) if per_query else t, C.c_void_p(partial_out.data_ptr()), st), name)
        return partial_out

    def hybrid_linear_merge_gathered_dev(self, gathered, ids_out, hybrid_out, semantic_out=None, keyword_out=None, temporal_out=None,
                                         stream=None):
        """gathered [world, 5, Q, k] int64 (every rank's partial_out) -> the global top-k by (hybrid desc, id asc): ids_out [Q, k]
        int64, hybrid_out and the optional component outputs [Q, k] float64. Needs no index."""
        import torch
        if gathered.dtype != torch.int64 or gathered.dim() != 4 or gathered.shape[1] != 5 or not gathered.is_contiguous():
            raise RagError("hybrid_linear_merge_gathered_dev: gathered must be a contiguous int64 [world, 5, n_queries, k] tensor")
        world, _, Q, k = gathered.shape
        for name, o, dt in (("ids_out", ids_out, torch.int64), ("hybrid_out", hybrid_out, torch.float64), ("semantic_out", semantic_out, torch.float64),
                            ("keyword_out", keyword_out, torch.float64), ("temporal_out", temporal_out, torch.float64)):
            if o is not None and (o.dtype != dt or tuple(o.shape) != (Q, k) or not o.is_contiguous()):
                raise RagError(f"hybrid_linear_merge_gathered_dev: {name} must be a contiguous {dt} [n_queries, k] tensor")
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        self._check(self.lib.rag_hybrid_linear_merge_gathered_dev(self.h, p(gathered), int(world), int(Q), int(k), p(ids_out), p(hybrid_out),
                                                                  p(semantic_out), p(keyword_out), p(temporal_out), st),
                    "rag_hybrid_linear_merge_gathered_dev")

    def bm25_scores(self, term_ptr, terms):
        term_ptr = _np(term_ptr, np.int32)
        terms = _np(terms, np.int32)
        Q = term_ptr.shape[0] - 1
        out = np.zeros((Q, self.bm25_docs), dtype=np.float64)
        self._check(self.lib.rag_bm25_scores_host(self.h, _ptr(term_ptr), _ptr(terms), Q, _ptr(out)), "rag_bm25_scores_host")
        return out

    def bm25_scores_adhoc(self, indptr, doc, tf, doc_len, idf, avgdl, term_ptr, terms, k1=1.5, b=0.75):
        """Raw BM25 scores [Q, n_docs] of an ad-hoc corpus (CSR as bm25_load); the resident postings are not touched."""
        indptr, doc, tf = _np(indptr, np.int64), _np(doc, np.int32), _np(tf, np.int32)
        doc_len, idf = _np(doc_len, np.int32), _np(idf, np.float64)
        term_ptr, terms = _np(term_ptr, np.int32), _np(terms, np.int32)
        Q = term_ptr.shape[0] - 1
        out = np.zeros((Q, doc_len.shape[0]), dtype=np.float64)
        self._check(self.lib.rag_bm25_scores_adhoc_host(self.h, _ptr(indptr), _ptr(doc), _ptr(tf), _ptr(doc_len), _ptr(idf),
                                                        doc_len.shape[0], idf.shape[0], float(avgdl), float(k1), float(b),
                                                        _ptr(term_ptr), _ptr(terms), Q, _ptr(out)), "rag_bm25_scores_adhoc_host")
        return out

    # ---- cross-encoder ----------------------------------------------------------------------------
    def ce_load(self, cfg, tensors):
        c = CeConfig(cfg["vocab_size"], cfg["hidden"], cfg["layers"], cfg["heads"], cfg["ffn"], cfg["max_pos"],
                     cfg.get("type_vocab", 2), 0, float(cfg.get("eps", 1e-12)))
        arrs = [_np(t, np.float32) for t in tensors]
        ptrs = (_P * len(arrs))(*[a.ctypes.data for a in arrs])
        self._check(self.lib.rag_ce_load_host(self.h, C.byref(c), ptrs, len(arrs)), "rag_ce_load_host")

    # ---- local embedding model (BERT encoder + mean pooling) ---------------------------------------
    def embed_load(self, cfg, tensors, normalize=True, pooling="mean"):
        """tensors: rag_ce_load_host's order WITHOUT the pooler / classifier (cross_encoder.flatten_state_dict(..., head=False)).
        pooling: "mean" over the real tokens, or "cls" (the last hidden state of row 0; no pooler dense / tanh)."""
        if pooling not in ("mean", "cls"):
            raise ValueError(f"embed_load: unsupported pooling mode {pooling!r} (mean or cls)")
        flags = (EMBED_NORMALIZE if normalize else 0) | (EMBED_POOL_CLS if pooling == "cls" else 0)
        c = CeConfig(cfg["vocab_size"], cfg["hidden"], cfg["layers"], cfg["heads"], cfg["ffn"], cfg["max_pos"],
                     cfg.get("type_vocab", 2), 0, float(cfg.get("eps", 1e-12)))
        arrs = [_np(t, np.float32) for t in tensors]
        ptrs = (_P * len(arrs))(*[a.ctypes.data for a in arrs])
        self._check(self.lib.rag_embed_load_host(self.h, C.byref(c), ptrs, len(arrs), flags), "rag_embed_load_host")
        self.embed_hidden = int(cfg["hidden"])
        self.embed_tok_dim = 0                                 # a load drops the heads (embed_heads_load)

    def model_seq_limit(self, which):
        """The longest seq_len a call on the loaded cross-encoder (which = 0) or embedder (1) may have: min(max_pos, 512 with
        32-wide heads, 8192 with 64-wide heads). RagError (RAG_ERR_STATE) when none is loaded."""
        out = C.c_int()
        self._check(self.lib.rag_model_seq_limit(self.h, int(which), C.byref(out)), "rag_model_seq_limit")
        return int(out.value)

    def ce_length_class(self, head_dim, seq_len):
        """The attention length class a call of seq_len runs in on a model of that head width; host-only, no GPU. RagError when the
        width is not 32 or 64 or seq_len is outside [1, that width's limit]."""
        out = C.c_int()
        rc = self.lib.rag_ce_length_class(int(head_dim), int(seq_len), C.byref(out))
        if rc != 0:
            raise RagError(f"rag_ce_length_class(head_dim={head_dim}, seq_len={seq_len}) failed ({rc})")
        return int(out.value)

    def embed(self, input_ids, token_type_ids, lens):
        """int32 [n, L], [n, L], [n] (numpy) -> float32 [n, hidden] sentence embeddings."""
        ids, tt, ln = _np(input_ids, np.int32), _np(token_type_ids, np.int32), _np(lens, np.int32)
        n, L = ids.shape
        out = np.empty((n, self.embed_hidden), dtype=np.float32)
        self._check(self.lib.rag_embed_host(self.h, _ptr(ids), _ptr(tt), _ptr(ln), n, L, _ptr(out)), "rag_embed_host")
        return out

    def embed_dev(self, input_ids, token_type_ids, lens, out, stream=None):
        """int32 CUDA tensors [n, L], [n, L], [n] -> float32 out [n, hidden]; asynchronous on `stream`."""
        import torch
        n, L = input_ids.shape
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_embed_dev(self.h, C.c_void_p(input_ids.data_ptr()), C.c_void_p(token_type_ids.data_ptr()),
                                           C.c_void_p(lens.data_ptr()), n, L, C.c_void_p(out.data_ptr()), st), "rag_embed_dev")

    # ---- token-vector and lexical heads of the embedder (bge-m3's three heads, ColBERT checkpoints) ------------
    def embed_heads_load(self, tok_w=None, tok_b=None, lex_w=None, lex_b=0.0):
        """Attach the token-vector head (tok_w [tok_dim, hidden], tok_b [tok_dim] or None) and / or the lexical head (lex_w [hidden]
        or [1, hidden], lex_b) to the loaded embedder. A head that is not given stays as it was; embed_load drops both."""
        tw = None if tok_w is None else _np(tok_w, np.float32)
        tb = None if tok_b is None else _np(tok_b, np.float32).reshape(-1)
        lw = None if lex_w is None else _np(lex_w, np.float32).reshape(-1)
        hidden = getattr(self, "embed_hidden", None)
        if tw is not None and (tw.ndim != 2 or (hidden is not None and tw.shape[1] != hidden) or (tb is not None and tb.shape[0] != tw.shape[0])):
            raise RagError(f"embed_heads_load: token head of shape {tw.shape} does not fit hidden {hidden}")
        if lw is not None and hidden is not None and lw.shape[0] != hidden:
            raise RagError(f"embed_heads_load: lexical head of {lw.shape[0]} weights does not fit hidden {hidden}")
        self._check(self.lib.rag_embed_heads_load_host(self.h, _ptr(tw), _ptr(tb), 0 if tw is None else tw.shape[0], _ptr(lw),
                                                       float(np.asarray(lex_b, dtype=np.float64).reshape(-1)[0])), "rag_embed_heads_load_host")
        if tw is not None:
            self.embed_tok_dim = int(tw.shape[0])

    def embed_multi(self, input_ids, token_type_ids, lens, dense=True, lexical=True, tokens=True, tok_rows_cap=None):
        """One forward, up to three outputs: (dense [n, hidden] | None, lexical weights [n, L] | None, token vectors
        [rows, tok_dim] packed text after text | None, row_off [n + 1] int64). Text i owns rows row_off[i]:row_off[i + 1]
        (clamped len - 1 of them). tok_rows_cap (default: exactly what the call needs) below that is an error."""
        ids, tt, ln = _np(input_ids, np.int32), _np(token_type_ids, np.int32), _np(lens, np.int32)
        n, L = ids.shape
        d = np.empty((n, self.embed_hidden), dtype=np.float32) if dense else None
        lx = np.empty((n, L), dtype=np.float32) if lexical else None
        tk = None
        cap = 0
        if tokens:
            cap = int((np.clip(ln, 1, L).astype(np.int64) - 1).sum()) if tok_rows_cap is None else int(tok_rows_cap)
            tk = np.empty((cap, int(getattr(self, "embed_tok_dim", 0))), dtype=np.float32)
        off = np.empty((n + 1,), dtype=np.int64)
        self._check(self.lib.rag_embed_multi_host(self.h, _ptr(ids), _ptr(tt), _ptr(ln), n, L, _ptr(d), _ptr(lx), _ptr(tk), cap, _ptr(off)),
                    "rag_embed_multi_host")
        if tk is not None:
            tk = tk[:int(off[n])]
        return d, lx, tk, off

    def embed_multi_dev(self, input_ids, token_type_ids, lens, dense=None, lex=None, tok=None, row_off=None, stream=None):
        """int32 CUDA tensors [n, L], [n, L], [n] -> whichever of dense [n, hidden], lex [n, L], tok [cap, tok_dim] float32 and
        row_off [n + 1] int64 CUDA tensors are given; asynchronous on `stream`. Token rows past tok's capacity are dropped and
        row_off[n] still holds the true total."""
        import torch
        n, L = input_ids.shape
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self._check(self.lib.rag_embed_multi_dev(self.h, p(input_ids), p(token_type_ids), p(lens), n, L, p(dense), p(lex), p(tok),
                                                 0 if tok is None else int(tok.shape[0]), p(row_off), st), "rag_embed_multi_dev")

    def maxsim(self, q_vecs, q_off, d_vecs, d_off, pair_q, pair_d):
        """Late interaction over packed float32 token vectors: out[p] = mean over the rows of query pair_q[p] of the largest dot
        with a row of document pair_d[p]; 0 for an index outside its side or an empty side. Returns float32 [n_pairs]."""
        q, d = _np(q_vecs, np.float32), _np(d_vecs, np.float32)
        qo, do = _np(q_off, np.int64), _np(d_off, np.int64)
        pq, pd = _np(pair_q, np.int32), _np(pair_d, np.int32)
        dim = q.shape[1] if q.ndim == 2 and q.shape[0] else d.shape[1]
        out = np.zeros((pq.shape[0],), dtype=np.float32)
        self._check(self.lib.rag_maxsim_host(self.h, _ptr(q), _ptr(qo), qo.shape[0] - 1, _ptr(d), _ptr(do), do.shape[0] - 1, _ptr(pq), _ptr(pd),
                                             pq.shape[0], int(dim), _ptr(out)), "rag_maxsim_host")
        return out

    def maxsim_dev(self, q_vecs, q_off, d_vecs, d_off, pair_q, pair_d, out, stream=None):
        """CUDA tensors: float32 [rows, dim] vectors, int64 offsets, int32 pairs -> float32 out [n_pairs]; asynchronous on `stream`."""
        import torch
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())
        self._check(self.lib.rag_maxsim_dev(self.h, p(q_vecs), p(q_off), q_off.shape[0] - 1, p(d_vecs), p(d_off), d_off.shape[0] - 1, p(pair_q),
                                            p(pair_d), pair_q.shape[0], int(q_vecs.shape[1]), p(out), st), "rag_maxsim_dev")

    def lexical_match(self, q_ids, q_weights, q_lens, d_ids, d_weights, d_lens, pair_q, pair_d, skip_ids=()):
        """Lexical match of pairs: sum over shared token ids of (largest weight in q) * (largest weight in d); weights <= 0 and the
        ids in skip_ids (at most 8) contribute nothing. ids / weights [n, L], lens [n] per side. Returns float32 [n_pairs]."""
        qi, qw, ql = _np(q_ids, np.int32), _np(q_weights, np.float32), _np(q_lens, np.int32)
        di, dw, dl = _np(d_ids, np.int32), _np(d_weights, np.float32), _np(d_lens, np.int32)
        pq, pd = _np(pair_q, np.int32), _np(pair_d, np.int32)
        sk = _np(list(skip_ids), np.int32)
        out = np.zeros((pq.shape[0],), dtype=np.float32)
        self._check(self.lib.rag_lexical_match_host(self.h, _ptr(qi), _ptr(qw), _ptr(ql), qi.shape[0], qi.shape[1], _ptr(di), _ptr(dw), _ptr(dl),
                                                    di.shape[0], di.shape[1], _ptr(pq), _ptr(pd), pq.shape[0], _ptr(sk), sk.shape[0], _ptr(out)),
                    "rag_lexical_match_host")
        return out

    def lexical_match_dev(self, q_ids, q_weights, q_lens, d_ids, d_weights, d_lens, pair_q, pair_d, out, skip_ids=(), stream=None):
        """The same on CUDA tensors (skip_ids stays a host sequence); float32 out [n_pairs], asynchronous on `stream`."""
        import torch
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())
        sk = _np(list(skip_ids), np.int32)
        self._check(self.lib.rag_lexical_match_dev(self.h, p(q_ids), p(q_weights), p(q_lens), q_ids.shape[0], q_ids.shape[1], p(d_ids),
                                                   p(d_weights), p(d_lens), d_ids.shape[0], d_ids.shape[1], p(pair_q), p(pair_d),
                                                   pair_q.shape[0], _ptr(sk), sk.shape[0], p(out), st), "rag_lexical_match_dev")

    def lexical_compact(self, ids, weights, lens, skip_ids=(), terms_cap=None):
        """Per-position lexical weights -> every text's sparse vector: ids / weights [n, L], lens [n] -> (term_ptr int32 [n + 1],
        terms int32, weights float32), each text's distinct ids ascending with the largest weight > 0 each carries; the ids in
        skip_ids (at most 8), ids < 0 and weights that are not > 0 are left out. The arrays LexicalPostings.encode_queries builds
        from encode_multi's maps. terms_cap (default: n * L, always enough) below the call's total is an error."""
        ii, ww, ln = _np(ids, np.int32), _np(weights, np.float32), _np(lens, np.int32)
        n, L = ii.shape
        sk = _np(list(skip_ids), np.int32)
        cap = n * L if terms_cap is None else int(terms_cap)
        ptr = np.zeros((n + 1,), dtype=np.int32)
        terms, qw = np.empty((max(cap, 1),), dtype=np.int32), np.empty((max(cap, 1),), dtype=np.float32)
        self._check(self.lib.rag_lexical_compact_host(self.h, _ptr(ii), _ptr(ww), _ptr(ln), n, L, _ptr(sk), sk.shape[0], _ptr(ptr), _ptr(terms),
                                                      _ptr(qw), cap), "rag_lexical_compact_host")
        return ptr, terms[:int(ptr[n])].copy(), qw[:int(ptr[n])].copy()

    def lexical_compact_dev(self, ids, weights, lens, term_ptr, terms, qweights, skip_ids=(), stream=None):
        """The same on CUDA tensors (skip_ids stays a host sequence): int32 term_ptr [n + 1], int32 terms and float32 qweights of
        one capacity (n * L always suffices); asynchronous on `stream`. Entries past the capacity are dropped and term_ptr[n]
        still holds the true total."""
        import torch
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        sk = _np(list(skip_ids), np.int32)
        cap = 0 if terms is None else int(terms.shape[0])
        self._check(self.lib.rag_lexical_compact_dev(self.h, p(ids), p(weights), p(lens), ids.shape[0], ids.shape[1], _ptr(sk), sk.shape[0],
                                                     p(term_ptr), p(terms), p(qweights), cap, st), "rag_lexical_compact_dev")

    # ---- resident token-vector store and late-interaction rerank (rag_tokvec_*, rag_retrieve_maxsim_dev) ---------
    TOKVEC_FORMS = {"fp16": 0, "mxfp8": 1}

    def _tokvec_form_code(self, form, what):
        """"fp16" / "mxfp8" -> RAG_TOKVEC_*; an integer goes to the library as it is (which rejects one it does not know)"""
        if isinstance(form, str):
            if form not in self.TOKVEC_FORMS:
                raise RagError(f"{what}: unknown form {form!r} (one of {sorted(self.TOKVEC_FORMS)})")
            return self.TOKVEC_FORMS[form]
        return int(form)

    def tokvec_reserve(self, n_docs_total, rows_total, dim, form="fp16"):
        """Room for n_docs_total documents and rows_total token-vector rows of `dim`; replaces any earlier store. form "fp16" (2 B
        per component) or "mxfp8" (E4M3 codes with a power-of-two scale per 32 components: 33/64 of the bytes, for capacity)."""
        self._check(self.lib.rag_tokvec_reserve_form(self.h, int(n_docs_total), int(rows_total), int(dim),
                                                     self._tokvec_form_code(form, "tokvec_reserve")), "rag_tokvec_reserve_form")
        self._tv_dim = int(dim)

    def tokvec_form(self):
        """"fp16" or "mxfp8": the form of the resident token-vector store; None without one."""
        f = C.c_int()
        self._check(self.lib.rag_tokvec_form(self.h, C.byref(f)), "rag_tokvec_form")
        return {v: k for k, v in self.TOKVEC_FORMS.items()}.get(int(f.value))

    def _tokvec_dim_check(self, width, what):
        if int(width) != getattr(self, "_tv_dim", int(width)):
            raise RagError(f"{what}: vectors of width {int(width)} for a store of dim {self._tv_dim}")

    def _tokvec_rerank_check(self, q_shape, q_rows_used, what):
        """query vectors must be as wide as the store (the library reads rows of the STORE's dim) and hold every row the offsets name
        (q_rows_used; None for device offsets, which are trusted as in maxsim_dev)"""
        dim = self.tokvec_info()["dim"]
        if dim and (len(q_shape) != 2 or int(q_shape[1]) != dim):
            raise RagError(f"{what}: query vectors of shape {tuple(q_shape)} for a store of dim {dim}")
        if q_rows_used is not None and q_rows_used > int(q_shape[0]):
            raise RagError(f"{what}: the query offsets end at row {q_rows_used}, past the {int(q_shape[0])} query rows")

    def tokvec_append(self, vecs, row_off):
        """The next documents from host arrays: float32 [rows, dim], int64 row offsets [n + 1] (taken relative to row_off[0])."""
        v, off = _np(vecs, np.float32), _np(row_off, np.int64)
        if v.ndim != 2 or off.ndim != 1 or off.shape[0] < 1:
            raise RagError("tokvec_append: expected vectors [rows, dim] and offsets [n + 1]")
        self._tokvec_dim_check(v.shape[1], "tokvec_append")
        if off.shape[0] > 1 and int(off[-1]) > v.shape[0]:
            raise RagError("tokvec_append: the offsets end past the vectors")
        self._check(self.lib.rag_tokvec_append_host(self.h, _ptr(v), _ptr(off), off.shape[0] - 1), "rag_tokvec_append_host")

    def tokvec_append_dev(self, vecs, row_off, n_docs=None, stream=None):
        """The same from CUDA tensors - the tok / row_off outputs of embed_multi_dev as they are; waits for `stream` and returns once
        the rows are resident and checked."""
        import torch
        assert vecs.is_cuda and vecs.dtype == torch.float32 and vecs.is_contiguous() and row_off.is_cuda and row_off.dtype == torch.int64
        self._tokvec_dim_check(vecs.shape[1], "tokvec_append_dev")
        n = row_off.shape[0] - 1 if n_docs is None else int(n_docs)
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_tokvec_append_dev(self.h, C.c_void_p(vecs.data_ptr()), C.c_void_p(row_off.data_ptr()), n, st),
                    "rag_tokvec_append_dev")

    def tokvec_load(self, vecs, offsets, form="fp16"):
        """reserve + append of a whole store from host arrays: float32 [rows, dim], int64 offsets [n_docs + 1]; form as tokvec_reserve."""
        v, off = _np(vecs, np.float32), _np(offsets, np.int64)
        if v.ndim != 2 or off.ndim != 1 or off.shape[0] < 2 or int(off[-1]) > v.shape[0]:
            raise RagError("tokvec_load: expected vectors [rows, dim] and offsets [n_docs + 1] that end inside them")
        self._check(self.lib.rag_tokvec_load_form_host(self.h, _ptr(v), _ptr(off), off.shape[0] - 1, int(v.shape[1]),
                                                       self._tokvec_form_code(form, "tokvec_load")), "rag_tokvec_load_form_host")
        self._tv_dim = int(v.shape[1])

    def tokvec_info(self):
        """{"n_docs", "rows", "dim", "hbm_bytes"} of the resident token-vector store (all 0 without one)."""
        docs, rows, dim, nb = C.c_int64(), C.c_int64(), C.c_int(), C.c_int64()
        self._check(self.lib.rag_tokvec_info(self.h, C.byref(docs), C.byref(rows), C.byref(dim), C.byref(nb)), "rag_tokvec_info")
        return {"n_docs": int(docs.value), "rows": int(rows.value), "dim": int(dim.value), "hbm_bytes": int(nb.value)}

    def tokvec_fetch(self, doc):
        """The stored (fp16-rounded, or code * 2^e of the 8-bit form) rows of one document as float32 [n, dim]."""
        dim = self.tokvec_info()["dim"]
        n = C.c_int64()
        rc = self.lib.rag_tokvec_fetch_host(self.h, int(doc), None, 0, C.byref(n))
        if rc != 0 and n.value <= 0:
            self._check(rc, "rag_tokvec_fetch_host")
        out = np.empty((int(n.value), dim), dtype=np.float32)
        if n.value:
            self._check(self.lib.rag_tokvec_fetch_host(self.h, int(doc), _ptr(out), int(n.value), C.byref(n)), "rag_tokvec_fetch_host")
        return out

    def tokvec_rerank(self, q_vecs, q_off, cand_rows, k):
        """MaxSim of each query's token vectors (float32 [rows, dim], int64 q_off [Q + 1]) against its candidate rows (int32
        [Q, pool], -1 = empty) over the resident store -> (ids [Q, k] int64, rows [Q, k] int32, scores [Q, k] float64,
        pair_scores [Q, pool] float32): score descending, equal scores in candidate order, -1 / -1 / 0.0 padded."""
        q, qo, cand = _np(q_vecs, np.float32), _np(q_off, np.int64), _np(cand_rows, np.int32)
        if q.ndim != 2 or cand.ndim != 2 or qo.shape != (cand.shape[0] + 1,):
            raise RagError("tokvec_rerank: expected query vectors [rows, dim], offsets [Q + 1] and candidate rows [Q, pool]")
        self._tokvec_rerank_check(q.shape, int(qo[-1]), "tokvec_rerank")
        Q, pool = cand.shape
        ids, rows = np.empty((Q, k), dtype=np.int64), np.empty((Q, k), dtype=np.int32)
        sc, ps = np.empty((Q, k), dtype=np.float64), np.empty((Q, pool), dtype=np.float32)
        self._check(self.lib.rag_tokvec_rerank_host(self.h, _ptr(q), _ptr(qo), _ptr(cand), Q, pool, int(k), _ptr(ids), _ptr(rows), _ptr(sc),
                                                    _ptr(ps)), "rag_tokvec_rerank_host")
        return ids, rows, sc, ps

    def tokvec_rerank_dev(self, q_vecs, q_off, cand_rows, k, ids_out, rows_out, scores_out, pair_scores_out=None, stream=None):
        """The same on CUDA tensors (rows_out / pair_scores_out may be None); asynchronous on `stream`."""
        import torch
        Q, pool = cand_rows.shape
        self._tokvec_rerank_check(tuple(q_vecs.shape), None, "tokvec_rerank_dev")
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self._check(self.lib.rag_tokvec_rerank_dev(self.h, p(q_vecs), p(q_off), p(cand_rows), int(Q), int(pool), int(k), p(ids_out), p(rows_out),
                                                   p(scores_out), p(pair_scores_out), st), "rag_tokvec_rerank_dev")

    def retrieve_maxsim_dev(self, q_emb, q_vecs, q_off, pool, k, term_ptr=None, terms=None, weights=None, rrf_k=60, tenant=-1, stream=None):
        """Dense (term_ptr None) or dense + learned-sparse RRF candidates -> MaxSim over the resident token vectors -> top-k, all on
        the device (CUDA tensors). Returns (ids [Q, k] int64, scores [Q, k] float64, candidates [Q, pool] int64)."""
        import torch
        Q, dev = q_emb.shape[0], q_emb.device
        key = ("rm", Q, pool, k)
        if getattr(self, "_rm_key", None) != key:
            self._rm = (torch.empty((Q, k), dtype=torch.int64, device=dev), torch.empty((Q, k), dtype=torch.float64, device=dev),
                        torch.empty((Q, pool), dtype=torch.int64, device=dev))
            self._rm_key = key
        ids, sc, cand = self._rm
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        mode = 0 if term_ptr is None else 1
        self._tokvec_rerank_check(tuple(q_vecs.shape), None, "retrieve_maxsim_dev")
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = ((self.lib.rag_retrieve_maxsim_tenants_dev, "rag_retrieve_maxsim_tenants_dev") if per_query
                    else (self.lib.rag_retrieve_maxsim_dev, "rag_retrieve_maxsim_dev"))
        self._check(fn(self.h, p(q_emb), p(term_ptr), p(terms), p(weights), p(q_vecs), p(q_off), int(Q), int(pool),
                       int(k), int(rrf_k), _ptr(t) if per_query else t, mode, p(ids), p(sc), p(cand), st), name)
        return ids, sc, cand

    def tokvec_search_dev(self, q_vecs, q_off, k, pool=None, tenant=-1, stream=None):
        """Exhaustive MaxSim search (mode 2 of rag_retrieve_maxsim_dev): every document of the resident token-vector store that
        the query may see is scored against the query's token vectors (CUDA tensors: q_vecs float32 [rows, dim], q_off int64
        [Q + 1]); no candidate stage, no query embedding. tenant: an int, or one number per query. pool (default k, at most 256)
        is how many of the best are ranked. Returns (ids [Q, k] int64, scores [Q, k] float64, candidates [Q, pool] int64 = the
        ids of the whole top-pool): score descending, the lower row first on equal scores, -1 / 0.0 padded; a score has the bits
        tokvec_rerank_dev reports for the pair. Asynchronous on `stream`."""
        import torch
        Q, dev = int(q_off.shape[0]) - 1, q_vecs.device
        pool = int(k) if pool is None else int(pool)
        key = ("ts", Q, pool, int(k), str(dev))
        if getattr(self, "_ts_key", None) != key:
            self._ts = (torch.empty((Q, k), dtype=torch.int64, device=dev), torch.empty((Q, k), dtype=torch.float64, device=dev),
                        torch.empty((Q, pool), dtype=torch.int64, device=dev))
            self._ts_key = key
        ids, sc, cand = self._ts
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._tokvec_rerank_check(tuple(q_vecs.shape), None, "tokvec_search_dev")
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = ((self.lib.rag_retrieve_maxsim_tenants_dev, "rag_retrieve_maxsim_tenants_dev") if per_query
                    else (self.lib.rag_retrieve_maxsim_dev, "rag_retrieve_maxsim_dev"))
        self._check(fn(self.h, None, None, None, None, p(q_vecs), p(q_off), int(Q), int(pool), int(k), 60,
                       _ptr(t) if per_query else t, 2, p(ids), p(sc), p(cand), st), name + " (mode 2)")
        return ids, sc, cand

    # ---- the three-way bge-m3 score over resident data (rag_sparse_score_rows_*, rag_m3_score_rows_dev, rag_retrieve_m3_dev) ----
    def sparse_score_rows(self, term_ptr, terms, weights, cand_rows):
        """The exact learned-sparse score of given rows: weighted queries (CSR as sparse_topk) and int32 rows [Q, pool] -> float64
        [Q, pool], the bits of sparse_scores(...)[q][row]; 0.0 for a slot < 0 or past the covered documents."""
        term_ptr, terms, weights = _np(term_ptr, np.int32), _np(terms, np.int32), _np(weights, np.float32)
        cand = _np(cand_rows, np.int32)
        if cand.ndim != 2 or term_ptr.shape != (cand.shape[0] + 1,):
            raise RagError("sparse_score_rows: expected term_ptr [Q + 1] and candidate rows [Q, pool]")
        Q, pool = cand.shape
        out = np.empty((Q, pool), dtype=np.float64)
        self._check(self.lib.rag_sparse_score_rows_host(self.h, _ptr(term_ptr), _ptr(terms), _ptr(weights), _ptr(cand), Q, pool, _ptr(out)),
                    "rag_sparse_score_rows_host")
        return out

    def sparse_score_rows_dev(self, term_ptr, terms, weights, cand_rows, scores_out, stream=None):
        """The same on CUDA tensors (int32 term arrays and rows, float32 weights, float64 scores_out [Q, pool]); asynchronous on `stream`."""
        import torch
        Q, pool = cand_rows.shape
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self._check(self.lib.rag_sparse_score_rows_dev(self.h, p(term_ptr), p(terms), p(weights), p(cand_rows), int(Q), int(pool), p(scores_out),
                                                       st), "rag_sparse_score_rows_dev")

    def m3_score_rows_dev(self, cand_rows, k, ids_out, scores_out, q_emb=None, term_ptr=None, terms=None, weights=None, q_vecs=None, q_off=None,
                          w=(0.4, 0.2, 0.4), rows_out=None, components_out=None, stream=None):
        """bge-m3's "colbert+sparse+dense" score of given rows (int32 [Q, pool], CUDA tensors throughout) and its top k: w = (dense,
        sparse, colbert); a weight of 0 leaves its component - and its inputs - out. components_out [Q, k, 3] float64 = (dense,
        sparse, colbert) of every returned row. Asynchronous on `stream`."""
        import torch
        Q, pool = cand_rows.shape
        if q_vecs is not None and float(w[2]) > 0:
            self._tokvec_rerank_check(tuple(q_vecs.shape), None, "m3_score_rows_dev")
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self._check(self.lib.rag_m3_score_rows_dev(self.h, p(q_emb), p(term_ptr), p(terms), p(weights), p(q_vecs), p(q_off), p(cand_rows), int(Q),
                                                   int(pool), int(k), float(w[0]), float(w[1]), float(w[2]), p(ids_out), p(rows_out),
                                                   p(scores_out), p(components_out), st), "rag_m3_score_rows_dev")

    def retrieve_m3_dev(self, q_emb, pool, k, term_ptr=None, terms=None, weights=None, q_vecs=None, q_off=None, mode=2, w=(0.4, 0.2, 0.4),
                        rrf_k=60, tenant=-1, stream=None):
        """Candidates -> three-way score -> top-k in one device-resident call (CUDA tensors). mode 0: dense top-pool; 1: dense +
        learned-sparse RRF top-pool; 2: the union of the dense and the sparse top-pool (2 * pool slots, pool <= 128). Returns (ids
        [Q, k] int64, scores [Q, k] float64, components [Q, k, 3] float64 = (dense, sparse, colbert), candidates [Q, slots] int64)."""
        import torch
        Q, dev = q_emb.shape[0], q_emb.device
        slots = 2 * int(pool) if int(mode) == 2 else int(pool)
        key = ("m3", Q, slots, k)
        if getattr(self, "_m3_key", None) != key:
            self._m3 = (torch.empty((Q, k), dtype=torch.int64, device=dev), torch.empty((Q, k), dtype=torch.float64, device=dev),
                        torch.empty((Q, k, 3), dtype=torch.float64, device=dev), torch.empty((Q, slots), dtype=torch.int64, device=dev))
            self._m3_key = key
        ids, sc, comp, cand = self._m3
        if q_vecs is not None and float(w[2]) > 0:
            self._tokvec_rerank_check(tuple(q_vecs.shape), None, "retrieve_m3_dev")
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = (self.lib.rag_retrieve_m3_tenants_dev, "rag_retrieve_m3_tenants_dev") if per_query else (self.lib.rag_retrieve_m3_dev, "rag_retrieve_m3_dev")
        self._check(fn(self.h, p(q_emb), p(term_ptr), p(terms), p(weights), p(q_vecs), p(q_off), int(Q), int(pool),
                       int(k), int(rrf_k), _ptr(t) if per_query else t, int(mode), float(w[0]), float(w[1]), float(w[2]), p(ids),
                       p(sc), p(comp), p(cand), st), name)
        return ids, sc, comp, cand

    # ---- the row-sharded three-way search: the steps between the two all-gathers (sharded.ShardedM3Index drives them) ----------
    def m3_candidates_gathered_dev(self, gathered, lists_out, scores_out, cand_out, mode=2, rrf_k=60, stream=None):
        """gathered [world, 4, Q, pool] int64 (every rank's dense ids | cosine bits | sparse ids | raw sparse score bits) -> merged
        lists [2, Q, pool] int64, their scores [2, Q, pool] float64 and the candidate ids [Q, slots] int64 of retrieve_m3_dev's
        mode (slots = 2 * pool in mode 2, else pool). CUDA tensors; needs no index."""
        import torch
        world, _, Q, pool = gathered.shape
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self._check(self.lib.rag_m3_candidates_gathered_dev(self.h, p(gathered), int(world), int(Q), int(pool), int(rrf_k), int(mode),
                                                            p(lists_out), p(scores_out), p(cand_out), st), "rag_m3_candidates_gathered_dev")

    def m3_score_ids_dev(self, cand_ids, partial_out, q_emb=None, term_ptr=None, terms=None, weights=None, q_vecs=None, q_off=None,
                         w=(0.4, 0.2, 0.4), stream=None):
        """The three components of the candidate ids [Q, slots] int64 whose rows this handle holds (id_base <= id < id_base + rows; explicit ids: the id map's answer, index_id_map)
        -> partial_out [4, Q, slots] int64 = owned flag | dense | sparse | colbert (float64 bits; 0 / 0.0 for a slot of another
        rank). A weight of 0 leaves its component - and its inputs - out."""
        import torch
        Q, slots = cand_ids.shape
        if q_vecs is not None and float(w[2]) > 0:
            self._tokvec_rerank_check(tuple(q_vecs.shape), None, "m3_score_ids_dev")
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self._check(self.lib.rag_m3_score_ids_dev(self.h, p(q_emb), p(term_ptr), p(terms), p(weights), p(q_vecs), p(q_off), p(cand_ids), int(Q),
                                                  int(slots), float(w[0]), float(w[1]), float(w[2]), p(partial_out), st), "rag_m3_score_ids_dev")

    def m3_combine_gathered_dev(self, cand_ids, gathered, ids_out, scores_out, components_out=None, w=(0.4, 0.2, 0.4), stream=None):
        """cand_ids [Q, slots] and every rank's partial block, gathered [world, 4, Q, slots] int64 -> the top k = ids_out.shape[1] of
        retrieve_m3_dev: ids [Q, k] int64, scores [Q, k] float64, components [Q, k, 3] float64 (may be None). Needs no index."""
        import torch
        world, _, Q, slots = gathered.shape
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self._check(self.lib.rag_m3_combine_gathered_dev(self.h, p(cand_ids), p(gathered), int(world), int(Q), int(slots), int(ids_out.shape[1]),
                                                         float(w[0]), float(w[1]), float(w[2]), p(ids_out), p(scores_out), p(components_out), st),
                    "rag_m3_combine_gathered_dev")

    def search_m3_tokens_dev(self, input_ids, token_type_ids, lens, pool, k, skip_ids=(), mode=2, w=(0.4, 0.2, 0.4), rrf_k=60, tenant=-1,
                             stream=None):
        """Query token ids -> the three-way ranking in ONE device-resident call (rag_search_m3_tokens_dev / _tenants_dev): the forward
        of the handle's embedder, the compaction of its lexical weights and retrieve_m3_dev, with the same bits as those three calls
        made one after another. int32 CUDA tensors [Q, L], [Q, L], [Q]; the other arguments and the result are retrieve_m3_dev's."""
        import torch
        Q, L = input_ids.shape
        dev = input_ids.device
        slots = 2 * int(pool) if int(mode) == 2 else int(pool)
        key = ("m3", Q, slots, k)
        if getattr(self, "_m3_key", None) != key:
            self._m3 = (torch.empty((Q, k), dtype=torch.int64, device=dev), torch.empty((Q, k), dtype=torch.float64, device=dev),
                        torch.empty((Q, k, 3), dtype=torch.float64, device=dev), torch.empty((Q, slots), dtype=torch.int64, device=dev))
            self._m3_key = key
        ids, sc, comp, cand = self._m3
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        sk = _np(list(skip_ids), np.int32)
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = (self.lib.rag_search_m3_tokens_tenants_dev, "rag_search_m3_tokens_tenants_dev") if per_query else \
            (self.lib.rag_search_m3_tokens_dev, "rag_search_m3_tokens_dev")
        self._check(fn(self.h, p(input_ids), p(token_type_ids), p(lens), int(Q), int(L), _ptr(sk), sk.shape[0], int(pool), int(k), int(rrf_k),
                       _ptr(t) if per_query else t, int(mode), float(w[0]), float(w[1]), float(w[2]), p(ids), p(sc), p(comp), p(cand), st), name)
        return ids, sc, comp, cand

    def tokens_load(self, tokens, lens, id_bits=16):
        """Passage token store: tokens [N, L] int32 token ids without [CLS]/[SEP], lens [N]; row-aligned with the index.
        id_bits=24 (rag_tokens_load_wide_host) holds ids up to 16777215 at 3 B per token: XLM-R's 250k-entry vocabulary."""
        tokens = _np(tokens, np.int32)
        lens = _np(lens, np.int32)
        if int(id_bits) == 16:
            self._check(self.lib.rag_tokens_load_host(self.h, _ptr(tokens), _ptr(lens), tokens.shape[0], tokens.shape[1]),
                        "rag_tokens_load_host")
        else:
            self._check(self.lib.rag_tokens_load_wide_host(self.h, _ptr(tokens), _ptr(lens), tokens.shape[0], tokens.shape[1], int(id_bits)),
                        "rag_tokens_load_wide_host")
        self._tok_L = int(tokens.shape[1])

    def tokens_reserve(self, n_rows_total, L, id_bits=16):
        if int(id_bits) == 16:
            self._check(self.lib.rag_tokens_reserve(self.h, int(n_rows_total), int(L)), "rag_tokens_reserve")
        else:
            self._check(self.lib.rag_tokens_reserve_wide(self.h, int(n_rows_total), int(L), int(id_bits)), "rag_tokens_reserve_wide")
        self._tok_L = int(L)

    def tokens_info(self):
        """{"rows", "L", "id_bits"} of the resident token store (all 0 without one)."""
        rows, L, bits = C.c_int64(), C.c_int(), C.c_int()
        self._check(self.lib.rag_tokens_info(self.h, C.byref(rows), C.byref(L), C.byref(bits)), "rag_tokens_info")
        return {"rows": int(rows.value), "L": int(L.value), "id_bits": int(bits.value)}

    def ce_set_pair_format(self, fmt):
        """Layout the pair builder writes from now on: PAIR_BERT (0, [cls] q [sep] d [sep], types 0 | 1) or PAIR_ROBERTA
        (1, [cls] q [sep] [sep] d [sep], all type 0). Applies to retrieve_rerank_dev and ce_build_pairs_dev."""
        self._check(self.lib.rag_ce_set_pair_format(self.h, int(fmt)), "rag_ce_set_pair_format")

    def tokens_append_dev(self, tokens, lens, stream=None):
        """Append a row block of the passage token store from device memory: tokens [n, L] int32, lens [n] int32 CUDA tensors."""
        import torch
        assert tokens.is_cuda and tokens.dtype == torch.int32 and tokens.is_contiguous() and lens.dtype == torch.int32
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_tokens_append_dev(self.h, C.c_void_p(tokens.data_ptr()), C.c_void_p(lens.data_ptr()), tokens.shape[0], st),
                    "rag_tokens_append_dev")

    def hybrid_fuse_gathered_dev(self, gathered, k, lists_out, scores_out, keys_out, rrf_out, ranks_out, rrf_k=60, stream=None):
        """gathered [world, 4, Q, pool] int64 (every rank's dense ids | cosine bits | BM25 ids | raw BM25 bits) -> merged lists
        [2, Q, pool], scores [2, Q, pool] (BM25 / global max), RRF keys / scores [Q, k], ranks [Q, k, 2]. CUDA tensors."""
        import torch
        world, _, Q, pool = gathered.shape
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_hybrid_fuse_gathered_dev(
            self.h, C.c_void_p(gathered.data_ptr()), int(world), int(Q), int(pool), int(k), int(rrf_k), C.c_void_p(lists_out.data_ptr()),
            C.c_void_p(scores_out.data_ptr()), C.c_void_p(keys_out.data_ptr()), C.c_void_p(rrf_out.data_ptr()),
            C.c_void_p(ranks_out.data_ptr()), st), "rag_hybrid_fuse_gathered_dev")

    def retrieve_rerank_dev(self, q_emb, q_tok, q_len, pool, k, term_ptr=None, terms=None, rrf_k=60, tenant=-1, L_pair=512,
                            cls_id=101, sep_id=102, stream=None):
        """Dense (term_ptr None) or hybrid candidates -> cross-encoder -> top-k, all on the device (CUDA tensors).
        Returns (ids [Q,k] int64, scores [Q,k] float64 sigmoid, logits [Q,k] float32, candidates [Q,pool] int64)."""
        import torch
        Q, dev = q_emb.shape[0], q_emb.device
        key = ("rr", Q, pool, k)
        if getattr(self, "_rr_key", None) != key:
            self._rr = (torch.empty((Q, k), dtype=torch.int64, device=dev), torch.empty((Q, k), dtype=torch.float64, device=dev),
                        torch.empty((Q, k), dtype=torch.float32, device=dev), torch.empty((Q, pool), dtype=torch.int64, device=dev))
            self._rr_key = key
        ids, sc, lg, cand = self._rr
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        mode = 0 if term_ptr is None else 1
        per_query, t = _tenant_arg(tenant, Q)
        fn, name = ((self.lib.rag_retrieve_rerank_tenants_dev, "rag_retrieve_rerank_tenants_dev") if per_query
                    else (self.lib.rag_retrieve_rerank_dev, "rag_retrieve_rerank_dev"))
        self._check(fn(
            self.h, C.c_void_p(q_emb.data_ptr()), C.c_void_p(term_ptr.data_ptr() if mode else 0),
            C.c_void_p(terms.data_ptr() if mode else 0), C.c_void_p(q_tok.data_ptr()), C.c_void_p(q_len.data_ptr()),
            int(q_tok.shape[1]), Q, int(pool), int(k), int(rrf_k), _ptr(t) if per_query else t, mode, int(cls_id), int(sep_id), int(L_pair),
            C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_void_p(lg.data_ptr()), C.c_void_p(cand.data_ptr()), st),
            name)
        return ids, sc, lg, cand

    def ce_build_pairs_dev(self, q_tok, q_len, cand, ids_out, tt_out, lens_out, token_id_base=0, cls_id=101, sep_id=102, stream=None):
        """[CLS] query [SEP] passage [SEP] rows for a [Q, pool] table of GLOBAL candidate ids (-1 = empty) against the
        loaded token store; ids_out / tt_out are [Q*pool, L_pair] int32, lens_out [Q*pool]."""
        import torch
        Q, pool = cand.shape
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_ce_build_pairs_dev(self.h, C.c_void_p(q_tok.data_ptr()), C.c_void_p(q_len.data_ptr()), int(q_tok.shape[1]),
                                                    C.c_void_p(cand.data_ptr()), Q, pool, int(token_id_base), int(ids_out.shape[1]),
                                                    int(cls_id), int(sep_id), C.c_void_p(ids_out.data_ptr()),
                                                    C.c_void_p(tt_out.data_ptr()), C.c_void_p(lens_out.data_ptr()), st),
                    "rag_ce_build_pairs_dev")

    def rerank_topk_dev(self, logits, cand, ids_out, scores_out, logits_out, stream=None):
        """sigmoid + stable (score desc, candidate order) top-k of logits [Q*pool] over the candidate table [Q, pool]."""
        import torch
        Q, pool = cand.shape
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_rerank_topk_dev(self.h, C.c_void_p(logits.data_ptr()), C.c_void_p(cand.data_ptr()), Q, pool,
                                                 int(ids_out.shape[1]), C.c_void_p(ids_out.data_ptr()),
                                                 C.c_void_p(scores_out.data_ptr()), C.c_void_p(logits_out.data_ptr()), st),
                    "rag_rerank_topk_dev")

    def ce_score_dev(self, input_ids, token_type_ids, lens, logits_out, stream=None):
        """int32 CUDA tensors [P, L], [P, L], [P] -> float32 logits_out [P]; asynchronous on `stream`."""
        import torch
        P, L = input_ids.shape
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        self._check(self.lib.rag_ce_score_dev(self.h, C.c_void_p(input_ids.data_ptr()), C.c_void_p(token_type_ids.data_ptr()),
                                              C.c_void_p(lens.data_ptr()), P, L, C.c_void_p(logits_out.data_ptr()), st),
                    "rag_ce_score_dev")

    def ce_score(self, input_ids, token_type_ids, lens):
        ids = _np(input_ids, np.int32)
        tt = _np(token_type_ids, np.int32)
        ln = _np(lens, np.int32)
        P, L = ids.shape
        out = np.empty((P,), dtype=np.float32)
        self._check(self.lib.rag_ce_score_host(self.h, _ptr(ids), _ptr(tt), _ptr(ln), P, L, _ptr(out)), "rag_ce_score_host")
        return out
