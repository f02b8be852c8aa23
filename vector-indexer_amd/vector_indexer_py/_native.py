"""ctypes declarations for libvi_amd.so (include/vi_amd.h).  No torch, no CPU fallback."""
import ctypes as C
import os

VI_OK, VI_ERR_INVALID_INPUT, VI_ERR_NOT_FOUND, VI_ERR_INVALID_DATA, VI_ERR_OTHER, VI_ERR_IO, VI_ERR_PANIC, \
    VI_ERR_DEVICE = range(8)
VI_ORDER_SCALAR, VI_ORDER_LANES = 0, 1
VI_ASSIGN_REFERENCE, VI_ASSIGN_EXACT = 0, 1
VI_IDS_ALLOW, VI_IDS_DENY = 0, 1
VI_FILTER_MAX_TERMS = 8
VI_TERM_TIMESTAMPS, VI_TERM_ID_RANGE, VI_TERM_IDS, VI_TERM_IDS_DEVICE, VI_TERM_MASK, VI_TERM_MASK_DEVICE, VI_TERM_FILTER = range(7)
VI_JOIN_AND, VI_JOIN_OR = 0, 1

_STATUS_NAME = {1: "InvalidInput", 2: "NotFound", 3: "InvalidData", 4: "Other", 5: "Io", 6: "Panic", 7: "Device"}

LIB_PATH = os.environ.get("VI_AMD_LIB") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                      "libvi_amd.so")

u64, u32, i32, i64, f32 = C.c_uint64, C.c_uint32, C.c_int32, C.c_int64, C.c_float
vp = C.c_void_p


class ViError(RuntimeError):
    """RuntimeError carrying the io::ErrorKind-like status of the failed call."""

    def __init__(self, status, message):
        super().__init__(message)
        self.status = status
        self.kind = _STATUS_NAME.get(status, str(status))


class Config(C.Structure):
    _fields_ = [("dimension", u32), ("index_dir", C.c_char_p), ("shards_dir", C.c_char_p),
                ("default_k", u64), ("default_n_probe", u64), ("max_k", u64), ("max_n_probe", u64),
                ("nlist_override", u64), ("seed", u64), ("assign_mode", i32), ("device", i32),
                ("rank", i32), ("world_size", i32), ("now_secs", u64), ("placement", i32), ("reserved0", i32)]


class SearchStats(C.Structure):
    _fields_ = [("nq", u64), ("k", u64), ("n_probe_eff", u64), ("coarse_candidates", u64),
                ("scanned_vectors", u64), ("scan_items", u64), ("ms_total", f32), ("ms_coarse", f32),
                ("ms_group", f32), ("ms_scan", f32), ("ms_merge", f32), ("fallback_queries", u64),
                ("filter_tile_blocks", u64), ("filter_rechecked", u64), ("filter_accepted", u64),
                ("rank_mode", u64), ("group_queries", u64), ("rank_int8", u64)]


class BuildStats(C.Structure):
    _fields_ = [("n", u64), ("nlist", u64), ("lists", u64), ("shards", u64), ("shard_bytes", u64), ("ms_total", f32),
                ("ms_upload", f32), ("ms_kmeans", f32), ("ms_group", f32), ("ms_super", f32), ("ms_export", f32),
                ("ms_index", f32)]


class AddStats(C.Structure):
    _fields_ = [("n", u64), ("lists_touched", u64), ("shards_rewritten", u64), ("bytes_written", u64), ("ms_total", f32),
                ("ms_assign", f32), ("ms_files", f32), ("ms_index", f32), ("ms_kernel", f32), ("kernel_bytes", u64)]


class RemoveStats(C.Structure):
    _fields_ = [("n_removed", u64), ("lists_touched", u64), ("lists_emptied", u64), ("shards_rewritten", u64),
                ("bytes_written", u64), ("ms_total", f32), ("ms_plan", f32), ("ms_files", f32), ("ms_index", f32),
                ("ms_kernel", f32), ("kernel_bytes", u64)]


class UpsertStats(C.Structure):
    _fields_ = [("n", u64), ("n_replaced", u64), ("lists_touched", u64), ("lists_emptied", u64), ("shards_rewritten", u64),
                ("bytes_written", u64), ("ms_total", f32), ("ms_plan", f32), ("ms_files", f32), ("ms_index", f32),
                ("ms_kernel", f32), ("kernel_bytes", u64)]


class RefineStats(C.Structure):
    """vi_refine_stats"""
    _fields_ = [("iterations_run", u64), ("moved", u64), ("lists_emptied", u64), ("shards_rewritten", u64),
                ("bytes_written", u64), ("means_bytes", u64), ("rehome_bytes", u64), ("ms_total", f32), ("ms_means", f32),
                ("ms_label", f32), ("ms_rehome", f32), ("ms_images", f32), ("ms_files", f32), ("ms_means_kernel", f32),
                ("ms_rehome_kernel", f32)]


class RebalanceRuleC(C.Structure):
    """vi_rebalance_rule"""
    _fields_ = [("iters", u64), ("split_rounds", u64), ("split_factor", C.c_double), ("receiver_max_len", u64),
                ("max_splits", u64), ("split_iters", u32), ("reserved0", u32)]


class RebalanceStats(C.Structure):
    """vi_rebalance_stats: the fields of vi_refine_stats, then the split steps"""
    _fields_ = RefineStats._fields_ + [("pairs_planned", u64), ("splits_done", u64), ("splits_skipped", u64),
                                       ("inner_iterations", u64), ("split_bytes", u64), ("ms_split", f32),
                                       ("ms_split_kernels", f32)]


class ListStats(C.Structure):
    """vi_list_stats"""
    _fields_ = [("lists", u64), ("empty_lists", u64), ("min_len", u64), ("max_len", u64), ("mean_len", C.c_double),
                ("imbalance", C.c_double)]


class FetchStats(C.Structure):
    _fields_ = [("n", u64), ("n_found", u64), ("slots_scanned", u64), ("bytes_moved", u64), ("ms_total", f32),
                ("ms_table", f32), ("ms_match", f32), ("ms_gather", f32)]


class ClusterStats(C.Structure):
    """vi_cluster_stats"""
    _fields_ = [("rows", u64), ("hits", u64), ("passes", u64), ("n_core", u64), ("n_border", u64), ("n_noise", u64),
                ("n_clusters", u64), ("chunk_rows", u64), ("link_bytes", u64), ("ms_resolve", f32), ("ms_search", f32),
                ("ms_link", f32), ("ms_label", f32)]


class ProbeRuleC(C.Structure):
    """vi_probe_rule"""
    _fields_ = [("min_probe", u32), ("ratio2", f32), ("max_codes", u64), ("n_probe_q", vp)]


class FilterTerm(C.Structure):
    """vi_filter_term: one term of vi_indexer_filter_compose"""
    _fields_ = [("kind", u32), ("negate", u32), ("lo", u64), ("hi", u64), ("data", vp), ("n", u64), ("filter", vp)]


WHERE_NONE = (1 << 64) - 1   # VI_WHERE_NONE


FETCH_ROWS_FN =C.CFUNCTYPE(C.c_int, vp, C.POINTER(u64), u64, vp)


class RowSource(C.Structure):
    """vi_row_source: fetch_rows(ctx, global_rows, n_rows, out_dev) -> 0 on success"""
    _fields_ = [("ctx", vp), ("fetch_rows", FETCH_ROWS_FN)]


class AssignStats(C.Structure):
    _fields_ = [("n", u64), ("k", u64), ("ambiguous_rows", u64), ("used_mfma", u32), ("ms_total", f32),
                ("ms_filter", f32), ("tier1_rows", u64), ("ambiguous_rows_dev", vp), ("ambiguous_cap", u64)]


SIGNATURES = {
    "vi_last_error": (C.c_char_p, []),
    "vi_abi_version": (u32, []),
    "vi_device_count": (C.c_int, []),
    "vi_calculate_num_clusters": (u64, [u64]),
    "vi_calculate_max_iterations": (u64, [u64]),
    "vi_minibatch_size": (u64, [u64]),
    "vi_l2sq_pairs": (C.c_int, [vp, vp, u64, u32, C.c_int, vp]),
    "vi_assign": (C.c_int, [vp, u64, u32, vp, u64, u64, C.c_int, vp, vp]),
    "vi_assign_device": (C.c_int, [i32, vp, u64, u32, vp, u64, u64, C.c_int, vp, vp]),
    "vi_kmeans_mini_batch": (C.c_int, [vp, u64, u32, u64, u64, f32, u64, C.c_int, vp, vp, C.POINTER(u64)]),
    "vi_kmeans_parallel": (C.c_int, [vp, u64, u32, u64, u64, f32, u64, C.c_int, vp, vp, C.POINTER(u64)]),
    "vi_kmeans_mini_batch_device": (C.c_int, [i32, vp, u64, u32, u64, u64, f32, u64, C.c_int, vp, vp, C.POINTER(u64)]),
    "vi_kmeans_parallel_device": (C.c_int, [i32, vp, u64, u32, u64, u64, f32, u64, C.c_int, vp, vp, C.POINTER(u64)]),
    "vi_kmeans_mini_batch_train": (C.c_int, [i32, vp, u64, u32, u64, u64, f32, u64, vp, C.POINTER(u64)]),
    "vi_kmeans_pp_init": (C.c_int, [i32, vp, u64, u32, u64, u64, vp]),
    "vi_kmeans_partial_sums_device": (C.c_int, [i32, vp, u64, u32, vp, u64, vp, vp]),
    "vi_kmeans_finish_update_device": (C.c_int, [i32, vp, vp, u64, u32, vp, vp, C.POINTER(f32), vp, C.POINTER(u64)]),
    "vi_kmeans_centroid_delta_device": (C.c_int, [i32, vp, vp, u64, u32, C.POINTER(f32)]),
    "vi_rng_seed_from_u64": (vp, [u64]),
    "vi_rng_gen_range": (u64, [vp, u64, u64]),
    "vi_rng_free": (None, [vp]),
    "vi_shard_save_to": (C.c_int, [C.c_char_p, u64, u32, u32, vp, vp, vp, vp, vp, vp, vp]),
    "vi_shard_get_centroid_vectors_from": (C.c_int, [C.c_char_p, u64, vp, u64, C.POINTER(u32), vp, vp, vp, vp]),
    "vi_shard_append_to": (C.c_int, [C.c_char_p, u64, u64, vp, vp, vp, vp, vp]),
    "vi_config_init": (None, [C.POINTER(Config), u32]),
    "vi_indexer_new": (C.c_int, [C.POINTER(Config), C.POINTER(vp)]),
    "vi_indexer_load": (C.c_int, [C.POINTER(Config), C.POINTER(vp)]),
    "vi_indexer_build_from_records": (C.c_int, [vp, vp, vp, vp, vp, u64]),
    "vi_indexer_build_from_vector_file": (C.c_int, [vp, C.c_char_p]),
    "vi_indexer_add_records": (C.c_int, [vp, vp, vp, vp, u64]),
    "vi_indexer_search": (C.c_int, [vp, vp, u64, u32, u64, u64, vp, vp, vp, vp, C.POINTER(u64)]),
    "vi_indexer_search_device": (C.c_int, [vp, vp, u64, u64, u64, vp, vp, vp]),
    "vi_indexer_probe_device": (C.c_int, [vp, vp, u64, u64, vp, vp, C.POINTER(u64)]),
    "vi_indexer_search_probed_device": (C.c_int, [vp, vp, u64, u64, u64, vp, vp, vp, vp, vp]),
    "vi_indexer_filter_timestamps": (C.c_int, [vp, u64, u64, C.POINTER(vp)]),
    "vi_indexer_filter_ids": (C.c_int, [vp, vp, u64, C.c_int, C.POINTER(vp)]),
    "vi_indexer_filter_ids_device": (C.c_int, [vp, vp, u64, C.c_int, C.POINTER(vp)]),
    "vi_filter_intersect": (C.c_int, [vp, vp, vp, C.POINTER(vp)]),
    "vi_indexer_filter_compose": (C.c_int, [vp, C.c_int, C.POINTER(FilterTerm), u32, vp, C.POINTER(vp)]),
    "vi_filter_union": (C.c_int, [vp, vp, vp, C.POINTER(vp)]),
    "vi_filter_complement": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "vi_indexer_filter_id_range": (C.c_int, [vp, u64, u64, C.POINTER(vp)]),
    "vi_indexer_filter_mask": (C.c_int, [vp, vp, u64, C.POINTER(vp)]),
    "vi_indexer_filter_mask_device": (C.c_int, [vp, vp, u64, C.POINTER(vp)]),
    "vi_filter_num_allowed": (u64, [vp]),
    "vi_filter_free": (None, [vp]),
    "vi_indexer_search_filtered": (C.c_int, [vp, vp, vp, u64, u32, u64, u64, vp, vp, vp, vp, C.POINTER(u64)]),
    "vi_indexer_search_filtered_device": (C.c_int, [vp, vp, vp, u64, u64, u64, vp, vp, vp]),
    "vi_indexer_search_probed_filtered_device": (C.c_int, [vp, vp, vp, u64, u64, u64, vp, vp, vp, vp, vp]),
    "vi_indexer_range_search": (C.c_int, [vp, vp, vp, u64, u32, f32, u64, C.POINTER(vp)]),
    "vi_indexer_range_search_device": (C.c_int, [vp, vp, vp, u64, f32, u64, C.POINTER(vp)]),
    "vi_range_result_total": (u64, [vp]),
    "vi_range_result_copy": (C.c_int, [vp, vp, vp, vp, vp]),
    "vi_range_result_device": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "vi_range_result_copy_device": (C.c_int, [vp, vp, vp, vp, vp]),
    "vi_range_result_free": (None, [vp]),
    "vi_range_merge_device": (C.c_int, [i32, u64, u32, vp, vp, vp, vp, C.POINTER(vp)]),
    "vi_range_merge_last_times": (C.c_int, [C.POINTER(f32), C.POINTER(f32), C.POINTER(f32)]),
    "vi_merge_partials_device": (C.c_int, [i32, u64, u64, u32, vp, vp, vp, vp, vp]),
    "vi_packed_result_bytes": (u64, [u64, u64]),
    "vi_merge_partials_packed_device": (C.c_int, [i32, u64, u64, u32, vp, vp, vp]),
    "vi_indexer_dimension": (u32, [vp]),
    "vi_indexer_num_centroids": (u64, [vp]),
    "vi_indexer_num_vectors": (u64, [vp]),
    "vi_indexer_num_shards": (u64, [vp]),
    "vi_indexer_centroids": (C.c_int, [vp, vp, vp]),
    "vi_indexer_free": (None, [vp]),
    "vi_indexer_last_stats": (C.c_int, [vp, C.POINTER(SearchStats)]),
    "vi_indexer_enable_timing": (None, [vp, C.c_int]),
    "vi_indexer_last_build_stats": (C.c_int, [vp, C.POINTER(BuildStats)]),
    "vi_indexer_last_add_stats": (C.c_int, [vp, C.POINTER(AddStats)]),
    "vi_indexer_retain": (C.c_int, [vp, vp, C.POINTER(u64)]),
    "vi_indexer_remove_ids": (C.c_int, [vp, vp, u64, C.POINTER(u64)]),
    "vi_shard_remove_from": (C.c_int, [C.c_char_p, u64, vp, u64, C.POINTER(u64)]),
    "vi_indexer_last_remove_stats": (C.c_int, [vp, C.POINTER(RemoveStats)]),
    "vi_indexer_upsert_records": (C.c_int, [vp, vp, vp, vp, u64, C.POINTER(u64)]),
    "vi_shard_upsert_to": (C.c_int, [C.c_char_p, u64, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]),
    "vi_indexer_last_upsert_stats": (C.c_int, [vp, C.POINTER(UpsertStats)]),
    "vi_indexer_refine": (C.c_int, [vp, u64, C.POINTER(u64)]),
    "vi_indexer_last_refine_stats": (C.c_int, [vp, C.POINTER(RefineStats)]),
    "vi_rebalance_rule_init": (None, [C.POINTER(RebalanceRuleC)]),
    "vi_indexer_rebalance": (C.c_int, [vp, C.POINTER(RebalanceRuleC), C.POINTER(u64)]),
    "vi_indexer_last_rebalance_stats": (C.c_int, [vp, C.POINTER(RebalanceStats)]),
    "vi_indexer_list_stats": (C.c_int, [vp, C.POINTER(ListStats)]),
    "vi_indexer_get_records": (C.c_int, [vp, vp, u64, vp, vp, vp, vp]),
    "vi_indexer_get_records_device": (C.c_int, [vp, vp, u64, vp, vp, vp, vp]),
    "vi_indexer_export_records": (C.c_int, [vp, u64, u64, vp, vp, vp, vp]),
    "vi_indexer_export_records_device": (C.c_int, [vp, u64, u64, vp, vp, vp, vp]),
    "vi_indexer_last_fetch_stats": (C.c_int, [vp, C.POINTER(FetchStats)]),
    "vi_indexer_search_by_ids": (C.c_int, [vp, vp, vp, u64, u64, u64, u32, vp, vp, vp, vp, vp, C.POINTER(u64)]),
    "vi_indexer_search_by_ids_device": (C.c_int, [vp, vp, vp, u64, u64, u64, u32, vp, vp, vp, vp]),
    "vi_indexer_knn_graph": (C.c_int, [vp, vp, u64, u64, u64, u64, u32, vp, vp, vp, C.POINTER(u64)]),
    "vi_indexer_knn_graph_device": (C.c_int, [vp, vp, u64, u64, u64, u64, u32, vp, vp, vp]),
    "vi_similar_last_times": (C.c_int, [C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), C.POINTER(u64), C.POINTER(u64)]),
    "vi_indexer_range_search_by_ids": (C.c_int, [vp, vp, vp, u64, f32, u64, u32, vp, C.POINTER(vp)]),
    "vi_indexer_range_search_by_ids_device": (C.c_int, [vp, vp, vp, u64, f32, u64, u32, vp, C.POINTER(vp)]),
    "vi_indexer_radius_graph": (C.c_int, [vp, vp, u64, u64, f32, u64, u32, C.POINTER(vp)]),
    "vi_indexer_cluster_radius": (C.c_int, [vp, vp, f32, u64, u32, vp, vp, C.POINTER(u64)]),
    "vi_indexer_cluster_radius_device": (C.c_int, [vp, vp, f32, u64, u32, vp, vp, C.POINTER(u64)]),
    "vi_cluster_last_stats": (C.c_int, [C.POINTER(ClusterStats)]),
    "vi_indexer_prune_probes_device": (C.c_int, [vp, vp, u64, u64, vp, vp, C.POINTER(ProbeRuleC), vp]),
    "vi_indexer_search_adaptive": (C.c_int, [vp, vp, C.POINTER(ProbeRuleC), vp, u64, u32, u64, u64, vp, vp, vp, vp, vp,
                                             C.POINTER(u64)]),
    "vi_indexer_search_adaptive_device": (C.c_int, [vp, vp, C.POINTER(ProbeRuleC), vp, u64, u64, u64, vp, vp, vp, vp]),
    "vi_prune_last_stats": (C.c_int, [C.POINTER(u64), C.POINTER(u64), C.POINTER(f32)]),
}

_lib = None


def lib():
    """Load libvi_amd.so.  Raises (never falls back) when the HIP library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ViError(VI_ERR_DEVICE, f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def id_array(ids):
    """any integer array-like of external ids -> flat contiguous uint64 (every u64 is an id; negatives are an error)"""
    import numpy as np
    if not isinstance(ids, np.ndarray):
        ids = list(ids)
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in ids):
            raise TypeError("ids must be integers")
        if any(x < 0 for x in ids):
            raise ValueError("ids must be non-negative (external ids are u64)")
        return np.array(ids, dtype=np.uint64)   # (python ints: the whole u64 range, which no signed dtype holds)
    if ids.size and ids.dtype.kind not in "iu":
        raise TypeError("ids must be integers")
    if ids.dtype.kind == "i" and (ids < 0).any():
        raise ValueError("ids must be non-negative (external ids are u64)")
    return np.ascontiguousarray(ids.reshape(-1), dtype=np.uint64)


def mask_array(mask):
    """a bool or uint8 array-like with one entry per record -> flat contiguous uint8 (non-zero admits)"""
    import numpy as np
    a = np.asarray(mask)
    if a.dtype != np.bool_ and a.dtype != np.uint8:
        raise TypeError("a mask is a bool or uint8 array")
    return np.ascontiguousarray(a.reshape(-1)).view(np.uint8)


def check(status, prefix=""):
    if status != VI_OK:
        msg = lib().vi_last_error()
        raise ViError(status, prefix + (msg.decode("utf-8", "replace") if msg else f"status {status}"))
