"""ctypes binding of libii2_hip.so — exactly the entry points include/ii2.h declares.

The library is the product; this module only loads it.  It fails loudly when the shared
object is missing (run `python -c "import __graft_entry__ as g; g.build()"`); there is no
Python / CPU fallback for any operation.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libii2_hip.so")

II2_HOST, II2_DEVICE = 0, 1
II2_UNIQUE_ID_BYTES = 128
II2_OP_AND, II2_OP_OR = 0, 1
ERRORS = {0: "OK", -1: "EINVAL", -2: "ENOMEM", -3: "EHIP", -4: "ECAPACITY", -5: "ERANGE", -6: "ECOMM", -7: "ENODEVICE"}


class SegInfo(C.Structure):
    _fields_ = [("n_lists", C.c_uint64), ("n_postings", C.c_uint64), ("n_blocks", C.c_uint64), ("n_bytes", C.c_uint64)]


class SegMetaInfo(C.Structure):
    _fields_ = [("n_postings", C.c_uint64), ("merge_blocks", C.c_uint64), ("merge_bytes", C.c_uint64), ("is_view", C.c_uint32),
                ("spans_mirrored", C.c_uint32)]


class MergeStats(C.Structure):
    _fields_ = [("n_in", C.c_uint64), ("n_out", C.c_uint64), ("n_terms_out", C.c_uint64), ("n_tiles", C.c_uint64)]


class BuildStats(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("n_postings", C.c_uint64), ("n_nonempty", C.c_uint64), ("n_passes", C.c_uint32)]


class DictBuildStats(C.Structure):
    _fields_ = [("n_terms", C.c_uint64), ("n_unique", C.c_uint64), ("n_bytes", C.c_uint64), ("min_len", C.c_uint32), ("max_len", C.c_uint32),
                ("n_passes", C.c_uint32), ("pad", C.c_uint32)]


class MatchStats(C.Structure):
    _fields_ = [("n_terms", C.c_uint64), ("n_matched", C.c_uint64), ("n_runs", C.c_uint64), ("n_staged", C.c_uint32), ("n_global", C.c_uint32)]


II2_MATCH_MAX_PATTERN, II2_MATCH_MAX_PATTERNS = 64, 64
II2_MATCH_CONTAINS, II2_MATCH_SUFFIX, II2_MATCH_GLOB = range(3)
II2_MATCH_NOCASE = 0x80
II2_MATCH_UTF8 = 0x08


class FuzzyStats(C.Structure):
    _fields_ = [("n_terms", C.c_uint64), ("n_matched", C.c_uint64), ("n_runs", C.c_uint64), ("n_tested", C.c_uint64), ("n_staged", C.c_uint32),
                ("n_global", C.c_uint32), ("word_bits", C.c_uint32), ("n_utf8", C.c_uint32)]


II2_FUZZY_MAX_PATTERN, II2_FUZZY_MAX_PATTERNS = 64, 16
II2_FUZZY_TRANSPOSE = 0x01


class RegexStats(C.Structure):
    _fields_ = [("n_terms", C.c_uint64), ("n_matched", C.c_uint64), ("n_runs", C.c_uint64), ("n_tested", C.c_uint64), ("n_staged", C.c_uint32),
                ("n_global", C.c_uint32), ("max_positions", C.c_uint32), ("pad", C.c_uint32)]


II2_REGEX_MAX_PATTERN, II2_REGEX_MAX_POSITIONS, II2_REGEX_MAX_PATTERNS = 256, 64, 8


class AlignPlan(C.Structure):
    _fields_ = [("n_terms", C.c_uint64), ("n_workgroups", C.c_uint64), ("brackets_staged", C.c_uint64), ("brackets_global", C.c_uint64),
                ("brackets_empty", C.c_uint64), ("max_bracket", C.c_uint64), ("long_terms", C.c_uint32), ("terms_per_workgroup", C.c_uint32),
                ("staged_cap", C.c_uint32), ("pad", C.c_uint32)]


class CountStats(C.Structure):
    _fields_ = [("n_lists", C.c_uint64), ("n_blocks", C.c_uint64), ("n_decoded", C.c_uint64), ("n_hits", C.c_uint64),
                ("n_windows", C.c_uint32)]


class HistStats(C.Structure):
    _fields_ = [("n_lists", C.c_uint64), ("n_blocks", C.c_uint64), ("n_decoded", C.c_uint64), ("n_hits", C.c_uint64), ("n_whole", C.c_uint64),
                ("n_split", C.c_uint64), ("n_wide", C.c_uint64), ("n_windows", C.c_uint32), ("n_buckets", C.c_uint32)]


II2_HIST_MAX_BUCKETS, II2_HIST_MAX_CELLS = 4096, 1 << 26
II2_HIST_SKIP, II2_HIST_WHOLE, II2_HIST_SPLIT, II2_HIST_WIDE = 0, 1, 2, 3


class ExplainStats(C.Structure):
    _fields_ = [("n_ids", C.c_uint64), ("n_lists", C.c_uint64), ("n_blocks", C.c_uint64), ("n_decoded", C.c_uint64), ("n_hits", C.c_uint64),
                ("n_windows", C.c_uint32), ("n_words", C.c_uint32), ("log2_slots", C.c_uint32), ("pad", C.c_uint32)]


II2_EXPLAIN_MAX_IDS = 1 << 24


class ExplainBatchStats(C.Structure):
    _fields_ = [("n_tiny", C.c_uint32), ("n_small", C.c_uint32), ("n_single", C.c_uint32), ("n_empty", C.c_uint32), ("n_rows", C.c_uint64),
                ("n_words", C.c_uint64), ("n_hits", C.c_uint64)]


II2_EXPLAIN_BATCH_IDS = 1024
II2_EXPLAIN_BATCH_EMPTY, II2_EXPLAIN_BATCH_TINY, II2_EXPLAIN_BATCH_SMALL, II2_EXPLAIN_BATCH_SINGLE = range(4)


class AtleastStats(C.Structure):
    _fields_ = [("n_counted", C.c_uint64), ("bound", C.c_uint64), ("form", C.c_uint32), ("n_planes", C.c_uint32),
                ("n_windows", C.c_uint32), ("n_late", C.c_uint32)]


class TopkStats(C.Structure):
    _fields_ = [("n_counted", C.c_uint64), ("n_eligible", C.c_uint64), ("n_cut", C.c_uint64), ("max_score", C.c_uint32),
                ("cut_score", C.c_uint32), ("n_planes", C.c_uint32), ("n_windows", C.c_uint32), ("n_marks", C.c_uint32), ("pad", C.c_uint32)]


class TopkwStats(C.Structure):
    _fields_ = [("n_counted", C.c_uint64), ("n_eligible", C.c_uint64), ("n_cut", C.c_uint64), ("total_weight", C.c_uint32),
                ("max_score", C.c_uint32), ("cut_score", C.c_uint32), ("n_planes", C.c_uint32), ("n_windows", C.c_uint32),
                ("n_marks", C.c_uint32), ("n_late", C.c_uint32), ("pad", C.c_uint32)]


class TopkBatchStats(C.Structure):
    _fields_ = [("n_tiny", C.c_uint32), ("n_small", C.c_uint32), ("n_single", C.c_uint32), ("n_empty", C.c_uint32), ("n_staged", C.c_uint64)]


II2_TOPK_MAX = 1 << 20
II2_TOPK_BATCH_EMPTY, II2_TOPK_BATCH_TINY, II2_TOPK_BATCH_SMALL, II2_TOPK_BATCH_SINGLE = range(4)
II2_LB_SEED_MISSING, II2_LB_SEED_READY, II2_LB_SEED_STALE, II2_LB_SEED_LATER = range(4)
II2_LB_GAVE_UP_PREFIX, II2_LB_GAVE_UP_GROUP, II2_LB_NO_PREFIX = 1, 2, 0xFF
II2_ATLEAST_NONE, II2_ATLEAST_SMALL, II2_ATLEAST_COUNT, II2_ATLEAST_AND, II2_ATLEAST_OR = range(5)

vp = C.c_void_p
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
u8p = C.POINTER(C.c_uint8)
vpp = C.POINTER(C.c_void_p)

# name -> (restype, argtypes); every symbol ii2.h declares
PROTOTYPES = {
    "ii2_abi_version": (C.c_int, []),
    "ii2_ctx_create": (C.c_int, [C.c_int, C.c_uint32, vpp]),
    "ii2_ctx_destroy": (None, [vp]),
    "ii2_last_error": (C.c_char_p, [vp]),
    "ii2_ctx_sync": (C.c_int, [vp]),
    "ii2_ctx_stream": (vp, [vp]),
    "ii2_ctx_device": (C.c_int, [vp]),
    "ii2_dev_alloc": (C.c_int, [vp, C.c_size_t, vpp]),
    "ii2_dev_free": (C.c_int, [vp, vp]),
    "ii2_copy_h2d": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "ii2_copy_d2h": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "ii2_seg_encode": (C.c_int, [vp, C.c_uint64, vp, vp, C.c_int, vpp]),
    "ii2_seg_build": (C.c_int, [vp, C.c_uint64, C.c_uint64, vp, vp, C.c_int, vpp, C.POINTER(BuildStats)]),
    "ii2_seg_import": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, vp, vp, vp, C.c_int, vpp]),
    "ii2_seg_decode": (C.c_int, [vp, vp, vp, vp, C.c_int]),
    "ii2_seg_export": (C.c_int, [vp, vp, vp, vp, vp]),
    "ii2_seg_select": (C.c_int, [vp, vp, C.c_uint64, vp, vpp]),
    "ii2_dict_create": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_int, vpp]),
    "ii2_dict_free": (None, [vp]),
    "ii2_dict_find": (C.c_int, [vp, C.c_uint32, vpp, C.c_uint64, vp, vp, vp, C.c_int, vp, vp, u64p]),
    "ii2_term_bounds": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_int, u64p, u64p]),
    "ii2_dict_match": (C.c_int, [vp, C.c_uint32, vpp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.POINTER(MatchStats)]),
    "ii2_term_match": (C.c_int, [C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_int)]),
    "ii2_dict_fuzzy": (C.c_int, [vp, C.c_uint32, vpp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.POINTER(FuzzyStats)]),
    "ii2_term_fuzzy": (C.c_int, [C.c_uint32, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_int), u32p]),
    "ii2_dict_regex": (C.c_int, [vp, C.c_uint32, vpp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.POINTER(RegexStats)]),
    "ii2_term_regex": (C.c_int, [C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_int), u32p]),
    "ii2_utf8_decode": (C.c_int, [vp, C.c_uint64, u32p, C.c_uint64, u64p, C.POINTER(C.c_int)]),
    "ii2_dict_build": (C.c_int, [vp, C.c_uint64, vp, vp, C.c_int, vpp, vp, C.POINTER(DictBuildStats)]),
    "ii2_dict_info": (C.c_int, [vp, u64p, u64p]),
    "ii2_dict_export": (C.c_int, [vp, vp, vp, vp]),
    "ii2_term_chunk": (C.c_int, [vp, C.c_uint64, C.c_uint32, u64p]),
    "ii2_dict_build_plan": (C.c_int, [vp, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ii2_align_dicts": (C.c_int, [vp, C.c_uint32, vpp, vpp]),
    "ii2_align_terms": (C.c_int, [vp, C.c_uint32, vp, vp, vp, vpp]),
    "ii2_align_plan": (C.c_int, [C.c_uint32, vp, vp, vp, C.POINTER(AlignPlan)]),
    "ii2_align_info": (C.c_int, [vp, u64p, C.POINTER(C.c_uint32)]),
    "ii2_align_export": (C.c_int, [vp, vp, vp, vp]),
    "ii2_seg_select_aligned": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint64, vpp]),
    "ii2_seg_select_aligned_all": (C.c_int, [vp, vpp, vp, vp, vpp]),
    "ii2_align_free": (None, [vp]),
    "ii2_seg_get_info": (C.c_int, [vp, C.POINTER(SegInfo)]),
    "ii2_seg_export_meta": (C.c_int, [vp, vp, vp, vp, vp, vp, C.POINTER(SegMetaInfo)]),
    "ii2_seg_free": (None, [vp]),
    "ii2_tomb_create": (C.c_int, [vp, vp, C.c_uint64, C.c_int, vpp]),
    "ii2_tomb_free": (None, [vp]),
    "ii2_merge_segments": (C.c_int, [vp, C.c_uint32, vpp, vp, vp, vp, C.c_uint64, C.POINTER(MergeStats)]),
    "ii2_merge_segments_to_seg": (C.c_int, [vp, C.c_uint32, vpp, vp, vpp, C.POINTER(MergeStats)]),
    "ii2_merge_small": (C.c_int, [vp, C.c_uint32, vpp, vp, vp, vp, vp, C.c_uint64, vpp, u64p, u64p, C.POINTER(MergeStats)]),
    "ii2_seg_dense_form": (C.c_int, [vp, vp, C.c_uint64, vp, vp, C.c_uint64]),
    "ii2_devmem_stats": (None, [u64p, u64p]),
    "ii2_read_small": (C.c_int, [vp, C.c_uint32, vpp, vp, vp, vp, vp, u64p, u64p, vp, C.c_uint64, u64p]),
    "ii2_intersect": (C.c_int, [vp, C.c_uint32, vpp, u64p, vp, vp, C.c_uint64, u64p]),
    "ii2_intersect_async": (C.c_int, [vp, C.c_uint32, vpp, u64p, vp, vp, C.c_uint64, vp]),
    "ii2_union": (C.c_int, [vp, C.c_uint32, vpp, u64p, vp, vp, C.c_uint64, u64p]),
    "ii2_union_ranges": (C.c_int, [vp, C.c_uint64, vpp, u64p, u64p, vp, vp, C.c_uint64, u64p]),
    "ii2_intersect_ranges": (C.c_int, [vp, C.c_uint64, u64p, vpp, u64p, u64p, vp, vp, C.c_uint64, u64p]),
    "ii2_andnot_ranges": (C.c_int, [vp, C.c_uint64, u64p, u8p, vpp, u64p, u64p, vp, vp, C.c_uint64, u64p]),
    "ii2_query_batch": (C.c_int, [vp, C.c_uint64, u8p, u64p, vpp, u64p, u64p, vp, vp, C.c_uint64, u64p]),
    "ii2_query_batch_groups": (C.c_int, [vp, C.c_uint64, u64p, u64p, u8p, vpp, u64p, u64p, vp, vp, C.c_uint64, u64p]),
    "ii2_count_ranges": (C.c_int, [vp, C.c_uint64, vpp, u64p, u64p, vp, C.c_uint64, vp, u64p, C.c_uint64, C.POINTER(CountStats)]),
    "ii2_histogram_ranges": (C.c_int, [vp, C.c_uint64, vpp, u64p, u64p, vp, C.c_uint64, vp, C.c_uint32, u64p, u64p, C.c_uint64, C.POINTER(HistStats)]),
    "ii2_histogram_ids": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint32, u64p, u64p, C.c_uint64]),
    "ii2_hist_bucket": (C.c_int, [u64p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64)]),
    "ii2_hist_block": (C.c_int, [u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), u32p, u32p]),
    "ii2_explain_ranges": (C.c_int, [vp, C.c_uint64, u64p, vpp, u64p, u64p, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(ExplainStats)]),
    "ii2_explain_slot": (C.c_int, [C.c_uint32, C.c_uint32, u32p]),
    "ii2_explain_batch": (C.c_int, [vp, C.c_uint64, u64p, u64p, vpp, u64p, u64p, vp, u64p, vp, C.c_uint64, u64p, C.POINTER(ExplainBatchStats)]),
    "ii2_explain_batch_plan": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, u32p]),
    "ii2_atleast_ranges": (C.c_int, [vp, C.c_uint64, u64p, u8p, C.c_uint32, vpp, u64p, u64p, vp, vp, C.c_uint64, u64p, C.POINTER(AtleastStats)]),
    "ii2_atleast_plan": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, u32p, u64p, u64p]),
    "ii2_atleast_word": (C.c_int, [C.c_uint32, C.c_uint32, u32p, C.c_uint32, u32p]),
    "ii2_topk_ranges": (C.c_int, [vp, C.c_uint64, u64p, u8p, C.c_uint32, C.c_uint64, vpp, u64p, u64p, vp, vp, vp, u64p, u64p, C.POINTER(TopkStats)]),
    "ii2_topk_cut": (C.c_int, [u64p, C.c_uint64, u32p, u32p, u64p, u64p]),
    "ii2_topk_word": (C.c_int, [C.c_uint32, u32p, C.c_uint32, C.c_uint32, u32p]),
    "ii2_topk_weighted_ranges": (C.c_int, [vp, C.c_uint64, u64p, u8p, u32p, C.c_uint32, C.c_uint64, vpp, u64p, u64p, vp, vp, vp, u64p, u64p,
                                           C.POINTER(TopkwStats)]),
    "ii2_topkw_word": (C.c_int, [C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint32, u32p]),
    "ii2_topkw_plan": (C.c_int, [C.c_uint64, u32p, u64p, C.c_uint32, C.c_uint32, u32p, u32p, u64p, u8p, u32p]),
    "ii2_topk_batch": (C.c_int, [vp, C.c_uint64, u64p, u64p, u8p, u32p, u32p, u32p, vpp, u64p, u64p, vp, vp, vp, C.c_uint64, u64p, u64p,
                                 C.POINTER(TopkBatchStats)]),
    "ii2_topk_batch_run": (C.c_int, [u8p, C.c_uint32, C.c_uint32, u8p, u32p, u32p]),
    "ii2_topk_batch_plan": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, u32p, u64p]),
    "ii2_merge_host": (C.c_int, [vp, C.c_uint32, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, C.POINTER(MergeStats)]),
    "ii2_intersect_host": (C.c_int, [vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, C.c_uint64, u64p]),
    "ii2_union_host": (C.c_int, [vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, C.c_uint64, u64p]),
    "ii2_comm_unique_id": (C.c_int, [vp]),
    "ii2_comm_init": (C.c_int, [vp, C.c_int, C.c_int, vp]),
    "ii2_allgatherv": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint64, u64p]),
    "ii2_allgatherv_bytes": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint64, u64p]),
    "ii2_seg_allgather": (C.c_int, [vp, vp, vpp]),
    "ii2_seg_concat": (C.c_int, [vp, C.c_uint32, vpp, vpp]),
    "ii2_seg_gather_plan": (C.c_int, [u64p, C.c_int, u64p, u64p, u64p]),
    "ii2_gatherv_offsets": (C.c_int, [u64p, C.c_int, C.c_uint64, u64p]),
    "ii2_selftest": (C.c_int, [vp]),
    "ii2_set_option": (C.c_int, [vp, C.c_char_p, C.c_int64]),
    "ii2_ctx_counters": (C.c_int, [vp, u64p, C.c_uint32]),
    "ii2_debug_read": (C.c_int, [vp, u64p, C.c_uint64]),
    "ii2_profile_read": (C.c_int, [vp, C.POINTER(C.c_double), u64p]),
    "ii2_profile_region": (C.c_int, [vp, C.c_int]),
    "ii2_profile_region_ms": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "ii2_ctx_paths": (C.c_int, [vp, u64p, C.c_uint32]),
    "ii2_path_name": (C.c_char_p, [C.c_uint32]),
    "ii2_merge_events": (C.c_int, [vp, u64p, C.c_uint32]),
    "ii2_merge_event_name": (C.c_char_p, [C.c_uint32]),
    "ii2_lookback_check": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
}

_lib = None


def load() -> C.CDLL:
    """Loads libii2_hip.so and types every entry point.  Raises if the library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                "(make -C inverted_index_2_amd/csrc). There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)      # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib
