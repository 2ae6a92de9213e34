"""ctypes binding of libreadbouncer_amd.so (the C ABI declared in include/readbouncer_amd.h).

This is plumbing for tests and bench.py: every call goes straight to the HIP library.  There is
no Python or CPU implementation of the hot path here -- if the shared library is missing the
import fails, and if no GPU is visible every compute call raises RBError(RB_ERR_NO_DEVICE).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libreadbouncer_amd.so")

(RB_OK, RB_ERR_NULL_FILTER, RB_ERR_SHORT_READ, RB_ERR_COUNT_KMER, RB_ERR_MISSING_FILE, RB_ERR_PARSE_IBF,
 RB_ERR_BAD_CHUNK, RB_ERR_STORE, RB_ERR_INVALID_ARG, RB_ERR_UNSUPPORTED, RB_ERR_NO_DEVICE, RB_ERR_HIP,
 RB_ERR_NOMEM) = range(13)
RB_MODE_CHECK_UNBLOCK, RB_MODE_CLASSIFY_CHUNK, RB_MODE_CLASSIFY_ANY = 0, 1, 2


class BatchDesc(C.Structure):
    _fields_ = [("d_seqs", C.c_void_p), ("d_offsets", C.c_void_p), ("d_lens", C.c_void_p), ("n_items", C.c_size_t),
                ("max_len", C.c_uint32), ("d_nmask", C.c_void_p), ("d_nmask_offsets", C.c_void_p),
                ("chunk_start", C.c_uint32), ("chunk_length", C.c_uint32), ("d_read_ids", C.c_void_p)]


class LocateOut(C.Structure):
    """rb_locate_out: any member may be NULL, not all"""
    _fields_ = [("max_count", C.c_void_p), ("best_bin", C.c_void_p), ("best_strand", C.c_void_p), ("hit_bins", C.c_void_p),
                ("status", C.c_void_p)]


class PrefixOut(C.Structure):
    """rb_prefix_out: any member may be NULL, not all"""
    _fields_ = [("max_count", C.c_void_p), ("decision", C.c_void_p), ("best_target", C.c_void_p), ("status", C.c_void_p),
                ("prefix_len", C.c_void_p), ("first_decided", C.c_void_p)]


RB_PREFIX_MAX = 64


class ResumeOut(C.Structure):
    """rb_resume_out: any member may be NULL, not all"""
    _fields_ = [("max_count", C.c_void_p), ("decision", C.c_void_p), ("best_target", C.c_void_p), ("status", C.c_void_p),
                ("total_len", C.c_void_p)]


RB_RESUME_FIRST, RB_RESUME_PEEK = 1, 2


class Hit(C.Structure):
    """rb_hit: one (bin, strand) at or above the threshold and its count -- 8 bytes"""
    _fields_ = [("bin", C.c_uint32), ("count", C.c_uint16), ("strand", C.c_uint8), ("reserved", C.c_uint8)]


class HitsOut(C.Structure):
    """rb_hits_out: any member may be NULL, but not hits, n_hits and bin_reads all at once"""
    _fields_ = [("hits", C.c_void_p), ("n_hits", C.c_void_p), ("status", C.c_void_p), ("bin_reads", C.c_void_p)]


# rb_hit as a numpy record
HIT_DTYPE = np.dtype([("bin", "<u4"), ("count", "<u2"), ("strand", "u1"), ("reserved", "u1")])


class Span(C.Structure):
    """rb_span: where along the read one (bin, strand) matched -- 24 bytes"""
    _fields_ = [(n, C.c_uint32) for n in ("count", "first", "last", "run_start", "run_len", "covered")]


class SpanQuery(C.Structure):
    """rb_span_query: (work item, bin)"""
    _fields_ = [("item", C.c_uint32), ("bin", C.c_uint32)]


class SpansOut(C.Structure):
    """rb_spans_out: any member may be NULL, not all"""
    _fields_ = [("spans", C.c_void_p), ("mask", C.c_void_p), ("n_kmers", C.c_void_p), ("status", C.c_void_p)]


# rb_span and rb_span_query as numpy records
SPAN_DTYPE = np.dtype([(n, "<u4") for n in ("count", "first", "last", "run_start", "run_len", "covered")])
SPAN_QUERY_DTYPE = np.dtype([("item", "<u4"), ("bin", "<u4")])


class PlanInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 48), ("table_bytes", C.c_uint64), ("block_words", C.c_uint32), ("stride_words", C.c_uint32),
                ("merged_members", C.c_uint32), ("lanes_per_block_log2", C.c_uint32), ("words_per_lane", C.c_uint32),
                ("column_slices", C.c_uint32), ("counter_planes", C.c_uint32), ("nontemporal", C.c_uint32), ("split_waves", C.c_uint32),
                ("phased", C.c_uint32), ("phase_shape", C.c_uint32), ("phase_shape_name", C.c_char * 64),
                ("phase_slice_log2", C.c_uint32), ("phase_slices", C.c_uint32), ("phase_window_ticks", C.c_uint32),
                ("phase_rule_ticks", C.c_uint32), ("reserved0", C.c_uint32), ("phase_slice_bytes", C.c_uint64),
                ("row_table_bytes", C.c_uint64)]


class RowTableInfo(C.Structure):
    """rb_row_table_info"""
    _fields_ = [("bytes", C.c_uint64), ("rows", C.c_uint64), ("want_bytes", C.c_uint64), ("build_ms", C.c_double), ("alloc_s", C.c_double),
                ("refused", C.c_uint32), ("builds", C.c_uint32)]


# rb_list_table_info and rb_wide_list_table_info: one layout under two names
_LIST_TABLE_INFO_FIELDS = [("bytes", C.c_uint64), ("rows", C.c_uint64), ("side_bytes", C.c_uint64), ("lines", C.c_uint32), ("side_rows", C.c_uint32),
                           ("side_capacity", C.c_uint32), ("refused", C.c_uint32), ("builds", C.c_uint32), ("stride_words", C.c_uint32),
                           ("census_rows", C.c_uint64), ("census_over", C.c_uint64 * 3), ("build_ms", C.c_double), ("alloc_s", C.c_double)]


class ListTableInfo(C.Structure):
    """rb_list_table_info"""
    _fields_ = _LIST_TABLE_INFO_FIELDS


class WideListTableInfo(C.Structure):
    """rb_wide_list_table_info (census_over: rows with more than 256, 384, 512 set bits)"""
    _fields_ = _LIST_TABLE_INFO_FIELDS


class PairTableInfo(C.Structure):
    """rb_pair_table_info (census_over: sampled pairs that need a tail or more, that need dense rows, whose row(x) has more than 128 bins)"""
    _fields_ = [("bytes", C.c_uint64), ("rows", C.c_uint64), ("side_bytes", C.c_uint64), ("tail_bytes", C.c_uint64), ("lines", C.c_uint32),
                ("side_rows", C.c_uint32), ("side_capacity", C.c_uint32), ("tail_rows", C.c_uint32), ("tail_capacity", C.c_uint32),
                ("refused", C.c_uint32), ("builds", C.c_uint32), ("stride_words", C.c_uint32), ("census_rows", C.c_uint64),
                ("census_over", C.c_uint64 * 3), ("census_one_line", C.c_uint64), ("build_ms", C.c_double), ("alloc_s", C.c_double)]


RB_ROW_TABLE_OFF, RB_ROW_TABLE_AUTO, RB_ROW_TABLE_FORCE, RB_ROW_TABLE_LISTS, RB_ROW_TABLE_PAIRS = 0, 1, 2, 3, 4
PAIR_CANON_ENTRIES, PAIR_TAIL_MARK, PAIR_TAIL_DWORDS = 256, 0xFFFD, 32  # rb_pair_lists.h
RB_PASS_LISTS_OFF, RB_PASS_LISTS_CURRENT, RB_PASS_LISTS_BUILD = 0, 1, 2
(RB_LIST_REFUSED_NONE, RB_LIST_REFUSED_K, RB_LIST_REFUSED_GEOMETRY, RB_LIST_REFUSED_MAX_BYTES, RB_LIST_REFUSED_FREE, RB_LIST_REFUSED_ALLOC,
 RB_LIST_REFUSED_CAPTURE, RB_LIST_REFUSED_DENSITY, RB_LIST_REFUSED_SIDE_FULL) = range(9)
LIST_SENTINEL, LIST_OVERFLOW_MARK = 0xFFFF, 0xFFFE  # rb_lists.h
(RB_ROW_REFUSED_NONE, RB_ROW_REFUSED_K, RB_ROW_REFUSED_NARROW, RB_ROW_REFUSED_MAX_BYTES, RB_ROW_REFUSED_FREE, RB_ROW_REFUSED_ALLOC,
 RB_ROW_REFUSED_CAPTURE) = range(7)


class PassPlan(C.Structure):
    """rb_pass_plan: the build the query passes take for one filter"""
    _fields_ = [("lanes_per_block_log2", C.c_uint32), ("words_per_lane", C.c_uint32), ("column_slices", C.c_uint32),
                ("counter_planes", C.c_uint32), ("nontemporal", C.c_uint32), ("hash_functions", C.c_uint32),
                ("spans_nontemporal", C.c_uint32), ("list_lines", C.c_uint32)]


class ResumePlan(C.Structure):
    """rb_resume_plan_info: what a resume call takes for one filter of the set"""
    _fields_ = [("lanes_per_block_log2", C.c_uint32), ("words_per_lane", C.c_uint32), ("column_slices", C.c_uint32),
                ("nontemporal", C.c_uint32), ("list_lines", C.c_uint32)]


class PrefixPlan(C.Structure):
    """rb_prefix_plan_info: what a prefix call takes for one filter"""
    _fields_ = [("lanes_per_block_log2", C.c_uint32), ("words_per_lane", C.c_uint32), ("column_slices", C.c_uint32),
                ("counter_planes", C.c_uint32), ("nontemporal", C.c_uint32), ("hash_functions", C.c_uint32), ("list_lines", C.c_uint32)]


class BinRef(C.Structure):
    """rb_bin_ref: one (source filter, bin) of an assemble plan -- 8 bytes"""
    _fields_ = [("filter", C.c_uint32), ("bin", C.c_uint32)]


# rb_bin_ref as a numpy record
BIN_REF_DTYPE = np.dtype([("filter", "<u4"), ("bin", "<u4")])
RB_ASSEMBLE_MAX_SOURCES = 8
RB_BIN_NONE = 2**64 - 1


class IbfCompare(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("file_bits", "rebuilt_bits", "new_bits", "payload_bits")]


class BinOccupancySummary(C.Structure):
    """rb_bin_occupancy_summary"""
    _fields_ = ([(n, C.c_uint64) for n in ("n_bins", "n_blocks", "n_hash", "bits_total", "empty_bins", "max_bits", "max_bin",
                                           "min_bits", "min_bin")] +
                [(n, C.c_double) for n in ("mean_load", "max_load", "mean_fpr", "max_fpr")] + [("bins_over_max_fp", C.c_uint64)])


class IbfInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in
                ("n_bins", "n_hash", "kmer_size", "n_bits", "bin_width", "n_blocks", "n_words")]


class RBError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        msg = lib().rb_last_error().decode(errors="replace")
        super().__init__("%s: status %d (%s) %s" % (where, status, lib().rb_status_string(status).decode(), msg))


# every exported symbol with (restype, argtypes); tests check the .so exports exactly these
_vp, _u64, _u32, _sz, _dbl, _int = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t, C.c_double, C.c_int
_pp = C.POINTER(C.c_void_p)
SIGNATURES = {
    "rb_status_string": (C.c_char_p, [_int]),
    "rb_last_error": (C.c_char_p, []),
    "rb_version": (C.c_char_p, []),
    "rb_device_count": (_int, []),
    "rb_ibf_open": (_int, [C.c_char_p, _pp]),
    "rb_ibf_create": (_int, [_u64, _u64, _u64, _u64, _pp]),
    "rb_ibf_store": (_int, [_vp, C.c_char_p]),
    "rb_ibf_get_info": (_int, [_vp, C.POINTER(IbfInfo)]),
    "rb_ibf_words": (_vp, [_vp]),
    "rb_ibf_close": (None, [_vp]),
    "rb_is_ibf_file": (_int, [C.c_char_p]),
    "rb_calculate_ci": (_int, [_dbl, C.c_uint8, _u32, _dbl, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16)]),
    "rb_threshold": (C.c_uint16, [_u64, _u64, _dbl, _dbl]),
    "rb_calculate_filter_size_bits": (_u64, [_u64, _u64, _u64, _dbl, _u64]),
    "rb_cut_out_nnns": (_sz, [C.c_char_p, _sz, C.c_char_p]),
    "rb_fragment_bounds": (_sz, [_u64, _u64, _u64, _u64, _vp, _vp, _sz]),
    "rb_dibf_create": (_int, [_int, _u64, _u64, _u64, _u64, _pp]),
    "rb_dibf_upload": (_int, [_int, _vp, _pp]),
    "rb_dibf_open": (_int, [_int, C.c_char_p, _pp]),
    "rb_dibf_download": (_int, [_vp, _pp]),
    "rb_dibf_get_info": (_int, [_vp, C.POINTER(IbfInfo)]),
    "rb_dibf_device_words": (_vp, [_vp]),
    "rb_dibf_touch": (_int, [_vp]),
    "rb_dibf_device_stride": (_u64, [_vp]),
    "rb_dibf_device": (_int, [_vp]),
    "rb_dibf_free": (None, [_vp]),
    "rb_dibf_resize_bins": (_int, [_vp, _u64, _pp]),
    "rb_dibf_assemble": (_int, [_pp, _sz, _vp, _vp, _u64, _pp]),
    "rb_dibf_select_bins": (_int, [_vp, _vp, _u64, _pp]),
    "rb_set_assemble_grid": (None, [_u32, _u32]),
    "rb_assemble_last_seconds": (_dbl, []),
    "rb_dibf_fill_synth": (_int, [_vp, _u64]),
    "rb_dibf_insert": (_int, [_vp, _vp, _sz, _vp, _vp, _vp, _sz]),
    "rb_dibf_add_sequence": (_int, [_vp, _vp, _sz, _u64, _u64, _u64, C.POINTER(_u64)]),
    "rb_engine_create": (_int, [_int, _pp, _sz, _pp, _sz, _pp]),
    "rb_engine_destroy": (None, [_vp]),
    "rb_classify_batch": (_int, [_vp, _vp, _vp, _vp, _sz, _dbl, _dbl, _int, _vp, _vp, _vp, _vp]),
    "rb_classify_batch_ptrs": (_int, [_vp, _vp, _vp, _sz, _dbl, _dbl, _int, _vp, _vp, _vp, _vp]),
    "rb_classify_batch_device_ex": (_int, [_vp, C.POINTER(BatchDesc), _dbl, _dbl, _int, _vp, _vp, _vp, _vp, _vp]),
    "rb_locate_batch_device": (_int, [_vp, C.POINTER(BatchDesc), _dbl, _dbl, C.POINTER(LocateOut), _vp]),
    "rb_locate_batch": (_int, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _dbl, _dbl, C.POINTER(LocateOut)]),
    "rb_prefix_batch_device": (_int, [_vp, C.POINTER(BatchDesc), _vp, C.c_uint32, _dbl, _dbl, _int, C.POINTER(PrefixOut), _vp]),
    "rb_prefix_batch": (_int, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, C.c_uint32, _dbl, _dbl, _int, C.POINTER(PrefixOut)]),
    "rb_resume_create": (_int, [_vp, _u32, _u32, _u32, _pp]),
    "rb_resume_destroy": (None, [_vp]),
    "rb_resume_bytes": (_u64, [_vp]),
    "rb_resume_batch_device": (_int, [_vp, C.POINTER(BatchDesc), _vp, _vp, _dbl, _dbl, _int, C.POINTER(ResumeOut), _vp]),
    "rb_resume_batch": (_int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _dbl, _dbl, _int, C.POINTER(ResumeOut)]),
    "rb_resume_counts": (_int, [_vp, _u32, _sz, _vp, _vp]),
    "rb_resume_set_lists": (_int, [_vp, _int]),
    "rb_resume_plan": (_int, [_vp, _sz, C.POINTER(ResumePlan)]),
    "rb_hits_batch_device": (_int, [_vp, C.POINTER(BatchDesc), _dbl, _dbl, C.c_uint16, C.c_uint32, C.POINTER(HitsOut), _vp]),
    "rb_hits_batch": (_int, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _dbl, _dbl, C.c_uint16, C.c_uint32, C.POINTER(HitsOut)]),
    "rb_spans_batch_device": (_int, [_vp, C.POINTER(BatchDesc), _sz, _vp, _sz, C.c_uint32, C.POINTER(SpansOut), _vp]),
    "rb_spans_batch": (_int, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _sz, _vp, _sz, C.c_uint32, C.POINTER(SpansOut)]),
    "rb_pack_reads": (_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "rb_host_alloc": (_int, [_sz, C.POINTER(_vp)]),
    "rb_host_free": (None, [_vp]),
    "rb_classify_batch_device": (_int, [_vp, _vp, _vp, _vp, _sz, _u32, _dbl, _dbl, _int, _vp, _vp, _vp, _vp, _vp]),
    "rb_engine_set_column_shard": (_int, [_vp, _int, _int]),
    "rb_decide_device": (_int, [_vp, _vp, _vp, _sz, _u32, _dbl, _dbl, _int, _vp, _vp, _vp, _vp]),
    "rb_decide_device_parts": (_int, [_vp, _vp, _u32, _u64, _vp, _sz, _u32, _dbl, _dbl, _int, _vp, _vp, _vp, _vp]),
    "rb_pool_create": (_int, [C.POINTER(_int), _sz, _pp, _sz, _pp, _sz, _pp]),
    "rb_pool_create_from_files": (_int, [C.POINTER(_int), _sz, C.POINTER(C.c_char_p), _sz, C.POINTER(C.c_char_p), _sz, _pp,
                                         C.POINTER(_dbl)]),
    "rb_pool_create_from_device": (_int, [C.POINTER(_int), _sz, _pp, _sz, _pp, _sz, _pp, C.POINTER(_dbl)]),
    "rb_pool_get_stats": (_int, [_vp, _sz, C.POINTER(_int), C.POINTER(_dbl), C.POINTER(_u64), C.POINTER(_u64), _int]),
    "rb_pool_destroy": (None, [_vp]),
    "rb_dibf_clone_to": (_int, [_vp, _int, _pp]),
    "rb_dibf_compare": (_int, [_vp, _vp, C.POINTER(IbfCompare)]),
    "rb_dibf_bin_occupancy": (_int, [_vp, _vp]),
    "rb_dibf_bin_occupancy_device": (_int, [_vp, _vp, _vp]),
    "rb_bin_occupancy_summarize": (_int, [_vp, _u64, _u64, _u64, _dbl, C.POINTER(BinOccupancySummary)]),
    "rb_bin_occupancy_derive": (_int, [_vp, _u64, _u64, _u64, _vp, _vp, _vp]),
    "rb_set_bin_occupancy_grid": (None, [_u32, _u32]),
    "rb_nt_threshold_default": (_u64, []),
    "rb_last_warning": (C.c_char_p, []),
    "rb_pool_size": (_sz, [_vp]),
    "rb_pool_set_min_split": (_int, [_vp, _sz]),
    "rb_pool_set_serialize": (_int, [_vp, _int]),
    "rb_pool_set_timing": (_int, [_vp, _int]),
    "rb_pool_kernel_time": (_int, [_vp, _sz, C.POINTER(_dbl), C.POINTER(_u64)]),
    "rb_pool_classify_batch": (_int, [_vp, _vp, _vp, _vp, _sz, _dbl, _dbl, _int, _vp, _vp, _vp, _vp]),
    "rb_live_create": (_int, [_vp, _dbl, _dbl, _u32, _pp]),
    "rb_live_destroy": (None, [_vp]),
    "rb_live_process": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "rb_live_pending": (_sz, [_vp]),
    "rb_live_forget": (_int, [_vp, C.c_char_p, _u32]),
    "rb_replay_arrivals": (_int, [_vp, _vp, _u32, _sz, _vp, _sz, _dbl, _dbl, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz),
                                  C.POINTER(_dbl)]),
    "rb_live_replay_arrivals": (_int, [_vp, _vp, _vp, _u32, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz),
                                       C.POINTER(_dbl)]),
    "rb_dibf_clone_to_ex": (_int, [_vp, _int, _pp, C.POINTER(_int), C.POINTER(_dbl)]),
    "rb_engine_set_revcomp_of_n": (_int, [_vp, _u32]),
    "rb_set_default_revcomp_of_n": (_int, [_u32]),
    "rb_set_placement_tries": (_int, [_int]),
    "rb_dibf_row_table_build": (_int, [_vp, _u64]),
    "rb_dibf_row_table_drop": (_int, [_vp]),
    "rb_dibf_row_table_info": (_int, [_vp, C.POINTER(RowTableInfo)]),
    "rb_dibf_row_table_download": (_int, [_vp, _vp, _u64]),
    "rb_engine_set_row_table": (_int, [_vp, _int, _u64]),
    "rb_engine_set_pass_lists": (_int, [_vp, _int]),
    "rb_engine_set_prefix_lists": (_int, [_vp, _int]),
    "rb_engine_plan_prefix": (_int, [_vp, _sz, _u32, _u32, C.POINTER(PrefixPlan)]),
    "rb_engine_prefix_lists_items": (_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _int]),
    "rb_dibf_list_table_build": (_int, [_vp, _u64]),
    "rb_dibf_list_table_drop": (_int, [_vp]),
    "rb_dibf_list_table_info": (_int, [_vp, C.POINTER(ListTableInfo)]),
    "rb_dibf_list_table_download": (_int, [_vp, _vp, _u64, _vp, _u64]),
    "rb_engine_set_list_min_dense_bytes": (_int, [_vp, _u64]),
    "rb_set_list_side_capacity": (None, [C.c_uint32]),
    "rb_dibf_pair_table_build": (_int, [_vp, _u64]),
    "rb_dibf_pair_table_drop": (_int, [_vp]),
    "rb_dibf_pair_table_info": (_int, [_vp, C.POINTER(PairTableInfo)]),
    "rb_dibf_pair_table_download": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _u64]),
    "rb_engine_set_pair_min_bytes": (_int, [_vp, _u64]),
    "rb_set_pair_side_capacity": (None, [C.c_uint32, C.c_uint32]),
    "rb_dibf_wide_list_table_build": (_int, [_vp, _u64]),
    "rb_dibf_wide_list_table_drop": (_int, [_vp]),
    "rb_dibf_wide_list_table_info": (_int, [_vp, C.POINTER(WideListTableInfo)]),
    "rb_dibf_wide_list_table_download": (_int, [_vp, _vp, _u64, _vp, _u64]),
    "rb_engine_set_wide_lists": (_int, [_vp, _int]),
    "rb_engine_set_wide_pass_lists": (_int, [_vp, _int]),
    "rb_engine_wide_pass_lines": (_int, [_vp, _sz, _u32, C.POINTER(C.c_uint32)]),
    "rb_engine_set_wide_prefix_lists": (_int, [_vp, _int]),
    "rb_engine_wide_prefix_lines": (_int, [_vp, _sz, _u32, _u32, C.POINTER(C.c_uint32)]),
    "rb_engine_wide_prefix_lists_items": (_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _int]),
    "rb_set_wide_list_side_capacity": (None, [C.c_uint32]),
    "rb_dibf_placement": (_int, [_vp, C.POINTER(_u32), C.POINTER(_dbl), C.POINTER(_dbl)]),
    "rb_dibf_placement_cost": (_int, [_vp, C.POINTER(_dbl), C.POINTER(_dbl), C.POINTER(_u64), C.POINTER(_u32)]),
    "rb_engine_set_merge": (_int, [_vp, _int]),
    "rb_engine_merge_info": (_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "rb_engine_set_split_threshold": (_int, [_vp, _u32]),
    "rb_engine_set_overlap": (_int, [_vp, _int]),
    "rb_engine_set_split_parts": (_int, [_vp, _u32, _u32]),
    "rb_engine_set_fold_decide": (_int, [_vp, _int]),
    "rb_engine_set_completion_word": (_int, [_vp, _int]),
    "rb_engine_set_nt_threshold": (_int, [_vp, _u64]),
    "rb_engine_set_host_slice_bytes": (_int, [_vp, _u64]),
    "rb_engine_set_serial_table_bytes": (_int, [_vp, _u64]),
    "rb_engine_set_phase_slices": (_int, [_vp, _u32, _u32]),
    "rb_engine_set_phase_equal_slices": (_int, [_vp, _u32]),
    "rb_engine_set_reads_per_wave": (_int, [_vp, _u32]),
    "rb_engine_set_phase_xcd_skew": (_int, [_vp, _u32]),
    "rb_engine_set_early_decision": (_int, [_vp, _int]),
    "rb_engine_set_bound_pruning": (_int, [_vp, _int]),
    "rb_engine_set_prune_parts": (_int, [_vp, C.c_uint32]),
    "rb_engine_set_prune_trace": (_int, [_vp, _vp]),
    "rb_engine_set_cert_load": (_int, [_vp, C.c_size_t, C.c_double]),
    "rb_engine_set_lead_min": (_int, [_vp, C.c_size_t, C.c_int]),
    "rb_engine_set_phased": (_int, [_vp, _u64, _u64, _u32, _u32, _u32]),
    "rb_engine_set_timing": (_int, [_vp, _int]),
    "rb_engine_kernel_time": (_int, [_vp, C.POINTER(_dbl), C.POINTER(_u64)]),
    "rb_engine_plan": (_int, [_vp, _sz, _sz, _u32, C.POINTER(PlanInfo)]),
    "rb_engine_plan_pass": (_int, [_vp, _sz, _u32, C.POINTER(PassPlan)]),
    "rb_engine_calibrate": (_int, [_vp, _sz, _u32, _dbl, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rb_dibf_probe_read_peak": (_int, [_vp, _u64, _u32, _int, _u32, _dbl, C.POINTER(_dbl), C.POINTER(_dbl)]),
}

_lib = None


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64.so (same SONAME as
    /opt/rocm's, different file).  If our library pulled in the system copy and torch loaded its own
    later, two runtimes would fight over the device; and loading torch's libraries after a runtime has
    already been initialised can make their code-object registration take minutes.  So when torch is
    installed it is imported BEFORE libreadbouncer_amd.so is loaded: its libraries register lazily and
    our library binds to the already loaded runtime by SONAME.  Without torch the system runtime is
    used.  torch stays plumbing: nothing else of it is touched here."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
    except Exception:
        pass


def lib():
    global _lib
    if _lib is None:
        # RB_AMD_LIBRARY: another build of the SAME library (tests load the -DRB_TESTING build in a child process); never a
        # different implementation -- the symbol table below is checked either way
        path = os.environ.get("RB_AMD_LIBRARY") or LIB_PATH
        if not os.path.exists(path):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no fallback implementation" % path)
        _preload_hip_runtime()
        L = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(st, where):
    if st != RB_OK:
        raise RBError(st, where)


def _ptr(a):
    """numpy array / int / None -> void* value"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data
    return int(a)


def _info(handle, fn):
    i = IbfInfo()
    _check(fn(handle, C.byref(i)), "get_info")
    return {k: getattr(i, k) for k, _ in IbfInfo._fields_}


class HostIBF:
    """rb_ibf: host image of a .ibf file (IBF::load_filter / TIbf ctor / seqan::store)."""

    def __init__(self, handle):
        self.h = handle
        self.info = _info(self.h, lib().rb_ibf_get_info)

    @classmethod
    def open(cls, path):
        h = C.c_void_p()
        _check(lib().rb_ibf_open(os.fsencode(path), C.byref(h)), "rb_ibf_open")
        return cls(h)

    @classmethod
    def create(cls, n_bins, n_hash, kmer_size, n_bits):
        h = C.c_void_p()
        _check(lib().rb_ibf_create(n_bins, n_hash, kmer_size, n_bits, C.byref(h)), "rb_ibf_create")
        return cls(h)

    def words(self):
        p = lib().rb_ibf_words(self.h)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(self.info["n_words"],))

    def store(self, path):
        _check(lib().rb_ibf_store(self.h, os.fsencode(path)), "rb_ibf_store")

    def close(self):
        if self.h:
            lib().rb_ibf_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceIBF:
    """rb_dibf: an IBF resident in HBM."""

    def __init__(self, handle):
        self.h = handle
        self.info = _info(self.h, lib().rb_dibf_get_info)

    @classmethod
    def create(cls, device, n_bins, n_hash, kmer_size, n_bits):
        h = C.c_void_p()
        _check(lib().rb_dibf_create(device, n_bins, n_hash, kmer_size, n_bits, C.byref(h)), "rb_dibf_create")
        return cls(h)

    @classmethod
    def upload(cls, device, host):
        h = C.c_void_p()
        _check(lib().rb_dibf_upload(device, host.h, C.byref(h)), "rb_dibf_upload")
        return cls(h)

    @classmethod
    def open(cls, device, path):
        h = C.c_void_p()
        _check(lib().rb_dibf_open(device, os.fsencode(path), C.byref(h)), "rb_dibf_open")
        return cls(h)

    def download(self):
        h = C.c_void_p()
        _check(lib().rb_dibf_download(self.h, C.byref(h)), "rb_dibf_download")
        return HostIBF(h)

    def clone_to(self, device):
        """device-to-device replica (xGMI between peers) in the HBM layout"""
        h = C.c_void_p()
        _check(lib().rb_dibf_clone_to(self.h, device, C.byref(h)), "rb_dibf_clone_to")
        return DeviceIBF(h)

    def clone_to_ex(self, device):
        """-> (replica, used_peer, seconds): how the copy travelled (peer mapping = xGMI between two GPUs) and how long"""
        h, peer, secs = C.c_void_p(), C.c_int(0), C.c_double(0)
        _check(lib().rb_dibf_clone_to_ex(self.h, device, C.byref(h), C.byref(peer), C.byref(secs)), "rb_dibf_clone_to_ex")
        return DeviceIBF(h), bool(peer.value), secs.value

    def compare(self, rebuilt):
        """bit statistics against a filter of the same geometry re-inserted from the reference sequences"""
        c = IbfCompare()
        _check(lib().rb_dibf_compare(self.h, rebuilt.h, C.byref(c)), "rb_dibf_compare")
        return {k: getattr(c, k) for k, _ in IbfCompare._fields_}

    def bin_occupancy(self):
        """-> np.uint64[n_bins]: blocks of the resident table whose bit for that bin is set (one streaming pass on the GPU)"""
        out = np.zeros(self.info["n_bins"], dtype=np.uint64)
        _check(lib().rb_dibf_bin_occupancy(self.h, _ptr(out)), "rb_dibf_bin_occupancy")
        return out

    def bin_occupancy_device(self, d_out, stream=None):
        """the same into device memory (u64 [n_bins]); asynchronous on `stream`, synchronised when stream is None"""
        _check(lib().rb_dibf_bin_occupancy_device(self.h, _ptr(d_out), _ptr(stream)), "rb_dibf_bin_occupancy_device")

    def device_words(self):
        return lib().rb_dibf_device_words(self.h)

    def device_stride(self):
        return lib().rb_dibf_device_stride(self.h)

    def probe_read_peak(self, row_bytes, nontemporal, loads_in_flight=12, table_bytes=0, target_ms=200.0):
        """measurement aid: GB/s of random whole-row gathers from this filter's table with no compute attached -> (GB/s, ms)"""
        g, ms = _dbl(0.0), _dbl(0.0)
        _check(lib().rb_dibf_probe_read_peak(self.h, table_bytes, row_bytes, int(bool(nontemporal)), loads_in_flight, target_ms,
                                             C.byref(g), C.byref(ms)), "rb_dibf_probe_read_peak")
        return g.value, ms.value

    def row_table_build(self, max_bytes=0):
        """build the row table (one row per N-free k-mer: the AND of its h blocks) unless a current one exists -> row_table_info()"""
        _check(lib().rb_dibf_row_table_build(self.h, int(max_bytes)), "rb_dibf_row_table_build")
        return self.row_table_info()

    def row_table_drop(self):
        _check(lib().rb_dibf_row_table_drop(self.h), "rb_dibf_row_table_drop")

    def row_table_info(self):
        """-> dict (rb_row_table_info): bytes and rows of the current table (0: none), want_bytes, build_ms, alloc_s, refused, builds"""
        i = RowTableInfo()
        _check(lib().rb_dibf_row_table_info(self.h, C.byref(i)), "rb_dibf_row_table_info")
        return {k: getattr(i, k) for k, _ in RowTableInfo._fields_}

    def row_table_download(self):
        """-> np.uint64[rows, stride words]: the current row table"""
        i = self.row_table_info()
        out = np.zeros(i["bytes"] // 8, dtype=np.uint64)
        _check(lib().rb_dibf_row_table_download(self.h, _ptr(out), len(out)), "rb_dibf_row_table_download")
        return out.reshape(i["rows"], -1) if i["rows"] else out

    def _list_table(self, prefix, op, max_bytes=0):
        """build / drop / info / download of rb_dibf_<prefix>_*: the list table ("list_table") and the wide one ("wide_list_table")"""
        def call(what, *args):
            _check(getattr(lib(), "rb_dibf_%s_%s" % (prefix, what))(self.h, *args), "rb_dibf_%s_%s" % (prefix, what))
        if op == "drop":
            return call("drop")
        if op == "build":
            call("build", int(max_bytes))
        i = (WideListTableInfo if prefix == "wide_list_table" else ListTableInfo)()
        call("info", C.byref(i))
        d = {k: getattr(i, k) for k, _ in _LIST_TABLE_INFO_FIELDS}
        d["census_over"] = list(i.census_over)
        if op != "download":
            return d
        slots = np.zeros(d["bytes"] // 2, dtype=np.uint16)
        side = np.zeros(d["side_rows"] * d["stride_words"], dtype=np.uint64)
        call("download", _ptr(slots) if len(slots) else None, len(slots), _ptr(side) if len(side) else None, len(side))
        return (slots.reshape(d["rows"], -1) if d["rows"] else slots), side.reshape(d["side_rows"], d["stride_words"])  # (a table none of whose rows overflow has no side rows)

    def list_table_build(self, max_bytes=0):
        """build the list table (per N-free k-mer the sorted bin numbers of its row, in slots of 1, 2 or 4 lines) unless a current one
        exists -> list_table_info()"""
        return self._list_table("list_table", "build", max_bytes)

    def list_table_drop(self):
        self._list_table("list_table", "drop")

    def list_table_info(self):
        """-> dict (rb_list_table_info)"""
        return self._list_table("list_table", "info")

    def list_table_download(self):
        """-> (np.uint16[rows, 64 x lines]: the slots, np.uint64[side rows in use, stride words]: the dense rows overflow slots name)"""
        return self._list_table("list_table", "download")

    def wide_list_table_build(self, max_bytes=0):
        """build the wide list table (filters of 8193 to 32 256 bins: per N-free k-mer the sorted bin numbers of its row, in slots of 4, 6
        or 8 lines) unless a current one exists -> wide_list_table_info()"""
        return self._list_table("wide_list_table", "build", max_bytes)

    def wide_list_table_drop(self):
        self._list_table("wide_list_table", "drop")

    def wide_list_table_info(self):
        """-> dict (rb_wide_list_table_info)"""
        return self._list_table("wide_list_table", "info")

    def wide_list_table_download(self):
        """-> (np.uint16[rows, 64 x lines]: the canonical slots, np.uint64[side rows in use, stride words]: the dense rows overflow slots name)"""
        return self._list_table("wide_list_table", "download")

    def pair_table_info(self):
        """-> dict (rb_pair_table_info)"""
        i = PairTableInfo()
        _check(lib().rb_dibf_pair_table_info(self.h, C.byref(i)), "rb_dibf_pair_table_info")
        d = {k: getattr(i, k) for k, _ in PairTableInfo._fields_}
        d["census_over"] = list(i.census_over)
        return d

    def pair_table_build(self, max_bytes=0):
        """build the pair table (per N-free k-mer x the bins of row(x) and of row(rc(x)) in one three-line slot) unless a current one
        exists -> pair_table_info()"""
        _check(lib().rb_dibf_pair_table_build(self.h, int(max_bytes)), "rb_dibf_pair_table_build")
        return self.pair_table_info()

    def pair_table_drop(self):
        _check(lib().rb_dibf_pair_table_drop(self.h), "rb_dibf_pair_table_drop")

    def pair_table_download(self):
        """-> (np.uint16[rows, 256]: the canonical slots, np.uint32[tail lines in use, 32]: the tail lines as the device holds them,
        np.uint64[side rows in use, stride words]: the dense rows, two per dense slot)"""
        d = self.pair_table_info()
        slots = np.zeros(d["rows"] * PAIR_CANON_ENTRIES, dtype=np.uint16)
        tails = np.zeros(d["tail_rows"] * PAIR_TAIL_DWORDS, dtype=np.uint32)
        side = np.zeros(d["side_rows"] * d["stride_words"], dtype=np.uint64)
        _check(lib().rb_dibf_pair_table_download(self.h, _ptr(slots) if len(slots) else None, len(slots), _ptr(tails) if len(tails) else None,
                                                 len(tails), _ptr(side) if len(side) else None, len(side)), "rb_dibf_pair_table_download")
        return (slots.reshape(d["rows"], PAIR_CANON_ENTRIES) if d["rows"] else slots), tails.reshape(-1, PAIR_TAIL_DWORDS), \
            side.reshape(d["side_rows"], d["stride_words"])

    def placement(self):
        """-> (allocations probed for this table: 0 = not placed by trial, GB/s of the kept one, GB/s of the slowest one)"""
        t, g, w = _u32(0), _dbl(0.0), _dbl(0.0)
        _check(lib().rb_dibf_placement(self.h, C.byref(t), C.byref(g), C.byref(w)), "rb_dibf_placement")
        return t.value, g.value, w.value

    def placement_cost(self):
        """-> dict: seconds of the trial, seconds waited after it, most HBM its candidates held, why a large table was not tried (0 / 1 / 2)"""
        ts, ss, pk, sk = _dbl(0.0), _dbl(0.0), _u64(0), _u32(0)
        _check(lib().rb_dibf_placement_cost(self.h, C.byref(ts), C.byref(ss), C.byref(pk), C.byref(sk)), "rb_dibf_placement_cost")
        return {"trial_s": ts.value, "settle_s": ss.value, "peak_bytes": pk.value, "skipped": sk.value}

    def resize_bins(self, new_bins):
        h = C.c_void_p()
        _check(lib().rb_dibf_resize_bins(self.h, new_bins, C.byref(h)), "rb_dibf_resize_bins")
        return DeviceIBF(h)

    @classmethod
    def assemble(cls, sources, plan):
        """a new filter whose bin j is the OR of the (filter, bin) pairs of plan[j], filter indexing `sources` (resident filters of one
        n_blocks, n_hash and kmer_size); plan: a list of lists of (filter, bin), or an (offsets, refs) pair (assemble_plan)"""
        offsets, refs = assemble_plan(plan)
        h = C.c_void_p()
        _check(lib().rb_dibf_assemble(_handle_array(sources), len(sources), _ptr(offsets), _ptr(refs), len(offsets) - 1, C.byref(h)),
               "rb_dibf_assemble")
        return cls(h)

    def select_bins(self, bins):
        """a new filter whose bin j is this filter's bin bins[j]; RB_BIN_NONE (or None) = an empty bin"""
        b = np.ascontiguousarray([RB_BIN_NONE if x is None else int(x) for x in bins], dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().rb_dibf_select_bins(self.h, _ptr(b), len(b), C.byref(h)), "rb_dibf_select_bins")
        return DeviceIBF(h)

    def fill_synth(self, seed):
        _check(lib().rb_dibf_fill_synth(self.h, seed), "rb_dibf_fill_synth")

    def insert(self, seq, starts, ends, bins):
        if isinstance(seq, str):
            seq = seq.encode()
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        ends = np.ascontiguousarray(ends, dtype=np.uint64)
        bins = np.ascontiguousarray(bins, dtype=np.uint64)
        buf = np.frombuffer(seq, dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq
        _check(lib().rb_dibf_insert(self.h, _ptr(np.ascontiguousarray(buf)), len(buf), _ptr(starts), _ptr(ends),
                                    _ptr(bins), len(starts)), "rb_dibf_insert")

    def add_sequence(self, seq, fragment_length, first_bin=0, overlap_length=1500):
        if isinstance(seq, str):
            seq = seq.encode()
        buf = np.ascontiguousarray(np.frombuffer(seq, dtype=np.uint8))
        nxt = C.c_uint64(0)
        _check(lib().rb_dibf_add_sequence(self.h, _ptr(buf), len(buf), fragment_length, overlap_length, first_bin,
                                          C.byref(nxt)), "rb_dibf_add_sequence")
        return nxt.value

    def free(self):
        if self.h:
            lib().rb_dibf_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _handle_array(filters):
    arr = (C.c_void_p * max(1, len(filters)))()
    for i, f in enumerate(filters):
        arr[i] = f.h
    return C.cast(arr, _pp)


class Engine:
    """rb_engine: per-GPU classifier over borrowed deplete/target filters."""

    def __init__(self, device, deplete, target):
        self._keep = (list(deplete), list(target))
        self.nd, self.nt = len(deplete), len(target)
        h = C.c_void_p()
        _check(lib().rb_engine_create(device, _handle_array(deplete), len(deplete), _handle_array(target), len(target),
                                      C.byref(h)), "rb_engine_create")
        self.h = h

    def classify(self, seqs, offsets, lens, error_rate=0.1, significance=0.95, mode=RB_MODE_CHECK_UNBLOCK):
        """host buffers in, host numpy arrays out: (maxcount[n, nf], best_target[n], decision[n], status[n])"""
        n = len(lens)
        nf = self.nd + self.nt
        maxcount = np.zeros((n, nf), dtype=np.uint16)
        best = np.full(n, -1, dtype=np.int32)
        decision = np.zeros(n, dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint8)
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        _check(lib().rb_classify_batch(self.h, _ptr(seqs), _ptr(offsets), _ptr(lens), n, error_rate, significance, mode,
                                       _ptr(maxcount), _ptr(best), _ptr(decision), _ptr(status)), "rb_classify_batch")
        return maxcount, best, decision, status

    def decide(self, seqs, offsets, lens, error_rate=0.1, significance=0.95, mode=RB_MODE_CHECK_UNBLOCK):
        """host buffers in, (decision[n], status[n]) out; the raw maxima and best_target are NOT asked for (NULL out pointers) -- the form
        of call the opt-in early-decision mode applies to (set_early_decision)"""
        n = len(lens)
        decision = np.zeros(n, dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint8)
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        _check(lib().rb_classify_batch(self.h, _ptr(seqs), _ptr(offsets), _ptr(lens), n, error_rate, significance, mode,
                                       None, None, _ptr(decision), _ptr(status)), "rb_classify_batch")
        return decision, status

    def classify_reads(self, reads, error_rate=0.1, significance=0.95, mode=RB_MODE_CHECK_UNBLOCK):
        """list of bytes objects (one buffer per read) through rb_classify_batch_ptrs"""
        n = len(reads)
        nf = self.nd + self.nt
        keep = [r.encode() if isinstance(r, str) else r for r in reads]
        ptrs = (C.c_char_p * max(1, n))(*keep)
        lens = np.array([len(r) for r in keep], dtype=np.uint32)
        maxcount = np.zeros((n, nf), dtype=np.uint16)
        best = np.full(n, -1, dtype=np.int32)
        decision = np.zeros(n, dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint8)
        _check(lib().rb_classify_batch_ptrs(self.h, C.cast(ptrs, C.c_void_p), _ptr(lens), n, error_rate, significance, mode,
                                            _ptr(maxcount), _ptr(best), _ptr(decision), _ptr(status)),
               "rb_classify_batch_ptrs")
        return maxcount, best, decision, status

    def classify_device(self, d_seqs, d_offsets, d_lens, n_reads, max_len, error_rate=0.1, significance=0.95,
                        mode=RB_MODE_CHECK_UNBLOCK, d_maxcount=None, d_best=None, d_decision=None, d_status=None,
                        stream=None):
        """raw device pointers (ints, e.g. torch.Tensor.data_ptr())"""
        _check(lib().rb_classify_batch_device(self.h, d_seqs, d_offsets, d_lens, n_reads, max_len, error_rate,
                                              significance, mode, d_maxcount, d_best, d_decision, d_status, stream),
               "rb_classify_batch_device")

    def classify_device_ex(self, d_seqs, d_offsets, d_lens, n_items, max_len, d_nmask=None, d_nmask_offsets=None,
                           chunk_start=0, chunk_length=0, d_read_ids=None, error_rate=0.1, significance=0.95,
                           mode=RB_MODE_CHECK_UNBLOCK, d_maxcount=None, d_best=None, d_decision=None, d_status=None,
                           stream=None):
        desc = BatchDesc(d_seqs, d_offsets, d_lens, n_items, max_len, d_nmask, d_nmask_offsets, chunk_start, chunk_length,
                         d_read_ids)
        _check(lib().rb_classify_batch_device_ex(self.h, C.byref(desc), error_rate, significance, mode, d_maxcount, d_best,
                                                 d_decision, d_status, stream), "rb_classify_batch_device_ex")

    def locate(self, seqs, offsets, lens, read_ids=None, error_rate=0.1, significance=0.95):
        """which bin and strand each selected read matched and how many bins hit (rb_locate_batch): host buffers in, a dict of host
        numpy arrays out -- max_count[n, nf] u16, best_bin[n, nf] i32, best_strand[n, nf] u8, hit_bins[n, nf] u32, status[n] u8, one
        row per work item (read_ids[j], or every read when read_ids is None)"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        ids = None if read_ids is None else np.ascontiguousarray(read_ids, dtype=np.uint32)
        n = len(lens) if ids is None else len(ids)
        nf = self.nd + self.nt
        res = {"max_count": np.zeros((n, nf), dtype=np.uint16), "best_bin": np.full((n, nf), -1, dtype=np.int32),
               "best_strand": np.zeros((n, nf), dtype=np.uint8), "hit_bins": np.zeros((n, nf), dtype=np.uint32),
               "status": np.zeros(n, dtype=np.uint8)}
        out = LocateOut(*[_ptr(res[k]) for k in ("max_count", "best_bin", "best_strand", "hit_bins", "status")])
        _check(lib().rb_locate_batch(self.h, _ptr(seqs), _ptr(offsets), _ptr(lens), len(lens), None if ids is None else _ptr(ids), n,
                                     error_rate, significance, C.byref(out)), "rb_locate_batch")
        return res

    def locate_device(self, d_seqs, d_offsets, d_lens, n_items, max_len, d_nmask=None, d_nmask_offsets=None, chunk_start=0,
                      chunk_length=0, d_read_ids=None, error_rate=0.1, significance=0.95, d_max_count=None, d_best_bin=None,
                      d_best_strand=None, d_hit_bins=None, d_status=None, stream=None):
        """raw device pointers like classify_device_ex (rb_locate_batch_device); any output may be None, not all"""
        desc = BatchDesc(d_seqs, d_offsets, d_lens, n_items, max_len, d_nmask, d_nmask_offsets, chunk_start, chunk_length,
                         d_read_ids)
        out = LocateOut(d_max_count, d_best_bin, d_best_strand, d_hit_bins, d_status)
        _check(lib().rb_locate_batch_device(self.h, C.byref(desc), error_rate, significance, C.byref(out), stream),
               "rb_locate_batch_device")

    def prefixes(self, seqs, offsets, lens, prefix_lens, read_ids=None, error_rate=0.1, significance=0.95, mode=RB_MODE_CHECK_UNBLOCK):
        """the maxima and the decision of each selected read at every prefix checkpoint, from one pass over its k-mers
        (rb_prefix_batch): host buffers in, a dict of host numpy arrays out -- max_count[n, P, nf] u16, decision[n, P] u8,
        best_target[n, P] i32, status[n, P] u8, prefix_len[n, P] u32, first_decided[n] u32, one row per (work item, checkpoint)"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        cps = np.ascontiguousarray(prefix_lens, dtype=np.uint32)
        ids = None if read_ids is None else np.ascontiguousarray(read_ids, dtype=np.uint32)
        n = len(lens) if ids is None else len(ids)
        nf, P = self.nd + self.nt, len(cps)
        res = {"max_count": np.zeros((n, P, nf), dtype=np.uint16), "decision": np.zeros((n, P), dtype=np.uint8),
               "best_target": np.full((n, P), -1, dtype=np.int32), "status": np.zeros((n, P), dtype=np.uint8),
               "prefix_len": np.zeros((n, P), dtype=np.uint32), "first_decided": np.full(n, P, dtype=np.uint32)}
        out = PrefixOut(*[_ptr(res[k]) for k in ("max_count", "decision", "best_target", "status", "prefix_len", "first_decided")])
        _check(lib().rb_prefix_batch(self.h, _ptr(seqs), _ptr(offsets), _ptr(lens), len(lens), None if ids is None else _ptr(ids), n,
                                     _ptr(cps), P, error_rate, significance, mode, C.byref(out)), "rb_prefix_batch")
        return res

    def prefixes_device(self, d_seqs, d_offsets, d_lens, n_items, max_len, prefix_lens, d_nmask=None, d_nmask_offsets=None, chunk_start=0,
                        chunk_length=0, d_read_ids=None, error_rate=0.1, significance=0.95, mode=RB_MODE_CHECK_UNBLOCK, d_max_count=None,
                        d_decision=None, d_best_target=None, d_status=None, d_prefix_len=None, d_first_decided=None, stream=None):
        """raw device pointers like locate_device (rb_prefix_batch_device; prefix_lens is a host sequence); any output may be None, not all"""
        cps = np.ascontiguousarray(prefix_lens, dtype=np.uint32)
        desc = BatchDesc(d_seqs, d_offsets, d_lens, n_items, max_len, d_nmask, d_nmask_offsets, chunk_start, chunk_length,
                         d_read_ids)
        out = PrefixOut(d_max_count, d_decision, d_best_target, d_status, d_prefix_len, d_first_decided)
        _check(lib().rb_prefix_batch_device(self.h, C.byref(desc), _ptr(cps), len(cps), error_rate, significance, mode, C.byref(out), stream),
               "rb_prefix_batch_device")

    def resume(self, n_slots, max_chunk_len, max_total_len):
        """a set of slots that keep a read's counts in HBM between chunks (rb_resume_create) -> Resume"""
        return Resume(self, n_slots, max_chunk_len, max_total_len)

    def hits(self, seqs, offsets, lens, read_ids=None, error_rate=0.1, significance=0.95, min_count=0, max_hits=64, bin_reads=None,
             hits=None):
        """every (bin, strand) of each selected read at or above the threshold, with its count (rb_hits_batch): host buffers in, a dict
        of host numpy arrays out -- hits[n, nf, max_hits] of HIT_DTYPE (only the first min(n_hits, max_hits) of a list are written:
        pass `hits` to keep what the rest held, else they are zero), n_hits[n, nf] u32 (exact, whatever max_hits), status[n] u8, and
        bin_reads when an u64 array with one entry per bin of every filter is passed: the call ADDS to it.  min_count 0 = the decision
        threshold; max_hits 0 = no records"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        ids = None if read_ids is None else np.ascontiguousarray(read_ids, dtype=np.uint32)
        n = len(lens) if ids is None else len(ids)
        nf = self.nd + self.nt
        res = {"n_hits": np.zeros((n, nf), dtype=np.uint32), "status": np.zeros(n, dtype=np.uint8)}
        if max_hits:
            if hits is None:
                hits = np.zeros((n, nf, max_hits), dtype=HIT_DTYPE)
            if hits.dtype != HIT_DTYPE or hits.shape != (n, nf, max_hits) or not hits.flags.c_contiguous:
                raise ValueError("hits must be a C-contiguous HIT_DTYPE array of shape (n_items, n_filters, max_hits)")
            res["hits"] = hits
        if bin_reads is not None:
            if bin_reads.dtype != np.uint64 or not bin_reads.flags.c_contiguous:
                raise ValueError("bin_reads must be a C-contiguous uint64 array")
            res["bin_reads"] = bin_reads
        out = HitsOut(_ptr(res["hits"]) if max_hits else None, _ptr(res["n_hits"]), _ptr(res["status"]),
                      None if bin_reads is None else _ptr(bin_reads))
        _check(lib().rb_hits_batch(self.h, _ptr(seqs), _ptr(offsets), _ptr(lens), len(lens), None if ids is None else _ptr(ids), n,
                                   error_rate, significance, min_count, max_hits, C.byref(out)), "rb_hits_batch")
        return res

    def hits_device(self, d_seqs, d_offsets, d_lens, n_items, max_len, d_nmask=None, d_nmask_offsets=None, chunk_start=0,
                    chunk_length=0, d_read_ids=None, error_rate=0.1, significance=0.95, min_count=0, max_hits=0, d_hits=None,
                    d_n_hits=None, d_status=None, d_bin_reads=None, stream=None):
        """raw device pointers like locate_device (rb_hits_batch_device); d_hits, d_n_hits and d_bin_reads may be None, not all three"""
        desc = BatchDesc(d_seqs, d_offsets, d_lens, n_items, max_len, d_nmask, d_nmask_offsets, chunk_start, chunk_length,
                         d_read_ids)
        out = HitsOut(d_hits, d_n_hits, d_status, d_bin_reads)
        _check(lib().rb_hits_batch_device(self.h, C.byref(desc), error_rate, significance, min_count, max_hits, C.byref(out), stream),
               "rb_hits_batch_device")

    def spans(self, seqs, offsets, lens, filter, queries, read_ids=None, mask_words=0, mask=None):
        """where along the read each queried bin matched (rb_spans_batch): host buffers in, a dict of host numpy arrays out --
        spans[n_queries, 2] of SPAN_DTYPE (strand 0, strand 1), n_kmers[n_queries] u32, status[n_queries] u8 and, with mask_words > 0,
        mask[n_queries, 2, mask_words] u64 (bit p & 63 of word p >> 6 = position p is a hit; every word is written: pass `mask` to
        see that over a fill of your own).  queries: SPAN_QUERY_DTYPE records or (item, bin) pairs against filter `filter` of the
        engine (deplete filters first); an item is read_ids[item], or read `item` when read_ids is None"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        ids = None if read_ids is None else np.ascontiguousarray(read_ids, dtype=np.uint32)
        n = len(lens) if ids is None else len(ids)
        q = np.asarray(queries)
        if q.dtype != SPAN_QUERY_DTYPE:
            pairs = np.asarray(queries, dtype=np.uint32).reshape(-1, 2)
            q = np.zeros(len(pairs), dtype=SPAN_QUERY_DTYPE)
            q["item"], q["bin"] = pairs[:, 0], pairs[:, 1]
        q = np.ascontiguousarray(q)
        nq = len(q)
        res = {"spans": np.zeros((nq, 2), dtype=SPAN_DTYPE), "n_kmers": np.zeros(nq, dtype=np.uint32), "status": np.zeros(nq, dtype=np.uint8)}
        if mask_words:
            if mask is None:
                mask = np.zeros((nq, 2, mask_words), dtype=np.uint64)
            if mask.dtype != np.uint64 or mask.shape != (nq, 2, mask_words) or not mask.flags.c_contiguous:
                raise ValueError("mask must be a C-contiguous uint64 array of shape (n_queries, 2, mask_words)")
            res["mask"] = mask
        out = SpansOut(_ptr(res["spans"]), _ptr(mask) if mask_words else None, _ptr(res["n_kmers"]), _ptr(res["status"]))
        _check(lib().rb_spans_batch(self.h, _ptr(seqs), _ptr(offsets), _ptr(lens), len(lens), None if ids is None else _ptr(ids), n,
                                    filter, _ptr(q), nq, mask_words, C.byref(out)), "rb_spans_batch")
        return res

    def spans_device(self, d_seqs, d_offsets, d_lens, n_items, max_len, filter, d_queries, n_queries, d_nmask=None, d_nmask_offsets=None,
                     chunk_start=0, chunk_length=0, d_read_ids=None, mask_words=0, d_spans=None, d_mask=None, d_n_kmers=None, d_status=None,
                     stream=None):
        """raw device pointers like hits_device (rb_spans_batch_device); any output may be None, not all"""
        desc = BatchDesc(d_seqs, d_offsets, d_lens, n_items, max_len, d_nmask, d_nmask_offsets, chunk_start, chunk_length,
                         d_read_ids)
        out = SpansOut(d_spans, d_mask, d_n_kmers, d_status)
        _check(lib().rb_spans_batch_device(self.h, C.byref(desc), filter, d_queries, n_queries, mask_words, C.byref(out), stream),
               "rb_spans_batch_device")

    def decide_device(self, d_maxcount, d_lens, n_reads, max_len, error_rate=0.1, significance=0.95,
                      mode=RB_MODE_CHECK_UNBLOCK, d_best=None, d_decision=None, d_status=None, stream=None):
        _check(lib().rb_decide_device(self.h, d_maxcount, d_lens, n_reads, max_len, error_rate, significance, mode,
                                      d_best, d_decision, d_status, stream), "rb_decide_device")

    def decide_device_parts(self, d_maxcount, n_parts, part_stride, d_lens, n_reads, max_len, error_rate=0.1,
                            significance=0.95, mode=RB_MODE_CHECK_UNBLOCK, d_best=None, d_decision=None, d_status=None,
                            stream=None):
        """decision over n_parts all-gathered partial maxcount tables (bin-sharded ranks), part_stride elements apart"""
        _check(lib().rb_decide_device_parts(self.h, d_maxcount, n_parts, part_stride, d_lens, n_reads, max_len, error_rate,
                                            significance, mode, d_best, d_decision, d_status, stream),
               "rb_decide_device_parts")

    def replay_arrivals(self, seqs, read_len, arrival_s, max_batch=16384, error_rate=0.1, significance=0.95):
        """work-conserving replay in C++ -> (decision[n], latency_s[n], call_reads[calls], call_service_s[calls], elapsed_s)"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        arrival_s = np.ascontiguousarray(arrival_s, dtype=np.float64)
        n = len(arrival_s)
        assert len(seqs) >= n * read_len
        dec = np.zeros(n, dtype=np.uint8)
        lat = np.zeros(n, dtype=np.float64)
        cr = np.zeros(n, dtype=np.uint32)
        cs = np.zeros(n, dtype=np.float64)
        calls, el = C.c_size_t(0), C.c_double(0)
        _check(lib().rb_replay_arrivals(self.h, _ptr(seqs), read_len, n, _ptr(arrival_s), max_batch, error_rate, significance,
                                        _ptr(dec), _ptr(lat), _ptr(cr), _ptr(cs), n, C.byref(calls), C.byref(el)),
               "rb_replay_arrivals")
        return dec, lat, cr[:calls.value], cs[:calls.value], el.value

    def set_column_shard(self, rank, world):
        _check(lib().rb_engine_set_column_shard(self.h, rank, world), "rb_engine_set_column_shard")

    def set_revcomp_of_n(self, ordinal):
        """3 (default): the reverse strand sees T where the read has N (ModComplementDna on a Dna5String); 4: N stays N"""
        _check(lib().rb_engine_set_revcomp_of_n(self.h, ordinal), "rb_engine_set_revcomp_of_n")

    def set_merge(self, mode):
        """filters of one hash geometry in one merged table: 0 never, 1 when it pays (default), 2 whenever two qualify"""
        _check(lib().rb_engine_set_merge(self.h, mode), "rb_engine_set_merge")

    def merge_info(self):
        """(merged tables, filters they serve, HBM bytes of the copies)"""
        t, f, b = C.c_uint32(), C.c_uint32(), C.c_uint64()
        _check(lib().rb_engine_merge_info(self.h, C.byref(t), C.byref(f), C.byref(b)), "rb_engine_merge_info")
        return t.value, f.value, b.value

    def plan(self, filter_index, n_reads, max_len):
        """what the engine would launch for that filter on such a batch -> dict (rb_plan_info)"""
        p = PlanInfo()
        _check(lib().rb_engine_plan(self.h, filter_index, n_reads, max_len, C.byref(p)), "rb_engine_plan")
        d = {k: getattr(p, k) for k, _ in PlanInfo._fields_}
        d["kernel"], d["phase_shape_name"] = p.kernel.decode(), p.phase_shape_name.decode()
        return d

    def plan_pass(self, filter_index, max_len):
        """the build locate, hits, prefixes and spans take for that filter on items of at most max_len bases -> dict (rb_pass_plan);
        list_lines: 0, or the slot size at which locate and hits take the filter's list table (set_pass_lists)"""
        p = PassPlan()
        _check(lib().rb_engine_plan_pass(self.h, filter_index, max_len, C.byref(p)), "rb_engine_plan_pass")
        return {k: getattr(p, k) for k, _ in PassPlan._fields_}

    def calibrate(self, n_reads=262144, read_len=250, max_ms=0.0):
        """fit the phased windows to this device -> (phased tables found, tables whose window changed)"""
        nt, nc = C.c_uint32(0), C.c_uint32(0)
        _check(lib().rb_engine_calibrate(self.h, n_reads, read_len, max_ms, C.byref(nt), C.byref(nc)), "rb_engine_calibrate")
        return nt.value, nc.value

    def set_split_threshold(self, max_reads):
        _check(lib().rb_engine_set_split_threshold(self.h, max_reads), "rb_engine_set_split_threshold")

    def set_overlap(self, on):
        _check(lib().rb_engine_set_overlap(self.h, int(on)), "rb_engine_set_overlap")

    def set_split_parts(self, max_parts, max_shares=4):
        _check(lib().rb_engine_set_split_parts(self.h, max_parts, max_shares), "rb_engine_set_split_parts")

    def set_fold_decide(self, on):
        _check(lib().rb_engine_set_fold_decide(self.h, int(on)), "rb_engine_set_fold_decide")

    def set_completion_word(self, on):
        _check(lib().rb_engine_set_completion_word(self.h, int(on)), "rb_engine_set_completion_word")

    def set_nt_threshold(self, table_bytes):
        _check(lib().rb_engine_set_nt_threshold(self.h, table_bytes), "rb_engine_set_nt_threshold")

    def set_serial_table_bytes(self, table_bytes):
        _check(lib().rb_engine_set_serial_table_bytes(self.h, table_bytes), "rb_engine_set_serial_table_bytes")

    def set_phased(self, min_table_bytes=5 << 18, max_table_bytes=128 << 20, base_ticks=0, ticks_per_mib=0, min_reads=2049):
        _check(lib().rb_engine_set_phased(self.h, min_table_bytes, max_table_bytes, base_ticks, ticks_per_mib, min_reads),
               "rb_engine_set_phased")

    def set_phase_slices(self, slice_log2=0, max_slices=32):
        """slices of 2^slice_log2 bytes (0: built-in rule; 1-5: as small as max_slices allows), at most max_slices"""
        _check(lib().rb_engine_set_phase_slices(self.h, slice_log2, max_slices), "rb_engine_set_phase_slices")

    def set_phase_equal_slices(self, n_slices=0):
        """n equal-length slices for the phased form (0 = the built-in rule); ignored while set_phase_slices names a slice size"""
        _check(lib().rb_engine_set_phase_equal_slices(self.h, n_slices), "rb_engine_set_phase_equal_slices")

    def set_reads_per_wave(self, reads):
        """two-word phased tables, reads of up to 256 k-mers: reads a wave carries through a pass of the windows (0: the one-read build)"""
        _check(lib().rb_engine_set_reads_per_wave(self.h, reads), "rb_engine_set_reads_per_wave")

    def set_early_decision(self, on):
        """opt-in: check_unblock calls without raw maxima stop counting a read once a bin has reached the larger of its two thresholds"""
        _check(lib().rb_engine_set_early_decision(self.h, int(on)), "rb_engine_set_early_decision")

    def set_bound_pruning(self, on):
        """plain count kernel: skip the gathers of bins that can no longer reach the read's maximum (default on; results identical)"""
        _check(lib().rb_engine_set_bound_pruning(self.h, int(on)), "rb_engine_set_bound_pruning")

    def set_prune_parts(self, mask):
        """refinements of bound pruning: bit 0 checks after every eight k-mers, bit 1 the stronger strand first, bit 2 the other strand
        certified from the first hash alone, bit 3 the line of the leading strand's best bin counted first and its other bins certified
        likewise (default 15; results identical)"""
        _check(lib().rb_engine_set_prune_parts(self.h, int(mask)), "rb_engine_set_prune_parts")

    def set_lead_min(self, filter_index, min_count):
        """count of the leading strand's first 64 k-mers from which bit 3 of set_prune_parts is attempted: < 0 derive from the filter's
        load (default), 0 always attempt"""
        _check(lib().rb_engine_set_lead_min(self.h, filter_index, int(min_count)), "rb_engine_set_lead_min")

    def set_cert_load(self, filter_index, load):
        """bit load (of the fullest bin) the certificate's attempt rule assumes for a filter: < 0 measure (default), 0 always attempt, >= 1 never"""
        _check(lib().rb_engine_set_cert_load(self.h, filter_index, float(load)), "rb_engine_set_cert_load")

    def set_row_table(self, mode, max_bytes=0):
        """RB_ROW_TABLE_OFF / _AUTO (default) / _FORCE / _LISTS (the list table wherever it serves): whether plain whole-wave launches gather one precomputed row per k-mer from the
        filter's row table, building it when there is none (results identical); max_bytes 0 keeps the limit (default 96 GiB)"""
        _check(lib().rb_engine_set_row_table(self.h, int(mode), int(max_bytes)), "rb_engine_set_row_table")

    def set_pass_lists(self, mode):
        """RB_PASS_LISTS_OFF (default) / _CURRENT (a filter's list table where it has a current one) / _BUILD (built when there is none):
        whether locate and hits are served from the list table (results identical; plan_pass reports list_lines)"""
        _check(lib().rb_engine_set_pass_lists(self.h, int(mode)), "rb_engine_set_pass_lists")

    def set_wide_lists(self, mode):
        """RB_PASS_LISTS_OFF (default) / _CURRENT / _BUILD: whether classify calls count a filter of 8193 to 32 256 bins from its wide
        list table (rb_engine_set_wide_lists; results identical; plan() names ibf_count_wide_lists_kernel)"""
        _check(lib().rb_engine_set_wide_lists(self.h, int(mode)), "rb_engine_set_wide_lists")

    def set_wide_pass_lists(self, mode):
        """RB_PASS_LISTS_OFF (default) / _CURRENT / _BUILD for locate and hits on filters of 8193 to 32 256 bins
        (rb_engine_set_wide_pass_lists): whether they are served from the filter's wide list table (results identical; a setting of its
        own beside set_wide_lists and set_pass_lists; wide_pass_lines reports the slot size)"""
        _check(lib().rb_engine_set_wide_pass_lists(self.h, int(mode)), "rb_engine_set_wide_pass_lists")

    def wide_pass_lines(self, filter_index, max_len):
        """0, or the slot size (4, 6 or 8 lines) at which a locate or hits call on items of at most max_len bases would take the filter's
        wide list table as things stand (rb_engine_wide_pass_lines: host arithmetic, nothing is built)"""
        lines = C.c_uint32(0)
        _check(lib().rb_engine_wide_pass_lines(self.h, filter_index, max_len, C.byref(lines)), "rb_engine_wide_pass_lines")
        return int(lines.value)

    def set_wide_prefix_lists(self, mode):
        """RB_PASS_LISTS_OFF (default) / _CURRENT / _BUILD for the prefix pass on filters of 8193 to 32 256 bins
        (rb_engine_set_wide_prefix_lists): whether prefixes are served from the filter's wide list table (results identical; a setting
        of its own beside set_prefix_lists, set_wide_pass_lists and set_wide_lists; wide_prefix_lines reports the slot size)"""
        _check(lib().rb_engine_set_wide_prefix_lists(self.h, int(mode)), "rb_engine_set_wide_prefix_lists")

    def wide_prefix_lines(self, filter_index, max_len, last_checkpoint):
        """0, or the slot size (4, 6 or 8 lines) at which a prefix call on items of at most max_len bases with that last checkpoint would
        take the filter's wide list table as things stand (rb_engine_wide_prefix_lines: host arithmetic, nothing is built)"""
        lines = C.c_uint32(0)
        _check(lib().rb_engine_wide_prefix_lines(self.h, filter_index, int(max_len), int(last_checkpoint), C.byref(lines)),
               "rb_engine_wide_prefix_lines")
        return int(lines.value)

    def wide_prefix_lists_items(self, reset=False):
        """-> (items the wide list form of the prefix pass took, items it left to the plain form) since the last reset, over the calls
        in which some filter was wide-served (rb_engine_wide_prefix_lists_items; the list form's pair is prefix_lists_items)"""
        listed, plain = C.c_uint64(0), C.c_uint64(0)
        _check(lib().rb_engine_wide_prefix_lists_items(self.h, C.byref(listed), C.byref(plain), int(bool(reset))),
               "rb_engine_wide_prefix_lists_items")
        return int(listed.value), int(plain.value)

    def set_prefix_lists(self, mode):
        """RB_PASS_LISTS_OFF (default) / _CURRENT / _BUILD for the prefix pass alone (rb_engine_set_prefix_lists): whether prefixes are
        served from a filter's list table (results identical; plan_prefix reports list_lines)"""
        _check(lib().rb_engine_set_prefix_lists(self.h, int(mode)), "rb_engine_set_prefix_lists")

    def plan_prefix(self, filter_index, max_len, last_checkpoint):
        """what a prefix call takes for that filter on items of at most max_len bases with that last checkpoint -> dict
        (rb_prefix_plan_info); list_lines: 0 = the plain form alone, else the list form's slot size"""
        p = PrefixPlan()
        _check(lib().rb_engine_plan_prefix(self.h, filter_index, int(max_len), int(last_checkpoint), C.byref(p)), "rb_engine_plan_prefix")
        return {name: int(getattr(p, name)) for name, _ in PrefixPlan._fields_}

    def prefix_lists_items(self, reset=False):
        """-> (items the list form of the prefix pass took, items it left to the plain form) since the last reset, over the calls in
        which some filter was list-served (rb_engine_prefix_lists_items)"""
        listed, plain = C.c_uint64(0), C.c_uint64(0)
        _check(lib().rb_engine_prefix_lists_items(self.h, C.byref(listed), C.byref(plain), int(bool(reset))), "rb_engine_prefix_lists_items")
        return int(listed.value), int(plain.value)

    def set_list_min_dense_bytes(self, n_bytes):
        """size of the dense row table from which RB_ROW_TABLE_AUTO prefers the list table (default 512 MiB; 0: always)"""
        _check(lib().rb_engine_set_list_min_dense_bytes(self.h, int(n_bytes)), "rb_engine_set_list_min_dense_bytes")

    def set_pair_min_bytes(self, n_bytes):
        """size of the pair table from which RB_ROW_TABLE_AUTO takes it instead of the list table (default 1 GiB; 0: always)"""
        _check(lib().rb_engine_set_pair_min_bytes(self.h, int(n_bytes)), "rb_engine_set_pair_min_bytes")

    def set_prune_trace(self, device_ptr):
        """device memory for one 8-byte record per (filter, read, column slice) of the plain count kernel's waves, or 0 / None: none"""
        _check(lib().rb_engine_set_prune_trace(self.h, C.c_void_p(device_ptr or None)), "rb_engine_set_prune_trace")

    def set_phase_xcd_skew(self, mode):
        """bit 0: every XCD on a different slice at any time; bit 1: the XCDs' windows start an eighth of a window apart"""
        _check(lib().rb_engine_set_phase_xcd_skew(self.h, mode), "rb_engine_set_phase_xcd_skew")

    def set_host_slice_bytes(self, slice_bytes):
        _check(lib().rb_engine_set_host_slice_bytes(self.h, slice_bytes), "rb_engine_set_host_slice_bytes")

    def set_timing(self, on):
        _check(lib().rb_engine_set_timing(self.h, int(on)), "rb_engine_set_timing")

    def kernel_time(self):
        """(total_ms, n_calls) of the count kernels since the last query; waits for them"""
        ms, n = C.c_double(0), C.c_uint64(0)
        _check(lib().rb_engine_kernel_time(self.h, C.byref(ms), C.byref(n)), "rb_engine_kernel_time")
        return ms.value, n.value

    def destroy(self):
        if self.h:
            lib().rb_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Resume:
    """rb_resume: slots in HBM that each hold one read's per-bin counts, both strands, for every filter of an engine, plus its last
    k - 1 bases and its length; a feed counts only the k-mers of the new chunks.  Destroyed before its engine."""

    def __init__(self, engine, n_slots, max_chunk_len, max_total_len):
        self.h = None
        self.engine = engine  # (keeps the engine alive as long as the slots)
        h = C.c_void_p()
        _check(lib().rb_resume_create(engine.h, n_slots, max_chunk_len, max_total_len, C.byref(h)), "rb_resume_create")
        self.h = h
        self.n_slots, self.max_chunk_len, self.max_total_len = n_slots, max_chunk_len, max_total_len

    @property
    def bytes(self):
        return int(lib().rb_resume_bytes(self.h))

    def set_lists(self, mode):
        """RB_PASS_LISTS_OFF (default) / _CURRENT / _BUILD for THIS slot set (rb_resume_set_lists): whether a feed's N-free items are
        counted from a filter's list table and merged into the slot; results and the slots' contents do not depend on it"""
        _check(lib().rb_resume_set_lists(self.h, int(mode)), "rb_resume_set_lists")

    def plan(self, filter_index):
        """what a feed takes for that filter as things stand -> dict (rb_resume_plan_info); list_lines: 0 = the plain form alone, else the
        slot size at which the list form serves the items it takes"""
        p = ResumePlan()
        _check(lib().rb_resume_plan(self.h, filter_index, C.byref(p)), "rb_resume_plan")
        return {name: int(getattr(p, name)) for name, _ in ResumePlan._fields_}

    def feed(self, seqs, offsets, lens, slots, flags=None, error_rate=0.1, significance=0.95, mode=RB_MODE_CHECK_UNBLOCK):
        """read i is the new chunk of slot slots[i] (rb_resume_batch): host buffers in, a dict of host numpy arrays out --
        max_count[n, nf] u16, decision[n] u8, best_target[n] i32, status[n] u8, total_len[n] u32"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        n, nf = len(lens), self.engine.nd + self.engine.nt
        assert len(slots) == n and (fl is None or len(fl) == n)
        if len(seqs) == 0:
            seqs = np.zeros(1, dtype=np.uint8)  # (a batch of empty chunks still names a buffer)
        res = {"max_count": np.zeros((n, nf), dtype=np.uint16), "decision": np.zeros(n, dtype=np.uint8),
               "best_target": np.full(n, -1, dtype=np.int32), "status": np.zeros(n, dtype=np.uint8),
               "total_len": np.zeros(n, dtype=np.uint32)}
        out = ResumeOut(*[_ptr(res[k]) for k in ("max_count", "decision", "best_target", "status", "total_len")])
        _check(lib().rb_resume_batch(self.h, _ptr(seqs), _ptr(offsets), _ptr(lens), n, _ptr(slots), None if fl is None else _ptr(fl),
                                     error_rate, significance, mode, C.byref(out)), "rb_resume_batch")
        return res

    def feed_device(self, d_seqs, d_offsets, d_lens, n_items, d_slots, d_flags=None, d_nmask=None, d_nmask_offsets=None, chunk_start=0,
                    chunk_length=0, d_read_ids=None, error_rate=0.1, significance=0.95, mode=RB_MODE_CHECK_UNBLOCK, d_max_count=None,
                    d_decision=None, d_best_target=None, d_status=None, d_total_len=None, stream=None):
        """raw device pointers like locate_device (rb_resume_batch_device); any output may be None, not all"""
        desc = BatchDesc(d_seqs, d_offsets, d_lens, n_items, 0, d_nmask, d_nmask_offsets, chunk_start, chunk_length, d_read_ids)
        out = ResumeOut(d_max_count, d_decision, d_best_target, d_status, d_total_len)
        _check(lib().rb_resume_batch_device(self.h, C.byref(desc), d_slots, d_flags, error_rate, significance, mode, C.byref(out), stream),
               "rb_resume_batch_device")

    def counts(self, slot, filter):
        """(counts u16 [2, n_bins]: forward and reverse complement, total_len) of one slot and filter (rb_resume_counts)"""
        filters = self.engine._keep[0] + self.engine._keep[1]
        n_bins = filters[filter].info["n_bins"] if 0 <= filter < len(filters) else 1  # (a filter the set does not have: the call says so)
        counts = np.zeros((2, n_bins), dtype=np.uint16)
        total = C.c_uint32(0)
        _check(lib().rb_resume_counts(self.h, slot, filter, _ptr(counts), C.addressof(total)), "rb_resume_counts")
        return counts, int(total.value)

    def destroy(self):
        if self.h:
            lib().rb_resume_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Pool:
    """rb_pool: one engine per device entry, filters replicated from host images, read-sharded batches."""

    def __init__(self, devices, deplete_images, target_images):
        self.nd, self.nt = len(deplete_images), len(target_images)
        self._keep = (list(deplete_images), list(target_images))
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _check(lib().rb_pool_create(devs, len(devices), _handle_array(deplete_images), self.nd,
                                    _handle_array(target_images), self.nt, C.byref(h)), "rb_pool_create")
        self.h = h

    @classmethod
    def from_files(cls, devices, deplete_paths, target_paths):
        """filters streamed once into devices[0] and replicated device to device; no host images"""
        self = cls.__new__(cls)
        self.nd, self.nt = len(deplete_paths), len(target_paths)
        self._keep = ()
        devs = (C.c_int * len(devices))(*devices)
        dp = (C.c_char_p * max(1, self.nd))(*[os.fsencode(x) for x in deplete_paths])
        tp = (C.c_char_p * max(1, self.nt))(*[os.fsencode(x) for x in target_paths])
        h = C.c_void_p()
        secs = C.c_double(0)
        _check(lib().rb_pool_create_from_files(devs, len(devices), dp, self.nd, tp, self.nt, C.byref(h), C.byref(secs)),
               "rb_pool_create_from_files")
        self.h = h
        self.replication_seconds = secs.value
        return self

    @classmethod
    def from_device(cls, devices, deplete, target):
        """replicas of filters that are already resident (DeviceIBF), copied device to device onto every entry of `devices`"""
        self = cls.__new__(cls)
        self.nd, self.nt = len(deplete), len(target)
        self._keep = (list(deplete), list(target))
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        secs = C.c_double(0)
        _check(lib().rb_pool_create_from_device(devs, len(devices), _handle_array(deplete), self.nd, _handle_array(target), self.nt,
                                                C.byref(h), C.byref(secs)), "rb_pool_create_from_device")
        self.h = h
        self.replication_seconds = secs.value
        return self

    def stats(self, reset=False):
        """per worker: (device, busy seconds inside its engine, reads served, parts of calls served)"""
        n = self.size()
        dev, busy, reads, calls = (C.c_int * n)(), (C.c_double * n)(), (C.c_uint64 * n)(), (C.c_uint64 * n)()
        _check(lib().rb_pool_get_stats(self.h, n, dev, busy, reads, calls, int(reset)), "rb_pool_get_stats")
        return [(dev[i], busy[i], reads[i], calls[i]) for i in range(n)]

    def set_timing(self, on):
        _check(lib().rb_pool_set_timing(self.h, int(on)), "rb_pool_set_timing")

    def kernel_time(self):
        """per worker: (summed K1 milliseconds since the last collection, bracketed launches) -- rb_engine_kernel_time of each engine"""
        n = self.size()
        ms, calls = (C.c_double * n)(), (C.c_uint64 * n)()
        _check(lib().rb_pool_kernel_time(self.h, n, ms, calls), "rb_pool_kernel_time")
        return [(ms[i], calls[i]) for i in range(n)]

    def classify_into(self, seqs_ptr, offsets_ptr, lens_ptr, n, maxcount_ptr, best_ptr, decision_ptr, status_ptr, error_rate=0.1,
                      significance=0.95, mode=RB_MODE_CHECK_UNBLOCK):
        """the C call on caller-owned buffers (e.g. page-locked ones from host_alloc), no numpy copies around it"""
        _check(lib().rb_pool_classify_batch(self.h, seqs_ptr, offsets_ptr, lens_ptr, n, error_rate, significance, mode, maxcount_ptr,
                                            best_ptr, decision_ptr, status_ptr), "rb_pool_classify_batch")

    def size(self):
        return lib().rb_pool_size(self.h)

    def set_min_split(self, reads_per_device):
        _check(lib().rb_pool_set_min_split(self.h, reads_per_device), "rb_pool_set_min_split")

    def set_serialize(self, on):
        _check(lib().rb_pool_set_serialize(self.h, int(on)), "rb_pool_set_serialize")

    def classify(self, seqs, offsets, lens, error_rate=0.1, significance=0.95, mode=RB_MODE_CHECK_UNBLOCK):
        n = len(lens)
        nf = self.nd + self.nt
        maxcount = np.zeros((n, nf), dtype=np.uint16)
        best = np.full(n, -1, dtype=np.int32)
        decision = np.zeros(n, dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint8)
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        _check(lib().rb_pool_classify_batch(self.h, _ptr(seqs), _ptr(offsets), _ptr(lens), n, error_rate, significance,
                                            mode, _ptr(maxcount), _ptr(best), _ptr(decision), _ptr(status)),
               "rb_pool_classify_batch")
        return maxcount, best, decision, status

    def destroy(self):
        if self.h:
            lib().rb_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Live:
    """rb_live: micro-batch form of classify_live_reads (once_seen bookkeeping + actions)."""

    def __init__(self, engine, error_rate=0.1, significance=0.95, max_undecided_len=1500):
        self._engine = engine
        h = C.c_void_p()
        _check(lib().rb_live_create(engine.h, error_rate, significance, max_undecided_len, C.byref(h)), "rb_live_create")
        self.h = h

    def process(self, ids, seqs):
        """ids, seqs: lists of bytes/str -> (action[n] uint8, status[n] uint8, classified_len[n] uint32)"""
        n = len(ids)
        ids = [i.encode() if isinstance(i, str) else i for i in ids]
        seqs = [s.encode() if isinstance(s, str) else s for s in seqs]

        def pack(items):
            lens = np.array([len(x) for x in items], dtype=np.uint32)
            offs = np.zeros(n, dtype=np.uint64)
            if n:
                offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
            buf = np.frombuffer(b"".join(items) or b"N", dtype=np.uint8).copy()
            return buf, offs, lens
        ib, io, il = pack(ids)
        sb, so, sl = pack(seqs)
        action = np.zeros(n, dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint8)
        clen = np.zeros(n, dtype=np.uint32)
        _check(lib().rb_live_process(self.h, _ptr(ib), _ptr(io), _ptr(il), _ptr(sb), _ptr(so), _ptr(sl), n, _ptr(action),
                                     _ptr(status), _ptr(clen)), "rb_live_process")
        return action, status, clen

    def replay_arrivals(self, read_ids, seqs, read_len, arrival_s, max_batch=16384):
        """work-conserving replay through the live step -> (action[n], latency_s[n], classified_len[n], call_reads, call_service_s,
        elapsed_s)"""
        read_ids = np.ascontiguousarray(read_ids, dtype=np.uint32)
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        arrival_s = np.ascontiguousarray(arrival_s, dtype=np.float64)
        n = len(arrival_s)
        assert len(seqs) >= n * read_len and len(read_ids) == n
        act = np.zeros(n, dtype=np.uint8)
        lat = np.zeros(n, dtype=np.float64)
        clen = np.zeros(n, dtype=np.uint32)
        cr = np.zeros(n, dtype=np.uint32)
        cs = np.zeros(n, dtype=np.float64)
        calls, el = C.c_size_t(0), C.c_double(0)
        _check(lib().rb_live_replay_arrivals(self.h, _ptr(read_ids), _ptr(seqs), read_len, n, _ptr(arrival_s), max_batch,
                                             _ptr(act), _ptr(lat), _ptr(clen), _ptr(cr), _ptr(cs), n, C.byref(calls),
                                             C.byref(el)), "rb_live_replay_arrivals")
        return act, lat, clen, cr[:calls.value], cs[:calls.value], el.value

    def pending(self):
        return lib().rb_live_pending(self.h)

    def forget(self, read_id):
        if isinstance(read_id, str):
            read_id = read_id.encode()
        _check(lib().rb_live_forget(self.h, read_id, len(read_id)), "rb_live_forget")

    def destroy(self):
        if self.h:
            lib().rb_live_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class HostBlock:
    """page-locked host memory from rb_host_alloc, seen as a numpy array of `dtype`"""

    def __init__(self, count, dtype=np.uint8):
        self.ptr = C.c_void_p()
        nbytes = int(count) * np.dtype(dtype).itemsize
        _check(lib().rb_host_alloc(max(1, nbytes), C.byref(self.ptr)), "rb_host_alloc")
        buf = (C.c_uint8 * max(1, nbytes)).from_address(self.ptr.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(count))

    def free(self):
        if self.ptr:
            self.array = None
            lib().rb_host_free(self.ptr)
            self.ptr = None


def set_bin_occupancy_grid(max_workgroups_per_slice=0, min_chunk_rows=0):
    """process-wide: how the per-bin occupancy pass cuts a table (0 / 0 = the built-in rule); counts never depend on it"""
    lib().rb_set_bin_occupancy_grid(int(max_workgroups_per_slice), int(min_chunk_rows))


def set_assemble_grid(max_workgroups=0, blocks_per_chunk=0):
    """rb_set_assemble_grid: how every later assemble of this process cuts a table (0, 0 = the built-in rule)"""
    lib().rb_set_assemble_grid(int(max_workgroups), int(blocks_per_chunk))


def assemble_last_seconds():
    """seconds the kernel of this thread's last assemble / select_bins ran"""
    return float(lib().rb_assemble_last_seconds())


def assemble_plan(plan):
    """an assemble plan in either form -> (offsets np.uint64[n_out_bins + 1], refs BIN_REF_DTYPE[n_refs]), the CSR arrays of
    rb_dibf_assemble.  `plan` is a list with one list of (filter, bin) pairs per out bin, or an (offsets, refs) pair of arrays,
    refs as BIN_REF_DTYPE records or an [n, 2] integer array.  Pure Python: no library call, no GPU."""
    if isinstance(plan, tuple) and len(plan) == 2 and isinstance(plan[0], np.ndarray):
        offsets = np.ascontiguousarray(plan[0], dtype=np.uint64)
        r = np.asarray(plan[1])
        if r.dtype != BIN_REF_DTYPE:
            r = np.asarray(r, dtype=np.int64).reshape(-1, 2)
            if r.size and (r.min() < 0 or r.max() >= 2**32):
                raise ValueError("assemble plan: a ref does not fit 32 bits")
            rec = np.zeros(len(r), dtype=BIN_REF_DTYPE)
            rec["filter"], rec["bin"] = r[:, 0], r[:, 1]
            r = rec
        refs = np.ascontiguousarray(r)
        if offsets.ndim != 1 or len(offsets) < 1:
            raise ValueError("assemble plan: offsets needs n_out_bins + 1 entries")
        if int(offsets[-1]) != len(refs):
            raise ValueError("assemble plan: offsets end at %d, there are %d refs" % (int(offsets[-1]), len(refs)))
        return offsets, refs
    lists = [list(l) for l in plan]
    offsets = np.zeros(len(lists) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64)
    refs = np.zeros(int(offsets[-1]), dtype=BIN_REF_DTYPE)
    i = 0
    for l in lists:
        for f, b in l:
            if not (0 <= int(f) < 2**32 and 0 <= int(b) < 2**32):
                raise ValueError("assemble plan: ref (%r, %r) does not fit 32 bits" % (f, b))
            refs[i] = (int(f), int(b))
            i += 1
    return offsets, refs


def nt_threshold_default():
    """table bytes beyond which the library reads with non-temporal loads"""
    return int(lib().rb_nt_threshold_default())


def set_placement_tries(tries):
    """process-wide: candidates a table of >= 1 GiB is allocated and probed as (default 5; 0 / 1 = off)"""
    _check(lib().rb_set_placement_tries(int(tries)), "rb_set_placement_tries")


def set_list_side_capacity(rows):
    """process-wide: rows of the side table of list tables built from now on (0: the default, 4^k / 512 + 64)"""
    lib().rb_set_list_side_capacity(int(rows))


def pack_reads(seqs, offsets, lens):
    """ASCII batch -> (packed uint8, packed_offsets uint64, nmask uint8, nmask_offsets uint64)"""
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n = len(lens)
    po_, no_ = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    pb, nb = C.c_uint64(0), C.c_uint64(0)
    _check(lib().rb_pack_reads(_ptr(seqs), _ptr(offsets), _ptr(lens), n, None, _ptr(po_), None, _ptr(no_), C.byref(pb),
                               C.byref(nb)), "rb_pack_reads")
    packed = np.zeros(max(1, pb.value), dtype=np.uint8)
    nmask = np.zeros(max(1, nb.value), dtype=np.uint8)
    _check(lib().rb_pack_reads(_ptr(seqs), _ptr(offsets), _ptr(lens), n, _ptr(packed), _ptr(po_), _ptr(nmask), _ptr(no_),
                               None, None), "rb_pack_reads")
    return packed, po_, nmask, no_


def threshold(readlen, k, error_rate=0.1, significance=0.95):
    return lib().rb_threshold(readlen, k, error_rate, significance)


def calculate_ci(error_rate, k, readlen, significance):
    lo, hi = C.c_uint16(), C.c_uint16()
    st = lib().rb_calculate_ci(error_rate, k, readlen, significance, C.byref(lo), C.byref(hi))
    return st, lo.value, hi.value


def calculate_filter_size_bits(fragment_length, k, h, max_fp, n_bins):
    return lib().rb_calculate_filter_size_bits(fragment_length, k, h, max_fp, n_bins)


def cut_out_nnns(seq):
    if isinstance(seq, str):
        seq = seq.encode()
    out = C.create_string_buffer(len(seq) + 1)
    n = lib().rb_cut_out_nnns(seq, len(seq), out)
    return out.raw[:n].decode()


def fragment_bounds(length, fragment_length, k, overlap=1500):
    n = lib().rb_fragment_bounds(length, fragment_length, k, overlap, None, None, 0)
    s = np.zeros(n, dtype=np.uint64)
    e = np.zeros(n, dtype=np.uint64)
    lib().rb_fragment_bounds(length, fragment_length, k, overlap, _ptr(s), _ptr(e), n)
    return s, e


def bin_occupancy_summary(bits, n_blocks, n_hash, max_fp=0.01):
    """rb_bin_occupancy_summarize -> dict (host arithmetic, no GPU)"""
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    out = BinOccupancySummary()
    _check(lib().rb_bin_occupancy_summarize(_ptr(bits), len(bits), n_blocks, n_hash, max_fp, C.byref(out)), "rb_bin_occupancy_summarize")
    return {k: getattr(out, k) for k, _ in BinOccupancySummary._fields_}


def bin_occupancy_derive(bits, n_blocks, n_hash):
    """rb_bin_occupancy_derive -> (load, fpr, est_kmers), float64[n_bins] each (host arithmetic, no GPU)"""
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    load, fpr, est = (np.zeros(len(bits), dtype=np.float64) for _ in range(3))
    _check(lib().rb_bin_occupancy_derive(_ptr(bits), len(bits), n_blocks, n_hash, _ptr(load), _ptr(fpr), _ptr(est)), "rb_bin_occupancy_derive")
    return load, fpr, est


def is_ibf_file(path):
    return bool(lib().rb_is_ibf_file(os.fsencode(path)))


def last_warning():
    return lib().rb_last_warning().decode(errors="replace")


def device_count():
    return lib().rb_device_count()
