"""ctypes binding of libmdbg_hip.so (include/mdbg_hip.h) -- thin, no compute in Python.

There is no fallback: a missing library raises at import of :func:`lib`, and a missing or
non-gfx950 GPU raises :class:`MdbgError` from :class:`Context`.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MDBG_LIB") or os.path.join(_HERE, "libmdbg_hip.so")   # MDBG_LIB: experimental variant

MDBG_READ_LOW_COMPLEXITY = 1
MDBG_READ_LOW_QUALITY = 2
RECORDS_PLAIN, RECORDS_INIT = 0, 1      # MDBG_RECORDS_*: the forms of mdbg_minimizers_to_record_bytes
SEQ_ENTIRE, SEQ_LEFT, SEQ_RIGHT = 0, 1, 2   # MDBG_SEQ_*: the parts of a window mdbg_spans_extract cuts out ...
SEQ_BITSET, SEQ_ASCII = 0, 1                # ... and the forms it writes them in
SEQ_REQUEST = np.dtype([("window", "<u8"), ("part", "<u4"), ("reserved", "<u4")])                  # mdbg_seq_request
SEQ_RANGE = np.dtype([("read", "<u4"), ("start", "<u4"), ("length", "<u4"), ("reversed", "<u4")])  # mdbg_seq_range
STITCH_PIECE = np.dtype([("window", "<u8"), ("part", "<u4"), ("flip", "<u4")])                      # mdbg_stitch_piece
STITCH_NONE = 0xFFFFFFFFFFFFFFFF            # MDBG_STITCH_NONE: no sequence for this k-min-mer
CHAIN_FOUND, CHAIN_TOO_LONG = 1, 2          # MDBG_CHAIN_*: the flags of a row of mdbg_map_chains
CHAIN = np.dtype([("ref_read", "<u4"), ("flags", "<u4"), ("score", "<i4"), ("n_matches", "<u4"), ("query_reversed", "<u4"), ("reserved", "<u4"),
                  ("n_diff_query", "<i8"), ("n_diff_reference", "<i8"), ("query_start", "<i8"), ("query_end", "<i8"),
                  ("reference_start", "<i8"), ("reference_end", "<i8"), ("alignment_score", "<i8")])        # mdbg_chain
SELECTED = np.dtype([("ref_read", "<u4"), ("score", "<i4"), ("n_matches", "<u4"), ("part", "<u4"), ("pair", "<u8")])   # mdbg_selected
VERIFY_CHAIN, VERIFY_KEPT, VERIFY_ABSENT, VERIFY_TOO_LONG = 1, 2, 4, 8      # MDBG_VERIFY_*: the flags of a row of mdbg_map_verify
VERIFIED = np.dtype([("neighbour", "<u4"), ("flags", "<u4"), ("query_reversed", "<u4"), ("n_anchors", "<u4"),
                     ("n_matches", "<i4"), ("n_mismatches", "<i4"), ("n_deletions", "<i4"), ("n_insertions", "<i4"),
                     ("overhang_start", "<u4"), ("overhang_end", "<u4"), ("align_length", "<u4"), ("n_seeds", "<u4"),
                     ("reference_start", "<u4"), ("reference_end", "<u4"), ("query_start", "<u4"), ("query_end", "<u4")])     # mdbg_verified
REALIGN_CHAIN, REALIGN_ABSENT, REALIGN_TOO_LONG, REALIGN_SHORT = 1, 4, 8, 16      # MDBG_REALIGN_*: the flags of a row of mdbg_map_realign
REALIGN_MATCH, REALIGN_MISMATCH, REALIGN_INSERTION, REALIGN_DELETION = 0, 1, 2, 3   # the kind of an entry
REALIGN_NONE = 0xFFFFFFFF                                                           # an entry's missing index
REALIGNED = np.dtype([("neighbour", "<u4"), ("flags", "<u4"), ("oriented_reversed", "<u4"), ("chain_reversed", "<u4"), ("n_anchors", "<u4"), ("n_entries", "<u4"),
                      ("n_matches", "<i4"), ("n_mismatches", "<i4"), ("n_deletions", "<i4"), ("n_insertions", "<i4"),
                      ("reference_start_index", "<u4"), ("reference_end_index", "<u4")])     # mdbg_realigned


class MdbgError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libmdbg_hip error {code}: {msg}")
        self.code = code


class ScanParams(C.Structure):
    _fields_ = [("minimizer_size", C.c_uint32), ("density", C.c_float), ("hpc", C.c_int32),
                ("min_read_quality", C.c_float), ("repetitive", C.POINTER(C.c_uint32)),
                ("n_repetitive", C.c_uint32), ("apply_read_filters", C.c_int32), ("quality_window", C.c_int32), ("no_end_trim", C.c_int32),
                ("ignore_qualities", C.c_int32)]


class MapParams(C.Structure):
    _fields_ = [("max_chaining_band", C.c_uint32), ("min_anchors", C.c_uint32), ("query_begin", C.c_uint32), ("query_end", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class VerifyParams(C.Structure):
    _fields_ = [("max_chaining_band", C.c_uint32), ("max_overhang", C.c_uint32), ("min_overlap_length", C.c_uint32), ("min_identity", C.c_float),
                ("minimizer_size", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class RealignParams(C.Structure):
    _fields_ = [("max_chaining_band", C.c_uint32), ("assembly_density", C.c_float), ("min_minimizers", C.c_uint32), ("reserved", C.c_uint32 * 5)]


# name -> (restype, argtypes); every symbol include/mdbg_hip.h declares
_P = C.c_void_p
_u64p = C.POINTER(C.c_uint64)
_u32p = C.POINTER(C.c_uint32)
SIGNATURES = {
    "mdbg_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "mdbg_destroy": (None, [_P]),
    "mdbg_last_error": (C.c_char_p, [_P]),
    "mdbg_synchronize": (C.c_int, [_P]),
    "mdbg_stream": (_P, [_P]),
    "mdbg_device_info": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), _u64p]),
    "mdbg_set_option": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "mdbg_timing_enable": (C.c_int, [_P, C.c_int]),
    "mdbg_timing_reset": (C.c_int, [_P]),
    "mdbg_timing_get": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_double), _u64p]),
    "mdbg_reads_from_ascii": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.POINTER(_P)]),
    "mdbg_reads_from_packed": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.POINTER(_P)]),
    "mdbg_reads_from_packed_async": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.POINTER(_P)]),
    "mdbg_reads_attach_qualities_async": (C.c_int, [_P, _P, C.c_char_p, _P]),
    "mdbg_reads_mark_ascii": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_char_p, _P]),
    "mdbg_reads_wait": (C.c_int, [_P, _P]),
    "mdbg_reads_attach_qualities": (C.c_int, [_P, _P, C.c_char_p, _P]),
    "mdbg_reads_synthetic": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, _P, _P, C.c_uint32,
                                       C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(_P)]),
    "mdbg_reads_info": (C.c_int, [_P, _u32p, _u64p, _u64p]),
    "mdbg_reads_get": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _u32p]),
    "mdbg_reads_packed_to_host": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _u64p]),
    "mdbg_reads_export_ascii": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P, _u64p]),
    "mdbg_reads_export_qualities": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _u64p]),
    "mdbg_memcpy_device": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "mdbg_host_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "mdbg_host_free": (None, [_P, _P]),
    "mdbg_reads_free": (None, [_P]),
    "mdbg_scan": (C.c_int, [_P, _P, C.POINTER(ScanParams), C.POINTER(_P)]),
    "mdbg_minimizers_info": (C.c_int, [_P, _u32p, _u64p]),
    "mdbg_minimizers_to_host": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mdbg_minimizers_from_host": (C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(_P)]),
    "mdbg_minimizers_device_ptrs": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "mdbg_minimizers_free": (None, [_P]),
    "mdbg_minimizers_concat": (C.c_int, [_P, C.POINTER(_P), C.c_uint32, C.POINTER(_P)]),
    "mdbg_apply_density_threshold": (C.c_int, [_P, _P, C.c_float, C.POINTER(_P)]),
    "mdbg_purge_palindromes": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "mdbg_repetitive_minimizers": (C.c_int, [_P, _P, _P, _u32p]),
    "mdbg_census_create": (C.c_int, [_P, C.POINTER(_P)]),
    "mdbg_census_add": (C.c_int, [_P, _P, _P]),
    "mdbg_census_top": (C.c_int, [_P, _P, _P, _u32p]),
    "mdbg_census_free": (None, [_P]),
    "mdbg_kminmer_count_first": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "mdbg_prev_from_records": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(_P)]),
    "mdbg_prev_overlay_unitigs": (C.c_int, [_P, _P, _P, _P, C.c_uint32]),
    "mdbg_kminmer_count_refined": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.POINTER(_P)]),
    "mdbg_kminmer_index": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.POINTER(_P)]),
    "mdbg_table_info": (C.c_int, [_P, _u32p, _u64p, _u64p, C.POINTER(C.c_int)]),
    "mdbg_table_to_host": (C.c_int, [_P, _P, _P, _P]),
    "mdbg_table_to_host_range": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, _P, _P]),
    "mdbg_table_checksum": (C.c_int, [_P, _P, _u64p]),
    "mdbg_table_stats": (C.c_int, [_P, _u64p]),
    "mdbg_first_pass_info": (C.c_int, [_P, _u64p]),
    "mdbg_scan_info": (C.c_int, [_P, _u64p]),
    "mdbg_scan_confirm_info": (C.c_int, [_P, _u64p]),
    "mdbg_scan_persistent_info": (C.c_int, [_P, _u64p]),
    "mdbg_first_pass_form": (C.c_int, [_P, _u64p]),
    "mdbg_first_pass_slot_fall_backs": (C.c_int, [_P, _u64p]),
    "mdbg_step_kernel_name": (C.c_char_p, [C.c_uint32]),
    "mdbg_kernel_attributes": (C.c_int, [_P, C.c_char_p, _u64p]),
    "mdbg_stream_spin": (C.c_int, [_P, C.c_uint32]),
    "mdbg_minimizers_slice": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mdbg_shard_exchange_local": (C.c_int, [_P, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p), _u64p, C.POINTER(C.c_void_p)]),
    "mdbg_device_clock_khz": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "mdbg_table_lookup": (C.c_int, [_P, _P, _P, _P, C.c_uint64, _P]),
    "mdbg_edge_index": (C.c_int, [_P, _P, C.POINTER(_P), _u64p]),
    "mdbg_unitig_edge_index": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(_P), _u64p]),
    "mdbg_small_contigs": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P]),
    "mdbg_table_keys_to_host": (C.c_int, [_P, _P, _P]),
    "mdbg_table_free": (None, [_P]),
    "mdbg_kminmer_spans": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(_P)]),
    "mdbg_spans_info": (C.c_int, [_P, _u32p, _u64p, _u64p, _u32p]),
    "mdbg_spans_to_host": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mdbg_spans_device_ptrs": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "mdbg_spans_free": (None, [_P]),
    "mdbg_spans_extract": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_int, C.POINTER(_P)]),
    "mdbg_reads_extract_ranges": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, C.POINTER(_P)]),
    "mdbg_sequences_info": (C.c_int, [_P, _u64p, _u64p, _u64p, C.POINTER(C.c_int)]),
    "mdbg_sequences_to_host": (C.c_int, [_P, _P, _P, _P, _P]),
    "mdbg_sequences_device_ptrs": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "mdbg_sequences_free": (None, [_P]),
    "mdbg_spans_stitch": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_int, C.POINTER(_P)]),
    "mdbg_reads_stitch_ranges": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_int, C.POINTER(_P)]),
    "mdbg_sequences_to_fasta_bytes": (C.c_int, [_P, _P, _P, _P, C.POINTER(_P), _u64p]),
    "mdbg_row_words": (C.c_uint32, [C.c_uint32]),
    "mdbg_shard_begin": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(_P), C.POINTER(_P), _u64p]),
    "mdbg_shard_reduce": (C.c_int, [_P, _P, _P, C.c_uint64, C.POINTER(_P)]),
    "mdbg_shard_finish": (C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(_P)]),
    "mdbg_shard_free": (None, [_P]),
    "mdbg_shard_from_table": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(_P), C.POINTER(_P), _u64p]),
    "mdbg_shard_keep": (C.c_int, [_P, _P, _P, C.POINTER(_P)]),
    "mdbg_comm_unique_id": (C.c_int, [_P]),
    "mdbg_comm_create": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(_P)]),
    "mdbg_comm_create_mode": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "mdbg_comm_mode": (C.c_int, [_P]),
    "mdbg_comm_note": (C.c_char_p, [_P]),
    "mdbg_comm_times": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "mdbg_comm_adopt": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(_P)]),
    "mdbg_comm_destroy": (None, [_P]),
    "mdbg_comm_stats": (C.c_int, [_P, _u64p, C.POINTER(C.c_double)]),
    "mdbg_shard_abort": (C.c_int, [_P, _P, C.c_int]),
    "mdbg_kminmer_count_first_sharded": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "mdbg_shard_exchange": (C.c_int, [_P, _P, _P, _P, _u64p, C.POINTER(_P)]),
    "mdbg_bytes_create": (C.c_int, [_P, C.c_uint64, C.POINTER(_P)]),
    "mdbg_bytes_upload_async": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, _u64p]),
    "mdbg_bytes_upload_done": (C.c_int, [_P, _P, C.c_uint64, C.c_int]),
    "mdbg_bytes_free": (None, [_P]),
    "mdbg_minimizers_from_record_bytes": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.POINTER(_P)]),
    "mdbg_prev_from_record_bytes": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(_P)]),
    "mdbg_minimizers_to_record_bytes": (C.c_int, [_P, _P, C.c_int, C.POINTER(_P), _u64p]),
    "mdbg_reads_from_fastx_bytes": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.POINTER(_P), _u64p]),
    "mdbg_bytes_inflate_bgzf": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint64, _u64p]),
    "mdbg_bytes_download": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64]),
    "mdbg_gzip_stream_create": (C.c_int, [_P, C.POINTER(_P)]),
    "mdbg_gzip_stream_free": (None, [_P]),
    "mdbg_bytes_inflate_gzip": (C.c_int, [_P, _P, _P, _P, C.c_uint64, _P, C.c_uint64, _u64p, _u64p]),
    "mdbg_bytes_copy": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_uint64]),
    "mdbg_fastx_whole_records": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, _u64p, C.POINTER(C.c_int)]),
    "mdbg_bytes_prefix_sum": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.c_uint64, _P, C.c_uint64]),
    "mdbg_bytes_sort_u64_pairs": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_uint64, _u64p]),
    "mdbg_minimizers_attach_positions": (C.c_int, [_P, _P, _P]),
    "mdbg_map_index_build": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(_P)]),
    "mdbg_map_index_info": (C.c_int, [_P, _u64p]),
    "mdbg_map_index_to_host": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "mdbg_map_index_free": (None, [_P]),
    "mdbg_map_anchors": (C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(MapParams), C.POINTER(_P)]),
    "mdbg_anchors_info": (C.c_int, [_P, _u64p]),
    "mdbg_anchors_to_host": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mdbg_anchors_device_ptrs": (C.c_int, [_P, C.POINTER(_P)]),
    "mdbg_anchors_free": (None, [_P]),
    "mdbg_map_chains": (C.c_int, [_P, _P, C.POINTER(MapParams), C.POINTER(_P)]),
    "mdbg_chains_info": (C.c_int, [_P, _u64p]),
    "mdbg_chains_to_host": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "mdbg_chains_device_ptrs": (C.c_int, [_P, C.POINTER(_P)]),
    "mdbg_chains_free": (None, [_P]),
    "mdbg_map_select": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(_P)]),
    "mdbg_selection_from_host": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, C.POINTER(_P)]),
    "mdbg_map_select_merge": (C.c_int, [_P, C.POINTER(_P), C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "mdbg_selection_to_alignment_bytes": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(_P), _u64p]),
    "mdbg_selection_info": (C.c_int, [_P, _u64p]),
    "mdbg_selection_to_host": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "mdbg_selection_device_ptrs": (C.c_int, [_P, C.POINTER(_P)]),
    "mdbg_selection_free": (None, [_P]),
    "mdbg_select_lds_positions": (C.c_uint32, []),
    "mdbg_minimizers_attach_strands": (C.c_int, [_P, _P, _P, _P]),
    "mdbg_map_verify": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(VerifyParams), C.POINTER(_P)]),
    "mdbg_verification_info": (C.c_int, [_P, _u64p]),
    "mdbg_verification_to_host": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "mdbg_verification_device_ptrs": (C.c_int, [_P, C.POINTER(_P)]),
    "mdbg_verification_free": (None, [_P]),
    "mdbg_verify_lds_anchors": (C.c_uint32, []),
    "mdbg_verify_min_matches": (C.c_int, [C.POINTER(VerifyParams), C.c_uint32, _u32p]),
    "mdbg_map_realign": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(RealignParams), C.POINTER(_P)]),
    "mdbg_map_realign_pairs": (C.c_int, [_P, C.c_uint64, _P, _P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(RealignParams), C.POINTER(_P)]),
    "mdbg_realignment_info": (C.c_int, [_P, _u64p]),
    "mdbg_realignment_to_host": (C.c_int, [_P, _P] + [_P] * 11),
    "mdbg_realignment_device_ptrs": (C.c_int, [_P, C.POINTER(_P)]),
    "mdbg_realignment_free": (None, [_P]),
    "mdbg_realign_lds_entries": (C.c_uint32, []),
    "mdbg_minimizers_attach_qualities": (C.c_int, [_P, _P, _P]),
}

# mdbg_bgzf_block: src u64, then csize, isize, crc, reserved u32
BGZF_BLOCK = np.dtype([("src", "<u8"), ("csize", "<u4"), ("isize", "<u4"), ("crc", "<u4"), ("reserved", "<u4")])

GZIP_TO_END = (1 << 64) - 1

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Context:
    """One HIP device + stream (mdbg_create)."""

    def __init__(self, device: int = 0):
        self.h = C.c_void_p()
        rc = lib().mdbg_create(device, C.byref(self.h))
        if rc:
            raise MdbgError(rc, (lib().mdbg_last_error(None) or b"").decode())

    def check(self, rc: int) -> None:
        if rc:
            raise MdbgError(rc, (lib().mdbg_last_error(self.h) or b"").decode())

    def close(self) -> None:
        if self.h:
            lib().mdbg_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self) -> None:
        self.check(lib().mdbg_synchronize(self.h))

    def device_info(self) -> dict:
        arch = C.create_string_buffer(64)
        ncu, hbm = C.c_int(), C.c_uint64()
        self.check(lib().mdbg_device_info(self.h, arch, 64, C.byref(ncu), C.byref(hbm)))
        clk = C.c_int()
        lib().mdbg_device_clock_khz(self.h, C.byref(clk))
        return dict(arch=arch.value.decode(), n_cu=ncu.value, hbm_bytes=hbm.value, clock_khz=clk.value)

    def set_option(self, name: str, value: int) -> None:
        self.check(lib().mdbg_set_option(self.h, name.encode(), value))

    def stream_spin(self, microseconds: int) -> None:
        """One idle wave for that long on the context's stream (mdbg_stream_spin); returns at once."""
        self.check(lib().mdbg_stream_spin(self.h, microseconds))

    def first_pass_info(self) -> dict:
        """How the last kminmer_count_first of this context ran (mdbg_first_pass_info)."""
        a = (C.c_uint64 * 8)()
        self.check(lib().mdbg_first_pass_info(self.h, a))
        names = ("path", "groups", "bucket_bits", "levels", "attempts", "lds_slots", "buckets", "instances")
        return {k: int(v) for k, v in zip(names, a)}

    def first_pass_form(self) -> dict:
        """Which form the split kernels this context last launched took (mdbg_first_pass_form)."""
        a = (C.c_uint64 * 4)()
        self.check(lib().mdbg_first_pass_form(self.h, a))
        return {"split_threads": int(a[0]), "split_tile": int(a[1])}

    def table_wave_priority(self) -> int:
        """The wave priority this context's last purge, first-pass or prefix-scan kernel was launched with ("table_wave_priority";
        mdbg_first_pass_form, form[2])."""
        a = (C.c_uint64 * 4)()
        self.check(lib().mdbg_first_pass_form(self.h, a))
        return int(a[2])

    def first_pass_slot_fall_backs(self) -> int:
        """Instances of the last partitioned first pass whose LDS slot the bucket count looked up a second time
        (mdbg_first_pass_slot_fall_backs)."""
        n = C.c_uint64()
        self.check(lib().mdbg_first_pass_slot_fall_backs(self.h, C.byref(n)))
        return int(n.value)

    @staticmethod
    def step_kernel_names() -> list[str]:
        """The kernels of the headline step that mdbg_kernel_attributes knows (mdbg_step_kernel_name)."""
        names, i = [], 0
        while (name := lib().mdbg_step_kernel_name(i)) is not None:
            names.append(name.decode())
            i += 1
        return names

    def kernel_attributes(self, kernel: str) -> dict:
        """Registers, LDS and threads of one kernel of the step in the loaded code object (mdbg_kernel_attributes)."""
        a = (C.c_uint64 * 8)()
        self.check(lib().mdbg_kernel_attributes(self.h, kernel.encode(), a))
        names = ("registers", "static_lds", "max_threads", "threads", "role", "scratch")
        return {k: int(v) for k, v in zip(names, a)}

    def scan_info(self) -> dict:
        """Which block-structured scan kernels this context has launched (mdbg_scan_info)."""
        a = (C.c_uint64 * 8)()
        self.check(lib().mdbg_scan_info(self.h, a))
        names = ("prefiltered_launches", "block_launches", "bitmaps_built", "bitmap_bits_set", "bitmap_log2_bits", "prefilter_waves",
                 "last_prefiltered", "reads_segmented")
        return {k: int(v) for k, v in zip(names, a)}

    def scan_confirm_info(self) -> dict:
        """The selected-key table of the pre-filtered scan's confirmation (mdbg_scan_confirm_info)."""
        a = (C.c_uint64 * 4)()
        self.check(lib().mdbg_scan_confirm_info(self.h, a))
        names = ("tables_built", "table_buckets", "table_overflowed", "last_by_table")
        return {k: int(v) for k, v in zip(names, a)}

    def scan_persistent_info(self) -> dict:
        """The form of this context's last pre-filtered scan launch (mdbg_scan_persistent_info)."""
        a = (C.c_uint64 * 4)()
        self.check(lib().mdbg_scan_persistent_info(self.h, a))
        return {"form": "persistent" if a[0] else "chunked", "workgroups": int(a[1]), "grab_reads": int(a[2]), "persistent_launches": int(a[3])}

    # -- timing ---------------------------------------------------------------------------
    def timing(self, on: bool) -> None:
        self.check(lib().mdbg_timing_enable(self.h, int(on)))

    def timing_reset(self) -> None:
        self.check(lib().mdbg_timing_reset(self.h))

    def timing_get(self, kernel: str) -> tuple[float, int]:
        ms, n = C.c_double(), C.c_uint64()
        self.check(lib().mdbg_timing_get(self.h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # -- reads ------------------------------------------------------------------------------
    def reads_from_ascii(self, seqs: list[bytes], quals: list[bytes] | None = None) -> "Reads":
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in seqs], out=offs[1:])
        bases = b"".join(seqs)
        q = b"".join(quals) if quals is not None else None
        h = C.c_void_p()
        self.check(lib().mdbg_reads_from_ascii(self.h, bases, q, _ptr(offs), len(seqs), C.byref(h)))
        return Reads(self, h)

    def reads_from_packed(self, words: np.ndarray, word_off: np.ndarray, lens: np.ndarray, quals: list[bytes] | None = None) -> "Reads":
        words = np.ascontiguousarray(words, dtype=np.uint64)
        word_off = np.ascontiguousarray(word_off, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        h = C.c_void_p()
        self.check(lib().mdbg_reads_from_packed(self.h, _ptr(words), _ptr(word_off), _ptr(lens), len(lens), C.byref(h)))
        if quals is not None:
            offs = np.zeros(len(quals) + 1, dtype=np.uint64)
            np.cumsum([len(q) for q in quals], out=offs[1:])
            self.check(lib().mdbg_reads_attach_qualities(self.h, h, b"".join(quals), _ptr(offs)))
        return Reads(self, h)

    def reads_from_packed_async(self, words: np.ndarray, word_off: np.ndarray, lens: np.ndarray, quals: bytes | None = None,
                                qual_off: np.ndarray | None = None) -> "Reads":
        """The upload is queued on the context's upload stream and the call returns; the arrays must stay alive and untouched until
        reads.wait() (they are kept on the returned object).  Consumers (scan) order themselves after it on the device."""
        h = C.c_void_p()
        self.check(lib().mdbg_reads_from_packed_async(self.h, _ptr(words), _ptr(word_off), _ptr(lens), len(lens), C.byref(h)))
        r = Reads(self, h)
        r._keep = (words, word_off, lens, quals, qual_off)
        if quals is not None:
            self.check(lib().mdbg_reads_attach_qualities_async(self.h, h, quals, _ptr(qual_off)))
        return r

    def reads_synthetic(self, spec, first_read: int = 0, n_reads: int | None = None) -> "Reads":
        """HBM-resident reads [first_read, first_read + n_reads) of a synth.SynthSpec."""
        n = spec.n_reads if n_reads is None else n_reads
        slen = np.asarray(spec.species_len, dtype=np.uint64)
        thr = np.ascontiguousarray(spec.weight_thresholds(), dtype=np.uint64)
        h = C.c_void_p()
        self.check(lib().mdbg_reads_synthetic(self.h, spec.seed, n, spec.read_len, first_read, _ptr(slen), _ptr(thr),
                                              len(slen), spec.sub_threshold(), spec.ins_threshold(), spec.del_threshold(), spec.window(),
                                              int(spec.with_quality), C.byref(h)))
        return Reads(self, h)

    # -- minimizer space ----------------------------------------------------------------------
    def minimizers_from_host(self, mins: np.ndarray, offsets: np.ndarray) -> "Minimizers":
        mins = np.ascontiguousarray(mins, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        h = C.c_void_p()
        self.check(lib().mdbg_minimizers_from_host(self.h, _ptr(mins), _ptr(offsets), len(offsets) - 1, C.byref(h)))
        return Minimizers(self, h)

    def scan(self, reads: "Reads", K: int = 15, density: float = 0.005, hpc: bool = True,
             min_read_quality: float = 0.0, repetitive=None, apply_read_filters: bool = True,
             quality_window: int = 0, no_end_trim: bool = False, ignore_qualities: bool = False) -> "Minimizers":
        rep = np.ascontiguousarray(repetitive if repetitive is not None else [], dtype=np.uint32)
        p = ScanParams(K, density, int(hpc), min_read_quality, rep.ctypes.data_as(C.POINTER(C.c_uint32)), len(rep),
                       int(apply_read_filters), int(quality_window), int(no_end_trim), int(ignore_qualities))
        h = C.c_void_p()
        self.check(lib().mdbg_scan(self.h, reads.h, C.byref(p), C.byref(h)))
        return Minimizers(self, h)

    def apply_density_threshold(self, m: "Minimizers", density: float) -> "Minimizers":
        h = C.c_void_p()
        self.check(lib().mdbg_apply_density_threshold(self.h, m.h, C.c_float(density), C.byref(h)))
        return Minimizers(self, h)

    def purge_palindromes(self, m: "Minimizers", first_k: int, last_k: int) -> "Minimizers":
        h = C.c_void_p()
        self.check(lib().mdbg_purge_palindromes(self.h, m.h, first_k, last_k, C.byref(h)))
        return Minimizers(self, h)

    def repetitive_minimizers(self, m: "Minimizers", max_out: int = 4096) -> np.ndarray:
        out = np.zeros(max_out, dtype=np.uint32)
        n = C.c_uint32(max_out)
        self.check(lib().mdbg_repetitive_minimizers(self.h, m.h, _ptr(out), C.byref(n)))
        return out[: n.value].copy()

    def census(self) -> "Census":
        h = C.c_void_p()
        self.check(lib().mdbg_census_create(self.h, C.byref(h)))
        return Census(self, h)

    # -- k-min-mer tables -----------------------------------------------------------------------
    def kminmer_count_first(self, m: "Minimizers", k: int = 4, min_abundance: int = 0) -> "Table":
        h = C.c_void_p()
        self.check(lib().mdbg_kminmer_count_first(self.h, m.h, k, min_abundance, C.byref(h)))
        return Table(self, h)

    def prev_from_records(self, records: bytes | np.ndarray) -> "Table":
        raw = records if isinstance(records, (bytes, bytearray)) else np.ascontiguousarray(records).tobytes()
        h = C.c_void_p()
        self.check(lib().mdbg_prev_from_records(self.h, raw, len(raw) // 20, C.byref(h)))
        return Table(self, h)

    def prev_overlay_unitigs(self, prev: "Table", unitigs: "Minimizers", abundance: np.ndarray, k_prev: int) -> None:
        ab = np.ascontiguousarray(abundance, dtype=np.uint32)
        self.check(lib().mdbg_prev_overlay_unitigs(self.h, prev.h, unitigs.h, _ptr(ab), k_prev))

    def kminmer_count_refined(self, reads: "Minimizers", unitigs: "Minimizers | None", k: int, prev: "Table") -> "Table":
        h = C.c_void_p()
        self.check(lib().mdbg_kminmer_count_refined(self.h, reads.h, unitigs.h if unitigs else None, k, prev.h, C.byref(h)))
        return Table(self, h)

    def kminmer_index(self, reads: "Minimizers", unitigs: "Minimizers | None", k: int, prev: "Table") -> "Table":
        h = C.c_void_p()
        self.check(lib().mdbg_kminmer_index(self.h, reads.h, unitigs.h if unitigs else None, k, prev.h, C.byref(h)))
        return Table(self, h)

    def kminmer_spans(self, reads: "Reads", m: "Minimizers", K: int = 15, hpc: bool = True, k: int = 4) -> "Spans":
        """Per window of k minimizers its identity and where it lies in the original read (mdbg_kminmer_spans); K and hpc as the scan's."""
        h = C.c_void_p()
        self.check(lib().mdbg_kminmer_spans(self.h, reads.h, m.h, K, int(hpc), k, C.byref(h)))
        return Spans(self, h)

    def spans_extract(self, reads: "Reads", spans: "Spans", windows, parts, form: int = SEQ_BITSET) -> "Sequences":
        """The oriented sequences of (window, part) requests, packed as DnaBitset2 keeps them or as characters (mdbg_spans_extract):
        windows are flat window indices, parts SEQ_ENTIRE / SEQ_LEFT / SEQ_RIGHT (one value or one per request)."""
        req = np.zeros(len(windows), SEQ_REQUEST)
        req["window"], req["part"] = windows, parts
        return self.spans_extract_requests(reads, spans, req, form)

    def spans_extract_requests(self, reads: "Reads", spans: "Spans", requests: np.ndarray, form: int = SEQ_BITSET) -> "Sequences":
        """... from an array of SEQ_REQUEST records as the C ABI takes them."""
        req = np.ascontiguousarray(requests, SEQ_REQUEST)
        h = _P()
        self.check(lib().mdbg_spans_extract(self.h, reads.h, spans.h, _ptr(req), len(req), form, C.byref(h)))
        return Sequences(self, h)

    def reads_extract_ranges(self, reads: "Reads", read, start, length, reversed, form: int = SEQ_BITSET) -> "Sequences":
        """The sequences of ranges [start, start + length) of reads, reverse-complemented where `reversed` (mdbg_reads_extract_ranges)."""
        rg = np.zeros(len(read), SEQ_RANGE)
        rg["read"], rg["start"], rg["length"], rg["reversed"] = read, start, length, reversed
        h = _P()
        self.check(lib().mdbg_reads_extract_ranges(self.h, reads.h, _ptr(rg), len(rg), form, C.byref(h)))
        return Sequences(self, h)

    def spans_stitch(self, reads: "Reads", spans: "Spans", pieces: np.ndarray, piece_offsets, form: int = SEQ_BITSET) -> "Sequences":
        """Contig c = the oriented pieces piece_offsets[c] .. piece_offsets[c + 1] one behind the other (mdbg_spans_stitch); pieces is an array
        of STITCH_PIECE records (stitch_pieces builds it by the reference's rule)."""
        pc = np.ascontiguousarray(pieces, STITCH_PIECE)
        off = np.ascontiguousarray(piece_offsets, np.uint64)
        h = _P()
        self.check(lib().mdbg_spans_stitch(self.h, reads.h, spans.h, _ptr(pc) if len(pc) else None, _ptr(off), len(off) - 1, form, C.byref(h)))
        return Sequences(self, h)

    def reads_stitch_ranges(self, reads: "Reads", read, start, length, reversed, piece_offsets, form: int = SEQ_BITSET) -> "Sequences":
        """... of ranges [start, start + length) of reads, reverse-complemented where `reversed` (mdbg_reads_stitch_ranges)."""
        rg = np.zeros(len(read), SEQ_RANGE)
        rg["read"], rg["start"], rg["length"], rg["reversed"] = read, start, length, reversed
        off = np.ascontiguousarray(piece_offsets, np.uint64)
        h = _P()
        self.check(lib().mdbg_reads_stitch_ranges(self.h, reads.h, _ptr(rg) if len(rg) else None, _ptr(off), len(off) - 1, form, C.byref(h)))
        return Sequences(self, h)

    def sequences_to_fasta_bytes(self, seqs: "Sequences", names=None, circular=None) -> "DeviceBytes":
        """The text CreateBaseContigsFunctor writes for sequences in SEQ_BITSET form: ">ctg<name><l|c>" and the bases, a line each
        (mdbg_sequences_to_fasta_bytes).  names: the contigs' indices (None: 0, 1, 2 ...); circular: their flags 0 / 1 / 2 (None: 0; 2 is
        written "c" like 1, as the reference writes it)."""
        nm = None if names is None else np.ascontiguousarray(names, np.uint32)
        fl = None if circular is None else np.ascontiguousarray(circular, np.uint8)
        h, n = _P(), C.c_uint64()
        self.check(lib().mdbg_sequences_to_fasta_bytes(self.h, seqs.h, None if nm is None or not len(nm) else _ptr(nm), None if fl is None or not len(fl) else _ptr(fl),
                                                       C.byref(h), C.byref(n)))
        return DeviceBytes(self, h, n.value)

    def memcpy_device(self, dst_ptr: int, src_ptr: int, nbytes: int) -> None:
        self.check(lib().mdbg_memcpy_device(self.h, C.c_void_p(dst_ptr), C.c_void_p(src_ptr), nbytes))

    def edge_index(self, nodes: "Table") -> tuple["Table", int]:
        """EdgeIndexer: (table of distinct prefix/suffix identities, checksum as the reference logs it)."""
        h = C.c_void_p()
        ck = C.c_uint64()
        self.check(lib().mdbg_edge_index(self.h, nodes.h, C.byref(h), C.byref(ck)))
        return Table(self, h), ck.value

    def unitig_edge_index(self, unitigs: "Minimizers", k: int) -> tuple["Table", int]:
        """UnitigEdgeIndexer: distinct prefix/suffix identities of the first and last k-min-mer of every unitig."""
        h = C.c_void_p()
        ck = C.c_uint64()
        self.check(lib().mdbg_unitig_edge_index(self.h, unitigs.h, k, C.byref(h), C.byref(ck)))
        return Table(self, h), ck.value

    # -- record files handed over as bytes (mdbg_bytes_*) ------------------------------------------
    def bytes_from_host(self, raw: bytes, piece: int = 1 << 22) -> "DeviceBytes":
        """A file's bytes on the device, uploaded in pieces (tests: from ordinary memory, so every piece is a blocking copy)."""
        h = C.c_void_p()
        self.check(lib().mdbg_bytes_create(self.h, len(raw), C.byref(h)))
        b = DeviceBytes(self, h, len(raw))
        buf = np.frombuffer(raw, dtype=np.uint8)
        last = C.c_uint64(0)
        for at in range(0, len(raw), piece):
            n = min(piece, len(raw) - at)
            self.check(lib().mdbg_bytes_upload_async(self.h, h, at, buf[at:].ctypes.data_as(C.c_void_p), n, C.byref(last)))
        if last.value:
            rc = lib().mdbg_bytes_upload_done(self.h, h, last.value, 1)
            if rc != 1:
                self.check(rc if rc < 0 else -1)
        return b

    def minimizers_from_record_bytes(self, b: "DeviceBytes", offsets: np.ndarray, want_circular: bool = False):
        """read_data_corrected.txt / unitig_data.txt records taken apart on the device (mdbg_minimizers_from_record_bytes)."""
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offs) - 1
        circ = np.zeros(n, dtype=np.uint8) if want_circular else None
        h = C.c_void_p()
        self.check(lib().mdbg_minimizers_from_record_bytes(self.h, b.h, _ptr(offs), n, _ptr(circ), C.byref(h)))
        m = Minimizers(self, h)
        return (m, circ) if want_circular else m

    def minimizers_to_record_bytes(self, m: "Minimizers", form: int = RECORDS_PLAIN) -> "DeviceBytes":
        """The bytes of the set's record file, composed on the device (mdbg_minimizers_to_record_bytes): RECORDS_PLAIN is
        read_data_corrected.txt / unitig_data.txt (formats.write_minimizer_reads), RECORDS_INIT is read_data_init.txt
        (formats.build_read_data_init; scan output only).  The kernel is queued, not waited for: ``download`` on this context is ordered behind it."""
        h = C.c_void_p()
        n = C.c_uint64(0)
        self.check(lib().mdbg_minimizers_to_record_bytes(self.h, m.h, form, C.byref(h), C.byref(n)))
        return DeviceBytes(self, h, int(n.value))

    def prev_from_record_bytes(self, b: "DeviceBytes", n_records: int) -> "Table":
        h = C.c_void_p()
        self.check(lib().mdbg_prev_from_record_bytes(self.h, b.h, n_records, C.byref(h)))
        return Table(self, h)

    def reads_from_fastx_bytes(self, b: "DeviceBytes", begin: int = 0, end: int | None = None) -> "Reads":
        """FASTA / FASTQ text on the device -> reads (mdbg_reads_from_fastx_bytes); [begin, end) holds whole records.  The returned
        object's ``fastx_info`` is dict(format, n_reads, n_bases, n_masked)."""
        if end is None:
            end = b.n
        h = C.c_void_p()
        info = (C.c_uint64 * 4)()
        self.check(lib().mdbg_reads_from_fastx_bytes(self.h, b.h, begin, end, C.byref(h), info))
        r = Reads(self, h)
        r.fastx_info = dict(format=int(info[0]), n_reads=int(info[1]), n_bases=int(info[2]), n_masked=int(info[3]))
        return r

    # -- BGZF blocks inflated on the device ---------------------------------------------------------
    def bytes_create(self, n: int) -> "DeviceBytes":
        """An empty device buffer of n bytes (mdbg_bytes_create): the text a BGZF file inflates to."""
        h = C.c_void_p()
        self.check(lib().mdbg_bytes_create(self.h, n, C.byref(h)))
        return DeviceBytes(self, h, n)

    def inflate_bgzf(self, comp: "DeviceBytes", blocks, text: "DeviceBytes", text_at: int = 0) -> int:
        """``blocks`` -- (src, csize, isize, crc) per BGZF block, as formats.bgzf_blocks gives them -- inflated from ``comp`` to
        ``text[text_at ...)`` (mdbg_bytes_inflate_bgzf); returns the bytes of text."""
        table = np.zeros(len(blocks), dtype=BGZF_BLOCK)
        for i, (src, csize, isize, crc) in enumerate(blocks):
            table[i] = (src, csize, isize, crc, 0)
        n_text = C.c_uint64(0)
        self.check(lib().mdbg_bytes_inflate_bgzf(self.h, comp.h, _ptr(table) if len(table) else None, len(table), text.h, text_at, C.byref(n_text)))
        return int(n_text.value)

    # -- ordinary gzip inflated on the device --------------------------------------------------------
    def gzip_stream(self) -> "GzipStream":
        """What one gzip file carries from call to call of ``inflate_gzip`` (mdbg_gzip_stream_create)."""
        h = C.c_void_p()
        self.check(lib().mdbg_gzip_stream_create(self.h, C.byref(h)))
        return GzipStream(self, h)

    def inflate_gzip(self, stream: "GzipStream", comp: "DeviceBytes", chunks, text: "DeviceBytes", text_at: int = 0) -> dict:
        """``chunks`` -- (start_bit, stop_bit) counted from the start of ``comp``, the last stop possibly GZIP_TO_END -- inflated to
        ``text[text_at ...)`` (mdbg_bytes_inflate_gzip); returns dict(n_text, members, ended, end_bit).  When the text does not fit,
        the MdbgError (code -5) carries the room needed as ``needed``."""
        table = np.zeros((len(chunks), 2), dtype=np.uint64)
        for i, (start, stop) in enumerate(chunks):
            table[i] = (start, stop)
        n_text = C.c_uint64(0)
        info = (C.c_uint64 * 4)()
        rc = lib().mdbg_bytes_inflate_gzip(self.h, stream.h, comp.h, _ptr(table) if len(table) else None, len(table), text.h, text_at, C.byref(n_text), info)
        if rc:
            e = MdbgError(rc, (lib().mdbg_last_error(self.h) or b"").decode())
            e.needed = int(n_text.value)
            raise e
        return dict(n_text=int(n_text.value), members=int(info[1]), ended=int(info[2]), end_bit=int(info[3]))

    def bytes_copy(self, dst: "DeviceBytes", dst_at: int, src: "DeviceBytes", src_at: int, n: int) -> None:
        """src[src_at, +n) to dst[dst_at, +n) on the device, in stream order (mdbg_bytes_copy)."""
        self.check(lib().mdbg_bytes_copy(self.h, dst.h, dst_at, src.h, src_at, n))

    def bytes_prefix_sum(self, src: "DeviceBytes", src_at: int, width: int, n: int, dst: "DeviceBytes", dst_at: int) -> None:
        """Exclusive prefix sums of the n values of ``width`` bytes at src[src_at ...): n + 1 uint64 at dst[dst_at ...), the last one the
        total; queued in stream order, not waited for (mdbg_bytes_prefix_sum)."""
        self.check(lib().mdbg_bytes_prefix_sum(self.h, src.h if src is not None else None, src_at, width, n, dst.h if dst is not None else None, dst_at))

    def bytes_sort_u64_pairs(self, keys: "DeviceBytes", keys_at: int, values: "DeviceBytes", values_at: int, n: int) -> dict:
        """The n uint64 keys at keys[keys_at ...) and their uint32 values at values[values_at ...) sorted by key in place, equal keys in
        their order (mdbg_bytes_sort_u64_pairs); returns dict(passes_run, passes_skipped)."""
        info = (C.c_uint64 * 2)()
        self.check(lib().mdbg_bytes_sort_u64_pairs(self.h, keys.h if keys is not None else None, keys_at, values.h if values is not None else None, values_at, n, info))
        return dict(passes_run=int(info[0]), passes_skipped=int(info[1]))

    # -- reads mapped against reads in minimizer space ------------------------------------------------
    def minimizers_with_positions(self, mins: np.ndarray, offsets: np.ndarray, positions: np.ndarray) -> "Minimizers":
        """A set from the host with the position array a scan output has (mdbg_minimizers_from_host + mdbg_minimizers_attach_positions)."""
        m = self.minimizers_from_host(mins, offsets)
        m.attach_positions(positions)
        return m

    @staticmethod
    def _map_params(band: int, min_anchors: int, query_begin: int, query_end: int) -> MapParams:
        return MapParams(band, min_anchors, query_begin, query_end, (C.c_uint32 * 4)())

    def map_index_build(self, chunk: "Minimizers", chunk_first_read: int = 0) -> "MapIndex":
        """Every window of two minimizers of the chunk's reads, grouped by pair (mdbg_map_index_build)."""
        h = C.c_void_p()
        self.check(lib().mdbg_map_index_build(self.h, chunk.h if chunk is not None else None, chunk_first_read, C.byref(h)))
        return MapIndex(self, h)

    def map_anchors(self, index: "MapIndex", queries: "Minimizers", query_first_read: int = 0, min_anchors: int = 3, query_begin: int = 0,
                    query_end: int = 0, band: int = 62) -> "Anchors":
        """The anchors of the query reads [query_begin, query_end) (0, 0: all) against the index, grouped per (query, reference read)
        (mdbg_map_anchors)."""
        h = C.c_void_p()
        p = self._map_params(band, min_anchors, query_begin, query_end)
        self.check(lib().mdbg_map_anchors(self.h, index.h if index is not None else None, queries.h if queries is not None else None, query_first_read, C.byref(p),
                                          C.byref(h)))
        return Anchors(self, h)

    def map_chains(self, anchors: "Anchors", band: int = 62) -> "Chains":
        """One chain row per pair of the anchors (mdbg_map_chains); band is max_chaining_band."""
        h = C.c_void_p()
        p = self._map_params(band, 0, 0, 0)
        self.check(lib().mdbg_map_chains(self.h, anchors.h if anchors is not None else None, C.byref(p), C.byref(h)))
        return Chains(self, h)

    def map_select(self, chains: "Chains", coverage: int = 20) -> "Selection":
        """The per-position selection of one chunk's chains (mdbg_map_select); coverage is _usedCoverageForCorrection."""
        h = C.c_void_p()
        self.check(lib().mdbg_map_select(self.h, chains.h if chains is not None else None, coverage, C.byref(h)))
        return Selection(self, h)

    def selection_from_host(self, sel_offsets, ref_read, match_offsets, matches) -> "Selection":
        """A selection made of stored parts; the library computes the scores from the lists (mdbg_selection_from_host)."""
        so = np.ascontiguousarray(sel_offsets, dtype=np.uint64)
        rr = np.ascontiguousarray(ref_read, dtype=np.uint32)
        mo = np.ascontiguousarray(match_offsets, dtype=np.uint64)
        mt = np.ascontiguousarray(matches, dtype=np.uint32)
        h = C.c_void_p()
        self.check(lib().mdbg_selection_from_host(self.h, len(so) - 1, _ptr(so), _ptr(rr) if len(rr) else None, _ptr(mo) if len(mo) else None,
                                                  _ptr(mt) if len(mt) else None, C.byref(h)))
        return Selection(self, h)

    def map_select_merge(self, parts, coverage: int = 20) -> "Selection":
        """The parts' rows of every query, in chunk order, selected again (mdbg_map_select_merge)."""
        arr = (C.c_void_p * max(len(parts), 1))(*[p.h if p is not None else None for p in parts])
        h = C.c_void_p()
        self.check(lib().mdbg_map_select_merge(self.h, arr, len(parts), coverage, C.byref(h)))
        return Selection(self, h)

    def selection_to_alignment_bytes(self, sel: "Selection", query_first_read: int = 0) -> "DeviceBytes":
        """The alignment file's bytes for the selection, composed on the device (mdbg_selection_to_alignment_bytes)."""
        h = C.c_void_p()
        n = C.c_uint64(0)
        self.check(lib().mdbg_selection_to_alignment_bytes(self.h, sel.h if sel is not None else None, query_first_read, C.byref(h), C.byref(n)))
        return DeviceBytes(self, h, int(n.value))

    @staticmethod
    def select_lds_positions() -> int:
        """Positions of a query up to which the selection counts in LDS (mdbg_select_lds_positions)."""
        return int(lib().mdbg_select_lds_positions())

    # -- the selected pairs verified at correction density --------------------------------------------
    def minimizers_with_strands(self, mins: np.ndarray, offsets: np.ndarray, positions: np.ndarray, directions: np.ndarray, read_lengths: np.ndarray) -> "Minimizers":
        """A set from the host with what mdbg_map_verify reads of a scan output: positions, directions, raw read lengths."""
        m = self.minimizers_with_positions(mins, offsets, positions)
        m.attach_strands(directions, read_lengths)
        return m

    @staticmethod
    def _verify_params(band: int, max_overhang: int, min_overlap_length: int, min_identity: float, minimizer_size: int) -> VerifyParams:
        return VerifyParams(band, max_overhang, min_overlap_length, min_identity, minimizer_size, (C.c_uint32 * 3)())

    def map_verify(self, sel: "Selection", reads: "Minimizers", target_first_read: int = 0, reads_first_read: int = 0, band: int = 62, max_overhang: int = 1000,
                   min_overlap_length: int = 1000, min_identity: float = 0.96, minimizer_size: int = 15) -> "Verification":
        """Every selected row's anchors at correction density, their chain, its summary and the verdict of filterAlignments (mdbg_map_verify)."""
        h = C.c_void_p()
        p = self._verify_params(band, max_overhang, min_overlap_length, min_identity, minimizer_size)
        self.check(lib().mdbg_map_verify(self.h, sel.h if sel is not None else None, target_first_read, reads.h if reads is not None else None, reads_first_read,
                                         C.byref(p), C.byref(h)))
        return Verification(self, h)

    @staticmethod
    def verify_lds_anchors() -> int:
        """Anchors of a pair (and minimizers of a neighbour) up to which mdbg_map_verify works in LDS (mdbg_verify_lds_anchors)."""
        return int(lib().mdbg_verify_lds_anchors())

    @staticmethod
    def verify_min_matches(n_seeds_max: int, min_identity: float = 0.96, minimizer_size: int = 15) -> np.ndarray:
        """min_matches[s], s = 0 ... n_seeds_max: the smallest n_matches whose identity passes (mdbg_verify_min_matches; host only)."""
        out = np.zeros(n_seeds_max + 1, np.uint32)
        p = Context._verify_params(1, 0, 0, min_identity, minimizer_size)
        rc = lib().mdbg_verify_min_matches(C.byref(p), n_seeds_max, out.ctypes.data_as(_u32p))
        if rc != 0:
            raise MdbgError(rc, "mdbg_verify_min_matches: invalid argument")
        return out

    # -- the kept pairs realigned at assembly density --------------------------------------------------
    def map_realign(self, v: "Verification", reads: "Minimizers", target_first_read: int = 0, reads_first_read: int = 0, band: int = 62, assembly_density: float = 0.005,
                    min_minimizers: int = 10) -> "Realignment":
        """Every kept pair thinned, oriented, joined, chained, listed and normalised, read from the verification on the device (mdbg_map_realign)."""
        h = C.c_void_p()
        p = RealignParams(band, assembly_density, min_minimizers, (C.c_uint32 * 5)())
        self.check(lib().mdbg_map_realign(self.h, v.h if v is not None else None, target_first_read, reads.h if reads is not None else None, reads_first_read, C.byref(p),
                                          C.byref(h)))
        return Realignment(self, h)

    def map_realign_pairs(self, kept_offsets: np.ndarray, kept_neighbour: np.ndarray, kept_reversed: np.ndarray, reads: "Minimizers", target_first_read: int = 0,
                          reads_first_read: int = 0, band: int = 62, assembly_density: float = 0.005, min_minimizers: int = 10) -> "Realignment":
        """The same for kept lists held on the host (mdbg_map_realign_pairs)."""
        off = np.ascontiguousarray(kept_offsets, dtype=np.uint64)
        nb = np.ascontiguousarray(kept_neighbour, dtype=np.uint32)
        rv = np.ascontiguousarray(kept_reversed, dtype=np.uint8)
        h = C.c_void_p()
        p = RealignParams(band, assembly_density, min_minimizers, (C.c_uint32 * 5)())
        self.check(lib().mdbg_map_realign_pairs(self.h, len(off) - 1, _ptr(off), _ptr(nb) if len(nb) else None, _ptr(rv) if len(rv) else None, target_first_read,
                                                reads.h if reads is not None else None, reads_first_read, C.byref(p), C.byref(h)))
        return Realignment(self, h)

    @staticmethod
    def realign_lds_entries() -> int:
        """Raw entries of a row up to which mdbg_map_realign normalises its list in LDS (mdbg_realign_lds_entries)."""
        return int(lib().mdbg_realign_lds_entries())

    def fastx_whole_records(self, text: "DeviceBytes", begin: int, end: int) -> tuple:
        """(cut, format): [begin, cut) of the text holds whole records when more may follow ``end`` (mdbg_fastx_whole_records)."""
        cut, fmt = C.c_uint64(0), C.c_int(0)
        self.check(lib().mdbg_fastx_whole_records(self.h, text.h, begin, end, C.byref(cut), C.byref(fmt)))
        return int(cut.value), int(fmt.value)

    def small_contigs(self, unitigs: "Minimizers", k: int, k_prev: int, prev: "Table") -> np.ndarray:
        """1 per unitig that IndexKminmerFunctor writes to smallContigs_k<k>.bin instead of indexing (k > 8 is the caller's test)."""
        n = unitigs.info()["n_reads"]
        flags = np.zeros(n, dtype=np.uint8)
        self.check(lib().mdbg_small_contigs(self.h, unitigs.h, k, k_prev, prev.h, flags.ctypes.data))
        return flags

    # -- the exchange inside the library (peer copies or RCCL) --------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = lib().mdbg_comm_unique_id(buf)
        if rc:
            raise MdbgError(rc, (lib().mdbg_last_error(None) or b"").decode())
        return buf.raw

    def minimizers_concat(self, parts: list) -> "Minimizers":
        """The reads of the parts, in order, as one set (appended on the device: mdbg_minimizers_concat)."""
        arr = (C.c_void_p * len(parts))(*[getattr(p.h, "value", p.h) for p in parts])
        h = C.c_void_p()
        self.check(lib().mdbg_minimizers_concat(self.h, arr, len(parts), C.byref(h)))
        return Minimizers(self, h)

    def minimizers_slice(self, m: "Minimizers", first_read: int, n_reads: int) -> "Minimizers":
        """Reads [first_read, first_read + n_reads) of m as a set of their own (mdbg_minimizers_slice)."""
        h = C.c_void_p()
        self.check(lib().mdbg_minimizers_slice(self.h, m.h, first_read, n_reads, C.byref(h)))
        return Minimizers(self, h)

    def comm_create(self, unique_id: bytes, rank: int, n_ranks: int, mode: "int | str" = -1) -> "Comm":
        """mode: "peer" | "rccl" | "auto" (or the MDBG_COMM_* value); -1: the environment's MDBG_COMM_MODE, "auto" when unset."""
        h = C.c_void_p()
        m = COMM_MODES[mode] if isinstance(mode, str) else int(mode)
        self.check(lib().mdbg_comm_create_mode(self.h, unique_id, rank, n_ranks, m, C.byref(h)))
        return Comm(h)

    def kminmer_count_first_sharded(self, comm: "Comm", m: "Minimizers", k: int = 4, min_abundance: int = 0) -> "Table":
        h = C.c_void_p()
        self.check(lib().mdbg_kminmer_count_first_sharded(self.h, comm.h, m.h, k, min_abundance, C.byref(h)))
        return Table(self, h)

    # -- sharded first pass (one process per GPU) ---------------------------------------------------
    def shard_from_table(self, local: "Table", n_ranks: int) -> "Shard":
        """Sharded k > firstK: the rows of a local refined / index table grouped by owner rank (reduce -> keep)."""
        h, d_rows = C.c_void_p(), C.c_void_p()
        counts = np.zeros(n_ranks, dtype=np.uint64)
        self.check(lib().mdbg_shard_from_table(self.h, local.h, n_ranks, C.byref(h), C.byref(d_rows), counts.ctypes.data_as(_u64p)))
        return Shard(self, h, local.info()["k"], d_rows.value or 0, counts)

    def shard_begin(self, m: "Minimizers", k: int, n_ranks: int) -> "Shard":
        h, d_rows = C.c_void_p(), C.c_void_p()
        counts = np.zeros(n_ranks, dtype=np.uint64)
        self.check(lib().mdbg_shard_begin(self.h, m.h, k, n_ranks, C.byref(h), C.byref(d_rows), counts.ctypes.data_as(_u64p)))
        sh = Shard(self, h, k, d_rows.value or 0, counts)
        sh.reads = m                             # mdbg_shard_begin: the reads must stay alive until mdbg_shard_free
        return sh


class Census:
    """Counts of minimizer values over several batches (mdbg_census_*)."""

    def __init__(self, ctx: "Context", h):
        self.ctx, self.h = ctx, h

    def add(self, m: "Minimizers") -> None:
        self.ctx.check(lib().mdbg_census_add(self.ctx.h, self.h, m.h))

    def top(self, max_out: int = 4096) -> np.ndarray:
        out = np.zeros(max_out, dtype=np.uint32)
        n = C.c_uint32(max_out)
        self.ctx.check(lib().mdbg_census_top(self.ctx.h, self.h, _ptr(out), C.byref(n)))
        return out[: n.value].copy()

    def free(self) -> None:
        if self.h:
            lib().mdbg_census_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


COMM_MODES = {"default": -1, "rccl": 0, "peer": 1, "auto": 2}


class Comm:
    """A communicator owned by the library (mdbg_comm_create_mode): peer copies or RCCL."""

    def __init__(self, h):
        self.h = h

    @property
    def mode(self) -> str:
        """The transport it ended up with: "peer" or "rccl" (mdbg_comm_mode)."""
        return {0: "rccl", 1: "peer"}.get(int(lib().mdbg_comm_mode(self.h)), "?")

    @property
    def note(self) -> str:
        """Why "auto" did not take the peer copies ("" if it did): mdbg_comm_note."""
        return (lib().mdbg_comm_note(self.h) or b"").decode()

    def stats(self) -> dict:
        """What the communicator carried so far (mdbg_comm_stats)."""
        st = (C.c_uint64 * 8)()
        ms = C.c_double()
        lib().mdbg_comm_stats(self.h, st, C.byref(ms))
        return dict(rank=int(st[0]), n_ranks=int(st[1]), rccl_ranks=int(st[2]), exchanges=int(st[3]), bytes_to_peers=int(st[4]),
                    bytes_from_peers=int(st[5]), bytes_local=int(st[6]), exchange_ms=float(ms.value), mode=self.mode, **self.times())

    def times(self) -> dict:
        """Where the time inside the exchanges went (mdbg_comm_times): the owner's reduction, waiting, and what is left: the transport's host time."""
        t = (C.c_double * 3)()
        lib().mdbg_comm_times(self.h, t)
        return dict(reduce_ms=float(t[1]), wait_ms=float(t[2]), host_ms=max(0.0, float(t[0]) - float(t[1]) - float(t[2])))

    def abort(self, ctx: "Context", code: int = -1) -> None:
        """This rank cannot enter the exchange its peers are about to enter: tell them (mdbg_shard_abort)."""
        lib().mdbg_shard_abort(ctx.h, self.h, code)

    def destroy(self) -> None:
        if self.h:
            lib().mdbg_comm_destroy(self.h)
            self.h = None


class DeviceView:
    """Zero-copy window on library-owned device memory for torch.as_tensor (__cuda_array_interface__)."""

    def __init__(self, ptr: int, shape: tuple, typestr: str = "<i8"):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}


class Shard:
    """State of one rank's sharded first pass: begin (rows to send) -> reduce (reply) -> finish (table)."""

    def __init__(self, ctx: Context, h, k: int, d_rows: int, counts: np.ndarray):
        self.ctx, self.h, self.k = ctx, h, k
        self.d_rows, self.counts = d_rows, counts
        self.row_words = lib().mdbg_row_words(k)

    @property
    def n_rows(self) -> int:
        return int(self.counts.sum())

    def reduce(self, d_recv: int, n_recv: int) -> int:
        """Device pointer of n_recv u64 replies (global count | bit 63 = lister) aligned with the received rows."""
        d_reply = C.c_void_p()
        self.ctx.check(lib().mdbg_shard_reduce(self.ctx.h, self.h, C.c_void_p(d_recv), n_recv, C.byref(d_reply)))
        return d_reply.value or 0

    def exchange(self, comm: "Comm") -> int:
        """Rows to their owners, reduce, replies back (inside the library, over the communicator's transport: peer copies or RCCL): device pointer of the replies for finish()."""
        d = C.c_void_p()
        self.ctx.check(lib().mdbg_shard_exchange(self.ctx.h, comm.h, self.h, C.c_void_p(self.d_rows), self.counts.ctypes.data_as(_u64p), C.byref(d)))
        return d.value or 0

    def finish(self, d_replies: int, min_abundance: int) -> "Table":
        h = C.c_void_p()
        self.ctx.check(lib().mdbg_shard_finish(self.ctx.h, self.h, C.c_void_p(d_replies), min_abundance, C.byref(h)))
        return Table(self.ctx, h)

    def keep(self, d_replies: int) -> "Table":
        """Sharded k > firstK: the rows of the local table this rank was told to list."""
        h = C.c_void_p()
        self.ctx.check(lib().mdbg_shard_keep(self.ctx.h, self.h, C.c_void_p(d_replies), C.byref(h)))
        return Table(self.ctx, h)

    def free(self):
        if self.h:
            lib().mdbg_shard_free(self.h)
            self.h = None


def exchange_local(ctx: Context, shards: list) -> list:
    """Both exchanges of a sharded pass among shards on one device (mdbg_shard_exchange_local): the replies' device pointers, one per shard."""
    n = len(shards)
    hs = (C.c_void_p * n)(*[s.h for s in shards])
    rows = (C.c_void_p * n)(*[C.c_void_p(s.d_rows) for s in shards])
    counts = np.ascontiguousarray(np.stack([np.asarray(s.counts, dtype=np.uint64) for s in shards]).reshape(-1))
    out = (C.c_void_p * n)()
    ctx.check(lib().mdbg_shard_exchange_local(ctx.h, hs, n, rows, counts.ctypes.data_as(_u64p), out))
    return [o or 0 for o in out]


class Reads:
    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h

    def info(self) -> dict:
        n, nb, nw = C.c_uint32(), C.c_uint64(), C.c_uint64()
        lib().mdbg_reads_info(self.h, C.byref(n), C.byref(nb), C.byref(nw))
        return dict(n_reads=n.value, n_bases=nb.value, n_words=nw.value)

    def get(self, index: int, with_quality: bool = False):
        L = C.c_uint32()
        self.ctx.check(lib().mdbg_reads_get(self.ctx.h, self.h, index, None, None, C.byref(L)))
        b = C.create_string_buffer(L.value + 1)
        q = C.create_string_buffer(L.value + 1) if with_quality else None
        self.ctx.check(lib().mdbg_reads_get(self.ctx.h, self.h, index, b, q, C.byref(L)))
        return (b.raw[: L.value], q.raw[: L.value]) if with_quality else b.raw[: L.value]

    def packed_to_host(self) -> dict:
        """The batch as the device holds it (mdbg_reads_packed_to_host): word_offsets, lengths, words, the invalid and break masks, the
        per-read masked flag, the masked list, and has_invalid / has_break / n_masked / n_words."""
        info = (C.c_uint64 * 4)()
        self.ctx.check(lib().mdbg_reads_packed_to_host(self.ctx.h, self.h, None, None, None, None, None, None, None, info))
        n, n_masked, nw = self.info()["n_reads"], int(info[2]), int(info[3])
        d = dict(word_offsets=np.zeros(n + 1, np.uint64), lengths=np.zeros(n, np.uint32), words=np.zeros(nw, np.uint64),
                 invalid=np.zeros(nw, np.uint32), breaks=np.zeros(nw, np.uint32), masked=np.zeros(n, np.uint8), masked_list=np.zeros(n_masked, np.uint32))
        self.ctx.check(lib().mdbg_reads_packed_to_host(self.ctx.h, self.h, *(_ptr(a) for a in d.values()), info))
        d.update(has_invalid=bool(info[0]), has_break=bool(info[1]), n_masked=int(info[2]), n_words=int(info[3]))
        return d

    def export_ascii(self, first: int, count: int) -> tuple[np.ndarray, np.ndarray]:
        """(bases u8[], offsets u64[count+1]) of reads [first, first+count)."""
        nb = C.c_uint64()
        self.ctx.check(lib().mdbg_reads_export_ascii(self.ctx.h, self.h, first, count, None, None, C.byref(nb)))
        bases = np.zeros(nb.value, dtype=np.uint8)
        offs = np.zeros(count + 1, dtype=np.uint64)
        self.ctx.check(lib().mdbg_reads_export_ascii(self.ctx.h, self.h, first, count, _ptr(bases), _ptr(offs), C.byref(nb)))
        return bases, offs

    def mark_ascii(self, index: list[int], seqs: list[bytes]) -> None:
        """The listed reads of a packed batch again as characters: their side masks are derived on the device (mdbg_reads_mark_ascii)."""
        idx = np.ascontiguousarray(index, dtype=np.uint32)
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in seqs], out=offs[1:])
        self.ctx.check(lib().mdbg_reads_mark_ascii(self.ctx.h, self.h, _ptr(idx), len(idx), b"".join(seqs), _ptr(offs)))

    def wait(self) -> None:
        """An asynchronous upload has arrived (mdbg_reads_wait)."""
        self.ctx.check(lib().mdbg_reads_wait(self.ctx.h, self.h))

    def export_qualities(self, first: int, count: int) -> np.ndarray:
        """phred+33 bytes of reads [first, first+count), concatenated (offsets as export_ascii's)."""
        nb = C.c_uint64()
        self.ctx.check(lib().mdbg_reads_export_qualities(self.ctx.h, self.h, first, count, None, C.byref(nb)))
        q = np.zeros(nb.value, dtype=np.uint8)
        self.ctx.check(lib().mdbg_reads_export_qualities(self.ctx.h, self.h, first, count, _ptr(q), C.byref(nb)))
        return q

    def free(self) -> None:
        if self.h:
            lib().mdbg_reads_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBytes:
    def __init__(self, ctx: "Context", h, n: int):
        self.ctx, self.h, self.n = ctx, h, n

    def download(self, at: int, n: int) -> bytes:
        """Bytes [at, at + n) of the buffer, copied back (mdbg_bytes_download)."""
        out = np.zeros(n, dtype=np.uint8)
        self.ctx.check(lib().mdbg_bytes_download(self.ctx.h, self.h, at, _ptr(out) if n else None, n))
        return out.tobytes()

    def free(self) -> None:
        if self.h:
            lib().mdbg_bytes_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class GzipStream:
    def __init__(self, ctx: "Context", h):
        self.ctx, self.h = ctx, h

    def free(self) -> None:
        if self.h:
            lib().mdbg_gzip_stream_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Minimizers:
    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h

    def info(self) -> dict:
        n, t = C.c_uint32(), C.c_uint64()
        lib().mdbg_minimizers_info(self.h, C.byref(n), C.byref(t))
        return dict(n_reads=n.value, n_minimizers=t.value)

    def to_host(self, full: bool = True) -> dict:
        i = self.info()
        n, t = i["n_reads"], i["n_minimizers"]
        out = dict(offsets=np.zeros(n + 1, np.uint64), minimizers=np.zeros(t, np.uint32))
        if full:
            out.update(pos=np.zeros(t, np.uint32), dir=np.zeros(t, np.uint8), qual=np.zeros(t, np.uint8),
                       read_length=np.zeros(n, np.uint32), mean_quality=np.zeros(n, np.float32),
                       flags=np.zeros(n, np.uint8))
        self.ctx.check(lib().mdbg_minimizers_to_host(
            self.ctx.h, self.h, _ptr(out["offsets"]), _ptr(out["minimizers"]), _ptr(out.get("pos")), _ptr(out.get("dir")),
            _ptr(out.get("qual")), _ptr(out.get("read_length")), _ptr(out.get("mean_quality")), _ptr(out.get("flags"))))
        return out

    def device_ptrs(self) -> tuple[int, int]:
        a, b = C.c_void_p(), C.c_void_p()
        lib().mdbg_minimizers_device_ptrs(self.h, C.byref(a), C.byref(b))
        return a.value or 0, b.value or 0

    def attach_positions(self, positions: np.ndarray) -> None:
        """One position per minimizer, strictly rising inside a read and below 2^31 (mdbg_minimizers_attach_positions)."""
        pos = np.ascontiguousarray(positions, dtype=np.uint32)
        self.ctx.check(lib().mdbg_minimizers_attach_positions(self.ctx.h, self.h, _ptr(pos) if len(pos) else None))

    def attach_strands(self, directions: np.ndarray, read_lengths: np.ndarray) -> None:
        """One direction byte (0 or 1) per minimizer and the raw length of every read (mdbg_minimizers_attach_strands)."""
        d = np.ascontiguousarray(directions, dtype=np.uint8)
        n = np.ascontiguousarray(read_lengths, dtype=np.uint32)
        self.ctx.check(lib().mdbg_minimizers_attach_strands(self.ctx.h, self.h, _ptr(d) if len(d) else None, _ptr(n) if len(n) else None))

    def attach_qualities(self, qualities: np.ndarray) -> None:
        """One quality byte per minimizer, what a scan output carries (mdbg_minimizers_attach_qualities)."""
        q = np.ascontiguousarray(qualities, dtype=np.uint8)
        self.ctx.check(lib().mdbg_minimizers_attach_qualities(self.ctx.h, self.h, _ptr(q) if len(q) else None))

    def free(self) -> None:
        if self.h:
            lib().mdbg_minimizers_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _MapHandle:
    _free = None

    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h

    def free(self) -> None:
        if self.h:
            getattr(lib(), self._free)(self.h)
            self.h = None

    close = free

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MapIndex(_MapHandle):
    """The windows of a chunk's reads grouped by minimizer pair (mdbg_map_index_build)."""
    _free = "mdbg_map_index_free"

    def info(self) -> dict:
        a = (C.c_uint64 * 4)()
        lib().mdbg_map_index_info(self.h, a)
        return dict(zip(("n_entries", "n_pairs", "longest_run", "n_reads"), [int(v) for v in a]))

    def to_host(self) -> dict:
        n = self.info()["n_entries"]
        out = dict(pair=np.zeros(n, np.uint64), read=np.zeros(n, np.uint32), position=np.zeros(n, np.uint32), index=np.zeros(n, np.uint32),
                   reversed=np.zeros(n, np.uint8))
        self.ctx.check(lib().mdbg_map_index_to_host(self.ctx.h, self.h, *[_ptr(a) for a in out.values()]))
        return out


class Anchors(_MapHandle):
    """The anchors of a batch of query reads, grouped per (query, reference read) (mdbg_map_anchors)."""
    _free = "mdbg_anchors_free"
    _NAMES = ("pair_offsets", "pair_ref_read", "anchor_offsets", "ref_read", "ref_position", "ref_index", "query_position", "query_index", "reversed")

    def info(self) -> dict:
        a = (C.c_uint64 * 4)()
        lib().mdbg_anchors_info(self.h, a)
        return dict(zip(("n_queries", "n_pairs", "n_anchors", "longest_pair"), [int(v) for v in a]))

    def to_host(self) -> dict:
        i = self.info()
        q, p, n = i["n_queries"], i["n_pairs"], i["n_anchors"]
        out = dict(pair_offsets=np.zeros(q + 1, np.uint64), pair_ref_read=np.zeros(p, np.uint32), anchor_offsets=np.zeros(p + 1, np.uint64),
                   ref_read=np.zeros(n, np.uint32), ref_position=np.zeros(n, np.uint32), ref_index=np.zeros(n, np.uint32),
                   query_position=np.zeros(n, np.uint32), query_index=np.zeros(n, np.uint32), reversed=np.zeros(n, np.uint8))
        self.ctx.check(lib().mdbg_anchors_to_host(self.ctx.h, self.h, *[_ptr(a) for a in out.values()]))
        return out

    def device_ptrs(self) -> dict:
        p = (C.c_void_p * 9)()
        lib().mdbg_anchors_device_ptrs(self.h, p)
        return dict(zip(self._NAMES, [x or 0 for x in p]))


class Chains(_MapHandle):
    """One chain row per pair of an Anchors, and the match lists (mdbg_map_chains)."""
    _free = "mdbg_chains_free"

    def info(self) -> dict:
        a = (C.c_uint64 * 4)()
        lib().mdbg_chains_info(self.h, a)
        return dict(zip(("n_queries", "n_pairs", "n_chains", "n_matches"), [int(v) for v in a]))

    def to_host(self) -> dict:
        i = self.info()
        out = dict(pair_offsets=np.zeros(i["n_queries"] + 1, np.uint64), chains=np.zeros(i["n_pairs"], CHAIN),
                   match_offsets=np.zeros(i["n_pairs"] + 1, np.uint64), matches=np.zeros(i["n_matches"], np.uint32))
        self.ctx.check(lib().mdbg_chains_to_host(self.ctx.h, self.h, *[_ptr(a) for a in out.values()]))
        return out

    def device_ptrs(self) -> dict:
        p = (C.c_void_p * 4)()
        lib().mdbg_chains_device_ptrs(self.h, p)
        return dict(zip(("pair_offsets", "chains", "match_offsets", "matches"), [x or 0 for x in p]))


class Selection(_MapHandle):
    """The selected rows of every query and their match lists (mdbg_map_select, mdbg_selection_from_host, mdbg_map_select_merge)."""
    _free = "mdbg_selection_free"

    def info(self) -> dict:
        a = (C.c_uint64 * 4)()
        lib().mdbg_selection_info(self.h, a)
        return dict(zip(("n_queries", "n_selected", "n_matches", "n_candidates"), [int(v) for v in a]))

    def to_host(self) -> dict:
        i = self.info()
        out = dict(sel_offsets=np.zeros(i["n_queries"] + 1, np.uint64), rows=np.zeros(i["n_selected"], SELECTED),
                   match_offsets=np.zeros(i["n_selected"] + 1, np.uint64), matches=np.zeros(i["n_matches"], np.uint32))
        self.ctx.check(lib().mdbg_selection_to_host(self.ctx.h, self.h, *[_ptr(a) for a in out.values()]))
        return out

    def device_ptrs(self) -> dict:
        p = (C.c_void_p * 4)()
        lib().mdbg_selection_device_ptrs(self.h, p)
        return dict(zip(("sel_offsets", "rows", "match_offsets", "matches"), [x or 0 for x in p]))


class Verification(_MapHandle):
    """One verified row per selected row and the kept neighbours of every target (mdbg_map_verify)."""
    _free = "mdbg_verification_free"
    _NAMES = ("row_offsets", "rows", "kept_offsets", "kept_neighbour", "kept_reversed")

    def info(self) -> dict:
        a = (C.c_uint64 * 4)()
        lib().mdbg_verification_info(self.h, a)
        return dict(zip(("n_targets", "n_rows", "n_chains", "n_kept"), [int(v) for v in a]))

    def to_host(self) -> dict:
        i = self.info()
        out = dict(row_offsets=np.zeros(i["n_targets"] + 1, np.uint64), rows=np.zeros(i["n_rows"], VERIFIED), kept_offsets=np.zeros(i["n_targets"] + 1, np.uint64),
                   kept_neighbour=np.zeros(i["n_kept"], np.uint32), kept_reversed=np.zeros(i["n_kept"], np.uint8))
        self.ctx.check(lib().mdbg_verification_to_host(self.ctx.h, self.h, *[_ptr(a) for a in out.values()]))
        return out

    def device_ptrs(self) -> dict:
        p = (C.c_void_p * 5)()
        lib().mdbg_verification_device_ptrs(self.h, p)
        return dict(zip(self._NAMES, [x or 0 for x in p]))


class Realignment(_MapHandle):
    """One realigned row per kept pair, the normalised alignment lists and the thinned targets (mdbg_map_realign)."""
    _free = "mdbg_realignment_free"
    _NAMES = ("row_offsets", "rows", "entry_offsets", "ref_index", "query_index", "query_minimizer", "query_quality", "kind", "target_offsets", "target_minimizer",
              "target_quality")

    def info(self) -> dict:
        a = (C.c_uint64 * 4)()
        lib().mdbg_realignment_info(self.h, a)
        return dict(zip(("n_targets", "n_rows", "n_chains", "n_entries"), [int(v) for v in a]))

    def to_host(self) -> dict:
        i = self.info()
        t, r, e = i["n_targets"], i["n_rows"], i["n_entries"]
        target_offsets = np.zeros(t + 1, np.uint64)
        self.ctx.check(lib().mdbg_realignment_to_host(self.ctx.h, self.h, *([None] * 8 + [_ptr(target_offsets), None, None])))      # the backbone's size first
        b = int(target_offsets[-1])
        out = dict(row_offsets=np.zeros(t + 1, np.uint64), rows=np.zeros(r, REALIGNED), entry_offsets=np.zeros(r + 1, np.uint64), ref_index=np.zeros(e, np.uint32),
                   query_index=np.zeros(e, np.uint32), query_minimizer=np.zeros(e, np.uint32), query_quality=np.zeros(e, np.uint8), kind=np.zeros(e, np.uint8),
                   target_offsets=target_offsets, target_minimizer=np.zeros(b, np.uint32), target_quality=np.zeros(b, np.uint8))
        self.ctx.check(lib().mdbg_realignment_to_host(self.ctx.h, self.h, *[_ptr(a) for a in out.values()]))
        return out

    def device_ptrs(self) -> dict:
        p = (C.c_void_p * 11)()
        lib().mdbg_realignment_device_ptrs(self.h, p)
        return dict(zip(self._NAMES, [x or 0 for x in p]))


class Spans:
    """The k-min-mer spans of a batch (mdbg_kminmer_spans)."""

    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h

    def info(self) -> dict:
        n, t, w, k = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        lib().mdbg_spans_info(self.h, C.byref(n), C.byref(t), C.byref(w), C.byref(k))
        return dict(n_reads=n.value, n_minimizers=t.value, n_windows=w.value, k=k.value)

    def to_host(self) -> dict:
        i = self.info()
        n, t, w = i["n_reads"], i["n_minimizers"], i["n_windows"]
        out = dict(window_offsets=np.zeros(n + 1, np.uint64), min_start=np.zeros(t, np.uint32), min_end=np.zeros(t, np.uint32),
                   hash_lo=np.zeros(w, np.uint64), hash_hi=np.zeros(w, np.uint64), reversed=np.zeros(w, np.uint8),
                   pos_start=np.zeros(w, np.uint32), pos_end=np.zeros(w, np.uint32),
                   seq_length_start=np.zeros(w, np.uint32), seq_length_end=np.zeros(w, np.uint32))
        self.ctx.check(lib().mdbg_spans_to_host(self.ctx.h, self.h, *[_ptr(a) for a in out.values()]))
        return out

    def device_ptrs(self) -> dict:
        p = [C.c_void_p() for _ in range(5)]
        lib().mdbg_spans_device_ptrs(self.h, *[C.byref(x) for x in p])
        return dict(zip(("window_offsets", "hash_lo", "hash_hi", "pos_start", "pos_end"), [x.value or 0 for x in p]))

    def free(self) -> None:
        if self.h:
            lib().mdbg_spans_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def stitch_pieces(contigs, window_offsets=None) -> tuple[np.ndarray, np.ndarray]:
    """(pieces, piece_offsets) for Context.spans_stitch by the rule of CreateBaseContigsFunctor.  contigs: per contig a list of
    (window, contig_reversed) -- window a flat window index, or (read, window of the read) when window_offsets is given, or None for a
    window without a stored sequence (skipped, but it still counts as a position).  Window 0 takes SEQ_ENTIRE, a later window SEQ_RIGHT
    when the contig's window is forward and SEQ_LEFT when it is reversed; flip is the contig window's orientation."""
    pieces = np.zeros(sum(len(c) for c in contigs), STITCH_PIECE)
    offsets = np.zeros(len(contigs) + 1, np.uint64)
    at = 0
    for c, contig in enumerate(contigs):
        for i, (window, rev) in enumerate(contig):
            if window is None:
                pieces[at] = (STITCH_NONE, 0, 0)
            else:
                if window_offsets is not None:
                    window = int(window_offsets[window[0]]) + int(window[1])
                pieces[at] = (window, SEQ_ENTIRE if i == 0 else SEQ_LEFT if rev else SEQ_RIGHT, 1 if rev else 0)
            at += 1
        offsets[c + 1] = at
    return pieces, offsets


class Sequences:
    """Sequences cut out of the reads (mdbg_spans_extract / mdbg_reads_extract_ranges) or stitched from them (mdbg_spans_stitch /
    mdbg_reads_stitch_ranges)."""

    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h

    def info(self) -> dict:
        n, b, y, f = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        lib().mdbg_sequences_info(self.h, C.byref(n), C.byref(b), C.byref(y), C.byref(f))
        return dict(n=n.value, n_bases=b.value, n_bytes=y.value, form=f.value)

    def to_host(self) -> dict:
        i = self.info()
        out = dict(byte_offsets=np.zeros(i["n"] + 1, np.uint64), lengths=np.zeros(i["n"], np.uint32), bytes=np.zeros(i["n_bytes"], np.uint8))
        self.ctx.check(lib().mdbg_sequences_to_host(self.ctx.h, self.h, *[_ptr(a) for a in out.values()]))
        return out

    def device_ptrs(self) -> dict:
        p = [C.c_void_p() for _ in range(3)]
        lib().mdbg_sequences_device_ptrs(self.h, *[C.byref(x) for x in p])
        return dict(zip(("byte_offsets", "lengths", "bytes"), [x.value or 0 for x in p]))

    def close(self) -> None:
        if self.h:
            lib().mdbg_sequences_free(self.h)
            self.h = None

    free = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Table:
    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h

    def info(self) -> dict:
        k, n, ns, hv = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_int()
        lib().mdbg_table_info(self.h, C.byref(k), C.byref(n), C.byref(ns), C.byref(hv))
        return dict(k=k.value, n_records=n.value, n_solid=ns.value, has_vectors=bool(hv.value))

    def to_host(self) -> tuple[np.ndarray, np.ndarray | None]:
        """(records as formats.ABUNDANCE_DTYPE array, vectors u32[n,k] or None)."""
        from .formats import ABUNDANCE_DTYPE
        i = self.info()
        rec = np.zeros(i["n_records"], dtype=ABUNDANCE_DTYPE)
        vec = np.zeros((i["n_records"], i["k"]), dtype=np.uint32) if i["has_vectors"] else None
        self.ctx.check(lib().mdbg_table_to_host(self.ctx.h, self.h, _ptr(rec), _ptr(vec)))
        return rec, vec

    def stats(self) -> dict:
        """What the pass that built the table walked (mdbg_table_stats)."""
        s = (C.c_uint64 * 4)()
        lib().mdbg_table_stats(self.h, s)
        return dict(minimizers=int(s[0]), instances=int(s[1]), keys=int(s[2]), slots=int(s[3]))

    def checksum(self) -> tuple:
        """(sum abundance * hash_lo -- the reference's "Checksum kminmer abundance" --, sum abundance, sum hash_hi, vector sum),
        all modulo 2^64, computed on the device (mdbg_table_checksum)."""
        s = (C.c_uint64 * 4)()
        self.ctx.check(lib().mdbg_table_checksum(self.ctx.h, self.h, s))
        return tuple(int(x) for x in s)

    def to_host_range(self, first: int, count: int) -> tuple[np.ndarray, np.ndarray | None]:
        """Rows [first, first + count) as to_host gives them."""
        from .formats import ABUNDANCE_DTYPE
        i = self.info()
        rec = np.zeros(count, dtype=ABUNDANCE_DTYPE)
        vec = np.zeros((count, i["k"]), dtype=np.uint32) if i["has_vectors"] else None
        self.ctx.check(lib().mdbg_table_to_host_range(self.ctx.h, self.h, first, count, _ptr(rec), _ptr(vec)))
        return rec, vec

    def keys_to_host(self) -> np.ndarray:
        """(n, 2) u64 array of (lo, hi) -- the 16-byte little-endian u128 records of edges.bin."""
        n = self.info()["n_records"]
        out = np.zeros((n, 2), dtype=np.uint64)
        self.ctx.check(lib().mdbg_table_keys_to_host(self.ctx.h, self.h, _ptr(out)))
        return out

    def lookup(self, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        hi = np.ascontiguousarray(hi, dtype=np.uint64)
        out = np.zeros(len(lo), dtype=np.uint32)
        self.ctx.check(lib().mdbg_table_lookup(self.ctx.h, self.h, _ptr(lo), _ptr(hi), len(lo), _ptr(out)))
        return out

    def free(self) -> None:
        if self.h:
            lib().mdbg_table_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
