"""ctypes binding of libsparkbam_hip.so (the C-ABI declared in include/sparkbam.h).

There is no CPU fallback: if the HIP library is missing or cannot be loaded, every
entry point raises.  The library is built in-tree by spark-bam_amd/csrc/Makefile
(``__graft_entry__.build()``).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SBH_LIB_PATH") or os.path.join(HERE, "libsparkbam_hip.so")

SBH_OK = 0
STATUS_NAMES = {
    0: "SBH_OK", 1: "SBH_E_ARG", 2: "SBH_E_HIP", 3: "SBH_E_NOMEM", 10: "SBH_E_HEADER_PARSE",
    11: "SBH_E_HEADER_SEARCH_FAILED", 12: "SBH_E_TRUNCATED", 13: "SBH_E_INFLATE_SIZE",
    14: "SBH_E_INFLATE_DATA", 15: "SBH_E_BAD_ISIZE", 16: "SBH_E_NO_READ_FOUND",
    17: "SBH_E_NEED_HALO", 18: "SBH_E_STATE", 19: "SBH_E_NOT_FOUND", 20: "SBH_E_BAD_RECORD",
    21: "SBH_E_UNSORTED",
}
SBH_E_ARG, SBH_E_HIP, SBH_E_HEADER_PARSE, SBH_E_HEADER_SEARCH_FAILED = 1, 2, 10, 11
SBH_E_TRUNCATED, SBH_E_INFLATE_SIZE, SBH_E_INFLATE_DATA, SBH_E_BAD_ISIZE = 12, 13, 14, 15
SBH_E_NO_READ_FOUND, SBH_E_NEED_HALO, SBH_E_STATE, SBH_E_NOT_FOUND = 16, 17, 18, 19
SBH_E_BAD_RECORD = 20
SBH_E_UNSORTED = 21  # sbh_bai_scan / sbh_bai_build: records out of coordinate order

FULL_SUCCESS = 0x80000000
FULL_UNKNOWN = 0x40000000
FULL_N_SHIFT = 20
FULL_FLAGS_MASK = 0x7FFFF
BLOCK_EMPTY, BLOCK_TRUNCATED = 1, 2
PATH_PARALLEL, PATH_STORED, PATH_SERIAL = 0, 1, 2  # sbh_inflate_paths

# Every symbol include/sparkbam.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "sbh_ctx_create", "sbh_ctx_destroy", "sbh_last_error", "sbh_last_error_detail", "sbh_ctx_set_stream",
    "sbh_ctx_synchronize", "sbh_version", "sbh_host_alloc", "sbh_host_free", "sbh_header_make", "sbh_shard_create",
    "sbh_shard_destroy", "sbh_shard_comp_device_ptr", "sbh_find_block_start", "sbh_index",
    "sbh_get_blocks", "sbh_inflate", "sbh_inflate_paths", "sbh_read_flat", "sbh_flat_device_ptr", "sbh_flat_of",
    "sbh_pos_of", "sbh_flat_bound", "sbh_set_contigs", "sbh_check_eager", "sbh_eager_bits", "sbh_check_full",
    "sbh_find_record_start", "sbh_count_records", "sbh_chain_from", "sbh_split", "sbh_split_starts",
    "sbh_check_records", "sbh_run_shard",
    "sbh_stage_times", "sbh_run_stream", "sbh_run_stream2", "sbh_records_scan", "sbh_records_fetch", "sbh_records_scan_regions", "sbh_verify_crc",
    "sbh_bgzf_compress_bound", "sbh_bgzf_compress", "sbh_bgzf_compress_level",
    "sbh_shard_load", "sbh_find_blocks", "sbh_check_stream", "sbh_split_records", "sbh_split_records_batch",
    "sbh_bai_scan", "sbh_bai_fetch", "sbh_bai_edges", "sbh_bai_bound", "sbh_bai_build",
    "sbh_records_sam_scan", "sbh_records_sam_fetch", "sbh_sam_render_host",
    "sbh_records_bam_scan", "sbh_records_bam_device_ptr", "sbh_records_bam_fetch", "sbh_records_bam_read",
    "sbh_bam_gather_host",
    "sbh_records_bam_scan_order", "sbh_records_bam_sorted", "sbh_bam_sort_host", "sbh_bam_header_set_so",
    "sbh_records_bam_scan_names", "sbh_records_bam_name_info", "sbh_bam_name_sort_host",
    "sbh_depth_create", "sbh_depth_destroy", "sbh_depth_reset", "sbh_records_depth_add", "sbh_depth_finish",
    "sbh_depth_fetch", "sbh_depth_runs_fetch", "sbh_depth_device_ptr", "sbh_depth_slots", "sbh_depth_add_host",
    "sbh_depth_finish_host",
    "sbh_pileup_create", "sbh_pileup_destroy", "sbh_pileup_reset", "sbh_records_pileup_add", "sbh_pileup_finish",
    "sbh_pileup_counts_fetch", "sbh_pileup_calls_fetch", "sbh_pileup_intervals_fetch", "sbh_pileup_device_ptr", "sbh_pileup_budget",
    "sbh_pileup_add_host", "sbh_pileup_finish_host",
    "sbh_tally_create", "sbh_tally_destroy", "sbh_tally_reset", "sbh_records_tally_add", "sbh_tally_fetch",
    "sbh_tally_add_host",
    "sbh_stats_create", "sbh_stats_destroy", "sbh_stats_reset", "sbh_records_stats_add", "sbh_stats_fetch",
    "sbh_stats_add_host",
    "sbh_records_fastq_scan", "sbh_records_fastq_device_ptr", "sbh_records_fastq_fetch", "sbh_fastq_render_host",
]
ORDER_SCAN, ORDER_COORDINATE = 0, 1  # SBH_ORDER_*
FASTQ_FASTA, FASTQ_SUFFIX, FASTQ_SUFFIX_ALWAYS, FASTQ_SPLIT = 1, 2, 4, 8  # SBH_FASTQ_*
LEVEL_HTSJDK, LEVEL_FAST = 5, -1  # sbh_bgzf_compress_level: htsjdk's zlib level 5 / this library's own coder


class SbhBlock(C.Structure):
    _fields_ = [("start", C.c_uint64), ("ustart", C.c_uint64), ("csize", C.c_uint32),
                ("hsize", C.c_uint32), ("usize", C.c_uint32), ("flags", C.c_uint32)]


class SbhShardResult(C.Structure):
    _fields_ = [("n_blocks", C.c_uint64), ("comp_bytes", C.c_uint64), ("flat_bytes", C.c_uint64),
                ("n_true", C.c_uint64), ("first_vpos", C.c_uint64), ("count", C.c_uint64),
                ("exit_flat", C.c_uint64), ("status", C.c_int32), ("anomalies", C.c_int32)]


class SbhStreamResult(C.Structure):
    _fields_ = [("n_windows", C.c_uint64), ("n_blocks", C.c_uint64), ("comp_bytes", C.c_uint64),
                ("flat_bytes", C.c_uint64), ("n_true", C.c_uint64), ("count", C.c_uint64),
                ("first_vpos", C.c_uint64), ("exit_vpos", C.c_uint64), ("status", C.c_int32),
                ("rewalks", C.c_int32), ("host_pinned", C.c_int32), ("pad", C.c_int32),
                ("ms_wall", C.c_double), ("ms_h2d", C.c_double), ("stage_ms", C.c_double * 6),
                ("halo_final", C.c_uint64), ("crc_bad_blocks", C.c_uint64), ("crc_first_bad", C.c_uint64),
                ("splits_host", C.c_uint64), ("ms_splits", C.c_double), ("ms_crc", C.c_double)]


class SbhStreamOpts(C.Structure):
    _fields_ = [("window", C.c_uint64), ("halo", C.c_uint64), ("reads_to_check", C.c_int32),
                ("max_read_size", C.c_int32), ("bgzf_blocks_to_check", C.c_int32), ("verify_crc", C.c_int32),
                ("split_start", C.c_void_p), ("split_end", C.c_void_p), ("n_splits", C.c_uint64),
                ("split_first_vpos", C.c_void_p), ("split_count", C.c_void_p), ("split_status", C.c_void_p),
                ("out_bits", C.c_void_p), ("out_bits_cap", C.c_uint64)]


class SbhCheckOpts(C.Structure):
    _fields_ = [("window", C.c_uint64), ("halo", C.c_uint64), ("reads_to_check", C.c_int32), ("full", C.c_int32),
                ("blocks", C.c_void_p), ("n_blocks", C.c_uint64), ("truth_vpos", C.c_void_p),
                ("n_truth", C.c_uint64), ("fp_vpos", C.c_void_p), ("fn_vpos", C.c_void_p), ("fp_cap", C.c_uint64),
                ("fn_cap", C.c_uint64), ("counts", C.c_void_p), ("rbe_hist", C.c_void_p),
                ("close_vpos", C.c_void_p), ("close_word", C.c_void_p), ("close_cap", C.c_uint64)]


class SbhCheckResult(C.Structure):
    _fields_ = [("n_windows", C.c_uint64), ("positions", C.c_uint64), ("comp_bytes", C.c_uint64),
                ("n_true", C.c_uint64), ("tp", C.c_uint64), ("fp", C.c_uint64), ("fn", C.c_uint64),
                ("unknown", C.c_uint64), ("n_success", C.c_uint64), ("n_close", C.c_uint64),
                ("halo_final", C.c_uint64), ("ms_wall", C.c_double), ("ms_h2d", C.c_double)]


class SbhRecordsSizes(C.Structure):
    _fields_ = [("n", C.c_uint64), ("name_bytes", C.c_uint64), ("cigar_ops", C.c_uint64),
                ("bases", C.c_uint64), ("aux_bytes", C.c_uint64)]


class SbhSplitRecordsResult(C.Structure):
    _fields_ = [("block_start", C.c_uint64), ("n_blocks", C.c_uint64), ("flat_size", C.c_uint64),
                ("owned_flat", C.c_uint64), ("first_flat", C.c_uint64),
                ("first_vpos", C.c_uint64), ("n_true", C.c_uint64), ("sizes", SbhRecordsSizes)]


class SbhBatchSplit(C.Structure):  # sbh_batch_split: one split of sbh_split_records_batch
    _fields_ = [("block_start", C.c_uint64), ("first_flat", C.c_uint64), ("first_vpos", C.c_uint64),
                ("owned_flat", C.c_uint64), ("rec_begin", C.c_uint64), ("rec_count", C.c_uint64),
                ("status", C.c_int32), ("host_path", C.c_int32)]


class SbhSplitBatchResult(C.Structure):
    _fields_ = [("block_start", C.c_uint64), ("n_blocks", C.c_uint64), ("flat_size", C.c_uint64),
                ("n_true", C.c_uint64), ("n_host", C.c_uint64), ("sizes", SbhRecordsSizes)]


class SbhBaiSizes(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_runs", C.c_uint64), ("n_no_coor", C.c_uint64),
                ("lin_size", C.c_uint64)]


class SbhSamSizes(C.Structure):
    _fields_ = [("n", C.c_uint64), ("text_bytes", C.c_uint64), ("n_host", C.c_uint64)]


class SbhRecordFilter(C.Structure):
    _fields_ = [("flag_require", C.c_uint32), ("flag_exclude", C.c_uint32), ("min_mapq", C.c_int32),
                ("pad", C.c_int32), ("row_begin", C.c_void_p), ("row_end", C.c_void_p), ("n_row_ranges", C.c_uint64)]


class SbhBamSizes(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_kept", C.c_uint64), ("bytes", C.c_uint64)]


class SbhBamNameInfo(C.Structure):  # sbh_bam_name_info
    _fields_ = [("n_names", C.c_uint64), ("n_single", C.c_uint64), ("n_pair", C.c_uint64), ("n_more", C.c_uint64),
                ("max_name", C.c_uint32), ("chunks_run", C.c_uint32), ("passes_run", C.c_uint32),
                ("already", C.c_int32)]


class SbhDepthAddResult(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_kept", C.c_uint64), ("n_counted", C.c_uint64), ("n_unplaced", C.c_uint64),
                ("cov_bases", C.c_uint64)]


class SbhPileupAddResult(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_kept", C.c_uint64), ("n_counted", C.c_uint64), ("n_unplaced", C.c_uint64),
                ("totals", C.c_uint64 * 8)]


class SbhPileupSizes(C.Structure):
    _fields_ = [("positions", C.c_uint64), ("n_intervals", C.c_uint64), ("nonzero", C.c_uint64),
                ("n_called", C.c_uint64), ("covered", C.c_uint64), ("totals", C.c_uint64 * 8),
                ("max_depth", C.c_uint32), ("pad", C.c_uint32)]


class SbhDepthSizes(C.Structure):
    _fields_ = [("slots", C.c_uint64), ("n_runs", C.c_uint64), ("covered", C.c_uint64), ("sum", C.c_uint64),
                ("max_depth", C.c_uint32), ("pad", C.c_uint32)]


class SbhTallyAddResult(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_kept", C.c_uint64)]


class SbhStatsParams(C.Structure):
    _fields_ = [("cycles", C.c_uint32), ("max_insert", C.c_uint32)]


class SbhStatsAddResult(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_kept", C.c_uint64), ("n_counted", C.c_uint64)]


class SbhFastqSizes(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_kept", C.c_uint64), ("text_bytes", C.c_uint64), ("part_bytes", C.c_uint64 * 3),
                ("part_rows", C.c_uint64 * 3)]


class SbhRecordsOut(C.Structure):  # host buffers (sbh_records_out); NULL = not copied
    _fields_ = [(f, C.c_void_p) for f in (
        "flat", "ref_id", "pos", "next_ref_id", "next_pos", "tlen", "flag", "bin", "mapq",
        "name_off", "cigar_off", "seq_off", "aux_off", "names", "cigar", "seq", "qual", "aux", "vpos")]


class SparkBamError(RuntimeError):
    """Maps an SBH_E_* status onto the reference's exception vocabulary.  `fields` are the
    values sbh_last_error_detail returned (what the reference's exception is built from)."""

    def __init__(self, code, message="", fields=()):
        self.code = code
        self.fields = tuple(fields)
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {message}")


class HeaderParseException(SparkBamError):
    """bgzf/.../block/HeaderParseException.scala:6-11: HeaderParseException(idx, actual, expected)."""

    def __init__(self, code, message="", fields=()):
        super().__init__(code, message, fields)
        _, self.idx, self.actual, self.expected = (list(fields) + [None] * 4)[:4]


class HeaderSearchFailedException(SparkBamError):
    """bgzf/.../block/HeaderSearchFailedException.scala:7-12: (path, start, positionsAttempted);
    the library knows no path: the caller that does sets it (with_path)."""

    def __init__(self, code, message="", fields=(), path=None):
        super().__init__(code, message, fields)
        self.start, self.positions_attempted = (list(fields) + [None] * 2)[:2]
        self.path = path

    def with_path(self, path):
        self.path = path
        return self


class NoReadFoundException(SparkBamError):
    """check/.../spark/FindRecordStart.scala:66-71: NoReadFoundException(path, start, maxReadSize)."""

    def __init__(self, code, message="", fields=(), path=None):
        super().__init__(code, message, fields)
        self.start, self.max_read_size = (list(fields) + [None] * 2)[:2]
        self.path = path

    def with_path(self, path, start=None):
        self.path = path
        if start is not None:
            self.start = start
        return self


# the status -> exception class the JNI shim throws (jni/sparkbam_jni.c EXCEPTIONS)
EXCEPTION_CLASSES = {}  # filled below, after the status constants


def error_for(code, message="", fields=()):
    return EXCEPTION_CLASSES.get(code, SparkBamError)(code, message, fields)


EXCEPTION_CLASSES.update({SBH_E_HEADER_PARSE: HeaderParseException,
                          SBH_E_HEADER_SEARCH_FAILED: HeaderSearchFailedException,
                          SBH_E_NO_READ_FOUND: NoReadFoundException})

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SparkBamError(SBH_E_STATE, f"HIP library not built: {LIB_PATH} "
                                         "(run __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    P, I32, U32, U64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64
    PU64, PI32, PU32 = C.POINTER(U64), C.POINTER(I32), C.POINTER(U32)
    sig = {
        "sbh_ctx_create": [I32, C.POINTER(P)],
        "sbh_ctx_destroy": [P],
        "sbh_ctx_set_stream": [P, P],
        "sbh_ctx_synchronize": [P],
        "sbh_host_alloc": [U64, C.POINTER(P)],
        "sbh_host_free": [P],
        "sbh_header_make": [P, U64, PI32, PI32],
        "sbh_shard_create": [P, P, U64, U64, U64, C.c_int, C.POINTER(P)],
        "sbh_shard_destroy": [P],
        "sbh_find_block_start": [P, U64, I32, PU64],
        "sbh_index": [P, U64, PU64, PU64],
        "sbh_get_blocks": [P, U64, U64, P],
        "sbh_inflate": [P, PU64],
        "sbh_read_flat": [P, U64, U64, P],
        "sbh_inflate_paths": [P, U64, U64, P],
        "sbh_flat_of": [P, U64, U32, PU64],
        "sbh_pos_of": [P, U64, PU64, PU32],
        "sbh_flat_bound": [P, U64, PU64],
        "sbh_set_contigs": [P, P, I32],
        "sbh_check_eager": [P, U64, U64, I32, P, PU64],
        "sbh_eager_bits": [P, U64, U64, P],
        "sbh_check_full": [P, U64, U64, I32, P, P, P, PU64, P, P, U64, PU64],
        "sbh_find_record_start": [P, U64, I32, I32, PU64, PI32],
        "sbh_count_records": [P, U64, U64, PU64],
        "sbh_split": [P, U64, U64, I32, I32, I32, PU64, PU64],
        "sbh_chain_from": [P, U64, U64, PU64, PU64],
        "sbh_split_starts": [P, P, P, U64, I32, I32, I32, P, P, P, PU64],
        "sbh_check_records": [P, P, P, U64, I32, P, U64, P, P, U64, P, U64],
        "sbh_run_shard": [P, U64, U64, I32, I32, C.POINTER(SbhShardResult)],
        "sbh_run_stream": [P, P, U64, U64, U64, U64, U64, U64, U64, P, I32, I32, I32, P, U64,
                           C.POINTER(SbhStreamResult)],
        "sbh_run_stream2": [P, P, U64, U64, U64, U64, U64, P, I32, C.POINTER(SbhStreamOpts),
                            C.POINTER(SbhStreamResult)],
        "sbh_records_scan": [P, U64, U64, C.POINTER(SbhRecordsSizes)],
        "sbh_records_fetch": [P, C.POINTER(SbhRecordsOut)],
        "sbh_split_records": [P, U64, U64, I32, I32, I32, I32, C.POINTER(SbhSplitRecordsResult)],
        "sbh_split_records_batch": [P, P, P, U64, I32, I32, I32, I32, C.POINTER(SbhBatchSplit),
                                    C.POINTER(SbhSplitBatchResult)],
        "sbh_records_scan_regions": [P, P, P, U64, P, P, P, C.c_uint32, C.POINTER(SbhRecordsSizes)],
        "sbh_verify_crc": [P, PU64, PU64],
        "sbh_shard_load": [P, P, U64, U64, C.c_int],
        "sbh_find_blocks": [P, P, U64, P, P, U64, I32, U64, P, U64, PU64],
        "sbh_check_stream": [P, P, U64, P, I32, C.POINTER(SbhCheckOpts), C.POINTER(SbhCheckResult)],
        "sbh_bai_scan": [P, U64, U64, C.POINTER(SbhBaiSizes)],
        "sbh_bai_fetch": [P, P, P],
        "sbh_bai_edges": [P, PI32, PI32, PI32, PI32],
        "sbh_bai_build": [P, U64, P, P, I32, U64, P, U64, PU64],
        "sbh_records_sam_scan": [P, P, P, I32, C.POINTER(SbhSamSizes)],
        "sbh_records_sam_fetch": [P, P, P],
        "sbh_sam_render_host": [P, U64, P, U64, P, P, I32, P, U64, P, PU64],
        "sbh_records_bam_scan": [P, P, U64, C.POINTER(SbhRecordFilter), C.POINTER(SbhBamSizes)],
        "sbh_records_bam_scan_order": [P, P, U64, C.POINTER(SbhRecordFilter), C.c_int, C.POINTER(SbhBamSizes)],
        "sbh_records_bam_sorted": [P, C.POINTER(C.c_int)],
        "sbh_bam_sort_host": [P, U64, P, U64, P, PU64],
        "sbh_records_bam_scan_names": [P, P, U64, C.POINTER(SbhRecordFilter), C.POINTER(SbhBamSizes)],
        "sbh_records_bam_name_info": [P, C.POINTER(SbhBamNameInfo)],
        "sbh_bam_name_sort_host": [P, U64, P, U64, P, C.POINTER(SbhBamNameInfo), PU64],
        "sbh_bam_header_set_so": [P, U64, C.c_char_p, P, U64, PU64],
        "sbh_records_bam_fetch": [P, P, P, P],
        "sbh_records_bam_read": [P, U64, U64, P],
        "sbh_bam_gather_host": [P, U64, P, U64, P, U64, C.POINTER(SbhRecordFilter), P, U64, P, P, PU64, PU64],
        "sbh_depth_create": [P, P, U32, I32, U32, C.POINTER(P)],
        "sbh_depth_destroy": [P],
        "sbh_depth_reset": [P],
        "sbh_records_depth_add": [P, P, C.POINTER(SbhRecordFilter), C.POINTER(SbhDepthAddResult)],
        "sbh_depth_finish": [P, C.POINTER(SbhDepthSizes)],
        "sbh_depth_fetch": [P, U32, U64, U64, P],
        "sbh_depth_runs_fetch": [P, U64, U64, P],
        "sbh_depth_add_host": [P, U64, P, U64, C.POINTER(SbhRecordFilter), P, U32, I32, U32, P,
                               C.POINTER(SbhDepthAddResult), PU64],
        "sbh_depth_finish_host": [P, P, U32, P, U64, C.POINTER(SbhDepthSizes)],
        "sbh_pileup_create": [P, P, U32, I32, I32, C.POINTER(P)],
        "sbh_pileup_destroy": [P],
        "sbh_pileup_reset": [P],
        "sbh_records_pileup_add": [P, P, C.POINTER(SbhRecordFilter), C.POINTER(SbhPileupAddResult)],
        "sbh_pileup_finish": [P, U32, U32, C.POINTER(SbhPileupSizes)],
        "sbh_pileup_counts_fetch": [P, U32, U64, U64, P],
        "sbh_pileup_calls_fetch": [P, U32, U64, U64, P],
        "sbh_pileup_intervals_fetch": [P, U64, U64, P],
        "sbh_pileup_budget": [P, PU64],
        "sbh_pileup_add_host": [P, U64, P, U64, C.POINTER(SbhRecordFilter), P, U32, I32, I32, P,
                                C.POINTER(SbhPileupAddResult), PU64],
        "sbh_pileup_finish_host": [P, P, U32, U32, U32, P, P, U64, C.POINTER(SbhPileupSizes)],
        "sbh_tally_create": [P, I32, C.POINTER(P)],
        "sbh_tally_destroy": [P],
        "sbh_tally_reset": [P],
        "sbh_records_tally_add": [P, P, C.POINTER(SbhRecordFilter), C.POINTER(SbhTallyAddResult)],
        "sbh_tally_fetch": [P, P, U64, U64, P],
        "sbh_tally_add_host": [P, U64, P, U64, C.POINTER(SbhRecordFilter), I32, P, P, C.POINTER(SbhTallyAddResult), PU64],
        "sbh_stats_create": [P, C.POINTER(SbhStatsParams), C.POINTER(P)],
        "sbh_stats_destroy": [P],
        "sbh_stats_reset": [P],
        "sbh_records_stats_add": [P, P, C.POINTER(SbhRecordFilter), C.POINTER(SbhStatsAddResult)],
        "sbh_stats_fetch": [P, P, P, P, P, P, P, P],
        "sbh_stats_add_host": [P, U64, P, U64, C.POINTER(SbhRecordFilter), C.POINTER(SbhStatsParams), P, P, P, P, P, P, P,
                               C.POINTER(SbhStatsAddResult), PU64],
        "sbh_records_fastq_scan": [P, C.POINTER(SbhRecordFilter), U32, I32, C.POINTER(SbhFastqSizes)],
        "sbh_records_fastq_fetch": [P, P, P, P],
        "sbh_fastq_render_host": [P, U64, P, U64, C.POINTER(SbhRecordFilter), U32, I32, P, U64, P, P,
                                  C.POINTER(SbhFastqSizes), PU64],
        "sbh_bgzf_compress": [P, P, U64, I32, P, U64, PU64, PU64, C.POINTER(C.c_float)],
        "sbh_bgzf_compress_level": [P, P, U64, I32, I32, P, U64, PU64, PU64, C.POINTER(C.c_float)],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = C.c_int
    L.sbh_bgzf_compress_bound.argtypes = [U64]
    L.sbh_bgzf_compress_bound.restype = U64
    L.sbh_bai_bound.argtypes = [U64, U64, I32]
    L.sbh_bai_bound.restype = U64
    L.sbh_depth_slots.argtypes = [P, U32]
    L.sbh_depth_slots.restype = U64
    L.sbh_depth_device_ptr.argtypes = [P, U32]
    L.sbh_depth_device_ptr.restype = P
    L.sbh_pileup_device_ptr.argtypes = [P, U32]
    L.sbh_pileup_device_ptr.restype = P
    L.sbh_stage_times.argtypes = [P, C.POINTER(C.c_double), I32]
    L.sbh_stage_times.restype = C.c_int
    L.sbh_last_error.argtypes = [P]
    L.sbh_last_error.restype = C.c_char_p
    L.sbh_last_error_detail.argtypes = [P, PI32, C.POINTER(C.c_int64), I32]
    L.sbh_last_error_detail.restype = I32
    L.sbh_version.argtypes = []
    L.sbh_version.restype = C.c_char_p
    for name in ("sbh_shard_comp_device_ptr", "sbh_flat_device_ptr", "sbh_records_bam_device_ptr",
                 "sbh_records_fastq_device_ptr"):
        getattr(L, name).argtypes = [P]
        getattr(L, name).restype = P
    _lib = L
    return L
