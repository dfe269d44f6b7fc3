/*
 * sparkbam.h -- C-ABI of libsparkbam_hip.so, the MI355X (gfx950) implementation of
 * spark-bam's BGZF-inflate + BAM record-boundary hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no framework types.  Each
 * entry point names the reference interface it replaces (paths relative to the
 * reference repository root).  The reference's host side is Scala on the JVM; the
 * JNI binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions:
 *  - Every call returns an int status: SBH_OK or one of SBH_E_*, which map one-to-one
 *    onto the reference's exceptions (see below).  sbh_last_error() gives the message.
 *  - The caller owns every host buffer.  A context owns its device memory.
 *  - Threading.  One context per device per process, shared by every thread (a Spark
 *    executor's concurrent tasks).  Any number of threads may call into one context at once
 *    as long as each SHARD is used by one thread at a time -- the reference's model, where
 *    each task builds its own channel and Checker (load/.../CanLoadBam.scala:316-320,
 *    check/.../PosChecker.scala:19-20 share buffers inside one checker only).  Each shard
 *    enqueues its device work on its own HIP stream, so two tasks' shards run concurrently
 *    and one task's waits cover its own work only; context-level calls (sbh_run_stream2,
 *    sbh_check_stream, sbh_find_blocks, sbh_bgzf_compress*) build their own shards per call
 *    (sbh_run_stream2 takes a window cache from a pool in the context, one per concurrent
 *    caller).  sbh_last_error / sbh_last_error_detail report the calling THREAD's last failed
 *    call on that context, so a task always reads back its own failure.  sbh_ctx_set_stream
 *    and sbh_ctx_destroy are setup/teardown calls: no other call may run on the context then
 *    (shards created after sbh_ctx_set_stream enqueue on the caller's stream instead of their own;
 *    which stream that may be, and the ordering the caller gets, are written at sbh_ctx_set_stream).
 *  - Offsets: "file offsets" are byte offsets in the compressed BGZF file; "flat"
 *    offsets index the shard's concatenated uncompressed bytes (the reference's
 *    UncompressedBytes view, bgzf/.../block/UncompressedBytes.scala:13-87).  A
 *    virtual position Pos(blockPos, offset) is the htsjdk long blockPos<<16|offset
 *    (bgzf/.../Pos.scala:24).
 */
#ifndef SPARKBAM_H
#define SPARKBAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define SBH_OK 0
#define SBH_E_ARG 1                  /* IllegalArgumentException                     */
#define SBH_E_HIP 2                  /* device/runtime failure                       */
#define SBH_E_NOMEM 3
#define SBH_E_HEADER_PARSE 10        /* HeaderParseException (Header.scala:50-57)    */
#define SBH_E_HEADER_SEARCH_FAILED 11 /* HeaderSearchFailedException (FindBlockStart.scala:31-35) */
#define SBH_E_TRUNCATED 12           /* EOFException escaping MetadataStream         */
#define SBH_E_INFLATE_SIZE 13        /* IOException "Expected N decompressed bytes"  (Stream.scala:52-54) */
#define SBH_E_INFLATE_DATA 14        /* java.util.zip.DataFormatException             */
#define SBH_E_BAD_ISIZE 15           /* ISIZE outside [0, 65536]                      */
#define SBH_E_NO_READ_FOUND 16       /* NoReadFoundException (FindRecordStart.scala:66-71) */
#define SBH_E_NEED_HALO 17           /* result depends on bytes past the resident range */
#define SBH_E_STATE 18               /* call order violated (e.g. check before inflate) */
#define SBH_E_NOT_FOUND 19           /* Pos not in the indexed block chain            */
#define SBH_E_BAD_RECORD 20          /* record does not fit its block / the stream (htsjdk decode throws) */
#define SBH_E_UNSORTED 21            /* BAI build: records not coordinate-sorted (htslib hts_idx_push refuses them) */

/* ---- full-checker result word (check/.../full/error/Flags.scala:21-45) ----
 *  bit 31     : Success(readsParsed)
 *  bit 30     : unknown (needs bytes past an open shard end; never in a valid run)
 *  bits 20-29 : readsParsed (Success) or readsBeforeError (Flags)
 *  bits 0-18  : the 19 Flags booleans in the serde order of Flags.scala:203-222:
 *    0 tooFewFixedBlockBytes  1 negativeReadIdx  2 tooLargeReadIdx  3 negativeReadPos
 *    4 tooLargeReadPos  5 negativeNextReadIdx  6 tooLargeNextReadIdx
 *    7 negativeNextReadPos  8 tooLargeNextReadPos  9 tooFewBytesForReadName
 *    10 nonNullTerminatedReadName  11 nonASCIIReadName  12 noReadName  13 emptyReadName
 *    14 tooFewBytesForCigarOps  15 invalidCigarOp  16 emptyMappedCigar
 *    17 emptyMappedSeq  18 tooFewRemainingBytesImplied                              */
#define SBH_FULL_SUCCESS 0x80000000u
#define SBH_FULL_UNKNOWN 0x40000000u
#define SBH_FULL_N_SHIFT 20
#define SBH_FULL_FLAGS_MASK 0x7FFFFu
/* Counts aggregation layout: counts[nnz * 19 + flag], nnz = Flags.numNonZeroFields
 * (Flags.scala:118-123) in [0, 21); rbe_hist[nnz * 64 + readsBeforeError]. */
#define SBH_NNZ_MAX 21
#define SBH_RBE_MAX 64

/* block flags */
#define SBH_BLOCK_EMPTY 1u     /* dataLength == 2: the stream ends at this block (Stream.scala:56-58) */
#define SBH_BLOCK_TRUNCATED 2u /* runs past the resident bytes                     */

typedef struct sbh_ctx sbh_ctx;
typedef struct sbh_shard sbh_shard;

/* bgzf Metadata(start, compressedSize, uncompressedSize) (bgzf/.../block/Metadata.scala:6-8)
 * plus the header size, flat start and inflate status. */
typedef struct {
  uint64_t start;  /* file offset of the block header */
  uint64_t ustart; /* flat offset of its first uncompressed byte */
  uint32_t csize;
  uint32_t hsize;
  uint32_t usize;
  uint32_t flags;  /* SBH_BLOCK_* */
} sbh_block;

/* ---- context ---- */
int sbh_ctx_create(int device, sbh_ctx **out);
int sbh_ctx_destroy(sbh_ctx *ctx);
const char *sbh_last_error(const sbh_ctx *ctx);
/* The last error's status and the fields the reference's exception is constructed from;
 * returns how many fields the error carries (fields[0..min(n, cap)) are written):
 *   SBH_E_HEADER_PARSE         {header file offset, idx, actual, expected}  -> HeaderParseException(idx: Int,
 *                              actual: Byte, expected: Byte) (bgzf/.../block/HeaderParseException.scala:6-11)
 *   SBH_E_HEADER_SEARCH_FAILED {start, positionsAttempted}  -> HeaderSearchFailedException(path, start,
 *                              positionsAttempted) (bgzf/.../block/HeaderSearchFailedException.scala:7-12)
 *   SBH_E_NO_READ_FOUND        {start (file offset of a split, or the flat position searched from),
 *                              maxReadSize} -> NoReadFoundException(path, start, maxReadSize)
 *                              (check/.../spark/FindRecordStart.scala:66-71)
 *   SBH_E_INFLATE_SIZE         {block start, expected bytes}  -> IOException (Stream.scala:52-54)
 *   SBH_E_INFLATE_DATA         {block start}  -> DataFormatException
 *   SBH_E_UNSORTED             {virtual offset of the first offending record}  (sbh_bai_scan)
 *   SBH_E_BAD_RECORD           {row of the first malformed record}  (sbh_records_sam_scan and
 *                              sbh_records_bam_scan only)
 *   anything else              no fields */
int32_t sbh_last_error_detail(const sbh_ctx *ctx, int32_t *code, int64_t *fields, int32_t cap);
/* Use a caller-owned hipStream_t.  Every shard created afterwards -- those the context-level calls
 * build for themselves included; idle window caches of sbh_run_stream2 are let go -- enqueues on it,
 * and so does sbh_bgzf_compress*.  Shards created before the call keep their own streams.
 *  - The stream must belong to the HIP runtime instance this library links (libamdhip64): create it
 *    with that runtime's hipStreamCreate*.  A handle of another instance loaded into the process
 *    means nothing here -- a torch build that ships its own libamdhip64.so has one, and then
 *    torch.cuda.current_stream().cuda_stream must not be passed; it may be when torch and this
 *    library resolve to the same libamdhip64.so.  NULL is legal and means the null stream.
 *  - Ordering.  What the caller enqueued on the stream before a call is complete before the call
 *    reads its inputs: a device-resident `comp` or `src` written on the stream (sbh_shard_create,
 *    sbh_shard_load, sbh_bgzf_compress*), page-locked host bytes a copy on the stream was filling
 *    (sbh_run_stream2).  Every call that enqueues device work returns with the stream drained
 *    (hipStreamQuery is hipSuccess), so its device results (sbh_flat_device_ptr, ...) can be used by
 *    work enqueued on the stream afterwards, or on any other stream.
 *  - The library never destroys the stream.  It must outlive every shard of the context; tasks that
 *    share the context then share the one stream, and one task's wait covers the others' work. */
int sbh_ctx_set_stream(sbh_ctx *ctx, void *hip_stream);
int sbh_ctx_synchronize(sbh_ctx *ctx);
const char *sbh_version(void);

/* Page-locked host memory (hipHostMalloc): compressed bytes handed over in it are copied to
 * HBM asynchronously, overlapping the kernels (sbh_run_stream).  A JNI binding wraps it in a
 * direct ByteBuffer. */
int sbh_host_alloc(uint64_t n, void **out);
int sbh_host_free(void *p);

/* Header.make (bgzf/.../block/Header.scala:48-83): host-side parse of 18 bytes. */
int sbh_header_make(const uint8_t *bytes, uint64_t avail, int32_t *hsize, int32_t *csize);

/* ---- shards: compressed bytes [file_offset, file_offset + n) resident in HBM ----
 * comp may be a host or a device pointer (comp_on_device); the shard keeps a copy
 * (device pointers are copied device-to-device).  file_size locates EOF: when
 * file_offset + n == file_size the resident bytes end at EOF, otherwise the end is
 * "open" and results that would need later bytes report SBH_E_NEED_HALO. */
int sbh_shard_create(sbh_ctx *ctx, const void *comp, uint64_t n, uint64_t file_offset,
                     uint64_t file_size, int comp_on_device, sbh_shard **out);
int sbh_shard_destroy(sbh_shard *sh);
/* Replace a shard's resident bytes with [file_offset, file_offset + n) of the same file (same
 * file_size), keeping its device allocations (grow-only): a window sliding along a file
 * (jni/Native.scala GpuWindow, sbh_check_stream) reuses one shard instead of allocating per
 * window.  Index, inflate and checker state are reset, and the last records scan with everything
 * derived from it (see "What a shard remembers" at sbh_index); the contig lengths are kept.  No
 * result of a later call depends on what the buffers held for the bytes before. */
int sbh_shard_load(sbh_shard *sh, const void *comp, uint64_t n, uint64_t file_offset, int comp_on_device);
/* Device pointer of the resident compressed bytes (padded). */
const void *sbh_shard_comp_device_ptr(sbh_shard *sh);

/* FindBlockStart.apply(path, start, in, bgzfBlocksToCheck) (FindBlockStart.scala:8-36):
 * smallest file offset >= start where bgzf_blocks_to_check consecutive headers parse. */
int sbh_find_block_start(sbh_shard *sh, uint64_t start, int32_t bgzf_blocks_to_check,
                         uint64_t *out);

/* MetadataStream from `start` (MetadataStream.scala:16-58) over the resident bytes:
 * builds the device block table (the chain of blocks from start, empty blocks
 * included and flagged) and the flat layout.  start must be a block start.
 *
 * What a shard remembers, and what forgets it.  A shard keeps the results of its stages on the
 * device so that the next stage can use them; each event below voids what was derived from the
 * state it replaces, and a call that needs a voided result returns SBH_E_STATE -- never a value
 * computed from the old bytes or the old flat offsets:
 *   sbh_shard_load, sbh_index, sbh_run_shard (which indexes; sbh_split_records and the batch run
 *     it): every flat offset is rebased, so the inflated bytes, the eager bitmap and the chain
 *     proof are void, and so are the last records scan (sbh_records_scan, _scan_regions,
 *     sbh_split_records*) and everything derived from it: its columns, the SAM text, the BAM
 *     stream, the FASTQ text, and the BAI scan.  sbh_index voids them even when it is given the
 *     start it was given before, and even when it then fails.
 *   sbh_inflate again: the same bytes at the same offsets; the scan and what was derived from it
 *     stay valid, the eager bitmap and the chain proof are void.
 *   sbh_set_contigs (the same lengths or others): the eager bitmap, the chain proof and the BAI
 *     scan are void; the records scan, the SAM text, the BAM stream and the FASTQ text stay valid.
 *   a new records scan: the SAM text, the BAM stream and the FASTQ text are void (the BAI scan,
 *     which walks a range of its own, is not); a records scan that fails leaves no valid scan.
 *   a stage call refused for its arguments (SBH_E_ARG: a bad record filter) voids nothing: the
 *     stage's last good result is still there.
 * The accumulators (sbh_depth, sbh_pileup, sbh_tally, sbh_stats) belong to the context, not to a shard: none
 * of these events touches what they hold, and an add that returns SBH_E_STATE adds nothing. */
int sbh_index(sbh_shard *sh, uint64_t start, uint64_t *n_blocks, uint64_t *flat_size);
int sbh_get_blocks(sbh_shard *sh, uint64_t first, uint64_t count, sbh_block *out);

/* StreamI._advance's Inflater(nowrap=true).inflate (Stream.scala:31-71) for every
 * indexed block: the shard's flat uncompressed buffer in HBM.  Fails with the first
 * block error in file order (SBH_E_INFLATE_SIZE / _DATA / _BAD_ISIZE, *bad_block). */
int sbh_inflate(sbh_shard *sh, uint64_t *bad_block);

/* CRC32 of every inflated block's bytes against its BGZF footer (the reference reads only
 * ISIZE, Stream.scala:47-54; SURVEY 8d asks for CRC32 as the in-run correctness check).
 * *n_bad = blocks whose CRC differs; *first_bad (optional) = the first one's file offset. */
int sbh_verify_crc(sbh_shard *sh, uint64_t *n_bad, uint64_t *first_bad);
/* Diagnostic (tests, performance triage; not part of the reference's interface): which decoder
 * produced each of blocks [first, first + count), one byte per block in out.  Valid after
 * sbh_inflate / sbh_run_shard (SBH_E_STATE otherwise).  The inflate path records nothing for it:
 * the call runs the shard's Huffman stage again (not the LZ77 stage: the flat bytes stay as they
 * are) and reads off which blocks the lane-parallel decoder hands on, so it costs about half an
 * inflate.  Empty blocks and blocks below the lane-parallel decoder's size limit report
 * SBH_PATH_SERIAL.  The block table (sbh_get_blocks) is unchanged by it. */
#define SBH_PATH_PARALLEL 0 /* the lane-parallel Huffman decoder (with or without its tail kernel) */
#define SBH_PATH_STORED 1   /* the payload is one stored deflate block: copied */
#define SBH_PATH_SERIAL 2   /* the exact serial decoder */
int sbh_inflate_paths(sbh_shard *sh, uint64_t first, uint64_t count, uint8_t *out);
/* Copy flat bytes [flat, flat + n) to host memory. */
int sbh_read_flat(sbh_shard *sh, uint64_t flat, uint64_t n, uint8_t *out);
/* Device pointer of the flat bytes (read-only: the library keeps the zero pad past the flat
 * end between calls and does not re-zero it when the size is unchanged). */
const void *sbh_flat_device_ptr(sbh_shard *sh);

/* Pos <-> flat (canonical positions, Pos.scala; curPos rolls to the next block). */
int sbh_flat_of(sbh_shard *sh, uint64_t block_pos, uint32_t offset, uint64_t *flat);
int sbh_pos_of(sbh_shard *sh, uint64_t flat, uint64_t *block_pos, uint32_t *offset);
/* Flat offset of the first block whose file offset is >= file_off (the flat image
 * of Pos(file_off, 0) as an exclusive bound). */
int sbh_flat_bound(sbh_shard *sh, uint64_t file_off, uint64_t *flat);

/* Contig lengths (BAM header n_ref x l_ref; check/.../header/Header.scala:37-53). */
int sbh_set_contigs(sbh_shard *sh, const int32_t *lens, int32_t n);

/* eager.Checker.apply at every flat position of [begin, end)
 * (check/.../eager/Checker.scala:24-126).  The bitmap stays on the device (used by
 * find_record_start / count_records); out_bits (optional, (end-begin+7)/8 bytes,
 * bit i = position begin+i, LSB first) receives a copy. */
int sbh_check_eager(sbh_shard *sh, uint64_t begin, uint64_t end, int32_t reads_to_check,
                    uint8_t *out_bits, uint64_t *n_true);

/* Copy [begin, end) of the eager bitmap the last sbh_check_eager / sbh_run_shard left on
 * the device (the batch behind Checker.apply(pos) answers).  begin must lie in the
 * bitmap's range at a multiple of 8 positions from its start; SBH_E_STATE if there is
 * no bitmap. */
int sbh_eager_bits(sbh_shard *sh, uint64_t begin, uint64_t end, uint8_t *out_bits);

/* full.Checker.apply at every flat position of [begin, end)
 * (check/.../full/Checker.scala:22-184) with the FullCheck aggregation
 * (cli/.../check/full/FullCheck.scala:142-192).  Optional outputs: out_words
 * (end-begin words), counts (21*19), rbe_hist (21*64), close-call positions
 * (numNonZeroFields <= 2) as (flat, word) pairs up to close_cap. */
int sbh_check_full(sbh_shard *sh, uint64_t begin, uint64_t end, int32_t reads_to_check,
                   uint32_t *out_words, uint64_t *counts, uint64_t *rbe_hist,
                   uint64_t *n_success, uint64_t *close_flat, uint32_t *close_word,
                   uint64_t close_cap, uint64_t *n_close);

/* FindRecordStart.withDelta (check/.../spark/FindRecordStart.scala:30-63) from flat
 * position from_flat: first eager-true position within max_read_size positions of
 * the stream. */
int sbh_find_record_start(sbh_shard *sh, uint64_t from_flat, int32_t reads_to_check,
                          int32_t max_read_size, uint64_t *out_flat, int32_t *out_delta);

/* Record chain from first_flat (PosStream.scala:14-22): number of records whose
 * start is < end_flat (RecordStream.takeWhile(pos < Pos(end, 0)),
 * CanLoadBam.scala:350-355).  Uses the eager bitmap when it covers the range and
 * the chain verifies against it; otherwise an exact sequential walk. */
int sbh_count_records(sbh_shard *sh, uint64_t first_flat, uint64_t end_flat,
                      uint64_t *count);

/* One Hadoop split of loadReadsAndPositions / loadSplitsAndReads
 * (load/.../CanLoadBam.scala:316-356): FindBlockStart(start) -> FindRecordStart ->
 * records while vpos < Pos(end, 0).  first_vpos = htsjdk virtual offset of the
 * first record (valid when *count > 0). */
int sbh_split(sbh_shard *sh, uint64_t start, uint64_t end, int32_t bgzf_blocks_to_check,
              int32_t reads_to_check, int32_t max_read_size, uint64_t *first_vpos,
              uint64_t *count);

/* The record chain from first_flat (PosStream.scala:14-22) as sbh_count_records, plus its
 * exit: the first chain record at/after end_flat (or the stream end).  The multi-GPU stitch
 * re-walks a shard from its upstream neighbour's exit with this. */
int sbh_chain_from(sbh_shard *sh, uint64_t first_flat, uint64_t end_flat, uint64_t *count,
                   uint64_t *exit_flat);

/* Every split of loadSplitsAndReads at once (CanLoadBam.scala:283-297, 316-356): for split
 * i = [starts[i], ends[i]) (file offsets) the same (status[i], first_vpos[i], counts[i]) as
 * sbh_split.  FindBlockStart + FindRecordStart of all splits run in one launch over the
 * eager bitmap, the record chain is proven once over their union, and every count is one
 * more launch; a split off that path (a failed or halo-crossing search, an empty block, a
 * record start outside the bitmap, a start that is a false positive) is decided by
 * sbh_split.  *n_host (optional) = how many were.  Returns SBH_OK unless the batch itself
 * failed; per-split errors are in status[]. */
int sbh_split_starts(sbh_shard *sh, const uint64_t *starts, const uint64_t *ends, uint64_t n,
                     int32_t bgzf_blocks_to_check, int32_t reads_to_check, int32_t max_read_size,
                     uint64_t *first_vpos, uint64_t *counts, int32_t *status, uint64_t *n_host);

/* check-bam -s's comparison of the eager checker with the `.records` truth
 * (cli/.../CheckerApp.scala:65-227, CheckBam.scala) on the device, over the flat ranges
 * [range_begin[r], range_end[r]) (sorted, disjoint): rec_vpos[] are the truth records as
 * htsjdk virtual positions (the `.records` lines, any order).  out[0..3] = true positives,
 * false positives, false negatives, truth records whose block is not in the shard.  fp_flat /
 * fn_flat (optional) receive up to fp_cap / fn_cap mismatching flat positions, sorted (all of
 * them when out[1] <= fp_cap, resp. out[2] <= fn_cap; past the cap an arbitrary subset, not
 * the first ones by position). */
int sbh_check_records(sbh_shard *sh, const uint64_t *range_begin, const uint64_t *range_end,
                      uint64_t n_ranges, int32_t reads_to_check, const uint64_t *rec_vpos,
                      uint64_t n_rec, uint64_t *out, uint64_t *fp_flat, uint64_t fp_cap,
                      uint64_t *fn_flat, uint64_t fn_cap);

/* The whole per-shard hot path as one call (the benchmark step): index from
 * index_start, inflate, eager check at every position of the owned flat range
 * [flat(own_begin_file), flat_bound(own_end_file)), then the owned split:
 * first record >= Pos(own_begin_block, 0) and the record count while
 * vpos < Pos(own_end_file, 0).  All device work is enqueued on the context stream;
 * results are read back at the end. */
typedef struct {
  uint64_t n_blocks;
  uint64_t comp_bytes;   /* compressed bytes of the owned blocks              */
  uint64_t flat_bytes;   /* uncompressed bytes of the owned blocks (positions) */
  uint64_t n_true;       /* eager-true positions in the owned range           */
  uint64_t first_vpos;   /* first record of the owned split (if count > 0)    */
  uint64_t count;        /* records of the owned split                        */
  uint64_t exit_flat;    /* first chain record at/after the owned end         */
  int32_t status;
  int32_t anomalies;     /* chain/bitmap disagreements resolved by the walk   */
} sbh_shard_result;

/* (The run indexes the shard from index_start: like sbh_index it invalidates the last records scan
 * and everything derived from it -- see "What a shard remembers" at sbh_index.) */
int sbh_run_shard(sbh_shard *sh, uint64_t index_start, uint64_t own_end_file,
                  int32_t reads_to_check, int32_t max_read_size, sbh_shard_result *res);

/* Device time (ms, HIP events) of the stages of the last sbh_run_shard: [0] index,
 * [1] inflate + eager check (one pipeline over block batches on three streams),
 * [2] k_eager, [3] record split/count, [4] k_huff, [5] k_lz -- [2], [4], [5] summed
 * over the pipeline's launches, each timed on its own stream.  Returns the number of
 * stages written (<= cap, at most 6). */
int sbh_stage_times(sbh_shard *sh, double *ms, int32_t cap);

/* ---- a shard streamed through bounded HBM ----
 * sbh_run_shard over host-resident compressed bytes [file_offset, file_offset + n) (pinned
 * memory lets the copies overlap the kernels), in windows of about `window` compressed bytes:
 * window w owns the blocks starting in [lo_w, hi_w), loads [lo_w, hi_w + halo), and its
 * successor's bytes are copied host -> HBM on a second stream while it runs, so HBM holds two
 * windows' compressed bytes and one window's working set however large the shard
 * (Stream.scala:80-122 / SplitRDD.scala:33-52 bound the reference per split).  index_start is
 * the owned range's first block (UINT64_MAX: FindBlockStart(file_offset, 5)).  Windows stitch
 * like ranks (a mismatch re-walks the later window from the earlier exit); a window
 * that needs bytes past its halo grows the halo x4 and runs again.  out_bits (optional, host,
 * zeroed by the caller, out_bits_cap bytes): the eager bit of every owned flat position. */
typedef struct {
  uint64_t n_windows, n_blocks;
  uint64_t comp_bytes;  /* compressed bytes of the owned blocks                      */
  uint64_t flat_bytes;  /* their uncompressed bytes (checked positions)              */
  uint64_t n_true;      /* eager-true owned positions                                */
  uint64_t count;       /* records of the owned range (the stitched chain)           */
  uint64_t first_vpos;  /* first record (UINT64_MAX if none)                         */
  uint64_t exit_vpos;   /* first chain record at/after the owned end (UINT64_MAX: none) */
  int32_t status, rewalks, host_pinned, pad;
  double ms_wall;       /* wall time of the call (host clock), copies included       */
  double ms_h2d;        /* summed host -> HBM copy time (HIP events on the copy stream) */
  double stage_ms[6];   /* sbh_stage_times summed over the windows                   */
  uint64_t halo_final;
  /* sbh_run_stream2 only (zero otherwise): */
  uint64_t crc_bad_blocks;  /* owned blocks whose BGZF footer CRC32 differs (opts.verify_crc) */
  uint64_t crc_first_bad;   /* file offset of the first such block                   */
  uint64_t splits_host;     /* splits decided by the exact per-split path (sbh_split)  */
  double ms_splits;         /* device + host time of the per-split work, summed       */
  double ms_crc;            /* CRC32 kernel time, summed over the windows              */
} sbh_stream_result;
int sbh_run_stream(sbh_ctx *ctx, const void *host_comp, uint64_t n, uint64_t file_offset,
                   uint64_t file_size, uint64_t index_start, uint64_t own_end_file, uint64_t window,
                   uint64_t halo, const int32_t *contig_len, int32_t n_contigs, int32_t reads_to_check,
                   int32_t max_read_size, uint8_t *out_bits, uint64_t out_bits_cap,
                   sbh_stream_result *res);

/* sbh_run_stream with per-split results and an in-run CRC check: loadSplitsAndReads' per-split
 * answer for a shard larger than HBM (CanLoadBam.scala:283-297,316-356 over SplitRDD.scala:
 * 33-52's partitions).  When n_splits > 0, split i = [split_start[i], split_end[i]) (file
 * offsets, sorted, split_start[i] < split_end[i] <= split_start[i + 1], every start in
 * [file_offset, own_end_file), the last end <= own_end_file): windows are cut at split starts,
 * so every split lies in one window, and each window's splits get sbh_split_starts' (status,
 * first_vpos, count) -- exactly what sbh_split returns for them on the whole file.
 * verify_crc: every owned block's inflated bytes against its footer CRC32 (crc_bad_blocks). */
typedef struct {
  uint64_t window, halo;
  int32_t reads_to_check, max_read_size, bgzf_blocks_to_check, verify_crc;
  const uint64_t *split_start, *split_end; /* n_splits entries, or NULL with n_splits = 0 */
  uint64_t n_splits;
  uint64_t *split_first_vpos, *split_count; /* out, n_splits entries                      */
  int32_t *split_status;                   /* out: SBH_OK or the split's SBH_E_* status */
  uint8_t *out_bits;
  uint64_t out_bits_cap;
} sbh_stream_opts;
int sbh_run_stream2(sbh_ctx *ctx, const void *host_comp, uint64_t n, uint64_t file_offset,
                    uint64_t file_size, uint64_t index_start, uint64_t own_end_file,
                    const int32_t *contig_len, int32_t n_contigs, const sbh_stream_opts *opts,
                    sbh_stream_result *res);

/* ---- the all-positions modes over a file of any size ----
 * Blocks.apply (check/src/main/scala/org/hammerlab/bam/check/Blocks.scala:47-208) picks the
 * BGZF blocks whose every position check-bam / full-check examine; CallPartition
 * (cli/.../CallPartition.scala:23-54) and FullCheck.checkPartition (cli/.../full/FullCheck.scala:
 * 65-86) then call the checkers at every offset of those blocks, reading the chain past them
 * freely.  Both calls below take the whole file in host memory (mapped or pinned) and move it
 * through HBM in windows of about `window` compressed bytes, so HBM use is bounded whatever
 * the file size; a window whose answers need bytes past its halo grows the halo x4 and runs
 * again. */

/* Blocks.apply's branch without a `.blocks` file (Blocks.scala:141-206): for split i =
 * [split_start[i], split_end[i]) (file offsets, ascending), FindBlockStart(split_start[i],
 * bgzf_blocks_to_check) then MetadataStream from there while the block start is < split_end[i]
 * (an empty block ends the stream, MetadataStream.scala:43-45).  Writes (start, csize, usize)
 * of each block into out[] (ustart / hsize / flags zero; ustart = the split index) up to cap
 * entries, in split order; *n_out = how many there are.  A split whose search fails answers
 * SBH_E_HEADER_SEARCH_FAILED (HeaderSearchFailedException) for the whole call. */
int sbh_find_blocks(sbh_ctx *ctx, const void *host_file, uint64_t file_size, const uint64_t *split_start,
                    const uint64_t *split_end, uint64_t n_splits, int32_t bgzf_blocks_to_check, uint64_t window,
                    sbh_block *out, uint64_t cap, uint64_t *n_out);

/* check-bam -s and full-check over the given blocks (file offsets of block starts, ascending --
 * Blocks.apply's partitions concatenated): every uncompressed offset of every listed block is
 * checked.  truth_vpos (optional, ascending htsjdk virtual positions: the `.records` file,
 * CheckerApp.scala:65-227) turns the eager calls into TP / FP / FN with the mismatching
 * positions (first fp_cap / fn_cap of them, as vpos); full != 0 adds full.Checker's FullCheck
 * aggregation (FullCheck.scala:142-192): Counts and readsBeforeError histograms by
 * numNonZeroFields (include/sparkbam.h layout above) and the close calls (<= 2 non-zero
 * fields) as (vpos, word) up to close_cap, ascending. */
typedef struct {
  uint64_t window, halo;
  int32_t reads_to_check, full;
  const uint64_t *blocks;
  uint64_t n_blocks;
  const uint64_t *truth_vpos; /* NULL: no comparison (n_true only) */
  uint64_t n_truth;
  uint64_t *fp_vpos, *fn_vpos;
  uint64_t fp_cap, fn_cap;
  uint64_t *counts;   /* full: 21 * 19 */
  uint64_t *rbe_hist; /* full: 21 * 64 */
  uint64_t *close_vpos;
  uint32_t *close_word;
  uint64_t close_cap;
} sbh_check_opts;
typedef struct {
  uint64_t n_windows, positions, comp_bytes; /* checked positions and their blocks' compressed bytes */
  uint64_t n_true;                           /* eager-true checked positions                      */
  uint64_t tp, fp, fn, unknown;              /* vs truth_vpos (unknown: truth records off the chain) */
  uint64_t n_success, n_close;               /* full                                             */
  uint64_t halo_final;
  double ms_wall, ms_h2d;
} sbh_check_result;
int sbh_check_stream(sbh_ctx *ctx, const void *host_file, uint64_t file_size, const int32_t *contig_len,
                     int32_t n_contigs, const sbh_check_opts *opts, sbh_check_result *res);

/* ---- record field extraction ----
 * RecordStream from first_flat while the record start is < end_flat, decoded like
 * htsjdk BAMRecordCodec.decode (check/.../iterator/RecordStream.scala:16-41,
 * load/.../CanLoadBam.scala:244-264), into columns.  Record starts follow the chain
 * (next = start + 4 + block_size; the verified eager bitmap when it covers the range).
 * sbh_records_scan decodes on the device and reports the sizes; sbh_records_fetch copies
 * the columns of the last scan into caller buffers (any pointer may be NULL). */
typedef struct {
  uint64_t n;           /* records                                              */
  uint64_t name_bytes;  /* read names, each l_read_name bytes with its NUL      */
  uint64_t cigar_ops;   /* CIGAR ops                                            */
  uint64_t bases;       /* sequence letters (= quality bytes)                   */
  uint64_t aux_bytes;   /* raw tag bytes                                        */
} sbh_records_sizes;
typedef struct {
  uint64_t *flat;                                          /* [n] record start (flat) */
  int32_t *ref_id, *pos, *next_ref_id, *next_pos, *tlen;   /* [n] as stored (pos 0-based, -1 unset) */
  uint16_t *flag, *bin;                                    /* [n] */
  uint8_t *mapq;                                           /* [n] */
  uint64_t *name_off, *cigar_off, *seq_off, *aux_off;      /* [n + 1] exclusive prefix offsets */
  char *names;                                             /* [name_bytes] */
  uint32_t *cigar;                                         /* [cigar_ops] op_len << 4 | op */
  char *seq;                                               /* [bases] "=ACMGRSVTWYHKDBN" letters */
  uint8_t *qual;                                           /* [bases] phred (0xff: absent) */
  uint8_t *aux;                                            /* [aux_bytes] tags as stored */
  uint64_t *vpos;                                          /* [n] record start as an htsjdk virtual
                                                              position (canonical Pos, Pos.scala:12-43);
                                                              available after sbh_split_records too */
} sbh_records_out;
/* A scan is valid until the next scan, sbh_shard_load, sbh_index or sbh_run_shard; a scan that fails
 * leaves none.  The fetch and every stage over "the rows of the last scan" return SBH_E_STATE without
 * a valid one (see "What a shard remembers" at sbh_index). */
int sbh_records_scan(sbh_shard *sh, uint64_t first_flat, uint64_t end_flat, sbh_records_sizes *out);
int sbh_records_fetch(sbh_shard *sh, const sbh_records_out *out);

/* One Hadoop FileSplit [start, end) of loadReadsAndPositions in ONE call (load/.../CanLoadBam.scala:
 * 316-356, the body of its fileSplitsRDD.flatMap): FindBlockStart(start, bgzf_blocks_to_check)
 * (FindBlockStart.scala:8-36), MetadataStream + inflate from that block, the eager check at every
 * position of [Pos(blockStart, 0), Pos(end, 0)), FindRecordStart from Pos(blockStart, 0)
 * (FindRecordStart.scala:11-30), and the records from it while pos < Pos(end, 0) (RecordStream.
 * takeWhile): their starts, and with decode != 0 BAMRecordCodec.decode's columns, for
 * sbh_records_fetch (decode == 0: only its `flat` column may be asked for).  The shard must hold
 * the split's bytes from `start` plus a halo (sbh_shard_load reuses one shard for every split a
 * thread runs).  Errors: SBH_E_HEADER_SEARCH_FAILED {start, positionsAttempted};
 * SBH_E_NO_READ_FOUND {blockStart, maxReadSize} (NoReadFoundException(path, blockStart,
 * maxReadSize)); SBH_E_NEED_HALO when an answer needs bytes past the resident range (reload with
 * a larger halo) -- a last record running past the halo included. */
typedef struct {
  uint64_t block_start;     /* FindBlockStart(start)                                        */
  uint64_t n_blocks;        /* blocks indexed from it (sbh_get_blocks), halo included        */
  uint64_t flat_size;       /* their uncompressed bytes                                      */
  uint64_t owned_flat;      /* flat image of Pos(end, 0): the split's positions [0, owned)   */
  uint64_t first_flat;      /* FindRecordStart(Pos(blockStart, 0)) (may be >= owned_flat)    */
  uint64_t first_vpos;      /* its htsjdk virtual position (when sizes.n > 0)                */
  uint64_t n_true;          /* eager-true positions of [0, owned_flat)                       */
  sbh_records_sizes sizes;  /* sizes.n = the split's records; column sizes when decoded      */
} sbh_split_records_result;
int sbh_split_records(sbh_shard *sh, uint64_t start, uint64_t end, int32_t bgzf_blocks_to_check,
                      int32_t reads_to_check, int32_t max_read_size, int32_t decode,
                      sbh_split_records_result *out);

/* Many FileSplits of loadReadsAndPositions in ONE call: split i = [starts[i], ends[i]) (file
 * offsets, ascending, starts[i] < ends[i] <= starts[i + 1], starts[0] inside the shard; anything
 * else is SBH_E_ARG), a Spark executor's concurrent tasks (or a prefetch of the next K splits)
 * served by one pass over their bytes instead of one pass each.  FindBlockStart(starts[0]), then
 * index + inflate + eager check + chain proof once from that block to Pos(ends[n - 1], 0)
 * (sbh_run_shard), every split's FindBlockStart / FindRecordStart / count as sbh_split_starts, the
 * record starts of all splits in one launch set whose launch count does not grow with n, and one
 * decode over all of them.  Every split answers what sbh_split_records answers for it alone on a
 * shard loaded from starts[i] to the same resident end: (status, block_start, first_vpos,
 * rec_count) and the records.  status is per split -- SBH_OK (rec_count may be 0: an empty
 * split), SBH_E_NO_READ_FOUND {block_start, maxReadSize}, SBH_E_HEADER_SEARCH_FAILED {starts[i],
 * 65536}, SBH_E_NEED_HALO when that split's answer needs bytes past an open shard end -- and the
 * splits with status SBH_OK have their records whatever the others answer.  The call itself fails
 * when the shared pass fails (inflate errors), with SBH_E_BAD_RECORD when a record of the batch is
 * malformed, and with SBH_E_NEED_HALO when the last record of the batch runs past an open shard
 * end (decode == 0 checks that too, so both modes answer the same statuses).
 * Afterwards sbh_records_fetch serves the batch's columns (vpos included; decode == 0: `flat`
 * and `vpos` only): the splits' records in split order, split i owning rows [rec_begin,
 * rec_begin + rec_count); `flat` offsets are the batch's (flat 0 = Pos(out->block_start, 0)), as
 * are first_flat / owned_flat.  host_path: the split was decided by sbh_split's exact path (an
 * empty block in the way, a search leaving the bitmap); its record starts are walked along the
 * chain into its rows.  out->n_host counts them. */
typedef struct {
  uint64_t block_start;  /* FindBlockStart(starts[i]) (status SBH_OK / SBH_E_NO_READ_FOUND)      */
  uint64_t first_flat;   /* first record (batch flat; when rec_count > 0)                        */
  uint64_t first_vpos;   /* its htsjdk virtual position (when rec_count > 0)                     */
  uint64_t owned_flat;   /* flat image of Pos(ends[i], 0)                                        */
  uint64_t rec_begin, rec_count; /* rows [rec_begin, rec_begin + rec_count) of the batch's columns */
  int32_t status, host_path;
} sbh_batch_split;
typedef struct {
  uint64_t block_start;     /* FindBlockStart of the first split that has one: flat 0            */
  uint64_t n_blocks;        /* blocks indexed from it                                           */
  uint64_t flat_size;       /* their uncompressed bytes                                         */
  uint64_t n_true;          /* eager-true positions below Pos(ends[n - 1], 0)                   */
  uint64_t n_host;          /* splits with host_path = 1                                        */
  sbh_records_sizes sizes;  /* sizes.n = records of all splits; column sizes when decoded       */
} sbh_split_batch_result;
int sbh_split_records_batch(sbh_shard *sh, const uint64_t *starts, const uint64_t *ends, uint64_t n,
                            int32_t bgzf_blocks_to_check, int32_t reads_to_check, int32_t max_read_size,
                            int32_t decode, sbh_batch_split *splits, sbh_split_batch_result *out);

/* ---- loadBamIntervals ----
 * CanLoadBam.loadBamIntervals (load/.../CanLoadBam.scala:78-154) after the host has turned
 * the intervals into BAI chunks (getIntevalChunks, :410-444; Index.scala:11-93): for each
 * chunk [chunk_begin[c], chunk_end[c]) (flat positions of the chunk's start/end Pos), the
 * records from the chunk start while the start is < the chunk end, in chunk order, kept
 * when region(record) (:446-454) overlaps one of the intervals: (iv_ref[k], [iv_begin[k],
 * iv_end[k])) 0-based half-open, sorted by (ref, begin) and disjoint (a merged LociSet).
 * Leaves the kept records' columns for sbh_records_fetch, like sbh_records_scan. */
int sbh_records_scan_regions(sbh_shard *sh, const uint64_t *chunk_begin, const uint64_t *chunk_end,
                             uint64_t n_chunks, const int32_t *iv_ref, const int64_t *iv_begin,
                             const int64_t *iv_end, uint32_t n_iv, sbh_records_sizes *out);

/* ---- BAI index construction ------------------------------------------------------------
 * What samtools index / htslib writes for a coordinate-sorted BAM, built from the records that
 * are already resident.  sbh_bai_scan restates hts_idx_push (htslib hts.c) for every record of
 * the chain from first_flat while the start is < end_flat (the range of sbh_records_scan), on
 * the device:
 *  - a record with ref_id < 0 only counts into n_no_coor;
 *  - otherwise beg = pos, end = pos + (sum of the M D N = X op lengths) when flag 0x4 is clear
 *    and that sum is > 0, else pos + 1; bin = hts_reg2bin(beg, end, 14, 5), computed (the stored
 *    bin field is ignored, as htslib ignores it); the record counts as unmapped for its reference
 *    when flag 0x4 is set;
 *  - a RUN is a maximal stretch of consecutive records with one (ref_id, bin): the chunk [vbeg of
 *    its first record, vend of its last) that hts_idx_push appends to the bin, where a record's
 *    vend is the next record's vbeg and, for the last record of the scan, the virtual offset
 *    bgzf_tell reports after it (at the end of the last non-empty block: the next member's
 *    address, offset 0);
 *  - the linear index (insert_to_l) holds, per 16 KiB window [beg >> 14, (end - 1) >> 14], the
 *    smallest vbeg of the records touching it: lin is one array over all references, reference
 *    r owning (l_ref >> 14) + 2 slots from the sum of the earlier references' counts, UINT64_MAX
 *    where no record touched; a window past a reference's last slot is clamped to it.
 * Errors: SBH_E_UNSORTED {virtual offset of the first offending record} when ref_id decreases,
 * pos decreases within a reference, or a record with a reference follows one without;
 * SBH_E_BAD_RECORD when ref_id >= n_ref, pos < 0 on a reference, or a record does not fit the
 * stream (for a record that does not fit, SBH_E_NEED_HALO instead when the shard's end is open:
 * more resident bytes may cure that, and only that).  Needs sbh_set_contigs.
 * The runs and the linear-index minima stay on the device for sbh_bai_fetch.
 *
 * Windows.  A file larger than HBM is scanned window by window (sbh_shard_load), each window
 * cut at a record boundary: the caller concatenates the windows' runs in file order, takes the
 * element-wise minimum of their lin arrays, adds their n_no_coor, and hands the whole to one
 * sbh_bai_build, which coalesces the run a seam cut in two.  The ordering check across a seam
 * is split: sbh_bai_build refuses a ref_id that decreases between consecutive runs, and the
 * caller compares sbh_bai_edges of the two windows -- the later window's first record against the
 * earlier window's last record with a reference (pos within one reference; any record with a
 * reference after a window that counted n_no_coor > 0). */
typedef struct {
  int32_t ref_id;
  uint32_t bin;
  uint64_t vbeg, vend, n_mapped, n_unmapped;
} sbh_bai_run;
typedef struct {
  uint64_t n_records, n_runs, n_no_coor, lin_size;
} sbh_bai_sizes;
/* The scan's result (sbh_bai_fetch, sbh_bai_edges) is valid until the next sbh_bai_scan,
 * sbh_set_contigs, sbh_shard_load, sbh_index or sbh_run_shard; SBH_E_STATE after any of them.  A
 * records scan does not touch it. */
int sbh_bai_scan(sbh_shard *sh, uint64_t first_flat, uint64_t end_flat, sbh_bai_sizes *out);
/* runs: n_runs entries; lin: lin_size entries (either may be NULL). */
int sbh_bai_fetch(sbh_shard *sh, sbh_bai_run *runs, uint64_t *lin);
/* (ref_id, pos) of the last scan's first record and of its last record with a reference;
 * ref_id -1 when the first record has none, resp. when no record has one. */
int sbh_bai_edges(sbh_shard *sh, int32_t *first_ref, int32_t *first_pos, int32_t *last_ref, int32_t *last_pos);

/* hts_idx_finish + the BAI writer (hts_idx_save), HOST ONLY: no context, works without a GPU,
 * like sbh_header_make.  runs may be the concatenation, in file order, of several scans' runs
 * (adjacent runs with equal (ref_id, bin) are coalesced first), lin their element-wise minimum.
 * Per reference: the metadata pseudo-bin 37450 {(vbeg of its first record, vend of its last),
 * (n_mapped, n_unmapped)}; compress_binning -- for level 5 .. 1, every bin of the level (its
 * chunks sorted first below level 5) whose chunks span fewer than 0x10000 block addresses is
 * appended to its parent (bin - 1) >> 3 and deleted, then bin 0 is sorted, then in every bin a
 * chunk starting in or before the block where the kept one ends is merged into it; the linear
 * index up to its last touched window, an untouched window taking the next touched one's value
 * (htslib's backward fill).  Layout: "BAI\1", n_ref, per reference its bins and intervals, then
 * n_no_coor; a reference without records writes n_bin = 0, n_intv = 0.
 * Deliberate deviation: bins are written in ascending bin id with 37450 last, where htslib writes
 * its hash table's order; readers do not depend on the order, so the parsed index equals
 * htslib's while the bytes need not.
 * SBH_E_ARG when cap < the size needed (*size is set to it; sbh_bai_bound(...) always suffices),
 * when two adjacent runs with equal (ref_id, bin) do not meet (the earlier vend != the later
 * vbeg: windows concatenated with a gap or an overlap) or when a bin id is >= 37450;
 * SBH_E_UNSORTED when ref_id decreases between runs, SBH_E_BAD_RECORD for a ref_id outside
 * [0, n_ref). */
uint64_t sbh_bai_bound(uint64_t n_runs, uint64_t lin_size, int32_t n_ref);
int sbh_bai_build(const sbh_bai_run *runs, uint64_t n_runs, const uint64_t *lin, const int32_t *contig_len,
                  int32_t n_ref, uint64_t n_no_coor, uint8_t *out, uint64_t cap, uint64_t *size);

/* ---- SAM text ----------------------------------------------------------------------------
 * The records of the last decoded scan as SAM text, one line per record ending in '\n', rendered
 * on the device: what htsjdk SAMRecord.getSAMString prints (the reference's .sam fixtures under test_bams).
 * Eleven tab-separated fields -- QNAME (the name bytes up to the first NUL), FLAG, RNAME (the
 * name of 0 <= ref_id < n_ref, else "*"), POS (pos + 1), MAPQ, CIGAR ("*" for no ops), RNEXT ("*"
 * for next_ref_id < 0, "=" for next_ref_id == ref_id, the name below n_ref, else "*"), PNEXT, TLEN,
 * SEQ ("*" for l_seq == 0), QUAL ("*" for l_seq == 0 or a first quality byte 0xFF, else byte + 33)
 * -- then "\tTG:T:VALUE" per tag: A the byte, c C s S i I ":i:" and the decimal value, Z / H the
 * bytes up to the NUL, B ":B:<sub>" and ",<value>" per element, f and B:f Java's Float.toString
 * (csrc/sam_core.h holds the definition for device and host).
 * rows = the rows of the last decoded scan on this shard (sbh_records_scan,
 * sbh_records_scan_regions, sbh_split_records / sbh_split_records_batch with decode != 0), in their
 * order: after a batch, split i's text is text[line_off[rec_begin] .. line_off[rec_begin +
 * rec_count]).  ref_names packed, name k = ref_names[ref_name_off[k] .. ref_name_off[k + 1]).
 * sbh_records_sam_scan renders into device memory and reports the sizes; sbh_records_sam_fetch
 * copies the text (text_bytes bytes, no terminator) and the lines' prefix offsets out (either
 * pointer may be NULL).  n_host = rows holding an f or B:f tag: their lines are rendered on the
 * host inside the library (Float.toString needs strtof) and land in the text with the fetch.
 * Errors: SBH_E_STATE without a valid decoded scan (none yet, or the last was decode == 0);
 * SBH_E_BAD_RECORD {row} for the first row whose CIGAR has an op code above 8 (htsjdk throws) or
 * whose tag area is malformed: an unknown type or B sub-type byte, a value running past the
 * record's tag bytes, a Z / H without a NUL inside them, a negative B count, 1 or 2 bytes left
 * after the last tag.  n == 0 gives text_bytes = 0 and line_off = [0].
 * A new scan, sbh_shard_load, sbh_index or sbh_run_shard invalidates the text (the fetch then
 * returns SBH_E_STATE); sbh_inflate and sbh_set_contigs do not. */
typedef struct { uint64_t n, text_bytes, n_host; } sbh_sam_sizes;
int sbh_records_sam_scan(sbh_shard *sh, const char *ref_names, const uint64_t *ref_name_off,
                         int32_t n_ref, sbh_sam_sizes *out);
int sbh_records_sam_fetch(sbh_shard *sh, char *text /* [text_bytes] */, uint64_t *line_off /* [n+1] */);
/* HOST ONLY, no context, no GPU (like sbh_bai_build): the same text for the records at starts[]
 * of a flat BAM stream.  line_off (n + 1 entries) is always filled; text == NULL: sizes only.
 * SBH_E_BAD_RECORD with *bad_row = the first row that does not fit the stream or its block_size
 * (as sbh_records_scan judges) or is malformed as above; SBH_E_ARG when text_cap < line_off[n]. */
int sbh_sam_render_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                        const char *ref_names, const uint64_t *ref_name_off, int32_t n_ref,
                        char *text, uint64_t text_cap, uint64_t *line_off, uint64_t *bad_row);

/* ---- BAM stream ---------------------------------------------------------------------------
 * Selected records of the last scan as one uncompressed BAM stream in device memory: `head`, then
 * the kept records' raw bytes [p, p + 4 + block_size) in row order, unchanged (bin is not
 * recomputed, nothing is re-encoded) -- what sbh_bgzf_compress_level(..., src_on_device = 1, ...)
 * turns into a BAM file and sbh_bai_scan of that file indexes, without the records leaving HBM.
 * rows = the rows of the last valid scan on this shard (sbh_records_scan, sbh_records_scan_regions,
 * sbh_split_records, sbh_split_records_batch), in their order; decode == 0 is enough (only the
 * record starts and the flat bytes are read).  Rows need not be ascending or distinct in the flat
 * stream: a record that overlapping BAI chunks deliver twice is written twice.
 * A row is kept when (flag & flag_require) == flag_require, (flag & flag_exclude) == 0,
 * mapq >= min_mapq and its index lies in one of the row ranges (csrc/bam_gather_core.h holds the
 * definition for device and host).  Every row, kept or not, is validated as sbh_records_scan
 * judges it: its 36 fixed bytes inside the stream, l_seq >= 0, block_size >= 32 + l_read_name +
 * 4 n_cigar + (l_seq + 1) / 2 + l_seq, its end inside the stream.
 * head: host memory copied to the front of the stream (the BAM header bytes, or the unfinished
 * tail of an earlier window's stream when a file is written window by window: BGZF members are
 * cut every 65498 bytes of the whole stream); rec_off[0] == head_bytes.
 * The call leaves the scan's rows, columns and SAM text as they are; a new scan, sbh_shard_load,
 * sbh_index or sbh_run_shard invalidates the BAM stream (and the scan it was built from: the next
 * sbh_records_bam_scan returns SBH_E_STATE until there is a new scan); a call refused with SBH_E_ARG
 * leaves the last stream in place.  It synchronises the shard's stream before it returns, so the
 * context-level compress call may follow directly on sbh_records_bam_device_ptr (NULL without a
 * valid BAM scan).  sbh_records_bam_fetch copies out what is asked for (any pointer may be NULL).
 * Errors: SBH_E_STATE without a valid scan; SBH_E_ARG for a filter outside the ranges below or
 * row ranges that are unsorted, overlapping or empty; SBH_E_BAD_RECORD {row} for the first invalid
 * row -- SBH_E_NEED_HALO instead when that row merely runs past an open shard end (sbh_bai_scan's
 * rule).  n == 0 or n_kept == 0 gives bytes = head_bytes and rec_off = [head_bytes]. */
typedef struct {
  uint32_t flag_require, flag_exclude;   /* both < 65536 */
  int32_t  min_mapq;                     /* 0..255 */
  int32_t  pad;
  const uint64_t *row_begin, *row_end;   /* rows [row_begin[k], row_end[k]) of the last scan: sorted, disjoint,
                                            non-empty; may reach past n (clipped).  n_row_ranges == 0: every row */
  uint64_t n_row_ranges;
} sbh_record_filter;
typedef struct { uint64_t n, n_kept, bytes; } sbh_bam_sizes;   /* bytes = head_bytes + the kept records' bytes */

int sbh_records_bam_scan(sbh_shard *sh, const uint8_t *head, uint64_t head_bytes,
                         const sbh_record_filter *filter /* NULL: keep all */, sbh_bam_sizes *out);
const void *sbh_records_bam_device_ptr(sbh_shard *sh);
int sbh_records_bam_fetch(sbh_shard *sh, uint8_t *stream /*[bytes]*/, uint64_t *rec_off /*[n_kept+1]*/,
                          uint64_t *rows /*[n_kept]: the scan row each kept record came from*/);
/* Bytes [offset, offset + n) of the stream (a window's unfinished tail, without the rest). */
int sbh_records_bam_read(sbh_shard *sh, uint64_t offset, uint64_t n, uint8_t *out);
/* The same stream with the kept rows in a chosen order.  SBH_ORDER_SCAN is sbh_records_bam_scan
 * (which calls this).  SBH_ORDER_COORDINATE: the kept rows in ascending order of
 *   key = (ref_id < 0 ? 0x7fffffff : ref_id) << 33 | (uint32)(pos + 1) << 1 | ((flag >> 4) & 1)
 * -- reference, position, reverse strand: samtools' bam1_cmp_core, unplaced records last -- rows
 * of equal key in scan order (a stable sort on the device; csrc/bam_sort_core.h holds the
 * definition for device and host).  The filter's row ranges index scan rows, and
 * sbh_records_bam_fetch's rows[k] is still the scan row the k-th record of the stream came from:
 * in this order, the permutation.  State, invalidation and errors as sbh_records_bam_scan;
 * SBH_E_ARG for any other order.  sbh_records_bam_sorted: after a coordinate-order scan,
 * *already = 1 when the kept rows were in order as scanned (nothing was moved); SBH_E_STATE
 * without such a scan. */
#define SBH_ORDER_SCAN 0
#define SBH_ORDER_COORDINATE 1
int sbh_records_bam_scan_order(sbh_shard *sh, const uint8_t *head, uint64_t head_bytes,
                               const sbh_record_filter *filter, int order, sbh_bam_sizes *out);
int sbh_records_bam_sorted(sbh_shard *sh, int *already);
/* HOST ONLY, no context, no GPU: perm[k] = the row of starts[] that comes k-th in that order.
 * SBH_E_BAD_RECORD with *bad_row = the first invalid row (sbh_bam_gather_host's validation). */
int sbh_bam_sort_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                      uint64_t *perm /*[n]*/, uint64_t *bad_row);
/* The same stream with the kept rows in read-name order (samtools sort -N): ascending name, then
 * ascending tie, rows equal in both in scan order (a stable sort on the device;
 * csrc/bam_name_core.h holds the definition for device and host).  The name is the
 * l_read_name - 1 bytes behind the fixed fields, compared as unsigned bytes after padding with
 * zeros to 256 bytes -- a prefix comes first; strcmp's order for the names SAM allows.
 *   tie = ((flag >> 6) & 3) << 2 | ((flag >> 11) & 1) << 1 | ((flag >> 8) & 1)
 * -- READ1 / READ2 as samtools compares flag & 0xc0, then primary, secondary, supplementary.  The
 * tie is this library's own and not htsjdk's comparator chain; natural order (sort -n) is not built.
 * State, invalidation, errors and sbh_records_bam_fetch (rows[k] = the scan row of the k-th output
 * record) as sbh_records_bam_scan_order; sbh_records_bam_sorted keeps returning SBH_E_STATE after
 * this call.  sbh_records_bam_name_info: the summary of the last valid BAM scan when that was a
 * name-order one (SBH_E_STATE otherwise): the groups of rows of one name and those of 1, 2 and
 * more rows, the longest name in bytes, the 8-byte chunks and the 8-bit radix passes the sort ran,
 * and already = 1 when the kept rows were in order as scanned (nothing ran, nothing was moved). */
typedef struct { uint64_t n_names, n_single, n_pair, n_more;
                 uint32_t max_name, chunks_run, passes_run; int32_t already; } sbh_bam_name_info;
int sbh_records_bam_scan_names(sbh_shard *sh, const uint8_t *head, uint64_t head_bytes,
                               const sbh_record_filter *filter, sbh_bam_sizes *out);
int sbh_records_bam_name_info(sbh_shard *sh, sbh_bam_name_info *out);
/* HOST ONLY, no context, no GPU: perm[k] = the row of starts[] that comes k-th in name order; info
 * (may be NULL) gets the group counts, max_name and already -- chunks_run and passes_run stay 0.
 * SBH_E_BAD_RECORD with *bad_row = the first invalid row (sbh_bam_gather_host's validation). */
int sbh_bam_name_sort_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                           uint64_t *perm /*[n]*/, sbh_bam_name_info *info /* may be NULL */, uint64_t *bad_row);
/* HOST ONLY: the BAM header bytes head[0, n) (magic, l_text, text, n_ref, references) with the
 * @HD line's SO: set to `so` -- an existing value replaced, "\tSO:<so>" appended to an @HD line
 * without one, "@HD\tVN:1.6\tSO:<so>\n" put in front of a text without @HD.  l_text follows, a
 * NUL-padded text keeps its padding behind the last line, everything else is untouched.  *out_n =
 * the result's size, also when cap is too small (SBH_E_ARG then; out may be NULL with cap 0:
 * at most n + 20 + strlen(so) bytes).  SBH_E_ARG too for bytes that are not a BAM header. */
int sbh_bam_header_set_so(const uint8_t *head, uint64_t n, const char *so, uint8_t *out, uint64_t cap,
                          uint64_t *out_n);
/* HOST ONLY, no context, no GPU (like sbh_sam_render_host): the same stream for the records at
 * starts[] of a flat BAM stream.  rec_off (room for n + 1) and rows (room for n) may be NULL;
 * out == NULL: sizes only (*n_kept, rec_off).  SBH_E_BAD_RECORD with *bad_row = the first invalid
 * row, kept or not; SBH_E_ARG for a bad filter or when out_cap < the stream's bytes. */
int sbh_bam_gather_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                        const uint8_t *head, uint64_t head_bytes, const sbh_record_filter *filter,
                        uint8_t *out, uint64_t out_cap, uint64_t *rec_off, uint64_t *rows,
                        uint64_t *n_kept, uint64_t *bad_row);

/* ---- Per-base depth -----------------------------------------------------------------------
 * How many kept records cover each reference position (samtools depth, bedtools genomecov -bg),
 * computed on the device from the flat bytes and record starts of a scan and accumulated across
 * shards in an sbh_depth, which belongs to a context and outlives the shards added to it
 * (csrc/depth_core.h holds the definition for device and host).
 * Spans: (ref_id, beg, end), 0-based half-open, 0 <= beg < end <= 2^31 - 1, ref_id in [0, n_ref)
 * and strictly ascending.  Span k owns end - beg + 1 int32 slots of one array (the last takes the
 * events that close at `end`); the accumulator costs 4 bytes per slot of HBM (SBH_E_NOMEM).
 * A row is KEPT when the filter passes it (sbh_record_filter; NULL: every row).  A kept row with
 * ref_id < 0 counts into n_unplaced; one whose reference has a span counts into n_counted and each
 * of its CIGAR ops M, =, X -- and D with SBH_DEPTH_DEL -- covers [x, x + len) cut to the span, x
 * starting at pos and advancing over M, D, N, =, X (64-bit arithmetic).  N never covers.  The
 * stored CIGAR field counts: a long read's CIGAR in a CG:B,I tag is not followed.  cov_bases = the
 * bases the add covered.
 * sbh_records_depth_add uses the rows of the last valid scan on the shard, in their order, as
 * sbh_records_bam_scan does (decode == 0 is enough; a row delivered twice counts twice), leaves the
 * scan's rows, columns, SAM text and BAM stream as they are and synchronises the shard's stream
 * before it returns.  Every row is validated as sbh_records_bam_scan validates it; a kept row with
 * an op code above 8 or ref_id >= n_ref is bad too.  SBH_E_BAD_RECORD {row} for the first bad row,
 * SBH_E_NEED_HALO instead when that row merely runs past an open shard end; a failed add leaves
 * the accumulator exactly as it was.  One thread at a time per sbh_depth; a shard of another
 * context gives SBH_E_ARG.
 * sbh_depth_finish: depth[s] = the inclusive prefix sum of the slots, in place.  A run is a
 * maximal stretch of equal depth inside one span (zero-depth runs included; the extra slot belongs
 * to none).  covered = positions of depth >= 1, sum = depth over all positions = every add's
 * cov_bases together.  After it an add or a second finish gives SBH_E_STATE until
 * sbh_depth_reset (zero, open for adds again); before it the fetches give SBH_E_STATE and the
 * device pointer is NULL.  sbh_depth_fetch: depth of positions beg + from .. beg + from + n of a
 * span; sbh_depth_runs_fetch: runs [first, first + count) in span and position order.
 * SBH_E_ARG for spans that are unsorted, share a reference, have beg >= end or a ref_id outside
 * [0, n_ref), for n_spans == 0 and for unknown flag bits. */
#define SBH_DEPTH_DEL 1u                      /* D ops cover (samtools depth -J) */
typedef struct sbh_depth sbh_depth;           /* owned by a context; outlives shards */
typedef struct { int32_t ref_id; int32_t pad; int64_t beg, end; } sbh_depth_span;
typedef struct { uint64_t n, n_kept, n_counted, n_unplaced, cov_bases; } sbh_depth_add_result;
typedef struct { uint64_t slots, n_runs, covered, sum; uint32_t max_depth, pad; } sbh_depth_sizes;
typedef struct { int32_t ref_id; uint32_t depth; int64_t beg, end; } sbh_depth_run;

int sbh_depth_create(sbh_ctx *ctx, const sbh_depth_span *spans, uint32_t n_spans, int32_t n_ref, uint32_t flags,
                     sbh_depth **out);
int sbh_depth_destroy(sbh_depth *d);
int sbh_depth_reset(sbh_depth *d);
int sbh_records_depth_add(sbh_shard *sh, sbh_depth *d, const sbh_record_filter *filter /* NULL: all */,
                          sbh_depth_add_result *out);
int sbh_depth_finish(sbh_depth *d, sbh_depth_sizes *out);
int sbh_depth_fetch(sbh_depth *d, uint32_t span, uint64_t from, uint64_t n, uint32_t *depth);
int sbh_depth_runs_fetch(sbh_depth *d, uint64_t first, uint64_t count, sbh_depth_run *runs);
const void *sbh_depth_device_ptr(sbh_depth *d, uint32_t span);   /* u32 depth of the span, after finish */
/* HOST ONLY, no context, no GPU.  sbh_depth_slots: the slots of the spans together, the sum of
 * end - beg + 1 (0 for spans the other calls refuse).  sbh_depth_add_host adds into slots[] (the
 * caller zeroes it first); SBH_E_BAD_RECORD with *bad_row = the first bad row, the slots untouched.
 * sbh_depth_finish_host turns slots[] into depth in place (the same 32 bits, unsigned) and writes
 * the first run_cap runs (runs may be NULL with run_cap 0); sizes->n_runs counts them all. */
uint64_t sbh_depth_slots(const sbh_depth_span *spans, uint32_t n_spans);
int sbh_depth_add_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                       const sbh_record_filter *filter, const sbh_depth_span *spans, uint32_t n_spans,
                       int32_t n_ref, uint32_t flags, int32_t *slots, sbh_depth_add_result *out,
                       uint64_t *bad_row);
int sbh_depth_finish_host(int32_t *slots /* in place -> depth */, const sbh_depth_span *spans, uint32_t n_spans,
                          sbh_depth_run *runs, uint64_t run_cap, sbh_depth_sizes *out);

/* ---- Per-base allele counts (pileup) --------------------------------------------------------
 * What the kept records show at each reference position: how many A, C, G, T, other codes,
 * deletions, insertions and low-quality bases, and the base they agree on.  Computed on the device
 * from the flat bytes and record starts of a scan and accumulated across shards in an sbh_pileup,
 * which belongs to a context and outlives the shards added to it (csrc/pileup_core.h holds the
 * definition for device and host).
 * Spans as sbh_depth's.  Span k owns end - beg positions of one array; every position has eight
 * uint32 channels, 32 bytes of HBM per position (SBH_E_NOMEM):
 *   SBH_PILE_A, _C, _G, _T   an M / = / X base with 4-bit code 1 / 2 / 4 / 8 and quality >= min_baseq
 *   SBH_PILE_N               the same with any other code (0, the IUPAC codes, 15)
 *   SBH_PILE_DEL             a D op covers the position
 *   SBH_PILE_INS             an I op of length >= 1 starts right after the position
 *   SBH_PILE_LOWQ            an M / = / X base with quality < min_baseq, whatever its code
 * Kept, placed and counted rows are sbh_depth's.  The walk starts at x = pos, q = 0: M, =, X give
 * reference position x + j query base q + j; D adds to DEL over [x, x + len); I adds to INS at
 * x - 1 when len >= 1 and x > pos (an insertion before the first reference-consuming base counts
 * nowhere); N, S, H, P add nothing; M, I, S, =, X advance q and M, D, N, =, X advance x (64-bit
 * arithmetic).  Quality bytes compare unsigned: 0xff passes every min_baseq.  With l_seq == 0
 * (SEQ *) every M / = / X position counts into N without a quality test.  The stored CIGAR field
 * counts: a CG:B,I tag is not followed.
 * sbh_records_pileup_add uses the rows of the last valid scan on the shard as sbh_records_depth_add
 * does and validates every row as it does; a kept row is bad too when an op code is above 8, when
 * ref_id >= n_ref, or when n_cigar > 0, l_seq > 0 and the lengths of its M, I, S, =, X ops do not
 * sum to l_seq.  SBH_E_BAD_RECORD {row} for the first bad row, SBH_E_NEED_HALO instead when that
 * row merely runs past an open shard end; a failed add leaves the accumulator exactly as it was.
 * totals[c] = what the add put into channel c.  One thread at a time per sbh_pileup.
 * sbh_pileup_finish (min_depth >= 1, call_pct in [1, 100]): per position depth = A + C + G + T + N
 * + LOWQ and total = A + C + G + T + N + DEL; the call byte is 0 when all eight channels are 0,
 * else the letter ('A' 'C' 'G' 'T' '*') of the largest of A, C, G, T, DEL when that maximum is
 * unique, total >= min_depth and best * 100 >= call_pct * total, else 'N'.  An interval is a
 * maximal stretch of positions with a non-zero call byte inside one span.  nonzero = positions
 * with a non-zero call byte, n_called = those called A, C, G, T or *, covered = positions of depth
 * >= 1, totals = every add's totals together.  The counts are not changed by a finish.  After it an
 * add or a second finish gives SBH_E_STATE until sbh_pileup_reset (zero, open for adds again);
 * before it the call and interval fetches give SBH_E_STATE.  sbh_pileup_counts_fetch works before
 * and after a finish and always writes [n][8] in channel order; sbh_pileup_device_ptr is the
 * span's first position in the device array, which has the same layout: position-major,
 * uint32 [positions][8], 32-byte rows (NULL for a span out of range).
 * SBH_E_ARG for bad spans (as sbh_depth's), min_baseq outside [0, 255], min_depth < 1, call_pct
 * outside [1, 100], and a shard of another context.
 * sbh_pileup_budget: the positions an accumulator created now could hold -- three quarters of the
 * device memory free at the call, at 33 bytes per position (the channels and the call byte). */
#define SBH_PILE_A 0
#define SBH_PILE_C 1
#define SBH_PILE_G 2
#define SBH_PILE_T 3
#define SBH_PILE_N 4
#define SBH_PILE_DEL 5
#define SBH_PILE_INS 6
#define SBH_PILE_LOWQ 7
typedef struct sbh_pileup sbh_pileup;         /* owned by a context; outlives shards */
typedef struct { uint64_t n, n_kept, n_counted, n_unplaced, totals[8]; } sbh_pileup_add_result;
typedef struct {
  uint64_t positions, n_intervals, nonzero, n_called, covered, totals[8];
  uint32_t max_depth, pad;
} sbh_pileup_sizes;

int sbh_pileup_create(sbh_ctx *ctx, const sbh_depth_span *spans, uint32_t n_spans, int32_t n_ref,
                      int32_t min_baseq, sbh_pileup **out);
int sbh_pileup_destroy(sbh_pileup *p);
int sbh_pileup_reset(sbh_pileup *p);
int sbh_records_pileup_add(sbh_shard *sh, sbh_pileup *p, const sbh_record_filter *filter /* NULL: all */,
                           sbh_pileup_add_result *out);
int sbh_pileup_finish(sbh_pileup *p, uint32_t min_depth, uint32_t call_pct, sbh_pileup_sizes *out);
int sbh_pileup_counts_fetch(sbh_pileup *p, uint32_t span, uint64_t from, uint64_t n, uint32_t *out /* [n][8] */);
int sbh_pileup_calls_fetch(sbh_pileup *p, uint32_t span, uint64_t from, uint64_t n, uint8_t *out);
int sbh_pileup_intervals_fetch(sbh_pileup *p, uint64_t first, uint64_t count, sbh_depth_span *out);
const void *sbh_pileup_device_ptr(sbh_pileup *p, uint32_t span);
int sbh_pileup_budget(sbh_ctx *ctx, uint64_t *max_positions);
/* HOST ONLY, no context, no GPU.  sbh_pileup_add_host adds into counts[positions][8] (the caller
 * zeroes it first; positions = the spans' end - beg together); SBH_E_BAD_RECORD with *bad_row =
 * the first bad row, the counts untouched.  sbh_pileup_finish_host writes calls[positions] and the
 * first interval_cap intervals (may be NULL with interval_cap 0); sizes->n_intervals counts them
 * all. */
int sbh_pileup_add_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                        const sbh_record_filter *filter, const sbh_depth_span *spans, uint32_t n_spans,
                        int32_t n_ref, int32_t min_baseq, uint32_t *counts, sbh_pileup_add_result *out,
                        uint64_t *bad_row);
int sbh_pileup_finish_host(const uint32_t *counts, const sbh_depth_span *spans, uint32_t n_spans,
                           uint32_t min_depth, uint32_t call_pct, uint8_t *calls, sbh_depth_span *intervals,
                           uint64_t interval_cap, sbh_pileup_sizes *out);

/* ---- Flag counts and per-reference read counts ---------------------------------------------
 * What samtools flagstat and samtools idxstats report, counted on the device in one pass over the
 * fixed fields of a record scan's rows and summed over any number of scans and shards in an
 * sbh_tally, which belongs to a context and outlives the shards added to it (csrc/tally_core.h
 * holds the definition for device and host).
 *
 * A row the filter keeps (NULL: every row) counts; a kept row whose reference id is >= n_ref is a
 * bad row, the mate's reference id is not validated, and every row, kept or not, must be a valid
 * record.  flag[SBH_TALLY_ROWS][2]: column 0 the QC-passed rows, column 1 the QC-failed ones
 * (0x200); the rows are total, primary, secondary, supplementary, duplicates, primary duplicates,
 * mapped, primary mapped, paired, read1, read2, properly paired, itself and mate mapped,
 * singletons, mate on a different reference, the same with mapq >= 5 -- flagstat's lines in its
 * order.  ref[n_ref + 1][2]: per reference id the rows with 0x4 clear (column 0) and set (column
 * 1); bin n_ref takes every row without a reference (idxstats' `*` line).
 *
 * sbh_records_tally_add uses the rows of the last valid scan on the shard, in their order, as
 * sbh_records_bam_scan does (a row delivered twice counts twice; decode == 0 is enough), and
 * leaves the scan's rows, columns, text and BAM stream alone.  It synchronises the shard's stream
 * before it returns: the shard may be destroyed right after.  A failed add -- SBH_E_BAD_RECORD
 * {row}, or SBH_E_NEED_HALO when the first bad row merely runs past an open shard end -- leaves
 * the accumulator exactly as it was.  There is no finish: sbh_tally_fetch may be called between
 * adds, and copies flag (32 words, or NULL) and bins [first_bin, first_bin + n_bins) of ref (2
 * n_bins words, or NULL); first_bin + n_bins > n_ref + 1 is SBH_E_ARG, and so are a negative n_ref
 * and a shard of another context.  One thread at a time per sbh_tally. */
typedef struct sbh_tally sbh_tally;           /* owned by a context; outlives shards */
typedef struct { uint64_t n, n_kept; } sbh_tally_add_result;
#define SBH_TALLY_ROWS 16
int sbh_tally_create(sbh_ctx *ctx, int32_t n_ref /* >= 0 */, sbh_tally **out);
int sbh_tally_destroy(sbh_tally *t);
int sbh_tally_reset(sbh_tally *t);
int sbh_records_tally_add(sbh_shard *sh, sbh_tally *t, const sbh_record_filter *filter /* NULL: all */,
                          sbh_tally_add_result *out);
int sbh_tally_fetch(sbh_tally *t, uint64_t *flag /* [16][2] or NULL */, uint64_t first_bin, uint64_t n_bins,
                    uint64_t *ref /* [n_bins][2] or NULL */);
/* HOST ONLY, no context, no GPU: adds into flag[16][2] and ref[n_ref + 1][2] (the caller zeroes
 * them first); SBH_E_BAD_RECORD with *bad_row = the first bad row, the arrays untouched. */
int sbh_tally_add_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                       const sbh_record_filter *filter, int32_t n_ref, uint64_t *flag, uint64_t *ref,
                       sbh_tally_add_result *out, uint64_t *bad_row);

/* ---- Read-level statistics ------------------------------------------------------------------
 * The histograms of samtools stats -- read lengths, per-cycle qualities of first and last fragments,
 * per-cycle base composition, GC content, insert sizes, mapping qualities and a table of summary
 * numbers -- counted on the device over the rows of a record scan and summed over any number of
 * scans and shards in an sbh_stats, which belongs to a context and outlives the shards added to it
 * (csrc/stats_core.h holds the definition for device and host, table by table).
 *
 * params: cycles in [1, 65536] (reads longer than that share the last row of the per-cycle tables),
 * max_insert in [1, 1 << 20] (larger insert sizes share the last bin); fixed at create.  A row the
 * filter keeps (NULL: every row) is counted when it is neither secondary nor supplementary; the
 * other kept rows add to sn's secondary / supplementary counters alone.  Every row, kept or not,
 * must be a valid record; no reference id is validated.  The tables (uint64):
 *   sn[SBH_STATS_SN]  read_len[cycles + 2]  qual[2][cycles + 1][SBH_STATS_QUALS]  base[cycles + 1][5]
 *   gc[2][101]  isize[max_insert + 1][3]  mapq[256]
 *
 * sbh_records_stats_add uses the rows of the last valid scan on the shard, in their order, as
 * sbh_records_tally_add does (decode == 0 is enough), leaves the scan alone and synchronises the
 * shard's stream before it returns.  A failed add -- SBH_E_BAD_RECORD {row}, or SBH_E_NEED_HALO when
 * the first bad row merely runs past an open shard end -- leaves the accumulator exactly as it was.
 * There is no finish: sbh_stats_fetch may be called between adds, and copies out the tables asked for
 * (any pointer may be NULL).  SBH_E_STATE without a valid scan; SBH_E_ARG for parameters out of
 * range, a bad filter and a shard of another context.  One thread at a time per sbh_stats. */
typedef struct sbh_stats sbh_stats;           /* owned by a context; outlives shards */
typedef struct { uint32_t cycles, max_insert; } sbh_stats_params;
typedef struct { uint64_t n, n_kept, n_counted; } sbh_stats_add_result;
#define SBH_STATS_QUALS 94
#define SBH_STATS_SN 23
int sbh_stats_create(sbh_ctx *ctx, const sbh_stats_params *params, sbh_stats **out);
int sbh_stats_destroy(sbh_stats *s);
int sbh_stats_reset(sbh_stats *s);
int sbh_records_stats_add(sbh_shard *sh, sbh_stats *s, const sbh_record_filter *filter /* NULL: all */,
                          sbh_stats_add_result *out);
int sbh_stats_fetch(sbh_stats *s, uint64_t *sn, uint64_t *read_len, uint64_t *qual, uint64_t *base, uint64_t *gc,
                    uint64_t *isize, uint64_t *mapq);
/* HOST ONLY, no context, no GPU: adds into the seven tables (the caller zeroes them first; none may
 * be NULL); SBH_E_BAD_RECORD with *bad_row = the first bad row, the tables untouched. */
int sbh_stats_add_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                       const sbh_record_filter *filter, const sbh_stats_params *params, uint64_t *sn,
                       uint64_t *read_len, uint64_t *qual, uint64_t *base, uint64_t *gc, uint64_t *isize,
                       uint64_t *mapq, sbh_stats_add_result *out, uint64_t *bad_row);

/* ---- FASTQ / FASTA text -------------------------------------------------------------------
 * What samtools fastq and samtools fasta write, rendered on the device from the flat bytes and
 * record starts of a scan (csrc/fastq_core.h holds the definition for device and host).  A row the
 * filter keeps (NULL: every row) becomes
 *     @NAME[/1|/2]\nSEQ\n+\nQUAL\n        or, with SBH_FASTQ_FASTA,        >NAME[/1|/2]\nSEQ\n
 * NAME: the name bytes up to the first NUL, as SAM text's QNAME.  Suffix: with SBH_FASTQ_SUFFIX,
 * /1 when flag & 0x1 and (flag & 0xC0) == 0x40, /2 when flag & 0x1 and (flag & 0xC0) == 0x80, else
 * none; SBH_FASTQ_SUFFIX_ALWAYS drops the 0x1 condition (and wins over SBH_FASTQ_SUFFIX); neither
 * bit: never a suffix.  SEQ: the "=ACMGRSVTWYHKDBN" letters, reverse-complemented when flag & 0x10
 * (A<>T C<>G M<>K R<>Y V<>B H<>D; = S W N stay).  QUAL: min(q, 93) + 33 per base, reversed when
 * flag & 0x10; when the first quality byte is 0xFF every byte is def_qual + 33 (samtools fastq -v,
 * 1 by default there).  l_seq == 0 gives empty SEQ and QUAL lines.
 * SBH_FASTQ_SPLIT: a kept row's class is 1 or 2 by the /1 and /2 conditions (without the 0x1
 * condition under SBH_FASTQ_SUFFIX_ALWAYS), else 0, and the text is three parts one after another
 * -- the class 1 lines, the class 2 lines, the class 0 lines, each in row order; part_bytes and
 * part_rows are in that order.  Without the bit: one part in row order (part 0; parts 1 and 2
 * empty).  samtools' -s singleton file needs reads collated by name and is not offered.
 * rows = the rows of the last valid scan on this shard, in their order, as the BAM stream takes them
 * (decode == 0 is enough); every row, kept or not, is validated as there.  The scan call leaves the
 * scan's rows, columns, SAM text and BAM stream alone and synchronises the shard's stream before it
 * returns, so the context-level compress call may follow directly on the device pointer (NULL
 * without a valid FASTQ scan); a new scan, sbh_shard_load, sbh_index or sbh_run_shard invalidates
 * the text, and the last three the scan itself.  The fetch
 * copies out what is asked for (any pointer may be NULL): the text, rec_off (n_kept + 1: where each
 * line begins, in the text's order, then text_bytes) and rows (n_kept: the scan row of each line).
 * Errors: SBH_E_STATE without a valid scan; SBH_E_ARG for unknown mode bits, def_qual outside
 * [0, 93] or a bad filter; SBH_E_BAD_RECORD {row} for the first invalid row, SBH_E_NEED_HALO instead
 * when that row merely runs past an open shard end.  n == 0 or n_kept == 0 gives text_bytes = 0 and
 * rec_off = [0]. */
#define SBH_FASTQ_FASTA 1u
#define SBH_FASTQ_SUFFIX 2u
#define SBH_FASTQ_SUFFIX_ALWAYS 4u
#define SBH_FASTQ_SPLIT 8u
typedef struct { uint64_t n, n_kept, text_bytes, part_bytes[3], part_rows[3]; } sbh_fastq_sizes;
int sbh_records_fastq_scan(sbh_shard *sh, const sbh_record_filter *filter /* NULL: keep all */,
                           uint32_t mode, int32_t def_qual, sbh_fastq_sizes *out);
const void *sbh_records_fastq_device_ptr(sbh_shard *sh);
int sbh_records_fastq_fetch(sbh_shard *sh, char *text /*[text_bytes]*/, uint64_t *rec_off /*[n_kept+1]*/,
                            uint64_t *rows /*[n_kept]*/);
/* HOST ONLY, no context, no GPU: the same text for the records at starts[] of a flat BAM stream.
 * rec_off (room for n + 1) and rows (room for n) may be NULL; text == NULL: sizes only.
 * SBH_E_BAD_RECORD with *bad_row = the first invalid row, kept or not; SBH_E_ARG for bad arguments
 * as above or when text_cap < text_bytes (*sizes is set then). */
int sbh_fastq_render_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                          const sbh_record_filter *filter, uint32_t mode, int32_t def_qual,
                          char *text, uint64_t text_cap, uint64_t *rec_off, uint64_t *rows,
                          sbh_fastq_sizes *sizes, uint64_t *bad_row);

/* ---- BGZF writer -------------------------------------------------
 * The block compressor behind HTSJDKRewrite (cli/src/main/scala/org/hammerlab/bam/rewrite/
 * HTSJDKRewrite.scala:62-67: SAMFileWriterFactory.makeBAMWriter -> htsjdk
 * BlockCompressedOutputStream): the uncompressed stream src[0, n) is cut every 65498 bytes and
 * each piece becomes one BGZF member, CRC32 + ISIZE footer, then the 28-byte empty EOF member.
 * sbh_bgzf_compress writes exactly htsjdk's bytes: each member is what java.util.zip.Deflater
 * (level 5, nowrap) = zlib 1.2.11 deflate_slow produces, and a member whose deflate stream does
 * not finish within htsjdk's 65518-byte buffer is re-deflated at level 0 (one stored block).
 * sbh_bgzf_compress_level: level 5 (SBH_LEVEL_HTSJDK) as above; 4 and 6..9 the same zlib at
 * that level (6 is samtools' default); 0 stored members; SBH_LEVEL_FAST this library's own
 * faster coder (hash-chain LZ77 with lazy matching, one dynamic-Huffman block per member, not
 * zlib's bytes).  src is a host or device pointer (src_on_device); out is host memory of at
 * least sbh_bgzf_compress_bound(n) bytes.  Device scratch is bounded by a batch of members,
 * whatever n: about 1.04 MB per member at levels 4..9 (prev 128 KiB, match records 512 KiB,
 * tokens 256 KiB, block record 16 KiB, two 65.6 KB slots), batches of up to 8192 members
 * (~8.5 GB; SBH_ZDEFLATE_BATCH overrides) and never more than half of the free HBM at the call
 * (at least 256 members); SBH_LEVEL_FAST batches up to 2048 members of ~0.4 MB.  The uncompressed
 * input (n bytes, when src is host memory) is staged in HBM as well.  *deflate_ms (optional): the
 * compress kernels' device time, summed over the batches (HIP events on the context's stream). */
#define SBH_LEVEL_HTSJDK 5
#define SBH_LEVEL_FAST (-1)
uint64_t sbh_bgzf_compress_bound(uint64_t n);
int sbh_bgzf_compress(sbh_ctx *ctx, const void *src, uint64_t n, int src_on_device, uint8_t *out,
                      uint64_t out_cap, uint64_t *out_size, uint64_t *n_blocks, float *deflate_ms);
int sbh_bgzf_compress_level(sbh_ctx *ctx, const void *src, uint64_t n, int src_on_device, int level,
                            uint8_t *out, uint64_t out_cap, uint64_t *out_size, uint64_t *n_blocks,
                            float *deflate_ms);

#ifdef __cplusplus
}
#endif
#endif /* SPARKBAM_H */
