"""Reference-shaped host API over the C-ABI.

Each function names the spark-bam entry point it mirrors (paths relative to the
reference repository root).  All byte work runs in libsparkbam_hip.so on the GPU;
this module only moves small results around (splits, counts, histograms).
"""
import ctypes as C
import os
from collections import namedtuple
from contextlib import ExitStack, closing, contextmanager

import numpy as np

from ._lib import FULL_FLAGS_MASK, FULL_N_SHIFT, SBH_E_ARG, SBH_E_NEED_HALO, SBH_OK, SparkBamError, lib
from .device import Context
from .records import Reads

FLAG_NAMES = [  # check/.../full/error/Flags.scala:203-222 (serde order)
    "tooFewFixedBlockBytes", "negativeReadIdx", "tooLargeReadIdx", "negativeReadPos",
    "tooLargeReadPos", "negativeNextReadIdx", "tooLargeNextReadIdx", "negativeNextReadPos",
    "tooLargeNextReadPos", "tooFewBytesForReadName", "nonNullTerminatedReadName",
    "nonASCIIReadName", "noReadName", "emptyReadName", "tooFewBytesForCigarOps",
    "invalidCigarOp", "emptyMappedCigar", "emptyMappedSeq", "tooFewRemainingBytesImplied",
]

DEFAULT_BGZF_BLOCKS_TO_CHECK = 5      # bgzf/.../block/package.scala:20
DEFAULT_READS_TO_CHECK = 10          # check/.../check/package.scala:17-18
DEFAULT_MAX_READ_SIZE = 100000000    # check/.../check/package.scala:28-29
DEFAULT_SPLIT_SIZE = 32 * 1024 * 1024  # Hadoop local-FS block size (MaxSplitSize default)


class Pos(namedtuple("Pos", "block_pos offset")):
    """bgzf Pos(blockPos, offset) (bgzf/.../Pos.scala:12-43)."""

    def to_htsjdk(self):
        return (self.block_pos << 16) | self.offset

    @classmethod
    def from_htsjdk(cls, v):
        return cls(v >> 16, v & 0xFFFF)

    def __str__(self):
        return f"{self.block_pos}:{self.offset}"

    def minus(self, other, ratio=3.0):  # Pos.- with EstimatedCompressionRatio (Pos.scala:17-22)
        return float(max(0, self.block_pos - other.block_pos + int((self.offset - other.offset) / ratio)))


Split = namedtuple("Split", "start end")  # check/.../spark/Split.scala:9-13
Metadata = namedtuple("Metadata", "start compressed_size uncompressed_size")  # Metadata.scala:6-8


class Header:
    @staticmethod
    def make(b):
        """Header.make (bgzf/.../block/Header.scala:48-83) -> (size, compressedSize)."""
        arr = np.frombuffer(bytes(b), dtype=np.uint8)
        hs, cs = C.c_int32(), C.c_int32()
        rc = lib().sbh_header_make(arr.ctypes.data_as(C.c_void_p), arr.size, C.byref(hs), C.byref(cs))
        if rc != SBH_OK:
            raise SparkBamError(rc, "bad BGZF header")
        return hs.value, cs.value


def file_splits(file_size, split_size):
    """Hadoop FileInputFormat.getSplits arithmetic (SPLIT_SLOP 1.1), as driven by
    FileSplits.asJava(path, splitSize) (load/.../CanLoadBam.scala:205,314)."""
    out, rem = [], file_size
    while rem / split_size > 1.1:
        out.append((file_size - rem, file_size - rem + split_size))
        rem -= split_size
    if rem != 0:
        out.append((file_size - rem, file_size))
    return out


def parse_bam_header(flat):
    """check/.../header/Header.scala:26-60: contig lengths + flat end of the header."""
    b = bytes(flat)
    if b[:4] != b"BAM\1":
        raise SparkBamError(1, "not a BAM file (missing BAM\\1 magic)")
    l_text = int.from_bytes(b[4:8], "little", signed=True)
    c = 8 + l_text
    n_ref = int.from_bytes(b[c:c + 4], "little", signed=True)
    c += 4
    names, lens = [], []
    for _ in range(n_ref):
        l_name = int.from_bytes(b[c:c + 4], "little", signed=True)
        names.append(b[c + 4:c + 4 + l_name].rstrip(b"\0").decode())
        c += 4 + l_name
        lens.append(int.from_bytes(b[c:c + 4], "little", signed=True))
        c += 4
    return names, np.asarray(lens, dtype=np.int32), c


def bam_header(shard):
    """Header(path) over an indexed + inflated shard starting at file offset 0."""
    n = min(shard.flat_size, 1 << 16)
    while True:
        try:
            return parse_bam_header(shard.read_flat(0, n))
        except (IndexError, ValueError):
            if n >= shard.flat_size:
                raise
            n = min(shard.flat_size, n * 4)


def _read(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview, np.ndarray)):
        return np.frombuffer(bytes(path_or_bytes), dtype=np.uint8) if not isinstance(
            path_or_bytes, np.ndarray) else path_or_bytes
    with open(path_or_bytes, "rb") as f:
        return np.frombuffer(f.read(), dtype=np.uint8)


@contextmanager
def _context(ctx):
    """The caller's context, or one of our own that is closed on the way out."""
    own_ctx = ctx is None
    ctx = ctx or Context(0)
    try:
        yield ctx
    finally:
        if own_ctx:
            ctx.close()


def _flag_filter(flag_require, flag_exclude, min_mapq):
    """records.record_filter's dict of the entries' three filter arguments."""
    return {"flag_require": flag_require, "flag_exclude": flag_exclude, "min_mapq": min_mapq}


def _adding(acc, f):
    """A delivery for _iter_windows: the window's records scanned, and the rows that the filter
    dict f keeps added to the accumulator; the add's counts are what the walk yields."""
    def deliver(sh, first, E, _names):
        sh.records_scan(first, E)
        return [acc.add(sh, f)]
    return deliver


class _Loaded(ExitStack):
    """A whole BGZF file resident on one device: indexed, inflated, header parsed.  Leaving it
    (`with`, or close()) closes the shard, then the context if it is our own."""

    def __init__(self, path_or_bytes, ctx=None, reads_to_check=DEFAULT_READS_TO_CHECK):
        super().__init__()
        self.data = _read(path_or_bytes)
        self.ctx = self.enter_context(_context(ctx))
        self.shard = self.ctx.shard(self.data)
        self.callback(self.shard.close)
        self.shard.index(0)
        self.shard.inflate()
        self.names, self.contig_len, self.header_end = bam_header(self.shard)
        self.shard.set_contigs(self.contig_len)
        self.reads_to_check = reads_to_check


def load_splits_and_reads(path_or_bytes, split_size=DEFAULT_SPLIT_SIZE, ctx=None,
                          bgzf_blocks_to_check=DEFAULT_BGZF_BLOCKS_TO_CHECK,
                          reads_to_check=DEFAULT_READS_TO_CHECK, max_read_size=DEFAULT_MAX_READ_SIZE):
    """CanLoadBam.loadSplitsAndReads (load/.../CanLoadBam.scala:268-302): the splits
    (first record of every non-empty partition, sliding2 with Pos(fileSize, 0)) and
    the per-partition record counts.  A file larger than sharded.RESIDENT_MAX compressed bytes
    is memory-mapped and streamed through HBM (windows cut at split starts, each split decided
    in its window) instead of being held resident."""
    from . import sharded  # (sharded builds on this module)
    size = os.path.getsize(path_or_bytes) if isinstance(path_or_bytes, (str, os.PathLike)) else len(path_or_bytes)
    if size > sharded.RESIDENT_MAX:
        splits, counts, _ = sharded.load_splits_and_reads(
            path_or_bytes, split_size, ctx=ctx, rank=0, world=1, bgzf_blocks_to_check=bgzf_blocks_to_check,
            reads_to_check=reads_to_check, max_read_size=max_read_size)
        return splits, counts
    with _Loaded(path_or_bytes, ctx, reads_to_check) as L:
        sh = L.shard
        # every split in one batch (FindBlockStart + FindRecordStart + counts on the device)
        status, v, n, _ = sh.split_starts(file_splits(L.data.size, split_size), bgzf_blocks_to_check,
                                          reads_to_check, max_read_size)
        bad = np.flatnonzero(status)
        if bad.size:
            raise SparkBamError(int(status[bad[0]]), f"split {int(bad[0])}")
        counts = [int(x) for x in n]
        firsts = [Pos.from_htsjdk(int(x)) for x, c in zip(v, n) if c > 0]
        ends = firsts[1:] + [Pos(L.data.size, 0)]
        return [Split(a, b) for a, b in zip(firsts, ends)], counts


def load_reads(path_or_bytes, ctx=None, reads_to_check=DEFAULT_READS_TO_CHECK, window=None):
    """CanLoadBam.loadReads (load/.../CanLoadBam.scala:244-264) on one device: every
    record of the file's BAM stream, in file order, decoded on the GPU into a columnar
    `Reads` batch (RecordStream.scala:16-41 semantics: records from the first one after
    the header while they start before the stream's end).  The eager bitmap of the
    record range is computed first, so record starts come from it in parallel (verified
    against the chain) rather than from a sequential chain walk.  A file larger than
    sharded.RESIDENT_MAX (or with `window` given) is decoded a window at a time (iter_reads)
    and the batches joined."""
    from . import sharded
    size = os.path.getsize(path_or_bytes) if isinstance(path_or_bytes, (str, os.PathLike)) else len(path_or_bytes)
    if window is not None or size > sharded.RESIDENT_MAX:
        with _context(ctx) as ctx:
            batches = list(iter_reads(path_or_bytes, window=window or sharded.STREAM_WINDOW, ctx=ctx,
                                      reads_to_check=reads_to_check))
            names = file_header(ctx, _file_array(path_or_bytes))[0]
        return Reads.concat(batches, names)
    with _Loaded(path_or_bytes, ctx, reads_to_check) as L:
        sh = L.shard
        end = sh.flat_size
        for b in sh.blocks():
            if b[5] & 1:  # BLOCK_EMPTY: the stream ends at its flat start
                end = b[3]
                break
        sh.check_eager(L.header_end, end, reads_to_check, want_bits=False)
        cols = sh.records(L.header_end, end)
        return Reads(cols, L.names)


def _vpos_of(flat, blocks):
    """htsjdk vpos of flat positions (numpy) from a shard's block table (Pos.scala's canonical
    form: a record at a block's end is Pos(next block, 0); empty blocks never hold one)."""
    blk = np.asarray([(b[0], b[3], b[2]) for b in blocks if b[2] > 0], dtype=np.int64).reshape(-1, 3)
    if flat.size == 0 or blk.size == 0:
        return np.zeros(flat.size, dtype=np.uint64)
    f = flat.astype(np.int64)
    i = np.searchsorted(blk[:, 1], f, side="right") - 1
    return (blk[i, 0].astype(np.uint64) << np.uint64(16)) | (f - blk[i, 1]).astype(np.uint64)


def iter_reads(path_or_bytes, window=None, halo=4 << 20, ctx=None, reads_to_check=DEFAULT_READS_TO_CHECK):
    """CanLoadBam.loadReads (load/.../CanLoadBam.scala:244-264) over a file of any size: the
    records from the first one after the header while they start before the stream's end
    (RecordStream.scala:16-41), decoded on the GPU a window of `window` compressed bytes at a
    time; yields one columnar `Reads` batch per window, in file order, each with a `vpos` column
    (htsjdk virtual offsets; `flat` is window-relative).  A window starts at the block of the
    previous window's chain exit, so batches never overlap."""
    return _iter_windows(path_or_bytes, lambda sh, f, E, names: Reads(sh.records(f, E), names), window, halo, ctx,
                         reads_to_check)


def _iter_windows(path_or_bytes, deliver, window=None, halo=4 << 20, ctx=None, reads_to_check=DEFAULT_READS_TO_CHECK):
    """iter_reads' walk through the file; deliver(shard, first_flat, end_flat, names) turns a
    window's records into what is yielded (anything with a len(): empty ones are dropped).

    Look first, deliver after: a window whose chain leaves the resident bytes runs again with a
    larger halo, so the chain's exit is looked at before deliver is called.  deliver is then called
    once per window and may commit as it goes (add to an accumulator, write to a sink)."""
    window = int(window or STREAM_WINDOW)
    data = _file_array(path_or_bytes)
    size = int(data.size)
    with _context(ctx) as ctx:
        names, contig_len, header_end = file_header(ctx, data)
        lo, start = 0, None  # window start (a block) and the record to start from (vpos; None: after the header)
        while lo < size:
            hi = lo + window
            while True:
                end = min(size, hi + halo)
                sh = ctx.shard(np.ascontiguousarray(data[lo:end]), file_offset=lo, file_size=size)
                try:
                    sh.set_contigs(contig_len)
                    sh.index(lo)
                    sh.inflate()
                    blocks = sh.blocks()
                    E = sh.flat_bound(hi)
                    if end < size and E == sh.flat_size:
                        raise SparkBamError(SBH_E_NEED_HALO, "no block past the window in the halo")
                    f = header_end if start is None else sh.flat_of(start >> 16, start & 0xFFFF)
                    seg = next((b[3] for b in blocks if b[5] & 1 and b[3] >= f), None)  # an empty block ends the stream
                    last = seg is not None and seg <= E or end == size and E == sh.flat_size
                    if seg is not None:
                        E = min(E, seg)
                    sh.check_eager(f, E, reads_to_check, want_bits=False)
                    x = sh.chain_from(f, E)[1] if E > f else f
                    if not last and x >= sh.flat_size:
                        raise SparkBamError(SBH_E_NEED_HALO, "the chain leaves the halo")
                    batch = deliver(sh, f, E, names) if E > f else None
                    nxt = None if last else int(Pos(*sh.pos_of(x)).to_htsjdk())
                    break
                except SparkBamError as err:
                    if err.code != SBH_E_NEED_HALO or end >= size:
                        raise
                    halo *= 4
                finally:
                    sh.close()
            if batch is not None and len(batch):
                yield batch
            if last:
                return
            start, lo = nxt, nxt >> 16


def view(path_or_bytes, header=False, out=None, window=None, ctx=None, reads_to_check=DEFAULT_READS_TO_CHECK):
    """The file's records as SAM text, one line per record (what `samtools view` / htsjdk
    SAMRecord.getSAMString print; the reference's test_bams .sam fixtures), rendered on the GPU
    (Shard.records_sam) a window at a time, with iter_reads' windowing.  header=True puts the BAM
    header text first, verbatim.  out: a binary file object the text is written to as it is
    produced (returns the byte count); None: returns the text as bytes."""
    data = _file_array(path_or_bytes)
    parts, total = [], 0

    def put(b):
        nonlocal total
        total += len(b)
        if out is None:
            parts.append(bytes(b))
        else:
            out.write(b)

    def deliver(sh, f, E, names):
        sh.records_scan(f, E)
        return sh.records_sam(names)[0]

    with _context(ctx) as ctx:
        if header:
            put(header_text(ctx, data))
        for text in _iter_windows(data, deliver, window, ctx=ctx, reads_to_check=reads_to_check):
            put(text.data)
    return b"".join(parts) if out is None else total


BGZF_PAYLOAD = 65498  # uncompressed bytes per member of the writer (htsjdk BlockCompressedOutputStream)
BGZF_EOF_BYTES = 28
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")  # the empty member that ends a file


def view_bam(path_or_bytes, out=None, flag_require=0, flag_exclude=0, min_mapq=0, rows=None, intervals=None,
             bai=None, level=5, window=None, index=False, ctx=None, reads_to_check=DEFAULT_READS_TO_CHECK,
             sort=None):
    """The file's records that pass the filters, as a BAM file: the header, then every record with
    (flag & flag_require) == flag_require, (flag & flag_exclude) == 0, mapq >= min_mapq and -- with
    `rows`, a range or a collection of ints -- a record index in it, byte for byte as stored, cut
    into 65498-byte BGZF members at `level` (htsjdk_rewrite's levels).  The records are selected
    and laid out on the GPU (Shard.records_bam) and compressed from device memory: they do not
    come to the host between inflate and deflate.

    Whole file: iter_reads' walk, `window` compressed bytes at a time; rows count records across
    the windows.  `intervals` (load_bam_intervals' strings; `bai` as there): only the records
    load_bam_intervals returns, in its order, the other filters on top; rows then count those.

    Members are cut every 65498 bytes of the whole stream, so a window compresses the largest
    multiple of that from the device and hands the rest (< 65498 bytes) to the next window's
    stream as its head; the last tail and the EOF member close the file.  The bytes do not depend
    on `window`.

    sort="coordinate": the kept records in stable coordinate order (Shard.records_bam's
    order="coordinate": reference, position, reverse strand, unplaced last), sorted on the GPU,
    behind a header whose @HD line says SO:coordinate.  Filters and `rows` apply before the sort.
    sort="name": the kept records in stable read-name order (Shard.records_bam's order="name":
    samtools sort -N's byte order, then READ1 / READ2, primary, secondary, supplementary), behind a
    header whose @HD line says SO:queryname.  index=True is then a ValueError: a BAI needs
    coordinate order.
    Either way the whole file must fit one window: a second window raises SparkBamError(SBH_E_ARG)
    (merging sorted windows is not done here; pass a larger `window`), and so does `intervals`.

    Returns the file bytes; with `out` (a path or a binary file object) writes them and returns
    the byte count.  index=True: also the `.bai` of the result (bai.build_bai) -- returned as
    (bam, bai), written to out + ".bai" when out is a path, or returned as (count, bai) when out
    is a file object."""
    if sort not in (None, "coordinate", "name"):
        raise ValueError("view_bam: sort is None, 'coordinate' or 'name', not %r" % (sort,))
    if sort == "name" and index:
        raise ValueError("view_bam: index=True needs coordinate order, not sort='name' (a BAI indexes by position)")
    if sort and intervals is not None:
        raise SparkBamError(SBH_E_ARG, "view_bam: sort needs the whole file in one window, not `intervals`")
    data = _file_array(path_or_bytes)
    from .records import bam_header_set_so, row_ranges
    want = None if rows is None else row_ranges(rows)
    pieces = []
    state = {"tail": None, "row_base": 0}

    def gather(sh):
        """The scan on sh -> (compressed whole members, the new tail, rows scanned); nothing is
        committed here: an interval group that has to run again with a larger halo calls this again."""
        base = state["row_base"]
        f = _flag_filter(flag_require, flag_exclude, min_mapq)
        if want is not None:
            f["rows"] = [(max(a - base, 0), b - base) for a, b in want if b > base]
        sh.records_bam(state["tail"], f, want_bytes=False, order=sort or "scan")
        whole = sh.bam_size - sh.bam_size % BGZF_PAYLOAD
        comp = b""
        if whole:
            comp = ctx.bgzf_compress(sh.bam_ptr(), whole, level=level)[0][:-BGZF_EOF_BYTES].tobytes()
        return comp, sh.bam_read(whole, sh.bam_size).tobytes(), sh.bam_n

    def commit(got):
        comp, tail, n = got
        pieces.append(comp)
        state["tail"] = tail
        state["row_base"] += n

    with _context(ctx) as ctx:
        state["tail"] = _header_flat(ctx, data)
        if sort:
            state["tail"] = bam_header_set_so(state["tail"], "queryname" if sort == "name" else sort)
        if intervals is None:
            def deliver(sh, f, E, names):
                sh.records_scan(f, E)
                return gather(sh)
            for got in _iter_windows(data, deliver, window, ctx=ctx, reads_to_check=reads_to_check):
                if sort and pieces:
                    raise SparkBamError(SBH_E_ARG, "view_bam: sort needs the file in one window; `window` (%d compressed "
                                                   "bytes) is smaller than the file (%d)"
                                        % (int(window or STREAM_WINDOW), int(data.size)))
                commit(got)
        else:
            from .intervals import iter_interval_groups

            def deliver_group(sh, chunks_flat, ivs):
                sh.records_regions(chunks_flat, ivs, fetch=False)
                return gather(sh)
            for got in iter_interval_groups(path_or_bytes, intervals, deliver_group, ctx=ctx, bai=bai,
                                            reads_to_check=reads_to_check)[0]:
                commit(got)
        # the last members (what is left is below one payload) and the EOF member
        pieces.append(ctx.bgzf_compress(np.frombuffer(state["tail"], dtype=np.uint8), level=level)[0].tobytes())
        result = b"".join(pieces)
        bai_bytes = None
        if index:
            from .bai import build_bai
            bai_bytes = build_bai(result, ctx=ctx)
    if out is None:
        return (result, bai_bytes) if index else result
    if isinstance(out, (str, os.PathLike)):
        with open(out, "wb") as fh:
            fh.write(result)
        if index:
            with open(str(out) + ".bai", "wb") as fh:
                fh.write(bai_bytes)
        return len(result)
    out.write(result)
    return (len(result), bai_bytes) if index else len(result)


def sort_bam(path_or_bytes, out=None, level=5, index=False, ctx=None, reads_to_check=DEFAULT_READS_TO_CHECK,
             order="coordinate"):
    """The file coordinate-sorted (what `samtools sort` writes, up to the compressed bytes): every
    record, in stable (reference, position, reverse strand) order with the unplaced ones last,
    under a header that says SO:coordinate.  order="name": sorted by read name instead (`samtools
    sort -N`'s byte order; the tie in view_bam's words) under SO:queryname; index=True is then a
    ValueError.  view_bam with that `sort` and the whole file as its one window; `out`, `level`,
    `index` and the return value as there."""
    if order not in ("coordinate", "name"):
        raise ValueError("sort_bam: order is 'coordinate' or 'name', not %r" % (order,))
    if order == "name" and index:
        raise ValueError("sort_bam: index=True needs coordinate order, not order='name' (a BAI indexes by position)")
    data = _file_array(path_or_bytes)
    return view_bam(data, out=out, level=level, index=index, ctx=ctx, reads_to_check=reads_to_check,
                    window=max(int(data.size), 1), sort=order)


def depth(path_or_bytes, region=None, flag_require=0, flag_exclude=0x704, min_mapq=0, count_del=False, window=None,
          ctx=None, reads_to_check=DEFAULT_READS_TO_CHECK):
    """Per-base depth of the file's records (what `samtools depth` and `bedtools genomecov -bg`
    report), computed on the GPU: every window of iter_reads' walk is scanned and added into one
    accumulator in HBM (Context.depth), which is then scanned into depth and runs of equal depth.

    region: "NAME" (that reference whole), "NAME:BEG-END" (1-based, inclusive) or None -- every
    reference whole, which costs 4 bytes of HBM per base of the genome.  A record counts when
    (flag & flag_require) == flag_require, (flag & flag_exclude) == 0 (default 0x704: unmapped,
    secondary, QC-fail, duplicate -- samtools depth's) and mapq >= min_mapq; its M, = and X ops
    cover, D too with count_del (samtools depth -J), N never.  Base qualities and mate overlaps
    are not looked at.  The whole file is read, whatever the region.

    Returns a coverage.DepthResult: `.runs`, `.stats`, `.depth(name)`, `.text(all_positions=False)`
    (samtools depth's lines) and `.bedgraph()` (genomecov -bg's)."""
    from .coverage import DEPTH_RUN_DTYPE, DepthResult, region_spans
    data = _file_array(path_or_bytes)
    with ExitStack() as stack:
        ctx = stack.enter_context(_context(ctx))
        names, contig_len, _ = file_header(ctx, data)
        try:
            spans = region_spans(region, names, contig_len)
        except ValueError as err:
            raise SparkBamError(SBH_E_ARG, str(err))
        acc = stack.enter_context(closing(ctx.depth(spans, len(contig_len), count_del)))
        deliver = _adding(acc, _flag_filter(flag_require, flag_exclude, min_mapq))
        totals = {}
        for (got,) in _iter_windows(data, deliver, window, ctx=ctx, reads_to_check=reads_to_check):
            for k, v in got.items():
                totals[k] = totals.get(k, 0) + v
        stats = dict(acc.finish())
        for k in ("n", "n_kept", "n_counted", "n_unplaced", "cov_bases"):
            stats[k] = totals.get(k, 0)
        runs = acc.runs() if stats["n_runs"] else np.zeros(0, dtype=DEPTH_RUN_DTYPE)
        # the accumulator is closed on the way out: a span's per-base depth is expanded from its runs on request
        spans_l = list(spans)

        def depths(k, runs=runs, spans=spans_l):
            ref, b, e = spans[k]
            r = runs[runs["ref_id"] == ref]
            return np.repeat(r["depth"], (r["end"] - r["beg"]).astype(np.int64)).astype(np.uint32)

        return DepthResult(runs, stats, spans_l, names, depths)


def pileup(path_or_bytes, region=None, flag_require=0, flag_exclude=0x704, min_mapq=0, min_baseq=0, min_depth=1,
           call_pct=75, max_positions=None, window=None, ctx=None, reads_to_check=DEFAULT_READS_TO_CHECK):
    """Per-base allele counts of the file's records, computed on the GPU: how many A, C, G, T, other
    codes (N), deletions, insertions and low-quality bases the kept records show at each position,
    and the base they agree on.  Every window of iter_reads' walk is scanned and added into one
    accumulator in HBM (Context.pileup), which is then turned into call bytes and intervals.

    region and the record filter as depth's.  min_baseq: a base whose quality is below it counts
    into LOWQ instead of its letter; the default 0 keeps every base, so that A+C+G+T+N+LOWQ is
    depth's number (`samtools mpileup` users will want 13, its -Q default).  min_depth, call_pct:
    a position is called A, C, G, T or * (deletion) when that channel alone is the largest, A+C+G+T+
    N+DEL >= min_depth and the channel holds at least call_pct percent of it; else N.

    The accumulator costs 33 bytes of HBM per position (all of GRCh37: about 99 GB), so the spans
    are grouped greedily into passes of at most max_positions positions, one walk of the file per
    pass, the results concatenated.  max_positions defaults to three quarters of the free device
    memory / 33 (Context.pileup_budget); a single span larger than it is a ValueError naming the span.

    Returns a pileup.PileupResult: `.intervals`, `.stats`, `.counts(name)`, `.calls(name)`,
    `.text(all_positions=False, header=False)` and `.consensus()` (FASTA)."""
    from .coverage import DEPTH_SPAN_DTYPE, region_spans
    from .pileup import PileupResult, span_passes
    data = _file_array(path_or_bytes)
    with _context(ctx) as ctx:
        names, contig_len, _ = file_header(ctx, data)
        try:
            spans = region_spans(region, names, contig_len)
        except ValueError as err:
            raise SparkBamError(SBH_E_ARG, str(err).replace("depth:", "pileup:"))
        budget = ctx.pileup_budget() if max_positions is None else int(max_positions)
        f = _flag_filter(flag_require, flag_exclude, min_mapq)
        stats, ivs, counts, calls = {"totals": [0] * 8}, [], [], []
        for group in span_passes(spans, budget):
            with closing(ctx.pileup(group, len(contig_len), min_baseq)) as acc:
                totals = {}
                for (got,) in _iter_windows(data, _adding(acc, f), window, ctx=ctx, reads_to_check=reads_to_check):
                    for k in ("n", "n_kept", "n_counted", "n_unplaced"):
                        totals[k] = totals.get(k, 0) + got[k]
                sz = acc.finish(min_depth, call_pct)
                for k in ("positions", "n_intervals", "nonzero", "n_called", "covered"):
                    stats[k] = stats.get(k, 0) + sz[k]
                stats["max_depth"] = max(stats.get("max_depth", 0), sz["max_depth"])
                stats["totals"] = [a + b for a, b in zip(stats["totals"], sz["totals"])]
                # every pass walks every record: the rows are the file's; a row is counted in the pass
                # that holds its reference's span
                for k in ("n", "n_kept", "n_unplaced"):
                    stats[k] = totals.get(k, 0)
                stats["n_counted"] = stats.get("n_counted", 0) + totals.get("n_counted", 0)
                ivs.append(acc.intervals() if sz["n_intervals"] else np.zeros(0, dtype=DEPTH_SPAN_DTYPE))
                for k in range(len(group)):
                    counts.append(acc.counts(k))
                    calls.append(acc.calls(k))
        return PileupResult(np.concatenate(ivs) if ivs else np.zeros(0, dtype=DEPTH_SPAN_DTYPE), stats, spans, names,
                            counts, calls, contig_len)


def _tally(path_or_bytes, flag_require, flag_exclude, min_mapq, window, ctx, reads_to_check):
    """flagstat's and idxstats' one pass: every window of iter_reads' walk scanned
    and counted into one accumulator in HBM (Context.tally)."""
    from .tally import TallyResult
    data = _file_array(path_or_bytes)
    with ExitStack() as stack:
        ctx = stack.enter_context(_context(ctx))
        names, contig_len, _ = file_header(ctx, data)
        acc = stack.enter_context(closing(ctx.tally(len(contig_len))))
        deliver = _adding(acc, _flag_filter(flag_require, flag_exclude, min_mapq))
        n = n_kept = 0
        for (got,) in _iter_windows(data, deliver, window, ctx=ctx, reads_to_check=reads_to_check):
            n, n_kept = n + got["n"], n_kept + got["n_kept"]
        flag, ref = acc.counts()
        return TallyResult(flag, ref, names, contig_len, n, n_kept)


def flagstat(path_or_bytes, flag_require=0, flag_exclude=0, min_mapq=0, window=None, ctx=None,
             reads_to_check=DEFAULT_READS_TO_CHECK):
    """What `samtools flagstat` reports, counted on the GPU: of the file's records with
    (flag & flag_require) == flag_require, (flag & flag_exclude) == 0 and mapq >= min_mapq (default:
    every record), how many are primary, secondary, supplementary, duplicate, mapped, paired, read1,
    read2, properly paired, mapped with their mate, singletons, or have their mate on another
    reference -- each split into QC-passed and QC-failed.  The file is walked `window` compressed
    bytes at a time (iter_reads' walk); the counts do not depend on `window`.

    Returns a tally.TallyResult: `.flag`, `.ref`, `.names`, `.lengths`, `.n_kept`,
    `.flagstat_text()` (samtools flagstat's lines) and `.idxstats_text()` (samtools idxstats')."""
    return _tally(path_or_bytes, flag_require, flag_exclude, min_mapq, window, ctx, reads_to_check)


def idxstats(path_or_bytes, flag_require=0, flag_exclude=0, min_mapq=0, window=None, ctx=None,
             reads_to_check=DEFAULT_READS_TO_CHECK):
    """What `samtools idxstats` reports, counted on the GPU from the records themselves (no index
    is read, and the file need not be sorted): per reference the records with flag 0x4 clear and
    set, and in a last bin those without a reference.  The same pass, arguments and result as
    flagstat."""
    return _tally(path_or_bytes, flag_require, flag_exclude, min_mapq, window, ctx, reads_to_check)


def stats(path_or_bytes, flag_require=0, flag_exclude=0, min_mapq=0, cycles=1024, max_insert=8000, window=None, ctx=None,
          reads_to_check=DEFAULT_READS_TO_CHECK):
    """What `samtools stats` reports about the reads themselves, counted on the GPU: of the file's
    records with (flag & flag_require) == flag_require, (flag & flag_exclude) == 0 and mapq >= min_mapq
    (default: every record) that are neither secondary nor supplementary, the read lengths, the
    qualities and the base composition per sequencing cycle (`cycles` rows; the bases of longer reads
    share a last row), the GC content per read, the insert sizes (`max_insert` bins; larger ones share
    a last bin) by pair orientation, the mapping qualities and a table of summary numbers
    (csrc/stats_core.h defines each).  The file is walked `window` compressed bytes at a time
    (iter_reads' walk) into one accumulator in HBM (Context.stats); the tables do not depend on
    `window`.

    Returns a stats.StatsResult: `.sn`, `.read_len`, `.qual`, `.base`, `.gc`, `.isize`, `.mapq`, `.n`,
    `.n_kept`, `.n_counted` and `.text()` (the report under samtools stats' section tags)."""
    from .stats import StatsResult
    data = _file_array(path_or_bytes)
    with ExitStack() as stack:
        ctx = stack.enter_context(_context(ctx))
        _, contig_len, _ = file_header(ctx, data)
        acc = stack.enter_context(closing(ctx.stats(cycles, max_insert)))
        deliver = _adding(acc, _flag_filter(flag_require, flag_exclude, min_mapq))
        tot = {"n": 0, "n_kept": 0, "n_counted": 0}
        for (got,) in _iter_windows(data, deliver, window, ctx=ctx, reads_to_check=reads_to_check):
            for k in tot:
                tot[k] += got[k]
        return StatsResult(acc.counts(), acc.cycles, acc.max_insert, tot["n"], tot["n_kept"], tot["n_counted"])


def fastq(path_or_bytes, out=None, out1=None, out2=None, out0=None, fasta=False, suffix="auto", flag_require=0,
          flag_exclude=0x900, min_mapq=0, def_qual=1, level=None, window=None, ctx=None,
          reads_to_check=DEFAULT_READS_TO_CHECK):
    """The file's records as FASTQ text -- FASTA with `fasta` -- as `samtools fastq` / `samtools
    fasta` write them, rendered on the GPU (Shard.records_fastq) a window at a time with iter_reads'
    windowing: `@NAME[/1|/2]`, the bases (reverse-complemented for a reverse-strand read), `+`, the
    qualities as min(q, 93) + 33 (reversed likewise; def_qual + 33 throughout when a record has
    none).  A record is written when (flag & flag_require) == flag_require, (flag & flag_exclude) ==
    0 (default 0x900: secondary and supplementary, samtools') and mapq >= min_mapq.  suffix: "auto"
    (/1 and /2 on paired reads), "never" (-n), "always" (-N).

    Sinks are paths or binary file objects.  `out` alone: one stream in file order.  Any of `out1`,
    `out2`, `out0`: read 1, read 2 and the other reads go to their own sinks; a class without one
    goes to `out`, or nowhere without `out`.  samtools' -s singleton file is not offered.  With
    `level` (Context.bgzf_compress's levels), or for a path ending in .gz (level 5 then), a sink
    receives BGZF members -- a valid multi-member gzip -- compressed from device memory, closed by
    one EOF member: the text does not come to the host uncompressed.

    Returns a fastq.FastqResult: .n, .n_kept, .part_bytes and .part_rows (uncompressed text bytes
    and records per class in the order read 1, read 2, others; all in entry 0 when not split), and
    .text (the text as bytes when no sink at all was given)."""
    from .fastq import FastqResult, fastq_mode
    split = any(s is not None for s in (out1, out2, out0))
    mode = fastq_mode(fasta, suffix, split)
    data = _file_array(path_or_bytes)
    f = _flag_filter(flag_require, flag_exclude, min_mapq)
    wanted = [s if s is not None else out for s in (out1, out2, out0)] if split else [out, None, None]
    collect = not split and out is None
    opened, sinks = {}, []  # a sink given twice is opened once: (file object, compression level or None)
    with ExitStack() as stack:  # (the files we open are closed first, then the context if it is ours)
        ctx = stack.enter_context(_context(ctx))
        for s in wanted:
            if s is None:
                sinks.append(None)
                continue
            key = os.fspath(s) if isinstance(s, (str, os.PathLike)) else id(s)
            if key not in opened:
                is_path = isinstance(s, (str, os.PathLike))
                name = str(key) if is_path else str(getattr(s, "name", ""))
                lv = level if level is not None else (5 if name.endswith(".gz") else None)
                opened[key] = (stack.enter_context(open(s, "wb")) if is_path else s, lv)
            sinks.append(opened[key])
        parts = []
        totals = {"n": 0, "n_kept": 0, "part_bytes": [0, 0, 0], "part_rows": [0, 0, 0]}
        plain = collect or any(lv is None for _, lv in opened.values())  # some text comes to the host as it is

        def deliver(sh, first, E, _names):
            sh.records_scan(first, E)
            got = sh.records_fastq(f, mode=mode, def_qual=def_qual, want_text=plain)
            text = got[0] if plain else None
            sz = sh.fastq_sizes
            at = 0
            for k in range(3):
                nb = sz["part_bytes"][k]
                if nb and sinks[k] is not None:
                    fh, lv = sinks[k]
                    if lv is None:
                        fh.write(text[at:at + nb].data)
                    else:
                        fh.write(ctx.bgzf_compress(sh.fastq_ptr() + at, nb, level=lv)[0][:-BGZF_EOF_BYTES].data)
                elif nb and collect:
                    parts.append(text[at:at + nb].tobytes())
                at += nb
            return [sz]

        for (sz,) in _iter_windows(data, deliver, window, ctx=ctx, reads_to_check=reads_to_check):
            totals["n"] += sz["n"]
            totals["n_kept"] += sz["n_kept"]
            for k in range(3):
                totals["part_bytes"][k] += sz["part_bytes"][k]
                totals["part_rows"][k] += sz["part_rows"][k]
        for fh, lv in opened.values():
            if lv is not None:
                fh.write(BGZF_EOF)
        return FastqResult(totals["n"], totals["n_kept"], totals["part_bytes"], totals["part_rows"],
                           b"".join(parts) if collect else None)


def _header_flat(ctx, data):
    """The BAM header's bytes (magic, text, reference dictionary: flat[0, header_end)), from the
    file's leading blocks inflated on the device."""
    size = int(data.size)
    n = min(size, 1 << 20)
    while True:
        sh = ctx.shard(np.ascontiguousarray(data[:n]), file_offset=0, file_size=size)
        try:
            sh.index(0)
            sh.inflate()
            flat = sh.read_flat(0, sh.flat_size)
        finally:
            sh.close()
        try:
            end = parse_bam_header(flat)[2]
        except (IndexError, ValueError):
            end = None
            if n >= size:
                raise
        if end is not None and end <= flat.size:
            return flat[:end].tobytes()
        if n >= size:
            raise SparkBamError(12, "truncated BAM header")
        n = min(size, n * 4)


def header_text(ctx, data):
    """The BAM header's text (the l_text bytes after the magic), from the file's leading blocks
    inflated on the device."""
    size = int(data.size)
    n = min(size, 1 << 20)
    while True:
        sh = ctx.shard(np.ascontiguousarray(data[:n]), file_offset=0, file_size=size)
        try:
            sh.index(0)
            sh.inflate()
            flat = sh.read_flat(0, sh.flat_size)
        finally:
            sh.close()
        if flat.size >= 8 and bytes(flat[:4]) != b"BAM\1":
            raise SparkBamError(1, "not a BAM file (missing BAM\\1 magic)")
        if flat.size >= 8:
            l_text = int.from_bytes(bytes(flat[4:8]), "little", signed=True)
            if 8 + l_text <= flat.size:
                return bytes(flat[8:8 + l_text])
        if n >= size:
            raise SparkBamError(12, "truncated BAM header")
        n = min(size, n * 4)


def load_bam_count(path_or_bytes, split_size=DEFAULT_SPLIT_SIZE, ctx=None, **kw):
    """sc.loadBam(path, splitSize).count (CanLoadBam.scala:196-266; CountReads)."""
    _, counts = load_splits_and_reads(path_or_bytes, split_size, ctx, **kw)
    return sum(counts)


DEFAULT_BLOCKS_SPLIT_SIZE = 2 << 20  # Blocks.apply's maxSplitSize(2 MB) (check/.../check/Blocks.scala:74-78)
STREAM_WINDOW = int(os.environ.get("SBH_STREAM_WINDOW", str(1 << 30)))  # compressed bytes per HBM window


def _file_array(path_or_bytes):
    """The whole file as numpy uint8: memory-mapped for a path (pages are read as windows
    move through HBM, never all at once)."""
    if isinstance(path_or_bytes, np.ndarray):
        return path_or_bytes
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(path_or_bytes), dtype=np.uint8)
    return np.memmap(path_or_bytes, dtype=np.uint8, mode="r")


def file_header(ctx, data):
    """Header(path) (check/.../header/Header.scala:26-60) from the file's leading blocks inflated
    on the device: (contig names, contig lengths, flat end of the header)."""
    size = int(data.size)
    n = min(size, 1 << 20)
    while True:
        sh = ctx.shard(np.ascontiguousarray(data[:n]), file_offset=0, file_size=size)
        try:
            sh.index(0)
            sh.inflate()
            try:
                return parse_bam_header(sh.read_flat(0, sh.flat_size))
            except (IndexError, ValueError):
                if n >= size:
                    raise
        finally:
            sh.close()
        n = min(size, n * 4)


def _in_ranges(ranges, x):
    return ranges is None or any(a <= x < b for a, b in ranges)


def blocks(path_or_bytes, split_size=None, ranges=None, blocks_path=None, ctx=None,
           bgzf_blocks_to_check=DEFAULT_BGZF_BLOCKS_TO_CHECK):
    """Blocks.apply (check/src/main/scala/org/hammerlab/bam/check/Blocks.scala:47-208): the BGZF
    blocks the all-positions modes examine, as (partitions, bounds) -- partitions a list of
    [Metadata, ...] per partition, bounds the [(start, end)] byte range of each.

    With a `.blocks` file (`blocks_path`, default the BAM path + ".blocks"): its blocks whose start
    lies in `ranges`, partitioned by their cumulative compressed size / split_size (:86-139).
    Without one: the file is cut every split_size bytes, the splits that meet `ranges` are kept,
    and each one's blocks are FindBlockStart(split start) then MetadataStream while the block
    start is < the split end (:141-206), found on the device (sbh_find_blocks)."""
    split = int(split_size or DEFAULT_BLOCKS_SPLIT_SIZE)
    if blocks_path is None and isinstance(path_or_bytes, (str, os.PathLike)):
        blocks_path = str(path_or_bytes) + ".blocks"
    if blocks_path is not None and os.path.exists(blocks_path):
        metas = []
        with open(blocks_path) as f:
            for line in f:
                if not line.strip():
                    continue
                parts = line.strip().split(",")
                if len(parts) != 3:
                    raise ValueError(f"Bad blocks-index line: {line.strip()}")
                m = Metadata(int(parts[0]), int(parts[1]), int(parts[2]))
                if _in_ranges(ranges, m.start):
                    metas.append(m)
        # partition = (compressed bytes of the blocks before it) / split_size; the partition count is
        # the last block's partition + 1 (as BlocksTest pins it: "block boundaries" has 5 partitions
        # for blocks at offsets 0, 25228, 50313 of 74344 bytes at a 10 KiB split size)
        out, off = [], 0
        for m in metas:
            k = off // split
            out += [[] for _ in range(k + 1 - len(out))]
            out[k].append(m)
            off += m.compressed_size
        return out, [(i * split, (i + 1) * split) for i in range(len(out))]
    data = _file_array(path_or_bytes)
    size = int(data.size)
    idxs = [i for i in range(-(-size // split))
            if ranges is None or any(a < (i + 1) * split and b > i * split and a < b for a, b in ranges)]
    with _context(ctx) as ctx:
        found = ctx.find_blocks(data, [(i * split, min(size, (i + 1) * split)) for i in idxs], bgzf_blocks_to_check)
    out = [[] for _ in idxs]
    for k, start, cs, us in found:
        if _in_ranges(ranges, start):
            out[k].append(Metadata(start, cs, us))
    return out, [(i * split, (i + 1) * split) for i in idxs]


def _all_positions(path_or_bytes, ranges, ctx, reads_to_check, split_size, blocks_path, window, **kw):
    """Blocks.apply, then every position of those blocks through sbh_check_stream (HBM windows
    of `window` compressed bytes, whatever the file size)."""
    data = _file_array(path_or_bytes)
    with _context(ctx) as ctx:
        parts, _ = blocks(path_or_bytes if not isinstance(path_or_bytes, (bytes, bytearray, memoryview))
                          else data, split_size, ranges, blocks_path, ctx)
        starts = [m.start for p in parts for m in p]
        _, contig_len, _ = file_header(ctx, data)
        return ctx.check_stream(data, contig_len, starts, window=window or STREAM_WINDOW,
                                reads_to_check=reads_to_check, **kw)


def check_bam(path_or_bytes, records=None, ranges=None, ctx=None, reads_to_check=DEFAULT_READS_TO_CHECK,
              split_size=None, blocks_path=None, window=None):
    """CheckBam -s (cli/.../check/eager/CheckBam.scala + CheckerApp.scala:65-227): the eager
    checker at every position of Blocks.apply's blocks vs the `.records` truth.  `records` is a
    list of (blockPos, offset); returns the summary numbers.  Any file size: the blocks move
    through HBM in windows (sbh_check_stream)."""
    truth = None
    if records is not None:
        truth = np.sort(np.asarray([(b << 16) | o for b, o in records], dtype=np.uint64))
    r = _all_positions(path_or_bytes, ranges, ctx, reads_to_check, split_size, blocks_path, window,
                       truth_vpos=truth)
    out = {"positions": r["positions"], "compressed": r["comp_bytes"], "n_windows": r["n_windows"]}
    if truth is None:
        return dict(out, reads=r["n_true"], true_positives=r["n_true"], false_positives=0, false_negatives=0,
                    fp_positions=[], fn_positions=[])
    if r["unknown"]:
        raise SparkBamError(19, f"{r['unknown']} .records positions are not block starts of this file")
    return dict(out, reads=r["tp"] + r["fn"], true_positives=r["tp"], false_positives=r["fp"],
                false_negatives=r["fn"], fp_positions=[Pos.from_htsjdk(int(v)) for v in r["fp_vpos"]],
                fn_positions=[Pos.from_htsjdk(int(v)) for v in r["fn_vpos"]])


def full_check(path_or_bytes, ranges=None, ctx=None, reads_to_check=DEFAULT_READS_TO_CHECK, split_size=None,
               blocks_path=None, window=None):
    """FullCheck (cli/.../check/full/FullCheck.scala:88-329) aggregation over Blocks.apply's
    blocks: Counts per numNonZeroFields, totals, and the critical (1-flag) / close (2-flag)
    positions.  Any file size (sbh_check_stream)."""
    r = _all_positions(path_or_bytes, ranges, ctx, reads_to_check, split_size, blocks_path, window, full=True)
    counts = r["counts"]
    totals = dict(zip(FLAG_NAMES, counts.sum(axis=0).astype(np.int64).tolist()))
    return {"positions": r["positions"], "compressed": r["comp_bytes"], "n_success": r["n_success"],
            "counts_by_nnz": counts, "rbe_by_nnz": r["rbe"], "totals": totals, "n_windows": r["n_windows"],
            "close": [(Pos.from_htsjdk(int(v)), int(w)) for v, w in zip(r["close_vpos"], r["close_word"])]}


def flags_of(word):
    return [FLAG_NAMES[i] for i in range(19) if word & (1 << i)]


def reads_before_error(word):
    return (word >> FULL_N_SHIFT) & 0x3FF


def word_flags_mask(word):
    return word & FULL_FLAGS_MASK


def here():
    return os.path.dirname(os.path.abspath(__file__))


def htsjdk_rewrite(path_or_bytes, out_path=None, read_ranges=None, ctx=None, level=5):
    """HTSJDKRewrite (cli/src/main/scala/org/hammerlab/bam/rewrite/HTSJDKRewrite.scala:40-67):
    the BAM's uncompressed stream -- header, then every record (or only those whose index is
    in `read_ranges`, a collection supporting `in`, like the reference's `-r` IntRanges,
    :48-58) -- re-cut into 65498-byte BGZF members on the GPU (sbh_bgzf_compress) plus the
    EOF member.  Records pass through byte-for-byte (htsjdk's decode/re-encode is the
    identity on the records of a BAM it wrote).  Returns the file bytes (numpy uint8); writes
    them to out_path when given.  The `-b`/`-i` index side-outputs are the CLI's
    `index-blocks` / `index-records` run on the result.

    The members are byte-identical to htsjdk's: cut at 65498 uncompressed bytes and each
    deflated as java.util.zip.Deflater(5, nowrap) = zlib 1.2.11 deflate_slow does (zdeflate.hip),
    so the file, `.blocks` and `.records` equal HTSJDKRewriteTest's fixtures.  `level` picks
    another zlib level (4..9, 0 = stored) or -1 for this library's faster, non-zlib coder."""
    with _Loaded(path_or_bytes, ctx) as L:
        sh = L.shard
        if read_ranges is None:
            out, _, _ = L.ctx.bgzf_compress(sh.flat_ptr(), sh.flat_size, level=level)
        else:
            flat = sh.read_flat()
            starts = sh.records(L.header_end, sh.flat_size)["flat"].astype(np.int64)
            ends = np.append(starts[1:], np.int64(sh.flat_size))
            idx = np.arange(starts.size)
            sel = np.asarray(read_ranges, dtype=np.int64) if isinstance(read_ranges, range) else \
                np.fromiter((int(i) for i in read_ranges), dtype=np.int64)  # any collection (IntRanges)
            keep = idx[np.isin(idx, sel)]
            parts = [flat[:L.header_end]] + [flat[starts[i]:ends[i]] for i in keep]
            out, _, _ = L.ctx.bgzf_compress(np.concatenate(parts), level=level)
    if out_path is not None:
        with open(out_path, "wb") as f:
            f.write(out.tobytes())
    return out
