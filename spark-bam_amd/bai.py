"""BAI construction on the GPU: the index samtools / htslib writes for a coordinate-sorted BAM.

`build_bai` keeps the per-record work on the device (Shard.bai_scan -> sbh_bai_scan: bins,
runs of equal (ref_id, bin) as chunks, the linear-index minima; bai.hip) and finishes on the
host with one sbh_bai_build call (htslib's compress_binning, chunk merging, backward fill and
the BAI layout).  With `window` the file moves through one reused shard a window at a time,
cut at record boundaries along the chain; the runs are concatenated, the linear-index arrays
reduced by element-wise minimum, and the finisher coalesces the run a seam cut in two, so the
bytes equal the whole-file result.

Bins are written in ascending id with the metadata pseudo-bin last (htslib writes its hash
order), so the result parses equal to samtools' `.bai` without being byte-equal to it.
"""
import ctypes as C

import numpy as np

from ._lib import SBH_E_NEED_HALO, SBH_E_UNSORTED, SBH_OK, SparkBamError, error_for, lib
from .api import (DEFAULT_READS_TO_CHECK, STREAM_WINDOW, Pos, _file_array, bam_header, file_header)
from .device import BAI_RUN_DTYPE, Context, _ptr


def bai_build(runs, lin, contig_len, n_no_coor=0):
    """sbh_bai_build (host only, no GPU): runs (BAI_RUN_DTYPE, file order; several scans'
    runs concatenated), lin (their element-wise minimum), the contig lengths and the count of
    records without a reference -> the `.bai` bytes."""
    runs = np.ascontiguousarray(runs, dtype=BAI_RUN_DTYPE)
    lin = np.ascontiguousarray(lin, dtype=np.uint64)
    cl = np.ascontiguousarray(np.asarray(contig_len, dtype=np.int32))
    cap = int(lib().sbh_bai_bound(int(runs.size), int(lin.size), int(cl.size)))
    out = np.empty(cap, dtype=np.uint8)
    size = C.c_uint64()
    rc = lib().sbh_bai_build(_ptr(runs) if runs.size else None, int(runs.size), _ptr(lin) if lin.size else None,
                             _ptr(cl) if cl.size else None, int(cl.size), int(n_no_coor), _ptr(out), cap,
                             C.byref(size))
    if rc != SBH_OK:
        raise error_for(rc, "sbh_bai_build")
    return out[:size.value].tobytes()


def resident_window(size):
    """The `window` build_bai takes for a file of `size` compressed bytes: None (whole file
    resident) up to sharded.RESIDENT_MAX, the streaming window above it."""
    from . import sharded
    return None if size <= sharded.RESIDENT_MAX else STREAM_WINDOW


def _stream_end(sh, from_flat):
    """Flat end of the BAM stream in the shard: the first empty block at/after from_flat ends it."""
    b = sh.block_arrays()
    hit = np.flatnonzero((b["flags"] & 1 != 0) & (b["ustart"] >= np.uint64(from_flat)))
    return (int(b["ustart"][hit[0]]), True) if hit.size else (sh.flat_size, False)


def build_bai(path_or_bytes, ctx=None, window=None, halo=4 << 20, reads_to_check=DEFAULT_READS_TO_CHECK):
    """The `.bai` of a coordinate-sorted BAM (a path, bytes or a numpy uint8 array) as bytes.
    window=None: the whole file resident on the device.  window=N: the file moves through one
    reused shard in windows of about N compressed bytes (plus a halo that grows x4 while a
    record or an eager check runs past it).  Raises SparkBamError with SBH_E_UNSORTED (fields:
    the first offending record's virtual offset) for a file that is not coordinate-sorted."""
    data = _file_array(path_or_bytes)
    size = int(data.size)
    own_ctx = ctx is None
    ctx = ctx or Context(0)
    try:
        if window is None:
            sh = ctx.shard(data)
            try:
                sh.index(0)
                sh.inflate()
                _, contig_len, header_end = bam_header(sh)
                sh.set_contigs(contig_len)
                end, _ = _stream_end(sh, header_end)
                if end > header_end:
                    sh.check_eager(header_end, end, reads_to_check, want_bits=False)
                runs, lin, n_no_coor = sh.bai_scan(header_end, end)
            finally:
                sh.close()
            return bai_build(runs, lin, contig_len, n_no_coor)
        return _build_windowed(ctx, data, size, int(window), int(halo), reads_to_check)
    finally:
        if own_ctx:
            ctx.close()


def _build_windowed(ctx, data, size, window, halo, reads_to_check):
    _, contig_len, header_end = file_header(ctx, data)
    all_runs, lin, n_no_coor = [], None, 0
    prev = None  # (ref_id, pos) of the last record with a reference so far
    lo, start, sh = 0, None, None
    try:
        while lo < size:
            hi = lo + window
            while True:
                end = min(size, hi + halo)
                comp = np.ascontiguousarray(data[lo:end])
                try:
                    if sh is None:
                        sh = ctx.shard(comp, file_offset=lo, file_size=size)
                        sh.set_contigs(contig_len)
                    else:
                        sh.load(comp, lo)
                    sh.index(lo)
                    sh.inflate()
                    E = sh.flat_bound(hi)
                    if end < size and E == sh.flat_size:
                        raise SparkBamError(SBH_E_NEED_HALO, "no block past the window in the halo")
                    f = header_end if start is None else sh.flat_of(start >> 16, start & 0xFFFF)
                    seg, ended = _stream_end(sh, f)
                    last = ended and seg <= E or end == size and E == sh.flat_size
                    E = min(E, seg)
                    if E > f:
                        sh.check_eager(f, E, reads_to_check, want_bits=False)
                    runs, wlin, nnc = sh.bai_scan(f, E)
                    edges = sh.bai_edges()
                    n, x = sh.chain_from(f, E) if E > f else (0, f)
                    if not last and x >= sh.flat_size:
                        raise SparkBamError(SBH_E_NEED_HALO, "the chain leaves the halo")
                    first_v = int(Pos(*sh.pos_of(f)).to_htsjdk()) if n else 0
                    nxt = None if last else int(Pos(*sh.pos_of(x)).to_htsjdk())
                    break
                except SparkBamError as err:
                    if err.code != SBH_E_NEED_HALO or end >= size:
                        raise
                    halo *= 4
            # the ordering check across the seam (inside a window the device makes it)
            if n and edges[0] >= 0 and (n_no_coor or (prev is not None and (edges[0], edges[1]) < prev)):
                raise SparkBamError(SBH_E_UNSORTED, f"record at {first_v >> 16}:{first_v & 0xFFFF} is out of "
                                                    "coordinate order", (first_v,))
            if edges[2] >= 0:
                prev = (edges[2], edges[3])
            all_runs.append(runs)
            lin = wlin if lin is None else np.minimum(lin, wlin)
            n_no_coor += nnc
            if last:
                break
            start, lo = nxt, nxt >> 16
    finally:
        if sh is not None:
            sh.close()
    runs = np.concatenate(all_runs) if all_runs else np.zeros(0, BAI_RUN_DTYPE)
    if lin is None:
        lin = np.full(int(sum((int(x) >> 14) + 2 for x in contig_len)), np.iinfo(np.uint64).max, np.uint64)
    return bai_build(runs, lin, contig_len, n_no_coor)


def write_bai(path, out=None, ctx=None, window=None):
    """Build the index of the BAM at `path` and write it to `out` (default: path + ".bai").
    A file larger than the resident limit is built in windows.  Returns the output path."""
    import os

    if window is None:
        window = resident_window(os.path.getsize(path))
    b = build_bai(path, ctx=ctx, window=window)
    out = str(path) + ".bai" if out is None else out
    with open(out, "wb") as f:
        f.write(b)
    return out
