"""FASTQ / FASTA text on the GPU (fastq.hip: k_fastq_sizes, the scans, k_fastq_index, k_fastq_emit;
sbh_records_fastq_scan / fetch) against the library's host renderer and the restatement of
fastq_corpus.py, byte for byte and offset for offset: every corpus and variant, whole and through
97-byte BGZF members; more rows than one pass of the grid; the bundled files after a decoded scan and
after a starts-only split scan; the SAM text and BAM stream of the same scan left alone; invalidation
by a new scan; malformed streams; an open shard end; the argument errors."""
import ctypes as C

import numpy as np
import pytest

from pkg import sb
import fastq_corpus as fc
import record_corpus as rc
from test_record_conformance_gpu import call
from test_tally_cpu import bundled

pytestmark = pytest.mark.gpu

SBH_E_ARG, SBH_E_STATE, SBH_E_BAD_RECORD = sb._lib.SBH_E_ARG, sb._lib.SBH_E_STATE, sb._lib.SBH_E_BAD_RECORD
SBH_E_NEED_HALO = sb._lib.SBH_E_NEED_HALO


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def scanned(ctx, c, payload=65280, level=6):
    """The stream as a BGZF file of `payload`-byte members, resident, inflated and scanned from its
    first record."""
    sh = ctx.shard(np.frombuffer(rc.bgzf(c.flat, payload, level), np.uint8).copy())
    call(sh.index, 0)
    call(sh.inflate)
    assert call(sh.records_scan, c.starts[0] if c.starts else len(c.flat), sh.flat_size) == len(c.starts)
    return sh


def device_equals(sh, c, want, **kw):
    """The device's text, offsets, rows and sizes: the restatement's, and the host renderer's."""
    text, rec_off, rows = call(sh.records_fastq, **kw)
    assert sh.fastq_sizes == want["sizes"]
    assert rec_off.dtype == np.uint64 and rec_off.tolist() == want["rec_off"]
    assert rows.dtype == np.uint64 and rows.tolist() == want["rows"]
    assert text.dtype == np.uint8 and text.tobytes() == want["text"]
    h_text, h_off, h_rows, h_sizes = sb.fastq_host(np.frombuffer(bytes(c.flat), np.uint8), c.starts, **kw)
    assert np.array_equal(text, h_text) and np.array_equal(rec_off, h_off) and np.array_equal(rows, h_rows)
    assert sh.fastq_sizes == h_sizes
    # the text left on the device is the same text
    assert call(sh.records_fastq, want_text=False, **kw) is None and sh.fastq_sizes == want["sizes"]
    assert sh.fastq_ptr()


@pytest.mark.parametrize("payload", (65280, 97))
@pytest.mark.parametrize("name", fc.SMALL)
def test_corpus(ctx, name, payload):
    c = fc.get(name)
    sh = scanned(ctx, c, payload)
    try:
        for v, kw in enumerate(fc.VARIANTS[name]):
            device_equals(sh, c, fc.expected(name, v), **kw)
    finally:
        sh.close()


def test_more_rows_than_one_grid_pass(ctx):
    c = fc.get("grid")
    assert len(c.starts) > fc.GRID_PASS
    sh = scanned(ctx, c, level=1)
    try:
        for v, kw in enumerate(fc.VARIANTS["grid"]):
            text, rec_off, rows = call(sh.records_fastq, **kw)
            want = fc.expected("grid", v)
            assert sh.fastq_sizes == want["sizes"] and text.tobytes() == want["text"]
            assert np.array_equal(rec_off, np.asarray(want["rec_off"], np.uint64))
            assert np.array_equal(rows, np.asarray(want["rows"], np.uint64))
    finally:
        sh.close()


@pytest.mark.parametrize("name", ["2.bam", "5k.bam", "1.bam"])
def test_bundled_file_after_both_kinds_of_scan(ctx, name):
    data, flat, starts, names, lens, first = bundled(name)
    c = fc.Case(flat, starts)
    kws = ({"filter": {"flag_exclude": 0x900}}, {"split": True, "suffix": "always", "fasta": True}, {"split": True, "def_qual": 40})
    wants = [fc.restate(flat, starts, **kw) for kw in kws]
    sh = ctx.shard(data)
    try:
        call(sh.set_contigs, lens)
        info, cols = call(sh.split_records, 0, data.size, decode=False)  # the starts alone
        assert info["n"] == len(starts) and cols["flat"].tolist() == starts
        for kw, want in zip(kws, wants):
            device_equals(sh, c, want, **kw)
        assert call(sh.records_scan, first, sh.flat_size) == len(starts)  # the decoded scan
        for kw, want in zip(kws, wants):
            device_equals(sh, c, want, **kw)
    finally:
        sh.close()


def test_sam_text_and_bam_stream_are_left_alone_and_a_new_scan_invalidates(ctx):
    c = fc.get("rows_257")
    sh = scanned(ctx, c)
    L = sb.lib()
    try:
        sam, line_off = call(sh.records_sam, ["chrM", "chr10", "chr2", "chr1"])
        bam, bam_off, bam_rows = call(sh.records_bam, rc.header(), {"flag_exclude": 0x10})
        bam_ptr = sh.bam_ptr()
        device_equals(sh, c, fc.expected("rows_257", 1), **fc.VARIANTS["rows_257"][1])
        ptr = sh.fastq_ptr()
        assert ptr and sh.bam_ptr() == bam_ptr
        text2 = np.empty(sam.size, np.uint8)
        off2 = np.zeros(line_off.size, np.uint64)
        assert L.sbh_records_sam_fetch(sh.h, text2.ctypes.data_as(C.c_void_p), off2.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(text2, sam) and np.array_equal(off2, line_off)
        assert np.array_equal(call(sh.bam_read, 0, bam.size), bam)
        # the other outputs after the FASTQ text: it stays as it is
        call(sh.records_sam, [])
        call(sh.records_bam, b"", None)
        got = np.empty(sh.fastq_sizes["text_bytes"], np.uint8)
        assert L.sbh_records_fastq_fetch(sh.h, got.ctypes.data_as(C.c_void_p), None, None) == 0
        assert got.tobytes() == fc.expected("rows_257", 1)["text"]
        # a second scan: no text any more
        assert call(sh.records_scan, c.starts[3], sh.flat_size) == len(c.starts) - 3
        assert not sh.fastq_ptr()
        assert L.sbh_records_fastq_fetch(sh.h, got.ctypes.data_as(C.c_void_p), None, None) == SBH_E_STATE
        device_equals(sh, fc.Case(c.flat, c.starts[3:]), fc.restate(c.flat, c.starts[3:], fasta=True), fasta=True)
        # and a load
        call(sh.load, np.frombuffer(rc.bgzf(c.flat, 65280), np.uint8).copy(), 0)
        assert not sh.fastq_ptr()
        with pytest.raises(sb.SparkBamError) as e:
            call(sh.records_fastq)
        assert e.value.code == SBH_E_STATE
    finally:
        sh.close()


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed_stream(ctx, m):
    """No scan delivers the malformed row (the scan itself answers SBH_E_BAD_RECORD), so the FASTQ
    scan finds no valid scan and answers SBH_E_STATE, as the depth and tally adds do; the good rows
    before it, scanned alone, render.  (The call's own answer for such a row, SBH_E_BAD_RECORD {3}, is
    the host function's in test_fastq_cpu.py and the driver's under the sanitizers.)"""
    bad = ctx.shard(np.frombuffer(rc.bgzf(m.stream.flat, 65280), np.uint8).copy())
    try:
        call(bad.index, 0)
        call(bad.inflate)
        with pytest.raises(sb.SparkBamError) as e:
            call(bad.records_scan, m.stream.first, bad.flat_size)
        assert e.value.code == SBH_E_BAD_RECORD
        with pytest.raises(sb.SparkBamError) as e:
            call(bad.records_fastq)
        assert (e.value.code, e.value.fields) == (SBH_E_STATE, ()) and not bad.fastq_ptr()
        assert call(bad.records_scan, m.stream.first, m.bad_start) == 3
        c = fc.Case(m.stream.flat, list(m.stream.starts[:3]))
        device_equals(bad, c, fc.restate(c.flat, c.starts, split=True), split=True)
    finally:
        bad.close()


def test_open_shard_end(ctx):
    """A shard that holds 2.bam's first ten members only; a record straddles its end.  The call
    answers SBH_E_NEED_HALO for a row that merely runs past an open shard end (the BAM stream's
    rule), but no scan delivers such a row: the starts-only split scan asks for the halo itself
    unless two whole members lie behind the split's end (test_depth_gpu.py's test of the same
    name).  What can be seen from outside: after the refused scan there is no text, and the rows of
    the split that fits render as the restatement has them."""
    data, flat, starts, _, lens, _ = bundled("2.bam")
    sh_all = ctx.shard(data)
    call(sh_all.index, 0)
    blocks = sh_all.blocks()
    sh_all.close()
    cut_file, cut_flat = blocks[10][0], blocks[10][3]
    assert cut_flat not in starts
    sh = ctx.shard(data[:cut_file].copy(), file_offset=0, file_size=data.size)
    try:
        call(sh.set_contigs, lens)
        with pytest.raises(sb.SparkBamError) as e:
            call(sh.split_records, 0, cut_file, bgzf_blocks_to_check=2, decode=False)
        assert e.value.code == SBH_E_NEED_HALO
        with pytest.raises(sb.SparkBamError) as e:
            call(sh.records_fastq)
        assert e.value.code == SBH_E_STATE
        _, cols = call(sh.split_records, 0, blocks[8][0] + 1, bgzf_blocks_to_check=2, decode=False)
        rows = cols["flat"].tolist()
        assert rows == [s for s in starts if s < blocks[9][3]]
        device_equals(sh, fc.Case(flat, rows), fc.restate(flat, rows, split=True), split=True)
    finally:
        sh.close()


def test_argument_errors(ctx):
    c, want = fc.get("flags"), fc.expected("flags", 0)
    sh = scanned(ctx, c)
    L = sb.lib()
    try:
        device_equals(sh, c, want)
        sz = sb._lib.SbhFastqSizes()
        for mode, dq in ((16, 1), (2 | 0x80000000, 1), (2, 94), (2, -1)):
            assert L.sbh_records_fastq_scan(sh.h, None, mode, dq, C.byref(sz)) == SBH_E_ARG
        assert L.sbh_records_fastq_scan(sh.h, None, 2, 1, None) == SBH_E_ARG
        for filt in ({"min_mapq": 256}, {"rows": [(5, 5)]}, {"rows": [(5, 9), (8, 12)]}):
            with pytest.raises(sb.SparkBamError) as e:
                call(sh.records_fastq, filt)
            assert e.value.code == SBH_E_ARG
        # a refused call leaves the text of the last good one
        got = np.empty(want["sizes"]["text_bytes"], np.uint8)
        assert L.sbh_records_fastq_fetch(sh.h, got.ctypes.data_as(C.c_void_p), None, None) == 0
        assert got.tobytes() == want["text"]
        # a shard without a scan
        sh2 = ctx.shard(np.frombuffer(rc.bgzf(c.flat, 65280), np.uint8).copy())
        with pytest.raises(sb.SparkBamError) as e:
            call(sh2.records_fastq)
        assert e.value.code == SBH_E_STATE and not sh2.fastq_ptr()
        sh2.close()
    finally:
        sh.close()
