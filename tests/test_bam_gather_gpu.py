"""Shard.records_bam (sbh_records_bam_scan: k_bam_keep, the scans, k_bam_index, k_bam_copy) against
the host gatherer sbh_bam_gather_host, which test_bam_gather_cpu.py holds to the numpy
restatement: the stream, rec_off and rows on every corpus of bam_gather_corpus.py, laid whole and
through 97-byte BGZF members, after each kind of scan; the grid edge; the state rules."""
import functools

import numpy as np
import pytest

from conftest import golden_bam
from oracle_lib import OracleFile
from pkg import sb
import bam_gather_corpus as bc
import record_corpus as rc
from test_record_conformance_gpu import call, open_shard

pytestmark = pytest.mark.gpu

SBH_E_ARG, SBH_E_STATE = sb._lib.SBH_E_ARG, sb._lib.SBH_E_STATE
PAYLOADS = (65280, 97)  # whole members, and members smaller than any record


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def built(kind, payload):
    s = dict(bc.streams() + (("interval", rc.interval_stream()),))[kind]
    data = np.frombuffer(rc.bgzf(s.flat, payload), np.uint8).copy()
    return s, data, OracleFile(data)


def same_as_host(sh, flat, starts, head=b"", **f):
    """records_bam on the shard's last scan == the host gatherer over the same rows."""
    want = sb.bam_gather_host(flat, starts, head, bc.filter_dict(**f))
    got = call(sh.records_bam, head, bc.filter_dict(**f))
    assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
    assert got[0].size == want[0].size and np.array_equal(got[0], want[0])
    assert sh.bam_size == want[0].size and sh.bam_n == len(starts) and sh.bam_n_kept == want[2].size
    return got


@pytest.mark.parametrize("payload", PAYLOADS)
@pytest.mark.parametrize("kind", ("decode", "ladder", "long"))
def test_after_records(ctx, kind, payload):
    s, data, of = built(kind, payload)
    sh = open_shard(ctx, s, data, of, "chain")
    try:
        assert call(sh.records_scan, s.first, sh.flat_size) == len(s.starts)
        n = len(s.starts)
        heads = bc.HEADS if kind == "ladder" else (bc.HEADS[0], bc.HEADS[5], rc.header())
        for head in heads:
            for pattern in bc.PATTERNS:
                same_as_host(sh, s.flat, s.starts, head, rows=bc.pattern_ranges(pattern, n))
            if kind == "ladder":
                same_as_host(sh, s.flat, s.starts, head, rows=bc.LADDER_ROWS)
        same_as_host(sh, s.flat, s.starts, b"hd", flag_require=0xFFFF, flag_exclude=0xFFFF)  # keeps none
        same_as_host(sh, s.flat, s.starts, b"", flag_require=0xFFFF, flag_exclude=1)  # head_bytes = 0, none kept
        same_as_host(sh, s.flat, s.starts, b"hd", rows=[(n - 2, n + 5), (n + 7, 2 ** 63)])  # ranges past n
        same_as_host(sh, s.flat, s.starts, rc.header(), flag_exclude=0x4, min_mapq=7)
        # a sub-range of the stream, and an empty one (n = 0)
        k = n // 2
        assert call(sh.records_scan, s.starts[k], s.starts[-1]) == n - 1 - k
        same_as_host(sh, s.flat, s.starts[k:-1], b"abc", rows=bc.pattern_ranges("alternating", n))
        assert call(sh.records_scan, s.starts[0], s.starts[0]) == 0
        stream, off, rows = same_as_host(sh, s.flat, [], b"only the head")
        assert bytes(stream) == b"only the head" and off.tolist() == [13] and rows.size == 0
        same_as_host(sh, s.flat, [], b"")
    finally:
        sh.close()


OVERLAP = "overlapping_chunks"


@pytest.mark.parametrize("payload", PAYLOADS)
def test_after_records_regions(ctx, payload):
    """The rows a region scan delivers, in its order -- a record that two overlapping chunks both
    hold is delivered twice and written twice."""
    s, data, of = built("interval", payload)
    sh = open_shard(ctx, s, data, of, "chain")
    try:
        whole = [(s.first, sh.flat_size)]
        cases = [(c.name, whole, c.intervals) for c in rc.INTERVAL_CASES]
        cases += [(c.name, rc.chunk_flats(c), rc.ALL_INTERVALS) for c in rc.CHUNK_CASES]
        cases += [(OVERLAP, [(s.first, rc.interval_start("edge")), (rc.interval_start("m_only"), sh.flat_size)],
                   rc.ALL_INTERVALS)]
        for name, chunks, intervals in cases:
            flats = call(sh.records_regions, chunks, list(intervals))["flat"].tolist()
            if name == OVERLAP:
                assert flats.count(rc.interval_start("m_only")) == 2 and flats != sorted(flats)
            for f in ({}, {"flag_exclude": 0x4}, {"rows": bc.pattern_ranges("alternating", len(flats))}):
                same_as_host(sh, s.flat, flats, rc.header(), **f)
    finally:
        sh.close()


@functools.lru_cache(maxsize=None)
def two_bam():
    data = np.fromfile(golden_bam("2.bam"), dtype=np.uint8)
    return data, OracleFile(data)


def test_after_split_records_without_decode(ctx):
    data, of = two_bam()
    sh = ctx.shard(data)
    try:
        call(sh.set_contigs, of.contig_len)
        info, cols = call(sh.split_records, 0, data.size, decode=False)
        assert info["n"] == 2500
        flat = call(sh.read_flat)
        for f in ({}, {"flag_require": 0x10}, {"min_mapq": 30}, {"rows": [(100, 1000)]}):
            same_as_host(sh, flat, cols["flat"], bytes(flat[:info["first_flat"]]), **f)
    finally:
        sh.close()


@pytest.mark.parametrize("decode", (False, True))
def test_after_split_records_batch(ctx, decode):
    data, of = two_bam()
    sh = ctx.shard(data)
    try:
        call(sh.set_contigs, of.contig_len)
        splits = sb.file_splits(data.size, 100000)
        info, per, cols = call(sh.split_records_batch, splits, decode=decode)
        assert info["n"] == 2500 and all(p["status"] == 0 for p in per)
        flat = call(sh.read_flat)
        for f in ({}, {"flag_require": 0x40, "flag_exclude": 0x10}, {"rows": bc.pattern_ranges("blocks63", 2500)}):
            same_as_host(sh, flat, cols["flat"], b"x" * 9, **f)
    finally:
        sh.close()


def test_grid_edge(ctx):
    """More rows than one pass of k_bam_keep / k_bam_heads / k_bam_index takes (1024 workgroups
    of 256 lanes = 262144 rows) and more output than one pass of k_bam_copy (2048 workgroups of
    256 granules of 16 bytes = 8 MiB): rc.grid_stream()'s 262181 records of 44 bytes."""
    s, a = rc.grid_stream()
    n = rc.GRID_RECORDS
    assert n > 1024 * 256 and 44 * n > 2048 * 256 * 16
    data = np.frombuffer(rc.bgzf(s.flat, 65280, level=1), np.uint8).copy()
    flat = np.frombuffer(s.flat, np.uint8)
    sh = ctx.shard(data)
    try:
        call(sh.index, 0)
        call(sh.inflate)
        assert call(sh.records_scan, s.first, sh.flat_size) == n
        stream, off, rows = call(sh.records_bam, rc.header())
        assert np.array_equal(stream, flat) and np.array_equal(rows, np.arange(n, dtype=np.uint64))
        assert np.array_equal(off, s.starts.astype(np.uint64).tolist() + [len(s.flat)])
        # flag 0x10 is set on the odd rows: runs of one record each, past both grids as well
        stream, off, rows = call(sh.records_bam, b"abcde", {"flag_exclude": 0x10})
        assert np.array_equal(rows, np.arange(0, n, 2, dtype=np.uint64))
        assert np.array_equal(off, 5 + 44 * np.arange(rows.size + 1, dtype=np.uint64))
        assert bytes(stream[:5]) == b"abcde"
        assert np.array_equal(stream[5:].reshape(-1, 44), a.view(np.uint8).reshape(n, 44)[::2])
        # the last rows alone: a range that begins past the first pass of the row kernels
        stream, off, rows = call(sh.records_bam, b"", {"rows": [(262144, n + 9)]})
        assert rows.tolist() == list(range(262144, n)) and np.array_equal(stream, flat[int(s.starts[262144]):])
    finally:
        sh.close()


def test_state_rules(ctx):
    data, of = two_bam()
    sh = ctx.shard(data)
    try:
        call(sh.index, 0)
        call(sh.inflate)
        flat = call(sh.read_flat)
        names, _, first = sb.bam_header(sh)
        with pytest.raises(sb.SparkBamError) as e:
            call(sh.records_bam, b"")  # no scan yet
        assert e.value.code == SBH_E_STATE and not sh.bam_ptr()
        cols = call(sh.records, first, sh.flat_size)
        starts = cols["flat"]
        assert starts.size == 2500
        text, line_off = call(sh.records_sam, names)
        head = bytes(flat[:first])
        same_as_host(sh, flat, starts, head, flag_require=0x10)
        assert sh.bam_ptr()
        # the scan's rows, columns and SAM state are as they were
        again = call(sh._records_fetch, sb._lib.SbhRecordsSizes(starts.size, cols["names"].size, cols["cigar"].size,
                                                                cols["seq"].size, cols["aux"].size))
        for k in cols:
            assert np.array_equal(again[k], cols[k]), k
        text2, line_off2 = call(sh.records_sam, names)
        assert np.array_equal(text2, text) and np.array_equal(line_off2, line_off)
        assert call(sh.bam_read, 0, first).tobytes() == head
        assert call(sh.bam_read, sh.bam_size - 7, sh.bam_size).size == 7
        # a new scan invalidates the stream; the next records_bam refreshes it
        call(sh.records_scan, int(starts[3]), sh.flat_size)
        assert not sh.bam_ptr()
        with pytest.raises(sb.SparkBamError) as e:
            call(sh.bam_read, 0, 1)
        assert e.value.code == SBH_E_STATE
        got = same_as_host(sh, flat, starts[3:], b"")
        assert sh.bam_ptr() and bytes(got[0][:4]) == bytes(flat[int(starts[3]):int(starts[3]) + 4])
    finally:
        sh.close()


@pytest.mark.parametrize("f", [
    {"rows": [(5, 9), (0, 3)]}, {"rows": [(0, 5), (4, 9)]}, {"rows": [(3, 3)]},
    {"flag_require": 65536}, {"flag_exclude": 65536}, {"min_mapq": -1}, {"min_mapq": 256},
], ids=str)
def test_bad_filters_are_arg_errors(ctx, f):
    s, data, of = built("decode", 65280)
    sh = open_shard(ctx, s, data, of, "chain")
    try:
        call(sh.records_scan, s.first, sh.flat_size)
        with pytest.raises(sb.SparkBamError) as e:
            call(sh.records_bam, b"", f)
        assert e.value.code == SBH_E_ARG
        same_as_host(sh, s.flat, s.starts, b"")  # the shard still answers
    finally:
        sh.close()
