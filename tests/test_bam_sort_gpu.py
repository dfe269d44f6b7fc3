"""Shard.records_bam(order="coordinate") (sbh_records_bam_scan_order: k_sort_keys, the radix passes of
k_sort_hist / k_sort_scatter, k_sort_apply, then the gather as it is) against the host: the stream,
rec_off and rows equal sbh_bam_gather_host applied to the starts permuted by sbh_bam_sort_host --
which test_bam_sort_cpu.py holds to the numpy restatement -- on every corpus of
bam_sort_corpus.py, after each kind of scan, with filters, with a record delivered twice; the
scan-order call through the new entry; the state rules.  Every comparison is exact equality."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import golden_bam
from oracle_lib import OracleFile
from pkg import sb
import bam_gather_corpus as bc
import bam_sort_corpus as sc
import record_corpus as rc
from test_record_conformance_gpu import call

pytestmark = pytest.mark.gpu

SBH_E_ARG, SBH_E_STATE = sb._lib.SBH_E_ARG, sb._lib.SBH_E_STATE


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def want_sorted(flat, starts, head=b"", **f):
    """(stream, rec_off, rows) from the two host entry points: the filter's kept rows, sorted."""
    starts = np.asarray(starts, np.uint64)
    kept = sb.bam_gather_host(flat, starts, b"", bc.filter_dict(**f))[2].astype(np.int64)
    rows = kept[sb.bam_sort_host(flat, starts[kept]).astype(np.int64)]
    stream, off, _ = sb.bam_gather_host(flat, starts[rows], head)
    return stream, off, rows.astype(np.uint64)


def same_as_host(sh, flat, starts, head=b"", **f):
    want = want_sorted(flat, starts, head, **f)
    got = call(sh.records_bam, head, bc.filter_dict(**f), order="coordinate")
    assert got[2].tolist() == want[2].tolist() and got[1].tolist() == want[1].tolist()
    assert got[0].size == want[0].size and np.array_equal(got[0], want[0])
    assert sh.bam_size == want[0].size and sh.bam_n == len(starts) and sh.bam_n_kept == want[2].size
    return got


def scanned(ctx, s, level=6):
    sh = ctx.shard(np.frombuffer(rc.bgzf(s.flat, 65280, level), np.uint8).copy())
    call(sh.index, 0)
    call(sh.inflate)
    assert call(sh.records_scan, s.first, sh.flat_size) == len(s.starts)
    return sh


@pytest.mark.parametrize("name", sc.SMALL)
def test_corpus(ctx, name):
    s = sc.stream(name)
    sh = scanned(ctx, s)
    try:
        got = same_as_host(sh, s.flat, s.starts, rc.header())
        # the host entry is the restatement (held on the CPU); the device rows, directly
        assert np.array_equal(got[2], sc.expected_perm(name))
        # (a stable permutation is the identity exactly when the keys never descend)
        ordered = np.array_equal(sc.expected_perm(name), np.arange(len(s.starts), dtype=np.uint64))
        assert ordered == (name in ("sorted", "all_equal") or len(s.starts) < 2) and sh.bam_sorted == ordered
        if ordered:  # nothing moved: the scan-order call's result, byte for byte
            plain = call(sh.records_bam, rc.header())
            again = call(sh.records_bam, rc.header(), order="coordinate")
            for a, b in zip(plain, again):
                assert np.array_equal(a, b)
        same_as_host(sh, s.flat, s.starts, b"abc", flag_exclude=0x10, rows=[(1, 3 * len(s.starts) // 4 + 2)])
    finally:
        sh.close()


def test_grid_edge(ctx):
    """More kept rows than one grid pass of the row kernels (262144), 129 scatter tiles."""
    s = sc.stream("grid")
    n = len(s.starts)
    assert n > 1024 * 256
    sh = scanned(ctx, s, level=1)
    try:
        stream, off, rows = call(sh.records_bam, b"", order="coordinate")
        perm = sc.expected_perm("grid")
        assert np.array_equal(rows, perm) and not sh.bam_sorted
        assert np.array_equal(off, 44 * np.arange(n + 1, dtype=np.uint64))
        flat = np.frombuffer(s.flat, np.uint8)[s.first:].reshape(n, 44)
        assert np.array_equal(stream.reshape(n, 44), flat[perm.astype(np.int64)])
    finally:
        sh.close()


def test_filters_on_the_shuffled_stream(ctx):
    s = sc.stream("shuffled")
    n = len(s.starts)
    sh = scanned(ctx, s)
    try:
        same_as_host(sh, s.flat, s.starts, rc.header(), flag_exclude=0x10, rows=[(5, 70), (sc.T - 3, n - 9)])
        same_as_host(sh, s.flat, s.starts, b"", rows=bc.pattern_ranges("alternating", n))
        stream, off, rows = same_as_host(sh, s.flat, s.starts, b"hd", flag_require=0xFFFF, flag_exclude=0xFFFF)
        assert bytes(stream) == b"hd" and off.tolist() == [2] and rows.size == 0 and sh.bam_sorted
        same_as_host(sh, s.flat, s.starts, b"", rows=[(n - 1, n)])  # one row kept
        # a sub-range of the stream, and an empty scan
        assert call(sh.records_scan, int(s.starts[100]), int(s.starts[-1])) == n - 101
        same_as_host(sh, s.flat, s.starts[100:-1], b"abc")
        assert call(sh.records_scan, int(s.starts[0]), int(s.starts[0])) == 0
        stream, off, rows = same_as_host(sh, s.flat, [], b"only the head")
        assert bytes(stream) == b"only the head" and off.tolist() == [13] and sh.bam_sorted
    finally:
        sh.close()


def test_a_record_delivered_twice(ctx):
    """A regions scan whose overlapping chunks both hold a record: both copies, adjacent, in scan order."""
    s = rc.interval_stream()
    sh = scanned(ctx, s)
    try:
        chunks = [(s.first, rc.interval_start("edge")), (rc.interval_start("m_only"), sh.flat_size)]
        flats = call(sh.records_regions, chunks, list(rc.ALL_INTERVALS))["flat"].tolist()
        twice = rc.interval_start("m_only")
        assert flats.count(twice) == 2 and flats != sorted(flats)
        _, _, rows = same_as_host(sh, s.flat, flats, rc.header())
        at = [k for k, r in enumerate(rows.tolist()) if flats[r] == twice]
        assert at[1] == at[0] + 1 and rows[at[0]] < rows[at[1]]
        assert np.array_equal(rows, sc.perm_ref(s.flat, flats))
        same_as_host(sh, s.flat, flats, b"", flag_exclude=0x4)
    finally:
        sh.close()


@functools.lru_cache(maxsize=None)
def two_bam_shuffled():
    """2.bam's records in a fixed shuffled order: (file bytes, flat, starts)."""
    flat = rc.inflate_members(open(golden_bam("2.bam"), "rb").read())
    of = OracleFile(np.fromfile(golden_bam("2.bam"), dtype=np.uint8))
    _, _, first = sb.parse_bam_header(np.frombuffer(flat, np.uint8))
    starts, p = [], first
    while p < len(flat):
        starts.append(p)
        p += 4 + int.from_bytes(flat[p:p + 4], "little")
    assert len(starts) == 2500
    order = np.random.default_rng(2500).permutation(2500)
    recs = [flat[starts[i]:(starts + [len(flat)])[i + 1]] for i in order]
    out = flat[:first] + b"".join(recs)
    st = np.cumsum([first] + [len(r) for r in recs])[:-1]
    return np.frombuffer(rc.bgzf(out, 65280), np.uint8).copy(), out, st, of.contig_len


def test_after_split_records_and_batch(ctx):
    data, flat, starts, contig_len = two_bam_shuffled()
    sh = ctx.shard(data)
    try:
        call(sh.set_contigs, contig_len)
        info, cols = call(sh.split_records, 0, data.size, decode=False)
        assert info["n"] == 2500 and cols["flat"].tolist() == starts.tolist()
        head = flat[:info["first_flat"]]
        for f in ({}, {"flag_require": 0x10}, {"min_mapq": 30, "rows": [(100, 1000)]}):
            same_as_host(sh, flat, starts, head, **f)
        assert not sh.bam_sorted
        info, per, cols = call(sh.split_records_batch, sb.file_splits(data.size, 100000), decode=True)
        assert info["n"] == 2500
        same_as_host(sh, flat, cols["flat"], b"x" * 9, flag_exclude=0x10)
    finally:
        sh.close()


def test_scan_order_through_the_new_entry_and_state(ctx):
    data, flat, starts, contig_len = two_bam_shuffled()
    sh = ctx.shard(data)
    L = sb.lib()
    try:
        call(sh.index, 0)
        call(sh.inflate)
        names, _, first = sb.bam_header(sh)
        head = np.frombuffer(flat[:first], np.uint8)
        sz = sb._lib.SbhBamSizes()
        hp = head.ctypes.data_as(C.c_void_p)
        assert L.sbh_records_bam_scan_order(sh.h, hp, head.size, None, 1, C.byref(sz)) == SBH_E_STATE  # no scan yet
        with pytest.raises(sb.SparkBamError) as e:
            sh.bam_sorted
        assert e.value.code == SBH_E_STATE
        cols = call(sh.records, first, sh.flat_size)
        text, line_off = call(sh.records_sam, names)
        old = call(sh.records_bam, bytes(head), {"flag_exclude": 0x10})
        with pytest.raises(sb.SparkBamError) as e:  # the last BAM scan was in scan order
            sh.bam_sorted
        assert e.value.code == SBH_E_STATE
        f, keep = sb.records.record_filter({"flag_exclude": 0x10})
        assert L.sbh_records_bam_scan_order(sh.h, hp, head.size, C.byref(f), 0, C.byref(sz)) == 0
        assert (sz.n, sz.n_kept, sz.bytes) == (2500, old[2].size, old[0].size)
        new = (np.empty(sz.bytes, np.uint8), np.zeros(sz.n_kept + 1, np.uint64), np.zeros(sz.n_kept, np.uint64))
        assert L.sbh_records_bam_fetch(sh.h, *(a.ctypes.data_as(C.c_void_p) for a in new)) == 0
        for a, b in zip(old, new):
            assert np.array_equal(a, b)
        for order in (2, -1):
            assert L.sbh_records_bam_scan_order(sh.h, hp, head.size, None, order, C.byref(sz)) == SBH_E_ARG
        with pytest.raises(ValueError):
            sh.records_bam(b"", order="queryname")
        same_as_host(sh, flat, starts, bytes(head))
        # the scan's columns and SAM text are as they were
        again = call(sh._records_fetch, sb._lib.SbhRecordsSizes(starts.size, cols["names"].size, cols["cigar"].size,
                                                                cols["seq"].size, cols["aux"].size))
        for k in cols:
            assert np.array_equal(again[k], cols[k]), k
        text2, line_off2 = call(sh.records_sam, names)
        assert np.array_equal(text2, text) and np.array_equal(line_off2, line_off)
        # a new scan invalidates the stream and the answer
        call(sh.records_scan, int(starts[3]), sh.flat_size)
        assert not sh.bam_ptr()
        with pytest.raises(sb.SparkBamError) as e:
            sh.bam_sorted
        assert e.value.code == SBH_E_STATE
        same_as_host(sh, flat, starts[3:], b"")
    finally:
        sh.close()
