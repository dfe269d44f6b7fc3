"""Shard.records_bam(order="name") (sbh_records_bam_scan_names: k_name_scan, k_name_keys per chunk with
the radix passes of k_sort_hist / k_sort_scatter, k_sort_apply, then the gather as it is, and
k_name_groups) against the host: the stream, rec_off and rows equal sbh_bam_gather_host applied to the
starts permuted by sbh_bam_name_sort_host -- which test_name_sort_cpu.py holds to the pure-Python
restatement -- on every corpus of name_sort_corpus.py, with filters, with a record delivered twice;
the summary (bam_name_info) against the restatement's; the state rules.  Every comparison is exact
equality."""
import ctypes as C

import numpy as np
import pytest

from pkg import sb
import bam_gather_corpus as bc
import bam_sort_corpus as sc
import name_sort_corpus as nc
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
    """(stream, rec_off, rows, info) from the two host entry points: the filter's kept rows, sorted."""
    starts = np.asarray(starts, np.uint64)
    kept = sb.bam_gather_host(flat, starts, b"", bc.filter_dict(**f))[2].astype(np.int64)
    perm, info = sb.bam_name_sort_host(flat, starts[kept])
    rows = kept[perm.astype(np.int64)]
    stream, off, _ = sb.bam_gather_host(flat, starts[rows], head)
    return stream, off, rows.astype(np.uint64), info


def same_as_host(sh, flat, starts, head=b"", **f):
    """The device call against the host's; the summary against the host's and -- chunks and passes --
    against the restatement over the kept rows.  Returns (stream, rec_off, rows, info)."""
    want = want_sorted(flat, starts, head, **f)
    got = call(sh.records_bam, head, bc.filter_dict(**f), order="name")
    assert got[2].tolist() == want[2].tolist() and got[1].tolist() == want[1].tolist()
    assert got[0].size == want[0].size and np.array_equal(got[0], want[0])
    assert sh.bam_size == want[0].size and sh.bam_n == len(starts) and sh.bam_n_kept == want[2].size
    info = sh.bam_name_info
    kept_starts = np.asarray(starts, np.uint64)[np.sort(want[2].astype(np.int64))]
    ref = nc.info_ref(flat, kept_starts, device=True)
    assert info == ref and {k: v for k, v in info.items() if k not in ("chunks_run", "passes_run")} == {
        k: v for k, v in want[3].items() if k not in ("chunks_run", "passes_run")}
    return got + (info,)


def scanned(ctx, s, level=6):
    sh = ctx.shard(np.frombuffer(rc.bgzf(s.flat, 65280, level), np.uint8).copy())
    call(sh.index, 0)
    call(sh.inflate)
    assert call(sh.records_scan, s.first, sh.flat_size) == len(s.starts)
    return sh


@pytest.mark.parametrize("name", nc.SMALL)
def test_corpus(ctx, name):
    s = nc.stream(name)
    sh = scanned(ctx, s)
    try:
        got = same_as_host(sh, s.flat, s.starts, rc.header())
        # the host entry is the restatement (held on the CPU); the device rows and summary, directly
        assert np.array_equal(got[2], nc.expected_perm(name)) and got[3] == nc.expected_info(name, device=True)
        nc.check_expect(name, got[3], device=True)
        ordered = np.array_equal(nc.expected_perm(name), np.arange(len(s.starts), dtype=np.uint64))
        assert got[3]["already"] == ordered
        if ordered:  # nothing moved: the scan-order call's result, byte for byte
            assert got[3]["chunks_run"] == got[3]["passes_run"] == 0
            plain = call(sh.records_bam, rc.header())
            again = call(sh.records_bam, rc.header(), order="name")
            for a, b in zip(plain, again):
                assert np.array_equal(a, b)
        same_as_host(sh, s.flat, s.starts, b"abc", flag_exclude=0x10, rows=[(1, 3 * len(s.starts) // 4 + 2)])
    finally:
        sh.close()


def test_grid_edge(ctx):
    """More kept rows than one grid pass of the row kernels (262144), 129 scatter tiles, 6-byte names."""
    s = nc.stream("grid")
    n = len(s.starts)
    assert n > 1024 * 256
    sh = scanned(ctx, s, level=1)
    try:
        stream, off, rows = call(sh.records_bam, b"", order="name")
        perm = nc.expected_perm("grid")
        assert np.array_equal(rows, perm)
        assert np.array_equal(off, 43 * np.arange(n + 1, dtype=np.uint64))
        flat = np.frombuffer(s.flat, np.uint8)[s.first:].reshape(n, 43)
        assert np.array_equal(stream.reshape(n, 43), flat[perm.astype(np.int64)])
        info = sh.bam_name_info
        assert info == nc.expected_info("grid", device=True)
        nc.check_expect("grid", info, device=True)
    finally:
        sh.close()


def test_filters_on_the_shuffled_stream(ctx):
    s = nc.stream("shuffled")
    n = len(s.starts)
    sh = scanned(ctx, s)
    try:
        same_as_host(sh, s.flat, s.starts, rc.header(), flag_exclude=0x10, rows=[(5, 70), (nc.T - 3, n - 9)])
        same_as_host(sh, s.flat, s.starts, b"", rows=bc.pattern_ranges("alternating", n))
        stream, off, rows, info = same_as_host(sh, s.flat, s.starts, b"hd", flag_require=0xFFFF, flag_exclude=0xFFFF)
        assert bytes(stream) == b"hd" and off.tolist() == [2] and rows.size == 0
        assert info == dict(n_names=0, n_single=0, n_pair=0, n_more=0, max_name=0, chunks_run=0, passes_run=0, already=True)
        _, _, _, info = same_as_host(sh, s.flat, s.starts, b"", rows=[(n - 1, n)])  # one row kept
        assert info["n_names"] == info["n_single"] == 1 and info["already"]
        # a sub-range of the stream, and an empty scan
        assert call(sh.records_scan, int(s.starts[100]), int(s.starts[-1])) == n - 101
        same_as_host(sh, s.flat, s.starts[100:-1], b"abc")
        assert call(sh.records_scan, int(s.starts[0]), int(s.starts[0])) == 0
        stream, off, rows, info = same_as_host(sh, s.flat, [], b"only the head")
        assert bytes(stream) == b"only the head" and off.tolist() == [13] and info["already"] and info["n_names"] == 0
    finally:
        sh.close()


def test_a_record_delivered_twice(ctx):
    """A regions scan whose overlapping chunks both hold a record: both copies, adjacent, in scan order,
    and one group of two."""
    s = rc.interval_stream()
    sh = scanned(ctx, s)
    try:
        chunks = [(s.first, rc.interval_start("edge")), (rc.interval_start("m_only"), sh.flat_size)]
        flats = call(sh.records_regions, chunks, list(rc.ALL_INTERVALS))["flat"].tolist()
        twice = rc.interval_start("m_only")
        assert flats.count(twice) == 2
        _, _, rows, info = same_as_host(sh, s.flat, flats, rc.header())
        at = [k for k, r in enumerate(rows.tolist()) if flats[r] == twice]
        assert at[1] == at[0] + 1 and rows[at[0]] < rows[at[1]]
        assert np.array_equal(rows, nc.perm_ref(s.flat, flats)) and info["n_pair"] >= 1
        same_as_host(sh, s.flat, flats, b"", flag_exclude=0x4)
    finally:
        sh.close()


def test_state_and_the_other_orders(ctx):
    s = nc.stream("pairs")
    sh = scanned(ctx, s)
    L = sb.lib()
    try:
        names = [c[0] for c in rc.CONTIGS]
        head = np.frombuffer(rc.header(), np.uint8)
        hp = head.ctypes.data_as(C.c_void_p)
        sz, ni = sb._lib.SbhBamSizes(), sb._lib.SbhBamNameInfo()
        assert L.sbh_records_bam_name_info(sh.h, C.byref(ni)) == SBH_E_STATE  # no BAM scan yet
        cols = call(sh.records, s.first, sh.flat_size)
        text, line_off = call(sh.records_sam, names)
        # a scan-order and a coordinate-order scan leave no name summary
        for order in ("scan", "coordinate"):
            call(sh.records_bam, rc.header(), order=order)
            with pytest.raises(sb.SparkBamError) as e:
                sh.bam_name_info
            assert e.value.code == SBH_E_STATE
        coord = call(sh.records_bam, rc.header(), order="coordinate")
        assert not sh.bam_sorted
        by_name = same_as_host(sh, s.flat, s.starts, rc.header())
        nc.check_expect("pairs", by_name[3], device=True)
        with pytest.raises(sb.SparkBamError) as e:  # the last BAM scan was in name order
            sh.bam_sorted
        assert e.value.code == SBH_E_STATE
        already = C.c_int()
        assert L.sbh_records_bam_sorted(sh.h, C.byref(already)) == SBH_E_STATE
        # each order gives its own result, whichever ran before it
        again = call(sh.records_bam, rc.header(), order="coordinate")
        for a, b in zip(coord, again):
            assert np.array_equal(a, b)
        assert np.array_equal(coord[2], sc.perm_ref(s.flat, s.starts)) and not np.array_equal(coord[2], by_name[2])
        same_as_host(sh, s.flat, s.starts, rc.header())
        # the old entry keeps refusing the value the new order has inside the library
        assert L.sbh_records_bam_scan_order(sh.h, hp, head.size, None, 2, C.byref(sz)) == SBH_E_ARG
        with pytest.raises(ValueError):
            sh.records_bam(b"", order="queryname")
        assert sh.bam_name_info == by_name[3]  # (a call refused for its argument leaves the last stream in place)
        # the scan's columns and SAM text are as they were
        again = call(sh._records_fetch, sb._lib.SbhRecordsSizes(len(s.starts), cols["names"].size, cols["cigar"].size,
                                                                cols["seq"].size, cols["aux"].size))
        for k in cols:
            assert np.array_equal(again[k], cols[k]), k
        text2, line_off2 = call(sh.records_sam, names)
        assert np.array_equal(text2, text) and np.array_equal(line_off2, line_off)
        # a new scan voids the stream and the summary
        call(sh.records_scan, int(s.starts[3]), sh.flat_size)
        assert not sh.bam_ptr()
        with pytest.raises(sb.SparkBamError) as e:
            sh.bam_name_info
        assert e.value.code == SBH_E_STATE
        assert L.sbh_records_bam_scan_names(sh.h, hp, head.size, None, None) == SBH_E_ARG
        same_as_host(sh, s.flat, s.starts[3:], b"")
    finally:
        sh.close()
