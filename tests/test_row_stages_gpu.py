"""The frame the filtered row stages share (bam_gather.hip: row_filter, stage_row_ranges, rows_verdict;
sbh_shard::row_ranges): the BAM stream, the tally, the FASTQ text, the depth and the pileup of ONE
scanned shard, alternating, each under row ranges of its own and each against its own host function;
two shards with different range counts into one tally and one depth accumulator; the one SBH_E_ARG
text of a bad filter from all five entry points, the stage's last good result still there; and a row
whose reference is out of range refused by depth, pileup and tally with the stage's own message, the
accumulator left as it was.  Every comparison is exact equality.

(The SBH_E_NEED_HALO half of rows_verdict has no test: the records scan refuses a row that runs past
the shard before any of these stages sees it -- test_fastq_gpu.py::test_open_shard_end.)"""
import ctypes as C

import numpy as np
import pytest

from pkg import sb
import pileup_corpus as pc
from test_depth_gpu import scanned
from test_record_conformance_gpu import call

pytestmark = pytest.mark.gpu

SBH_E_ARG, SBH_E_BAD_RECORD = sb._lib.SBH_E_ARG, sb._lib.SBH_E_BAD_RECORD
FILTER_TEXT = b"record filter: flags < 65536, 0 <= min_mapq <= 255, row ranges sorted, disjoint and non-empty"
UNFIT = "record %d of the scan does not fit its block or the stream"
SPANS = [(0, 0, 1000)]
N = 200  # rows of the stream: row ranges straddle the wave edges 63|64 and 127|128


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def stream():
    """pileup_corpus's 200 filter records on reference 0: valid rows for every one of the five stages."""
    c = pc.get("filter_rows")
    assert len(c.starts) == N and c.spans == SPANS
    return np.frombuffer(bytes(c.flat), np.uint8), list(c.starts)


def last_error(ctx):
    return bytes(sb.lib().sbh_last_error(ctx.h))


def host_depth(*adds):
    """The host's answer for the adds (flat, starts, filter), one after the other into one set of slots:
    (the add results, (depth, runs, sizes))."""
    slots, results = None, []
    for flat, starts, f in adds:
        add, slots = sb.depth_host(flat, starts, SPANS, pc.N_REF, f, slots=slots, finish=False)
        results.append(add)
    return results, sb.coverage.finish_host(slots, SPANS)


def depth_equals(acc, depth, runs, sizes):
    """finish and every fetch against the host's (its depth has one extra slot behind each span)."""
    assert call(acc.finish) == sizes
    assert np.array_equal(call(acc.runs), runs)
    off = 0
    for k, (_, b, e) in enumerate(SPANS):
        assert np.array_equal(call(acc.depth, k), depth[off:off + e - b])
        off += e - b + 1


def test_alternating_stages_on_one_scanned_shard(ctx, stream):
    flat, starts = stream
    head = b"head"
    f_bam = {"rows": [(0, 1), (63, 65), (N - 1, N)]}
    f_tally = {"rows": [(60, 130)], "flag_exclude": 0x4}
    f_depth = {"rows": [(0, 1), (5, 9), (63, 65), (127, 129), (N - 1, N)]}
    f_pile = {"rows": [(62, 64), (126, N)], "min_mapq": 7}
    sh = scanned(ctx, flat, starts[0], N)
    tal, dep, pil = ctx.tally(pc.N_REF), ctx.depth(SPANS, pc.N_REF), ctx.pileup(SPANS, pc.N_REF)
    try:
        bam1 = call(sh.records_bam, head, f_bam)
        for got, want in zip(bam1, sb.bam_gather_host(flat, starts, head, f_bam)):
            assert np.array_equal(got, want)
        assert bam1[2].tolist() == [0, 63, 64, N - 1]

        flag, ref, n_kept = sb.tally_host(flat, starts, pc.N_REF, f_tally)
        assert call(tal.add, sh, f_tally) == {"n": N, "n_kept": n_kept}
        got_flag, got_ref = call(tal.counts)
        assert np.array_equal(got_flag, flag) and np.array_equal(got_ref, ref)

        text, rec_off, rows = call(sh.records_fastq)  # no filter: no ranges at all
        h_text, h_off, h_rows, h_sizes = sb.fastq_host(flat, starts)
        assert np.array_equal(text, h_text) and np.array_equal(rec_off, h_off) and np.array_equal(rows, h_rows)
        assert sh.fastq_sizes == h_sizes and h_sizes["n_kept"] == N

        (add,), finished = host_depth((flat, starts, f_depth))
        assert call(dep.add, sh, f_depth) == add and add["n_kept"] == 10
        depth_equals(dep, *finished)

        h_add, h_counts, h_calls, h_iv, h_sizes = sb.pileup_host(flat, starts, SPANS, pc.N_REF, f_pile)
        assert call(pil.add, sh, f_pile) == h_add
        assert call(pil.finish) == h_sizes
        assert np.array_equal(call(pil.counts), h_counts) and np.array_equal(call(pil.calls), h_calls)
        assert np.array_equal(call(pil.intervals), h_iv)

        # the first filter again, after four other stages have staged ranges of their own
        for got, want in zip(call(sh.records_bam, head, f_bam), bam1):
            assert np.array_equal(got, want)
    finally:
        for a in (tal, dep, pil, sh):
            a.close()


def test_two_shards_with_different_range_counts_into_one_accumulator(ctx, stream):
    flat, starts = stream
    cb = pc.case(pc._filters_records()[40:180], SPANS)  # another stream: 140 of the records
    flat_b, starts_b = np.frombuffer(bytes(cb.flat), np.uint8), list(cb.starts)
    f_a = {"rows": [(0, 1), (63, 65), (100, 128), (N - 1, N)]}
    f_b = {"rows": [(60, 139)]}
    sa, shb = scanned(ctx, flat, starts[0], N), scanned(ctx, flat_b, starts_b[0], len(starts_b))
    tal, dep = ctx.tally(pc.N_REF), ctx.depth(SPANS, pc.N_REF)
    try:
        flag, ref, kept_a = sb.tally_host(flat, starts, pc.N_REF, f_a)
        flag, ref, kept_b = sb.tally_host(flat_b, starts_b, pc.N_REF, f_b, flag=flag, ref=ref)
        (add_a, add_b), finished = host_depth((flat, starts, f_a), (flat_b, starts_b, f_b))
        assert call(tal.add, sa, f_a) == {"n": N, "n_kept": kept_a} and kept_a == 32
        assert call(dep.add, sa, f_a) == add_a
        assert call(tal.add, shb, f_b) == {"n": len(starts_b), "n_kept": kept_b} and kept_b == 79
        assert call(dep.add, shb, f_b) == add_b
        got_flag, got_ref = call(tal.counts)
        assert np.array_equal(got_flag, flag) and np.array_equal(got_ref, ref)
        depth_equals(dep, *finished)
    finally:
        for a in (tal, dep, sa, shb):
            a.close()


def test_bad_filter_is_one_message_and_leaves_the_last_result(ctx, stream):
    flat, starts = stream
    good = {"rows": [(3, 70)]}
    sh = scanned(ctx, flat, starts[0], N)
    tal, dep, pil = ctx.tally(pc.N_REF), ctx.depth(SPANS, pc.N_REF), ctx.pileup(SPANS, pc.N_REF)
    try:
        bam = call(sh.records_bam, b"hd", good)
        fq = call(sh.records_fastq, good)
        fq_sizes = sh.fastq_sizes
        call(tal.add, sh, good), call(dep.add, sh, good), call(pil.add, sh, good)
        counts, table = call(tal.counts), call(pil.counts)
        for bad in ({"min_mapq": 256}, {"rows": [(5, 9), (8, 12)]}):
            for entry in (lambda: sh.records_bam(b"hd", bad), lambda: sh.records_fastq(bad), lambda: tal.add(sh, bad),
                          lambda: dep.add(sh, bad), lambda: pil.add(sh, bad)):
                with pytest.raises(sb.SparkBamError) as e:
                    call(entry)
                assert e.value.code == SBH_E_ARG and e.value.fields == () and last_error(ctx) == FILTER_TEXT
        # what each stage held before the refused calls is still there
        assert np.array_equal(call(sh.bam_read, 0, bam[0].size), bam[0])
        text = np.empty(fq_sizes["text_bytes"], np.uint8)
        rec_off, rows = np.zeros(fq_sizes["n_kept"] + 1, np.uint64), np.zeros(fq_sizes["n_kept"], np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert sb.lib().sbh_records_fastq_fetch(sh.h, p(text), p(rec_off), p(rows)) == 0
        assert np.array_equal(text, fq[0]) and np.array_equal(rec_off, fq[1]) and np.array_equal(rows, fq[2])
        for got, want in zip(call(tal.counts), counts):
            assert np.array_equal(got, want)
        assert np.array_equal(call(pil.counts), table)
        depth_equals(dep, *host_depth((flat, starts, good))[1])
    finally:
        for a in (tal, dep, pil, sh):
            a.close()


@pytest.mark.parametrize("stage, also", [("depth", ", or its CIGAR or reference is out of range"),
                                         ("pileup", ", or its CIGAR, query length or reference is out of range"),
                                         ("tally", ", or its reference is out of range")])
def test_reference_out_of_range_is_the_stage_s_bad_record(ctx, stream, stage, also):
    flat, starts = stream
    off_ref, row = pc.BAD_KEPT["ref_out_of_range"]()  # row 1 sits on reference N_REF
    good = {"rows": [(10, 70)]}
    sh = scanned(ctx, flat, starts[0], N)
    so = scanned(ctx, off_ref.flat, off_ref.starts[0], len(off_ref.starts))
    acc = {"depth": lambda: ctx.depth(SPANS, pc.N_REF), "pileup": lambda: ctx.pileup(SPANS, pc.N_REF),
           "tally": lambda: ctx.tally(pc.N_REF)}[stage]()
    try:
        call(acc.add, sh, good)
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, so)
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (row,)
        assert last_error(ctx) == ((UNFIT % row) + also).encode()
        # the accumulator holds the first add and nothing else: the host's answer for that add alone
        if stage == "depth":
            depth_equals(acc, *host_depth((flat, starts, good))[1])
        elif stage == "pileup":
            assert np.array_equal(call(acc.counts), sb.pileup_host(flat, starts, SPANS, pc.N_REF, good, finish=False)[1])
        else:
            flag, ref, _ = sb.tally_host(flat, starts, pc.N_REF, good)
            got_flag, got_ref = call(acc.counts)
            assert np.array_equal(got_flag, flag) and np.array_equal(got_ref, ref)
    finally:
        for a in (acc, sh, so):
            a.close()
