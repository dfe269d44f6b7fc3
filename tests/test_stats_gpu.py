"""Read-level statistics on the device (sbh_records_stats_add: k_stats_rows, k_stats_bases,
k_stats_commit; sbh_stats_fetch) against the numpy restatement of stats_corpus.py on every corpus; a
failed add leaving the accumulator as it was; two shards into one accumulator; the argument and state
errors; the bundled files against the host function; api.stats in one and in several windows; and the
per-cycle tables recomputed from api.fastq's text.  Every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_bam
from pkg import sb
import record_corpus as rc
import stats_corpus as sc
from test_depth_gpu import scanned
from test_record_conformance_gpu import call
from test_tally_cpu import bundled
from walk_spy import walked

pytestmark = pytest.mark.gpu

SBH_E_ARG, SBH_E_STATE, SBH_E_BAD_RECORD = sb._lib.SBH_E_ARG, sb._lib.SBH_E_STATE, sb._lib.SBH_E_BAD_RECORD


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def counts_equal(acc, want):
    t = call(acc.counts)
    sc.tables_equal(t, want)
    sc.invariants(t, want)


def added(want):
    return {"n": want["n"], "n_kept": want["n_kept"], "n_counted": want["n_counted"]}


@pytest.mark.parametrize("name", [k for k in sc.SMALL if sc.in_file_order(sc.get(k)) and sc.get(k).starts])
def test_corpus(ctx, name):
    c, want = sc.get(name), sc.expected(name)
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts), level=1)
    acc = ctx.stats(c.cycles, c.max_insert)
    try:
        assert call(acc.add, sh, c.filter) == added(want)
        counts_equal(acc, want)
        # reset and the same rows again: the same answer; once more without a reset: twice the answer
        call(acc.reset)
        assert call(acc.add, sh, c.filter) == added(want)
        counts_equal(acc, want)
        assert call(acc.add, sh, c.filter) == added(want)
        counts_equal(acc, dict(sc.added(want, want), noq_bases=[2 * x for x in want["noq_bases"]]))
    finally:
        acc.close()
        sh.close()


@pytest.mark.parametrize("name", sc.LARGE)
def test_more_rows_than_one_grid_pass(ctx, name):
    c, want = sc.get(name), sc.expected(name)
    assert len(c.starts) > sc.BASES_PASS > sc.GRID_PASS and int(want["qual"].max()) > 65536
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts), level=1)
    acc = ctx.stats(c.cycles, c.max_insert)
    try:
        assert call(acc.add, sh) == added(want)
        counts_equal(acc, want)
        # a filter on top, row ranges on both sides of either kernel's pass edges and across them
        f = {"flag_exclude": sc.MREVERSE, "rows": [(5, 100000), (262100, 262144), (262144, 262181), (524200, 524300), (524310, 524325)]}
        w2 = sc.restate(c.flat, c.starts, c.cycles, c.max_insert, f)
        assert 0 < w2["n_kept"] < want["n_kept"]
        assert call(acc.add, sh, f) == added(w2)
        sc.tables_equal(call(acc.counts), sc.added(want, w2))
    finally:
        acc.close()
        sh.close()


def test_row_order_and_a_row_counted_again_and_again(ctx):
    """The device takes a scan's rows in file order: the reversed corpus is the same sum, and the row
    given three times is the whole scan once, then row 7 alone twice more."""
    for name, again in (("rows_reversed", 0), ("row_given_three_times", 2)):
        c, want = sc.get(name), sc.expected(name)
        file_order = sorted(set(c.starts))
        sh = scanned(ctx, c.flat, file_order[0], len(file_order))
        acc = ctx.stats(c.cycles, c.max_insert)
        try:
            kept = call(acc.add, sh)["n_kept"]
            for _ in range(again):
                kept += call(acc.add, sh, {"rows": [(7, 8)]})["n_kept"]
            assert kept == want["n_kept"]
            sc.tables_equal(call(acc.counts), want)
        finally:
            acc.close()
            sh.close()


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed_stream_leaves_the_accumulator_as_it_was(ctx, m):
    """As for the tally: no scan delivers the malformed row (the scan itself answers SBH_E_BAD_RECORD), so
    the add finds no valid scan and answers SBH_E_STATE; the good rows before it, scanned alone, count.
    (The add's own answer for such a row is the host function's in test_stats_cpu.py and the driver's
    under the sanitizers.)"""
    good, want = sc.get("qualities"), sc.expected("qualities")
    sh = scanned(ctx, good.flat, good.starts[0], len(good.starts))
    bad = ctx.shard(np.frombuffer(rc.bgzf(m.stream.flat, 65280), np.uint8).copy())
    acc = ctx.stats(good.cycles, good.max_insert)
    try:
        assert call(acc.add, sh) == added(want)
        call(bad.index, 0)
        call(bad.inflate)
        with pytest.raises(sb.SparkBamError) as e:
            call(bad.records_scan, m.stream.first, bad.flat_size)
        assert e.value.code == SBH_E_BAD_RECORD
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, bad)
        assert (e.value.code, e.value.fields) == (SBH_E_STATE, ())
        counts_equal(acc, want)
        assert call(bad.records_scan, m.stream.first, m.bad_start) == 3
        w3 = sc.restate(m.stream.flat, m.stream.starts[:3], good.cycles, good.max_insert)
        assert call(acc.add, bad) == {"n": 3, "n_kept": 3, "n_counted": 3}
        sc.tables_equal(call(acc.counts), sc.added(want, w3))
    finally:
        acc.close()
        sh.close()
        bad.close()


def test_a_refused_add_leaves_the_accumulator_as_it_was(ctx):
    """A filled accumulator, then adds that are refused for their filter: nothing gets in.  (A malformed row
    cannot reach the device add through the public calls: the test above.)"""
    good, want = sc.get("insert_sizes"), sc.expected("insert_sizes")
    sh = scanned(ctx, good.flat, good.starts[0], len(good.starts))
    acc = ctx.stats(good.cycles, good.max_insert)
    try:
        assert call(acc.add, sh) == added(want)
        for f in ({"min_mapq": 256}, {"rows": [(5, 5)]}, {"flag_require": 0x10000}):
            with pytest.raises(sb.SparkBamError) as e:
                call(acc.add, sh, f)
            assert e.value.code == SBH_E_ARG
        counts_equal(acc, want)
    finally:
        acc.close()
        sh.close()


def test_two_shards_into_one_accumulator_and_a_fetch_in_between(ctx):
    """The first and the second half of 1.bam's records as two files, each on a shard of its own."""
    _, flat, starts, _, _, first = bundled("1.bam")
    cut = starts[len(starts) // 2]
    halves = ((flat[:cut], starts[:len(starts) // 2]), (flat[:first] + flat[cut:], [s - cut + first for s in starts[len(starts) // 2:]]))
    acc = ctx.stats(200, 1000)
    try:
        so_far = None
        for part, st in halves:
            want = sc.restate(part, st, 200, 1000)
            sh = scanned(ctx, part, first, len(st))
            try:
                assert call(acc.add, sh) == added(want)
            finally:
                sh.close()  # the accumulator outlives the shard
            so_far = want if so_far is None else sc.added(so_far, want)
            sc.tables_equal(call(acc.counts), so_far)  # a fetch between the adds
        sc.tables_equal(so_far, sb.stats_host(np.frombuffer(flat, np.uint8), starts, 200, 1000)[0])
    finally:
        acc.close()


def test_argument_and_state_errors(ctx):
    c, want = sc.get("which"), sc.expected("which")
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts))
    acc = ctx.stats(c.cycles, c.max_insert)
    other = sb.Context(0)
    L = sb.lib()
    try:
        for cyc, ins in ((0, 16), (sc.STAT_CYCLES_MAX + 1, 16), (8, 0), (8, sc.STAT_INSERT_MAX + 1)):
            h, p = C.c_void_p(), sb._lib.SbhStatsParams(cyc, ins)
            assert L.sbh_stats_create(ctx.h, C.byref(p), C.byref(h)) == SBH_E_ARG and not h.value
            with pytest.raises(sb.SparkBamError) as e:
                ctx.stats(cyc, ins)
            assert e.value.code == SBH_E_ARG
        h = C.c_void_p()
        assert L.sbh_stats_create(ctx.h, None, C.byref(h)) == SBH_E_ARG and not h.value
        with pytest.raises(sb.SparkBamError) as e:
            ctx.stats(-1, 16)
        assert e.value.code == SBH_E_ARG
        assert call(acc.add, sh) == added(want)
        # any pointer of the fetch may be NULL: one table alone, nothing at all
        for k, name in enumerate(sc.TABLES):
            one = np.zeros(sc.shapes(c.cycles, c.max_insert)[name], np.uint64)
            ptrs = [None] * 7
            ptrs[k] = one.ctypes.data_as(C.c_void_p)
            assert L.sbh_stats_fetch(acc.h, *ptrs) == 0 and np.array_equal(one, want[name])
        assert L.sbh_stats_fetch(acc.h, *[None] * 7) == 0 and L.sbh_stats_fetch(None, *[None] * 7) == SBH_E_ARG
        # a shard of another context; a shard without a scan: nothing gets in
        sh2 = scanned(other, c.flat, c.starts[0], len(c.starts))
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, sh2)
        assert e.value.code == SBH_E_ARG
        sh3 = ctx.shard(np.frombuffer(rc.bgzf(c.flat, 65280), np.uint8).copy())
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, sh3)
        assert e.value.code == SBH_E_STATE
        sh3.close()
        counts_equal(acc, want)
    finally:
        other.close()
        acc.close()
        sh.close()


@pytest.mark.parametrize("name", ["2.bam", "5k.bam"])
def test_bundled_file_is_the_host_function_s(ctx, name):
    data, flat, starts, _, lens, first = bundled(name)
    u8 = np.frombuffer(flat, np.uint8)
    sh = ctx.shard(data)
    acc, small = ctx.stats(), ctx.stats(8, 16)
    try:
        call(sh.set_contigs, lens)
        info, _ = call(sh.split_records, 0, data.size, decode=False)  # the starts alone
        assert info["n"] == len(starts)
        for a, (cyc, ins) in ((acc, (1024, 8000)), (small, (8, 16))):
            for f in (None, {"flag_exclude": 0x400, "min_mapq": 1}):
                call(a.reset)
                want, n_kept, n_counted = sb.stats_host(u8, starts, cyc, ins, f)
                assert call(a.add, sh, f) == {"n": len(starts), "n_kept": n_kept, "n_counted": n_counted}
                sc.tables_equal(call(a.counts), want)
    finally:
        acc.close()
        small.close()
        sh.close()


def test_api_in_one_window_and_in_several(ctx):
    _, flat, starts, _, _, _ = bundled("5k.bam")
    u8 = np.frombuffer(flat, np.uint8)
    path = golden_bam("5k.bam")
    want, _, _ = sb.stats_host(u8, starts, 1024, 8000)
    one, w_one = walked(sb.stats, path, ctx)
    many, w_many = walked(sb.stats, path, ctx, window=100000)
    rerun, w_rerun = walked(sb.stats, path, ctx, halo=16, window=150000)
    assert len(w_one) == 1 and len(set(o for o, _ in w_many)) >= 3 and len(w_many) == len(set(o for o, _ in w_many))
    assert len(w_rerun) > len(set(o for o, _ in w_rerun)) >= 3
    for r in (one, many, rerun):
        sc.tables_equal(r.tables, want)
        assert r.n == r.n_kept == r.n_counted == 4910 and (r.cycles, r.max_insert) == (1024, 8000)
        assert r.text() == sb.stats_text(want, 1024, 8000) and r.text().startswith(b"SN\tsequences:\t4910\n")
    # filters and parameters through the same entry, in windows: the host function over the whole file
    f = {"flag_require": 0x40, "flag_exclude": 0x400, "min_mapq": 20}
    w, n_kept, n_counted = sb.stats_host(u8, starts, 50, 300, f)
    r = call(sb.stats, path, flag_require=0x40, flag_exclude=0x400, min_mapq=20, cycles=50, max_insert=300, ctx=ctx, window=120000)
    sc.tables_equal(r.tables, w)
    assert (r.n, r.n_kept, r.n_counted) == (4910, n_kept, n_counted) and r.text() == sb.stats_text(w, 50, 300)


@pytest.mark.parametrize("name", ["2.bam", "5k.bam"])
def test_per_cycle_tables_are_the_fastq_text_s(ctx, name):
    """A stage that exists already, as a second route to read_len, base and qual: FASTQ prints the reads
    as they were sequenced, the qualities as min(q, 93) + 33, /2 behind the name of a last fragment."""
    _, flat, starts, _, _, _ = bundled(name)
    flags = np.array([int.from_bytes(flat[s + 18:s + 20], "little") for s in starts])
    assert not ((flags & 0xC0) == 0xC0).any() and (flags & 1).all()  # /2 is `which` in this file
    got = call(sb.stats, golden_bam(name), flag_exclude=0x900, cycles=120, ctx=ctx)
    assert int(got.sn[sc.SN.index("no_qualities")]) == 0  # (FASTQ would print a default quality for such a read)
    lines = call(sb.fastq, golden_bam(name), flag_exclude=0x900, ctx=ctx).text.split(b"\n")
    assert lines[-1] == b"" and len(lines) == 4 * got.n_counted + 1
    want = sc.zeros(120, 8000)
    for k in range(0, len(lines) - 1, 4):
        w = 1 if lines[k].endswith(b"/2") else 0
        seq, qual = lines[k + 1], lines[k + 3]
        want["read_len"][min(len(seq), 121)] += 1
        for cyc, (b, q) in enumerate(zip(seq, qual)):
            want["base"][min(cyc, 120), b"ACGT".find(bytes((b,))) if b in b"ACGT" else 4] += 1
            want["qual"][w, min(cyc, 120), q - 33] += 1
    for k in ("read_len", "base", "qual"):
        assert np.array_equal(got.tables[k], want[k]), k


def test_no_rows(ctx):
    """A file of a header alone: the scan delivers no row, the add counts none."""
    flat = rc.header()
    sh = scanned(ctx, flat, len(flat), 0)
    acc = ctx.stats(8, 16)
    try:
        assert call(acc.add, sh) == {"n": 0, "n_kept": 0, "n_counted": 0}
        counts_equal(acc, sc.expected("rows_0"))
    finally:
        acc.close()
        sh.close()
