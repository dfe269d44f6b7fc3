"""Per-base allele counts on the device (sbh_records_pileup_add: k_pile_check, k_pile_events;
sbh_pileup_finish: k_pile_calls, k_pile_fold, k_pile_intervals) against the numpy restatement of
pileup_corpus.py: the add's counts, the table, the calls, the intervals and the stats on every
corpus; the hand-worked table; the existing depth code as an independent check on every corpus and
bundled file; a failed add leaving the table as it was; two shards into one accumulator; the state
rules; the bundled files with literal expected numbers; api.pileup in several windows and passes, and with a
window that runs twice.
Every comparison is exact equality."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import golden_bam
from pkg import sb
import pileup_corpus as pc
import record_corpus as rc
from test_depth_gpu import call, fixture, scanned
from walk_spy import walked

pytestmark = pytest.mark.gpu

SBH_E_ARG, SBH_E_STATE, SBH_E_BAD_RECORD = sb._lib.SBH_E_ARG, sb._lib.SBH_E_STATE, sb._lib.SBH_E_BAD_RECORD
EXCLUDE = {"flag_exclude": 0x704}


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def counts_equal(acc, want, spans):
    for k, a, b in pc.span_slices(spans):
        got = call(acc.counts, k)
        assert got.dtype == np.uint32 and got.shape == (b - a, 8) and np.array_equal(got, want["counts"][a:b])


def finished_equals(acc, want, spans, min_depth=1, call_pct=75):
    """finish + every fetch against the restatement's counts, calls, intervals and stats."""
    sizes = call(acc.finish, min_depth, call_pct)
    assert sizes == want["stats"]
    ivs = call(acc.intervals)
    assert ivs.dtype == pc.SPAN_DTYPE and np.array_equal(ivs, want["intervals"])
    counts_equal(acc, want, spans)
    for k, a, b in pc.span_slices(spans):
        got = call(acc.calls, k)
        assert got.dtype == np.uint8 and np.array_equal(got, want["calls"][a:b])
    if ivs.size > 2:  # a slice of the intervals, of the calls, of the counts
        assert np.array_equal(call(acc.intervals, 1, ivs.size - 2), want["intervals"][1:-1])
    _, b, e = spans[0]
    if e - b > 2:
        assert np.array_equal(call(acc.calls, 0, 1, e - b - 2), want["calls"][1:e - b - 1])
        assert np.array_equal(call(acc.counts, 0, 1, e - b - 2), want["counts"][1:e - b - 1])
    assert acc.device_ptr(0)
    return sizes


def depth_agrees(ctx, sh, spans, n_ref, filter, want):
    """The same rows, filter and spans through sbh_depth: A+C+G+T+N+LOWQ is its depth, + DEL its
    depth with D counted; covered and the sum are its stats."""
    cnt = want["counts"]
    for count_del, cols in ((False, [0, 1, 2, 3, 4, 7]), (True, [0, 1, 2, 3, 4, 5, 7])):
        d = ctx.depth(spans, n_ref, count_del)
        try:
            call(d.add, sh, filter)
            sizes = call(d.finish)
            per_pos = cnt[:, cols].sum(axis=1)
            for k, a, b in pc.span_slices(spans):
                assert np.array_equal(call(d.depth, k), per_pos[a:b])
            assert sizes["sum"] == int(per_pos.sum())
            if not count_del:
                assert sizes["covered"] == want["stats"]["covered"] and sizes["max_depth"] == want["stats"]["max_depth"]
        finally:
            d.close()


def finished(counts, spans):
    """The restatement's finish of a count table, the table with it."""
    return dict(pc.finish(counts, spans), counts=counts)


def in_file_order(c):
    return list(c.starts) == sorted(set(c.starts))


@pytest.mark.parametrize("name", [k for k in pc.SMALL if in_file_order(pc.get(k))])
def test_corpus(ctx, name):
    c, want = pc.get(name), pc.expected(name)
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts))
    acc = ctx.pileup(c.spans, pc.N_REF, c.min_baseq)
    try:
        add = call(acc.add, sh, c.filter)
        assert add == want["add"]
        counts_equal(acc, want, c.spans)  # (before the finish too)
        sizes = finished_equals(acc, want, c.spans, c.min_depth, c.call_pct)
        assert sizes["totals"] == add["totals"]
        depth_agrees(ctx, sh, c.spans, pc.N_REF, c.filter, want)
        # reset and the same rows again: the same answer
        call(acc.reset)
        assert call(acc.add, sh, c.filter) == want["add"]
        assert call(acc.finish, c.min_depth, c.call_pct) == want["stats"]
        assert np.array_equal(call(acc.intervals), want["intervals"])
    finally:
        acc.close()
        sh.close()


def test_the_hand_worked_case(ctx):
    h, c = pc.HAND, pc.hand_case()
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts))
    acc = ctx.pileup(c.spans, pc.N_REF, c.min_baseq)
    try:
        assert call(acc.add, sh) == h["add"]
        assert call(acc.finish, c.min_depth, c.call_pct) == h["stats"]
        assert call(acc.counts).tolist() == h["table"] and call(acc.calls).tobytes() == h["calls"]
        assert [(x[0], x[2], x[3]) for x in call(acc.intervals).tolist()] == h["intervals"]
    finally:
        acc.close()
        sh.close()


def test_twenty_thousand_reads_on_one_place(ctx):
    c, want = pc.get("contention"), pc.expected("contention")
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts))
    acc = ctx.pileup(c.spans, pc.N_REF, c.min_baseq)
    try:
        assert call(acc.add, sh) == want["add"]
        got = call(acc.counts, 0, 1000, 103)
        assert got.sum(axis=1).tolist() == [20000] * 52 + [40000] + [20000] * 50
        assert sorted(set(got.ravel().tolist())) == [0, 20000]
    finally:
        acc.close()
        sh.close()


def test_grid_edge(ctx):
    """More rows than one grid pass of the row kernels (262144)."""
    c, want = pc.get("grid"), pc.expected("grid")
    assert len(c.starts) > 1024 * 256
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts), level=1)
    acc = ctx.pileup(c.spans, pc.N_REF)
    try:
        assert call(acc.add, sh) == want["add"]
        f = {"rows": [(5, 100000), (262100, 262181)]}
        w2 = pc.restate(c.flat, c.starts, c.spans, pc.N_REF, f)
        assert call(acc.add, sh, f) == w2["add"]
        finished_equals(acc, finished(want["counts"] + w2["counts"], c.spans), c.spans)
    finally:
        acc.close()
        sh.close()


def test_rows_counted_again_and_again(ctx):
    """The whole scan once, then row 7 alone three times more: the corpus's reversed-and-tripled rows."""
    c, want = pc.get("rows_reversed_and_tripled"), pc.expected("rows_reversed_and_tripled")
    file_order = sorted(set(c.starts))
    sh = scanned(ctx, c.flat, file_order[0], len(file_order))
    acc = ctx.pileup(c.spans, pc.N_REF)
    try:
        totals = call(acc.add, sh)["totals"]
        for _ in range(3):
            totals = [a + b for a, b in zip(totals, call(acc.add, sh, {"rows": [(7, 8)]})["totals"])]
        assert finished_equals(acc, want, c.spans)["totals"] == totals == want["add"]["totals"]
    finally:
        acc.close()
        sh.close()


@pytest.mark.parametrize("name", pc.BAD_KEPT)
def test_failed_add_leaves_the_accumulator_as_it_was(ctx, name):
    good, want = pc.get("composite"), pc.expected("composite")
    bad, row = pc.BAD_KEPT[name]()
    sh = scanned(ctx, good.flat, good.starts[0], len(good.starts))
    sb_ = scanned(ctx, bad.flat, bad.starts[0], len(bad.starts))
    acc = ctx.pileup(good.spans, pc.N_REF, good.min_baseq)
    try:
        assert call(acc.add, sh) == want["add"]
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, sb_)
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (row,)
        counts_equal(acc, want, good.spans)
        # dropped by the filter, the same row is no error
        assert call(acc.add, sb_, {"rows": [(row, row + 1)], "flag_require": 0x10})["n_kept"] == 0
        finished_equals(acc, want, good.spans, good.min_depth, good.call_pct)
    finally:
        acc.close()
        sh.close()
        sb_.close()


@functools.lru_cache(maxsize=None)
def fixture_want(name, min_baseq=0, min_depth=1, call_pct=75):
    """The restatement over the stretch [lo, hi) of reference 0 that holds every record."""
    _, flat, starts, _, lens, _ = fixture(name)
    u8 = np.frombuffer(flat, np.uint8)
    st = np.asarray(starts, np.int64)
    pos = pc._i32(u8, st + 8)[pc._i32(u8, st + 4) == 0]
    lo, hi = max(int(pos.min()) - 1, 0), int(pos.max()) + 2000
    assert 0 < lo and hi < lens[0]
    want = pc.restate(flat, starts, [(0, lo, hi)], len(lens), EXCLUDE, min_baseq, min_depth, call_pct)
    assert not want["counts"][0].any() and not want["counts"][-1].any()
    return want, (lo, hi)


# Per-channel totals (A C G T N DEL INS LOWQ) over reference 0 with flag_exclude 0x704, at min_baseq 0
# and 13, and the positions with depth >= 1.  They come from a plain walk of the records in Python:
# one loop over the inflated file's records, one over each record's CIGAR words, one over each op's
# bases, reading the nibble and the quality byte by index and adding 1 to a list -- no numpy.  The
# sums of the first five at min_baseq 0 are the depth suite's literals 230383 / 449355 / 281810.
FIXTURE_NUMBERS = {
    "2.bam": ([51080, 60760, 65050, 53491, 2, 21, 5, 0], [48910, 57704, 61554, 51680, 0, 21, 5, 10535], 12339),
    "5k.bam": ([99516, 123344, 117839, 108653, 3, 59, 10, 0], [95848, 117665, 112106, 105008, 0, 59, 10, 18728], 18441),
    "1.bam": ([84865, 62406, 59728, 74787, 24, 27, 7, 0], [84506, 62001, 59438, 74432, 0, 27, 7, 1433], 8511),
}
DEPTH_SUMS = {"2.bam": 230383, "5k.bam": 449355, "1.bam": 281810}


@pytest.mark.parametrize("name", FIXTURE_NUMBERS)
def test_bundled_file_after_both_kinds_of_scan(ctx, name):
    data, flat, starts, names, lens, first = fixture(name)
    t0, t13, covered = FIXTURE_NUMBERS[name]
    want, (lo, hi) = fixture_want(name)
    want13, _ = fixture_want(name, 13, 3, 80)
    assert want["add"]["totals"] == t0 and want13["add"]["totals"] == t13
    assert sum(t0[:5]) + t0[7] == DEPTH_SUMS[name] == sum(t13[:5]) + t13[7] and want["stats"]["covered"] == covered
    spans = [(0, lo, hi)]
    sh = ctx.shard(data)
    acc, acc13 = ctx.pileup(spans, len(lens)), ctx.pileup(spans, len(lens), 13)
    try:
        call(sh.set_contigs, lens)
        info, cols = call(sh.split_records, 0, data.size, decode=False)  # the starts alone
        assert info["n"] == len(starts) and cols["flat"].tolist() == starts
        assert call(acc.add, sh, EXCLUDE) == want["add"]
        assert call(acc13.add, sh, EXCLUDE)["totals"] == t13
        sizes = finished_equals(acc, want, spans)
        assert sizes["totals"] == t0 and sizes["covered"] == covered
        finished_equals(acc13, want13, spans, 3, 80)
        depth_agrees(ctx, sh, spans, len(lens), EXCLUDE, want)
        depth_agrees(ctx, sh, spans, len(lens), EXCLUDE, want13)
        call(acc.reset)
        assert call(sh.records_scan, first, sh.flat_size) == len(starts)  # the decoded scan
        assert call(acc.add, sh, EXCLUDE) == want["add"]
        finished_equals(acc, want, spans)
    finally:
        acc.close()
        acc13.close()
        sh.close()


def test_two_shards_into_one_accumulator(ctx):
    """The first and the second half of 2.bam's records as two files, each on a shard of its own."""
    _, flat, starts, _, lens, first = fixture("2.bam")
    want, (lo, hi) = fixture_want("2.bam")
    cut = starts[len(starts) // 2]
    halves = (flat[:cut], flat[:first] + flat[cut:])
    acc = ctx.pileup([(0, lo, hi)], len(lens))
    try:
        adds = []
        for part, n in zip(halves, (len(starts) // 2, len(starts) - len(starts) // 2)):
            sh = scanned(ctx, part, first, n)
            try:
                adds.append(call(acc.add, sh, EXCLUDE))
            finally:
                sh.close()  # the accumulator outlives the shard
        for k in ("n", "n_kept", "n_counted", "n_unplaced"):
            assert adds[0][k] + adds[1][k] == want["add"][k]
        assert [a + b for a, b in zip(adds[0]["totals"], adds[1]["totals"])] == want["add"]["totals"]
        finished_equals(acc, want, [(0, lo, hi)])
    finally:
        acc.close()


def test_state_rules(ctx):
    c, want = pc.get("composite"), pc.expected("composite")
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts))
    acc = ctx.pileup(c.spans, pc.N_REF, c.min_baseq)
    other = sb.Context(0)
    L = sb.lib()
    try:
        with pytest.raises(sb.SparkBamError) as e:  # call and interval fetches before finish
            call(acc.calls, 0)
        assert e.value.code == SBH_E_STATE
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.intervals)
        assert e.value.code == SBH_E_STATE
        assert not call(acc.counts, 0).any()  # (the counts may be fetched at any time)
        assert call(acc.add, sh) == want["add"]
        for md, pct in ((0, 75), (1, 0), (1, 101)):
            with pytest.raises(sb.SparkBamError) as e:
                call(acc.finish, md, pct)
            assert e.value.code == SBH_E_ARG
        assert call(acc.finish, c.min_depth, c.call_pct) == want["stats"]
        with pytest.raises(sb.SparkBamError) as e:  # an add after finish
            call(acc.add, sh)
        assert e.value.code == SBH_E_STATE
        with pytest.raises(sb.SparkBamError) as e:  # a second finish
            call(acc.finish)
        assert e.value.code == SBH_E_STATE
        assert np.array_equal(call(acc.intervals), want["intervals"])  # (the refused calls changed nothing)
        counts_equal(acc, want, c.spans)
        out = np.zeros((300, 8), np.uint32)
        for span, start, n in ((1, 0, 1), (0, 0, 201), (0, 200, 1), (0, 201, 0)):
            assert L.sbh_pileup_counts_fetch(acc.h, span, start, n, out.ctypes.data_as(C.c_void_p)) == SBH_E_ARG
            assert L.sbh_pileup_calls_fetch(acc.h, span, start, n, out.ctypes.data_as(C.c_void_p)) == SBH_E_ARG
        assert L.sbh_pileup_counts_fetch(acc.h, 0, 200, 0, None) == 0
        assert L.sbh_pileup_intervals_fetch(acc.h, 0, want["intervals"].size + 1, out.ctypes.data_as(C.c_void_p)) == SBH_E_ARG
        assert not acc.device_ptr(1)
        call(acc.reset)
        assert call(acc.add, sh) == want["add"]
        finished_equals(acc, want, c.spans, c.min_depth, c.call_pct)
        # a shard of another context
        call(acc.reset)
        sh2 = scanned(other, c.flat, c.starts[0], len(c.starts))
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, sh2)
        assert e.value.code == SBH_E_ARG
        # a shard without a scan
        sh3 = ctx.shard(np.frombuffer(rc.bgzf(c.flat, 65280), np.uint8).copy())
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, sh3)
        assert e.value.code == SBH_E_STATE
        sh3.close()
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, sh, {"min_mapq": 256})
        assert e.value.code == SBH_E_ARG
        finished_equals(acc, finished(np.zeros_like(want["counts"]), c.spans), c.spans)  # nothing got in
    finally:
        other.close()
        acc.close()
        sh.close()


@pytest.mark.parametrize("spans, n_ref, min_baseq", [([], 4, 0), ([(1, 0, 10), (0, 0, 10)], 4, 0), ([(1, 0, 10), (1, 20, 30)], 4, 0),
                                                      ([(0, 10, 10)], 4, 0), ([(4, 0, 10)], 4, 0), ([(-1, 0, 10)], 4, 0),
                                                      ([(0, 0, 2 ** 31)], 4, 0), ([(0, 0, 10)], 4, -1), ([(0, 0, 10)], 4, 256)])
def test_create_refuses_bad_arguments(ctx, spans, n_ref, min_baseq):
    with pytest.raises(sb.SparkBamError) as e:
        ctx.pileup(spans, n_ref, min_baseq)
    assert e.value.code == SBH_E_ARG


def test_budget(ctx):
    n = ctx.pileup_budget()
    assert 10 ** 6 < n < 288 * 2 ** 30 // 33


def test_api_pileup_in_windows_and_passes(ctx):
    _, _, _, names, lens, _ = fixture("2.bam")
    want, (lo, hi) = fixture_want("2.bam")
    region = "%s:%d-%d" % (names[0], lo + 1, hi)
    one = call(sb.pileup, golden_bam("2.bam"), region=region, ctx=ctx)
    assert np.array_equal(one.intervals, want["intervals"]) and np.array_equal(one.counts(names[0]), want["counts"])
    assert np.array_equal(one.calls(names[0]), want["calls"])
    assert {k: one.stats[k] for k in want["stats"]} == want["stats"] and one.stats["n_counted"] == 2284
    many = call(sb.pileup, golden_bam("2.bam"), region=region, ctx=ctx, window=100000)
    assert many.stats == one.stats
    pm = __import__("sys").modules[sb.__name__ + ".pileup"]
    text = pm.pileup_text(want["intervals"], [(0, lo, hi)], lambda k: want["counts"], names)
    assert many.text() == one.text() == text and text.count(b"\n") == want["stats"]["nonzero"]
    assert many.text(True, True) == one.text(True, True) and one.text(True, True).count(b"\n") == hi - lo + 1
    fasta = pm.consensus_fasta([(0, lo, hi)], lambda k: want["calls"], names, lens)
    assert many.consensus() == one.consensus() == fasta and fasta.startswith(b">%s:%d-%d\n" % (names[0].encode(), lo + 1, hi))
    # another filter and other parameters, through the same entry
    w2 = pc.restate(fixture("2.bam")[1], fixture("2.bam")[2], [(0, lo, hi)], len(lens), {"flag_exclude": 0, "min_mapq": 30}, 13,
                    3, 90)
    d = call(sb.pileup, golden_bam("2.bam"), region=region, flag_exclude=0, min_mapq=30, min_baseq=13, min_depth=3, call_pct=90,
             ctx=ctx, window=150000)
    assert np.array_equal(d.counts(names[0]), w2["counts"]) and np.array_equal(d.calls(names[0]), w2["calls"])
    with pytest.raises(sb.SparkBamError) as e:
        sb.pileup(golden_bam("2.bam"), region="no_such_reference", ctx=ctx)
    assert e.value.code == SBH_E_ARG
    with pytest.raises(ValueError) as e:
        sb.pileup(golden_bam("2.bam"), region=region, ctx=ctx, max_positions=hi - lo - 1)
    assert "(ref 0, %d, %d)" % (lo, hi) in str(e.value)


def test_api_pileup_halo_rerun_adds_once(ctx):
    """A first halo of 16 bytes: windows run again (x 4 each time) until the block behind the window
    and the chain's exit are resident.  A window that runs twice is added once: the one-window answer."""
    _, _, _, names, _, _ = fixture("2.bam")
    _, (lo, hi) = fixture_want("2.bam")
    region = "%s:%d-%d" % (names[0], lo + 1, hi)
    one = call(sb.pileup, golden_bam("2.bam"), region=region, ctx=ctx)
    rerun, w_rerun = walked(sb.pileup, golden_bam("2.bam"), ctx, halo=16, window=150000, region=region)
    assert len(w_rerun) > len(set(o for o, _ in w_rerun)) >= 3
    assert np.array_equal(rerun.intervals, one.intervals) and rerun.stats == one.stats
    assert np.array_equal(rerun.counts(names[0]), one.counts(names[0]))
    assert np.array_equal(rerun.calls(names[0]), one.calls(names[0]))


def test_api_pileup_three_passes_are_one(ctx):
    """A file with records on four small references: under max_positions = 2000 the spans go in three
    passes (1000 | 1500 | 800 + 1200), and the text and the FASTA are the one-pass bytes."""
    contigs = (("a", 1000), ("b", 1500), ("c", 800), ("d", 1200))
    recs = [pc.read(10 + 7 * i, [(5, pc.M), (1, pc.I), (2, pc.D), (6, pc.M)], ref=i % 4, seed=i) for i in range(100)]
    hdr = rc.header(contigs)
    starts = (len(hdr) + np.concatenate(([0], np.cumsum([len(r) for r in recs])))[:-1]).tolist()
    flat = hdr + b"".join(recs)
    data = rc.bgzf(flat, 65280)
    spans = [(k, 0, n) for k, (_, n) in enumerate(contigs)]
    pm = __import__("sys").modules[sb.__name__ + ".pileup"]
    assert [len(g) for g in pm.span_passes(spans, 2000)] == [1, 1, 2]
    want = pc.restate(flat, starts, spans, 4, EXCLUDE, 20, 2, 60)
    one = call(sb.pileup, data, min_baseq=20, min_depth=2, call_pct=60, ctx=ctx, max_positions=10 ** 6)
    three = call(sb.pileup, data, min_baseq=20, min_depth=2, call_pct=60, ctx=ctx, max_positions=2000)
    assert one.stats == three.stats and {k: one.stats[k] for k in want["stats"]} == want["stats"]
    assert one.stats["n_counted"] == 100 and one.stats["n"] == 100
    assert np.array_equal(one.intervals, want["intervals"]) and np.array_equal(three.intervals, want["intervals"])
    for k, a, b in pc.span_slices(spans):
        for r in (one, three):
            assert np.array_equal(r.counts(contigs[k][0]), want["counts"][a:b])
            assert np.array_equal(r.calls(contigs[k][0]), want["calls"][a:b])
    assert one.text() == three.text() and one.text(True, True) == three.text(True, True)
    assert one.consensus() == three.consensus() and one.consensus().startswith(b">a\n")
    with pytest.raises(ValueError) as e:
        sb.pileup(data, ctx=ctx, max_positions=1400)
    assert "(ref 1, 0, 1500)" in str(e.value)
