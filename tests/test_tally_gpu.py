"""Flag counts and per-reference read counts on the device (sbh_records_tally_add: k_tally_rows,
k_tally_commit; sbh_tally_fetch) against the numpy restatement of tally_corpus.py on every corpus; a
failed add leaving the accumulator as it was; two shards into one accumulator; the argument errors;
the bundled files with literal expected numbers and against their `.bai`; api.flagstat and
api.idxstats in one and in several windows.  Every comparison is exact equality."""
import ctypes as C
import struct

import numpy as np
import pytest

from conftest import golden_bam
from pkg import sb
import record_corpus as rc
import tally_corpus as tc
from test_depth_gpu import scanned
from test_record_conformance_gpu import call
from test_tally_cpu import BUNDLED, FLAGSTAT_1BAM, FLAGSTAT_2BAM, bundled, bundled_flag, bundled_ref
from walk_spy import walked

pytestmark = pytest.mark.gpu

SBH_E_ARG, SBH_E_STATE, SBH_E_BAD_RECORD = sb._lib.SBH_E_ARG, sb._lib.SBH_E_STATE, sb._lib.SBH_E_BAD_RECORD


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def counts_equal(acc, want):
    flag, ref = call(acc.counts)
    assert flag.dtype == np.uint64 and flag.shape == (16, 2) and np.array_equal(flag, want["flag"])
    assert ref.dtype == np.uint64 and ref.shape == want["ref"].shape and np.array_equal(ref, want["ref"])
    assert int(ref[:, 0].sum()) == int(flag[6].sum()) and int(ref.sum()) == int(flag[0].sum())  # the invariants


def added(want):
    return {"n": want["n"], "n_kept": want["n_kept"]}


@pytest.mark.parametrize("name", [k for k in tc.SMALL if tc.in_file_order(tc.get(k)) and tc.get(k).starts])
def test_corpus(ctx, name):
    c, want = tc.get(name), tc.expected(name)
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts))
    acc = ctx.tally(c.n_ref)
    try:
        assert call(acc.add, sh, c.filter) == added(want)
        counts_equal(acc, want)
        # reset and the same rows again: the same answer; once more without a reset: twice the answer
        call(acc.reset)
        assert call(acc.add, sh, c.filter) == added(want)
        counts_equal(acc, want)
        assert call(acc.add, sh, c.filter) == added(want)
        counts_equal(acc, {"flag": 2 * want["flag"], "ref": 2 * want["ref"]})
    finally:
        acc.close()
        sh.close()


@pytest.mark.parametrize("name", tc.LARGE)
def test_more_rows_than_one_grid_pass(ctx, name):
    c, want = tc.get(name), tc.expected(name)
    assert len(c.starts) > tc.GRID_PASS
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts), level=1)
    acc = ctx.tally(c.n_ref)
    try:
        assert call(acc.add, sh) == added(want)
        counts_equal(acc, want)
        # a filter on top, rows on both sides of the pass edge: counts from the restatement
        f = {"flag_exclude": tc.REVERSE, "rows": [(5, 100000), (262100, 262181)]}
        w2 = tc.restate(c.flat, c.starts, c.n_ref, f)
        assert call(acc.add, sh, f) == added(w2)
        counts_equal(acc, {"flag": want["flag"] + w2["flag"], "ref": want["ref"] + w2["ref"]})
    finally:
        acc.close()
        sh.close()


def test_row_order_and_a_row_counted_again_and_again(ctx):
    """The device takes a scan's rows in file order: the reversed corpus is the same sum, and the row
    given three times is the whole scan once, then row 7 alone twice more."""
    for name, again in (("rows_reversed", 0), ("row_given_three_times", 2)):
        c, want = tc.get(name), tc.expected(name)
        file_order = sorted(set(c.starts))
        sh = scanned(ctx, c.flat, file_order[0], len(file_order))
        acc = ctx.tally(c.n_ref)
        try:
            kept = call(acc.add, sh)["n_kept"]
            for _ in range(again):
                kept += call(acc.add, sh, {"rows": [(7, 8)]})["n_kept"]
            assert kept == want["n_kept"]
            counts_equal(acc, want)
        finally:
            acc.close()
            sh.close()


def test_failed_add_leaves_the_accumulator_as_it_was(ctx):
    good, want = tc.get("mate_chr"), tc.expected("mate_chr")
    off_ref = tc.TID_KEPT()
    sh = scanned(ctx, good.flat, good.starts[0], len(good.starts))
    so = scanned(ctx, off_ref.flat, off_ref.starts[0], len(off_ref.starts))
    acc = ctx.tally(tc.N_REF)
    try:
        assert call(acc.add, sh) == added(want)
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, so)
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (2,)
        counts_equal(acc, want)
        # dropped by the filter, the same row is no error, and the valid ones count
        w2 = tc.restate(off_ref.flat, off_ref.starts, tc.N_REF, {"rows": [(0, 2), (3, 4)]})
        assert call(acc.add, so, {"rows": [(0, 2), (3, 4)]}) == {"n": 4, "n_kept": 3}
        counts_equal(acc, {"flag": want["flag"] + w2["flag"], "ref": want["ref"] + w2["ref"]})
    finally:
        acc.close()
        sh.close()
        so.close()


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed_stream_leaves_the_accumulator_as_it_was(ctx, m):
    """What depth's add gives on the same streams: no scan delivers the malformed row (the scan
    itself answers SBH_E_BAD_RECORD), so either add finds no valid scan and answers SBH_E_STATE; the
    good rows before it, scanned alone, count.  (The add's own answer for such a row, SBH_E_BAD_RECORD
    {3}, is the host function's in test_tally_cpu.py and the driver's under the sanitizers.)"""
    good, want = tc.get("pair_rows"), tc.expected("pair_rows")
    sh = scanned(ctx, good.flat, good.starts[0], len(good.starts))
    bad = ctx.shard(np.frombuffer(rc.bgzf(m.stream.flat, 65280), np.uint8).copy())
    acc = ctx.tally(tc.N_REF)
    dep = ctx.depth([(0, 0, 2000)], tc.N_REF)
    try:
        assert call(acc.add, sh) == added(want)
        call(bad.index, 0)
        call(bad.inflate)
        with pytest.raises(sb.SparkBamError) as e:
            call(bad.records_scan, m.stream.first, bad.flat_size)
        assert e.value.code == SBH_E_BAD_RECORD
        got = []
        for a in (dep, acc):
            with pytest.raises(sb.SparkBamError) as e:
                call(a.add, bad)
            got.append((e.value.code, e.value.fields))
        assert got[0] == got[1] == (SBH_E_STATE, ())
        counts_equal(acc, want)
        assert call(bad.records_scan, m.stream.first, m.bad_start) == 3
        w3 = tc.restate(m.stream.flat, m.stream.starts[:3], tc.N_REF)
        assert call(acc.add, bad) == {"n": 3, "n_kept": 3}
        counts_equal(acc, {"flag": want["flag"] + w3["flag"], "ref": want["ref"] + w3["ref"]})
    finally:
        dep.close()
        acc.close()
        sh.close()
        bad.close()


def test_two_shards_into_one_accumulator_and_a_fetch_in_between(ctx):
    """The first and the second half of 1.bam's records as two files, each on a shard of its own."""
    _, flat, starts, _, lens, first = bundled("1.bam")
    cut = starts[len(starts) // 2]
    halves = ((flat[:cut], starts[:len(starts) // 2]), (flat[:first] + flat[cut:], [s - cut + first for s in starts[len(starts) // 2:]]))
    acc = ctx.tally(len(lens))
    try:
        so_far = None
        for part, st in halves:
            want = tc.restate(part, st, len(lens))
            sh = scanned(ctx, part, first, len(st))
            try:
                assert call(acc.add, sh) == added(want)
            finally:
                sh.close()  # the accumulator outlives the shard
            so_far = want if so_far is None else {"flag": so_far["flag"] + want["flag"], "ref": so_far["ref"] + want["ref"]}
            counts_equal(acc, so_far)  # a fetch between the adds
        counts_equal(acc, {"flag": bundled_flag("1.bam"), "ref": bundled_ref("1.bam", len(lens))})
    finally:
        acc.close()


def test_argument_errors(ctx):
    c, want = tc.get("pair_rows"), tc.expected("pair_rows")
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts))
    acc = ctx.tally(tc.N_REF)
    other = sb.Context(0)
    L = sb.lib()
    try:
        h = C.c_void_p()
        assert L.sbh_tally_create(ctx.h, -1, C.byref(h)) == SBH_E_ARG and not h.value
        with pytest.raises(sb.SparkBamError) as e:
            ctx.tally(-5)
        assert e.value.code == SBH_E_ARG
        assert call(acc.add, sh) == added(want)
        ref = np.zeros((tc.N_REF + 2, 2), np.uint64)
        p = ref.ctypes.data_as(C.c_void_p)
        for first_bin, n_bins in ((0, tc.N_REF + 2), (tc.N_REF + 1, 1), (tc.N_REF + 2, 0), (2 ** 64 - 1, 2)):
            assert L.sbh_tally_fetch(acc.h, None, first_bin, n_bins, p) == SBH_E_ARG
        assert not ref.any()
        # a slice of the bins, the flag counters alone, nothing at all
        assert L.sbh_tally_fetch(acc.h, None, 1, 2, p) == 0 and np.array_equal(ref[:2], want["ref"][1:3]) and not ref[2:].any()
        assert L.sbh_tally_fetch(acc.h, None, tc.N_REF + 1, 0, p) == 0 and L.sbh_tally_fetch(acc.h, None, 0, 0, None) == 0
        flag = np.zeros((16, 2), np.uint64)
        assert L.sbh_tally_fetch(acc.h, flag.ctypes.data_as(C.c_void_p), 0, 0, None) == 0 and np.array_equal(flag, want["flag"])
        # a shard of another context; a shard without a scan; a bad filter: nothing gets in
        sh2 = scanned(other, c.flat, c.starts[0], len(c.starts))
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, sh2)
        assert e.value.code == SBH_E_ARG
        sh3 = ctx.shard(np.frombuffer(rc.bgzf(c.flat, 65280), np.uint8).copy())
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, sh3)
        assert e.value.code == SBH_E_STATE
        sh3.close()
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, sh, {"min_mapq": 256})
        assert e.value.code == SBH_E_ARG
        counts_equal(acc, want)
    finally:
        other.close()
        acc.close()
        sh.close()


def bai_pseudo_bins(bai_bytes):
    """[(num_mapped, num_unmapped)] per reference from the metadata pseudo-bins, and the trailing
    count of reads without coordinates."""
    idx = sb.read_bai(bai_bytes)
    per_ref = [(r.metadata.num_mapped, r.metadata.num_unmapped) if r.metadata else (0, 0) for r in idx.references]
    return per_ref, struct.unpack("<Q", bytes(bai_bytes)[-8:])[0]


@pytest.mark.parametrize("name", BUNDLED)
def test_bundled_file_after_both_kinds_of_scan(ctx, name):
    data, flat, starts, names, lens, first = bundled(name)
    want = {"flag": bundled_flag(name), "ref": bundled_ref(name, len(lens))}
    sh = ctx.shard(data)
    acc = ctx.tally(len(lens))
    try:
        call(sh.set_contigs, lens)
        info, cols = call(sh.split_records, 0, data.size, decode=False)  # the starts alone
        assert info["n"] == len(starts) and cols["flat"].tolist() == starts
        assert call(acc.add, sh) == {"n": len(starts), "n_kept": len(starts)}
        counts_equal(acc, want)
        call(acc.reset)
        assert call(sh.records_scan, first, sh.flat_size) == len(starts)  # the decoded scan
        assert call(acc.add, sh) == {"n": len(starts), "n_kept": len(starts)}
        counts_equal(acc, want)
    finally:
        acc.close()
        sh.close()


@pytest.mark.parametrize("name", ["2.bam", "5k.bam"])
def test_per_reference_counts_are_the_bai_s(ctx, name):
    """Two independent routes to the same numbers: the committed index's pseudo-bins, and the ones
    build_bai computes on the GPU."""
    data, _, _, _, lens, _ = bundled(name)
    with open(golden_bam(name) + ".bai", "rb") as f:
        committed, no_coor = bai_pseudo_bins(f.read())
    built, no_coor_built = bai_pseudo_bins(call(sb.build_bai, data, ctx=ctx))
    r = call(sb.idxstats, data, ctx=ctx)
    ours = [tuple(int(x) for x in row) for row in r.ref[:-1]]
    assert ours == committed == built and ours[0] == BUNDLED[name][1]
    assert no_coor == no_coor_built == 0 and r.ref[-1].tolist() == [0, 0]


def test_api_in_one_window_and_in_several(ctx):
    _, flat, starts, names, lens, _ = bundled("5k.bam")
    want_flag, want_ref = bundled_flag("5k.bam"), bundled_ref("5k.bam", len(lens))
    path = golden_bam("5k.bam")
    one, w_one = walked(sb.flagstat, path, ctx)
    idx, _ = walked(sb.idxstats, path, ctx)
    many, w_many = walked(sb.flagstat, path, ctx, window=100000)
    # a first halo of 16 bytes: windows run again (x 4 each time) until the block behind the window
    # and the chain's exit are resident
    rerun, w_rerun = walked(sb.idxstats, path, ctx, halo=16, window=150000)
    assert len(w_one) == 1 and len(set(o for o, _ in w_many)) >= 3 and len(w_many) == len(set(o for o, _ in w_many))
    assert len(w_rerun) > len(set(o for o, _ in w_rerun)) >= 3
    for r in (one, idx, many, rerun):
        assert np.array_equal(r.flag, want_flag) and np.array_equal(r.ref, want_ref)
        assert r.n_kept == r.n == 4910 and r.names == names and r.lengths == lens
        assert r.flagstat_text() == sb.flagstat_text(want_flag) and r.idxstats_text() == sb.idxstats_text(want_ref, names, lens)
    assert one.flagstat_text().startswith(b"4910 + 0 in total")
    # filters through the same entry, in windows: the restatement over the whole file
    w = tc.restate(flat, starts, len(lens), {"flag_require": 0x40, "flag_exclude": 0x400, "min_mapq": 20})
    r = call(sb.flagstat, path, flag_require=0x40, flag_exclude=0x400, min_mapq=20, ctx=ctx, window=120000)
    assert np.array_equal(r.flag, w["flag"]) and np.array_equal(r.ref, w["ref"]) and r.n_kept == w["n_kept"] and r.n == 4910


def test_api_text_literals(ctx):
    assert call(sb.flagstat, golden_bam("2.bam"), ctx=ctx).flagstat_text() == FLAGSTAT_2BAM
    assert call(sb.flagstat, golden_bam("1.bam"), ctx=ctx).flagstat_text() == FLAGSTAT_1BAM


def test_no_rows(ctx):
    """A file of a header alone: the scan delivers no row, the add counts none."""
    flat = rc.header()
    sh = scanned(ctx, flat, len(flat), 0)
    acc = ctx.tally(tc.N_REF)
    try:
        assert call(acc.add, sh) == {"n": 0, "n_kept": 0}
        counts_equal(acc, tc.expected("rows_0"))
    finally:
        acc.close()
        sh.close()
