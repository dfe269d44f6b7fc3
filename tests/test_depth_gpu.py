"""Per-base depth on the device (sbh_records_depth_add: k_depth_check, k_depth_events;
sbh_depth_finish: k_depth_tile_sums, k_depth_apply, k_depth_runs) against the numpy restatement of
depth_corpus.py: the add's counts, the stats, the runs and the fetched depth on every corpus; a
failed add leaving the accumulator as it was; two shards into one accumulator; the state rules; the
bundled files with literal expected numbers; api.depth over the whole genome, in several windows and
with a window that runs twice.  Every comparison is exact equality."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import golden_bam
from pkg import sb
import depth_corpus as dc
import record_corpus as rc
from test_record_conformance_gpu import call
from walk_spy import walked

pytestmark = pytest.mark.gpu

SBH_E_ARG, SBH_E_STATE, SBH_E_BAD_RECORD = sb._lib.SBH_E_ARG, sb._lib.SBH_E_STATE, sb._lib.SBH_E_BAD_RECORD
SBH_E_NEED_HALO = sb._lib.SBH_E_NEED_HALO
EXCLUDE = {"flag_exclude": 0x704}


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def scanned(ctx, flat, first, n, level=6):
    """The stream resident, inflated and scanned from its first record."""
    sh = ctx.shard(np.frombuffer(rc.bgzf(flat, 65280, level), np.uint8).copy())
    call(sh.index, 0)
    call(sh.inflate)
    assert call(sh.records_scan, first, sh.flat_size) == n
    return sh


def finished_equals(acc, want, spans):
    """finish + every fetch against the restatement's depth, runs and stats."""
    sizes = call(acc.finish)
    assert sizes == want["stats"]
    runs = call(acc.runs)
    assert runs.dtype == dc.RUN_DTYPE and np.array_equal(runs, want["runs"])
    off = 0
    for k, (_, b, e) in enumerate(spans):
        d = call(acc.depth, k)
        assert d.dtype == np.uint32 and np.array_equal(d, want["depth"][off:off + e - b])
        off += e - b + 1
    if runs.size > 2:  # a slice of the runs, a slice of the depth
        assert np.array_equal(call(acc.runs, 1, runs.size - 2), want["runs"][1:-1])
    _, b, e = spans[0]
    if e - b > 2:
        assert np.array_equal(call(acc.depth, 0, 1, e - b - 2), want["depth"][1:e - b - 1])
    assert acc.device_ptr(0)
    return sizes


def in_file_order(c):
    return list(c.starts) == sorted(set(c.starts))


@pytest.mark.parametrize("name", [k for k in dc.SMALL if in_file_order(dc.get(k))])
def test_corpus(ctx, name):
    c, want = dc.get(name), dc.expected(name)
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts))
    acc = ctx.depth(c.spans, dc.N_REF, c.count_del)
    try:
        add = call(acc.add, sh, c.filter)
        assert add == want["add"]
        sizes = finished_equals(acc, want, c.spans)
        assert sizes["sum"] == add["cov_bases"]
        # reset and the same rows again: the same answer
        call(acc.reset)
        assert call(acc.add, sh, c.filter) == want["add"]
        assert call(acc.finish) == want["stats"] and np.array_equal(call(acc.runs), want["runs"])
    finally:
        acc.close()
        sh.close()


def test_grid_edge(ctx):
    """More rows than one grid pass of the row kernels (262144)."""
    c, want = dc.get("grid"), dc.expected("grid")
    assert len(c.starts) > 1024 * 256
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts), level=1)
    acc = ctx.depth(c.spans, dc.N_REF)
    try:
        assert call(acc.add, sh) == want["add"]
        # rows of one reference in three, with a filter on top: counts from the restatement
        f = {"flag_require": 0x10, "rows": [(5, 100000), (262100, 262181)]}
        w2 = dc.restate(c.flat, c.starts, c.spans, dc.N_REF, f)
        assert call(acc.add, sh, f) == w2["add"]
        finished_equals(acc, dc.finish(want["diff"] + w2["diff"], c.spans), c.spans)
    finally:
        acc.close()
        sh.close()


def test_rows_counted_again_and_again(ctx):
    """The whole scan once, then row 7 alone three times more: depth_corpus's reversed-and-tripled rows."""
    c, want = dc.get("rows_reversed_and_tripled"), dc.expected("rows_reversed_and_tripled")
    file_order = sorted(set(c.starts))
    sh = scanned(ctx, c.flat, file_order[0], len(file_order))
    acc = ctx.depth(c.spans, dc.N_REF)
    try:
        total = call(acc.add, sh)["cov_bases"]
        for _ in range(3):
            total += call(acc.add, sh, {"rows": [(7, 8)]})["cov_bases"]
        assert finished_equals(acc, want, c.spans)["sum"] == total == want["add"]["cov_bases"]
    finally:
        acc.close()
        sh.close()


def test_failed_add_leaves_the_accumulator_as_it_was(ctx):
    good, want = dc.get("composite"), dc.expected("composite")
    bad = dc.OP9_KEPT()
    off_ref = dc.case([dc.one(1, [(4, dc.M)]), dc.one(2, [(4, dc.M)]), dc.one(1, [(4, dc.M)], ref=dc.N_REF - 1)],
                      [(0, 0, 100)])
    sh = scanned(ctx, good.flat, good.starts[0], len(good.starts))
    sb_ = scanned(ctx, bad.flat, bad.starts[0], len(bad.starts))
    so = scanned(ctx, off_ref.flat, off_ref.starts[0], len(off_ref.starts))
    acc = ctx.depth(good.spans, dc.N_REF - 1)  # one reference fewer: off_ref's last row is out of range
    try:
        assert call(acc.add, sh) == want["add"]
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, sb_)
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (1,)
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.add, so)
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (2,)
        # dropped by the filter, the same rows are no error (and the valid ones count)
        assert call(acc.add, sb_, {"rows": [(1, 2)], "flag_require": 0x10})["n_kept"] == 0
        finished_equals(acc, want, good.spans)
    finally:
        acc.close()
        for s in (sh, sb_, so):
            s.close()


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(file bytes, flat, record starts, names, lengths, first) of a bundled BAM."""
    data = np.fromfile(golden_bam(name), dtype=np.uint8)
    flat = rc.inflate_members(data.tobytes())
    names, lens, first = sb.parse_bam_header(np.frombuffer(flat, np.uint8))
    starts, p = [], first
    while p < len(flat):
        starts.append(p)
        p += 4 + int.from_bytes(flat[p:p + 4], "little")
    return data, flat, starts, names, [int(x) for x in lens], first


@functools.lru_cache(maxsize=None)
def fixture_want(name, count_del=False, exclude=0x704, min_mapq=0):
    """The restatement over the stretch [lo, hi) of reference 0 that holds every record, one empty
    base on each side; `whole` widens its two outer zero runs to the whole reference."""
    _, flat, starts, _, lens, _ = fixture(name)
    u8 = np.frombuffer(flat, np.uint8)
    st = np.asarray(starts, np.int64)
    on0 = dc._i32(u8, st + 4) == 0
    pos = dc._i32(u8, st + 8)[on0]
    lo, hi = max(int(pos.min()) - 1, 0), int(pos.max()) + 100000
    assert 0 < lo and hi < lens[0]
    f = {"flag_exclude": exclude, "min_mapq": min_mapq}
    want = dc.restate(flat, starts, [(0, lo, hi)], len(lens), f, count_del)
    assert want["depth"][0] == 0 and want["depth"][-2] == 0 and want["add"]["cov_bases"] == want["stats"]["sum"]
    whole = want["runs"].copy()
    whole["beg"][0], whole["end"][-1] = 0, lens[0]
    return want, whole, (lo, hi)


def whole_ref_equals(acc, name, want, whole, lo_hi):
    _, _, _, _, lens, _ = fixture(name)
    lo, hi = lo_hi
    sizes = call(acc.finish)
    assert sizes == dict(want["stats"], slots=lens[0] + 1, n_runs=whole.size)
    assert np.array_equal(call(acc.runs), whole)
    assert np.array_equal(call(acc.depth, 0, lo, hi - lo), want["depth"][:-1])
    assert not call(acc.depth, 0, 0, lo).any() and not call(acc.depth, 0, hi, min(lens[0] - hi, 1 << 20)).any()
    return sizes


FIXTURE_NUMBERS = {  # kept placed records, sum, max_depth, covered: from a plain walk of the files
    "2.bam": (2284, 230383, 308, 12339),
    "5k.bam": (4454, 449355, 471, 18441),
    "1.bam": (3755, 281810, 245, 8511),
}


@pytest.mark.parametrize("name", FIXTURE_NUMBERS)
def test_bundled_file_after_both_kinds_of_scan(ctx, name):
    data, flat, starts, names, lens, first = fixture(name)
    want, whole, lo_hi = fixture_want(name)
    n_counted, total, max_depth, covered = FIXTURE_NUMBERS[name]
    assert (want["add"]["n_counted"], want["stats"]["sum"], want["stats"]["max_depth"], want["stats"]["covered"]) == \
        (n_counted, total, max_depth, covered)
    sh = ctx.shard(data)
    acc = ctx.depth([(0, 0, lens[0])], len(lens))
    try:
        call(sh.set_contigs, lens)
        info, cols = call(sh.split_records, 0, data.size, decode=False)  # the starts alone
        assert info["n"] == len(starts) and cols["flat"].tolist() == starts
        assert call(acc.add, sh, EXCLUDE) == want["add"]
        sizes = whole_ref_equals(acc, name, want, whole, lo_hi)
        assert (sizes["sum"], sizes["max_depth"], sizes["covered"]) == (total, max_depth, covered)
        call(acc.reset)
        assert call(sh.records_scan, first, sh.flat_size) == len(starts)  # the decoded scan
        assert call(acc.add, sh, EXCLUDE) == want["add"]
        whole_ref_equals(acc, name, want, whole, lo_hi)
    finally:
        acc.close()
        sh.close()


def test_two_shards_into_one_accumulator(ctx):
    """The first and the second half of 2.bam's records as two files, each on a shard of its own."""
    _, flat, starts, _, lens, first = fixture("2.bam")
    want, whole, lo_hi = fixture_want("2.bam")
    cut = starts[len(starts) // 2]
    halves = (flat[:cut], flat[:first] + flat[cut:])
    acc = ctx.depth([(0, 0, lens[0])], len(lens))
    try:
        adds = []
        for part, n in zip(halves, (len(starts) // 2, len(starts) - len(starts) // 2)):
            sh = scanned(ctx, part, first, n)
            try:
                adds.append(call(acc.add, sh, EXCLUDE))
            finally:
                sh.close()  # the accumulator outlives the shard
        assert {k: adds[0][k] + adds[1][k] for k in adds[0]} == want["add"]
        whole_ref_equals(acc, "2.bam", want, whole, lo_hi)
    finally:
        acc.close()


def test_open_shard_end(ctx):
    """A shard that holds the file's first ten members only; a record straddles its end.  The add
    answers SBH_E_NEED_HALO for a row that merely runs past an open shard end (sbh_records_bam_scan's
    rule), but no scan delivers such a row: the starts-only split scan asks for the halo itself
    unless two whole members lie behind the split's end, and then every row ends inside the resident
    bytes.  What can be seen from outside: the refused scans leave the accumulator as it was, and
    the rows of the split that fits are added as the restatement has them."""
    data, flat, starts, _, lens, first = fixture("2.bam")
    want, whole, lo_hi = fixture_want("2.bam")
    sh_all = ctx.shard(data)
    call(sh_all.index, 0)
    blocks = sh_all.blocks()
    sh_all.close()
    cut_file, cut_flat = blocks[10][0], blocks[10][3]
    assert cut_flat not in starts  # a record straddles the resident end
    acc = ctx.depth([(0, 0, lens[0])], len(lens))
    sh = ctx.shard(data[:cut_file].copy(), file_offset=0, file_size=data.size)
    full = ctx.shard(data)
    try:
        call(full.index, 0)
        call(full.inflate)
        assert call(full.records_scan, first, full.flat_size) == len(starts)
        assert call(acc.add, full, EXCLUDE) == want["add"]
        call(sh.set_contigs, lens)
        for end in (cut_file, blocks[9][0] + 1):
            with pytest.raises(sb.SparkBamError) as e:
                call(sh.split_records, 0, end, bgzf_blocks_to_check=2, decode=False)
            assert e.value.code == SBH_E_NEED_HALO
            with pytest.raises(sb.SparkBamError) as e:  # no valid scan: nothing to add
                call(acc.add, sh, EXCLUDE)
            assert e.value.code == SBH_E_STATE
        whole_ref_equals(acc, "2.bam", want, whole, lo_hi)
        # two members of halo: the split's rows, all inside the resident bytes
        info, cols = call(sh.split_records, 0, blocks[8][0] + 1, bgzf_blocks_to_check=2, decode=False)
        rows = cols["flat"].tolist()
        assert rows == [s for s in starts if s < blocks[9][3]] and info["flat_size"] == cut_flat
        call(acc.reset)
        w = dc.restate(flat, rows, [(0, lo_hi[0], lo_hi[1])], len(lens), EXCLUDE)
        assert call(acc.add, sh, EXCLUDE) == w["add"]
        assert call(acc.finish)["sum"] == w["stats"]["sum"]
        assert np.array_equal(call(acc.depth, 0, lo_hi[0], lo_hi[1] - lo_hi[0]), w["depth"][:-1])
    finally:
        acc.close()
        sh.close()
        full.close()


def test_state_rules(ctx):
    c, want = dc.get("composite"), dc.expected("composite")
    sh = scanned(ctx, c.flat, c.starts[0], len(c.starts))
    acc = ctx.depth(c.spans, dc.N_REF)
    other = sb.Context(0)
    L = sb.lib()
    try:
        with pytest.raises(sb.SparkBamError) as e:  # fetches before finish
            call(acc.depth, 0)
        assert e.value.code == SBH_E_STATE
        with pytest.raises(sb.SparkBamError) as e:
            call(acc.runs)
        assert e.value.code == SBH_E_STATE
        assert not acc.device_ptr(0)
        assert call(acc.add, sh) == want["add"]
        assert call(acc.finish) == want["stats"]
        with pytest.raises(sb.SparkBamError) as e:  # an add after finish
            call(acc.add, sh)
        assert e.value.code == SBH_E_STATE
        with pytest.raises(sb.SparkBamError) as e:  # a second finish
            call(acc.finish)
        assert e.value.code == SBH_E_STATE
        assert np.array_equal(call(acc.runs), want["runs"])  # (the refused calls changed nothing)
        for span, start, n in ((1, 0, 1), (0, 0, 101), (0, 100, 1), (0, 101, 0)):
            out = np.zeros(200, np.uint32)
            assert L.sbh_depth_fetch(acc.h, span, start, n, out.ctypes.data_as(C.c_void_p)) == SBH_E_ARG
        assert L.sbh_depth_fetch(acc.h, 0, 100, 0, None) == 0
        assert L.sbh_depth_runs_fetch(acc.h, 0, want["runs"].size + 1, out.ctypes.data_as(C.c_void_p)) == SBH_E_ARG
        assert not acc.device_ptr(1)
        call(acc.reset)
        assert call(acc.add, sh) == want["add"]
        finished_equals(acc, want, c.spans)
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
        finished_equals(acc, dc.finish(np.zeros_like(want["diff"]), c.spans), c.spans)  # nothing got in
    finally:
        other.close()
        acc.close()
        sh.close()


@pytest.mark.parametrize("spans, n_ref, count_del", [([], 4, False), ([(1, 0, 10), (0, 0, 10)], 4, False),
                                                      ([(1, 0, 10), (1, 20, 30)], 4, False), ([(0, 10, 10)], 4, False),
                                                      ([(4, 0, 10)], 4, False), ([(-1, 0, 10)], 4, False),
                                                      ([(0, 0, 2 ** 31)], 4, False)])
def test_create_refuses_bad_spans(ctx, spans, n_ref, count_del):
    with pytest.raises(sb.SparkBamError) as e:
        ctx.depth(spans, n_ref, count_del)
    assert e.value.code == SBH_E_ARG


def test_create_refuses_unknown_flags(ctx):
    sp = dc.span_array([(0, 0, 10)])
    h = C.c_void_p()
    assert sb.lib().sbh_depth_create(ctx.h, sp.ctypes.data_as(C.c_void_p), 1, 4, 2, C.byref(h)) == SBH_E_ARG
    assert not h.value


def test_the_add_leaves_the_scan_and_the_bam_stream_alone(ctx):
    data, flat, starts, names, lens, first = fixture("2.bam")
    sh = ctx.shard(data)
    acc = ctx.depth([(0, 0, lens[0])], len(lens))
    try:
        call(sh.index, 0)
        call(sh.inflate)
        cols = call(sh.records, first, sh.flat_size)
        text, line_off = call(sh.records_sam, names)
        before = call(sh.records_bam, flat[:first], {"flag_exclude": 0x10})
        call(acc.add, sh, EXCLUDE)
        ptr = sh.bam_ptr()
        assert ptr
        after = (np.empty(before[0].size, np.uint8), np.zeros(before[1].size, np.uint64), np.zeros(before[2].size, np.uint64))
        assert sb.lib().sbh_records_bam_fetch(sh.h, *(a.ctypes.data_as(C.c_void_p) for a in after)) == 0
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        again = call(sh._records_fetch, sb._lib.SbhRecordsSizes(len(starts), cols["names"].size, cols["cigar"].size,
                                                                cols["seq"].size, cols["aux"].size))
        for k in cols:
            assert np.array_equal(again[k], cols[k]), k
        text2, line_off2 = call(sh.records_sam, names)
        assert np.array_equal(text2, text) and np.array_equal(line_off2, line_off)
    finally:
        acc.close()
        sh.close()


def test_api_depth_over_every_reference(ctx):
    """region=None: all 84 references of 2.bam, 3.1 G slots.  Reference 0 as the one-span answer,
    one zero run on each of the others."""
    _, _, _, names, lens, _ = fixture("2.bam")
    want, whole, _ = fixture_want("2.bam")
    r = call(sb.depth, golden_bam("2.bam"), ctx=ctx)
    assert r.stats["slots"] == sum(lens) + len(lens) and r.stats["slots"] > 3 * 10 ** 9
    assert np.array_equal(r.runs[:whole.size], whole)
    rest = r.runs[whole.size:]
    assert rest["ref_id"].tolist() == list(range(1, len(lens))) and not rest["depth"].any()
    assert rest["beg"].tolist() == [0] * (len(lens) - 1) and rest["end"].tolist() == lens[1:]
    for k in ("covered", "sum", "max_depth"):
        assert r.stats[k] == want["stats"][k]
    assert {k: r.stats[k] for k in want["add"]} == want["add"]
    assert r.bedgraph() == sb.depth_bedgraph(whole, names)


def test_api_depth_in_windows_and_renderers(ctx):
    _, _, _, names, lens, _ = fixture("2.bam")
    want, whole, (lo, hi) = fixture_want("2.bam")
    region = "%s:%d-%d" % (names[0], lo + 1, hi)
    one = call(sb.depth, golden_bam("2.bam"), region=region, ctx=ctx)
    assert np.array_equal(one.runs, want["runs"]) and np.array_equal(one.depth(names[0]), want["depth"][:-1])
    assert one.stats["n_counted"] == 2284
    many = call(sb.depth, golden_bam("2.bam"), region=region, ctx=ctx, window=100000)
    assert many.stats == one.stats
    assert many.text() == one.text() == sb.depth_text(want["runs"], names)
    assert many.bedgraph() == one.bedgraph() == sb.depth_bedgraph(want["runs"], names)
    assert many.text(all_positions=True) == one.text(all_positions=True)
    assert one.text(all_positions=True).count(b"\n") == hi - lo
    # -J and another filter, through the same entry
    w2, _, _ = fixture_want("2.bam", True, 0, 30)
    d = call(sb.depth, golden_bam("2.bam"), region=region, flag_exclude=0, min_mapq=30, count_del=True, ctx=ctx, window=150000)
    assert np.array_equal(d.runs, w2["runs"]) and d.stats["sum"] == w2["stats"]["sum"]
    with pytest.raises(sb.SparkBamError) as e:
        sb.depth(golden_bam("2.bam"), region="no_such_reference", ctx=ctx)
    assert e.value.code == SBH_E_ARG


def test_api_depth_halo_rerun_adds_once(ctx):
    """A first halo of 16 bytes: windows run again (x 4 each time) until the block behind the window
    and the chain's exit are resident.  A window that runs twice is added once: the one-window answer."""
    _, _, _, names, _, _ = fixture("2.bam")
    _, _, (lo, hi) = fixture_want("2.bam")
    region = "%s:%d-%d" % (names[0], lo + 1, hi)
    one = call(sb.depth, golden_bam("2.bam"), region=region, ctx=ctx)
    rerun, w_rerun = walked(sb.depth, golden_bam("2.bam"), ctx, halo=16, window=150000, region=region)
    assert len(w_rerun) > len(set(o for o, _ in w_rerun)) >= 3
    assert np.array_equal(rerun.runs, one.runs) and rerun.stats == one.stats
