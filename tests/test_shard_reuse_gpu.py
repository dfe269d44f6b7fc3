"""One shard, several files: what the second tenant of a shard gets, and which results an event voids.

Part A.  A shard runs the whole stage tour (shard_reuse.tour) for one file, sbh_shard_load swaps the
bytes, and the tour runs again for the next file.  The second tour must equal shard_reuse.expected,
key by key and exactly, and the tour of a fresh shard: a kernel that leans on a buffer tail, a closing
entry or a counter word being zero is right on a fresh allocation and wrong here, and so is a cached
flag that outlives the bytes it describes.  Then: a small scan after a large one with no load between
them, accumulators reset between two files, and a context's stream-window cache between two files.

Part B.  The invalidation table: on MID_B, a fresh shard is taken through index, inflate, set_contigs,
check_eager, a records scan of all rows, records_sam, records_bam (coordinate order), records_fastq
and bai_scan, and each accumulator takes the scan once.  Then one event, then one consumer.  Every
cell of EVENTS x CONSUMERS is either S -- SBH_E_STATE, the accumulator left as it was -- or V -- the
value the host computes for the bytes and rows now current.  The rule is written at sbh_index in
include/sparkbam.h.  TABLE holds one row per event and one letter per consumer (a CPU test holds its
shape to EVENTS x CONSUMERS), and the test of an event asserts that it ran len(CONSUMERS) cells, so
the parametrised test runs len(EVENTS) * len(CONSUMERS) of them.

The CPU tests (no gpu mark) hold the tenants to what they claim and check that expected() creates no
context, shard or accumulator.

Measured on an MI355X (this file alone, one process): see DESIGN.md, "Reused shards"."""
import ctypes as C
import math

import numpy as np
import pytest

import bai_ref
import shard_reuse as sr
from pkg import sb

gpu = pytest.mark.gpu
SBH_E_ARG, SBH_E_STATE, SBH_E_BAD_RECORD = sb._lib.SBH_E_ARG, sb._lib.SBH_E_STATE, sb._lib.SBH_E_BAD_RECORD


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def call(f, *a, **kw):
    """f(*a): a device error ends the session (nothing more runs on this GPU)."""
    try:
        return f(*a, **kw)
    except sb.SparkBamError as e:
        if e.code == sb._lib.SBH_E_HIP:
            pytest.exit("HIP error: %s" % e, returncode=3)
        raise


def shard_for(ctx, name):
    """A fresh shard holding the tenant as the tail of the FILE_SIZE-byte file."""
    return ctx.shard(sr.data_of(name), file_offset=sr.offset_of(name), file_size=sr.FILE_SIZE)


_FRESH = {}


def fresh_tour(ctx, name, path):
    """The tour of a fresh shard, computed once per (tenant, path) and left unchanged."""
    if (name, path) not in _FRESH:
        sh = shard_for(ctx, name)
        try:
            _FRESH[name, path] = sr.tour(sh, ctx, name, path, sr.offset_of(name))
        finally:
            sh.close()
    return _FRESH[name, path]


def assert_tour(got, name, path, where):
    want, keys = sr.expected(name), sr.keys_for(name, path)
    compared = set()
    wrong = []
    for k in sorted(keys):
        compared.add(k)
        if k not in got or not sr.same(got[k], want[k]):
            wrong.append(k)
    assert not wrong, "%s: %s (%s) differs from the host's answer in %s" % (where, name, path, wrong)
    assert compared == keys == set(got), (where, sorted(keys ^ set(got)))


# ------------------------------------------------------------------------- CPU: the tenants

ALL_KEYS = {"index", "run", "blocks", "flat", "crc", "eager", "full", "find_record_start", "count", "chain",
            "split_starts", "split_batch", "records", "sam", "bam_scan", "bam_coord", "fastq", "fastq_split",
            "bai_whole", "bai", "bai_edges", "tally", "depth", "pileup"}


def _refs(name):
    return sr.expected(name)["records"]["ref_id"]


def test_big_holds_its_claims():
    t, L, e = sr.tenant("BIG"), sr.layout("BIG"), sr.expected("BIG")
    n = len(L.starts)
    assert len(t.data) < 1 << 20
    assert n >= 2049 and math.ceil(n / sr.sc.SORT_TILE) > 1  # two-level scans over n + 1 rows, two sort tiles
    assert sr.descents("BIG") > 0 and e["bam_coord"][1] is False
    ref, flag = _refs("BIG"), e["records"]["flag"]
    assert set(ref.tolist()) == {-1, 0, 1, 2} and np.all(ref[-20:] == -1) and np.all(ref[:-20] >= 0)
    assert np.count_nonzero((flag & 4 != 0) & (ref >= 0)) > 100  # unmapped reads that still have a position
    # float-tag rows: counted by the builder, seen in the host's SAM text
    text = bytes(e["sam"][0]).split(b"\n")[:-1]
    assert len(text) == n
    assert sum(b"\tXF:f:" in ln or b"\tXB:B:f," in ln for ln in text) == t.n_float == e["sam"][2] > 0
    ops = np.diff(e["records"]["cigar_off"].astype(np.int64))
    assert np.count_nonzero(ops > 32) == t.n_long_cigar > 0  # BAI_COOP_OPS
    assert all(k > 0 for k in e["fastq_split"][3]["part_rows"])  # read 1, read 2, others
    flags = e["blocks"]["flags"]
    k = int(np.flatnonzero(e["blocks"]["start"] == t.empty_index)[0])
    assert flags[k] == sb.BLOCK_EMPTY and 0 < k < flags.size - 1 and flags[-1] == sb.BLOCK_EMPTY
    assert np.count_nonzero(flags == sb.BLOCK_EMPTY) == 2 and np.count_nonzero(e["blocks"]["usize"][:k] > 0) >= 4
    assert len(sr.segments("BIG")) == 2 and len(L.all_starts) == n + 5
    lin_size = bai_ref.build(t.data, t.sorted_rows).lin_off[-1]
    assert lin_size == e["bai"][1].size and lin_size > 3000
    assert e["bai_whole"][:2] == ("error", sr.SBH_E_UNSORTED)
    assert sr.false_positives("BIG") == 1 and e["eager"][0] == len(L.all_starts) + 1


def test_small_holds_its_claims():
    t, L, e = sr.tenant("SMALL"), sr.layout("SMALL"), sr.expected("SMALL")
    assert len(L.starts) == 3 and L.n_ref == 1 and set(_refs("SMALL").tolist()) == {0}
    assert e["blocks"]["flags"].tolist() == [0, sb.BLOCK_EMPTY] and t.empty_index is None
    assert sr.descents("SMALL") == 0 and e["bam_coord"][1] is True
    assert t.n_float == 0 == e["sam"][2] and sr.false_positives("SMALL") == 0
    assert e["bai"][1].size == (5000 >> 14) + 2 and sr.same(e["bai"], e["bai_whole"])


def test_mid_holds_its_claims():
    t, L, e = sr.tenant("MID"), sr.layout("MID"), sr.expected("MID")
    assert len(L.starts) == 257 and L.n_ref == 2 and set(_refs("MID").tolist()) == {0, 1}
    assert sr.descents("MID") == 0 and e["bam_coord"][1] is True and t.n_float == 0
    assert np.count_nonzero(e["blocks"]["flags"]) == 1 and t.n_long_cigar > 0
    recs = bai_ref.records_of(t.data)[0]
    for k in (sr.MID_ENDS_MEMBER, 256):  # the last byte of a member: the end is Pos(next member, 0)
        assert recs[k].vend & 0xffff == 0 and recs[k].vend >> 16 > recs[k].vbeg >> 16
    assert recs[sr.MID_ENDS_MEMBER].vend == recs[sr.MID_ENDS_MEMBER + 1].vbeg
    assert sr.false_positives("MID") == 0


def test_mid_b_is_mid_with_a_malformed_record_behind_its_end():
    m, b = sr.layout("MID"), sr.layout("MID_B")
    assert b.flat[:len(m.flat)] == m.flat and b.starts == m.starts and b.seg_end == m.seg_end
    assert b.all_starts == m.starts + [m.seg_end] and len(sr.segments("MID_B")) == 2
    with pytest.raises(sb.SparkBamError) as e:
        sb.bam_gather_host(np.frombuffer(b.flat, np.uint8), [b.all_starts[-1]])
    assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (0,)


def test_expected_is_computed_without_a_device(monkeypatch):
    def refuse(self, *a, **kw):
        raise AssertionError("expected() must not create a context, a shard or an accumulator")
    for cls in (sb.Context, sb.Shard, sb.Tally, sb.Depth, sb.Pileup):
        monkeypatch.setattr(cls, "__init__", refuse)
    sr.expected.cache_clear()
    sr.eager_expected.cache_clear()
    for name in ("BIG", "SMALL", "MID"):
        assert set(sr.expected(name)) == ALL_KEYS
        assert sr.keys_for(name, "run") == ALL_KEYS and sr.keys_for(name, "steps") == ALL_KEYS - {"run"}


def test_the_comparison_is_exact():
    a = {"x": (np.arange(5, dtype=np.uint64), b"ab"), "y": [1, {"n": 2}]}
    assert sr.same(a, {"x": (np.arange(5, dtype=np.int64), np.frombuffer(b"ab", np.uint8)), "y": [1, {"n": 2}]})
    for other in ({"x": (np.arange(5, dtype=np.uint64), b"ab")}, {"x": (np.arange(6, dtype=np.uint64), b"ab"), "y": [1, {"n": 2}]},
                  {"x": (np.arange(5, dtype=np.uint64), b"ac"), "y": [1, {"n": 2}]},
                  {"x": (np.arange(5, dtype=np.uint64), b"ab"), "y": [1, {"n": 3}]},
                  {"x": ("error", 18, ()), "y": [1, {"n": 2}]}):
        assert not sr.same(a, other)
    assert not sr.same(np.asarray([-1], np.int64), np.asarray([2 ** 64 - 1], np.uint64))
    assert sr.differing({"a": 1, "b": 2}, {"a": 1, "c": 2}) == ["b", "c"]


# ------------------------------------------------------------------------- part A: the second tenant

@gpu
@pytest.mark.parametrize("path", ["steps", "run"])
@pytest.mark.parametrize("name", ["BIG", "SMALL", "MID"])
def test_fresh_shard_tour_equals_the_host(ctx, name, path):
    assert_tour(fresh_tour(ctx, name, path), name, path, "fresh shard")


CHAINS = [("BIG", "SMALL"), ("SMALL", "BIG"), ("BIG", "MID", "SMALL"), ("BIG", "BIG")]
PATHS = [("steps", "steps"), ("run", "steps"), ("steps", "run")]


@gpu
@pytest.mark.parametrize("paths", PATHS, ids=["%s-%s" % p for p in PATHS])
@pytest.mark.parametrize("chain", CHAINS, ids=["-".join(c) for c in CHAINS])
def test_second_tenant(ctx, chain, paths):
    sh = shard_for(ctx, chain[0])
    try:
        sr.tour(sh, ctx, chain[0], paths[0], sr.offset_of(chain[0]))
        for k, name in enumerate(chain[1:]):
            call(sh.load, sr.data_of(name), sr.offset_of(name))
            got = sr.tour(sh, ctx, name, paths[1], sr.offset_of(name))
            assert_tour(got, name, paths[1], "tenant %d after %s" % (k + 2, "-".join(chain[:k + 1])))
            assert sr.differing(got, fresh_tour(ctx, name, paths[1])) == []
    finally:
        sh.close()


def consumers_of(sh, ctx, name, starts):
    """The stages over the rows of the scan `sh` holds, in stage_expected's layout."""
    t, L = sr.tenant(name), sr.layout(name)
    F = sr.filters(len(starts))
    out = {"sam": call(sh.records_sam, L.names), "bam_scan": call(sh.records_bam, L.head, F["bam"]),
           "bam_coord": (call(sh.records_bam, L.head, None, order="coordinate"), sh.bam_sorted)}
    for key, split in (("fastq", False), ("fastq_split", True)):
        out[key] = call(sh.records_fastq, None, split=split) + (sh.fastq_sizes,)
    tal, dep, pil = ctx.tally(L.n_ref), ctx.depth(t.spans, L.n_ref), ctx.pileup(t.spans, L.n_ref)
    try:
        out["tally"] = (call(tal.add, sh, F["tally"]), call(tal.counts))
        out["depth"] = (call(dep.add, sh, F["depth"]), call(dep.finish), call(dep.runs),
                        [call(dep.depth, k) for k in range(len(t.spans))])
        out["pileup"] = (call(pil.add, sh, F["pileup"]), call(pil.finish), call(pil.intervals),
                         [call(pil.counts, k) for k in range(len(t.spans))],
                         [call(pil.calls, k) for k in range(len(t.spans))])
    finally:
        for acc in (tal, dep, pil):
            acc.close()
    return out


@gpu
def test_small_scan_after_a_large_one_on_the_same_bytes(ctx):
    L = sr.layout("BIG")
    sh = shard_for(ctx, "BIG")
    try:
        call(sh.index, sr.offset_of("BIG"))
        call(sh.inflate)
        for a, b in ((0, len(L.starts)), (100, 103)):
            starts = L.starts[a:b]
            end = L.starts[b] if b < len(L.starts) else L.seg_end
            cols = call(sh.records, starts[0], end)
            got = consumers_of(sh, ctx, "BIG", starts)
            got["records"] = dict(cols, vpos=sr.unshift_vpos(cols["vpos"], sr.offset_of("BIG")))
            want = sr.stage_expected("BIG", starts, L.head, sr.filters(len(starts)))
            want["records"] = sr.columns_expected("BIG", starts)
            want["bam_coord"] = sr.coordinate_expected("BIG", starts, L.head)
            assert sr.differing(got, want) == [], (a, b)
    finally:
        sh.close()


@gpu
def test_accumulators_reset_between_two_files(ctx):
    """One Depth, one Pileup, one Tally over SMALL's one reference: BIG's scan added and finished,
    reset(), SMALL's scan added and finished -- the host's answer for SMALL alone."""
    t, L, B = sr.tenant("SMALL"), sr.layout("SMALL"), sr.layout("BIG")
    spans = t.spans
    tal, dep, pil = ctx.tally(3), ctx.depth(spans, 3), ctx.pileup(spans, 3)  # (BIG's three references fit)
    shards = []
    try:
        for name, lay in (("BIG", B), ("SMALL", L)):
            sh = shard_for(ctx, name)
            shards.append(sh)
            call(sh.index, sr.offset_of(name))
            call(sh.inflate)
            call(sh.records_scan, lay.first, lay.seg_end)
            add = (call(tal.add, sh), call(dep.add, sh), call(pil.add, sh))
            got = {"tally": (add[0], call(tal.counts)),
                   "depth": (add[1], call(dep.finish), call(dep.runs), [call(dep.depth, 0)]),
                   "pileup": (add[2], call(pil.finish), call(pil.intervals), [call(pil.counts, 0)], [call(pil.calls, 0)])}
            flat = np.frombuffer(lay.flat, np.uint8)
            flag, ref, n_kept = sb.tally_host(flat, lay.starts, 3)
            d = sb.depth_host(flat, lay.starts, spans, 3)
            p = sb.pileup_host(flat, lay.starts, spans, 3)
            want = {"tally": ({"n": len(lay.starts), "n_kept": n_kept}, (flag, ref)),
                    "depth": (d[0], d[3], d[2], [d[1][:spans[0][2]]]),
                    "pileup": (p[0], p[4], p[3], [p[1]], [p[2]])}
            assert sr.differing(got, want) == [], name
            for acc in (tal, dep, pil):
                call(acc.reset)
    finally:
        for a in [tal, dep, pil] + shards:
            a.close()


STREAM_KEYS = ("n_windows", "n_blocks", "comp_bytes", "flat_bytes", "n_true", "count", "first_vpos", "exit_vpos", "status",
               "crc_bad_blocks", "crc_first_bad")


def stream_over(c, name, window):
    t, L = sr.tenant(name), sr.layout(name)
    s, bits = call(c.run_stream, sr.data_of(name), L.lens, index_start=0, window=window, halo=1 << 16, want_bits=True,
                   splits=sr.splits_of(len(t.data)), verify_crc=True)
    return ({k: s[k] for k in STREAM_KEYS}, bits, s["split_status"], s["split_first_vpos"], s["split_count"])


@gpu
def test_context_window_cache_serves_a_second_file(ctx):
    big, small = sr.tenant("BIG"), sr.expected("SMALL")
    # (windows are cut at member and split starts: a window of half the file gives two or three)
    first = stream_over(ctx, "BIG", len(big.data) // 2 + 1)
    assert first[0]["n_windows"] >= 2 and first[0]["status"] == 0
    got = stream_over(ctx, "SMALL", 1 << 20)
    with sb.Context(0) as other:
        fresh = stream_over(other, "SMALL", 1 << 20)
    assert sr.same(got, fresh)
    res, bits, status, first_vpos, count = got
    assert res["count"] == 3 == small["run"]["count"] and res["n_true"] == small["eager"][0]
    assert res["first_vpos"] == small["run"]["first_vpos"] and res["crc_bad_blocks"] == 0
    assert sr.same(bits, small["eager"][1])
    want_status, want_first, want_count = small["split_starts"]
    assert sr.same(status, want_status) and sr.same(count, want_count)
    assert sr.same(np.where(count > 0, first_vpos, 0), want_first)


# ------------------------------------------------------------------------- part B: the invalidation table

EVENTS = ("load_same", "index_0", "index_2nd_inflate", "run_2nd", "inflate_again", "contigs_same", "contigs_more",
          "scan_sub", "scan_fails", "bam_refused")
CONSUMERS = ("records_fetch", "records_sam", "sam_fetch",
             "records_bam", "bam_fetch", "bam_read", "bam_sorted",
             "records_fastq", "fastq_fetch",
             "bai_fetch", "bai_edges",
             "tally_add", "depth_add", "pileup_add",
             "eager_bits", "count_records")
# S: SBH_E_STATE (an accumulator left as it was); V: the host's value for the bytes and rows now current.
# Columns in CONSUMERS' order, grouped as there: records | BAM | FASTQ | BAI | accumulators | bitmap, count.
TABLE = {
    # load, index and run void everything scan-derived and everything inflate-derived
    "load_same":         "SSS SSSS SS SS SSS SS",
    "index_0":           "SSS SSSS SS SS SSS SS",
    "index_2nd_inflate": "SSS SSSS SS SS SSS SV",  # (inflated again: the chain can be counted; no bitmap yet)
    "run_2nd":           "SSS SSSS SS SS SSS VV",  # (the run leaves its bitmap)
    # the same bytes at the same offsets: the scan stays, the bitmap goes
    "inflate_again":     "VVV VVVV VV VV VVV SV",
    # set_contigs voids the BAI scan and the bitmap, the same lengths or not
    "contigs_same":      "VVV VVVV VV SS VVV SV",
    "contigs_more":      "VVV VVVV VV SS VVV SV",
    # a new scan voids SAM, BAM and FASTQ: the scans render the new rows, the fetches have nothing
    "scan_sub":          "VVS VSSS VS VV VVV VV",
    # a failed scan leaves no valid scan; the BAI scan and the bitmap are not its business
    "scan_fails":        "SSS SSSS SS VV SSS VV",
    # a refused filter leaves the last good result
    "bam_refused":       "VVV VVVV VV VV VVV VV",
}
B_FILTER = {"flag_exclude": 0x10}
BAD_FILTER = {"min_mapq": 256}
SUB = (100, 103)


def test_the_table_has_a_cell_for_every_event_and_consumer():
    assert tuple(TABLE) == EVENTS and len(set(CONSUMERS)) == len(CONSUMERS) == 16 and len(EVENTS) == 10
    for ev in EVENTS:
        row = TABLE[ev].replace(" ", "")
        assert len(row) == len(CONSUMERS) and set(row) <= {"S", "V"}, ev
    # the rule, where it can be said in one line: nothing scan-derived survives a load, an index or a run
    for ev in ("load_same", "index_0", "index_2nd_inflate", "run_2nd"):
        assert TABLE[ev].replace(" ", "")[:14] == "S" * 14


class World:
    """MID_B on the host: what the setup leaves, and what each consumer must give after an event."""

    def __init__(self):
        self.name = "MID_B"
        self.t, self.L = sr.tenant(self.name), sr.layout(self.name)
        L = self.L
        self.flat = np.frombuffer(L.flat, np.uint8)
        self.data = sr.data_of(self.name)
        self.m2, self.u2 = L.members[1][0], L.members[1][2]  # the second member: file offset, flat offset
        self.bad_start = L.all_starts[-1]
        self.sam = sb.sam_text_host(self.flat, L.starts, L.names)
        self.bam = sr.coordinate_expected(self.name, L.starts, L.head)[0]
        self.fastq = sb.fastq_host(self.flat, L.starts)
        self.bai = sr.bai_expected(self.name, (0, len(L.starts)))
        self.edges = sr.edges_expected(self.name, (0, len(L.starts)))
        self._acc = {}

    def rows(self, ev):
        a, b = SUB if ev == "scan_sub" else (0, len(self.L.starts))
        return self.L.starts[a:b]

    def accumulated(self, adds):
        """(tally counts, depth's finish, pileup counts) after the full scan was added `adds[0]` times
        and then the rows of adds[1:] each once."""
        key = tuple(tuple(s) for s in adds)
        if key not in self._acc:
            t, L = self.t, self.L
            flag = ref = slots = counts = None
            last = {}
            for starts in adds:
                flag, ref, kept = sb.tally_host(self.flat, starts, L.n_ref, None, flag=flag, ref=ref)
                last["tally"] = {"n": len(starts), "n_kept": kept}
                last["depth"], slots = sb.depth_host(self.flat, starts, t.spans, L.n_ref, None, slots=slots, finish=False)
                last["pileup"], counts = sb.pileup_host(self.flat, starts, t.spans, L.n_ref, None, counts=counts, finish=False)
            depth, runs, sizes = sb.coverage.finish_host(slots.copy(), t.spans)
            self._acc[key] = (last, (flag, ref), (sizes, runs), counts)
        return self._acc[key]


@pytest.fixture(scope="module")
def world():
    return World()


def set_up(ctx, W):
    """A fresh shard through every stage, and the three accumulators holding its scan once."""
    L, t = W.L, W.t
    sh = ctx.shard(W.data)
    call(sh.index, 0)
    call(sh.inflate)
    call(sh.set_contigs, L.lens)
    call(sh.check_eager, 0, sh.flat_size, want_bits=False)
    assert call(sh.records_scan, L.first, L.seg_end) == len(L.starts)
    assert sr.same(call(sh.records_sam, L.names), W.sam)
    assert sr.same(call(sh.records_bam, L.head, None, order="coordinate"), W.bam)
    assert sr.same(call(sh.records_fastq), W.fastq[:3])
    assert sr.same(call(sh.bai_scan, L.first, L.seg_end), W.bai)
    acc = {"tally_add": ctx.tally(L.n_ref), "depth_add": ctx.depth(t.spans, L.n_ref), "pileup_add": ctx.pileup(t.spans, L.n_ref)}
    for a in acc.values():
        call(a.add, sh)
    return sh, acc


def happen(ev, sh, W):
    L = W.L
    if ev == "load_same":
        call(sh.load, W.data, 0)
    elif ev == "index_0":
        call(sh.index, 0)
    elif ev == "index_2nd_inflate":
        call(sh.index, W.m2)
        call(sh.inflate)
    elif ev == "run_2nd":
        r = call(sh.run, W.m2, len(W.t.data))
        assert r["status"] == 0 and r["flat_bytes"] == len(L.flat) - W.u2
    elif ev == "inflate_again":
        call(sh.inflate)
    elif ev == "contigs_same":
        call(sh.set_contigs, L.lens)
    elif ev == "contigs_more":
        call(sh.set_contigs, list(L.lens) + [777])
    elif ev == "scan_sub":
        assert call(sh.records_scan, L.starts[SUB[0]], L.starts[SUB[1]]) == SUB[1] - SUB[0]
    elif ev == "scan_fails":
        with pytest.raises(sb.SparkBamError) as e:
            call(sh.records_scan, W.bad_start, len(L.flat))
        assert e.value.code == SBH_E_BAD_RECORD
    elif ev == "bam_refused":
        with pytest.raises(sb.SparkBamError) as e:
            call(sh.records_bam, L.head, BAD_FILTER)
        assert e.value.code == SBH_E_ARG
    else:
        raise AssertionError(ev)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def consume(c, ev, sh, acc, W):
    """Consumer c after event ev: (what it gave, what the host says it must give when the cell is V)."""
    L, lib = W.L, sb.lib()
    rows = W.rows(ev)
    if c == "records_fetch":
        want = sr.columns_expected(W.name, rows)
        sz = sb._lib.SbhRecordsSizes(len(rows), want["names"].size, want["cigar"].size, want["seq"].size, want["aux"].size)
        return sh._records_fetch(sz), want
    if c == "records_sam":
        return sh.records_sam(L.names), sb.sam_text_host(W.flat, rows, L.names)
    if c == "sam_fetch":
        text, off = np.empty(W.sam[0].size, np.uint8), np.zeros(len(L.starts) + 1, np.uint64)
        sh._c(lib.sbh_records_sam_fetch(sh.h, _p(text), _p(off)))
        return (text, off), W.sam
    if c == "records_bam":
        return sh.records_bam(L.head, B_FILTER), sb.bam_gather_host(W.flat, rows, L.head, B_FILTER)
    if c == "bam_fetch":
        got = tuple(np.zeros_like(x) for x in W.bam)
        sh._c(lib.sbh_records_bam_fetch(sh.h, *(_p(x) for x in got)))
        return got, W.bam
    if c == "bam_read":
        return sh.bam_read(0, W.bam[0].size), W.bam[0]
    if c == "bam_sorted":
        return sh.bam_sorted, True
    if c == "records_fastq":
        return sh.records_fastq(), sb.fastq_host(W.flat, rows)[:3]
    if c == "fastq_fetch":
        got = tuple(np.zeros_like(x) for x in W.fastq[:3])
        sh._c(lib.sbh_records_fastq_fetch(sh.h, *(_p(x) for x in got)))
        return got, W.fastq[:3]
    if c == "bai_fetch":
        runs, lin = np.zeros_like(W.bai[0]), np.zeros_like(W.bai[1])
        sh._c(lib.sbh_bai_fetch(sh.h, _p(runs), _p(lin)))
        return (runs, lin), W.bai[:2]
    if c == "bai_edges":
        return sh.bai_edges(), W.edges
    if c in acc:
        return acc[c].add(sh), W.accumulated([L.starts, rows])[0][c.split("_")[0]]
    if c == "eager_bits":
        k = 1 if ev == "run_2nd" else 0
        return sh.eager_bits(0, len(L.flat) - (W.u2 if k else 0)), sr.eager_expected(W.name, k)[1]
    if c == "count_records":
        u = W.u2 if ev in ("index_2nd_inflate", "run_2nd") else 0
        inside = [s - u for s in L.starts if s >= u]
        return sh.count_records(inside[0], L.seg_end - u), len(inside)
    raise AssertionError(c)


def accumulator_holds(c, a, W, adds):
    """The accumulator behind consumer c holds exactly the adds given."""
    _, tally, (sizes, runs), counts = W.accumulated(adds)
    if c == "tally_add":
        return sr.same(call(a.counts), tally)
    if c == "depth_add":
        return sr.same((call(a.finish), call(a.runs)), (sizes, runs))
    got = np.concatenate([call(a.counts, k) for k in range(len(W.t.spans))])
    return sr.same(got, counts)


@gpu
@pytest.mark.parametrize("ev", EVENTS)
def test_invalidation_table(ctx, world, ev):
    W, cells = world, 0
    row = TABLE[ev].replace(" ", "")
    for c, outcome in zip(CONSUMERS, row):
        sh, acc = set_up(ctx, W)
        try:
            happen(ev, sh, W)
            if outcome == "S":
                with pytest.raises(sb.SparkBamError) as e:
                    call(consume, c, ev, sh, acc, W)
                assert e.value.code == SBH_E_STATE, (ev, c, e.value)
                if c in acc:
                    assert accumulator_holds(c, acc[c], W, [W.L.starts]), (ev, c)
            else:
                got, want = call(consume, c, ev, sh, acc, W)
                assert sr.same(got, want), (ev, c)
                if c in acc:
                    assert accumulator_holds(c, acc[c], W, [W.L.starts, W.rows(ev)]), (ev, c)
            cells += 1
        finally:
            for a in list(acc.values()) + [sh]:
                a.close()
    assert cells == len(CONSUMERS)
