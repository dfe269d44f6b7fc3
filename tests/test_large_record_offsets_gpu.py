"""Record stages with flat offsets past 2^31 and 2^32.  A resident shard holds several GB of flat
bytes, so every kernel that takes a record's flat start adds it to a 64-bit base in production; the
stages' conformance corpora all lie in files of a few hundred KB, where a start needs 20 bits.

The stages are translation invariant, so the same hand-built corpora are replayed here behind a gap
of zeros (shifted_corpus.py) that puts the middle record's byte 0 (its start has bit 31 alone, or no
low bit at all, set) or byte 2 (the boundary inside its block_size word) exactly on 2^31 or on 2^32,
with the rest of the corpus on either side, and compared with the references the unshifted tests
use.  Only flat starts, virtual positions and BAI offsets move; they are remapped on the host through
the two member tables.  A stage's corpora lie one after another behind one gap, each scanned at its
own row range, and the whole set is laid three times (thrice()): once wholly below the boundary,
once with the boundary in its middle record, once wholly above it -- so every case of every corpus,
a long CIGAR handed round a wave as much as a one-op read, meets offsets on both sides.  The
interval, split and BAI corpora, which cannot be repeated, lie once with their middle record across.

Every comparison is exact equality; nothing the device returns goes into an expected value; nothing
as large as the gap comes to the host.  test_large_offsets_gpu.py and test_large_comp_offsets_gpu.py
cover the index, inflate, CRC, the checkers and the split prologue in the same way."""
import contextlib
import functools
import time

import numpy as np
import pytest

import bai_ref
import bam_gather_corpus as bc
import bam_sort_corpus as bsc
import depth_corpus as dc
import fastq_corpus as fc
import oracle_records as orr
import pileup_corpus as pc
import record_corpus as rc
import sam_corpus as smc
import shifted_corpus as sc
import tally_corpus as tc
import test_bam_gather_gpu as t_gather
import test_bam_sort_gpu as t_sort
import test_depth_gpu as t_depth
import test_fastq_gpu as t_fastq
import test_pileup_gpu as t_pileup
import test_sam_gpu as t_sam
import test_tally_gpu as t_tally
from oracle_lib import OR_OK, OracleFile
from pkg import sb
from test_bai_gpu import coop_stream, hand, same_runs  # noqa: F401  (hand: the fixture)
from test_record_conformance_gpu import call

pytestmark = pytest.mark.gpu

# (boundary, byte of the middle record that lies on it, payload of the records' members)
PLACES = [(1 << b, d, p) for b in (31, 32) for d, p in ((0, 65280), (2, 4096))]
place = pytest.mark.parametrize("place", PLACES, ids=["2^%d-d%d" % (B.bit_length() - 1, d) for B, d, _ in PLACES])
CONTIG_LEN = [ln for _, ln in rc.CONTIGS]


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def across(s, where, k=None):
    """The stream behind the gap that puts byte d of its record k (the middle one) on B."""
    B, d, payload = where
    k = len(s.starts) // 2 if k is None else k
    sf = sc.shift_stream(s, B, k, d, payload)
    assert sf.starts[k] == B - d and sf.starts[0] < B < sf.starts[-1]
    return sf, k


def thrice(parts, middle=None):
    """parts, parts again (or the one part `middle`, an index), parts once more, behind one header:
    (the Stream, [(index into parts, (first row, one past the last))] as laid, the middle row of
    the middle block).  With that row on the boundary every part lies wholly below it once and
    wholly above it once, and the middle block has rows on both sides."""
    order = list(range(len(parts)))
    order = order + (order if middle is None else [middle]) + order
    s, rows = sc.combine([parts[i] for i in order])
    a, b = rows[len(parts)][0], rows[-len(parts) - 1][1]
    return s, list(zip(order, rows)), (a + b) // 2


@contextlib.contextmanager
def resident(ctx, sf):
    """The file on a shard, indexed and inflated once; closed on the way out."""
    sh = ctx.shard(sf.data)
    try:
        t0 = time.perf_counter()
        _, fs = call(sh.index, 0)
        t1 = time.perf_counter()
        call(sh.inflate)
        print("%.2f GiB flat in %d members: index %.0f ms, inflate %.0f ms"
              % (fs / 2 ** 30, len(sf.members), 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)))
        assert fs == sf.flat_size
        yield sh
    finally:
        sh.close()


def scan_rows(sh, sf, rows):
    """records_scan over rows [lo, hi) of the shifted stream."""
    lo, hi = rows
    end = sf.starts[hi] if hi < len(sf.starts) else sf.flat_size
    assert call(sh.records_scan, sf.starts[lo], end) == hi - lo


def cols_equal(got, want):
    """test_records_gpu.assert_cols_equal without `flat`, which moves (and is compared on its own)."""
    assert set(got) - {"flat", "vpos"} == set(want) - {"flat"}
    for k in set(want) - {"flat"}:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------------- addressing helpers

@place
def test_addressing_helpers(ctx, place):
    s = rc.interval_stream()
    sf, k = across(s, place)
    B, P = place[0], sf.shift
    with resident(ctx, sf) as sh:
        assert call(sh.read_flat, B - 8, 16).tobytes() == s.flat[B - 8 - P:B + 8 - P]
        assert not call(sh.read_flat, sf.first - 16, 16).any()  # (the gap's last bytes)
        for f, v in zip(sf.starts[k - 1:k + 2], sc.vpos_of(sf.members, sf.starts[k - 1:k + 2]).tolist()):
            assert call(sh.pos_of, f) == (v >> 16, v & 0xFFFF)
            assert call(sh.flat_of, v >> 16, v & 0xFFFF) == f


# ------------------------------------------------------------------------- records, records_scan

@place
def test_records(ctx, place):
    """The decode stream three times over, the middle copy's middle record on the boundary: every
    case (the 65535-op CIGAR, the 255-byte name, ...) lies below it once and above it once."""
    s, _, k = thrice([rc.decode_stream()])
    sf, k = across(s, place, k)
    n = len(s.starts)
    want = rc.expected_columns(rc.DECODE_CASES * 3)
    with resident(ctx, sf) as sh:
        got = call(sh.records, sf.first, sh.flat_size)
        assert got["flat"].tolist() == sf.starts
        cols_equal(got, want)
        assert got["vpos"].tolist() == sc.vpos_of(sf.members, sf.starts).tolist()
        # from the record on the boundary on, without the copy-out; then those rows
        assert call(sh.records_scan, sf.starts[k], sf.starts[-1]) == n - 1 - k
        sub = call(sh.records, sf.starts[k], sf.starts[-1])
        assert sub["flat"].tolist() == sf.starts[k:-1]
        cols_equal(sub, orr.decode(s.flat, s.starts[k:-1]))


# ------------------------------------------------------------------------- records_regions

@place
def test_records_regions(ctx, place):
    s = rc.interval_stream()
    sf, k = across(s, place)
    P = sf.shift
    whole = [(s.first, len(s.flat))]
    cases = [(c.name, whole, c.intervals, c.kept) for c in rc.INTERVAL_CASES]
    cases += [(c.name, rc.chunk_flats(c), rc.ALL_INTERVALS, c.kept) for c in rc.CHUNK_CASES]
    with resident(ctx, sf) as sh:
        for name, chunks, intervals, kept in cases:
            got = call(sh.records_regions, [(a + P, b + P) for a, b in chunks], list(intervals))
            flats = [rc.interval_start(x) + P for x in kept]
            assert got["flat"].tolist() == flats, name
            assert got["vpos"].tolist() == sc.vpos_of(sf.members, flats).tolist(), name
            cols_equal(got, orr.interval_records(s.flat, chunks, rc.loci_by_ref(intervals))[0])


# ------------------------------------------------------------------------- split_records_batch

E_NO_READ_FOUND = sb._lib.SBH_E_NO_READ_FOUND


@place
@pytest.mark.parametrize("from_zero", (False, True), ids=("from_records", "from_zero"))
def test_split_records_batch(ctx, place, from_zero):
    """Three splits of the compressed range from the records' first member to the end of the file.
    What each split holds is the CPU oracle's answer for the same split of the file without the gap
    (member for member the same bytes behind it), its virtual positions moved by the gap's
    compressed size; the rows are the shifted starts, their virtual positions from the member table.

    The call indexes from its first split's member, so those three alone see flat offsets that count
    from the records' first member.  from_zero puts a split over the header and the gap in front: the
    index then starts at the file's start, the three splits' records lie at their flat offsets past the
    boundary, and the split in front answers NoReadFoundException (no record within maxReadSize =
    100 000 000 positions of Pos(0, 0); the first lies 2^31 bytes on or more)."""
    s = rc.decode_stream()
    sf, _ = across(s, place)
    twin = sc.unshifted(s.flat, s.first, s.starts, place[2])
    lo, hi = int(sf.members[sf.rec_member, 0]), int(sf.data.size)
    dc_ = lo - int(twin.members[twin.rec_member, 0])
    cut = [lo, lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3, hi]
    splits = list(zip(cut[:-1], cut[1:]))
    of = OracleFile(twin.data.copy())
    want = [of.split(a - dc_, b - dc_) for a, b in splits]
    of.close()
    assert all(r == OR_OK for r, _, _ in want) and sum(n for _, _, n in want) > 0
    vpos = sc.vpos_of(sf.members, sf.starts).tolist()
    base = 0 if from_zero else sf.first  # (where the call's flat offsets count from)
    with resident(ctx, sf) as sh:
        call(sh.set_contigs, CONTIG_LEN)
        info, per, cols = call(sh.split_records_batch, ([(0, lo)] if from_zero else []) + splits)
        assert info["block_start"] == (0 if from_zero else lo)
        if from_zero:
            front = per.pop(0)
            assert (front["status"], front["rec_count"], front["block_start"]) == (E_NO_READ_FOUND, 0, 0)
        rows, delivered = 0, []
        for i, ((_, v, n), p) in enumerate(zip(want, per)):
            assert (p["status"], p["rec_count"], p["rec_begin"]) == (0, n, rows), i
            if n:
                v += dc_ << 16
                assert p["first_vpos"] == v, i
                at = vpos.index(v)
                assert cols["vpos"][rows:rows + n].tolist() == vpos[at:at + n], i
                assert cols["flat"][rows:rows + n].tolist() == [f - base for f in sf.starts[at:at + n]], i
                delivered += range(at, at + n)
            rows += n
        assert info["n"] == rows == cols["vpos"].size
        cols_equal(cols, orr.decode(s.flat, [s.starts[i] for i in delivered]))


# ------------------------------------------------------------------------- bai_scan

def bai_across(ctx, data, where, payload):
    """bai_ref.build of the unshifted file, every virtual offset remapped through the two member
    tables, against Shard.bai_scan of the shifted one."""
    want = bai_ref.build(data)
    blocks, flat = bai_ref.members(data)
    old = np.asarray(blocks, np.int64)
    lens, first = bai_ref.contigs_of(flat)
    sf, _ = across(rc.Stream(flat, first, [r.start for r in want.records]), where[:2] + (payload,))
    runs = want.runs.copy()
    for key in ("vbeg", "vend"):
        runs[key] = sc.remap_vpos(old, sf.members, sf.shift, want.runs[key])
    lin = sc.remap_vpos(old, sf.members, sf.shift, want.lin)
    assert (runs["vbeg"] >> np.uint64(16)).min() >= sf.members[sf.rec_member, 0]
    with resident(ctx, sf) as sh:
        call(sh.set_contigs, lens)
        got_runs, got_lin, nnc = call(sh.bai_scan, sf.first, sh.flat_size)
    assert same_runs(got_runs, runs), (got_runs, runs)
    assert np.array_equal(got_lin, lin) and nnc == want.n_no_coor


@place
def test_bai_scan_hand_corpus(ctx, place, hand):  # noqa: F811
    bai_across(ctx, hand[1], place, 300)


@place
def test_bai_scan_cooperative_cigar_sum(ctx, place):
    bai_across(ctx, coop_stream(), place, 700)


# ------------------------------------------------------------------------- records_sam

@place
def test_records_sam(ctx, place):
    """The corpus three times over, each copy scanned and rendered on its own: below the boundary,
    across it at its middle record, above it."""
    s, laid, k = thrice([smc.stream()])
    sf, _ = across(s, place, k)
    want_text, want_off = t_sam.corpus_want()
    with resident(ctx, sf) as sh:
        for _, (lo, hi) in laid:
            end = sf.starts[hi] if hi < len(sf.starts) else sf.flat_size
            assert call(sh.records, sf.starts[lo], end)["flat"].tolist() == sf.starts[lo:hi]
            text, line_off = call(sh.records_sam, smc.REF_NAMES)
            assert sh.sam_n_host == len(smc.FLOAT_ROWS)
            assert np.array_equal(line_off, want_off)
            for i, (label, _) in enumerate(smc.CASES):
                a, b = int(want_off[i]), int(want_off[i + 1])
                assert bytes(text[a:b]) == bytes(want_text[a:b]), label
            assert text.size == want_text.size


# ------------------------------------------------------------------------- records_bam, scan order

@functools.lru_cache(maxsize=None)
def gather_streams():
    return thrice([s for _, s in bc.streams()])


@place
def test_records_bam(ctx, place):
    s, laid, k = gather_streams()
    sf, _ = across(s, place, k)
    with resident(ctx, sf) as sh:
        for i, r in laid:
            kind, part = bc.streams()[i]
            scan_rows(sh, sf, r)
            n = len(part.starts)
            for head in (bc.HEADS[0], bc.HEADS[5], rc.header()):
                for pattern in bc.PATTERNS:
                    t_gather.same_as_host(sh, part.flat, part.starts, head, rows=bc.pattern_ranges(pattern, n))
            if kind == "ladder":  # every (source mod 16, destination mod 16) pair
                for head in bc.HEADS:
                    t_gather.same_as_host(sh, part.flat, part.starts, head, rows=bc.LADDER_ROWS)
            t_gather.same_as_host(sh, part.flat, part.starts, rc.header(), flag_exclude=0x4, min_mapq=7)


# ------------------------------------------------------------------------- records_bam, coordinate order

SORT_NAMES = tuple(k for k in bsc.SMALL if len(bsc.stream(k).starts))
ACROSS_SORT = "shuffled"


@functools.lru_cache(maxsize=None)
def sort_streams():
    """Every corpus, the shuffled one across the boundary, every corpus again."""
    return thrice([bsc.stream(k) for k in SORT_NAMES], SORT_NAMES.index(ACROSS_SORT))


@place
def test_records_bam_coordinate_order(ctx, place):
    s, laid, k = sort_streams()
    lo, hi = laid[len(SORT_NAMES)][1]
    assert laid[len(SORT_NAMES)][0] == SORT_NAMES.index(ACROSS_SORT) and lo < k < hi
    sf, k = across(s, place, k)
    # in the sorted result the rows from below the boundary and those from above it interleave
    above = bsc.expected_perm(ACROSS_SORT) >= np.uint64(k - lo)
    assert np.count_nonzero(above[1:] != above[:-1]) > 100
    with resident(ctx, sf) as sh:
        for i, r in laid:
            name = SORT_NAMES[i]
            part = bsc.stream(name)
            scan_rows(sh, sf, r)
            got = t_sort.same_as_host(sh, part.flat, part.starts, rc.header())
            assert np.array_equal(got[2], bsc.expected_perm(name)), name
            t_sort.same_as_host(sh, part.flat, part.starts, b"abc", flag_exclude=0x10, rows=[(1, 3 * (r[1] - r[0]) // 4 + 2)])


# ------------------------------------------------------------------------- depth

DEPTH_NAMES = tuple(k for k in dc.SMALL if t_depth.in_file_order(dc.get(k)))


@functools.lru_cache(maxsize=None)
def depth_streams():
    return thrice([dc.get(k) for k in DEPTH_NAMES])


@place
def test_depth(ctx, place):
    s, laid, k = depth_streams()
    sf, _ = across(s, place, k)
    with resident(ctx, sf) as sh:
        for i, r in laid:
            name = DEPTH_NAMES[i]
            c, want = dc.get(name), dc.expected(name)
            scan_rows(sh, sf, r)
            acc = ctx.depth(c.spans, dc.N_REF, c.count_del)
            try:
                assert call(acc.add, sh, c.filter) == want["add"], name
                t_depth.finished_equals(acc, want, c.spans)
            finally:
                acc.close()


# ------------------------------------------------------------------------- pileup

PILEUP_NAMES = tuple(k for k in pc.SMALL if t_pileup.in_file_order(pc.get(k)))


@functools.lru_cache(maxsize=None)
def pileup_streams():
    return thrice([pc.get(k) for k in PILEUP_NAMES])


@place
def test_pileup(ctx, place):
    s, laid, k = pileup_streams()
    sf, _ = across(s, place, k)
    with resident(ctx, sf) as sh:
        for i, r in laid:
            name = PILEUP_NAMES[i]
            c, want = pc.get(name), pc.expected(name)
            scan_rows(sh, sf, r)
            acc = ctx.pileup(c.spans, pc.N_REF, c.min_baseq)
            try:
                add = call(acc.add, sh, c.filter)
                assert add == want["add"], name
                t_pileup.counts_equal(acc, want, c.spans)
                sizes = t_pileup.finished_equals(acc, want, c.spans, c.min_depth, c.call_pct)
                assert sizes["totals"] == add["totals"], name
            finally:
                acc.close()


# ------------------------------------------------------------------------- tally

TALLY_NAMES = tuple(k for k in tc.SMALL if tc.in_file_order(tc.get(k)) and tc.get(k).starts)


@functools.lru_cache(maxsize=None)
def tally_streams():
    return thrice([tc.get(k) for k in TALLY_NAMES])


@place
def test_tally(ctx, place):
    s, laid, k = tally_streams()
    sf, _ = across(s, place, k)
    with resident(ctx, sf) as sh:
        for i, r in laid:
            name = TALLY_NAMES[i]
            c, want = tc.get(name), tc.expected(name)
            scan_rows(sh, sf, r)
            acc = ctx.tally(c.n_ref)
            try:
                assert call(acc.add, sh, c.filter) == t_tally.added(want), name
                t_tally.counts_equal(acc, want)
            finally:
                acc.close()


# ------------------------------------------------------------------------- records_fastq

FASTQ_NAMES = tuple(k for k in fc.SMALL if fc.get(k).starts)


@functools.lru_cache(maxsize=None)
def fastq_streams():
    return thrice([fc.get(k) for k in FASTQ_NAMES])


@place
def test_records_fastq(ctx, place):
    """Every corpus under every variant: one stream, and split three ways (read 1, read 2, others)."""
    s, laid, k = fastq_streams()
    sf, _ = across(s, place, k)
    assert any(kw.get("split") for k in FASTQ_NAMES for kw in fc.VARIANTS[k])
    with resident(ctx, sf) as sh:
        for i, r in laid:
            name = FASTQ_NAMES[i]
            scan_rows(sh, sf, r)
            for v, kw in enumerate(fc.VARIANTS[name]):
                t_fastq.device_equals(sh, fc.get(name), fc.expected(name, v), **kw)
