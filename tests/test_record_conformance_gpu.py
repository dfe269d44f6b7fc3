"""Record delivery conformance on the GPU: the hand-built streams of record_corpus.py through
Shard.records and Shard.records_regions (k_chain_positions / the bitmap and chain-marking
paths, k_rec_sizes, k_rec_fields, k_region_keep, k_compact_u64, k_rec_vpos), column for column
against oracle_records and, for the interval and chunk tables, against the kept records written
down by hand.  test_record_corpus_cpu.py holds the oracle to the same literals.

Every table runs twice: with no eager pass (record starts by the sequential chain walk) and
after set_contigs + check_eager over the whole stream (starts from the bitmap, or -- where the
checker rejects some of these deliberately odd records -- from the chain marked through it).
RecordStream follows block_size whatever a checker thinks, so both give the same rows."""
import functools

import numpy as np
import pytest

from oracle_lib import OracleFile
import oracle_records as orr
from pkg import sb
import record_corpus as rc
from test_records_gpu import assert_cols_equal

pytestmark = pytest.mark.gpu

SBH_E_ARG, SBH_E_HIP, SBH_E_BAD_RECORD = sb._lib.SBH_E_ARG, sb._lib.SBH_E_HIP, sb._lib.SBH_E_BAD_RECORD
WAYS = ("chain", "eager")


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
        if e.code == SBH_E_HIP:
            pytest.exit("HIP error: %s" % e, returncode=3)
        raise


@functools.lru_cache(maxsize=None)
def built(kind, payload):
    """(the stream, its BGZF file, the oracle over the file) -- built once per module."""
    streams = {"decode": rc.decode_stream, "interval": rc.interval_stream}
    s = streams[kind]() if kind in streams else {m.name: m.stream for m in rc.MALFORMED_CASES}[kind]
    data = np.frombuffer(rc.bgzf(s.flat, payload), np.uint8).copy()
    return s, data, OracleFile(data)


@functools.lru_cache(maxsize=None)
def decode_want():
    s = rc.decode_stream()
    return orr.decode(s.flat, orr.record_starts(s.flat, s.first, len(s.flat)))


def open_shard(ctx, s, data, of, way):
    """The file resident and inflated; way "eager": the eager bitmap over the whole stream."""
    sh = ctx.shard(data)
    _, fs = call(sh.index, 0)
    call(sh.inflate)
    assert fs == len(s.flat)
    if way == "eager":
        call(sh.set_contigs, of.contig_len)
        n, bits = call(sh.check_eager, 0, fs)
        n_ref, bits_ref = of.eager_range(0, fs)
        assert n == n_ref and np.array_equal(bits, bits_ref)  # (the bitmap delivery starts from is the oracle's)
    return sh


def vpos_of(of, flats):
    return [(lambda b, o: b << 16 | o)(*of.pos_of(int(f))) for f in flats]


# ------------------------------------------------------------------------- decode table

@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("payload", rc.PAYLOADS)
def test_decode_table(ctx, payload, way):
    s, data, of = built("decode", payload)
    if way == "eager":  # the bitmap is not the chain: delivery has to mark the chain through it
        _, bits = of.eager_range(0, of.flat_size)
        assert not all(bits[p >> 3] >> (p & 7) & 1 for p in s.starts)
    sh = open_shard(ctx, s, data, of, way)
    try:
        got = call(sh.records, s.first, sh.flat_size)
        assert got["flat"].tolist() == s.starts
        assert_cols_equal(got, decode_want())
        assert got["vpos"].tolist() == vpos_of(of, s.starts)
        # a sub-range from a later record on: the same rows
        k = len(s.starts) // 2
        sub = call(sh.records, s.starts[k], s.starts[-1])
        assert_cols_equal(sub, orr.decode(s.flat, s.starts[k:-1]))
    finally:
        sh.close()


# ------------------------------------------------------------------------- interval and chunk tables

@pytest.fixture(scope="module", params=[(w, p) for w in WAYS for p in (65280, 97)], ids=lambda x: "%s-%d" % x)
def interval_shard(ctx, request):
    way, payload = request.param
    s, data, of = built("interval", payload)
    sh = open_shard(ctx, s, data, of, way)
    yield sh, s, of
    sh.close()


def check_regions(sh, s, of, chunks, intervals, kept_labels):
    got = call(sh.records_regions, chunks, list(intervals))
    assert got["flat"].tolist() == [rc.interval_start(x) for x in kept_labels]
    want, per = orr.interval_records(s.flat, chunks, rc.loci_by_ref(intervals))
    assert_cols_equal(got, want)
    assert got["vpos"].tolist() == vpos_of(of, want["flat"])
    return per


@pytest.mark.parametrize("case", rc.INTERVAL_CASES, ids=lambda c: c.name)
def test_interval_table(interval_shard, case):
    sh, s, of = interval_shard
    check_regions(sh, s, of, [(s.first, sh.flat_size)], case.intervals, case.kept)


def test_chain_count_from_every_record(interval_shard):
    """The chain counted from each record on, whether or not the eager checker accepts that
    record: set bits further on that chain among themselves are not the chain from it."""
    sh, s, of = interval_shard
    n = len(s.starts)
    for k, p in enumerate(s.starts):
        assert call(sh.count_records, p, sh.flat_size) == n - k, k
        assert call(sh.chain_from, p, s.starts[-1]) == (n - 1 - k, s.starts[-1]), k


@pytest.mark.parametrize("case", rc.CHUNK_CASES, ids=lambda c: c.name)
def test_chunk_table(interval_shard, case):
    sh, s, of = interval_shard
    per = check_regions(sh, s, of, rc.chunk_flats(case), rc.ALL_INTERVALS, case.kept)
    assert tuple(per) == case.per


@pytest.mark.parametrize("name,intervals,chunk_past", rc.INTERVAL_ARG_ERRORS, ids=[e[0] for e in rc.INTERVAL_ARG_ERRORS])
def test_interval_argument_errors(interval_shard, name, intervals, chunk_past):
    sh, s, of = interval_shard
    chunks = [(sh.flat_size + 1, sh.flat_size + 2)] if chunk_past else [(s.first, sh.flat_size)]
    with pytest.raises(sb.SparkBamError) as e:
        call(sh.records_regions, chunks, list(intervals))
    assert e.value.code == SBH_E_ARG
    # the shard still answers
    check_regions(sh, s, of, [(s.first, sh.flat_size)], rc.ALL_INTERVALS, rc.ALL_KEPT)


# ------------------------------------------------------------------------- malformed records

@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("payload", (65280, 97))
@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed_record(ctx, m, payload, way):
    """records and records_regions raise SBH_E_BAD_RECORD (the calls return: the chain walks stop
    on a block_size that does not advance), and the shard then still delivers the good prefix."""
    s, data, of = built(m.name, payload)
    sh = open_shard(ctx, s, data, of, way)
    try:
        with pytest.raises(sb.SparkBamError) as e:
            call(sh.records, s.first, sh.flat_size)
        assert e.value.code == SBH_E_BAD_RECORD
        with pytest.raises(sb.SparkBamError) as e:
            call(sh.records_regions, [(s.first, sh.flat_size)], list(rc.BAD_KEEPING_INTERVALS))
        assert e.value.code == SBH_E_BAD_RECORD
        good = orr.decode(s.flat, s.starts[:3])
        assert_cols_equal(call(sh.records, s.first, m.bad_start), good)
        assert_cols_equal(call(sh.records_regions, [(s.first, m.bad_start)], list(rc.BAD_KEEPING_INTERVALS)), good)
    finally:
        sh.close()


# ------------------------------------------------------------------------- grid stride

def rows(cols, a, b):
    """Rows [a, b) of a column dict, offsets rebased (vpos dropped)."""
    out = {}
    for k in ("flat", "ref_id", "pos", "next_ref_id", "next_pos", "tlen", "flag", "bin", "mapq"):
        out[k] = cols[k][a:b]
    for off, packed in (("name_off", ("names",)), ("cigar_off", ("cigar",)), ("seq_off", ("seq", "qual")),
                        ("aux_off", ("aux",))):
        o = cols[off][a:b + 1]
        out[off] = o - o[0]
        for p in packed:
            out[p] = cols[p][int(o[0]):int(o[-1])]
    return out


@pytest.mark.parametrize("way", WAYS)
def test_grid_stride(ctx, way):
    """More records than k_rec_fields' grid has waves (262144): every row's fixed columns against
    a numpy view of the flat bytes, the first and last 2000 rows column for column against the
    oracle's decode."""
    s, a = rc.grid_stream()
    n = rc.GRID_RECORDS
    data = np.frombuffer(rc.bgzf(s.flat, 65280, level=1), np.uint8).copy()
    of = OracleFile(data)
    sh = ctx.shard(data)
    try:
        _, fs = call(sh.index, 0)
        call(sh.inflate)
        assert fs == len(s.flat)
        if way == "eager":
            call(sh.set_contigs, of.contig_len)
            assert call(sh.check_eager, 0, fs, want_bits=False)[0] == n  # (every record accepted: the bitmap path)
        got = call(sh.records, s.first, fs)
    finally:
        sh.close()
    assert got["flat"].size == n and np.array_equal(got["flat"], s.starts.astype(np.uint64))
    for k in ("ref_id", "pos", "next_ref_id", "next_pos", "tlen", "flag", "bin", "mapq"):
        assert got[k].dtype == orr.decode(s.flat, [])[k].dtype and np.array_equal(got[k], a[k]), k
    assert np.array_equal(got["name_off"], 8 * np.arange(n + 1, dtype=np.uint64))
    assert np.array_equal(got["names"].reshape(n, 8), a.view(np.uint8).reshape(n, 44)[:, 36:])
    for k in ("cigar_off", "seq_off", "aux_off"):
        assert not got[k].any() and got[k].size == n + 1
    assert got["cigar"].size == got["seq"].size == got["qual"].size == got["aux"].size == 0
    assert np.array_equal(got["vpos"], sh_vpos(of, s.starts))
    spot = list(range(0, n, 1483)) + [n - 1]  # (the closed form above against the oracle's own Pos)
    assert got["vpos"][spot].tolist() == vpos_of(of, s.starts[spot])
    for lo, hi in ((0, 2000), (n - 2000, n)):
        assert_cols_equal(rows(got, lo, hi), orr.decode(s.flat, [int(p) for p in s.starts[lo:hi]]))


def sh_vpos(of, starts):
    """Canonical virtual positions of many flat starts from the oracle's block table (payload
    65280: block k holds flat bytes [65280 k, 65280 (k + 1)))."""
    cstart = np.asarray([b[0] for b in of.blocks], dtype=np.uint64)
    k = np.asarray(starts, dtype=np.uint64) // np.uint64(65280)
    return (cstart[k] << np.uint64(16)) | (np.asarray(starts, dtype=np.uint64) % np.uint64(65280))
