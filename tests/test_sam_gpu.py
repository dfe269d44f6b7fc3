"""SAM text on the GPU (sam.hip: k_sam_sizes, the scan, k_sam_emit; sbh_records_sam_scan / fetch)
against the library's host renderer (sbh_sam_render_host, which test_sam_cpu.py holds to the
reference's 2.sam and to Reads.sam_lines), byte for byte and offset for offset: the hand-built
corpus of sam_corpus.py whole and through 97-byte BGZF members, 2.bam against the fixture, more
records than the emit launch has waves, malformed rows, call-order errors, and the text after an
interval scan and after a batch of splits."""
import functools

import numpy as np
import pytest

from conftest import golden_bam
from oracle_lib import OracleFile, file_splits
from pkg import sb
import record_corpus as rc
import sam_corpus as sc
from test_sam_cpu import two_bam

pytestmark = pytest.mark.gpu

SBH_E_HIP, SBH_E_STATE, SBH_E_BAD_RECORD = sb._lib.SBH_E_HIP, sb._lib.SBH_E_STATE, sb._lib.SBH_E_BAD_RECORD


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


def open_stream(ctx, flat, payload=65280, level=6):
    """The flat bytes as a BGZF file, resident and inflated."""
    sh = ctx.shard(np.frombuffer(rc.bgzf(flat, payload, level), np.uint8).copy())
    _, fs = call(sh.index, 0)
    call(sh.inflate)
    assert fs == len(flat)
    return sh


@functools.lru_cache(maxsize=None)
def corpus_want():
    s = sc.stream()
    return sb.sam_text_host(s.flat, s.starts, sc.REF_NAMES)


@pytest.mark.parametrize("payload", (65280, 97))
def test_corpus_equals_host_renderer(ctx, payload):
    s = sc.stream()
    want_text, want_off = corpus_want()
    sh = open_stream(ctx, s.flat, payload)
    try:
        assert call(sh.records, s.first, sh.flat_size)["flat"].tolist() == s.starts
        text, line_off = call(sh.records_sam, sc.REF_NAMES)
        # exactly the float rows went to the host: no other case can pass on the host path
        assert sh.sam_n_host == len(sc.FLOAT_ROWS)
        assert np.array_equal(line_off, want_off)
        for i, (label, _) in enumerate(sc.CASES):
            a, b = int(want_off[i]), int(want_off[i + 1])
            assert bytes(text[a:b]) == bytes(want_text[a:b]), label
        assert text.size == want_text.size
    finally:
        sh.close()


def test_corpus_without_float_rows_stays_on_the_device(ctx):
    keep = [i for i in range(len(sc.CASES)) if i not in sc.FLOAT_ROWS]
    s = rc.lay([sc.CASES[i][1] for i in keep])
    want_text, want_off = sb.sam_text_host(s.flat, s.starts, sc.REF_NAMES)
    sh = open_stream(ctx, s.flat)
    try:
        call(sh.records, s.first, sh.flat_size)
        text, line_off = call(sh.records_sam, sc.REF_NAMES)
        assert sh.sam_n_host == 0
        assert np.array_equal(line_off, want_off) and np.array_equal(text, want_text)
        # a sub-range from a later record on, and other reference names (bytes; none at all)
        k = len(keep) // 2
        call(sh.records, s.starts[k], s.starts[-1])
        text, line_off = call(sh.records_sam, [b"a", b"", b"a-longer-name-than-the-others" * 3, b"d"])
        w_text, w_off = sb.sam_text_host(s.flat, s.starts[k:-1], [b"a", b"", b"a-longer-name-than-the-others" * 3, b"d"])
        assert np.array_equal(line_off, w_off) and np.array_equal(text, w_text)
        text, line_off = call(sh.records_sam, [])
        w_text, w_off = sb.sam_text_host(s.flat, s.starts[k:-1], [])
        assert np.array_equal(line_off, w_off) and np.array_equal(text, w_text)
    finally:
        sh.close()


@pytest.fixture(scope="module")
def two_bam_shard(ctx):
    data = np.fromfile(golden_bam("2.bam"), dtype=np.uint8)
    sh = ctx.shard(data)
    call(sh.index, 0)
    call(sh.inflate)
    flat, starts, names = two_bam()
    call(sh.set_contigs, OracleFile(data).contig_len)
    yield sh, data, flat, starts, names
    sh.close()


def test_2bam_equals_the_reference_sam(two_bam_shard):
    sh, _, flat, starts, names = two_bam_shard
    _, lines = sc.fixture_lines()
    call(sh.check_eager, starts[0], sh.flat_size, want_bits=False)
    assert call(sh.records_scan, starts[0], sh.flat_size) == 2500
    text, line_off = call(sh.records_sam, names)
    assert sh.sam_n_host == 0
    assert bytes(text) == b"".join(lines)
    assert line_off.tolist() == np.cumsum([0] + [len(l) for l in lines]).tolist()


def test_2bam_after_an_interval_scan(two_bam_shard):
    sh, _, flat, starts, names = two_bam_shard
    _, lines = sc.fixture_lines()
    cols = call(sh.records_regions, [(starts[0], sh.flat_size)], [(0, 13000, 14000), (0, 60000, 61000)])
    rows = [starts.index(int(f)) for f in cols["flat"]]
    assert 0 < len(rows) < 2500 and rows == sorted(rows)
    text, line_off = call(sh.records_sam, names)
    assert bytes(text) == b"".join(lines[r] for r in rows)
    assert line_off.size == len(rows) + 1 and int(line_off[-1]) == text.size


def test_2bam_after_a_batch_of_splits(two_bam_shard):
    sh, data, flat, starts, names = two_bam_shard
    _, lines = sc.fixture_lines()
    splits = file_splits(data.size, data.size // 3 + 1)
    assert len(splits) == 3
    info, per, cols = call(sh.split_records_batch, splits)
    assert info["n"] == 2500 and all(p["status"] == 0 and p["rec_count"] for p in per)
    text, line_off = call(sh.records_sam, names)
    for p in per:
        a, b = p["rec_begin"], p["rec_begin"] + p["rec_count"]
        rows = [starts.index(int(f)) for f in cols["flat"][a:b]]
        assert bytes(text[int(line_off[a]):int(line_off[b])]) == b"".join(lines[r] for r in rows)


def test_more_records_than_waves(ctx):
    """262144 + 37 records: the emit launch is capped at 65536 workgroups of four waves, as
    k_rec_fields' is, so the grid-stride loop runs."""
    s, _ = rc.grid_stream()
    starts = s.starts.astype(np.uint64)
    want_text, want_off = sb.sam_text_host(s.flat, starts, sc.REF_NAMES)
    sh = open_stream(ctx, s.flat, level=1)
    try:
        call(sh.set_contigs, [ln for _, ln in rc.CONTIGS])
        assert call(sh.check_eager, 0, sh.flat_size, want_bits=False)[0] == rc.GRID_RECORDS
        assert call(sh.records_scan, s.first, sh.flat_size) == rc.GRID_RECORDS
        text, line_off = call(sh.records_sam, sc.REF_NAMES)
        assert sh.sam_n_host == 0
        assert np.array_equal(line_off, want_off) and np.array_equal(text, want_text)
    finally:
        sh.close()
    assert bytes(text[:int(line_off[1])]) == b"0000000\t4\tchr10\t1\t0\t*\tchr2\t262182\t-131072\t*\t*\n"


@pytest.mark.parametrize("m", sc.MALFORMED, ids=lambda m: m.name)
def test_malformed_row_is_named(ctx, m):
    s = m.stream
    sh = open_stream(ctx, s.flat)
    try:
        call(sh.records, s.first, sh.flat_size)  # (the decode takes the tag bytes as they are)
        with pytest.raises(sb.SparkBamError) as e:
            call(sh.records_sam, sc.REF_NAMES)
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (m.bad_row,)
        assert "record %d " % m.bad_row in str(e.value)
        # the good rows before it still render
        call(sh.records, s.first, s.starts[m.bad_row])
        text, line_off = call(sh.records_sam, sc.REF_NAMES)
        w_text, w_off = sb.sam_text_host(s.flat, s.starts[:m.bad_row], sc.REF_NAMES)
        assert np.array_equal(line_off, w_off) and np.array_equal(text, w_text)
    finally:
        sh.close()


def test_call_order_and_empty_scan(two_bam_shard):
    sh, data, flat, starts, names = two_bam_shard
    fresh = sh.ctx.shard(data)
    try:
        call(fresh.index, 0)
        call(fresh.inflate)
        with pytest.raises(sb.SparkBamError) as e:  # no scan yet
            call(fresh.records_sam, names)
        assert e.value.code == SBH_E_STATE
        call(fresh.set_contigs, OracleFile(data).contig_len)
        call(fresh.split_records, 0, data.size, decode=False)
        with pytest.raises(sb.SparkBamError) as e:  # the last scan holds the starts only
            call(fresh.records_sam, names)
        assert e.value.code == SBH_E_STATE
        assert call(fresh.records_scan, starts[0], starts[0]) == 0  # n == 0
        text, line_off = call(fresh.records_sam, names)
        assert text.size == 0 and line_off.tolist() == [0]
        assert call(fresh.records_scan, starts[0], starts[3]) == 3
        text, line_off = call(fresh.records_sam, names)
        _, lines = sc.fixture_lines()
        assert bytes(text) == b"".join(lines[:3])
    finally:
        fresh.close()
