"""view_bam end to end: the reference's HTSJDKRewriteTest slice, htsjdk_rewrite's own bytes (whose
subset path gathers on the host: the two paths pin each other), windows, filters against the
oracle's decode, and regions against load_bam_intervals."""
import functools
import random

import numpy as np
import pytest

from conftest import golden_bam
from oracle_lib import OracleFile
import oracle_records as orr
from pkg import sb

pytestmark = pytest.mark.gpu

LEVEL_FAST = sb._lib.LEVEL_FAST
ROUND_TRIPPED = ["2.bam", "1.bam", "1.2203053-2211029.bam"]  # (test_zdeflate_gpu.py's fixtures)


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def decoded(name):
    """(oracle, flat, record starts, decoded columns) of a fixture."""
    of = OracleFile.from_path(golden_bam(name))
    flat = of.uncompressed()
    _, first = orr.bam_refs(flat)
    starts = orr.record_starts(bytes(flat), first, len(flat))
    return of, flat, first, starts, orr.decode(bytes(flat), starts)


def records_of(data):
    """(header bytes, [record bytes]) of a BAM file's bytes, by the oracle."""
    flat = OracleFile(np.frombuffer(bytes(data), np.uint8).copy()).uncompressed()
    _, first = orr.bam_refs(flat)
    starts = list(orr.record_starts(bytes(flat), first, len(flat))) + [len(flat)]
    return bytes(flat[:first]), [bytes(flat[a:b]) for a, b in zip(starts, starts[1:])]


def test_reference_slice(ctx):
    got = sb.view_bam(golden_bam("2.bam"), rows=range(100, 1000), ctx=ctx)
    assert got == open(golden_bam("2.100-1000.bam"), "rb").read()


@pytest.mark.parametrize("level", (5, LEVEL_FAST))
@pytest.mark.parametrize("name", ROUND_TRIPPED)
def test_no_filter_equals_htsjdk_rewrite(ctx, name, level):
    want = sb.htsjdk_rewrite(golden_bam(name), ctx=ctx, level=level).tobytes()
    assert sb.view_bam(golden_bam(name), level=level, ctx=ctx) == want


@pytest.mark.parametrize("seed", (1, 2))
def test_random_rows_equal_htsjdk_rewrite(ctx, seed):
    rng = random.Random(seed)
    rows = sorted(rng.sample(range(2500), rng.choice([1, 40, 1700])))
    want = sb.htsjdk_rewrite(golden_bam("2.bam"), read_ranges=rows, ctx=ctx).tobytes()
    assert sb.view_bam(golden_bam("2.bam"), rows=rows, ctx=ctx) == want


@pytest.mark.parametrize("kw", ({}, {"flag_exclude": 0x10, "rows": range(333, 4321)}), ids=("all", "filtered"))
def test_windows_do_not_change_the_bytes(ctx, kw):
    path, window = golden_bam("5k.bam"), 300000
    assert len(list(sb.api.iter_reads(path, window=window, ctx=ctx))) >= 3
    one = sb.view_bam(path, ctx=ctx, **kw)
    assert sb.view_bam(path, window=window, ctx=ctx, **kw) == one
    assert sb.view_bam(path, window=150000, ctx=ctx, **kw) == one
    header, recs = records_of(one)
    _, all_recs = records_of(open(path, "rb").read())
    if not kw:
        assert recs == all_recs
    else:
        assert 0 < len(recs) < len(all_recs[333:4321]) and set(recs) <= set(all_recs[333:4321])


@pytest.mark.parametrize("f", [
    {"flag_require": 0x10}, {"flag_exclude": 0x4}, {"flag_require": 0x40, "flag_exclude": 0x10}, {"min_mapq": 30},
    {"min_mapq": 1}, {"flag_require": 0x10, "min_mapq": 1, "rows": range(1000, 2400)},
], ids=str)
def test_filters_keep_the_oracles_records(ctx, f):
    of, flat, first, starts, cols = decoded("2.bam")
    flag, mapq = cols["flag"].astype(np.int64), cols["mapq"].astype(np.int64)
    rq, ex, mq = f.get("flag_require", 0), f.get("flag_exclude", 0), f.get("min_mapq", 0)
    keep = ((flag & rq) == rq) & ((flag & ex) == 0) & (mapq >= mq)
    if "rows" in f:
        keep &= np.isin(np.arange(len(starts)), np.asarray(f["rows"]))
    want = np.flatnonzero(keep)
    assert 0 < want.size < len(starts)
    ends = list(starts[1:]) + [len(flat)]
    header, recs = records_of(sb.view_bam(golden_bam("2.bam"), ctx=ctx, **f))
    assert header == bytes(flat[:first])
    assert recs == [bytes(flat[starts[i]:ends[i]]) for i in want]


def interval_records(of, flat, res):
    """load_bam_intervals' records as raw bytes, in vpos order."""
    out = []
    for v in sorted(int(x) for x in res.reads.cols["vpos"]):
        p = of.flat_of(v >> 16, v & 0xFFFF)
        out.append(bytes(flat[p:p + 4 + int.from_bytes(bytes(flat[p:p + 4]), "little")]))
    return out


@pytest.mark.parametrize("text,count", [("1:0-100000", 2450), ("1:13000-14000,1:60000-61000", 129),
                                        ("1:2000000-3000000", 0)])
def test_regions_equal_load_bam_intervals(ctx, text, count):
    """LoadBAMTest's intervals on 2.bam; the output's own index answers them with the same records."""
    of, flat, first, starts, cols = decoded("2.bam")
    want = interval_records(of, flat, sb.load_bam_intervals(golden_bam("2.bam"), text, ctx=ctx))
    assert len(want) == count
    bam, bai = sb.view_bam(golden_bam("2.bam"), intervals=text, index=True, ctx=ctx)
    header, recs = records_of(bam)
    assert header == bytes(flat[:first]) and recs == want  # (2.bam is sorted: chunk order is vpos order)
    out_of = OracleFile(np.frombuffer(bam, np.uint8).copy())
    again = sb.load_bam_intervals(np.frombuffer(bam, np.uint8), text, bai=bai, ctx=ctx)
    assert interval_records(out_of, out_of.uncompressed(), again) == want
    # the other filters apply on top
    mapq = {bytes(flat[s:e]): int(q) for s, e, q in zip(starts, list(starts[1:]) + [len(flat)], cols["mapq"])}
    _, some = records_of(sb.view_bam(golden_bam("2.bam"), intervals=text, min_mapq=1, ctx=ctx))
    assert some == [r for r in want if mapq[r] >= 1]
