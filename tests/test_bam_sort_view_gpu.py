"""sort_bam / view_bam(sort="coordinate") end to end on 2.bam with its records shuffled on the host:
the output's records are the shuffled file's in the restatement's order (not merely ascending),
its header says SO:coordinate, its index builds and equals the index of the same records
assembled on the host, and regions read back through it give what the original 2.bam gives."""
import functools

import numpy as np
import pytest

from conftest import golden_bam
from pkg import sb
import bai_ref
import bam_sort_corpus as sc
import record_corpus as rc
from test_bam_view_gpu import interval_records, records_of
from oracle_lib import OracleFile

pytestmark = pytest.mark.gpu

SBH_E_ARG, SBH_E_UNSORTED = sb._lib.SBH_E_ARG, sb._lib.SBH_E_UNSORTED


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def shuffled():
    """(the shuffled file's bytes, its header, its records in file order, the expected records)."""
    header, recs = records_of(open(golden_bam("2.bam"), "rb").read())
    order = np.random.default_rng(20).permutation(len(recs))
    recs = [recs[i] for i in order]
    s = rc.Stream(header + b"".join(recs), len(header), np.cumsum([len(header)] + [len(r) for r in recs])[:-1])
    want = [recs[i] for i in sc.perm_ref(s.flat, s.starts).tolist()]
    return rc.bgzf(s.flat, 65280), header, recs, want


def test_sort_bam_of_a_shuffled_file(ctx):
    data, header, recs, want = shuffled()
    assert want != recs and sorted(want) == sorted(recs)
    got = sb.sort_bam(data, ctx=ctx)
    got_header, got_recs = records_of(got)
    assert got_recs == want
    assert got_header == sb.bam_header_set_so(header, "coordinate") and b"\tSO:coordinate\n" in got_header
    # the same records assembled on the host index the same; the shuffled input does not index
    # (cut and compressed as the writer does, so that virtual offsets are comparable: the stream is
    # the host's, member for member)
    host_stream = np.frombuffer(got_header + b"".join(want), np.uint8)
    host_file = ctx.bgzf_compress(host_stream, level=5)[0].tobytes()
    assert host_file == got
    bai = sb.build_bai(got, ctx=ctx)
    assert bai_ref.parsed(bai) == bai_ref.parsed(sb.build_bai(host_file, ctx=ctx))
    assert bai_ref.parsed(bai) == bai_ref.parsed(bai_ref.build(host_file).bytes)  # the host indexer's answer too
    with pytest.raises(sb.SparkBamError) as e:
        sb.build_bai(data, ctx=ctx)
    assert e.value.code == SBH_E_UNSORTED
    # index=True gives that index; view_bam(sort=) with the file in one window is sort_bam
    assert sb.sort_bam(data, index=True, ctx=ctx) == (got, bai)
    assert sb.view_bam(data, sort="coordinate", ctx=ctx) == got


def test_filters_and_rows_apply_before_the_sort(ctx):
    data, header, recs, _ = shuffled()
    kept = [r for r in recs[100:1900] if not (r[18] | r[19] << 8) & 0x10]
    s = rc.lay(kept)
    want = [kept[i] for i in sc.perm_ref(s.flat, s.starts).tolist()]
    got = sb.view_bam(data, sort="coordinate", flag_exclude=0x10, rows=range(100, 1900), ctx=ctx)
    assert 0 < len(want) < 1800 and records_of(got)[1] == want


def test_sorted_input_is_view_bam_s_stream(ctx):
    path = golden_bam("2.bam")
    a_header, a = records_of(sb.sort_bam(path, ctx=ctx))
    b_header, b = records_of(sb.view_bam(path, ctx=ctx))
    assert a == b and a_header == b_header  # (2.bam's header says SO:coordinate already)


def test_one_window_only(ctx):
    path = golden_bam("5k.bam")
    assert len(list(sb.api.iter_reads(path, window=300000, ctx=ctx))) >= 3
    with pytest.raises(sb.SparkBamError) as e:
        sb.view_bam(path, sort="coordinate", window=300000, ctx=ctx)
    assert e.value.code == SBH_E_ARG and "window" in str(e.value)
    with pytest.raises(sb.SparkBamError) as e:
        sb.view_bam(golden_bam("2.bam"), sort="coordinate", intervals="1:0-100000", ctx=ctx)
    assert e.value.code == SBH_E_ARG
    with pytest.raises(ValueError):
        sb.view_bam(golden_bam("2.bam"), sort="queryname", ctx=ctx)


def test_regions_through_the_sorted_file_s_index(ctx):
    """The sorted shuffle answers a region with the records the original sorted 2.bam gives."""
    data = shuffled()[0]
    bam, bai = sb.sort_bam(data, index=True, ctx=ctx)
    of = OracleFile.from_path(golden_bam("2.bam"))
    out_of = OracleFile(np.frombuffer(bam, np.uint8).copy())
    for text, count in (("1:13000-14000,1:60000-61000", 129), ("1:0-100000", 2450)):
        want = interval_records(of, of.uncompressed(), sb.load_bam_intervals(golden_bam("2.bam"), text, ctx=ctx))
        again = sb.load_bam_intervals(np.frombuffer(bam, np.uint8), text, bai=bai, ctx=ctx)
        got = interval_records(out_of, out_of.uncompressed(), again)
        assert len(want) == count and sorted(got) == sorted(want)
