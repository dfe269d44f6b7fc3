"""sort_bam(order="name") / view_bam(sort="name") end to end on 2.bam with its records shuffled on the
host: the output's records are the shuffled file's in the restatement's order, its header differs
from the input's only in SO:queryname, filters and rows apply before the sort, what name order
cannot have is refused, and coordinate-sorting the name-sorted file gives the records that
coordinate-sorting the shuffle gives."""
import struct

import numpy as np
import pytest

from conftest import golden_bam
from pkg import sb
import name_sort_corpus as nc
import record_corpus as rc
from test_bam_view_gpu import records_of
from test_bam_sort_view_gpu import shuffled

pytestmark = pytest.mark.gpu

SBH_E_ARG = sb._lib.SBH_E_ARG


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def in_name_order(header, recs):
    s = rc.Stream(header + b"".join(recs), len(header), np.cumsum([len(header)] + [len(r) for r in recs])[:-1])
    return [recs[i] for i in nc.perm_ref(s.flat, s.starts).tolist()]


def test_sort_bam_by_name_of_a_shuffled_file(ctx):
    data, header, recs, _ = shuffled()
    want = in_name_order(header, recs)
    assert want != recs and sorted(want) == sorted(recs)
    got = sb.sort_bam(data, order="name", ctx=ctx)
    got_header, got_recs = records_of(got)
    assert got_recs == want
    # the input's header but for SO:queryname in its text (and the l_text that follows the text's length)
    l_text = struct.unpack_from("<i", header, 4)[0]
    text = header[8:8 + l_text]
    want_text = text.replace(b"\tSO:coordinate\n", b"\tSO:queryname\n", 1)
    assert want_text != text
    assert got_header == header[:4] + struct.pack("<i", len(want_text)) + want_text + header[8 + l_text:]
    assert got_header == sb.bam_header_set_so(header, "queryname")
    # the stream is the host's, member for member; view_bam(sort=) with the file in one window is sort_bam
    host_stream = np.frombuffer(got_header + b"".join(want), np.uint8)
    assert ctx.bgzf_compress(host_stream, level=5)[0].tobytes() == got
    assert sb.view_bam(data, sort="name", ctx=ctx) == got


def test_filters_and_rows_apply_before_the_sort(ctx):
    data, header, recs, _ = shuffled()
    kept = [r for r in recs[100:1900] if not (r[18] | r[19] << 8) & 0x10]
    want = in_name_order(header, kept)
    got = sb.view_bam(data, sort="name", flag_exclude=0x10, rows=range(100, 1900), ctx=ctx)
    assert 0 < len(want) < 1800 and records_of(got)[1] == want


def test_what_name_order_refuses(ctx):
    data = shuffled()[0]
    for f in (lambda: sb.sort_bam(data, order="name", index=True, ctx=ctx),
              lambda: sb.view_bam(data, sort="name", index=True, ctx=ctx),
              lambda: sb.sort_bam(data, order="queryname", ctx=ctx)):
        with pytest.raises(ValueError):
            f()
    path = golden_bam("5k.bam")
    with pytest.raises(sb.SparkBamError) as e:  # a second window
        sb.view_bam(path, sort="name", window=300000, ctx=ctx)
    assert e.value.code == SBH_E_ARG and "window" in str(e.value)
    with pytest.raises(sb.SparkBamError) as e:
        sb.view_bam(golden_bam("2.bam"), sort="name", intervals="1:0-100000", ctx=ctx)
    assert e.value.code == SBH_E_ARG


def test_coordinate_sorting_the_name_sorted_file(ctx):
    data = shuffled()[0]
    by_name = sb.sort_bam(data, order="name", ctx=ctx)
    a_header, a = records_of(sb.sort_bam(by_name, ctx=ctx))
    b_header, b = records_of(sb.sort_bam(data, ctx=ctx))
    assert sorted(a) == sorted(b) and len(a) == 2500 and a_header == b_header
