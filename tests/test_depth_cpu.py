"""The host side of per-base depth (csrc/depth_core.h through the library, no GPU):
sbh_depth_add_host and sbh_depth_finish_host against the numpy restatement of depth_corpus.py on
every corpus, malformed rows, the argument errors, sbh_depth_slots, and the two text renderers on a
hand-written example."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pkg import sb
import depth_corpus as dc
import record_corpus as rc

SBH_OK, SBH_E_ARG, SBH_E_BAD_RECORD = 0, sb._lib.SBH_E_ARG, sb._lib.SBH_E_BAD_RECORD
M, I, D, N = dc.M, dc.I, dc.D, dc.N


def test_constants_are_the_library_s():
    with open(os.path.join(ROOT, "spark-bam_amd", "csrc", "depth_core.h")) as f:
        src = f.read()
    assert int(re.search(r"constexpr uint32_t DEPTH_TILE = (\d+);", src).group(1)) == dc.DEPTH_TILE
    assert int(re.search(r"constexpr uint32_t DEPTH_LANE_OPS = (\d+);", src).group(1)) == dc.DEPTH_LANE_OPS


def test_builder_rows_are_rec_s_bytes():
    flat, starts = dc.one_op_stream(2, [5, -1, 2 ** 31 - 2], [100, 1, 268435455], op=dc.X, flag=0x10, mapq=9)
    for i, (pos, ln) in enumerate(((5, 100), (-1, 1), (2 ** 31 - 2, 268435455))):
        want = rc.rec(2, pos, 9, 4681, 0x10, -1, -1, 0, b"abc", ((ln, dc.X),), (), b"", b"")
        assert flat[starts[i]:starts[i] + 44] == want


def test_restatement_on_a_hand_computed_example():
    # reference 0, span [10, 20): one read 5M2D3M from 8, one 4M from 18
    c = dc.case([dc.one(8, [(5, M), (2, D), (3, M)]), dc.one(18, [(4, M)])], [(0, 10, 20)])
    r = dc.restate(c.flat, c.starts, c.spans)
    #            pos: 10 11 12 13 14 15 16 17 18 19 | extra
    assert r["depth"].tolist() == [1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0]
    assert r["add"] == dict(n=2, n_kept=2, n_counted=2, n_unplaced=0, cov_bases=8)
    assert [tuple(x) for x in r["runs"].tolist()] == [(0, 1, 10, 13), (0, 0, 13, 15), (0, 1, 15, 20)]
    assert r["stats"] == dict(slots=11, n_runs=3, covered=8, sum=8, max_depth=1)
    r = dc.restate(c.flat, c.starts, c.spans, count_del=True)
    assert r["depth"].tolist() == [1] * 10 + [0] and r["stats"]["n_runs"] == 1 and r["add"]["cov_bases"] == 10


def host(c, finish=True):
    return sb.depth_host(np.frombuffer(bytes(c.flat), np.uint8), c.starts, c.spans, dc.N_REF, c.filter, c.count_del,
                         finish=finish)


@pytest.mark.parametrize("name", dc.CORPORA)
def test_host_is_the_restatement(name):
    c, want = dc.get(name), dc.expected(name)
    assert want["bad_row"] is None
    add, depth, runs, sizes = host(c)
    assert add == want["add"]
    assert depth.dtype == np.uint32 and np.array_equal(depth, want["depth"])
    assert runs.dtype == dc.RUN_DTYPE and np.array_equal(runs, want["runs"])
    assert sizes == want["stats"]
    assert sizes["sum"] == add["cov_bases"]  # the invariant: every covered base is one unit of depth


def test_corpora_say_what_they_are_for():
    e = dc.expected
    assert e("contention")["stats"] == dict(slots=5001, n_runs=3, covered=100, sum=2000000, max_depth=20000)
    assert e("staircase")["stats"]["n_runs"] == 20002 and e("staircase")["stats"]["max_depth"] == 20000
    assert e("runs_alternating")["stats"]["n_runs"] == dc.T + 1
    assert e("span_without_records")["runs"].tolist() == [(0, 0, 7, 77)]
    assert e("wrap_64bit")["add"]["cov_bases"] == 50 + 50 + 3 and e("wrap_64bit")["stats"]["covered"] == 50
    assert e("pos_max")["add"]["cov_bases"] == 1 + 2
    assert e("pos_minus_one")["add"]["cov_bases"] == 9
    assert e("deletion")["add"]["cov_bases"] == 20 and e("deletion_counted")["add"]["cov_bases"] == 25
    assert e("skip")["add"]["cov_bases"] == e("skip_del")["add"]["cov_bases"] == 20
    assert e("each_op_alone")["add"]["cov_bases"] == 21 and e("each_op_alone_del")["add"]["cov_bases"] == 28
    assert e("filter_nothing_kept")["add"]["n_kept"] == 0 and e("filter_nothing_kept")["stats"]["n_runs"] == 1
    assert e("unplaced")["add"] == dict(n=3, n_kept=3, n_counted=1, n_unplaced=2, cov_bases=5)
    assert e("ref_without_span")["add"]["n_counted"] == 1
    assert e("grid")["add"]["n_kept"] == rc.GRID_RECORDS and e("grid")["add"]["cov_bases"] == 0
    t = [tuple(x) for x in e("runs_tile_edges")["runs"].tolist()]
    assert (0, 1, dc.T - 10, 2 * dc.T + 10) in t and (0, 1, 3 * dc.T, 3 * dc.T + 2) in t


def test_adds_accumulate_and_a_row_given_three_times_counts_three_times():
    c = dc.get("rows_reversed_and_tripled")
    flat = np.frombuffer(bytes(c.flat), np.uint8)
    half = len(c.starts) // 2
    add1, slots = sb.depth_host(flat, c.starts[:half], c.spans, dc.N_REF, finish=False)
    add2, slots = sb.depth_host(flat, c.starts[half:], c.spans, dc.N_REF, slots=slots, finish=False)
    depth, runs, sizes = sb.coverage.finish_host(slots, c.spans)
    want = dc.expected("rows_reversed_and_tripled")
    assert np.array_equal(depth, want["depth"]) and np.array_equal(runs, want["runs"]) and sizes == want["stats"]
    assert add1["cov_bases"] + add2["cov_bases"] == sizes["sum"]
    once = dc.restate(c.flat, c.starts[:200], c.spans)
    thrice = dc.restate(c.flat, [c.starts[200]] * 3, c.spans)
    assert np.array_equal(want["diff"], once["diff"] + thrice["diff"]) and thrice["depth"].max() == 3


def test_op_code_9_in_a_kept_row():
    c = dc.OP9_KEPT()
    assert dc.restate(c.flat, c.starts, c.spans)["bad_row"] == 1
    slots = np.zeros(dc.slots_of(c.spans), np.int32)
    with pytest.raises(sb.SparkBamError) as e:
        sb.depth_host(np.frombuffer(bytes(c.flat), np.uint8), c.starts, c.spans, dc.N_REF, slots=slots, finish=False)
    assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (1,) and not slots.any()


def test_reference_out_of_range_in_a_kept_row():
    c = dc.case([dc.one(1, [(4, M)]), dc.one(1, [(4, M)], ref=dc.N_REF), dc.one(1, [(4, M)], ref=dc.N_REF, flag=0x400)],
                [(0, 0, 100)])
    flat = np.frombuffer(bytes(c.flat), np.uint8)
    with pytest.raises(sb.SparkBamError) as e:
        sb.depth_host(flat, c.starts, c.spans, dc.N_REF)
    assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (1,)
    assert dc.restate(c.flat, c.starts, c.spans)["bad_row"] == 1
    add, _, _, _ = sb.depth_host(flat, [c.starts[0], c.starts[2]], c.spans, dc.N_REF, {"flag_exclude": 0x400})
    assert add["n_kept"] == 1


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed_row(m):
    spans = [(1, 0, 2000)]
    flat = np.frombuffer(bytes(m.stream.flat), np.uint8)
    assert dc.restate(m.stream.flat, m.stream.starts, spans)["bad_row"] == 3
    slots = np.zeros(dc.slots_of(spans), np.int32)
    with pytest.raises(sb.SparkBamError) as e:
        sb.depth_host(flat, m.stream.starts, spans, dc.N_REF, slots=slots, finish=False)
    assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (3,) and not slots.any()
    # the bad row is judged even when the filter would drop it
    with pytest.raises(sb.SparkBamError) as e:
        sb.depth_host(flat, m.stream.starts, spans, dc.N_REF, {"flag_require": 0x1000}, slots=slots, finish=False)
    assert e.value.fields == (3,) and not slots.any()
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        with pytest.raises(sb.SparkBamError) as e:
            sb.depth_host(flat, m.stream.starts[:2] + [p], spans, dc.N_REF, slots=slots, finish=False)
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (2,) and not slots.any()


BAD_SPANS = {
    "none": [],
    "unsorted": [(1, 0, 10), (0, 0, 10)],
    "two_on_one_reference": [(1, 0, 10), (1, 20, 30)],
    "empty": [(0, 10, 10)],
    "reversed": [(0, 10, 5)],
    "negative_beg": [(0, -1, 5)],
    "past_the_last_position": [(0, 0, 2 ** 31)],
    "ref_negative": [(-1, 0, 10)],
    "ref_past_n_ref": [(dc.N_REF, 0, 10)],
}


@pytest.mark.parametrize("name", BAD_SPANS)
def test_bad_spans(name):
    spans = BAD_SPANS[name]
    s = rc.lay([dc.one(1, [(4, M)])])
    with pytest.raises(sb.SparkBamError) as e:
        sb.depth_host(np.frombuffer(s.flat, np.uint8), s.starts, spans, dc.N_REF, slots=np.zeros(64, np.int32))
    assert e.value.code == SBH_E_ARG
    sp = dc.span_array(spans)
    if name != "ref_past_n_ref":  # (sbh_depth_slots knows no n_ref)
        assert sb.lib().sbh_depth_slots(sp.ctypes.data_as(C.c_void_p) if sp.size else None, sp.size) == 0


def test_other_argument_errors():
    s = rc.lay([dc.one(1, [(4, M)])])
    flat = np.frombuffer(s.flat, np.uint8)
    sp = dc.span_array([(0, 0, 10)])
    st = np.asarray(s.starts, np.uint64)
    slots = np.zeros(11, np.int32)
    res, bad = sb._lib.SbhDepthAddResult(), C.c_uint64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lambda flags, f=None: sb.lib().sbh_depth_add_host(p(flat), flat.size, p(st), st.size, f, p(sp), 1, dc.N_REF,  # noqa: E731
                                                             flags, p(slots), C.byref(res), C.byref(bad))
    assert call(0) == SBH_OK and call(1) == SBH_OK
    assert call(2) == SBH_E_ARG and call(0x80000000) == SBH_E_ARG  # unknown flag bits
    f = sb._lib.SbhRecordFilter(0x10000, 0, 0, 0, None, None, 0)
    assert call(0, C.byref(f)) == SBH_E_ARG
    for filt in ({"min_mapq": 256}, {"rows": [(5, 5)]}, {"rows": [(5, 9), (8, 12)]}):
        with pytest.raises(sb.SparkBamError) as e:
            sb.depth_host(flat, s.starts, [(0, 0, 10)], dc.N_REF, filt)
        assert e.value.code == SBH_E_ARG
    sz = sb._lib.SbhDepthSizes()
    assert sb.lib().sbh_depth_finish_host(None, p(sp), 1, None, 0, C.byref(sz)) == SBH_E_ARG
    assert sb.lib().sbh_depth_finish_host(p(slots), p(sp), 1, None, 5, C.byref(sz)) == SBH_E_ARG


def test_depth_slots():
    slots = lambda spans: sb.lib().sbh_depth_slots(dc.span_array(spans).ctypes.data_as(C.c_void_p), len(spans))  # noqa: E731
    assert slots([(0, 0, 1)]) == 2
    assert slots([(0, 5, 10), (3, 0, 100)]) == 6 + 101
    assert slots([(k, 0, 2 ** 31 - 1) for k in range(5)]) == 5 * 2 ** 31  # past 32 bits


def test_finish_host_with_a_short_run_buffer():
    c, want = dc.get("staircase"), dc.expected("staircase")
    _, slots = host(c, finish=False)
    sp = dc.span_array(c.spans)
    runs = np.zeros(10, dc.RUN_DTYPE)
    sz = sb._lib.SbhDepthSizes()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert sb.lib().sbh_depth_finish_host(p(slots), p(sp), 1, p(runs), 10, C.byref(sz)) == SBH_OK
    assert sz.n_runs == want["stats"]["n_runs"] and np.array_equal(runs, want["runs"][:10])


RUNS = np.array([(0, 0, 0, 2), (0, 2, 2, 4), (0, 1, 4, 5), (0, 0, 5, 7), (2, 3, 10, 12)], dtype=dc.RUN_DTYPE)
NAMES = ["chrM", "chr10", "chr2", "chr1"]


def test_text_renderers_on_a_hand_written_example():
    assert sb.depth_text(RUNS, NAMES) == b"chrM\t3\t2\nchrM\t4\t2\nchrM\t5\t1\nchr2\t11\t3\nchr2\t12\t3\n"
    assert sb.depth_text(RUNS, NAMES, all_positions=True) == (
        b"chrM\t1\t0\nchrM\t2\t0\nchrM\t3\t2\nchrM\t4\t2\nchrM\t5\t1\nchrM\t6\t0\nchrM\t7\t0\nchr2\t11\t3\nchr2\t12\t3\n")
    assert sb.depth_bedgraph(RUNS, NAMES) == b"chrM\t2\t4\t2\nchrM\t4\t5\t1\nchr2\t10\t12\t3\n"
    assert sb.depth_text(RUNS[:0], NAMES) == b"" and sb.depth_bedgraph(RUNS[:0], NAMES) == b""


def test_region_spans():
    rs = sb.coverage.region_spans
    lens = [16571, 135534747, 2147483647, 249250621]
    assert rs(None, NAMES, lens) == [(0, 0, 16571), (1, 0, 135534747), (2, 0, 2147483647), (3, 0, 249250621)]
    assert rs("chr2", NAMES, lens) == [(2, 0, 2147483647)]
    assert rs("chr10:5-10", NAMES, lens) == [(1, 4, 10)]  # 1-based, inclusive
    assert rs("chrM:16000-99999", NAMES, lens) == [(0, 15999, 16571)]  # cut to the reference
    for bad in ("chrX", "chrX:1-5", "chrM:10-5", "chrM:0-5", "chrM:1"):
        with pytest.raises(ValueError):
            rs(bad, NAMES, lens)


def test_exports():
    assert {"sbh_depth_create", "sbh_depth_destroy", "sbh_depth_reset", "sbh_records_depth_add", "sbh_depth_finish",
            "sbh_depth_fetch", "sbh_depth_runs_fetch", "sbh_depth_device_ptr", "sbh_depth_slots", "sbh_depth_add_host",
            "sbh_depth_finish_host"} <= set(sb._lib.EXPORTS)
    assert callable(sb.depth) and callable(sb.depth_host)
