"""sbh_bam_gather_host (csrc/bam_gather_core.h's host gatherer, no GPU) against the numpy
restatement in bam_gather_corpus.py: every corpus under every keep pattern and head length,
the predicate's edges, the errors, the reference's 2.100-1000.bam fixture, and filter counts on
2.bam computed from the oracle's decode."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import golden_bam
from oracle_lib import OracleFile
import oracle_records as orr
from pkg import sb
import bam_gather_corpus as bc
import record_corpus as rc

SBH_E_ARG, SBH_E_BAD_RECORD = sb._lib.SBH_E_ARG, sb._lib.SBH_E_BAD_RECORD


def check(flat, starts, head=b"", **f):
    want = bc.gather_ref(flat, starts, head, **f)
    got = sb.bam_gather_host(flat, starts, head, bc.filter_dict(**f))
    assert bytes(got[0]) == want[0]
    assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
    assert int(got[1][0]) == len(head)
    return got


@pytest.mark.parametrize("pattern", bc.PATTERNS)
@pytest.mark.parametrize("name,s", bc.streams(), ids=lambda x: x if isinstance(x, str) else "")
def test_corpus_patterns(name, s, pattern):
    heads = bc.HEADS if name == "ladder" else (bc.HEADS[0], bc.HEADS[5], rc.header())
    for head in heads:
        stream, off, rows = check(s.flat, s.starts, head, rows=bc.pattern_ranges(pattern, len(s.starts)))
        if pattern == "all":
            assert bytes(stream) == head + bytes(s.flat[s.first:]) and rows.size == len(s.starts)
        if name == "ladder" and pattern == "all":
            check(s.flat, s.starts, head, rows=bc.LADDER_ROWS)


def test_ladder_meets_every_residue_pair():
    s = bc.ladder_stream()
    for h in range(16):
        assert len(bc.residue_pairs(s, h, bc.LADDER_ROWS)) == 256, h


def test_long_record_is_longer_than_a_member():
    s = bc.long_stream()
    assert s.starts[2] - s.starts[1] > 70000 and s.starts[1] - s.starts[0] == 37


def test_keeps_none_and_empty_inputs():
    s = rc.decode_stream()
    stream, off, rows = check(s.flat, s.starts, b"head", flag_require=0xFFFF, flag_exclude=0xFFFF)
    assert bytes(stream) == b"head" and off.tolist() == [4] and rows.size == 0
    stream, off, rows = check(s.flat, s.starts, b"", flag_require=0xFFFF, flag_exclude=1)  # head_bytes = 0, none kept
    assert stream.size == 0 and off.tolist() == [0]
    lad = bc.ladder_stream()
    stream, off, rows = check(lad.flat, lad.starts, b"", flag_require=0xFFFF)  # (no ladder record has every bit)
    assert stream.size == 0 and off.tolist() == [0]
    stream, off, rows = check(s.flat, [], b"hd")  # n = 0
    assert bytes(stream) == b"hd" and off.tolist() == [2] and rows.size == 0
    stream, off, rows = check(b"", [], b"")
    assert stream.size == 0 and off.tolist() == [0]


def test_duplicate_and_descending_starts():
    s = bc.ladder_stream()
    st = list(s.starts[:40])
    check(s.flat, st[::-1], b"x" * 3)
    check(s.flat, st + st, b"x" * 3)
    check(s.flat, [st[5]] * 7 + st[::-1] + [st[5]], b"", rows=[(1, 3), (6, 20), (30, 1000)])


def test_row_ranges_reaching_past_n():
    s = rc.decode_stream()
    n = len(s.starts)
    _, _, rows = check(s.flat, s.starts, b"", rows=[(n - 2, n + 5), (n + 7, 2 ** 63)])
    assert rows.tolist() == [n - 2, n - 1]
    _, _, rows = check(s.flat, s.starts, b"", rows=[(n, n + 1)])
    assert rows.size == 0


def test_predicate_edges():
    recs = [rc.rec(0, 1, mapq, 0, flag, -1, -1, 0, b"q", (), (), b"", b"")
            for mapq, flag in ((29, 0), (30, 0), (31, 0), (255, 0xFFFF), (0, 0x10), (30, 0x410), (30, 0x400))]
    s = rc.lay(recs)
    assert check(s.flat, s.starts, min_mapq=30)[2].tolist() == [1, 2, 3, 5, 6]      # mapq == min_mapq stays
    assert check(s.flat, s.starts, min_mapq=31)[2].tolist() == [2, 3]               # one below goes
    assert check(s.flat, s.starts, min_mapq=255)[2].tolist() == [3]
    assert check(s.flat, s.starts, flag_require=0x10, flag_exclude=0x10)[2].size == 0  # a shared bit keeps nothing
    assert check(s.flat, s.starts, flag_require=0xFFFF)[2].tolist() == [3]          # flag 0xFFFF
    assert check(s.flat, s.starts, flag_exclude=0xFFFF)[2].tolist() == [0, 1, 2]
    assert check(s.flat, s.starts, flag_require=0x10, flag_exclude=0x400)[2].tolist() == [4]
    assert check(s.flat, s.starts, flag_require=0x400, min_mapq=30, rows=[(0, 6)])[2].tolist() == [3, 5]


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed_rows(m):
    s = m.stream
    for f in (None, {"flag_require": 0xFFFF}, {"rows": [(0, 1)]}):  # the filter would drop the bad row: still reported
        with pytest.raises(sb.SparkBamError) as e:
            sb.bam_gather_host(s.flat, s.starts, b"hd", f)
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (3,)
    stream, _, rows = sb.bam_gather_host(s.flat, s.starts[:3], b"", None)  # the good ones alone
    assert rows.tolist() == [0, 1, 2] and bytes(stream) == bytes(s.flat[s.starts[0]:s.starts[3]])


@pytest.mark.parametrize("f", [
    {"rows": [(5, 9), (0, 3)]}, {"rows": [(0, 5), (4, 9)]}, {"rows": [(3, 3)]}, {"rows": [(4, 2)]},
    {"flag_require": 65536}, {"flag_exclude": 65536}, {"min_mapq": -1}, {"min_mapq": 256},
], ids=str)
def test_bad_filters_are_arg_errors(f):
    s = rc.decode_stream()
    with pytest.raises(sb.SparkBamError) as e:
        sb.bam_gather_host(s.flat, s.starts, b"", f)
    assert e.value.code == SBH_E_ARG
    sb.bam_gather_host(s.flat, s.starts, b"", {"rows": [(0, 3), (3, 5)]})  # touching ranges are disjoint


def test_out_cap_too_small():
    s = rc.decode_stream()
    flat = np.frombuffer(s.flat, np.uint8)
    st = np.asarray(s.starts, np.uint64)
    total = len(bc.gather_ref(s.flat, s.starts, b"abc")[0])
    head = np.frombuffer(b"abc", np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for cap, rc_want in ((total - 1, SBH_E_ARG), (total, 0)):
        out = np.full(total + 8, 0xEE, np.uint8)
        n_kept, bad = C.c_uint64(), C.c_uint64()
        got = sb.lib().sbh_bam_gather_host(p(flat), flat.size, p(st), st.size, p(head), 3, None, p(out), cap, None, None,
                                           C.byref(n_kept), C.byref(bad))
        assert got == rc_want and n_kept.value == st.size
        assert out[total:].tolist() == [0xEE] * 8
        if cap < total:
            assert out.tolist() == [0xEE] * (total + 8)  # refused before anything is written


@functools.lru_cache(maxsize=None)
def two_bam():
    flat = OracleFile.from_path(golden_bam("2.bam")).uncompressed()
    _, first = orr.bam_refs(flat)
    starts = orr.record_starts(bytes(flat), first, len(flat))
    return flat, first, starts, orr.decode(bytes(flat), starts)


def test_golden_slice_of_2bam():
    """HTSJDKRewriteTest's fixture: 2.bam's header, then its records 100..999."""
    flat, first, starts, _ = two_bam()
    want = OracleFile.from_path(golden_bam("2.100-1000.bam")).uncompressed()
    stream, off, rows = sb.bam_gather_host(flat, starts, bytes(flat[:first]), {"rows": [(100, 1000)]})
    assert bytes(stream) == bytes(want)
    assert rows.tolist() == list(range(100, 1000)) and int(off[0]) == first


@pytest.mark.parametrize("f,kept", [
    ({"flag_require": 0x10}, 1094), ({"flag_exclude": 0x4}, 2450), ({"flag_require": 0x40, "flag_exclude": 0x10}, 722),
    ({"min_mapq": 30}, 124), ({"min_mapq": 1}, 666),
], ids=str)
def test_filter_counts_on_2bam(f, kept):
    flat, first, starts, cols = two_bam()
    flag, mapq = cols["flag"].astype(np.int64), cols["mapq"].astype(np.int64)
    rq, ex, mq = f.get("flag_require", 0), f.get("flag_exclude", 0), f.get("min_mapq", 0)
    want = np.flatnonzero(((flag & rq) == rq) & ((flag & ex) == 0) & (mapq >= mq))
    assert 0 < want.size < len(starts) == 2500
    assert want.size == kept
    stream, off, rows = sb.bam_gather_host(flat, starts, b"", f)
    assert rows.tolist() == want.tolist()
    ends = list(starts[1:]) + [len(flat)]
    assert bytes(stream) == b"".join(bytes(flat[starts[i]:ends[i]]) for i in want)
