"""sbh_sam_render_host (csrc/sam_core.h's host renderer, no GPU): the reference's SAM text of
2.bam byte for byte, the hand-built corpus of sam_corpus.py against Reads.sam_lines over the
oracle's decode, Float.toString literals, malformed CIGARs and tag areas, and the capacity check."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

from conftest import golden_bam
from oracle_lib import OracleFile
import oracle_records as orr
from pkg import sb
import record_corpus as rc
import sam_corpus as sc

SBH_E_ARG, SBH_E_BAD_RECORD = sb._lib.SBH_E_ARG, sb._lib.SBH_E_BAD_RECORD


@functools.lru_cache(maxsize=None)
def two_bam():
    """(flat bytes, record starts, reference names) of 2.bam from the oracle."""
    flat = OracleFile.from_path(golden_bam("2.bam")).uncompressed()
    names, first = orr.bam_refs(flat)
    return flat, orr.record_starts(bytes(flat), first, len(flat)), names


def test_2bam_equals_the_reference_sam():
    flat, starts, names = two_bam()
    _, lines = sc.fixture_lines()
    assert len(starts) == len(lines) == 2500
    text, line_off = sb.sam_text_host(flat, starts, names)
    assert bytes(text) == b"".join(lines)
    assert line_off.tolist() == np.cumsum([0] + [len(l) for l in lines]).tolist()
    none, sizes_only = sb.sam_text_host(flat, starts, names, want_text=False)
    assert none is None and np.array_equal(sizes_only, line_off)


def test_corpus_equals_sam_lines():
    s = sc.stream()
    text, line_off = sb.sam_text_host(s.flat, s.starts, sc.REF_NAMES)
    want = sb.Reads(orr.decode(s.flat, s.starts), sc.REF_NAMES)
    assert want.n == len(sc.CASES)
    for i, (label, _) in enumerate(sc.CASES):
        got = bytes(text[int(line_off[i]):int(line_off[i + 1])])
        if i in sc.NOT_ASCII:
            assert got.endswith(b"\t" + bytes([133, 233, 255]) + b"\n"), label
            continue
        assert got == want.sam_line(i).encode("latin-1") + b"\n", label
    assert int(line_off[-1]) == text.size


def test_corpus_edge_literals():
    """A few lines written down by hand, so the comparison above does not rest on sam_line alone."""
    s = sc.stream()
    text, line_off = sb.sam_text_host(s.flat, s.starts, sc.REF_NAMES)
    line = {label: bytes(text[int(line_off[i]):int(line_off[i + 1])]) for i, (label, _) in enumerate(sc.CASES)}
    assert line["edges_low"] == b"r\t0\t*\t0\t0\t*\t*\t0\t-2147483648\t*\t*\n"
    assert line["edges_high"] == b"r\t65535\tchr1\t2147483647\t255\t*\t=\t2147483647\t2147483647\t*\t*\n"
    assert line["pos_int_max"] == b"r\t4\tchr10\t2147483648\t7\t*\tchr2\t2147483648\t-33\t*\t*\n"
    assert line["pos_negative"] == b"r\t4\tchr10\t-4\t7\t*\tchr2\t-2147483647\t-33\t*\t*\n"
    assert line["ref_past_end_eq"] == b"r\t4\t*\t778\t7\t*\t=\t889\t-33\t*\t*\n"
    assert line["next_past_end"] == b"r\t4\tchrM\t778\t7\t*\t*\t889\t-33\t*\t*\n"
    assert line["name0"] == b"\t4\tchr10\t778\t7\t*\tchr2\t889\t-33\t*\t*\n"
    assert line["cigar_all_ops"].split(b"\t")[5] == b"1M2I3D4N5S6H7P8=9X"
    assert line["cigar1"].split(b"\t")[5] == b"0M"
    assert line["int_tags"].split(b"\t")[11:] == [
        b"Xc:i:-128", b"Xc:i:127", b"XC:i:0", b"XC:i:255", b"Xs:i:-32768", b"Xs:i:32767", b"XS:i:0", b"XS:i:65535",
        b"Xi:i:-2147483648", b"Xi:i:2147483647", b"XI:i:0", b"XI:i:4294967295\n"]
    assert line["float_bf"].split(b"\t")[11:] == [b"XB:B:f,0.25,-2.5,12.75", b"XE:B:f\n"]
    assert line["tag_h"].split(b"\t")[11:] == [b"XH:H:1AE301", b"XE:H:\n"]
    assert line["b_c"].split(b"\t")[11:13] == [b"B0:B:c", b"B1:B:c,-128"]


@pytest.mark.parametrize("x,want", sc.FLOATS, ids=[w for _, w in sc.FLOATS])
def test_float_to_string(x, want):
    s = rc.lay([sc.float_record(x)])
    text, _ = sb.sam_text_host(s.flat, s.starts, sc.REF_NAMES)
    assert bytes(text).split(b"\t")[11:] == [b"XF:f:" + want.encode(), b"XB:B:f," + want.encode() + b"\n"]


def render_raw(flat, starts, text_cap=None):
    """sbh_sam_render_host itself: (status, bad_row, line_off, text)."""
    flat = np.frombuffer(flat, np.uint8)
    st = np.asarray(starts, np.uint64)
    names, off = sb.records.pack_ref_names(sc.REF_NAMES)
    line_off = np.zeros(st.size + 1, np.uint64)
    bad = C.c_uint64(12345)
    text = None if text_cap is None else np.zeros(max(text_cap, 1), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc_ = sb.lib().sbh_sam_render_host(p(flat), flat.size, p(st), st.size, p(names), p(off), off.size - 1,
                                       None if text is None else p(text), text_cap or 0, p(line_off), C.byref(bad))
    return rc_, bad.value, line_off, text


@pytest.mark.parametrize("m", sc.MALFORMED, ids=lambda m: m.name)
def test_malformed_row_is_named(m):
    rc_, bad, line_off, _ = render_raw(m.stream.flat, m.stream.starts)
    assert rc_ == SBH_E_BAD_RECORD and bad == m.bad_row
    # the good rows before it render
    ok, bad, _, _ = render_raw(m.stream.flat, m.stream.starts[:m.bad_row])
    assert ok == 0 and bad == 2 ** 64 - 1
    with pytest.raises(sb.SparkBamError) as e:
        sb.sam_text_host(m.stream.flat, m.stream.starts, sc.REF_NAMES)
    assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (m.bad_row,)


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_record_that_does_not_fit_is_bad(m):
    """The rows records_scan refuses (record_corpus.MALFORMED_CASES) are refused here too."""
    rc_, bad, _, _ = render_raw(m.stream.flat, m.stream.starts)
    assert rc_ == SBH_E_BAD_RECORD and bad == 3


def test_text_cap_one_byte_short():
    s = sc.stream()
    _, _, line_off, _ = render_raw(s.flat, s.starts)
    total = int(line_off[-1])
    rc_, _, _, text = render_raw(s.flat, s.starts, text_cap=total)
    assert rc_ == 0
    short, _, _, _ = render_raw(s.flat, s.starts, text_cap=total - 1)
    assert short == SBH_E_ARG
    assert bytes(text[:total]) == bytes(sb.sam_text_host(s.flat, s.starts, sc.REF_NAMES)[0])


def test_no_records():
    s = sc.stream()
    text, line_off = sb.sam_text_host(s.flat, [], sc.REF_NAMES)
    assert text.size == 0 and line_off.tolist() == [0]
