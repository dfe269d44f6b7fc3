"""The host side of the coordinate sort (csrc/bam_sort_core.h through the library, no GPU):
sbh_bam_sort_host against the numpy restatement of bam_sort_corpus.py on every corpus, malformed
rows, and sbh_bam_header_set_so on each header shape and on 2.bam's own header."""
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT, golden_bam
from pkg import sb
import bam_sort_corpus as sc
import record_corpus as rc

SBH_E_ARG, SBH_E_BAD_RECORD = sb._lib.SBH_E_ARG, sb._lib.SBH_E_BAD_RECORD


def test_tile_constant_is_the_library_s():
    with open(os.path.join(ROOT, "spark-bam_amd", "csrc", "bam_sort_core.h")) as f:
        m = re.search(r"SORT_WAVES = (\d+), SORT_ITEMS = (\d+), SORT_TILE = SORT_WAVES \* 64 \* SORT_ITEMS;", f.read())
    assert m and int(m.group(1)) * 64 * int(m.group(2)) == sc.SORT_TILE


def test_builder_rows_are_rec_s_bytes():
    ref, pos, flag = sc.CORPORA["edge_65"]()
    s = sc.stream_of(ref, pos, flag)
    for i in (0, 7, 64):
        want = rc.rec(int(ref[i]), int(pos[i]), i % 251, 4681, int(flag[i]), -1, -1, i % 1000 - 500, b"%07d" % i,
                      (), (), b"", b"")
        assert s.flat[int(s.starts[i]):int(s.starts[i]) + 44] == want


def test_restated_keys_on_known_records():
    s = rc.lay([rc.rec(2, 99, 0, 0, 0x10, -1, -1, 0, b"a", (), (), b"", b""),
                rc.rec(-1, -1, 0, 0, 0, -1, -1, 0, b"b", (), (), b"", b""),
                rc.rec(0, 2 ** 31 - 1, 0, 0, 0, -1, -1, 0, b"c", (), (), b"", b""),
                rc.rec(0, -2, 0, 0, 0, -1, -1, 0, b"d", (), (), b"", b"")])
    assert sc.keys_of(s.flat, s.starts).tolist() == [2 << 33 | 100 << 1 | 1, 0x7FFFFFFF << 33, 2 ** 31 << 1,
                                                    0xFFFFFFFF << 1]
    # pos == -2 wraps behind every real position of its reference (the header comment's rule)
    assert sb.bam_sort_host(s.flat, s.starts).tolist() == [2, 3, 0, 1]


@pytest.mark.parametrize("name", sc.CORPORA)
def test_sort_host_is_the_restatement(name):
    s = sc.stream(name)
    perm = sb.bam_sort_host(s.flat, s.starts)
    want = sc.expected_perm(name)
    assert perm.dtype == np.uint64 and np.array_equal(perm, want)
    if name in ("all_equal", "sorted"):
        assert np.array_equal(perm, np.arange(len(s.starts), dtype=np.uint64))
    if name == "two_alternating":  # the odd rows (the smaller key) in order, then the even ones
        n = len(s.starts)
        assert perm.tolist() == list(range(1, n, 2)) + list(range(0, n, 2))
    if name == "unplaced_mixed":
        k = sc.keys_of(s.flat, s.starts)[perm.astype(np.int64)]
        n_un = int((np.arange(len(s.starts)) % 3 == 0).sum())
        assert (k[-n_un:] >> np.uint64(33) == 0x7FFFFFFF).all() and (k[:-n_un] >> np.uint64(33) < 5).all()


def test_sort_host_rows_in_any_order_and_twice():
    s = sc.stream("shuffled")
    st = np.concatenate([s.starts[:50][::-1], s.starts[:50], s.starts[7:8].repeat(3)])
    assert np.array_equal(sb.bam_sort_host(s.flat, st), sc.perm_ref(s.flat, st))


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed_row(m):
    with pytest.raises(sb.SparkBamError) as e:
        sb.bam_sort_host(m.stream.flat, m.stream.starts)
    assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (3,)
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        with pytest.raises(sb.SparkBamError) as e:
            sb.bam_sort_host(m.stream.flat, m.stream.starts[:2] + [p])
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (2,)


@pytest.mark.parametrize("shape", sc.HEADER_SHAPES, ids=lambda s: s[0])
def test_header_set_so_shapes(shape):
    _, text, pad, want_text = shape
    head = sc.header_with(text, pad)
    got = sb.bam_header_set_so(head, "coordinate")
    assert got == sc.header_with(want_text, pad)
    names, lens, end = sb.parse_bam_header(np.frombuffer(got, np.uint8))
    assert (names, list(lens), end) == ([c[0] for c in rc.CONTIGS], [c[1] for c in rc.CONTIGS], len(got))
    assert sb.bam_header_set_so(got, "coordinate") == got  # idempotent
    assert sb.bam_header_set_so(got, "unsorted") == sc.header_with(want_text.replace("SO:coordinate", "SO:unsorted", 1), pad)


def test_header_set_so_on_2_bam():
    data = open(golden_bam("2.bam"), "rb").read()
    flat = rc.inflate_members(data)
    names, lens, end = sb.parse_bam_header(np.frombuffer(flat, np.uint8))
    head = flat[:end]
    l_text = struct.unpack_from("<i", head, 4)[0]
    text = head[8:8 + l_text]
    assert text.startswith(b"@HD\tVN:1.5\tGO:none\tSO:coordinate\n")
    assert sb.bam_header_set_so(head, "coordinate") == head
    got = sb.bam_header_set_so(head, "queryname")
    want_text = text.replace(b"SO:coordinate", b"SO:queryname", 1)
    assert got == head[:4] + struct.pack("<i", len(want_text)) + want_text + head[8 + l_text:]
    n2, l2, e2 = sb.parse_bam_header(np.frombuffer(got, np.uint8))
    assert (n2, list(l2), e2) == (names, list(lens), len(got))


@pytest.mark.parametrize("bad", [b"", b"BAM\1", b"BAX\1" + bytes(8), b"BAM\1" + struct.pack("<i", -1) + bytes(4),
                                 b"BAM\1" + struct.pack("<i", 9) + bytes(8)], ids=repr)
def test_header_set_so_refuses_what_is_no_header(bad):
    with pytest.raises(sb.SparkBamError) as e:
        sb.bam_header_set_so(bad, "coordinate")
    assert e.value.code == SBH_E_ARG


@pytest.mark.parametrize("so", ["", "a\tb", "x\ny"])
def test_header_set_so_refuses_a_bad_value(so):
    with pytest.raises(sb.SparkBamError) as e:
        sb.bam_header_set_so(rc.header(), so)
    assert e.value.code == SBH_E_ARG


def test_exports():
    assert {"sbh_records_bam_scan_order", "sbh_records_bam_sorted", "sbh_bam_sort_host",
            "sbh_bam_header_set_so"} <= set(sb._lib.EXPORTS)
    assert callable(sb.sort_bam) and callable(sb.bam_sort_host)
