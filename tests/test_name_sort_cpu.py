"""The host side of the read-name sort (csrc/bam_name_core.h through the library, no GPU):
sbh_bam_name_sort_host against the pure-Python restatement of name_sort_corpus.py on every corpus --
the permutation and the group summary -- the written-down expectations of the built cases, rows in
any order, and malformed rows."""
import numpy as np
import pytest

from pkg import sb
import name_sort_corpus as nc
import record_corpus as rc

SBH_E_BAD_RECORD = sb._lib.SBH_E_BAD_RECORD


def test_restatement_on_known_records():
    rows = [(b"b", 0), (b"a", nc.READ2), (b"a", nc.READ1), (b"a", nc.READ1 | nc.SUPPLEMENTARY), (b"a", nc.READ1 | nc.SECONDARY),
            (b"", 0), (b"ab", 0), (b"a\xff", 0), (b"a", nc.READ1)]
    s = nc.stream_of(rows)
    padded, tie, length = nc.fields_of(s.flat, s.starts)
    assert tie[:5] == [0, 8, 4, 6, 5] and length == [1, 1, 1, 1, 1, 0, 2, 2, 1] and padded[6] == b"ab" + bytes(254)
    # the empty name, then "a": read 1 primary (twice, in scan order), secondary, supplementary, read 2; then the
    # names "a" is a prefix of, bytes unsigned; then "b"
    assert nc.perm_ref(s.flat, s.starts).tolist() == [5, 2, 8, 4, 3, 1, 6, 7, 0]
    assert nc.info_ref(s.flat, s.starts) == dict(n_names=5, n_single=4, n_pair=0, n_more=1, max_name=2, chunks_run=0,
                                                 passes_run=0, already=False)
    assert sb.bam_name_sort_host(s.flat, s.starts)[0].tolist() == [5, 2, 8, 4, 3, 1, 6, 7, 0]


def test_an_l_read_name_of_zero_is_the_empty_name():
    s = nc.stream_of([(b"", 0, 0), (b"", 0)])
    assert s.flat[s.starts[0] + 12] == 0 and s.flat[s.starts[1] + 12] == 1
    perm, info = sb.bam_name_sort_host(s.flat, s.starts)
    assert perm.tolist() == [0, 1] and info["n_names"] == 1 and info["n_pair"] == 1 and info["max_name"] == 0


@pytest.mark.parametrize("name", nc.SMALL + ("grid",))
def test_name_sort_host_is_the_restatement(name):
    s = nc.stream(name)
    perm, info = sb.bam_name_sort_host(s.flat, s.starts)
    want = nc.expected_perm(name)
    assert perm.dtype == np.uint64 and np.array_equal(perm, want)
    assert info == nc.expected_info(name)
    nc.check_expect(name, info, device=False)
    assert info["already"] == np.array_equal(want, np.arange(len(s.starts), dtype=np.uint64))
    assert info["n_single"] + 2 * info["n_pair"] <= len(s.starts) and (info["n_more"] > 0) == (
        info["n_single"] + 2 * info["n_pair"] < len(s.starts))


def test_byte_edges_come_out_as_written():
    s = nc.stream("byte_edges")
    # each pair's smaller name second in the stream; the triple: AA, AB, BA; the last pair by its first byte
    names = [nc.CORPORA["byte_edges"]()[int(i)][0] for i in sb.bam_name_sort_host(s.flat, s.starts)[0]]
    assert names == sorted(names) and names.index(b"mmmmmmmABmmmmmmm") < names.index(b"mmmmmmmBAmmmmmmm")
    assert names[0] == b"\x01\x02\x03\x04\x05\x06\x07\x08"


def test_rows_in_any_order_and_twice():
    s = nc.stream("shuffled")
    st = np.concatenate([s.starts[:50][::-1], s.starts[:50], s.starts[7:8] * 3])
    perm, info = sb.bam_name_sort_host(s.flat, st)
    assert np.array_equal(perm, nc.perm_ref(s.flat, st)) and info == nc.info_ref(s.flat, st)
    perm, info = sb.bam_name_sort_host(b"", [])
    assert perm.size == 0 and info == nc.info_ref(b"", [])


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed_row(m):
    with pytest.raises(sb.SparkBamError) as e:
        sb.bam_name_sort_host(m.stream.flat, m.stream.starts)
    assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (3,)
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        with pytest.raises(sb.SparkBamError) as e:
            sb.bam_name_sort_host(m.stream.flat, m.stream.starts[:2] + [p])
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (2,)


def test_exports():
    assert {"sbh_records_bam_scan_names", "sbh_records_bam_name_info", "sbh_bam_name_sort_host"} <= set(sb._lib.EXPORTS)
    assert callable(sb.bam_name_sort_host)
