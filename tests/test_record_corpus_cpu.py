"""The record conformance corpus (record_corpus.py) against the CPU oracle and against its
own hand-written expectations: the GPU suite compares the kernels with oracle_records, and
this file compares oracle_records with literals, so the reference the GPU is held to is
itself pinned.  No GPU."""
import struct

import numpy as np
import pytest

from oracle_lib import OracleFile
import oracle_records as orr
import record_corpus as rc


def _decode_all(s):
    return orr.decode(s.flat, orr.record_starts(s.flat, s.first, len(s.flat)))


def test_header_is_a_bam_header_over_four_contigs_out_of_name_order():
    names, first = orr.bam_refs(rc.header())
    assert names == [n for n, _ in rc.CONTIGS] and first == len(rc.header())
    assert len(names) >= 4 and names != sorted(names)


def test_decode_table_round_trips_through_the_oracle():
    s = rc.decode_stream()
    assert orr.record_starts(s.flat, s.first, len(s.flat)) == s.starts
    got = _decode_all(s)
    want = rc.expected_columns(rc.DECODE_CASES)
    assert got.pop("flat").tolist() == s.starts
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k], want[k]), k


def test_decode_table_covers_what_it_claims():
    cases = {c.label: c for c in rc.DECODE_CASES}
    s = rc.decode_stream()
    assert set(rc.SEQ_LENGTHS) <= {len(c.seq_codes) for c in rc.DECODE_CASES}
    assert set(rc.NAME_LENGTHS) <= {len(c.name) + 1 for c in rc.DECODE_CASES}
    assert set(rc.CIGAR_COUNTS) | {65535} <= {len(c.cigar) for c in rc.DECODE_CASES}
    assert set(rc.AUX_LENGTHS) <= {len(c.aux) for c in rc.DECODE_CASES}
    # all 16 codes in the high nibble and in the low one
    flat = s.flat
    for label, phase in (("codes_hi", 0), ("codes_lo", 1)):
        c = cases[label]
        assert {x for k, x in enumerate(c.seq_codes) if k % 2 == phase} >= set(range(0, 16, 2))
        assert {x for k, x in enumerate(c.seq_codes) if k % 2 != phase} >= set(range(1, 16, 2))
    hi = {x for c in rc.DECODE_CASES for x in c.seq_codes[0::2]}
    lo = {x for c in rc.DECODE_CASES for x in c.seq_codes[1::2]}
    assert hi == lo == set(range(16))
    # the spare nibble of an odd l_seq is really set in the bytes, and is not a base
    for label in ("odd_spare", "odd_spare1"):
        c = cases[label]
        p = s.starts[[x.label for x in rc.DECODE_CASES].index(label)]
        last = p + 36 + len(c.name) + 1 + 4 * len(c.cigar) + len(c.seq_codes) // 2
        assert len(c.seq_codes) % 2 == 1 and flat[last] & 15 == c.spare != 0
    assert set(cases["qual_ff"].qual) == {0xFF}
    # n_cigar_op and flag at their limits in the shared word
    for label, word in (("cig_max", 0x0000FFFF), ("flag_max", 0xFFFF0001)):
        p = s.starts[[x.label for x in rc.DECODE_CASES].index(label)]
        assert struct.unpack_from("<I", flat, p + 16)[0] == word
    assert {op for _, op in cases["cig_max"].cigar} == set(range(16))
    # a CIGAR's first word at each of the four addresses mod 4
    at = {(p + 36 + len(c.name) + 1) % 4 for p, c in zip(s.starts, rc.DECODE_CASES) if c.cigar}
    assert at == {0, 1, 2, 3}
    # tag bytes: none (block_size exactly the parts), with 0x00 and 0xFF, and a B array
    assert any(not c.aux and struct.unpack_from("<i", flat, p)[0] == 32 + len(c.name) + 1 + 4 * len(c.cigar)
               + (len(c.seq_codes) + 1) // 2 + len(c.seq_codes) for p, c in zip(s.starts, rc.DECODE_CASES))
    assert {0x00, 0xFF} <= set(cases["aux65"].aux) and cases["aux_b_array"].aux[2:4] == b"BS"
    lo_, hi_ = cases["edges_low"], cases["edges_high"]
    assert (lo_.ref_id, lo_.next_ref, lo_.pos, lo_.next_pos, lo_.tlen, lo_.bin, lo_.mapq) == \
        (-1, -1, -1, -1, -2 ** 31, 0xFFFF, 255)
    assert hi_.tlen == 2 ** 31 - 1


@pytest.mark.parametrize("payload", rc.PAYLOADS)
def test_built_files_inflate_to_the_flat_bytes(payload):
    streams = [rc.decode_stream(), rc.interval_stream()] + [m.stream for m in rc.MALFORMED_CASES]
    for s in streams:
        data = rc.bgzf(s.flat, payload)
        assert rc.inflate_members(data) == s.flat
        assert data.endswith(rc.EOF_MEMBER)
    if payload == 97:  # most records straddle members, and some start exactly at a member's end
        for s in (rc.decode_stream(), rc.interval_stream()):
            ends = s.starts[1:] + [len(s.flat)]
            assert 2 * sum(a // 97 != (b - 1) // 97 for a, b in zip(s.starts, ends)) > len(s.starts)
    s = rc.decode_stream()
    for label, at in rc.MEMBER_END_STARTS:
        p = s.starts[[c.label for c in rc.DECODE_CASES].index(label)]
        assert 0 < p < len(s.flat) and p % at == 0


def test_oracle_file_reads_the_built_bgzf():
    s = rc.decode_stream()
    of = OracleFile(np.frombuffer(rc.bgzf(s.flat, 4096), np.uint8))
    assert of.flat_size == len(s.flat) and of.uncompressed().tobytes() == s.flat
    assert of.header_end == s.first and of.contig_len.tolist() == [ln for _, ln in rc.CONTIGS]


def test_eager_checker_rejects_some_decode_records():
    """The decode table is deliberately odd: the eager checker must not accept every record of
    it, so a bitmap over it is not the record chain and delivery has to mark the chain."""
    s = rc.decode_stream()
    of = OracleFile(np.frombuffer(rc.bgzf(s.flat, 65280), np.uint8))
    _, bits = of.eager_range(0, of.flat_size)
    accepted = [bool(bits[p >> 3] >> (p & 7) & 1) for p in s.starts]
    assert not all(accepted)


def test_interval_table_literals_match_the_oracle():
    s = rc.interval_stream()
    labels = [c.label for c in rc.INTERVAL_RECORDS]
    assert len(set(labels)) == len(labels)
    cols = _decode_all(s)
    assert cols["flat"].tolist() == s.starts
    for case in rc.INTERVAL_CASES:
        by_ref = rc.loci_by_ref(case.intervals)
        kept = tuple(labels[i] for i in range(len(labels)) if orr.region_kept(cols, i, by_ref))
        assert kept == case.kept, case.name


def test_interval_table_regions_are_the_ones_written_next_to_them():
    cols = _decode_all(rc.interval_stream())
    want = {"neg1_s1": (0, -1, 0), "neg1_s5": (0, -1, 4), "m_only": (0, 100, 110), "d_only": (0, 200, 210),
            "n_only": (0, 300, 310), "eq_only": (0, 400, 410), "x_only": (0, 500, 510), "mix": (0, 600, 620),
            "hi_ops": (0, 700, 705), "edge": (0, 1000, 1020), "c1_a": (1, 50, 60), "c1_b": (1, 5000, 5010),
            "c2_a": (2, 100, 110), "c2_big10": (2, 2 ** 31 - 8, 2 ** 31 + 2), "c2_big20": (2, 2 ** 31 - 8, 2 ** 31 + 12),
            "c3_a": (3, 10, 20), "c3_b": (3, 1000, 1010)}
    empty = {"no_cigar", "clip_only", "unmapped_placed"}
    for i, c in enumerate(rc.INTERVAL_RECORDS):
        r = orr.region(cols, i)
        if c.label in want:
            assert r == want[c.label], c.label
        elif c.label in empty:
            assert r is not None and r[1] >= r[2], c.label
        else:
            assert c.label == "noref_cigar" and r is None


def test_interval_table_covers_what_it_claims():
    ivs = [case.intervals for case in rc.INTERVAL_CASES]
    assert () in ivs
    assert any({r for r, _, _ in iv} == {0, 2} for iv in ivs) and any({r for r, _, _ in iv} == {3} for iv in ivs)
    assert any(max(b for _, _, b in iv) > 2 ** 31 and min(a for _, a, _ in iv) > 2 ** 31 for iv in ivs if iv)
    assert any(len([1 for r, _, _ in iv if r == 1]) >= 4 for iv in ivs)
    assert {c.ref_id for c in rc.INTERVAL_RECORDS} == {-1, 0, 1, 2, 3}
    ops = {op for c in rc.INTERVAL_RECORDS for _, op in c.cigar}
    assert ops == set(range(16))
    # every accepted interval list is what the library asks for: non-empty, sorted, disjoint
    for iv in ivs:
        assert all(a < b for _, a, b in iv)
        assert all((r0, b0) <= (r1, a1) for (r0, _, b0), (r1, a1, _) in zip(iv, iv[1:]))


def test_chunk_table_literals_match_the_oracle():
    s = rc.interval_stream()
    by_ref = rc.loci_by_ref(rc.ALL_INTERVALS)
    for case in rc.CHUNK_CASES:
        cols, per = orr.interval_records(s.flat, rc.chunk_flats(case), by_ref)
        assert cols["flat"].tolist() == [rc.interval_start(x) for x in case.kept], case.name
        assert tuple(per) == case.per, case.name
    names = {c.name for c in rc.CHUNK_CASES}
    assert names == {"ends_at_record_start", "ends_one_byte_in", "adjacent", "empty_chunk", "end_past_stream"}


def test_malformed_cases_are_malformed_where_they_say():
    assert [m.name for m in rc.MALFORMED_CASES] == ["block_size_one_short", "l_seq_minus_one", "block_size_minus_five",
                                                    "35_bytes_left", "one_byte_past_stream"]
    parts = len(rc.rec_bytes(rc.BAD)) - 4
    for m in rc.MALFORMED_CASES:
        s = m.stream
        assert len(s.starts) >= 4 and m.bad_start == s.starts[3]
        good = orr.decode(s.flat, s.starts[:3])  # the good prefix decodes
        want = rc.expected_columns(rc.GOOD)
        assert all(np.array_equal(good[k], want[k]) for k in want)
        left = len(s.flat) - m.bad_start
        bsz, = struct.unpack_from("<i", s.flat, m.bad_start)
        if m.name == "35_bytes_left":
            assert left == 35
            continue
        l_seq, = struct.unpack_from("<i", s.flat, m.bad_start + 20)
        assert left == 4 + parts
        assert {"block_size_one_short": bsz == parts - 1, "l_seq_minus_one": l_seq == -1 and bsz == parts,
                "block_size_minus_five": bsz == -5, "one_byte_past_stream": m.bad_start + 4 + bsz == len(s.flat) + 1}[m.name]
    # the interval the GPU test uses would keep the bad record were it well-formed
    s = rc.lay([rc.rec_bytes(c) for c in rc.GOOD + (rc.BAD,)])
    cols = _decode_all(s)
    assert orr.region_kept(cols, 3, rc.loci_by_ref(rc.BAD_KEEPING_INTERVALS))


def test_grid_stream_rows_are_what_the_builder_gives():
    s, a = rc.grid_stream()
    assert len(s.starts) == rc.GRID_RECORDS > 262144 and len(s.flat) - s.first == 44 * rc.GRID_RECORDS
    for i in (0, 1, 9, 10, 65535, 262143, 262144, rc.GRID_RECORDS - 1):
        p = int(s.starts[i])
        assert s.flat[p:p + 44] == rc.rec_bytes(rc.grid_case(i)), i
    idx = list(range(50)) + list(range(rc.GRID_RECORDS - 50, rc.GRID_RECORDS))
    got = orr.decode(s.flat, [int(s.starts[i]) for i in idx])
    want = rc.expected_columns([rc.grid_case(i) for i in idx])
    for k in want:
        assert np.array_equal(got[k], want[k]), k
