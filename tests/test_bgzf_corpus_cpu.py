"""The BGZF container corpus (bgzf_corpus.py) held to references that share nothing with it:
Python's zlib for every member's bytes and footer, the oracle's MetadataStream
(or_metadata_next / or_metadata_stream) for the member tables, the oracle's FindBlockStart for
the probe literals -- and the coverage the corpus claims, asserted on the corpus itself."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

import bgzf_corpus as bc
from oracle_lib import OR_END, OR_OK, OR_SEARCH_FAILED, OR_TRUNCATED, lib, metadata_next, metadata_stream


def valid_files():
    """(file, indices of members whose footer CRC is wrong on purpose)."""
    out = [(f, ()) for f in bc.index_files() if f.name != "tail_min"]
    out += [(f, ()) for f in bc.crc_sizes()]
    out += [(c.file, c.bad) for c in bc.crc_bad() + (bc.crc_stream_case(),)]
    out += [(f, ()) for k, f in bc.fbs_files().items() if k != "planted"]
    return out


def test_stored_raw_is_deflate_builds_stored_block():
    for n in (0, 1, 2, 31, 255, 256, 4096):
        d = bc.quiet(n, n)
        assert bc.stored_raw(d) == bc.stored_raw_bits(d)


def test_member_builder_fields():
    x = bc.subfield(1, 2, b"abc") + bc.subfield(3, 4, b"")
    m = bc.bgzf_member(b"\x03\x00", 7, 0x01020304, x)
    assert len(m) == 18 + 11 + 2 + 8 and m[10:12] == struct.pack("<H", 17)
    assert struct.unpack("<H", m[16:18])[0] == len(m) - 1 and m[18:29] == x
    assert m[-8:] == struct.pack("<II", 0x01020304, 7)
    assert bc.bgzf_member(b"\x03\x00", 0, 0)[:18] == bc.header18(28)
    assert bc.bgzf_member(b"\x03\x00", 0, 0) == bc.EOF_MEMBER


@pytest.mark.parametrize("f,bad", valid_files(), ids=lambda v: v.name if isinstance(v, bc.File) else None)
def test_members_decode_with_zlib(f, bad):
    """Member by member: raw inflate of the bytes behind the header gives the builder's flat bytes,
    and the footer is their crc32 and length (a wrong CRC exactly on the members named)."""
    flat, ust = bytearray(), bc.ustarts(f.table)[0]
    for i, m in enumerate(f.table):
        raw = f.data[m.start:m.start + m.csize]
        assert raw[:4] == bc.MAGIC and struct.unpack("<H", raw[10:12])[0] == m.hsize - 12
        assert struct.unpack("<H", raw[16:18])[0] == m.csize - 1
        d = zlib.decompressobj(-15)
        u = d.decompress(raw[m.hsize:-8]) + d.flush()
        assert d.eof and d.unused_data == b""
        crc, isize = struct.unpack("<II", raw[-8:])
        assert isize == len(u) == m.usize and m.empty == (m.csize - m.hsize - 8 == 2)
        assert len(flat) == ust[i]
        if i in bad:
            assert zlib.crc32(u) != crc, (f.name, i)
        else:
            assert zlib.crc32(u) == crc, (f.name, i)
        flat += u
    if not bad:
        assert bytes(flat) == f.flat
    else:
        assert len(flat) == len(f.flat)  # (payload edits: the flat bytes differ at the edits only)
    last = f.table[-1]
    assert f.name in ("false",) or f.name.startswith("tails") or last.start + last.csize == len(f.data)


def test_whole_files_decode_with_gzip():
    """The multi-member gzip reader agrees too (files that are chains from offset 0 to their end)."""
    for f in (bc.edges(), bc.shapes(), bc.planted(), bc.many()) + bc.crc_sizes():
        assert gzip.decompress(f.data) == f.flat, f.name


@pytest.mark.parametrize("f", bc.index_files() + bc.crc_sizes() + tuple(bc.fbs_files().values()),
                         ids=lambda f: f.name)
def test_table_equals_metadata_stream(f):
    data = np.frombuffer(f.data, np.uint8)
    pos = f.table[0].start if f.table else 0
    for m in f.table:
        rc, got = metadata_next(data, pos)
        assert rc == (OR_END if m.empty else OR_OK), (f.name, m)
        assert got == (m.start, m.csize, m.hsize, m.usize, int(m.empty)), (f.name, m)
        pos += m.csize
    # what follows the table is no member wholly inside the file
    rc, _ = metadata_next(data, pos)
    assert rc != OR_OK and (rc != OR_END or pos + 18 > len(f.data)), f.name
    # MetadataStream from the first member stops at the first empty one
    want = []
    for m in f.table:
        if m.empty:
            break
        want.append(tuple(m[:4]) + (0,))
    got = metadata_stream(data, f.table[0].start if f.table else 0)
    if any(m.empty for m in f.table) or pos + 18 > len(f.data):
        assert got == want, f.name
    else:
        assert got < 0, f.name  # (a cut inside the next member, or bytes that are no header)


@pytest.mark.parametrize("p", bc.FBS, ids=lambda p: p.name)
def test_fbs_literals_are_the_oracles_answers(p):
    f = bc.fbs_files()[p.file]
    data = np.frombuffer(f.data, np.uint8)
    out = C.c_int64(-1)
    rc = lib().or_find_block_start(data.ctypes.data_as(C.c_void_p), data.size, p.start, p.blocks_to_check,
                                   C.byref(out))
    got = {OR_OK: (bc.OK, out.value), OR_SEARCH_FAILED: (bc.SEARCH_FAILED,), OR_TRUNCATED: (bc.TRUNCATED,)}[rc]
    assert got == p.want
    assert p.cut is None or p.start < p.cut < len(f.data)
    assert bc.FBS_FALSE_LEN == len(bc.fbs_files()["false"].data)


def test_fbs_gap_holds_no_magic_and_probes_cover_the_outcomes():
    gap = bc.fbs_files()["gap"]
    assert bc.candidates(gap.data)[0] == bc.FBS_GAP == gap.table[0].start
    assert 31 not in gap.data[:bc.FBS_GAP]
    wants = {p.want[0] for p in bc.FBS}
    assert wants == {bc.OK, bc.SEARCH_FAILED, bc.TRUNCATED}
    assert {p.blocks_to_check for p in bc.FBS} >= {0, 1, 3, 4, 5, 6}
    last = [p for p in bc.FBS if p.file == "false" and bc.FBS_FALSE_LEN - p.start <= 17]
    assert last


# ------------------------------------------------------------------------------- coverage
def test_edges_cover_every_listed_offset():
    f = bc.edges()
    have = {}
    for m, e in zip(f.table, f.meta):
        if e:
            kind, b, d = e
            assert m.start == b - d
            assert b % bc.SEG == 0 and (b % bc.CHUNK == 0) == (kind == "chunk")
            have.setdefault(kind, set()).add(d)
    assert have["chunk"] == set(range(-1, 19)) and have["seg"] == set(bc.EDGE_D_SEG)
    assert {m.start % 16 for m in f.table} == set(range(16))
    # a magic that begins in a vector's last three bytes (the scan's separate path), also across
    # a segment edge and a chunk edge
    late = [m.start for m in f.table if m.start % 16 >= 13]
    assert any(s % bc.CHUNK > bc.CHUNK - 4 for s in late)
    assert any(bc.SEG - 4 < s % bc.SEG and s % bc.CHUNK < bc.CHUNK - 4 for s in late)
    # no header but the members': every candidate is on the chain
    assert bc.candidates(f.data) == [m.start for m in f.table]
    assert 300_000 < len(f.data) < 400_000


def test_tails_cover_every_residue_and_the_header_cuts():
    for base in ("tails_small_", "tails_"):
        fs = [f for f in bc.tails() if f.name.startswith(base) and (base == "tails_small_" or "small" not in f.name)]
        assert {len(f.data) % 16 for f in fs} == set(range(16))
        by = {f.name[len(base):]: f for f in fs}
        e = len(by["member_end"].data)
        assert [len(by[k].data) - e for k in ("hdr1", "hdr17", "hdr18", "hdr19")] == [1, 17, 18, 19]
        assert by["member_end"].table == by["hdr19"].table == by["short1"].table
        assert by["member_end"].table[-1].start + by["member_end"].table[-1].csize == e
        assert len(by["short1"].data) + 1 == by["whole"].table[len(by["short1"].table)].start + \
            by["whole"].table[len(by["short1"].table)].csize
        assert (len(by["whole"].data) > bc.CHUNK) == (base == "tails_")
    t = bc.tail_min()
    assert t.table[-1].start + 18 == len(t.data) and t.table[-1].csize == 18


def test_shapes_hold_what_they_name():
    f = bc.shapes()
    by = dict(zip(f.meta, f.table))
    assert by["xlen13_deflate"].hsize == by["xlen13_stored"].hsize == 25
    assert by["xlen17_deflate"].hsize == by["xlen17_stored"].hsize == 29
    assert by["stored0"][1:] == (31, 18, 0, False)
    assert by["isize65536"].usize == 65536
    assert by["empty_pair1"].start - by["empty_pair0"].start == 28
    # two real candidates in one thread's 64 bytes of the rescan
    assert by["empty_pair0"].start // 64 == by["empty_pair1"].start // 64 or \
        by["empty_pair1"].start // 64 == by["after_pair"].start // 64
    assert [m.empty for m in f.table].count(True) == 4 and f.table[-1].empty


def test_planted_candidates_and_chunks():
    f = bc.planted()
    cand = bc.candidates(f.data)
    assert cand == sorted([m.start for m in f.table] + [p for p, _, _ in bc.PLANTS])
    per = {}
    for c in cand:
        per[c // bc.CHUNK] = per.get(c // bc.CHUNK, 0) + 1
    assert 1 in per.values() and max(per.values()) >= 3
    off = {lab: (p, cs) for p, cs, lab in bc.PLANTS}
    starts = {m.start for m in f.table}
    for lab in ("a_mid", "a_edge"):
        p, cs = off[lab]
        assert p + cs not in cand
    for lab in ("b_mid", "b_edge"):
        p, cs = off[lab]
        assert p + cs in starts
    for lab in ("c_mid", "c_edge"):
        p0, p1, p2 = (off[lab + str(i)] for i in range(3))
        assert p0[0] + p0[1] == p1[0] and p1[0] + p1[1] == p2[0] and p2[0] + p2[1] in starts
    d = [off["d_mid%d" % i][0] for i in range(3)]
    assert d[1] - d[0] == d[2] - d[1] == 18 and d[0] // 64 == d[2] // 64
    for lab in ("a_edge", "b_edge", "c_edge0", "d_edge1"):
        p = off[lab][0]
        assert p // bc.CHUNK != (p + 17) // bc.CHUNK  # the 18 bytes straddle a chunk edge
    for lab in ("a_mid", "b_mid", "c_mid0", "d_mid0"):
        p = off[lab][0]
        assert 100 < p % bc.CHUNK < bc.CHUNK - 100


def test_many_exceeds_one_scan_workgroup_and_the_crc_grid():
    f = bc.many()
    assert len(f.table) > 2048 and sum(not m.empty for m in f.table) > 1024
    assert len(bc.candidates(f.data)) == len(f.table) > 256 * 8  # k_scan_local: SCAN_T x SCAN_PER
    assert {m.usize for m in f.table if not m.empty} == {1, 2, 3}
    c = [c for c in bc.crc_bad() if c.name == "many_same_workgroup"][0]
    assert len(c.bad) >= 2 and min(c.bad) >= 1024 and len({b % 1024 for b in c.bad}) == 1


def test_crc_sizes_reach_every_alignment():
    for kind in bc.PATTERNS:
        files = [f for f in bc.crc_sizes() if "_%s_" % kind in f.name]
        seen, pairs = {}, set()
        for f in files:
            ust = bc.ustarts(f.table)[0]
            for m, meta, u in zip(f.table, f.meta, ust):
                if meta is None:
                    continue
                assert meta[2] == u % 16 and meta[1] == m.usize
                if meta[0] == "size":
                    seen.setdefault(m.usize, set()).add(u % 16)
                if m.usize >= 4:
                    pairs.add((m.usize % 4, u % 16))
        for s in bc.CRC_SMALL:
            assert seen[s] == set(range(16)), (kind, s)
        for s in bc.CRC_LARGE:
            assert seen[s] == set(bc.CRC_LARGE_ALIGN), (kind, s)
        assert pairs == {(r, a) for r in range(4) for a in range(16)}
    # data that begins with zero bytes, and data the pre-inversion alone tells from front padding
    assert bc.pattern("zero5one", 12, 0) == b"\0\0\0\0\0\1" * 2


def test_crc_bad_cases_are_what_they_say():
    cases = bc.crc_bad()
    assert {c.n_bad for c in cases} >= {1, 3, 4, 16, 48}
    for c in cases + (bc.crc_stream_case(),):
        assert c.n_bad == len(c.bad) and c.first_bad == min(c.file.table[i].start for i in c.bad)
    names = {c.name for c in cases}
    assert {"footer_byte%d" % k for k in range(4)} <= names and "empty_mid_crc" in names
    assert {"payload_258_at%s" % o for o in (0, 1, 2, 3, 4, "last")} <= names
