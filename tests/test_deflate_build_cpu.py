"""The inflate conformance corpus on the CPU: every case test_inflate_conformance_gpu.py decodes is
built here and checked against zlib, against the oracle's or_stream_next (StreamI._advance,
oracle/sbam_oracle.c) and for the structural property it exists for, so a mistake in a generator
shows before a GPU is involved."""
import zlib

import pytest

import deflate_build as db
import inflate_corpus as ic

oracle_member, oracle_file = ic.oracle_member, ic.oracle_file

ALL = ic.valid_cases() + ic.bad_cases()


def test_corpus_covers_the_issue():
    names = {c.name for c in ALL}
    assert len(ic.valid_cases()) >= 80 and len(ic.bad_cases()) >= 50
    assert sum(c.path == ic.PAR for c in ic.valid_cases()) >= 70
    assert {"isize_65537", "one_byte_short_of_isize", "block_type_3_first", "fixed_symbol_287_deep"} <= names


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_case(c):
    assert c.prop[1], c.prop[0]
    assert c.raw is not None and 18 + len(c.raw) + 8 <= 65536
    if c.outcome == ic.OK:
        assert zlib.decompress(c.raw, -15) == c.full
        assert c.expect == c.full[:c.isize] and zlib.crc32(c.expect) == c.crc
        if c.path == ic.PAR:
            assert c.isize >= ic.PAR_MIN_USIZE
    elif c.outcome == ic.DATA:
        with pytest.raises(zlib.error):
            zlib.decompress(c.raw, -15)
    data, at, fdata = ic.placed(c)
    assert (at + 18) % 4 == c.phase
    assert oracle_member(data, 0) == (ic.OK, fdata)  # the filler
    outcome, got = oracle_member(data + db.EOF_MEMBER, at)
    assert outcome == c.outcome
    assert got == c.expect


def test_writer_matches_zlib_on_its_own_output():
    # the builder's fixed and dynamic blocks, stored blocks and alignment against zlib's inflate
    toks = [1, 2, 3, (3, 3), 200, 255, (258, 1), (10, 7)]
    w = db.Bits()
    db.fixed_block(w, toks, False)
    db.stored_block(w, b"stored", False)
    db.dynamic_block(w, ic.GEN_LIT, ic.GEN_DIST, toks, True)
    want = bytes(db.expand(toks)) + b"stored"
    want += bytes(db.expand(toks, bytearray(want))[len(want):])
    assert zlib.decompress(w.bytes(), -15) == want
    assert db.kraft(db.FIXED_LIT_LENS) == 32768 and db.kraft(ic.GEN_LIT) == db.kraft(ic.GEN_DIST) == 32768


def test_place_sets_the_phase():
    m = db.member_of(zlib.compress(b"x" * 100, 6)[2:-4], b"x" * 100)
    for at in range(4):
        for phase in range(4):
            f = db.place([m], phase, at)
            assert (at + len(f) - len(m) + 18) % 4 == phase
            assert oracle_file(b"\0" * 0 + f + db.EOF_MEMBER)[0] is None
