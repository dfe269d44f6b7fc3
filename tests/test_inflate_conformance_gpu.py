"""Inflate conformance on the GPU: hand-built deflate streams (inflate_corpus.py, written token by
token with deflate_build.py) through shard / index / inflate / read_flat, byte-exact against the
oracle's or_stream_next (StreamI._advance, Stream.scala:31-71) and against expand(), with the
decoder that produced each block (sbh_inflate_paths) asserted: a case written to attack the
lane-parallel k_huff must not quietly run k_huff_serial instead.

test_deflate_build_cpu.py checks the same corpus against zlib and the oracle and asserts the
structural property each case exists for."""
import numpy as np
import pytest

import inflate_corpus as ic
from deflate_build import EOF_MEMBER
from pkg import sb

pytestmark = pytest.mark.gpu

ERR = {ic.SIZE: 13, ic.DATA: 14, ic.BAD_ISIZE: 15}  # SBH_E_INFLATE_SIZE, _DATA, _BAD_ISIZE


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def decode(ctx, data):
    """(None, flat bytes, paths, bad CRCs) or (error code, file offset of the bad block, None, None)."""
    sh = ctx.shard(np.frombuffer(data, dtype=np.uint8).copy())
    try:
        _, flat = sh.index(0)
        sh.inflate()
        return None, bytes(sh.read_flat(0, flat)), sh.inflate_paths(), sh.verify_crc()[0]
    except sb.SparkBamError as e:
        if e.code == 2:  # SBH_E_HIP: a device error -- nothing more runs on this GPU
            pytest.exit("HIP error: %s" % e, returncode=3)
        return e.code, (e.fields[0] if e.fields else None), None, None
    finally:
        sh.close()


def reference(data):
    """The oracle's (None, flat bytes) or (library error code, offset of the first bad member)."""
    outcome, v = ic.oracle_file(data)
    return (None, v) if outcome is None else (ERR[outcome], v)


@pytest.mark.parametrize("c", ic.valid_cases(), ids=lambda c: c.name)
def test_valid(ctx, c):
    data, _, fdata = ic.placed(c)
    data += EOF_MEMBER
    err, flat, paths, bad_crc = decode(ctx, data)
    assert err is None
    assert (None, flat) == reference(data)
    assert flat == fdata + c.expect
    assert bad_crc == 0
    # the filler is one stored block; the EOF member (an empty block) is the serial decoder's
    assert list(paths) == [ic.STORED, c.path, ic.SERIAL]


@pytest.mark.parametrize("c", ic.bad_cases(), ids=lambda c: c.name)
def test_invalid(ctx, c):
    data, at, _ = ic.placed(c)
    data += EOF_MEMBER
    want = reference(data)
    assert want[0] == ERR[c.outcome] and want[1] == at
    err, where, _, _ = decode(ctx, data)
    assert err == want[0]
    if c.outcome != ic.BAD_ISIZE:  # (that error carries no fields)
        assert where == at
    # between two sound members: the first bad block in file order decides
    g1, g2 = ic.good_member(1)[0], ic.good_member(2)[0]
    mid, at, _ = ic.placed(c, len(g1))
    data = g1 + mid + g2 + EOF_MEMBER
    want = reference(data)
    assert want == (ERR[c.outcome], at)
    err, where, _, _ = decode(ctx, data)
    assert err == want[0]
    if c.outcome != ic.BAD_ISIZE:
        assert where == at


def test_two_bad_members_first_in_file_order(ctx):
    by = {c.name: c for c in ic.bad_cases()}
    a, b = by["fixed_distance_30_deep"], by["one_byte_short_of_isize"]
    for x, y in ((a, b), (b, a)):
        g = ic.good_member(3)[0]
        px, at, _ = ic.placed(x, len(g))
        py, _, _ = ic.placed(y, len(g) + len(px))
        data = g + px + py + EOF_MEMBER
        assert reference(data) == (ERR[x.outcome], at)
        err, where, _, _ = decode(ctx, data)
        assert (err, where) == (ERR[x.outcome], at)


def test_combined_file(ctx):
    # every valid member in one shard and one launch: a header record left by one block must
    # never serve another
    parts, flat, paths, at = [], [], [], 0
    for c in ic.valid_cases():
        d, _, fdata = ic.placed(c, at)
        parts.append(d)
        at += len(d)
        flat += [fdata, c.expect]
        paths += [ic.STORED, c.path]
    data = b"".join(parts) + EOF_MEMBER
    err, got, got_paths, bad_crc = decode(ctx, data)
    assert err is None and bad_crc == 0
    want = b"".join(flat)
    assert len(got) == len(want)
    if got != want:  # (name the first member that differs)
        pos = 0
        for c, f in zip([x for c in ic.valid_cases() for x in (c.name + ":filler", c.name)], flat):
            assert got[pos:pos + len(f)] == f, c
            pos += len(f)
    assert (None, got) == reference(data)
    wrong = [(c.name, int(p)) for c, p in zip(ic.valid_cases(), got_paths[1::2]) if p != c.path]
    assert not wrong
    assert list(got_paths) == paths + [ic.SERIAL]


def test_inflate_paths_needs_an_inflate(ctx):
    c = ic.valid_cases()[0]
    sh = ctx.shard(np.frombuffer(ic.placed(c)[0] + EOF_MEMBER, dtype=np.uint8).copy())
    try:
        sh.index(0)
        with pytest.raises(sb.SparkBamError) as e:
            sh.inflate_paths()
        assert e.value.code == 18  # SBH_E_STATE
        before = sh.blocks()
        sh.inflate()
        assert sh.inflate_paths().dtype == np.uint8
        assert sh.blocks() == before  # the host block table is as it was
    finally:
        sh.close()
