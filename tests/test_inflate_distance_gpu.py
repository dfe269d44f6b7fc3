"""Distances at and past the bytes before their match (zlib's "invalid distance too far back",
java.util.zip.DataFormatException at Stream.scala:49-51): a BGZF member whose deflate stream
(fixed Huffman codes, written here token by token) carries a match reaching exactly to the
member's first byte inflates to zlib's bytes; one byte further is SBH_E_INFLATE_DATA, as zlib
fails it -- in a member's first deflate block (k_huff's lane-parallel passes), in a short final
deflate block (k_huff_tail), and in the second member of a file whose first is sound.  The
lane-parallel passes leave that test to k_lz, which sees every match token once."""
import zlib

import numpy as np
import pytest

from deflate_build import EOF_MEMBER, expand
from deflate_build import fixed_member as member
from pkg import sb

pytestmark = pytest.mark.gpu

SBH_E_INFLATE_DATA = 14


def literals(n, seed):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(0, 256, n)]


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def inflate(ctx, data):
    """(None, bytes) or (error code, None)."""
    sh = ctx.shard(np.frombuffer(data, dtype=np.uint8).copy())
    try:
        _, flat = sh.index(0)
        sh.inflate()
        return None, bytes(sh.read_flat(0, flat))
    except sb.SparkBamError as e:
        return e.code, None
    finally:
        sh.close()


def zlib_outcome(raws):
    try:
        return None, b"".join(zlib.decompress(r, -15) for r in raws)
    except zlib.error:
        return SBH_E_INFLATE_DATA, None


@pytest.mark.parametrize("at", [0, 3000, 5990])
@pytest.mark.parametrize("extra", [0, 1, 700])
def test_first_deflate_block(ctx, at, extra):
    # `at` literals, a match whose distance is the bytes before it plus `extra`, then literals to
    # 6000+ bytes: the lane-parallel path (usize >= 4096, staged)
    lead = literals(max(at, 1), 1)
    toks = lead + [(40, len(lead) + extra)] + literals(6000 - len(lead), 2)
    data, raw, u = member([toks], 6040)
    got = inflate(ctx, data + EOF_MEMBER)
    want = zlib_outcome([raw])
    assert got == want
    assert (got[0] is None) == (extra == 0) and (u is None) == (extra > 0)


@pytest.mark.parametrize("extra", [0, 1])
def test_short_final_block(ctx, extra):
    # a long first deflate block and a short last one (k_huff_tail's) whose match reaches to the
    # member's first byte, or one past it
    b1 = literals(7000, 3)
    b2 = literals(300, 4) + [(10, 7300 + extra)] + literals(50, 5)
    data, raw, u = member([b1, b2], 7360)
    got = inflate(ctx, data + EOF_MEMBER)
    assert got == zlib_outcome([raw])
    assert (got[0] is None) == (extra == 0)


def test_second_member(ctx):
    good, raw1, _ = member([literals(6000, 6) + [(100, 6000)]], 6100)
    bad, raw2, _ = member([literals(5000, 7) + [(20, 5001)] + literals(1000, 8)], 6020)
    got = inflate(ctx, good + bad + EOF_MEMBER)
    assert got == (SBH_E_INFLATE_DATA, None) == zlib_outcome([raw1, raw2])
    got = inflate(ctx, good + good + EOF_MEMBER)
    assert got[0] is None and got[1] == zlib.decompress(raw1, -15) * 2


@pytest.mark.parametrize("at,extra", [(3000, 0), (3000, 1), (3000, 20000), (10, 32768 - 10)])
def test_long_far_match(ctx, at, extra):
    # a 258-byte match (k_lz marks it with a start every 32 bytes) reaching exactly to the first
    # byte, one byte past it, far past it, and distance 32768 at a small offset
    lead = literals(at, 9)
    toks = lead + [(258, len(lead) + extra)] + literals(6000, 10)
    data, raw, u = member([toks], at + 6258)
    got = inflate(ctx, data + EOF_MEMBER)
    assert got == zlib_outcome([raw])
    assert (got[0] is None) == (extra == 0)


@pytest.mark.parametrize("extra", [0, 1, 5000])
def test_far_match_after_carried_cut(ctx, extra):
    # long matches fill k_lz's 6656-byte pointer pass before the chunk's 1536 tokens are used up,
    # so the chunk is cut and carried; the (far) match comes after several such cuts
    lead = literals(400, 11)
    toks = list(lead)
    for i in range(60):  # ~15 KB of 258-byte matches (several passes' worth), literals between
        toks += [(258, 300 + i)] + literals(3, 100 + i)
    n = len(expand(toks))
    toks += [(100, n + extra)] + literals(4000, 12)
    data, raw, u = member([toks], n + 4100)
    got = inflate(ctx, data + EOF_MEMBER)
    assert got == zlib_outcome([raw])
    assert (got[0] is None) == (extra == 0)
