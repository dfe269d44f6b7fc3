"""k_huff's emit pass (emit_asm, inflate.hip): one token per lane and loop iteration -- a length
code and its distance code decoded together -- four iterations to a group, one 16-byte store per
group and lane, and the 1..3 tokens of a lane that leaves inside a group written after the loop.

Members are built token by token (deflate_build.py) or with zlib (`Z_BLOCK` splits, as
test_tail_header_gpu.py does), each at about the smallest size that still takes the lane-parallel
path (usize >= 4096), a few members to a file and one launch.  Every member must inflate to
zlib's bytes with a good CRC, and every one of its blocks must come from the lane-parallel
decoder (sbh_inflate_paths == 0): a wrong token falls back to the serial decoder, which would
give the right bytes all the same."""
import random
import struct
import zlib

import numpy as np
import pytest

from deflate_build import (DIST_EXTRA, EOF_MEMBER, LEN_EXTRA, Bits, canon, dist_code, dynamic_block, expand, fixed_block,
                           kraft, len_code, member_of)
from pkg import sb

pytestmark = pytest.mark.gpu

PAR, SERIAL = 0, 2  # sbh_inflate_paths
HT, MIN_SLICE = 256, 128  # inflate.hip: k_huff lanes per block, least bits per lane

# literals 0..225 at 8 bits, the rest (end-of-block, every length symbol) at 9: no two literals
# fit one 10-bit lookup, so every literal is a token of its own
GEN_LIT = [8] * 226 + [9] * 60
GEN_DIST = [4, 4] + [5] * 28
# literal codes of 1..5 bits ('a'..'e'): any two fit one 10-bit lookup (literal pairs)
PAIR_LIT = [0] * 258
PAIR_LIT[97], PAIR_LIT[98], PAIR_LIT[99], PAIR_LIT[100], PAIR_LIT[101], PAIR_LIT[256], PAIR_LIT[257] = 1, 2, 3, 4, 5, 6, 6
# mixed: 'a'..'m' at 2..6 bits (pairs), eight literals at 8, length symbols 257..260 at 5 and 6,
# end-of-block at 6: lone literals, pairs and matches of many bit lengths
MIX_LIT = [0] * 261
for _s, _l in zip(range(97, 110), (2, 3, 3, 4, 5, 5, 5, 5, 4, 4, 6, 6, 6)):
    MIX_LIT[_s] = _l
for _s in range(48, 56):
    MIX_LIT[_s] = 8
MIX_LIT[256], MIX_LIT[257], MIX_LIT[258], MIX_LIT[259], MIX_LIT[260] = 6, 5, 5, 6, 6
MIX_DIST = [2, 2, 3, 3, 3, 4, 4]  # distances 1..12
assert kraft(PAIR_LIT) == 32768 and kraft(MIX_LIT) == 32768 and kraft(MIX_DIST) == 32768
# long codes: ten short literals ('a'..'j', 1..10 bits) and, at 11..15 bits, two literals, the
# length symbols 257 and 258, end-of-block and a third literal; distance symbols 14..29 on the
# comb 15, 15, 14, .., 1 (symbols 14..19: 11..15 bits)
LONG_LIT = [0] * 259
for _i in range(10):
    LONG_LIT[97 + _i] = _i + 1
LONG_LIT[65], LONG_LIT[66], LONG_LIT[257], LONG_LIT[258], LONG_LIT[256], LONG_LIT[67] = 11, 12, 13, 14, 15, 15
LONG_DIST = [0] * 30
for _i, _l in enumerate(list(range(1, 15)) + [15, 15]):
    LONG_DIST[29 - _i] = _l
assert kraft(LONG_LIT) == 32768 and kraft(LONG_DIST) == 32768


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def run(ctx, members):
    """Inflate the members [(BGZF member, its bytes)] in one file: bytes and CRCs must match, and
    every member's block must have come from the lane-parallel decoder."""
    data = b"".join(m for m, _ in members) + EOF_MEMBER
    want = b"".join(bytes(u) for _, u in members)
    sh = ctx.shard(np.frombuffer(data, dtype=np.uint8).copy())
    try:
        _, flat = sh.index(0)
        sh.inflate()  # (raises unless every block's status is OK)
        got = bytes(sh.read_flat(0, flat))
        paths = [int(p) for p in sh.inflate_paths()]
        bad_crc = sh.verify_crc()[0]
    finally:
        sh.close()
    assert flat == len(want)
    if got != want:  # (name the first member that differs)
        pos = 0
        for i, (_, u) in enumerate(members):
            assert got[pos:pos + len(u)] == bytes(u), "member %d" % i
            pos += len(u)
    assert bad_crc == 0
    # (the EOF member, an empty block, is the serial decoder's)
    assert paths == [PAR] * len(members) + [SERIAL]


def built(blocks):
    """A member of deflate blocks [(lit lens, dist lens, tokens)] (lit lens None: the fixed code),
    checked against zlib; returns (member, bytes, [dynamic_block's positions])."""
    w, toks, info = Bits(), [], []
    for i, (lit, dist, t) in enumerate(blocks):
        final = i == len(blocks) - 1
        if lit is None:
            fixed_block(w, t, final)
            info.append(None)
        else:
            info.append(dynamic_block(w, lit, dist, t, final))
        toks += t
    raw, u = w.bytes(), bytes(expand(toks))
    assert zlib.decompress(raw, -15) == u and len(u) >= 4096
    return member_of(raw, u), u, info, raw


def mixed_tokens(rng, n):
    """n tokens over MIX_LIT / MIX_DIST: about half matches, the literals mostly pairable."""
    toks, out = [97, 98, 99, 100, 48, 49, 50, 51, 101, 102, 103, 104], 12
    while len(toks) < n:
        r = rng.random()
        if r < 0.48:
            ln = rng.choice((3, 4, 5, 6))
            toks.append((ln, 1 + rng.randrange(12 if rng.random() < 0.8 else 4)))
            out += ln
        elif r < 0.9:
            toks.append(97 + rng.randrange(13))
            out += 1
        else:
            toks.append(48 + rng.randrange(8))
            out += 1
    return toks


def test_all_literals(ctx):
    rng = random.Random(1)
    ms = [built([(GEN_LIT, GEN_DIST, [rng.randrange(226) for _ in range(n)])])[:2] for n in (4096, 4097, 4099)]
    run(ctx, ms)


def test_all_matches(ctx):
    # one literal, then nothing but (3, 1): every iteration's every lane takes the distance part
    ms = [built([(GEN_LIT, GEN_DIST, [65] + [(3, 1)] * n)])[:2] for n in (1365, 1366, 1367)]
    run(ctx, ms)


def test_literal_match_alternation(ctx):
    rng = random.Random(2)
    ms = []
    for first in (0, 1):  # a literal first, a match first (after the literals it needs)
        toks = [rng.randrange(226) for _ in range(4 + first)]
        for _ in range(1030):
            toks += [(3, 1 + rng.randrange(4)), rng.randrange(226)]
        ms.append(built([(GEN_LIT, GEN_DIST, toks)])[:2])
    run(ctx, ms)


def test_pair_heavy_literals(ctx):
    rng = random.Random(3)
    ms = []
    for seed in range(3):
        toks = []
        for i in range(420):  # even and odd runs of pairable literals between matches
            toks += [97 + min(4, int(rng.expovariate(0.7))) for _ in range(2 + (i + seed) % 9)] + [(3, 1 + rng.randrange(2))]
        toks += [97] * (1500 + seed) + [100, 101, 99, 101]  # a pair, then a pair before end-of-block
        ms.append(built([(PAIR_LIT, [1, 1], toks)])[:2])
    run(ctx, ms)


def lane_cuts_inside_a_match(info, raw, toks, lit, dist):
    """How many of k_huff's lane cuts (bit p0 + S * i of the stream, p0 the first symbol's bit)
    fall after the start of a match's length code and at or before the start of its distance code."""
    lc, dc = canon((list(lit) + [0] * 288)[:288]), canon((list(dist) + [0] * 32)[:32])
    p0 = info["symbols"]
    S = max((8 * len(raw) - p0) // HT + 1, MIN_SLICE)
    pos, n = p0, 0
    for t in toks:
        if isinstance(t, tuple):
            c, ds = len_code(t[0]), dist_code(t[1])
            dpos = pos + lc[257 + c][1] + LEN_EXTRA[c]
            n += (dpos - p0) // S > (pos - p0) // S  # a cut in (pos, dpos]
            pos = dpos + dc[ds][1] + DIST_EXTRA[ds]
        else:
            pos += lc[t][1]
    return n


def test_every_alignment(ctx):
    # the same tokens behind 0..31 more leading literals: the lanes' cuts and the groups of four
    # land at every alignment of the token sequence
    rng = random.Random(4)
    base = mixed_tokens(rng, 1700)
    lead = [48 + rng.randrange(8) if i % 3 else 97 + rng.randrange(13) for i in range(31)]
    ms, split = [], 0
    for k in range(32):
        toks = lead[:k] + base
        m, u, info, raw = built([(MIX_LIT, MIX_DIST, toks)])
        split += lane_cuts_inside_a_match(info[0], raw, toks, MIX_LIT, MIX_DIST)
        ms.append((m, u))
    # (a length code that is the last code starting before a cut, its distance code past it)
    assert split >= 32
    run(ctx, ms)


def test_long_codes(ctx):
    # literal, length and distance codes of 11..15 bits (resolved through pk / sent), a long
    # distance code directly after a long length code
    rng = random.Random(5)
    ms = []
    for seed in range(2):
        toks = [97 + rng.randrange(10) for _ in range(1100 + seed)]
        out = len(toks)
        while out < 4200:
            r = rng.random()
            if r < 0.45:
                dc, ls = 14 + rng.randrange(6), 257 + rng.randrange(2)  # distance codes of 15, 15, 14, 13, 12, 11 bits
                toks.append(("L", ls, 0, dc, rng.choice((0, (1 << DIST_EXTRA[dc]) - 1))))
                out += ls - 254
            elif r < 0.75:
                toks.append(rng.choice((65, 66, 67)))
                out += 1
            elif r < 0.85:
                toks.append(("L", 257, 0, 20, 0))  # a table-sized distance code after a long length code
                out += 3
            else:
                toks.append(97 + rng.randrange(10))
                out += 1
        ms.append(built([(LONG_LIT, LONG_DIST, toks)])[:2])
    run(ctx, ms)


def test_short_stream_few_lanes(ctx):
    # 4 KB from a few hundred bits: most lanes start at or past the end of the stream
    ms = [built([(GEN_LIT, GEN_DIST, [7 + n] + [(258, 1)] * (16 + n) + [(3, 1)] * n)])[:2] for n in range(4)]
    for m, _ in ms:
        assert 8 * len(m) < HT * MIN_SLICE
    run(ctx, ms)


def test_several_deflate_blocks(ctx):
    # the second (and third) deflate block's tokens start at a token index that is no multiple of
    # four; a fixed-code block after a dynamic one.  Blocks of equal size, so that k_huff itself
    # decodes the later ones
    rng = random.Random(6)
    ms = []
    for n in (701, 702, 703):
        a, b, c = (mixed_tokens(rng, n + i) for i in range(3))
        ms.append(built([(MIX_LIT, MIX_DIST, a), (MIX_LIT, MIX_DIST, b), (MIX_LIT, MIX_DIST, c)])[:2])
    for n in (1101, 1102, 1103):
        a, b = mixed_tokens(rng, n), mixed_tokens(rng, n)
        ms.append(built([(MIX_LIT, MIX_DIST, a), (GEN_LIT, GEN_DIST, b)])[:2])
        ms.append(built([(MIX_LIT, MIX_DIST, a), (None, None, b)])[:2])
    run(ctx, ms)


def zlib_member(parts):
    """A member by zlib (level 6), every part ending its own deflate block (`Z_BLOCK`)."""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = b""
    for i, p in enumerate(parts):
        raw += co.compress(p) + co.flush(zlib.Z_FINISH if i == len(parts) - 1 else zlib.Z_BLOCK)
    u = b"".join(parts)
    assert zlib.decompress(raw, -15) == u
    body = raw + struct.pack("<II", zlib.crc32(u), len(u))
    hdr = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", 18 + len(body) - 1)
    return hdr + body, u


def test_short_tails(ctx):
    # a final deflate block of 1..5 tokens (bytes the first part never has: literals) behind a
    # `Z_BLOCK` split: k_huff_tail's emit leaves inside its first or second group
    ms = []
    for k in (1, 2, 3, 4, 5):
        head = np.random.default_rng(10 + k).integers(0, 128, 4200 + k, dtype=np.uint8).tobytes()
        ms.append(zlib_member([head, bytes(range(200, 200 + k))]))
    run(ctx, ms)
