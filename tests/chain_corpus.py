"""Hand-built record chains for the kernels that consume the eager bitmap (test infrastructure;
plain Python and numpy, no GPU): the chain proof (k_verify_chain_w), the first-record search
(k_first_set), the chain marker (k_cm_*), the exact walk (k_chain_walk) and the split counters
(k_split_popcount / k_split_count_cc / k_split_cm_count).

A layout names the flat positions of its set bits directly: `land_at(p)` appends one filler
record so that the next record starts at flat p, and a "bait" run lays minimal records into a big
record's payload, where the eager checker accepts them (false positives) although the chain never
visits them.  Every layout returns its flat bytes, the set bits it declares at its readsToCheck
and the chain it declares; test_chain_corpus_cpu.py holds the declarations to the CPU oracle and
asserts the geometry each layout is there for, so an edit that loses an edge fails there.

The expected value everywhere is `walk()`: the PosStream loop (next = s + 4 + int32 at s), which
shares nothing with check.hip.

Grid (positions of a bitmap whose `begin` is 0; a call's `begin` shifts all of it):
  W = 32    a bitmap word
  L = 128   a lane of the proof (4 words)
  C = 8192  a wave chunk of the proof (VC_CHUNK words): also the unit of the chunk counts
  G = 32768 a workgroup trip of the proof (4 waves), and one k_first_set span (FS_SPAN words)
  P = 512   a prefix group of the chain marker (WPRE_GROUP words), counted from the word of `from`
"""
import bisect
import functools
import struct
import zlib
from collections import namedtuple

import numpy as np

from checker_corpus import FILL, MIN, SMALL, raw
from deflate_build import EOF_MEMBER, member_of

# copies of the kernels' constants (test_chain_corpus_cpu.py holds them to the sources)
VC_CHUNK, WPRE_GROUP, FS_SPAN, CM_PEEL_MAX, PC_WORDS = 256, 16, 1024, 4096, 8192
PROOF_GRID, PROOF_WG_WORDS, FS_GRID = 2048, 1024, 256     # launch_verify_chain_count / launch_first_set
W, L, C, G, P = 32, 4 * 32, VC_CHUNK * 32, FS_SPAN * 32, WPRE_GROUP * 32
WAVE = 64
assert (L * WAVE, PROOF_WG_WORDS * 32) == (C, G)

CONTIGS = SMALL
REC = len(MIN)                  # 38
# a minimal record without an 0xFF byte and with no byte whose low nibble is above 8: it passes
# the eager checker wherever it lies, a CIGAR of another record included
ZMIN = raw(ref=0, pos=0, nref=0, npos=0)
assert len(ZMIN) == REC and all(b & 15 <= 8 for b in ZMIN)


def header(first=None):
    """The BAM header over CONTIGS; `first`: the text is padded with NULs so that the header ends
    (and the first record starts) at exactly that flat position."""
    refs = b"".join(struct.pack("<i", 2) + b"%x\0" % i + struct.pack("<i", ln) for i, ln in enumerate(CONTIGS))
    bare = 12 + len(refs)
    text = 0 if first is None else first - bare
    assert text >= 0
    return b"BAM\1" + struct.pack("<i", text) + b"\0" * text + struct.pack("<i", len(CONTIGS)) + refs


HEADER_LEN = len(header())
assert HEADER_LEN == 42


def rec_of_size(n, fill=FILL):
    """A record of exactly n >= 38 bytes: MIN's 38 checked bytes, then filler."""
    assert n >= REC
    r = raw(extra=bytes([fill]) * (n - REC))
    assert len(r) == n and struct.unpack_from("<i", r)[0] == n - 4
    return r


# ------------------------------------------------------------------------------ the restatement
def walk(flat, first, E):
    """(count, exit) of the PosStream chain from `first` over records whose start is < E."""
    out = starts(flat, first, E)
    return len(out), min(out[-1] + 4 + struct.unpack_from("<i", flat, out[-1])[0], len(flat)) if out else first


def starts(flat, first, E):
    """The record starts of that chain.  (A step that does not move forward is a malformed stream,
    where the reference throws: no case of this corpus walks into one.)"""
    out, total = [], len(flat)
    s = first
    while s < E and s + 4 <= total:
        out.append(s)
        step = 4 + struct.unpack_from("<i", flat, s)[0]
        assert step > 0, (first, s, step)
        s += step
    return out


# ------------------------------------------------------------------------------ the builder
Lay = namedtuple("Lay", "flat bits chain name rtc clean marks")
# flat: bytes; bits: sorted flat positions of the declared set bits at readsToCheck `rtc`; chain:
# the record starts from the header's end; clean: the bitmap is exactly the chain (the proof
# answers, no anomaly); marks: name -> position(s) the layout is about.


class Stream:
    """Records appended one after another; every candidate start (chain records and bait) is kept
    with whether the eager checker passes the record there and where its header points."""

    def __init__(self, first=None):
        self.out = bytearray(header(first))
        self.chain, self.cand, self.marks = [], {}, {}

    @property
    def pos(self):
        return len(self.out)

    def rec(self, data=MIN, ok=True):
        s = self.pos
        self.chain.append(s)
        self.cand[s] = (ok, s + 4 + struct.unpack_from("<i", data)[0])
        self.out += data
        return s

    def land_at(self, p):
        """One filler record so that the next record starts at flat p."""
        self.rec(rec_of_size(p - self.pos))
        assert self.pos == p

    def at(self, p, data=MIN, ok=True):
        self.land_at(p)
        return self.rec(data, ok)

    def run(self, n, data=MIN):
        return [self.rec(data) for _ in range(n)]

    def until(self, p, data=MIN):
        """Minimal records while they end at or before p."""
        while self.pos + len(data) <= p:
            self.rec(data)

    def host(self, m, pre=2, post=4, last=MIN, at=None):
        """A big record whose payload holds a bait run: `pre` filler bytes, m minimal records (the
        last one `last`), `post` filler bytes.  post 0: the run ends exactly on the record's end,
        so the bait chain joins the real one.  Returns (host start, bait starts)."""
        if at is not None:
            self.land_at(at)
        body = bytes([FILL]) * pre + MIN * (m - 1) + last + bytes([FILL]) * post
        s = self.rec(raw(extra=body))
        b0 = s + REC + pre
        bait = [b0 + REC * j for j in range(m - 1)] + [b0 + REC * (m - 1)]
        for k, b in enumerate(bait):
            self.cand[b] = (True, b + (REC if k < m - 1 else len(last)))
        assert self.pos == bait[-1] + len(last) + post
        return s, bait

    def done(self, name, rtc=10):
        flat, total = bytes(self.out), len(self.out)
        bits = []
        for p in sorted(self.cand):             # eager/Checker.scala:24-126 over the declared structure
            n, cur = 0, p
            while True:
                if n == rtc:
                    ok = True
                elif cur + 36 > total:          # (the stream ends: Success only at a nominal start, n > 0)
                    ok = cur == total and n > 0
                elif cur not in self.cand or not self.cand[cur][0]:
                    ok = False
                else:
                    n, cur = n + 1, self.cand[cur][1]
                    continue
                break
            if ok:
                bits.append(p)
        chain = tuple(self.chain)
        return Lay(flat, tuple(bits), chain, name, rtc, tuple(bits) == chain, dict(self.marks))


# ------------------------------------------------------------------------------ the hand-worked case
def hand_worked():
    """42-byte header; MIN at 42 and 80; at 118 a 158-byte record whose payload is 2 filler bytes,
    three MIN (158, 196, 234) and 4 filler bytes; MIN at 276, 314, 352; the stream ends at 390.
    At readsToCheck 2 the bait at 158 and 196 passes (two records each), 234 does not (its chain
    reads filler at 272)."""
    s = Stream()
    s.run(2)
    s.host(3)
    s.run(3)
    return s.done("hand_worked", rtc=2)


HAND_BITS = (42, 80, 118, 158, 196, 276, 314, 352)
HAND_CHAIN = (42, 80, 118, 276, 314, 352)
HAND_TOTAL = 390
# (first, E): (count, exit).  300 lies in word 9 (288..319) between the set bits 276 (word 8) and 314
HAND_CASES = {
    (42, 390): (6, 390), (42, 300): (4, 314), (42, 314): (4, 314), (42, 315): (5, 352), (80, 277): (3, 314),
    (118, 119): (1, 276), (118, 276): (1, 276), (276, 1000): (3, 390), (352, 390): (1, 390), (42, 42): (0, 42),
    (158, 272): (3, 272), (196, 235): (2, 272),  # from the bait, up to the filler its chain lands on
}


# ------------------------------------------------------------------------------ clean layouts
def dense():
    s = Stream()
    s.until(HEADER_LEN + 3 * C + 2 * L)
    s.marks["span"] = (HEADER_LEN, s.pos)
    return s.done("dense")


def word_edges():
    """Set bits on bit 0 and bit 31 of a word, and on both sides of a lane, P-group, chunk and
    workgroup boundary B: one record at B - 1 (the next at B + 37), and further on one at B - 38
    and one at B."""
    s = Stream()
    s.run(3)
    below, at = [], []
    # (B - 1 is bit 31 of a word -- and of a lane / group / chunk / workgroup; B is bit 0)
    for B, kind in ((W * 13, "below"), (W * 21, "at"), (L * 7, "below"), (L * 9, "at"), (P * 3, "below"),
                    (P * 5, "at"), (C, "below"), (C + L * 63, "at"), (2 * C, "at"), (3 * C, "below"), (G, "below"),
                    (G + P * 7, "at"), (G + C, "at"), (2 * G, "at"), (2 * G + C, "below")):
        if kind == "below":
            below.append(s.at(B - 1))
            s.rec()
            assert s.chain[-2:] == [B - 1, B + REC - 1]
        else:
            s.at(B - REC)
            at.append(s.rec())
            assert s.chain[-2:] == [B - REC, B]
    s.run(12)
    s.marks.update(below=tuple(below), at=tuple(at))
    return s.done("word_edges")


def empty_lanes():
    """Records of L + 1, 2 L and 5 L bytes (the successor comes from a later lane), a wave chunk whose
    only set bit lies in lane 0 and one whose only set bit lies in lane 63."""
    s = Stream()
    s.run(2)
    for n in (L + 1, 2 * L, 5 * L, L + 1, L + 1, 2 * L, 5 * L + 3):
        s.rec(rec_of_size(n))
    a = s.at(2 * C + 5, rec_of_size(C + 63 * L + 7 - 5))            # chunk 2: lane 0 only
    b = s.rec(rec_of_size(C - 63 * L - 7 + 40))                     # chunk 3: lane 63 only
    assert (a, b) == (2 * C + 5, 3 * C + 63 * L + 7)
    c = s.rec(rec_of_size(L + 1))                                   # chunk 4, from position 40
    for n in (2 * L, L + 1, 5 * L):
        s.rec(rec_of_size(n))
    s.run(11)
    s.marks.update(lane0=a, lane63=b, after=c)
    return s.done("empty_lanes")


def empty_waves():
    """Records of C + 1, 2 C + 7 and 3 C + 1 bytes: the scan past the wave crosses 0, 1 and 2 whole
    empty chunks; a long record that ends on the first position of a chunk."""
    s = Stream()
    s.run(2)
    m = {}
    m["c1"] = s.at(C - 50, rec_of_size(C + 1))                      # chunk 0 -> chunk 1 (next chunk: none empty)
    m["c2"] = s.rec(rec_of_size(2 * C + 7))                         # chunk 1 -> chunk 3 (chunk 2 empty)
    m["c3"] = s.rec(rec_of_size(3 * C + 1))                         # chunk 3 -> chunk 6 (4 and 5 empty)
    m["to_chunk_start"] = s.rec(rec_of_size(10 * C - s.pos))        # chunk 6 -> the first position of chunk 10
    m["chunk_start"] = s.rec()
    assert m["chunk_start"] == 10 * C
    m["c3b"] = s.rec(rec_of_size(3 * C + 1))                        # chunk 10 -> 13: and nothing but it in chunk 10
    s.run(11)
    s.marks.update(m)
    return s.done("empty_waves")


TAILS = (0, 1, 2, 3, 4, 5, 37)


@functools.lru_cache(maxsize=None)
def tail(k, boundary=None):
    """The stream ends k bytes after the start of a last, cut record (readsToCheck 1: every whole
    record before it is a set bit whatever follows).  boundary: the stream's length."""
    s = Stream()
    s.run(4)
    if boundary is not None:
        s.land_at(boundary - k - 2 * REC)
        s.run(2)
    s.marks["cut"] = s.pos
    if k >= 4:
        s.chain.append(s.pos)                   # (its length field is there: the walk counts it)
    s.out += rec_of_size(64)[:k]
    lay = s.done(f"tail_{k}" + ("" if boundary is None else f"_{boundary}"), rtc=1)
    assert boundary is None or len(lay.flat) == boundary
    return lay


def tail_overhang(boundary=None):
    """A last record that is whole as far as the checker reads (38 bytes) and whose nominal end lies
    100 bytes past the stream's end."""
    s = Stream()
    s.run(4)
    if boundary is not None:
        s.land_at(boundary - 2 * REC)
        s.rec()
    s.marks["last"] = s.rec(raw(bs=34 + 100))
    lay = s.done("tail_overhang" + ("" if boundary is None else f"_{boundary}"), rtc=1)
    assert boundary is None or len(lay.flat) == boundary
    return lay


# ------------------------------------------------------------------------------ bait layouts
def bait_dead_end(rtc):
    """Bait runs that end in filler: the false positives' chain lands on a clear bit."""
    s = Stream()
    s.run(3)
    _, b1 = s.host(rtc + 3)
    s.run(2)
    _, b2 = s.host(2 * rtc + 1, at=C - 3 * REC - 7)                 # a run that crosses the first chunk edge
    s.run(14)
    s.marks.update(bait=tuple(b1 + b2))
    return s.done(f"bait_dead_end_{rtc}", rtc=rtc)


def bait_joins():
    """A bait run that ends exactly on the enclosing record's end: its chain steps onto a real
    record, which then has two predecessors."""
    s = Stream()
    s.run(3)
    h, b = s.host(6, post=0)
    s.marks.update(host=h, bait=tuple(b), joined=s.pos)
    s.run(5)
    h2, b2 = s.host(40, post=0, at=C + 17)                           # a second, longer one past the chunk edge
    s.marks.update(host2=h2, bait2=tuple(b2), joined2=s.pos)
    s.run(30)
    return s.done("bait_joins")


def bait_leaves_E():
    """A bait run whose last record is 600 bytes long and ends on the enclosing record's end: for an
    E inside that last record the bait's chain leaves [first, E) -- an off-chain node whose
    successor is terminal -- and for the stream's end it joins."""
    s = Stream()
    s.run(3)
    h, b = s.host(5, post=0, last=rec_of_size(600))
    s.marks.update(host=h, bait=tuple(b), E=(b[-1] + 1, b[-1] + 300, s.pos - 1, s.pos))
    s.run(12)
    return s.done("bait_leaves_E")


def bait_leaves_total():
    """The same with the stream's end for E (readsToCheck 1, where a record is a set bit whatever
    follows it): the last bait's header points 5000 bytes on, past the stream's end."""
    s = Stream()
    s.run(3)
    h, b = s.host(4, post=6, last=raw(bs=34 + 5000))
    s.marks.update(host=h, bait=tuple(b))
    s.run(12)
    assert b[-1] + 5038 > s.pos
    return s.done("bait_leaves_total", rtc=1)


def bait_long():
    """A bait run of CM_PEEL_MAX + 5 set bits (the peel gives up, the exact walk decides), one of
    CM_PEEL_MAX - 1 (the peel stays under its limit) and one of CM_PEEL_MAX + 1 (a root and exactly
    CM_PEEL_MAX steps: the most the peel takes)."""
    s = Stream()
    s.run(3)
    _, b1 = s.host(CM_PEEL_MAX + 5 + 9)            # (the last 9 of a dead-end run are clear at readsToCheck 10)
    s.run(4)
    s.marks["between"] = s.pos
    _, b2 = s.host(CM_PEEL_MAX - 1 + 9)
    s.run(4)
    s.marks["between2"] = s.pos
    _, b3 = s.host(CM_PEEL_MAX + 1 + 9)
    s.run(12)
    s.marks.update(over=tuple(b1[:-9]), under=tuple(b2[:-9]), most=tuple(b3[:-9]))
    return s.done("bait_long")


def overlap_after(ops=40):
    """A chain record r with a false positive at r + 16 (readsToCheck 2).  r is mapped (flag 0), l_seq 1,
    `ops` CIGAR ops, name 'UUUU\\0'; read from r + 16 the fields are block_size = ops, refID 1, pos -1,
    l_read_name 2, flag 4 (r's tlen), l_seq 0x55555555 (the name: the implied size wraps negative),
    mate 0 / 0 (the NUL and r's first two ops, all zero), name 'A\\0' (r's ops 2 and 3); its chain
    steps to r + 20 + ops, a ZMIN inside r's CIGAR."""
    assert ops >= 40
    cig = [0, 0, 0x41000000, 0] + [0] * (ops - 4)
    body = bytearray(b"".join(struct.pack("<I", o) for o in cig))
    q = 20 + ops - 41                               # r + 20 + ops, relative to the first op (r + 41)
    body[q:q + REC] = ZMIN
    assert q + REC <= len(body) and all(body[k] & 15 <= 8 for k in range(0, len(body), 4))
    r = raw(ref=-1, pos=-1, flag=0, lseq=1, nref=-1, npos=2, tlen=0x00040000, name=b"UUUU\0", nc=ops,
            ops=(), extra=bytes(body) + b"\x10\x20")
    return r, 16, 20 + ops


def overlap_before(B=132):
    """A chain record r' with a false positive 16 bytes BEFORE it (readsToCheck 2), in the payload of
    the record before.  r' is unmapped, block_size B, l_seq 0x41, mate 0 / 0; read from r' - 16 the
    fields are refID 0, pos 0, l_read_name 2 (the 16 bytes before r'), n_cigar B / flag 0 (r's
    block_size), l_seq -1 (r's refID), mate -1 / 2, name 'A\\0' (r's l_seq), B ops over r' and what
    follows (ZMIN records: no low nibble above 8).  Returns (the 16 bytes, r', records that follow,
    where the false positive's chain lands relative to r')."""
    rp = raw(bs=B, lseq=0x41, nref=0, npos=0, extra=b"\0" * (B - 34))
    assert len(rp) == B + 4
    need = 22 + 4 * B                               # its ops end here (relative to r')
    k = -(-(need - len(rp)) // REC)                 # ZMIN records behind r' that its ops and its chain need
    land = len(rp) + REC * k
    bs = land + 16 - 4
    assert bs >= 32 + 2 + 4 * B - 1
    pre = struct.pack("<iiiI", bs, 0, 0, 2)
    return pre, rp, k, land


def bait_first_word():
    """False positives in the same bitmap word as a chain record, after it and before it
    (readsToCheck 2), and plain bait further on so that the marker's prefix groups are all met."""
    s = Stream()
    s.run(3)
    r, d, nxt = overlap_after()
    a = s.at(20 * W + 3, r)                                          # bits 3 and 19 of word 20
    s.cand[a + d] = (True, a + nxt)
    s.cand[a + nxt] = (True, a + nxt + REC)
    s.run(4)
    pre, rp, k, land = overlap_before()
    b = 40 * W + 20                                                  # r' on bit 20, the false positive on bit 4
    s.land_at(b - 76)
    s.rec(raw(extra=bytes([FILL]) * 22 + pre))                       # 38 + 22 + 16 bytes
    assert s.pos == b
    s.rec(rp)
    s.cand[b - 16] = (True, b + land)
    s.run(k + 4, ZMIN)
    _, bait = s.host(5)
    s.run(30)
    s.marks.update(after=(a, a + d), before=(b - 16, b), bait=tuple(bait))
    return s.done("bait_first_word", rtc=2)


def short_step():
    """Three set bits in one bitmap word (readsToCheck 1): a false positive on bit 0, a chain record A
    on bit 20 and A's own successor B on bit 28 -- the one way a chain steps inside the word of
    `from`.  A: block_size 4, refID -1, pos 300, l_read_name 2, 65 ops, flag 4, l_seq -194 (implied
    32 + 2 + 260 - 96 - 194 = 4), mate 1 / 1, tlen -1, name 'A\0'.  Read from A + 8: block_size 300
    (A's pos), refID 2 (A's l_read_name word), pos 0x40041, l_read_name 0x3E (A's l_seq), one op /
    flag 0 (A's mate refID), l_seq 1, mate -1 / 0x41, a name of 61 'A' at A + 44, the op, one base:
    implied 100.  A's 65 ops lie over B's name and payload (no low nibble above 8).  Read from
    A - 20 (the end of the payload before A): block_size 40, 0 / 0, l_read_name 2, flag 4, l_seq 4
    (A's block_size), mate -1 / 300, name 'A\0' (A's n_cigar).  A dead-end bait run further on keeps
    the bitmap from being the chain, so that the marker runs."""
    s = Stream()
    s.run(3)
    A = 30 * W + 20
    s.land_at(A - 64)
    s.rec(raw(extra=bytes([FILL]) * 6 + struct.pack("<iiiII", 40, 0, 0, 2, 4 << 16)))
    assert s.pos == A
    a = raw(bs=4, ref=-1, pos=300, nc=0x41, flag=4, lseq=-194, nref=1, npos=1, tlen=-1)
    assert len(a) == REC
    b = b"\0\0" + struct.pack("<i", 0) + b"A" * 61 + b"\0" + struct.pack("<I", 0x10) + b"\x10\x20"
    b += b"\0" * (312 - REC - len(b))
    s.out += a + b
    s.chain += [A, A + 8]
    s.cand.update({A - 20: (True, A + 24), A: (True, A + 8), A + 8: (True, A + 312)})
    assert s.pos == A + 312 and all((a + b)[k] & 15 <= 8 for k in range(REC, REC + 260, 4))
    s.run(4)
    _, bait = s.host(3)
    s.run(12)
    s.marks.update(word=(A - 20, A, A + 8), bait=tuple(bait))
    return s.done("short_step", rtc=1)


def rejected():
    """Chain records the eager checker rejects (a name byte '@') with a valid length, at readsToCheck 1:
    first in the stream, in the middle (twice: one alone, two in a row) and last."""
    bad = raw(name=b"@\0")
    assert len(bad) == REC
    s = Stream()
    m = {"first": s.rec(bad, ok=False)}
    s.run(6)
    m["middle"] = s.rec(bad, ok=False)
    s.run(5)
    m["pair"] = (s.at(C - 5, bad, ok=False), s.rec(bad, ok=False))
    s.run(7)
    m["last"] = s.rec(bad, ok=False)
    s.marks.update(m)
    return s.done("rejected", rtc=1)


# ------------------------------------------------------------------------------ the large one
GRID_REC = 65000
GRID_FIRST = FS_GRID * G + 5 * W + 3            # past every k_first_set workgroup's first span
GRID_N = PROOF_GRID * G // GRID_REC + 4         # more positions than one trip of the proof's grid covers


@functools.lru_cache(maxsize=1)
def grid_wrap():
    """A header of GRID_FIRST bytes (k_first_set's grid of 256 workgroups takes a second trip
    before it meets a bit), then GRID_N records of 65000 bytes: more than 2048 x 1024 bitmap words
    from the first record's chunk on, so the proof's grid-stride loop takes a second trip."""
    one = np.frombuffer(rec_of_size(GRID_REC, 0), np.uint8)
    flat = np.concatenate([np.frombuffer(header(GRID_FIRST), np.uint8), np.tile(one, GRID_N)]).tobytes()
    chain = tuple(GRID_FIRST + GRID_REC * i for i in range(GRID_N))
    assert len(flat) == GRID_FIRST + GRID_REC * GRID_N
    assert (len(flat) - GRID_FIRST // C * C + 31) // 32 > PROOF_GRID * PROOF_WG_WORDS
    return Lay(flat, chain, chain, "grid_wrap", 10, True, {})


def grid_wrap_prefix():
    """The same header and three of the records (what the CPU test holds to the oracle)."""
    flat = header(GRID_FIRST) + rec_of_size(GRID_REC, 0) * 3
    chain = tuple(GRID_FIRST + GRID_REC * i for i in range(3))
    return Lay(flat, chain, chain, "grid_wrap_prefix", 10, True, {})


def dense_edges():
    """Minimal records back to back over 9 G (more than PC_WORDS bitmap words), with a record on the
    last position of chunks 0, 2 and 4 and on the first position of chunks 2, 4 and 6: where the
    split counters' ranges begin and end."""
    s = Stream()
    m = {"below": [], "at": []}
    for k in (1, 3, 5):
        s.until(k * C - 1 - REC)
        m["below"].append(s.at(k * C - 1))
        s.until((k + 1) * C - 2 * REC)
        s.at((k + 1) * C - REC)
        m["at"].append(s.rec())
    s.until(9 * G)
    s.marks.update({k: tuple(v) for k, v in m.items()})
    return s.done("dense_edges")


def first_at(p):
    """A header that puts the first record at flat p, then minimal records over two chunks."""
    s = Stream(first=p)
    s.until(p + 2 * C)
    return s.done(f"first_at_{p}")


FIRST_AT = (G - 1, G, G + 1, 2 * G)

LAYOUTS = {
    "dense": dense, "dense_edges": dense_edges, "word_edges": word_edges, "empty_lanes": empty_lanes, "empty_waves": empty_waves,
    "tail_overhang": tail_overhang, "tail_overhang_on_word": functools.partial(tail_overhang, 40 * W),
    "tail_overhang_past_word": functools.partial(tail_overhang, 40 * W + 1),
    "bait_dead_end_2": functools.partial(bait_dead_end, 2), "bait_dead_end_10": functools.partial(bait_dead_end, 10),
    "bait_joins": bait_joins, "bait_leaves_E": bait_leaves_E, "bait_leaves_total": bait_leaves_total,
    "bait_long": bait_long,
    "bait_first_word": bait_first_word, "short_step": short_step, "rejected": rejected, "hand_worked": hand_worked,
}
for _k in TAILS:
    LAYOUTS[f"tail_{_k}"] = functools.partial(tail, _k)
LAYOUTS["tail_0_on_word"] = functools.partial(tail, 0, 40 * W)
LAYOUTS["tail_0_past_word"] = functools.partial(tail, 0, 40 * W + 1)
LAYOUTS["tail_5_on_word"] = functools.partial(tail, 5, 40 * W)
for _p in FIRST_AT:
    LAYOUTS[f"first_at_{_p}"] = functools.partial(first_at, _p)
CLEAN = ("dense", "dense_edges", "word_edges", "empty_lanes", "empty_waves") + tuple(f"first_at_{p}" for p in FIRST_AT)
BAIT = ("bait_dead_end_2", "bait_dead_end_10", "bait_joins", "bait_leaves_E", "bait_leaves_total", "bait_long",
        "bait_first_word", "short_step", "hand_worked")
TAIL = tuple(k for k in LAYOUTS if k.startswith("tail_"))


@functools.lru_cache(maxsize=None)
def _layout(name):
    return LAYOUTS[name]()


def layout(name):
    """(the large one is kept by grid_wrap's own cache, which its test clears)"""
    return grid_wrap() if name == "grid_wrap" else _layout(name)


# ------------------------------------------------------------------------------ range sweeps
def lane_of(p, begin=0):
    return (p - begin) // L % WAVE


def edge_records(lay, begin=0):
    """The chain records on an edge of the grid anchored at `begin`: bit 0 or 31 of a word, lane 0
    or 63 of a wave, the first or last record of a wave chunk; and the chain's first and last."""
    ch = [s for s in lay.chain if s >= begin]
    out = []
    for i, s in enumerate(ch):
        q = s - begin
        first_of_chunk = i == 0 or (ch[i - 1] - begin) // C != q // C
        last_of_chunk = i + 1 == len(ch) or (ch[i + 1] - begin) // C != q // C
        if q % W in (0, W - 1) or lane_of(s, begin) in (0, WAVE - 1) or first_of_chunk or last_of_chunk:
            out.append(s)
    return out


def thin(xs, n):
    """At most n of xs, evenly spaced, the first and last among them."""
    xs = list(xs)
    if len(xs) <= n:
        return xs
    return [xs[(len(xs) - 1) * k // (n - 1)] for k in range(n)]


def marked(lay):
    """The positions a layout marks, a long run thinned to its first, middle and last."""
    out = []
    for v in lay.marks.values():
        out += thin(v, 3) if isinstance(v, tuple) else [v]
    return sorted(set(out))


def edges(lay, begin=0, n_first=6, n_end=8, cap=300):
    """(first, E) pairs, `cap` at most, no RNG: `first` over the edge records and the chain records a
    layout marks; E one before / at / one past each of them, the stream's last positions, past the
    stream, and first + 1."""
    total = len(lay.flat)
    recs = edge_records(lay, begin)
    on_chain = set(lay.chain)
    firsts = sorted(set(thin(recs, n_first)) | {p for p in marked(lay) if p in on_chain and p >= begin})
    ends = {total - k for k in range(6)} | {total + 100}
    for s in thin(recs, n_end) + marked(lay) + firsts:
        ends |= {s - 1, s, s + 1}
    out = []
    for f in firsts:
        out += [(f, e) for e in sorted(ends | {f + 1}) if e >= begin]
    return thin(out, cap)


# ------------------------------------------------------------------------------ split ranges
# label: (flat where the split's first member starts, flat where the member its end names starts)
def dense_edges_splits():
    lay = layout("dense_edges")
    bits = lay.bits
    below, at = lay.marks["below"], lay.marks["at"]
    nxt = lambda p: next(q for q in bits if q >= p)
    assert below == (C - 1, 3 * C - 1, 5 * C - 1) and at == (2 * C, 4 * C, 6 * C)
    # label: (first member's flat, end member's flat)
    cases = {
        "same chunk": (nxt(C + 100), nxt(C + 5000)),
        "adjacent chunks": (nxt(C + 100), nxt(2 * C + 3000)),
        "two chunks apart": (nxt(C + 100) + 1, nxt(3 * C + 700)),            # (a member that starts inside a record)
        "many inner chunks": (nxt(200), nxt(6 * C + 1000)),
        "E in a chunk's first word": (nxt(C + 100), 2 * C + 5),
        "E on a chunk's first position": (nxt(200), 2 * C),
        "E on a chunk's last position": (nxt(200), 3 * C - 1),                # the set bit at E is not counted
        "E on a chunk's last position, no inner chunk": (nxt(3 * C + 700), 5 * C - 1),
        "first on a chunk's last position": (C - 1, nxt(2 * C + 3000)),
        "first on a chunk's last position, inner chunks": (3 * C - 1, nxt(6 * C + 1000)),
        "first on a chunk's first position": (4 * C, 6 * C),
        "to the stream's end": (nxt(6 * C + 1000), len(lay.flat)),
    }
    def apart(k):
        """chunks between the range's first and last word (k - 1 of them lie strictly inside)"""
        f, x2 = nxt(cases[k][0]), cases[k][1]
        return ((x2 + W - 1) // W - 1) // VC_CHUNK - f // W // VC_CHUNK

    assert [apart(k) for k in ("same chunk", "adjacent chunks", "two chunks apart")] == [0, 1, 2]
    assert apart("E on a chunk's last position, no inner chunk") == 1 and apart("many inner chunks") == 6
    assert apart("E on a chunk's first position") == 1 and apart("E in a chunk's first word") == 1
    # E cuts a chunk's last word at a set bit: the range's words end on the chunk grid
    assert all((e + W - 1) // W % VC_CHUNK == 0 and e in bits for e in (3 * C - 1, 5 * C - 1))
    return cases


def popcount_splits():
    """Splits of more than PC_WORDS bitmap words whose first words lie at 4-word alignments 0..3."""
    lay = layout("dense_edges")
    firsts = {}
    for p in lay.bits:
        if p > 3000 and p // W % 4 not in firsts:
            firsts[p // W % 4] = p
    assert sorted(firsts) == [0, 1, 2, 3]
    ends = [next(q for q in lay.bits if q >= 9 * G - 2000 - 400 * k) for k in range(4)]
    cases = {f"first word {a} mod 4": (firsts[a], ends[a]) for a in range(4)}
    assert all((e - f) // W > PC_WORDS for f, e in cases.values())
    return cases


def marked_splits():
    """Splits of bait_joins, whose chain is marked through the false positives."""
    lay = layout("bait_joins")
    bait, bait2 = lay.marks["bait"], lay.marks["bait2"]
    cases = {
        "first is a chain record": (lay.chain[1], lay.marks["joined2"]),
        "first is the host": (lay.marks["host"], lay.chain[-5]),
        "first is a false positive": (bait[2] - 1, lay.chain[-5]),            # (a member that starts in the filler before it)
        "first is a false positive of the long run": (bait2[7], len(lay.flat)),
        "E inside the bait": (lay.chain[2], bait2[20]),
    }
    nxt = lambda p: next(q for q in lay.bits if q >= p)
    assert [nxt(x1) in lay.chain for x1, _ in cases.values()] == [True, True, False, False, True]
    return cases


# ------------------------------------------------------------------------------ the container
def compress(flat, payload=65280, level=1, cuts=()):
    """The flat bytes as BGZF members of `payload` bytes (a member ends at every flat offset of
    `cuts` as well) and the EOF member: (file bytes, [file offset of each data member], [its first
    flat position])."""
    out, offs, flats, n = [], [], [], 0
    marks = sorted({0, len(flat)} | {c for c in cuts if 0 < c < len(flat)})
    for x, y in zip(marks, marks[1:]):
        for o in range(x, y, payload):
            chunk = flat[o:min(o + payload, y)]
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            m = member_of(c.compress(chunk) + c.flush(), chunk)
            offs.append(n)
            flats.append(o)
            out.append(m)
            n += len(m)
    return b"".join(out) + EOF_MEMBER, offs, flats


def vpos_of(p, offs, flats):
    """The htsjdk virtual position of flat p (a position at a member's start belongs to that member)."""
    k = bisect.bisect_right(flats, p) - 1
    return offs[k] << 16 | (p - flats[k])
