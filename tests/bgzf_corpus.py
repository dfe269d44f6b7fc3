"""Hand-built BGZF containers for the index, FindBlockStart and CRC32 kernels -- TEST INFRASTRUCTURE.

Plain Python: zlib, struct, random and deflate_build; no GPU and no project code.  Every file comes
with the table of its members -- (start, csize, hsize, usize, empty) -- and the flat bytes it
inflates to, both written down while the members are laid (`Lay.add`), never parsed back.

  EDGES      stored members whose headers start at prescribed offsets around every 16384-byte
             chunk edge and 4096-byte segment edge of the candidate scan
  TAILS      cuts of small files: the ragged last chunk ending at, inside and just past a header
  SHAPES     XLEN != 6, the 31-byte stored member of no bytes, ISIZE 65536, empty members mid-file
  PLANTED    header-shaped bytes inside stored payloads (candidates that are off the chain)
  MANY       4101 tiny members: more than one scan workgroup, more than the CRC kernel's grid
  CRC_SIZES  every alignment 0..15 of the flat bytes for each size the CRC kernel branches on
  CRC_BAD    corrupted copies of those, each with its (n_bad, first_bad)
  FBS        FindBlockStart probes with their outcomes as literals

Files are built on first use and cached (functools.lru_cache): treat them as read-only.
"""
import functools
import random
import struct
import zlib
from collections import namedtuple

from deflate_build import EOF_MEMBER, Bits, member, stored_block

CHUNK, SEG = 16384, 4096  # k_cand_count: bytes per workgroup and per round of 16-byte loads
MAGIC = bytes([31, 139, 8, 4])

Member = namedtuple("Member", "start csize hsize usize empty")
File = namedtuple("File", "name data table flat meta")  # meta: per member, whatever the group records


# ------------------------------------------------------------------------------------- builder
def stored_raw(data):
    """The raw deflate stream of one final stored block (what deflate_build.stored_block writes;
    test_bgzf_corpus_cpu holds the two equal): 5 bytes and the data."""
    n = len(data)
    assert n < 65536
    return b"\x01" + struct.pack("<HH", n, n ^ 0xffff) + bytes(data)


def stored_raw_bits(data):
    w = Bits()
    stored_block(w, data, True)
    return w.bytes()


def deflate_raw(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(bytes(data)) + c.flush()


def subfield(si1, si2, data):
    """One gzip extra subfield: SI1 SI2 SLEN data (RFC 1952 2.3.1.1)."""
    return bytes([si1, si2]) + struct.pack("<H", len(data)) + bytes(data)


def bgzf_member(raw, isize, crc, extra=b"", bsize=None):
    """The BGZF member around the raw deflate bytes: ISIZE and CRC as given, `extra` (whole gzip
    subfields) after the BC subfield so that XLEN = 6 + len(extra) and hsize = 18 + len(extra).
    bsize: the BSIZE field when it is not to be the member's size - 1."""
    if not extra and bsize is None:
        return member(raw, isize, crc)
    total = 18 + len(extra) + len(raw) + 8
    assert total <= 65536, total
    hdr = (bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255]) + struct.pack("<H", 6 + len(extra)) + b"BC\x02\x00" +
           struct.pack("<H", total - 1 if bsize is None else bsize) + bytes(extra))
    return hdr + bytes(raw) + struct.pack("<II", crc & 0xffffffff, isize & 0xffffffff)


def header18(csize, xlen=6):
    """Header-shaped bytes: what Header.make accepts (31 139 8 4 .. 66 67 2 ..), BSIZE = csize - 1."""
    return (bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255]) + struct.pack("<H", xlen) + b"BC\x02\x00" +
            struct.pack("<H", csize - 1))


def quiet(n, seed):
    """n seeded bytes with no 31 among them: no gzip magic can begin here."""
    b = bytearray(random.Random(seed).randbytes(n))
    return bytes(b.translate(bytes(30 if i == 31 else i for i in range(256))))


class Lay:
    """A file under construction: bytes, member table, flat bytes, one meta entry per member."""

    def __init__(self, name):
        self.name, self.data, self.table, self.flat, self.meta = name, bytearray(), [], bytearray(), []

    @property
    def pos(self):
        return len(self.data)

    def add(self, data, *, how="stored", extra=b"", isize=None, crc=None, meta=None):
        """One member of `data`: how = "stored" | "deflate" | "fit" (level 6 where that fits a
        member, stored otherwise).  Returns its index in the table."""
        data = bytes(data)
        if how == "fit":
            raw = deflate_raw(data)
            if 18 + len(extra) + len(raw) + 8 > 65536:
                raw = stored_raw(data)
        else:
            raw = stored_raw(data) if how == "stored" else deflate_raw(data)
        m = bgzf_member(raw, len(data) if isize is None else isize, zlib.crc32(data) if crc is None else crc, extra)
        self.table.append(Member(self.pos, len(m), 18 + len(extra), len(data) if isize is None else isize, False))
        self.data += m
        self.flat += data
        self.meta.append(meta)
        return len(self.table) - 1

    def add_empty(self, crc=0, meta=None):
        """The 28-byte member of no bytes (the EOF member's shape)."""
        m = EOF_MEMBER[:-8] + struct.pack("<II", crc, 0)
        self.table.append(Member(self.pos, 28, 18, 0, True))
        self.data += m
        self.meta.append(meta)
        return len(self.table) - 1

    def add_raw_member(self, m, hsize, usize, meta=None):
        """Member bytes made elsewhere (not inflatable ones included); adds nothing to flat."""
        self.table.append(Member(self.pos, len(m), hsize, usize, False))
        self.data += m
        self.meta.append(meta)
        return len(self.table) - 1

    def done(self):
        return File(self.name, bytes(self.data), tuple(self.table), bytes(self.flat), tuple(self.meta))


def ustarts(table):
    """Flat offset of every member: the running sum of the sizes that reach the flat bytes (not
    those of empty members, nor an ISIZE above 65536, which the index gives no bytes)."""
    out, u = [], 0
    for m in table:
        out.append(u)
        if not m.empty and m.usize <= 65536:
            u += m.usize
    return out, u


def candidates(data, n=None):
    """Every offset of `data[:n]` where Header.make's seven byte tests hold and 18 bytes remain."""
    n = len(data) if n is None else n
    out, p = [], data.find(MAGIC)
    while 0 <= p and p + 18 <= n:
        if data[p + 12:p + 15] == b"BC\x02":
            out.append(p)
        p = data.find(MAGIC, p + 1)
    return out


# --------------------------------------------------------------------------------------- EDGES
EDGE_D_CHUNK = tuple(range(18, -2, -1))          # header start = boundary - d: 18 .. -1
EDGE_D_SEG = (18, 16, 15, 14, 13, 4, 3, 2, 1, 0)


def edge_targets():
    """[(offset, kind, boundary, d)]: one header per boundary, chunk edges 16384 j (j = 1, 2, ...)
    and, inside the first chunks, a 4096-multiple that is no chunk edge."""
    t = [(CHUNK * (j + 1) - d, "chunk", CHUNK * (j + 1), d) for j, d in enumerate(EDGE_D_CHUNK)]
    t += [(CHUNK * j + SEG * (1 + j % 3) - d, "seg", CHUNK * j + SEG * (1 + j % 3), d)
          for j, d in enumerate(EDGE_D_SEG)]
    return sorted(t)


@functools.lru_cache(maxsize=None)
def edges():
    """meta: the (kind, boundary, d) of the edge a member's own header was laid at."""
    f, edge = Lay("edges"), None
    for i, (off, kind, b, d) in enumerate(edge_targets()):
        f.add(quiet(off - f.pos - 31, 100 + i), meta=edge)  # ends at `off`: the next header starts there
        edge = (kind, b, d)
    f.add(quiet(777, 99), meta=edge)
    f.add_empty()
    return f.done()


# --------------------------------------------------------------------------------------- TAILS
def _tails_base(name, lead):
    f = Lay(name)
    if lead:
        f.add(quiet(lead, 7))
    for i, n in enumerate((40, 7, 100, 33, 58, 1)):
        f.add(quiet(n, 20 + i))
    return f.done()


@functools.lru_cache(maxsize=None)
def tails():
    """[(File cut to its length, label)]: the file ends in the ragged last chunk -- chunk 0 of a file
    below 16384 bytes, chunk 1 behind a 16431-byte first member -- at a member's end with no EOF
    member, at the next header's byte 1, 17, 18, 19, one byte short of that member's end, and at
    further lengths inside it until every residue mod 16 has occurred."""
    out = []
    for base in (_tails_base("tails_small", 0), _tails_base("tails", 16400)):
        k = len(base.table) - 5  # the member whose end is the cut; the next one has 100 payload bytes
        e, nxt = base.table[k].start + base.table[k].csize, base.table[k + 1]
        assert nxt.start == e and nxt.csize == 131
        cuts = [(e, "member_end"), (e + 1, "hdr1"), (e + 17, "hdr17"), (e + 18, "hdr18"), (e + 19, "hdr19"),
                (e + nxt.csize - 1, "short1"), (len(base.data), "whole")]
        seen = {c % 16 for c, _ in cuts}
        for c in range(e + 20, e + 60):
            if c % 16 not in seen:
                seen.add(c % 16)
                cuts.append((c, "in%d" % (c - e)))
        for c, label in cuts:
            tab = tuple(m for m in base.table if m.start + m.csize <= c)
            _, fs = ustarts(tab)
            out.append(File("%s_%s" % (base.name, label), base.data[:c], tab, base.flat[:fs], None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tail_min():
    """A file whose last 18 bytes are a whole member by Header.make's arithmetic: XLEN 2 (hsize 14),
    BSIZE 17 (csize 18), so that csize - hsize - 4 = 0 and ISIZE is read from the header's own last
    four bytes (02 00 11 00).  Nothing inflates it; MetadataStream lists it.  The member before it
    ends exactly 18 bytes before the end of the file: k_cand_link's `q + 18 > n` at equality."""
    f = Lay("tail_min")
    for i, n in enumerate((16400, 40, 7)):
        f.add(quiet(n, 40 + i))
    f.add_raw_member(header18(18, xlen=2), 14, 0x00110002)
    return f.done()


# -------------------------------------------------------------------------------------- SHAPES
@functools.lru_cache(maxsize=None)
def shapes():
    rng = random.Random(5)
    text = bytes(rng.choice(b"ACGT") for _ in range(3000))
    x1 = subfield(ord("X"), ord("Y"), b"\x01\x02\x03")
    x2 = x1 + subfield(ord("R"), ord("G"), b"")
    f = Lay("shapes")
    f.add(text, how="deflate", extra=x1, meta="xlen13_deflate")
    f.add(quiet(200, 1), extra=x1, meta="xlen13_stored")
    f.add(text[::-1], how="deflate", extra=x2, meta="xlen17_deflate")
    f.add(quiet(333, 2), extra=x2, meta="xlen17_stored")
    f.add(b"", meta="stored0")
    f.add(bytes(rng.choice(b"ACGTN") for _ in range(65536)), how="deflate", meta="isize65536")
    f.add_empty(meta="empty_mid")
    f.add(quiet(50, 3), meta="after_empty")
    f.add_empty(meta="empty_pair0")
    f.add_empty(meta="empty_pair1")
    f.add(text[:999], how="deflate", meta="after_pair")
    f.add_empty(meta="eof")
    return f.done()


# ------------------------------------------------------------------------------------- PLANTED
PLANT_L = 5000  # csize of the regular members: member k starts at 5000 k
# (offset, csize written in the planted header, label); every target is known from the layout
PLANTS = (
    (2000, 300, "a_mid"),                       # (a) points at quiet bytes
    (CHUNK - 7, 1000, "a_edge"),
    (7000, 10000 - 7000, "b_mid"),              # (b) lands on the real header at 10000
    (2 * CHUNK - 9, 35000 - (2 * CHUNK - 9), "b_edge"),
    (21000, 1000, "c_mid0"), (22000, 1500, "c_mid1"), (23500, 1500, "c_mid2"),        # (c) -> 25000
    (3 * CHUNK - 3, 51000 - (3 * CHUNK - 3), "c_edge0"), (51000, 1000, "c_edge1"), (52000, 3000, "c_edge2"),
    (26053, 200, "d_mid0"), (26071, 200, "d_mid1"), (26089, 200, "d_mid2"),           # (d) 18 apart
    (4 * CHUNK - 25, 200, "d_edge0"), (4 * CHUNK - 7, 200, "d_edge1"), (4 * CHUNK + 11, 200, "d_edge2"),
)
PLANT_C_MID, PLANT_C_EDGE = 21000, 3 * CHUNK - 3


@functools.lru_cache(maxsize=None)
def planted():
    """14 stored members of 5000 bytes, two of 20000 (a chunk with one candidate), the EOF member;
    PLANTS written into the payloads.  meta: the planted offsets (on the File, not per member)."""
    f = Lay("planted")
    for k in range(16):
        size = PLANT_L if k < 14 else 20000
        pay = bytearray(quiet(size - 31, 300 + k))
        s = f.pos
        for off, cs, _ in PLANTS:
            if s <= off < s + size:
                assert s + 23 <= off and off + 18 <= s + size - 8, off  # inside this payload
                pay[off - s - 23:off - s - 5] = header18(cs)
        f.add(pay)
    f.add_empty()
    return f.done()


# ---------------------------------------------------------------------------------------- MANY
MANY_N = 2048 * 2 + 5


@functools.lru_cache(maxsize=None)
def many():
    f = Lay("many")
    rng = random.Random(11)
    for i in range(MANY_N):
        f.add(bytes(rng.randrange(32, 256) for _ in range(1 + i % 3)))
    f.add_empty()
    return f.done()


# ----------------------------------------------------------------------------------- CRC_SIZES
CRC_SMALL = (1, 2, 3, 4, 5, 6, 7, 15, 16, 17, 255, 256, 257, 258, 259, 511, 512, 513)
CRC_LARGE = (65279, 65280, 65535, 65536)
CRC_LARGE_ALIGN = (0, 1, 7, 15)
PATTERNS = ("random", "zero", "ff", "zero5one")


def pattern(kind, n, seed):
    if kind == "zero":
        return bytes(n)
    if kind == "ff":
        return b"\xff" * n
    if kind == "zero5one":
        return (b"\x00\x00\x00\x00\x00\x01" * (n // 6 + 1))[:n]
    rng = random.Random(seed)
    if n <= 65280:
        return rng.randbytes(n)
    # 7 bits of entropy a byte, over an alphabet of both halves of the byte range: level 6 brings
    # 65536 of them under a member's 65536 bytes, which no coding of uniform bytes does
    alpha = bytes(rng.sample(range(256), 128))
    return bytes(alpha[b & 127] for b in rng.randbytes(n))


def _crc_small(kind, how):
    f = Lay("crc_small_%s_%s" % (kind, how))
    for s in CRC_SMALL:
        for r in range(16):
            f.add(pattern(kind, s, 1000 * s + r), how=how, meta=("size", s, len(f.flat) % 16))
            if s % 2 == 0:
                f.add(pattern(kind, 1, s + r), how=how, meta=("spacer", 1, len(f.flat) % 16))
    f.add_empty()
    return f.done()


def _crc_large(kind, how, sizes=CRC_LARGE):
    f = Lay("crc_large_%s_%s" % (kind, how))
    for s in sizes:
        for a in CRC_LARGE_ALIGN:
            gap = (a - len(f.flat)) % 16
            if gap:
                f.add(pattern(kind, gap, s + a), how=how, meta=("spacer", gap, len(f.flat) % 16))
            f.add(pattern(kind, s, 7 * s + a), how=how, meta=("size", s, len(f.flat) % 16))
    f.add_empty()
    return f.done()


@functools.lru_cache(maxsize=None)
def crc_sizes():
    return tuple(_crc_small(k, "fit") for k in PATTERNS) + tuple(_crc_large(k, "fit") for k in PATTERNS)


# ------------------------------------------------------------------------------------- CRC_BAD
BadCase = namedtuple("BadCase", "name file bad n_bad first_bad")  # bad: indices into file.table


def _case(name, f, data, bad):
    bad = sorted(set(bad))
    return BadCase(name, f._replace(name=name, data=bytes(data)), tuple(bad), len(bad), f.table[bad[0]].start)


def _members_of(f, size):
    return [i for i, m in enumerate(f.meta) if m and m[0] == "size" and m[1] == size]


def _payload_edit(f, data, i, off):
    """One byte of stored member i's payload changed, footer left alone."""
    m = f.table[i]
    assert 0 <= off < m.usize and m.csize == m.usize + 31
    data[m.start + 23 + off] ^= 0x5a


def seg_boundaries(usize):
    """First and last 256-byte segment boundary of the CRC kernel, as payload offsets: segments
    end at the block's last byte, so the boundaries are usize - 256 k."""
    return usize - 256 * ((usize - 1) // 256), usize - 256


@functools.lru_cache(maxsize=None)
def crc_bad():
    out = []
    fit = _crc_small("random", "fit")
    # footer edits: one bit in each of the four CRC bytes, on separate members
    picks = [_members_of(fit, s)[3 * k + 1] for k, s in enumerate((5, 17, 258, 513))]
    both = bytearray(fit.data)
    for k, i in enumerate(picks):
        one = bytearray(fit.data)
        for d in (one, both):
            d[fit.table[i].start + fit.table[i].csize - 8 + k] ^= 1 << (2 * k + 1)
        out.append(_case("footer_byte%d" % k, fit, one, [i]))
    out.append(_case("footer_all4", fit, both, picks))
    # an empty member mid-file with a non-zero CRC
    e = Lay("empty_crc")
    for k in range(5):
        e.add(pattern("random", 300 + k, k), how="fit")
    i = e.add_empty(crc=0x00010000)
    for k in range(5):
        e.add(pattern("random", 200 + k, 9 + k), how="fit")
    e.add_empty()
    e = e.done()
    out.append(_case("empty_mid_crc", e, e.data, [i]))
    # payload edits of stored members
    st = _crc_small("random", "stored")
    for off in (0, 1, 2, 3, 4, -1):
        for size in (5, 258):
            i = _members_of(st, size)[(off + 7) % 16]
            d = bytearray(st.data)
            _payload_edit(st, d, i, off % size)
            out.append(_case("payload_%d_at%s" % (size, "last" if off < 0 else off), st, d, [i]))
    for size in (513,):
        first, last = seg_boundaries(size)
        for off in (first - 1, first, last - 1, last):
            i = _members_of(st, size)[off % 16]
            d = bytearray(st.data)
            _payload_edit(st, d, i, off)
            out.append(_case("segedge_%d_at%d" % (size, off), st, d, [i]))
    big = _crc_large("random", "stored", (65279, 65280))
    for size in (65279, 65280):
        first, last = seg_boundaries(size)
        for k, off in enumerate((first - 1, first, last - 1, last)):
            i = _members_of(big, size)[k]
            d = bytearray(big.data)
            _payload_edit(big, d, i, off)
            out.append(_case("segedge_%d_at%d" % (size, off), big, d, [i]))
    # every member of a sixteen-alignment run; three runs at once
    for sizes in ((257,), (5, 256, 511)):
        d, bad = bytearray(st.data), []
        for size in sizes:
            for k, i in enumerate(_members_of(st, size)):
                _payload_edit(st, d, i, (k * 37) % size)
                bad.append(i)
        out.append(_case("run_" + "_".join(map(str, sizes)), st, d, bad))
    # MANY: blocks past the CRC kernel's 1024 workgroups, all taken by the same workgroup
    m = many()
    d, bad = bytearray(m.data), [1030, 1030 + 1024, 1030 + 2048]
    for i in bad:
        _payload_edit(m, d, i, 0)
    out.append(_case("many_same_workgroup", m, d, bad))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def crc_stream_clean():
    """For the windowed path: 60 stored members of 2000 random bytes (2031 bytes each)."""
    f = Lay("crc_stream")
    for k in range(60):
        f.add(pattern("random", 2000, 50 + k))
    f.add_empty()
    return f.done()


@functools.lru_cache(maxsize=None)
def crc_stream_case():
    """One payload byte changed in members 17, 18 and 40 of crc_stream_clean().  With 32768-byte
    windows and a halo of 8192 bytes or more, members 17 and 18 (at 34527 and 36558) are owned by
    the second window and lie in the first one's halo."""
    f = crc_stream_clean()
    d, bad = bytearray(f.data), [17, 18, 40]
    for i in bad:
        _payload_edit(f, d, i, 5 + i)
    return _case("stream_halo", f, d, bad)


# ----------------------------------------------------------------------------------------- FBS
OK, SEARCH_FAILED, TRUNCATED = "ok", "search failed", "truncated"
# file: key of fbs_files(); want: (OK, offset) | (SEARCH_FAILED,) | (TRUNCATED,); cut: a shard
# length inside the look-ahead of the deciding attempt, where the answer has to be "need more
# bytes" (None: the attempt reads nothing past `start`)
Probe = namedtuple("Probe", "name file start blocks_to_check want cut")

FBS_GAP = 65546          # fbs "gap": this many quiet bytes, then the chain


def _fbs_gap():
    """65546 quiet bytes that belong to no member, then a chain.  (A gap of 65536 bytes without a
    header cannot lie inside a valid chain: a member is at most 65536 bytes, header included.)"""
    f = Lay("gap")
    f.data += quiet(FBS_GAP, 61)
    for k in range(6):
        f.add(quiet(100 + k, 62 + k))
    f.add_empty()
    return f.done()


def _fbs_false():
    """Members of 3000 bytes (member k at 3000 k) with, in their payloads:
      member 1  a header at 3500 whose BSIZE points at quiet bytes
      member 2  a chain 6500 -> 7000 -> 7500 -> quiet bytes (three links hold, the fourth does not)
      member 3  a header at 10000 with csize 20: csize - hsize - 4 < 0
      member 8  a header at 25000 with csize 60000: past the end of the file
    then X (27000, 131 bytes), an empty member (27131), 50 quiet bytes and the end of the file."""
    f = Lay("false")
    plants = {3500: 100, 6500: 500, 7000: 500, 7500: 500, 10000: 20, 25000: 60000}
    for k in range(9):
        pay = bytearray(quiet(3000 - 31, 80 + k))
        for off, cs in plants.items():
            if 3000 * k <= off < 3000 * (k + 1):
                pay[off - 3000 * k - 23:off - 3000 * k - 5] = header18(cs)
        f.add(pay)
    assert f.pos == 27000
    f.add(quiet(100, 95))
    f.add_empty()
    f.data += quiet(50, 96)
    return f.done()


@functools.lru_cache(maxsize=None)
def fbs_files():
    return {"gap": _fbs_gap(), "false": _fbs_false(), "planted": planted()}


FBS_FALSE_LEN = 27000 + 131 + 28 + 50

FBS = (
    # the first header 65535 bytes on is the last position tried; 65536 bytes on is never tried
    Probe("gap_65535", "gap", FBS_GAP - 65535, 5, (OK, FBS_GAP), FBS_GAP + 200),
    Probe("gap_65536", "gap", FBS_GAP - 65536, 5, (SEARCH_FAILED,), FBS_GAP - 20000),
    Probe("gap_from0", "gap", 0, 5, (SEARCH_FAILED,), 40000),
    # a false header 10 bytes on whose second link fails: the search goes on to the real one
    Probe("false_retry", "false", 3490, 5, (OK, 6000), 6000 + 3000 * 4 + 10),
    Probe("false_depth1", "false", 3490, 1, (OK, 3500), 3510),
    # three false links hold: accepted to depth 3, refused from depth 4
    Probe("chain3_k1", "false", 6490, 1, (OK, 6500), 6510),
    Probe("chain3_k3", "false", 6490, 3, (OK, 6500), 7510),
    Probe("chain3_k4", "false", 6490, 4, (OK, 9000), 9000 + 3000 * 3 + 5),
    Probe("chain3_k6", "false", 6490, 6, (OK, 9000), 9000 + 3000 * 5 + 5),
    # csize - hsize - 4 < 0: the exception escapes, the good header at 12000 is never reached
    Probe("neg_remaining", "false", 9995, 5, (TRUNCATED,), 10010),
    # csize runs past the end of the file
    Probe("past_eof", "false", 24996, 5, (TRUNCATED,), 26000),
    # an empty member second: success with two blocks, although quiet bytes follow it
    Probe("empty_second", "false", 26997, 5, (OK, 27000), 27140),
    Probe("last17", "false", FBS_FALSE_LEN - 10, 5, (OK, FBS_FALSE_LEN - 10), FBS_FALSE_LEN - 1),
    Probe("last17_edge", "false", FBS_FALSE_LEN - 17, 5, (OK, FBS_FALSE_LEN - 17), None),
    Probe("depth0", "false", 5, 0, (OK, 5), None),
    Probe("depth0_gap", "gap", 10, 0, (OK, 10), None),
) + tuple(
    # PLANTED (c): three false links and then the real chain -- it holds at every depth, so the
    # reference itself answers the false header
    Probe("planted_c_%s_k%d" % (lab, k), "planted", p0 - 10, k, (OK, p0), p0 + 12)
    for lab, p0 in (("mid", PLANT_C_MID), ("edge", PLANT_C_EDGE)) for k in (1, 3, 4, 5, 6))


def index_files():
    """Every file the index is held to: (File, ...)."""
    return (edges(),) + tails() + (tail_min(), shapes(), planted(), many())
