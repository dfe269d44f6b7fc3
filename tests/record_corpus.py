"""Hand-built BAM record streams for the record-delivery conformance suite (test
infrastructure; plain Python, no GPU).

A record builder whose header fields may lie about what follows them, a BAM header over
four contigs, a BGZF wrapper (zlib members of a chosen payload size + the EOF member), and
four case tables:

* DECODE_CASES   -- valid records laid one after another: every length at which a wave
                    striding by 64 over name / CIGAR / bases / qualities / tags can go
                    wrong, both nibble phases, CIGAR words at every byte alignment, and the
                    fixed fields at their edges.
* INTERVAL_RECORDS / INTERVAL_CASES / INTERVAL_ARG_ERRORS / CHUNK_CASES
                 -- records on contigs 0..3 and query intervals, with the kept records
                    written down by hand from the semantics in oracle_records.region's
                    docstring (Region(contig, pos, pos + reference span), empty for an
                    unmapped read or an empty span, none without a contig; kept when a
                    half-open interval of the contig overlaps it).  They are literals, not
                    computed.
* MALFORMED_CASES -- three good records, then one that htsjdk's decode would throw on.
* grid_stream()  -- 262144 + 37 minimal records (more than k_rec_fields' grid holds waves,
                    so its grid-stride loop runs), a running counter in pos and in the name.
"""
import functools
import struct
import zlib
from collections import namedtuple

import numpy as np

from deflate_build import EOF_MEMBER, member_of

SEQ = "=ACMGRSVTWYHKDBN"
M, I, D, N, S, H, P, EQ, X = range(9)  # CIGAR op codes

# (name, length): dictionary order differs from name order
CONTIGS = (("chrM", 16571), ("chr10", 135534747), ("chr2", 2147483647), ("chr1", 249250621))
PAYLOADS = (65280, 4096, 97)


def rec(ref_id, pos, mapq, bin, flag, next_ref, next_pos, tlen, name, cigar, seq_codes, qual, aux,
        block_size=None, l_seq=None, n_cigar=None, spare=0):
    """One BAM record's bytes.  name: bytes without the NUL (the builder appends it); cigar:
    (length, op code) pairs; seq_codes: 4-bit base codes, the first in the high nibble; spare:
    the low nibble of the last byte of an odd-length sequence.  block_size / l_seq / n_cigar
    override what the header says (not what follows it)."""
    name_z = bytes(name) + b"\0"
    assert len(name_z) <= 255 and len(qual) == len(seq_codes)
    cig = b"".join(struct.pack("<I", (ln << 4 | op) & 0xffffffff) for ln, op in cigar)
    packed = bytearray((len(seq_codes) + 1) // 2)
    for k, c in enumerate(seq_codes):
        packed[k // 2] |= (c & 15) << (0 if k & 1 else 4)
    if len(seq_codes) & 1:
        packed[-1] |= spare & 15
    nc = len(cigar) if n_cigar is None else n_cigar
    ls = len(seq_codes) if l_seq is None else l_seq
    body = struct.pack("<iiIIiiii", ref_id, pos, (bin & 0xffff) << 16 | (mapq & 0xff) << 8 | len(name_z),
                       (flag & 0xffff) << 16 | (nc & 0xffff), ls, next_ref, next_pos, tlen)
    body += name_z + cig + bytes(packed) + bytes(qual) + bytes(aux)
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def header(contigs=CONTIGS):
    """BAM header bytes (magic, text, reference dictionary)."""
    text = "@HD\tVN:1.5\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in contigs)
    out = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(contigs))
    for n, ln in contigs:
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    return out


def bgzf(flat, payload, level=6):
    """The flat bytes cut into BGZF members of `payload` bytes (zlib raw deflate), plus the
    EOF member."""
    out = []
    for o in range(0, len(flat), payload):
        chunk = bytes(flat[o:o + payload])
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        out.append(member_of(c.compress(chunk) + c.flush(), chunk))
    return b"".join(out) + EOF_MEMBER


def inflate_members(data):
    """zlib's reading of a BGZF file: the members' inflated bytes joined."""
    data, out, p = bytes(data), [], 0
    while p < len(data):
        total = struct.unpack_from("<H", data, p + 16)[0] + 1
        u = zlib.decompress(data[p + 18:p + total - 8], -15)
        assert struct.unpack_from("<II", data, p + total - 8) == (zlib.crc32(u), len(u))
        out.append(u)
        p += total
    return b"".join(out)


Stream = namedtuple("Stream", "flat first starts")  # flat bytes, first record, every record's start


def lay(records, tail=b""):
    """Header + the records one after another (+ loose tail bytes)."""
    hdr = header()
    starts, p = [], len(hdr)
    for r in records:
        starts.append(p)
        p += len(r)
    return Stream(hdr + b"".join(records) + tail, len(hdr), starts)


# ------------------------------------------------------------------------- decode cases

Rec = namedtuple("Rec", "label ref_id pos mapq bin flag next_ref next_pos tlen name cigar seq_codes qual aux spare")
_DEFAULTS = dict(ref_id=1, pos=777, mapq=7, bin=4681, flag=4, next_ref=2, next_pos=888, tlen=-33, name=b"r",
                 cigar=(), seq_codes=(), qual=b"", aux=b"", spare=0)


def _r(label, **kw):
    d = dict(_DEFAULTS, **kw)
    if "name" not in kw:
        d["name"] = label.encode()
    return Rec(label, **d)


def rec_bytes(c, **overrides):
    return rec(c.ref_id, c.pos, c.mapq, c.bin, c.flag, c.next_ref, c.next_pos, c.tlen, c.name, c.cigar,
               c.seq_codes, c.qual, c.aux, spare=c.spare, **overrides)


def _codes(n, k0):
    return tuple((3 * k + k0) % 16 for k in range(n))


def _quals(n, k0):
    return bytes((7 * k + k0) % 94 for k in range(n))


def _name(n):
    """n printable bytes (the record's l_read_name is n + 1)."""
    return bytes(33 + (k * 5 + n) % 94 for k in range(n))


def _cigar(n, codes=9):
    return tuple((k + 1, k % codes) for k in range(n))


def _aux(n):
    return bytes((0x00, 0xFF, 0x7F, 0x80)[k % 4] if k % 3 else (k * 37 + 11) % 256 for k in range(n))


SEQ_LENGTHS = (0, 1, 2, 63, 64, 65, 129, 1000)
NAME_LENGTHS = (1, 2, 63, 64, 65, 255)  # l_read_name, the NUL included
CIGAR_COUNTS = (0, 1, 63, 64, 65)
AUX_LENGTHS = (0, 1, 64, 65)
B_ARRAY_TAG = b"XBBS" + struct.pack("<iHHH", 3, 0, 0xFFFF, 0x1234)

DECODE_CASES = tuple(
    [_r("seq%d" % n, seq_codes=_codes(n, n), qual=_quals(n, n)) for n in SEQ_LENGTHS]
    + [
        # all 16 codes from the high nibble on, then the same shifted by one base
        _r("codes_hi", seq_codes=tuple(range(16)), qual=_quals(16, 1)),
        _r("codes_lo", seq_codes=(15,) + tuple(range(16)), qual=_quals(17, 2)),
        # an odd l_seq whose last byte has a non-zero spare low nibble
        _r("odd_spare", seq_codes=(1, 2, 4, 8, 15), qual=_quals(5, 3), spare=0xF),
        _r("odd_spare1", seq_codes=(0,), qual=b"\x00", spare=0x5),
        _r("qual_ff", seq_codes=_codes(10, 5), qual=b"\xff" * 10),
    ]
    + [_r("name%d" % n, name=_name(n - 1)) for n in NAME_LENGTHS]
    + [_r("cig%d" % n, cigar=_cigar(n), flag=0, seq_codes=_codes(3, n), qual=_quals(3, n)) for n in CIGAR_COUNTS]
    + [
        # n_cigar_op and flag share a word: each at its 16-bit limit next to the other's zero / one
        _r("cig_max", cigar=_cigar(65535, codes=16), flag=0),
        _r("flag_max", cigar=((9, M),), flag=0xFFFF),
    ]
    # four records of a multiple of 4 bytes each, names of 2..5 bytes: their CIGARs begin at
    # four different addresses mod 4 whatever the stream before them
    + [_r("align%d" % k, name=_name(k - 1), cigar=((0xFFFFFFF, X), (k, M)), aux=_aux((4 - k) % 4)) for k in (2, 3, 4, 5)]
    + [_r("aux%d" % n, aux=_aux(n), seq_codes=_codes(2, n), qual=_quals(2, n)) for n in AUX_LENGTHS]
    + [
        _r("aux_b_array", aux=B_ARRAY_TAG),
        _r("edges_low", ref_id=-1, pos=-1, next_ref=-1, next_pos=-1, tlen=-2 ** 31, bin=0xFFFF, mapq=255),
        _r("edges_high", ref_id=3, pos=2 ** 31 - 1, next_ref=3, next_pos=2 ** 31 - 1, tlen=2 ** 31 - 1, bin=0,
           mapq=0),
    ])


def _pad_to(cases, label, modulus):
    """cases + a record whose tag bytes end the stream so far on a multiple of `modulus`: the
    record after it starts exactly at the end of a BGZF member of that payload."""
    end = len(header()) + sum(len(rec_bytes(c)) for c in cases) + len(rec_bytes(_r(label)))
    return cases + (_r(label, aux=_aux(-end % modulus)),)


# a record starting exactly where a member of payload 4096 ends, and one for payload 97
DECODE_CASES = _pad_to(DECODE_CASES, "pad4096", 4096) + (_r("at4096", seq_codes=_codes(7, 1), qual=_quals(7, 1)),)
DECODE_CASES = _pad_to(DECODE_CASES, "pad97", 97) + (_r("at97", seq_codes=_codes(9, 2), qual=_quals(9, 2)),)
MEMBER_END_STARTS = (("at4096", 4096), ("at97", 97))


@functools.lru_cache(maxsize=None)
def decode_stream():
    return lay([rec_bytes(c) for c in DECODE_CASES])


def expected_columns(cases):
    """The columns of oracle_records.decode's layout (without `flat`), from the values the
    builder was given."""
    fixed = {"ref_id": np.int32, "pos": np.int32, "next_ref_id": np.int32, "next_pos": np.int32, "tlen": np.int32,
             "flag": np.uint16, "bin": np.uint16, "mapq": np.uint8}
    field = {"next_ref_id": "next_ref"}
    out = {k: np.asarray([getattr(c, field.get(k, k)) for c in cases], dtype=dt) for k, dt in fixed.items()}
    names = b"".join(bytes(c.name) + b"\0" for c in cases)
    out["names"] = np.frombuffer(names, np.uint8)
    out["cigar"] = np.asarray([ln << 4 | op for c in cases for ln, op in c.cigar], np.uint32)
    out["seq"] = np.frombuffer("".join(SEQ[x] for c in cases for x in c.seq_codes).encode(), np.uint8)
    out["qual"] = np.frombuffer(b"".join(bytes(c.qual) for c in cases), np.uint8)
    out["aux"] = np.frombuffer(b"".join(bytes(c.aux) for c in cases), np.uint8)
    for k, ln in (("name_off", lambda c: len(c.name) + 1), ("cigar_off", lambda c: len(c.cigar)),
                  ("seq_off", lambda c: len(c.seq_codes)), ("aux_off", lambda c: len(c.aux))):
        out[k] = np.cumsum([0] + [ln(c) for c in cases]).astype(np.uint64)
    return out


# ------------------------------------------------------------------------- interval cases

def _iv(label, ref_id, pos, cigar, flag=0):
    n = sum(ln for ln, op in cigar if op in (M, I, S, EQ, X))  # (bases the CIGAR reads)
    return _r(label, ref_id=ref_id, pos=pos, flag=flag, cigar=tuple(cigar), seq_codes=_codes(n, pos % 16),
              qual=_quals(n, pos % 94), next_ref=ref_id, next_pos=max(pos, 0), tlen=0)


# In stream order.  Region [pos, pos + span) in the comment; "-" = no region / an empty one.
INTERVAL_RECORDS = (
    _iv("neg1_s1", 0, -1, [(1, M)]),                       # [-1, 0)
    _iv("neg1_s5", 0, -1, [(5, M)]),                       # [-1, 4)
    _iv("m_only", 0, 100, [(10, M)]),                      # [100, 110)
    _iv("d_only", 0, 200, [(10, D)]),                      # [200, 210)
    _iv("n_only", 0, 300, [(10, N)]),                      # [300, 310)
    _iv("eq_only", 0, 400, [(10, EQ)]),                    # [400, 410)
    _iv("x_only", 0, 500, [(10, X)]),                      # [500, 510)
    _iv("mix", 0, 600, [(3, S), (5, M), (2, I), (4, D), (1, P), (6, N), (2, EQ), (3, X), (7, H)]),  # [600, 620)
    _iv("hi_ops", 0, 700, [(5, M)] + [(100, op) for op in range(9, 16)]),                           # [700, 705)
    _iv("edge", 0, 1000, [(20, M)]),                       # [1000, 1020)
    _iv("no_cigar", 0, 1100, []),                          # - (mapped, span 0)
    _iv("clip_only", 0, 1200, [(5, S), (3, I)]),           # - (span 0)
    _iv("unmapped_placed", 0, 1300, [(10, M)], flag=4),    # - (flag 4: getAlignmentEnd = 0)
    _iv("c1_a", 1, 50, [(10, M)]),                         # [50, 60)
    _iv("c1_b", 1, 5000, [(10, M)]),                       # [5000, 5010)
    _iv("c2_a", 2, 100, [(10, M)]),                        # [100, 110)
    _iv("c2_big10", 2, 2147483640, [(10, M)]),             # [2^31 - 8, 2^31 + 2)
    _iv("c2_big20", 2, 2147483640, [(20, M)]),             # [2^31 - 8, 2^31 + 12)
    _iv("c3_a", 3, 10, [(10, M)]),                         # [10, 20)
    _iv("c3_b", 3, 1000, [(10, M)]),                       # [1000, 1010)
    _iv("noref_cigar", -1, 1400, [(10, M)]),               # - (no contig)
)

IntervalCase = namedtuple("IntervalCase", "name intervals kept")  # intervals: (ref, begin, end); kept: labels

ALL_INTERVALS = ((0, 0, 20000), (1, 0, 1000000), (2, 0, 2 ** 32), (3, 0, 300000000))
ALL_KEPT = ("neg1_s5", "m_only", "d_only", "n_only", "eq_only", "x_only", "mix", "hi_ops", "edge", "c1_a", "c1_b",
            "c2_a", "c2_big10", "c2_big20", "c3_a", "c3_b")

INTERVAL_CASES = (
    # the reference span of each op alone and of the mix: the region's last base, then one past it
    IntervalCase("span_last_base", ((0, 109, 110), (0, 209, 210), (0, 309, 310), (0, 409, 410), (0, 509, 510),
                                    (0, 619, 620), (0, 704, 705)),
                 ("m_only", "d_only", "n_only", "eq_only", "x_only", "mix", "hi_ops")),
    IntervalCase("span_one_past", ((0, 110, 111), (0, 210, 211), (0, 310, 311), (0, 410, 411), (0, 510, 511),
                                   (0, 620, 621), (0, 705, 706)), ()),
    # record [b, e) = [1000, 1020)
    IntervalCase("at_end", ((0, 1020, 1030),), ()),
    IntervalCase("last_base", ((0, 1019, 1030),), ("edge",)),
    IntervalCase("before", ((0, 990, 1000),), ()),
    IntervalCase("first_base", ((0, 990, 1001),), ("edge",)),
    IntervalCase("inside", ((0, 1005, 1010),), ("edge",)),
    IntervalCase("containing", ((0, 995, 1025),), ("edge",)),
    # no CIGAR, S/I only, a placed unmapped mate, and (whatever the contig) refID -1
    IntervalCase("empty_regions", ((0, 1050, 1500),), ()),
    IntervalCase("pos_minus_one", ((0, 0, 3),), ("neg1_s5",)),
    IntervalCase("contigs_0_2", ((0, 0, 20000), (2, 0, 200)),
                 ("neg1_s5", "m_only", "d_only", "n_only", "eq_only", "x_only", "mix", "hi_ops", "edge", "c2_a")),
    IntervalCase("contig_3_only", ((3, 0, 2000),), ("c3_a", "c3_b")),
    IntervalCase("several_hit", ((1, 0, 10), (1, 20, 30), (1, 40, 45), (1, 59, 70), (1, 4000, 4999), (1, 5009, 5010)),
                 ("c1_a", "c1_b")),
    IntervalCase("several_miss", ((1, 0, 10), (1, 20, 50), (1, 60, 70), (1, 5010, 6000)), ()),
    IntervalCase("one_per_contig", ((0, 105, 106), (1, 55, 56), (2, 105, 106), (3, 15, 16)),
                 ("m_only", "c1_a", "c2_a", "c3_a")),
    IntervalCase("past_2_31", ((2, 2 ** 31 + 5, 2 ** 32 + 7),), ("c2_big20",)),
    IntervalCase("across_2_31", ((2, 2147483600, 2 ** 31 + 1), (2, 2 ** 31 + 2, 2 ** 31 + 3)),
                 ("c2_big10", "c2_big20")),
    IntervalCase("no_intervals", (), ()),
    IntervalCase("everything", ALL_INTERVALS, ALL_KEPT),
)

# each is SBH_E_ARG; (name, intervals, chunk begins past the stream)
INTERVAL_ARG_ERRORS = (
    ("empty_interval", ((0, 5, 5),), False),
    ("unsorted_begin", ((0, 10, 20), (0, 0, 5)), False),
    ("unsorted_ref", ((1, 0, 5), (0, 0, 5)), False),
    ("overlapping", ((0, 0, 10), (0, 5, 15)), False),
    ("chunk_past_stream", ((0, 0, 10),), True),
)

# Chunk ends as (record label, byte delta); "^" the first record, "$" the end of the stream.
# Intervals are ALL_INTERVALS; kept: labels in delivery order; per: kept records per chunk.
ChunkCase = namedtuple("ChunkCase", "name chunks kept per")
CHUNK_CASES = (
    ChunkCase("ends_at_record_start", ((("^", 0), ("edge", 0)),),
              ("neg1_s5", "m_only", "d_only", "n_only", "eq_only", "x_only", "mix", "hi_ops"), (8,)),
    ChunkCase("ends_one_byte_in", ((("^", 0), ("edge", 1)),),
              ("neg1_s5", "m_only", "d_only", "n_only", "eq_only", "x_only", "mix", "hi_ops", "edge"), (9,)),
    ChunkCase("adjacent", ((("^", 0), ("x_only", 0)), (("x_only", 0), ("c1_b", 0))),
              ("neg1_s5", "m_only", "d_only", "n_only", "eq_only", "x_only", "mix", "hi_ops", "edge", "c1_a"), (5, 5)),
    ChunkCase("empty_chunk", ((("mix", 0), ("mix", 0)),), (), (0,)),
    ChunkCase("end_past_stream", ((("c2_big20", 0), ("$", 1000)),), ("c2_big20", "c3_a", "c3_b"), (3,)),
)


@functools.lru_cache(maxsize=None)
def interval_stream():
    return lay([rec_bytes(c) for c in INTERVAL_RECORDS])


def interval_start(label):
    """Flat start of a record of the interval stream ("^": the first; "$": the stream's end)."""
    s = interval_stream()
    if label == "$":
        return len(s.flat)
    return s.starts[0 if label == "^" else [c.label for c in INTERVAL_RECORDS].index(label)]


def chunk_flats(case):
    return [(interval_start(a) + da, interval_start(b) + db) for (a, da), (b, db) in case.chunks]


def loci_by_ref(intervals):
    out = {}
    for ref, a, b in intervals:
        out.setdefault(ref, []).append((a, b))
    return out


# ------------------------------------------------------------------------- malformed cases

GOOD = tuple(_iv("good%d" % k, 0, 10 + 20 * k, [(10, M)]) for k in range(3))
BAD = _iv("bad", 0, 100, [(10, M)])          # [100, 110): the interval below would keep it
BAD_KEEPING_INTERVALS = ((0, 0, 1000),)
_BAD_PARTS = len(rec_bytes(BAD)) - 4          # what block_size must be for BAD's parts

MalformedCase = namedtuple("MalformedCase", "name stream bad_start")


def _malformed(name, bad_bytes):
    s = lay([rec_bytes(c) for c in GOOD] + [bad_bytes])
    return MalformedCase(name, s, s.starts[-1])


MALFORMED_CASES = (
    _malformed("block_size_one_short", rec_bytes(BAD, block_size=_BAD_PARTS - 1)),
    _malformed("l_seq_minus_one", rec_bytes(BAD, l_seq=-1)),
    _malformed("block_size_minus_five", rec_bytes(BAD, block_size=-5)),
    _malformed("35_bytes_left", rec_bytes(BAD)[:35]),
    _malformed("one_byte_past_stream", rec_bytes(BAD, block_size=_BAD_PARTS + 1)),
)


# ------------------------------------------------------------------------- grid stride

GRID_RECORDS = 262144 + 37  # k_rec_fields' grid is 65536 workgroups of 4 waves
GRID_DTYPE = np.dtype([("block_size", "<i4"), ("ref_id", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"),
                       ("mapq", "u1"), ("bin", "<u2"), ("n_cigar_op", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"),
                       ("next_ref_id", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "S8")])


def grid_case(i):
    """Record i of the grid-stride stream as a table entry."""
    return _r("g%d" % i, ref_id=1 + i % 3, pos=i, mapq=i % 251, bin=i % 65521, flag=4 | (i % 2) << 4,
              next_ref=1 + (i + 1) % 3,
              next_pos=GRID_RECORDS - i, tlen=i - 131072, name=b"%07d" % i)


@functools.lru_cache(maxsize=None)
def grid_stream():
    """(Stream, the records as a GRID_DTYPE array): 44-byte records, built vectorised; the CPU
    test pins rows of it against rec()."""
    i = np.arange(GRID_RECORDS, dtype=np.int64)
    a = np.zeros(GRID_RECORDS, GRID_DTYPE)
    a["block_size"] = GRID_DTYPE.itemsize - 4
    a["ref_id"], a["pos"], a["l_read_name"] = 1 + i % 3, i, 8
    a["mapq"], a["bin"], a["flag"] = i % 251, i % 65521, 4 | (i % 2) << 4
    a["next_ref_id"], a["next_pos"], a["tlen"] = 1 + (i + 1) % 3, GRID_RECORDS - i, i - 131072
    digits = np.stack([(i // 10 ** k) % 10 + 48 for k in range(6, -1, -1)] + [np.zeros_like(i)], axis=1)
    a["name"] = np.ascontiguousarray(digits.astype(np.uint8)).view("S8")[:, 0]
    hdr = header()
    starts = len(hdr) + GRID_DTYPE.itemsize * i
    return Stream(hdr + a.tobytes(), len(hdr), starts), a
