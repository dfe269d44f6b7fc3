"""Hand-built BAM records for the SAM-text tests (test infrastructure; plain Python, no GPU),
built with record_corpus.rec() over its four-contig header.

* CASES      -- valid records at every width the renderer's 64-lane strides can get wrong (name,
               CIGAR, bases, Z values, B arrays of 0 / 1 / 63 / 64 / 65 / many elements), the
               fixed fields at their edges, every branch of the RNAME / RNEXT rules, every
               integer tag type at both ends of its range, a record with 40 tags and one with
               none, and three rows with float values (FLOAT_ROWS).
* MALFORMED  -- three good records, then one whose CIGAR or tag area the library refuses.
* FLOATS     -- (value bits, Float.toString text) literals.
"""
import functools
import struct
from collections import namedtuple

import record_corpus as rc

REF_NAMES = [n for n, _ in rc.CONTIGS]
N_REF = len(REF_NAMES)


def tag(name, typ, payload=b""):
    return name.encode() + typ.encode() + payload


def tag_z(name, n, typ="Z"):
    return tag(name, typ, bytes(33 + (7 * k + n) % 94 for k in range(n)) + b"\0")


_B_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}
_B_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1),
            "I": (0, 2 ** 32 - 1)}


def tag_b(name, sub, values):
    return tag(name, "B", sub.encode() + struct.pack("<i%d%s" % (len(values), _B_FMT[sub]), len(values), *values))


def _b_values(sub, n):
    """n values of the sub-type: both ends of its range first, then a spread of widths."""
    lo, hi = _B_RANGE[sub]
    spread = [lo, hi, 0, 9, 10, -1 if lo < 0 else 99, hi // 7, lo // 3, 100, hi // 1000]
    return [spread[k % len(spread)] for k in range(n)]


def _rec(name=b"r", ref_id=1, pos=777, mapq=7, flag=4, next_ref=2, next_pos=888, tlen=-33, cigar=(), seq=(), qual=b"",
         aux=b""):
    return rc.rec(ref_id, pos, mapq, 4681, flag, next_ref, next_pos, tlen, name, cigar, seq, qual, aux)


OP_LENGTHS = (0, 9, 10, 99999999, 268435455)
B_COUNTS = (0, 1, 63, 64, 65, 1000)


def _cigar(n):
    return tuple((OP_LENGTHS[k % 5], k % 9) for k in range(n))


def _cases():
    out = []
    add = lambda label, **kw: out.append((label, _rec(**kw)))  # noqa: E731
    for n in (0, 1, 63, 64, 65, 254):
        add("name%d" % n, name=rc._name(n))
    for n in (0, 1, 63, 64, 65, 200):
        add("cigar%d" % n, cigar=_cigar(n), flag=0)
    add("cigar_all_ops", cigar=tuple((k + 1, k) for k in range(9)), flag=0)
    for n in (0, 1, 2, 63, 64, 65, 129):
        add("seq%d" % n, seq=rc._codes(n, n), qual=rc._quals(n, n))
    add("qual_ff", seq=rc._codes(10, 5), qual=b"\xff" + bytes(range(1, 10)))
    add("qual_93", seq=rc._codes(66, 1), qual=bytes([93] * 66))
    add("qual_wrap", seq=rc._codes(3, 1), qual=bytes([0, 254, 250]))  # (q + 33) & 0xFF: 33, 31, 27
    add("qual_high", seq=rc._codes(3, 1), qual=bytes([100, 200, 222]))  # bytes 133, 233, 255 (see NOT_ASCII)
    add("edges_low", flag=0, mapq=0, pos=-1, next_pos=-1, tlen=-2 ** 31, ref_id=-1, next_ref=-1)
    add("edges_high", flag=65535, mapq=255, pos=2 ** 31 - 2, next_pos=2 ** 31 - 2, tlen=2 ** 31 - 1, ref_id=N_REF - 1,
        next_ref=N_REF - 1)
    add("pos_int_max", pos=2 ** 31 - 1, next_pos=2 ** 31 - 1)   # prints 2147483648
    add("pos_negative", pos=-5, next_pos=-2 ** 31)
    add("ref_first", ref_id=0, next_ref=N_REF - 1)             # RNEXT by name
    add("ref_past_end", ref_id=N_REF, next_ref=0)              # RNAME *, RNEXT by name
    add("ref_past_end_eq", ref_id=N_REF, next_ref=N_REF)       # RNAME *, RNEXT = (the rule's order)
    add("next_past_end", ref_id=0, next_ref=N_REF)             # RNEXT *
    add("next_unset_ref_set", ref_id=2, next_ref=-1)           # RNEXT *
    add("ref_unset_next_set", ref_id=-1, next_ref=1)           # RNAME *, RNEXT by name
    ints = b"".join(tag("X" + t, t, struct.pack("<" + _B_FMT[t], v)) for t in "cCsSiI" for v in _B_RANGE[t])
    add("int_tags", aux=ints)
    add("tag_a", aux=tag("XA", "A", b"!") + tag("XB", "A", b"~"))
    for n in (0, 1, 63, 64, 65, 300):
        add("z%d" % n, aux=tag("XI", "i", struct.pack("<i", n)) + tag_z("XZ", n) + tag("XC", "C", b"\x07"))
    add("tag_h", aux=tag("XH", "H", b"1AE301\0") + tag("XE", "H", b"\0"))
    for sub in "cCsSiI":
        add("b_" + sub, aux=b"".join(tag_b("B%d" % k, sub, _b_values(sub, n)) for k, n in enumerate(B_COUNTS)))
    add("tags40", aux=b"".join((tag("%c%c" % (65 + k // 10, 48 + k % 10), "s", struct.pack("<h", 811 * k - 16000)) if k % 3
                                else tag_z("%c%c" % (65 + k // 10, 48 + k % 10), k)) for k in range(40)),
        seq=rc._codes(5, 2), qual=rc._quals(5, 2), cigar=((5, 0),), flag=0)
    add("no_tags", seq=rc._codes(4, 2), qual=rc._quals(4, 2))
    # records of 1023, 1024 and 1025 bytes: the kernels walk a record of up to 1024 bytes in LDS
    base = len(_rec(seq=rc._codes(33, 1), qual=rc._quals(33, 1), aux=tag_z("XZ", 0) + tag("XC", "C", b"\x09")))
    for size in (1023, 1024, 1025):
        add("stage%d" % size, seq=rc._codes(33, 1), qual=rc._quals(33, 1),
            aux=tag_z("XZ", size - base) + tag("XC", "C", b"\x09"))
        assert len(out[-1][1]) == size
    f32 = lambda x: struct.pack("<f", x)  # noqa: E731
    add("float_f", aux=tag("XI", "i", struct.pack("<i", -7)) + tag("XF", "f", f32(1.5)) + tag_z("XZ", 70))
    add("float_bf", aux=tag_b("XB", "f", (0.25, -2.5, 12.75)) + tag_b("XE", "f", ()))
    add("float_both", name=rc._name(65), cigar=_cigar(65), seq=rc._codes(65, 3), qual=rc._quals(65, 3), flag=0,
        aux=tag_b("XS", "s", _b_values("s", 65)) + tag("XF", "f", f32(-0.0)) + tag_b("XB", "f", (0.5,) * 70))
    add("after_floats", aux=tag("XA", "A", b"z"))
    return tuple(out)


CASES = _cases()
NOT_ASCII = tuple(i for i, (label, _) in enumerate(CASES) if label == "qual_high")  # Reads.qual decodes as ASCII
FLOAT_ROWS = tuple(i for i, (label, _) in enumerate(CASES) if label.startswith("float_"))
assert len(FLOAT_ROWS) == 3


@functools.lru_cache(maxsize=None)
def stream():
    return rc.lay([r for _, r in CASES])


# ------------------------------------------------------------------------- malformed rows

GOOD = tuple(_rec(name=b"good%d" % k, aux=tag("XI", "i", struct.pack("<i", k))) for k in range(3))
_OK = tag("XA", "A", b"x")  # a good tag before the bad one: the walk has to get there
MALFORMED_AUX = (
    ("unknown_type", _OK + tag("XX", "q", b"\0")),
    ("unknown_b_subtype", _OK + tag("XB", "B", b"A" + struct.pack("<i", 1) + b"x")),
    ("z_without_nul", _OK + tag("XZ", "Z", b"abc")),
    ("h_without_nul", _OK + tag("XH", "H", b"")),
    ("b_over_the_end", _OK + tag("XB", "B", b"i" + struct.pack("<i", 5) + b"\0" * 16)),
    ("b_negative_count", _OK + tag("XB", "B", b"c" + struct.pack("<i", -1))),
    ("b_count_bytes_cut", _OK + tag("XB", "B", b"c\x01\x00")),
    ("truncated_i", _OK + tag("XI", "i", b"\x01\x02")),
    ("truncated_a", _OK + tag("XA", "A")),
    ("two_bytes_left", _OK + b"ab"),
    ("one_byte_left", _OK + b"a"),
)
Malformed = namedtuple("Malformed", "name stream bad_row")
MALFORMED = tuple(Malformed(n, rc.lay(list(GOOD) + [_rec(name=b"bad", aux=a)]), 3) for n, a in MALFORMED_AUX) + (
    Malformed("cigar_op_9", rc.lay(list(GOOD) + [_rec(name=b"bad", cigar=((5, 0), (5, 9)), flag=0)]), 3),
    # two bad rows: the smaller one is named
    Malformed("two_bad_rows", rc.lay([GOOD[0], _rec(name=b"bad", aux=b"ab"), GOOD[1],
                                      _rec(name=b"bad", cigar=((1, 15),), flag=0)]), 1),
)

# ------------------------------------------------------------------------- Float.toString literals

FLOATS = (
    (1.5, "1.5"), (1.0, "1.0"), (0.1, "0.1"), (0.3, "0.3"), (1 / 3, "0.33333334"), (100.0, "100.0"), (0.001, "0.001"),
    (1e-4, "1.0E-4"), (9999999.0, "9999999.0"), (1e7, "1.0E7"), (12345678.0, "1.2345678E7"),
    (16777216.0, "1.6777216E7"), (1e10, "1.0E10"), (-2.5, "-2.5"), (-0.0, "-0.0"),
    (3.4028234663852886e38, "3.4028235E38"), (1.1754943508222875e-38, "1.17549435E-38"),
    (1.401298464324817e-45, "1.4E-45"), (float("nan"), "NaN"), (float("inf"), "Infinity"),
    (float("-inf"), "-Infinity"),
)


def float_record(x):
    """A record holding x as an f tag and as a B:f element."""
    return _rec(name=b"f", aux=tag("XF", "f", struct.pack("<f", x)) + tag_b("XB", "f", (x,)))


def fixture_lines():
    """(header bytes, record lines each with its newline) of tests/golden/sam/2.sam.gz."""
    import gzip
    import os

    from conftest import GOLDEN
    with gzip.open(os.path.join(GOLDEN, "sam", "2.sam.gz")) as f:
        raw = f.read()
    lines = raw.split(b"\n")
    assert lines[-1] == b""
    lines = [l + b"\n" for l in lines[:-1]]
    k = next(i for i, l in enumerate(lines) if not l.startswith(b"@"))
    assert all(not l.startswith(b"@") for l in lines[k:])
    return b"".join(lines[:k]), lines[k:]
