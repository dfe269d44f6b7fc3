"""Hand-built inputs for the FASTQ / FASTA text (sbh_fastq_render_host / sbh_records_fastq_scan), and
an independent restatement of the definition in csrc/fastq_core.h: the packed bases through
bytes.hex() and a translate table, the reverse complement as a second translate table and [::-1],
the qualities as a 256-entry table -- not a port of the library's index arithmetic.  That restatement
is the expected value everywhere, compared by exact equality (test infrastructure; plain Python, no
GPU).

Records are record_corpus.rec's bytes laid behind record_corpus.header().  A corpus is a stream; its
VARIANTS are the keyword sets it is rendered under: fasta, suffix ("auto" / "never" / "always"),
split, def_qual, filter (records.record_filter's dict).  Row i of a scan is sized by lane i % 64 of
k_fastq_sizes and written by wave i % 4 of a workgroup of k_fastq_emit.
"""
import functools
import struct
from collections import namedtuple

import numpy as np

import record_corpus as rc

GRID_PASS = 1024 * 256  # rows one pass of k_fastq_sizes' grid holds
PAIRED, REVERSE, READ1, READ2, SECONDARY, SUPPLEMENTARY = 0x1, 0x10, 0x40, 0x80, 0x100, 0x800
PART_CLASSES = (1, 2, 0)

Case = namedtuple("Case", "flat starts")

# ------------------------------------------------------------------------------ the restatement

_HEX_TO_BASE = bytes.maketrans(b"0123456789abcdef", b"=ACMGRSVTWYHKDBN")
_COMPLEMENT = bytes.maketrans(b"ACMGRSVTWYHKDBN=", b"TGKCYSBAWRDMHVN=")
_QUAL = bytes(min(q, 93) + 33 for q in range(256))


def _kept(flag, mapq, i, f):
    if (flag & f.get("flag_require", 0)) != f.get("flag_require", 0) or flag & f.get("flag_exclude", 0):
        return False
    if mapq < f.get("min_mapq", 0):
        return False
    return f.get("rows") is None or any(a <= i < b for a, b in f["rows"])


def read_class(flag, suffix):
    """1, 2 or 0: the /1 and /2 conditions, without the 0x1 requirement under suffix="always"."""
    if not flag & PAIRED and suffix != "always":
        return 0
    return {READ1: 1, READ2: 2}.get(flag & (READ1 | READ2), 0)


def line(record, fasta=False, suffix="auto", def_qual=1):
    """One record's lines from its bytes (block_size word first)."""
    l_name, n_cig, flag, l_seq = record[12], *struct.unpack_from("<HHi", record, 16)
    name = record[36:36 + l_name].split(b"\0")[0]
    at = 36 + l_name + 4 * n_cig
    packed, qual = record[at:at + (l_seq + 1) // 2], record[at + (l_seq + 1) // 2:at + (l_seq + 1) // 2 + l_seq]
    seq = packed.hex().encode().translate(_HEX_TO_BASE)[:l_seq]
    q = bytes([def_qual + 33]) * l_seq if l_seq and qual[0] == 0xFF else qual.translate(_QUAL)
    if flag & REVERSE:
        seq, q = seq.translate(_COMPLEMENT)[::-1], q[::-1]
    c = read_class(flag, suffix)
    tail = b"/%d" % c if c and suffix != "never" else b""
    if fasta:
        return b">" + name + tail + b"\n" + seq + b"\n"
    return b"@" + name + tail + b"\n" + seq + b"\n+\n" + q + b"\n"


def restate(flat, starts, fasta=False, suffix="auto", split=False, def_qual=1, filter=None):
    """The definition restated.  Returns a dict: bad_row (None or the first invalid row; nothing else
    then), text (bytes), rec_off, rows (lists, layout order), sizes (sbh_fastq_sizes as a dict)."""
    flat, total, f = bytes(flat), len(flat), filter or {}
    parts = {c: [] for c in PART_CLASSES}
    for i, p in enumerate(int(s) for s in starts):
        if p > total or total - p < 36:
            return {"bad_row": i}
        bsz, _, _, w12, w16, l_seq = struct.unpack_from("<iiiIIi", flat, p)
        l_name, mapq, n_cig, flag = w12 & 0xFF, (w12 >> 8) & 0xFF, w16 & 0xFFFF, w16 >> 16
        if l_seq < 0 or bsz < 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq or bsz + 4 > total - p:
            return {"bad_row": i}
        if _kept(flag, mapq, i, f):
            c = read_class(flag, suffix) if split else 1
            parts[c].append((i, line(flat[p:p + 4 + bsz], fasta, suffix, def_qual)))
    text, rec_off, rows, part_bytes, part_rows = [], [], [], [], []
    at = 0
    for c in PART_CLASSES:
        part_bytes.append(sum(len(ln) for _, ln in parts[c]))
        part_rows.append(len(parts[c]))
        for i, ln in parts[c]:
            rec_off.append(at)
            rows.append(i)
            text.append(ln)
            at += len(ln)
    rec_off.append(at)
    return {"bad_row": None, "text": b"".join(text), "rec_off": rec_off, "rows": rows,
            "sizes": {"n": len(starts), "n_kept": len(rows), "text_bytes": at, "part_bytes": part_bytes, "part_rows": part_rows}}


# ----------------------------------------------------------------------------------- builders

def one(name=b"r", flag=0, codes=(), qual=None, mapq=30, cigar=(), aux=b"", spare=0):
    qual = rc._quals(len(codes), 3) if qual is None else qual
    return rc.rec(0, 100, mapq, 4681, flag, -1, -1, 0, name, cigar, codes, qual, aux, spare=spare)


def case(records):
    s = rc.lay(list(records))
    return Case(s.flat, list(s.starts))


def no_name_bytes(flag=0, codes=(1, 2, 4, 8, 15)):
    """A record whose l_read_name is 0 (the smallest row_check admits): not even the NUL."""
    r = bytearray(one(b"", flag, codes))
    assert r[12] == 1 and r[36] == 0
    del r[36]
    r[12] = 0
    r[0:4] = struct.pack("<i", len(r) - 4)
    return bytes(r)


SEQ_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1500)  # the last: a record above 1024 bytes
PAIR_FLAGS = (0x41, 0x81, 0xC1, 0x01, 0x40, 0x80)


def _seq_lengths():
    return case([one(b"s%d_%s" % (n, b"fr"[r:r + 1]), REVERSE * r, rc._codes(n, n), rc._quals(n, n), spare=0xF * (n & 1))
                 for n in SEQ_LENGTHS for r in (0, 1)])


def _quals():
    out = []
    for r in (0, 1):
        fl = REVERSE * r
        out += [one(b"all_ff", fl, rc._codes(10, 5), b"\xff" * 10),
                one(b"first_ff", fl, rc._codes(7, 1), b"\xff" + bytes(range(6))),
                one(b"later_ff", fl, rc._codes(7, 2), bytes((0, 40, 0xFF, 12, 0xFF, 93, 1))),
                one(b"last_ff", fl, rc._codes(4, 3), bytes((5, 6, 7, 0xFF))),
                one(b"edges", fl, rc._codes(9, 4), bytes((0, 92, 93, 94, 222, 233, 254, 1, 60))),
                one(b"one_ff", fl, (4,), b"\xff"), one(b"one_233", fl, (8,), b"\xe9")]
    return case(out)


def _names():
    return case([one(b"x", 0, rc._codes(5, 1)), one(rc._name(254), REVERSE, rc._codes(6, 2)),
                 one(b"ab\0cd", 0x41, rc._codes(4, 3)), one(b"\0hidden", 0x91, rc._codes(3, 4)), one(b"", 0, rc._codes(2, 5)),
                 no_name_bytes(), no_name_bytes(0x51), one(b"slash/1", 0x41, rc._codes(1, 6)),
                 # the name is followed by CIGAR words, and tags follow the qualities
                 one(b"cig", REVERSE, rc._codes(9, 7), cigar=((4, rc.S), (5, rc.M)), aux=b"NMC\x05XSZabc\0")])


def _flags():
    return case([one(b"f%03x" % (f | r), f | r, rc._codes(5 + (f >> 6), f & 15)) for f in PAIR_FLAGS for r in (0, REVERSE)])


def mixed(n, seed, flags=(0, REVERSE, 0x41, 0x51, 0x81, 0x91, 0xC1, 0x01, 0x40, 0x80, 0x141, 0x881, 0x4)):
    """n records of arbitrary length (0..70 bases), strand, class and name."""
    r = np.random.RandomState(seed)
    out = []
    for i in range(n):
        ls = int(r.randint(0, 71))
        q = bytes(r.randint(0, 256, ls).astype(np.uint8)) if i % 5 else b"\xff" * ls
        out.append(one(b"m%d_" % i + rc._name(int(r.randint(0, 20))), int(flags[r.randint(0, len(flags))]),
                       tuple(int(x) for x in r.randint(0, 16, ls)), q, mapq=int(r.randint(0, 61))))
    return case(out)


def _grid():
    s = rc.grid_stream()[0]
    return Case(s.flat, s.starts.tolist())


_ONE_PER_WAVE = [(64 * w + (5 * w) % 64, 64 * w + (5 * w) % 64 + 1) for w in range(8)]
_MODES = ({}, {"fasta": True}, {"split": True}, {"suffix": "never"}, {"suffix": "always", "split": True, "fasta": True})
_SUFFIXES = tuple({"suffix": s, "split": sp} for s in ("auto", "never", "always") for sp in (False, True))

CORPORA = {
    "seq_lengths": _seq_lengths,
    "all_codes": lambda: case([one(b"hi", 0, tuple(range(16))), one(b"hi_r", REVERSE, tuple(range(16))),
                               one(b"lo", 0, (15,) + tuple(range(16))), one(b"lo_r", REVERSE, (15,) + tuple(range(16)), spare=9)]),
    "quals": _quals,
    "names": _names,
    "flags": _flags,
    # split with a class empty, with only class 0, and with the classes alternating lane by lane
    "split_no_class_2": lambda: case([one(b"a%d" % k, (0x41, 0x00, 0x51, 0x10)[k % 4], rc._codes(k % 7, k)) for k in range(70)]),
    "split_only_class_0": lambda: case([one(b"o%d" % k, (0, REVERSE, 0xC1, 0x01)[k % 4], rc._codes(k % 5, k)) for k in range(70)]),
    "split_alternating": lambda: case([one(b"l%d" % k, (0x41, 0x81, 0x01)[k % 3] | REVERSE * (k % 2), rc._codes(k % 9, k))
                                       for k in range(200)]),
    "filters": lambda: mixed(512, 7),
    "grid": _grid,
}
VARIANTS = {
    "seq_lengths": _MODES,
    "all_codes": ({}, {"fasta": True}),
    "quals": ({"def_qual": 0}, {"def_qual": 1}, {"def_qual": 93}, {"fasta": True}),
    "names": _MODES,
    "flags": _SUFFIXES + ({"fasta": True, "suffix": "always"},),
    "split_no_class_2": ({"split": True}, {"split": True, "suffix": "never"}),
    "split_only_class_0": ({"split": True}, {}),
    "split_alternating": ({"split": True}, {"split": True, "fasta": True}, {}),
    "filters": ({"filter": {"flag_require": 0x400}}, {"filter": {"rows": _ONE_PER_WAVE}, "split": True},
                {"filter": {"rows": [(5, 50), (100, 130), (511, 512)]}}, {"filter": {"flag_exclude": 0x900}},
                {"filter": {"flag_exclude": 0x900, "min_mapq": 30, "flag_require": 0x1}, "split": True},
                {"filter": {"rows": []}}),
    "grid": ({}, {"split": True, "filter": {"flag_exclude": REVERSE, "rows": [(5, 100000), (262100, 262181)]}}),
}
for _n in (0, 1, 63, 64, 65, 255, 256, 257):
    CORPORA["rows_%d" % _n] = functools.partial(lambda n: mixed(n, 100 + n), _n)
    VARIANTS["rows_%d" % _n] = ({}, {"split": True}, {"fasta": True})
LARGE = ("grid",)
SMALL = tuple(k for k in CORPORA if k not in LARGE)
ALL = tuple((k, v) for k in CORPORA for v in range(len(VARIANTS[k])))
ALL_SMALL = tuple((k, v) for k, v in ALL if k in SMALL)


def ident(kv):
    return "%s-%d" % kv


@functools.lru_cache(maxsize=None)
def get(name):
    return CORPORA[name]()


@functools.lru_cache(maxsize=None)
def expected(name, variant):
    c = get(name)
    return restate(c.flat, c.starts, **VARIANTS[name][variant])


def driver_input(flat, starts, mode, def_qual, filter=None):
    """The sanitizer driver's input file (tests/sanitize/fastq_driver.cpp)."""
    f = filter or {}
    rows = f.get("rows")
    if rows is not None and not rows:  # no rows asked for: one range no row lies in (records.record_filter's)
        rows = [(2 ** 64 - 2, 2 ** 64 - 1)]
    rows = rows or []
    return (struct.pack("<Q", len(flat)) + bytes(flat) + struct.pack("<Q", len(starts))
            + np.asarray(starts, "<u8").tobytes()
            + struct.pack("<IiIIi", mode, def_qual, f.get("flag_require", 0), f.get("flag_exclude", 0), f.get("min_mapq", 0))
            + struct.pack("<Q", len(rows)) + np.asarray([a for a, _ in rows], "<u8").tobytes()
            + np.asarray([b for _, b in rows], "<u8").tobytes())
