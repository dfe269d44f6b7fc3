"""Hand-built inputs for the BAM gather (sbh_bam_gather_host / sbh_records_bam_scan): streams
from record_corpus.rec / lay, keep patterns as row ranges, and a ten-line numpy restatement
of the definition in csrc/bam_gather_core.h (test infrastructure; plain Python, no GPU).

* ladder_stream() -- records of every total length 37..68 (l_read_name 1..32, l_seq 0), the
                     ladder repeated LADDER_REPEATS times with a 49-byte spacer record after each
                     repeat.  The copy kernel moves 16-byte granules of the output from wherever
                     they lie in the flat stream, so what matters is the pair (source mod 16,
                     destination mod 16) of a record's first byte.  A ladder is 1680 = 16 x 105
                     bytes and its partial sums meet every residue; with the spacers dropped
                     (LADDER_ROWS) each repeat moves the source one byte on against the
                     destination, so each head length 0..15 meets all 256 pairs.
* long_stream()   -- one record of more than 70 000 bytes (longer than a BGZF member and than
                     many copy tiles) between two 37-byte ones.
* keep patterns   -- all, first only, last only, alternating, alternating blocks of 63 / 64 / 65.
"""
import functools
import struct

import numpy as np

import record_corpus as rc

LADDER_LENGTHS = tuple(range(37, 37 + 32))
LADDER_REPEATS = 16
HEADS = tuple(bytes((7 * k + h) % 251 for k in range(h)) for h in range(16))  # head lengths 0..15


def ladder_record(i):
    """Record i of the ladder: 36 fixed bytes + a name of (i % 32) bytes and its NUL."""
    k = i % 32
    return rc.rec(i % 4, 1000 + i, i % 256, 4681, (i * 2654435761) & 0xFFFF, -1, -1, 0,
                  bytes(65 + (i + j) % 26 for j in range(k)), (), (), b"", b"")


SPACER = rc.rec(0, 0, 0, 4681, 0x800, -1, -1, 0, b"spacer-49-bs", (), (), b"", b"")
LADDER_ROWS = [(33 * r, 33 * r + 32) for r in range(LADDER_REPEATS)]  # every row but the spacers


@functools.lru_cache(maxsize=None)
def ladder_stream():
    recs = [x for r in range(LADDER_REPEATS) for x in [ladder_record(32 * r + k) for k in range(32)] + [SPACER]]
    assert tuple(len(r) for r in recs[:32]) == LADDER_LENGTHS and len(SPACER) == 49
    return rc.lay(recs)


@functools.lru_cache(maxsize=None)
def long_stream():
    n = 47011
    big = rc.rec(1, 5, 30, 4681, 0, -1, -1, 0, b"long", ((n, rc.M),), rc._codes(n, 3), rc._quals(n, 5), rc._aux(65))
    assert len(big) > 70000
    return rc.lay([ladder_record(0), big, ladder_record(0)])


def pattern_ranges(name, n):
    """Row ranges [(begin, end), ...] of a keep pattern over n rows (None: no ranges, keep all)."""
    if name == "all":
        return None
    if name == "first":
        return [(0, 1)]
    if name == "last":
        return [(n - 1, n)] if n else [(0, 1)]
    if name == "alternating":
        return [(i, i + 1) for i in range(0, max(n, 1), 2)]
    b = int(name[len("blocks"):])
    return [(i, i + b) for i in range(0, max(n, 1), 2 * b)]  # (the last one may reach past n)


PATTERNS = ("all", "first", "last", "alternating", "blocks63", "blocks64", "blocks65")


def fields(flat, starts):
    """(flag, mapq, 4 + block_size) of the records at starts (numpy)."""
    flat = np.frombuffer(bytes(flat), np.uint8)
    st = np.asarray(starts, np.int64)
    u32 = lambda o: sum(flat[st + o + k].astype(np.int64) << (8 * k) for k in range(4))  # noqa: E731
    return u32(16) >> 16, flat[st + 13].astype(np.int64), u32(0) + 4


def gather_ref(flat, starts, head=b"", flag_require=0, flag_exclude=0, min_mapq=0, rows=None):
    """The definition restated: (stream bytes, rec_off, rows) for valid records."""
    flag, mapq, size = fields(flat, starts) if len(starts) else (np.zeros(0, np.int64),) * 3
    idx = np.arange(len(starts))
    keep = ((flag & flag_require) == flag_require) & ((flag & flag_exclude) == 0) & (mapq >= min_mapq)
    if rows is not None:
        keep &= np.isin(idx, np.concatenate([np.arange(a, min(b, len(starts))) for a, b in rows] + [np.zeros(0, int)]))
    kept = idx[keep]
    parts = [bytes(flat[starts[i]:starts[i] + size[i]]) for i in kept]
    off = np.cumsum([len(head)] + [len(p) for p in parts]).astype(np.uint64)
    return bytes(head) + b"".join(parts), off, kept.astype(np.uint64)


def residue_pairs(stream, head_len, ranges):
    """{(source mod 16, destination mod 16)} of the kept records' first bytes."""
    _, off, kept = gather_ref(stream.flat, stream.starts, b"\0" * head_len, rows=ranges)
    return {(int(stream.starts[int(r)]) % 16, int(o) % 16) for r, o in zip(kept, off[:-1])}


def filter_dict(flag_require=0, flag_exclude=0, min_mapq=0, rows=None):
    f = {"flag_require": flag_require, "flag_exclude": flag_exclude, "min_mapq": min_mapq}
    if rows is not None:
        f["rows"] = rows
    return f


def streams():
    """(name, Stream) of every valid corpus."""
    return (("decode", rc.decode_stream()), ("ladder", ladder_stream()), ("long", long_stream()))


def driver_input(flat, starts, head, flag_require=0, flag_exclude=0, min_mapq=0, rows=None):
    """The sanitizer driver's input file (tests/sanitize/bam_gather_driver.cpp)."""
    rows = rows or []
    return (struct.pack("<Q", len(flat)) + bytes(flat) + struct.pack("<Q", len(starts))
            + np.asarray(starts, "<u8").tobytes() + struct.pack("<Q", len(head)) + bytes(head)
            + struct.pack("<IIiIQ", flag_require, flag_exclude, min_mapq, 0, len(rows))
            + np.asarray([a for a, _ in rows], "<u8").tobytes() + np.asarray([b for _, b in rows], "<u8").tobytes())
