"""Hand-built inputs for the read-name sort (sbh_bam_name_sort_host / sbh_records_bam_scan_names):
record streams whose names and flags are chosen, and the pure-Python restatement of the definition
in csrc/bam_name_core.h -- the name padded with zeros to 256 bytes, then the tie, then
sorted(..., key=...), which is stable and compares bytes as unsigned.  That restatement is the
expected value everywhere (test infrastructure; plain Python, no GPU).

Records are record_corpus.rec's bytes behind record_corpus.header(); pos, mapq and tlen vary with the
row index, so records of equal name and tie differ and a stream comparison sees a tie broken the
wrong way.  The group counts every case expects come from a Counter over the padded names, which
needs no order; where a case is built to give particular counts they are also written down (EXPECT).
"""
import functools
import struct
from collections import Counter

import numpy as np

import record_corpus as rc

SORT_TILE = 2048
T = SORT_TILE
GRID_ROWS = rc.GRID_RECORDS  # one more than a full grid pass of the row kernels takes
READ1, READ2, SECONDARY, SUPPLEMENTARY = 0x40, 0x80, 0x100, 0x800
INFO_KEYS = ("n_names", "n_single", "n_pair", "n_more", "max_name", "chunks_run", "passes_run", "already")


def record(i, name, flag, l_read_name=None):
    """Row i's record: `name` (bytes, without the NUL) and `flag`; l_read_name=0 rewrites the length
    byte of an empty name, whose NUL then counts as a tag byte."""
    r = bytearray(rc.rec(i % 3, 1000 + i, i % 251, 4681, flag, -1, -1, i % 1000 - 500, name, (), (), b"", b""))
    if l_read_name is not None:
        assert l_read_name == 0 and not name
        r[12] = 0
    return bytes(r)


def stream_of(rows):
    """rows: (name, flag) or (name, flag, l_read_name) per record."""
    return rc.lay([record(i, *row) for i, row in enumerate(rows)])


# ------------------------------------------------------------------------- the restatement

def fields_of(flat, starts):
    """(padded names, ties, name lengths) of the records at starts, from the stream's bytes."""
    flat = bytes(flat)
    padded, tie, length = [], [], []
    for s in (int(x) for x in starts):
        l_read_name = flat[s + 12]
        n = l_read_name - 1 if l_read_name else 0
        flag = struct.unpack_from("<H", flat, s + 18)[0]
        padded.append(flat[s + 36:s + 36 + n].ljust(256, b"\0"))
        tie.append(((flag >> 6) & 3) << 2 | ((flag >> 11) & 1) << 1 | ((flag >> 8) & 1))
        length.append(n)
    return padded, tie, length


def perm_ref(flat, starts):
    """perm[k] = the index into starts of the record that comes k-th."""
    padded, tie, _ = fields_of(flat, starts)
    return np.asarray(sorted(range(len(padded)), key=lambda i: (padded[i], tie[i])), dtype=np.uint64)


def info_ref(flat, starts, device=False):
    """sbh_bam_name_info of the records at starts, as a dict.  chunks_run and passes_run are the
    device's (the host entry leaves them 0): when the rows are not in order as given, a chunk runs
    when it is not the same in every row, and within it -- and within the tie -- one pass per byte
    that is not the same in every row."""
    padded, tie, length = fields_of(flat, starts)
    sizes = Counter(Counter(padded).values())
    key = [(p, t) for p, t in zip(padded, tie)]
    already = all(key[k - 1] <= key[k] for k in range(1, len(key)))
    chunks = passes = 0
    if device and not already:
        a = np.frombuffer(b"".join(padded), np.uint8).reshape(len(padded), 256)
        varies = (a != a[0]).any(axis=0).reshape(32, 8)
        chunks = int(varies.any(axis=1).sum())
        passes = int(varies.sum()) + (len(set(tie)) > 1)
    return dict(n_names=sum(sizes.values()), n_single=sizes.get(1, 0), n_pair=sizes.get(2, 0),
                n_more=sum(v for k, v in sizes.items() if k > 2), max_name=max(length, default=0), chunks_run=chunks,
                passes_run=passes, already=already)


def sorted_ref(flat, starts, head=b"", keep=None):
    """(stream, rec_off, rows) of the name-order call: `keep` = the scan rows the filter keeps (None:
    all), in scan order."""
    st = np.asarray(starts, np.int64)
    keep = np.arange(st.size) if keep is None else np.asarray(keep, np.int64)
    rows = keep[perm_ref(flat, st[keep]).astype(np.int64)] if keep.size else keep
    flat = bytes(flat)
    parts = [flat[int(st[r]):int(st[r]) + 4 + struct.unpack_from("<i", flat, int(st[r]))[0]] for r in rows]
    off = np.cumsum([len(head)] + [len(p) for p in parts]).astype(np.uint64)
    return bytes(head) + b"".join(parts), off, rows.astype(np.uint64)


# ------------------------------------------------------------------------- the cases

def _rng(name):
    return np.random.default_rng(sum(name.encode()) * 7919 + len(name))


def _printable(g, n_bytes):
    return bytes(g.integers(33, 127, n_bytes).astype(np.uint8))


def _random_rows(name, n):
    """n rows over a pool of n // 2 + 1 printable names of 1..40 bytes: names repeat, flags vary."""
    g = _rng(name)
    pool = [_printable(g, int(g.integers(1, 41))) for _ in range(n // 2 + 1)]
    flags = (0, READ1, READ2, READ1 | 0x10, READ2 | SECONDARY, SUPPLEMENTARY)
    return [(pool[int(g.integers(len(pool)))], flags[int(g.integers(len(flags)))]) for _ in range(n)]


def _lengths():
    """Names of 0 bytes (l_read_name 0 and 1), 1, 7, 8, 9, 16, 17 and 254 bytes, four of each with
    different bytes, in an order that is not theirs."""
    g = _rng("lengths")
    rows = [(b"", 0, 0), (b"", READ1), (b"", 0, 0), (b"", 0)]
    for n in (1, 7, 8, 9, 16, 17, 254):
        rows += [(_printable(g, n), 0) for _ in range(4)]
    return [rows[i] for i in g.permutation(len(rows))]


def _byte_edges():
    """Pairs that differ in byte 7 alone, in byte 8 alone, in the last byte of a 254-byte name alone --
    the larger one first -- and a triple that differs in bytes 7 and 8 against the chunk order."""
    long_ = bytes(65 + k % 26 for k in range(253))
    return [(b"abcdefgZxxxxxxxx", 0), (b"abcdefgAxxxxxxxx", 0),        # byte 7: chunk 0's last
            (b"ABCDEFGHZxxxxxxx", 0), (b"ABCDEFGHAxxxxxxx", 0),        # byte 8: chunk 1's first
            (long_ + b"z", 0), (long_ + b"a", 0),                      # byte 253: chunk 31
            (b"mmmmmmmBAmmmmmmm", 0), (b"mmmmmmmABmmmmmmm", 0), (b"mmmmmmmAAmmmmmmm", 0),
            (b"\x01\x02\x03\x04\x05\x06\x07\x08", 0), (b"\x08\x07\x06\x05\x04\x03\x02\x01", 0)]  # big-endian chunks


def _prefixes():
    return [(n, 0) for n in (b"abcdefghi", b"abcdefgh", b"abcdefg", b"abcdefghij", b"ab", b"abc", b"a", b"", b"abcdefgh0",
                             b"abcdefghijklmnopq", b"abcdefghijklmnop", b"abcdefghijklmno", b"ab\0", b"ab\0c", b"ab\1")]


def _high_bytes():
    names = [bytes([b]) + b"tail" for b in (0xff, 0x80, 0x7f, 0x81, 0x01, 0xfe, 0x41)]
    names += [b"same\xff", b"same\x7f", b"same\x80", b"same", b"\xff" * 9, b"\xff" * 8, b"\x80" * 17]
    return [(n, 0) for n in names]


def _skip_chunk():
    """24-byte names: chunks 0 and 2 the same in every row, chunk 1 differs (in two of its bytes)."""
    return [(b"AAAAAAAA" + b"mm%c%cmmmm" % (97 + (i * 7) % 5, 97 + (i * 3) % 4) + b"ZZZZZZZZ", 0) for i in range(40)]


def _tie16():
    """One name, the 16 combinations of READ1 / READ2 / SECONDARY / SUPPLEMENTARY, each twice."""
    g = _rng("tie16")
    flags = [(READ1 if k & 1 else 0) | (READ2 if k & 2 else 0) | (SECONDARY if k & 4 else 0) | (SUPPLEMENTARY if k & 8 else 0)
             for k in range(16)] * 2
    return [(b"read/one", flags[i] | (0x10 if j % 3 == 0 else 0)) for j, i in enumerate(g.permutation(32))]


N_PAIRS, N_SINGLE, N_TRIPLE = 1000, 37, 5


def _pairs():
    g = _rng("pairs")
    rows = [(b"pair%05d" % k, f) for k in range(N_PAIRS) for f in (READ1 | 1, READ2 | 1)]
    rows += [(b"single%04d" % k, 0) for k in range(N_SINGLE)]
    rows += [(b"triple%02d" % k, f) for k in range(N_TRIPLE) for f in (READ1 | 1, READ2 | 1, READ2 | 1 | SUPPLEMENTARY)]
    return [rows[i] for i in g.permutation(len(rows))]


def _in_order(rows):
    s = stream_of(rows)
    return [rows[int(i)] for i in perm_ref(s.flat, s.starts)]


N = 2 * T + 1
CORPORA = {}
for _n in (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
    CORPORA["edge_%d" % _n] = functools.partial(_random_rows, "edge_%d" % _n, _n)
CORPORA.update({
    "lengths": _lengths,
    "byte_edges": _byte_edges,
    "prefixes": _prefixes,
    "high_bytes": _high_bytes,
    "skip_chunk": _skip_chunk,
    "tie16": _tie16,
    "all_identical": lambda: [(b"the same name", READ1)] * 300,
    "pairs": _pairs,
    "sorted": lambda: _in_order(_random_rows("sorted", N)),
    "reverse_sorted": lambda: _in_order(_random_rows("sorted", N))[::-1],
    "shuffled": lambda: _random_rows("shuffled", N),
})
SMALL = tuple(CORPORA)

# what a case is built to give, beyond what info_ref computes for it
EXPECT = {
    "skip_chunk": dict(chunks_run=1, passes_run=2, max_name=24),
    "all_identical": dict(n_names=1, n_single=0, n_pair=0, n_more=1, already=True, chunks_run=0, passes_run=0),
    "tie16": dict(n_names=1, n_more=1, chunks_run=0, passes_run=1, already=False),
    "pairs": dict(n_names=N_PAIRS + N_SINGLE + N_TRIPLE, n_single=N_SINGLE, n_pair=N_PAIRS, n_more=N_TRIPLE),
    "sorted": dict(already=True, chunks_run=0, passes_run=0),
    "reverse_sorted": dict(already=False),
    "shuffled": dict(already=False),
    "lengths": dict(max_name=254, chunks_run=32),
    "edge_0": dict(n_names=0, already=True, max_name=0),
    "edge_1": dict(n_names=1, n_single=1, already=True),
}

# 43-byte records with 6-byte names: the fixed fields, the name and its NUL
GRID_DTYPE = np.dtype([("block_size", "<i4"), ("ref_id", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"),
                       ("mapq", "u1"), ("bin", "<u2"), ("n_cigar_op", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"),
                       ("next_ref_id", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "S7")])


@functools.lru_cache(maxsize=None)
def grid_stream():
    """GRID_ROWS rows, built vectorised: rows 2 j and 2 j + 1 are READ1 and READ2 of one 6-digit name,
    the names scattered over the stream's order (j -> 2654435761 j mod 10^6 is one-to-one below 10^6)."""
    i = np.arange(GRID_ROWS, dtype=np.int64)
    a = np.zeros(GRID_ROWS, GRID_DTYPE)
    a["block_size"] = GRID_DTYPE.itemsize - 4
    a["ref_id"], a["pos"], a["l_read_name"] = i % 3, i, 7
    a["mapq"], a["bin"], a["flag"] = i % 251, 4681, np.where(i % 2 == 0, READ1, READ2)
    a["next_ref_id"], a["next_pos"], a["tlen"] = -1, -1, i % 1000 - 500
    v = (i // 2 * 2654435761) % 10 ** 6
    digits = np.stack([(v // 10 ** k) % 10 + 48 for k in range(5, -1, -1)] + [np.zeros_like(v)], axis=1)
    a["name"] = np.ascontiguousarray(digits.astype(np.uint8)).view("S7")[:, 0]
    hdr = rc.header()
    return rc.Stream(hdr + a.tobytes(), len(hdr), len(hdr) + GRID_DTYPE.itemsize * i)


GRID_EXPECT = dict(n_names=GRID_ROWS // 2 + 1, n_single=1, n_pair=GRID_ROWS // 2, n_more=0, max_name=6, chunks_run=1,
                   passes_run=7, already=False)


@functools.lru_cache(maxsize=None)
def stream(name):
    return grid_stream() if name == "grid" else stream_of(CORPORA[name]())


@functools.lru_cache(maxsize=None)
def expected_perm(name):
    s = stream(name)
    return perm_ref(s.flat, s.starts)


@functools.lru_cache(maxsize=None)
def _expected_info(name, device):
    s = stream(name)
    return info_ref(s.flat, s.starts, device)


def expected_info(name, device=False):
    return dict(_expected_info(name, device))


def check_expect(name, info, device):
    """The written-down values of a case against an info dict (the host's leaves the device's two 0)."""
    want = GRID_EXPECT if name == "grid" else EXPECT.get(name, {})
    for k, v in want.items():
        assert info[k] == (0 if not device and k in ("chunks_run", "passes_run") else v), (name, k, info[k], v)


def driver_input(flat, starts):
    """The sanitizer driver's input file (tests/sanitize/name_sort_driver.cpp)."""
    return (struct.pack("<Q", len(flat)) + bytes(flat) + struct.pack("<Q", len(starts))
            + np.asarray(starts, "<u8").tobytes())
