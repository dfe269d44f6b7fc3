"""Hand-built inputs for the coordinate sort (sbh_bam_sort_host / sbh_records_bam_scan_order): record
streams whose keys are chosen, and the numpy restatement of the definition in
csrc/bam_sort_core.h -- keys from the fixed fields, then np.argsort(kind="stable").  That
restatement is the expected value everywhere (test infrastructure; plain Python, no GPU).

Records are record_corpus.rec's bytes: 44 of them each, built vectorised in record_corpus's
GRID_DTYPE (test_bam_sort_cpu.py pins rows against rec()), laid behind record_corpus.header().
The name holds the row index and mapq / tlen vary with it, so records of equal key differ and a
stream comparison sees a tie broken the wrong way.

SORT_TILE is the element count of a scatter tile (csrc/bam_sort_core.h; the CPU test reads the
header and holds this copy to it).
"""
import functools
import struct

import numpy as np

import record_corpus as rc

SORT_TILE = 2048
T = SORT_TILE
GRID_ROWS = rc.GRID_RECORDS  # one more than a full grid pass of the row kernels takes
REVERSE = 0x10


def stream_of(ref_id, pos, flag):
    """The Stream of records with the given fixed fields (arrays of one length)."""
    ref_id, pos, flag = (np.asarray(x, np.int64) for x in (ref_id, pos, flag))
    n = ref_id.size
    i = np.arange(n, dtype=np.int64)
    a = np.zeros(n, rc.GRID_DTYPE)
    a["block_size"] = rc.GRID_DTYPE.itemsize - 4
    a["ref_id"], a["pos"], a["l_read_name"] = ref_id, pos, 8
    a["mapq"], a["bin"], a["flag"] = i % 251, 4681, flag
    a["next_ref_id"], a["next_pos"], a["tlen"] = -1, -1, i % 1000 - 500
    digits = np.stack([(i // 10 ** k) % 10 + 48 for k in range(6, -1, -1)] + [np.zeros_like(i)], axis=1)
    a["name"] = np.ascontiguousarray(digits.astype(np.uint8)).view("S8")[:, 0] if n else b""
    hdr = rc.header()
    return rc.Stream(hdr + a.tobytes(), len(hdr), len(hdr) + rc.GRID_DTYPE.itemsize * i)


def keys_of(flat, starts):
    """The definition restated: uint64 keys of the records at starts."""
    flat = np.frombuffer(bytes(flat), np.uint8) if not isinstance(flat, np.ndarray) else flat
    st = np.asarray(starts, np.int64)
    if not st.size:
        return np.zeros(0, np.uint64)
    u32 = lambda o: sum(flat[st + o + k].astype(np.uint64) << np.uint64(8 * k) for k in range(4))  # noqa: E731
    ref_id, pos, flag = u32(4), u32(8), u32(16) >> np.uint64(16)
    ref = np.where(ref_id >= 2 ** 31, np.uint64(0x7FFFFFFF), ref_id)
    pos1 = (pos + np.uint64(1)) & np.uint64(0xFFFFFFFF)
    return ref << np.uint64(33) | pos1 << np.uint64(1) | (flag >> np.uint64(4)) & np.uint64(1)


def perm_ref(flat, starts):
    """perm[k] = the index into starts of the record that comes k-th."""
    return np.argsort(keys_of(flat, starts), kind="stable").astype(np.uint64)


def _rng(name):
    return np.random.default_rng(sum(name.encode()) * 7919 + len(name))


def _wide(name, n):
    """n keys in which every digit that can differ does: 31-bit references (-1 among them), 32-bit
    positions from -1 up, both strands."""
    g = _rng(name)
    ref = g.integers(0, 2 ** 31, n)
    ref[g.random(n) < 0.1] = -1
    return ref, g.integers(-1, 2 ** 31, n), REVERSE * g.integers(0, 2, n)


def _file_like(name, n, n_ref=25):
    """n keys as an aligner's output holds them: a few references, unplaced records among them."""
    g = _rng(name)
    ref = g.integers(0, n_ref, n)
    ref[g.random(n) < 0.05] = -1
    pos = g.integers(0, 2 ** 28, n)
    pos[ref < 0] = -1
    return ref, pos, REVERSE * g.integers(0, 2, n)


def _sorted_fields(n):
    ref, pos, flag = _file_like("sorted", n)
    order = np.argsort(keys_of(*stream_of(ref, pos, flag)[::2]), kind="stable")
    return ref[order], pos[order], flag[order]


N = 2 * T + 1
_i = np.arange(N, dtype=np.int64)
_z = np.zeros(N, np.int64)

CORPORA = {}
for _n in (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
    CORPORA["edge_%d" % _n] = functools.partial(_wide, "edge_%d" % _n, _n)
CORPORA.update({
    # stability
    "all_equal": lambda: (_z + 3, _z + 1000, _z),
    "two_alternating": lambda: (_z + 3, 2000 - 1000 * (_i % 2), _z),
    # one digit alone differs
    "only_reverse": lambda: (_z + 1, _z + 77, REVERSE * ((_i * 7 // 3) % 2)),
    "only_pos_low_byte": lambda: (_z + 1, 0x01020300 + (_i * 37) % 256 - 1, _z),  # pos + 1's low byte: key bits 1..8
    "only_pos_high_byte": lambda: (_z + 1, ((_i * 37) % 127 << 24) + 0x00ABCDEF, _z),
    "only_ref_high": lambda: (256 * ((_i * 2654435761) % (1 << 22)), _z + 5, _z),  # the passes real files skip
    # ends of the domain
    "unplaced_mixed": lambda: (np.where(_i % 3 == 0, -1, 4 - _i % 5), np.where(_i % 3 == 0, -1, (_i * 7919) % 100000), _z),
    "pos_minus_one": lambda: (_i % 2, np.where(_i % 4 < 2, -1, 0), REVERSE * (_i % 8 < 4)),
    "pos_max": lambda: (_i % 2, np.where(_i % 4 < 2, 2 ** 31 - 1, 2 ** 31 - 2), _z),
    # orders
    "sorted": lambda: _sorted_fields(N),
    "reverse_sorted": lambda: tuple(x[::-1].copy() for x in _sorted_fields(N)),
    "shuffled": lambda: _file_like("shuffled", N),
    # more rows than one grid pass of the row kernels
    "grid": lambda: _file_like("grid", GRID_ROWS),
})
SMALL = tuple(k for k in CORPORA if k != "grid")


@functools.lru_cache(maxsize=None)
def stream(name):
    return stream_of(*CORPORA[name]())


@functools.lru_cache(maxsize=None)
def expected_perm(name):
    s = stream(name)
    return perm_ref(s.flat, s.starts)


def sorted_ref(flat, starts, head=b"", keep=None):
    """(stream, rec_off, rows) of the coordinate-order call: `keep` = the scan rows the filter keeps
    (None: all), in scan order."""
    st = np.asarray(starts, np.int64)
    keep = np.arange(st.size) if keep is None else np.asarray(keep, np.int64)
    rows = keep[perm_ref(flat, st[keep]).astype(np.int64)] if keep.size else keep
    flat = bytes(flat)
    parts = [flat[int(st[r]):int(st[r]) + 4 + struct.unpack_from("<i", flat, int(st[r]))[0]] for r in rows]
    off = np.cumsum([len(head)] + [len(p) for p in parts]).astype(np.uint64)
    return bytes(head) + b"".join(parts), off, rows.astype(np.uint64)


def driver_input(flat, starts, head, so):
    """The sanitizer driver's input file (tests/sanitize/bam_sort_driver.cpp)."""
    return (struct.pack("<Q", len(flat)) + bytes(flat) + struct.pack("<Q", len(starts))
            + np.asarray(starts, "<u8").tobytes() + struct.pack("<Q", len(head)) + bytes(head)
            + struct.pack("<Q", len(so)) + bytes(so))


def header_with(text, pad=0, contigs=rc.CONTIGS):
    """BAM header bytes with the given text (+ pad NULs inside l_text) and rc's references."""
    t = text.encode() + b"\0" * pad
    out = b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(contigs))
    for n, ln in contigs:
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    return out


SQ = "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in rc.CONTIGS)
# (name, text, pad, the text expected for so = "coordinate")
HEADER_SHAPES = (
    ("so_present", "@HD\tVN:1.5\tSO:unsorted\n" + SQ, 0, "@HD\tVN:1.5\tSO:coordinate\n" + SQ),
    ("so_in_the_middle", "@HD\tVN:1.5\tSO:queryname\tGO:none\n" + SQ, 0, "@HD\tVN:1.5\tSO:coordinate\tGO:none\n" + SQ),
    ("hd_without_so", "@HD\tVN:1.4\n" + SQ, 0, "@HD\tVN:1.4\tSO:coordinate\n" + SQ),
    ("no_hd", SQ + "@CO\tSO:unsorted in a comment\n", 0, "@HD\tVN:1.6\tSO:coordinate\n" + SQ + "@CO\tSO:unsorted in a comment\n"),
    ("nul_padded", "@HD\tVN:1.5\tSO:unknown\n" + SQ, 5, "@HD\tVN:1.5\tSO:coordinate\n" + SQ),
    ("empty_text", "", 0, "@HD\tVN:1.6\tSO:coordinate\n"),
    ("hd_only_no_newline", "@HD\tVN:1.0", 0, "@HD\tVN:1.0\tSO:coordinate"),
)
