"""Hand-built inputs for the read-level statistics (sbh_stats_add_host / sbh_records_stats_add), and
the numpy restatement of the definition in csrc/stats_core.h: boolean masks over the fixed columns
read from the raw bytes, one flat array of (row, base index) pairs for the per-base tables, np.bincount
for the bins.  That restatement is the expected value everywhere (test infrastructure; plain Python,
no GPU).

Records are record_corpus.rec's bytes laid behind record_corpus.header(); the corpora of many rows
are built vectorised (GRID_DTYPE's fixed part, then SEQ and QUAL) and pinned against rec() by the CPU
test.  On the device row i of a scan is looked at by lane i % 64 of wave (i // 64) % 4 of workgroup
(i // 256) % 1024 of k_stats_rows, in pass i // 262144 of its grid-stride loop; k_stats_bases takes it in
the batch of 64 rows of wave (i // 64) % 16 of workgroup (i // 1024) % 512, in pass i // 524288, its
descriptor in lane i % 64, and walks it base by base, lane j % 64 taking base j (bases 0 .. 127 from
registers loaded a read ahead, the rest in a loop).

The constants below are the library's (csrc/stats_core.h; the CPU test reads the header and holds
these copies to it).
"""
import functools
import struct
from collections import namedtuple

import numpy as np

import record_corpus as rc

STAT_QUALS, STAT_SN = 94, 23
STAT_CYCLES_MAX, STAT_INSERT_MAX = 65536, 1 << 20
STAT_LDS_CYCLES, STAT_LDS_QUALS, STAT_LDS_MAX_READ = 160, 48, 65536
STAT_LDS_LENGTHS, STAT_LDS_INSERTS = 2048, 2048
GRID_PASS = 1024 * 256  # rows one pass of k_stats_rows' grid holds
BASES_PASS = 512 * 16 * 64  # rows one pass of k_stats_bases' grid holds
SN = ("sequences", "first_fragments", "last_fragments", "mapped", "unmapped", "paired", "properly_paired", "duplicates",
      "mq0", "qc_failed", "secondary", "supplementary", "total_length", "total_first_length", "total_last_length",
      "bases_mapped", "sum_quality", "no_qualities", "max_length", "pairs_inward", "pairs_outward", "pairs_other",
      "pairs_different_chr")
TABLES = ("sn", "read_len", "qual", "base", "gc", "isize", "mapq")
PAIRED, PROPER, UNMAP, MUNMAP, REVERSE, MREVERSE, READ1, READ2 = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80
SECONDARY, QCFAIL, DUP, SUPPLEMENTARY = 0x100, 0x200, 0x400, 0x800
FLAG_BITS = tuple(1 << k for k in range(12))
INT32_MIN = -2 ** 31

# flat bytes, record starts (any order, repeats allowed), the two parameters, the filter as
# records.record_filter's dict (None: all)
Case = namedtuple("Case", "flat starts cycles max_insert filter")


# ------------------------------------------------------------------------------ the restatement

def _u32(flat, at):
    at = np.asarray(at, np.int64)
    return sum(flat[at + k].astype(np.int64) << (8 * k) for k in range(4))


def _i32(flat, at):
    v = _u32(flat, at)
    return np.where(v >= 2 ** 31, v - 2 ** 32, v)


def shapes(cycles, max_insert):
    return {"sn": (STAT_SN,), "read_len": (cycles + 2,), "qual": (2, cycles + 1, STAT_QUALS), "base": (cycles + 1, 5),
            "gc": (2, 101), "isize": (max_insert + 1, 3), "mapq": (256,)}


def zeros(cycles, max_insert):
    return {k: np.zeros(s, np.uint64) for k, s in shapes(cycles, max_insert).items()}


def _hist(shape, index):
    """Counts of the index tuples, as a uint64 array of `shape`."""
    size = int(np.prod(shape))
    return np.bincount(np.ravel_multi_index(index, shape), minlength=size).astype(np.uint64).reshape(shape)


_CHANNEL = np.full(16, 4)
_CHANNEL[[1, 2, 4, 8]] = [0, 1, 2, 3]


def restate(flat, starts, cycles, max_insert, filter=None):
    """The definition restated.  Returns a dict: bad_row (None or the first bad row; no tables then),
    n, n_kept, n_counted and the seven tables (uint64, shapes())."""
    flat = np.frombuffer(bytes(flat), np.uint8) if not isinstance(flat, np.ndarray) else flat
    total = int(flat.size)
    st_u = np.asarray(starts, np.uint64)
    n = int(st_u.size)
    filter = filter or {}
    C, I = cycles, max_insert
    out = dict(zeros(C, I), bad_row=None, n=n, n_kept=0, n_counted=0)
    if not n:
        return out
    if total < 36:
        out["bad_row"] = 0
        return out
    fixed = st_u <= np.uint64(total - 36)
    p = np.where(fixed, st_u, np.uint64(0)).astype(np.int64)
    bsz, tid, pos, mtid, mpos, tlen = (_i32(flat, p + k) for k in (0, 4, 8, 24, 28, 32))
    l_name, mapq = flat[p + 12].astype(np.int64), flat[p + 13].astype(np.int64)
    w16, l_seq = _u32(flat, p + 16), _i32(flat, p + 20)
    n_cig, flag = w16 & 0xFFFF, w16 >> 16
    valid = fixed & (l_seq >= 0) & (bsz >= 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq) & (bsz + 4 <= total - p)
    if not valid.all():
        out["bad_row"] = int(np.flatnonzero(~valid)[0])
        return out
    keep = (flag & filter.get("flag_require", 0)) == filter.get("flag_require", 0)
    keep &= (flag & filter.get("flag_exclude", 0)) == 0
    keep &= mapq >= filter.get("min_mapq", 0)
    if filter.get("rows") is not None:
        in_rows = np.zeros(n, bool)
        for a, b in filter["rows"]:
            in_rows[a:b] = True
        keep &= in_rows
    sn = dict.fromkeys(SN, 0)
    sn["secondary"] = int((keep & ((flag & SECONDARY) != 0)).sum())
    sn["supplementary"] = int((keep & ((flag & SUPPLEMENTARY) != 0) & ((flag & SECONDARY) == 0)).sum())
    cnt = keep & ((flag & (SECONDARY | SUPPLEMENTARY)) == 0)
    f, q, t, mt, ps, mps, tl, L = (a[cnt] for a in (flag, mapq, tid, mtid, pos, mpos, tlen, l_seq))
    seq_at = (p + 36 + l_name + 4 * n_cig)[cnt]
    qual_at = seq_at + (L + 1) // 2
    on = lambda bit: (f & bit) != 0  # noqa: E731
    last = on(PAIRED) & on(READ2)
    mapped, rev = ~on(UNMAP), on(REVERSE)
    sn.update(sequences=int(f.size), first_fragments=int((~last).sum()), last_fragments=int(last.sum()),
              mapped=int(mapped.sum()), unmapped=int((~mapped).sum()), paired=int(on(PAIRED).sum()),
              properly_paired=int((on(PAIRED) & on(PROPER) & mapped).sum()), duplicates=int(on(DUP).sum()),
              mq0=int((mapped & (q == 0)).sum()), qc_failed=int(on(QCFAIL).sum()), total_length=int(L.sum()),
              total_first_length=int(L[~last].sum()), total_last_length=int(L[last].sum()), bases_mapped=int(L[mapped].sum()),
              max_length=int(L.max()) if L.size else 0,
              pairs_different_chr=int((on(PAIRED) & mapped & ~on(MUNMAP) & (t != mt) & on(READ1)).sum()))
    out["read_len"] = np.bincount(np.where(L <= C, L, C + 1), minlength=C + 2).astype(np.uint64)
    out["mapq"] = np.bincount(q[mapped], minlength=256).astype(np.uint64)
    # insert sizes
    pair = on(PAIRED) & mapped & ~on(MUNMAP) & (t == mt) & (t >= 0) & (tl > 0)
    left_rev = np.where(ps <= mps, rev, on(MREVERSE))
    col = np.where(rev == on(MREVERSE), 2, np.where(left_rev, 1, 0))
    out["isize"] = _hist((I + 1, 3), (np.minimum(tl, I)[pair], col[pair]))
    sn.update(pairs_inward=int(out["isize"][:, 0].sum()), pairs_outward=int(out["isize"][:, 1].sum()),
              pairs_other=int(out["isize"][:, 2].sum()))
    # the per-base tables: one entry per base of the counted rows
    has_seq = L > 0
    q0 = np.where(has_seq, flat[np.where(has_seq, qual_at, 0)], 0xFF)
    has_qual = has_seq & (q0 != 0xFF)
    sn["no_qualities"] = int((~has_qual).sum())
    row_of = np.repeat(np.arange(L.size), L)
    j = np.arange(int(L.sum())) - np.repeat(np.cumsum(L) - L, L)
    Lb, revb, wb = L[row_of], rev[row_of], last[row_of].astype(np.int64)
    byte = flat[seq_at[row_of] + j // 2].astype(np.int64)
    code = np.where(j % 2 == 0, byte >> 4, byte & 15)
    ch = _CHANNEL[code]
    ch = np.where(revb & (ch < 4), 3 - ch, ch)
    cyc = np.minimum(np.where(revb, Lb - 1 - j, j), C)
    out["base"] = _hist((C + 1, 5), (cyc, ch))
    qv = flat[qual_at[row_of] + j].astype(np.int64)
    hq = has_qual[row_of]
    out["qual"] = _hist((2, C + 1, STAT_QUALS), (wb[hq], cyc[hq], np.minimum(qv[hq], STAT_QUALS - 1)))
    sn["sum_quality"] = int(qv[hq].sum())
    g = np.bincount(row_of, weights=(code == 2) | (code == 4), minlength=L.size).astype(np.int64)
    out["gc"] = _hist((2, 101), (last[has_seq].astype(np.int64), 100 * g[has_seq] // L[has_seq]))
    out["noq_bases"] = [int(L[~has_qual & ~last].sum()), int(L[~has_qual & last].sum())]
    out["sn"] = np.array([sn[k] for k in SN], np.uint64)
    out["n_kept"], out["n_counted"] = int(keep.sum()), int(f.size)
    return out


def invariants(t, want=None):
    """The invariants stats_core.h states, on a set of tables (want: the restatement's dict, for the
    ones that need the no-quality rows' bases)."""
    sn = dict(zip(SN, (int(x) for x in t["sn"])))
    assert int(t["read_len"].sum()) == sn["sequences"] == sn["first_fragments"] + sn["last_fragments"]
    assert sn["sequences"] == sn["mapped"] + sn["unmapped"] and int(t["mapq"].sum()) == sn["mapped"]
    assert int(t["base"].sum()) == sn["total_length"] == sn["total_first_length"] + sn["total_last_length"]
    assert [int(t["isize"][:, k].sum()) for k in range(3)] == [sn["pairs_inward"], sn["pairs_outward"], sn["pairs_other"]]
    assert int(t["qual"].sum()) <= sn["total_length"] and int(t["gc"].sum()) <= sn["sequences"]
    if want is not None and "noq_bases" in want:
        for w, k in ((0, "total_first_length"), (1, "total_last_length")):
            assert int(t["qual"][w].sum()) + want["noq_bases"][w] == sn[k]
    if int(t["qual"][:, :, STAT_QUALS - 1].sum()) == 0:  # no quality above 92: the bins did not clamp
        assert int((t["qual"].sum(axis=(0, 1)) * np.arange(STAT_QUALS, dtype=np.uint64)).sum()) == sn["sum_quality"]


# ----------------------------------------------------------------------------------- builders

def codes(n, k0=1):
    return tuple((3 * k + k0) % 16 for k in range(n))


def quals(n, k0=0):
    """Every quality 0..93 within 94 bases, 47 and 48 among them."""
    return bytes((7 * k + k0) % 94 for k in range(n))


def one(L=10, flag=0, mapq=30, tid=0, mtid=-1, pos=100, mpos=-1, tlen=0, seq=None, qual=None, name=b"r", k0=0):
    seq = codes(L, 1 + k0) if seq is None else tuple(seq)
    qual = quals(len(seq), k0) if qual is None else bytes(qual)
    return rc.rec(tid, pos, mapq, 4681, flag, mtid, mpos, tlen, name, ((len(seq), rc.M),) if seq else (), seq, qual, b"")


def case(records, cycles=8, max_insert=16, filter=None, order=None):
    s = rc.lay(list(records))
    starts = list(s.starts) if order is None else [s.starts[i] for i in order]
    return Case(s.flat, starts, cycles, max_insert, filter)


def stream_dtype(L):
    return np.dtype(rc.GRID_DTYPE.descr + [("seq", "u1", ((L + 1) // 2,)), ("qual", "u1", (L,))])


def stream(n, L, flag, mapq=30, tid=0, mtid=0, pos=None, mpos=0, tlen=0, seq_byte=0x12, qual=30, cycles=8, max_insert=16,
           filter=None):
    """n records of L bases each, vectorised: rec(tid, pos, mapq, 4681, flag, mtid, mpos, tlen, b"r" padded to 8
    bytes by NULs, no CIGAR, the SEQ bytes seq_byte, the qualities qual); every argument a scalar or an array
    of n (seq_byte: n x ceil(L / 2), qual: n x L)."""
    dt = stream_dtype(L)
    a = np.zeros(n, dt)
    a["block_size"] = dt.itemsize - 4
    a["ref_id"], a["pos"], a["l_read_name"], a["mapq"], a["bin"] = tid, np.arange(n) if pos is None else pos, 8, mapq, 4681
    a["flag"], a["l_seq"], a["next_ref_id"], a["next_pos"], a["tlen"], a["name"] = flag, L, mtid, mpos, tlen, b"r"
    a["seq"], a["qual"] = seq_byte, qual
    hdr = rc.header()
    return Case(hdr + a.tobytes(), (len(hdr) + dt.itemsize * np.arange(n)).tolist(), cycles, max_insert, filter)


def mixed(n, seed, cycles=8, max_insert=16, filter=None, max_len=40):
    """n rows of arbitrary flags, lengths, bases, qualities, mates and insert sizes."""
    r = np.random.RandomState(seed)
    recs = []
    for _ in range(n):
        L = int(r.randint(0, max_len + 1))
        q = r.randint(0, 100, L).astype(np.uint8)
        if L and r.randint(0, 8) == 0:
            q[0] = 0xFF
        recs.append(one(flag=int(r.randint(0, 4096)), mapq=int(r.randint(0, 61)), tid=int(r.randint(-1, 3)),
                        mtid=int(r.randint(-1, 3)), pos=int(r.randint(0, 50)), mpos=int(r.randint(0, 50)),
                        tlen=int(r.randint(-5, max_insert + 5)), seq=r.randint(0, 16, L).tolist(), qual=q.tobytes()))
    return case(recs, cycles, max_insert, filter)


def _reordered(c, order):
    return c._replace(starts=[c.starts[i] for i in order])


_LENGTHS_8 = (0, 1, 2, 7, 8, 9, 24, 63, 64, 65, 127, 128, 129)
# around the LDS window's last row (159 | 160), cycles (199, 200, 201), three times cycles
_LENGTHS_200 = (0, 1, 63, 64, 65, 127, 128, 129, 159, 160, 161, 199, 200, 201, 600)


def _lengths(ls, cycles):
    """Every length forward and reverse, as first and as last fragment."""
    return case([one(L, fl, k0=k) for k, L in enumerate(ls) for fl in (0, REVERSE, PAIRED | READ2, PAIRED | READ2 | REVERSE)],
                cycles)


def _qualities():
    edge = bytes((0, 47, 48, 92, 93, 94, 254, 255, 46, 49))
    return case([one(qual=edge), one(qual=edge, flag=REVERSE), one(qual=edge, flag=PAIRED | READ2),
                 one(qual=b"\xff" + edge[1:]), one(qual=b"\xff" * 10, flag=PAIRED | READ2 | REVERSE),  # no qualities
                 one(qual=b"\x00" + b"\xff" * 9),                                                      # 0xff only later
                 one(0), one(0, PAIRED | READ2), one(1, qual=b"\xff"), one(1, qual=b"\x5d")], 8)


def _insert_sizes(I=16):
    P = PAIRED
    recs = [one(flag=P, mtid=0, tlen=t, mpos=200) for t in (0, 1, I - 1, I, I + 1, -5, INT32_MIN, 2 ** 31 - 1)]
    # the three orders of pos and mpos with each strand combination
    recs += [one(flag=P | s, mtid=0, pos=a, mpos=b, tlen=5) for s in (0, REVERSE, MREVERSE, REVERSE | MREVERSE)
             for a, b in ((100, 200), (100, 100), (200, 100))]
    recs += [one(flag=P, tid=0, mtid=1, tlen=5), one(flag=P | READ1, tid=0, mtid=1, tlen=5), one(flag=P | READ1, tid=1, mtid=0),
             one(flag=P | READ1 | UNMAP, tid=0, mtid=1), one(flag=P | READ1 | MUNMAP, tid=0, mtid=1), one(flag=READ1, tid=0, mtid=1),
             one(flag=P, tid=-1, mtid=-1, tlen=5), one(flag=P | UNMAP, mtid=0, tlen=5), one(flag=P | MUNMAP, mtid=0, tlen=5),
             one(flag=0, mtid=0, tlen=5), one(flag=P | SECONDARY, mtid=0, tlen=5), one(flag=P, tid=3, mtid=3, tlen=3, mpos=0)]
    return case(recs, 8, I)


def _large():
    """More rows than a pass of either grid; 11 bases a read against 8 cycles: three bases of every read in
    the overflow row, more than a million adds into the cells of one quality."""
    n = BASES_PASS + 37
    i = np.arange(n)
    fl = np.where(i % 2 == 1, REVERSE, 0) | np.where(i % 3 == 0, PAIRED | READ2, PAIRED | READ1) | np.where(i % 11 == 0, UNMAP, 0)
    fl |= np.where(i % 13 == 0, SECONDARY, 0) | np.where(i % 17 == 0, MREVERSE, 0)
    q = np.full((n, 11), 30)
    q[:, 3] = i % 50
    q[i % 1000 == 7, 0] = 0xFF
    seq = np.stack([(0x12, 0x48, 0x1F, 0x84, 0x21, 0x80)[k] + 0 * i for k in range(6)], axis=1)
    seq[:, 2] = np.where(i % 4 == 0, 0x24, 0x1F)
    return stream(n, 11, fl, mapq=i % 61, tid=i % 3, mtid=(i // 5) % 3, mpos=(i * 7) % n, tlen=i % 23 - 3, seq_byte=seq, qual=q)


CORPORA = {
    "lengths_cycles_8": lambda: _lengths(_LENGTHS_8, 8),
    "lengths_cycles_200": lambda: _lengths(_LENGTHS_200, 200),
    # cycles below, at and above the LDS window's rows: the overflow row inside and outside the window
    "lengths_cycles_159": lambda: _lengths((158, 159, 160, 161, 500), 159),
    "lengths_cycles_160": lambda: _lengths((159, 160, 161, 162, 500), 160),
    "lengths_cycles_1": lambda: _lengths((0, 1, 2, 3, 65), 1),
    "qualities": _qualities,
    # every 4-bit code in every position parity, forward and reverse, odd and even lengths
    "base_codes": lambda: case([one(seq=tuple((k + s) % 16 for k in range(L)), flag=fl)
                                for L in (16, 17) for s in (0, 1, 5) for fl in (0, REVERSE)], 32),
    "odd_length_spare_nibble": lambda: case([rc.rec(0, 1, 30, 4681, fl, -1, -1, 0, b"r", (), (2, 4, 2), b"\x10\x20\x30", b"", spare=s)
                                             for fl in (0, REVERSE) for s in (0, 2, 15)]),
    "which": lambda: case([one(5 + k, fl) for k, fl in enumerate((0, PAIRED, READ1, READ2, READ1 | READ2, PAIRED | READ1,
                                                                  PAIRED | READ2, PAIRED | READ1 | READ2))]),
    "flag_bits": lambda: case([one(flag=f, mapq=m) for f in (0,) + FLAG_BITS for m in (0, 30)]),
    "secondary_and_supplementary": lambda: case([one(flag=f, mtid=0, tlen=4) for f in (
        SECONDARY, SUPPLEMENTARY, SECONDARY | SUPPLEMENTARY, SECONDARY | PAIRED | READ2, SUPPLEMENTARY | UNMAP, 0, PAIRED)]),
    "insert_sizes": _insert_sizes,
    # bins on both sides of k_stats_rows' LDS windows, and the last ones
    "long_inserts_and_lengths": lambda: case([one(flag=PAIRED | MREVERSE, mtid=0, tlen=t, mpos=300) for t in (2047, 2048, 2049, 4999, 5000, 5001)]
                                             + [one(L) for L in (2046, 2047, 2048, 2999, 3000, 3001)], 3000, 5000),
    "mapq_values": lambda: case([one(mapq=m, flag=f) for m in (0, 1, 254, 255) for f in (0, UNMAP)]),
    # reads at the length that bypasses the LDS window, and one below it
    "read_of_65536": lambda: case([one(65535, REVERSE), one(65536, PAIRED | READ2), one(65537)], 200, 16),
    "filter_require": lambda: mixed(300, 7, filter={"flag_require": PAIRED | READ1}),
    "filter_exclude": lambda: mixed(300, 8, filter={"flag_exclude": 0x704}),
    "filter_mapq": lambda: mixed(300, 9, filter={"min_mapq": 30}),
    "filter_rows": lambda: mixed(300, 10, filter={"rows": [(5, 50), (100, 130), (299, 300)]}),
    "filter_rows_nothing_kept": lambda: mixed(100, 11, filter={"rows": []}),
    "mixed_cycles_200": lambda: mixed(200, 12, 200, 16, max_len=400),
    "rows_reversed": lambda: _reordered(mixed(200, 13), range(199, -1, -1)),
    "row_given_three_times": lambda: _reordered(mixed(200, 14), list(range(200)) + [7, 7]),
}
for _n in (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257):
    CORPORA["rows_%d" % _n] = functools.partial(lambda n: mixed(n, 100 + n), _n)
# one row fewer than, exactly and one more than the batches of one workgroup of k_stats_bases
for _n in (1023, 1024, 1025):
    CORPORA["rows_%d" % _n] = functools.partial(lambda n: stream(n, 3, np.arange(n) % 2 * REVERSE, seq_byte=0x24,
                                                                 qual=np.arange(n)[:, None] % 94 + np.zeros((1, 3), int)), _n)
CORPORA["large"] = _large
LARGE = ("large",)
SMALL = tuple(k for k in CORPORA if k not in LARGE)


@functools.lru_cache(maxsize=None)
def get(name):
    return CORPORA[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    c = get(name)
    return restate(c.flat, c.starts, c.cycles, c.max_insert, c.filter)


def in_file_order(c):
    return list(c.starts) == sorted(set(c.starts))


def tables_equal(got, want):
    for k in TABLES:
        assert got[k].dtype == np.uint64 and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:5].tolist())


def added(a, b):
    """The tables of two adds: sums, and the larger max_length."""
    out = {k: a[k] + b[k] for k in TABLES}
    out["sn"][SN.index("max_length")] = max(a["sn"][SN.index("max_length")], b["sn"][SN.index("max_length")])
    return out


def driver_input(flat, starts, cycles, max_insert, filter=None):
    """The sanitizer driver's input file (tests/sanitize/stats_driver.cpp)."""
    f = filter or {}
    rows = f.get("rows")
    if rows is not None and not rows:  # no rows asked for: one range no row lies in (records.record_filter's)
        rows = [(2 ** 64 - 2, 2 ** 64 - 1)]
    rows = rows or []
    return (struct.pack("<Q", len(flat)) + bytes(flat) + struct.pack("<Q", len(starts))
            + np.asarray(starts, "<u8").tobytes()
            + struct.pack("<IIIIi", cycles, max_insert, f.get("flag_require", 0), f.get("flag_exclude", 0), f.get("min_mapq", 0))
            + struct.pack("<Q", len(rows)) + np.asarray([a for a, _ in rows], "<u8").tobytes()
            + np.asarray([b for _, b in rows], "<u8").tobytes())
