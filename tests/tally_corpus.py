"""Hand-built inputs for the flag counts and per-reference read counts (sbh_tally_add_host /
sbh_records_tally_add), and the numpy restatement of the definition in csrc/tally_core.h: boolean
masks over the flag, mapq, tid and mtid columns read from the raw bytes, np.bincount for the bins.
That restatement is the expected value everywhere (test infrastructure; plain Python, no GPU).

Records are record_corpus.rec's bytes laid behind record_corpus.header(); the corpora whose rows
must sit on particular lanes of a wave are built vectorised from record_corpus.GRID_DTYPE (44-byte
records) and pinned against rec() by the CPU test.  Row i of a scan is looked at by lane i % 64 of
wave (i // 64) % 4 of workgroup (i // 256) % 1024, in pass i // 262144 of the grid-stride loop.

TALLY_LDS_BINS is the library's (csrc/tally_core.h; the CPU test reads the header and holds this
copy to it).
"""
import functools
import struct
from collections import namedtuple

import numpy as np

import record_corpus as rc

TALLY_ROWS = 16
TALLY_LDS_BINS = 2048
GRID_PASS = 1024 * 256  # rows one pass of k_tally_rows' grid holds
N_REF = len(rc.CONTIGS)
PAIRED, PROPER, UNMAP, MUNMAP, REVERSE, MREVERSE, READ1, READ2 = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80
SECONDARY, QCFAIL, DUP, SUPPLEMENTARY = 0x100, 0x200, 0x400, 0x800
FLAG_BITS = tuple(1 << k for k in range(12))

# flat bytes, record starts (any order, repeats allowed), the number of references, the filter as
# records.record_filter's dict (None: all)
Case = namedtuple("Case", "flat starts n_ref filter")


# ------------------------------------------------------------------------------ the restatement

def _u32(flat, at):
    at = np.asarray(at, np.int64)
    return sum(flat[at + k].astype(np.int64) << (8 * k) for k in range(4))


def _i32(flat, at):
    v = _u32(flat, at)
    return np.where(v >= 2 ** 31, v - 2 ** 32, v)


def restate(flat, starts, n_ref, filter=None):
    """The definition restated.  Returns a dict: bad_row (None or the first bad row; nothing else
    then), n, n_kept, flag (uint64[16, 2]), ref (uint64[n_ref + 1, 2])."""
    flat = np.frombuffer(bytes(flat), np.uint8) if not isinstance(flat, np.ndarray) else flat
    total = int(flat.size)
    st_u = np.asarray(starts, np.uint64)
    n = int(st_u.size)
    filter = filter or {}
    out = {"bad_row": None, "n": n, "n_kept": 0, "flag": np.zeros((TALLY_ROWS, 2), np.uint64),
           "ref": np.zeros((n_ref + 1, 2), np.uint64)}
    if not n:
        return out
    if total < 36:
        out["bad_row"] = 0
        return out
    fixed = st_u <= np.uint64(total - 36)
    p = np.where(fixed, st_u, np.uint64(0)).astype(np.int64)
    bsz, tid, mtid = _i32(flat, p), _i32(flat, p + 4), _i32(flat, p + 24)
    l_name, mapq = flat[p + 12].astype(np.int64), flat[p + 13].astype(np.int64)
    w16, l_seq = _u32(flat, p + 16), _i32(flat, p + 20)
    n_cig, flag = w16 & 0xFFFF, w16 >> 16
    valid = fixed & (l_seq >= 0) & (bsz >= 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq) & (bsz + 4 <= total - p)
    keep = valid & ((flag & filter.get("flag_require", 0)) == filter.get("flag_require", 0))
    keep &= (flag & filter.get("flag_exclude", 0)) == 0
    keep &= mapq >= filter.get("min_mapq", 0)
    if filter.get("rows") is not None:
        in_rows = np.zeros(n, bool)
        for a, b in filter["rows"]:
            in_rows[a:b] = True
        keep &= in_rows
    bad = ~valid | (keep & (tid >= n_ref))
    if bad.any():
        out["bad_row"] = int(np.flatnonzero(bad)[0])
        return out
    f, q, t, mt = flag[keep], mapq[keep], tid[keep], mtid[keep]
    on = lambda bit: (f & bit) != 0  # noqa: E731
    fail = on(QCFAIL)
    sec = on(SECONDARY)
    sup = on(SUPPLEMENTARY) & ~sec
    prim = ~sec & ~sup
    mapped = ~on(UNMAP)
    paired = prim & on(PAIRED)
    both = paired & mapped & ~on(MUNMAP)
    diff = both & (mt != t)
    masks = [np.ones(f.size, bool), prim, sec, sup, on(DUP), prim & on(DUP), mapped, prim & mapped, paired,
             paired & on(READ1), paired & on(READ2), paired & on(PROPER) & mapped, both, paired & on(MUNMAP) & mapped,
             diff, diff & (q >= 5)]
    out["flag"] = np.array([[int((m & ~fail).sum()), int((m & fail).sum())] for m in masks], np.uint64)
    bins = np.where(t < 0, n_ref, t)
    out["ref"] = np.stack([np.bincount(bins[mapped], minlength=n_ref + 1),
                           np.bincount(bins[~mapped], minlength=n_ref + 1)], axis=1).astype(np.uint64)
    out["n_kept"] = int(f.size)
    return out


# ----------------------------------------------------------------------------------- builders

def one(tid=0, flag=0, mapq=30, mtid=-1, pos=100, name=b"r"):
    return rc.rec(tid, pos, mapq, 4681, flag, mtid, -1, 0, name, ((10, rc.M),), (), b"", b"")


def case(records, n_ref=N_REF, filter=None, order=None):
    s = rc.lay(list(records))
    starts = list(s.starts) if order is None else [s.starts[i] for i in order]
    return Case(s.flat, starts, n_ref, filter)


def stream(tid, flag=0, mapq=30, mtid=-1, n_ref=N_REF, filter=None):
    """One 44-byte record per entry of `tid` (rec(tid, i, mapq, 4681, flag, mtid, -1, 0, b"r", (), ...) with the
    name padded to 8 bytes by NULs), vectorised: row i is the i-th record."""
    tid = np.asarray(tid, np.int64)
    a = np.zeros(tid.size, rc.GRID_DTYPE)
    a["block_size"] = rc.GRID_DTYPE.itemsize - 4
    a["ref_id"], a["pos"], a["l_read_name"], a["mapq"], a["bin"] = tid, np.arange(tid.size), 8, mapq, 4681
    a["flag"], a["next_ref_id"], a["next_pos"], a["name"] = flag, mtid, -1, b"r"
    hdr = rc.header()
    return Case(hdr + a.tobytes(), (len(hdr) + rc.GRID_DTYPE.itemsize * np.arange(tid.size)).tolist(), n_ref, filter)


def mixed(n, n_ref, seed, filter=None, lowest=-2):
    """n rows of arbitrary flags, mapq 0..60 and references lowest..n_ref - 1, mates likewise."""
    r = np.random.RandomState(seed)
    pick = lambda: np.minimum(r.randint(lowest, max(n_ref, lowest + 1), n), n_ref - 1)  # noqa: E731
    return stream(pick(), r.randint(0, 4096, n), r.randint(0, 61, n), pick(), n_ref, filter)


def _lanes(n, where, then=1, other=0):
    """n rows of reference `other`, the rows of `where` on reference `then`."""
    t = np.full(n, other)
    t[list(where)] = then
    return t


def _reordered(c, order):
    return Case(c.flat, [c.starts[i] for i in order], c.n_ref, c.filter)


def _three_rounds():
    """Wave 0 of workgroup 0 meets reference 0 in its first pass, 1 in its second, 0 again in its third;
    every other row sits on reference 2 or, every seventh, on none."""
    n = 2 * GRID_PASS + 101
    t = np.where(np.arange(n) % 7 == 0, -1, 2)
    t[0:64], t[GRID_PASS:GRID_PASS + 64], t[2 * GRID_PASS:2 * GRID_PASS + 64] = 0, 1, 0
    return stream(t, np.where(np.arange(n) % 5 == 0, UNMAP | PAIRED, PAIRED | READ1), 30, np.where(np.arange(n) % 3, 2, 1))


def _grid():
    s = rc.grid_stream()[0]
    return Case(s.flat, s.starts.tolist(), N_REF, None)


_PAIR = PAIRED | PROPER | READ1 | READ2
_BIG = 200000
CORPORA = {
    # each of the 12 flag bits alone and flag 0, then each bit together with QC-fail
    "flag_bits": lambda: case([one(flag=f) for f in (0,) + FLAG_BITS] + [one(flag=f | QCFAIL) for f in FLAG_BITS]),
    # both bits: secondary only; and neither kind of non-primary row adds to the pair rows
    "secondary_and_supplementary": lambda: case([one(flag=f) for f in (
        SECONDARY | SUPPLEMENTARY, SECONDARY, SUPPLEMENTARY, SECONDARY | _PAIR, SUPPLEMENTARY | _PAIR,
        SECONDARY | SUPPLEMENTARY | _PAIR, SECONDARY | DUP, SUPPLEMENTARY | DUP | QCFAIL, SECONDARY | UNMAP)]),
    "pair_rows": lambda: case([one(flag=f) for f in (
        PAIRED | PROPER | UNMAP, PAIRED | PROPER, PAIRED | MUNMAP, PAIRED | MUNMAP | UNMAP, PAIRED, PAIRED | READ1,
        PAIRED | READ2, PAIRED | READ1 | READ2, PROPER | READ1, PAIRED | UNMAP, PAIRED | PROPER | MUNMAP | QCFAIL)]),
    # row 14 and 15: the mate elsewhere at mapq 4 and 5; no mate reference; neither has one
    "mate_chr": lambda: case([one(0, PAIRED, 4, 1), one(0, PAIRED, 5, 1), one(0, PAIRED, 30, -1), one(-1, PAIRED, 30, -1),
                              one(1, PAIRED, 255, 0), one(1, PAIRED, 0, 1), one(0, PAIRED | UNMAP, 30, 1),
                              one(0, PAIRED | MUNMAP, 30, 1), one(0, 0, 30, 1), one(0, PAIRED | QCFAIL, 5, 3),
                              one(0, PAIRED | SECONDARY, 30, 1), one(2, PAIRED, 5, 99)]),
    "tid_values": lambda: case([one(-1), one(-7), one(-1, UNMAP), one(-7, UNMAP | QCFAIL), one(0), one(0, UNMAP),
                                one(N_REF - 1), one(N_REF - 1, UNMAP), one(-2 ** 31), one(1, DUP)]),
    # a row off the references that the filter drops is no error
    "tid_n_ref_filtered_out": lambda: case([one(0), one(N_REF, DUP), one(2 ** 31 - 1, DUP | UNMAP), one(1)],
                                           filter={"flag_exclude": DUP}),
    "n_ref_0": lambda: mixed(300, 0, 1, lowest=-3),
    "n_ref_1": lambda: mixed(300, 1, 2),
    "n_ref_2": lambda: mixed(300, 2, 3),
    # 2 (n_ref + 1) counters two below, at and two above the LDS budget: every bin in use, the last ones too
    "lds_below": lambda: mixed(3000, TALLY_LDS_BINS // 2 - 2, 4),
    "lds_exact": lambda: mixed(3000, TALLY_LDS_BINS // 2 - 1, 5),
    "lds_above": lambda: mixed(3000, TALLY_LDS_BINS // 2, 6),
    "lds_exact_last_bins": lambda: stream(np.tile([TALLY_LDS_BINS // 2 - 2, -1, 0], 100), np.tile([0, UNMAP], 150),
                                          n_ref=TALLY_LDS_BINS // 2 - 1),
    # the first wave mixes bins 0, the last and `*`; the next three hold one each
    "n_ref_200000": lambda: stream(np.concatenate((np.tile([0, _BIG - 1, -1], 22)[:64], np.full(64, _BIG - 1), np.full(64, -1),
                                                   np.full(70, 0))), np.tile([0, UNMAP, PAIRED], 88)[:262], n_ref=_BIG),
    "wave_one_bin": lambda: stream(np.full(64, 2), np.tile([0, UNMAP, PAIRED | QCFAIL, DUP], 16)),
    "wave_alternating": lambda: stream(np.arange(256) % 2, np.tile([0, 0, UNMAP], 86)[:256]),
    "wave_change_after_lane_0": lambda: stream(_lanes(64, range(1, 64))),
    "wave_change_after_lane_31": lambda: stream(_lanes(64, range(32, 64))),
    "wave_change_after_lane_62": lambda: stream(_lanes(64, [63])),
    "wave_only_lane_63_kept": lambda: stream(_lanes(64, [63], 1, 3), np.where(np.arange(64) == 63, REVERSE, 0),
                                             filter={"flag_require": REVERSE}),
    # waves 0 and 2 on different bins with no row of wave 1 kept; then three waves on three bins
    "wave_nothing_kept_between": lambda: stream(np.repeat([0, 3, 1, 0, 2, 1], 64), np.repeat([0, DUP, 0, UNMAP, 0, 0], 64),
                                                filter={"flag_exclude": DUP}),
    # the dropped lanes of a wave sit on another bin than its kept lanes
    "wave_dropped_on_other_bin": lambda: stream(np.where(np.arange(128) % 3 == 0, 2, 1),
                                                np.where(np.arange(128) % 3 == 0, DUP, np.arange(128) % 2 * UNMAP),
                                                filter={"flag_exclude": DUP}),
    "filter_require": lambda: mixed(500, N_REF, 7, {"flag_require": PAIRED | READ1}),
    "filter_exclude": lambda: mixed(500, N_REF, 8, {"flag_exclude": 0x704}),
    "filter_mapq": lambda: mixed(500, N_REF, 9, {"min_mapq": 30}),
    "filter_rows": lambda: mixed(500, N_REF, 10, {"rows": [(5, 50), (100, 130), (499, 500)]}),
    "filter_rows_nothing_kept": lambda: mixed(500, N_REF, 11, {"rows": []}),
    "filter_rows_one_per_wave": lambda: mixed(512, N_REF, 12, {"rows": [(64 * w + (5 * w) % 64, 64 * w + (5 * w) % 64 + 1)
                                                                        for w in range(8)]}),
    "rows_reversed": lambda: _reordered(mixed(200, N_REF, 13), range(199, -1, -1)),
    "row_given_three_times": lambda: _reordered(mixed(200, N_REF, 14), list(range(200)) + [7, 7]),
}
for _n in (0, 1, 63, 64, 65, 255, 256, 257):
    CORPORA["rows_%d" % _n] = functools.partial(lambda n: mixed(n, N_REF, 100 + n), _n)
# more rows than one pass of the grid, and a wave that meets a bin again two passes later
CORPORA["grid"] = _grid
CORPORA["grid_three_rounds"] = _three_rounds
LARGE = ("grid", "grid_three_rounds")
SMALL = tuple(k for k in CORPORA if k not in LARGE)
# a kept row on reference n_ref: SBH_E_BAD_RECORD {2}
TID_KEPT = lambda: case([one(0), one(N_REF - 1), one(N_REF), one(1)])  # noqa: E731


@functools.lru_cache(maxsize=None)
def get(name):
    return CORPORA[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    c = get(name)
    return restate(c.flat, c.starts, c.n_ref, c.filter)


def in_file_order(c):
    return list(c.starts) == sorted(set(c.starts))


def driver_input(flat, starts, n_ref, filter=None):
    """The sanitizer driver's input file (tests/sanitize/tally_driver.cpp)."""
    f = filter or {}
    rows = f.get("rows")
    if rows is not None and not rows:  # no rows asked for: one range no row lies in (records.record_filter's)
        rows = [(2 ** 64 - 2, 2 ** 64 - 1)]
    rows = rows or []
    return (struct.pack("<Q", len(flat)) + bytes(flat) + struct.pack("<Q", len(starts))
            + np.asarray(starts, "<u8").tobytes()
            + struct.pack("<iIIi", n_ref, f.get("flag_require", 0), f.get("flag_exclude", 0), f.get("min_mapq", 0))
            + struct.pack("<Q", len(rows)) + np.asarray([a for a, _ in rows], "<u8").tobytes()
            + np.asarray([b for _, b in rows], "<u8").tobytes())
