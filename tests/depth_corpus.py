"""Hand-built inputs for per-base depth (sbh_depth_add_host / sbh_records_depth_add and the two
finishes), and the numpy restatement of the definition in csrc/depth_core.h: per-op intervals from
the raw bytes, np.add.at on a difference array, np.cumsum, runs by np.flatnonzero(np.diff(...)).
That restatement is the expected value everywhere (test infrastructure; plain Python, no GPU).

Records are record_corpus.rec's bytes laid behind record_corpus.header() (four references); the
large corpora are built vectorised from one dtype and pinned against rec() by the CPU test.

DEPTH_TILE and DEPTH_LANE_OPS are the library's (csrc/depth_core.h; the CPU test reads the header
and holds these copies to it).
"""
import functools
import struct
from collections import namedtuple

import numpy as np

import record_corpus as rc

DEPTH_TILE = 4096
DEPTH_LANE_OPS = 16
T, L = DEPTH_TILE, DEPTH_LANE_OPS
N_REF = len(rc.CONTIGS)
POS_MAX = 2 ** 31 - 1
M, I, D, N, S, H, P, EQ, X = range(9)
SPAN_DTYPE = np.dtype([("ref_id", "<i4"), ("pad", "<i4"), ("beg", "<i8"), ("end", "<i8")])
RUN_DTYPE = np.dtype([("ref_id", "<i4"), ("depth", "<u4"), ("beg", "<i8"), ("end", "<i8")])

# flat bytes, record starts (any order, repeats allowed), spans [(ref_id, beg, end)], the filter as
# records.record_filter's dict (None: all), D covers
Case = namedtuple("Case", "flat starts spans filter count_del")


# ------------------------------------------------------------------------------ the restatement

def slots_of(spans):
    return sum(e - b + 1 for _, b, e in spans)


def _u32(flat, at):
    at = np.asarray(at, np.int64)
    return sum(flat[at + k].astype(np.int64) << (8 * k) for k in range(4))


def _i32(flat, at):
    v = _u32(flat, at)
    return np.where(v >= 2 ** 31, v - 2 ** 32, v)


def restate(flat, starts, spans, n_ref=N_REF, filter=None, count_del=False):
    """The definition restated.  Returns a dict: bad_row (None or the first bad row; nothing else
    then), add (n, n_kept, n_counted, n_unplaced, cov_bases), diff (int64 per slot), depth (uint32
    per slot, extra slots included), runs (RUN_DTYPE), stats (slots, n_runs, covered, sum,
    max_depth)."""
    flat = np.frombuffer(bytes(flat), np.uint8) if not isinstance(flat, np.ndarray) else flat
    total = int(flat.size)
    st_u = np.asarray(starts, np.uint64)
    n = int(st_u.size)
    filter = filter or {}
    S = slots_of(spans)
    out = {"bad_row": None, "add": dict(n=n, n_kept=0, n_counted=0, n_unplaced=0, cov_bases=0)}
    diff = np.zeros(S, np.int64)
    if n:
        fixed = st_u <= np.uint64(total - 36) if total >= 36 else np.zeros(n, bool)
        p = np.where(fixed, st_u, np.uint64(0)).astype(np.int64)
        if total < 36:
            out["bad_row"] = 0
            return out
        bsz, ref, pos = _i32(flat, p), _i32(flat, p + 4), _i32(flat, p + 8)
        l_name, mapq = flat[p + 12].astype(np.int64), flat[p + 13].astype(np.int64)
        w16, l_seq = _u32(flat, p + 16), _i32(flat, p + 20)
        n_cig, flag = w16 & 0xFFFF, w16 >> 16
        valid = fixed & (l_seq >= 0) & (bsz >= 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq) & (bsz + 4 <= total - p)
        keep = valid & ((flag & filter.get("flag_require", 0)) == filter.get("flag_require", 0))
        keep &= (flag & filter.get("flag_exclude", 0)) == 0
        keep &= mapq >= filter.get("min_mapq", 0)
        if filter.get("rows") is not None:
            row = np.arange(n)
            keep &= np.any([(row >= a) & (row < b) for a, b in filter["rows"]] or [np.zeros(n, bool)], axis=0)
        # every op of every kept row, flattened: row index, address of the word
        kr = np.flatnonzero(keep)
        nc = n_cig[kr]
        first = np.concatenate(([0], np.cumsum(nc)))[:-1]
        of_row = np.repeat(np.arange(kr.size), nc)
        k = np.arange(int(nc.sum())) - np.repeat(first, nc)
        w = _u32(flat, (p[kr] + 36 + l_name[kr])[of_row] + 4 * k) if of_row.size else np.zeros(0, np.int64)
        ln, op = w >> 4, w & 15
        bad = ~valid
        bad[kr[ref[kr] >= n_ref]] = True
        bad[kr[np.unique(of_row[op > 8])]] = True
        if bad.any():
            out["bad_row"] = int(np.flatnonzero(bad)[0])
            return out
        adv = np.where(np.isin(op, (M, D, N, EQ, X)), ln, 0)
        before = np.cumsum(adv) - adv  # exclusive, over all rows; minus the value at the row's first op
        x = pos[kr][of_row] + before - before[np.repeat(first, nc)]
        covers = np.isin(op, (M, EQ, X)) | ((op == D) & bool(count_del))
        span_of = np.full(n_ref, -1, np.int64)
        for j, (r, _, _) in enumerate(spans):
            span_of[r] = j
        sp_beg = np.asarray([b for _, b, _ in spans], np.int64)
        sp_end = np.asarray([e for _, _, e in spans], np.int64)
        sp_off = np.concatenate(([0], np.cumsum(sp_end - sp_beg + 1)))[:-1]
        placed = ref[kr] >= 0
        row_span = np.where(placed, span_of[np.where(placed, ref[kr], 0)], -1)
        j = row_span[of_row]
        a = np.maximum(x, sp_beg[j])
        b = np.minimum(x + ln, sp_end[j])
        sel = covers & (j >= 0) & (a < b)
        np.add.at(diff, (sp_off[j] + a - sp_beg[j])[sel], 1)
        np.add.at(diff, (sp_off[j] + b - sp_beg[j])[sel], -1)
        out["add"].update(n_kept=int(kr.size), n_unplaced=int((~placed).sum()), n_counted=int((row_span >= 0).sum()),
                          cov_bases=int((b - a)[sel].sum()))
    out["diff"] = diff
    out.update(finish(diff, spans))
    return out


def finish(diff, spans):
    """depth, runs and stats of a difference array (sums of several adds' diffs included)."""
    depth = np.cumsum(diff)
    assert depth.min(initial=0) >= 0 and depth.max(initial=0) < 2 ** 32
    runs, off = [], 0
    covered = total = 0
    mx = 0
    for r, beg, end in spans:
        d = depth[off:off + end - beg]
        assert depth[off + end - beg] == 0  # the extra slot brings the sum back
        heads = np.concatenate(([0], np.flatnonzero(np.diff(d)) + 1))
        part = np.zeros(heads.size, RUN_DTYPE)
        part["ref_id"], part["depth"], part["beg"] = r, d[heads], beg + heads
        part["end"] = np.concatenate((beg + heads[1:], [end]))
        runs.append(part)
        covered += int((d > 0).sum())
        total += int(d.sum())
        mx = max(mx, int(d.max()))
        off += end - beg + 1
    runs = np.concatenate(runs) if runs else np.zeros(0, RUN_DTYPE)
    return {"depth": depth.astype(np.uint32), "runs": runs,
            "stats": dict(slots=int(depth.size), n_runs=int(runs.size), covered=covered, sum=total, max_depth=mx)}


# ----------------------------------------------------------------------------------- builders

def one(pos, cigar, ref=0, flag=0, mapq=30, name=b"r", aux=b""):
    return rc.rec(ref, pos, mapq, 4681, flag, -1, -1, 0, name, tuple(cigar), (), b"", aux)


def case(records, spans, filter=None, count_del=False, order=None):
    s = rc.lay(list(records))
    starts = list(s.starts) if order is None else [s.starts[i] for i in order]
    return Case(s.flat, starts, list(spans), filter, count_del)


ONE_OP = np.dtype([("block_size", "<i4"), ("ref_id", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"), ("mapq", "u1"),
                   ("bin", "<u2"), ("n_cigar_op", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"), ("next_ref_id", "<i4"),
                   ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "S4"), ("cigar", "<u4")])


def one_op_stream(ref, pos, length, op=M, flag=0, mapq=30):
    """Records of one CIGAR op each (44 bytes: rec(..., name=b"abc", cigar=((length, op),))), vectorised."""
    pos = np.asarray(pos, np.int64)
    a = np.zeros(pos.size, ONE_OP)
    a["block_size"] = ONE_OP.itemsize - 4
    a["ref_id"], a["pos"], a["l_read_name"], a["mapq"], a["bin"] = ref, pos, 4, mapq, 4681
    a["n_cigar_op"], a["flag"], a["next_ref_id"], a["next_pos"] = 1, flag, -1, -1
    a["name"] = b"abc"
    a["cigar"] = np.asarray(length, np.int64) << 4 | op
    hdr = rc.header()
    return hdr + a.tobytes(), (len(hdr) + ONE_OP.itemsize * np.arange(pos.size)).tolist()


def _mixed_cigar(n, salt=0):
    """n ops cycling through all nine codes, lengths 1..5."""
    return tuple(((k + salt) % 5 + 1, (M, I, D, N, S, EQ, X, P, H)[(k + salt) % 9]) for k in range(n))


def _around(beg, end):
    """Reads at every edge of the span [beg, end)."""
    ln = end - beg
    return [one(beg - 5, [(10, M)]),        # starts before beg
            one(end - 3, [(10, M)]),        # ends after end
            one(beg, [(ln, M)]),            # exactly the span
            one(beg - 10, [(10, M)]),       # ends exactly on beg: outside
            one(end, [(5, M)]),             # starts exactly on end: outside
            one(end - 1, [(1, M)]),         # the last base
            one(beg, [(1, M)]),             # the first base
            one(beg + ln // 2, [(1, EQ)]),
            one(end + 1000, [(7, M)])]      # entirely outside


WRAP = tuple(x for _ in range(35) for x in ((50, M), (268435455, N)))  # 70 ops; x passes 2^32 after 17 Ns


def _filters_records():
    flags = (0, 0x4, 0x100, 0x200, 0x400, 0x10, 0x1, 0x14, 0x800)
    return [one(10 + 3 * i, [(20 + i % 7, M)], flag=flags[i % len(flags)], mapq=(i * 7) % 61) for i in range(200)]


CORPORA = {}
for _ln in (1, 2, T - 1, T, T + 1, 2 * T + 1):
    CORPORA["span_len_%d" % _ln] = functools.partial(lambda ln: case(_around(100, 100 + ln), [(0, 100, 100 + ln)]), _ln)
CORPORA.update({
    # span 0 owns slots [0, T): its extra slot is tile 0's last; span 1 begins tile 1
    "seam_tile_last": lambda: case(_around(0, T - 1) + [one(50, [(10, M)], ref=1), one(55, [(3, M)], ref=1)],
                                   [(0, 0, T - 1), (1, 50, 60)]),
    # span 0 owns slots [0, T]: its extra slot is tile 1's first
    "seam_tile_first": lambda: case(_around(0, T) + [one(48, [(10, M)], ref=1), one(59, [(3, M)], ref=1)],
                                    [(0, 0, T), (1, 50, 60)]),
    "ref_without_span": lambda: case([one(10, [(5, M)]), one(10, [(50, M)], ref=2), one(12, [(5, M)], ref=1)],
                                     [(0, 0, 100), (3, 0, 100)]),
    "span_without_records": lambda: case([one(10, [(5, M)], ref=1)], [(0, 7, 77)]),
    "pos_minus_one": lambda: case([one(-1, [(10, M)]), one(-1, [(1, M)]), one(-1, [(0, M)])], [(0, 0, 50)]),
    "pos_max": lambda: case([one(POS_MAX - 1, [(5, M)], ref=2), one(POS_MAX - 3, [(2, M)], ref=2)],
                            [(2, POS_MAX - 100, POS_MAX)]),
    "each_op_alone": lambda: case([one(10 + op, [(7, op)]) for op in range(9)], [(0, 0, 100)]),
    "each_op_alone_del": lambda: case([one(10 + op, [(7, op)]) for op in range(9)], [(0, 0, 100)], count_del=True),
    "zero_length_op": lambda: case([one(10, [(0, M)]), one(10, [(3, M), (0, M), (0, D), (2, M)])], [(0, 0, 100)]),
    "composite": lambda: case([one(10, [(10, M), (5, I), (10, M)]), one(10, [(5, S), (10, M), (5, H)]),
                               one(10, [(10, M), (3, P), (10, M)]), one(10, [(10, EQ), (1, X), (10, EQ)])], [(0, 0, 100)]),
    "deletion": lambda: case([one(10, [(10, M), (5, D), (10, M)])], [(0, 0, 100)]),
    "deletion_counted": lambda: case([one(10, [(10, M), (5, D), (10, M)])], [(0, 0, 100)], count_del=True),
    "skip": lambda: case([one(10, [(10, M), (100, N), (10, M)])], [(0, 0, 200)]),
    "skip_del": lambda: case([one(10, [(10, M), (100, N), (10, M)])], [(0, 0, 200)], count_del=True),
    "no_cigar": lambda: case([one(10, []), one(11, [(4, M)]), one(12, [])], [(0, 0, 100)]),
    "op9_filtered_out": lambda: case([one(10, [(4, M)]), one(10, [(4, 9)], flag=0x400), one(12, [(4, M)])], [(0, 0, 100)],
                                     filter={"flag_exclude": 0x400}),
    # records of a multiple of 4 bytes each, l_read_name 2..5: the CIGAR words start at all four alignments
    "alignments": lambda: case([one(10 * k, [(3, M), (2, D), (4, M)], name=b"abcd"[:k - 1], aux=bytes((4 - k) % 4))
                                for k in (2, 3, 4, 5)], [(0, 0, 100)], count_del=True),
    "handover_counts": lambda: case([one(90 + i, _mixed_cigar(nc, i)) for i, nc in
                                     enumerate((1, L, L + 1, 63, 64, 65, 129, 4097))], [(0, 100, 9000)], count_del=True),
    "handover_lanes": lambda: case([one(100 + i, _mixed_cigar(40 if i in (0, 31, 63) else 2, i)) for i in range(64)],
                                   [(0, 120, 250)]),
    "handover_all_long": lambda: case([one(100 + i, _mixed_cigar(L + 1 + i, i)) for i in range(64)], [(0, 0, 400)]),
    # only the first M can count: a 32-bit x would come back into the span
    "wrap_64bit": lambda: case([one(0, WRAP), one(0, WRAP[:L]), one(7, [(3, M)])], [(0, 0, 2 ** 20)]),
    "contention": lambda: Case(*one_op_stream(0, np.full(20000, 1000), 100), [(0, 0, 5000)], None, False),
    "staircase": lambda: Case(*one_op_stream(0, np.full(20000, 1000), np.arange(1, 20001)), [(0, 0, 30000)], None, False),
    # depth alternates at every slot: the most runs a span can hold
    "runs_alternating": lambda: Case(*one_op_stream(0, np.arange(0, T + 1, 2), 1), [(0, 0, T + 1)], None, False),
    # a run over tiles 0, 1 and 2; a head on tile 3's first slot
    "runs_tile_edges": lambda: case([one(T - 10, [(T + 20, M)]), one(3 * T, [(9, M)]), one(3 * T + 2, [(3, X)])],
                                    [(0, 0, 4 * T + 10)]),
    "filter_require": lambda: case(_filters_records(), [(0, 0, 1000)], filter={"flag_require": 0x10}),
    "filter_exclude": lambda: case(_filters_records(), [(0, 0, 1000)], filter={"flag_exclude": 0x704}),
    "filter_mapq": lambda: case(_filters_records(), [(0, 0, 1000)], filter={"min_mapq": 30}),
    "filter_rows": lambda: case(_filters_records(), [(0, 0, 1000)], filter={"rows": [(5, 50), (100, 130)]}),
    "filter_nothing_kept": lambda: case(_filters_records(), [(0, 0, 1000)], filter={"flag_require": 0x1000}),
    "rows_reversed_and_tripled": lambda: case(_filters_records(), [(0, 0, 1000)],
                                              order=list(range(199, -1, -1)) + [7, 7, 7]),
    "unplaced": lambda: case([one(10, [(5, M)], ref=-1), one(-1, [], ref=-1, flag=4), one(10, [(5, M)])], [(0, 0, 100)]),
})
# more rows than one grid pass of the row kernels (no CIGAR ops: rows are counted, nothing is covered)
CORPORA["grid"] = lambda: Case(rc.grid_stream()[0].flat, rc.grid_stream()[0].starts.tolist(), [(1, 0, 1000)], None, False)
SMALL = tuple(k for k in CORPORA if k != "grid")
# the stream with an op code 9 in a kept row: SBH_E_BAD_RECORD {1}
OP9_KEPT = lambda: case([one(10, [(4, M)]), one(10, [(4, M), (4, 9)]), one(12, [(4, M)])], [(0, 0, 100)])  # noqa: E731


@functools.lru_cache(maxsize=None)
def get(name):
    return CORPORA[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    c = get(name)
    return restate(c.flat, c.starts, c.spans, N_REF, c.filter, c.count_del)


def span_array(spans):
    a = np.zeros(len(spans), SPAN_DTYPE)
    for k, (r, b, e) in enumerate(spans):
        a[k] = (r, 0, b, e)
    return a


def driver_input(flat, starts, spans, n_ref=N_REF, filter=None, count_del=False):
    """The sanitizer driver's input file (tests/sanitize/depth_driver.cpp)."""
    f = filter or {}
    rows = f.get("rows") or []
    return (struct.pack("<Q", len(flat)) + bytes(flat) + struct.pack("<Q", len(starts))
            + np.asarray(starts, "<u8").tobytes() + struct.pack("<Q", len(spans)) + span_array(spans).tobytes()
            + struct.pack("<iIIIi", n_ref, 1 if count_del else 0, f.get("flag_require", 0), f.get("flag_exclude", 0),
                          f.get("min_mapq", 0))
            + struct.pack("<Q", len(rows)) + np.asarray([a for a, _ in rows], "<u8").tobytes()
            + np.asarray([b for _, b in rows], "<u8").tobytes())
