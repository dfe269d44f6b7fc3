"""Hand-built inputs for per-base allele counts (sbh_pileup_add_host / sbh_records_pileup_add and the
two finishes), and the numpy restatement of the definition in csrc/pileup_core.h.  The restatement
works from the raw bytes: every CIGAR op of every kept row flattened, op starts by np.cumsum, every
aligned or deleted base inside a span expanded into an index array, np.add.at on an [S, 8] array;
calls and intervals by vectorised numpy.  It is the expected value everywhere (test
infrastructure; plain Python, no GPU) and shares no code with the header.

Records are record_corpus.rec's bytes laid behind record_corpus.header() (four references).

PILE_TILE, PILE_GROUP, PILE_LANE_OPS and PILE_WINDOW are the library's (csrc/pileup_core.h; the CPU test reads
the header and holds these copies to it).
"""
import functools
import struct
from collections import namedtuple

import numpy as np

import record_corpus as rc

PILE_TILE = 1024
PILE_GROUP = 64
PILE_LANE_OPS = 16
PILE_WINDOW = 2048
T, G, L, W = PILE_TILE, PILE_GROUP, PILE_LANE_OPS, PILE_WINDOW
N_REF = len(rc.CONTIGS)
POS_MAX = 2 ** 31 - 1
M, I, D, N, S, H, P, EQ, X = range(9)
A_, C_, G_, T_, N_, DEL, INS, LOWQ = range(8)
SPAN_DTYPE = np.dtype([("ref_id", "<i4"), ("pad", "<i4"), ("beg", "<i8"), ("end", "<i8")])

# flat bytes, record starts (any order, repeats allowed), spans [(ref_id, beg, end)], the filter as
# records.record_filter's dict (None: all), min_baseq, min_depth, call_pct
Case = namedtuple("Case", "flat starts spans filter min_baseq min_depth call_pct")


# ------------------------------------------------------------------------------ the restatement

def positions_of(spans):
    return sum(e - b for _, b, e in spans)


def _u32(flat, at):
    at = np.asarray(at, np.int64)
    return sum(flat[at + k].astype(np.int64) << (8 * k) for k in range(4))


def _i32(flat, at):
    v = _u32(flat, at)
    return np.where(v >= 2 ** 31, v - 2 ** 32, v)


def _excl_by_row(v, first, nc):
    """Exclusive running sum of v inside each row's stretch of ops."""
    before = np.cumsum(v) - v
    return before - before[np.repeat(first, nc)] if v.size else before


def restate(flat, starts, spans, n_ref=N_REF, filter=None, min_baseq=0, min_depth=1, call_pct=75):
    """The definition restated.  Returns a dict: bad_row (None or the first bad row; nothing else
    then), add (n, n_kept, n_counted, n_unplaced, totals), counts (int64 [S, 8]) and finish()'s
    calls, intervals and stats."""
    flat = np.frombuffer(bytes(flat), np.uint8) if not isinstance(flat, np.ndarray) else flat
    total = int(flat.size)
    st_u = np.asarray(starts, np.uint64)
    n = int(st_u.size)
    filter = filter or {}
    counts = np.zeros((positions_of(spans), 8), np.int64)
    out = {"bad_row": None, "add": dict(n=n, n_kept=0, n_counted=0, n_unplaced=0, totals=[0] * 8)}
    if n:
        if total < 36:
            out["bad_row"] = 0
            return out
        fixed = st_u <= np.uint64(total - 36)
        p = np.where(fixed, st_u, np.uint64(0)).astype(np.int64)
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
        kr = np.flatnonzero(keep)
        nc = n_cig[kr]
        first = np.concatenate(([0], np.cumsum(nc)))[:-1]
        of_row = np.repeat(np.arange(kr.size), nc)
        k = np.arange(int(nc.sum())) - np.repeat(first, nc)
        cig_at = p[kr] + 36 + l_name[kr]
        w = _u32(flat, cig_at[of_row] + 4 * k) if of_row.size else np.zeros(0, np.int64)
        ln, op = w >> 4, w & 15
        q_adv = np.where(np.isin(op, (M, I, S, EQ, X)), ln, 0)
        q_sum = np.bincount(of_row, weights=q_adv.astype(np.float64), minlength=kr.size).astype(np.int64)
        bad = ~valid
        bad[kr[ref[kr] >= n_ref]] = True
        bad[kr[np.unique(of_row[op > 8])]] = True
        bad[kr[(nc > 0) & (l_seq[kr] > 0) & (q_sum != l_seq[kr])]] = True
        if bad.any():
            out["bad_row"] = int(np.flatnonzero(bad)[0])
            return out
        x = pos[kr][of_row] + _excl_by_row(np.where(np.isin(op, (M, D, N, EQ, X)), ln, 0), first, nc)
        q = _excl_by_row(q_adv, first, nc)
        span_of = np.full(n_ref, -1, np.int64)
        for j, (r, _, _) in enumerate(spans):
            span_of[r] = j
        sp_beg = np.asarray([b for _, b, _ in spans], np.int64)
        sp_end = np.asarray([e for _, _, e in spans], np.int64)
        sp_off = np.concatenate(([0], np.cumsum(sp_end - sp_beg)))[:-1]
        placed = ref[kr] >= 0
        row_span = np.where(placed, span_of[np.where(placed, ref[kr], 0)], -1)
        j = row_span[of_row]
        # aligned and deleted stretches cut to the span, one entry per base
        a = np.maximum(x, sp_beg[j])
        b = np.minimum(x + ln, sp_end[j])
        sel = np.flatnonzero((np.isin(op, (M, EQ, X)) | (op == D)) & (j >= 0) & (a < b))
        cnt = (b - a)[sel]
        rep = np.repeat(sel, cnt)
        pp = a[rep] + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        slot = sp_off[j[rep]] + pp - sp_beg[j[rep]]
        row_of = kr[of_row[rep]]
        qi = q[rep] + pp - x[rep]
        has_seq = l_seq[row_of] > 0
        seq_at = cig_at[of_row[rep]] + 4 * n_cig[row_of]
        qi0 = np.where(has_seq & (op[rep] != D), qi, 0)
        byte = flat[np.where(has_seq, seq_at + qi0 // 2, 0)].astype(np.int64)
        code = np.where(qi0 % 2 == 0, byte >> 4, byte & 15)
        qual = flat[np.where(has_seq, seq_at + (l_seq[row_of] + 1) // 2 + qi0, 0)].astype(np.int64)
        letter = np.full(16, N_, np.int64)
        letter[[1, 2, 4, 8]] = (A_, C_, G_, T_)
        ch = np.where(op[rep] == D, DEL, np.where(~has_seq, N_, np.where(qual < min_baseq, LOWQ, letter[code])))
        np.add.at(counts, (slot, ch), 1)
        # insertions: one count at the position before
        isel = (op == I) & (ln >= 1) & (j >= 0) & (x > pos[kr][of_row]) & (x - 1 >= sp_beg[j]) & (x - 1 < sp_end[j])
        np.add.at(counts, ((sp_off[j] + x - 1 - sp_beg[j])[isel], INS), 1)
        out["add"].update(n_kept=int(kr.size), n_unplaced=int((~placed).sum()), n_counted=int((row_span >= 0).sum()),
                          totals=[int(v) for v in counts.sum(axis=0)])
    out["counts"] = counts
    out.update(finish(counts, spans, min_depth, call_pct))
    return out


def finish(counts, spans, min_depth=1, call_pct=75):
    """calls (uint8), intervals (SPAN_DTYPE) and stats of a count table (sums of several adds' too)."""
    assert counts.max(initial=0) < 2 ** 32
    five = counts[:, [A_, C_, G_, T_, DEL]]
    best = five.max(axis=1, initial=0)
    unique = (five == best[:, None]).sum(axis=1) == 1
    total = counts[:, [A_, C_, G_, T_, N_, DEL]].sum(axis=1)
    called = unique & (total >= min_depth) & (best * 100 >= call_pct * total)
    letters = np.frombuffer(b"ACGT*", np.uint8)
    calls = np.where(~counts.any(axis=1), 0, np.where(called, letters[five.argmax(axis=1)], ord("N"))).astype(np.uint8)
    depth = counts[:, [A_, C_, G_, T_, N_, LOWQ]].sum(axis=1)
    ivs, off = [], 0
    for r, beg, end in spans:
        nz = np.concatenate(([0], (calls[off:off + end - beg] != 0).astype(np.int8), [0]))
        edge = np.diff(nz)
        part = np.zeros(int((edge == 1).sum()), SPAN_DTYPE)
        part["ref_id"], part["beg"], part["end"] = r, beg + np.flatnonzero(edge == 1), beg + np.flatnonzero(edge == -1)
        ivs.append(part)
        off += end - beg
    ivs = np.concatenate(ivs) if ivs else np.zeros(0, SPAN_DTYPE)
    stats = dict(positions=int(calls.size), n_intervals=int(ivs.size), nonzero=int((calls != 0).sum()),
                 n_called=int(np.isin(calls, letters).sum()), covered=int((depth > 0).sum()),
                 max_depth=int(depth.max(initial=0)), totals=[int(v) for v in counts.sum(axis=0)])
    return {"calls": calls, "intervals": ivs, "stats": stats}


# ----------------------------------------------------------------------------------- builders

def qlen(cigar):
    return sum(ln for ln, op in cigar if op in (M, I, S, EQ, X))


def read(pos, cigar, ref=0, flag=0, mapq=30, name=b"r", aux=b"", codes=None, qual=None, seed=0, **kw):
    """A record whose SEQ and QUAL are as long as its CIGAR says: codes (3 k + seed) % 16 and
    qualities (7 k + seed) % 94 unless given.  An odd l_seq leaves 0xF in the last byte's low
    nibble: a read one nibble too far would show as a count."""
    n = qlen(cigar)
    codes = tuple((3 * k + seed) % 16 for k in range(n)) if codes is None else tuple(codes)
    qual = bytes((7 * k + seed) % 94 for k in range(len(codes))) if qual is None else bytes(qual)
    return rc.rec(ref, pos, mapq, 4681, flag, -1, -1, 0, name, tuple(cigar), codes, qual, aux, spare=0xF, **kw)


def case(records, spans, filter=None, min_baseq=0, min_depth=1, call_pct=75, order=None):
    s = rc.lay(list(records))
    starts = list(s.starts) if order is None else [s.starts[i] for i in order]
    return Case(s.flat, starts, list(spans), filter, min_baseq, min_depth, call_pct)


def repeated(record, n, spans, pos=None, code=None, **kw):
    """n copies of one record, vectorised; pos / code (arrays) patch each copy's position and its
    first base's code (the high nibble of the first SEQ byte)."""
    base = np.frombuffer(record, np.uint8)
    a = np.tile(base, (n, 1))
    if pos is not None:
        a[:, 8:12] = np.asarray(pos, "<i4").view(np.uint8).reshape(n, 4)
    if code is not None:
        at = 36 + int(base[12]) + 4 * (int(base[16]) | int(base[17]) << 8)
        a[:, at] = (np.asarray(code, np.uint8) << 4) | (a[:, at] & 15)
    hdr = rc.header()
    return Case(hdr + a.tobytes(), (len(hdr) + base.size * np.arange(n)).tolist(), list(spans), kw.get("filter"),
                kw.get("min_baseq", 0), kw.get("min_depth", 1), kw.get("call_pct", 75))


def _mixed_cigar(n, salt=0):
    """n ops cycling through all nine codes, lengths 1..5."""
    return tuple(((k + salt) % 5 + 1, (M, I, D, N, S, EQ, X, P, H)[(k + salt) % 9]) for k in range(n))


def _around(beg, end):
    """Reads at every edge of the span [beg, end), and insertions anchored at beg - 1, beg, end - 1
    and end."""
    ln = end - beg
    return [read(beg - 5, [(10, M)], seed=1),        # starts before beg
            read(end - 3, [(10, M)], seed=2),        # ends after end
            read(beg, [(ln, M)], seed=3),            # exactly the span
            read(beg - 10, [(10, M)], seed=4),       # ends exactly on beg: outside
            read(end, [(5, M)], seed=5),             # starts exactly on end: outside
            read(end - 1, [(1, M)], seed=6),         # the last base
            read(beg, [(1, M)], seed=7),             # the first base
            read(beg + ln // 2, [(1, EQ)], seed=8),
            read(end + 1000, [(7, M)], seed=9),      # entirely outside
            read(beg - 4, [(8, D)], seed=10),        # a deletion over the first edge
            read(end - 4, [(2, M), (8, D), (1, M)], seed=11)] + \
           [read(at, [(1, M), (2, I), (1, M)], seed=12 + k) for k, at in enumerate((beg - 1, beg, end - 1, end))]


WRAP = tuple(x for _ in range(35) for x in ((50, M), (268435455, N)))  # 70 ops; x passes 2^32 after 17 Ns


def _filters_records():
    flags = (0, 0x4, 0x100, 0x200, 0x400, 0x10, 0x1, 0x14, 0x800)
    return [read(10 + 3 * i, [(20 + i % 7, M)], flag=flags[i % len(flags)], mapq=(i * 7) % 61, seed=i) for i in range(200)]


def _quality_case(mb):
    q = bytes(sorted({max(mb - 1, 0), mb, 0, 255}))
    return case([read(10, [(len(q), M)], codes=(1, 2, 4, 8)[:len(q)], qual=q),
                 read(12, [(len(q), M)], codes=(8, 4, 2, 1)[:len(q)], qual=q[::-1])], [(0, 0, 50)], min_baseq=mb)


def _call_edges():
    """min_baseq 13, min_depth 3, call_pct 75; one-base reads stacked per position."""
    def stack(at, spec, q=30):  # spec: "AAAC" -> one read per letter
        return [read(at, [(1, M)], codes=({"A": 1, "C": 2, "G": 4, "T": 8, "N": 15}[c],), qual=bytes([q])) for c in spec]
    dele = lambda at: read(at - 1, [(1, M), (1, D), (1, M)], codes=(1, 1), qual=b"\x1e\x1e")  # noqa: E731
    return (stack(10, "AAAC")                        # 300 == 75 * 4: 'A'
            + stack(20, "AAACC")                     # 300 < 375: 'N'
            + stack(30, "AACC")                      # a tie: 'N'
            + stack(40, "A") + [dele(40), dele(40), dele(40)]   # DEL 3 of 4 at 40: '*' (and A at 39, 41: below min_depth)
            + stack(50, "GG")                        # total == min_depth - 1: 'N'
            + stack(60, "NNNN")                      # N only: 'N'
            + stack(70, "TTTT", q=12)                # LOWQ only: 'N'
            + stack(80, "TTT")                       # total == min_depth: 'T'
            + stack(90, "CCCN"))                     # N counts in the total: 300 == 75 * 4: 'C'


CORPORA = {}
for _ln in (1, T - 1, T, T + 1, 2 * T + 1):
    CORPORA["span_len_%d" % _ln] = functools.partial(lambda ln: case(_around(100, 100 + ln), [(0, 100, 100 + ln)]), _ln)
for _mb in (0, 13, 255):
    CORPORA["quality_%d" % _mb] = functools.partial(_quality_case, _mb)
CORPORA.update({
    "l_seq_edges": lambda: case([read(10 + 300 * k, [(n, M)], seed=k) for k, n in
                                 enumerate((1, 2, 3, G - 1, G, G + 1, 2 * G + 1))], [(0, 0, 2200)]),
    "l_seq_edges_clipped": lambda: case([read(10 + 300 * k, [(2, S), (n, M), (1, S)], seed=k) for k, n in
                                         enumerate((1, 2, 3, G - 1, G, G + 1, 2 * G + 1))], [(0, 0, 2200)], min_baseq=20),
    "all_codes": lambda: case([read(10, [(16, M)], codes=range(16)), read(12, [(17, M)], codes=(15,) + tuple(range(16)))],
                              [(0, 0, 50)]),
    # records of 4 m + 1 bytes each, l_read_name 2..5: the records start at all four alignments, and so
    # do their CIGAR words, SEQ and QUAL
    "alignments": lambda: case([read(10 * k + i, [(3, M), (2, D), (4, M), (1, S)], name=b"abcd"[:k - 1], aux=bytes((1 - k) % 4),
                                     seed=k + i) for i, k in enumerate((2, 3, 4, 5, 2, 3, 4, 5))], [(0, 0, 100)], min_baseq=10),
    "seam_spans": lambda: case(_around(0, T - 1) + [read(50, [(10, M)], ref=1), read(55, [(3, M)], ref=1),
                                                    read(48, [(20, M)], ref=3)],
                               [(0, 0, T - 1), (1, 50, 60), (3, 59, 60)]),
    "ref_without_span": lambda: case([read(10, [(5, M)]), read(10, [(50, M)], ref=2), read(12, [(5, M)], ref=1)],
                                     [(0, 0, 100), (3, 0, 100)]),
    "span_without_records": lambda: case([read(10, [(5, M)], ref=1)], [(0, 7, 77)]),
    "pos_minus_one": lambda: case([read(-1, [(10, M)]), read(-1, [(1, M)]), read(-1, [(0, M)])], [(0, 0, 50)]),
    "pos_max": lambda: case([read(POS_MAX - 1, [(5, M)], ref=2), read(POS_MAX - 3, [(2, M), (1, I), (1, M)], ref=2)],
                            [(2, POS_MAX - 100, POS_MAX)]),
    "each_op_alone": lambda: case([read(10 + op, [(7, op)], seed=op) for op in range(9)], [(0, 0, 100)]),
    "zero_length_op": lambda: case([read(10, [(0, M)]), read(10, [(3, M), (0, M), (0, D), (2, M)]),
                                    read(20, [(5, M), (0, I), (5, M)])], [(0, 0, 100)]),
    "composite": lambda: case([read(10, [(10, M), (5, I), (10, M)], seed=1), read(10, [(5, S), (10, M), (5, H)], seed=2),
                               read(10, [(10, M), (3, P), (10, M)], seed=3), read(10, [(10, EQ), (1, X), (10, EQ)], seed=4),
                               read(30, [(3, S), (5, M), (2, I), (5, M), (4, D), (5, M), (3, S)], seed=5),
                               read(60, [(2, I), (10, M)], seed=6),           # a leading insertion: counted nowhere
                               read(80, [(10, M), (2, I)], seed=7),           # trailing: counted at the last base
                               read(100, [(5, M), (10, N), (2, I), (5, M)], seed=8),
                               read(130, [(5, H), (5, S), (10, M)], seed=9),
                               read(150, [(3, S), (2, I), (4, M)], seed=10)], [(0, 0, 200)], min_baseq=15),
    "deletion": lambda: case([read(10, [(10, M), (5, D), (10, M)])], [(0, 0, 100)]),
    "skip": lambda: case([read(10, [(10, M), (100, N), (10, M)])], [(0, 0, 200)]),
    "no_cigar": lambda: case([read(10, []), read(11, [(4, M)]), read(12, [], codes=(1, 2, 4), qual=b"abc")], [(0, 0, 100)]),
    "no_seq": lambda: case([read(10, [(10, M)], codes=(), qual=b""), read(12, [(3, M), (2, I), (2, D), (3, M)], codes=(), qual=b""),
                            read(14, [(4, M)])], [(0, 0, 100)], min_baseq=255),
    "op9_filtered_out": lambda: case([read(10, [(4, M)]), read(10, [(4, 9)], flag=0x400, codes=(), qual=b""), read(12, [(4, M)])],
                                     [(0, 0, 100)], filter={"flag_exclude": 0x400}),
    "qsum_short_filtered_out": lambda: case([read(10, [(4, M)]), read(10, [(9, M)], flag=0x400, codes=(1,) * 10, qual=bytes(10)),
                                             read(12, [(4, M)])], [(0, 0, 100)], filter={"flag_exclude": 0x400}),
    "qsum_over_filtered_out": lambda: case([read(10, [(4, M)]), read(10, [(11, M)], flag=0x400, codes=(1,) * 10, qual=bytes(10)),
                                            read(12, [(4, M)])], [(0, 0, 100)], filter={"rows": [(0, 1), (2, 3)]}),
    "handover_counts": lambda: case([read(90 + i, _mixed_cigar(nc, i), seed=i) for i, nc in
                                     enumerate((1, L, L + 1, 63, 64, 65, 129, 4097))], [(0, 100, 9000)], min_baseq=30),
    "handover_lanes": lambda: case([read(100 + i, _mixed_cigar(40 if i in (0, 31, 63) else 2, i), seed=i) for i in range(64)],
                                   [(0, 120, 250)]),
    "handover_all_long": lambda: case([read(100 + i, _mixed_cigar(L + 1 + i, i), seed=i) for i in range(64)], [(0, 0, 400)]),
    # only the first M can count: a 32-bit x would come back into the span
    "wrap_64bit": lambda: case([read(0, WRAP), read(0, WRAP[:L], seed=3), read(7, [(3, M)])], [(0, 0, 2 ** 20)]),
    # 20 000 identical reads on one place: every counter there is 20 000
    "contention": lambda: repeated(read(1000, [(50, M), (3, D), (1, I), (50, M)], seed=5), 20000, [(0, 0, 5000)], min_baseq=40),
    # calls alternate zero and non-zero at every position: the most intervals a span can hold
    "intervals_alternating": lambda: repeated(read(0, [(1, M)], codes=(1,), qual=b"\x1e"), T // 2 + 1, [(0, 0, T + 1)],
                                              pos=np.arange(0, T + 1, 2), code=1 << (np.arange(T // 2 + 1) % 4)),
    # an interval ending on tile 0's last position, one starting on tile 2's first, one over tiles 3, 4 and 5
    "intervals_tile_edges": lambda: case([read(T - 7, [(7, M)]), read(2 * T, [(9, M)], seed=1), read(2 * T + 2, [(3, X)], seed=2),
                                          read(4 * T - 10, [(T + 20, M)], seed=3)], [(0, 0, 6 * T + 10)]),
    # the events kernel's window opens at the first row's position: reads before it, on both its ends,
    # behind it, a deletion over all of it, and an insertion anchored on its last position
    "window_edges": lambda: case([read(5000, [(10, M)]), read(10, [(10, M)], seed=1), read(5000 + W - 5, [(10, M)], seed=2),
                                  read(5000 + W, [(3, M)], seed=3), read(4995, [(10, M)], seed=4),
                                  read(5000, [(3, M), (W, D), (3, M)], seed=5), read(5000 + W - 1, [(1, M), (2, I), (1, M)], seed=6),
                                  read(4990, [(9, M), (W + 3, N), (7, M)], seed=7)], [(0, 0, 5000 + 2 * W)], min_baseq=25),
    # the window crosses from one span into the next
    "window_two_spans": lambda: case([read(90, [(20, M)]), read(95, [(10, M), (3, D), (10, M)], seed=1), read(0, [(30, M)], ref=1, seed=2),
                                      read(5, [(30, M)], ref=1, seed=3)], [(0, 50, 100), (1, 10, 4000)]),
    "call_edges": lambda: case(_call_edges(), [(0, 0, 100)], min_baseq=13, min_depth=3, call_pct=75),
    "call_pct_100": lambda: case(_call_edges(), [(0, 0, 100)], min_baseq=0, min_depth=1, call_pct=100),
    "call_pct_1": lambda: case(_call_edges(), [(0, 0, 100)], min_baseq=0, min_depth=4, call_pct=1),
    "filter_require": lambda: case(_filters_records(), [(0, 0, 1000)], filter={"flag_require": 0x10}),
    "filter_exclude": lambda: case(_filters_records(), [(0, 0, 1000)], filter={"flag_exclude": 0x704}),
    "filter_mapq": lambda: case(_filters_records(), [(0, 0, 1000)], filter={"min_mapq": 30}),
    "filter_rows": lambda: case(_filters_records(), [(0, 0, 1000)], filter={"rows": [(5, 50), (100, 130)]}),
    "filter_nothing_kept": lambda: case(_filters_records(), [(0, 0, 1000)], filter={"flag_require": 0x1000}),
    "rows_reversed_and_tripled": lambda: case(_filters_records(), [(0, 0, 1000)], order=list(range(199, -1, -1)) + [7, 7, 7]),
    "unplaced": lambda: case([read(10, [(5, M)], ref=-1), read(-1, [], ref=-1, flag=4), read(10, [(5, M)])], [(0, 0, 100)]),
})
# more rows than one grid pass of the row kernels: one-base reads, a running position and code
GRID_ROWS = 262144 + 37
CORPORA["grid"] = lambda: repeated(read(0, [(1, M)], codes=(1,), qual=b"\x1e", ref=1), GRID_ROWS, [(1, 5, 995)],
                                   pos=np.arange(GRID_ROWS) % 1000, code=1 << (np.arange(GRID_ROWS) % 5))
SMALL = tuple(k for k in CORPORA if k != "grid")

# streams with a bad kept row: name -> (case, the row)
BAD_KEPT = {
    "op9": lambda: (case([read(10, [(4, M)]), read(10, [(4, M), (4, 9)], codes=(1,) * 4, qual=bytes(4)), read(12, [(4, M)])],
                         [(0, 0, 100)]), 1),
    "qsum_short": lambda: (case([read(10, [(4, M)]), read(12, [(4, M)]), read(10, [(9, M)], codes=(1,) * 10, qual=bytes(10))],
                                [(0, 0, 100)]), 2),
    "qsum_over": lambda: (case([read(10, [(11, M)], codes=(1,) * 10, qual=bytes(10)), read(12, [(4, M)])], [(0, 0, 100)]), 0),
    "qsum_over_long": lambda: (case([read(10, [(4, M)]), read(10, [(1, M)] * (L + 5), codes=(1,) * (L + 4), qual=bytes(L + 4))],
                                    [(0, 0, 100)]), 1),
    "op9_long": lambda: (case([read(10, [(4, M)]), read(10, [(1, M)] * 70 + [(1, 9)], codes=(1,) * 70, qual=bytes(70))],
                              [(0, 0, 100)]), 1),
    "ref_out_of_range": lambda: (case([read(1, [(4, M)]), read(1, [(4, M)], ref=N_REF)], [(0, 0, 100)]), 1),
}

# The hand-worked case: three reads, span [98, 116) of reference 0, min_baseq 10, min_depth 2,
# call_pct 60.  The table, the calls and the intervals are literals, worked out by hand:
#   read 1  pos 100  4M1D3M      ACGT|ACG, the G at 102 has quality 5
#   read 2  pos 102  2S3M2I3M    NN|GTT|AA|ACC
#   read 3  pos 103  3M4N4M      TTN|A=GT
HAND = dict(
    records=lambda: [read(100, [(4, M), (1, D), (3, M)], codes=(1, 2, 4, 8, 1, 2, 4), qual=bytes((30, 30, 5, 30, 30, 30, 30))),
                     read(102, [(2, S), (3, M), (2, I), (3, M)], codes=(15, 15, 4, 8, 8, 1, 1, 1, 2, 2), qual=bytes([40] * 10)),
                     read(103, [(3, M), (4, N), (4, M)], codes=(8, 8, 15, 1, 0, 4, 8), qual=bytes([20] * 7))],
    spans=[(0, 98, 116)], min_baseq=10, min_depth=2, call_pct=60,
    #         A  C  G  T  N DEL INS LOWQ
    table=[[0, 0, 0, 0, 0, 0, 0, 0],   # 98
           [0, 0, 0, 0, 0, 0, 0, 0],   # 99
           [1, 0, 0, 0, 0, 0, 0, 0],   # 100
           [0, 1, 0, 0, 0, 0, 0, 0],   # 101
           [0, 0, 1, 0, 0, 0, 0, 1],   # 102
           [0, 0, 0, 3, 0, 0, 0, 0],   # 103
           [0, 0, 0, 2, 0, 1, 1, 0],   # 104
           [2, 0, 0, 0, 1, 0, 0, 0],   # 105
           [0, 2, 0, 0, 0, 0, 0, 0],   # 106
           [0, 1, 1, 0, 0, 0, 0, 0],   # 107
           [0, 0, 0, 0, 0, 0, 0, 0],   # 108
           [0, 0, 0, 0, 0, 0, 0, 0],   # 109
           [1, 0, 0, 0, 0, 0, 0, 0],   # 110
           [0, 0, 0, 0, 1, 0, 0, 0],   # 111
           [0, 0, 1, 0, 0, 0, 0, 0],   # 112
           [0, 0, 0, 1, 0, 0, 0, 0],   # 113
           [0, 0, 0, 0, 0, 0, 0, 0],   # 114
           [0, 0, 0, 0, 0, 0, 0, 0]],  # 115
    calls=b"\0\0NNNTTACN\0\0NNNN\0\0",
    intervals=[(0, 100, 108), (0, 110, 114)],
    add=dict(n=3, n_kept=3, n_counted=3, n_unplaced=0, totals=[4, 4, 3, 6, 2, 1, 1, 1]),
    stats=dict(positions=18, n_intervals=2, nonzero=12, n_called=4, covered=12, max_depth=3,
               totals=[4, 4, 3, 6, 2, 1, 1, 1]),
)


def hand_case():
    return case(HAND["records"](), HAND["spans"], None, HAND["min_baseq"], HAND["min_depth"], HAND["call_pct"])


@functools.lru_cache(maxsize=None)
def get(name):
    return CORPORA[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    c = get(name)
    return restate(c.flat, c.starts, c.spans, N_REF, c.filter, c.min_baseq, c.min_depth, c.call_pct)


def span_array(spans):
    a = np.zeros(len(spans), SPAN_DTYPE)
    for k, (r, b, e) in enumerate(spans):
        a[k] = (r, 0, b, e)
    return a


def span_slices(spans):
    """[(span index, first position, one past the last)] in the concatenated position arrays."""
    out, off = [], 0
    for k, (_, b, e) in enumerate(spans):
        out.append((k, off, off + e - b))
        off += e - b
    return out


def driver_input(flat, starts, spans, n_ref=N_REF, filter=None, min_baseq=0, min_depth=1, call_pct=75):
    """The sanitizer driver's input file (tests/sanitize/pileup_driver.cpp)."""
    f = filter or {}
    rows = f.get("rows") or []
    return (struct.pack("<Q", len(flat)) + bytes(flat) + struct.pack("<Q", len(starts))
            + np.asarray(starts, "<u8").tobytes() + struct.pack("<Q", len(spans)) + span_array(spans).tobytes()
            + struct.pack("<iIIIIIi", n_ref, min_baseq, min_depth, call_pct, f.get("flag_require", 0),
                          f.get("flag_exclude", 0), f.get("min_mapq", 0))
            + struct.pack("<Q", len(rows)) + np.asarray([a for a, _ in rows], "<u8").tobytes()
            + np.asarray([b for _, b in rows], "<u8").tobytes())
