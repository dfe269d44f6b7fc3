"""CPU restatement of BAI construction for parity tests (test infrastructure; plain Python,
never the product path).

htslib's hts_idx_push / hts_idx_finish as one loop over the records of a BAM file: zlib
inflates the BGZF members, oracle_records walks the record chain, and every record is pushed
in file order.  Rules:

  * vbeg = virtual offset of the record's start, vend = that of its end (= the next record's
    vbeg; past the last non-empty member: (its start + its csize) << 16).
  * ref_id < 0: counts into n_no_coor, nothing else.
  * otherwise beg = pos; end = pos + reference length (M D N = X) when flag 4 is clear and the
    length is > 0, else pos + 1; bin = reg2bin(beg, end), the stored bin ignored; unmapped for
    its reference when flag 4 is set.
  * a run = consecutive records of one (ref_id, bin): one chunk [first vbeg, last vend).
  * linear index: window w in [beg >> 14, (end - 1) >> 14] (clamped to (l_ref >> 14) + 1) keeps
    the smallest vbeg; n_intv = last touched + 1; untouched windows below take the next one's.
  * finish: levels 5..1, bins of the level (sorted below level 5) spanning < 0x10000 block
    addresses go to the parent; bin 0 sorted; chunks meeting in one block merged.
  * layout: BAI\\1, n_ref, per reference bins ascending with 37450 last, intervals; n_no_coor.
"""
import struct
import zlib
from collections import namedtuple

import numpy as np

import oracle_records as orr

META_BIN = 37450
U64_MAX = (1 << 64) - 1
RUN_DTYPE = np.dtype([("ref_id", "<i4"), ("bin", "<u4"), ("vbeg", "<u8"), ("vend", "<u8"),
                      ("n_mapped", "<u8"), ("n_unmapped", "<u8")])

Ref = namedtuple("Ref", "runs lin n_no_coor bytes contig_len lin_off records")
Rec = namedtuple("Rec", "start vbeg vend ref_id pos flag beg end bin")


class Unsorted(Exception):
    def __init__(self, vpos):
        super().__init__(f"unsorted at {vpos >> 16}:{vpos & 0xffff}")
        self.vpos = vpos


class BadRecord(Exception):
    pass


def members(data):
    """[(file offset, csize, flat start, usize)] and the flat bytes of a BGZF file."""
    data = bytes(data)
    out, flat, p, u0 = [], [], 0, 0
    while p < len(data):
        csize = struct.unpack_from("<H", data, p + 16)[0] + 1
        u = zlib.decompress(data[p + 18:p + csize - 8], -15)
        out.append((p, csize, u0, len(u)))
        flat.append(u)
        u0 += len(u)
        p += csize
    return out, b"".join(flat)


def virtual_offset(blocks, f):
    live = [b for b in blocks if b[3] > 0]
    for c, cs, u, us in live:
        if u <= f < u + us:
            return c << 16 | (f - u)
    c, cs, u, us = live[-1]
    assert f == u + us
    return (c + cs) << 16


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return 4681 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return 585 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return 73 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return 9 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return 1 + (beg >> 26)
    return 0


def level_of(b):
    for lv, first in ((5, 4681), (4, 585), (3, 73), (2, 9), (1, 1)):
        if b >= first:
            return lv
    return 0


def contigs_of(flat):
    l_text = struct.unpack_from("<i", flat, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", flat, p)[0]
    p += 4
    lens = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", flat, p)[0]
        lens.append(struct.unpack_from("<i", flat, p + 4 + ln)[0])
        p += 8 + ln
    return lens, p


def records_of(data):
    """Every record of the file with its coordinates, in file order."""
    blocks, flat = members(data)
    lens, first = contigs_of(flat)
    starts = orr.record_starts(flat, first, len(flat))
    out = []
    for k, s in enumerate(starts):
        bsz, ref, pos, bmn, fnc = struct.unpack_from("<iiiII", flat, s)
        flag, ncig = fnc >> 16, fnc & 0xffff
        q = s + 36 + (bmn & 0xff)
        span = 0
        for op in struct.unpack_from("<%dI" % ncig, flat, q):
            if op & 15 in orr.REF_OPS:
                span += op >> 4
        end = pos + span if not flag & 4 and span > 0 else pos + 1
        out.append(Rec(s, virtual_offset(blocks, s), virtual_offset(blocks, s + 4 + bsz), ref, pos, flag, pos, end,
                       reg2bin(pos, end) if ref >= 0 else None))
    return out, lens


def finish(bins):
    """compress_binning over {bin: [[beg, end], ...]} (in place)."""
    for lv in (5, 4, 3, 2, 1):
        for b in sorted(k for k in bins if level_of(k) == lv):
            ch = bins[b]
            if lv < 5:
                ch.sort()
            if (ch[-1][1] >> 16) - (ch[0][0] >> 16) < 0x10000:
                bins.setdefault((b - 1) >> 3, []).extend(ch)
                del bins[b]
    if 0 in bins:
        bins[0].sort()
    for b, ch in bins.items():
        kept = [list(ch[0])]
        for c in ch[1:]:
            if kept[-1][1] >> 16 >= c[0] >> 16:
                kept[-1][1] = max(kept[-1][1], c[1])
            else:
                kept.append(list(c))
        bins[b] = kept
    return bins


def serialise(n_ref, bins_of, meta_of, lin_of, n_no_coor):
    o = [b"BAI\1", struct.pack("<i", n_ref)]
    for r in range(n_ref):
        if r not in meta_of:
            o.append(struct.pack("<ii", 0, 0))
            continue
        bins = bins_of[r]
        o.append(struct.pack("<i", len(bins) + 1))
        for b in sorted(bins):
            o.append(struct.pack("<Ii", b, len(bins[b])))
            for u, v in bins[b]:
                o.append(struct.pack("<QQ", u, v))
        o.append(struct.pack("<IiQQQQ", META_BIN, 2, *meta_of[r]))
        li = lin_of[r]
        o.append(struct.pack("<i", len(li)))
        o.append(struct.pack("<%dQ" % len(li), *li))
    o.append(struct.pack("<Q", n_no_coor))
    return b"".join(o)


def build(data, rows=None):
    """rows = (a, b): only records [a, b) of the file are pushed (a scan of a sub-range)."""
    recs, lens = records_of(data)
    if rows is not None:
        recs = recs[rows[0]:rows[1]]
    n_ref = len(lens)
    lin_off = [0]
    for ln in lens:
        lin_off.append(lin_off[-1] + (ln >> 14) + 2)
    lin = [U64_MAX] * lin_off[-1]
    runs, bins_of, meta_of = [], {}, {}
    n_no_coor, prev, seen_no_coor = 0, None, False
    for rc in recs:
        if rc.ref_id < 0:
            n_no_coor += 1
            seen_no_coor = True
            prev = None
            continue
        if rc.ref_id >= n_ref or rc.pos < 0:
            raise BadRecord(rc.vbeg)
        if seen_no_coor or (prev is not None and (rc.ref_id, rc.pos) < (prev.ref_id, prev.pos)):
            raise Unsorted(rc.vbeg)
        um = 1 if rc.flag & 4 else 0
        if prev is not None and (prev.ref_id, prev.bin) == (rc.ref_id, rc.bin):
            runs[-1][3] = rc.vend
            runs[-1][4] += 1 - um
            runs[-1][5] += um
            bins_of[rc.ref_id][rc.bin][-1][1] = rc.vend
        else:
            runs.append([rc.ref_id, rc.bin, rc.vbeg, rc.vend, 1 - um, um])
            bins_of.setdefault(rc.ref_id, {}).setdefault(rc.bin, []).append([rc.vbeg, rc.vend])
        m = meta_of.setdefault(rc.ref_id, [rc.vbeg, rc.vend, 0, 0])
        m[1] = rc.vend
        m[2 + um] += 1
        wmax = (lens[rc.ref_id] >> 14) + 1
        for w in range(rc.beg >> 14, ((rc.end - 1) >> 14) + 1):
            k = lin_off[rc.ref_id] + min(w, wmax)
            lin[k] = min(lin[k], rc.vbeg)
        prev = rc
    lin_of = {}
    for r in meta_of:
        finish(bins_of[r])
        li = lin[lin_off[r]:lin_off[r + 1]]
        while li and li[-1] == U64_MAX:
            li.pop()
        for k in range(len(li) - 2, -1, -1):
            if li[k] == U64_MAX:
                li[k] = li[k + 1]
        lin_of[r] = li
    out = serialise(n_ref, bins_of, meta_of, lin_of, n_no_coor)
    runs_a = np.zeros(len(runs), RUN_DTYPE)
    for k, r in enumerate(runs):
        runs_a[k] = tuple(r)
    return Ref(runs_a, np.asarray(lin, dtype=np.uint64), n_no_coor, out, lens, lin_off, recs)


def parsed(bai_bytes):
    """A `.bai` as comparable plain data: per reference ({bin: [(beg, end)]}, metadata or None,
    [offsets]) and the trailing n_no_coor (None when absent)."""
    b, p = bytes(bai_bytes), 8
    assert b[:4] == b"BAI\1"
    refs = []
    for _ in range(struct.unpack_from("<i", b, 4)[0]):
        n_bin = struct.unpack_from("<i", b, p)[0]
        p += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            bid, nch = struct.unpack_from("<Ii", b, p)
            p += 8
            ch = [struct.unpack_from("<QQ", b, p + 16 * k) for k in range(nch)]
            p += 16 * nch
            if bid == META_BIN:
                assert meta is None and nch == 2
                meta = (ch[0], ch[1])
            else:
                assert bid not in bins
                bins[bid] = ch
        n_intv = struct.unpack_from("<i", b, p)[0]
        p += 4
        offs = list(struct.unpack_from("<%dQ" % n_intv, b, p))
        p += 8 * n_intv
        refs.append((bins, meta, offs))
    n_no_coor = struct.unpack_from("<Q", b, p)[0] if p + 8 <= len(b) else None
    assert p + (8 if n_no_coor is not None else 0) == len(b)
    return refs, n_no_coor
