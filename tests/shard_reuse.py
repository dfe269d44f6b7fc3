"""Tenants and the stage tour for the reused-shard suite (test infrastructure; test_shard_reuse_gpu.py).

A shard is built to be reused: sbh_shard_load swaps the resident bytes and keeps every device buffer,
and the buffers only grow and are never cleared.  The suite runs every stage on one shard for one
file (the first tenant), loads another file into the same shard (the second tenant) and runs every
stage again; what the second tenant gets must be what a fresh shard gives and what the host computes.

Three tenants, built with record_corpus' rec / bgzf / header, seeds fixed, each well under 1 MB:

  BIG    leaves every reused buffer full of non-zero values: more than 2048 records in its first
         segment (the scans over n + 1 rows take their two-level path, the row kernels run several
         workgroups, the sort more than one tile), three references and a trailing run of records
         without one, coordinate order broken (the radix passes run) behind a sorted prefix (a BAI scan
         of the prefix succeeds and fills a linear index of several thousand windows; a scan of the whole
         is SBH_E_UNSORTED), unmapped reads with a position, rows with f and B:f tags (SAM's host rows),
         CIGARs above 32 ops, paired flags (FASTQ's parts), a valid record hidden in the last record's
         tag bytes (an eager false positive: the chain is marked through the bitmap, cm_*), an empty
         member in mid-file with a second segment of a few records behind it, a dozen data members.
  SMALL  three records on one reference, one data member and the EOF member; another dictionary
         (n_ref = 1), coordinate-sorted, no float tags, no empty member in mid-file.
  MID    257 records (one past a workgroup) on two references, sorted; record 100 ends on the last
         byte of a member, and so does the last record.
  MID_B  (the invalidation table only) MID with one malformed record of record_corpus behind its
         end-of-stream member, so that a records scan that fails exists; its first segment is MID's.

Every tenant is loaded as the tail of one imaginary file of FILE_SIZE bytes: sbh_shard_load keeps the
shard's file size, and a shard ends at EOF (closed end: no SBH_E_NEED_HALO) only when its bytes end
there.  tour() reports file offsets and virtual positions relative to the tenant's first byte, so
expected() does not depend on where the tenant was loaded.

tour(sh, ctx, tenant, path, off) runs every stage on a shard that holds the tenant's bytes and returns
a dict of comparable values; expected(name) is the same dict computed without a device: the flat
bytes from zlib, the block table from a host walk of the member headers (bai_ref.members), bits, full
words, FindRecordStart, counts and splits from the oracle (OracleFile, one per segment), the columns
from oracle_records.decode, the BAI scan from bai_ref.build, and the stage outputs from the library's
host entry points, which the stage tests hold to their numpy restatements (bam_gather_host,
bam_sort_host, sam_text_host, fastq_host, tally_host, depth_host, pileup_host).  Those live in the one
shared library; "without a device" means that no context, shard or accumulator is created.

Every tour entry has a CPU reference; none is compared to a fresh shard alone.  "run" exists only on
the "run" path (sbh_run_shard's result), every other key on both.
"""
import functools
import struct
from collections import namedtuple

import numpy as np

import bai_ref
import bam_sort_corpus as sc
import oracle_records as orr
from deflate_build import EOF_MEMBER
from oracle_lib import OR_OK, OracleFile
from pkg import sb
from record_corpus import D, EQ, I, M, MALFORMED_CASES, N, S, X, bgzf, header, rec

FILE_SIZE = 1 << 20
SBH_E_HIP, SBH_E_UNSORTED = 2, 21
STATUS_OF_ORACLE = {0: 0, 7: 11, 8: 16}  # OR_OK, OR_SEARCH_FAILED, OR_NO_READ_FOUND as SBH_* codes
U64_MAX = np.uint64(2 ** 64 - 1)

Tenant = namedtuple("Tenant", "name data contigs spans sorted_rows n_float n_long_cigar empty_index")


# ------------------------------------------------------------------------------------- builders

def read(ref, pos, cigar, flag=0, mapq=30, name=b"r", aux=b"", seed=0, l_seq=None):
    """A record valid for every stage: SEQ and QUAL as long as the CIGAR says (l_seq when there is
    none), a mate on the same reference for a paired flag."""
    n = sum(ln for ln, op in cigar if op in (M, I, S, EQ, X)) if l_seq is None else l_seq
    codes = tuple((3 * k + seed) % 16 for k in range(n))
    qual = bytes((7 * k + seed) % 94 for k in range(n))
    nref, npos = (ref, max(pos, 0) + 100) if flag & 1 and ref >= 0 else (-1, -1)
    return rec(ref, pos, mapq, 4681, flag, nref, npos, 0, name, tuple(cigar), codes, qual, aux, spare=0xF)


def long_cigar(k):
    ops = ((3, M), (1, I), (2, D), (2, EQ), (1, X), (2, N))
    return tuple(ops[j % 6] for j in range(33 + k % 9)) + ((2, M),)


FLAGS = (0, 0x10, 0x4, 0x100, 0x400, 0x200, 0x41, 0x81, 0x800, 0x53, 0xA1)


def _row(i, ref, pos):
    """Row i of BIG / MID: (bytes, has a float tag, has a long CIGAR)."""
    flag = FLAGS[i % len(FLAGS)]
    aux, is_float = b"", False
    if i % 50 == 7:
        aux, is_float = b"XFf" + struct.pack("<f", i / 8.0), True
    elif i % 75 == 11:
        aux, is_float = b"XBBf" + struct.pack("<iff", 2, i / 4.0, -1.5), True
    elif i % 3 == 0:
        aux = b"NMC" + bytes([i % 7]) + b"XZZt%d\0" % i
    is_long = i % 97 == 5 and not flag & 4
    if flag & 4:  # unmapped, placed
        b = read(ref, pos, (), flag, (i * 7) % 61, b"q%05d" % i, aux, i, l_seq=20 + i % 5)
    elif is_long:
        b = read(ref, pos, long_cigar(i), flag, (i * 7) % 61, b"q%05d" % i, aux, i)
    else:
        b = read(ref, pos, ((20 + i % 7, M),), flag, (i * 7) % 61, b"q%05d" % i, aux, i)
    return b, is_float, is_long


def no_ref(i, aux=b""):
    return read(-1, -1, (), 0x4 | (0x41 if i % 2 else 0), 0, b"u%05d" % i, aux, i, l_seq=15)


BIG_CONTIGS = (("big0", 30000000), ("big1", 25000000), ("big2", 20000))
BIG_PAYLOAD = 16000


@functools.lru_cache(maxsize=None)
def big():
    rng = np.random.default_rng(0xB16)
    rows, n_float, n_long = [], 0, 0

    def put(ref, pos):
        nonlocal n_float, n_long
        b, f, lg = _row(len(rows), ref, pos)
        rows.append(b)
        n_float, n_long = n_float + f, n_long + lg

    for ref, n, step, far in ((0, 700, 23, 29000000), (1, 700, 25, 24000000), (2, 400, 45, None)):
        for k in range(n):
            put(ref, 10 + step * k)
        if far is not None:  # the last window of the reference's linear index
            put(ref, far)
    n_sorted = len(rows)
    for k in range(240):  # coordinate order broken
        put(int(rng.integers(0, 2)), int(rng.integers(0, 18000)))
    for k in range(19):
        rows.append(no_ref(len(rows)))
    # a whole record in the last record's tag bytes, ending where that record ends: the eager check
    # passes there (the chain from it ends with the stream), and it is not a record of the chain
    hidden = no_ref(99999)
    rows.append(no_ref(len(rows), b"XBBC" + struct.pack("<i", len(hidden)) + hidden))
    seg1 = bgzf(header(BIG_CONTIGS) + b"".join(rows), BIG_PAYLOAD)  # (its EOF member is the one in mid-file)
    seg2 = bgzf(b"".join(read(0, 100 + 10 * k, ((25, M),), name=b"s%d" % k, seed=k) for k in range(5)), BIG_PAYLOAD)
    spans = [(0, 0, 20000), (1, 0, 20000), (2, 0, 20000)]
    empty = bai_ref.members(seg1)[0][-1][0]
    return Tenant("BIG", seg1 + seg2, BIG_CONTIGS, spans, (0, n_sorted), n_float, n_long, empty)


SMALL_CONTIGS = (("s0", 5000),)


@functools.lru_cache(maxsize=None)
def small():
    rows = [read(0, 100, ((30, M),), 0, 40, b"a"), read(0, 200, ((10, M), (2, I), (10, M)), 0x10, 20, b"b", b"NMC\2"),
            read(0, 300, ((25, M),), 0, 3, b"c")]
    return Tenant("SMALL", bgzf(header(SMALL_CONTIGS) + b"".join(rows), 65280), SMALL_CONTIGS, [(0, 0, 5000)], (0, 3),
                  0, 0, None)


MID_CONTIGS = (("m0", 100000), ("m1", 40000))
MID_PAYLOAD = 4096
MID_ENDS_MEMBER = 100  # the row padded to end on the last byte of a member


def _mid_rows():
    rows, n_long = [], 0
    for i in range(257):
        ref, pos = (0, 50 + 61 * i) if i < 150 else (1, 20 + 37 * (i - 150))
        flag = (0, 0x10, 0x4, 0x400)[i % 4]
        cigar = () if flag & 4 else long_cigar(i) if i % 97 == 5 else ((20 + i % 7, M),)
        n_long += i % 97 == 5 and not flag & 4
        aux = b"NMC" + bytes([i % 5]) if i % 2 else b""
        if i == MID_ENDS_MEMBER:
            before = len(header(MID_CONTIGS)) + sum(len(r) for r in rows)
            base = len(read(ref, pos, cigar, flag, i % 61, b"m%04d" % i, b"XZZ\0", i, l_seq=18 if flag & 4 else None))
            aux = b"XZZ" + b"p" * (-(before + base) % MID_PAYLOAD) + b"\0"
        rows.append(read(ref, pos, cigar, flag, i % 61, b"m%04d" % i, aux, i, l_seq=18 if flag & 4 else None))
    return rows, n_long


@functools.lru_cache(maxsize=None)
def mid():
    rows, n_long = _mid_rows()
    return Tenant("MID", bgzf(header(MID_CONTIGS) + b"".join(rows), MID_PAYLOAD), MID_CONTIGS,
                  [(0, 0, 20000), (1, 0, 20000)], (0, 257), 0, n_long, None)


@functools.lru_cache(maxsize=None)
def mid_b():
    """MID, then (behind its end-of-stream member) record_corpus' l_seq_minus_one record alone."""
    m = mid()
    bad = [c for c in MALFORMED_CASES if c.name == "l_seq_minus_one"][0]
    tail = bytes(bad.stream.flat[bad.bad_start:])
    return m._replace(name="MID_B", data=m.data + bgzf(tail, MID_PAYLOAD), empty_index=len(m.data) - len(EOF_MEMBER))


TENANTS = {"BIG": big, "SMALL": small, "MID": mid, "MID_B": mid_b}


def tenant(name):
    return TENANTS[name]()


def data_of(name):
    return np.frombuffer(tenant(name).data, np.uint8)


def offset_of(name):
    """Where the tenant lies in the imaginary file: its last byte is the file's last."""
    return FILE_SIZE - len(tenant(name).data)


# ------------------------------------------------------------------------------------- the layout

Layout = namedtuple("Layout", "members flat names lens first seg_end starts all_starts sub head n_ref")


def is_empty_member(data, p, csize):
    return csize == len(EOF_MEMBER) and bytes(data[p:p + 20]) == EOF_MEMBER[:20]


@functools.lru_cache(maxsize=None)
def layout(name):
    """What the host knows of the tenant before any stage runs: members, flat bytes, header, the first
    segment's record starts (the rows of every scan) and the sub-range the tour also asks for."""
    t = tenant(name)
    members, flat = bai_ref.members(t.data)
    names, first = orr.bam_refs(flat)
    lens = np.asarray([ln for _, ln in t.contigs], np.int32)
    assert names == [n for n, _ in t.contigs]
    empties = [u for p, cs, u, us in members if is_empty_member(t.data, p, cs)]
    seg_end = empties[0]
    starts = orr.record_starts(flat, first, seg_end)
    all_starts = orr.record_starts(flat, first, len(flat))
    n = len(starts)
    sub = (starts[n // 3], starts[2 * n // 3] + 1)
    return Layout(members, flat, names, lens, first, seg_end, starts, all_starts, sub, bytes(flat[:first]), len(lens))


def rows_for(n):
    """Row ranges valid for any n >= 3: the first row, a middle stretch over a wave edge, the last."""
    return [(0, 1), (n - 1, n)] if n < 10 else [(0, 1), (n // 3, n // 3 + 70 if n > 300 else n // 3 + 2), (n - 1, n)]


def filters(n):
    return {"bam": {"rows": rows_for(n), "flag_exclude": 0x400}, "tally": {"flag_exclude": 0x200},
            "depth": {"flag_exclude": 0x704, "rows": rows_for(n)}, "pileup": {"min_mapq": 7}}


def splits_of(size):
    return sb.file_splits(size, size // 3 + 1)


def vpos_of(members, flats):
    """htsjdk virtual positions of flat positions: canonical (a position at a member's end is the next
    member with bytes, offset 0), relative to the tenant's first byte."""
    live = [(p, u) for p, cs, u, us in members if us > 0]
    ust = np.asarray([u for _, u in live], np.int64)
    pst = np.asarray([p for p, _ in live], np.uint64)
    f = np.asarray(flats, np.int64)
    k = np.searchsorted(ust, f, side="right") - 1
    return (pst[k] << np.uint64(16)) | (f - ust[k]).astype(np.uint64)


# ------------------------------------------------------------------------------------- comparing

def same(a, b):
    """Exact equality of two tour values (dicts, sequences, arrays, bytes, ints)."""
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)) or isinstance(b, (tuple, list)):
        return (isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b)
                and all(same(x, y) for x, y in zip(a, b)))
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(bytes(a), np.uint8)
    if isinstance(b, (bytes, bytearray)):
        b = np.frombuffer(bytes(b), np.uint8)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        if not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray)) or a.shape != b.shape:
            return False
        if a.dtype.names or b.dtype.names:
            return a.dtype == b.dtype and a.tobytes() == b.tobytes()
        if a.dtype.kind in "iu" and b.dtype.kind in "iu" and a.dtype != b.dtype:  # (by value: the oracle's are signed)
            return all(int(x) == int(y) for x, y in zip(a.ravel().tolist(), b.ravel().tolist()))
        return bool(np.array_equal(a, b))
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (bool, np.bool_)) or isinstance(b, (bool, np.bool_)):
        return bool(a) == bool(b) and isinstance(a, (bool, np.bool_)) == isinstance(b, (bool, np.bool_))
    return int(a) == int(b) if isinstance(a, (int, np.integer)) and isinstance(b, (int, np.integer)) else a == b


def differing(got, want):
    """The keys of two tour dicts whose values differ (a key one of them lacks differs)."""
    return sorted(k for k in set(got) | set(want) if k not in got or k not in want or not same(got[k], want[k]))


def attempt(f, *a, **kw):
    """f(*a), or ("error", code, fields) for the library's refusal.  A device error ends the session:
    nothing more runs on this GPU."""
    try:
        return f(*a, **kw)
    except sb.SparkBamError as e:
        if e.code == SBH_E_HIP:
            import pytest
            pytest.exit("HIP error: %s" % e, returncode=3)
        return ("error", int(e.code), tuple(int(x) for x in e.fields))


# ------------------------------------------------------------------------------------- the tour

def unshift_vpos(v, off):
    """Virtual positions of a shard at file offset off, relative to the tenant's first byte."""
    v = np.asarray(v, np.uint64).copy()
    live = v != U64_MAX
    v[live] -= np.uint64(off << 16)
    return v


def bai_value(got, off):
    if isinstance(got, tuple) and got and isinstance(got[0], str):
        return (got[0], got[1], tuple(x - (off << 16) for x in got[2]))
    runs, lin, nnc = got
    runs = runs.copy()
    runs["vbeg"] -= np.uint64(off << 16)
    runs["vend"] -= np.uint64(off << 16)
    return (runs, unshift_vpos(lin, off), int(nnc))


def tour(sh, ctx, name, path, off=0):
    """Every stage on `sh`, which holds tenant `name` at file offset off: a dict of comparable values.
    path "steps": index, inflate, set_contigs, check_eager; "run": set_contigs, sbh_run_shard."""
    t, L = tenant(name), layout(name)
    size, n = len(t.data), len(L.starts)
    F = filters(n)
    out = {}
    if path == "steps":
        out["index"] = attempt(sh.index, off)
        attempt(sh.inflate)
        sh.set_contigs(L.lens)
        out["eager"] = attempt(sh.check_eager, 0, sh.flat_size)
    else:
        sh.set_contigs(L.lens)
        r = attempt(sh.run, off, off + size)
        if isinstance(r, dict):
            sh.n_blocks, sh.flat_size = r["n_blocks"], r["flat_bytes"]
            out["index"] = (r["n_blocks"], r["flat_bytes"])
            out["eager"] = (r["n_true"], attempt(sh.eager_bits, 0, sh.flat_size))
            r = dict(r, first_vpos=r["first_vpos"] - (off << 16))
        out["run"] = r
    b = sh.block_arrays()
    out["blocks"] = dict(b, start=b["start"] - np.uint64(off))
    out["flat"] = attempt(sh.read_flat, 0, sh.flat_size)
    out["crc"] = attempt(sh.verify_crc)
    full = attempt(sh.check_full, 0, min(65536, L.seg_end), want_words=True)
    out["full"] = {k: full[k] for k in ("n_success", "counts", "rbe", "words")} if isinstance(full, dict) else full
    out["find_record_start"] = attempt(sh.find_record_start, 0)
    out["count"] = [attempt(sh.count_records, a, e) for a, e in ((L.first, L.seg_end), L.sub)]
    out["chain"] = [attempt(sh.chain_from, a, e) for a, e in ((L.first, L.seg_end), L.sub)]
    splits = [(a + off, e + off) for a, e in splits_of(size)]
    st = attempt(sh.split_starts, splits)
    if len(st) == 4:
        status, v, c, _ = st
        st = (status, np.where(c > 0, v - np.uint64(off << 16), 0).astype(np.uint64), c)
    out["split_starts"] = st
    bt = attempt(sh.split_records_batch, splits)
    if len(bt) == 3 and isinstance(bt[0], dict):
        info, per, cols = bt
        bt = ([(s["status"], s["rec_begin"], s["rec_count"], s["first_vpos"] - (off << 16) if s["rec_count"] else 0)
               for s in per], dict(cols, vpos=unshift_vpos(cols["vpos"], off)))
    out["split_batch"] = bt
    cols = attempt(sh.records, L.first, L.seg_end)
    out["records"] = dict(cols, vpos=unshift_vpos(cols["vpos"], off)) if isinstance(cols, dict) else cols
    sam = attempt(sh.records_sam, L.names)
    out["sam"] = sam + (sh.sam_n_host,) if len(sam) == 2 else sam
    out["bam_scan"] = attempt(sh.records_bam, L.head, F["bam"])
    out["bam_coord"] = (attempt(sh.records_bam, L.head, None, order="coordinate"), attempt(lambda: sh.bam_sorted))
    for key, split in (("fastq", False), ("fastq_split", True)):
        fq = attempt(sh.records_fastq, None, split=split)
        out[key] = fq + (sh.fastq_sizes,) if len(fq) == 3 and not isinstance(fq[0], str) else fq
    out["bai_whole"] = bai_value(attempt(sh.bai_scan, L.first, L.seg_end), off)
    a, e = t.sorted_rows
    out["bai"] = bai_value(attempt(sh.bai_scan, L.starts[a], L.starts[e] if e < n else L.seg_end), off)
    out["bai_edges"] = attempt(sh.bai_edges)
    # the records scan again: the BAI scans above walked ranges of their own
    attempt(sh.records_scan, L.first, L.seg_end)
    tal, dep, pil = ctx.tally(L.n_ref), ctx.depth(t.spans, L.n_ref), ctx.pileup(t.spans, L.n_ref)
    try:
        out["tally"] = (attempt(tal.add, sh, F["tally"]), attempt(tal.counts))
        out["depth"] = (attempt(dep.add, sh, F["depth"]), attempt(dep.finish), attempt(dep.runs),
                        [attempt(dep.depth, k) for k in range(len(t.spans))])
        out["pileup"] = (attempt(pil.add, sh, F["pileup"]), attempt(pil.finish), attempt(pil.intervals),
                         [attempt(pil.counts, k) for k in range(len(t.spans))],
                         [attempt(pil.calls, k) for k in range(len(t.spans))])
    finally:
        for acc in (tal, dep, pil):
            acc.close()
    return out


RUN_ONLY = {"run"}


def keys_for(name, path):
    return set(expected(name)) - (RUN_ONLY if path == "steps" else set())


# ------------------------------------------------------------------------------------- expected

def segments(name):
    """[(file offset of the segment's first member, flat begin, flat end)] of the segments with bytes:
    an empty member ends one."""
    t, L = tenant(name), layout(name)
    out, cur = [], None
    for p, cs, u, us in L.members:
        if is_empty_member(t.data, p, cs):
            if cur is not None:
                out.append(cur + (u,))
            cur = None
        elif cur is None:
            cur = (p, u)
    assert cur is None  # (every tenant ends with the EOF member)
    return out


@functools.lru_cache(maxsize=None)
def eager_expected(name, from_member=0):
    """(set bits, the bitmap packed LSB first) of the eager check over the flat stream from member
    `from_member` on: one oracle stream per segment (the reference's stream ends at an empty member)."""
    t, L = tenant(name), layout(name)
    data = np.frombuffer(t.data, np.uint8)
    p0, u0 = L.members[from_member][0], L.members[from_member][2]
    total, bits = 0, []
    for p, ub, ue in segments(name):
        if ue <= u0:
            continue
        of = OracleFile(data, start=max(p, p0))
        of.contig_len = L.lens
        lo = max(ub, u0)
        assert of.flat_size == ue - lo
        k, b = of.eager_range(0, ue - lo)
        total += k
        bits.append(np.unpackbits(b, bitorder="little")[:ue - lo])
        of.close()
    return total, np.packbits(np.concatenate(bits), bitorder="little")


def bai_expected(name, rows):
    try:
        r = bai_ref.build(tenant(name).data, rows)
    except bai_ref.Unsorted as e:
        return ("error", SBH_E_UNSORTED, (e.vpos,))
    return (r.runs, r.lin, r.n_no_coor)


def edges_expected(name, rows):
    recs = bai_ref.records_of(tenant(name).data)[0][rows[0]:rows[1]]
    placed = [r for r in recs if r.ref_id >= 0]
    first = (recs[0].ref_id, recs[0].pos) if recs else (-1, 0)
    return first + ((placed[-1].ref_id, placed[-1].pos) if placed else (-1, 0))


def columns_expected(name, starts):
    L = layout(name)
    cols = orr.decode(L.flat, starts)
    cols["vpos"] = vpos_of(L.members, starts) if len(starts) else np.zeros(0, np.uint64)
    return cols


def coordinate_expected(name, starts, head):
    """(stream, rec_off, rows) of the coordinate-order call over all rows, and whether they were in
    order already: the permutation is the library's host function's, the bytes are laid here."""
    L = layout(name)
    flat = np.frombuffer(L.flat, np.uint8)
    perm = sb.bam_sort_host(flat, starts)
    parts = [L.flat[starts[int(r)]:starts[int(r)] + 4 + struct.unpack_from("<i", L.flat, starts[int(r)])[0]] for r in perm]
    off = np.cumsum([len(head)] + [len(p) for p in parts]).astype(np.uint64)
    return (np.frombuffer(head + b"".join(parts), np.uint8), off, perm), descents(name, starts) == 0


def descents(name, starts=None):
    """Adjacent rows (of the first segment, or those at `starts`) out of coordinate order, by
    bam_sort_corpus' key."""
    L = layout(name)
    k = sc.keys_of(L.flat, L.starts if starts is None else starts)
    return int(np.count_nonzero(k[1:] < k[:-1]))


def stage_expected(name, starts, head, F):
    """The outputs of the stages over the rows at `starts`, from the library's host entry points."""
    t, L = tenant(name), layout(name)
    flat = np.frombuffer(L.flat, np.uint8)
    out = {}
    text, line_off = sb.sam_text_host(flat, starts, L.names)
    out["sam"] = (text, line_off)
    out["bam_scan"] = sb.bam_gather_host(flat, starts, head, F["bam"])
    for key, split in (("fastq", False), ("fastq_split", True)):
        out[key] = sb.fastq_host(flat, starts, None, split=split)
    flag, ref, n_kept = sb.tally_host(flat, starts, L.n_ref, F["tally"])
    out["tally"] = ({"n": len(starts), "n_kept": n_kept}, (flag, ref))
    add, depth, runs, sizes = sb.depth_host(flat, starts, t.spans, L.n_ref, F["depth"])
    per, o = [], 0
    for _, b, e in t.spans:  # (the host's depth has one extra slot behind each span)
        per.append(depth[o:o + e - b])
        o += e - b + 1
    out["depth"] = (add, sizes, runs, per)
    add, counts, calls, iv, sizes = sb.pileup_host(flat, starts, t.spans, L.n_ref, F["pileup"])
    cper, kper, o = [], [], 0
    for _, b, e in t.spans:
        cper.append(counts[o:o + e - b])
        kper.append(calls[o:o + e - b])
        o += e - b
    out["pileup"] = (add, sizes, iv, cper, kper)
    return out


def chain_expected(name, a, e):
    """(records of the chain from a that start below e, the first chain record at or after e)."""
    L = layout(name)
    inside = [s for s in L.starts if a <= s < e]
    after = [s for s in L.starts if s >= e]
    return len(inside), (after[0] if after else L.seg_end)


@functools.lru_cache(maxsize=None)
def expected(name):
    t, L = tenant(name), layout(name)
    data = np.frombuffer(t.data, np.uint8)
    size, n = len(t.data), len(L.starts)
    F = filters(n)
    of = OracleFile(data)
    assert of.flat_size == L.seg_end and of.header_end == L.first and np.array_equal(of.contig_len, L.lens)
    out = {"index": (len(L.members), len(L.flat))}
    out["blocks"] = {
        "start": np.asarray([p for p, cs, u, us in L.members], np.uint64),
        "ustart": np.asarray([u for p, cs, u, us in L.members], np.uint64),
        "usize": np.asarray([us for p, cs, u, us in L.members], np.uint64),
        "csize": np.asarray([cs for p, cs, u, us in L.members], np.uint64),
        "flags": np.asarray([sb.BLOCK_EMPTY if is_empty_member(t.data, p, cs) else 0 for p, cs, u, us in L.members],
                            np.uint32)}
    out["flat"] = np.frombuffer(L.flat, np.uint8)
    out["crc"] = (0, 0)
    out["eager"] = eager_expected(name)
    E = min(65536, L.seg_end)
    ns, counts, rbe, words = of.full_range(0, E, want_words=True)
    out["full"] = {"n_success": ns, "counts": counts, "rbe": rbe, "words": words}
    rc, first, delta = of.find_record_start(0)
    assert rc == OR_OK and first == L.first
    out["find_record_start"] = (first, delta)
    ranges = ((L.first, L.seg_end), L.sub)
    out["chain"] = [chain_expected(name, a, e) for a, e in ranges]
    out["count"] = [c for c, _ in out["chain"]]
    # splits: the oracle's (status, first record, count) per split; the batch's rows are the count
    # records of the chain from that first record
    all_vpos = vpos_of(L.members, L.all_starts)
    status, firsts, cnts, per, rows = [], [], [], [], []
    for a, e in splits_of(size):
        rc, v, c = of.split(a, e)
        status.append(STATUS_OF_ORACLE[rc])
        c = c if rc == OR_OK else 0
        firsts.append(v if c else 0)
        cnts.append(c)
        per.append((STATUS_OF_ORACLE[rc], len(rows), c, v if c else 0))
        if c:
            k = int(np.flatnonzero(all_vpos == np.uint64(v))[0])
            rows += L.all_starts[k:k + c]
    out["split_starts"] = (np.asarray(status, np.int32), np.asarray(firsts, np.uint64), np.asarray(cnts, np.uint64))
    out["split_batch"] = (per, columns_expected(name, rows))
    out["records"] = columns_expected(name, L.starts)
    st = stage_expected(name, L.starts, L.head, F)
    out["sam"] = st.pop("sam") + (t.n_float,)
    out.update(st)
    out["bam_coord"] = coordinate_expected(name, L.starts, L.head)
    out["bai_whole"] = bai_expected(name, (0, n))
    out["bai"] = bai_expected(name, t.sorted_rows)
    out["bai_edges"] = edges_expected(name, t.sorted_rows)
    out["run"] = {"n_blocks": len(L.members), "comp_bytes": size, "flat_bytes": len(L.flat), "n_true": out["eager"][0],
                  "first_vpos": int(vpos_of(L.members, [L.first])[0]), "count": n, "exit_flat": L.seg_end, "status": 0,
                  "anomalies": false_positives(name)}
    of.close()
    return out


def false_positives(name):
    """Eager-true positions of the first segment's record range that are not records of the chain."""
    L = layout(name)
    bits = np.unpackbits(eager_expected(name)[1], bitorder="little")
    assert all(bits[s] for s in L.starts)
    return int(bits[L.first:L.seg_end].sum()) - len(L.starts)
