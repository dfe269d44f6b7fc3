"""Columnar BAM records decoded on the GPU (sbh_records_scan / sbh_records_fetch) and
their SAM text.

The reference hands htsjdk SAMRecords out of RecordStream / CanLoadBam.loadReads
(check/.../iterator/RecordStream.scala:16-41, load/.../CanLoadBam.scala:244-264); here a
batch is a set of numpy columns filled by libsparkbam_hip.so.  `sam_line` renders one
record the way htsjdk's SAMRecord.getSAMString does (the format of the reference's
test_bams/*.sam files), for inspection and tests; the decode itself is the GPU's.
"""
import struct

import numpy as np

CIGAR_OPS = "MIDNSHP=X"

# The columns sbh_records_fetch fills (sbh_records_out field order): name -> (dtype, length
# from (n, name_bytes, cigar_ops, bases, aux_bytes)).  Offset columns hold n + 1 entries.
RECORD_COLUMNS = (
    ("flat", np.uint64, lambda n, nm, cg, bs, ax: n), ("ref_id", np.int32, lambda n, *_: n),
    ("pos", np.int32, lambda n, *_: n), ("next_ref_id", np.int32, lambda n, *_: n),
    ("next_pos", np.int32, lambda n, *_: n), ("tlen", np.int32, lambda n, *_: n),
    ("flag", np.uint16, lambda n, *_: n), ("bin", np.uint16, lambda n, *_: n),
    ("mapq", np.uint8, lambda n, *_: n), ("name_off", np.uint64, lambda n, *_: n + 1),
    ("cigar_off", np.uint64, lambda n, *_: n + 1), ("seq_off", np.uint64, lambda n, *_: n + 1),
    ("aux_off", np.uint64, lambda n, *_: n + 1), ("names", np.uint8, lambda n, nm, cg, bs, ax: nm),
    ("cigar", np.uint32, lambda n, nm, cg, bs, ax: cg), ("seq", np.uint8, lambda n, nm, cg, bs, ax: bs),
    ("qual", np.uint8, lambda n, nm, cg, bs, ax: bs), ("aux", np.uint8, lambda n, nm, cg, bs, ax: ax),
)


def record_columns(n=0, name_bytes=0, cigar_ops=0, bases=0, aux_bytes=0):
    """Uninitialised columns for n records (offset columns zeroed when n == 0, so an empty
    batch has the same schema as a full one)."""
    z = (n, name_bytes, cigar_ops, bases, aux_bytes)
    cols = {k: (np.zeros if n == 0 else np.empty)(f(*z), dt) for k, dt, f in RECORD_COLUMNS}
    return cols


# packed column -> the [n + 1] offsets addressing it
PACKED = {"names": "name_off", "cigar": "cigar_off", "seq": "seq_off", "qual": "seq_off", "aux": "aux_off"}


def slice_columns(cols, a, b, copy=True):
    """Rows [a, b) of a column batch as a batch of its own: fixed columns sliced, packed columns
    cut at their offsets, the offsets rebased to start at 0.  copy=False: views of the batch's
    arrays (only the small offset columns are new), for a batch nobody else writes.  Columns the
    batch does not hold (a starts-only batch) are skipped."""
    out = {}
    for k, v in cols.items():
        if k in PACKED:
            o = cols[PACKED[k]]
            out[k] = v[int(o[a]):int(o[b])]
        elif k in PACKED.values():
            out[k] = v[a:b + 1] - v[a]
            continue
        else:
            out[k] = v[a:b]
        if copy:
            out[k] = out[k].copy()
    return out


_B_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}


def _java_float(x):
    """java.lang.Float.toString for the finite values a BAM 'f' tag holds."""
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "Infinity" if x > 0 else "-Infinity"
    for p in range(1, 10):  # shortest digits that read back as the same float32
        s = "%.*g" % (p, x)
        if np.float32(float(s)) == np.float32(x):
            break
    if "e" in s or "E" in s:
        m, e = s.split("e")
        if "." not in m:
            m += ".0"
        return "%sE%d" % (m, int(e))
    return s if "." in s else s + ".0"


def tags_text(aux):
    """The SAM text of a record's raw tag bytes (TAG:TYPE:VALUE, tab separated)."""
    out, i, b = [], 0, bytes(aux)
    while i + 3 <= len(b):
        tag, t = b[i:i + 2].decode("ascii"), chr(b[i + 2])
        i += 3
        if t == "A":
            out.append("%s:A:%s" % (tag, chr(b[i])))
            i += 1
        elif t in "cCsSiI":
            fmt = _B_FMT[t]
            n = struct.calcsize(fmt)
            out.append("%s:i:%d" % (tag, struct.unpack_from("<" + fmt, b, i)[0]))
            i += n
        elif t == "f":
            out.append("%s:f:%s" % (tag, _java_float(struct.unpack_from("<f", b, i)[0])))
            i += 4
        elif t in "ZH":
            j = b.index(b"\0", i)
            out.append("%s:%s:%s" % (tag, t, b[i:j].decode("latin-1")))
            i = j + 1
        elif t == "B":
            sub, n = chr(b[i]), struct.unpack_from("<i", b, i + 1)[0]
            i += 5
            fmt = _B_FMT[sub]
            vals = struct.unpack_from("<%d%s" % (n, fmt), b, i)
            i += n * struct.calcsize(fmt)
            txt = ",".join(_java_float(v) if sub == "f" else str(v) for v in vals)
            out.append("%s:B:%s%s" % (tag, sub, "," + txt if n else ""))
        else:
            raise ValueError("unknown tag type %r" % t)
    return out


def pack_ref_names(ref_names):
    """Contig names (str or bytes) packed for the C-ABI: (uint8 bytes, uint64 [n + 1] offsets)."""
    raw = [n if isinstance(n, (bytes, bytearray)) else str(n).encode("latin-1") for n in ref_names]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    if raw:
        off[1:] = np.cumsum([len(r) for r in raw])
    return np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8), off


def sam_text_host(flat, starts, ref_names, want_text=True):
    """The SAM text of the records at `starts` of a flat BAM stream, rendered on the host by the
    library (sbh_sam_render_host: no GPU, the renderer the device path shares its definition with
    and uses for rows with float tags): (text as uint8, line_off uint64 [n + 1]); want_text=False:
    (None, line_off).  Raises SparkBamError(SBH_E_BAD_RECORD) with `.fields = (row,)` for the first
    malformed record.  Unlike sam_line / tags_text it refuses a malformed tag area, as htsjdk does."""
    import ctypes as C

    from ._lib import SBH_OK, SparkBamError, lib
    flat = np.ascontiguousarray(np.frombuffer(flat, dtype=np.uint8) if not isinstance(flat, np.ndarray) else flat)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    names, off = pack_ref_names(ref_names)
    line_off = np.zeros(st.size + 1, dtype=np.uint64)
    bad = C.c_uint64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(text):
        rc = lib().sbh_sam_render_host(p(flat), flat.size, p(st), st.size, p(names), p(off), off.size - 1,
                                       p(text) if text is not None and text.size else None,
                                       0 if text is None else text.size, p(line_off), C.byref(bad))
        if rc != SBH_OK:
            raise SparkBamError(rc, "record %d is malformed" % bad.value if rc == 20 else "sam_text_host", (bad.value,))
    call(None)
    if not want_text:
        return None, line_off
    text = np.empty(int(line_off[-1]), dtype=np.uint8)
    if text.size:
        call(text)
    return text, line_off


def record_filter(filter):
    """sbh_record_filter from None (keep all) or a dict with any of flag_require, flag_exclude,
    min_mapq and rows -- [(begin, end), ...] half-open row ranges, sorted and disjoint.  Returns
    (ctypes struct or None, the arrays it points into)."""
    from ._lib import SbhRecordFilter
    if filter is None:
        return None, ()
    unknown = set(filter) - {"flag_require", "flag_exclude", "min_mapq", "rows"}
    if unknown:
        raise ValueError("record filter: unknown keys %s" % sorted(unknown))
    rows = filter.get("rows")
    rb = np.ascontiguousarray([a for a, _ in rows] if rows is not None else [], dtype=np.uint64)
    re_ = np.ascontiguousarray([b for _, b in rows] if rows is not None else [], dtype=np.uint64)
    if rows is not None and not rb.size:  # no rows asked for: one range no row lies in
        rb, re_ = np.asarray([2 ** 64 - 2], np.uint64), np.asarray([2 ** 64 - 1], np.uint64)
    f = SbhRecordFilter(int(filter.get("flag_require", 0)) & 0xFFFFFFFF, int(filter.get("flag_exclude", 0)) & 0xFFFFFFFF,
                        int(filter.get("min_mapq", 0)), 0, rb.ctypes.data if rb.size else None,
                        re_.ctypes.data if rb.size else None, int(rb.size))
    return f, (rb, re_)


def row_ranges(rows):
    """Sorted, disjoint half-open ranges [(begin, end), ...] holding exactly the given row
    indices (a range, or any iterable of ints; duplicates count once)."""
    if isinstance(rows, range) and rows.step == 1:
        return [(rows.start, rows.stop)] if rows.stop > rows.start else []
    a = np.unique(np.fromiter((int(i) for i in rows), dtype=np.int64))
    if not a.size:
        return []
    cut = np.flatnonzero(np.diff(a) != 1)
    begins = np.concatenate(([a[0]], a[cut + 1]))
    ends = np.concatenate((a[cut], [a[-1]])) + 1
    return [(int(b), int(e)) for b, e in zip(begins, ends)]


def bam_gather_host(flat, starts, head=b"", filter=None):
    """The BAM stream Shard.records_bam builds on the GPU, gathered on the host by the library
    (sbh_bam_gather_host: no GPU, the definition the device path shares): head, then the raw
    bytes of the records at starts[] that the filter keeps.  Returns (stream uint8, rec_off
    uint64 [n_kept + 1], rows uint64 [n_kept]).  Raises SparkBamError(SBH_E_BAD_RECORD) with
    `.fields = (row,)` for the first invalid record, kept or not."""
    import ctypes as C

    from ._lib import SBH_OK, SparkBamError, lib
    flat = np.ascontiguousarray(np.frombuffer(flat, dtype=np.uint8) if not isinstance(flat, np.ndarray) else flat)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    hd = np.frombuffer(bytes(head), dtype=np.uint8)
    f, keep = record_filter(filter)
    rec_off = np.zeros(st.size + 1, dtype=np.uint64)
    rows = np.zeros(max(st.size, 1), dtype=np.uint64)
    n_kept, bad = C.c_uint64(), C.c_uint64()
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731

    def call(out):
        rc = lib().sbh_bam_gather_host(p(flat), flat.size, p(st), st.size, p(hd), hd.size,
                                       C.byref(f) if f is not None else None, None if out is None else p(out),
                                       0 if out is None else out.size, p(rec_off), p(rows), C.byref(n_kept),
                                       C.byref(bad))
        if rc != SBH_OK:
            raise SparkBamError(rc, "record %d is malformed" % bad.value if rc == 20 else "bam_gather_host", (bad.value,))
    call(None)
    out = np.empty(int(rec_off[n_kept.value]), dtype=np.uint8)
    if out.size:
        call(out)
    del keep
    return out, rec_off[:n_kept.value + 1].copy(), rows[:n_kept.value].copy()


def bam_sort_host(flat, starts):
    """The permutation Shard.records_bam(order="coordinate") applies on the GPU, computed on the
    host by the library (sbh_bam_sort_host: no GPU, the key the device path shares): perm[k] = the
    index into starts[] of the record that comes k-th in stable coordinate order (reference,
    position, reverse strand; unplaced last; ties in starts[] order).  Raises
    SparkBamError(SBH_E_BAD_RECORD) with `.fields = (row,)` for the first invalid record."""
    import ctypes as C

    from ._lib import SBH_OK, SparkBamError, lib
    flat = np.ascontiguousarray(np.frombuffer(flat, dtype=np.uint8) if not isinstance(flat, np.ndarray) else flat)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    perm = np.zeros(st.size, dtype=np.uint64)
    bad = C.c_uint64()
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    rc = lib().sbh_bam_sort_host(p(flat), flat.size, p(st), st.size, p(perm), C.byref(bad))
    if rc != SBH_OK:
        raise SparkBamError(rc, "record %d is malformed" % bad.value if rc == 20 else "bam_sort_host", (bad.value,))
    return perm


def bam_name_sort_host(flat, starts):
    """The permutation Shard.records_bam(order="name") applies on the GPU, computed on the host by
    the library (sbh_bam_name_sort_host: no GPU, the order the device path shares): (perm, info),
    perm[k] = the index into starts[] of the record that comes k-th in stable read-name order (names
    as unsigned bytes, a prefix first; then READ1 / READ2, primary, secondary, supplementary; ties
    in starts[] order), info = Shard.bam_name_info's dict with chunks_run = passes_run = 0.  Raises
    SparkBamError(SBH_E_BAD_RECORD) with `.fields = (row,)` for the first invalid record."""
    import ctypes as C

    from ._lib import SBH_OK, SbhBamNameInfo, SparkBamError, lib
    flat = np.ascontiguousarray(np.frombuffer(flat, dtype=np.uint8) if not isinstance(flat, np.ndarray) else flat)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    perm = np.zeros(st.size, dtype=np.uint64)
    bad, info = C.c_uint64(), SbhBamNameInfo()
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    rc = lib().sbh_bam_name_sort_host(p(flat), flat.size, p(st), st.size, p(perm), C.byref(info), C.byref(bad))
    if rc != SBH_OK:
        raise SparkBamError(rc, "record %d is malformed" % bad.value if rc == 20 else "bam_name_sort_host", (bad.value,))
    out = {k: int(getattr(info, k)) for k, _ in SbhBamNameInfo._fields_}
    out["already"] = bool(out["already"])
    return perm, out


def bam_header_set_so(head, so):
    """The BAM header bytes (magic, l_text, text, references) with the @HD line's SO: set to `so`
    (sbh_bam_header_set_so, host only)."""
    import ctypes as C

    from ._lib import SBH_OK, SparkBamError, lib
    hd = np.frombuffer(bytes(head), dtype=np.uint8)
    so = so.encode("ascii") if isinstance(so, str) else bytes(so)
    out = np.empty(hd.size + 20 + len(so), dtype=np.uint8)
    n = C.c_uint64()
    rc = lib().sbh_bam_header_set_so(hd.ctypes.data_as(C.c_void_p) if hd.size else None, hd.size, so,
                                     out.ctypes.data_as(C.c_void_p), out.size, C.byref(n))
    if rc != SBH_OK:
        raise SparkBamError(rc, "bam_header_set_so: not a BAM header, or not a sort-order value")
    return out[:n.value].tobytes()


class Reads:
    """A decoded batch: fixed fields as arrays, variable-length fields packed."""

    def __init__(self, cols, ref_names):
        self.cols = cols
        self.ref_names = list(ref_names)
        self.n = int(cols["flat"].size)

    def __len__(self):
        return self.n

    OFFSETS = {"name_off": "names", "cigar_off": "cigar", "seq_off": "seq", "aux_off": "aux"}

    @classmethod
    def concat(cls, batches, ref_names):
        """One batch of the records of several, in order (windowed loadReads, api.iter_reads)."""
        batches = [b for b in batches if b.n]
        if not batches:
            cols = record_columns()
            cols["vpos"] = np.empty(0, np.uint64)
            return cls(cols, ref_names)
        cols = {}
        for k in batches[0].cols:
            if k in cls.OFFSETS:
                parts, base = [], 0
                for b in batches:
                    o = b.cols[k]
                    parts.append(o[:-1] + base)
                    base += int(o[-1])
                parts.append(np.asarray([base], dtype=batches[0].cols[k].dtype))
                cols[k] = np.concatenate(parts)
            else:
                cols[k] = np.concatenate([b.cols[k] for b in batches])
        return cls(cols, ref_names)

    def _slice(self, name, off, i):
        o = self.cols[off]
        return self.cols[name][int(o[i]):int(o[i + 1])]

    def name(self, i):
        return bytes(self._slice("names", "name_off", i)).split(b"\0", 1)[0].decode("latin-1")

    def cigar(self, i):
        ops = self._slice("cigar", "cigar_off", i)
        return "".join("%d%s" % (int(v) >> 4, CIGAR_OPS[int(v) & 15]) for v in ops) or "*"

    def seq(self, i):
        return bytes(self._slice("seq", "seq_off", i)).decode("ascii") or "*"

    def qual(self, i):
        q = self._slice("qual", "seq_off", i)
        if q.size == 0 or q[0] == 0xFF:
            return "*"
        return bytes((q + 33).astype(np.uint8)).decode("ascii")

    def tags(self, i):
        return tags_text(self._slice("aux", "aux_off", i))

    def sam_line(self, i):
        c = self.cols
        ref, nref = int(c["ref_id"][i]), int(c["next_ref_id"][i])
        rname = self.ref_names[ref] if 0 <= ref < len(self.ref_names) else "*"
        if nref < 0:
            rnext = "*"
        elif nref == ref:
            rnext = "="
        else:
            rnext = self.ref_names[nref] if nref < len(self.ref_names) else "*"
        fields = [self.name(i), str(int(c["flag"][i])), rname, str(int(c["pos"][i]) + 1),
                  str(int(c["mapq"][i])), self.cigar(i), rnext, str(int(c["next_pos"][i]) + 1),
                  str(int(c["tlen"][i])), self.seq(i), self.qual(i)]
        return "\t".join(fields + self.tags(i))

    def sam_lines(self):
        return [self.sam_line(i) for i in range(self.n)]
