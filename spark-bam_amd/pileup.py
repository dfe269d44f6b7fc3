"""Per-base allele counts: the host-side pieces around sbh_pileup (include/sparkbam.h,
csrc/pileup_core.h).

The counts, call bytes and intervals come from the device (device.Pileup) or from the library's
host functions (pileup_host below: no GPU); the count table and the consensus FASTA are rendered
here, on the host."""
import ctypes as C

import numpy as np

from .coverage import DEPTH_SPAN_DTYPE, span_array

CHANNELS = ("A", "C", "G", "T", "N", "DEL", "INS", "LOWQ")  # SBH_PILE_*
BYTES_PER_POSITION = 33  # eight u32 channels and the call byte
TEXT_HEADER = b"#chrom\tpos\tA\tC\tG\tT\tN\tdel\tins\tlowq\n"


def _names(names):
    return [n if isinstance(n, str) else bytes(n).decode("latin-1") for n in names]


def span_passes(spans, max_positions):
    """The spans grouped greedily, in order, into passes of at most max_positions positions each.
    ValueError names a span that alone is larger than the budget."""
    passes, cur, used = [], [], 0
    for r, b, e in spans:
        n = int(e) - int(b)
        if n > max_positions:
            raise ValueError("pileup: span (ref %d, %d, %d) has %d positions, more than max_positions = %d: "
                             "give a smaller region" % (r, b, e, n, max_positions))
        if cur and used + n > max_positions:
            passes.append(cur)
            cur, used = [], 0
        cur.append((int(r), int(b), int(e)))
        used += n
    if cur:
        passes.append(cur)
    return passes


def pileup_text(intervals, spans, counts, names, all_positions=False, header=False):
    """`NAME\\tPOS\\tA\\tC\\tG\\tT\\tN\\tDEL\\tINS\\tLOWQ\\n` per position of the intervals (with
    all_positions: per position of the spans), POS 1-based.  counts: callable, span index -> uint32
    [len, 8].  header: a first line naming the columns."""
    names = _names(names)
    out = [TEXT_HEADER] if header else []
    for k, (ref, b, e) in enumerate(spans):
        if all_positions:
            cut = [(b, e)]
        else:
            iv = intervals[intervals["ref_id"] == ref]
            cut = [(int(x), int(y)) for x, y in zip(iv["beg"], iv["end"])]
        if not cut:
            continue
        c = counts(k)
        head = names[ref] + "\t"
        for x, y in cut:
            rows = c[x - b:y - b].tolist()
            out.append("".join([head + str(p + 1) + "\t" + "\t".join(map(str, row)) + "\n"
                                for p, row in zip(range(x, y), rows)]).encode("latin-1"))
    return b"".join(out)


def consensus_fasta(spans, calls, names, lengths=None):
    """FASTA of the call bytes: `>NAME` for a span that is its whole reference (lengths known),
    `>NAME:BEG-END` (1-based, inclusive) otherwise; call byte 0 prints as N, `*` is dropped, 60
    letters a line.  calls: callable, span index -> uint8 [len]."""
    names = _names(names)
    out = []
    for k, (ref, b, e) in enumerate(spans):
        whole = lengths is not None and b == 0 and e == int(lengths[ref])
        out.append((">%s\n" % names[ref] if whole else ">%s:%d-%d\n" % (names[ref], b + 1, e)).encode("latin-1"))
        c = np.array(calls(k), dtype=np.uint8)
        c[c == 0] = ord("N")
        s = c[c != ord("*")].tobytes()
        out.append(b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)))
    return b"".join(out)


def pileup_host(flat, starts, spans, n_ref, filter=None, min_baseq=0, counts=None, finish=True, min_depth=1,
                call_pct=75):
    """Allele counts of the records at `starts` of a flat BAM stream over `spans`, computed on the
    host by the library (sbh_pileup_add_host, sbh_pileup_finish_host: no GPU, the definition the
    device path shares).  Returns (add result dict, counts uint32 [positions, 8]) when finish is
    False -- `counts` (zeros when None is given) can take further adds -- else (add result dict,
    counts, calls uint8, intervals, sizes dict).  Raises SparkBamError(SBH_E_BAD_RECORD) with
    `.fields = (row,)` for the first bad record; the counts are then untouched."""
    from ._lib import SBH_OK, SbhPileupAddResult, SparkBamError, lib
    from .records import record_filter
    flat = np.ascontiguousarray(np.frombuffer(flat, dtype=np.uint8) if not isinstance(flat, np.ndarray) else flat)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    sp = span_array(spans)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    if counts is None:
        counts = np.zeros((sum(int(e) - int(b) for _, b, e in spans), 8), dtype=np.uint32)
    f, keep = record_filter(filter)
    res, bad = SbhPileupAddResult(), C.c_uint64()
    rc = lib().sbh_pileup_add_host(p(flat), flat.size, p(st), st.size, C.byref(f) if f is not None else None, p(sp),
                                   sp.size, int(n_ref), int(min_baseq), counts.ctypes.data_as(C.c_void_p), C.byref(res),
                                   C.byref(bad))
    del keep
    if rc != SBH_OK:
        raise SparkBamError(rc, "record %d is malformed" % bad.value if rc == 20 else "pileup_host", (bad.value,))
    add = add_dict(res)
    if not finish:
        return add, counts
    return (add, counts) + finish_host(counts, spans, min_depth, call_pct)


def add_dict(res):
    d = {k: int(getattr(res, k)) for k in ("n", "n_kept", "n_counted", "n_unplaced")}
    d["totals"] = [int(v) for v in res.totals]
    return d


def sizes_dict(sz):
    d = {k: int(getattr(sz, k)) for k in ("positions", "n_intervals", "nonzero", "n_called", "covered", "max_depth")}
    d["totals"] = [int(v) for v in sz.totals]
    return d


def finish_host(counts, spans, min_depth=1, call_pct=75):
    """sbh_pileup_finish_host on counts[positions, 8]: (calls uint8, intervals, sizes dict).  A
    first pass counts the intervals, the second writes them."""
    from ._lib import SBH_OK, SbhPileupSizes, SparkBamError, lib
    sp = span_array(spans)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    calls = np.zeros(counts.shape[0], dtype=np.uint8)
    sz = SbhPileupSizes()
    cp, kp = counts.ctypes.data_as(C.c_void_p), calls.ctypes.data_as(C.c_void_p)
    rc = lib().sbh_pileup_finish_host(cp, p(sp), sp.size, int(min_depth), int(call_pct), kp, None, 0, C.byref(sz))
    iv = np.zeros(int(sz.n_intervals), dtype=DEPTH_SPAN_DTYPE)
    if rc == SBH_OK:
        rc = lib().sbh_pileup_finish_host(cp, p(sp), sp.size, int(min_depth), int(call_pct), kp, p(iv), iv.size,
                                          C.byref(sz))
    if rc != SBH_OK:
        raise SparkBamError(rc, "pileup finish_host")
    return calls, iv, sizes_dict(sz)


class PileupResult:
    """What api.pileup returns: `.intervals` (DEPTH_SPAN_DTYPE: ref_id, beg, end; the maximal
    stretches of positions where any channel is non-zero), `.stats` (positions, n_intervals, nonzero,
    n_called, covered, max_depth, totals[8] and the adds' n, n_kept, n_counted, n_unplaced),
    `.spans`, `.names`, and per reference `.counts(name)` (uint32 [len, 8], channels CHANNELS) and
    `.calls(name)` (uint8)."""

    def __init__(self, intervals, stats, spans, names, counts, calls, lengths=None):
        self.intervals, self.stats, self.spans = intervals, stats, list(spans)
        self.names = _names(names)
        self.lengths = lengths
        self._counts, self._calls = list(counts), list(calls)

    def _span(self, name):
        ref = self.names.index(name)
        for k, s in enumerate(self.spans):
            if s[0] == ref:
                return k
        raise KeyError("pileup: no span on reference %r" % (name,))

    def counts(self, name):
        """uint32 [len, 8]: the channels of every position of `name`'s span, in order."""
        return self._counts[self._span(name)]

    def calls(self, name):
        """uint8 [len]: the call byte of every position of `name`'s span (0, A C G T * or N)."""
        return self._calls[self._span(name)]

    def text(self, all_positions=False, header=False):
        return pileup_text(self.intervals, self.spans, lambda k: self._counts[k], self.names, all_positions, header)

    def consensus(self):
        return consensus_fasta(self.spans, lambda k: self._calls[k], self.names, self.lengths)
