"""Per-base depth: the host-side pieces around sbh_depth (include/sparkbam.h, csrc/depth_core.h).

The runs of equal depth come from the device (device.Depth) or from the library's host functions
(depth_host below: no GPU); the two text forms are rendered here, on the host, from the runs."""
import ctypes as C
import re

import numpy as np

# sbh_depth_span, sbh_depth_run (include/sparkbam.h)
DEPTH_SPAN_DTYPE = np.dtype([("ref_id", "<i4"), ("pad", "<i4"), ("beg", "<i8"), ("end", "<i8")])
DEPTH_RUN_DTYPE = np.dtype([("ref_id", "<i4"), ("depth", "<u4"), ("beg", "<i8"), ("end", "<i8")])
DEPTH_DEL = 1  # SBH_DEPTH_DEL
DEFAULT_FLAG_EXCLUDE = 0x704  # UNMAP, SECONDARY, QCFAIL, DUP: samtools depth's default

_REGION = re.compile(r"^(.+):(\d+)-(\d+)$")


def span_array(spans):
    """[(ref_id, beg, end), ...] (0-based half-open) as the sbh_depth_span array."""
    a = np.zeros(len(spans), dtype=DEPTH_SPAN_DTYPE)
    for k, (r, b, e) in enumerate(spans):
        a[k] = (int(r), 0, int(b), int(e))
    return a


def region_spans(region, names, lengths):
    """The spans of a `region`: None -- every reference whole; "NAME" -- that reference whole;
    "NAME:BEG-END" -- its positions BEG..END, 1-based and inclusive as samtools writes regions
    (the span is [BEG - 1, END), cut to the reference's length).  A name that itself holds a
    colon is tried whole first.  ValueError for an unknown name or an empty range."""
    names = [n if isinstance(n, str) else bytes(n).decode("latin-1") for n in names]
    if region is None:
        return [(k, 0, int(n)) for k, n in enumerate(lengths) if int(n) > 0]
    if region in names:
        k = names.index(region)
        beg, end = 0, int(lengths[k])
    else:
        m = _REGION.match(region)
        if not m or m.group(1) not in names:
            raise ValueError("depth: unknown reference in region %r" % (region,))
        k = names.index(m.group(1))
        beg, end = int(m.group(2)) - 1, min(int(m.group(3)), int(lengths[k]))
    if beg < 0 or beg >= end:
        raise ValueError("depth: empty region %r" % (region,))
    return [(k, beg, end)]


def depth_text(runs, names, all_positions=False):
    """`RNAME\\tPOS\\tDEPTH\\n` per position, POS 1-based: samtools depth's lines (with
    all_positions, `samtools depth -a`'s: the zero-depth positions of the spans too)."""
    names = [n if isinstance(n, str) else bytes(n).decode("latin-1") for n in names]
    out = []
    for r in runs:
        d = int(r["depth"])
        if not d and not all_positions:
            continue
        head, tail = names[int(r["ref_id"])] + "\t", "\t%d\n" % d
        out.append("".join([head + str(p) + tail for p in range(int(r["beg"]) + 1, int(r["end"]) + 1)]))
    return "".join(out).encode("latin-1")


def depth_bedgraph(runs, names):
    """`RNAME\\tBEG\\tEND\\tDEPTH\\n` per run of depth > 0, 0-based half-open: bedtools genomecov
    -bg's lines."""
    names = [n if isinstance(n, str) else bytes(n).decode("latin-1") for n in names]
    return "".join("%s\t%d\t%d\t%d\n" % (names[int(r["ref_id"])], int(r["beg"]), int(r["end"]), int(r["depth"]))
                   for r in runs if int(r["depth"])).encode("latin-1")


def depth_host(flat, starts, spans, n_ref, filter=None, count_del=False, slots=None, finish=True):
    """Depth of the records at `starts` of a flat BAM stream over `spans`, computed on the host by
    the library (sbh_depth_add_host, sbh_depth_finish_host: no GPU, the definition the device path
    shares).  Returns (add result dict, slots) when finish is False -- `slots` (int32, zeros when
    None is given) can take further adds -- else (add result dict, depth uint32 over all slots, runs,
    sizes dict).  Raises SparkBamError(SBH_E_BAD_RECORD) with `.fields = (row,)` for the first bad
    record; the slots are then untouched."""
    from ._lib import SBH_OK, SbhDepthAddResult, SparkBamError, lib
    from .records import record_filter
    flat = np.ascontiguousarray(np.frombuffer(flat, dtype=np.uint8) if not isinstance(flat, np.ndarray) else flat)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    sp = span_array(spans)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    total = lib().sbh_depth_slots(p(sp), sp.size)
    if slots is None:
        slots = np.zeros(max(int(total), 1), dtype=np.int32)
    f, keep = record_filter(filter)
    res, bad = SbhDepthAddResult(), C.c_uint64()
    rc = lib().sbh_depth_add_host(p(flat), flat.size, p(st), st.size, C.byref(f) if f is not None else None, p(sp),
                                  sp.size, int(n_ref), DEPTH_DEL if count_del else 0, p(slots), C.byref(res),
                                  C.byref(bad))
    del keep
    if rc != SBH_OK:
        raise SparkBamError(rc, "record %d is malformed" % bad.value if rc == 20 else "depth_host", (bad.value,))
    add = {k: int(getattr(res, k)) for k, _ in SbhDepthAddResult._fields_}
    if not finish:
        return add, slots
    return (add,) + finish_host(slots, spans)


def finish_host(slots, spans):
    """sbh_depth_finish_host on slots[] (int32, turned into depth in place): (depth uint32, runs,
    sizes dict).  A first pass over a copy counts the runs, the second writes them."""
    from ._lib import SBH_OK, SbhDepthSizes, SparkBamError, lib
    sp = span_array(spans)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    sz = SbhDepthSizes()
    probe = slots.copy()
    rc = lib().sbh_depth_finish_host(p(probe), p(sp), sp.size, None, 0, C.byref(sz))
    runs = np.zeros(int(sz.n_runs), dtype=DEPTH_RUN_DTYPE)
    if rc == SBH_OK:
        rc = lib().sbh_depth_finish_host(p(slots), p(sp), sp.size, p(runs), runs.size, C.byref(sz))
    if rc != SBH_OK:
        raise SparkBamError(rc, "depth finish_host")
    return slots.view(np.uint32), runs, {k: int(getattr(sz, k)) for k, _ in SbhDepthSizes._fields_ if k != "pad"}


class DepthResult:
    """What api.depth returns: `.runs` (DEPTH_RUN_DTYPE: ref_id, depth, beg, end; every span cut
    into its maximal stretches of equal depth, zero-depth ones included), `.stats` (slots, n_runs,
    covered, sum, max_depth, and the adds' n, n_kept, n_counted, n_unplaced, cov_bases), `.spans`,
    `.names`, and the per-base depth of one reference's span (`.depth(name)`, uint32)."""

    def __init__(self, runs, stats, spans, names, depths):
        self.runs, self.stats, self.spans = runs, stats, list(spans)
        self.names = [n if isinstance(n, str) else bytes(n).decode("latin-1") for n in names]
        self._depths = depths  # callable: span index -> uint32 array

    def depth(self, name):
        """The depth of every position of `name`'s span, in order (position spans[k][1] first)."""
        ref = self.names.index(name)
        for k, s in enumerate(self.spans):
            if s[0] == ref:
                return self._depths(k)
        raise KeyError("depth: no span on reference %r" % (name,))

    def text(self, all_positions=False):
        return depth_text(self.runs, self.names, all_positions)

    def bedgraph(self):
        return depth_bedgraph(self.runs, self.names)
