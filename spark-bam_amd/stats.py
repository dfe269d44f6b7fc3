"""Read-level statistics: the host-side pieces around sbh_stats (include/sparkbam.h,
csrc/stats_core.h).

The tables come from the device (device.Stats) or from the library's host function (stats_host
below: no GPU); the report -- tab-separated lines under samtools stats' section tags -- is rendered
here, on the host, from the tables, byte for byte as csrc/stats_core.h's stats_text renders it."""
import ctypes as C
import math

import numpy as np

STATS_QUALS = 94  # SBH_STATS_QUALS
# sn[k] is (index into SN_ROWS)
SN_ROWS = ("sequences", "first_fragments", "last_fragments", "mapped", "unmapped", "paired", "properly_paired",
           "duplicates", "mq0", "qc_failed", "secondary", "supplementary", "total_length", "total_first_length",
           "total_last_length", "bases_mapped", "sum_quality", "no_qualities", "max_length", "pairs_inward",
           "pairs_outward", "pairs_other", "pairs_different_chr")
STATS_SN = len(SN_ROWS)  # SBH_STATS_SN
_LABELS = ("sequences", "first fragments", "last fragments", "reads mapped", "reads unmapped", "reads paired",
           "reads properly paired", "reads duplicated", "reads MQ0", "reads QC failed", "secondary alignments",
           "supplementary alignments", "total length", "total first fragment length", "total last fragment length",
           "bases mapped", "quality sum", "reads without qualities", "maximum length", "inward oriented pairs",
           "outward oriented pairs", "pairs with other orientation", "pairs on different chromosomes")
# the tables in sbh_stats_fetch's order
TABLES = ("sn", "read_len", "qual", "base", "gc", "isize", "mapq")
_MASK = 2 ** 64 - 1


def check_params(cycles, max_insert):
    """(cycles, max_insert) as ints that fit the C struct; the library judges their range."""
    from ._lib import SBH_E_ARG, SparkBamError
    c, i = int(cycles), int(max_insert)
    if not (0 <= c < 2 ** 32 and 0 <= i < 2 ** 32):
        raise SparkBamError(SBH_E_ARG, "stats: cycles %d or max_insert %d out of range" % (c, i))
    return c, i


def table_shapes(cycles, max_insert):
    c, i = int(cycles), int(max_insert)
    return {"sn": (STATS_SN,), "read_len": (c + 2,), "qual": (2, c + 1, STATS_QUALS), "base": (c + 1, 5), "gc": (2, 101),
            "isize": (i + 1, 3), "mapq": (256,)}


def empty_tables(cycles, max_insert):
    return {k: np.zeros(s, np.uint64) for k, s in table_shapes(cycles, max_insert).items()}


def stats_text(tables, cycles, max_insert):
    """The report (bytes) from the tables (a dict as empty_tables': sn, read_len, qual, base, gc, isize,
    mapq): `SN\\tlabel:\\tvalue` for the counters in SN_ROWS' order and the derived average length,
    average quality, insert size average and standard deviation (over the bins below max_insert);
    `FFQ` / `LFQ` cycle (1-based) and a count per quality up to the largest in use; `GCF` / `GCL` the
    non-empty GC bins; `GCC` cycle and the A C G T N counts; `IS` size, total, inward, outward, other up
    to the last non-empty bin; `RL` and `MAPQ` the non-empty bins."""
    c, i = int(cycles), int(max_insert)
    t = {k: np.asarray(tables[k], np.uint64).reshape(s) for k, s in table_shapes(c, i).items()}
    sn = [int(x) for x in t["sn"]]
    out = ["SN\t%s:\t%d\n" % (_LABELS[k], sn[k]) for k in range(STATS_SN)]
    qual, base = t["qual"], t["base"]
    rows_used = np.flatnonzero(qual.any(axis=(0, 2)) | base.any(axis=1))
    n_rows = int(rows_used[-1]) + 1 if rows_used.size else 0
    quals_used = np.flatnonzero(qual.any(axis=(0, 1)))
    n_quals = int(quals_used[-1]) + 1 if quals_used.size else 0
    per_q = [int(x) for x in qual.sum(axis=(0, 1), dtype=np.uint64)]
    qn = sum(q * v for q, v in enumerate(per_q)) & _MASK
    qd = sum(per_q) & _MASK
    tot = [int(a) + int(b) + int(d) & _MASK for a, b, d in t["isize"].tolist()]
    sizes_used = [s for s, v in enumerate(tot) if v]
    n_sizes = sizes_used[-1] + 1 if sizes_used else 0
    n = sum(tot[s] for s in sizes_used if s < i) & _MASK
    s1 = sum(s * tot[s] for s in sizes_used if s < i) & _MASK
    s2 = sum(s * s * tot[s] for s in sizes_used if s < i) & _MASK
    avg = float(s1) / float(n) if n else 0.0
    var = float(s2) / float(n) - avg * avg if n else 0.0
    var = 0.0 if var < 0 else var
    out.append("SN\taverage length:\t%d\n" % (sn[12] // sn[0] if sn[0] else 0))
    out.append("SN\taverage quality:\t%.1f\n" % (float(qn) / float(qd) if qd else 0.0))
    out.append("SN\tinsert size average:\t%.1f\n" % avg)
    out.append("SN\tinsert size standard deviation:\t%.1f\n" % math.sqrt(var))
    for w, tag in ((0, "FFQ"), (1, "LFQ")):
        for row in range(n_rows):
            out.append("%s\t%d%s\n" % (tag, row + 1, "".join("\t%d" % int(v) for v in qual[w, row, :n_quals])))
    for w, tag in ((0, "GCF"), (1, "GCL")):
        out.extend("%s\t%d\t%d\n" % (tag, b, int(t["gc"][w, b])) for b in np.flatnonzero(t["gc"][w]).tolist())
    for row in range(n_rows):
        out.append("GCC\t%d\t%d\t%d\t%d\t%d\t%d\n" % ((row + 1,) + tuple(int(v) for v in base[row])))
    isz = t["isize"]
    out.extend("IS\t%d\t%d\t%d\t%d\t%d\n" % (s, tot[s], int(isz[s, 0]), int(isz[s, 1]), int(isz[s, 2])) for s in range(n_sizes))
    out.extend("RL\t%d\t%d\n" % (k, int(t["read_len"][k])) for k in np.flatnonzero(t["read_len"]).tolist())
    out.extend("MAPQ\t%d\t%d\n" % (q, int(t["mapq"][q])) for q in np.flatnonzero(t["mapq"]).tolist())
    return "".join(out).encode("latin-1")


def stats_host(flat, starts, cycles=1024, max_insert=8000, filter=None, tables=None):
    """The tables of the records at `starts` of a flat BAM stream, computed on the host by the library
    (sbh_stats_add_host: no GPU, the definition the device path is held to).  Returns (tables, n_kept,
    n_counted); `tables` given (empty_tables' dict): added into it.  A bad row raises
    SparkBamError(SBH_E_BAD_RECORD) with the row in .fields and leaves the tables untouched."""
    from ._lib import SBH_OK, SbhStatsAddResult, SbhStatsParams, SparkBamError, lib
    from .records import record_filter
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    c, i = check_params(cycles, max_insert)
    f, keep = record_filter(filter)
    res, bad, prm = SbhStatsAddResult(), C.c_uint64(), SbhStatsParams(c, i)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    if tables is None:
        # (parameters out of range: the library refuses them before it touches a table)
        ok = 1 <= c <= 65536 and 1 <= i <= 1 << 20
        tables = empty_tables(c if ok else 1, i if ok else 1)
    else:
        shapes = table_shapes(c, i)
        if any(tables[k].shape != shapes[k] or tables[k].dtype != np.uint64 or not tables[k].flags.c_contiguous for k in TABLES):
            raise ValueError("stats_host: the tables are empty_tables(cycles, max_insert)'s")
    rc = lib().sbh_stats_add_host(p(flat), flat.size, p(st), st.size, C.byref(f) if f is not None else None, C.byref(prm),
                                  *[p(tables[k]) for k in TABLES], C.byref(res), C.byref(bad))
    del keep
    if rc != SBH_OK:
        raise SparkBamError(rc, "record %d is malformed" % bad.value if rc == 20 else "stats_host", (bad.value,) if rc == 20 else ())
    return tables, int(res.n_kept), int(res.n_counted)


class StatsResult:
    """What api.stats returns: the tables `.sn` (uint64[23], SN_ROWS), `.read_len`, `.qual`, `.base`,
    `.gc`, `.isize`, `.mapq` (empty_tables' shapes), `.cycles`, `.max_insert`, `.n`, `.n_kept` and
    `.n_counted` (records seen, records the filter kept, those of them that are neither secondary nor
    supplementary), and `.text()`."""

    def __init__(self, tables, cycles, max_insert, n, n_kept, n_counted):
        self.tables = {k: tables[k] for k in TABLES}
        for k in TABLES:
            setattr(self, k, tables[k])
        self.cycles, self.max_insert = int(cycles), int(max_insert)
        self.n, self.n_kept, self.n_counted = int(n), int(n_kept), int(n_counted)

    def text(self):
        return stats_text(self.tables, self.cycles, self.max_insert)
