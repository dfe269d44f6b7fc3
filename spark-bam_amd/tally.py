"""Flag counts and per-reference read counts: the host-side pieces around sbh_tally
(include/sparkbam.h, csrc/tally_core.h).

The counts come from the device (device.Tally) or from the library's host function (tally_host
below: no GPU); the two text forms -- samtools flagstat's and samtools idxstats' -- are rendered
here, on the host, from the counts."""
import ctypes as C

import numpy as np

TALLY_ROWS = 16  # SBH_TALLY_ROWS
# flag[k] counts the kept rows of (index into FLAG_ROWS)
FLAG_ROWS = ("total", "primary", "secondary", "supplementary", "duplicates", "primary_duplicates", "mapped",
             "primary_mapped", "paired", "read1", "read2", "properly_paired", "both_mapped", "singletons",
             "mate_on_different_chr", "mate_on_different_chr_mapq5")
_LABELS = ("in total (QC-passed reads + QC-failed reads)", "primary", "secondary", "supplementary", "duplicates",
           "primary duplicates", "mapped", "primary mapped", "paired in sequencing", "read1", "read2",
           "properly paired", "with itself and mate mapped", "singletons", "with mate mapped to a different chr",
           "with mate mapped to a different chr (mapQ>=5)")
# the row a line's percentages are taken of: total for mapped, primary for primary mapped, paired
# for properly paired and singletons
_PERCENT_OF = {6: 0, 7: 1, 11: 8, 13: 8}


def _percent(n, d):
    return "%.2f%%" % (100.0 * n / d) if d else "N/A"


def flagstat_text(flag):
    """samtools flagstat's sixteen lines (bytes) from flag uint64[16, 2]: `pass + fail label`, the
    mapped, primary mapped, properly paired and singletons lines with ` (P : P)`, P a percentage
    with two decimals or N/A."""
    flag = np.asarray(flag, dtype=np.uint64).reshape(TALLY_ROWS, 2)
    out = []
    for k in range(TALLY_ROWS):
        a, b = int(flag[k, 0]), int(flag[k, 1])
        line = "%d + %d %s" % (a, b, _LABELS[k])
        if k in _PERCENT_OF:
            d = _PERCENT_OF[k]
            line += " (%s : %s)" % (_percent(a, int(flag[d, 0])), _percent(b, int(flag[d, 1])))
        out.append(line + "\n")
    return "".join(out).encode("latin-1")


def idxstats_text(ref, names, lengths):
    """samtools idxstats' lines (bytes) from ref uint64[n_ref + 1, 2]: `name\\tlength\\tmapped\\t
    unmapped\\n` per reference in header order, then `*\\t0\\tM\\tU\\n` from the last bin."""
    ref = np.asarray(ref, dtype=np.uint64).reshape(-1, 2)
    if ref.shape[0] != len(names) + 1 or len(lengths) != len(names):
        raise ValueError("idxstats_text: %d bins for %d names and %d lengths" % (ref.shape[0], len(names), len(lengths)))
    out = ["%s\t%d\t%d\t%d\n" % (names[k], int(lengths[k]), int(ref[k, 0]), int(ref[k, 1])) for k in range(len(names))]
    out.append("*\t0\t%d\t%d\n" % (int(ref[-1, 0]), int(ref[-1, 1])))
    return "".join(out).encode("latin-1")


def tally_host(flat, starts, n_ref, filter=None, flag=None, ref=None):
    """Counts of the records at `starts` of a flat BAM stream, computed on the host by the library
    (sbh_tally_add_host: no GPU, the definition the device path is held to).  Returns (flag
    uint64[16, 2], ref uint64[n_ref + 1, 2], n_kept); `flag` and `ref` given: added into them.  A bad
    row raises SparkBamError(SBH_E_BAD_RECORD) with the row in .fields and leaves both untouched."""
    from ._lib import SBH_OK, SbhTallyAddResult, SparkBamError, lib
    from .records import record_filter
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    flag = np.zeros((TALLY_ROWS, 2), np.uint64) if flag is None else flag
    ref = np.zeros((max(int(n_ref), 0) + 1, 2), np.uint64) if ref is None else ref
    if flag.shape != (TALLY_ROWS, 2) or ref.shape != (int(n_ref) + 1, 2) or flag.dtype != np.uint64 or ref.dtype != np.uint64:
        raise ValueError("tally_host: flag is uint64[16, 2], ref uint64[n_ref + 1, 2]")
    f, keep = record_filter(filter)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    res, bad = SbhTallyAddResult(), C.c_uint64()
    rc = lib().sbh_tally_add_host(p(flat), flat.size, p(st), st.size, C.byref(f) if f is not None else None, int(n_ref),
                                  p(flag), p(ref), C.byref(res), C.byref(bad))
    del keep
    if rc != SBH_OK:
        raise SparkBamError(rc, "record %d is malformed or off the references" % bad.value if rc == 20 else "tally_host",
                            (bad.value,) if rc == 20 else ())
    return flag, ref, int(res.n_kept)


class TallyResult:
    """What api.flagstat and api.idxstats return: `.flag` (uint64[16, 2]: FLAG_ROWS by QC-pass,
    QC-fail), `.ref` (uint64[n_ref + 1, 2]: mapped, unmapped per reference, the last bin the reads
    without one), `.names`, `.lengths`, `.n` and `.n_kept` (records seen, records the filter kept)."""

    def __init__(self, flag, ref, names, lengths, n, n_kept):
        self.flag, self.ref, self.names, self.lengths = flag, ref, list(names), [int(x) for x in lengths]
        self.n, self.n_kept = int(n), int(n_kept)

    def flagstat_text(self):
        return flagstat_text(self.flag)

    def idxstats_text(self):
        return idxstats_text(self.ref, self.names, self.lengths)
