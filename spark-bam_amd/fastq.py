"""FASTQ / FASTA text of BAM records: the host-side pieces around sbh_records_fastq_scan
(include/sparkbam.h, csrc/fastq_core.h) -- the mode word from keyword arguments, the library's host
renderer (fastq_host below: no GPU), and what api.fastq returns."""
import ctypes as C

import numpy as np

from ._lib import FASTQ_FASTA, FASTQ_SPLIT, FASTQ_SUFFIX, FASTQ_SUFFIX_ALWAYS

PART_CLASSES = (1, 2, 0)  # the class whose lines part k of a split text holds
_SUFFIX = {"auto": FASTQ_SUFFIX, "never": 0, "always": FASTQ_SUFFIX_ALWAYS}


def fastq_mode(fasta=False, suffix="auto", split=False):
    """The SBH_FASTQ_* mode word: fasta (no `+` and quality lines), suffix "auto" (/1 and /2 on
    paired reads: samtools' default), "never" (-n) or "always" (-N), split (the text in three
    parts: read 1, read 2, the others)."""
    if suffix not in _SUFFIX:
        raise ValueError("fastq: suffix is 'auto', 'never' or 'always', not %r" % (suffix,))
    return (FASTQ_FASTA if fasta else 0) | _SUFFIX[suffix] | (FASTQ_SPLIT if split else 0)


def sizes_dict(sz):
    """sbh_fastq_sizes as a dict: n, n_kept, text_bytes, part_bytes [3], part_rows [3]."""
    return {"n": int(sz.n), "n_kept": int(sz.n_kept), "text_bytes": int(sz.text_bytes),
            "part_bytes": [int(x) for x in sz.part_bytes], "part_rows": [int(x) for x in sz.part_rows]}


def fastq_host(flat, starts, filter=None, fasta=False, suffix="auto", split=False, def_qual=1, want_text=True, mode=None):
    """The text Shard.records_fastq renders on the GPU, rendered on the host by the library
    (sbh_fastq_render_host: no GPU, the definition the device path shares) for the records at
    starts[] of a flat BAM stream.  Returns (text uint8 or None, rec_off uint64 [n_kept + 1], rows
    uint64 [n_kept], sizes dict).  Raises SparkBamError(SBH_E_BAD_RECORD) with `.fields = (row,)`
    for the first invalid record, kept or not."""
    from ._lib import SBH_OK, SbhFastqSizes, SparkBamError, lib
    from .records import record_filter
    flat = np.ascontiguousarray(np.frombuffer(flat, dtype=np.uint8) if not isinstance(flat, np.ndarray) else flat)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    mode = fastq_mode(fasta, suffix, split) if mode is None else int(mode)
    f, keep = record_filter(filter)
    fp = C.byref(f) if f is not None else None
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    sz, bad = SbhFastqSizes(), C.c_uint64()
    rec_off, rows = np.zeros(st.size + 1, np.uint64), np.zeros(max(st.size, 1), np.uint64)

    def call(text):
        rc = lib().sbh_fastq_render_host(p(flat), flat.size, p(st), st.size, fp, mode, int(def_qual),
                                         p(text) if text is not None else None, text.size if text is not None else 0,
                                         p(rec_off), p(rows), C.byref(sz), C.byref(bad))
        if rc != SBH_OK:
            raise SparkBamError(rc, "record %d is malformed" % bad.value if rc == 20 else "fastq_host",
                                (bad.value,) if rc == 20 else ())

    call(None)
    text = None
    if want_text:
        text = np.empty(sz.text_bytes, np.uint8)
        call(text)
    del keep
    return text, rec_off[:sz.n_kept + 1], rows[:sz.n_kept], sizes_dict(sz)


class FastqResult:
    """What api.fastq returns: `.n` and `.n_kept` (records seen, records written), `.part_bytes` and
    `.part_rows` (text bytes and records of read 1, read 2 and the others when the output was split;
    everything in entry 0 otherwise) and `.text` (the interleaved text as bytes when no sink was
    given, else None)."""

    def __init__(self, n, n_kept, part_bytes, part_rows, text):
        self.n, self.n_kept, self.part_bytes, self.part_rows, self.text = int(n), int(n_kept), list(part_bytes), list(part_rows), text
