"""The host side of the FASTQ / FASTA text (csrc/fastq_core.h through the library, no GPU):
sbh_fastq_render_host against the independent restatement of fastq_corpus.py on every corpus and
variant, sizes-only calls, malformed rows, the argument errors, 2.bam's text against the reference's
own SAM fixture, and the bundled files' totals as literals."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from pkg import sb
import fastq_corpus as fc
import record_corpus as rc
import sam_corpus as sc
from test_tally_cpu import bundled

SBH_OK, SBH_E_ARG, SBH_E_BAD_RECORD = 0, sb._lib.SBH_E_ARG, sb._lib.SBH_E_BAD_RECORD

# (records, text bytes) under -F 0x900, FASTQ with suffixes; then FASTA; from the restatement
BUNDLED_TOTALS = {
    "2.bam": ((2500, 628697), (2500, 368697)),
    "5k.bam": ((4910, 1234794), (4910, 724154)),
    "1.bam": ((4917, 954177), (4917, 565734)),
}


def host(c, **kw):
    return sb.fastq_host(np.frombuffer(bytes(c.flat), np.uint8), c.starts, **kw)


def same(got, want):
    text, rec_off, rows, sizes = got
    assert sizes == want["sizes"]
    assert rec_off.dtype == np.uint64 and rec_off.tolist() == want["rec_off"]
    assert rows.dtype == np.uint64 and rows.tolist() == want["rows"]
    if text is not None:
        assert text.dtype == np.uint8 and text.tobytes() == want["text"]


def test_restatement_on_hand_written_lines():
    codes = (1, 2, 4, 8, 15, 3, 0)  # A C G T N M =
    r = fc.one(b"q", 0x51, codes, bytes((0, 10, 93, 94, 255, 40, 2)))
    assert fc.line(r[:]) == b"@q/1\n=KNACGT\n+\n#I~~~+!\n"
    assert fc.line(r[:], fasta=True, suffix="never") == b">q\n=KNACGT\n"
    f = fc.one(b"q", 0x80, codes, b"\xff" * 7)
    assert fc.line(f[:]) == b"@q\nACGTNM=\n+\n\"\"\"\"\"\"\"\n"
    assert fc.line(f[:], suffix="always", def_qual=0) == b"@q/2\nACGTNM=\n+\n!!!!!!!\n"
    c = fc.case([r, f, fc.one(b"z", 0, ())])
    w = fc.restate(c.flat, c.starts, split=True, suffix="always")
    assert w["text"] == b"@q/1\n=KNACGT\n+\n#I~~~+!\n@q/2\nACGTNM=\n+\n\"\"\"\"\"\"\"\n@z\n\n+\n\n"
    assert w["rec_off"] == [0, 23, 46, 53] and w["rows"] == [0, 1, 2]
    assert w["sizes"] == {"n": 3, "n_kept": 3, "text_bytes": 53, "part_bytes": [23, 23, 7], "part_rows": [1, 1, 1]}
    w = fc.restate(c.flat, c.starts, split=True)  # 0x80 without 0x1: class 0
    assert w["rows"] == [0, 1, 2] and w["sizes"]["part_rows"] == [1, 0, 2]


def test_constants_are_the_library_s():
    with open(os.path.join(ROOT, "include", "sparkbam.h")) as f:
        src = f.read()
    for name, v in (("FASTA", 1), ("SUFFIX", 2), ("SUFFIX_ALWAYS", 4), ("SPLIT", 8)):
        assert "#define SBH_FASTQ_%s %du\n" % (name, v) in src and getattr(sb._lib, "FASTQ_" + name) == v
    with open(os.path.join(ROOT, "spark-bam_amd", "csrc", "fastq_core.h")) as f:
        core = f.read()
    assert re.search(r"MODE_FASTA = 1u, MODE_SUFFIX = 2u, MODE_SUFFIX_ALWAYS = 4u, MODE_SPLIT = 8u;", core)
    assert sb.fastq_mode() == 2 and sb.fastq_mode(True, "never", True) == 9 and sb.fastq_mode(suffix="always") == 4
    assert sys.modules[sb.fastq_mode.__module__].PART_CLASSES == fc.PART_CLASSES and callable(sb.fastq)
    with pytest.raises(ValueError):
        sb.fastq_mode(suffix="sometimes")


@pytest.mark.parametrize("kv", fc.ALL, ids=fc.ident)
def test_host_is_the_restatement(kv):
    name, v = kv
    c, want = fc.get(name), fc.expected(name, v)
    assert want["bad_row"] is None
    same(host(c, **fc.VARIANTS[name][v]), want)
    # sizes only: the same numbers, offsets and rows
    same(host(c, want_text=False, **fc.VARIANTS[name][v]), want)


def test_corpora_say_what_they_are_for():
    e = fc.expected
    lens = [int.from_bytes(fc.get("seq_lengths").flat[s + 20:s + 24], "little") for s in fc.get("seq_lengths").starts]
    assert lens == [n for n in fc.SEQ_LENGTHS for _ in (0, 1)]
    assert max(b - a for a, b in zip(fc.get("seq_lengths").starts, fc.get("seq_lengths").starts[1:])) > 1024
    t = e("all_codes", 0)["text"].split(b"\n")
    assert t[1] == b"=ACMGRSVTWYHKDBN" and t[5] == b"NVHMDRWABSYCKGT=" and t[9] == b"N=ACMGRSVTWYHKDBN" and t[13] == b"NVHMDRWABSYCKGT=N"
    q0, q93 = e("quals", 0)["text"], e("quals", 2)["text"]
    assert b"@all_ff\n" + bytes(b"=ACMGRSVTWYHKDBN"[(3 * k + 5) % 16] for k in range(10)) + b"\n+\n!!!!!!!!!!\n" in q0
    assert b"\n+\n~~~~~~~~~~\n" in q93 and b"\n+\n!}~~~~~\"]\n" in q0 and b"\n+\n]\"~~~~~}!\n" in q0
    assert b"@later_ff\n" in q0 and b"\n+\n!I~-~~\"\n" in q0 and q0.count(b"\n") == 4 * 14
    n = e("names", 0)["text"]
    assert n.startswith(b"@x\n") and b"@ab/1\n" in n and b"@\nRT\n" in n and b"@\nACGTN\n" in n and b"@/1\nNACGT\n" in n
    assert b"@" + rc._name(254) + b"\n" in n and b"@slash/1/1\n" in n
    heads = lambda v: e("flags", v)["text"].split(b"\n")[0:-1:4]  # noqa: E731 (the @ lines, "@fXXX" and the suffix)
    assert [ln[5:] for ln in heads(0)] == [b"/1", b"/1", b"/2", b"/2"] + [b""] * 8
    assert [ln[5:] for ln in heads(4)] == [b"/1", b"/1", b"/2", b"/2", b"", b"", b"", b"", b"/1", b"/1", b"/2", b"/2"]
    assert all(len(ln) == 5 for ln in heads(2))
    assert e("flags", 1)["sizes"]["part_rows"] == [2, 2, 8] and e("flags", 5)["sizes"]["part_rows"] == [4, 4, 4]
    assert e("flags", 3)["sizes"]["part_rows"] == [2, 2, 8]  # suffix="never" still asks for 0x1
    assert e("split_no_class_2", 0)["sizes"]["part_rows"] == [35, 0, 35] and e("split_only_class_0", 0)["sizes"]["part_rows"] == [0, 0, 70]
    assert e("split_alternating", 0)["sizes"]["part_rows"] == [67, 67, 66]
    assert e("split_alternating", 0)["rows"][:3] == [0, 3, 6] and e("split_alternating", 0)["rows"][67:69] == [1, 4]
    assert e("filters", 0)["sizes"]["n_kept"] == 0 and e("filters", 0)["rec_off"] == [0] and e("filters", 5)["sizes"]["n_kept"] == 0
    assert e("filters", 1)["sizes"]["n_kept"] == 8 and sorted(e("filters", 1)["rows"]) == [a for a, _ in fc._ONE_PER_WAVE]
    assert e("rows_0", 0)["sizes"] == {"n": 0, "n_kept": 0, "text_bytes": 0, "part_bytes": [0, 0, 0], "part_rows": [0, 0, 0]}
    g = e("grid", 0)
    assert g["sizes"]["n_kept"] == rc.GRID_RECORDS == fc.GRID_PASS + 37 and g["text"][:26] == b"@0000000\n\n+\n\n@0000001\n\n+\n\n"


def test_text_cap_and_exact_buffers():
    c, want = fc.get("flags"), fc.expected("flags", 0)
    flat, st = np.frombuffer(bytes(c.flat), np.uint8), np.asarray(c.starts, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    sz, bad = sb._lib.SbhFastqSizes(), C.c_uint64()
    n = want["sizes"]["text_bytes"]
    text = np.full(n + 8, 0x5a, np.uint8)
    call = lambda cap, mode=2, dq=1, f=None: sb.lib().sbh_fastq_render_host(  # noqa: E731
        p(flat), flat.size, p(st), st.size, f, mode, dq, p(text), cap, None, None, C.byref(sz), C.byref(bad))
    assert call(n - 1) == SBH_E_ARG and sz.text_bytes == n and (text == 0x5a).all()
    assert call(n) == SBH_OK and text[:n].tobytes() == want["text"] and (text[n:] == 0x5a).all()
    assert call(n, mode=16) == SBH_E_ARG and call(n, mode=2 | 32) == SBH_E_ARG
    assert call(n, dq=94) == SBH_E_ARG and call(n, dq=-1) == SBH_E_ARG and call(n, dq=93) == SBH_OK
    f = sb._lib.SbhRecordFilter(0x10000, 0, 0, 0, None, None, 0)
    assert call(n, f=C.byref(f)) == SBH_E_ARG
    assert sb.lib().sbh_fastq_render_host(p(flat), flat.size, p(st), st.size, None, 2, 1, None, 0, None, None, None, None) == SBH_E_ARG
    for filt in ({"min_mapq": 256}, {"rows": [(5, 5)]}, {"rows": [(5, 9), (8, 12)]}):
        with pytest.raises(sb.SparkBamError) as e:
            host(c, filter=filt)
        assert e.value.code == SBH_E_ARG


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed_row(m):
    c = fc.Case(m.stream.flat, list(m.stream.starts))
    assert fc.restate(c.flat, c.starts)["bad_row"] == 3
    for kw in ({}, {"split": True, "fasta": True}, {"filter": {"flag_require": 0x1000 >> 1}}, {"want_text": False}):
        with pytest.raises(sb.SparkBamError) as e:
            host(c, **kw)  # the bad row is judged even when the filter would drop it
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (3,)
    for p in (len(c.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        with pytest.raises(sb.SparkBamError) as e:
            sb.fastq_host(np.frombuffer(bytes(c.flat), np.uint8), c.starts[:2] + [p])
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (2,)
    # the good rows alone render
    same(sb.fastq_host(np.frombuffer(bytes(c.flat), np.uint8), c.starts[:3]), fc.restate(c.flat, c.starts[:3]))


_RC = bytes.maketrans(b"ACGTN", b"TGCAN")


def test_2bam_against_the_reference_sam():
    """Every record of 2.bam kept under -F 0x900 against the reference's own 2.sam.gz: name and
    suffix from QNAME and FLAG, lines 2 and 4 from SEQ and QUAL, turned round when 0x10 is set."""
    _, flat, starts, _, _, _ = bundled("2.bam")
    text, rec_off, rows, sizes = sb.fastq_host(np.frombuffer(flat, np.uint8), starts, filter={"flag_exclude": 0x900})
    _, sam = sc.fixture_lines()
    assert len(sam) == len(starts) == sizes["n"]
    kept = [i for i, ln in enumerate(sam) if not int(ln.split(b"\t")[1]) & 0x900]
    assert rows.tolist() == kept and sizes["n_kept"] == len(kept)
    blob, n_rev = text.tobytes(), 0
    for k, i in enumerate(kept):
        f = sam[i].rstrip(b"\n").split(b"\t")
        flag, seq, qual = int(f[1]), f[9], f[10]
        seq = b"" if seq == b"*" else seq
        qual = b"\"" * len(seq) if qual == b"*" else qual
        if flag & 0x10:
            seq, qual, n_rev = seq.translate(_RC)[::-1], qual[::-1], n_rev + 1
        tail = b"/1" if flag & 0x1 and flag & 0xC0 == 0x40 else b"/2" if flag & 0x1 and flag & 0xC0 == 0x80 else b""
        assert blob[int(rec_off[k]):int(rec_off[k + 1])] == b"@" + f[0] + tail + b"\n" + seq + b"\n+\n" + qual + b"\n", i
    assert n_rev > 500


@pytest.mark.parametrize("name", BUNDLED_TOTALS)
def test_bundled_files(name):
    _, flat, starts, _, _, _ = bundled(name)
    u8 = np.frombuffer(flat, np.uint8)
    for fasta, literal in zip((False, True), BUNDLED_TOTALS[name]):
        want = fc.restate(flat, starts, fasta=fasta, filter={"flag_exclude": 0x900})
        assert (want["sizes"]["n_kept"], want["sizes"]["text_bytes"]) == literal
        same(sb.fastq_host(u8, starts, filter={"flag_exclude": 0x900}, fasta=fasta), want)
    same(sb.fastq_host(u8, starts, split=True, suffix="always"), fc.restate(flat, starts, split=True, suffix="always"))


def test_exports():
    assert {"sbh_records_fastq_scan", "sbh_records_fastq_device_ptr", "sbh_records_fastq_fetch",
            "sbh_fastq_render_host"} <= set(sb._lib.EXPORTS)
    for k in ("fastq", "fastq_host", "fastq_mode", "FastqResult"):
        assert k in sb.__all__ and getattr(sb, k)
    assert callable(sb.Shard.records_fastq) and callable(sb.Shard.fastq_ptr)
