"""csrc/fastq_core.h's host renderer built with -fsanitize=address,undefined and run as a stand-alone
program (tests/sanitize/fastq_driver.cpp) over the small FASTQ corpora and the malformed streams,
every buffer at its exact size: a memory or UB error aborts the program.  Nothing is loaded into
Python; the program's answers are compared, by FNV hash, with the restatement of fastq_corpus.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pkg import sb
import fastq_corpus as fc
import record_corpus as rc

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
NO_ROW = 2 ** 64 - 1
FNV0 = 0xcbf29ce484222325


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fastq_san") / "fastq_driver")
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "fastq_driver.cpp"), "-o", exe], check=True)
    return exe


def fnv1a64(b):
    h = FNV0
    for x in bytes(b):
        h = ((h ^ x) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def run(driver, tmp_path, flat, starts, fasta=False, suffix="auto", split=False, def_qual=1, filter=None, mode=None):
    p = tmp_path / "in.bin"
    p.write_bytes(fc.driver_input(flat, starts, sb.fastq_mode(fasta, suffix, split) if mode is None else mode, def_qual, filter))
    r = subprocess.run([driver, str(p)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    f = r.stdout.split()
    return dict(status=int(f[0]), bad_row=int(f[1]), text=int(f[11], 16), rec_off=int(f[12], 16), rows=int(f[13], 16),
                sizes={"n": int(f[2]), "n_kept": int(f[3]), "text_bytes": int(f[4]), "part_bytes": [int(x) for x in f[5:8]],
                       "part_rows": [int(x) for x in f[8:11]]})


@pytest.mark.parametrize("kv", fc.ALL_SMALL, ids=fc.ident)
def test_corpora(driver, tmp_path, kv):
    name, v = kv
    c, want = fc.get(name), fc.expected(name, v)
    got = run(driver, tmp_path, c.flat, c.starts, **fc.VARIANTS[name][v])
    assert got["status"] == 0 and got["bad_row"] == NO_ROW and got["sizes"] == want["sizes"]
    assert got["text"] == fnv1a64(want["text"])
    assert got["rec_off"] == fnv1a64(np.asarray(want["rec_off"], "<u8").tobytes())
    assert got["rows"] == fnv1a64(np.asarray(want["rows"], "<u8").tobytes())


def test_no_rows_and_no_bytes(driver, tmp_path):
    for flat in (rc.header(), b""):
        got = run(driver, tmp_path, flat, [], split=True)
        assert got["status"] == 0 and got["sizes"] == fc.expected("rows_0", 0)["sizes"]
        assert got["text"] == FNV0 and got["rec_off"] == fnv1a64(bytes(8)) and got["rows"] == FNV0


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed(driver, tmp_path, m):
    got = run(driver, tmp_path, m.stream.flat, m.stream.starts)
    assert (got["status"], got["bad_row"]) == (1, 3)
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        got = run(driver, tmp_path, m.stream.flat, m.stream.starts[:2] + [p], split=True)
        assert (got["status"], got["bad_row"]) == (1, 2)


def test_bad_arguments_are_refused(driver, tmp_path):
    c = fc.get("flags")
    assert run(driver, tmp_path, c.flat, c.starts, mode=16)["status"] == 2
    assert run(driver, tmp_path, c.flat, c.starts, def_qual=94)["status"] == 2
    assert run(driver, tmp_path, c.flat, c.starts, def_qual=-1)["status"] == 2
    assert run(driver, tmp_path, c.flat, c.starts, filter={"rows": [(5, 5)]})["status"] == 2
    assert run(driver, tmp_path, c.flat, c.starts, filter={"min_mapq": 256})["status"] == 2
