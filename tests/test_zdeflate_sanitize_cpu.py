"""csrc/zdeflate_core.h's serial definition built with -fsanitize=address,undefined and run as a
stand-alone program (tests/sanitize/zdeflate_driver.cpp) over the conformance corpus
(tests/zdeflate_corpus.py), with the source and every scratch array at exactly the promised size: a
memory or UB error aborts the program.  Nothing is loaded into Python; each stream's size and FNV
hash are compared with libz's bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import zdeflate_corpus as zc
from conftest import ROOT
from test_zdeflate_cpu import zlib_raw

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("zdeflate_san") / "zdeflate_driver")
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "zdeflate_driver.cpp"), "-o", exe], check=True)
    return exe


def fnv1a64(b):
    h = 0xcbf29ce484222325
    for x in np.frombuffer(bytes(b), np.uint8).tolist():
        h = ((h ^ x) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def run(driver, tmp_path, records):
    p = tmp_path / "corpus.bin"
    p.write_bytes(b"".join(struct.pack("<II", lv, len(d)) + d for d, lv in records))
    r = subprocess.run([driver, str(p)], env=ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [(int(a), int(b, 16)) for a, b in (l.split() for l in r.stdout.splitlines())]
    assert len(got) == len(records)
    for (d, lv), g in zip(records, got):
        z = zlib_raw(d, lv)
        assert g == (len(z), fnv1a64(z)), (len(d), lv)


def test_small_cases_every_level(driver, tmp_path):
    run(driver, tmp_path, [(c.data, lv) for c in zc.CASES if len(c.data) < zc.SMALL for lv in (4, 5, 6, 7, 8, 9)])


def test_large_cases(driver, tmp_path):
    """(one level each, in turn: the Python side hashes every stream)"""
    big = [c for c in zc.CASES if len(c.data) >= zc.SMALL]
    run(driver, tmp_path, [(c.data, c.levels[i % len(c.levels)]) for i, c in enumerate(big)])


def test_degenerate_sizes(driver, tmp_path):
    """No bytes at all, and lengths around MIN_MATCH, where the hash and the lookahead run out."""
    run(driver, tmp_path, [(bytes([65] * n), lv) for n in (0, 1, 2, 3, 4, 5) for lv in (4, 5, 9)])
