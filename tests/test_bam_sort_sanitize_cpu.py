"""csrc/bam_sort_core.h's host sorter and header rewrite built with -fsanitize=address,undefined and
run as a stand-alone program (tests/sanitize/bam_sort_driver.cpp) over the sort corpora, malformed
streams and every header shape: a memory or UB error aborts the program.  Nothing is loaded into
Python; the program's answers are compared, by size and FNV hash, with the numpy restatement."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import bam_sort_corpus as sc
import record_corpus as rc

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
NO_ROW = 2 ** 64 - 1
FNV0 = 0xcbf29ce484222325


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sort_san") / "bam_sort_driver")
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "bam_sort_driver.cpp"), "-o", exe], check=True)
    return exe


def fnv1a64(b):
    h = FNV0
    for x in np.frombuffer(bytes(b), np.uint8).tolist():
        h = ((h ^ x) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def run(driver, tmp_path, flat, starts, head=None, so=b"coordinate"):
    p = tmp_path / "in.bin"
    p.write_bytes(sc.driver_input(flat, starts, rc.header() if head is None else head, so))
    r = subprocess.run([driver, str(p)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    status, bad, hp, hstatus, hn, hh = r.stdout.split()
    return (int(status), int(bad), int(hp, 16)), (int(hstatus), int(hn), int(hh, 16))


@pytest.mark.parametrize("name", sc.SMALL)
def test_corpora(driver, tmp_path, name):
    s = sc.stream(name)
    got, _ = run(driver, tmp_path, s.flat, s.starts)
    assert got == (0, NO_ROW, fnv1a64(sc.expected_perm(name).astype("<u8").tobytes()))


def test_rows_in_any_order_and_none(driver, tmp_path):
    s = sc.stream("shuffled")
    st = np.concatenate([s.starts[:50][::-1], s.starts[:50], s.starts[7:8].repeat(3)])
    assert run(driver, tmp_path, s.flat, st)[0] == (0, NO_ROW, fnv1a64(sc.perm_ref(s.flat, st).astype("<u8").tobytes()))
    assert run(driver, tmp_path, s.flat, [])[0] == (0, NO_ROW, FNV0)
    assert run(driver, tmp_path, b"", [])[0] == (0, NO_ROW, FNV0)


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed(driver, tmp_path, m):
    assert run(driver, tmp_path, m.stream.flat, m.stream.starts)[0] == (1, 3, FNV0)
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        assert run(driver, tmp_path, m.stream.flat, m.stream.starts[:2] + [p])[0] == (1, 2, FNV0)


@pytest.mark.parametrize("shape", sc.HEADER_SHAPES, ids=lambda s: s[0])
def test_header_shapes(driver, tmp_path, shape):
    _, text, pad, want_text = shape
    want = sc.header_with(want_text, pad)
    assert run(driver, tmp_path, b"", [], sc.header_with(text, pad))[1] == (0, len(want), fnv1a64(want))


@pytest.mark.parametrize("head", [b"", b"BAM\1", b"BAM\1\xff\xff\xff\x7f" + bytes(6), b"BAM\1\x09\0\0\0" + bytes(8),
                                  rc.header()[:-1][:20]], ids=repr)
def test_truncated_headers_are_refused(driver, tmp_path, head):
    assert run(driver, tmp_path, b"", [], head)[1][0] == 1


def test_bad_values_are_refused(driver, tmp_path):
    for so in (b"", b"a\tb"):
        assert run(driver, tmp_path, b"", [], rc.header(), so)[1][0] == 1
