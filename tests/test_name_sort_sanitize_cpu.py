"""csrc/bam_name_core.h's host sorter built with -fsanitize=address,undefined and run as a stand-alone
program (tests/sanitize/name_sort_driver.cpp) over the small name corpora, malformed streams and
starts past the stream: a memory or UB error aborts the program.  Nothing is loaded into Python; the
program's answers are compared, by FNV hash and by the summary's numbers, with the restatement."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import name_sort_corpus as nc
import record_corpus as rc

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
NO_ROW = 2 ** 64 - 1
FNV0 = 0xcbf29ce484222325


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("name_san") / "name_sort_driver")
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "name_sort_driver.cpp"), "-o", exe], check=True)
    return exe


def fnv1a64(b):
    h = FNV0
    for x in np.frombuffer(bytes(b), np.uint8).tolist():
        h = ((h ^ x) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def run(driver, tmp_path, flat, starts):
    """((status, bad row, perm hash), info dict without the device's two numbers)"""
    p = tmp_path / "in.bin"
    p.write_bytes(nc.driver_input(flat, starts))
    r = subprocess.run([driver, str(p)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    w = r.stdout.split()
    info = dict(zip(("n_names", "n_single", "n_pair", "n_more", "max_name"), map(int, w[3:8])), already=bool(int(w[8])))
    return (int(w[0]), int(w[1]), int(w[2], 16)), info


def want_info(flat, starts):
    info = nc.info_ref(flat, starts)
    del info["chunks_run"], info["passes_run"]
    return info


@pytest.mark.parametrize("name", nc.SMALL)
def test_corpora(driver, tmp_path, name):
    s = nc.stream(name)
    got, info = run(driver, tmp_path, s.flat, s.starts)
    assert got == (0, NO_ROW, fnv1a64(nc.expected_perm(name).astype("<u8").tobytes()))
    assert info == want_info(s.flat, s.starts)


def test_the_last_record_s_name_ends_the_buffer(driver, tmp_path):
    """A 254-byte name whose NUL is the stream's last byte, and an l_read_name of 0 in the last record."""
    for last in ((bytes(range(1, 255)), 0), (b"", 0, 0)):
        s = nc.stream_of([(b"zz", 0), last, (b"a", 0)][::-1] + [last])
        assert s.starts[-1] + len(nc.record(3, *last)) == len(s.flat)
        got, info = run(driver, tmp_path, s.flat, s.starts)
        assert got == (0, NO_ROW, fnv1a64(nc.perm_ref(s.flat, s.starts).astype("<u8").tobytes()))
        assert info == want_info(s.flat, s.starts)


def test_rows_in_any_order_and_none(driver, tmp_path):
    s = nc.stream("shuffled")
    st = np.concatenate([s.starts[:50][::-1], s.starts[:50], s.starts[7:8] * 3])
    got, info = run(driver, tmp_path, s.flat, st)
    assert got == (0, NO_ROW, fnv1a64(nc.perm_ref(s.flat, st).astype("<u8").tobytes())) and info == want_info(s.flat, st)
    assert run(driver, tmp_path, s.flat, [])[0] == (0, NO_ROW, FNV0)
    assert run(driver, tmp_path, b"", [])[0] == (0, NO_ROW, FNV0)


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed(driver, tmp_path, m):
    assert run(driver, tmp_path, m.stream.flat, m.stream.starts)[0] == (1, 3, FNV0)
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        assert run(driver, tmp_path, m.stream.flat, m.stream.starts[:2] + [p])[0] == (1, 2, FNV0)
