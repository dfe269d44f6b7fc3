"""csrc/stats_core.h's host add and its renderer built with -fsanitize=address,undefined and run as a
stand-alone program (tests/sanitize/stats_driver.cpp) over the small stats corpora and the malformed
streams: a memory or UB error aborts the program.  Nothing is loaded into Python; the program's
answers are compared, by FNV hash, with the numpy restatement's tables and the Python renderer's
bytes."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pkg import sb
import record_corpus as rc
import stats_corpus as sc

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
NO_ROW = 2 ** 64 - 1
FNV0 = 0xcbf29ce484222325


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stats_san") / "stats_driver")
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "stats_driver.cpp"), "-o", exe], check=True)
    return exe


def fnv1a64(b):
    h = FNV0
    for x in np.frombuffer(bytes(b), np.uint8).tolist():
        h = ((h ^ x) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def table_hash(a):
    """The driver's hash of a table: (index, value) of its non-zero words, in order."""
    flat = np.asarray(a, np.uint64).ravel()
    at = np.flatnonzero(flat)
    return fnv1a64(np.stack([at.astype("<u8"), flat[at].astype("<u8")], axis=1).tobytes())


def run(driver, tmp_path, flat, starts, cycles, max_insert, filter=None):
    p = tmp_path / "in.bin"
    p.write_bytes(sc.driver_input(flat, starts, cycles, max_insert, filter))
    r = subprocess.run([driver, str(p)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    f = r.stdout.split()
    out = dict(status=int(f[0]), bad_row=int(f[1]), n=int(f[2]), n_kept=int(f[3]), n_counted=int(f[4]), text=int(f[12], 16))
    out.update({k: int(f[5 + i], 16) for i, k in enumerate(sc.TABLES)})
    return out


# (read_of_65536's restatement-side hashing is of a few hundred words: the tables are hashed by their non-zero words)
@pytest.mark.parametrize("name", sc.SMALL)
def test_corpora(driver, tmp_path, name):
    c, want = sc.get(name), sc.expected(name)
    got = run(driver, tmp_path, c.flat, c.starts, c.cycles, c.max_insert, c.filter)
    assert got["status"] == 0 and got["bad_row"] == NO_ROW
    assert (got["n"], got["n_kept"], got["n_counted"]) == (want["n"], want["n_kept"], want["n_counted"])
    for k in sc.TABLES:
        assert got[k] == table_hash(want[k]), k
    # the C++ renderer prints the Python renderer's bytes
    assert got["text"] == fnv1a64(sb.stats_text(want, c.cycles, c.max_insert))


def test_no_rows_and_no_bytes(driver, tmp_path):
    for flat in (rc.header(), b""):
        for cycles, max_insert in ((1, 1), (8, 16), (sc.STAT_CYCLES_MAX, sc.STAT_INSERT_MAX)):
            got = run(driver, tmp_path, flat, [], cycles, max_insert)
            assert got["status"] == 0 and got["n_kept"] == 0 and all(got[k] == FNV0 for k in sc.TABLES)
            assert got["text"] == fnv1a64(sb.stats_text(sc.zeros(8, 16), 8, 16))  # (no table line: the same bytes at any size)


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed(driver, tmp_path, m):
    got = run(driver, tmp_path, m.stream.flat, m.stream.starts, 8, 16)
    assert (got["status"], got["bad_row"]) == (1, 3)
    assert run(driver, tmp_path, m.stream.flat, m.stream.starts, 8, 16, {"flag_require": 0x1000})["bad_row"] == 3
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        got = run(driver, tmp_path, m.stream.flat, m.stream.starts[:2] + [p], 8, 16)
        assert (got["status"], got["bad_row"]) == (1, 2)


def test_bad_parameters_and_filters_are_refused(driver, tmp_path):
    c = sc.get("which")
    for cycles, max_insert in ((0, 16), (sc.STAT_CYCLES_MAX + 1, 16), (8, 0), (8, sc.STAT_INSERT_MAX + 1)):
        assert run(driver, tmp_path, c.flat, c.starts, cycles, max_insert)["status"] == 2
    assert run(driver, tmp_path, c.flat, c.starts, 8, 16, {"rows": [(5, 5)]})["status"] == 2
    assert run(driver, tmp_path, c.flat, c.starts, 8, 16, {"min_mapq": 256})["status"] == 2
