"""csrc/bam_gather_core.h's host gatherer built with -fsanitize=address,undefined and run as a
stand-alone program (tests/sanitize/bam_gather_driver.cpp) over the residue ladder, the long
record, the decode corpus and every malformed stream: a memory or UB error aborts the program.
Nothing is loaded into Python; the program's answers are compared, by size and FNV hash, with
the numpy restatement."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import bam_gather_corpus as bc
import record_corpus as rc

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
NO_ROW = 2 ** 64 - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bam_san") / "bam_gather_driver")
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "bam_gather_driver.cpp"), "-o", exe], check=True)
    return exe


def fnv1a64(b):
    h = 0xcbf29ce484222325
    for x in np.frombuffer(bytes(b), np.uint8).tolist():
        h = ((h ^ x) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def run(driver, tmp_path, flat, starts, head, **f):
    p = tmp_path / "in.bin"
    p.write_bytes(bc.driver_input(flat, starts, head, **f))
    r = subprocess.run([driver, str(p)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    status, bad, n_kept, total, h, hi = r.stdout.split()
    return int(status), int(bad), int(n_kept), int(total), int(h, 16), int(hi, 16)


def want(flat, starts, head, **f):
    stream, off, rows = bc.gather_ref(flat, starts, head, **f)
    return 0, NO_ROW, len(rows), len(stream), fnv1a64(stream), fnv1a64(off.astype("<u8").tobytes()
                                                                      + rows.astype("<u8").tobytes())


def test_ladder_every_head(driver, tmp_path):
    s = bc.ladder_stream()
    for head in bc.HEADS:
        assert run(driver, tmp_path, s.flat, s.starts, head, rows=bc.LADDER_ROWS) == \
            want(s.flat, s.starts, head, rows=bc.LADDER_ROWS)


@pytest.mark.parametrize("pattern", bc.PATTERNS)
def test_long_and_decode_streams(driver, tmp_path, pattern):
    for name, s in bc.streams():
        rows = bc.pattern_ranges(pattern, len(s.starts))
        assert run(driver, tmp_path, s.flat, s.starts, bc.HEADS[7], rows=rows) == \
            want(s.flat, s.starts, bc.HEADS[7], rows=rows), name


def test_filters_and_odd_rows(driver, tmp_path):
    s = rc.decode_stream()
    n = len(s.starts)
    for f in ({"flag_require": 0xFFFF, "flag_exclude": 0xFFFF}, {"flag_exclude": 4, "min_mapq": 7},
              {"rows": [(n - 2, n + 5), (n + 7, 2 ** 63)]}):
        assert run(driver, tmp_path, s.flat, s.starts, b"", **f) == want(s.flat, s.starts, b"", **f)
    st = list(s.starts[:9])
    twice = st[::-1] + st + [st[4]] * 3  # descending, then duplicates
    assert run(driver, tmp_path, s.flat, twice, b"abc") == want(s.flat, twice, b"abc")
    assert run(driver, tmp_path, s.flat, [], b"abc") == want(s.flat, [], b"abc")
    assert run(driver, tmp_path, b"", [], b"") == want(b"", [], b"")
    assert run(driver, tmp_path, s.flat, s.starts, b"", rows=[(3, 3)])[0] == 5  # an empty range: refused


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed(driver, tmp_path, m):
    for f in ({}, {"flag_require": 0xFFFF}, {"rows": [(0, 1)]}):
        status, bad, n_kept, total, _, _ = run(driver, tmp_path, m.stream.flat, m.stream.starts, b"hd", **f)
        assert (status, bad, n_kept, total) == (1, 3, 0, 2)
    # a start past the stream, and one so large that start + 36 wraps
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):
        status, bad, _, _, _, _ = run(driver, tmp_path, m.stream.flat, m.stream.starts[:2] + [p], b"")
        assert (status, bad) == (1, 2)
