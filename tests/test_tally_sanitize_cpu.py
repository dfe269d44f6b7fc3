"""csrc/tally_core.h's host add and its two renderers built with -fsanitize=address,undefined and run
as a stand-alone program (tests/sanitize/tally_driver.cpp) over the small tally corpora and the
malformed streams: a memory or UB error aborts the program.  Nothing is loaded into Python; the
program's answers are compared, by FNV hash, with the numpy restatement and the Python renderers."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pkg import sb
import record_corpus as rc
import tally_corpus as tc

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
NO_ROW = 2 ** 64 - 1
FNV0 = 0xcbf29ce484222325


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tally_san") / "tally_driver")
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "tally_driver.cpp"), "-o", exe], check=True)
    return exe


def fnv1a64(b):
    h = FNV0
    for x in np.frombuffer(bytes(b), np.uint8).tolist():
        h = ((h ^ x) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def run(driver, tmp_path, flat, starts, n_ref, filter=None):
    p = tmp_path / "in.bin"
    p.write_bytes(tc.driver_input(flat, starts, n_ref, filter))
    r = subprocess.run([driver, str(p)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    f = r.stdout.split()
    return dict(status=int(f[0]), bad_row=int(f[1]), n=int(f[2]), n_kept=int(f[3]), flag=int(f[4], 16), ref=int(f[5], 16),
                flagstat=int(f[6], 16), idxstats=int(f[7], 16))


def names_of(n_ref):
    """The driver's references."""
    return ["ref%d" % k for k in range(n_ref)], [1000 + k for k in range(n_ref)]


# (n_ref_200000 hashes 3 MB of counters and 4 MB of text in Python: about two seconds)
@pytest.mark.parametrize("name", tc.SMALL)
def test_corpora(driver, tmp_path, name):
    c, want = tc.get(name), tc.expected(name)
    got = run(driver, tmp_path, c.flat, c.starts, c.n_ref, c.filter)
    assert got["status"] == 0 and got["bad_row"] == NO_ROW
    assert (got["n"], got["n_kept"]) == (want["n"], want["n_kept"])
    assert got["flag"] == fnv1a64(want["flag"].astype("<u8").tobytes())
    assert got["ref"] == fnv1a64(want["ref"].astype("<u8").tobytes())
    # the C++ renderers print the Python renderers' bytes
    assert got["flagstat"] == fnv1a64(sb.flagstat_text(want["flag"]))
    assert got["idxstats"] == fnv1a64(sb.idxstats_text(want["ref"], *names_of(c.n_ref)))


def test_no_rows_and_no_bytes(driver, tmp_path):
    for flat in (rc.header(), b""):
        for n_ref in (0, 3):
            got = run(driver, tmp_path, flat, [], n_ref)
            assert got["status"] == 0 and got["n_kept"] == 0
            assert got["flag"] == fnv1a64(bytes(256)) and got["ref"] == fnv1a64(bytes(16 * (n_ref + 1)))
            assert got["flagstat"] == fnv1a64(sb.flagstat_text(np.zeros((16, 2), np.uint64)))


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed(driver, tmp_path, m):
    got = run(driver, tmp_path, m.stream.flat, m.stream.starts, tc.N_REF)
    assert (got["status"], got["bad_row"]) == (1, 3)
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        got = run(driver, tmp_path, m.stream.flat, m.stream.starts[:2] + [p], tc.N_REF)
        assert (got["status"], got["bad_row"]) == (1, 2)


def test_reference_out_of_range(driver, tmp_path):
    c = tc.TID_KEPT()
    got = run(driver, tmp_path, c.flat, c.starts, c.n_ref)
    assert (got["status"], got["bad_row"]) == (1, 2)
    # the largest reference id there is, kept, against the exactly-sized counters of one reference
    c = tc.case([tc.one(0), tc.one(2 ** 31 - 1)])
    assert (lambda g: (g["status"], g["bad_row"]))(run(driver, tmp_path, c.flat, c.starts, 1)) == (1, 1)
    assert (lambda g: (g["status"], g["bad_row"]))(run(driver, tmp_path, c.flat, c.starts, 0)) == (1, 0)


def test_bad_filters_and_n_ref_are_refused(driver, tmp_path):
    c = tc.get("pair_rows")
    assert run(driver, tmp_path, c.flat, c.starts, -1)["status"] == 2
    assert run(driver, tmp_path, c.flat, c.starts, tc.N_REF, {"rows": [(5, 5)]})["status"] == 2
    assert run(driver, tmp_path, c.flat, c.starts, tc.N_REF, {"min_mapq": 256})["status"] == 2
