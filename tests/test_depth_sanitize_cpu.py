"""csrc/depth_core.h's host add and finish built with -fsanitize=address,undefined and run as a
stand-alone program (tests/sanitize/depth_driver.cpp) over the small depth corpora, the malformed
streams and the 64-bit-position rows: a memory or UB error aborts the program.  Nothing is loaded
into Python; the program's answers are compared, by size and FNV hash, with the numpy restatement."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import depth_corpus as dc
import record_corpus as rc

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
NO_ROW = 2 ** 64 - 1
FNV0 = 0xcbf29ce484222325
ADD_KEYS = ("n", "n_kept", "n_counted", "n_unplaced", "cov_bases")
SIZE_KEYS = ("slots", "n_runs", "covered", "sum", "max_depth")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("depth_san") / "depth_driver")
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "depth_driver.cpp"), "-o", exe], check=True)
    return exe


def fnv1a64(b):
    h = FNV0
    for x in np.frombuffer(bytes(b), np.uint8).tolist():
        h = ((h ^ x) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def run(driver, tmp_path, flat, starts, spans, n_ref=dc.N_REF, filter=None, count_del=False):
    p = tmp_path / "in.bin"
    p.write_bytes(dc.driver_input(flat, starts, spans, n_ref, filter, count_del))
    r = subprocess.run([driver, str(p)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    f = r.stdout.split()
    return dict(status=int(f[0]), bad_row=int(f[1]), add=dict(zip(ADD_KEYS, map(int, f[2:7]))),
                stats=dict(zip(SIZE_KEYS, map(int, f[7:12]))), depth=int(f[12], 16), runs=int(f[13], 16))


# (the two 20 000-row corpora hash 30 000 slots in Python: still well under a second each)
@pytest.mark.parametrize("name", dc.SMALL)
def test_corpora(driver, tmp_path, name):
    c, want = dc.get(name), dc.expected(name)
    got = run(driver, tmp_path, c.flat, c.starts, c.spans, dc.N_REF, c.filter, c.count_del)
    assert got["status"] == 0 and got["bad_row"] == NO_ROW
    assert got["add"] == want["add"] and got["stats"] == want["stats"]
    assert got["depth"] == fnv1a64(want["depth"].astype("<u4").tobytes())
    assert got["runs"] == fnv1a64(want["runs"].tobytes())


def test_no_rows_and_no_bytes(driver, tmp_path):
    for flat in (rc.header(), b""):
        got = run(driver, tmp_path, flat, [], [(0, 5, 9)])
        assert got["status"] == 0 and got["stats"] == dict(slots=5, n_runs=1, covered=0, sum=0, max_depth=0)
        assert got["depth"] == fnv1a64(bytes(20))


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed(driver, tmp_path, m):
    got = run(driver, tmp_path, m.stream.flat, m.stream.starts, [(1, 0, 2000)])
    assert (got["status"], got["bad_row"]) == (1, 3)
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        got = run(driver, tmp_path, m.stream.flat, m.stream.starts[:2] + [p], [(1, 0, 2000)])
        assert (got["status"], got["bad_row"]) == (1, 2)


def test_bad_op_and_reference(driver, tmp_path):
    c = dc.OP9_KEPT()
    got = run(driver, tmp_path, c.flat, c.starts, c.spans)
    assert (got["status"], got["bad_row"]) == (1, 1)
    c = dc.case([dc.one(1, [(4, dc.M)]), dc.one(1, [(4, dc.M)], ref=dc.N_REF)], [(0, 0, 100)])
    got = run(driver, tmp_path, c.flat, c.starts, c.spans)
    assert (got["status"], got["bad_row"]) == (1, 1)


def test_64_bit_positions_at_the_last_slot(driver, tmp_path):
    # the span ends at the last position there is: the closing events of both rows fall on its
    # extra slot, the last int of the exactly-sized array
    c = dc.case([dc.one(dc.POS_MAX - 2, dc.WRAP, ref=2), dc.one(dc.POS_MAX - 1, [(268435455, dc.M)] * 16, ref=2)],
                [(2, dc.POS_MAX - 50, dc.POS_MAX)])
    want = dc.restate(c.flat, c.starts, c.spans)
    assert want["add"]["cov_bases"] == 2 + 1 and want["depth"].tolist()[-4:] == [0, 1, 2, 0]
    got = run(driver, tmp_path, c.flat, c.starts, c.spans)
    assert got["status"] == 0 and got["add"] == want["add"] and got["stats"] == want["stats"]
    assert got["depth"] == fnv1a64(want["depth"].astype("<u4").tobytes())


def test_bad_spans_and_filters_are_refused(driver, tmp_path):
    s = rc.lay([dc.one(1, [(4, dc.M)])])
    for spans in ([], [(1, 0, 10), (0, 0, 10)], [(0, 10, 10)], [(dc.N_REF, 0, 10)], [(0, 0, 2 ** 31)]):
        assert run(driver, tmp_path, s.flat, s.starts, spans)["status"] == 2
    assert run(driver, tmp_path, s.flat, s.starts, [(0, 0, 10)], filter={"rows": [(5, 5)]})["status"] == 2
