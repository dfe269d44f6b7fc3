"""csrc/pileup_core.h's host add and finish built with -fsanitize=address,undefined and run as a
stand-alone program (tests/sanitize/pileup_driver.cpp) over the small pileup corpora, the hand-worked
case, the bad kept rows, the malformed streams and a span that ends on the last position there is: a
memory or UB error aborts the program.  The flat bytes, the counts, the calls and the intervals are
heap blocks of exactly their sizes.  Nothing is loaded into Python; the program's answers are
compared, by size and FNV hash, with the numpy restatement."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import pileup_corpus as pc
import record_corpus as rc

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
NO_ROW = 2 ** 64 - 1
FNV0 = 0xcbf29ce484222325
SIZE_KEYS = ("positions", "n_intervals", "nonzero", "n_called", "covered", "max_depth")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pileup_san") / "pileup_driver")
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "pileup_driver.cpp"), "-o", exe], check=True)
    return exe


def fnv1a64(b):
    h = FNV0
    for x in np.frombuffer(bytes(b), np.uint8).tolist():
        h = ((h ^ x) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def run(driver, tmp_path, c, n_ref=pc.N_REF):
    p = tmp_path / "in.bin"
    p.write_bytes(pc.driver_input(c.flat, c.starts, c.spans, n_ref, c.filter, c.min_baseq, c.min_depth, c.call_pct))
    r = subprocess.run([driver, str(p)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    f = r.stdout.split()
    v = list(map(int, f[:28]))
    return dict(status=v[0], bad_row=v[1], add=dict(n=v[2], n_kept=v[3], n_counted=v[4], n_unplaced=v[5], totals=v[6:14]),
                stats=dict(zip(SIZE_KEYS, v[14:20]), totals=v[20:28]), counts=int(f[28], 16), calls=int(f[29], 16),
                intervals=int(f[30], 16))


def equals(got, want):
    assert got["status"] == 0 and got["bad_row"] == NO_ROW
    assert got["add"] == want["add"] and got["stats"] == want["stats"]
    assert got["counts"] == fnv1a64(want["counts"].astype("<u4").tobytes())
    assert got["calls"] == fnv1a64(want["calls"].tobytes())
    assert got["intervals"] == fnv1a64(want["intervals"].tobytes())


# (the largest small corpus hashes 6 K positions x 33 bytes in Python: well under a second;
# wrap_64bit's 2^20 positions are left to the CPU and GPU tests, which compare arrays)
@pytest.mark.parametrize("name", [k for k in pc.SMALL if k != "wrap_64bit"])
def test_corpora(driver, tmp_path, name):
    equals(run(driver, tmp_path, pc.get(name)), pc.expected(name))


def test_the_hand_worked_case(driver, tmp_path):
    h = pc.HAND
    got = run(driver, tmp_path, pc.hand_case())
    assert got["status"] == 0 and got["add"] == h["add"] and got["stats"] == h["stats"]
    assert got["counts"] == fnv1a64(np.asarray(h["table"], "<u4").tobytes())
    assert got["calls"] == fnv1a64(h["calls"]) and got["intervals"] == fnv1a64(pc.span_array(h["intervals"]).tobytes())


def test_the_last_record_ends_the_heap_block(driver, tmp_path):
    """An odd l_seq and its qualities are the flat block's last bytes: one nibble or byte further is
    past the allocation."""
    c = pc.case([pc.read(10, [(5, pc.M)]), pc.read(12, [(2, pc.S), (2 * pc.G + 1, pc.M)], seed=3)], [(0, 0, 200)], min_baseq=40)
    equals(run(driver, tmp_path, c), pc.restate(c.flat, c.starts, c.spans, pc.N_REF, None, 40))


def test_no_rows_and_no_bytes(driver, tmp_path):
    for flat in (rc.header(), b""):
        got = run(driver, tmp_path, pc.Case(flat, [], [(0, 5, 9)], None, 0, 1, 75))
        assert got["status"] == 0
        assert got["stats"] == dict(positions=4, n_intervals=0, nonzero=0, n_called=0, covered=0, max_depth=0, totals=[0] * 8)
        assert got["counts"] == fnv1a64(bytes(128)) and got["calls"] == fnv1a64(bytes(4)) and got["intervals"] == FNV0


@pytest.mark.parametrize("name", pc.BAD_KEPT)
def test_bad_kept_rows(driver, tmp_path, name):
    c, row = pc.BAD_KEPT[name]()
    got = run(driver, tmp_path, c)
    assert (got["status"], got["bad_row"]) == (1, row)


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed(driver, tmp_path, m):
    got = run(driver, tmp_path, pc.Case(m.stream.flat, m.stream.starts, [(1, 0, 2000)], None, 0, 1, 75))
    assert (got["status"], got["bad_row"]) == (1, 3)
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        got = run(driver, tmp_path, pc.Case(m.stream.flat, m.stream.starts[:2] + [p], [(1, 0, 2000)], None, 0, 1, 75))
        assert (got["status"], got["bad_row"]) == (1, 2)


def test_64_bit_positions_at_the_last_position(driver, tmp_path):
    # the span ends at the last position there is: the last counted base, deletion and insertion
    # fall on the last row of the exactly-sized table; what follows runs past 2^32
    c = pc.case([pc.read(pc.POS_MAX - 2, pc.WRAP, ref=2),
                 pc.read(pc.POS_MAX - 3, [(2, pc.M), (1, pc.I), (5, pc.D), (268435455, pc.N)] + [(268435455, pc.M)] * 2, ref=2,
                         codes=(), qual=b"")],
                [(2, pc.POS_MAX - 50, pc.POS_MAX)])
    want = pc.restate(c.flat, c.starts, c.spans)
    assert sum(want["add"]["totals"]) == 2 + (2 + 1 + 1) and want["counts"][-1].tolist() == [0, 0, 0, 0, 1, 1, 0, 0]
    equals(run(driver, tmp_path, c), want)


def test_bad_spans_filters_and_parameters_are_refused(driver, tmp_path):
    s = rc.lay([pc.read(1, [(4, pc.M)])])
    for spans in ([], [(1, 0, 10), (0, 0, 10)], [(0, 10, 10)], [(pc.N_REF, 0, 10)], [(0, 0, 2 ** 31)]):
        assert run(driver, tmp_path, pc.Case(s.flat, s.starts, spans, None, 0, 1, 75))["status"] == 2
    assert run(driver, tmp_path, pc.Case(s.flat, s.starts, [(0, 0, 10)], {"rows": [(5, 5)]}, 0, 1, 75))["status"] == 2
    for mb, md, pct in ((256, 1, 75), (0, 0, 75), (0, 1, 0), (0, 1, 101)):
        assert run(driver, tmp_path, pc.Case(s.flat, s.starts, [(0, 0, 10)], None, mb, md, pct))["status"] == 2
