"""csrc/sam_core.h's host renderer built with -fsanitize=address,undefined and run as a
stand-alone program (tests/sanitize/sam_driver.cpp) over 2.bam's flat bytes, the hand-built corpus,
the Float.toString literals and every malformed row: a memory or UB error aborts the program.
Nothing is loaded into Python; the program's answers are compared with the library's."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pkg import sb
import record_corpus as rc
import sam_corpus as sc
from test_sam_cpu import two_bam

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sam_san") / "sam_driver")
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "sam_driver.cpp"), "-o", exe], check=True)
    return exe


def fnv1a64(b):
    h = 0xcbf29ce484222325
    for x in np.frombuffer(b, np.uint8).tolist():
        h = ((h ^ x) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def run(driver, tmp_path, flat, starts, names):
    packed, off = sb.records.pack_ref_names(names)
    p = tmp_path / "in.bin"
    with open(p, "wb") as f:
        f.write(struct.pack("<Q", len(flat)) + bytes(flat) + struct.pack("<Q", len(starts)))
        f.write(np.asarray(starts, "<u8").tobytes() + struct.pack("<Q", len(names)) + off.astype("<u8").tobytes())
        f.write(bytes(packed[:int(off[-1])]))
    r = subprocess.run([driver, str(p)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    status, bad, n, total, h = r.stdout.split()
    return int(status), int(bad), int(n), int(total), int(h, 16)


def test_2bam(driver, tmp_path):
    flat, starts, names = two_bam()
    _, lines = sc.fixture_lines()
    want = b"".join(lines)
    assert run(driver, tmp_path, flat, starts, names) == (0, 2 ** 64 - 1, 2500, len(want), fnv1a64(want))


def test_corpus_and_floats(driver, tmp_path):
    s = rc.lay([r for _, r in sc.CASES] + [sc.float_record(x) for x, _ in sc.FLOATS])
    want = bytes(sb.sam_text_host(s.flat, s.starts, sc.REF_NAMES)[0])
    assert run(driver, tmp_path, s.flat, s.starts, sc.REF_NAMES) == (0, 2 ** 64 - 1, len(s.starts), len(want),
                                                                     fnv1a64(want))


@pytest.mark.parametrize("m", sc.MALFORMED + tuple(rc.MALFORMED_CASES), ids=lambda m: m.name)
def test_malformed(driver, tmp_path, m):
    bad_row = getattr(m, "bad_row", 3)
    status, bad, n, total, _ = run(driver, tmp_path, m.stream.flat, m.stream.starts, sc.REF_NAMES)
    assert (status, bad, n, total) == (1, bad_row, len(m.stream.starts), 0)
