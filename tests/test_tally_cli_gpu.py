"""`spark-bam flagstat`, `idxstats` and `view -c` (cli/spark_bam.cpp) against the Python renderers,
byte for byte, and against the literals of test_tally_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_bam
from pkg import sb
import tally_corpus as tc
from test_tally_cpu import FLAGSTAT_1BAM, FLAGSTAT_2BAM, bundled, bundled_flag, bundled_ref

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "cli", "spark-bam")


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("name, literal", [("2.bam", FLAGSTAT_2BAM), ("1.bam", FLAGSTAT_1BAM)])
def test_the_commands_print_the_python_renderers_bytes(tmp_path, name, literal):
    _, flat, starts, names, lens, _ = bundled(name)
    bam = golden_bam(name)
    assert run("flagstat", bam) == sb.flagstat_text(bundled_flag(name)) == literal
    assert run("idxstats", bam) == sb.idxstats_text(bundled_ref(name, len(lens)), names, lens)
    assert run("view", "-c", bam) == b"%d\n" % len(starts)
    # the filter, into a file: the restatement's counts through the Python renderers
    f = {"flag_require": 0x1, "flag_exclude": 0x404, "min_mapq": 20}
    w = tc.restate(np.frombuffer(flat, np.uint8), starts, len(lens), f)
    opts = ("-f", "1", "-F", "0x404", "-q", "20")
    path = str(tmp_path / "out.txt")
    assert run("flagstat", *opts, "-o", path, bam) == b""
    with open(path, "rb") as fh:
        assert fh.read() == sb.flagstat_text(w["flag"])
    assert run("idxstats", *opts, bam) == sb.idxstats_text(w["ref"], names, lens)
    assert run("view", "-c", *opts, bam) == b"%d\n" % w["n_kept"]


def test_view_c_counts_the_mapped_reads_of_2_bam():
    assert run("view", "-c", "-F", "4", golden_bam("2.bam")) == b"2450\n"


def test_an_unknown_option_is_a_usage_error():
    bam = golden_bam("2.bam")
    for args in (("flagstat", "-x", bam), ("idxstats", "--bedgraph", bam), ("view", "-c", "-x", bam),
                 ("view", "-c", "-b", "-o", "out.bam", bam)):
        r = subprocess.run([CLI, *args], capture_output=True, timeout=300)
        assert r.returncode != 0 and b"usage" in r.stderr and r.stdout == b""
    r = subprocess.run([CLI, "flagstat"], capture_output=True, timeout=300)
    assert r.returncode != 0 and b"missing BAM path" in r.stderr
