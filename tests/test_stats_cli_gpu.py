"""`spark-bam stats` (cli/spark_bam.cpp, csrc/stats_core.h's renderer) against api.stats' text (the
Python renderer), byte for byte."""
import os
import subprocess

import pytest

from conftest import ROOT, golden_bam
from pkg import sb

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "cli", "spark-bam")


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_the_command_prints_the_python_renderer_s_bytes(tmp_path):
    bam = golden_bam("2.bam")
    with sb.Context(0) as ctx:
        plain = sb.stats(bam, ctx=ctx).text()
        filtered = sb.stats(bam, flag_exclude=0x404, min_mapq=20, ctx=ctx).text()
        small = sb.stats(bam, flag_require=1, cycles=8, max_insert=16, ctx=ctx).text()
    assert plain.startswith(b"SN\tsequences:\t2500\n") and plain != filtered != small
    assert run("stats", bam) == plain
    assert run("stats", "-F", "0x404", "-q", "20", bam) == filtered
    assert run("stats", "-f", "1", "--cycles", "8", "-i", "16", bam) == small
    for text, opts in ((plain, ()), (small, ("-f", "1", "--cycles", "8", "-i", "16"))):
        path = str(tmp_path / "out.txt")
        assert run("stats", *opts, "-o", path, bam) == b""
        with open(path, "rb") as fh:
            assert fh.read() == text


def test_bad_options_are_usage_errors():
    bam = golden_bam("2.bam")
    for args in (("stats", "-x", bam), ("stats", "--cycles", "0", bam), ("stats", "-i", "1048577", bam), ("stats", "--cycles", "65537", bam)):
        r = subprocess.run([CLI, *args], capture_output=True, timeout=300)
        assert r.returncode != 0 and r.stdout == b"" and (b"usage" in r.stderr or b"stats:" in r.stderr)
