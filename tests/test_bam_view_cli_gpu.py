"""`spark-bam view -b` (cli/spark_bam.cpp) against the reference's HTSJDKRewriteTest slice, api.view_bam
and `spark-bam index-bai`."""
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
    return r


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_row_range_is_the_reference_slice(tmp_path):
    out = str(tmp_path / "slice.bam")
    run("view", "-b", "-r", "100-1000", "-o", out, golden_bam("2.bam"))
    assert read(out) == read(golden_bam("2.100-1000.bam"))


@pytest.mark.parametrize("args,kw", [
    (("-f", "0x10"), {"flag_require": 0x10}),
    (("-f", "64", "-F", "0x10"), {"flag_require": 0x40, "flag_exclude": 0x10}),
    (("-q", "30"), {"min_mapq": 30}),
    (("-F", "4", "-q", "1", "-r", "5-50,40-90,2000-2400", "--level", "-1"),
     {"flag_exclude": 4, "min_mapq": 1, "rows": list(range(5, 90)) + list(range(2000, 2400)), "level": -1}),
], ids=("f", "f-F", "q", "F-q-r-level"))
def test_filters_equal_view_bam(tmp_path, args, kw):
    out = str(tmp_path / "f.bam")
    run("view", "-b", "-o", out, *args, golden_bam("2.bam"))
    with sb.Context(0) as ctx:
        assert read(out) == sb.view_bam(golden_bam("2.bam"), ctx=ctx, **kw)


def test_bam_output_needs_an_output_path():
    r = subprocess.run([CLI, "view", "-b", golden_bam("2.bam")], capture_output=True, timeout=300)
    assert r.returncode != 0 and b"usage" in r.stderr and r.stdout == b""
    r = subprocess.run([CLI, "view", "-f", "16", golden_bam("2.bam")], capture_output=True, timeout=300)
    assert r.returncode != 0 and b"-b" in r.stderr and r.stdout == b""


def test_index_bai_side_output(tmp_path):
    out = str(tmp_path / "q.bam")
    run("view", "-b", "-q", "1", "--index-bai", "-o", out, golden_bam("2.bam"))
    run("index-bai", out, out + ".again")
    assert read(out + ".bai") == read(out + ".again") and read(out + ".bai")[:4] == b"BAI\1"
