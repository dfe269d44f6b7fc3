"""`spark-bam sort` and `spark-bam view -b --sort` (cli/spark_bam.cpp) against api.sort_bam /
api.view_bam(sort="coordinate") on 2.bam with its records shuffled, and `--index-bai`."""
import os
import subprocess

import pytest

from conftest import ROOT
from pkg import sb
from test_bam_sort_view_gpu import shuffled

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "cli", "spark-bam")


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def shuffled_path(tmp_path_factory):
    p = tmp_path_factory.mktemp("sort_cli") / "shuffled.bam"
    p.write_bytes(shuffled()[0])
    return str(p)


def test_sort_and_view_sort_equal_the_python_calls(tmp_path, shuffled_path):
    a, b, c = (str(tmp_path / n) for n in ("a.bam", "b.bam", "c.bam"))
    run("sort", "-o", a, "--index-bai", shuffled_path)
    run("view", "-b", "--sort", "--index-bai", "-o", b, shuffled_path)
    run("view", "-b", "--sort", "-F", "0x10", "-r", "100-1900", "--level", "-1", "-o", c, shuffled_path)
    with sb.Context(0) as ctx:
        bam, bai = sb.sort_bam(shuffled_path, index=True, ctx=ctx)
        filtered = sb.view_bam(shuffled_path, sort="coordinate", flag_exclude=0x10, rows=range(100, 1900), level=-1,
                               ctx=ctx)
    assert read(a) == bam and read(b) == bam and read(c) == filtered
    assert read(a + ".bai") == bai and read(b + ".bai") == bai and bai[:4] == b"BAI\1"


def test_sort_needs_an_output_path(shuffled_path):
    r = subprocess.run([CLI, "sort", shuffled_path], capture_output=True, timeout=300)
    assert r.returncode != 0 and b"usage" in r.stderr and r.stdout == b""
    r = subprocess.run([CLI, "view", "--sort", shuffled_path], capture_output=True, timeout=300)
    assert r.returncode != 0 and b"-b" in r.stderr and r.stdout == b""
