"""`spark-bam sort -N` and `spark-bam view -b --sort-name` (cli/spark_bam.cpp) against
api.sort_bam(order="name") / api.view_bam(sort="name") on 2.bam with its records shuffled, and the
refusal of `--index-bai` in name order."""
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
    p = tmp_path_factory.mktemp("name_cli") / "shuffled.bam"
    p.write_bytes(shuffled()[0])
    return str(p)


def test_sort_n_and_view_sort_name_equal_the_python_calls(tmp_path, shuffled_path):
    a, b, c = (str(tmp_path / n) for n in ("a.bam", "b.bam", "c.bam"))
    run("sort", "-N", "-o", a, shuffled_path)
    run("view", "-b", "--sort-name", "-o", b, shuffled_path)
    run("view", "-b", "--sort-name", "-F", "0x10", "-r", "100-1900", "--level", "-1", "-o", c, shuffled_path)
    with sb.Context(0) as ctx:
        bam = sb.sort_bam(shuffled_path, order="name", ctx=ctx)
        filtered = sb.view_bam(shuffled_path, sort="name", flag_exclude=0x10, rows=range(100, 1900), level=-1, ctx=ctx)
    assert read(a) == bam and read(b) == bam and read(c) == filtered and bam != filtered


def test_name_order_with_index_bai_is_refused(tmp_path, shuffled_path):
    out = str(tmp_path / "x.bam")
    for args in (("sort", "-N", "--index-bai", "-o", out, shuffled_path),
                 ("view", "-b", "--sort-name", "--index-bai", "-o", out, shuffled_path)):
        r = subprocess.run([CLI, *args], capture_output=True, timeout=300)
        assert r.returncode != 0 and b"coordinate order" in r.stderr and r.stdout == b""
        assert not os.path.exists(out) and not os.path.exists(out + ".bai")
    r = subprocess.run([CLI, "view", "-b", "--sort", "--sort-name", "-o", out, shuffled_path], capture_output=True, timeout=300)
    assert r.returncode != 0 and b"not both" in r.stderr
