"""`spark-bam depth` (cli/spark_bam.cpp) on 2.bam against api.depth's two renderers, byte for byte,
and against the numpy restatement of depth_corpus.py."""
import os
import subprocess

import pytest

from conftest import ROOT, golden_bam
from pkg import sb
from test_depth_gpu import fixture, fixture_want

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "cli", "spark-bam")
BAM = golden_bam("2.bam")


def run(*args):
    r = subprocess.run([CLI, "depth", *args], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def region():
    _, _, _, names, _, _ = fixture("2.bam")
    _, _, (lo, hi) = fixture_want("2.bam")
    return "%s:%d-%d" % (names[0], lo + 1, hi)


def test_depth_equals_the_python_renderers_and_the_restatement(tmp_path, region):
    _, _, _, names, _, _ = fixture("2.bam")
    want, whole, (lo, hi) = fixture_want("2.bam")
    with sb.Context(0) as ctx:
        every = sb.depth(BAM, ctx=ctx)
        part = sb.depth(BAM, region=region, ctx=ctx)
        with_del = sb.depth(BAM, region=region, count_del=True, ctx=ctx)
        q30 = sb.depth(BAM, region=region, flag_exclude=0, min_mapq=30, ctx=ctx)
    # every reference: samtools depth's lines, and genomecov -bg's
    assert run(BAM) == every.text() == sb.depth_text(whole, names)
    assert run("--bedgraph", BAM) == every.bedgraph() == sb.depth_bedgraph(whole, names)
    # a stretch of reference 0 with every position
    out = run("-a", "-r", region, BAM)
    assert out == part.text(all_positions=True) == sb.depth_text(want["runs"], names, all_positions=True)
    assert out.count(b"\n") == hi - lo
    assert run("-r", region, "--bedgraph", BAM) == part.bedgraph() == sb.depth_bedgraph(want["runs"], names)
    # -J, against the restatement with deletions counted
    wj, _, _ = fixture_want("2.bam", True)
    assert run("-J", "-r", region, BAM) == with_del.text() == sb.depth_text(wj["runs"], names)
    # other filters, into a file
    wq, _, _ = fixture_want("2.bam", False, 0, 30)
    path = str(tmp_path / "depth.txt")
    assert run("-F", "0", "-q", "30", "-r", region, "-o", path, BAM) == b""
    with open(path, "rb") as f:
        assert f.read() == q30.text() == sb.depth_text(wq["runs"], names)
    # a whole reference by name
    assert run("-r", names[0], BAM) == every.text()


def test_a_bad_region_is_an_argument_error():
    for bad in ("no_such_reference", "no_such_reference:1-5", "1:10-5", "1:0-5", "1:5"):
        r = subprocess.run([CLI, "depth", "-r", bad, BAM], capture_output=True, timeout=300)
        assert r.returncode != 0 and b"region" in r.stderr and r.stdout == b""
    r = subprocess.run([CLI, "depth"], capture_output=True, timeout=300)
    assert r.returncode != 0 and b"missing BAM path" in r.stderr
