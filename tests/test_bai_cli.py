"""`spark-bam index-bai` and `htsjdk-rewrite --index-bai` (cli/spark_bam.cpp) on the GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_bam
from pkg import sb

CLI = os.path.join(ROOT, "cli", "spark-bam")


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.mark.gpu
def test_index_bai_writes_what_build_bai_returns(tmp_path):
    out = str(tmp_path / "2.bai")
    run("index-bai", golden_bam("2.bam"), out)
    with open(out, "rb") as f:
        got = f.read()
    assert got == sb.build_bai(golden_bam("2.bam"))


@pytest.mark.gpu
def test_index_bai_default_output_path(tmp_path):
    bam = str(tmp_path / "x.bam")
    with open(golden_bam("2.bam"), "rb") as f, open(bam, "wb") as g:
        g.write(f.read())
    run("index-bai", bam)
    assert len(sb.read_bai(bam + ".bai").references) == 84


@pytest.mark.gpu
def test_rewrite_with_index_answers_interval_queries_like_the_original(tmp_path):
    out = str(tmp_path / "rewritten.bam")
    run("htsjdk-rewrite", "--index-bai", golden_bam("2.bam"), out)
    idx = sb.read_bai(out + ".bai")
    assert len(idx.references) == 84 and idx.references[0].metadata.num_mapped == 2450
    with sb.Context(0) as ctx:
        for text in ("1:0-100000", "1:13000-14000,1:60000-61000", "1:2000000-3000000"):
            want = sb.load_bam_intervals(golden_bam("2.bam"), text, ctx=ctx).reads.cols
            got = sb.load_bam_intervals(out, text, ctx=ctx).reads.cols  # (reads rewritten.bam.bai)
            for k in ("ref_id", "pos", "name_off", "names", "flag"):
                assert np.array_equal(got[k], want[k]), (text, k)
            assert want["pos"].size == {"1:0-100000": 2450, "1:2000000-3000000": 0}.get(text, 129)
