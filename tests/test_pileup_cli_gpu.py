"""`spark-bam pileup` and `spark-bam consensus` (cli/spark_bam.cpp) on 2.bam against api.pileup's two
renderers, byte for byte, and against the numpy restatement of pileup_corpus.py; the refusal of
spans that do not fit the budget."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT, golden_bam
from pkg import sb
import pileup_corpus as pc
from test_depth_gpu import fixture
from test_pileup_gpu import fixture_want

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "cli", "spark-bam")
BAM = golden_bam("2.bam")
pm = sys.modules[sb.__name__ + ".pileup"]  # (sb.pileup is the function)


def run(cmd, *args):
    r = subprocess.run([CLI, cmd, *args], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def region():
    _, _, _, names, _, _ = fixture("2.bam")
    _, (lo, hi) = fixture_want("2.bam")
    return "%s:%d-%d" % (names[0], lo + 1, hi)


def test_pileup_equals_the_python_renderer_and_the_restatement(tmp_path, region):
    _, flat, starts, names, lens, _ = fixture("2.bam")
    want, (lo, hi) = fixture_want("2.bam")
    spans = [(0, lo, hi)]
    with sb.Context(0) as ctx:
        part = sb.pileup(BAM, region=region, ctx=ctx)
        q13 = sb.pileup(BAM, region=region, flag_exclude=0, min_mapq=30, min_baseq=13, ctx=ctx)
    out = run("pileup", "-r", region, BAM)
    assert out == part.text() == pm.pileup_text(want["intervals"], spans, lambda k: want["counts"], names)
    assert out.count(b"\n") == want["stats"]["nonzero"]
    out = run("pileup", "-a", "-H", "-r", region, BAM)
    assert out == part.text(all_positions=True, header=True) and out.count(b"\n") == hi - lo + 1
    assert out.startswith(b"#chrom\tpos\tA\tC\tG\tT\tN\tdel\tins\tlowq\n%s\t%d\t0\t" % (names[0].encode(), lo + 1))
    # other filters and a base-quality threshold, into a file
    w13 = pc.restate(flat, starts, spans, len(lens), {"flag_exclude": 0, "min_mapq": 30}, 13)
    path = str(tmp_path / "pileup.txt")
    assert run("pileup", "-F", "0", "-q", "30", "-Q", "13", "-r", region, "-o", path, BAM) == b""
    with open(path, "rb") as f:
        assert f.read() == q13.text() == pm.pileup_text(w13["intervals"], spans, lambda k: w13["counts"], names)


def test_consensus_equals_the_python_renderer_and_the_restatement(region):
    _, flat, starts, names, lens, _ = fixture("2.bam")
    want, (lo, hi) = fixture_want("2.bam")
    spans = [(0, lo, hi)]
    w = pc.restate(flat, starts, spans, len(lens), {"flag_exclude": 0x704}, 13, 3, 90)
    with sb.Context(0) as ctx:
        plain = sb.pileup(BAM, region=region, ctx=ctx)
        strict = sb.pileup(BAM, region=region, min_baseq=13, min_depth=3, call_pct=90, ctx=ctx)
    assert run("consensus", "-r", region, BAM) == plain.consensus() == pm.consensus_fasta(spans, lambda k: want["calls"], names, lens)
    out = run("consensus", "-Q", "13", "-d", "3", "-c", "90", "-r", region, BAM)
    assert out == strict.consensus() == pm.consensus_fasta(spans, lambda k: w["calls"], names, lens)
    assert out.startswith(b">%s:%d-%d\n" % (names[0].encode(), lo + 1, hi))
    assert all(len(line) <= 60 for line in out.split(b"\n")[1:])


def test_spans_over_the_budget_are_refused(region):
    _, (lo, hi) = fixture_want("2.bam")
    for cmd in ("pileup", "consensus"):
        r = subprocess.run([CLI, cmd, "-r", region, "--max-positions", str(hi - lo - 1), BAM], capture_output=True, timeout=300)
        assert r.returncode != 0 and b"-r" in r.stderr and b"budget" in r.stderr and r.stdout == b""
    assert run("pileup", "-r", region, "--max-positions", str(hi - lo), BAM).count(b"\n") > 0


def test_bad_arguments():
    for bad in ("no_such_reference", "1:10-5", "1:5"):
        r = subprocess.run([CLI, "pileup", "-r", bad, BAM], capture_output=True, timeout=300)
        assert r.returncode != 0 and b"region" in r.stderr and r.stdout == b""
    for args in (("pileup", "-Q", "256"), ("consensus", "-c", "0"), ("consensus", "-d", "0"), ("pileup", "-d", "2"),
                 ("consensus", "-a")):
        r = subprocess.run([CLI, *args, "-r", "1:1-100", BAM], capture_output=True, timeout=300)
        assert r.returncode != 0 and r.stdout == b"", args
    r = subprocess.run([CLI, "pileup"], capture_output=True, timeout=300)
    assert r.returncode != 0 and b"missing BAM path" in r.stderr
