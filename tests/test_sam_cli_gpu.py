"""`spark-bam view` (cli/spark_bam.cpp) and api.view on the GPU against the reference's SAM text of
2.bam (tests/golden/sam/2.sam.gz: 90 header lines + 2500 records, 1 819 886 bytes)."""
import gzip
import io
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT, golden_bam
from pkg import sb
import sam_corpus as sc

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "cli", "spark-bam")


@pytest.fixture(scope="module")
def want():
    with gzip.open(os.path.join(GOLDEN, "sam", "2.sam.gz")) as f:
        raw = f.read()
    assert len(raw) == 1819886
    return raw


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_view_with_header(want):
    assert run("view", "-h", golden_bam("2.bam")) == want
    assert run("view", "--header", golden_bam("2.bam")) == want


def test_view_records_only(want):
    header, lines = sc.fixture_lines()
    assert header + b"".join(lines) == want
    assert run("view", golden_bam("2.bam")) == b"".join(lines)


def test_view_output_file(want, tmp_path):
    out = str(tmp_path / "2.sam")
    assert run("view", "-h", "-o", out, golden_bam("2.bam")) == b""
    with open(out, "rb") as f:
        assert f.read() == want


def test_api_view(want):
    with sb.Context(0) as ctx:
        assert sb.view(golden_bam("2.bam"), header=True, ctx=ctx) == want
        _, lines = sc.fixture_lines()
        assert sb.view(golden_bam("2.bam"), ctx=ctx) == b"".join(lines)
        # windows of 150 000 compressed bytes: four of them over the 531 753-byte file
        class Sink(io.BytesIO):
            writes = 0

            def write(self, b):
                self.writes += 1
                return super().write(b)

        sink = Sink()
        n = sb.view(golden_bam("2.bam"), header=True, out=sink, window=150000, ctx=ctx)
        assert sink.getvalue() == want and n == len(want)
        assert sink.writes - 1 >= 3  # (the header, then one write per window)
