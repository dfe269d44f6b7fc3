"""api.fastq and `spark-bam fastq` / `fasta` (cli/spark_bam.cpp) against the restatement of
fastq_corpus.py, byte for byte: one stream, several windows with a halo re-run, the -1 / -2 / -0
split, FASTA, and BGZF-compressed sinks."""
import gzip
import io
import os
import subprocess

import pytest

from conftest import ROOT, golden_bam
from pkg import sb
import fastq_corpus as fc
import walk_spy
from test_record_conformance_gpu import call
from test_tally_cpu import bundled

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "cli", "spark-bam")
F900 = {"flag_exclude": 0x900}
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def walked(path, ctx, halo=None, **kw):
    """sb.fastq(path, ctx=ctx, **kw) and the walk it made (walk_spy.walked; fastq reads no header of
    its own, so one shard comes before the first window)."""
    return walk_spy.walked(sb.fastq, path, ctx, halo=halo, header_shards=1, **kw)


def want_of(name, **kw):
    _, flat, starts, _, _, _ = bundled(name)
    kw.setdefault("filter", F900)
    return fc.restate(flat, starts, **kw)


def parts_of(w):
    """The three parts of a split text."""
    a, b = w["sizes"]["part_bytes"][0], w["sizes"]["part_bytes"][0] + w["sizes"]["part_bytes"][1]
    return w["text"][:a], w["text"][a:b], w["text"][b:]


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_one_stream(ctx):
    bam, want = golden_bam("2.bam"), want_of("2.bam")
    r = call(sb.fastq, bam, ctx=ctx)
    assert r.text == want["text"] and (r.n, r.n_kept) == (2500, want["sizes"]["n_kept"])
    assert r.part_bytes == want["sizes"]["part_bytes"] and r.part_rows == want["sizes"]["part_rows"]
    assert run("fastq", bam) == want["text"]
    # into a file object, with other options; the same through the command
    kw = dict(suffix="never", def_qual=7, filter={"flag_require": 0x40, "flag_exclude": 0x904, "min_mapq": 20})
    w = want_of("2.bam", **kw)
    out = io.BytesIO()
    r = call(sb.fastq, bam, out=out, suffix="never", def_qual=7, flag_require=0x40, flag_exclude=0x904, min_mapq=20, ctx=ctx)
    assert out.getvalue() == w["text"] and r.text is None and r.n_kept == w["sizes"]["n_kept"]
    assert run("fastq", "-n", "-v", "7", "-f", "0x40", "-F", "0x904", "-q", "20", bam) == w["text"]
    assert run("fastq", "-N", "-F", "0", golden_bam("1.bam")) == want_of("1.bam", suffix="always", filter={})["text"]


def test_several_windows_and_a_halo_rerun(ctx):
    path = golden_bam("5k.bam")
    want = want_of("5k.bam")
    many, w_many = walked(path, ctx, window=100000)
    # a first halo of 16 bytes: windows run again (x 4 each time) until the block behind the window
    # and the chain's exit are resident -- and are not written twice
    out = io.BytesIO()
    rerun, w_rerun = walked(path, ctx, halo=16, window=150000, out=out)
    assert len(set(o for o, _ in w_many)) >= 3 and len(w_many) == len(set(o for o, _ in w_many))
    assert len(w_rerun) > len(set(o for o, _ in w_rerun)) >= 3
    assert many.text == want["text"] and out.getvalue() == want["text"]
    for r in (many, rerun):
        assert (r.n, r.n_kept, r.part_bytes) == (4910, want["sizes"]["n_kept"], want["sizes"]["part_bytes"])


def test_split_sinks(ctx, tmp_path):
    bam = golden_bam("1.bam")
    w = want_of("1.bam", split=True)
    p1, p2, p0 = (str(tmp_path / n) for n in ("r1.fq", "r2.fq", "r0.fq"))
    r = call(sb.fastq, bam, out1=p1, out2=p2, out0=p0, ctx=ctx, window=200000)
    assert (read(p1), read(p2), read(p0)) == parts_of(w)
    assert r.part_rows == w["sizes"]["part_rows"] and r.part_bytes == w["sizes"]["part_bytes"] and r.text is None
    assert run("fastq", "-1", p1 + "c", "-2", p2 + "c", "-0", p0 + "c", bam) == b""
    assert (read(p1 + "c"), read(p2 + "c"), read(p0 + "c")) == parts_of(w)
    # a class without a sink goes to `out`, or nowhere
    out = io.BytesIO()
    call(sb.fastq, bam, out=out, out1=p1, ctx=ctx)
    assert read(p1) == parts_of(w)[0] and out.getvalue() == parts_of(w)[1] + parts_of(w)[2]
    assert run("fastq", "-2", p2, bam) == b"" and read(p2) == parts_of(w)[1]
    assert run("fastq", "-2", p2, "-o", p0, bam) == b"" and read(p0) == parts_of(w)[0] + parts_of(w)[2]
    # one sink named twice is opened once
    call(sb.fastq, bam, out1=p1, out2=p1, ctx=ctx)
    assert read(p1) == parts_of(w)[0] + parts_of(w)[1]


def test_fasta(ctx, tmp_path):
    bam = golden_bam("2.bam")
    w = want_of("2.bam", fasta=True)
    assert call(sb.fastq, bam, fasta=True, ctx=ctx).text == w["text"] == run("fasta", bam)
    ws = want_of("2.bam", fasta=True, split=True, suffix="always")
    p1, p2 = str(tmp_path / "a.fa"), str(tmp_path / "b.fa")
    assert run("fasta", "-N", "-1", p1, "-2", p2, "-o", str(tmp_path / "o.fa"), bam) == b""
    assert (read(p1), read(p2), read(str(tmp_path / "o.fa"))) == parts_of(ws)


def test_gz_sinks(ctx, tmp_path):
    """Each compressed file: a multi-member gzip of the plain output that ends with the 28-byte BGZF
    EOF member, the only member of no bytes."""
    bam = golden_bam("5k.bam")
    w, ws = want_of("5k.bam"), want_of("5k.bam", split=True)

    def plain(path):
        data = read(path)
        assert data.endswith(EOF_MEMBER) and data.count(EOF_MEMBER) == 1
        return gzip.decompress(data)

    one = str(tmp_path / "all.fq.gz")
    call(sb.fastq, bam, out=one, ctx=ctx, window=100000)  # members end short at window ends
    assert plain(one) == w["text"]
    paths = [str(tmp_path / n) for n in ("r1.fq.gz", "r2.fq.gz", "r0.fq")]
    call(sb.fastq, bam, out1=paths[0], out2=paths[1], out0=paths[2], ctx=ctx, window=150000)
    assert (plain(paths[0]), plain(paths[1]), read(paths[2])) == parts_of(ws)
    # level given: every sink is compressed, a file object too
    out = io.BytesIO()
    call(sb.fastq, bam, out=out, level=-1, ctx=ctx)
    assert out.getvalue().endswith(EOF_MEMBER) and gzip.decompress(out.getvalue()) == w["text"]
    # the command
    assert run("fastq", "-o", one, bam) == b"" and plain(one) == w["text"]
    assert run("fastq", "-1", paths[0], "-2", paths[1], "-0", paths[2], bam) == b""
    assert (plain(paths[0]), plain(paths[1]), read(paths[2])) == parts_of(ws)
    assert run("fastq", "--level", "6", "-0", paths[2], bam) == b"" and plain(paths[2]) == parts_of(ws)[2]
    # nothing kept: the EOF member alone
    assert run("fastq", "-f", "0x800", "-F", "0", "-o", one, bam) == b"" and read(one) == EOF_MEMBER


def test_usage_errors():
    bam = golden_bam("2.bam")
    for args in (("fastq", "-x", bam), ("fasta", "--bedgraph", bam), ("fastq", "-n", "-N", bam), ("fastq", "-v", "94", bam)):
        r = subprocess.run([CLI, *args], capture_output=True, timeout=300)
        assert r.returncode != 0 and r.stdout == b"" and (b"usage" in r.stderr or b"-v takes" in r.stderr)
    r = subprocess.run([CLI, "fastq"], capture_output=True, timeout=300)
    assert r.returncode != 0 and b"missing BAM path" in r.stderr
    with pytest.raises(ValueError):
        sb.fastq(bam, suffix="sometimes")
