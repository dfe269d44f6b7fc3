"""A context that was given the caller's stream (sbh_ctx_set_stream, Context(stream=...)).

include/sparkbam.h promises that shards created afterwards enqueue on that stream, so that an input
the caller wrote on it before a call is seen by the call, and that every call returns with the stream
drained.  The stream, the device memory and the stream-ordered copies come from hip_rt: the HIP
runtime instance the library itself links.

A.  Input ordering.  A device buffer holds file A.  Behind a closed hip_rt.Gate on the stream S, a
    copy of file B over the buffer is enqueued.  Right before the call under test the gate is
    closed and S answers not-ready, so the copy has not run.  The call must see B: shard create,
    shard load, bgzf_compress (two flat streams in place of the files), and a shard must keep its
    own copy of the bytes it was created from.  A's answer is asserted to differ from B's.  The same
    for sbh_run_stream2's page-locked host input, filled by a copy on S behind the gate.
B.  Results on the caller's stream: flat_ptr(), bam_ptr() and fastq_ptr() copied on S with no
    library call between the stage and the copy.
C.  Equivalence sweep: every stage once on the supplied-stream context at a small corpus, held to
    the reference its own suite uses and to what a context that owns its streams gives.
D.  Lifetime and state: S stays the caller's after the shards and the context are closed; a shard
    from before set_stream keeps its own stream; run_stream before and after set_stream; two
    threads sharing S; work of a call after set_stream is ordered behind S.
E.  Device-pointer input on a context that owns its streams.

After every library call this file makes on the supplied-stream context, hipStreamQuery(S) is
success: on_s for the calls written out here, every_call_drains for the calls the sweep's helpers
make, and an autouse fixture asks once more after each test."""
import contextlib
import functools
from unittest import mock

import numpy as np
import pytest

import bai_ref
import bam_sort_corpus as sc
import depth_corpus as dc
import fastq_corpus as fc
import hip_rt
import oracle_records as orr
import pileup_corpus as pc
import record_corpus as rc
import sam_corpus
import shard_reuse as sr
import stats_corpus
import tally_corpus as tc
import test_bai_gpu as t_bai
import test_depth_gpu as t_depth
import test_fastq_gpu as t_fastq
import test_pileup_gpu as t_pileup
import test_sam_gpu as t_sam
import test_shard_reuse_gpu as t_reuse
import test_stats_gpu as t_stats
import test_tally_gpu as t_tally
from conftest import golden_bam, read_blocks, read_records
from oracle_lib import OR_OK, OracleFile, file_splits
from pkg import sb
from test_bam_sort_gpu import same_as_host, scanned, want_sorted
from test_record_conformance_gpu import call
from test_records_gpu import assert_cols_equal
from test_threads_gpu import _run_threads

pytestmark = pytest.mark.gpu

A_NAME, B_NAME = "shuffled", "reverse_sorted"


# ------------------------------------------------------------------------- fixtures and helpers

@pytest.fixture(scope="module")
def S():
    s = hip_rt.stream_create()
    yield s
    hip_rt.stream_synchronize(s)
    hip_rt.stream_destroy(s)


@pytest.fixture(scope="module")
def sctx(S):
    """The context under test: every shard of it is to run on S."""
    c = sb.Context(0, stream=S)
    yield c
    c.close()


@pytest.fixture(scope="module")
def octx():
    """A context that owns its streams, to compare against."""
    c = sb.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def drained_after_each_test(S):
    yield
    assert hip_rt.stream_ready(S)


def on_s(S, f, *a, **kw):
    """call(f, *a) on the supplied-stream context: it returns with S drained."""
    out = call(f, *a, **kw)
    assert hip_rt.stream_ready(S), getattr(f, "__name__", f)
    return out


@functools.lru_cache(maxsize=None)
def file_of(name):
    """(the BGZF file of the sort corpus' stream, stored members; its flat bytes) as uint8 arrays."""
    s = sc.stream(name)
    return (np.frombuffer(rc.bgzf(s.flat, 65280, 0), np.uint8).copy(), np.frombuffer(bytes(s.flat), np.uint8).copy())


@functools.lru_cache(maxsize=None)
def sorted_want(name):
    s = sc.stream(name)
    return want_sorted(s.flat, s.starts)


def test_the_two_files_cannot_be_told_apart_by_size_only():
    """A and B: the same size, and no row of their coordinate permutations agrees."""
    (fa, ua), (fb, ub) = file_of(A_NAME), file_of(B_NAME)
    assert fa.size == fb.size == 180590 and ua.size == ub.size and not np.array_equal(fa, fb)
    pa, pb = sc.expected_perm(A_NAME), sc.expected_perm(B_NAME)
    assert pa.size == pb.size == 4097 and np.all(pa != pb)
    assert np.array_equal(sorted_want(B_NAME)[2], pb) and not np.array_equal(sorted_want(A_NAME)[0], sorted_want(B_NAME)[0])


class Staged:
    """A device buffer that holds `first`; behind a closed gate on S, a copy of `then` over it."""

    def __init__(self, S, first, then):
        assert first.size == then.size
        self.S, self.n = S, int(first.size)
        self.dev = hip_rt.malloc(self.n)
        self.pin = sb.PinnedBuffer(self.n)
        self.pin_first = sb.PinnedBuffer(self.n)
        self.pin.array[:] = then
        self.pin_first.array[:] = first
        hip_rt.memcpy(self.dev, first, self.n, hip_rt.H2D)
        assert hip_rt.stream_ready(S)
        self.gate = hip_rt.Gate(S)
        hip_rt.memcpy_async(self.dev, self.pin.array, self.n, hip_rt.H2D, S)

    def premise(self):
        """Right before the call under test: the copy behind the gate has not run."""
        assert self.gate.closed() and not hip_rt.stream_ready(self.S)

    def overwrite_with_first(self):
        hip_rt.memcpy_async(self.dev, self.pin_first.array, self.n, hip_rt.H2D, self.S)

    def close(self):
        self.gate.finish()
        hip_rt.free(self.dev)
        self.pin.close()
        self.pin_first.close()


@contextlib.contextmanager
def staged(S, first, then):
    st = Staged(S, first, then)
    try:
        yield st
    finally:
        st.close()


def coordinate_sorted(sh, name):
    """index, inflate, scan, records_bam(order="coordinate") of a shard that holds a sort-corpus file."""
    s = sc.stream(name)
    _, fs = call(sh.index, 0)
    call(sh.inflate)
    assert fs == len(s.flat)
    assert call(sh.records_scan, s.first, fs) == len(s.starts)
    return call(sh.records_bam, b"", None, order="coordinate")


def assert_is_b(got):
    want = sorted_want(B_NAME)
    assert np.array_equal(got[2], sc.expected_perm(B_NAME))
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


# ------------------------------------------------------------------------- A: input ordering

def test_shard_create_sees_the_input_written_on_the_stream(S, sctx):
    fa, fb = file_of(A_NAME)[0], file_of(B_NAME)[0]
    sorted_want(B_NAME)
    with staged(S, fa, fb) as st:
        st.premise()
        sh = call(sctx.shard, st.dev, on_device=True, nbytes=st.n)
        drained = hip_rt.stream_ready(S)
        try:
            assert_is_b(coordinate_sorted(sh, B_NAME))
            assert drained
        finally:
            sh.close()


def test_shard_load_sees_the_input_written_on_the_stream(S, sctx):
    fa, fb = file_of(A_NAME)[0], file_of(B_NAME)[0]
    sorted_want(B_NAME)
    sh = on_s(S, sctx.shard, fa)
    try:
        on_s(S, sh.index, 0)
        with staged(S, fa, fb) as st:
            st.premise()
            call(sh.load, st.dev, 0, on_device=True, nbytes=st.n)
            drained = hip_rt.stream_ready(S)
            assert_is_b(coordinate_sorted(sh, B_NAME))
            assert drained
    finally:
        sh.close()


@pytest.mark.parametrize("level", [5, -1])
def test_bgzf_compress_sees_the_input_written_on_the_stream(S, sctx, octx, level):
    ua, ub = file_of(A_NAME)[1], file_of(B_NAME)[1]
    want = call(octx.bgzf_compress, ub, level=5)[0] if level == 5 else None
    with staged(S, ua, ub) as st:
        st.premise()
        out, nb, _ = call(sctx.bgzf_compress, st.dev, st.n, level)
        drained = hip_rt.stream_ready(S)
    assert nb >= ub.size // 65536
    assert rc.inflate_members(out.tobytes()) == ub.tobytes() != ua.tobytes()
    if want is not None:
        assert np.array_equal(out, want)
    assert drained


def test_the_shard_keeps_a_copy_of_its_input(S, sctx):
    fa, fb = file_of(A_NAME)[0], file_of(B_NAME)[0]
    sorted_want(B_NAME)
    with staged(S, fa, fb) as st:
        st.premise()
        sh = call(sctx.shard, st.dev, on_device=True, nbytes=st.n)
        try:
            st.overwrite_with_first()  # the caller reuses its buffer, on its stream
            assert_is_b(coordinate_sorted(sh, B_NAME))
            got = np.empty(st.n, np.uint8)
            hip_rt.stream_synchronize(S)
            hip_rt.memcpy(got, st.dev, st.n, hip_rt.D2H)
            assert np.array_equal(got, fa)  # (the overwrite did run)
        finally:
            sh.close()


@pytest.mark.parametrize("cache", ["from_before_set_stream", "from_after_set_stream"])
def test_run_stream_sees_host_input_written_on_the_stream(S, octx, cache):
    """sbh_run_stream2 reads page-locked host bytes with copies on a stream of its window cache.
    Behind the gate, a device-to-host copy on S fills those bytes with 2.bam; until then they are
    zeros, which run_stream refuses.  The context has streamed a file already, so the call takes an
    idle window cache and creates no shard: one made before set_stream (let go by set_stream, or the
    call would wait on that shard's own stream and read zeros) or one made after it."""
    data, of = two_bam()
    want = of.eager_range(0, of.flat_size)
    dev = hip_rt.malloc(data.size)
    pin = sb.PinnedBuffer(data.size)
    kw = dict(index_start=0, window=data.size // 5, halo=1 << 16)
    c = sb.Context(0)
    try:
        hip_rt.memcpy(dev, data, data.size, hip_rt.H2D)
        if cache == "from_before_set_stream":
            streamed(c)
        assert sb.lib().sbh_ctx_set_stream(c.h, S) == 0
        if cache == "from_after_set_stream":
            streamed(c)
        pin.array[:] = 0
        with pytest.raises(sb.SparkBamError):  # (what the bytes give before the copy)
            call(octx.run_stream, pin.array, of.contig_len, **kw)
        gate = hip_rt.Gate(S)
        try:
            hip_rt.memcpy_async(pin.array, dev, data.size, hip_rt.D2H, S)
            assert gate.closed() and not hip_rt.stream_ready(S)
            r, bits = call(c.run_stream, pin.array, of.contig_len, want_bits=True, **kw)
            drained = hip_rt.stream_ready(S)
        finally:
            gate.finish()
        assert r["status"] == 0 and r["host_pinned"] == 1 and r["n_windows"] >= 3
        assert r["count"] == 2500 and r["n_true"] == want[0] and np.array_equal(bits, want[1])
        assert drained
    finally:
        c.close()
        hip_rt.stream_synchronize(S)
        hip_rt.free(dev)
        pin.close()


# ------------------------------------------------------------------------- B: results on the stream

def test_results_are_visible_to_work_on_the_stream(S, sctx):
    """After inflate, a scan, records_bam and records_fastq: the three device results copied on S,
    no library call between the stages and the copies."""
    s = sc.stream(A_NAME)
    flat = file_of(A_NAME)[1]
    sh = on_s(S, sctx.shard, file_of(A_NAME)[0])
    pins = []
    try:
        on_s(S, sh.index, 0)
        on_s(S, sh.inflate)
        assert on_s(S, sh.records_scan, s.first, sh.flat_size) == len(s.starts)
        assert on_s(S, sh.records_bam, b"", None, want_bytes=False, order="coordinate") is None
        assert on_s(S, sh.records_fastq, want_text=False) is None
        srcs = ((sh.flat_ptr(), sh.flat_size), (sh.bam_ptr(), sh.bam_size), (sh.fastq_ptr(), sh.fastq_sizes["text_bytes"]))
        for p, n in srcs:
            assert p and n
            pins.append(sb.PinnedBuffer(n))
            hip_rt.memcpy_async(pins[-1].array, p, n, hip_rt.D2H, S)
        hip_rt.stream_synchronize(S)
        got = [p.array.copy() for p in pins]
        assert np.array_equal(got[0], flat) and np.array_equal(got[0], on_s(S, sh.read_flat))
        assert np.array_equal(got[1], sorted_want(A_NAME)[0]) and np.array_equal(got[1], on_s(S, sh.bam_read, 0, sh.bam_size))
        text = sb.fastq_host(flat, s.starts)[0]
        assert np.array_equal(got[2], text) and np.array_equal(got[2], on_s(S, sh.records_fastq)[0])
    finally:
        sh.close()
        for p in pins:
            p.close()


# ------------------------------------------------------------------------- C: the equivalence sweep

_OWN = {}


@contextlib.contextmanager
def every_call_drains(S, ctx):
    """Inside the block, every library call the Python layer makes on `ctx`, its shards and its
    accumulators (device._check sees each status) is followed by hipStreamQuery(S) == success."""
    real = sb.device._check

    def check(handle, rc):
        real(handle, rc)
        if getattr(handle, "value", handle) == ctx.h.value:
            assert hip_rt.stream_ready(S), "a call returned with work pending on the caller's stream"

    with mock.patch.object(sb.device, "_check", check):
        yield


def both(key, stage, S, sctx, octx):
    """stage(ctx) on the supplied-stream context, held to the own-stream context's result (computed
    once and left unchanged); the stage itself holds what it returns to its reference."""
    with every_call_drains(S, sctx):
        got = stage(sctx)
    assert hip_rt.stream_ready(S)
    if key not in _OWN:
        _OWN[key] = stage(octx)
    assert sr.same(got, _OWN[key]), key
    return got


@functools.lru_cache(maxsize=None)
def two_bam():
    data = np.fromfile(golden_bam("2.bam"), dtype=np.uint8)
    return data, OracleFile(data)


def vpos(of, flat):
    bp, off = of.pos_of(int(flat))
    return bp << 16 | off


def two_bam_steps(ctx):
    """index, inflate, check_eager, find_record_start and split_starts on 2.bam, against the oracle."""
    data, of = two_bam()
    sh = ctx.shard(data)
    try:
        out = {"index": call(sh.index, 0)}
        assert out["index"] == (len(of.blocks) + 1, of.flat_size)
        call(sh.inflate)
        out["flat"] = call(sh.read_flat)
        assert np.array_equal(out["flat"], of.uncompressed())
        call(sh.set_contigs, of.contig_len)
        out["eager"] = call(sh.check_eager, 0, sh.flat_size)
        n_ref, bits_ref = of.eager_range(0, of.flat_size)
        assert out["eager"][0] == n_ref == 2500 and np.array_equal(out["eager"][1], bits_ref)
        out["find_record_start"] = call(sh.find_record_start, 0)
        assert (OR_OK,) + out["find_record_start"] == of.find_record_start(0)
        splits = file_splits(data.size, 100 * 1024)
        status, v, c, _ = call(sh.split_starts, splits)
        out["split_starts"] = (status, np.where(c > 0, v, 0), c)
        for k, (a, e) in enumerate(splits):
            code, want_v, want_n = of.split(a, e)
            assert code == OR_OK and status[k] == 0 and int(c[k]) == want_n and (want_n == 0 or int(v[k]) == want_v), k
        assert int(c.sum()) == 2500
        return out
    finally:
        sh.close()


def two_bam_run(ctx):
    """sbh_run_shard on 2.bam, against the oracle."""
    data, of = two_bam()
    sh = ctx.shard(data)
    try:
        call(sh.set_contigs, of.contig_len)
        r = call(sh.run, 0, data.size)
        n_ref, bits_ref = of.eager_range(0, of.flat_size)
        assert r["status"] == 0 and (r["n_blocks"], r["flat_bytes"]) == (len(of.blocks) + 1, of.flat_size)
        assert r["comp_bytes"] == data.size and r["n_true"] == n_ref and r["count"] == 2500
        assert r["first_vpos"] == vpos(of, of.header_end) and r["exit_flat"] == of.flat_size
        bits = call(sh.eager_bits, 0, r["flat_bytes"])
        assert np.array_equal(bits, bits_ref)
        return r, bits
    finally:
        sh.close()


def two_bam_split_records(ctx):
    """sbh_split_records per split and sbh_split_records_batch over all of them on 2.bam: the
    oracle's first record and count per split, the oracle's decode of the rows."""
    data, of = two_bam()
    splits = file_splits(data.size, 100 * 1024)
    flat = of.uncompressed().tobytes()
    want = []
    for a, e in splits:
        code, v, n = of.split(a, e)
        assert code == OR_OK
        chain = [int(f) for f in of.record_chain(of.flat_of(v >> 16, v & 0xffff))[:n]] if n else []
        want.append((v, n, chain))
    out = []
    sh = ctx.shard(data)
    try:
        call(sh.set_contigs, of.contig_len)
        for (a, e), (v, n, chain) in zip(splits, want):
            call(sh.load, data, 0)
            info, cols = call(sh.split_records, a, e)
            assert info["n"] == n and (n == 0 or info["first_vpos"] == v)
            assert cols["vpos"].tolist() == [vpos(of, f) for f in chain]
            dec = orr.decode(flat, chain)
            assert_cols_equal({k: x for k, x in cols.items() if k not in ("flat", "vpos")},
                              {k: x for k, x in dec.items() if k != "flat"})
            assert np.all(dec["flat"] - cols["flat"] == (dec["flat"][0] - cols["flat"][0] if n else 0))
            out.append((info["n"], info["first_vpos"] if n else 0, cols))
        call(sh.load, data, 0)
        info, per, cols = call(sh.split_records_batch, splits)
        rows = [f for _, _, chain in want for f in chain]
        assert [(p["status"], p["rec_count"]) for p in per] == [(0, n) for _, n, _ in want]
        assert [p["first_vpos"] for p, (v, n, _) in zip(per, want) if n] == [v for v, n, _ in want if n]
        assert cols["vpos"].tolist() == [vpos(of, f) for f in rows]
        assert_cols_equal({k: x for k, x in cols.items() if k != "flat"},
                          {k: x for k, x in orr.decode(flat, rows).items() if k != "flat"})
        out.append(([(p["status"], p["rec_begin"], p["rec_count"]) for p in per], cols))
        return out
    finally:
        sh.close()


def records_and_text(ctx):
    """The record columns and the SAM text of sam_corpus' stream: the oracle's decode, the host renderer."""
    s = sam_corpus.stream()
    sh = t_sam.open_stream(ctx, s.flat)
    try:
        cols = call(sh.records, s.first, sh.flat_size)
        assert cols["flat"].tolist() == s.starts
        assert_cols_equal(cols, orr.decode(s.flat, s.starts))
        text, off = call(sh.records_sam, sam_corpus.REF_NAMES)
        want_text, want_off = t_sam.corpus_want()
        assert sh.sam_n_host == len(sam_corpus.FLOAT_ROWS)
        assert np.array_equal(off, want_off) and np.array_equal(text, want_text)
        return cols, text, off
    finally:
        sh.close()


def bam_streams(ctx):
    """records_bam in scan order and in coordinate order on edge_2049 (a tile and one row more)."""
    s = sc.stream("edge_%d" % (sc.SORT_TILE + 1))
    sh = scanned(ctx, s)
    try:
        plain = call(sh.records_bam, rc.header())
        want = sb.bam_gather_host(s.flat, s.starts, rc.header())
        for a, b in zip(plain, want):
            assert np.array_equal(a, b)
        coord = same_as_host(sh, s.flat, s.starts, rc.header())
        assert np.array_equal(coord[2], sc.expected_perm("edge_%d" % (sc.SORT_TILE + 1)))
        return plain, coord
    finally:
        sh.close()


def smallest(corpus, names):
    """The suite's smallest corpus, rows in file order, that has more rows than one wave (one row
    would say nothing about a row kernel); the largest one where none has."""
    ok = [k for k in names if corpus.get(k).starts and list(corpus.get(k).starts) == sorted(set(corpus.get(k).starts))]
    size = lambda k: (len(corpus.get(k).starts), len(corpus.get(k).flat))  # noqa: E731
    wide = [k for k in ok if len(corpus.get(k).starts) > 64]
    return min(wide, key=size) if wide else max(ok, key=size)


def fastq_text(ctx):
    name = smallest(fc, fc.SMALL)
    c = fc.get(name)
    sh = t_fastq.scanned(ctx, c)
    try:
        out = []
        for v, kw in enumerate(fc.VARIANTS[name]):
            t_fastq.device_equals(sh, c, fc.expected(name, v), **kw)
            out.append(call(sh.records_fastq, **kw))
        return out
    finally:
        sh.close()


def bai_index(ctx):
    """bai_scan over 2.bam and the built index: bai_ref's, and samtools' golden file."""
    data = two_bam()[0].tobytes()
    want = t_bai.check_all(ctx, data)
    with open(golden_bam("2.bam") + ".bai", "rb") as f:
        assert bai_ref.parsed(want.bytes) == bai_ref.parsed(f.read())
    return t_bai.scan(ctx, data), sb.build_bai(data, ctx=ctx)


def depth_stage(ctx):
    name = smallest(dc, dc.SMALL)
    c, want = dc.get(name), dc.expected(name)
    sh = t_depth.scanned(ctx, c.flat, c.starts[0], len(c.starts))
    acc = ctx.depth(c.spans, dc.N_REF, c.count_del)
    try:
        add = call(acc.add, sh, c.filter)
        assert add == want["add"]
        sizes = t_depth.finished_equals(acc, want, c.spans)
        return add, sizes, call(acc.runs), [call(acc.depth, k) for k in range(len(c.spans))]
    finally:
        acc.close()
        sh.close()


def pileup_stage(ctx):
    name = smallest(pc, pc.SMALL)
    c, want = pc.get(name), pc.expected(name)
    sh = t_depth.scanned(ctx, c.flat, c.starts[0], len(c.starts))
    acc = ctx.pileup(c.spans, pc.N_REF, c.min_baseq)
    try:
        add = call(acc.add, sh, c.filter)
        assert add == want["add"]
        sizes = t_pileup.finished_equals(acc, want, c.spans, c.min_depth, c.call_pct)
        k = range(len(c.spans))
        return add, sizes, call(acc.intervals), [call(acc.counts, i) for i in k], [call(acc.calls, i) for i in k]
    finally:
        acc.close()
        sh.close()


def stats_stage(ctx):
    name = smallest(stats_corpus, stats_corpus.SMALL)
    c, want = stats_corpus.get(name), stats_corpus.expected(name)
    sh = t_depth.scanned(ctx, c.flat, c.starts[0], len(c.starts), level=1)
    acc = ctx.stats(c.cycles, c.max_insert)
    try:
        add = call(acc.add, sh, c.filter)
        assert add == t_stats.added(want)
        t_stats.counts_equal(acc, want)
        return add, call(acc.counts)
    finally:
        acc.close()
        sh.close()


def tally_stage(ctx):
    name = smallest(tc, tc.SMALL)
    c, want = tc.get(name), tc.expected(name)
    sh = t_depth.scanned(ctx, c.flat, c.starts[0], len(c.starts))
    acc = ctx.tally(c.n_ref)
    try:
        add = call(acc.add, sh, c.filter)
        assert add == t_tally.added(want)
        t_tally.counts_equal(acc, want)
        return add, call(acc.counts)
    finally:
        acc.close()
        sh.close()


def compress_from_host(ctx):
    """bgzf_compress from host memory at levels 0, 5 and -1: zlib reads the input back."""
    u = file_of(A_NAME)[1]
    out = []
    for level in (0, 5, -1):
        data, nb, _ = call(ctx.bgzf_compress, u, level=level)
        assert nb >= u.size // 65536 and rc.inflate_members(data.tobytes()) == u.tobytes(), level
        out.append(data)
    return out


STREAM_KEYS = ("n_windows", "n_blocks", "comp_bytes", "flat_bytes", "n_true", "count", "first_vpos", "exit_vpos", "status",
               "crc_bad_blocks")


def streamed(ctx):
    """sbh_run_stream2 over 2.bam in windows of a fifth of the file, with splits and the CRC check:
    the oracle's bits, counts and per-split answers."""
    data, of = two_bam()
    splits = file_splits(data.size, 100 * 1024)
    s, bits = call(ctx.run_stream, data, of.contig_len, index_start=0, window=data.size // 5, halo=1 << 16,
                   want_bits=True, splits=splits, verify_crc=True)
    n_ref, bits_ref = of.eager_range(0, of.flat_size)
    assert s["status"] == 0 and s["n_windows"] >= 3 and s["crc_bad_blocks"] == 0
    assert s["flat_bytes"] == of.flat_size and s["comp_bytes"] == data.size
    assert s["n_true"] == n_ref and s["count"] == 2500 and s["first_vpos"] == vpos(of, of.header_end)
    assert np.array_equal(bits, bits_ref)
    for k, (a, e) in enumerate(splits):
        code, v, n = of.split(a, e)
        assert code == OR_OK and s["split_status"][k] == 0 and int(s["split_count"][k]) == n, k
        assert n == 0 or int(s["split_first_vpos"][k]) == v, k
    return ({k: s[k] for k in STREAM_KEYS}, bits, s["split_status"], s["split_count"],
            np.where(s["split_count"] > 0, s["split_first_vpos"], 0))


def blocks_and_all_positions(ctx):
    """sbh_find_blocks and sbh_check_stream over 2.bam in windows: the `.blocks` file, the `.records`
    truth (every record found, nothing else called) and the oracle's eager bits."""
    data, of = two_bam()
    splits = [(a, min(a + 65536, data.size)) for a in range(0, data.size, 65536)]
    found = call(ctx.find_blocks, data, splits, window=150000)
    assert [b[1:] for b in found] == read_blocks("2.bam")
    truth = np.sort(np.asarray([(b << 16) | o for b, o in read_records("2.bam")], dtype=np.uint64))
    r = call(ctx.check_stream, data, of.contig_len, [b[1] for b in found], truth_vpos=truth, window=150000)
    n_ref, _ = of.eager_range(0, of.flat_size)
    assert r["n_windows"] >= 3 and r["positions"] == of.flat_size and r["n_true"] == n_ref
    assert (r["tp"], r["fp"], r["fn"], r["unknown"]) == (2500, n_ref - 2500, 0, 0)
    keys = ("n_windows", "positions", "comp_bytes", "n_true", "tp", "fp", "fn", "unknown")
    return found, {k: r[k] for k in keys}, r["fp_vpos"], r["fn_vpos"]


SWEEP = {"2bam_steps": two_bam_steps, "2bam_run": two_bam_run, "2bam_split_records": two_bam_split_records,
         "records_and_sam": records_and_text, "bam_scan_and_coordinate": bam_streams, "fastq": fastq_text,
         "bai": bai_index, "depth": depth_stage, "pileup": pileup_stage, "stats": stats_stage, "tally": tally_stage,
         "bgzf_compress_host": compress_from_host, "run_stream": streamed, "find_blocks_check_stream": blocks_and_all_positions}


@pytest.mark.parametrize("stage", list(SWEEP))
def test_sweep(S, sctx, octx, stage):
    both(stage, SWEEP[stage], S, sctx, octx)


@pytest.mark.parametrize("path", ["steps", "run"])
def test_sweep_stage_tour(S, sctx, octx, path):
    """shard_reuse's tour of every stage over MID (257 records, two references, long CIGARs, a record
    ending on a member's last byte), against the host's answers and the own-stream context's tour."""
    sh = t_reuse.shard_for(sctx, "MID")
    try:
        with every_call_drains(S, sctx):
            got = sr.tour(sh, sctx, "MID", path, sr.offset_of("MID"))
    finally:
        sh.close()
    assert hip_rt.stream_ready(S)
    t_reuse.assert_tour(got, "MID", path, "supplied stream")
    assert sr.differing(got, t_reuse.fresh_tour(octx, "MID", path)) == []


# ------------------------------------------------------------------------- D: lifetime and state

def eager_of_two_bam(ctx):
    data, of = two_bam()
    sh = ctx.shard(data)
    try:
        call(sh.index, 0)
        call(sh.inflate)
        call(sh.set_contigs, of.contig_len)
        return call(sh.check_eager, 0, sh.flat_size)
    finally:
        sh.close()


def test_the_stream_stays_the_callers_after_everything_is_closed():
    data, of = two_bam()
    want = of.eager_range(0, of.flat_size)
    s2 = hip_rt.stream_create()
    dev = hip_rt.malloc(data.size)
    pin, back = sb.PinnedBuffer(data.size), sb.PinnedBuffer(data.size)
    try:
        c = sb.Context(0, stream=s2)
        n, bits = eager_of_two_bam(c)
        assert n == want[0] and np.array_equal(bits, want[1])
        r, _ = call(c.run_stream, data, of.contig_len, index_start=0, window=data.size // 3)
        assert r["count"] == 2500
        sh = c.shard(data)  # (closed with the context)
        call(sh.index, 0)
        c.close()
        assert sh.h is None
        assert hip_rt.stream_ready(s2)
        pin.array[:] = data
        back.array[:] = 0
        hip_rt.memcpy_async(dev, pin.array, data.size, hip_rt.H2D, s2)
        hip_rt.memcpy_async(back.array, dev, data.size, hip_rt.D2H, s2)
        hip_rt.stream_synchronize(s2)
        assert np.array_equal(back.array, data) and hip_rt.stream_ready(s2)
    finally:
        hip_rt.stream_synchronize(s2)
        hip_rt.free(dev)
        pin.close()
        back.close()
        hip_rt.stream_destroy(s2)  # (still a stream: the destroy succeeds)


def test_a_shard_from_before_set_stream_keeps_its_own_stream(S):
    data, of = two_bam()
    want = of.eager_range(0, of.flat_size)
    with sb.Context(0) as c:
        old = c.shard(data)
        call(old.index, 0)
        assert sb.lib().sbh_ctx_set_stream(c.h, S) == 0
        call(old.inflate)
        call(old.set_contigs, of.contig_len)
        n, bits = call(old.check_eager, 0, old.flat_size)
        assert n == want[0] and np.array_equal(bits, want[1])
        n, bits = eager_of_two_bam(c)  # a shard from after the call, on S
        assert hip_rt.stream_ready(S) and n == want[0] and np.array_equal(bits, want[1])
        old.close()
        assert hip_rt.stream_ready(S)


def test_run_stream_before_and_after_set_stream(S):
    with sb.Context(0) as c:
        before = streamed(c)
        assert sb.lib().sbh_ctx_set_stream(c.h, S) == 0
        after = streamed(c)
        assert hip_rt.stream_ready(S)
        assert sr.same(before, after)


@pytest.mark.parametrize("what", ["run_stream", "bgzf_compress"])
def test_a_context_call_after_set_stream_is_ordered_behind_the_stream(S, what):
    """"Every call returns with the stream drained", with work of the caller's still pending on S: a
    closed gate on S, then one context-level call.  When the call returns the gate's host function
    has run -- exactly, whatever the call's duration -- and S answers ready."""
    data, of = two_bam()
    with sb.Context(0) as c:
        streamed(c)
        assert sb.lib().sbh_ctx_set_stream(c.h, S) == 0
        gate = hip_rt.Gate(S)
        try:
            assert gate.closed() and not hip_rt.stream_ready(S)
            if what == "run_stream":
                r, _ = call(c.run_stream, data, of.contig_len, index_start=0, window=data.size // 3)
                assert r["count"] == 2500
            else:
                call(c.bgzf_compress, file_of(A_NAME)[1], level=-1)
            passed = gate.left.is_set()
            ready = hip_rt.stream_ready(S)
        finally:
            gate.finish()
        assert passed and ready


def test_two_threads_share_the_stream(S, sctx):
    """The header's threading contract with one shared stream: each thread its own shard."""
    data, of = two_bam()
    want = of.eager_range(0, of.flat_size)
    s = sc.stream(A_NAME)
    got = {}

    def checker():
        got["eager"] = eager_of_two_bam(sctx)

    def sorter():
        sh = sctx.shard(file_of(A_NAME)[0])
        try:
            got["sorted"] = coordinate_sorted(sh, A_NAME)
        finally:
            sh.close()

    _run_threads([checker, sorter, checker])
    assert hip_rt.stream_ready(S)
    assert got["eager"][0] == want[0] and np.array_equal(got["eager"][1], want[1])
    w = sorted_want(A_NAME)
    assert len(s.starts) == w[2].size and all(np.array_equal(a, b) for a, b in zip(got["sorted"], w))


# ------------------------------------------------------------------------- E: device pointers, own streams

def test_device_pointer_input_on_an_own_stream_context(octx):
    """shard(ptr, on_device=True) and load(..., on_device=True): the pointer from hip_rt after a
    synchronous copy, and from another shard's flat_ptr() (a BGZF file stored inside a BGZF file)."""
    fa, fb = file_of(A_NAME)[0], file_of(B_NAME)[0]
    dev = hip_rt.malloc(fa.size)
    outer = octx.shard(np.frombuffer(rc.bgzf(fb.tobytes(), 65280, 1), np.uint8).copy())
    shards = [outer]
    try:
        hip_rt.memcpy(dev, fa, fa.size, hip_rt.H2D)
        sh = call(octx.shard, dev, on_device=True, nbytes=fa.size)
        shards.append(sh)
        host = call(octx.shard, fa)
        shards.append(host)
        got, want = coordinate_sorted(sh, A_NAME), coordinate_sorted(host, A_NAME)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert all(np.array_equal(a, b) for a, b in zip(got, sorted_want(A_NAME)))
        # the other file, from the flat bytes of the outer shard
        _, fs = call(outer.index, 0)
        call(outer.inflate)
        assert fs == fb.size
        call(sh.load, outer.flat_ptr(), 0, on_device=True, nbytes=fs)
        assert_is_b(coordinate_sorted(sh, B_NAME))
        fresh = call(octx.shard, outer.flat_ptr(), on_device=True, nbytes=fs)
        shards.append(fresh)
        assert_is_b(coordinate_sorted(fresh, B_NAME))
        call(host.load, fb, 0)
        assert_is_b(coordinate_sorted(host, B_NAME))
    finally:
        for x in shards:
            x.close()
        hip_rt.free(dev)
