"""Batched record delivery: many FileSplits of one shard in one call (sbh_split_records_batch,
Shard.split_records_batch, SplitWorker.split_batch, load_reads_and_positions(batch=K)).

The oracle is the per-split path (Shard.split_records / SplitWorker.split), itself pinned to the
reference's answers in test_canloadbam_gpu.py: for every split of a batch, (status, block_start,
first_vpos, rec_count) and every column of its records equal what sbh_split_records answers for
that split alone on a shard loaded from the split's start to the same resident end.  Reference
numbers are checked directly too: LoadBAMTest's 2.bam partition sizes at 20000-byte splits
(load/src/test/.../LoadBAMTest.scala), ComputeSplitsTest's 1.bam splits at 230 KiB and
CountReadsTest's 4917 reads.
"""
import os
import sys

import numpy as np
import pytest

from conftest import golden_bam
from oracle_lib import OracleFile, file_splits
from pkg import sb
from test_splits_gpu import SYN

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))

clb = __import__(sb.__name__ + ".canloadbam", fromlist=["x"])
rec = __import__(sb.__name__ + ".records", fromlist=["x"])

OK, E_ARG, E_HSF, E_NOREAD, E_HALO, E_BAD_RECORD = 0, 1, 11, 16, 17, 20
COUNTS_2BAM_20000 = [96, 102, 105, 101, 99, 102, 101, 106, 0, 105, 105, 102, 104, 103, 104, 106,
                     104, 106, 0, 105, 195, 101, 0, 99, 98, 99, 52]


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


class Corpus:
    def __init__(self, data):
        self.data = data
        self.contigs = OracleFile(data).contig_len
        self.ref = {}  # (splits, resident end, kwargs) -> the per-split answers, computed once


@pytest.fixture(scope="module")
def corpora():
    import synth
    made = {}

    def get(name):
        if name not in made:
            if name.endswith(".bam"):
                data = np.fromfile(golden_bam(name), dtype=np.uint8)
            else:
                kw, nrec = SYN[name]
                p = synth.params(kw["seed"], shape=kw["shape"], level=kw["level"], empty_every=kw.get("empty_every", 0))
                data = synth.make_bam(p, nrec)[0]
            made[name] = Corpus(data)
        return made[name]
    return get


def per_split(ctx, c, splits, res_end=None, **kw):
    """Shard.split_records for every split alone, on a shard holding [start, res_end) of the file:
    [(status, info or error fields, columns or None)].  One shard, reloaded per split."""
    res_end = c.data.size if res_end is None else res_end
    key = (tuple(splits), res_end, tuple(sorted(kw.items())))
    if key in c.ref:
        return c.ref[key]
    out, sh = [], None
    try:
        for s, e in splits:
            if sh is None:
                sh = ctx.shard(c.data[s:res_end], file_offset=s, file_size=c.data.size)
                sh.set_contigs(c.contigs)
            else:
                sh.load(c.data[s:res_end], s)
            try:
                info, cols = sh.split_records(s, e, **kw)
                out.append((OK, info, cols))
            except sb.SparkBamError as err:
                out.append((err.code, err.fields, None))
    finally:
        if sh is not None:
            sh.close()
    c.ref[key] = out
    return out


def batch(ctx, c, splits, res_end=None, **kw):
    """The batch over a shard holding [first start, res_end): (info, per-split dicts, columns, and
    the flat offset of every split's own first block, which its per-split flat offsets count from)."""
    res_end = c.data.size if res_end is None else res_end
    lo = splits[0][0]
    sh = ctx.shard(c.data[lo:res_end], file_offset=lo, file_size=c.data.size)
    try:
        sh.set_contigs(c.contigs)
        info, per, cols = sh.split_records_batch(splits, **kw)
        base = [sh.flat_of(s["block_start"]) if s["status"] == OK and s["rec_count"] else 0 for s in per]
    finally:
        sh.close()
    return info, per, cols, base


def assert_equal_per_split(ref, per, cols, base, where=""):
    assert len(ref) == len(per)
    rows = 0
    for i, ((st, info, rc), s) in enumerate(zip(ref, per)):
        at = f"{where} split {i}"
        assert s["status"] == st, at
        assert s["rec_begin"] == rows, at
        if st == E_NOREAD:
            assert s["block_start"] == info[0] and s["rec_count"] == 0, at  # (fields: blockStart, maxReadSize)
        if st != OK:
            assert s["rec_count"] == 0, at
            continue
        assert (s["block_start"], s["rec_count"]) == (info["block_start"], info["n"]), at
        rows += s["rec_count"]
        if not info["n"]:
            continue
        assert s["first_vpos"] == info["first_vpos"], at
        mine = rec.slice_columns(cols, s["rec_begin"], s["rec_begin"] + s["rec_count"])
        assert set(mine) == set(rc), at
        for k in rc:
            a = mine[k] - np.uint64(base[i]) if k == "flat" else mine[k]
            assert np.array_equal(a, rc[k]), (at, k)
    assert rows == cols["flat"].size == cols["vpos"].size


def pos_str(v):
    return f"{int(v) >> 16}:{int(v) & 0xFFFF}"


# ---- reference numbers ----------------------------------------------------------------------

def test_2bam_20000_partition_sizes(ctx, corpora):
    c = corpora("2.bam")
    info, per, cols, _ = batch(ctx, c, file_splits(c.data.size, 20000))
    assert [s["rec_count"] for s in per] == COUNTS_2BAM_20000  # LoadBAMTest "2e4", empty partitions included
    assert [s["status"] for s in per] == [OK] * len(per)
    assert info["n"] == 2500 == cols["vpos"].size


def test_1bam_230k_splits(ctx, corpora):
    c = corpora("1.bam")
    info, per, cols, _ = batch(ctx, c, file_splits(c.data.size, 230 * 1024))
    firsts = [pos_str(s["first_vpos"]) for s in per if s["rec_count"]] + [f"{c.data.size}:0"]
    assert [f"{a}-{b}" for a, b in zip(firsts, firsts[1:])] == [
        "0:45846-239479:312", "239479:312-484396:25", "484396:25-597482:0"]  # ComputeSplitsTest "eager 230KB"
    assert info["n"] == 4917  # CountReadsTest
    for s in per:
        if s["rec_count"]:
            assert int(cols["vpos"][s["rec_begin"]]) == s["first_vpos"]


# ---- every column equals the per-split path ---------------------------------------------------

CASES = [("2.bam", 20000), ("1.bam", 100000), ("5k.bam", 64 * 1024)] + \
        [(name, -div) for name in ("short_l6", "long", "adversarial", "adversarial_empty") for div in (13, 40)]


def splits_of(c, size):
    if size < 0:  # cut into -size splits (test_splits_gpu.py's rule)
        size = max(c.data.size // -size, 20000)
    return file_splits(c.data.size, size)


@pytest.mark.parametrize("name,size", CASES)
def test_batch_equals_per_split(ctx, corpora, name, size):
    c = corpora(name)
    splits = splits_of(c, size)
    ref = per_split(ctx, c, splits)
    if E_BAD_RECORD in [st for st, _, _ in ref]:
        # adversarial_empty: the last record before each empty block runs over it, and an empty
        # block ends the stream, so sbh_split_records fails the splits holding those records
        # (htsjdk's truncated record) -- and so does the batch that holds them, as a whole.  The
        # same corpus is compared column by column below: starts only (decode = 0, no record is
        # measured), and decoded over splits that leave those records out.
        assert name == "adversarial_empty"
        print(f"{name} @ {size}: per-split statuses {[st for st, _, _ in ref]}")
        with pytest.raises(sb.SparkBamError) as e:
            batch(ctx, c, splits)
        assert e.value.code == E_BAD_RECORD
        return
    info, per, cols, base = batch(ctx, c, splits)
    print(f"{name} @ {size}: {len(splits)} splits, n_host = {info['n_host']}")
    assert info["n_host"] == sum(s["host_path"] for s in per)
    assert_equal_per_split(ref, per, cols, base, name)


@pytest.mark.parametrize("div", [13, 40])
def test_host_path_starts_only(ctx, corpora, div):
    """adversarial_empty, starts only: empty blocks end the stream, so the splits past the first
    one take sbh_split's exact path (host_path = 1) and their record starts are walked along the
    chain into their rows -- the same starts and virtual positions as the per-split path."""
    c = corpora("adversarial_empty")
    splits = splits_of(c, -div)
    info, per, cols, base = batch(ctx, c, splits, decode=False)
    print(f"adversarial_empty @ -{div} (starts only): {len(splits)} splits, n_host = {info['n_host']}")
    assert info["n_host"] == sum(s["host_path"] for s in per) > 0
    assert any(s["host_path"] and s["rec_count"] for s in per)
    assert_equal_per_split(per_split(ctx, c, splits, decode=False), per, cols, base)


def bgzf_blocks(data):
    """(file offset, is empty) of every BGZF block, from the headers (BSIZE) and footers (ISIZE)."""
    out, q = [], 0
    while q + 18 <= data.size:
        cs = (int(data[q + 16]) | int(data[q + 17]) << 8) + 1
        out.append((q, not data[q + cs - 4:q + cs].any()))
        q += cs
    return out


def test_host_path_decoded(ctx, corpora):
    """adversarial_empty, decoded: one split per stream segment (the blocks between two empty
    blocks), from one byte past the empty block -- FindBlockStart's window starts inside it -- to
    the segment's third block, so no split holds the record that runs over the next empty block.
    The splits behind the first empty block take the exact path; every column equals the
    per-split path's."""
    c = corpora("adversarial_empty")
    blocks = bgzf_blocks(c.data)
    empties = [i for i, (_, empty) in enumerate(blocks) if empty]
    splits = [(0, blocks[2][0])]
    for i in empties[:5]:
        assert not blocks[i + 1][1] and not blocks[i + 3][1]
        splits.append((blocks[i][0] + 1, blocks[i + 3][0]))
    info, per, cols, base = batch(ctx, c, splits)
    print(f"adversarial_empty, a split per segment: {len(splits)} splits, n_host = {info['n_host']}")
    assert [s["status"] for s in per] == [OK] * len(splits) and all(s["rec_count"] for s in per)
    assert info["n_host"] == sum(s["host_path"] for s in per) >= 5
    assert_equal_per_split(per_split(ctx, c, splits), per, cols, base)
    _, per0, cols0, _ = batch(ctx, c, splits, decode=False)
    assert per0 == per and np.array_equal(cols0["flat"], cols["flat"]) and np.array_equal(cols0["vpos"], cols["vpos"])


def test_many_small_splits(ctx, corpora):
    c = corpora("2.bam")
    splits = file_splits(c.data.size, 4096)
    assert len(splits) > 64
    info, per, cols, base = batch(ctx, c, splits)
    assert sum(1 for s in per if s["status"] == OK and not s["rec_count"]) > 20  # splits holding no block start
    assert_equal_per_split(per_split(ctx, c, splits), per, cols, base)
    assert sum(s["rec_count"] for s in per) == 2500 == info["n"]


def test_gaps_every_other_split(ctx, corpora):
    c = corpora("2.bam")
    splits = file_splits(c.data.size, 20000)
    some = splits[1::2]
    info, per, cols, base = batch(ctx, c, some)
    assert [s["rec_count"] for s in per] == COUNTS_2BAM_20000[1::2]
    assert [s["rec_begin"] for s in per] == np.concatenate([[0], np.cumsum(COUNTS_2BAM_20000[1::2])[:-1]]).tolist()
    assert info["n"] == sum(COUNTS_2BAM_20000[1::2])  # only the asked splits' records
    assert_equal_per_split(per_split(ctx, c, some), per, cols, base)


def test_single_split_equals_split_records(ctx, corpora):
    c = corpora("2.bam")
    s, e = file_splits(c.data.size, 20000)[3]
    (st, info, rc), = per_split(ctx, c, [(s, e)])
    binfo, per, cols, base = batch(ctx, c, [(s, e)])
    assert st == OK and base == [0]  # the same shard, the same flat offsets
    assert_equal_per_split([(st, info, rc)], per, cols, base)
    assert (binfo["block_start"], binfo["n_blocks"], binfo["flat_size"]) == \
        (info["block_start"], info["n_blocks"], info["flat_size"])
    assert (per[0]["first_flat"], per[0]["owned_flat"]) == (info["first_flat"], info["owned_flat"])
    assert np.array_equal(cols["flat"], rc["flat"])


@pytest.mark.parametrize("name,size", [("2.bam", 20000), ("adversarial", -13)])
def test_starts_only_equals_decoded(ctx, corpora, name, size):
    c = corpora(name)
    splits = splits_of(c, size)
    _, per1, cols1, _ = batch(ctx, c, splits)
    _, per0, cols0, _ = batch(ctx, c, splits, decode=False)
    assert per0 == per1
    assert set(cols0) == {"flat", "vpos"}
    assert np.array_equal(cols0["flat"], cols1["flat"]) and np.array_equal(cols0["vpos"], cols1["vpos"])


# ---- an open shard end ------------------------------------------------------------------------

@pytest.mark.parametrize("decode", [True, False])
def test_open_end_statuses(ctx, corpora, decode):
    """The shard holds [0, ends[k]) of 2.bam and the file goes on: no halo.  Every split answers
    what it answers alone over the same resident bytes -- NEED_HALO where its answer needs the
    missing bytes -- and the splits that are decided keep their records."""
    c = corpora("2.bam")
    splits = file_splits(c.data.size, 20000)[:11]
    res_end = splits[-1][1]
    ref = per_split(ctx, c, splits, res_end, decode=decode)
    info, per, cols, base = batch(ctx, c, splits, res_end, decode=decode)
    assert_equal_per_split(ref, per, cols, base)
    assert E_HALO in [s["status"] for s in per]
    ok = [s for s in per if s["status"] == OK]
    assert ok and sum(s["rec_count"] for s in ok) == info["n"] > 0


# ---- per-split errors -------------------------------------------------------------------------

def test_no_read_found_split(ctx, corpora):
    """1.bam's first record lies 45846 bytes into its first block: with maxReadSize 1000 split 0
    is NoReadFoundException(path, 0, 1000); the other splits have their records."""
    c = corpora("1.bam")
    splits = file_splits(c.data.size, 100000)
    ref = per_split(ctx, c, splits, max_read_size=1000)
    info, per, cols, base = batch(ctx, c, splits, max_read_size=1000)
    assert_equal_per_split(ref, per, cols, base)
    assert (per[0]["status"], per[0]["block_start"]) == (E_NOREAD, 0) and ref[0][1][:2] == (0, 1000)
    assert info["n"] > 0
    path = golden_bam("1.bam")
    with pytest.raises(sb.NoReadFoundException) as e:
        clb.load_reads_and_positions(path, split_size=100000, max_read_size=1000, ctx=ctx, batch=8)
    with pytest.raises(sb.NoReadFoundException) as e1:
        clb.load_reads_and_positions(path, split_size=100000, max_read_size=1000, ctx=ctx)
    assert (e.value.path, e.value.start, e.value.max_read_size) == (path, 0, 1000)
    assert (e1.value.path, e1.value.start, e1.value.max_read_size) == (path, 0, 1000)


def test_header_search_failed_split(ctx):
    """A batch whose first splits hold no BGZF header: each is HeaderSearchFailedException(path,
    start, 65536) on its own, and the splits behind them still get their records."""
    data = np.fromfile(golden_bam("2.bam"), dtype=np.uint8)
    rng = np.random.default_rng(5)
    junk = rng.integers(0, 256, 200_000, dtype=np.uint8)
    junk[junk == 31] = 30  # no gzip magic anywhere
    c = Corpus.__new__(Corpus)
    c.data, c.contigs, c.ref = np.concatenate([junk, data]), OracleFile(data).contig_len, {}
    splits = [(0, 70_000), (70_000, 134_000), (200_000, 300_000), (300_000, 400_000)]
    ref = per_split(ctx, c, splits)
    info, per, cols, base = batch(ctx, c, splits)
    assert [s["status"] for s in per] == [E_HSF, E_HSF, OK, OK]
    assert_equal_per_split(ref, per, cols, base)
    assert info["n"] > 0


@pytest.mark.parametrize("splits", [
    [(20000, 40000), (0, 20000)],          # unsorted
    [(0, 30000), (20000, 40000)],          # overlapping
    [(0, 20000), (20000, 20000)],          # an empty split
    [(600000, 700000)],                    # the first start outside the shard
    [],
])
def test_bad_arguments(ctx, corpora, splits):
    c = corpora("2.bam")
    sh = ctx.shard(c.data, file_size=c.data.size)
    try:
        sh.set_contigs(c.contigs)
        with pytest.raises(sb.SparkBamError) as e:
            sh.split_records_batch(splits)
        assert e.value.code == E_ARG
    finally:
        sh.close()


# ---- the facade -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def facade_ref(ctx):
    made = {}

    def get(name, size):
        if (name, size) not in made:
            made[name, size] = clb.load_reads_and_positions(golden_bam(name), split_size=size, ctx=ctx)
        return made[name, size]
    return get


def assert_same_partitions(parts, ref):
    assert len(parts) == len(ref)
    for i, (p, q) in enumerate(zip(parts, ref)):
        assert p.n == q.n and set(p.cols) == set(q.cols), i
        for k in q.cols:
            assert p.cols[k].dtype == q.cols[k].dtype and np.array_equal(p.cols[k], q.cols[k]), (i, k)


@pytest.mark.parametrize("name,size", [("2.bam", 20000), ("1.bam", 100000)])
@pytest.mark.parametrize("k", [2, 8, "all"])
def test_facade_batch_equals_per_split(ctx, facade_ref, name, size, k):
    parts = clb.load_reads_and_positions(golden_bam(name), split_size=size, ctx=ctx, batch=k)
    assert_same_partitions(parts, facade_ref(name, size))


def test_facade_batch_threads(ctx, facade_ref):
    parts = clb.load_reads_and_positions(golden_bam("2.bam"), split_size=20000, ctx=ctx, threads=4, batch=4)
    assert_same_partitions(parts, facade_ref("2.bam", 20000))
    splits, parts = clb.load_splits_and_reads(golden_bam("1.bam"), split_size=230 * 1024, ctx=ctx, batch="all")
    assert [f"{a}-{b}" for a, b in splits] == ["0:45846-239479:312", "239479:312-484396:25", "484396:25-597482:0"]
    assert sum(p.n for p in parts) == 4917
    assert [p.n for p in clb.load_bam(golden_bam("2.bam"), split_size=20000, ctx=ctx, batch=8)] == COUNTS_2BAM_20000
