"""The BGZF container kernels held to the hand-built corpus of bgzf_corpus.py (which
test_bgzf_corpus_cpu.py holds to zlib and the oracle): the candidate scan, the chain and the block
table (bgzf_index.hip: k_cand_count, k_cand_write, k_cand_link, k_chain_emit, the two-level scan)
on both chain paths, the inflate over those tables, k_block_crc in both directions (every size and
alignment it branches on passes; every corrupted member is counted, and no other), the in-run CRC
of the windowed path, and k_find_block_start against the probe literals, whole and cut."""
import numpy as np
import pytest

import bgzf_corpus as bc
from pkg import knob, sb
from test_index_chain_gpu import both, index_run

pytestmark = pytest.mark.gpu

E = sb._lib
SBH_E_HIP = E.SBH_E_HIP


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def call(f, *a, **kw):
    """f(*a): a device error ends the session (nothing more runs on this GPU)."""
    try:
        return f(*a, **kw)
    except sb.SparkBamError as e:
        if e.code == SBH_E_HIP:
            pytest.exit("HIP error: %s" % e, returncode=3)
        raise


def arr(b):
    return np.frombuffer(b, np.uint8)


def want_blocks(table, file_offset=0):
    """sh.blocks() of a member table: (start, csize, usize, ustart, hsize, flags)."""
    ust, total = bc.ustarts(table)
    return [(m.start + file_offset, m.csize, 0 if m.empty else m.usize, u, m.hsize, sb.BLOCK_EMPTY if m.empty else 0)
            for m, u in zip(table, ust)], total


def no_hip(res):
    if isinstance(res[0], str) and "SBH_E_HIP" in res[1]:
        pytest.exit("HIP error: %s" % res[1], returncode=3)
    return res


def explain(got, want):
    if isinstance(got, str) or len(got) != len(want):
        return "table of %s entries, want %d" % (got if isinstance(got, str) else len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "entry %d: got %s, want %s (start, csize, usize, ustart, hsize, flags)" % (i, g, w)
    return "equal"


# --------------------------------------------------------------------------------------- index
@pytest.mark.parametrize("f", bc.index_files(), ids=lambda f: f.name)
def test_index_gives_the_builders_table(ctx, f):
    want, total = want_blocks(f.table)
    for jump in (False, True):
        res = no_hip(index_run(ctx, arr(f.data), f.table[0].start, jump))
        assert len(res) == 3, res
        nb, fs, bl = res
        assert bl == want, "%s jump=%s: %s" % (f.name, jump, explain(bl, want))
        assert (nb, fs) == (len(f.table), total)


def chain_jump(on):
    return knob("SBH_CHAIN_JUMP", "1" if on else "0")


@pytest.mark.parametrize("residue,count", [(1, 20), (7, 30), (13, 2)])
def test_edges_as_a_shard_off_the_chunk_grid(ctx, residue, count):
    """File bytes [off, end) with file_offset = off: every edge moves by off mod 16384 against the
    scan's chunks (and by off mod 16 against its vectors); the table comes back in file offsets."""
    f = bc.edges()
    first = [i for i, m in enumerate(f.table) if m.start % 16 == residue][0]
    last = min(first + count, len(f.table)) - 1
    off, end = f.table[first].start, f.table[last].start + f.table[last].csize
    assert off % bc.CHUNK and off % 16
    tab = [m._replace(start=m.start - off) for m in f.table[first:last + 1]]
    want, total = want_blocks(tab, off)
    for jump in (False, True):
        with chain_jump(jump):
            sh = ctx.shard(arr(f.data[off:end]), file_offset=off, file_size=len(f.data))
            try:
                nb, fs = call(sh.index)
                bl = sh.blocks()
            finally:
                sh.close()
        assert bl == want, "jump=%s: %s" % (jump, explain(bl, want))
        assert (nb, fs) == (len(tab), total)


def test_both_paths_agree_from_a_later_start(ctx):
    f = bc.planted()
    for k in (1, 4, 13):
        nb, fs, bl = no_hip(both(ctx, arr(f.data), start=f.table[k].start))
        want, total = want_blocks([m for m in f.table[k:]])
        assert [b[:3] + b[4:] for b in bl] == [w[:3] + w[4:] for w in want] and nb == len(want)


# ------------------------------------------------------------------- inflate over those tables
@pytest.mark.parametrize("f", (bc.shapes(), bc.planted()), ids=lambda f: f.name)
def test_inflate_over_the_table(ctx, f):
    sh = ctx.shard(arr(f.data))
    try:
        nb, fs = call(sh.index, 0)
        assert (nb, fs) == (len(f.table), len(f.flat))
        call(sh.inflate)
        got = call(sh.read_flat)
        assert got.size == len(f.flat)
        ust = bc.ustarts(f.table)[0]
        for m, u, label in zip(f.table, ust, f.meta):
            if not m.empty:
                assert bytes(got[u:u + m.usize]) == f.flat[u:u + m.usize], (label, m)
        assert call(sh.verify_crc) == (0, 0)
    finally:
        sh.close()


# ----------------------------------------------------------------------------------------- CRC
def crc_of(ctx, f, check_flat):
    sh = ctx.shard(arr(f.data))
    try:
        nb, fs = call(sh.index, f.table[0].start)
        assert (nb, fs) == (len(f.table), len(f.flat))
        call(sh.inflate)
        if check_flat:  # a CRC pass over wrong bytes must not go unnoticed
            got = bytes(call(sh.read_flat))
            if got != f.flat:
                ust = bc.ustarts(f.table)[0]
                bad = [(i, m, f.meta[i]) for i, (m, u) in enumerate(zip(f.table, ust))
                       if got[u:u + m.usize] != f.flat[u:u + m.usize]]
                raise AssertionError("%s: inflated bytes differ in members %s" % (f.name, bad[:8]))
        return call(sh.verify_crc)
    finally:
        sh.close()


@pytest.mark.parametrize("f", bc.crc_sizes(), ids=lambda f: f.name)
def test_crc_passes_at_every_size_and_alignment(ctx, f):
    got = crc_of(ctx, f, True)
    if got != (0, 0):
        first = [(m, meta) for m, meta in zip(f.table, f.meta) if m.start == got[1]]
        raise AssertionError("%s: %d blocks called bad, the first %s (size, alignment of the flat bytes)" %
                             (f.name, got[0], first))


@pytest.mark.parametrize("c", bc.crc_bad(), ids=lambda c: c.name)
def test_crc_counts_exactly_the_corrupted_members(ctx, c):
    got = crc_of(ctx, c.file, False)
    assert got == (c.n_bad, c.first_bad), "%s: corrupted members %s" % (
        c.name, [(i, c.file.table[i], c.file.meta[i]) for i in c.bad][:20])


def test_crc_in_the_windowed_run_counts_each_bad_block_once(ctx):
    """32768-byte windows: members 17 and 18 start in the second window and are inflated with the
    first one too (its halo: the payload is not BAM records, so the record search asks for more
    bytes until a window's load reaches the end of the file, and every bad block is inflated by
    each window up to the one that owns it).  Each counts once, in the window that owns it, and
    crc_first_bad is the lowest one's offset."""
    c = bc.crc_stream_case()
    data = arr(c.file.data).copy()
    t = c.file.table
    assert t[16].start < 32768 <= t[17].start and t[18].start + t[18].csize <= 32768 + 8192
    s, _ = call(ctx.run_stream, data, np.array([1000], np.int32), index_start=0, window=32768, halo=8192,
                verify_crc=True)
    assert s["status"] == 0 and s["n_windows"] == 4 and s["halo_final"] >= 8192
    assert s["n_blocks"] == len(t)
    assert (s["crc_bad_blocks"], s["crc_first_bad"]) == (c.n_bad, c.first_bad), [t[i] for i in c.bad]
    good, _ = call(ctx.run_stream, arr(bc.crc_stream_clean().data).copy(), np.array([1000], np.int32), index_start=0,
                   window=32768, halo=8192, verify_crc=True)
    assert good["status"] == 0 and good["n_windows"] == 4 and good["crc_bad_blocks"] == 0


# ------------------------------------------------------------------------------ FindBlockStart
def fbs(ctx, data, start, k, file_size=None):
    sh = ctx.shard(data, file_size=file_size)
    try:
        return (bc.OK, call(sh.find_block_start, start, k))
    except sb.SparkBamError as e:
        return ("error", e.code, e.fields)
    finally:
        sh.close()


@pytest.mark.parametrize("p", bc.FBS, ids=lambda p: p.name)
def test_find_block_start_returns_the_literal(ctx, p):
    f = bc.fbs_files()[p.file]
    got = fbs(ctx, arr(f.data), p.start, p.blocks_to_check)
    if p.want[0] == bc.OK:
        assert got == p.want
    elif p.want[0] == bc.SEARCH_FAILED:
        assert got == ("error", E.SBH_E_HEADER_SEARCH_FAILED, (p.start, 65536))
    else:
        assert got[:2] == ("error", E.SBH_E_TRUNCATED)
    if p.cut is not None:  # the shard ends inside the look-ahead and the file goes on
        got = fbs(ctx, arr(f.data[:p.cut]), p.start, p.blocks_to_check, file_size=len(f.data))
        assert got[:2] == ("error", E.SBH_E_NEED_HALO), "cut at %d" % p.cut
