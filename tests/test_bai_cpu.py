"""The host-only BAI finisher (sbh_bai_build: htslib's hts_idx_finish + the BAI layout), called
through ctypes without a GPU.  Inputs come from bai_ref (the CPU restatement of hts_idx_push)
or are written by hand; expectations for the hand cases are literals."""
import ctypes as C
import random

import numpy as np
import pytest

import bai_ref
from conftest import golden_bam
from pkg import sb

E_ARG, E_BAD_RECORD, E_UNSORTED = 1, 20, 21
U64_MAX = np.iinfo(np.uint64).max


def build_raw(runs, lin, contig_len, n_no_coor=0, cap=None):
    """(status, bytes or None, size) of one sbh_bai_build call."""
    L = sb.lib()
    runs = np.ascontiguousarray(runs, dtype=bai_ref.RUN_DTYPE)
    lin = np.ascontiguousarray(lin, dtype=np.uint64)
    cl = np.ascontiguousarray(contig_len, dtype=np.int32)
    if cap is None:
        cap = int(L.sbh_bai_bound(runs.size, lin.size, cl.size))
    out = np.zeros(max(cap, 1), np.uint8)
    size = C.c_uint64()
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    rc = L.sbh_bai_build(p(runs), runs.size, p(lin), p(cl), cl.size, n_no_coor, out.ctypes.data_as(C.c_void_p), cap,
                         C.byref(size))
    return rc, (out[:size.value].tobytes() if rc == 0 else None), size.value


@pytest.fixture(scope="module", params=["2.bam", "5k.bam"])
def ref(request):
    with open(golden_bam(request.param), "rb") as f:
        r = bai_ref.build(f.read())
    with open(golden_bam(request.param) + ".bai", "rb") as f:
        return request.param, r, f.read()


def test_fixture_parses_equal_to_samtools_index(ref):
    name, r, gold = ref
    rc, out, _ = build_raw(r.runs, r.lin, r.contig_len, r.n_no_coor)
    assert rc == 0
    assert out == r.bytes
    assert bai_ref.parsed(out) == bai_ref.parsed(gold)
    # and through the package's own reader: bins as a map, offsets, metadata
    a, b = sb.read_bai(out), sb.read_bai(gold)
    assert len(a.references) == len(b.references)
    for x, y in zip(a.references, b.references):
        assert {k.id: k.chunks for k in x.bins} == {k.id: k.chunks for k in y.bins}
        assert x.offsets == y.offsets and x.metadata == y.metadata


def test_metadata_of_2bam_is_the_pinned_one():
    with open(golden_bam("2.bam"), "rb") as f:
        r = bai_ref.build(f.read())
    _, out, _ = build_raw(r.runs, r.lin, r.contig_len, r.n_no_coor)
    refs, nnc = bai_ref.parsed(out)
    assert refs[0][1] == ((5650, 34847129600), (2450, 50)) and nnc == 0
    assert sorted(refs[0][0]) == [585, 4681, 4683, 4685]  # 4682 and 4684 folded into 585


def cut(run, rng):
    """One run as two runs of the same key meeting at a point strictly inside it."""
    mid = rng.randrange(int(run["vbeg"]) + 1, int(run["vend"]))
    nm, nu = rng.randint(0, int(run["n_mapped"])), rng.randint(0, int(run["n_unmapped"]))
    a = (run["ref_id"], run["bin"], run["vbeg"], mid, nm, nu)
    b = (run["ref_id"], run["bin"], mid, run["vend"], int(run["n_mapped"]) - nm, int(run["n_unmapped"]) - nu)
    return [a, b]


def test_seams_do_not_change_the_bytes(ref):
    _, r, _ = ref
    rng = random.Random(0xBA1)
    every = np.array([x for run in r.runs for x in cut(run, rng)], bai_ref.RUN_DTYPE)
    some = np.array([x for run in r.runs for x in (cut(run, rng) if rng.random() < 0.5 else [tuple(run)])],
                    bai_ref.RUN_DTYPE)
    assert every.size == 2 * r.runs.size and r.runs.size < some.size < every.size
    for runs in (every, some):
        rc, out, _ = build_raw(runs, r.lin, r.contig_len, r.n_no_coor)
        assert rc == 0 and out == r.bytes


# ---- the finish step, by hand.  Chunks are (first block address, last block address); one
# reference of 1 Mbp; every window untouched.

def _runs(*items):
    return np.array([(0, b, u << 16, v << 16, 1, 0) for b, u, v in items], bai_ref.RUN_DTYPE)


def _bins(runs, n_no_coor=0):
    lin = np.full((1000000 >> 14) + 2, U64_MAX, np.uint64)
    rc, out, _ = build_raw(runs, lin, [1000000], n_no_coor)
    assert rc == 0
    (bins, meta, offs), = bai_ref.parsed(out)[0]
    assert offs == []
    return {b: [(u >> 16, v >> 16) for u, v in ch] for b, ch in bins.items()}, meta


FAR = ((585, 1, 2), (585, 0x30000, 0x30001))  # keeps bin 585 wider than 0x10000 blocks


def test_leaf_spanning_ffff_blocks_folds_into_its_parent():
    bins, meta = _bins(_runs(FAR[0], (4681, 0x10, 0x1000F), FAR[1]))
    assert bins == {585: [(1, 2), (0x10, 0x1000F), (0x30000, 0x30001)]}
    assert meta == ((1 << 16, 0x30001 << 16), (3, 0))


def test_leaf_spanning_10000_blocks_stays():
    bins, _ = _bins(_runs(FAR[0], (4681, 0x10, 0x10010), FAR[1]))
    assert bins == {4681: [(0x10, 0x10010)], 585: [(1, 2), (0x30000, 0x30001)]}


def test_fold_cascades_two_levels():
    bins, _ = _bins(_runs((73, 1, 2), (4681, 0x10, 0x11), (73, 0x30000, 0x30001)))
    assert bins == {73: [(1, 2), (0x10, 0x11), (0x30000, 0x30001)]}


def test_parent_sorts_its_children_and_merges_same_block_chunks():
    runs = np.array([(0, 585, 1 << 16, 2 << 16, 1, 0),
                     (0, 4682, 0x100 << 16, 0x101 << 16 | 5, 1, 0),
                     (0, 4683, 0x101 << 16 | 5, 0x102 << 16, 1, 0),
                     (0, 4681, 0x500 << 16, 0x501 << 16, 1, 0),
                     (0, 585, 0x30000 << 16, 0x30001 << 16, 1, 0)], bai_ref.RUN_DTYPE)
    bins, _ = _bins(runs)
    assert bins == {585: [(1, 2), (0x100, 0x102), (0x500, 0x501), (0x30000, 0x30001)]}


def test_bin_0_is_sorted():
    # the leaf cascades 585 -> 73 -> 9 -> 1 -> 0 and lands between bin 0's own chunks
    bins, _ = _bins(_runs((0, 0x30000, 0x30001), (4681, 0x10, 0x11), (0, 1, 2)))
    assert bins == {0: [(1, 2), (0x10, 0x11), (0x30000, 0x30001)]}


def test_linear_index_fill_property():
    l_ref = 200000
    recs = [(0, 100, 100 << 16), (5 * 16384 + 10, 5 * 16384 + 60, 200 << 16),
            (5 * 16384 + 20, 7 * 16384 + 1, 300 << 16), (10 * 16384, 10 * 16384 + 5, 400 << 16)]
    lin = np.full((l_ref >> 14) + 2, U64_MAX, np.uint64)
    for beg, end, v in recs:
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            lin[w] = min(int(lin[w]), v)
    runs = np.array([(0, 0, recs[0][2], 500 << 16, 4, 0)], bai_ref.RUN_DTYPE)
    rc, out, _ = build_raw(runs, lin, [l_ref])
    assert rc == 0
    (_, _, offs), = bai_ref.parsed(out)[0]
    assert len(offs) == 11  # the largest touched window + 1
    for w, o in enumerate(offs):
        over = [v for beg, end, v in recs if beg >> 14 <= w <= (end - 1) >> 14]
        assert all(o <= v for v in over)
        if over:
            assert o == min(over)
    assert offs[1:5] == [200 << 16] * 4 and offs[8:10] == [400 << 16] * 2  # backward fill


def test_cap_too_small_is_an_argument_error(ref):
    _, r, _ = ref
    rc, _, size = build_raw(r.runs, r.lin, r.contig_len, r.n_no_coor, cap=len(r.bytes) - 1)
    assert rc == E_ARG and size == len(r.bytes)
    assert build_raw(r.runs, r.lin, r.contig_len, r.n_no_coor, cap=len(r.bytes))[1] == r.bytes


def test_no_runs_is_an_index_of_empty_references():
    lens = [16571, 5, 40000]
    lin = np.full(sum((x >> 14) + 2 for x in lens), U64_MAX, np.uint64)
    rc, out, _ = build_raw(np.zeros(0, bai_ref.RUN_DTYPE), lin, lens, n_no_coor=7)
    assert rc == 0
    assert bai_ref.parsed(out) == ([({}, None, [])] * 3, 7)
    assert len(sb.read_bai(out).references) == 3


def test_equal_key_runs_must_meet_and_bins_must_be_real():
    lin = np.full((1000 >> 14) + 2, U64_MAX, np.uint64)
    for second_vbeg in ((2 << 16) + 1, (2 << 16) - 1):  # a gap, an overlap
        runs = np.array([(0, 4681, 1 << 16, 2 << 16, 1, 0), (0, 4681, second_vbeg, 3 << 16, 1, 0)], bai_ref.RUN_DTYPE)
        assert build_raw(runs, lin, [1000])[0] == E_ARG
    for b in (37450, 37451, 1 << 31):
        assert build_raw(np.array([(0, b, 1 << 16, 2 << 16, 1, 0)], bai_ref.RUN_DTYPE), lin, [1000])[0] == E_ARG
    assert build_raw(np.array([(0, 37449, 1 << 16, 2 << 16, 1, 0)], bai_ref.RUN_DTYPE), lin, [1000])[0] == 0


def test_run_order_and_range_are_checked():
    lin = np.full(2 * ((1000 >> 14) + 2), U64_MAX, np.uint64)
    back = np.array([(1, 4681, 1 << 16, 2 << 16, 1, 0), (0, 4681, 2 << 16, 3 << 16, 1, 0)], bai_ref.RUN_DTYPE)
    assert build_raw(back, lin, [1000, 1000])[0] == E_UNSORTED
    off = np.array([(2, 4681, 1 << 16, 2 << 16, 1, 0)], bai_ref.RUN_DTYPE)
    assert build_raw(off, lin, [1000, 1000])[0] == E_BAD_RECORD
