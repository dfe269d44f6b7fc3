"""BAI construction on the GPU (sbh_bai_scan / sbh_bai_fetch, build_bai) against bai_ref, the
CPU restatement of htslib's hts_idx_push / hts_idx_finish, and against the samtools-written
golden indexes.  The corpora are built with record_corpus' helpers; a property the corpus
must have (a record ending on a member end, runs meeting inside one member, ...) is asserted
on the reference's side before the device's answer is compared."""
import random

import numpy as np
import pytest

import bai_ref
from conftest import golden_bam
from pkg import sb
from record_corpus import D, EQ, I, M, N, S, X, bgzf, header, rec

gpu = pytest.mark.gpu

E_BAD_RECORD, E_UNSORTED = 20, 21
B = 256  # workgroup size of the scan kernels (bai.hip BAI_T)
CONTIGS = (("c0", 1 << 29), ("c1", 1000), ("c2", 100000), ("c3", 50))  # c1 and c3 stay empty


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def r_(ref, pos, cigar=((10, M),), flag=0, bin=4681, name=b"r", aux=b""):
    n = sum(ln for ln, op in cigar if op in (M, I, S, 7, 8))
    n = min(n, 40)  # (l_seq need not match the CIGAR for the index)
    return rec(ref, pos, 30, bin, flag, -1, -1, 0, name, tuple(cigar), (1,) * n, b"\x20" * n, aux)


def spread_cigar(nops, total):
    """nops CIGAR ops whose reference length is exactly `total`: the even ops consume the
    reference (M D N = X in turn, unequal lengths, every one needed for the sum), the odd ops
    (I, S) do not."""
    counted = (nops + 1) // 2
    base = total // counted
    assert base > 8
    lens = [base + (k % 7) - 3 for k in range(counted)]
    lens[-1] += total - sum(lens)
    ops = []
    for k in range(nops):
        ops.append((lens[k // 2], (M, D, N, EQ, X)[(k // 2) % 5]) if k % 2 == 0 else (3, (I, S)[(k // 2) % 2]))
    assert sum(ln for ln, op in ops if op in (M, D, N, EQ, X)) == total
    return tuple(ops)


def bam(records, payload=300, contigs=CONTIGS):
    return bgzf(header(contigs) + b"".join(records), payload)


def scan(ctx, data, eager=False):
    """Shard.bai_scan over every record of the file: (runs, lin, n_no_coor)."""
    data = np.frombuffer(data, np.uint8)
    sh = ctx.shard(data)
    try:
        sh.index(0)
        sh.inflate()
        _, lens, hdr_end = sb.bam_header(sh)
        sh.set_contigs(lens)
        end = sh.flat_size  # (the EOF member holds no bytes)
        if eager:
            sh.check_eager(hdr_end, end, want_bits=False)
        return sh.bai_scan(hdr_end, end)
    finally:
        sh.close()


def same_runs(got, want):
    return got.dtype == want.dtype and got.size == want.size and got.tobytes() == want.tobytes()


def check_all(ctx, data, eager=False):
    want = bai_ref.build(data)
    runs, lin, nnc = scan(ctx, data, eager)
    assert same_runs(runs, want.runs), (runs, want.runs)
    assert np.array_equal(lin, want.lin)
    assert nnc == want.n_no_coor
    assert sb.build_bai(data, ctx=ctx) == want.bytes
    return want


# ------------------------------------------------------------------ golden fixtures

@gpu
@pytest.mark.parametrize("name", ["2.bam", "5k.bam"])
def test_golden_fixture(ctx, name):
    with open(golden_bam(name), "rb") as f:
        data = f.read()
    with open(golden_bam(name) + ".bai", "rb") as f:
        gold = f.read()
    out = sb.build_bai(golden_bam(name), ctx=ctx)
    assert out == bai_ref.build(data).bytes
    assert bai_ref.parsed(out) == bai_ref.parsed(gold)


@gpu
def test_windowed_build_equals_whole_file(ctx, monkeypatch):
    loads = []
    real = sb.Shard.load
    monkeypatch.setattr(sb.Shard, "load", lambda self, *a, **k: (loads.append(a[1]), real(self, *a, **k))[1])
    whole = sb.build_bai(golden_bam("2.bam"), ctx=ctx)
    assert not loads
    assert sb.build_bai(golden_bam("2.bam"), ctx=ctx, window=150000) == whole
    assert len(loads) >= 2  # the first window creates the shard: >= 3 windows


# ------------------------------------------------------------------ the hand-built corpus

def corpus():
    rng = random.Random(0x1DE)
    noise = lambda n: bytes(rng.randrange(256) for _ in range(n))  # noqa: E731
    # 3000 ops whose reference length puts the record's last base on the last position of window
    # 4273 (one more would touch window 4274) and the record in a level-4 bin of its own
    long_pos = 70000000
    long_cigar = spread_cigar(3000, 4274 * 16384 - long_pos)
    recs = [
        ("plain", r_(0, 100, bin=0)),                                    # the stored bin is wrong
        ("two_windows", r_(0, 16383, ((2, M),))),                        # windows 0 and 1: level 4
        ("placed_unmapped", r_(0, 20000, flag=4)),                       # end = pos + 1, counted unmapped
        ("clips_only", r_(0, 20100, ((5, S), (3, I)))),                  # no reference length: end = pos + 1
        ("no_cigar", r_(0, 20200, ())),
        ("n_4_windows", r_(0, 30000, ((5, M), (40000, N), (5, M)))),     # windows 1..4
        ("level3", r_(0, 100000, ((5, M), (100000, N), (5, M)))),
        ("level2", r_(0, 1000000, ((5, M), (200000, N), (5, M)))),
        ("level1", r_(0, 8000000, ((5, M), (1000000, N), (5, M)))),
        ("level0", r_(0, 67000000, ((5, M), (1000000, N), (5, M)))),
        ("before_long", r_(0, 70000000)),
        ("long_cigar", r_(0, long_pos, long_cigar)),
        ("after_long", r_(0, 70000100)),
    ]
    # c2: bin 4681 (A) and bin 585 (B, reads reaching window 1) interleaved, positions rising.
    # A1 B1 A2 lie close together; B2 is ~100 KB of incompressible tags, so A3 starts far away
    # and neither bin folds into its parent.
    reach = ((5, M), (17000, N), (5, M))
    recs += [("a1_%d" % k, r_(2, 100 + k)) for k in range(2)]
    recs += [("b1", r_(2, 110, reach))]
    recs += [("a2_%d" % k, r_(2, 120 + k)) for k in range(2)]
    recs += [("b2_%d" % k, r_(2, 130, reach, aux=b"XZZ" + noise(200).replace(b"\0", b"\1") + b"\0"))
             for k in range(500)]
    recs += [("a3_%d" % k, r_(2, 140 + k)) for k in range(2)]
    recs += [("tail_%d" % k, r_(-1, -1, (), flag=4)) for k in range(3)]
    return recs


PAYLOAD = 300


@pytest.fixture(scope="module")
def hand():
    recs = corpus()
    # "ends_member": a record whose last byte is the last byte of a BGZF member
    k = [lab for lab, _ in recs].index("after_long") + 1
    before = len(header(CONTIGS)) + sum(len(b) for _, b in recs[:k])
    base = len(r_(0, 70000200, aux=b"XZZ\0"))
    pad = (-(before + base)) % PAYLOAD
    recs.insert(k, ("ends_member", r_(0, 70000200, aux=b"XZZ" + b"p" * pad + b"\0")))
    data = bam([b for _, b in recs], PAYLOAD)
    return [lab for lab, _ in recs], data


def test_hand_corpus_has_the_cases_it_claims(hand):
    labels, data = hand
    want = bai_ref.build(data)
    by = dict(zip(labels, want.records))
    assert len(want.records) == len(labels)
    assert by["two_windows"].end - 1 >> 14 == 1 and by["two_windows"].beg >> 14 == 0
    assert (by["n_4_windows"].end - 1 >> 14) - (by["n_4_windows"].beg >> 14) >= 2
    levels = {bai_ref.level_of(r.bin) for r in want.records if r.ref_id == 0}
    assert levels == {0, 1, 2, 3, 4, 5}
    lc = by["long_cigar"]
    assert lc.bin != bai_ref.reg2bin(lc.pos, lc.pos + 1) and lc.end - 1 >> 14 > lc.beg >> 14
    assert lc.end % 16384 == 0  # a sum one over touches one more window; a much smaller one, fewer
    assert lc.bin not in (by["before_long"].bin, by["after_long"].bin)
    for lab in ("placed_unmapped", "clips_only", "no_cigar"):
        assert by[lab].end == by[lab].pos + 1
    e = by["ends_member"]
    assert e.vend & 0xffff == 0 and e.vend >> 16 > e.vbeg >> 16
    assert e.vend == by[labels[labels.index("ends_member") + 1]].vbeg
    # bin 4681 of c2: A1 and A2 meet in one member (one chunk), A3 starts in a later one
    assert by["b1"].vbeg >> 16 == by["a2_0"].vbeg >> 16
    assert by["b2_499"].vend >> 16 > by["b2_0"].vbeg >> 16
    refs, nnc = bai_ref.parsed(want.bytes)
    assert nnc == 3 and refs[1] == ({}, None, []) and refs[3] == ({}, None, [])
    a = refs[2][0][4681]
    assert len(a) == 2 and a[0] == (by["a1_0"].vbeg, by["a2_1"].vend) and a[1][0] == by["a3_0"].vbeg
    assert 585 in refs[2][0]
    assert refs[2][1][1] == (2 + 2 + 2 + 501, 0)
    assert refs[0][1][1] == (len([r for r in want.records if r.ref_id == 0]) - 1, 1)


@gpu
@pytest.mark.parametrize("eager", [False, True])
def test_hand_corpus(ctx, hand, eager):
    _, data = hand
    check_all(ctx, data, eager)


@gpu
def test_hand_corpus_windowed(ctx, hand):
    _, data = hand
    assert sb.build_bai(data, ctx=ctx, window=20000) == bai_ref.build(data).bytes


# ------------------------------------------------------------------ kernel shapes

def shaped(n, change_at=(), every=False):
    """n records on c0; the key changes before each index of change_at (or at every record)."""
    out, w = [], 0
    for i in range(n):
        if every or i in change_at:
            w += 1
        out.append(r_(0, w * 16384 + 100 + (0 if every else i)))
    return bam(out, 700)


SHAPES = [("n%d" % n, n, tuple(range(7, n, 7)), False) for n in (1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1)] + [
    ("change_at_lane_64", 130, (64,), False),
    ("change_at_workgroup_edge", B + 44, (B,), False),
    ("single_run", 2 * B + 1, (), False),
    ("every_record_a_run", 2 * B + 1, (), True),
]


@gpu
@pytest.mark.parametrize("label,n,change_at,every", SHAPES, ids=[s[0] for s in SHAPES])
def test_kernel_shapes(ctx, label, n, change_at, every):
    data = shaped(n, change_at, every)
    want = bai_ref.build(data)
    assert len(want.records) == n
    assert want.runs.size == (n if every else 1 + len(change_at))
    runs, lin, nnc = scan(ctx, data)
    assert same_runs(runs, want.runs), (runs, want.runs)
    assert np.array_equal(lin, want.lin) and nnc == 0
    assert sb.build_bai(data, ctx=ctx) == want.bytes


# Long CIGARs (the wave-cooperative sum of k_bai_keys: more than 32 ops) at chosen lanes: lane 0,
# two in one wave, the last lane of a wave, lane 0 of the next wave, around the threshold (32 ops
# stay in the lane) and far above it.  Every op count comes twice: once ending on a window's first
# position (any sum that is too small loses the window) and once on a window's last (any sum that
# is too large gains one).  Each record reaches one window further than the one before, so it is
# the first record of its last window and the linear index shows the error.
COOP = ((0, 33, "first"), (1, 33, "last"), (37, 3000, "last"), (38, 3000, "first"), (50, 32, "first"),
        (51, 32, "last"), (63 + 64, 64, "first"), (128, 65, "last"), (129, 65, "first"), (130, 64, "last"),
        (140, 4097, "first"), (141, 4097, "last"))


def coop_stream():
    out = []
    for i in range(200):
        pos = 100 + i
        hit = [(n, c) for n, c in enumerate(COOP) if c[0] == i]
        if hit:
            (n, (_, nops, kind)), = hit
            w = 2 + n  # the window the record reaches
            end = w * 16384 + 1 if kind == "first" else (w + 1) * 16384
            out.append(r_(0, pos, spread_cigar(nops, end - pos)))
        else:
            out.append(r_(0, pos))
    return bam(out, 700)


def test_coop_stream_pins_every_long_sum():
    want = bai_ref.build(coop_stream())
    for i, nops, kind in COOP:
        r = want.records[i]
        assert r.end - r.pos > 16384 and r.bin != bai_ref.reg2bin(r.pos, r.pos + 1)
        assert r.end % 16384 == (1 if kind == "first" else 0)
        # the first record to touch its last window, and it stops there
        w = r.end - 1 >> 14
        assert min((x for x in want.records if x.beg >> 14 <= w <= x.end - 1 >> 14), key=lambda x: x.vbeg) == r
        assert int(want.lin[w]) == r.vbeg and int(want.lin[w + 1]) != r.vbeg


@gpu
def test_cooperative_cigar_sum(ctx):
    data = coop_stream()
    want = bai_ref.build(data)
    runs, lin, nnc = scan(ctx, data)
    assert same_runs(runs, want.runs), (runs, want.runs)
    assert np.array_equal(lin, want.lin) and nnc == 0


# ------------------------------------------------------------------ ordering and malformed

def _vbeg(data, k):
    return bai_ref.records_of(data)[0][k].vbeg


@gpu
@pytest.mark.parametrize("label,records,bad", [
    ("pos_decreasing", [r_(0, 100), r_(0, 200), r_(0, 150), r_(0, 300)], 2),
    ("ref_decreasing", [r_(0, 100), r_(2, 200), r_(0, 300)], 2),
    ("mapped_after_no_ref", [r_(0, 100), r_(-1, -1, (), flag=4), r_(2, 300), r_(2, 400)], 2),
])
def test_unsorted_input_is_refused(ctx, label, records, bad):
    data = bam(records)
    with pytest.raises(sb.SparkBamError) as e:
        scan(ctx, data)
    assert e.value.code == E_UNSORTED
    assert e.value.fields == (_vbeg(data, bad),)
    with pytest.raises(sb.SparkBamError) as e:
        sb.build_bai(data, ctx=ctx)
    assert e.value.code == E_UNSORTED


@gpu
def test_windowed_build_checks_order_across_seams(ctx):
    # sorted inside each ~1 KB window, but the third window restarts at a lower position
    fill = b"XZZ" + bytes(random.Random(5).randrange(1, 256) for _ in range(150)) + b"\0"
    recs = [r_(0, 1000 + k, aux=fill) for k in range(30)] + [r_(0, 500 + k, aux=fill) for k in range(30)]
    data = bam(recs)
    with pytest.raises(sb.SparkBamError) as e:
        sb.build_bai(data, ctx=ctx, window=1000)
    assert e.value.code == E_UNSORTED


@gpu
def test_ref_id_past_the_dictionary_is_a_bad_record(ctx):
    with pytest.raises(sb.SparkBamError) as e:
        scan(ctx, bam([r_(0, 100), r_(len(CONTIGS), 200)]))
    assert e.value.code == E_BAD_RECORD
    with pytest.raises(sb.SparkBamError) as e:
        scan(ctx, bam([r_(0, 100), r_(2, -1)]))
    assert e.value.code == E_BAD_RECORD


@gpu
def test_off_reference_record_is_bad_even_when_the_shard_end_is_open(ctx):
    """More resident bytes cannot cure ref_id >= n_ref: SBH_E_BAD_RECORD, never SBH_E_NEED_HALO."""
    fill = b"XZZ" + bytes(random.Random(7).randrange(1, 256) for _ in range(150)) + b"\0"
    data = bam([r_(0, 100), r_(len(CONTIGS), 200)] + [r_(2, 300 + k, aux=fill) for k in range(20)])
    blocks, _ = bai_ref.members(data)
    cut = blocks[len(blocks) // 2][0]  # a member start well past the bad record, before the end
    sh = ctx.shard(np.frombuffer(data[:cut], np.uint8), file_offset=0, file_size=len(data))
    try:
        sh.index(0)
        sh.inflate()
        _, lens, hdr_end = sb.bam_header(sh)
        sh.set_contigs(lens)
        with pytest.raises(sb.SparkBamError) as e:
            sh.bai_scan(hdr_end, sh.flat_size)
        assert e.value.code == E_BAD_RECORD
    finally:
        sh.close()


# ------------------------------------------------------------------ end to end

@gpu
@pytest.mark.parametrize("text", ["1:0-100000", "1:13000-14000,1:60000-61000", "1:2000000-3000000"])
def test_load_bam_intervals_with_a_built_index(ctx, text):
    path = golden_bam("2.bam")
    want = sb.load_bam_intervals(path, text, ctx=ctx)
    got = sb.load_bam_intervals(path, text, ctx=ctx, bai="build")
    assert np.array_equal(got.reads.cols["vpos"], want.reads.cols["vpos"])
    assert got.counts == want.counts and len(got.reads) == len(want.reads)
