"""Record-chain conformance on the GPU: the hand-built layouts of chain_corpus.py through the
kernels that consume the eager bitmap -- the chain proof (k_verify_chain_w), the first-record
search (k_first_set), the chain marker (k_cm_*), the exact walk (k_chain_walk) and the split
counters (k_split_popcount / k_split_count_cc / k_split_cm_count) -- by way of the public calls
(count_records, chain_from, records, run, split_starts, run_stream).  Every comparison is exact
equality with chain_corpus.walk() / starts(); test_chain_corpus_cpu.py holds those, the declared
set bits and every geometry claim to the CPU oracle."""
import functools

import numpy as np
import pytest

import chain_corpus as cc
from oracle_lib import OR_OK, OracleFile
from pkg import sb

pytestmark = pytest.mark.gpu

SBH_E_HIP = sb._lib.SBH_E_HIP
W, L, C, G, REC = cc.W, cc.L, cc.C, cc.G, cc.REC
ANOMALOUS = tuple(n for n in cc.LAYOUTS if n in cc.BAIT or n == "rejected")
CLASSES = ("bit 0", "bit 31", "lane 0", "lane 63", "first of a chunk", "last of a chunk")


def call(f, *a, **kw):
    """f(*a): a device error ends the session (nothing more runs on this GPU)."""
    try:
        return f(*a, **kw)
    except sb.SparkBamError as e:
        if e.code == SBH_E_HIP:
            pytest.exit("HIP error: %s" % e, returncode=3)
        raise


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def file_of(name, payload=65280, level=1, cuts=()):
    data, offs, flats = cc.compress(cc.layout(name).flat, payload, level, cuts)
    return np.frombuffer(data, np.uint8).copy(), offs, flats


def fresh(ctx, name, payload=65280, level=1, cuts=()):
    lay = cc.layout(name)
    sh = ctx.shard(file_of(name, payload, level, cuts)[0])
    _, fs = call(sh.index, 0)
    call(sh.inflate)
    assert fs == len(lay.flat)
    call(sh.set_contigs, np.asarray(cc.CONTIGS, np.int32))
    return sh


@pytest.fixture(scope="module")
def shard(ctx):
    """shard(name, ...): the layout resident, indexed and inflated (one per module)."""
    cache = {}

    def get(name, payload=65280, level=1, cuts=()):
        key = (name, payload, level, cuts)
        if key not in cache:
            cache[key] = fresh(ctx, *key)
        return cache[key]

    yield get
    for sh in cache.values():
        sh.close()


def bitmap(sh, lay, begin=0):
    """check_eager over [begin, total) at the layout's readsToCheck; the bitmap is the declared one."""
    total = len(lay.flat)
    n, bits = call(sh.check_eager, begin, total, lay.rtc)
    got = np.flatnonzero(np.unpackbits(bits, bitorder="little")[:total - begin]) + begin
    assert tuple(got.tolist()) == tuple(p for p in lay.bits if p >= begin) and n == got.size


def sweep(sh, lay, pairs, decode_every=0):
    """[(first, E, count, (count, exit))] of the device, each equal to walk()."""
    out = []
    for k, (f, e) in enumerate(pairs):
        want = cc.walk(lay.flat, f, e)
        n = call(sh.count_records, f, e)
        assert n == want[0], f"{lay.name}: count_records({f}, {e}) = {n}, the walk counts {want[0]}"
        got = call(sh.chain_from, f, e)
        assert got == want, f"{lay.name}: chain_from({f}, {e}) = {got}, the walk gives {want}"
        if decode_every and k % decode_every == 0 and want[0]:
            flat = call(sh.records, f, e)["flat"]
            assert [int(x) for x in flat] == cc.starts(lay.flat, f, e), (lay.name, f, e)
        out.append((f, e, n, got))
    return out


# ------------------------------------------------------------------------------ proof and fallbacks
MODES = [(n, m) for n in cc.LAYOUTS for m in (("peel", "doubling") if n in ANOMALOUS else ("default",))]


@pytest.mark.parametrize("name,marking", MODES)
def test_ranges_at_every_edge(shard, name, marking, monkeypatch):
    """count_records, chain_from and (on every 7th range) the decoded records' starts over the
    layout's edge sweep; layouts with false positives or rejected records under both markers."""
    if marking != "default":
        monkeypatch.setenv("SBH_CM_DOUBLING", "1" if marking == "doubling" else "0")
    lay, sh = cc.layout(name), shard(name)
    bitmap(sh, lay)
    # (a cut last record does not decode, nor does short_step's record of block_size 4)
    whole = name not in cc.TAIL and not name.startswith("tail_overhang") and name != "short_step"
    sweep(sh, lay, cc.edges(lay), decode_every=7 if whole else 0)


def test_hand_worked_literals(shard, monkeypatch):
    lay, sh = cc.layout("hand_worked"), shard("hand_worked")
    for dbl in ("0", "1"):
        monkeypatch.setenv("SBH_CM_DOUBLING", dbl)
        bitmap(sh, lay)
        for (f, e), want in cc.HAND_CASES.items():
            assert call(sh.count_records, f, e) == want[0], (f, e)
            assert call(sh.chain_from, f, e) == want, (f, e)


@pytest.mark.parametrize("name", ["word_edges", "empty_waves", "bait_first_word", "first_at_32767", "first_at_32768"])
def test_first_record_search_at_every_edge(shard, name):
    """find_record_start (k_first_set over the resident bitmap) from one before, at and one past
    every edge record and marked position: the next declared set bit, whether it lies in the same
    word (behind or ahead of `from`), in the next, or chunks away."""
    lay, sh = cc.layout(name), shard(name)
    bitmap(sh, lay)
    bits = np.asarray(lay.bits)
    froms = {0, lay.bits[0] - 1}
    for s in cc.edge_records(lay) + cc.marked(lay):
        froms |= {s - 1, s, s + 1}
    same_word = 0
    for p in sorted(f for f in froms if 0 <= f <= lay.bits[-1]):
        want = int(bits[np.searchsorted(bits, p)])
        same_word += any(q // W == p // W and q < p for q in lay.bits[max(0, np.searchsorted(bits, p) - 1):][:1])
        assert call(sh.find_record_start, p, lay.rtc) == (want, want - p), p
    assert same_word >= 3                       # a set bit before `from` in from's own word


# ------------------------------------------------------------------------------ begin != 0
def classes_met(lay, begin, firsts):
    met = set()
    recs = set(cc.edge_records(lay, begin))
    ch = [s for s in lay.chain if s >= begin]
    for f in firsts:
        assert f in recs
        q, i = f - begin, ch.index(f)
        met |= {c for c, on in (("bit 0", q % W == 0), ("bit 31", q % W == W - 1), ("lane 0", cc.lane_of(f, begin) == 0),
                                ("lane 63", cc.lane_of(f, begin) == cc.WAVE - 1),
                                ("first of a chunk", i == 0 or (ch[i - 1] - begin) // C != q // C),
                                ("last of a chunk", i + 1 == len(ch) or (ch[i + 1] - begin) // C != q // C)) if on}
    return met


@pytest.mark.parametrize("name", ["word_edges", "empty_lanes", "empty_waves", "bait_joins", "bait_first_word"])
def test_a_bitmap_that_does_not_begin_at_0(shard, name):
    """The word, lane and chunk grid is anchored at the bitmap's `begin`: the same sweep after
    check_eager(b, total) for b around a word and a chunk edge and at a record in mid-file, over
    the records that lie on the SHIFTED grid's edges; which edge classes each shift met is asserted
    from the declared bits."""
    lay, sh = cc.layout(name), shard(name)
    mid = lay.chain[len(lay.chain) // 2]
    met = {}
    for b in (1, 31, 32, 33, C - 1, C, C + 1, mid):
        if b >= lay.chain[-3]:
            continue
        bitmap(sh, lay, b)
        pairs = cc.edges(lay, b, n_first=4, n_end=4, cap=120)
        assert pairs and all(f >= b and e >= b for f, e in pairs)
        sweep(sh, lay, pairs)
        recs = set(cc.edge_records(lay, b))
        met[b] = classes_met(lay, b, {f for f, _ in pairs if f in recs})
        assert met[b] >= {"first of a chunk", "last of a chunk"}, (b, met[b])
    assert len(met) >= 4
    if name == "word_edges":        # a record on bit 31 of begin 0's grid is on bit 0 of begin 31's, and so on
        assert set().union(*met.values()) == set(CLASSES), met
        assert "bit 0" in met[31] | met[C - 1] and "bit 31" in met[1] | met[33] | met[C + 1], met


# ------------------------------------------------------------------------------ sbh_run_shard's tail
def expect_run(lay, offs, flats):
    first, total = lay.bits[0], len(lay.flat)
    n, x = cc.walk(lay.flat, first, total)
    return {"count": n, "exit_flat": x, "n_true": len(lay.bits), "first_vpos": cc.vpos_of(first, offs, flats),
            "flat_bytes": total}


@pytest.mark.parametrize("name", list(cc.LAYOUTS))
def test_run_shard(ctx, name):
    """run(0, size): k_first_set -> k_verify_chain_w from the device's first record, with the chunk
    counts; first_at_*: the first set bit is the last bit of a k_first_set span, or the first of
    the next."""
    lay = cc.layout(name)
    data, offs, flats = file_of(name)
    sh = fresh(ctx, name)
    try:
        r = call(sh.run, 0, data.size, lay.rtc)
        want = expect_run(lay, offs, flats)
        assert r["status"] == 0 and {k: r[k] for k in want} == want
        from_first = lay.bits == tuple(cc.starts(lay.flat, lay.bits[0], len(lay.flat)))
        assert (r["anomalies"] == 0) == from_first, r["anomalies"]
        assert from_first == (name not in ANOMALOUS and lay.clean)
    finally:
        sh.close()


def test_grid_wrap(ctx):
    """More bitmap words than one trip of the proof's grid covers (2048 workgroups x 1024 words), the
    first record past k_first_set's first trip (256 workgroups x 1024 words): run() and ranges that
    end on either side of the second trip's first chunk.  76 MB of flat bytes, the one large case:
    0.14 s on an MI355X, building and compressing the stream included."""
    lay = cc.layout("grid_wrap")
    data, offs, flats = cc.compress(lay.flat)
    data = np.frombuffer(data, np.uint8)
    total, first = len(lay.flat), cc.GRID_FIRST
    sh = ctx.shard(data)
    try:
        call(sh.set_contigs, np.asarray(cc.CONTIGS, np.int32))
        r = call(sh.run, 0, data.size)
        want = expect_run(lay, offs, flats)
        assert want["count"] == cc.GRID_N and want["exit_flat"] == total
        assert r["status"] == 0 and {k: r[k] for k in want} == want and r["anomalies"] == 0
        trip = first // C * C + cc.PROOF_GRID * G                       # the second trip's first position
        k = (trip - first) // cc.GRID_REC
        assert 0 < k < cc.GRID_N - 2
        a, b = lay.chain[k], lay.chain[k + 1]
        assert a < trip <= b
        pairs = [(first, total), (first, a), (first, a + 1), (first, b), (first, b + 1), (first, trip), (a, total),
                 (b, total), (lay.chain[1], lay.chain[-1]), (lay.chain[-1], total + 100), (lay.chain[3], b + 1)]
        for f, e in pairs:
            i, j = (f - first) // cc.GRID_REC, min(cc.GRID_N, -(-(min(e, total) - first) // cc.GRID_REC))
            assert cc.walk(lay.flat, f, e) == (j - i, min(total, first + cc.GRID_REC * j))     # (from construction)
        sweep(sh, lay, pairs)
        assert call(sh.find_record_start, 0)[0] == first
    finally:
        sh.close()
        cc.grid_wrap.cache_clear()


# ------------------------------------------------------------------------------ split counts
def check_splits(sh, of, lay, splits, offs, flats, labels):
    status, v, n, n_host = call(sh.split_starts, splits)
    for i, (s, e) in enumerate(splits):
        x1, x2 = flats[offs.index(s)], (flats[offs.index(e)] if e in offs else len(lay.flat))
        first = next((p for p in lay.bits if p >= x1), None)
        assert first is not None
        want = cc.walk(lay.flat, first, x2)[0]
        assert int(status[i]) == 0 and int(n[i]) == want, (labels[i], x1, x2, int(status[i]), int(n[i]), want)
        assert want == 0 or int(v[i]) == cc.vpos_of(first, offs, flats), labels[i]
        v1, n1 = call(sh.split, s, e, 5, lay.rtc)
        assert (n1, v1 if n1 else 0) == (want, int(v[i]) if n1 else 0), labels[i]
        rc, vr, nr = of.split(s, e, reads_to_check=lay.rtc)
        assert rc == OR_OK and nr == want and (nr == 0 or vr == int(v[i])), labels[i]
    return n_host


def splits_of(cases, offs, flats, total, size):
    at = {f: o for f, o in zip(flats, offs)}
    return [(at[x1], at[x2] if x2 < total else size) for x1, x2 in cases.values()], list(cases)


def test_split_counts_from_chunk_counts(ctx, monkeypatch):
    """split_starts after run() on dense_edges in 300-byte members: ranges whose first and last word
    lie in one chunk, in adjacent chunks, two chunks apart (no, no and one inner chunk of the proof's
    counts), on chunk edges; all on the device.  Then a run that owns the first 5 chunks only, so
    that splits leave the proven range; then SBH_SPLIT_CC=0: k_split_popcount over more than
    PC_WORDS words."""
    lay = cc.layout("dense_edges")
    total = len(lay.flat)
    cases = dict(cc.dense_edges_splits(), **cc.popcount_splits())
    cuts = tuple(sorted({x for pair in cases.values() for x in pair if x < total} | {5 * C}))
    data, offs, flats = file_of("dense_edges", 300, 1, cuts)
    of = OracleFile(data)
    splits, labels = splits_of(cases, offs, flats, total, data.size)
    sh = fresh(ctx, "dense_edges", 300, 1, cuts)
    try:
        r = call(sh.run, 0, data.size)
        assert r["count"] == len(lay.chain) and r["anomalies"] == 0
        for _ in range(2):
            assert check_splits(sh, of, lay, splits, offs, flats, labels) == 0
        # a run that owns [0, 5 C): the splits that end past it leave [chain_first, chain_E)
        own = offs[flats.index(5 * C)]
        r = call(sh.run, 0, own)
        assert r["flat_bytes"] == 5 * C and r["count"] == cc.walk(lay.flat, lay.chain[0], 5 * C)[0]
        assert sum(1 for x1, x2 in cases.values() if x2 > 5 * C) >= 3
        check_splits(sh, of, lay, splits, offs, flats, labels)
        monkeypatch.setenv("SBH_SPLIT_CC", "0")
        r = call(sh.run, 0, data.size)
        assert check_splits(sh, of, lay, splits, offs, flats, labels) == 0
    finally:
        sh.close()


def test_split_counts_on_a_marked_chain(ctx):
    """bait_joins in 97-byte members: after run() the chain is marked through the false positives
    (k_split_cm_count): a split whose first record is a marked node, one whose first record is a
    false positive (the per-split path), one that ends inside the bait."""
    lay = cc.layout("bait_joins")
    total, cases = len(lay.flat), cc.marked_splits()
    cuts = tuple(sorted({x for pair in cases.values() for x in pair if x < total}))
    data, offs, flats = file_of("bait_joins", 97, 1, cuts)
    of = OracleFile(data)
    splits, labels = splits_of(cases, offs, flats, total, data.size)
    sh = fresh(ctx, "bait_joins", 97, 1, cuts)
    try:
        r = call(sh.run, 0, data.size)
        assert r["count"] == len(lay.chain) and r["anomalies"] == len(lay.bits) - len(lay.chain)
        n_host = check_splits(sh, of, lay, splits, offs, flats, labels)
        assert 2 <= n_host < len(splits)
    finally:
        sh.close()


# ------------------------------------------------------------------------------ streamed
@pytest.mark.parametrize("name,members", [("dense", 16), ("empty_waves", 16), ("empty_waves", 24), ("bait_joins", 16)])
def test_streamed_run(ctx, name, members):
    """run_stream over stored members of C / 16 bytes.  A window of 16 members: every window edge is
    a chunk edge (in empty_waves some lie between two empty chunks, in bait_joins it lies just
    before the long bait run's host).  A window of 24: every other edge lies in mid-chunk, in
    empty_waves inside empty chunks."""
    lay = cc.layout(name)
    data, offs, flats = file_of(name, C // 16, 0)
    member = offs[1] - offs[0]
    assert all(b - a == member for a, b in zip(offs[:-1], offs[1:-1])) and flats[16] == C
    n_chunks = len(lay.flat) // C
    empty = [k for k in range(n_chunks) if not any(p // C == k for p in lay.bits)]
    edges = [flats[k] for k in range(members, len(flats), members)]
    if members == 16:
        assert all(x % C == 0 for x in edges)
        assert name != "empty_waves" or any(x // C in empty and x // C - 1 in empty for x in edges)
    else:
        assert sum(1 for x in edges if x % C and x // C in empty) >= 2
    want = expect_run(lay, offs, flats)
    s, _ = call(ctx.run_stream, data, np.asarray(cc.CONTIGS, np.int32), index_start=0, window=members * member,
                halo=1 << 20)
    assert s["status"] == 0 and s["n_windows"] >= len(edges)
    keys = ("count", "n_true", "first_vpos", "flat_bytes")
    assert {k: s[k] for k in keys} == {k: want[k] for k in keys}
    sh = fresh(ctx, name, C // 16, 0)
    try:
        r = call(sh.run, 0, data.size)
        assert {k: r[k] for k in keys} == {k: s[k] for k in keys}
    finally:
        sh.close()


# ------------------------------------------------------------------------------ repeatability
@pytest.mark.parametrize("name", ["word_edges", "bait_joins"])
def test_two_fresh_shards_answer_alike(ctx, name):
    """The proof's atomics take a min or add exact integers: two runs on two fresh shards give the
    same tuples."""
    lay = cc.layout(name)
    got = []
    for _ in range(2):
        sh = fresh(ctx, name)
        try:
            bitmap(sh, lay)
            got.append(sweep(sh, lay, cc.edges(lay)))
        finally:
            sh.close()
    assert got[0] == got[1] and len(got[0]) >= 100
