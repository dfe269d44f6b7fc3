"""Checker conformance on the GPU: the hand-built probes of checker_corpus.py through k_eager,
k_full and everything that serves their results (Shard.check_eager / check_full / run, the
windowed checkers), at every position against the CPU oracle and, at the probes' first bytes,
against the literals written down from the Scala.  test_checker_corpus_cpu.py holds the oracle to
the same literals.

The layouts put every probe on a 16-byte grid (plus a shift), so a call's `begin` decides where in
a tile the probe lies: the offset tests compute each probe's tile offset from `begin` themselves
and assert which (probe, offset class) pairs were met, and that the probe's tile was a fast tile
of k_full on `long` and not on `short`."""
import functools

import numpy as np
import pytest

import checker_corpus as cc
from oracle_lib import OR_OK
from pkg import sb

pytestmark = pytest.mark.gpu

SBH_E_HIP, SBH_E_NEED_HALO = sb._lib.SBH_E_HIP, sb._lib.SBH_E_NEED_HALO
assert SBH_E_NEED_HALO == 17
RTCS = (0, 1, 2, 3, 10)
SHIFTS = (0, 1, 12, 15)                   # full tile offsets 0 / 16, 1, 8192 - 36, 15 / 8191 (mod 16)
EAGER_CLASSES = (0, 1, cc.ETILE - 1)
FULL_CLASSES = (0, 1, 15, 16, cc.FTILE - 1, cc.FTILE - 36)


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
def file_of(kind, ctg, shift=0, payload=65280, level=6):
    lay = cc.layout(kind, ctg, shift) if kind != "end" else cc.end_layout(ctg)
    return np.frombuffer(cc.compress(lay, payload, level), np.uint8).copy()


@functools.lru_cache(maxsize=None)
def want(kind, ctg, shift=0, rtc=10):
    """(eager bools, full words) of the oracle at every flat position of the layout, segment by
    segment (they do not depend on a call's range)."""
    lay = cc.layout(kind, ctg, shift) if kind != "end" else cc.end_layout(ctg)
    e, w = [], []
    for of, _ in cc.oracles(lay):
        _, bits = of.eager_range(0, of.flat_size, rtc)
        e.append(np.unpackbits(bits, bitorder="little")[:of.flat_size].astype(bool))
        if "OPS11" in lay.sections and rtc not in (0, 10):
            # every OPS11 position fails in its first record (a 17476-byte CIGAR each, seconds of
            # oracle time): such a word is the same for every readsToCheck >= 1 (full/Checker.scala:27-28)
            a, z = lay.sections["OPS11"]
            z -= cc.OPS11_CIGAR_AT
            w10 = want(kind, ctg, shift, 10)[1][a:z]
            assert int(w10.max()) < 1 << cc.N_SHIFT
            w += [of.full_range(0, a, rtc, want_words=True)[3], w10,
                  of.full_range(z, of.flat_size, rtc, want_words=True)[3]]
        else:
            w.append(of.full_range(0, of.flat_size, rtc, want_words=True)[3])
    return np.concatenate(e), np.concatenate(w)


@pytest.fixture(scope="module")
def shard(ctx):
    """shard(kind, ctg, shift): the layout resident, indexed and inflated (one per module)."""
    cache = {}

    def get(kind, ctg, shift=0, payload=65280, level=6):
        key = (kind, ctg, shift, payload, level)
        if key not in cache:
            lay = cc.layout(kind, ctg, shift) if kind != "end" else cc.end_layout(ctg)
            sh = ctx.shard(file_of(*key))
            _, fs = call(sh.index, 0)
            call(sh.inflate)
            assert fs == len(lay.flat)
            call(sh.set_contigs, np.asarray(lay.contigs, np.int32))
            cache[key] = sh
        return cache[key]

    yield get
    for sh in cache.values():
        sh.close()


def eager_of(sh, begin, end, rtc=10):
    n, bits = call(sh.check_eager, begin, end, rtc)
    got = np.unpackbits(bits, bitorder="little")[:end - begin].astype(bool)
    assert n == int(got.sum())
    return got


def words_of(sh, begin, end, rtc=10):
    return call(sh.check_full, begin, end, rtc, want_words=True, close_cap=0)["words"]


def same(got, ref, begin, what):
    d = np.flatnonzero(got != ref)
    assert d.size == 0, f"{what}: {d.size} positions differ, first at flat {begin + int(d[0])}: " \
                        f"{int(got[d[0]]):#x} vs {int(ref[d[0]]):#x}"


def begins(lay, n_random=12):
    """About 30 range starts: tile edges, the first probe, the sections, and some anywhere."""
    size, first = len(lay.flat), lay.probes[0][1]
    out = {0, 1, 15, 16, 17, cc.FTILE - 1, cc.FTILE, cc.ETILE - 1, cc.ETILE, first - 1, first, first + 1,
           first - cc.ETILE + 1, first - cc.EW, first - cc.EW + 1}
    for a, b in lay.sections.values():
        out |= {a - 1, a, a + 1, a + 17}
    rng = np.random.default_rng(len(lay.flat))
    out |= set(int(x) for x in rng.integers(0, size - 64, n_random))
    return sorted(x for x in out if 0 <= x < size)


# ------------------------------------------------------------------------------ whole streams
@pytest.mark.parametrize("kind,ctg", [(k, c) for k in ("long", "short", "segmented") for c in ("BIG", "SMALL")])
def test_every_position_over_many_begins(shard, kind, ctg):
    """check_eager and check_full from ~30 `begin` values to the stream's end (and to ends inside
    tiles): every position equals the oracle, every probe start the literal."""
    lay, sh = cc.layout(kind, ctg), shard(kind, ctg)
    e_ref, w_ref = want(kind, ctg)
    size = len(lay.flat)
    for p, f in lay.probes:                                     # (the literals, once, from the oracle's copy)
        assert int(w_ref[f]) == cc.word(p, 10) and bool(e_ref[f]) == cc.eager(p, 10), p.label
    bs = begins(lay)
    assert len(bs) >= 25
    for k, b in enumerate(bs):
        e = size if k % 3 else min(size, b + 1 + (size - b) * (k % 7 + 1) // 8)
        same(eager_of(sh, b, e), e_ref[b:e], b, f"eager [{b}, {e})")
        same(words_of(sh, b, e), w_ref[b:e], b, f"full [{b}, {e})")


# ------------------------------------------------------------------------------ tile offsets
def header_len(p):
    """Fixed fields + name + CIGAR of the probe's first record, as its header says."""
    rnl, nc = p.data[12], int.from_bytes(p.data[16:18], "little")
    return 36 + rnl + 4 * nc


def chain_starts(p):
    """Starts, relative to the probe, of the records a passing probe's chain reads (in step)."""
    if p.how[0] != "more" or p.tags.get("abnormal"):
        return []
    return [len(p.data) + len(cc.MIN) * j for j in range(9)]


def eager_offsets(p, f):
    """{class: tile offset of the probe} for k_eager: the three edges, and for long probes the
    offsets that put a chain record at window offset EW - 1 / EW and the end of name + CIGAR
    exactly at / one byte past the staged bytes (one_record's need - s0 > sn, s0 = t0 & ~15)."""
    out = {c: c for c in EAGER_CLASSES}
    for d in chain_starts(p):
        for name, o in (("chain EW-1", cc.EW - 1 - d), ("chain EW", cc.EW - d)):
            if 0 <= o < cc.ETILE:
                out.setdefault(name, o)
    h = header_len(p)
    for name, n in (("staged exact", cc.ESTAGE), ("staged past", cc.ESTAGE + 1)):
        for o in range(max(0, cc.ESTAGE - h - 32), min(cc.ETILE, cc.ESTAGE - h + 32)):
            if f + h - ((f - o) & ~15) == n and o >= 0:
                out.setdefault(name, o)
    return out


@pytest.mark.parametrize("kind", ["long", "short", "segmented"])
def test_eager_tile_offsets(shard, kind):
    """Every probe at eager tile offsets 0, 1 and 16383 (tiles start at begin + k * 16384), the long
    ones also where their chain crosses the window's end and where their name + CIGAR ends at
    the staged bytes' end."""
    met = set()
    for ctg in ("BIG", "SMALL"):
        lay, sh = cc.layout(kind, ctg), shard(kind, ctg)
        e_ref, _ = want(kind, ctg)
        for p, f in lay.probes:
            for name, o in eager_offsets(p, f).items():
                b, e = f - o, min(len(lay.flat), f + 48)
                assert b >= 0 and (f - b) % cc.ETILE == o
                got = eager_of(sh, b, e)
                same(got, e_ref[b:e], b, f"{p.label} at eager tile offset {o}")
                assert bool(got[f - b]) == cc.eager(p, 10), p.label
                met.add((p.label, name))
    for ctg in ("BIG", "SMALL"):
        for p, _ in cc.layout(kind, ctg).probes:
            assert all((p.label, c) in met for c in EAGER_CLASSES), p.label
    classes = {c for _, c in met}
    assert classes >= {"chain EW-1", "chain EW", "staged exact", "staged past"}, classes


def full_offsets(p, shift):
    """{class: tile offset} a layout of this shift can give the probe in k_full (tiles start at
    (begin & ~15) + k * 8192): the six edges, for long probes the offsets that put their last op at
    FSN - 4 and at FSN, for passing ones the one where a later record of the chain starts past
    FSN - 299 (chain_full's FULL_SLOW exit)."""
    out = {c: c for c in FULL_CLASSES if c % 16 == shift}
    h = header_len(p)
    for name, o in (("last op FSN-4", cc.FSN - h), ("last op FSN", cc.FSN + 4 - h)):
        if 0 <= o < cc.FTILE and o % 16 == shift and h > 36 + 255:
            out[name] = o
    o = cc.FTILE - 16 + shift
    if any(o + d + 36 + 255 + 8 > cc.FSN for d in chain_starts(p)):
        out["chain past FSN-299"] = o
    return out


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kind", ["long", "short"])
def test_full_tile_offsets(shard, kind, shift):
    """Every probe at full tile offsets 0, 1, 15, 16, 8191 and 8192 - 36 (one layout per residue
    mod 16), over exactly its tile and the next: fast tiles on `long`, none on `short`."""
    met = set()
    for ctg in ("BIG", "SMALL"):
        lay, sh = cc.layout(kind, ctg, shift), shard(kind, ctg, shift)
        _, w_ref = want(kind, ctg, shift)
        size = len(lay.flat)
        for p, f in lay.probes:
            assert f % 16 == shift
            for name, o in full_offsets(p, shift).items():
                s0 = f - o
                b, e = s0, min(size, s0 + 2 * cc.FTILE)
                assert s0 >= 0 and s0 % 16 == 0
                fast = e - s0 >= cc.FTILE and cc.fast_tile(lay, s0)
                assert fast == (kind == "long"), (p.label, name)
                got = words_of(sh, b, e)
                same(got, w_ref[b:e], b, f"{p.label} at full tile offset {o}")
                assert int(got[f - b]) == cc.word(p, 10), p.label
                met.add((p.label, name))
    for ctg in ("BIG", "SMALL"):
        for p, _ in cc.layout(kind, ctg, shift).probes:
            assert all((p.label, c) in met for c in FULL_CLASSES if c % 16 == shift), p.label
    extra = {12: "last op FSN-4", 0: "last op FSN"}
    if shift in extra:
        assert extra[shift] in {c for _, c in met}
    if shift == 0:
        assert sum(1 for _, c in met if c == "chain past FSN-299") >= 2
    assert {c % 16 for c in FULL_CLASSES} == set(SHIFTS)


def test_ops11_bad_byte_at_the_staged_window_edge(shard):
    """The OPS11 bad bytes at window offsets FSN - 1 and FSN of a fast tile (the last staged byte,
    the first byte only the op index sees), and the section's rule at every clean position."""
    lay, sh = cc.layout("long", "BIG"), shard("long", "BIG")
    _, w_ref = want("long", "BIG")
    a, z = lay.sections["OPS11"]
    bad = cc.ops11_bad(a)
    edge = {x % 1024: x for x in bad}
    for x, off in ((edge[(cc.FSN - 1) % 1024], cc.FSN - 1), (edge[cc.FSN % 1024], cc.FSN)):
        s0 = x - off
        assert s0 % 16 == 0 and s0 >= a and cc.fast_tile(lay, s0)
        got = words_of(sh, s0, s0 + cc.FTILE)
        same(got, w_ref[s0:s0 + cc.FTILE], s0, f"OPS11 bad byte at window offset {off}")
        hit = [p for p in range(s0, s0 + cc.FTILE) if cc.ops11_word(p, bad) != cc.OPS11_WORD]
        assert hit and all(int(got[p - s0]) == cc.OPS11_WORD | cc.BAD_OP for p in hit)
    for b in (a, a + 1, bad[4] - 1024 - 5, bad[5] & ~1023):       # op-index lines start at begin & ~1023
        e = min(z, b + 5 * cc.FTILE)
        same(words_of(sh, b, e), w_ref[b:e], b, f"OPS11 from {b}")


# ------------------------------------------------------------------------------ aggregation
@pytest.mark.parametrize("kind,ctg", [("long", "BIG"), ("short", "BIG"), ("segmented", "BIG"), ("short", "SMALL")])
def test_counts_and_close_calls(shard, kind, ctg):
    """counts, rbe, the success count and the close-call list (as a set) over whole streams and over
    ranges that start and end inside tiles; a tile with more than FCCAP close calls; a close_cap
    smaller than the number of close calls."""
    lay, sh = cc.layout(kind, ctg), shard(kind, ctg)
    size = len(lay.flat)
    ranges = [(0, size), (1, size - 1), (cc.FTILE + 77, size - cc.FTILE - 5), (lay.probes[0][1] + 3, lay.probes[-1][1] + 9)]
    if "CLOSE16" in lay.sections:
        a, b = lay.sections["CLOSE16"]
        ranges += [(a, a + cc.FTILE), (a - 100, b)]
        c16 = cc.tally(want(kind, ctg)[1][a:a + cc.FTILE], a)[3]
        assert len(c16) > cc.FCCAP and cc.fast_tile(lay, a) == (kind == "long")
    for rtc in (10, 1):
        w_ref = want(kind, ctg, 0, rtc)[1]
        for b, e in ranges:
            counts, rbe, ns, close = cc.tally(w_ref[b:e], b)
            r = call(sh.check_full, b, e, rtc)
            assert r["n_success"] == ns, (b, e, rtc)
            assert np.array_equal(r["counts"].astype(np.int64), counts), (b, e, rtc)
            assert np.array_equal(r["rbe"].astype(np.int64), rbe), (b, e, rtc)
            got = list(zip(r["close_flat"].tolist(), r["close_word"].tolist()))
            assert r["n_close"] == len(close) == len(got) and set(got) == close, (b, e, rtc)
    counts, rbe, ns, close = cc.tally(want(kind, ctg)[1], 0)
    cap = len(close) // 2
    assert cap > 0
    r = call(sh.check_full, 0, size, 10, close_cap=cap)
    got = list(zip(r["close_flat"].tolist(), r["close_word"].tolist()))
    assert r["n_close"] == len(close) and len(got) == cap and len(set(got)) == cap and set(got) <= close
    assert np.array_equal(r["counts"].astype(np.int64), counts) and r["n_success"] == ns


@pytest.mark.parametrize("rtc", RTCS)
@pytest.mark.parametrize("kind", ["long", "short", "segmented"])
def test_reads_to_check(shard, kind, rtc):
    lay, sh = cc.layout(kind, "BIG"), shard(kind, "BIG")
    e_ref, w_ref = want(kind, "BIG", 0, rtc)
    size = len(lay.flat)
    for p, f in lay.probes:
        assert int(w_ref[f]) == cc.word(p, rtc) and bool(e_ref[f]) == cc.eager(p, rtc), (p.label, rtc)
    for b, e in ((0, size), (lay.probes[0][1] - 5, size - 3)):
        same(eager_of(sh, b, e, rtc), e_ref[b:e], b, f"eager rtc {rtc}")
        same(words_of(sh, b, e, rtc), w_ref[b:e], b, f"full rtc {rtc}")


# ------------------------------------------------------------------------------ ends of streams
@pytest.mark.parametrize("label", [p.label for p in cc.END_CASES])
def test_end_of_stream_cases(ctx, label):
    """Each end case at the end of a segment closed by an empty member and at the end of the file."""
    lay = cc.end_layout(label)
    sh = ctx.shard(file_of("end", label))
    try:
        _, fs = call(sh.index, 0)
        call(sh.inflate)
        assert fs == len(lay.flat)
        call(sh.set_contigs, np.asarray(lay.contigs, np.int32))
        for rtc in (10, 1, 2, 3):
            e_ref, w_ref = want("end", label, 0, rtc)
            for b in (lay.probes[1][1] - 3, lay.probes[0][1], 1, 0):
                got_e, got_w = eager_of(sh, b, fs, rtc), words_of(sh, b, fs, rtc)
                same(got_e, e_ref[b:], b, f"{label} eager rtc {rtc}")
                same(got_w, w_ref[b:], b, f"{label} full rtc {rtc}")
            for p, f in lay.probes:     # (got_*: the whole stream, from 0)
                assert int(got_w[f]) == cc.word(p, rtc) and bool(got_e[f]) == cc.eager(p, rtc), (label, rtc)
    finally:
        sh.close()


# ------------------------------------------------------------------------------ windowed checkers
WINDOW, HALO = 4096, 8192                   # a window owns one stored 4096-byte member: a seam every 4096 positions
MIN_LOADS = {"BIG": 5, "SMALL": 2}          # (a window starts at the first block asked for: the probes' first)
NRS_PARTS = 4


@functools.lru_cache(maxsize=None)
def around_probes(ctg):
    """Flat positions within 40 of a probe start of short/<ctg>, in order, with their Pos."""
    lay = cc.layout("short", ctg)
    (of, _), = cc.oracles(lay, 4096, 0)
    flats = sorted({x for _, f in lay.probes for x in range(f - 40, f + 41) if 0 <= x < len(lay.flat)})
    return of, flats, [sb.Pos(*of.pos_of(x)) for x in flats]


@pytest.mark.parametrize("ctg", ["BIG", "SMALL"])
def test_windowed_eager_checker(ctx, ctg):
    from spark_bam_amd.checkers import WindowedEagerChecker
    lay = cc.layout("short", ctg)
    of, flats, poss = around_probes(ctg)
    e_ref, _ = want("short", ctg)
    with WindowedEagerChecker(file_of("short", ctg, 0, 4096, 0), np.asarray(lay.contigs, np.int32), window=WINDOW,
                              halo=HALO, ctx=ctx) as ck:
        got = np.array([ck.apply(p) for p in poss])
        assert ck.loads >= MIN_LOADS[ctg], "probes should straddle window seams"
    same(got, e_ref[flats], 0, "WindowedEagerChecker.apply")
    at = {f: i for i, f in enumerate(flats)}
    for p, f in lay.probes:
        assert bool(got[at[f]]) == cc.eager(p, 10), p.label


@pytest.mark.parametrize("ctg", ["BIG", "SMALL"])
def test_windowed_full_checker(ctx, ctg):
    from spark_bam_amd.checkers import WindowedFullChecker
    lay = cc.layout("short", ctg)
    of, flats, poss = around_probes(ctg)
    _, w_ref = want("short", ctg)
    with WindowedFullChecker(file_of("short", ctg, 0, 4096, 0), np.asarray(lay.contigs, np.int32), window=WINDOW,
                             halo=HALO, ctx=ctx) as ck:
        got = np.array([ck.apply(p) for p in poss], np.uint32)
        assert ck.loads >= MIN_LOADS[ctg]
    same(got, w_ref[flats], 0, "WindowedFullChecker.apply")
    at = {f: i for i, f in enumerate(flats)}
    for p, f in lay.probes:
        assert int(got[at[f]]) == cc.word(p, 10), p.label


@pytest.mark.parametrize("ctg,part", [("BIG", k) for k in range(NRS_PARTS)] + [("SMALL", 0)])
def test_windowed_next_read_start(ctx, ctg, part):
    """next_read_start_with_delta from every probe start and the 40 positions either side (the
    search begins inside probes and runways, skips failing probes, crosses window seams): Pos and
    delta are the oracle's FindRecordStart, and the delta at a probe start is 0 exactly where the
    literal says the probe passes.  (BIG: the positions in NRS_PARTS consecutive runs.)"""
    from spark_bam_amd.checkers import WindowedEagerChecker
    lay = cc.layout("short", ctg)
    of, flats, poss = around_probes(ctg)
    literal = {f: cc.eager(p, 10) for p, f in lay.probes}
    n = len(flats)
    lo, hi = (0, n) if ctg == "SMALL" else (n * part // NRS_PARTS, n * (part + 1) // NRS_PARTS)
    assert hi - lo >= 1000
    with WindowedEagerChecker(file_of("short", ctg, 0, 4096, 0), np.asarray(lay.contigs, np.int32), window=WINDOW,
                              halo=HALO, ctx=ctx) as ck:
        for x, pos in zip(flats[lo:hi], poss[lo:hi]):
            rc, flat, d = of.find_record_start(x)
            got = ck.next_read_start_with_delta(pos)
            if rc == OR_OK:
                assert got is not None and got[0] == sb.Pos(*of.pos_of(flat)) and got[1] == d, (x, got, flat, d)
            else:
                assert got is None, (x, got)
            if x in literal:
                assert (rc == OR_OK and d == 0) == literal[x], x
        assert ck.loads >= 2


# ------------------------------------------------------------------------------ the pipelined run
@pytest.mark.parametrize("min_blocks", [1, 2])
@pytest.mark.parametrize("payload", [4096, 97])
@pytest.mark.parametrize("ctg", ["BIG", "SMALL"])
def test_pipelined_run(ctx, ctg, payload, min_blocks, monkeypatch):
    """run() checks behind the inflate frontier, batch by batch: with 4096- and 97-byte members
    frontiers fall inside probes (positions deferred past the frontier, the long-record queue); its
    bitmap is the oracle's.  run() reports neither count, so what is asserted is what makes them
    run: by the shard's own block table a member ends strictly inside the first record of a
    passing probe and, with BIG, inside that of a long candidate (block_size 2048, >= 32 ops)."""
    monkeypatch.setenv("SBH_PIPE_MIN_BLOCKS", str(min_blocks))
    lay = cc.layout("short", ctg)
    data = file_of("short", ctg, 0, payload)
    e_ref, _ = want("short", ctg)
    sh = ctx.shard(data)
    try:
        call(sh.set_contigs, np.asarray(lay.contigs, np.int32))
        r = call(sh.run, 0, data.size)
        assert r["flat_bytes"] == len(lay.flat)
        bits = call(sh.eager_bits, 0, len(lay.flat))
        call(sh.index, 0)                                       # (the block table, for the host)
        edges = sorted({int(b[3]) for b in sh.blocks()})
        assert len(edges) >= len(lay.flat) // payload
        cut = [p.label for p, f in lay.probes if p.how[0] == "more" and any(f < x < f + len(p.data) for x in edges)]
        assert cut, "no member ends inside a passing probe"
        assert ctg == "SMALL" or any(c.startswith("long_bs2048") for c in cut), cut
        got = np.unpackbits(bits, bitorder="little")[:len(lay.flat)].astype(bool)
        same(got, e_ref, 0, f"run() bitmap, payload {payload}, batches of {min_blocks}")
        assert r["n_true"] == int(e_ref.sum())
        for p, f in lay.probes:
            assert bool(got[f]) == cc.eager(p, 10), p.label
    finally:
        sh.close()


# ------------------------------------------------------------------------------ open ends
def test_open_ended_shards_never_answer_differently(ctx, shard):
    """Byte-range shards of `long` whose last member ends inside a passing probe's fixed fields,
    its name, between its ops, inside an op, and inside OPS11: a check over any range either asks
    for more halo (SBH_E_NEED_HALO) or equals the whole file's; a range holding the start of the
    probe the halo cuts must ask."""
    lay = cc.layout("long", "BIG")
    e_ref, w_ref = want("long", "BIG")
    at = {p.label: f for p, f in lay.probes}
    f = at["cigar9"]                       # 36 fixed bytes, 'A\0', nine ops, then its runway
    a11 = lay.sections["OPS11"][0]
    cuts = {"fixed fields": f + 20, "name": f + 37, "between ops": f + 38 + 8, "inside an op": f + 38 + 10,
            "OPS11": a11 + 50001}
    data = np.frombuffer(cc.compress(lay, 65280, 6, tuple(cuts.values())), np.uint8).copy()
    whole = ctx.shard(data)
    shards = []
    try:
        call(whole.index, 0)
        ends = {b[3]: b[0] for b in whole.blocks()}            # flat start of a member -> its file offset
        for where, cut in cuts.items():
            sh = ctx.shard(data[:ends[cut]], file_offset=0, file_size=data.size)
            shards.append(sh)
            _, fs = call(sh.index, 0)
            call(sh.inflate)
            assert fs == cut
            call(sh.set_contigs, np.asarray(lay.contigs, np.int32))
            probe = f if cut < a11 else None
            ranges = [(0, cut), (cut - 30000, cut), (cut - 5000, cut - 40), (cut - 20000, cut - 4500),
                      (cut - 64, cut), (cut - 1, cut)]
            if probe is not None:
                ranges += [(probe - 100, probe + 1), (probe, cut), (probe - 100, probe), (probe + 1, cut)]
            asked = answered = 0
            for b, e in ranges:
                for kind in ("eager", "full"):
                    try:
                        got = eager_of(sh, b, e) if kind == "eager" else words_of(sh, b, e)
                    except sb.SparkBamError as err:
                        assert err.code == SBH_E_NEED_HALO, (where, b, e, kind, err)
                        asked += 1
                        continue
                    answered += 1
                    assert probe is None or not b <= probe < e, f"{where}: [{b}, {e}) holds the cut probe's start"
                    same(got, (e_ref if kind == "eager" else w_ref)[b:e], b, f"{where}: {kind} [{b}, {e})")
            assert asked >= 4 and answered >= 2, (where, asked, answered)
    finally:
        for sh in shards:
            sh.close()
        whole.close()
