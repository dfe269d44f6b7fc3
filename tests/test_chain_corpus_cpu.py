"""The chain corpus against the CPU oracle (no GPU): every layout's declared set bits are the
oracle's eager bitmap, walk() is the oracle's record chain, the geometry each layout is there for
holds in the declared bits, the hand-worked literals hold, and the copied constants are the
sources'.  test_chain_conformance_gpu.py runs the same layouts through the kernels."""
import functools
import os
import re

import numpy as np
import pytest

import chain_corpus as cc
from oracle_lib import OracleFile
from record_corpus import bgzf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, L, C, G, P, REC = cc.W, cc.L, cc.C, cc.G, cc.P, cc.REC
NAMES = tuple(cc.LAYOUTS)


@functools.lru_cache(maxsize=None)
def oracle(name):
    lay = cc.grid_wrap_prefix() if name == "grid_wrap" else cc.layout(name)
    of = OracleFile(np.frombuffer(bgzf(lay.flat, 65280, 1), np.uint8))
    assert of.flat_size == len(lay.flat) and bytes(of.uncompressed()) == lay.flat
    assert tuple(int(x) for x in of.contig_len) == cc.CONTIGS and of.header_end == lay.chain[0]
    return lay, of


def test_constants_are_the_sources():
    src = {}
    for f in ("sbh_internal.h", "check.hip", "splits.hip"):
        with open(os.path.join(ROOT, "spark-bam_amd", "csrc", f)) as fh:
            src[f] = fh.read()
    for name, f in (("VC_CHUNK", "sbh_internal.h"), ("WPRE_GROUP", "sbh_internal.h"), ("FS_SPAN", "check.hip"),
                    ("CM_PEEL_MAX", "check.hip"), ("PC_WORDS", "splits.hip")):
        m = re.search(r"constexpr uint(?:32|64)_t %s = (\d+);" % name, src[f])
        assert m and int(m.group(1)) == getattr(cc, name), name
    # the proof's launch: 1024 words a workgroup and trip, 2048 workgroups at most; k_first_set's: 256
    m = re.search(r"std::min<uint64_t>\(ngrid\(nw, (\d+)\), (\d+)\);\s*hipLaunchKernelGGL\(k_verify_chain_w", src["check.hip"])
    assert m and (int(m.group(1)), int(m.group(2))) == (cc.PROOF_WG_WORDS, cc.PROOF_GRID)
    m = re.search(r"std::min<uint64_t>\(ngrid\(nw, FS_SPAN\), (\d+)\);\s*hipLaunchKernelGGL\(k_first_set", src["check.hip"])
    assert m and int(m.group(1)) == cc.FS_GRID
    assert re.search(r"constexpr int WAVE = 64;|constexpr uint32_t WAVE = 64;|#define WAVE 64", src["sbh_internal.h"] + src["check.hip"])


@pytest.mark.parametrize("name", NAMES + ("grid_wrap",))
def test_declared_bits_are_the_oracle_s(name):
    lay, of = oracle(name)
    _, bits = of.eager_range(0, of.flat_size, lay.rtc)
    got = np.flatnonzero(np.unpackbits(bits, bitorder="little")[:of.flat_size])
    assert tuple(got.tolist()) == lay.bits
    assert tuple(cc.starts(lay.flat, lay.chain[0], len(lay.flat))) == lay.chain
    assert lay.clean == (lay.bits == lay.chain)
    assert (name in cc.CLEAN) <= lay.clean and not (name in cc.BAIT and lay.clean)


@pytest.mark.parametrize("name", NAMES)
def test_walk_is_the_oracle_s_record_chain(name):
    lay, of = oracle(name)
    pairs = cc.edges(lay)
    assert 40 <= len(pairs) <= 300 and pairs == cc.edges(lay)
    total = len(lay.flat)
    for f, e in pairs:
        ref = [int(x) for x in of.record_chain(f, min(e, total))]
        assert cc.starts(lay.flat, f, e) == ref, (f, e)
        n, x = cc.walk(lay.flat, f, e)
        assert n == len(ref) and f <= x <= total, (f, e)
        # the exit is the chain's next record: the walk from it goes on where this one stopped
        assert x >= min(e, total) or x + 4 > total or n == 0, (f, e, x)
        assert cc.starts(lay.flat, f, total + 1)[:n + 1][-1] in (x, ref[-1] if ref else f), (f, e)


def test_the_sweep_meets_its_edges():
    """edges(): firsts on bit 0 / 31, lanes 0 / 63, first and last of a chunk; E one before, at and one
    past a record, at the stream's last positions, past it, and first + 1."""
    lay = cc.layout("word_edges")
    pairs = cc.edges(lay)
    firsts, total = {f for f, _ in pairs}, len(lay.flat)
    assert {f % W for f in firsts} >= {0, W - 1} and {cc.lane_of(f) for f in firsts} >= {0, cc.WAVE - 1}
    for f in firsts:
        es = {e for g, e in cc.edges(lay, cap=10 ** 6) if g == f}
        assert es >= {f - 1, f, f + 1, total + 100} | {total - k for k in range(6)}, f
    # an E that cuts a word between two set bits
    a, fp = cc.layout("bait_first_word").marks["after"]
    assert any(f == a and a < e <= fp for f, e in cc.edges(cc.layout("bait_first_word")))


def test_hand_worked_literals():
    lay = cc.layout("hand_worked")
    assert (lay.bits, lay.chain, len(lay.flat), lay.rtc) == (cc.HAND_BITS, cc.HAND_CHAIN, cc.HAND_TOTAL, 2)
    assert len(cc.HAND_CASES) >= 10
    for (f, e), want in cc.HAND_CASES.items():
        assert cc.walk(lay.flat, f, e) == want, (f, e)
    assert 288 < 300 < 314 < 320 and 276 // W == 8            # E 300 cuts word 9 before its set bit


# ------------------------------------------------------------------------------ geometry
def chunk_bits(lay, k):
    return [p for p in lay.bits if p // C == k]


def steps(lay):
    """set bit -> where its header points"""
    return {p: p + 4 + int.from_bytes(lay.flat[p:p + 4], "little", signed=True) for p in lay.bits}


def test_dense_geometry():
    lay = cc.layout("dense")
    a, b = lay.marks["span"]
    assert b - a >= 3 * C and lay.clean
    lanes = {p // L for p in lay.bits}
    assert all(k in lanes for k in range(a // L + 1, b // L))            # every lane holds a bit
    words = [p // W for p in lay.bits]
    assert len(set(words)) == len(words)                                 # a word holds 0 or 1


def test_word_edges_geometry():
    lay = cc.layout("word_edges")
    below, at, bits = lay.marks["below"], lay.marks["at"], set(lay.bits)
    assert lay.clean and all(p % W == W - 1 and p + REC in bits for p in below)
    assert all(p % W == 0 and p - REC in bits for p in at)
    for unit in (W, L, P, C, G):
        assert any((p + 1) % unit == 0 for p in below) and any(p % unit == 0 for p in at), unit
        # ... and one that is on no coarser grid (a word edge inside a lane, a lane edge inside a chunk)
    assert any((p + 1) % L for p in below) and any(p % L for p in at)
    assert any((p + 1) % L == 0 and (p + 1) % P for p in below) and any(p % L == 0 and p % P for p in at)
    assert any(cc.lane_of(p) == cc.WAVE - 1 and p % L == 0 for p in at)  # the first position of lane 63
    assert any(cc.lane_of(p) == cc.WAVE - 1 and p % L == L - 1 for p in below)   # the last of a chunk


def test_empty_lanes_geometry():
    lay = cc.layout("empty_lanes")
    sizes = [b - a for a, b in zip(lay.chain, lay.chain[1:])]
    assert lay.clean and {L + 1, 2 * L, 5 * L} <= set(sizes)
    a, b, c = lay.marks["lane0"], lay.marks["lane63"], lay.marks["after"]
    assert chunk_bits(lay, a // C) == [a] and cc.lane_of(a) == 0
    assert chunk_bits(lay, b // C) == [b] and cc.lane_of(b) == cc.WAVE - 1 and b // C == a // C + 1
    assert c // C == b // C + 1 and chunk_bits(lay, c // C)[0] == c
    gaps = {(q // L - p // L) for p, q in zip(lay.bits, lay.bits[1:]) if p // C == q // C}
    assert gaps >= {1, 2, 5}                                             # successors one, two and five lanes on


def test_empty_waves_geometry():
    lay = cc.layout("empty_waves")
    sizes = [b - a for a, b in zip(lay.chain, lay.chain[1:])]
    assert lay.clean and {C + 1, 2 * C + 7, 3 * C + 1} <= set(sizes)
    empty = {q // C - p // C - 1 for p, q in zip(lay.bits, lay.bits[1:]) if q // C != p // C}
    assert empty >= {0, 1, 2, 3}                                         # whole empty chunks between two set bits
    s = lay.marks["chunk_start"]
    assert s % C == 0 and lay.bits[lay.bits.index(s) - 1] // C == s // C - 4
    assert chunk_bits(lay, s // C) == [s, lay.marks["c3b"]]
    # "the last position before E": E = s + 1 for a record s that a long record steps to
    assert (lay.marks["c2"], lay.marks["c3"] + 1) in cc.edges(lay, cap=10 ** 6)


def test_tail_geometry():
    for k in cc.TAILS:
        lay = cc.layout(f"tail_{k}")
        cut = lay.marks["cut"]
        assert len(lay.flat) - cut == k and cut not in lay.bits and (cut in lay.chain) == (k >= 4)
        assert lay.bits[-1] == cut - REC and lay.rtc == 1
        assert cc.walk(lay.flat, lay.chain[0], len(lay.flat)) == (4 + (k >= 4), cut if k < 4 else len(lay.flat))
    for name, rem in (("tail_0_on_word", 0), ("tail_0_past_word", 1), ("tail_5_on_word", 0),
                      ("tail_overhang_on_word", 0), ("tail_overhang_past_word", 1)):
        assert len(cc.layout(name).flat) % W == rem
    for name in ("tail_overhang", "tail_overhang_on_word", "tail_overhang_past_word"):
        lay = cc.layout(name)
        last = lay.marks["last"]
        assert lay.bits[-1] == last and steps(lay)[last] == len(lay.flat) + 100 - 0 and lay.clean
        assert cc.walk(lay.flat, last, len(lay.flat)) == (1, len(lay.flat))


@pytest.mark.parametrize("rtc", [2, 10])
def test_bait_dead_end_geometry(rtc):
    lay = cc.layout(f"bait_dead_end_{rtc}")
    bait, st = set(lay.marks["bait"]), steps(lay)
    fp = [p for p in lay.bits if p not in lay.chain]
    assert lay.rtc == rtc and len(lay.bits) > len(lay.chain) and fp and set(fp) <= bait
    ends = [p for p in fp if st[p] not in lay.bits]
    assert len(ends) == 2 and all(st[p] in bait for p in ends)           # each run's chain lands on a clear bit
    assert {p // C for p in fp} >= {0, 1}                                # a run crosses the chunk edge


def test_bait_joins_geometry():
    lay = cc.layout("bait_joins")
    st = steps(lay)
    for j, b in ((lay.marks["joined"], lay.marks["bait"]), (lay.marks["joined2"], lay.marks["bait2"])):
        pred = [p for p in lay.bits if st[p] == j]
        assert len(pred) == 2 and j in lay.chain and set(b) <= set(lay.bits)
        assert sorted(p in lay.chain for p in pred) == [False, True]
    others = [q for q in set(st.values()) if q in st and q not in (lay.marks["joined"], lay.marks["joined2"])]
    assert all(sum(1 for p in st if st[p] == q) == 1 for q in others)


def test_bait_leaves_geometry():
    lay = cc.layout("bait_leaves_E")
    st, last = steps(lay), lay.marks["bait"][-1]
    assert last in lay.bits and last not in lay.chain and st[last] in lay.chain
    assert all(last < e <= st[last] for e in lay.marks["E"])             # its step leaves [first, E)
    lay = cc.layout("bait_leaves_total")
    st, last = steps(lay), lay.marks["bait"][-1]
    assert lay.rtc == 1 and last in lay.bits and last not in lay.chain and st[last] > len(lay.flat)


def test_bait_long_geometry():
    lay = cc.layout("bait_long")
    st = steps(lay)
    for key, n in (("over", cc.CM_PEEL_MAX + 5), ("under", cc.CM_PEEL_MAX - 1), ("most", cc.CM_PEEL_MAX + 1)):
        run = lay.marks[key]
        assert len(run) == n and set(run) <= set(lay.bits) and not set(run) & set(lay.chain)
        assert all(st[p] == q for p, q in zip(run, run[1:])) and st[run[-1]] not in lay.bits
        assert not any(st[p] == run[0] for p in lay.bits)                # the run's first bit is a root
    assert lay.marks["over"][-1] < lay.marks["between"] < lay.marks["under"][0]
    assert lay.marks["under"][-1] < lay.marks["between2"] < lay.marks["most"][0]
    assert lay.marks["between"] in lay.chain and lay.marks["between2"] in lay.chain


def test_bait_first_word_geometry():
    lay = cc.layout("bait_first_word")
    a, fa = lay.marks["after"]
    fb, b = lay.marks["before"]
    assert lay.rtc == 2 and a // W == fa // W and a < fa and fb // W == b // W and fb < b
    assert {a, fa, fb, b} <= set(lay.bits) and a in lay.chain and b in lay.chain
    assert fa not in lay.chain and fb not in lay.chain
    # the marker's prefix groups are counted from the word of `from`: a chain record's successor in
    # the first, second and last word of a group, for a range from the chain's first record
    w0 = lay.chain[0] // W
    res = {(q // W - w0) % cc.WPRE_GROUP for q in lay.chain[1:]}
    assert res >= {0, 1, cc.WPRE_GROUP - 1}
    assert any(q // W == w0 + 1 for q in lay.chain[1:2])                 # (and the k == 0 term: a successor in word w0 + 1)


def test_short_step_geometry():
    lay = cc.layout("short_step")
    fp, a, b = lay.marks["word"]
    assert lay.rtc == 1 and fp // W == a // W == b // W and fp < a < b and {fp, a, b} <= set(lay.bits)
    assert fp not in lay.chain and lay.chain[lay.chain.index(a) + 1] == b and steps(lay)[a] == b
    assert not lay.clean and set(lay.marks["bait"]) <= set(lay.bits)     # (an anomaly further on: the marker runs)
    assert (a, len(lay.flat)) in cc.edges(lay, cap=10 ** 6)


def test_rejected_geometry():
    lay = cc.layout("rejected")
    m = lay.marks
    bad = (m["first"], m["middle"]) + m["pair"] + (m["last"],)
    assert lay.rtc == 1 and set(bad) <= set(lay.chain) and not set(bad) & set(lay.bits)
    assert set(lay.bits) == set(lay.chain) - set(bad)
    assert m["first"] == lay.chain[0] and m["last"] == lay.chain[-1] and m["pair"][1] == m["pair"][0] + REC
    assert m["pair"][0] // C == 0 and m["pair"][1] // C == 1             # the pair lies across a chunk edge


def test_first_at_and_grid_wrap_geometry():
    for p in cc.FIRST_AT:
        lay = cc.layout(f"first_at_{p}")
        assert lay.bits[0] == lay.chain[0] == p and lay.clean and lay.bits[-1] > p + C
    spans = {p // G: p % G for p in cc.FIRST_AT}
    assert spans[0] == G - 1 and spans[1] in (0, 1) and spans[2] == 0    # the last bit of a span, the first of the next
    lay = cc.grid_wrap_prefix()
    assert lay.chain[0] == cc.GRID_FIRST > cc.FS_GRID * G
    assert cc.GRID_FIRST + cc.GRID_REC * cc.GRID_N - cc.GRID_FIRST // C * C > cc.PROOF_GRID * G
    assert cc.GRID_REC * (cc.GRID_N - 8) < cc.PROOF_GRID * G               # (and no larger than it has to be)


def test_split_ranges_geometry():
    """The split ranges the GPU test places (their own assertions: chunks apart, ends on the chunk
    grid at a set bit, first words at every 4-word alignment, spans over PC_WORDS words)."""
    lay = cc.layout("dense_edges")
    assert lay.clean and len(lay.flat) > 32 * cc.PC_WORDS
    assert len(cc.dense_edges_splits()) >= 12 and len(cc.popcount_splits()) == 4 and len(cc.marked_splits()) == 5
