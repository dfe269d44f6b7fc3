"""Batched record delivery (sbh_split_records_batch), the parts that need no GPU:

  * the entry point is declared in include/sparkbam.h, listed in the binding's EXPORTS and
    exported by the built library;
  * a numpy model of the device contract behind it (records.hip: k_chunk_popcounts /
    k_word_prefix over the union, k_range_counts, k_ranges_positions): the set bits of n sorted,
    disjoint flat ranges of one bitmap, range i's r-th bit at pos[off[i] + r], off the exclusive
    prefix of the ranges' counts (+ the rows reserved behind a range).  The model follows the
    kernels step for step -- word prefix per group of 16 words once over the union, a rank
    lookup per range end, a binary search over E per bitmap word -- and is checked against a
    brute-force listing of each range's set bits.
"""
import os
import re

import numpy as np
import pytest

from pkg import ROOT, sb

GROUP = 16  # WPRE_GROUP: bitmap words per prefix entry


def test_batch_entry_point_declared_and_exported():
    with open(os.path.join(ROOT, "include", "sparkbam.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint\s+sbh_split_records_batch\s*\(", hdr)
    for t in ("sbh_batch_split", "sbh_split_batch_result"):
        assert re.search(r"\}\s*" + t + r"\s*;", hdr), t
    assert "sbh_split_records_batch" in sb._lib.EXPORTS
    assert hasattr(sb.lib(), "sbh_split_records_batch")
    # the ctypes mirrors have the header's fields, in order
    body = re.search(r"typedef struct \{([^}]*)\}\s*sbh_batch_split;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip()
             for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in sb._lib.SbhBatchSplit._fields_]


# ---- the model ------------------------------------------------------------------------------

def masked_word(words, begin, U0, U1, w):
    """Word w of the bitmap (bit k = position begin + 32 w + k) with the bits outside [U0, U1) cleared."""
    if w >= (U1 - begin + 31) // 32:
        return 0
    v = int(words[w])
    p0 = begin + 32 * w
    if p0 < U0:
        v &= (0xFFFFFFFF << (U0 - p0)) & 0xFFFFFFFF
    if p0 + 32 > U1:
        v &= (1 << (U1 - p0)) - 1
    return v


def popc(v):
    return bin(v).count("1")


def model(words, begin, first, E, reserve):
    """(off[0..n], pos) as the launch set computes them.  first / E: non-decreasing, first[i] <=
    E[i] <= first[i + 1], inside the union [U0, U1) = [first of the first live range, last E)."""
    n = len(first)
    live = [i for i in range(n) if first[i] < E[i]]
    U0, U1 = first[live[0]], E[live[-1]]
    wb = (U0 - begin) // 32
    nw = (U1 - begin + 31) // 32 - wb
    # k_chunk_popcounts + scan + k_word_prefix: set bits of the union before each group of words
    wpre, c = [], 0
    for r in range(nw):
        if r % GROUP == 0:
            wpre.append(c)
        c += popc(masked_word(words, begin, U0, U1, wb + r))

    def rank(x):  # union_rank: set bits of [U0, x)
        r = (x - begin) // 32 - wb
        g = min(r, nw - 1) // GROUP
        c = wpre[g]
        for k in range(g * GROUP, r):
            c += popc(masked_word(words, begin, U0, U1, wb + k))
        below = (x - begin) & 31
        if below:
            c += popc(masked_word(words, begin, U0, U1, wb + r) & ((1 << below) - 1))
        return c

    # k_range_counts + scan
    rbase = [rank(first[i]) for i in range(n)]
    cnt = [(rank(E[i]) - rbase[i] if E[i] > first[i] else 0) + reserve[i] for i in range(n)]
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    # k_ranges_positions: per word, the ranges it intersects
    pos = np.full(int(off[-1]), -1, dtype=np.int64)
    base = 0
    for r in range(nw):
        if r % 64 == 0:
            base = wpre[r // GROUP]  # the wave's base; a lane adds the popcounts before it
        v = masked_word(words, begin, U0, U1, wb + r)
        p0 = begin + 32 * (wb + r)
        if v:
            lo, hi = 0, n  # first range with E > p0
            while lo < hi:
                m = (lo + hi) // 2
                if E[m] <= p0:
                    lo = m + 1
                else:
                    hi = m
            i = lo
            while i < n and first[i] < p0 + 32:
                a, b = first[i], E[i]
                if a < b:
                    m = v
                    if a > p0:
                        m &= (0xFFFFFFFF << (a - p0)) & 0xFFFFFFFF
                    if b < p0 + 32:
                        m &= (1 << (b - p0)) - 1
                    for bit in range(32):
                        if m >> bit & 1:
                            at = off[i] - rbase[i] + base + popc(v & ((1 << bit) - 1))
                            assert off[i] <= at < off[i + 1] - reserve[i]
                            assert pos[at] == -1
                            pos[at] = p0 + bit
                i += 1
        base += popc(v)
    return off, pos


def brute(words, begin, first, E, reserve):
    bits = np.unpackbits(np.asarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    off, out = [0], []
    for a, b, r in zip(first, E, reserve):
        p = np.flatnonzero(bits[a - begin:b - begin]) + a if b > a else np.zeros(0, np.int64)
        out += p.tolist() + [-1] * r
        off.append(len(out))
    return np.asarray(off, np.int64), np.asarray(out, np.int64)


def check(words, begin, first, E, reserve=None):
    reserve = reserve or [0] * len(first)
    off, pos = model(words, begin, first, E, reserve)
    off_b, pos_b = brute(words, begin, first, E, reserve)
    assert np.array_equal(off, off_b)
    assert np.array_equal(pos, pos_b)
    return off


def test_model_handmade_shapes():
    rng = np.random.default_rng(11)
    words = rng.integers(0, 1 << 32, 200, dtype=np.uint64).astype(np.uint32)
    begin = 1000  # bit 0 = position 1000: words do not line up with the ranges
    # two ranges meeting mid-word, a range inside one word, three ranges inside one word, a boundary
    # exactly on a word boundary, empty ranges (before, between, after), gaps, reserved rows
    first = [1003, 1003, 1050, 1100, 1290, 1300, 1304, 1309, 1320 + 32 * 7, 2000, 2400, 2400]
    E = [1003, 1050, 1090, 1288, 1295, 1304, 1309, 1311, 1320 + 32 * 9, 2400, 2400, 2400 + 32 * 40 + 5]
    res = [0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 7, 0]
    off = check(words, begin, first, E, res)
    assert off[1] == 0 and off[11] - off[10] == 7
    # the union ending exactly on a word boundary of the bitmap, and one range over everything
    check(words, begin, [1000 + 32 * 3], [1000 + 32 * 100])
    check(words, 0, [0], [32 * 200])
    check(words, 0, [5, 37], [37, 64])


@pytest.mark.parametrize("seed", range(12))
def test_model_random_ranges(seed):
    rng = np.random.default_rng(seed)
    nwords = int(rng.integers(3, 400))
    dense = rng.random() < 0.5
    words = rng.integers(0, 1 << 32, nwords, dtype=np.uint64).astype(np.uint32)
    if not dense:  # sparse, like record starts (at most a bit per word or two)
        words &= rng.integers(0, 1 << 32, nwords, dtype=np.uint64).astype(np.uint32)
        words &= rng.integers(0, 1 << 32, nwords, dtype=np.uint64).astype(np.uint32)
        words &= rng.integers(0, 1 << 32, nwords, dtype=np.uint64).astype(np.uint32)
    begin = int(rng.integers(0, 5000))
    total = 32 * nwords
    ncut = int(rng.integers(2, min(total, 120)))
    cuts = np.sort(rng.choice(np.arange(begin, begin + total + 1), ncut, replace=False))
    first, E, res = [], [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        kind = rng.integers(0, 4)
        a, b = int(a), int(b)
        if kind == 0:    # a gap: no range
            continue
        if kind == 1:    # an empty range (with rows reserved for it, sometimes)
            first.append(a), E.append(a), res.append(int(rng.integers(0, 3)))
            continue
        if kind == 2:    # a range, then a gap before the next cut
            b = int(rng.integers(a + 1, b + 1))
        first.append(a), E.append(b), res.append(0)
    if not any(a < b for a, b in zip(first, E)):
        first.append(int(cuts[-2])), E.append(int(cuts[-1])), res.append(0)
    # (empty ranges lie inside the union, as the caller normalises them)
    live = [i for i in range(len(first)) if first[i] < E[i]]
    U0, U1 = first[live[0]], E[live[-1]]
    first = [min(max(a, U0), U1) for a in first]
    E = [min(max(b, U0), U1) for b in E]
    check(words, begin, first, E, res)
