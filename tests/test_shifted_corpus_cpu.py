"""shifted_corpus.py held to what it claims (no GPU): with a small gap zlib reads the file back as
header + zeros + records and the member table is the one a walk of the file finds; with the gap that
puts a record across 2^31 or 2^32 -- by arithmetic and a walk of the member headers, the gap is never
inflated -- the chosen byte lies exactly on the boundary, records lie on both sides of it, and every
remapped virtual offset points at its record's first byte inside the right member."""
import time
import zlib

import numpy as np
import pytest

import record_corpus as rc
import shifted_corpus as sc

BOUNDARIES = (1 << 31, 1 << 32)


def member_bytes(sf, i):
    c, n = int(sf.members[i, 0]), int(sf.members[i, 1])
    return zlib.decompress(bytes(sf.data[c + 18:c + n - 8]), -15)


@pytest.mark.parametrize("payload", (65280, 97))
@pytest.mark.parametrize("gap_members, rest", [(0, 0), (0, 5), (3, 0), (3, 1234)])
def test_small_gap_reads_back(payload, gap_members, rest):
    s = rc.interval_stream()
    k, d = len(s.starts) // 2, 2
    P = gap_members * sc.GAP_PAYLOAD + rest
    sf = sc.shift_stream(s, s.starts[k] + d + P, k, d, payload)
    assert sf.shift == P and sf.first == s.first + P and sf.flat_size == len(s.flat) + P
    assert rc.inflate_members(sf.data) == s.flat[:s.first] + bytes(P) + s.flat[s.first:]
    assert np.array_equal(sc.walk(sf.data), sf.members)
    assert sf.starts == [p + P for p in s.starts]
    # the records begin a member of their own, right behind the gap's
    assert int(sf.members[sf.rec_member, 2]) == sf.first and int(sf.members[sf.rec_member - 1, 3]) > 0
    assert sf.members[-1].tolist()[1:] == [28, sf.flat_size, 0]


def test_unshifted_is_the_tail_of_every_shift():
    s = rc.decode_stream()
    twin = sc.unshifted(s.flat, s.first, s.starts, 4096)
    sf = sc.shift_stream(s, 10 ** 6, 3, 1, 4096)
    assert twin.shift == 0 and rc.inflate_members(twin.data) == s.flat
    n = twin.members.shape[0] - twin.rec_member
    assert bytes(twin.data[twin.members[twin.rec_member, 0]:]) == bytes(sf.data[sf.members[sf.rec_member, 0]:])
    assert np.array_equal(twin.members[-n:, [1, 3]], sf.members[-n:, [1, 3]])


def test_vpos_maps():
    s = rc.interval_stream()
    sf = sc.shift_stream(s, 300000, 4, 0, 97)
    # a walk over every flat position of the records: member by member, offset by offset
    live = [(int(c), int(f), int(u)) for c, _, f, u in sf.members if u]
    want = [c << 16 | o for c, f, u in live for o in range(u) if f + o >= sf.first]
    flats = np.arange(sf.first, sf.flat_size)
    assert sc.vpos_of(sf.members, flats).tolist() == want
    assert np.array_equal(sc.flat_of_vpos(sf.members, want), flats)
    # the end of the stream: the EOF member's start
    assert sc.vpos_of(sf.members, [sf.flat_size]).tolist() == [int(sf.members[-1, 0]) << 16]
    assert sc.flat_of_vpos(sf.members, [int(sf.members[-1, 0]) << 16]).tolist() == [sf.flat_size]
    # through two tables, an untouched linear-index window left alone
    old = sc.unshifted(s.flat, s.first, s.starts, 300)
    v = sc.vpos_of(old.members, s.starts + [len(s.flat)])
    got = sc.remap_vpos(old.members, sf.members, sf.shift, np.append(v, np.uint64(sc.U64_MAX)))
    assert got[:-1].tolist() == sc.vpos_of(sf.members, sf.starts + [sf.flat_size]).tolist() and int(got[-1]) == sc.U64_MAX


def test_combine_keeps_every_corpus_at_its_rows():
    a, b = rc.interval_stream(), rc.decode_stream()
    s, rows = sc.combine([a, b, a])
    assert rows == [(0, len(a.starts)), (len(a.starts), len(a.starts) + len(b.starts)),
                    (len(a.starts) + len(b.starts), 2 * len(a.starts) + len(b.starts))]
    assert s.flat == a.flat + b.flat[b.first:] + a.flat[a.first:] and s.first == a.first
    for (lo, hi), part in zip(rows, (a, b, a)):
        end = s.starts[hi] if hi < len(s.starts) else len(s.flat)
        assert s.flat[s.starts[lo]:end] == part.flat[part.first:]
        assert [p - s.starts[lo] for p in s.starts[lo:hi]] == [p - part.first for p in part.starts]


@pytest.mark.parametrize("d", (0, 2))
@pytest.mark.parametrize("B", BOUNDARIES, ids=("2^31", "2^32"))
@pytest.mark.parametrize("payload", (65280, 97))
def test_across_the_boundary(B, d, payload):
    s = rc.interval_stream()
    k = len(s.starts) // 2
    t0 = time.perf_counter()
    sf = sc.shift_stream(s, B, k, d, payload)
    print("built in %.0f ms: %d file bytes, %d members" % (1e3 * (time.perf_counter() - t0), sf.data.size, len(sf.members)))
    assert sf.data.size < 16 << 20  # (the gap is a few MB of members, never its zeros)
    assert sf.starts[k] == B - d and sf.shift == B - d - s.starts[k]
    assert sf.starts[0] < B and sf.starts[k - 1] < B < sf.starts[k + 1] and sf.starts[-1] > B
    assert sf.flat_size == len(s.flat) + sf.shift and sf.first == s.first + sf.shift
    # the table: what a walk of the member headers finds; whole zero members, then one shorter one
    assert np.array_equal(sc.walk(sf.data), sf.members)
    gap = sf.members[1:sf.rec_member]
    assert int(sf.members[0, 3]) == s.first and int(gap[:, 3].sum()) == sf.shift
    assert (gap[:-1, 3] == sc.GAP_PAYLOAD).all() and 0 < gap[-1, 3] <= sc.GAP_PAYLOAD
    assert len(set(gap[:-1, 1].tolist())) == 1  # (one member, replicated)
    # every start's virtual offset: the record's first bytes at that offset of that member
    v = sc.vpos_of(sf.members, sf.starts)
    for p_old, p_new, vp in zip(s.starts, sf.starts, v.tolist()):
        i = int(np.searchsorted(sf.members[:, 0], vp >> 16))
        assert int(sf.members[i, 0]) == vp >> 16 and i >= sf.rec_member
        assert int(sf.members[i, 2]) + (vp & 0xFFFF) == p_new and (vp & 0xFFFF) < int(sf.members[i, 3])
        u = member_bytes(sf, i)[vp & 0xFFFF:][:36]  # (the fixed fields, or what the member holds of them)
        assert u and u == s.flat[p_old:p_old + len(u)]
    assert np.array_equal(sc.flat_of_vpos(sf.members, v), np.asarray(sf.starts))
