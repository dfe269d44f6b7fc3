"""Hand-built members for the byte-exact BGZF writer (spark-bam_amd/csrc/zdeflate.hip) -- TEST
INFRASTRUCTURE.  Each case is one member's payload built to reach one named edge of the five GPU
stages (k_zprev, k_zinfo, k_zparse, k_ztrees, k_zemit), with a `check` that proves from zlib's own
stream (deflate_parse.py) -- or, where zlib's bytes cannot show it, from the host definition's
trace (sbh_host_zdeflate_trace) -- that the case still reaches that edge.
tests/test_zdeflate_corpus_cpu.py runs the checks and pins the host definition to zlib on every
case; tests/test_zdeflate_conformance_gpu.py runs the kernels over the same payloads.

Builders are deterministic.  Two fillers carry the planted structures:
  Uniq   bytes 64..127 chosen so that every trigram's 15-bit hash occurs once: no match and no
         chain other than the planted ones (at most ~17000 bytes: there are 32768 hashes);
  noisy  random bytes 32..47 for the full-size cases, rich in short matches.  A trigram holding a
         byte 48..63 (the plants) differs from every filler trigram in hash bit 4, 9 or 14, so a
         plant's chains hold plants only.
Where a property needs a search, the builder searches a stated finite range and raises.

Not built, and why:
  * A candidate chain with cmp() == 2: impossible.  Two trigrams with an equal hash and equal first
    two bytes have an equal third byte (it enters the hash unshifted); `same_hash_cmp` covers cmp
    0, 1 and >= 3.
  * One emit thread's token range spanning two block boundaries: a thread takes at most 256
    tokens and blocks close at 16383 symbols, so two boundaries lie in one range only when the
    final block is empty (`final_empty`); `dsd_phase_*` has a range that begins inside the stored
    block and ends in the dynamic block after it.
  * A level-5 stream of 65519 bytes: there is none.  A block costs at most its stored form (5
    bytes more than its bytes) unless the window slide has taken its buffer away, and such a block
    spans more than 32506 bytes in at most 16383 symbols, so it is mostly matches and far smaller
    than stored; five blocks would need more than 65532 symbols.  So a 65498-byte member gives at
    most 65498 + 4 * 5 = 65518 bytes, which is the far side of htsjdk's fallback
    (`fallback_65518`); 65516 and 65517 are the near side.  _fallback's search (3 seeds, random
    bytes with a tail of 0..47 bytes of 0 or 255) finds the other three and reports this one.
Both 15-bit caps and the 7-bit cap are reached by construction, not by search: match lengths and
distances are symbols LZ cannot absorb (`lit_cap15`, `dist_cap15`), and dyadic literal counts fix
the literal tree's lengths in advance (`bl_cap7`).
"""
import ctypes as C
import os
import random
import zlib

import numpy as np

import deflate_parse as dp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAYLOAD = 65498
OUT_CAP = 65518
WSIZE, MAX_DIST, SLIDE_AT = 32768, 32506, 65274
CFG = {4: (4, 4, 16, 16), 5: (8, 16, 32, 32), 6: (8, 16, 128, 128), 7: (8, 32, 128, 256), 8: (32, 128, 258, 1024),
       9: (32, 258, 258, 4096)}  # good, lazy, nice, chain
ZB_STORED, ZB_STATIC, ZB_DYN = 0, 1, 2
SMALL = 8192  # levels 8 / 9 run below this size (the host chain walk is slow)


def zhash(b0, b1, b2):
    return ((b0 << 10) ^ (b1 << 5) ^ b2) & 0x7fff


def hashes(data):
    return [zhash(data[i], data[i + 1], data[i + 2]) for i in range(len(data) - 2)]


def zlib_raw(data, level=5):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    return c.compress(bytes(data)) + c.flush()


# ---- the host definition's trace ---------------------------------------------------------------
class Trace:
    def __init__(self, data, level):
        path = os.path.join(ROOT, "tools", "libzdeflate_host.so")
        if not os.path.exists(path):
            import pytest
            pytest.skip("tools/libzdeflate_host.so not built (run __graft_entry__.build())", allow_module_level=True)
        L = C.CDLL(path)
        n = len(data)
        a = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
        self.prev, self.info = np.zeros(n + 1, np.uint16), np.zeros(n + 1, np.uint64)
        visit, self.tok = np.zeros(2 * n + 2, np.uint32), np.zeros(n + 2, np.uint32)
        blocks, cnt = np.zeros(8 * 8, np.uint32), np.zeros(3, np.uint32)
        L.sbh_host_zdeflate_trace.argtypes = [C.c_void_p, C.c_uint32, C.c_int] + [C.c_void_p] * 6
        L.sbh_host_zdeflate_trace.restype = None
        L.sbh_host_zdeflate_trace(a.ctypes.data, n, level, self.prev.ctypes.data, self.info.ctypes.data,
                                  visit.ctypes.data, self.tok.ctypes.data, blocks.ctypes.data, cnt.ctypes.data)
        nv, self.ntok, nb = (int(x) for x in cnt)
        self.visits = {int(p): int(pl) for p, pl in visit[:2 * nv].reshape(-1, 2)}  # position -> prev_length
        self.order = [int(p) for p in visit[:2 * nv:2]]
        self.tok = self.tok[:self.ntok]
        # rows: tok0, tok1, byte0, byte1, nobuf, type, opt_lenb, static_lenb
        self.blocks = blocks[:8 * nb].reshape(-1, 8).astype(np.int64)

    def rec(self, p, quarter):
        """(M, S) of position p's record over the full chain or the quarter chain."""
        r = int(self.info[p])
        return ((r >> 25) & 0x1ff, (r >> 34) & 0xffff) if quarter else (r & 0x1ff, (r >> 9) & 0xffff)

    def tokens(self):
        return [(((int(t) >> 16) & 0xff) + 3, int(t) & 0xffff) if int(t) >> 31 else int(t) for t in self.tok]


class View:
    """What zlib (and the host definition) did with one case at one level, computed on demand."""

    def __init__(self, case, level):
        self.case, self.data, self.level = case, case.data, level
        self.good, self.lazy, self.nice, self.chain = CFG[level]
        self._c = {}

    def _get(self, k, f):
        if k not in self._c:
            self._c[k] = f()
        return self._c[k]

    raw = property(lambda s: s._get("raw", lambda: zlib_raw(s.data, s.level)))
    blocks = property(lambda s: s._get("blocks", lambda: dp.parse(s.raw)))
    at = property(lambda s: s._get("at", lambda: dict(dp.positions(s.blocks))))
    trace = property(lambda s: s._get("trace", lambda: Trace(s.data, s.level)))

    def literal(self, p):
        return isinstance(self.at.get(p), int)


class Case:
    def __init__(self, name, data, why, check, levels=None):
        self.name, self.data, self.why, self.check = name, bytes(data), why, check
        assert len(self.data) <= PAYLOAD, name
        self.levels = levels or ((4, 5, 6, 9) if len(self.data) < SMALL else (4, 5, 6))
        self.full = len(self.data) == PAYLOAD


# ---- fillers -----------------------------------------------------------------------------------
def rnd(seed, n, lo, hi):
    r = random.Random(seed)
    return bytes(r.randrange(lo, hi) for _ in range(n))


def noisy(seed, n):
    return bytearray(rnd(seed, n, 32, 48))


class Uniq:
    """A payload under construction: fill() adds filler whose every new trigram hash is unused so
    far; put() adds bytes as they are.  reserve() keeps hashes (the plants') away from the filler."""

    def __init__(self, seed, lo=64, hi=128):
        self.d, self.used, self.r, self.lo, self.hi = bytearray(), set(), random.Random(seed), lo, hi
        self._filled = False

    def reserve(self, *plants):
        for p in plants:
            self.used.update(hashes(p))
        return self

    def __len__(self):
        return len(self.d)

    def _note(self):
        if len(self.d) >= 3:
            self.used.add(zhash(*self.d[-3:]))

    def fill(self, n):
        for _ in range(n):
            for _try in range(400):
                b = self.r.randrange(self.lo, self.hi)
                if len(self.d) < 2 or zhash(self.d[-2], self.d[-1], b) not in self.used:
                    break
            else:  # (behind a plant planted many times: any byte 128..255 that gives an unused hash)
                for b in range(128, 256):
                    if zhash(self.d[-2], self.d[-1], b) not in self.used:
                        break
                else:  # (no hash left: a new trigram, which collides with one but matches none)
                    for b in range(self.lo, self.hi):
                        if bytes([self.d[-2], self.d[-1], b]) not in self.d:
                            break
                    else:
                        raise ValueError("Uniq: no unused trigram left at %d" % len(self.d))
            self.d.append(b)
            self._note()
            self._filled = True
        return self

    def fill_to(self, pos):
        assert pos >= len(self.d), (pos, len(self.d))
        return self.fill(pos - len(self.d))

    def put(self, b):
        b = bytes(b)
        if self._filled and len(self.d) >= 3 and len(b) >= 2:
            # re-pick the last filler byte so that the trigrams running into b are unused too
            self.used.discard(zhash(*self.d[-3:]))
            x0 = self.d.pop()
            cand = [x0] + list(range(self.lo, self.hi)) + list(range(128, 256))
            # (x, b0, b1) has 32 hashes only, and late in a long payload few hashes are left: then
            # trigrams that are new (hash collisions, never matches) will do
            for strict in (2, 1, 0):
                for x in cand:
                    t = (bytes([self.d[-2], self.d[-1], x]), bytes([self.d[-1], x, b[0]]), bytes([x, b[0], b[1]]))
                    hs = [zhash(*y) for y in t]
                    if len(set(hs)) == 3 and not set(hs[:strict]) & self.used and all(
                            y not in self.d for y in t[strict:]):
                        break
                else:
                    continue
                break
            else:
                raise ValueError("Uniq: no byte fits before the plant at %d" % len(self.d))
            self.d.append(x)
            self._note()
        self._filled = False
        for x in b:
            self.d.append(x)
            self._note()
        return len(self.d) - len(bytes(b))

    def copy(self, src, n):
        return self.put(bytes(self.d[src:src + n]))


def plant(seed, n, lo=48, hi=64):
    """n plant bytes with no repeated trigram hash inside the plant."""
    return bytes(Uniq(7000 + seed, lo, hi).fill(n).d)


CASES = []


def case(name, data, why, check, levels=None):
    CASES.append(Case(name, data, why, check, levels))


def _is(v, p, tok):
    assert v.at.get(p) == tok, (v.case.name, v.level, p, v.at.get(p), tok)


# ---- k_zprev -----------------------------------------------------------------------------------
def _lengths():
    hp = {1: 0, 2: 0, 3: 1, 4: 2, 66: 64, 67: 65, 130: 128}
    for n in hp:
        data = rnd(n, n, 97, 99)

        def check(v, n=n):
            assert len(v.data) == n and max(n - 2, 0) == hp[n]
            t = v.trace
            if n <= 4:
                assert [b.kind for b in v.blocks] == [dp.FIXED]  # the static choice wins on tiny inputs
            if n >= 66:
                assert t.prev[hp[n] - 1] != 0  # the last hashed position has a predecessor
            if n == 67:
                assert t.prev[64] != 0  # the one live lane of the second step
        case("len_%d" % n, data, "k_zprev: hp = %d positions (dead lanes in the last step)" % hp[n], check)


def _step_one_hash():
    u = Uniq(1).reserve(b"000")
    u.fill(64)
    u.put(b"0" * 66)
    u.fill(62)

    def check(v):
        h = hashes(v.data)
        assert len(set(h[64:128])) == 1 and h[63] != h[64] and h[128] != h[64]
        p = v.trace.prev
        assert p[64] == 0 and all(p[q] == q - 1 for q in range(65, 128))
    case("step_one_hash", u.d, "k_zprev: all 64 lanes of step 1 share one hash", check)


def _pair_63_64():
    u = Uniq(2).reserve(b"000")
    u.fill(63)
    u.put(b"0000")
    u.fill(61)

    def check(v):
        h = hashes(v.data)
        assert h[63] == h[64] and h.count(h[63]) == 2
        assert v.trace.prev[64] == 63 and v.trace.prev[63] == 0
    case("pair_63_64", u.d, "k_zprev: a hash group split across the step boundary 63 | 64", check)


def _hash_every_step():
    u = Uniq(3).reserve(b"012")
    at = []
    for k in range(64):
        u.fill_to(64 * k + (k * 7) % 61)
        at.append(u.put(b"012"))
    u.fill_to(4096)

    def check(v):
        h = hashes(v.data)
        H = zhash(48, 49, 50)
        assert [q for q in range(len(h)) if h[q] == H] == at and [q // 64 for q in at] == list(range(64))
        p, q, chain = v.trace.prev, at[-1], []
        while q:
            chain.append(q)
            q = int(p[q])
        assert chain == at[:0:-1]  # (position 0 is NIL in zlib: the plant at 0 is never a candidate)
    case("hash_every_step", u.d, "k_zprev: one hash in every step of 4096 bytes (head table carried 63 times)", check)


def _same_hash_cmp():
    A, Bm, D = bytes([48, 49, 50]), bytes([48, 48, 18]), bytes([16, 49, 50])
    tail = plant(5, 5)
    u = Uniq(4).reserve(A + tail, Bm, D)
    u.fill(10)
    q1 = u.put(A + tail)
    u.fill(4)
    sites = [(q1, "A")]
    for t, name in ((Bm, "B"), (D, "D"), (A, "A"), (D, "D"), (Bm, "B")):
        sites.append((u.put(t), name))
        u.fill(4)
    p = u.put(A + tail)
    u.fill(7)

    def check(v):
        assert zhash(*A) == zhash(*Bm) == zhash(*D)
        pv, q, seen = v.trace.prev, p, []
        while pv[q]:
            q = int(pv[q])
            seen.append(q)
        assert seen == [s for s, _ in sites][::-1]
        cmps = set()
        for s in seen:
            c = 0
            while c < 3 and v.data[s + c] == v.data[p + c]:
                c += 1
            cmps.add(c)
        assert cmps == {0, 1, 3}
        _is(v, p, (8, p - q1))  # found behind five candidates that are not matches
    case("same_hash_cmp", u.d, "k_zprev / k_zinfo: three trigrams with one hash interleaved (cmp 0, 1, >= 3)", check)


# ---- k_zinfo -----------------------------------------------------------------------------------
EDGES = (16384, 32768, 49152)


def _m258():
    for which in ("dst", "src"):
        for k in (-258, -257, -100, -1, 0):
            d = noisy(10 + k % 7, 49152 + 3600)
            sites = []
            for i, s in enumerate(EDGES):
                P = plant(20 + i, 258)
                src = s + k if which == "src" else s + k - 3000
                dst = src + 3000
                d[src:src + 258], d[dst:dst + 258] = P, P
                d[src - 1], d[dst - 1] = 32, 33
                sites.append(dst)

            def check(v, sites=sites):
                for dst in sites:
                    _is(v, dst, (258, 3000))
                    assert v.trace.visits.get(dst + 1) == 258 and dst + 2 not in v.trace.visits
            case("m258_%s_%d" % (which, k), d,
                 "k_zinfo: a 258-byte match whose %s starts at slab edge %+d (16384, 32768, 49152)" % (which, k), check)


def _dist_head():
    for name, (d1, d2) in (("a", (32506, 32507)), ("b", (32507, 32506))):
        d = noisy(30, 49152 + 300)
        P1, P2 = bytes(range(48, 56)), bytes(range(56, 64))
        for p, dist, P in ((40000, d1, P1), (49152, d2, P2)):
            d[p - dist:p - dist + 8], d[p:p + 8] = P, P
            d[p - dist - 1], d[p - 1] = 32, 33
            d[p - dist + 8], d[p + 8] = 34, 35

        def check(v, d1=d1, d2=d2):
            for p, dist in ((40000, d1), (49152, d2)):
                if dist == MAX_DIST:
                    _is(v, p, (8, MAX_DIST))
                else:
                    assert all(v.literal(p + i) for i in range(6)), (p, [v.at.get(p + i) for i in range(6)])
        case("dist_head_" + name, d, "k_zinfo: hash head at distance %d from 40000 and %d from 49152: 32506 is "
             "taken, 32507 is not" % (d1, d2), check)


def _chain_cut():
    d = noisy(31, 45300)
    X1, X2 = bytes(range(48, 56)), bytes(range(56, 64))
    for p, q, mid, X, other in ((40000, 40000 - MAX_DIST, 20000, X1, 60), (45000, 45001 - MAX_DIST, 25000, X2, 50)):
        d[q:q + 8], d[p:p + 8] = X, X
        d[mid:mid + 5] = X[:4] + bytes([other])
        d[q - 1], d[mid - 1], d[p - 1] = 32, 33, 34
        d[q + 8], d[p + 8] = 34, 35

    def check(v):
        pv = v.trace.prev
        assert pv[40000] == 20000 and pv[20000] == 40000 - MAX_DIST  # prev(cur) == limit: cut
        assert pv[45000] == 25000 and pv[25000] == 45001 - MAX_DIST  # limit + 1: walked
        _is(v, 40000, (4, 20000))
        _is(v, 45000, (8, MAX_DIST - 1))
    case("chain_cut", d, "k_zinfo: the chain's next candidate exactly at limit (dropped) and at limit + 1 (taken)",
         check)


def _two_nice():
    S = plant(6, 60)
    u = Uniq(6).reserve(S, S[:40] + b"\x30")
    u.fill(20)
    q1 = u.put(S)
    u.fill(9)
    q2 = u.put(S[:40] + bytes([S[40] ^ 1]))
    u.fill(9)
    p = u.put(S)
    u.fill(9)

    def check(v):
        # the nearer candidate (40 bytes) ends the search where 40 >= nice; else the longer one wins
        _is(v, p, (40, p - q2) if v.nice <= 40 else (60, p - q1))
    case("two_nice", u.d, "k_zinfo: two candidates reaching nice = 16 / 32: the first on the chain wins", check)


def _end_lookahead():
    T = plant(7, 20)
    u = Uniq(7).reserve(T)
    u.fill(30)
    u.put(T)
    u.fill(11)
    q2 = u.put(T)
    u.fill(13)
    p = u.put(T)

    def check(v):
        assert p + 20 == len(v.data) and (20 < v.nice or v.level == 4)
        _is(v, p, (20, p - q2))
        assert v.trace.rec(p, False) == (20, q2)
    case("end_lookahead", u.d, "k_zinfo: a candidate reaching the lookahead (20 < nice) at the member's end", check)


def _chain_positions():
    T1, T2 = plant(8, 12), plant(9, 12, 32, 48)
    u = Uniq(8).reserve(T1, T2)
    u.fill(16)
    sites = {}
    for T, weak, key in ((T1, 8, "p9"), (T2, 32, "p33")):
        q = u.put(T)
        u.fill(5)
        for _ in range(weak):
            u.put(T[:3])
            u.fill(4)
        sites[key] = (u.put(T), q)
        u.fill(6)

    def check(v):
        p, q = sites["p9"]
        _is(v, p, (12, p - q))  # ninth on the chain: inside every level's chain
        p, q = sites["p33"]
        if v.chain > 32:
            _is(v, p, (12, p - q))
        else:  # the 33rd candidate is out of reach: a length-3 match, deferred by the one at p + 1
            assert v.literal(p)
            _is(v, p + 1, (11, p - q))
    case("chain_positions", u.d, "k_zinfo: the best candidate 9th and 33rd on the chain (levels 4, 5, 6 disagree)",
         check)


def _quarter():
    u = Uniq(9)
    plants = [(plant(10, 12), 8, 5), (plant(11, 12), 32, 6)]
    u.reserve(*[U for U, _, _ in plants])
    u.fill(16)
    sites = {}
    for U, weak, level in plants:
        q = u.put(U)
        u.fill(5)
        r = u.put(b"\x2f" + U[:8] + b"\x2e")  # G = one byte + U[:8], then a byte that ends the match
        u.fill(5)
        for _ in range(weak):
            u.put(U[:3])
            u.fill(4)
        g = u.put(b"\x2f" + U)
        u.fill(6)
        sites[level] = (g, r, q)

    def check(v):
        if v.level not in sites:
            return
        g, r, q = sites[v.level]
        t = v.trace
        assert t.visits.get(g + 1) == 9 and v.good <= 9 < v.lazy  # searched with the quarter chain
        assert t.rec(g + 1, True) == (3, g - 7) and t.rec(g + 1, False) == (12, q)
        _is(v, g, (9, g - r))  # the quarter chain's answer: the 12-byte match is not seen
    case("quarter_chain", u.d, "k_zinfo / k_zparse: prev_length >= good at a position whose quarter chain and full "
         "chain give different answers (level 5 and level 6 sites)", check)


# ---- k_zparse ----------------------------------------------------------------------------------
def _defer3():
    W = plant(12, 10)
    u = Uniq(12).reserve(W)
    u.fill(12)
    for a, b in ((0, 4), (1, 6), (2, 8), (3, 10)):
        u.put(W[a:b] + b"\x2f")
        u.fill(5)
    p = u.put(W)
    u.fill(8)

    def check(v):
        assert v.literal(p) and v.literal(p + 1) and v.literal(p + 2)
        assert v.at[p + 3][0] == 7
        assert [v.trace.visits.get(p + i) for i in range(1, 5)] == [4, 5, 6, 7]
    case("defer3", u.d, "k_zparse: a match deferred by a longer one at p + 1, three times in a row", check,
         levels=(5, 6, 9))  # (level 4 stops looking at prev_length >= max_lazy = 4)


def _max_lazy():
    W = plant(13, 21)
    u = Uniq(13).reserve(W)
    u.fill(12)
    q = u.put(W[:16] + b"\x2f")
    u.fill(5)
    u.put(W[1:21] + b"\x2e")
    u.fill(5)
    p = u.put(W)
    u.fill(8)

    def check(v):
        if v.lazy <= 16:  # no search at p + 1: the longer match there is never seen
            _is(v, p, (16, p - q))
            assert v.trace.visits.get(p + 1) == 16
        else:
            assert v.literal(p) and v.at[p + 1][0] == 20
    case("max_lazy", u.d, "k_zparse: prev_length >= max_lazy, so the longer match at p + 1 is not searched", check)


def _too_far():
    A, B2 = b"\x30\x31\x32", b"\x33\x34\x35"
    u = Uniq(14).reserve(A, B2)
    u.fill(100)
    qa = u.put(A)
    u.fill(50)
    qb = u.put(B2)
    u.fill_to(qa + 4096)
    u.put(A)
    u.fill_to(qb + 4097)
    u.put(B2)
    u.fill(20)

    def check(v):
        _is(v, qa + 4096, (3, 4096))
        assert all(v.literal(qb + 4097 + i) for i in range(3))
        assert v.trace.rec(qb + 4097, False) == (3, qb)  # found, then dropped by the parse
    case("too_far", u.d, "k_zparse: a length-3 match at distance 4096 (kept) and 4097 (TOO_FAR: dropped)", check)


def _window_jumps():
    P = [plant(15, 258), plant(16, 128), plant(17, 128)]
    u = Uniq(15).reserve(*P)
    u.fill(7)
    src = []
    for x in P:
        src.append(u.put(x))
        u.fill(3)
    dst = []
    for x, lane in zip(P, (62, 63, 0)):
        o = (len(u) + 70) // 64 * 64 + lane
        u.fill_to(o)
        dst.append(u.put(x))
        u.fill(3)
    u.fill(40)

    def check(v):
        for o, s, n in zip(dst, src, (258, 128, 128)):
            _is(v, o, (n, o - s))
        vis = v.trace.order
        o = dst[0]  # emitted at window lane 63: the next record is 320 past the window's start
        assert (o + 1) % 64 == 63 and vis[vis.index(o + 1) + 1] == o + 258 == (o + 1) // 64 * 64 + 320
        for o, land in ((dst[1], 127), (dst[2], 128)):
            w0 = (o + 1) // 64 * 64
            assert vis[vis.index(o + 1) + 1] == w0 + land
    case("window_jumps", u.d, "k_zparse: a 258 match emitted at window lane 63; jumps landing at w0 + 127 (shift "
         "path) and w0 + 128 (reload path)", check)


def _token_counts():
    for n in (1, 63, 64, 65, 128, 255, 256, 257):
        u = Uniq(100 + n).fill(n)

        def check(v, n=n):
            assert v.trace.ntok == n and all(isinstance(t, int) for t in v.trace.tokens())
            assert isinstance(dp.all_tokens(v.blocks)[-1], int)  # the member ends with a pending literal
        case("tokens_%d" % n, u.d, "k_zparse / k_zemit: %d tokens (token groups of 64; emit threads with empty "
             "ranges)" % n, check)
    big = Uniq(20).fill(16383 + 64)

    def check(v):
        assert [b.nsyms for b in v.blocks] == [16383, 64] and isinstance(v.blocks[0].tokens[-1], int)
        assert v.trace.ntok == 16383 + 64
    case("tokens_16447", big.d, "k_zparse: 16383 + 64 tokens; the block's 16383rd symbol is a literal", check)
    for name, more in (("sym16383_match", 100), ("final_empty", 0)):
        u = Uniq(20).fill(16382)
        u.copy(100, 40)
        u.fill(more)

        def check(v, more=more):
            assert [b.nsyms for b in v.blocks] == [16383, more]
            assert v.blocks[0].tokens[-1] == (40, 16282)
            if not more:  # the match ends the member: an empty final block, which goes static
                assert v.blocks[1].kind == dp.FIXED and v.blocks[1].final
                assert len(v.data) == 16382 + 40
        case(name, u.d, "k_zparse / k_ztrees / k_zemit: the 16383rd symbol is a match" +
             ("" if more else " that also ends the member (empty final block)"), check)
    u = Uniq(21).fill(50)
    u.copy(10, 10)
    u.fill(1)

    def check(v):
        t = dp.all_tokens(v.blocks)
        assert isinstance(t[-1], int) and t[-2] == (10, 40)
    case("pending_literal", u.d, "k_zparse: the member ends with a pending literal right after a match", check)


def _slides():
    for at in (32767, 32768, 32769):
        d = noisy(40, PAYLOAD)
        P = bytes(range(48, 56))
        p2 = at + MAX_DIST
        d[at:at + 8], d[p2:p2 + 8] = P, P
        d[p2 - 8:p2] = bytes(range(56, 64))  # never seen before: the parse arrives at p2 with no match
        d[at + 8], d[p2 + 8] = 34, 35

        def check(v, at=at, p2=p2):
            assert len(v.data) == PAYLOAD and p2 - at == MAX_DIST
            if at == WSIZE:  # the slide NILs the head entry 32768 seen from 65274
                assert p2 == SLIDE_AT and v.literal(p2)
                _is(v, p2 + 1, (7, MAX_DIST))
                assert v.trace.prev[p2] == WSIZE and v.trace.rec(p2, False) == (0, 0)
            else:
                _is(v, p2, (8, MAX_DIST))
        case("slide_%d" % at, d, "k_zinfo: the head at %d seen from %d at distance 32506 (the window slide NILs "
             "exactly 32768)" % (at, p2), check)


# ---- k_ztrees ----------------------------------------------------------------------------------
def _dist_codes():
    u = Uniq(22).fill(600)

    def check(v):
        b, = v.blocks
        assert b.kind == dp.DYNAMIC and not b.matches() and b.dist_lens == [1, 1]
    case("no_match_block", u.d, "k_ztrees: no match in the block: the distance tree gets its two forced codes", check)
    u = Uniq(23).fill(600)
    u.copy(300, 6)
    u.fill(50)
    u.copy(360, 6)
    u.fill(50)

    def check(v):
        b, = v.blocks
        assert b.kind == dp.DYNAMIC and b.matches() == [(6, 300), (6, 296)]
        assert [i for i, n in enumerate(b.dist_lens) if n] == [0, 16] and b.dist_lens[16] == 1
    case("one_dist_code", u.d, "k_ztrees: exactly one distance code used (the second is forced)", check)


def _static_tie():
    for n in range(8, 200):
        for seed in range(4):
            data = rnd(1000 * seed + n, n, 97, 101)
            b = Trace(data, 5).blocks
            if len(b) == 1 and b[0][5] == ZB_STATIC and b[0][6] == b[0][7]:
                def check(v):
                    tb = v.trace.blocks
                    if v.level == 5:
                        assert tb[0][5] == ZB_STATIC and tb[0][6] == tb[0][7]  # static_lenb == opt_lenb
                        assert [k.kind for k in v.blocks] == [dp.FIXED]
                return case("static_tie", data, "k_ztrees: static_lenb == opt_lenb (level 5): the tie goes static",
                            check)
    raise ValueError("no static / dynamic tie in 8..199 bytes of a 4-letter alphabet, 4 seeds each")


def _dsd():
    """dynamic, stored, dynamic; the stored block starting at each of the 8 bit phases."""
    mid = rnd(50, 16500, 0, 256)
    tail = Uniq(51).fill(900).d
    found = {}
    for seed in range(200):
        if len(found) == 8:
            break
        data = bytes(Uniq(600 + seed).fill(16383).d) + mid + bytes(tail)
        b0 = dp.parse(zlib_raw(data, 5), max_blocks=1)[0]
        if b0.kind == dp.DYNAMIC and b0.nsyms == 16383:
            found.setdefault(b0.end % 8, data)
    if len(found) != 8:
        raise ValueError("stored-block bit phases found in 200 seeds: %s" % sorted(found))
    for ph in range(8):
        def check(v, ph=ph):
            assert [b.kind for b in v.blocks] == [dp.DYNAMIC, dp.STORED, dp.DYNAMIC]
            if v.level == 5:
                assert v.blocks[1].start % 8 == ph
            # an emit thread's token range begins inside the stored block and ends in the next one
            tb, n = v.trace.blocks, v.trace.ntok
            K = (n + 255) // 256
            assert tb[1][5] == ZB_STORED and any(tb[1][0] < t * K < tb[1][1] < (t + 1) * K for t in range(256))
        case("dsd_phase_%d" % ph, found[ph], "k_ztrees / k_zemit: dynamic, stored, dynamic blocks; the stored block "
             "starts at bit phase %d" % ph, check)


def huff_depth(freqs):
    """Depth of the unrestricted Huffman tree over the non-zero frequencies (ties: shallower first)."""
    import heapq
    h = [(f, 0) for f in freqs if f]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1] if h else 0


def _skewed_distances():
    """Length-4 copies of windows of a Uniq base, each window used once, at distances chosen by
    their code: distance code c is used fib(c) times, so the distance tree's shape is chosen freely
    (LZ cannot absorb a distance).  Rare codes are the near ones and go first, while the base is
    still within their reach."""
    from deflate_build import DIST_BASE
    fib = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597]
    u = Uniq(24).fill(16383 + 300)  # block 0: 16383 literals; the copies fall into block 1
    base_end, taken, n_copy = len(u), set(), 0
    for c, f in zip(range(14, 30), fib):
        for _ in range(f):
            u.fill(1)
            pos = len(u)
            lo, hi = DIST_BASE[c], (DIST_BASE[c + 1] if c < 29 else 32769)
            for src in range(max(pos - hi + 1, 0) // 2 * 2 + 2, min(pos - lo, base_end - 4) + 1, 2):
                if src not in taken:
                    break
            else:
                raise ValueError("no unused base window at distance code %d from %d" % (c, pos))
            taken.add(src)
            u.copy(src, 4)
            n_copy += 1
    # the one use of distance code 13, with a rare length code: a token wider than 32 bits
    u.fill(3)
    u._filled = False  # (the copy's source ends at the last filler byte: leave it as it is)
    far = u.put(bytes(u.d[-100:]) * 2)
    u.fill(5)

    def check(v):
        b = v.blocks[1]
        assert v.blocks[0].nsyms == 16383 and b.kind == dp.DYNAMIC
        from deflate_build import dist_code
        f = [0] * 30
        for _, d in b.matches():
            f[dist_code(d)] += 1
        assert sum(f) >= n_copy
        assert huff_depth(f) > 15 and max(b.dist_lens) == 15  # gen_bitlen's overflow repair ran
        assert max(b.widths) > 32 and v.at[far] == (200, 100) and b.widths[b.tokens.index((200, 100))] > 32
    case("dist_cap15", u.d, "k_ztrees / k_zemit: Fibonacci distance-code counts: the distance tree overflows 15 bits "
         "(overflow repair); one token wider than 32 bits", check)


def literals_without_matches(counts, seed):
    """A byte string with counts[b] occurrences of every byte b and no trigram twice (so no match),
    drawn at random by the remaining counts; None when the draw gets stuck."""
    r, left, out, seen = random.Random(seed), dict(counts), bytearray(), set()
    total = sum(left.values())
    while total:
        for _try in range(200):
            k = r.randrange(total)
            for b, c in left.items():
                k -= c
                if k < 0:
                    break
            if len(out) < 2 or (out[-2], out[-1], b) not in seen:
                break
        else:
            return None
        if len(out) >= 2:
            seen.add((out[-2], out[-1], b))
        out.append(b)
        left[b] -= 1
        total -= 1
    return bytes(out)


def _bl_cap7():
    """Literals only, with dyadic counts, so that the literal tree's lengths are known in advance:
    59 codes of 6 bits, 1 of 7, 4 of 8, 11 of 9, 9 of 10, 38 of 11 and 24 of 12 (one of them the
    end of block), equal lengths never adjacent.  With the two forced 1-bit distance codes and the
    two runs of zeros, the code-length symbols' counts need an 8-bit code: gen_bitlen repairs it
    to 7.  (The counts come from a random search over Kraft-complete length sets.)"""
    lens = {6: 59, 7: 1, 8: 4, 9: 11, 10: 9, 11: 38, 12: 23}
    order, prev = [], None
    left = dict(lens)
    while sum(left.values()):
        ln = max((k for k in left if left[k] and k != prev), key=lambda k: left[k])
        order.append(ln)
        left[ln] -= 1
        prev = ln
    counts = {64 + i: 1 << (12 - ln) for i, ln in enumerate(order)}
    for seed in range(20):
        data = literals_without_matches(counts, seed)
        if data is not None:
            break
    else:
        raise ValueError("bl_cap7: no match-free arrangement in 20 seeds")

    def check(v):
        b, = v.blocks
        assert b.kind == dp.DYNAMIC and not b.matches()
        assert [b.lit_lens[64 + i] for i in range(len(order))] == order
        assert huff_depth([b.cl_syms.count(x) for x in range(19)]) > 7 and max(b.cl_lens) == 7
    case("bl_cap7", data, "k_ztrees: the code-length tree overflows 7 bits (gen_bitlen's repair on bl_tree)", check)


def _lit_cap15():
    """Match lengths cannot be absorbed by LZ either: copies of unused windows of a Uniq base with
    Fibonacci counts per length code, under ~220 uses of each of 64 literals: the chain of rare
    length codes hangs below the literals and the literal/length tree overflows 15 bits."""
    fib = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233]  # (the end of block is the sequence's first 1)
    lengths = [22, 18, 16, 14, 12, 10, 9, 8, 7, 6, 5, 4]  # codes 269, 268, ..., 258
    u = Uniq(25).fill(14000)
    src = 8
    for ln, f in zip(lengths, fib):
        for _ in range(f):
            u.fill(1)
            u.copy(src, ln)
            src += ln + 2
    u.fill(4)
    assert src < 13000

    def check(v):
        b, = v.blocks
        from deflate_build import len_code
        f = [0] * 286
        for t in b.tokens:
            f[257 + len_code(t[0]) if isinstance(t, tuple) else t] += 1
        f[256] = 1
        assert sorted(x for x in f[257:] if x) == sorted(fib)
        assert b.kind == dp.DYNAMIC and huff_depth(f) > 15 and max(b.lit_lens) == 15
    case("lit_cap15", u.d, "k_ztrees: Fibonacci length-code counts under the literals: the literal/length tree "
         "overflows 15 bits (overflow repair)", check)


# ---- k_zemit -----------------------------------------------------------------------------------
def _fallback():
    want = {65516, 65517, 65518, 65519}
    found = {}
    for seed in range(3):
        base = rnd(60 + seed, PAYLOAD, 0, 256)
        for n in (PAYLOAD, PAYLOAD - 1):
            for tail in range(0, 48):
                for fillb in (0, 255):
                    d = base[:n - tail] + bytes([fillb]) * tail
                    size = len(zlib_raw(d, 5))
                    if size in want and size not in found and (n == PAYLOAD or size == 65517):
                        found[size] = d
        if len(found) == 4:
            break
    missing = sorted(want - set(found))
    for size in sorted(found):
        def check(v, size=size):
            if v.level == 5:
                assert len(v.raw) == size
        case("fallback_%d" % size, found[size], "k_zemit: a level-5 stream of %d bytes (%s htsjdk's 65518-byte "
             "buffer: %s)" % (size, "fits" if size < OUT_CAP else "fills", "kept" if size < OUT_CAP else
                              "level-0 fallback"), check)
    return missing


_lengths()
_step_one_hash()
_pair_63_64()
_hash_every_step()
_same_hash_cmp()
_m258()
_dist_head()
_chain_cut()
_two_nice()
_end_lookahead()
_chain_positions()
_quarter()
_defer3()
_max_lazy()
_too_far()
_window_jumps()
_token_counts()
_slides()
_dist_codes()
_static_tie()
_dsd()
_skewed_distances()
_bl_cap7()
_lit_cap15()
FALLBACK_MISSING = _fallback()

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FULL = [c for c in CASES if c.full]


def pairs():
    """(case, level) for every run."""
    return [(c, lv) for c in CASES for lv in c.levels]


def pair_id(p):
    return "%s-L%d" % (p[0].name, p[1])
