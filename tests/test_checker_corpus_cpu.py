"""The checker corpus against the CPU oracle, and the coverage its table claims (no GPU).

tests/checker_corpus.py writes the checkers' answers down by hand from the Scala; the oracle
(oracle/sbam_oracle.c: eager_check, full_check) is this project's own reading of the same Scala.
Here the oracle is held to every literal, on every layout, so that the GPU suite
(test_checker_conformance_gpu.py) compares the kernels with an oracle that is itself pinned."""
import numpy as np
import pytest

import checker_corpus as cc

RTCS = (10, 1, 2, 3, 0)
LAYOUTS = [(k, c, 0) for k in ("long", "short", "segmented") for c in ("BIG", "SMALL")] + [("short", "BIG", 15)]


def check_literals(lay, rtcs=RTCS):
    ctg = np.asarray(lay.contigs, np.int32)
    segs = cc.oracles(lay)
    bad = []
    for p, f in lay.probes:
        of, base = next((o, a) for (o, a), (a0, b0) in zip(segs, lay.segments) if a0 <= f < b0)
        for rtc in rtcs:
            w, e = of.full(f - base, rtc, ctg), of.eager(f - base, rtc, ctg)
            if w != cc.word(p, rtc) or e != cc.eager(p, rtc):
                bad.append((p.label, rtc, hex(w), hex(cc.word(p, rtc)), e))
    assert not bad, bad[:20]


@pytest.mark.parametrize("kind,ctg,shift", LAYOUTS)
def test_oracle_gives_every_literal(kind, ctg, shift):
    check_literals(cc.layout(kind, ctg, shift))


@pytest.mark.parametrize("label", [p.label for p in cc.END_CASES])
def test_oracle_gives_every_end_literal(label):
    """At the end of a segment that an empty member closes, and at the end of the file."""
    lay = cc.end_layout(label)
    assert [f + len(p.data) for p, f in lay.probes] == [b for _, b in lay.segments]
    check_literals(lay)


def test_table_holds_the_seed_words():
    """The words worked out by hand before the table was written, as the table now states them
    (constants against cc.word: the oracle is not asked here).  Two of them, `idx 0, pos 16571`
    and `idx -1, pos 2**31 - 1`, were first checked as a minimal record alone at the end of a
    stream (0x80100000, Success(1)); in the table a runway follows them, so the word is
    Success(10) = 0x80a00000."""
    w = {p.label: cc.word(p, 10) for p in cc.PROBES + cc.END_CASES}
    assert w["end_clean_1"] == 0x80100000 and w["end_minimal_one_short"] == 0x200
    assert w["refpos_SMALL_read_-2_-2"] == 0xa and w["refpos_SMALL_read_3_-2"] == 0xc
    assert w["refpos_SMALL_read_0_16571"] == 0x80a00000 and w["refpos_SMALL_read_0_16572"] == 0x10
    assert w["refpos_SMALL_read_-1_2147483647"] == 0x80a00000
    assert w["mapped_no_cigar_no_seq"] == 0x30000
    assert w["name_at"] == w["name_del"] == w["name_space"] == 0x800 and w["name_AB"] == 0x400
    assert w["cigar_op_nibble9"] == 0x8000 and w["end_cut_inside_op"] == 0x4000
    assert w["end_abnormal_min"] == 0x200001 and w["lseq_max_bs_max"] == 0x100001


def test_table_coverage():
    """What the table holds, computed from the table."""
    every = cc.PROBES + cc.HEAVY + cc.END_CASES
    words = [cc.word(p, 10) for p in every]
    seen = 0
    for w in words:
        if not w & cc.SUCCESS:
            seen |= w & 0x7FFFF
    assert seen == 0x7FFFF, [cc.FLAGS[i] for i in range(19) if not seen >> i & 1]
    alone = {w & 0x7FFFF for w in words if not w & cc.SUCCESS}
    for i, name in enumerate(cc.FLAGS):
        assert 1 << i in alone, f"{name} never alone"
    assert {p.n for p in every if p.how[0] == "flags"} >= {0, 1, 2, 3}
    assert {p.n for p in every if p.how[0] == "end"} >= {1, 2, 3, 9}
    # getRefPosError's eight outcomes (PosChecker.scala:47-62), both pairs, both dictionaries
    for ctg in ("SMALL", "BIG"):
        for pair in ("read", "mate"):
            got = {p.tags["refpos"][1] for p in cc.PROBES if p.ctg == ctg and p.tags.get("refpos", ("",))[0] == pair}
            assert got >= {0, 1, 1 | 4, 2, 2 | 4, 4, 8}, (ctg, pair, got)   # None + the seven errors
            idx = {p.tags["refpos"][2] for p in cc.PROBES if p.ctg == ctg and p.tags.get("refpos", ("",))[0] == pair}
            n = len(cc.DICTS[ctg])
            assert idx >= {-2, -1, 0, n - 1, n}, (ctg, pair)
    big = {p.tags["refpos"][2:] for p in cc.PROBES if p.ctg == "BIG" and "refpos" in p.tags}
    for i in (1023, 1024, 1499):
        assert (i, 1000 + i) in big and (i, 1001 + i) in big       # pos == len, len + 1 past FCTG
    small = {p.tags["refpos"][2:] for p in cc.PROBES if p.ctg == "SMALL" and "refpos" in p.tags}
    assert {(-1, cc.I32_MAX), (0, -2), (0, -1), (0, 0), (0, 16571), (0, 16572), (2, cc.I32_MAX)} <= small
    assert len(cc.BIG) > cc.FCTG and cc.I32_MAX in cc.SMALL
    # read names
    assert {p.tags["name_len"] for p in cc.PROBES if "name_len" in p.tags} == set(cc.NAME_LENGTHS)
    for n in cc.NAME_LENGTHS[2:]:
        at = {p.tags["bad_at"] for p in cc.PROBES if p.tags.get("name_len") == n and "bad_at" in p.tags}
        assert at == {a for a in cc.BAD_AT if a < n - 1}, n
        assert all(0x40 in {p.tags["bad_byte"] for p in cc.PROBES if p.tags.get("name_len") == n and
                            p.tags.get("bad_at") == a} for a in at)
    assert {p.tags["bad_byte"] for p in cc.PROBES if "bad_byte" in p.tags} == set(cc.BAD_BYTES)
    assert {p.tags["ok_byte"] for p in cc.PROBES if "ok_byte" in p.tags} == set(cc.EDGE_OK_BYTES)
    assert {p.tags["past_nul"] for p in cc.PROBES if "past_nul" in p.tags} == {2, 33}
    assert {p.tags["second_name"] for p in cc.PROBES if "second_name" in p.tags} == {0x20, 0x40, 0x7F}
    # CIGARs
    assert {p.tags["n_ops"] for p in every if "n_ops" in p.tags} == set(cc.OP_COUNTS)
    assert {p.tags["n_ops"] for p in every if p.tags.get("bad_op", 0) is None} == set(cc.OP_COUNTS[:-1])
    assert {p.tags["bad_op"] for p in every if p.tags.get("bad_op") is not None} >= set(cc.BAD_OP_AT)
    assert {p.tags["n_ops"] for p in every if p.tags.get("last")} == set(cc.OP_COUNTS[1:])
    assert {p.tags["nibble"] for p in every if "nibble" in p.tags} == {8, 9}
    assert {p.tags["high_ff"] for p in every if "high_ff" in p.tags} == {8, 9}
    assert {p.tags["long_bs"] for p in every if "long_bs" in p.tags} == {(b, n) for b in (cc.XQ_MIN_REC - 1, cc.XQ_MIN_REC)
                                                                          for n in (cc.XQ_MIN_OPS - 1, cc.XQ_MIN_OPS, 33)}
    assert {p.tags["swap"] for p in every if "swap" in p.tags} >= {"both", "n_cigar == 0", "l_seq == 0", "neither"}
    # arithmetic, abnormal records, the end of the stream
    assert {p.tags["arith"] for p in every if "arith" in p.tags} >= {
        "l_seq -1", "l_seq -1000", "l_seq 0x7FFFFFFF", "l_seq 0x80000000", "block_size implied",
        "block_size implied - 1", "block_size 0x7FFFFFFF", "implied wraps negative"}
    assert sum(1 for p in every if p.tags.get("abnormal")) >= 8
    assert {p.tags["clean"] for p in cc.END_CASES if "clean" in p.tags} == {1, 2, 9}
    assert {p.tags["past"] for p in cc.END_CASES if "past" in p.tags} == {1, 35}
    assert {p.tags["cut"] for p in cc.END_CASES if "cut" in p.tags} == {"fixed", "name", "between ops", "inside op"}
    assert {p.tags["order"] for p in cc.END_CASES if "order" in p.tags} >= {"bad op first", "cut first"}
    assert len({p.label for p in every}) == len(every)


def test_layout_geometry():
    """`long` stays below 1 MB and every probe's tile and its successor are fast tiles wherever a
    tile may start; `short` and `segmented` have no fast tile; probes are 16-aligned plus the shift."""
    for ctg in ("BIG", "SMALL"):
        lay = cc.layout("long", ctg)
        assert len(lay.flat) < 1000000
        first = lay.probes[0][1]
        assert first >= cc.EW
        for p, f in lay.probes:
            assert f % 16 == 0 and cc.fast_tile(lay, f + len(p.data) + cc.FTILE), p.label
        for kind in ("short", "segmented"):
            lay = cc.layout(kind, ctg)
            assert not any(cc.fast_tile(lay, a) for a, _ in lay.segments)
    assert all(f % 16 == 15 for _, f in cc.layout("short", "BIG", 15).probes)
    assert len(cc.layout("segmented", "BIG").segments) == 2


@pytest.fixture(scope="module")
def long_big():
    lay = cc.layout("long", "BIG")
    (of, _), = cc.oracles(lay)
    return lay, of


def test_pass16_is_one_success_in_sixteen(long_big):
    lay, of = long_big
    a, b = lay.sections["PASS16"]
    assert a % 16 == 0
    _, _, _, w1 = of.full_range(a, a + 3 * cc.FTILE, reads_to_check=1, want_words=True)
    ok = (w1 & cc.SUCCESS) != 0
    assert np.array_equal(np.flatnonzero(ok), np.arange(0, 3 * cc.FTILE, 16))
    assert all(int(ok[t * cc.FTILE:(t + 1) * cc.FTILE].sum()) == cc.SLOWCAP for t in range(3))
    _, _, _, w10 = of.full_range(a, a + 3 * cc.FTILE, reads_to_check=10, want_words=True)
    assert set(w10[::16].tolist()) == {cc.PASS16_WORD_RTC10}
    assert not ((w10 & cc.SUCCESS) != 0).any()


def test_close16_overfills_the_close_call_buffer(long_big):
    lay, of = long_big
    a, b = lay.sections["CLOSE16"]
    assert a % 16 == 0 and b - a >= cc.FTILE
    _, _, _, w = of.full_range(a, a + cc.FTILE, want_words=True)
    assert set(w[::16].tolist()) == {cc.CLOSE16_WORD}
    nnz = np.array([bin(int(x) & 0x7FFFF).count("1") + ((int(x) >> 20 & 0x3FF) > 0) for x in w])
    assert int(((nnz <= 2) & ((w & cc.SUCCESS) == 0)).sum()) > cc.FCCAP


def test_ops11_matches_its_rule(long_big):
    lay, of = long_big
    a, b = lay.sections["OPS11"]
    bad = cc.ops11_bad(a)
    assert all(a < x < b for x in bad) and all(lay.flat[x] == 0x19 for x in bad)
    assert {x % 4 for x in bad} == {0, 1, 2, 3}
    assert {x % 1024 for x in bad} >= {31, 32, 1023, 0, 1}
    # (the literal example of the rule: B = 21505 gives positions 3980, 3984, ..., 21452)
    hit = [p for p in range(0, 30000) if cc.ops11_word(p, (21505,)) != cc.OPS11_WORD]
    assert hit == list(range(3980, 21453, 4)) and len(hit) == 4369
    _, _, _, w = of.full_range(a, b, want_words=True)
    clean = np.ones(b - a, bool)
    clean[b - a - cc.OPS11_CIGAR_AT + 1:] = False      # header or name bytes past the section
    for x in bad:
        clean[max(0, x - a - cc.OPS11_CIGAR_AT + 1):x - a + 1] = False     # a bad byte among the 53 bytes before the ops
    want = np.full(b - a, cc.OPS11_WORD, np.uint32)
    for x in bad:
        first = x - cc.OPS11_CIGAR_AT - 4 * (cc.OPS11_OPS - 1)
        want[first - a:x - cc.OPS11_CIGAR_AT - a + 1:4] |= cc.BAD_OP
    assert want[clean].tolist().count(cc.OPS11_WORD | cc.BAD_OP) == len(bad) * cc.OPS11_OPS
    assert all(int(want[p - a]) == cc.ops11_word(p, bad) for p in range(a, b, 997))
    d = np.flatnonzero((w != want) & clean)
    assert d.size == 0, (int(d[0]) + a, hex(int(w[d[0]])), hex(int(want[d[0]])))


def test_tally_is_the_oracles():
    """cc.tally (the GPU suite's expected counts, rbe and successes from oracle words) against
    the oracle's own aggregation."""
    lay = cc.layout("short", "BIG")
    (of, _), = cc.oracles(lay)
    for rtc in (1, 10):
        ns, counts, rbe, w = of.full_range(100, len(lay.flat) - 7, rtc, want_words=True)
        c2, r2, ns2, _ = cc.tally(w, 100)
        assert ns == ns2 and np.array_equal(counts, c2) and np.array_equal(rbe, r2)


def test_pass16_overflows_a_wave_survivor_list():
    """k_eager's waves each list the refID survivors of a quarter of the window (EW / 4 positions,
    at most SEGCAP): in PASS16 nine positions of sixteen carry a refID inside BIG, so every wave's
    list overflows and the tile takes the shared-queue fallback."""
    lay = cc.layout("long", "BIG")
    a, b = lay.sections["PASS16"]
    ref = np.frombuffer(lay.flat, np.uint8)[a:b]
    v = (ref[4:-3].astype(np.int64) | ref[5:-2].astype(np.int64) << 8 | ref[6:-1].astype(np.int64) << 16
         | ref[7:].astype(np.int64) << 24)                      # refID of the record at each position
    v = np.where(v >= 1 << 31, v - (1 << 32), v)
    inside = (v >= -1) & (v < len(cc.BIG))
    assert int(inside[:16].sum()) == 9
    share = cc.EW // 4
    assert min(int(inside[k:k + share].sum()) for k in range(0, 3 * cc.ETILE, 997)) > cc.SEGCAP
