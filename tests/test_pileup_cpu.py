"""The host side of per-base allele counts (csrc/pileup_core.h through the library, no GPU):
sbh_pileup_add_host and sbh_pileup_finish_host against the numpy restatement of pileup_corpus.py on
every corpus and against a table worked out by hand, bad kept rows, the argument errors, the two
renderers against literal text, and the grouping of spans into passes.  Every comparison is exact
equality."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from pkg import sb
import depth_corpus as dc
import pileup_corpus as pc
import record_corpus as rc

pm = sys.modules[sb.__name__ + ".pileup"]  # (sb.pileup is the function)
SBH_OK, SBH_E_ARG, SBH_E_BAD_RECORD = 0, sb._lib.SBH_E_ARG, sb._lib.SBH_E_BAD_RECORD
M, I, D, N, S = pc.M, pc.I, pc.D, pc.N, pc.S


def test_constants_are_the_library_s():
    with open(os.path.join(ROOT, "spark-bam_amd", "csrc", "pileup_core.h")) as f:
        src = f.read()
    for name in ("PILE_TILE", "PILE_GROUP", "PILE_LANE_OPS", "PILE_WINDOW"):
        assert int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1)) == getattr(pc, name)
    assert pm.CHANNELS == ("A", "C", "G", "T", "N", "DEL", "INS", "LOWQ")


def host(c, finish=True):
    return sb.pileup_host(np.frombuffer(bytes(c.flat), np.uint8), c.starts, c.spans, pc.N_REF, c.filter, c.min_baseq,
                          finish=finish, min_depth=c.min_depth, call_pct=c.call_pct)


def equals(got, want):
    add, counts, calls, ivs, sizes = got
    assert add == want["add"]
    assert counts.dtype == np.uint32 and np.array_equal(counts, want["counts"])
    assert calls.dtype == np.uint8 and np.array_equal(calls, want["calls"])
    assert ivs.dtype == pc.SPAN_DTYPE and np.array_equal(ivs, want["intervals"])
    assert sizes == want["stats"]
    assert sizes["totals"] == add["totals"]  # the invariant: a finish sees what the adds put in


def test_the_hand_worked_case():
    """Host functions and restatement against literals written by hand (pileup_corpus.HAND)."""
    h, c = pc.HAND, pc.hand_case()
    want = dict(add=h["add"], counts=np.asarray(h["table"], np.int64), calls=np.frombuffer(h["calls"], np.uint8),
                intervals=pc.span_array(h["intervals"]), stats=h["stats"])
    equals(host(c), want)
    r = pc.restate(c.flat, c.starts, c.spans, pc.N_REF, None, c.min_baseq, c.min_depth, c.call_pct)
    assert r["bad_row"] is None and r["add"] == h["add"] and r["stats"] == h["stats"]
    assert r["counts"].tolist() == h["table"] and r["calls"].tobytes() == h["calls"]
    assert [(x[0], x[2], x[3]) for x in r["intervals"].tolist()] == h["intervals"]


@pytest.mark.parametrize("name", pc.CORPORA)
def test_host_is_the_restatement(name):
    c, want = pc.get(name), pc.expected(name)
    assert want["bad_row"] is None
    equals(host(c), want)


def test_corpora_say_what_they_are_for():
    e = pc.expected
    c = e("contention")["counts"]
    assert c[1000:1103].sum(axis=1).tolist() == [20000] * 52 + [40000] + [20000] * 50  # (1052: the D's last base and the I)
    assert c[1052, pc.INS] == 20000 and c[1050:1053, pc.DEL].tolist() == [20000] * 3 and e("contention")["stats"]["max_depth"] == 20000
    assert e("intervals_alternating")["stats"]["n_intervals"] == pc.T // 2 + 1
    iv = [tuple(x) for x in e("intervals_tile_edges")["intervals"].tolist()]
    assert iv == [(0, 0, pc.T - 7, pc.T), (0, 0, 2 * pc.T, 2 * pc.T + 9), (0, 0, 4 * pc.T - 10, 5 * pc.T + 10)]
    assert e("call_edges")["calls"][[10, 20, 30, 40, 50, 60, 70, 80, 90]].tobytes() == b"ANN*NNNTC"
    assert e("call_edges")["counts"][70].tolist() == [0, 0, 0, 0, 0, 0, 0, 4]
    assert e("call_pct_100")["calls"][[10, 80, 90]].tobytes() == b"NTN" and e("call_pct_1")["calls"][[20, 30]].tobytes() == b"AN"
    assert e("wrap_64bit")["add"]["totals"][:5] != [0] * 5 and sum(e("wrap_64bit")["add"]["totals"]) == 50 + 50 + 3
    assert sum(e("pos_minus_one")["add"]["totals"]) == 9 and sum(e("pos_max")["add"]["totals"]) == 1 + 2 + 1 + 1
    assert e("no_seq")["add"]["totals"] == [0, 0, 0, 0, 16, 2, 1, 4]  # (the third read has a SEQ: quality < 255)
    assert e("all_codes")["add"]["totals"] == [2, 2, 2, 2, 25, 0, 0, 0]
    assert e("quality_13")["add"]["totals"][pc.LOWQ] == 4 and e("quality_0")["add"]["totals"][pc.LOWQ] == 0
    assert e("quality_255")["add"]["totals"][pc.LOWQ] == 4 and sum(e("quality_255")["add"]["totals"]) == 6
    assert e("unplaced")["add"] == dict(n=3, n_kept=3, n_counted=1, n_unplaced=2, totals=e("unplaced")["add"]["totals"])
    assert e("grid")["add"]["n_kept"] == pc.GRID_ROWS > 1024 * 256
    comp = e("composite")["counts"]
    assert comp[59:72, pc.INS].sum() == 0 and comp[89, pc.INS] == 1 and comp[114, pc.INS] == 1 and comp[104, pc.INS] == 0
    assert comp[150:160, pc.INS].sum() == 0  # 3S2I4M: the insertion comes before the first aligned base
    a = pc.get("alignments")
    assert sorted({s % 4 for s in a.starts}) == [0, 1, 2, 3]
    # an odd l_seq leaves 0xF in the padding nibble: read as a base it would be an N
    s = pc.get("l_seq_edges")
    flat = np.frombuffer(bytes(s.flat), np.uint8)
    assert flat[s.starts[0] + 36 + 2 + 4] == ((0 % 16) << 4 | 0xF)


def test_adds_accumulate_and_a_row_given_three_times_counts_three_times():
    c = pc.get("rows_reversed_and_tripled")
    flat = np.frombuffer(bytes(c.flat), np.uint8)
    half = len(c.starts) // 2
    add1, counts = sb.pileup_host(flat, c.starts[:half], c.spans, pc.N_REF, finish=False)
    add2, counts = sb.pileup_host(flat, c.starts[half:], c.spans, pc.N_REF, counts=counts, finish=False)
    calls, ivs, sizes = pm.finish_host(counts, c.spans)
    want = pc.expected("rows_reversed_and_tripled")
    assert np.array_equal(counts, want["counts"]) and np.array_equal(calls, want["calls"]) and sizes == want["stats"]
    assert [a + b for a, b in zip(add1["totals"], add2["totals"])] == sizes["totals"]
    once = pc.restate(c.flat, c.starts[:200], c.spans)
    thrice = pc.restate(c.flat, [c.starts[200]] * 3, c.spans)
    assert np.array_equal(want["counts"], once["counts"] + thrice["counts"]) and thrice["counts"].max() == 3


@pytest.mark.parametrize("name", pc.BAD_KEPT)
def test_a_bad_kept_row_is_reported_and_nothing_is_added(name):
    c, row = pc.BAD_KEPT[name]()
    assert pc.restate(c.flat, c.starts, c.spans)["bad_row"] == row
    counts = np.zeros((pc.positions_of(c.spans), 8), np.uint32)
    with pytest.raises(sb.SparkBamError) as e:
        sb.pileup_host(np.frombuffer(bytes(c.flat), np.uint8), c.starts, c.spans, pc.N_REF, counts=counts, finish=False)
    assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (row,) and not counts.any()


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed_rows(m):
    with pytest.raises(sb.SparkBamError) as e:
        sb.pileup_host(np.frombuffer(bytes(m.stream.flat), np.uint8), m.stream.starts, [(1, 0, 2000)], pc.N_REF)
    assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (3,)


def test_depth_s_corpora_count_into_n():
    """depth_corpus's records have no SEQ: every aligned base is an N, and A+C+G+T+N+LOWQ is depth."""
    for name in ("composite", "deletion", "each_op_alone", "handover_counts", "wrap_64bit"):
        c, want = dc.get(name), dc.expected(name)
        add, counts, calls, ivs, sizes = sb.pileup_host(np.frombuffer(bytes(c.flat), np.uint8), c.starts, c.spans, dc.N_REF,
                                                        c.filter)
        assert not counts[:, [0, 1, 2, 3, 7]].any()
        off = d_off = 0
        for _, b, e in c.spans:
            got = counts[off:off + e - b, pc.N_] + (counts[off:off + e - b, pc.DEL] if c.count_del else 0)
            assert np.array_equal(got, want["depth"][d_off:d_off + e - b])
            off, d_off = off + e - b, d_off + e - b + 1


def test_argument_errors():
    c = pc.get("composite")
    flat = np.frombuffer(bytes(c.flat), np.uint8)
    for kw in (dict(min_baseq=-1), dict(min_baseq=256), dict(min_depth=0), dict(call_pct=0), dict(call_pct=101)):
        with pytest.raises(sb.SparkBamError) as e:
            sb.pileup_host(flat, c.starts, c.spans, pc.N_REF, **kw)
        assert e.value.code == SBH_E_ARG, kw
    for spans in ([], [(1, 0, 10), (0, 0, 10)], [(0, 10, 10)], [(pc.N_REF, 0, 10)], [(0, 0, 2 ** 31)]):
        with pytest.raises(sb.SparkBamError) as e:
            sb.pileup_host(flat, c.starts, spans, pc.N_REF, counts=np.zeros((16, 8), np.uint32))
        assert e.value.code == SBH_E_ARG
    with pytest.raises(sb.SparkBamError) as e:
        sb.pileup_host(flat, c.starts, c.spans, pc.N_REF, {"rows": [(5, 5)]})
    assert e.value.code == SBH_E_ARG


def test_finish_writes_only_the_intervals_asked_for():
    c, want = pc.get("intervals_alternating"), pc.expected("intervals_alternating")
    counts = np.ascontiguousarray(want["counts"], np.uint32)
    sp = pc.span_array(c.spans)
    calls = np.zeros(counts.shape[0], np.uint8)
    iv = np.zeros(5, pc.SPAN_DTYPE)
    iv["ref_id"] = -7
    sz = sb._lib.SbhPileupSizes()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert sb.lib().sbh_pileup_finish_host(p(counts), p(sp), 1, 1, 75, p(calls), p(iv), 3, C.byref(sz)) == SBH_OK
    assert sz.n_intervals == want["stats"]["n_intervals"] and np.array_equal(iv[:3], want["intervals"][:3])
    assert iv["ref_id"][3:].tolist() == [-7, -7]


NAMES = ["chrM", "chr10", "chr2", "chr1"]


def test_renderers_against_literal_text():
    h, c = pc.HAND, pc.hand_case()
    add, counts, calls, ivs, sizes = host(c)
    r = sb.PileupResult(ivs, sizes, c.spans, NAMES, [counts], [calls], [n for _, n in rc.CONTIGS])
    assert r.text() == (b"chrM\t101\t1\t0\t0\t0\t0\t0\t0\t0\n"
                        b"chrM\t102\t0\t1\t0\t0\t0\t0\t0\t0\n"
                        b"chrM\t103\t0\t0\t1\t0\t0\t0\t0\t1\n"
                        b"chrM\t104\t0\t0\t0\t3\t0\t0\t0\t0\n"
                        b"chrM\t105\t0\t0\t0\t2\t0\t1\t1\t0\n"
                        b"chrM\t106\t2\t0\t0\t0\t1\t0\t0\t0\n"
                        b"chrM\t107\t0\t2\t0\t0\t0\t0\t0\t0\n"
                        b"chrM\t108\t0\t1\t1\t0\t0\t0\t0\t0\n"
                        b"chrM\t111\t1\t0\t0\t0\t0\t0\t0\t0\n"
                        b"chrM\t112\t0\t0\t0\t0\t1\t0\t0\t0\n"
                        b"chrM\t113\t0\t0\t1\t0\t0\t0\t0\t0\n"
                        b"chrM\t114\t0\t0\t0\t1\t0\t0\t0\t0\n")
    a = r.text(all_positions=True, header=True).split(b"\n")
    assert a[0] == b"#chrom\tpos\tA\tC\tG\tT\tN\tdel\tins\tlowq" and len(a) == 1 + 18 + 1
    assert a[1] == b"chrM\t99\t0\t0\t0\t0\t0\t0\t0\t0" and a[18] == b"chrM\t116\t0\t0\t0\t0\t0\t0\t0\t0"
    assert r.text(header=True) == pm.TEXT_HEADER + r.text()
    assert r.consensus() == b">chrM:99-116\nNNNNNTTACNNNNNNNNN\n"
    assert np.array_equal(r.counts("chrM"), counts) and r.calls("chrM").tobytes() == h["calls"]
    with pytest.raises(KeyError):
        r.counts("chr2")


def test_consensus_drops_deletions_wraps_at_60_and_names_whole_references():
    calls = np.frombuffer(b"A" * 59 + b"*C" + b"\0" + b"G" * 70, np.uint8)
    fa = sb.consensus_fasta([(1, 0, calls.size), (3, 5, 8)], lambda k: calls if k == 0 else calls[:3], NAMES,
                            [1, calls.size, 1, 100])
    assert fa == (b">chr10\n" + b"A" * 59 + b"C\n" + b"N" + b"G" * 59 + b"\n" + b"G" * 11 + b"\n" + b">chr1:6-8\nAAA\n")


def test_span_passes():
    sp = [(0, 0, 10), (1, 0, 10), (2, 5, 10), (3, 0, 20)]
    assert pm.span_passes(sp, 20) == [[(0, 0, 10), (1, 0, 10)], [(2, 5, 10)], [(3, 0, 20)]]
    assert pm.span_passes(sp, 10 ** 6) == [sp]
    with pytest.raises(ValueError) as e:
        pm.span_passes(sp, 19)
    assert "(ref 3, 0, 20)" in str(e.value)


def test_three_passes_are_one_pass():
    """The grouping as api.pileup does it, on the host: each pass adds every record into its own spans
    only; the concatenation is the one-pass answer."""
    recs = [pc.read(10 + 7 * i, [(5, M), (1, I), (2, D), (6, M)], ref=i % 4, seed=i) for i in range(60)]
    spans = [(0, 0, 300), (1, 100, 400), (2, 0, 250), (3, 50, 500)]
    c = pc.case(recs, spans, min_baseq=20, min_depth=2, call_pct=60)
    want = pc.restate(c.flat, c.starts, c.spans, pc.N_REF, None, 20, 2, 60)
    groups = pm.span_passes(spans, 600)
    assert [len(g) for g in groups] == [2, 1, 1]
    flat = np.frombuffer(bytes(c.flat), np.uint8)
    parts = [sb.pileup_host(flat, c.starts, g, pc.N_REF, None, 20, min_depth=2, call_pct=60) for g in groups]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), want["counts"])
    assert np.array_equal(np.concatenate([p[2] for p in parts]), want["calls"])
    assert np.array_equal(np.concatenate([p[3] for p in parts]), want["intervals"])
    assert sum(p[0]["n_counted"] for p in parts) == want["add"]["n_counted"] == 60
    assert [sum(p[4]["totals"][k] for p in parts) for k in range(8)] == want["stats"]["totals"]
