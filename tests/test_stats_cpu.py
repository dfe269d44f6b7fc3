"""The host side of the read-level statistics (csrc/stats_core.h through the library, no GPU):
sbh_stats_add_host against the numpy restatement of stats_corpus.py on every corpus, the invariants,
malformed rows, the argument errors, the Python renderer against a literal, and the bundled 2.bam
against a walk of its SAM text that shares nothing with the restatement."""
import ctypes as C
import gzip
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from pkg import sb
import record_corpus as rc
import stats_corpus as sc
from test_tally_cpu import FLAGSTAT_2BAM, bundled

stm = sys.modules["spark_bam_amd.stats"]  # (sb.stats is api.stats, the function)
SBH_OK, SBH_E_ARG, SBH_E_BAD_RECORD = 0, sb._lib.SBH_E_ARG, sb._lib.SBH_E_BAD_RECORD


def host(c, **kw):
    return sb.stats_host(np.frombuffer(bytes(c.flat), np.uint8), c.starts, c.cycles, c.max_insert, c.filter, **kw)


def sn_of(t):
    return dict(zip(sc.SN, (int(x) for x in t["sn"])))


def test_constants_are_the_library_s():
    with open(os.path.join(ROOT, "spark-bam_amd", "csrc", "stats_core.h")) as f:
        src = f.read()
    for name in ("STAT_QUALS", "STAT_SN", "STAT_LDS_MAX_READ"):
        assert int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1)) == getattr(sc, name)
    assert re.search(r"STAT_CYCLES_MAX = (\d+), STAT_INSERT_MAX = 1u << (\d+);", src).groups() == ("65536", "20")
    assert re.search(r"STAT_LDS_CYCLES = (\d+), STAT_LDS_QUALS = (\d+);", src).groups() == (str(sc.STAT_LDS_CYCLES), str(sc.STAT_LDS_QUALS))
    assert re.search(r"STAT_LDS_LENGTHS = (\d+), STAT_LDS_INSERTS = (\d+);", src).groups() == (str(sc.STAT_LDS_LENGTHS),
                                                                                             str(sc.STAT_LDS_INSERTS))
    for k, name in enumerate(sc.SN):  # the header's table of sn, entry by entry
        assert re.search(r"//\s+(?:.*\s)?%d %s\b" % (k, name), src), name
    with open(os.path.join(ROOT, "include", "sparkbam.h")) as f:
        h = f.read()
    assert "#define SBH_STATS_QUALS %d\n" % sc.STAT_QUALS in h and "#define SBH_STATS_SN %d\n" % sc.STAT_SN in h
    assert sb.SN_ROWS == sc.SN and stm.STATS_QUALS == sc.STAT_QUALS and stm.TABLES == sc.TABLES
    assert stm.table_shapes(8, 16) == sc.shapes(8, 16)


def test_builder_rows_are_rec_s_bytes():
    c = sc.stream(3, 5, [0x10, 0xFFF, 0], [9, 0, 255], [2, -1, 7], [1, -1, 7], None, [4, 5, 6], [-3, 0, 2 ** 31 - 1],
                  seq_byte=[[0x12, 0x48, 0xF3]] * 3, qual=[[1, 2, 3, 4, 5]] * 3)
    for i, (fl, mq, tid, mtid, mpos, tlen) in enumerate(((0x10, 9, 2, 1, 4, -3), (0xFFF, 0, -1, -1, 5, 0), (0, 255, 7, 7, 6, 2 ** 31 - 1))):
        want = rc.rec(tid, i, mq, 4681, fl, mtid, mpos, tlen, b"r" + bytes(6), (), (1, 2, 4, 8, 15), bytes((1, 2, 3, 4, 5)), b"", spare=3)
        assert c.flat[c.starts[i]:c.starts[i] + len(want)] == want and len(want) == sc.stream_dtype(5).itemsize


def test_restatement_on_a_hand_computed_example():
    P, R = sc.PAIRED, sc.REVERSE
    c = sc.case([
        # first fragment, forward: A C G T N at cycles 1..5, qualities 10 20 30 93 94(->93)
        sc.one(flag=P | sc.READ1 | sc.MREVERSE, mtid=0, pos=100, mpos=150, tlen=60, seq=(1, 2, 4, 8, 15), qual=bytes((10, 20, 30, 93, 94))),
        # its mate, reverse: SEQ A A C as stored is G T T as sequenced; cycles 3 2 1
        sc.one(flag=P | sc.READ2 | R, mtid=0, pos=150, mpos=100, tlen=-60, seq=(1, 1, 2), qual=bytes((5, 6, 7))),
        sc.one(flag=sc.SECONDARY, seq=(1,), qual=b"\x01"),
        sc.one(flag=sc.UNMAP, mapq=0, seq=(2, 4), qual=b"\xff\x03"),
    ], cycles=4, max_insert=50)
    r = sc.restate(c.flat, c.starts, 4, 50)
    assert (r["n"], r["n_kept"], r["n_counted"], r["bad_row"]) == (4, 4, 3, None)
    assert sn_of(r) == dict(sequences=3, first_fragments=2, last_fragments=1, mapped=2, unmapped=1, paired=2, properly_paired=0,
                            duplicates=0, mq0=0, qc_failed=0, secondary=1, supplementary=0, total_length=10, total_first_length=7,
                            total_last_length=3, bases_mapped=8, sum_quality=10 + 20 + 30 + 93 + 94 + 18, no_qualities=1,
                            max_length=5, pairs_inward=1, pairs_outward=0, pairs_other=0, pairs_different_chr=0)
    assert np.flatnonzero(r["read_len"]).tolist() == [2, 3, 5] and r["read_len"][5] == 1  # 5 > cycles: bin cycles + 1
    q = np.zeros((2, 5, 94), np.uint64)
    q[0, 0, 10] = q[0, 1, 20] = q[0, 2, 30] = q[0, 3, 93] = q[0, 4, 93] = 1
    q[1, 2, 5] = q[1, 1, 6] = q[1, 0, 7] = 1
    assert np.array_equal(r["qual"], q)
    #                             A  C  G  T  N     cycle 1: A, G (the mate's C complemented), C (the unmapped read)
    assert r["base"].tolist() == [[1, 1, 1, 0, 0], [0, 1, 1, 1, 0], [0, 0, 1, 1, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 1]]
    assert np.argwhere(r["gc"]).tolist() == [[0, 40], [0, 100], [1, 33]]
    assert np.argwhere(r["isize"]).tolist() == [[50, 0]] and np.flatnonzero(r["mapq"]).tolist() == [30]


@pytest.mark.parametrize("name", sc.CORPORA)
def test_host_is_the_restatement(name):
    c, want = sc.get(name), sc.expected(name)
    assert want["bad_row"] is None
    t, n_kept, n_counted = host(c)
    sc.tables_equal(t, want)
    assert (n_kept, n_counted) == (want["n_kept"], want["n_counted"]) and n_counted == int(t["sn"][0])
    sc.invariants(t, want)


def test_corpora_say_what_they_are_for():
    e = sc.expected
    w = e("lengths_cycles_200")
    assert np.flatnonzero(w["read_len"]).tolist() == [0, 1, 63, 64, 65, 127, 128, 129, 159, 160, 161, 199, 200, 201]
    assert w["read_len"][201] == 8  # 201 and 600, four rows each
    # both sides of the LDS window's last row and of its last quality bin are in use, in both tables
    assert w["qual"][:, 159:161].sum(axis=2).min() > 0 and w["qual"][:, :160, 47:49].sum(axis=1).min() > 0
    assert w["qual"][:, 160:, 47:49].sum(axis=1).min() > 0 and w["qual"][:, 200].sum() > 0 and w["base"][159:161].sum(axis=1).min() > 0
    for k in ("lengths_cycles_159", "lengths_cycles_160"):
        C = sc.get(k).cycles
        assert e(k)["qual"][:, C].sum() > 0 and e(k)["qual"][:, C - 1].sum() > 0
    q = e("qualities")
    assert sn_of(q)["no_qualities"] == 5 and q["qual"][0, :, 93].sum() == 4 + 4 + 9 + 1  # 93, 94, 254, 255 twice; nine 255; one 93
    assert [int(q["qual"][:, :, b].sum()) for b in (0, 47, 48, 92)] == [4, 3, 3, 3]
    assert (e("base_codes")["base"].sum(axis=0) > 0).all() and sn_of(e("which"))["last_fragments"] == 2
    s = sn_of(e("secondary_and_supplementary"))
    assert (s["secondary"], s["supplementary"], s["sequences"], s["pairs_other"]) == (3, 2, 2, 1)
    i = e("insert_sizes")
    assert np.flatnonzero(i["isize"].sum(axis=1)).tolist() == [1, 3, 5, 15, 16] and i["isize"][16].sum() == 3
    assert i["isize"][5].tolist() == [3, 3, 6] and sn_of(i)["pairs_different_chr"] == 2
    li = e("long_inserts_and_lengths")
    assert np.flatnonzero(li["isize"].sum(axis=1)).tolist() == [2047, 2048, 2049, 4999, 5000] and li["isize"][5000, 0] == 2
    assert np.flatnonzero(li["read_len"]).tolist() == [10, 2046, 2047, 2048, 2999, 3000, 3001]
    big = e("read_of_65536")
    assert sn_of(big)["max_length"] == 65537 and int(big["base"][200].sum()) == 3 * 65536 - 600
    lg = e("large")
    assert lg["n"] == sc.BASES_PASS + 37 == 2 * sc.GRID_PASS + 37 and int(lg["qual"].max()) > 65536 and sn_of(lg)["secondary"] > 0
    assert e("rows_1025")["n_counted"] == 1025 and e("rows_0")["n"] == 0
    assert e("filter_rows_nothing_kept")["n_kept"] == 0 and not e("filter_rows_nothing_kept")["sn"].any()
    for k in ("filter_require", "filter_exclude", "filter_mapq", "filter_rows"):
        assert 0 < e(k)["n_kept"] < e(k)["n"]


def test_adds_accumulate_and_a_row_given_three_times_counts_three_times():
    c, want = sc.get("row_given_three_times"), sc.expected("row_given_three_times")
    flat = np.frombuffer(bytes(c.flat), np.uint8)
    t, k1, _ = sb.stats_host(flat, c.starts[:90], c.cycles, c.max_insert)
    t, k2, _ = sb.stats_host(flat, c.starts[90:], c.cycles, c.max_insert, tables=t)
    sc.tables_equal(t, want)
    assert k1 + k2 == want["n_kept"] == 202
    once = sc.restate(c.flat, c.starts[:200], c.cycles, c.max_insert)
    row7 = sc.restate(c.flat, [c.starts[7]], c.cycles, c.max_insert)
    sc.tables_equal(want, sc.added(once, sc.added(row7, row7)))
    r = sc.get("rows_reversed")
    sc.tables_equal(sc.expected("rows_reversed"), sc.restate(r.flat, r.starts[::-1], r.cycles, r.max_insert))


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed_row(m):
    flat = np.frombuffer(bytes(m.stream.flat), np.uint8)
    assert sc.restate(m.stream.flat, m.stream.starts, 8, 16)["bad_row"] == 3
    t = stm.empty_tables(8, 16)
    untouched = lambda: not any(t[k].any() for k in sc.TABLES)  # noqa: E731
    with pytest.raises(sb.SparkBamError) as e:
        sb.stats_host(flat, m.stream.starts, 8, 16, tables=t)
    assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (3,) and untouched()
    # the bad row is judged even when the filter would drop it
    with pytest.raises(sb.SparkBamError) as e:
        sb.stats_host(flat, m.stream.starts, 8, 16, {"flag_require": 0x1000}, tables=t)
    assert e.value.fields == (3,) and untouched()
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        with pytest.raises(sb.SparkBamError) as e:
            sb.stats_host(flat, m.stream.starts[:2] + [p], 8, 16, tables=t)
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (2,) and untouched()
    # the good rows alone
    sc.tables_equal(sb.stats_host(flat, m.stream.starts[:3], 8, 16, tables=t)[0], sc.restate(m.stream.flat, m.stream.starts[:3], 8, 16))


def test_argument_errors():
    c = sc.get("which")
    flat = np.frombuffer(bytes(c.flat), np.uint8)
    st = np.asarray(c.starts, np.uint64)
    t = stm.empty_tables(8, 16)
    res, bad = sb._lib.SbhStatsAddResult(), C.c_uint64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(cycles=8, max_insert=16, f=None, drop=None, prm=True):
        ptrs = [None if k == drop else p(t[k]) for k in sc.TABLES]
        q = sb._lib.SbhStatsParams(cycles, max_insert)
        return sb.lib().sbh_stats_add_host(p(flat), flat.size, p(st), st.size, f, C.byref(q) if prm else None, *ptrs,
                                           C.byref(res), C.byref(bad))

    assert call() == SBH_OK and (res.n, res.n_kept, res.n_counted) == (8, 8, 8)
    before = {k: t[k].copy() for k in sc.TABLES}
    for cyc, ins in ((0, 16), (65537, 16), (8, 0), (8, (1 << 20) + 1), (2 ** 32 - 1, 2 ** 32 - 1)):
        assert call(cyc, ins) == SBH_E_ARG
    assert call(prm=False) == SBH_E_ARG
    for k in sc.TABLES:
        assert call(drop=k) == SBH_E_ARG
    f = sb._lib.SbhRecordFilter(0x10000, 0, 0, 0, None, None, 0)
    assert call(f=C.byref(f)) == SBH_E_ARG
    sc.tables_equal(t, before)
    for filt in ({"min_mapq": 256}, {"rows": [(5, 5)]}, {"rows": [(5, 9), (8, 12)]}):
        with pytest.raises(sb.SparkBamError) as e:
            sb.stats_host(flat, c.starts, 8, 16, filt)
        assert e.value.code == SBH_E_ARG
    for cyc, ins in ((0, 16), (65537, 16), (8, 0), (8, (1 << 20) + 1), (-1, 16), (8, 2 ** 32)):
        with pytest.raises(sb.SparkBamError) as e:
            sb.stats_host(flat, c.starts, cyc, ins)
        assert e.value.code == SBH_E_ARG
    with pytest.raises(ValueError):
        sb.stats_host(flat, c.starts, 9, 16, tables=t)
    # the largest parameters there are: accepted (no rows: nothing to count)
    big, _, _ = sb.stats_host(flat, [], sc.STAT_CYCLES_MAX, sc.STAT_INSERT_MAX)
    assert big["qual"].shape == (2, 65537, 94) and big["isize"].shape == ((1 << 20) + 1, 3) and not big["read_len"].any()


TEXT_LITERAL = (
    b"SN\tsequences:\t3\nSN\tfirst fragments:\t2\nSN\tlast fragments:\t1\nSN\treads mapped:\t2\nSN\treads unmapped:\t1\n"
    b"SN\treads paired:\t2\nSN\treads properly paired:\t0\nSN\treads duplicated:\t0\nSN\treads MQ0:\t0\nSN\treads QC failed:\t0\n"
    b"SN\tsecondary alignments:\t1\nSN\tsupplementary alignments:\t0\nSN\ttotal length:\t9\n"
    b"SN\ttotal first fragment length:\t6\nSN\ttotal last fragment length:\t3\nSN\tbases mapped:\t7\nSN\tquality sum:\t58\n"
    b"SN\treads without qualities:\t1\nSN\tmaximum length:\t4\nSN\tinward oriented pairs:\t1\nSN\toutward oriented pairs:\t1\n"
    b"SN\tpairs with other orientation:\t0\nSN\tpairs on different chromosomes:\t0\n"
    b"SN\taverage length:\t3\nSN\taverage quality:\t8.3\nSN\tinsert size average:\t3.0\nSN\tinsert size standard deviation:\t0.0\n"
    b"FFQ\t1\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t1\nFFQ\t2\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t1\nFFQ\t3\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t1\n"
    b"FFQ\t4\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t1\n"
    b"LFQ\t1\t0\t0\t0\t0\t0\t0\t0\t1\t0\t0\t0\nLFQ\t2\t0\t0\t0\t0\t0\t0\t1\t0\t0\t0\t0\nLFQ\t3\t0\t0\t0\t0\t0\t1\t0\t0\t0\t0\t0\n"
    b"LFQ\t4\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\n"
    b"GCF\t50\t1\nGCF\t100\t1\nGCL\t33\t1\n"
    b"GCC\t1\t1\t1\t1\t0\t0\nGCC\t2\t0\t1\t1\t1\t0\nGCC\t3\t0\t0\t1\t1\t0\nGCC\t4\t0\t0\t0\t1\t0\n"
    b"IS\t0\t0\t0\t0\t0\nIS\t1\t0\t0\t0\t0\nIS\t2\t0\t0\t0\t0\nIS\t3\t1\t1\t0\t0\nIS\t4\t1\t0\t1\t0\n"
    b"RL\t2\t1\nRL\t3\t1\nRL\t4\t1\nMAPQ\t30\t2\n")


def test_text_literal():
    P, R = sc.PAIRED, sc.REVERSE
    c = sc.case([
        sc.one(flag=P | sc.READ1 | sc.MREVERSE, mtid=0, pos=100, mpos=150, tlen=3, seq=(1, 2, 4, 8), qual=bytes((10, 10, 10, 10))),
        sc.one(flag=P | sc.READ2 | R, mtid=0, pos=90, mpos=100, tlen=9, seq=(1, 1, 2), qual=bytes((5, 6, 7))),
        sc.one(flag=sc.SECONDARY, seq=(1,), qual=b"\x01"),
        sc.one(flag=sc.UNMAP, mapq=0, seq=(2, 4), qual=b"\xff\x03"),
    ], cycles=3, max_insert=4)
    t, _, _ = host(c)
    assert sb.stats_text(t, 3, 4) == TEXT_LITERAL
    r = sb.StatsResult(t, 3, 4, 4, 4, 3)
    assert r.text() == TEXT_LITERAL and (r.n, r.n_kept, r.n_counted) == (4, 4, 3) and r.sn is t["sn"]
    # nothing counted: the counters and the derived lines, no table line
    z = sb.stats_text(stm.empty_tables(3, 4), 3, 4).split(b"\n")
    assert len(z) == sc.STAT_SN + 4 + 1 and z[-2] == b"SN\tinsert size standard deviation:\t0.0" and z[0] == b"SN\tsequences:\t0"
    # the standard deviation of sizes 2 and 4 (the bin max_insert = 6 stays out of it), a rounded average
    t2 = stm.empty_tables(3, 6)
    t2["isize"][2, 0], t2["isize"][4, 1], t2["isize"][6, 2] = 3, 3, 100
    z = sb.stats_text(t2, 3, 6)
    assert b"SN\tinsert size average:\t3.0\nSN\tinsert size standard deviation:\t1.0\n" in z and b"IS\t6\t100\t0\t0\t100\n" in z


def sam_walk(path, cycles, max_insert):
    """The tables of a SAM text, column by column, in plain Python."""
    t = {k: np.zeros(s, np.int64) for k, s in sc.shapes(cycles, max_insert).items()}
    sn = dict.fromkeys(sc.SN, 0)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    with gzip.open(path, "rt") as f:
        for line in f:
            if line.startswith("@"):
                continue
            c = line.rstrip("\n").split("\t")
            flag, rname, pos, mapq, rnext, pnext, tlen, seq, qual = int(c[1]), c[2], int(c[3]), int(c[4]), c[6], int(c[7]), int(c[8]), c[9], c[10]
            if flag & 0x100:
                sn["secondary"] += 1
                continue
            if flag & 0x800:
                sn["supplementary"] += 1
                continue
            seq = "" if seq == "*" else seq
            L = len(seq)
            last = 1 if flag & 1 and flag & 0x80 else 0
            mapped, rev = not flag & 4, bool(flag & 0x10)
            sn["sequences"] += 1
            sn["last_fragments" if last else "first_fragments"] += 1
            sn["mapped" if mapped else "unmapped"] += 1
            sn["paired"] += flag & 1
            sn["properly_paired"] += 1 if flag & 1 and flag & 2 and mapped else 0
            sn["duplicates"] += 1 if flag & 0x400 else 0
            sn["mq0"] += 1 if mapped and mapq == 0 else 0
            sn["qc_failed"] += 1 if flag & 0x200 else 0
            sn["total_length"] += L
            sn["total_last_length" if last else "total_first_length"] += L
            sn["bases_mapped"] += L if mapped else 0
            sn["max_length"] = max(sn["max_length"], L)
            t["read_len"][L if L <= cycles else cycles + 1] += 1
            if mapped:
                t["mapq"][mapq] += 1
            same = rname != "*" and rnext in ("=", rname)
            both = flag & 1 and mapped and not flag & 8
            if both and not same and flag & 0x40:
                sn["pairs_different_chr"] += 1
            if both and same and tlen > 0:
                mrev = bool(flag & 0x20)
                col = 2 if rev == mrev else (1 if (rev if pos <= pnext else mrev) else 0)
                t["isize"][min(tlen, max_insert), col] += 1
                sn[("pairs_inward", "pairs_outward", "pairs_other")[col]] += 1
            if qual == "*" or not L:
                sn["no_qualities"] += 1
            if not L:
                continue
            t["gc"][last, 100 * sum(b in "CG" for b in seq) // L] += 1
            as_read = "".join(comp.get(b, "N") for b in reversed(seq)) if rev else seq
            for cyc, b in enumerate(as_read):
                t["base"][min(cyc, cycles), "ACGT".find(b) if b in "ACGT" else 4] += 1
            if qual != "*":
                for cyc, ch in enumerate(reversed(qual) if rev else qual):
                    t["qual"][last, min(cyc, cycles), min(ord(ch) - 33, 93)] += 1
                    sn["sum_quality"] += ord(ch) - 33
    t["sn"] = np.array([sn[k] for k in sc.SN], np.int64)
    return {k: v.astype(np.uint64) for k, v in t.items()}


@pytest.mark.parametrize("cycles,max_insert", [(1024, 8000), (50, 200)])
def test_bundled_2bam_against_its_sam_text(cycles, max_insert):
    _, flat, starts, _, _, _ = bundled("2.bam")
    t, n_kept, n_counted = sb.stats_host(np.frombuffer(flat, np.uint8), starts, cycles, max_insert)
    want = sam_walk(os.path.join(GOLDEN, "sam", "2.sam.gz"), cycles, max_insert)
    sc.tables_equal(t, want)
    sc.invariants(t)
    assert n_kept == n_counted == 2500
    # flagstat's literals of the same file (test_tally_cpu.py): total, mapped, paired, properly paired, duplicates
    lines = FLAGSTAT_2BAM.split(b"\n")
    lit = lambda k: int(lines[k].split(b" ")[0])  # noqa: E731
    s = sn_of(t)
    assert (s["sequences"], s["mapped"], s["paired"], s["properly_paired"], s["duplicates"]) == (lit(0), lit(6), lit(8), lit(11), lit(4))
    assert (s["first_fragments"], s["last_fragments"]) == (lit(9), lit(10))


@pytest.mark.parametrize("name", ["2.bam", "5k.bam", "1.bam"])
def test_bundled_files_are_the_restatement(name):
    _, flat, starts, _, _, _ = bundled(name)
    u8 = np.frombuffer(flat, np.uint8)
    for f in (None, {"flag_exclude": 0x400, "min_mapq": 1}):
        t, n_kept, n_counted = sb.stats_host(u8, starts, 1024, 8000, f)
        want = sc.restate(u8, starts, 1024, 8000, f)
        sc.tables_equal(t, want)
        sc.invariants(t, want)
        assert (n_kept, n_counted) == (want["n_kept"], want["n_counted"])


def test_exports():
    assert {"sbh_stats_create", "sbh_stats_destroy", "sbh_stats_reset", "sbh_records_stats_add", "sbh_stats_fetch",
            "sbh_stats_add_host"} <= set(sb._lib.EXPORTS)
    for k in ("stats", "stats_host", "stats_text", "Stats", "StatsResult", "SN_ROWS"):
        assert k in sb.__all__ and getattr(sb, k)
    assert callable(sb.stats) and sb.api.stats is sb.stats
