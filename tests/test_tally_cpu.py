"""The host side of the flag counts and per-reference read counts (csrc/tally_core.h through the
library, no GPU): sbh_tally_add_host against the numpy restatement of tally_corpus.py on every
corpus, the two invariants, malformed rows, the argument errors, and the two text renderers against
literals."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden_bam
from pkg import sb
import record_corpus as rc
import tally_corpus as tc

SBH_OK, SBH_E_ARG, SBH_E_BAD_RECORD = 0, sb._lib.SBH_E_ARG, sb._lib.SBH_E_BAD_RECORD

FLAGSTAT_2BAM = b"""2500 + 0 in total (QC-passed reads + QC-failed reads)
2500 + 0 primary
0 + 0 secondary
0 + 0 supplementary
166 + 0 duplicates
166 + 0 primary duplicates
2450 + 0 mapped (98.00% : N/A)
2450 + 0 primary mapped (98.00% : N/A)
2500 + 0 paired in sequencing
1249 + 0 read1
1251 + 0 read2
2383 + 0 properly paired (95.32% : N/A)
2400 + 0 with itself and mate mapped
50 + 0 singletons (2.00% : N/A)
10 + 0 with mate mapped to a different chr
0 + 0 with mate mapped to a different chr (mapQ>=5)
"""

# the percentages by hand: 4547 / 4570, 340 / 347, 4508 / 4570, 332 / 347, 24 / 4570, 7 / 347
FLAGSTAT_1BAM = b"""4570 + 347 in total (QC-passed reads + QC-failed reads)
4570 + 347 primary
0 + 0 secondary
0 + 0 supplementary
792 + 93 duplicates
792 + 93 primary duplicates
4547 + 340 mapped (99.50% : 97.98%)
4547 + 340 primary mapped (99.50% : 97.98%)
4570 + 347 paired in sequencing
2271 + 171 read1
2299 + 176 read2
4508 + 332 properly paired (98.64% : 95.68%)
4523 + 333 with itself and mate mapped
24 + 7 singletons (0.53% : 2.02%)
12 + 1 with mate mapped to a different chr
12 + 1 with mate mapped to a different chr (mapQ>=5)
"""

FLAGSTAT_NOTHING = b"""0 + 0 in total (QC-passed reads + QC-failed reads)
0 + 0 primary
0 + 0 secondary
0 + 0 supplementary
0 + 0 duplicates
0 + 0 primary duplicates
0 + 0 mapped (N/A : N/A)
0 + 0 primary mapped (N/A : N/A)
0 + 0 paired in sequencing
0 + 0 read1
0 + 0 read2
0 + 0 properly paired (N/A : N/A)
0 + 0 with itself and mate mapped
0 + 0 singletons (N/A : N/A)
0 + 0 with mate mapped to a different chr
0 + 0 with mate mapped to a different chr (mapQ>=5)
"""

# rows 0, 4, 6, 8, 9, 10, 11, 12, 13, 14, 15 as (pass, fail), from a plain walk of the files (rows 1,
# 5 and 7 equal rows 0, 4 and 6; rows 2 and 3 are zero); then bin 0's mapped and unmapped
BUNDLED = {
    "2.bam": ([(2500, 0), (166, 0), (2450, 0), (2500, 0), (1249, 0), (1251, 0), (2383, 0), (2400, 0), (50, 0), (10, 0), (0, 0)],
              (2450, 50)),
    "5k.bam": ([(4910, 0), (333, 0), (4787, 0), (4910, 0), (2450, 0), (2460, 0), (4620, 0), (4664, 0), (123, 0), (28, 0),
                (5, 0)], (4787, 123)),
    "1.bam": ([(4570, 347), (792, 93), (4547, 340), (4570, 347), (2271, 171), (2299, 176), (4508, 332), (4523, 333),
               (24, 7), (12, 1), (12, 1)], (4887, 30)),
}


def bundled_flag(name):
    """The literal flag[16][2] of a bundled file."""
    rows, _ = BUNDLED[name]
    total, dup, mapped = rows[0], rows[1], rows[2]
    return np.array([total, total, (0, 0), (0, 0), dup, dup, mapped, mapped] + rows[3:], np.uint64)


def bundled_ref(name, n_ref):
    ref = np.zeros((n_ref + 1, 2), np.uint64)
    ref[0] = BUNDLED[name][1]
    return ref


@functools.lru_cache(maxsize=None)
def bundled(name):
    """(file bytes, flat, record starts, names, lengths, first) of a bundled BAM."""
    data = np.fromfile(golden_bam(name), dtype=np.uint8)
    flat = rc.inflate_members(data.tobytes())
    names, lens, first = sb.parse_bam_header(np.frombuffer(flat, np.uint8))
    starts, p = [], first
    while p < len(flat):
        starts.append(p)
        p += 4 + int.from_bytes(flat[p:p + 4], "little")
    return data, flat, starts, names, [int(x) for x in lens], first


def host(c, **kw):
    return sb.tally_host(np.frombuffer(bytes(c.flat), np.uint8), c.starts, c.n_ref, c.filter, **kw)


def test_constants_are_the_library_s():
    with open(os.path.join(ROOT, "spark-bam_amd", "csrc", "tally_core.h")) as f:
        src = f.read()
    assert int(re.search(r"constexpr uint32_t TALLY_LDS_BINS = (\d+);", src).group(1)) == tc.TALLY_LDS_BINS
    assert int(re.search(r"constexpr uint32_t TALLY_ROWS = (\d+);", src).group(1)) == tc.TALLY_ROWS == sb.tally.TALLY_ROWS
    with open(os.path.join(ROOT, "include", "sparkbam.h")) as f:
        assert "#define SBH_TALLY_ROWS %d\n" % tc.TALLY_ROWS in f.read()
    # the three sizes around the LDS budget
    assert [2 * (tc.get(k).n_ref + 1) - tc.TALLY_LDS_BINS for k in ("lds_below", "lds_exact", "lds_above")] == [-2, 0, 2]


def test_builder_rows_are_rec_s_bytes():
    c = tc.stream([2, -1, 199999], [0x10, 0xFFF, 0], [9, 0, 255], [1, -1, 7])
    for i, (tid, flag, mapq, mtid) in enumerate(((2, 0x10, 9, 1), (-1, 0xFFF, 0, -1), (199999, 0, 255, 7))):
        want = rc.rec(tid, i, mapq, 4681, flag, mtid, -1, 0, b"r" + bytes(6), (), (), b"", b"")
        assert c.flat[c.starts[i]:c.starts[i] + 44] == want


def test_restatement_on_a_hand_computed_example():
    P, U, MU, Q = tc.PAIRED, tc.UNMAP, tc.MUNMAP, tc.QCFAIL
    c = tc.case([tc.one(0, P | tc.PROPER | tc.READ1, 30, 0), tc.one(0, P | tc.READ2, 5, 1), tc.one(1, P | MU | Q, 30, 1),
                 tc.one(-1, P | U, 0, -1), tc.one(2, tc.SECONDARY | P), tc.one(3, tc.SUPPLEMENTARY | tc.DUP | Q)])
    r = tc.restate(c.flat, c.starts, tc.N_REF)
    #                          total   prim    sec     sup     dup     pdup    mapped  pmapped paired  r1      r2
    assert r["flag"].tolist() == [[4, 2], [3, 1], [1, 0], [0, 1], [0, 1], [0, 0], [3, 2], [2, 1], [3, 1], [1, 0], [1, 0],
                                  # proper both    single  diff    diff q5
                                  [1, 0], [2, 0], [0, 1], [1, 0], [1, 0]]
    assert r["ref"].tolist() == [[2, 0], [1, 0], [1, 0], [1, 0], [0, 1]]
    assert (r["n"], r["n_kept"], r["bad_row"]) == (6, 6, None)


@pytest.mark.parametrize("name", tc.CORPORA)
def test_host_is_the_restatement(name):
    c, want = tc.get(name), tc.expected(name)
    assert want["bad_row"] is None
    flag, ref, n_kept = host(c)
    assert flag.dtype == np.uint64 and flag.shape == (16, 2) and np.array_equal(flag, want["flag"])
    assert ref.dtype == np.uint64 and ref.shape == (c.n_ref + 1, 2) and np.array_equal(ref, want["ref"])
    assert n_kept == want["n_kept"]
    # the two invariants
    assert int(ref[:, 0].sum()) == int(flag[6].sum())
    assert int(ref.sum()) == int(flag[0].sum()) == n_kept


def test_corpora_say_what_they_are_for():
    e = tc.expected
    f = e("flag_bits")["flag"].tolist()
    # 13 rows and 12: the QC-fail bit alone is the thirteenth row of the second column
    assert f[0] == [12, 13] and f[2] == [1, 1] and f[3] == [1, 1] and f[4] == [1, 1] and f[8] == [1, 1] and f[9] == [0, 0]
    f = e("secondary_and_supplementary")["flag"].tolist()
    assert f[1] == [0, 0] and f[2] == [6, 0] and f[3] == [2, 1] and f[8:14] == [[0, 0]] * 6 and f[5] == [0, 0]
    f = e("pair_rows")["flag"].tolist()
    # (the QC-fail row is proper and mapped with its mate unmapped: a properly paired singleton)
    assert f[8] == [9, 1] and f[11] == [1, 1] and f[13] == [1, 1] and f[12] == [5, 0] and f[9] == [2, 0] and f[10] == [2, 0]
    f = e("mate_chr")["flag"].tolist()
    assert f[12] == [7, 1] and f[14] == [5, 1] and f[15] == [4, 1]
    assert e("tid_values")["ref"].tolist() == [[1, 1], [1, 0], [0, 0], [1, 1], [3, 2]]
    assert e("tid_n_ref_filtered_out")["n_kept"] == 2
    assert e("n_ref_0")["ref"].shape == (1, 2) and int(e("n_ref_0")["ref"].sum()) == 300
    for k in ("lds_below", "lds_exact", "lds_above"):  # the last reference and the `*` bin are in use
        assert e(k)["ref"][-2:].sum(axis=1).min() > 0
    big = e("n_ref_200000")["ref"]
    assert np.flatnonzero(big.sum(axis=1)).tolist() == [0, 199999, 200000] and int(big.sum()) == 262
    assert e("wave_only_lane_63_kept")["ref"].tolist() == [[0, 0], [1, 0], [0, 0], [0, 0], [0, 0]]
    assert e("wave_nothing_kept_between")["ref"].tolist() == [[64, 64], [128, 0], [64, 0], [0, 0], [0, 0]]
    assert e("wave_dropped_on_other_bin")["ref"][2].tolist() == [0, 0] and e("wave_dropped_on_other_bin")["n_kept"] == 85
    assert e("filter_rows_nothing_kept")["n_kept"] == 0 and e("filter_rows_one_per_wave")["n_kept"] == 8
    assert e("rows_0")["n"] == 0 and e("grid")["n_kept"] == rc.GRID_RECORDS == tc.GRID_PASS + 37
    g = e("grid_three_rounds")
    assert g["n"] == 2 * tc.GRID_PASS + 101 and g["ref"][0].tolist() == [128 - 26, 26] and g["ref"][1].tolist() == [64 - 13, 13]
    assert np.array_equal(e("rows_reversed")["flag"], tc.restate(tc.get("rows_reversed").flat, tc.get("rows_reversed").starts[::-1],
                                                                 tc.N_REF)["flag"])


def test_adds_accumulate_and_a_row_given_three_times_counts_three_times():
    c, want = tc.get("row_given_three_times"), tc.expected("row_given_three_times")
    flat = np.frombuffer(bytes(c.flat), np.uint8)
    flag, ref, k1 = sb.tally_host(flat, c.starts[:90], c.n_ref)
    flag, ref, k2 = sb.tally_host(flat, c.starts[90:], c.n_ref, flag=flag, ref=ref)
    assert np.array_equal(flag, want["flag"]) and np.array_equal(ref, want["ref"]) and k1 + k2 == want["n_kept"] == 202
    once = tc.restate(c.flat, c.starts[:200], c.n_ref)
    row7 = tc.restate(c.flat, [c.starts[7]], c.n_ref)
    assert np.array_equal(want["flag"], once["flag"] + 2 * row7["flag"]) and np.array_equal(want["ref"], once["ref"] + 2 * row7["ref"])


def test_reference_out_of_range_in_a_kept_row():
    c = tc.TID_KEPT()
    assert tc.restate(c.flat, c.starts, c.n_ref)["bad_row"] == 2
    flat = np.frombuffer(bytes(c.flat), np.uint8)
    flag, ref = np.full((16, 2), 7, np.uint64), np.full((c.n_ref + 1, 2), 9, np.uint64)
    with pytest.raises(sb.SparkBamError) as e:
        sb.tally_host(flat, c.starts, c.n_ref, flag=flag, ref=ref)
    assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (2,)
    assert (flag == 7).all() and (ref == 9).all()
    # one reference more: the same rows are fine
    assert sb.tally_host(flat, c.starts, c.n_ref + 1)[1][c.n_ref].tolist() == [1, 0]


@pytest.mark.parametrize("m", rc.MALFORMED_CASES, ids=lambda m: m.name)
def test_malformed_row(m):
    flat = np.frombuffer(bytes(m.stream.flat), np.uint8)
    assert tc.restate(m.stream.flat, m.stream.starts, tc.N_REF)["bad_row"] == 3
    flag, ref = np.zeros((16, 2), np.uint64), np.zeros((tc.N_REF + 1, 2), np.uint64)
    with pytest.raises(sb.SparkBamError) as e:
        sb.tally_host(flat, m.stream.starts, tc.N_REF, flag=flag, ref=ref)
    assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (3,) and not flag.any() and not ref.any()
    # the bad row is judged even when the filter would drop it
    with pytest.raises(sb.SparkBamError) as e:
        sb.tally_host(flat, m.stream.starts, tc.N_REF, {"flag_require": 0x1000}, flag=flag, ref=ref)
    assert e.value.fields == (3,) and not flag.any() and not ref.any()
    for p in (len(m.stream.flat) + 1, 2 ** 64 - 8):  # a start past the stream; one whose + 36 wraps
        with pytest.raises(sb.SparkBamError) as e:
            sb.tally_host(flat, m.stream.starts[:2] + [p], tc.N_REF, flag=flag, ref=ref)
        assert e.value.code == SBH_E_BAD_RECORD and e.value.fields == (2,) and not flag.any() and not ref.any()


def test_argument_errors():
    c = tc.get("pair_rows")
    flat = np.frombuffer(bytes(c.flat), np.uint8)
    st = np.asarray(c.starts, np.uint64)
    flag, ref = np.zeros((16, 2), np.uint64), np.zeros((tc.N_REF + 1, 2), np.uint64)
    res, bad = sb._lib.SbhTallyAddResult(), C.c_uint64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lambda n_ref, fl, rf, f=None: sb.lib().sbh_tally_add_host(p(flat), flat.size, p(st), st.size, f, n_ref,  # noqa: E731
                                                                     fl, rf, C.byref(res), C.byref(bad))
    assert call(tc.N_REF, p(flag), p(ref)) == SBH_OK and res.n == res.n_kept == st.size
    assert call(-1, p(flag), p(ref)) == SBH_E_ARG
    assert call(tc.N_REF, None, p(ref)) == SBH_E_ARG and call(tc.N_REF, p(flag), None) == SBH_E_ARG
    f = sb._lib.SbhRecordFilter(0x10000, 0, 0, 0, None, None, 0)
    assert call(tc.N_REF, p(flag), p(ref), C.byref(f)) == SBH_E_ARG
    for filt in ({"min_mapq": 256}, {"rows": [(5, 5)]}, {"rows": [(5, 9), (8, 12)]}):
        with pytest.raises(sb.SparkBamError) as e:
            sb.tally_host(flat, c.starts, tc.N_REF, filt)
        assert e.value.code == SBH_E_ARG


@pytest.mark.parametrize("name", BUNDLED)
def test_bundled_files(name):
    _, flat, starts, names, lens, _ = bundled(name)
    u8 = np.frombuffer(flat, np.uint8)
    flag, ref, n_kept = sb.tally_host(u8, starts, len(lens))
    want = tc.restate(u8, starts, len(lens))
    assert np.array_equal(flag, want["flag"]) and np.array_equal(ref, want["ref"])
    assert np.array_equal(flag, bundled_flag(name)) and np.array_equal(ref, bundled_ref(name, len(lens)))
    assert n_kept == len(starts) == int(flag[0].sum())


def test_flagstat_text_literals():
    assert sb.flagstat_text(bundled_flag("2.bam")) == FLAGSTAT_2BAM
    _, flat, starts, _, lens, _ = bundled("2.bam")
    assert sb.flagstat_text(sb.tally_host(np.frombuffer(flat, np.uint8), starts, len(lens))[0]) == FLAGSTAT_2BAM
    _, flat, starts, _, lens, _ = bundled("1.bam")
    assert sb.flagstat_text(sb.tally_host(np.frombuffer(flat, np.uint8), starts, len(lens))[0]) == FLAGSTAT_1BAM
    assert sb.flagstat_text(np.zeros((16, 2), np.uint64)) == FLAGSTAT_NOTHING
    # a percentage of more than one digit before the point, and one that rounds up to 100.00
    f = np.zeros((16, 2), np.uint64)
    f[0], f[6] = (3, 200000), (3, 199999)
    assert b"3 + 199999 mapped (100.00% : 100.00%)\n" in sb.flagstat_text(f)
    f[0], f[6] = (2 ** 63, 3), (2 ** 62, 1)
    assert b"4611686018427387904 + 1 mapped (50.00% : 33.33%)\n" in sb.flagstat_text(f)


def test_idxstats_text_format():
    ref = np.array([[5, 1], [0, 0], [2 ** 40, 7], [3, 4]], np.uint64)
    assert sb.idxstats_text(ref, ["chrM", "chr10", "chr2"], [16571, 135534747, 2147483647]) == (
        b"chrM\t16571\t5\t1\nchr10\t135534747\t0\t0\nchr2\t2147483647\t1099511627776\t7\n*\t0\t3\t4\n")
    assert sb.idxstats_text(np.array([[0, 9]], np.uint64), [], []) == b"*\t0\t0\t9\n"
    with pytest.raises(ValueError):
        sb.idxstats_text(ref, ["a"], [1])
    _, flat, starts, names, lens, _ = bundled("2.bam")
    text = sb.idxstats_text(sb.tally_host(np.frombuffer(flat, np.uint8), starts, len(lens))[1], names, lens)
    lines = text.split(b"\n")
    assert lines[0] == b"%s\t%d\t2450\t50" % (names[0].encode(), lens[0]) and lines[len(lens)] == b"*\t0\t0\t0"
    assert len(lines) == len(lens) + 2 and lines[-1] == b""


def test_exports():
    assert {"sbh_tally_create", "sbh_tally_destroy", "sbh_tally_reset", "sbh_records_tally_add", "sbh_tally_fetch",
            "sbh_tally_add_host"} <= set(sb._lib.EXPORTS)
    for k in ("flagstat", "idxstats", "tally_host", "flagstat_text", "idxstats_text", "Tally", "TallyResult"):
        assert k in sb.__all__ and getattr(sb, k)
