// stats_core.h -- read-level statistics (the histograms of samtools stats) of a record scan's rows,
// written once for both sides: the device kernels (stats.hip) and the host functions below
// (sbh_stats_add_host, cli/spark_bam.cpp, tests/sanitize/stats_driver.cpp).  SBH_HD is __host__
// __device__ under hipcc, empty otherwise.
//
// Parameters, fixed at create: cycles C in [1, 65536], max_insert I in [1, 1 << 20].
//
// Fields of one record (r = its first byte): flag, mapq, tid, mtid as tally_core.h reads them;
// pos = (int32) ld32(r + 8), mpos = (int32) ld32(r + 28), tlen = (int32) ld32(r + 32), L = l_seq; SEQ
// and QUAL through pileup_core.h's accessors (query base i: code = SEQ[i >> 1] >> 4 for even i, & 15
// for odd i; quality QUAL[i]).  which = 1 (last) when 0x1 and 0x80 are both set, else 0 (first); rev =
// 0x10.
//
// Rows.  A row that passes the filter (bam_gather_core.h; no filter: every row) is KEPT.  Every row,
// kept or not, passes row_check -- which proves SEQ and QUAL lie inside the record; nothing else is
// validated, and no table is indexed by a reference id.  The smallest bad row is reported, and nothing
// is added when there is one.  A kept row is COUNTED when it is neither secondary (0x100) nor
// supplementary (0x800); a kept row that is not counted adds to sn[secondary] (0x100) or
// sn[supplementary] (0x800 without 0x100) and to nothing else.
//
// Tables of the counted rows, u64 each:
//   read_len[C + 2]      bin L for L <= C, bin C + 1 for a longer read
//   qual[2][C + 1][94]   [which]; skipped for a row with L == 0 or QUAL[0] == 0xff (sn[no_qualities]
//                        counts those); else for each query base i: cycle c = rev ? L - 1 - i : i, row
//                        min(c, C), bin min(QUAL[i], 93)
//   base[C + 1][5]       the same rows for every row with L > 0, qualities or not; the channel is
//                        pileup_core.h's code_channel (A C G T N), complemented for a rev row (A<->T,
//                        C<->G): the table describes the read as it was sequenced, the orientation
//                        fastq prints
//   gc[2][101]           [which]; for L > 0: bin floor(100 g / L), g = the bases with code 2 or 4
//   isize[I + 1][3]      a row with 0x1 set, 0x4 and 0x8 clear, tid == mtid >= 0 and tlen > 0 (one row
//                        of a pair); bin min(tlen, I); column 2 (other) when rev == mate-rev (0x20),
//                        else the left read is this one when pos <= mpos, the mate otherwise, and the
//                        column is 0 (inward) when the left read is forward, 1 (outward) when not
//   mapq[256]            rows with 0x4 clear
//   sn[STAT_SN]          in this order:
//      0 sequences  1 first_fragments  2 last_fragments     (counted rows; by which)
//      3 mapped  4 unmapped                                  (0x4 clear / set)
//      5 paired  6 properly_paired                           (0x1; 0x1 and 0x2 and not 0x4)
//      7 duplicates (0x400)  8 mq0 (mapped, mapq == 0)  9 qc_failed (0x200)
//     10 secondary  11 supplementary                         (kept rows that are not counted)
//     12 total_length  13 total_first_length  14 total_last_length   (sums of L)
//     15 bases_mapped (the sum of L over mapped rows)
//     16 sum_quality (the sum of QUAL[i], unclamped, over the bases of rows that enter qual)
//     17 no_qualities
//     18 max_length (a maximum, not a sum: a fetch after two adds holds the larger)
//     19 pairs_inward  20 pairs_outward  21 pairs_other      (the rows of isize, by column)
//     22 pairs_different_chr (0x1, 0x4 and 0x8 clear, tid != mtid, 0x40 set)
//
// Invariants: sum(read_len) == sequences; sum(qual[w]) + (the bases of w's rows without qualities) ==
// the total length of w; sum(base) == total_length; sum(gc[w]) == w's rows with L > 0;
// sum(isize[:, k]) == the pair counter of column k; sum(mapq) == mapped.  sum(qual * bin) equals
// sum_quality only while no quality exceeds 93: the bins clamp, the sum does not.
//
// Every entry but max_length is an integer sum over kept rows: exact, and independent of the order of
// the rows and of the path a base takes on the device.
#pragma once
#include <stdint.h>

#include "pileup_core.h"

namespace sbh_stat {

constexpr uint32_t STAT_QUALS = 94;  // SBH_STATS_QUALS
constexpr uint32_t STAT_SN = 23;     // SBH_STATS_SN
constexpr uint32_t STAT_CYCLES_MAX = 65536, STAT_INSERT_MAX = 1u << 20;
constexpr uint32_t STAT_GC_BINS = 101, STAT_BASES = 5, STAT_MAPQS = 256;
// The LDS window of k_stats_bases: table rows below STAT_LDS_CYCLES and quality bins below
// STAT_LDS_QUALS are gathered per workgroup (u32 cells) and flushed once; every other add goes straight
// to the staging words.  2 x 160 x 48 cells of qual, 160 x 5 of base, 2 x 101 of gc: 65448 bytes.
constexpr uint32_t STAT_LDS_CYCLES = 160, STAT_LDS_QUALS = 48;
// a read this long or longer bypasses the LDS window altogether: below it one read adds less than
// 2^16 to any cell, and a workgroup of k_stats_bases sees at most 2^16 reads a launch
constexpr uint32_t STAT_LDS_MAX_READ = 65536;
// the LDS windows of k_stats_rows: read-length bins and insert-size bins below these (u32 cells)
constexpr uint32_t STAT_LDS_LENGTHS = 2048, STAT_LDS_INSERTS = 2048;

constexpr uint32_t SN_SEQUENCES = 0, SN_FIRST = 1, SN_LAST = 2, SN_MAPPED = 3, SN_UNMAPPED = 4, SN_PAIRED = 5;
constexpr uint32_t SN_PROPER = 6, SN_DUP = 7, SN_MQ0 = 8, SN_QCFAIL = 9, SN_SECONDARY = 10, SN_SUPPLEMENTARY = 11;
constexpr uint32_t SN_TOTAL_LEN = 12, SN_FIRST_LEN = 13, SN_LAST_LEN = 14, SN_BASES_MAPPED = 15, SN_SUM_QUAL = 16;
constexpr uint32_t SN_NO_QUAL = 17, SN_MAX_LEN = 18, SN_INWARD = 19, SN_OUTWARD = 20, SN_OTHER = 21, SN_DIFF_CHR = 22;

struct Params {  // sbh_stats_params' layout
  uint32_t cycles, max_insert;
};
SBH_HD inline bool params_ok(const Params &P) {
  return P.cycles >= 1 && P.cycles <= STAT_CYCLES_MAX && P.max_insert >= 1 && P.max_insert <= STAT_INSERT_MAX;
}

// The tables one behind another, as the device holds them (u64 words): sn, read_len, qual, base, gc,
// isize, mapq.
struct Layout {
  uint64_t read_len, qual, base, gc, isize, mapq, words;
};
SBH_HD inline Layout layout_of(const Params &P) {
  Layout l;
  const uint64_t C = P.cycles, I = P.max_insert;
  l.read_len = STAT_SN;
  l.qual = l.read_len + C + 2;
  l.base = l.qual + 2 * (C + 1) * STAT_QUALS;
  l.gc = l.base + (C + 1) * STAT_BASES;
  l.isize = l.gc + 2 * STAT_GC_BINS;
  l.mapq = l.isize + (I + 1) * 3;
  l.words = l.mapq + STAT_MAPQS;
  return l;
}

SBH_HD inline bool counted(uint32_t flag) { return !(flag & 0x900u); }
SBH_HD inline uint32_t which_of(uint32_t flag) { return (flag & 0x81u) == 0x81u ? 1u : 0u; }
SBH_HD inline const uint8_t *qual_of(const uint8_t *r) {
  return sbh_pile::seq_of(r) + ((uint64_t)sbh_pile::l_seq_of(r) + 1) / 2;
}
// the table row of query base i of a read of L bases
SBH_HD inline uint32_t cycle_row(uint64_t i, uint64_t L, bool rev, uint32_t C) {
  const uint64_t c = rev ? L - 1 - i : i;
  return c < C ? (uint32_t)c : C;
}
SBH_HD inline uint32_t seq_code(const uint8_t *seq, uint64_t i) {
  const uint32_t b = seq[i >> 1];
  return (i & 1) ? (b & 15u) : (b >> 4);
}
// the channel of a base with this code as it was sequenced
SBH_HD inline uint32_t base_channel(uint32_t code, bool rev) {
  const uint32_t ch = sbh_pile::code_channel(code);
  return rev && ch < 4 ? 3 - ch : ch;
}
SBH_HD inline bool is_gc(uint32_t code) { return code == 2 || code == 4; }
SBH_HD inline uint32_t gc_bin(uint64_t g, uint64_t L) { return (uint32_t)(100 * g / L); }  // L > 0, g <= L

// bit k of the result: a kept row with these fields adds one to sn[k] (the counters that count rows;
// no_qualities, the pair columns and the sums are not among them)
SBH_HD inline uint32_t sn_rows_of(uint32_t flag, uint32_t mapq, int32_t tid, int32_t mtid) {
  if (!counted(flag)) return (flag & 0x100u) ? 1u << SN_SECONDARY : 1u << SN_SUPPLEMENTARY;
  const bool mapped = !(flag & 0x4u), paired = flag & 0x1u, last = which_of(flag);
  uint32_t m = 1u << SN_SEQUENCES;
  m |= (uint32_t)!last << SN_FIRST | (uint32_t)last << SN_LAST | (uint32_t)mapped << SN_MAPPED | (uint32_t)!mapped << SN_UNMAPPED;
  m |= (uint32_t)paired << SN_PAIRED | (uint32_t)(paired && (flag & 0x2u) && mapped) << SN_PROPER;
  m |= (uint32_t)((flag & 0x400u) != 0) << SN_DUP | (uint32_t)(mapped && mapq == 0) << SN_MQ0;
  m |= (uint32_t)((flag & 0x200u) != 0) << SN_QCFAIL;
  m |= (uint32_t)(paired && mapped && !(flag & 0x8u) && tid != mtid && (flag & 0x40u)) << SN_DIFF_CHR;
  return m;
}

// a counted row's entry of isize: false when it has none, else *bin <= I and *col < 3
SBH_HD inline bool isize_slot(uint32_t flag, int32_t tid, int32_t mtid, int32_t pos, int32_t mpos, int32_t tlen, uint32_t I,
                              uint32_t *bin, uint32_t *col) {
  if (!(flag & 0x1u) || (flag & 0xCu) || tid != mtid || tid < 0 || tlen <= 0) return false;
  *bin = (uint32_t)tlen < I ? (uint32_t)tlen : I;
  const bool rev = flag & 0x10u, mrev = flag & 0x20u;
  *col = rev == mrev ? 2u : (pos <= mpos ? rev : mrev) ? 1u : 0u;
  return true;
}

}  // namespace sbh_stat

// ---- the host side (plain host functions under hipcc too) --------------------------------------
#include <math.h>
#include <stdio.h>

#include <string>

namespace sbh_stat {

struct AddResult {  // sbh_stats_add_result's layout
  uint64_t n, n_kept, n_counted;
};
struct Tables {  // sn[STAT_SN], read_len[C + 2], qual[2][C + 1][94], base[C + 1][5], gc[2][101], isize[I + 1][3], mapq[256]
  uint64_t *sn, *read_len, *qual, *base, *gc, *isize, *mapq;
};

// Validate everything, then add into the tables.  Returns 0 or 1 (a bad row: *bad_row, the tables
// untouched).
inline int add_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n, const sbh_bam::Filter &F,
                    const Params &P, const Tables &T, AddResult *res, uint64_t *bad_row) {
  *res = AddResult{n, 0, 0};
  *bad_row = sbh_bam::first_bad_row(flat, flat_size, starts, n, F, [](const uint8_t *) { return true; });
  if (*bad_row != sbh_bam::NO_ROW) return 1;
  const uint32_t C = P.cycles;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t *r = flat + starts[i];
    if (!sbh_bam::row_keep(r, i, F)) continue;
    ++res->n_kept;
    const uint32_t fl = sbh_bam::ld32(r + 16) >> 16, mapq = r[13];
    const int32_t tid = (int32_t)sbh_bam::ld32(r + 4), mtid = (int32_t)sbh_bam::ld32(r + 24);
    const uint32_t m = sn_rows_of(fl, mapq, tid, mtid);
    for (uint32_t k = 0; k < STAT_SN; ++k)
      if ((m >> k) & 1u) ++T.sn[k];
    if (!counted(fl)) continue;
    ++res->n_counted;
    const uint64_t L = (uint64_t)sbh_pile::l_seq_of(r);
    const uint32_t w = which_of(fl);
    const bool rev = fl & 0x10u, mapped = !(fl & 0x4u);
    T.sn[SN_TOTAL_LEN] += L;
    T.sn[w ? SN_LAST_LEN : SN_FIRST_LEN] += L;
    if (mapped) T.sn[SN_BASES_MAPPED] += L, ++T.mapq[mapq];
    if (L > T.sn[SN_MAX_LEN]) T.sn[SN_MAX_LEN] = L;
    ++T.read_len[L <= C ? L : (uint64_t)C + 1];
    uint32_t bin = 0, col = 0;
    if (isize_slot(fl, tid, mtid, (int32_t)sbh_bam::ld32(r + 8), (int32_t)sbh_bam::ld32(r + 28), (int32_t)sbh_bam::ld32(r + 32),
                   P.max_insert, &bin, &col)) {
      ++T.isize[3 * (uint64_t)bin + col];
      ++T.sn[SN_INWARD + col];
    }
    const uint8_t *seq = sbh_pile::seq_of(r), *qual = qual_of(r);
    const bool has_qual = L > 0 && qual[0] != 0xff;
    if (!has_qual) ++T.sn[SN_NO_QUAL];
    if (!L) continue;
    uint64_t g = 0;
    for (uint64_t j = 0; j < L; ++j) {
      const uint32_t row = cycle_row(j, L, rev, C), code = seq_code(seq, j);
      ++T.base[(uint64_t)row * STAT_BASES + base_channel(code, rev)];
      g += is_gc(code);
      if (has_qual) {
        const uint32_t q = qual[j];
        ++T.qual[((uint64_t)w * (C + 1) + row) * STAT_QUALS + (q < STAT_QUALS - 1 ? q : STAT_QUALS - 1)];
        T.sn[SN_SUM_QUAL] += q;
      }
    }
    ++T.gc[(uint64_t)w * STAT_GC_BINS + gc_bin(g, L)];
  }
  return 0;
}

inline const char *const *sn_labels() {
  static const char *const label[STAT_SN] = {
      "sequences", "first fragments", "last fragments", "reads mapped", "reads unmapped", "reads paired",
      "reads properly paired", "reads duplicated", "reads MQ0", "reads QC failed", "secondary alignments",
      "supplementary alignments", "total length", "total first fragment length", "total last fragment length",
      "bases mapped", "quality sum", "reads without qualities", "maximum length", "inward oriented pairs",
      "outward oriented pairs", "pairs with other orientation", "pairs on different chromosomes"};
  return label;
}

// The report, tab-separated lines under samtools stats' section tags (the tags and what a section
// means are samtools'; the bytes are this renderer's and stats.py's, which agree):
//   SN   label:  value     the STAT_SN counters in their order, then, derived here from the tables:
//                          average length (total_length / sequences, integer division; 0 without
//                          sequences), average quality (sum(qual * bin) / sum(qual), %.1f), insert size
//                          average and insert size standard deviation (over the bins below I, %.1f)
//   FFQ / LFQ  cycle (1-based), then one count per quality 0 .. the largest quality bin in use in
//              either table; a line per table row up to the last row in use in qual or base
//   GCF / GCL  bin, count: the non-empty bins of gc[0] / gc[1]
//   GCC  cycle, A, C, G, T, N: the same rows as FFQ
//   IS   size, total, inward, outward, other: up to the last non-empty bin
//   RL   length, count: the non-empty bins (bin C + 1 prints as C + 1)
//   MAPQ mapq, count: the non-empty bins
inline std::string stats_text(const Params &P, const Tables &T) {
  const uint64_t C = P.cycles, I = P.max_insert;
  auto u = [](uint64_t v) { return std::to_string((unsigned long long)v); };
  auto f1 = [](double v) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.1f", v);
    return std::string(buf);
  };
  std::string out;
  const char *const *label = sn_labels();
  for (uint32_t k = 0; k < STAT_SN; ++k) out += std::string("SN\t") + label[k] + ":\t" + u(T.sn[k]) + "\n";
  // rows and quality bins in use
  uint64_t n_rows = 0, n_quals = 0, qn = 0, qd = 0;
  for (uint64_t w = 0; w < 2; ++w)
    for (uint64_t row = 0; row <= C; ++row)
      for (uint64_t q = 0; q < STAT_QUALS; ++q) {
        const uint64_t v = T.qual[(w * (C + 1) + row) * STAT_QUALS + q];
        if (!v) continue;
        if (row + 1 > n_rows) n_rows = row + 1;
        if (q + 1 > n_quals) n_quals = q + 1;
        qn += q * v, qd += v;
      }
  for (uint64_t row = 0; row <= C; ++row)
    for (uint64_t ch = 0; ch < STAT_BASES; ++ch)
      if (T.base[row * STAT_BASES + ch] && row + 1 > n_rows) n_rows = row + 1;
  uint64_t in_ = 0, is1 = 0, is2 = 0, n_sizes = 0;
  for (uint64_t s = 0; s <= I; ++s) {
    const uint64_t t = T.isize[3 * s] + T.isize[3 * s + 1] + T.isize[3 * s + 2];
    if (!t) continue;
    n_sizes = s + 1;
    if (s < I) in_ += t, is1 += s * t, is2 += s * s * t;  // (mod 2^64, as stats.py's)
  }
  const double avg = in_ ? (double)is1 / (double)in_ : 0.0;
  double var = in_ ? (double)is2 / (double)in_ - avg * avg : 0.0;
  if (var < 0) var = 0;
  out += "SN\taverage length:\t" + u(T.sn[SN_SEQUENCES] ? T.sn[SN_TOTAL_LEN] / T.sn[SN_SEQUENCES] : 0) + "\n";
  out += "SN\taverage quality:\t" + f1(qd ? (double)qn / (double)qd : 0.0) + "\n";
  out += "SN\tinsert size average:\t" + f1(avg) + "\n";
  out += "SN\tinsert size standard deviation:\t" + f1(sqrt(var)) + "\n";
  for (uint64_t w = 0; w < 2; ++w)
    for (uint64_t row = 0; row < n_rows; ++row) {
      out += (w ? "LFQ\t" : "FFQ\t") + u(row + 1);
      for (uint64_t q = 0; q < n_quals; ++q) out += "\t" + u(T.qual[(w * (C + 1) + row) * STAT_QUALS + q]);
      out += "\n";
    }
  for (uint64_t w = 0; w < 2; ++w)
    for (uint64_t b = 0; b < STAT_GC_BINS; ++b)
      if (T.gc[w * STAT_GC_BINS + b]) out += (w ? "GCL\t" : "GCF\t") + u(b) + "\t" + u(T.gc[w * STAT_GC_BINS + b]) + "\n";
  for (uint64_t row = 0; row < n_rows; ++row) {
    out += "GCC\t" + u(row + 1);
    for (uint64_t ch = 0; ch < STAT_BASES; ++ch) out += "\t" + u(T.base[row * STAT_BASES + ch]);
    out += "\n";
  }
  for (uint64_t s = 0; s < n_sizes; ++s)
    out += "IS\t" + u(s) + "\t" + u(T.isize[3 * s] + T.isize[3 * s + 1] + T.isize[3 * s + 2]) + "\t" + u(T.isize[3 * s]) + "\t" +
           u(T.isize[3 * s + 1]) + "\t" + u(T.isize[3 * s + 2]) + "\n";
  for (uint64_t l = 0; l <= C + 1; ++l)
    if (T.read_len[l]) out += "RL\t" + u(l) + "\t" + u(T.read_len[l]) + "\n";
  for (uint64_t q = 0; q < STAT_MAPQS; ++q)
    if (T.mapq[q]) out += "MAPQ\t" + u(q) + "\t" + u(T.mapq[q]) + "\n";
  return out;
}

}  // namespace sbh_stat
