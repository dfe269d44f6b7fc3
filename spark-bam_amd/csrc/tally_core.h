// tally_core.h -- flag counts (samtools flagstat) and per-reference read counts (samtools idxstats)
// of a record scan's rows, written once for both sides: the device kernel (tally.hip) and the host
// functions below (sbh_tally_add_host, cli/spark_bam.cpp, tests/sanitize/tally_driver.cpp).
// SBH_HD is __host__ __device__ under hipcc, empty otherwise.
//
// Fields of one record (r = its first byte): flag = ld32(r + 16) >> 16, mapq = r[13],
// tid = (int32) ld32(r + 4), mtid = (int32) ld32(r + 24).
//
// A row that passes the filter (bam_gather_core.h; no filter: every row) is KEPT.  A kept row with
// tid >= n_ref is a bad row; mtid is not validated.  Every row, kept or not, passes row_check.  The
// smallest bad row is reported, and nothing is added when there is one.
//
// Flag counts: flag[TALLY_ROWS][2].  The column is 1 for a QC-fail row (0x200), else 0.  A kept row
// counts in
//    0 total                  always
//    1 primary                neither 0x100 nor 0x800
//    2 secondary              0x100 (wins over 0x800 when both are set)
//    3 supplementary          0x800 and not 0x100
//    4 duplicates             0x400
//    5 primary duplicates     primary and 0x400
//    6 mapped                 not 0x4
//    7 primary mapped         primary and not 0x4
//    8 paired                 primary and 0x1
//    9 read1                  paired and 0x40
//   10 read2                  paired and 0x80
//   11 properly paired        paired and 0x2 and not 0x4
//   12 itself and mate mapped paired and not 0x4 and not 0x8
//   13 singletons             paired and 0x8 and not 0x4
//   14 mate on a different chr       row 12 and mtid != tid
//   15 the same, mapQ >= 5           row 14 and mapq >= 5
// (samtools flagstat's loop, 1.13 and later).
//
// Per-reference counts: ref[n_ref + 1][2].  The bin is tid for 0 <= tid < n_ref and n_ref for every
// tid < 0 (idxstats' `*` line); the column is 0 (mapped) when 0x4 is clear, else 1 (unmapped).
// sum(ref[:, 0]) == flag[6][0] + flag[6][1] and sum(ref) == flag[0][0] + flag[0][1].
#pragma once
#include <stdint.h>

#include "bam_gather_core.h"

namespace sbh_tal {

constexpr uint32_t TALLY_ROWS = 16;  // SBH_TALLY_ROWS
// per-reference counters (2 per bin, u64) a workgroup of k_tally_rows keeps in LDS: 16 KiB, so that
// eight workgroups of 256 -- every wave slot of a CU -- fit its 160 KiB; a file with more than
// TALLY_LDS_BINS / 2 - 1 references counts its mixed waves by global atomics instead
constexpr uint32_t TALLY_LDS_BINS = 2048;

// bit k of the result: a kept row with these fields counts in row k (the table above)
SBH_HD inline uint32_t rows_of(uint32_t flag, uint32_t mapq, int32_t tid, int32_t mtid) {
  const bool sec = flag & 0x100u, sup = !sec && (flag & 0x800u), prim = !sec && !sup;
  const bool dup = flag & 0x400u, mapped = !(flag & 0x4u), paired = prim && (flag & 0x1u);
  const bool both = paired && mapped && !(flag & 0x8u), diff = both && mtid != tid;
  uint32_t m = 1u;
  m |= (uint32_t)prim << 1 | (uint32_t)sec << 2 | (uint32_t)sup << 3 | (uint32_t)dup << 4;
  m |= (uint32_t)(prim && dup) << 5 | (uint32_t)mapped << 6 | (uint32_t)(prim && mapped) << 7;
  m |= (uint32_t)paired << 8 | (uint32_t)(paired && (flag & 0x40u)) << 9 | (uint32_t)(paired && (flag & 0x80u)) << 10;
  m |= (uint32_t)(paired && (flag & 0x2u) && mapped) << 11 | (uint32_t)both << 12;
  m |= (uint32_t)(paired && (flag & 0x8u) && mapped) << 13 | (uint32_t)diff << 14 | (uint32_t)(diff && mapq >= 5) << 15;
  return m;
}
SBH_HD inline uint32_t qc_col(uint32_t flag) { return (flag & 0x200u) ? 1u : 0u; }
// the per-reference counter of a kept, validated row (tid < n_ref): 2 bin + column, below 2 (n_ref + 1)
SBH_HD inline uint64_t ref_slot(uint32_t flag, int32_t tid, int32_t n_ref) {
  return 2 * (uint64_t)(tid < 0 ? n_ref : tid) + ((flag & 0x4u) ? 1u : 0u);
}

}  // namespace sbh_tal

// ---- the host side (plain host functions under hipcc too) --------------------------------------
#include <stdio.h>

#include <string>

namespace sbh_tal {

struct AddResult {  // sbh_tally_add_result's layout
  uint64_t n, n_kept;
};

// Validate everything, then add into flag[TALLY_ROWS][2] and ref[n_ref + 1][2].  Returns 0 or 1 (a
// bad row: *bad_row, the arrays untouched).
inline int add_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n, const sbh_bam::Filter &F,
                    int32_t n_ref, uint64_t *flag, uint64_t *ref, AddResult *res, uint64_t *bad_row) {
  *res = AddResult{n, 0};
  *bad_row = sbh_bam::first_bad_row(flat, flat_size, starts, n, F,
                                    [n_ref](const uint8_t *r) { return (int32_t)sbh_bam::ld32(r + 4) < n_ref; });
  if (*bad_row != sbh_bam::NO_ROW) return 1;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t *r = flat + starts[i];
    if (!sbh_bam::row_keep(r, i, F)) continue;
    ++res->n_kept;
    const uint32_t fl = sbh_bam::ld32(r + 16) >> 16;
    const int32_t tid = (int32_t)sbh_bam::ld32(r + 4);
    const uint32_t m = rows_of(fl, r[13], tid, (int32_t)sbh_bam::ld32(r + 24));
    for (uint32_t k = 0; k < TALLY_ROWS; ++k)
      if ((m >> k) & 1u) ++flag[2 * k + qc_col(fl)];
    ++ref[ref_slot(fl, tid, n_ref)];
  }
  return 0;
}

// "%.2f%%" of 100 n / d in double, "N/A" when d == 0
inline std::string percent(uint64_t n, uint64_t d) {
  if (!d) return "N/A";
  char buf[64];
  snprintf(buf, sizeof buf, "%.2f%%", 100.0 * (double)n / (double)d);
  return buf;
}

// samtools flagstat's sixteen lines from flag[TALLY_ROWS][2]
inline std::string flagstat_text(const uint64_t *flag) {
  static const char *const label[TALLY_ROWS] = {
      "in total (QC-passed reads + QC-failed reads)", "primary", "secondary", "supplementary", "duplicates",
      "primary duplicates", "mapped", "primary mapped", "paired in sequencing", "read1", "read2", "properly paired",
      "with itself and mate mapped", "singletons", "with mate mapped to a different chr",
      "with mate mapped to a different chr (mapQ>=5)"};
  // the row a percentage is taken of: total for mapped, primary for primary mapped, paired for the pair rows
  static const int of[TALLY_ROWS] = {-1, -1, -1, -1, -1, -1, 0, 1, -1, -1, -1, 8, -1, 8, -1, -1};
  std::string out;
  for (uint32_t k = 0; k < TALLY_ROWS; ++k) {
    out += std::to_string((unsigned long long)flag[2 * k]) + " + " + std::to_string((unsigned long long)flag[2 * k + 1]) +
           " " + label[k];
    if (of[k] >= 0)
      out += " (" + percent(flag[2 * k], flag[2 * of[k]]) + " : " + percent(flag[2 * k + 1], flag[2 * of[k] + 1]) + ")";
    out += "\n";
  }
  return out;
}

// samtools idxstats' lines from ref[n_ref + 1][2]: name, length, mapped, unmapped per reference in
// header order, then the `*` line from bin n_ref
inline std::string idxstats_text(const uint64_t *ref, const std::string *names, const int32_t *lengths, int32_t n_ref) {
  std::string out;
  for (int32_t k = 0; k < n_ref; ++k)
    out += names[k] + "\t" + std::to_string(lengths[k]) + "\t" + std::to_string((unsigned long long)ref[2 * k]) + "\t" +
           std::to_string((unsigned long long)ref[2 * k + 1]) + "\n";
  out += "*\t0\t" + std::to_string((unsigned long long)ref[2 * (uint64_t)n_ref]) + "\t" +
         std::to_string((unsigned long long)ref[2 * (uint64_t)n_ref + 1]) + "\n";
  return out;
}

}  // namespace sbh_tal
