// bam_gather_core.h -- which rows of a record scan go into a BAM stream, written once for both
// sides: the device kernels (bam_gather.hip: k_bam_keep) and the host gatherer below
// (sbh_bam_gather_host, tests/sanitize/bam_gather_driver.cpp).
// SBH_HD is __host__ __device__ under hipcc, empty otherwise.
//
// Validity (k_rec_sizes' rule, records.hip): a row at flat offset p of a stream of `total` bytes
// is valid when
//   - its 36 fixed bytes lie inside the stream,
//   - l_seq >= 0,
//   - block_size >= 32 + l_read_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq,
//   - the record ends inside the stream: p + 4 + block_size <= total.
// Every row is validated, kept or not.  A row that fails only because the stream ends too early
// (the fixed bytes or the record's end lie past `total`) is "past": more resident bytes may cure it.
//
// Predicate: a row is kept when (flag & flag_require) == flag_require, (flag & flag_exclude) == 0,
// mapq >= min_mapq and its index lies in one of the row ranges [row_begin[k], row_end[k]) -- sorted,
// disjoint, non-empty; no ranges: every index passes.
//
// A kept row contributes its bytes [p, p + 4 + block_size) unchanged (bin is not recomputed).
#pragma once
#include <stdint.h>

#ifndef SBH_HD
#define SBH_HD
#endif

namespace sbh_bam {

constexpr uint64_t NO_ROW = ~0ull;

struct Filter {
  uint32_t flag_require, flag_exclude;
  int32_t min_mapq;
  const uint64_t *row_begin, *row_end;
  uint64_t n_row_ranges;
};

SBH_HD inline uint32_t ld32(const uint8_t *p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

constexpr int ROW_OK = 0, ROW_BAD = 1, ROW_PAST = 2;

// the row's verdict; *bytes = 4 + block_size when it is valid
SBH_HD inline int row_check(const uint8_t *flat, uint64_t total, uint64_t p, uint64_t *bytes) {
  *bytes = 0;
  if (p > total || total - p < 36) return ROW_PAST;
  const uint8_t *r = flat + p;
  const int64_t bsz = (int32_t)ld32(r);
  const int64_t l_name = r[12], n_cig = ld32(r + 16) & 0xffff, ls = (int32_t)ld32(r + 20);
  if (ls < 0 || bsz < 32 + l_name + 4 * n_cig + (ls + 1) / 2 + ls) return ROW_BAD;
  if ((uint64_t)bsz + 4 > total - p) return ROW_PAST;
  *bytes = (uint64_t)bsz + 4;
  return ROW_OK;
}

// row lies in one of the sorted, disjoint ranges (none: every row does)
SBH_HD inline bool row_in_ranges(const uint64_t *rb, const uint64_t *re, uint64_t nr, uint64_t row) {
  if (!nr) return true;
  uint64_t lo = 0, hi = nr;  // first range with end > row
  while (lo < hi) {
    const uint64_t m = (lo + hi) >> 1;
    if (re[m] <= row) lo = m + 1;
    else hi = m;
  }
  return lo < nr && rb[lo] <= row;
}

// r = the first byte of a valid record
SBH_HD inline bool row_keep(const uint8_t *r, uint64_t row, const Filter &F) {
  const uint32_t flag = ld32(r + 16) >> 16, mapq = r[13];
  return (flag & F.flag_require) == F.flag_require && (flag & F.flag_exclude) == 0 &&
         (int32_t)mapq >= F.min_mapq && row_in_ranges(F.row_begin, F.row_end, F.n_row_ranges, row);
}

}  // namespace sbh_bam

// ---- the host side (plain host functions under hipcc too) --------------------------------------
#include <string.h>

namespace sbh_bam {

inline bool filter_ok(const Filter &F) {
  if (F.flag_require >= 65536u || F.flag_exclude >= 65536u || F.min_mapq < 0 || F.min_mapq > 255) return false;
  if (F.n_row_ranges && (!F.row_begin || !F.row_end)) return false;
  for (uint64_t k = 0; k < F.n_row_ranges; ++k)
    if (F.row_begin[k] >= F.row_end[k] || (k && F.row_begin[k] < F.row_end[k - 1])) return false;
  return true;
}

// The opening of the four accumulators' add_host (depth_core.h, pileup_core.h, tally_core.h,
// stats_core.h): every row is validated, kept or not, as gather_host below validates them, and
// a kept row must also pass pred(r) -- the stage's own test, r the row's first byte.  Returns the first
// row that fails, or NO_ROW.
template <class Pred>
inline uint64_t first_bad_row(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n, const Filter &F,
                              Pred pred) {
  uint64_t len = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (row_check(flat, flat_size, starts[i], &len) != ROW_OK || (row_keep(flat + starts[i], i, F) && !pred(flat + starts[i])))
      return i;
  return NO_ROW;
}

// head, then the kept rows' bytes, in row order.  rec_off (n + 1 slots, n_kept + 1 written) and
// rows (n slots, n_kept written) may be NULL; out == NULL: sizes only.  Returns 0, 1 (a malformed
// row: *bad_row), 2 (out_cap too small) -- *n_kept and *bytes are set for 0 and 2.
inline int gather_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n, const uint8_t *head,
                       uint64_t head_bytes, const Filter &F, uint8_t *out, uint64_t out_cap, uint64_t *rec_off,
                       uint64_t *rows, uint64_t *n_kept, uint64_t *bytes, uint64_t *bad_row) {
  *bad_row = NO_ROW;
  *n_kept = 0;
  *bytes = head_bytes;
  uint64_t len = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (row_check(flat, flat_size, starts[i], &len) != ROW_OK) {
      *bad_row = i;
      return 1;
    }
  uint64_t k = 0, at = head_bytes;
  for (uint64_t i = 0; i < n; ++i) {
    (void)row_check(flat, flat_size, starts[i], &len);
    if (!row_keep(flat + starts[i], i, F)) continue;
    if (rec_off) rec_off[k] = at;
    if (rows) rows[k] = i;
    ++k;
    at += len;
  }
  if (rec_off) rec_off[k] = at;
  *n_kept = k;
  *bytes = at;
  if (!out) return 0;
  if (out_cap < at) return 2;
  if (head_bytes) memcpy(out, head, head_bytes);
  at = head_bytes;
  for (uint64_t i = 0; i < n; ++i) {
    (void)row_check(flat, flat_size, starts[i], &len);
    if (!row_keep(flat + starts[i], i, F)) continue;
    memcpy(out + at, flat + starts[i], len);
    at += len;
  }
  return 0;
}

}  // namespace sbh_bam
