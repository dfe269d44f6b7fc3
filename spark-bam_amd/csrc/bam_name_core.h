// bam_name_core.h -- the read-name order of a record scan's rows, written once for both sides: the
// device kernels (bam_name.hip: k_name_scan, k_name_keys, k_name_groups) and the host sorter below
// (sbh_bam_name_sort_host, tests/sanitize/name_sort_driver.cpp).  SBH_HD is __host__ __device__
// under hipcc, empty otherwise.
//
// For a record whose row passed row_check (r = its first byte):
//   l = r[12] is l_read_name; the name is the L = l ? l - 1 : 0 bytes at r + 36.  They lie inside
//   the record: row_check demands block_size >= 32 + l_read_name, so r + 36 + L <= r + 4 + block_size.
//   name_chunk(r, c), c in [0, 32): bytes [8c, 8c + 8) of the name as a big-endian u64; a byte at an
//   index >= L counts as 0, a byte below L as it is (NUL and values >= 0x80 included).
//   name_tie(r) = ((flag >> 6) & 3) << 2 | ((flag >> 11) & 1) << 1 | ((flag >> 8) & 1)
// Order: ascending name, then ascending name_tie, then scan order (the sort is STABLE, on both
// sides).  Ascending chunks 0, 1, .. 31 are the names padded with zeros to 256 bytes and compared as
// unsigned bytes: a name that is a prefix of another comes first, and for the ASCII names the SAM
// specification allows this is strcmp's and String.compareTo's order (samtools sort -N).  Two names
// that differ only in trailing NUL bytes are the same name here.
//
// The tie: READ1 / READ2 as samtools compares flag & 0xc0, then primary before secondary before
// supplementary.  It is this project's own; it makes no claim to match htsjdk's longer comparator
// chain (SAMRecordQueryNameComparator goes on to strand, mate fields and attributes).
//
// A group is a maximal run of rows of one name in that order; the summary counts the groups and
// those of 1, 2 and more rows.
#pragma once
#include <stdint.h>

#include "bam_gather_core.h"

namespace sbh_bam {

constexpr uint32_t NAME_CHUNKS = 32;  // 8-byte chunks of a name padded to 256 bytes

// r = the first byte of a valid record
SBH_HD inline uint32_t name_len(const uint8_t *r) { return r[12] ? (uint32_t)r[12] - 1u : 0u; }

// c < NAME_CHUNKS; reads name bytes below L only
SBH_HD inline uint64_t name_chunk(const uint8_t *r, uint32_t c) {
  const uint32_t L = name_len(r), b = 8 * c;
  uint64_t v = 0;
  for (uint32_t j = 0; j < 8; ++j) v = v << 8 | (b + j < L ? (uint64_t)r[36 + b + j] : 0ull);
  return v;
}

SBH_HD inline uint32_t name_tie(const uint8_t *r) {
  const uint32_t flag = ld32(r + 16) >> 16;
  return ((flag >> 6) & 3u) << 2 | ((flag >> 11) & 1u) << 1 | ((flag >> 8) & 1u);
}

// three-way comparison of the padded names alone (chunks past both names are zero on both sides)
SBH_HD inline int name_cmp_names(const uint8_t *ra, const uint8_t *rb) {
  const uint32_t La = name_len(ra), Lb = name_len(rb), L = La > Lb ? La : Lb;
  for (uint32_t c = 0; 8 * c < L; ++c) {
    const uint64_t a = name_chunk(ra, c), b = name_chunk(rb, c);
    if (a != b) return a < b ? -1 : 1;
  }
  return 0;
}

// three-way comparison of (name, tie)
SBH_HD inline int name_cmp(const uint8_t *ra, const uint8_t *rb) {
  const int c = name_cmp_names(ra, rb);
  if (c) return c;
  const uint32_t a = name_tie(ra), b = name_tie(rb);
  return a < b ? -1 : a > b ? 1 : 0;
}

// what sbh_bam_name_info holds (include/sparkbam.h: the same fields in the same order)
struct NameInfo {
  uint64_t n_names, n_single, n_pair, n_more;
  uint32_t max_name, chunks_run, passes_run;
  int32_t already;
};

}  // namespace sbh_bam

// ---- the host side (plain host functions under hipcc too) --------------------------------------
#include <algorithm>

namespace sbh_bam {

// perm[k] = the row that comes k-th in stable (name, tie) order.  Every row is validated first
// (row_check).  info (may be null): the group counts over that order, the longest name and whether
// the rows were in order as given; chunks_run and passes_run are the device's and stay 0.
// Returns 0 or 1 (a malformed row: *bad_row).
inline int name_sort_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n, uint64_t *perm,
                          NameInfo *info, uint64_t *bad_row) {
  *bad_row = NO_ROW;
  if (info) *info = NameInfo{0, 0, 0, 0, 0, 0, 0, 1};
  uint64_t len = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (row_check(flat, flat_size, starts[i], &len) != ROW_OK) {
      *bad_row = i;
      return 1;
    }
  for (uint64_t i = 0; i < n; ++i) perm[i] = i;
  std::stable_sort(perm, perm + n,
                   [&](uint64_t a, uint64_t b) { return name_cmp(flat + starts[a], flat + starts[b]) < 0; });
  if (!info) return 0;
  uint64_t run = 0;  // rows of the group under way
  auto close = [&]() {
    if (!run) return;
    ++info->n_names;
    ++(run == 1 ? info->n_single : run == 2 ? info->n_pair : info->n_more);
  };
  for (uint64_t k = 0; k < n; ++k) {
    const uint8_t *r = flat + starts[perm[k]];
    info->max_name = std::max(info->max_name, name_len(r));
    if (k && name_cmp(flat + starts[k - 1], flat + starts[k]) > 0) info->already = 0;
    if (k && name_cmp_names(flat + starts[perm[k - 1]], r) != 0) close(), run = 0;
    ++run;
  }
  close();
  return 0;
}

}  // namespace sbh_bam
