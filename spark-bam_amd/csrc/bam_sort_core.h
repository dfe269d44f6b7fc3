// bam_sort_core.h -- the coordinate order of a record scan's rows, written once for both sides:
// the device kernels (bam_sort.hip: k_sort_keys) and the host sorter below (sbh_bam_sort_host,
// tests/sanitize/bam_sort_driver.cpp).  SBH_HD is __host__ __device__ under hipcc, empty otherwise.
//
// Key of a record, from its 36 fixed bytes (r = the record's first byte):
//   ref_id = i32 at r + 4, pos = i32 at r + 8, flag = u16 at r + 18
//   ref  = ref_id < 0 ? 0x7fffffff : ref_id             (31 bits: unplaced records last)
//   key  = (u64)ref << 33 | (u64)(u32)(pos + 1) << 1 | ((flag >> 4) & 1)
// Ascending keys are samtools' bam1_cmp_core order: reference, position, reverse strand.  Rows
// with equal keys keep the order they have in the scan: the sort is STABLE, on both sides.
//
// pos + 1 is computed in 32 unsigned bits, as the cast says: pos == -1 gives 0 (first within its
// reference), and a pos below -1 -- which no valid file holds -- wraps to a large value and sorts
// behind every real position of its reference (pos == -2 gives 0xffffffff, the very last).  That
// is defined here so that host and device agree on such a file; it is not samtools' signed order.
//
// Buffers of the device path for m kept rows of a scan of n (sbh_shard::Bam, sized for n because
// the keys are computed before m has come to the host): two key arrays (u64 [n]) and two row arrays
// (u32 [n]; the call refuses n >= 2^32 - 1) that the passes ping-pong between, the histogram
// (u64 [256 * ceil(n / SORT_TILE) + 1]) and the permuted starts and lengths (u64 [n + 1] each).
#pragma once
#include <stdint.h>

#include "bam_gather_core.h"

namespace sbh_bam {

// elements a workgroup of k_sort_hist / k_sort_scatter ranks: 4 waves x 64 lanes x 8 rounds
constexpr uint32_t SORT_WAVES = 4, SORT_ITEMS = 8, SORT_TILE = SORT_WAVES * 64 * SORT_ITEMS;

// r = the first byte of a record whose 36 fixed bytes are readable
SBH_HD inline uint64_t sort_key(const uint8_t *r) {
  const int32_t ref_id = (int32_t)ld32(r + 4);
  const uint32_t pos1 = ld32(r + 8) + 1u, rev = (ld32(r + 16) >> 20) & 1u;
  const uint64_t ref = ref_id < 0 ? 0x7fffffffull : (uint64_t)ref_id;
  return ref << 33 | (uint64_t)pos1 << 1 | rev;
}

}  // namespace sbh_bam

// ---- the host side (plain host functions under hipcc too) --------------------------------------
#include <algorithm>
#include <string>
#include <vector>

namespace sbh_bam {

// perm[k] = the row that comes k-th in stable key order.  Every row is validated first (row_check).
// Returns 0 or 1 (a malformed row: *bad_row).
inline int sort_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n, uint64_t *perm,
                     uint64_t *bad_row) {
  *bad_row = NO_ROW;
  uint64_t len = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (row_check(flat, flat_size, starts[i], &len) != ROW_OK) {
      *bad_row = i;
      return 1;
    }
  std::vector<uint64_t> key(n);
  for (uint64_t i = 0; i < n; ++i) key[i] = sort_key(flat + starts[i]), perm[i] = i;
  std::stable_sort(perm, perm + n, [&](uint64_t a, uint64_t b) { return key[a] < key[b]; });
  return 0;
}

// The BAM header bytes head[0, n) (magic, l_text, text, n_ref, references) with the @HD line's SO:
// set to `so`: an existing SO: value is replaced, an @HD line without one gets "\tSO:<so>"
// appended, a text without @HD gets "@HD\tVN:1.6\tSO:<so>\n" in front.  l_text follows; the NUL
// padding of a padded text stays behind the last line; everything else is untouched.
// Returns 0, 1 (not a BAM header: magic, l_text or the text's bounds; `so` empty or with a
// control character) or 2 (cap too small; *out_n is set).
inline int header_set_so(const uint8_t *head, uint64_t n, const char *so, uint8_t *out, uint64_t cap, uint64_t *out_n) {
  *out_n = 0;
  if (n < 12 || memcmp(head, "BAM\1", 4) != 0 || !so || !*so) return 1;
  for (const char *c = so; *c; ++c)
    if ((unsigned char)*c < 0x20 || *c == 0x7f) return 1;
  const int64_t l_text = (int32_t)ld32(head + 4);
  if (l_text < 0 || (uint64_t)l_text > n - 12) return 1;
  const char *text = reinterpret_cast<const char *>(head + 8);
  uint64_t used = (uint64_t)l_text;  // the text without its NUL padding
  while (used && text[used - 1] == 0) --used;
  std::string t(text, used);
  const std::string tag = std::string("SO:") + so;
  if (t.compare(0, 3, "@HD") == 0 && (t.size() == 3 || t[3] == '\t' || t[3] == '\n')) {
    size_t eol = t.find('\n');
    if (eol == std::string::npos) eol = t.size();
    size_t f = 3;  // the fields of the line, each led by its tab
    bool done = false;
    while (f < eol) {
      const size_t next = std::min(t.find('\t', f + 1), eol);
      if (t.compare(f, 4, "\tSO:") == 0) {
        t.replace(f + 1, next - f - 1, tag);
        done = true;
        break;
      }
      f = next;
    }
    if (!done) t.insert(eol, "\t" + tag);
  } else {
    t.insert(0, "@HD\tVN:1.6\t" + tag + "\n");
  }
  const uint64_t pad = (uint64_t)l_text - used, nt = t.size() + pad, rest = n - 8 - (uint64_t)l_text;
  if (nt > 0x7fffffffull) return 1;
  *out_n = 8 + nt + rest;
  if (!out || cap < *out_n) return 2;
  memcpy(out, head, 4);
  for (int k = 0; k < 4; ++k) out[4 + k] = (uint8_t)(nt >> (8 * k));
  memcpy(out + 8, t.data(), t.size());
  memset(out + 8 + t.size(), 0, pad);
  memcpy(out + 8 + nt, head + 8 + l_text, rest);
  return 0;
}

}  // namespace sbh_bam
