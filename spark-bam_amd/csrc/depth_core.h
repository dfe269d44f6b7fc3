// depth_core.h -- per-base depth of a record scan's rows, written once for both sides: the device
// kernels (depth.hip) and the host functions below (sbh_depth_add_host, sbh_depth_finish_host,
// tests/sanitize/depth_driver.cpp).  SBH_HD is __host__ __device__ under hipcc, empty otherwise.
//
// Spans.  An accumulator covers n_spans spans (ref_id, beg, end): 0-based, half-open,
// 0 <= beg < end <= 2^31 - 1, ref_id in [0, n_ref) and strictly ascending (one span per reference
// at most).  Span k owns len_k + 1 slots of one int32 array from off[k] = the sum of the earlier
// spans' len + 1.  The extra slot takes the closing events that fall at `end`, so the running sum
// is back at 0 where a span ends and one scan over the whole array needs no reset between spans.
// Slot indices are 64-bit.
//
// Events of one record (r = its first byte).  A row that passes the filter (bam_gather_core.h) is
// KEPT.  A kept row with ref_id < 0 counts into n_unplaced and adds nothing; with ref_id >= n_ref it
// is a bad row; with a reference that has no span it adds nothing.  Otherwise x = pos (int64) and,
// for each CIGAR word w = u32 at r + 36 + l_read_name + 4 k (any byte alignment), k < n_cigar:
//   len = w >> 4, op = w & 15;  op > 8 is a bad row (on every kept row, placed or not)
//   M(0), =(7), X(8) cover; D(2) covers with SBH_DEPTH_DEL; N(3) never does
//   a covering op's [x, x + len) is cut to the span's [beg, end); a non-empty cut [a, b) adds +1 at
//   slot off + a - beg, -1 at slot off + b - beg and b - a to cov_bases
//   M, D, N, =, X advance x by len
// All position arithmetic is 64-bit: 65535 ops of up to 2^28 - 1 bases pass 2^32, and a wrapped x
// would land back inside a span.  Flag 0x4 has no meaning of its own: the filter decides.  A long
// read's CIGAR moved to a CG:B,I tag is NOT followed: the stored CIGAR field is what counts.
//
// Validation.  Every row, kept or not, passes row_check; op codes and the reference range are checked
// on kept rows only.  The smallest bad row is reported, and nothing is added when there is one.
//
// Finish.  depth[s] = the inclusive prefix sum of the slots.  A RUN is a maximal stretch of equal
// depth inside one span: it is broken at every span start, the extra slot belongs to none, and
// zero-depth runs are included.  depth[s - 1] is the exclusive prefix at s, so slot s heads a run
// exactly when it is a span's first slot or its own value is not 0.  Stats: n_runs, max_depth,
// covered (non-extra slots of depth >= 1), sum (depth over the non-extra slots = every add's
// cov_bases together).
#pragma once
#include <stdint.h>

#include "bam_gather_core.h"

namespace sbh_dep {

// slots a workgroup of k_depth_tile_sums / _apply / _runs owns: 4 waves x 4 rounds x 64 lanes x 4
constexpr uint32_t DEPTH_TILE = 4096;
// CIGAR ops a lane of k_depth_events walks itself; a row with more is handed to its wave
constexpr uint32_t DEPTH_LANE_OPS = 16;
constexpr uint32_t FLAG_DEL = 1u;  // SBH_DEPTH_DEL
constexpr int64_t POS_MAX = 0x7fffffffll;

struct Span {  // sbh_depth_span's layout
  int32_t ref_id, pad;
  int64_t beg, end;
};

SBH_HD inline bool op_covers(uint32_t op, uint32_t flags) {
  return op == 0 || op == 7 || op == 8 || (op == 2 && (flags & FLAG_DEL));
}
SBH_HD inline bool op_advances(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

// the span of ref_id among n ascending ones, or n
SBH_HD inline uint32_t span_of(const Span *sp, uint32_t n, int32_t ref_id) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t m = (lo + hi) >> 1;
    if (sp[m].ref_id < ref_id) lo = m + 1;
    else hi = m;
  }
  return lo < n && sp[lo].ref_id == ref_id ? lo : n;
}

// [x, x + len) cut to [beg, end): false when nothing is left
SBH_HD inline bool clip(int64_t x, int64_t len, int64_t beg, int64_t end, int64_t *a, int64_t *b) {
  *a = x > beg ? x : beg;
  *b = x + len < end ? x + len : end;
  return *a < *b;
}

// r = the first byte of a valid record: its CIGAR words, and whether every op code is <= 8
SBH_HD inline const uint8_t *cigar_of(const uint8_t *r) { return r + 36 + r[12]; }
SBH_HD inline uint32_t n_cigar_of(const uint8_t *r) { return sbh_bam::ld32(r + 16) & 0xffffu; }
SBH_HD inline bool ops_ok(const uint8_t *r) {
  const uint8_t *c = cigar_of(r);
  for (uint32_t k = 0, n = n_cigar_of(r); k < n; ++k)
    if ((c[4 * k] & 15u) > 8) return false;
  return true;
}

}  // namespace sbh_dep

// ---- the host side (plain host functions under hipcc too) --------------------------------------
namespace sbh_dep {

struct AddResult {  // sbh_depth_add_result's layout
  uint64_t n, n_kept, n_counted, n_unplaced, cov_bases;
};
struct Sizes {  // sbh_depth_sizes' layout
  uint64_t slots, n_runs, covered, sum;
  uint32_t max_depth, pad;
};
struct Run {  // sbh_depth_run's layout
  int32_t ref_id;
  uint32_t depth;
  int64_t beg, end;
};

inline bool spans_ok(const Span *sp, uint32_t n, int32_t n_ref) {
  if (!sp || !n) return false;
  for (uint32_t k = 0; k < n; ++k) {
    if (sp[k].ref_id < 0 || sp[k].ref_id >= n_ref || sp[k].beg < 0 || sp[k].beg >= sp[k].end || sp[k].end > POS_MAX)
      return false;
    if (k && sp[k].ref_id <= sp[k - 1].ref_id) return false;
  }
  return true;
}

// the slots of the spans together (valid spans: the caller has checked them)
inline uint64_t slots_of(const Span *sp, uint32_t n) {
  uint64_t s = 0;
  for (uint32_t k = 0; k < n; ++k) s += (uint64_t)(sp[k].end - sp[k].beg) + 1;
  return s;
}

// Validate everything, then add.  Returns 0 or 1 (a bad row: *bad_row, the slots untouched).
inline int add_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n, const sbh_bam::Filter &F,
                    const Span *sp, uint32_t n_spans, int32_t n_ref, uint32_t flags, int32_t *slots, AddResult *res,
                    uint64_t *bad_row) {
  *res = AddResult{n, 0, 0, 0, 0};
  *bad_row = sbh_bam::first_bad_row(flat, flat_size, starts, n, F,
                                    [n_ref](const uint8_t *r) { return (int32_t)sbh_bam::ld32(r + 4) < n_ref && ops_ok(r); });
  if (*bad_row != sbh_bam::NO_ROW) return 1;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t *r = flat + starts[i];
    if (!sbh_bam::row_keep(r, i, F)) continue;
    ++res->n_kept;
    const int32_t ref_id = (int32_t)sbh_bam::ld32(r + 4);
    if (ref_id < 0) {
      ++res->n_unplaced;
      continue;
    }
    const uint32_t k = span_of(sp, n_spans, ref_id);
    if (k == n_spans) continue;
    ++res->n_counted;
    uint64_t off = 0;
    for (uint32_t j = 0; j < k; ++j) off += (uint64_t)(sp[j].end - sp[j].beg) + 1;
    int64_t x = (int32_t)sbh_bam::ld32(r + 8);
    const uint8_t *c = cigar_of(r);
    for (uint32_t j = 0, nc = n_cigar_of(r); j < nc; ++j) {
      const uint32_t w = sbh_bam::ld32(c + 4 * j), op = w & 15u;
      const int64_t l = w >> 4;
      int64_t a, b;
      if (op_covers(op, flags) && clip(x, l, sp[k].beg, sp[k].end, &a, &b)) {
        // (unsigned adds: the sum of a slot may pass through any value before the scan)
        slots[off + (uint64_t)(a - sp[k].beg)] = (int32_t)((uint32_t)slots[off + (uint64_t)(a - sp[k].beg)] + 1u);
        slots[off + (uint64_t)(b - sp[k].beg)] = (int32_t)((uint32_t)slots[off + (uint64_t)(b - sp[k].beg)] - 1u);
        res->cov_bases += (uint64_t)(b - a);
      }
      if (op_advances(op)) x += l;
    }
  }
  return 0;
}

// slots -> depth in place (the same 32 bits read as u32); runs: the first run_cap of them (may be
// NULL with run_cap 0); sz->n_runs counts them all.
inline void finish_host(int32_t *slots, const Span *sp, uint32_t n_spans, Run *runs, uint64_t run_cap, Sizes *sz) {
  *sz = Sizes{slots_of(sp, n_spans), 0, 0, 0, 0, 0};
  uint64_t s = 0;
  uint32_t d = 0;
  for (uint32_t k = 0; k < n_spans; ++k) {
    const uint64_t len = (uint64_t)(sp[k].end - sp[k].beg);
    for (uint64_t j = 0; j <= len; ++j, ++s) {
      const uint32_t v = (uint32_t)slots[s];
      d += v;
      slots[s] = (int32_t)d;
      if (j == len) break;  // the extra slot: in no run, in no stat
      if (j == 0 || v != 0) {
        if (sz->n_runs && sz->n_runs <= run_cap && j) runs[sz->n_runs - 1].end = sp[k].beg + (int64_t)j;
        if (sz->n_runs < run_cap) runs[sz->n_runs] = Run{sp[k].ref_id, d, sp[k].beg + (int64_t)j, sp[k].end};
        ++sz->n_runs;
      }
      if (d > sz->max_depth) sz->max_depth = d;
      if (d) ++sz->covered;
      sz->sum += d;
    }
    ++s;
  }
}

}  // namespace sbh_dep
