// pileup_core.h -- per-base allele counts of a record scan's rows, written once for both sides: the
// device kernels (pileup.hip) and the host functions below (sbh_pileup_add_host,
// sbh_pileup_finish_host, tests/sanitize/pileup_driver.cpp).  SBH_HD is __host__ __device__ under
// hipcc, empty otherwise.
//
// Spans are depth_core.h's: (ref_id, beg, end), 0-based, half-open, one per reference, ascending.
// Span k owns len_k = end - beg positions from off[k] = the sum of the earlier spans' lengths (no
// extra slot: nothing here is a difference array).  A position has eight u32 channels, stored
// position-major: counts[8 s + c].
//
//   A C G T (0..3)  an M / = / X base with 4-bit code 1 / 2 / 4 / 8 and quality >= min_baseq
//   N (4)           the same with any other code (0, the IUPAC codes, 15)
//   DEL (5)         a D op covers the position
//   INS (6)         an I op of length >= 1 starts right after the position
//   LOWQ (7)        an M / = / X base with quality < min_baseq, whatever its code
//
// Walk of one record (r = its first byte).  Kept, unplaced and "no span" are depth_core.h's.  x =
// pos (int64), q = 0, l_seq from the record; for each CIGAR word w (bytewise), len = w >> 4, op = w
// & 15:
//   M(0) =(7) X(8)  for j < len: reference position x + j takes query base q + j; counted when
//                   x + j lies in [beg, end)
//   D(2)            every position of [x, x + len) inside the span: DEL + 1
//   I(1)            len >= 1, x > pos and x - 1 in [beg, end): INS + 1 at x - 1 (an insertion before
//                   the first reference-consuming base is counted nowhere)
//   N S H P         nothing
//   M I S = X advance q; M D N = X advance x.  64-bit arithmetic throughout.
// Query base i: code = SEQ[i >> 1] >> 4 for even i, & 15 for odd i; quality = QUAL[i], compared
// unsigned (0xff passes every threshold).  l_seq == 0 with a CIGAR: every M / = / X position counts
// into N, no quality test.  A CG:B,I tag is not followed.
//
// Validation.  Every row passes row_check.  A kept row is bad when an op code is above 8, when
// ref_id >= n_ref, or when n_cigar > 0, l_seq > 0 and the M I S = X lengths do not sum to l_seq: a
// query index past SEQ is impossible after validation.  The smallest bad row is reported, and
// nothing is added when there is one.
//
// Finish (min_depth >= 1, call_pct in [1, 100]).  depth = A+C+G+T+N+LOWQ, total = A+C+G+T+N+DEL
// (64-bit).  Call byte: 0 when all eight channels are 0; else the letter "ACGT*" of the largest of A,
// C, G, T, DEL when that maximum is unique, total >= min_depth and best * 100 >= call_pct * total;
// else 'N'.  An INTERVAL is a maximal stretch of non-zero call bytes inside one span.
#pragma once
#include <stdint.h>

#include "depth_core.h"

namespace sbh_pile {

using sbh_dep::Span;

// positions a workgroup of k_pile_calls / k_pile_intervals owns
constexpr uint32_t PILE_TILE = 1024;
// lanes of k_pile_events that share one read: consecutive lanes take consecutive aligned bases
constexpr uint32_t PILE_GROUP = 64;
// CIGAR ops a lane of k_pile_check walks itself; a row with more is handed to its wave
constexpr uint32_t PILE_LANE_OPS = 16;
// positions of the LDS window a workgroup of k_pile_events gathers a pass's adds in (32 KiB)
constexpr uint32_t PILE_WINDOW = 2048;
constexpr uint32_t CH_A = 0, CH_C = 1, CH_G = 2, CH_T = 3, CH_N = 4, CH_DEL = 5, CH_INS = 6, CH_LOWQ = 7, NCH = 8;

SBH_HD inline bool op_aligned(uint32_t op) { return op == 0 || op == 7 || op == 8; }
SBH_HD inline bool op_query(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }
SBH_HD inline uint32_t code_channel(uint32_t code) {
  return code == 1 ? CH_A : code == 2 ? CH_C : code == 4 ? CH_G : code == 8 ? CH_T : CH_N;
}
SBH_HD inline int64_t l_seq_of(const uint8_t *r) { return (int32_t)sbh_bam::ld32(r + 20); }
SBH_HD inline const uint8_t *seq_of(const uint8_t *r) { return sbh_dep::cigar_of(r) + 4 * (uint64_t)sbh_dep::n_cigar_of(r); }

// the channel of query base i (i < l_seq) of a record whose SEQ and QUAL start at seq and qual
SBH_HD inline uint32_t base_channel(const uint8_t *seq, const uint8_t *qual, uint64_t i, uint32_t min_baseq) {
  if (qual[i] < min_baseq) return CH_LOWQ;
  const uint32_t b = seq[i >> 1];
  return code_channel((i & 1) ? (b & 15u) : (b >> 4));
}

// r = the first byte of a valid record: every op code <= 8, and the query lengths sum to l_seq
// when there is a CIGAR and a SEQ
SBH_HD inline bool walk_ok(const uint8_t *r) {
  const uint8_t *c = sbh_dep::cigar_of(r);
  const uint32_t n = sbh_dep::n_cigar_of(r);
  uint64_t qsum = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t w = sbh_bam::ld32(c + 4 * (uint64_t)k), op = w & 15u;
    if (op > 8) return false;
    if (op_query(op)) qsum += w >> 4;
  }
  const int64_t ls = l_seq_of(r);
  return n == 0 || ls == 0 || qsum == (uint64_t)ls;
}

// the call byte of one position's eight channels
SBH_HD inline uint8_t call_of(const uint32_t c[NCH], uint32_t min_depth, uint32_t call_pct) {
  if (!(c[0] | c[1] | c[2] | c[3] | c[4] | c[5] | c[6] | c[7])) return 0;
  const uint32_t v[5] = {c[CH_A], c[CH_C], c[CH_G], c[CH_T], c[CH_DEL]};
  uint32_t best = 0, at = 0, ties = 0;
  for (uint32_t k = 0; k < 5; ++k) {
    if (v[k] > best) best = v[k], at = k, ties = 0;
    else if (v[k] == best) ++ties;
  }
  const uint64_t total = (uint64_t)c[CH_A] + c[CH_C] + c[CH_G] + c[CH_T] + c[CH_N] + c[CH_DEL];
  if (ties || total < min_depth || (uint64_t)best * 100u < (uint64_t)call_pct * total) return 'N';
  return (uint8_t)("ACGT*"[at]);
}
SBH_HD inline uint64_t depth_of(const uint32_t c[NCH]) {
  return (uint64_t)c[CH_A] + c[CH_C] + c[CH_G] + c[CH_T] + c[CH_N] + c[CH_LOWQ];
}
SBH_HD inline bool is_called(uint8_t call) { return call != 0 && call != 'N'; }

}  // namespace sbh_pile

// ---- the host side (plain host functions under hipcc too) --------------------------------------
namespace sbh_pile {

struct AddResult {  // sbh_pileup_add_result's layout
  uint64_t n, n_kept, n_counted, n_unplaced, totals[NCH];
};
struct Sizes {  // sbh_pileup_sizes' layout
  uint64_t positions, n_intervals, nonzero, n_called, covered, totals[NCH];
  uint32_t max_depth, pad;
};

inline uint64_t positions_of(const Span *sp, uint32_t n) {
  uint64_t s = 0;
  for (uint32_t k = 0; k < n; ++k) s += (uint64_t)(sp[k].end - sp[k].beg);
  return s;
}

// Validate everything, then add.  Returns 0 or 1 (a bad row: *bad_row, the counts untouched).
inline int add_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n, const sbh_bam::Filter &F,
                    const Span *sp, uint32_t n_spans, int32_t n_ref, uint32_t min_baseq, uint32_t *counts, AddResult *res,
                    uint64_t *bad_row) {
  *res = AddResult{n, 0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
  *bad_row = sbh_bam::first_bad_row(flat, flat_size, starts, n, F,
                                    [n_ref](const uint8_t *r) { return (int32_t)sbh_bam::ld32(r + 4) < n_ref && walk_ok(r); });
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
    const uint32_t k = sbh_dep::span_of(sp, n_spans, ref_id);
    if (k == n_spans) continue;
    ++res->n_counted;
    uint64_t off = 0;
    for (uint32_t j = 0; j < k; ++j) off += (uint64_t)(sp[j].end - sp[j].beg);
    const int64_t beg = sp[k].beg, end = sp[k].end, pos0 = (int32_t)sbh_bam::ld32(r + 8), ls = l_seq_of(r);
    int64_t x = pos0;
    uint64_t q = 0;
    const uint8_t *c = sbh_dep::cigar_of(r), *seq = seq_of(r), *qual = seq + (ls + 1) / 2;
    auto bump = [&](int64_t p, uint32_t ch) {
      ++counts[NCH * (off + (uint64_t)(p - beg)) + ch];
      ++res->totals[ch];
    };
    for (uint32_t j = 0, nc = sbh_dep::n_cigar_of(r); j < nc; ++j) {
      const uint32_t w = sbh_bam::ld32(c + 4 * (uint64_t)j), op = w & 15u;
      const int64_t l = w >> 4;
      int64_t a, b;
      if ((op_aligned(op) || op == 2) && sbh_dep::clip(x, l, beg, end, &a, &b)) {
        for (int64_t p = a; p < b; ++p)
          bump(p, op == 2 ? CH_DEL : ls == 0 ? CH_N : base_channel(seq, qual, q + (uint64_t)(p - x), min_baseq));
      } else if (op == 1 && l >= 1 && x > pos0 && x - 1 >= beg && x - 1 < end) {
        bump(x - 1, CH_INS);
      }
      if (op_query(op)) q += (uint64_t)l;
      if (sbh_dep::op_advances(op)) x += l;
    }
  }
  return 0;
}

// counts -> calls[positions]; intervals: the first cap of them (may be NULL with cap 0);
// sz->n_intervals counts them all.
inline void finish_host(const uint32_t *counts, const Span *sp, uint32_t n_spans, uint32_t min_depth, uint32_t call_pct,
                        uint8_t *calls, Span *ivals, uint64_t cap, Sizes *sz) {
  *sz = Sizes{positions_of(sp, n_spans), 0, 0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0}, 0, 0};
  uint64_t s = 0, mx = 0;
  for (uint32_t k = 0; k < n_spans; ++k) {
    const uint64_t len = (uint64_t)(sp[k].end - sp[k].beg);
    bool open = false;
    for (uint64_t j = 0; j < len; ++j, ++s) {
      const uint32_t *c = counts + NCH * s;
      const uint8_t call = call_of(c, min_depth, call_pct);
      calls[s] = call;
      if (call && !open) {
        if (sz->n_intervals < cap) ivals[sz->n_intervals] = Span{sp[k].ref_id, 0, sp[k].beg + (int64_t)j, sp[k].end};
        ++sz->n_intervals;
      }
      if (!call && open && sz->n_intervals <= cap) ivals[sz->n_intervals - 1].end = sp[k].beg + (int64_t)j;
      open = call != 0;
      sz->nonzero += call != 0;
      sz->n_called += is_called(call);
      const uint64_t d = depth_of(c);
      sz->covered += d != 0;
      mx = d > mx ? d : mx;
      for (uint32_t ch = 0; ch < NCH; ++ch) sz->totals[ch] += c[ch];
    }
  }
  sz->max_depth = mx > 0xffffffffull ? 0xffffffffu : (uint32_t)mx;
}

}  // namespace sbh_pile
