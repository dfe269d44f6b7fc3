// api_check.hip -- the C-ABI's checker stage (host only): contig lengths, the eager and full
// checkers (check.hip), FindRecordStart, the chain proof and record count, single and batched
// splits (splits.hip), and check-bam's comparison with the truth.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sbh_host.h"

using namespace sbh;

extern "C" {

int sbh_set_contigs(sbh_shard *sh, const int32_t *lens, int32_t n) {
  if (!sh || n < 0 || (n && !lens)) return SBH_E_ARG;
  int rc = set_device(sh->ctx);
  if (rc) return rc;
  HIPCHK(sh->ctx, sh->ctg.ensure(n + 1));
  if (n) HIPCHK(sh->ctx, hipMemcpyAsync(sh->ctg.p, lens, (uint64_t)n * 4, hipMemcpyHostToDevice, sh->st));
  HIPCHK(sh->ctx, hipStreamSynchronize(sh->st));
  sh->nctg = n;
  sh->h_ctg.assign(lens, lens + n);
  sh->bai.valid = sh->bai.off_ok = false;
  sh->bits_valid = sh->chain_ok = sh->cm_valid = false;
  return SBH_OK;
}

static int need_checkable(sbh_shard *sh, uint64_t begin, uint64_t end, int32_t rtc) {
  if (!sh->inflated) return fail(sh->ctx, SBH_E_STATE, "check before inflate");
  if (sh->nctg < 0) return fail(sh->ctx, SBH_E_STATE, "contig lengths not set");
  if (begin > end || end > sh->utotal) return fail(sh->ctx, SBH_E_ARG, "range [%llu,%llu) outside [0,%llu)",
                                                  (unsigned long long)begin, (unsigned long long)end,
                                                  (unsigned long long)sh->utotal);
  if (rtc < 0 || rtc > 1023) return fail(sh->ctx, SBH_E_ARG, "readsToCheck must be in [0, 1023]");
  return SBH_OK;
}

}  // extern "C"

int sbh::eager_range(sbh_shard *sh, uint64_t begin, uint64_t end, int32_t rtc, uint64_t *n_true) {
  sbh_ctx *ctx = sh->ctx;
  hipStream_t st = sh->st;
  const uint64_t nwords = (end - begin + 31) / 32;
  sh->chain_ok = sh->cm_valid = false;
  HIPCHK(ctx, sh->bits.ensure(nwords + 1));
  HIPCHK(ctx, sh->xq.ensure(2 * XQ_CAP_MAX));
  unsigned long long *c = sh->ctr.p;
  HIPCHK(ctx, hipMemsetAsync(c + ctr::EAGER_TRUE, 0, ctr::EAGER_END * 8, st));
  HIPCHK(ctx, hipMemsetAsync(c + ctr::EAGER_HALO_FIRST, 0xff, 8, st));
  mark(sh, 4);
  HIPCHK(ctx, launch_eager(sh->U.p, sh->utotal + sh->pad, begin, end, sh->d_seg.p, (uint32_t)sh->seg_end.size(),
                           sh->open_last ? 1 : 0, sh->ctg.p, sh->nctg, rtc, sh->bits.p, c, st, ~0ull, nullptr, 0,
                           sh->xq.p, XQ_CAP_MAX));
  HIPCHK(ctx, launch_eager_xq(sh->U.p, begin, sh->d_seg.p, (uint32_t)sh->seg_end.size(), sh->open_last ? 1 : 0,
                              sh->ctg.p, sh->nctg, rtc, sh->bits.p, c, sh->xq.p, XQ_CAP_MAX, st));
  mark(sh, 5);
  // (the true count and the two need-halo words)
  HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::EAGER_TRUE, c + ctr::EAGER_TRUE, (ctr::EAGER_HALO_FIRST + 1) * 8,
                             hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  sh->bits_valid = true;
  sh->bits_begin = begin;
  sh->bits_end = end;
  sh->bits_rtc = rtc;
  if (n_true) *n_true = sh->h_ctr[ctr::EAGER_TRUE];
  if (sh->h_ctr[ctr::EAGER_HALO_N]) {
    sh->bits_valid = false;
    return fail(ctx, SBH_E_NEED_HALO, "%llu positions (first %llu) need bytes past the shard",
                sh->h_ctr[ctr::EAGER_HALO_N], sh->h_ctr[ctr::EAGER_HALO_FIRST]);
  }
  return SBH_OK;
}

extern "C" {

int sbh_check_eager(sbh_shard *sh, uint64_t begin, uint64_t end, int32_t rtc, uint8_t *out_bits, uint64_t *n_true) {
  if (!sh) return SBH_E_ARG;
  int rc = need_checkable(sh, begin, end, rtc);
  if (rc) return rc;
  rc = set_device(sh->ctx);
  if (rc) return rc;
  rc = eager_range(sh, begin, end, rtc, n_true);
  if (rc) return rc;
  if (out_bits && end > begin) {
    HIPCHK(sh->ctx, hipMemcpyAsync(out_bits, sh->bits.p, (end - begin + 7) / 8, hipMemcpyDeviceToHost, sh->st));
    HIPCHK(sh->ctx, hipStreamSynchronize(sh->st));
  }
  return SBH_OK;
}

int sbh_eager_bits(sbh_shard *sh, uint64_t begin, uint64_t end, uint8_t *out_bits) {
  if (!sh || (!out_bits && end > begin)) return SBH_E_ARG;
  if (!sh->bits_valid) return fail(sh->ctx, SBH_E_STATE, "no eager bitmap");
  if (begin > end || begin < sh->bits_begin || end > sh->bits_end || (begin - sh->bits_begin) % 8)
    return fail(sh->ctx, SBH_E_ARG, "range [%llu,%llu) outside the bitmap [%llu,%llu) or unaligned",
                (unsigned long long)begin, (unsigned long long)end, (unsigned long long)sh->bits_begin,
                (unsigned long long)sh->bits_end);
  if (end == begin) return SBH_OK;
  int rc = set_device(sh->ctx);
  if (rc) return rc;
  const uint8_t *src = reinterpret_cast<const uint8_t *>(sh->bits.p) + (begin - sh->bits_begin) / 8;
  HIPCHK(sh->ctx, hipMemcpyAsync(out_bits, src, (end - begin + 7) / 8, hipMemcpyDeviceToHost, sh->st));
  HIPCHK(sh->ctx, hipStreamSynchronize(sh->st));
  return SBH_OK;
}

int sbh_check_full(sbh_shard *sh, uint64_t begin, uint64_t end, int32_t rtc, uint32_t *out_words, uint64_t *counts,
                   uint64_t *rbe_hist, uint64_t *n_success, uint64_t *close_flat, uint32_t *close_word,
                   uint64_t close_cap, uint64_t *n_close) {
  if (!sh) return SBH_E_ARG;
  int rc = need_checkable(sh, begin, end, rtc);
  if (rc) return rc;
  rc = set_device(sh->ctx);
  if (rc) return rc;
  sbh_ctx *ctx = sh->ctx;
  hipStream_t st = sh->st;
  const uint64_t nctr = ctr::FULL_END;
  unsigned long long *c = sh->ctr.p;
  HIPCHK(ctx, hipMemsetAsync(c, 0, nctr * 8, st));
  HIPCHK(ctx, hipMemsetAsync(c + ctr::FULL_UNKNOWN_MIN, 0xff, 8, st));
  uint32_t *words = nullptr;
  if (out_words) {
    HIPCHK(ctx, sh->words.ensure(end - begin + 1));
    words = sh->words.p;
  }
  const uint64_t cap = close_cap;
  HIPCHK(ctx, sh->close_pos.ensure(cap + 1));
  HIPCHK(ctx, sh->close_word.ensure(cap + 1));
  // the op index launch_full builds: one bit per byte from begin (1 KiB-aligned) to the
  // farthest CIGAR byte a position before `end` can name, plus four residue summaries
  const uint64_t u_pad = sh->utotal + sh->pad, ob0 = begin & ~1023ull;
  const uint64_t ob_top = std::min<uint64_t>(end + 36 + 255 + 4ull * 65535 + 4, u_pad);
  const uint64_t ob_nw = (((ob_top - ob0 + 31) / 32) + 63) & ~63ull;
  HIPCHK(ctx, sh->opix.ensure(ob_nw + ob_nw / 8));
  HIPCHK(ctx, launch_full(sh->U.p, u_pad, begin, end, sh->d_seg.p, (uint32_t)sh->seg_end.size(),
                          sh->open_last ? 1 : 0, sh->ctg.p, sh->nctg, rtc, words, c, sh->close_pos.p,
                          sh->close_word.p, cap, sh->opix.p, sh->opix.cap, st));
  HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr, c, nctr * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (sh->h_ctr[ctr::FULL_UNKNOWN_N])
    return fail(ctx, SBH_E_NEED_HALO, "%llu positions (first %llu) need bytes past the shard",
                sh->h_ctr[ctr::FULL_UNKNOWN_N], sh->h_ctr[ctr::FULL_UNKNOWN_MIN]);
  if (n_success) *n_success = sh->h_ctr[ctr::FULL_SUCCESS];
  const uint64_t nclose = sh->h_ctr[ctr::FULL_CLOSE_N];
  if (n_close) *n_close = nclose;
  if (counts) for (int i = 0; i < (int)ctr::FULL_COUNTS_N; ++i) counts[i] = sh->h_ctr[ctr::FULL_COUNTS + i];
  if (rbe_hist) for (int i = 0; i < (int)ctr::FULL_RBE_N; ++i) rbe_hist[i] = sh->h_ctr[ctr::FULL_RBE_HIST + i];
  const uint64_t ncopy = std::min<uint64_t>(nclose, cap);
  if (ncopy && (close_flat || close_word)) {
    // positions arrive in atomic order: sort them on the host
    std::vector<uint64_t> p(ncopy);
    std::vector<uint32_t> w(ncopy);
    HIPCHK(ctx, hipMemcpyAsync(p.data(), sh->close_pos.p, ncopy * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(w.data(), sh->close_word.p, ncopy * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    std::vector<uint64_t> idx(ncopy);
    for (uint64_t i = 0; i < ncopy; ++i) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return p[a] < p[b]; });
    for (uint64_t i = 0; i < ncopy; ++i) {
      if (close_flat) close_flat[i] = p[idx[i]];
      if (close_word) close_word[i] = w[idx[i]];
    }
  }
  if (out_words && end > begin) {
    HIPCHK(ctx, hipMemcpyAsync(out_words, sh->words.p, (end - begin) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  return SBH_OK;
}

}  // extern "C"

uint64_t sbh::seg_end_of(const sbh_shard *sh, uint64_t p) {
  for (uint64_t e : sh->seg_end)
    if (e > p) return e;
  return sh->seg_end.back();
}
static bool seg_is_open(const sbh_shard *sh, uint64_t p) {
  return sh->open_last && seg_end_of(sh, p) == sh->seg_end.back();
}

extern "C" {

// FindRecordStart.withDelta (check/.../spark/FindRecordStart.scala:30-63)
int sbh_find_record_start(sbh_shard *sh, uint64_t from, int32_t rtc, int32_t max_read_size, uint64_t *out_flat,
                          int32_t *out_delta) {
  if (!sh || !out_flat) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  int rc = need_checkable(sh, from, from, rtc);
  if (rc) return rc;
  rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  const uint64_t seg = seg_end_of(sh, from);
  const uint64_t limit = std::min<uint64_t>(seg, from + (uint64_t)std::max(max_read_size, 0));
  uint64_t lo = from;
  uint64_t window = 1 << 20;
  while (lo < limit) {
    uint64_t hi;
    bool covered = sh->bits_valid && sh->bits_rtc == rtc && sh->bits_begin <= lo && lo < sh->bits_end;
    if (covered) {
      hi = std::min(limit, sh->bits_end);
    } else {
      hi = std::min(limit, lo + window);
      window = std::min<uint64_t>(window * 4, 1ull << 28);
      rc = eager_range(sh, lo, hi, rtc, nullptr);
      if (rc == SBH_E_NEED_HALO) {
        // unknowns are fine only if a true position precedes the first unknown
        const uint64_t first_unknown = sh->h_ctr[ctr::EAGER_HALO_FIRST];
        unsigned long long *best = sh->ctr.p + ctr::FRS_BEST;
        HIPCHK(ctx, hipMemsetAsync(best, 0xff, 8, st));
        sh->bits_valid = true;
        HIPCHK(ctx, launch_first_set(sh->bits.p, lo, lo, first_unknown, best, st));
        HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::FRS_BEST, best, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        sh->bits_valid = false;
        if (sh->h_ctr[ctr::FRS_BEST] != ~0ull) {
          *out_flat = sh->h_ctr[ctr::FRS_BEST];
          if (out_delta) *out_delta = (int32_t)(sh->h_ctr[ctr::FRS_BEST] - from);
          return SBH_OK;
        }
        return rc;
      }
      if (rc) return rc;
    }
    unsigned long long *best = sh->ctr.p + ctr::FRS_BEST;
    HIPCHK(ctx, hipMemsetAsync(best, 0xff, 8, st));
    HIPCHK(ctx, launch_first_set(sh->bits.p, sh->bits_begin, lo, hi, best, st));
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::FRS_BEST, best, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (sh->h_ctr[ctr::FRS_BEST] != ~0ull) {
      *out_flat = sh->h_ctr[ctr::FRS_BEST];
      if (out_delta) *out_delta = (int32_t)(sh->h_ctr[ctr::FRS_BEST] - from);
      return SBH_OK;
    }
    lo = hi;
  }
  if (lo >= seg && seg_is_open(sh, from) && (uint64_t)max_read_size > seg - from)
    return fail(ctx, SBH_E_NEED_HALO, "record search from %llu runs past the shard", (unsigned long long)from);
  return fail_with(ctx, SBH_E_NO_READ_FOUND, {(int64_t)from, max_read_size},
                   "no read start within %d positions of flat %llu", max_read_size, (unsigned long long)from);
}

}  // extern "C"

// Records of the chain from `first` whose start is < E; *exit_flat (optional) = the
// first chain record at/after E (the successor of the last counted record, clamped to
// the stream end) -- what the next shard's first record must equal when stitching.

// `known`: the four chain-proof counters (anomalies, first anomaly, set bits, exit) that a
// k_verify_chain_w launch over this same [first, E) and bitmap already left in
// h_ctr[ctr::PROOF_ANOM, ctr::PROOF_END) (sbh_run_shard's tail): the proof is not run again.
int sbh::count_records_impl(sbh_shard *sh, uint64_t first, uint64_t E, uint64_t *count, int32_t *anomalies,
                            uint64_t *exit_flat, bool known) {
  sbh_ctx *ctx = sh->ctx;
  hipStream_t st = sh->st;
  const uint64_t total = seg_end_of(sh, first);
  E = std::min(E, total);
  if (anomalies) *anomalies = 0;
  sh->cm_valid = false;
  sh->chain_ok = false;
  if (first >= E) {
    *count = 0;
    if (exit_flat) *exit_flat = first;
    return SBH_OK;
  }
  unsigned long long *c = sh->ctr.p;
  const bool covered = sh->bits_valid && sh->bits_begin <= first && E <= sh->bits_end;
  if (covered) {
    // the proof counters: anomalies, first anomaly, set bits in [first, E), chain exit
    unsigned long long *init = sh->h_ctr + ctr::H_PROOF_INIT;  // pinned
    init[0] = 0;
    init[1] = ~0ull;
    init[2] = 0;
    init[3] = ~0ull;
    if (!known) {
      HIPCHK(ctx, hipMemcpyAsync(c + ctr::PROOF_ANOM, init, 4 * 8, hipMemcpyHostToDevice, st));
      HIPCHK(ctx, sh->cc.ensure((sh->bits_end - sh->bits_begin + 31) / 32 / VC_CHUNK + 2));
      // verify bitmap == chain and count the set bits in one pass (k_verify_chain_w: wave-
      // cooperative successors, so sparse bitmaps of long records cost no word-by-word scans)
      HIPCHK(ctx, launch_verify_chain_count(sh->U.p, sh->bits.p, sh->bits_begin, sh->bits_end, first, E, total,
                                            c + ctr::PROOF_ANOM, c + ctr::PROOF_FIRST_ANOM, c + ctr::PROOF_EXIT,
                                            c + ctr::PROOF_SET, st, nullptr, sh->cc.p));
      HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::PROOF_ANOM, c + ctr::PROOF_ANOM, 4 * 8, hipMemcpyDeviceToHost, st));
      // The proof walks the set bits of [first, E), and `first` need not be one of them: a caller's
      // record start (a BAI chunk, a stitched exit) that the eager checker rejects.  Set bits
      // further on that chain among themselves are then a suffix of the chain, not the chain,
      // so first's own bit comes back with the counters and a clear one is an anomaly at `first`.
      const uint64_t fbit = first - sh->bits_begin;
      sh->h_ctr[ctr::H_PROOF_FIRST_WORD] = 0;
      HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_PROOF_FIRST_WORD, sh->bits.p + fbit / 32, 4, hipMemcpyDeviceToHost,
                                 st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      if (!((sh->h_ctr[ctr::H_PROOF_FIRST_WORD] >> (fbit & 31)) & 1)) {
        ++sh->h_ctr[ctr::PROOF_ANOM];
        sh->h_ctr[ctr::PROOF_FIRST_ANOM] = std::min<uint64_t>(sh->h_ctr[ctr::PROOF_FIRST_ANOM], first);
      }
    }
    const uint64_t n = sh->h_ctr[ctr::PROOF_SET];
    if (sh->h_ctr[ctr::PROOF_ANOM] == 0 && sh->h_ctr[ctr::PROOF_EXIT] != ~0ull) {
      sh->chain_ok = true;
      sh->cc_ok = true;  // (this proof's chunk counts, or the run's tail proof's over the same range)
      sh->chain_first = first;
      sh->chain_E = E;
      *count = n;
      if (exit_flat) *exit_flat = sh->h_ctr[ctr::PROOF_EXIT];
      return SBH_OK;
    }
    if (anomalies) *anomalies = (int32_t)std::min<uint64_t>(sh->h_ctr[ctr::PROOF_ANOM], INT32_MAX);
    // the bitmap is not exactly the chain (false positives / rejected chain records): mark
    // the chain through the set bits by pointer doubling; the exact walk only when the
    // chain leaves the set bits
    if (n > 0 && n < 0xfffffff0ull) {
      const uint64_t nw = (E - sh->bits_begin + 31) / 32 - (first - sh->bits_begin) / 32;
      HIPCHK(ctx, sh->cm_wcnt.ensure(nw + 2));  // (chunk sums + prefix: 2 per 4096 words)
      HIPCHK(ctx, sh->cm_wpre.ensure(nw));
      HIPCHK(ctx, sh->cm_pos.ensure(n));
      HIPCHK(ctx, sh->cm_mark.ensure(n + 1));
      HIPCHK(ctx, sh->cm_mpre.ensure(n + 1));
      HIPCHK(ctx, sh->cm_j.ensure(n + 1));
      HIPCHK(ctx, sh->cm_j2.ensure(n + 1));
      HIPCHK(ctx, sh->cm_j0.ensure(n + 1));
      HIPCHK(ctx, sh->tmp.ensure(std::max(scan_tmp_words(nw), scan_tmp_words(n + 1))));
      HIPCHK(ctx, launch_rec_positions_bits(sh->bits.p, sh->bits_begin, first, E, sh->cm_wcnt.p, sh->cm_wpre.p,
                                            sh->tmp.p, sh->cm_pos.p, st));
      HIPCHK(ctx, hipMemsetAsync(c + ctr::MARK_EXIT, 0xff, 8, st));
      uint32_t *code = reinterpret_cast<uint32_t *>(sh->h_ctr + ctr::H_MARK_CODE);
      HIPCHK(ctx, launch_chain_mark(sh->U.p, sh->bits.p, sh->bits_begin, first, E, total, sh->cm_pos.p,
                                    sh->cm_wpre.p, n, sh->cm_j.p, sh->cm_j2.p, sh->cm_j0.p, sh->cm_mark.p,
                                    c + ctr::MARK_EXIT, code, env_flag("SBH_CM_DOUBLING"), st));
      HIPCHK(ctx, hipMemsetAsync(sh->cm_mark.p + n, 0, 8, st));
      HIPCHK(ctx, scan_exclusive_u64(sh->cm_mark.p, sh->cm_mpre.p, n + 1, sh->tmp.p, st));
      HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_MARK_COUNT, sh->cm_mpre.p + n, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_MARK_FIRST, sh->cm_pos.p, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_MARK_EXIT, c + ctr::MARK_EXIT, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      if (*code == (uint32_t)n && sh->h_ctr[ctr::H_MARK_FIRST] == first) {
        sh->cm_valid = true;
        sh->cm_first = first;
        sh->cm_E = E;
        sh->cm_n = n;
        *count = sh->h_ctr[ctr::H_MARK_COUNT];
        if (exit_flat) *exit_flat = sh->h_ctr[ctr::H_MARK_EXIT];
        // set bits off the chain (false positives); 0 means the bitmap is the chain
        if (anomalies) *anomalies = (int32_t)std::min<uint64_t>(n - *count, INT32_MAX);
        return SBH_OK;
      }
    }
  }
  HIPCHK(ctx, launch_chain_walk(sh->U.p, first, E, total, c + ctr::WALK_COUNT, c + ctr::WALK_EXIT, st));
  // (WALK_COUNT and WALK_EXIT)
  HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::WALK_COUNT, c + ctr::WALK_COUNT, 2 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  *count = sh->h_ctr[ctr::WALK_COUNT];
  if (exit_flat) *exit_flat = sh->h_ctr[ctr::WALK_EXIT];
  return SBH_OK;
}

extern "C" {

int sbh_count_records(sbh_shard *sh, uint64_t first, uint64_t end_flat, uint64_t *count) {
  if (!sh || !count) return SBH_E_ARG;
  if (!sh->inflated) return fail(sh->ctx, SBH_E_STATE, "count before inflate");
  if (first > sh->utotal) return SBH_E_ARG;
  int rc = set_device(sh->ctx);
  if (rc) return rc;
  return count_records_impl(sh, first, std::min(end_flat, sh->utotal), count, nullptr);
}

// CanLoadBam.loadReadsAndPositions, one split (load/.../CanLoadBam.scala:316-356)
int sbh_split(sbh_shard *sh, uint64_t start, uint64_t end, int32_t k, int32_t rtc, int32_t mrs, uint64_t *first_vpos,
              uint64_t *count) {
  if (!sh || !first_vpos || !count) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  if (!sh->inflated) return fail(ctx, SBH_E_STATE, "split before inflate");
  uint64_t b = 0;
  int rc = sbh_find_block_start(sh, start, k, &b);
  if (rc) return rc;
  const int64_t bi = block_index_of(sh, b);
  if (bi < 0) {
    if (b >= sh->file_size || (sh->at_eof && b >= sh->file_off + sh->n))
      return fail_with(ctx, SBH_E_NO_READ_FOUND, {(int64_t)start, mrs}, "split at %llu: no blocks left",
                       (unsigned long long)start);
    return fail(ctx, SBH_E_NOT_FOUND, "block start %llu is not on the indexed chain", (unsigned long long)b);
  }
  if (sh->hb[bi].flags & SBH_BLOCK_EMPTY)  // the stream from an empty block ends at once
    return fail_with(ctx, SBH_E_NO_READ_FOUND, {(int64_t)start, mrs}, "split at %llu starts at an empty block",
                     (unsigned long long)start);
  uint64_t first = 0;
  int32_t delta = 0;
  rc = sbh_find_record_start(sh, sh->hb[bi].ustart, rtc, mrs, &first, &delta);
  if (rc) return rc;
  uint64_t E = 0;
  (void)sbh_flat_bound(sh, end, &E);
  if (!sh->at_eof && end > sh->hb.back().start && E == sh->utotal)
    return fail(ctx, SBH_E_NEED_HALO, "split end %llu past the resident blocks", (unsigned long long)end);
  rc = count_records_impl(sh, first, E, count, nullptr);
  if (rc) return rc;
  uint64_t bp = 0;
  uint32_t off = 0;
  rc = sbh_pos_of(sh, first, &bp, &off);
  if (rc) return rc;
  *first_vpos = (bp << 16) | off;
  return SBH_OK;
}

// The record chain from first_flat (PosStream.scala:14-22): records whose start is < end_flat,
// and the chain's exit (its first record at/after end_flat, or where the stream ends).
int sbh_chain_from(sbh_shard *sh, uint64_t first_flat, uint64_t end_flat, uint64_t *count, uint64_t *exit_flat) {
  if (!sh || !count) return SBH_E_ARG;
  if (!sh->inflated) return fail(sh->ctx, SBH_E_STATE, "chain before inflate");
  if (first_flat > sh->utotal) return SBH_E_ARG;
  int rc = set_device(sh->ctx);
  if (rc) return rc;
  uint64_t ex = first_flat;
  rc = count_records_impl(sh, first_flat, std::min(end_flat, sh->utotal), count, nullptr, &ex);
  if (!rc && exit_flat) *exit_flat = ex;
  return rc;
}

// Every split of loadReadsAndPositions / loadSplitsAndReads at once (CanLoadBam.scala:283-297,
// 316-356; SURVEY 8b sbh_split_starts): one launch runs FindBlockStart + FindRecordStart for
// all splits (splits.hip), one proves the record chain over their union, one counts every
// split.  Splits off the common path take the exact per-split path (sbh_split), so each
// split's (status, first_vpos, count) equals sbh_split's.
int sbh_split_starts(sbh_shard *sh, const uint64_t *starts, const uint64_t *ends, uint64_t n, int32_t k, int32_t rtc,
                     int32_t mrs, uint64_t *first_vpos, uint64_t *counts, int32_t *status, uint64_t *n_host) {
  return split_starts_impl(sh, starts, ends, n, k, rtc, mrs, first_vpos, counts, status, n_host, nullptr);
}

}  // extern "C"

// SBH_SPLIT_CC=0: split counts by a popcount of each split's whole bitmap range (A/B)
static bool split_cc_on() { return env_flag("SBH_SPLIT_CC", true); }

int sbh::split_starts_impl(sbh_shard *sh, const uint64_t *starts, const uint64_t *ends, uint64_t n, int32_t k,
                           int32_t rtc, int32_t mrs, uint64_t *first_vpos, uint64_t *counts, int32_t *status,
                           uint64_t *n_host, uint8_t *hostf) {
  if (!sh || (n && (!starts || !ends || !first_vpos || !counts || !status)) || k < 0) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  if (!sh->inflated) return fail(ctx, SBH_E_STATE, "splits before inflate");
  int rc = need_checkable(sh, 0, 0, rtc);
  if (rc) return rc;
  rc = set_device(ctx);
  if (rc) return rc;
  if (n_host) *n_host = 0;
  if (!n) return SBH_OK;
  hipStream_t st = sh->st;
  const uint64_t end_res = sh->file_off + sh->n;
  // the eager bitmap from the stream start (reused when one is resident, e.g. sbh_run_shard's
  // over the owned range; a record start past its end takes the host path)
  if (!(sh->bits_valid && sh->bits_rtc == rtc && sh->bits_begin == 0)) {
    rc = eager_range(sh, 0, sh->utotal, rtc, nullptr);
    if (rc && rc != SBH_E_NEED_HALO) return rc;
    sh->bits_valid = true;  // positions needing the halo are clear; record starts past them go to the host path
    sh->bits_begin = 0;
    sh->bits_end = sh->utotal;
    sh->bits_rtc = rtc;
    if (rc == SBH_E_NEED_HALO) sh->bits_end = std::min<uint64_t>(sh->utotal, sh->h_ctr[ctr::EAGER_HALO_FIRST]);
  }
  auto rel_start = [&](uint64_t i) -> uint64_t {  // (a start off the shard: host path, flagged below)
    return starts[i] < sh->file_off || starts[i] >= end_res ? 0 : starts[i] - sh->file_off;
  };
  auto rel_end = [&](uint64_t i) -> uint64_t { return ends[i] >= sh->file_off ? ends[i] - sh->file_off : 0; };
  const SplitArgs a{sh->comp.p, sh->n, sh->at_eof ? 1 : 0, sh->cand.p, sh->ncand, sh->cand_from, k,
                    sh->b_cstart.p, sh->b_ustart.p, sh->b_flags.p, sh->nblocks, sh->utotal,
                    sh->hb.empty() ? 0 : sh->hb.back().start - sh->file_off, sh->d_seg.p,
                    (uint32_t)sh->seg_end.size(), sh->bits.p, sh->bits_begin, sh->bits_end,
                    (int64_t)std::max(mrs, 0)};
  // Fast path (the step's case): the chain proof covers the splits and left its chunk counts.
  // The ranges go over in one copy, the prologue and the counts run back to back, and
  // [first, E, count, code] come back in one copy: one round trip.  A split whose range leaves
  // the proven chain (SPLIT_NOCOUNT) sends the call down the general path below.
  if (sh->chain_ok && sh->cc_ok && sh->chain_E > 0 && split_cc_on()) {
    const uint64_t words = 5 * n + (n + 1) / 2;
    if (sh->sp_pin_cap < words) {
      if (sh->sp_pin) (void)hipHostFree(sh->sp_pin);
      sh->sp_pin = nullptr;
      sh->sp_pin_cap = 0;
      HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void **>(&sh->sp_pin), words * 8));
      sh->sp_pin_cap = words;
    }
    HIPCHK(ctx, sh->sp_pack.ensure(words));
    uint64_t *hp = sh->sp_pin, *dp = sh->sp_pack.p;
    for (uint64_t i = 0; i < n; ++i) {
      hp[i] = rel_start(i);
      hp[n + i] = rel_end(i);
    }
    uint32_t *dcode = reinterpret_cast<uint32_t *>(dp + 5 * n);
    HIPCHK(ctx, set_words(dp, hp, 2 * n, st));
    HIPCHK(ctx, launch_split_prologue(a, dp, dp + n, n, dp + 2 * n, dp + 3 * n, dcode, st));
    HIPCHK(ctx, launch_split_count_cc(sh->bits.p, sh->bits_begin, sh->cc.p, dp + 2 * n, dp + 3 * n, dcode, n,
                                      reinterpret_cast<unsigned long long *>(dp + 4 * n), st, sh->chain_first,
                                      sh->chain_E));
    // (the same page-locked words: the stream runs the copy in after the copy out has read them)
    HIPCHK(ctx, hipMemcpyAsync(hp + 2 * n, dp + 2 * n, (words - 2 * n) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint64_t *first = hp + 2 * n, *E = hp + 3 * n, *cnt = hp + 4 * n;
    const uint32_t *code = reinterpret_cast<const uint32_t *>(hp + 5 * n);
    bool all = true;
    for (uint64_t i = 0; i < n && all; ++i)
      all = !(code[i] == SPLIT_OK && starts[i] >= sh->file_off && starts[i] < end_res && first[i] < E[i] &&
              cnt[i] == SPLIT_NOCOUNT);
    if (all) {
      uint64_t nh = 0;
      for (uint64_t i = 0; i < n; ++i) {
        const uint32_t ci = starts[i] < sh->file_off || starts[i] >= end_res ? SPLIT_HOST : code[i];
        if (ci == SPLIT_OK) {
          uint64_t bp = 0;
          uint32_t off = 0;
          rc = sbh_pos_of(sh, first[i], &bp, &off);
          if (rc) return rc;
          first_vpos[i] = (bp << 16) | off;
          counts[i] = first[i] < E[i] ? cnt[i] : 0;
          status[i] = SBH_OK;
        } else if (ci == SPLIT_NOREAD) {
          first_vpos[i] = counts[i] = 0;
          status[i] = SBH_E_NO_READ_FOUND;
        } else {
          ++nh;
          if (hostf) hostf[i] = 1;
          first_vpos[i] = counts[i] = 0;
          // (sbh_split leaves sp_pin alone: first / E / cnt stay valid)
          status[i] = sbh_split(sh, starts[i], ends[i], k, rtc, mrs, &first_vpos[i], &counts[i]);
        }
      }
      if (n_host) *n_host = nh;
      return SBH_OK;
    }
  }
  std::vector<uint64_t> rs(n), re(n);
  for (uint64_t i = 0; i < n; ++i) {
    rs[i] = rel_start(i);
    re[i] = rel_end(i);
  }
  HIPCHK(ctx, sh->sp_start.ensure(n));
  HIPCHK(ctx, sh->sp_end.ensure(n));
  HIPCHK(ctx, sh->sp_first.ensure(n));
  HIPCHK(ctx, sh->sp_E.ensure(n));
  HIPCHK(ctx, sh->sp_code.ensure(n));
  HIPCHK(ctx, sh->sp_count.ensure(n));
  HIPCHK(ctx, hipMemcpyAsync(sh->sp_start.p, rs.data(), 8 * n, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(sh->sp_end.p, re.data(), 8 * n, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, launch_split_prologue(a, sh->sp_start.p, sh->sp_end.p, n, sh->sp_first.p, sh->sp_E.p, sh->sp_code.p, st));
  std::vector<uint64_t> first(n), E(n);
  std::vector<uint32_t> code(n);
  HIPCHK(ctx, hipMemcpyAsync(first.data(), sh->sp_first.p, 8 * n, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(E.data(), sh->sp_E.p, 8 * n, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(code.data(), sh->sp_code.p, 4 * n, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  uint64_t fmin = ~0ull, Emax = 0, span = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (starts[i] < sh->file_off || starts[i] >= end_res) code[i] = SPLIT_HOST;
    if (code[i] != SPLIT_OK || first[i] >= E[i]) continue;
    fmin = std::min(fmin, first[i]);
    Emax = std::max(Emax, E[i]);
    span = std::max(span, E[i] - first[i]);
  }
  bool dense = false, marked = false;
  if (fmin < Emax) {
    // the chain proof over the union of the splits: the bitmap verified equal to the chain
    // (then a split's count is a popcount), or the chain marked through the set bits
    dense = sh->chain_ok && sh->chain_first <= fmin && Emax <= sh->chain_E;
    marked = sh->cm_valid && sh->cm_first <= fmin && Emax <= sh->cm_E;
    if (!dense && !marked) {
      uint64_t cnt = 0;
      rc = count_records_impl(sh, fmin, Emax, &cnt, nullptr);
      if (rc) return rc;
      dense = sh->chain_ok && sh->chain_first <= fmin && Emax <= sh->chain_E;
      marked = sh->cm_valid && sh->cm_first <= fmin && Emax <= sh->cm_E;
    }
  }
  HIPCHK(ctx, hipMemsetAsync(sh->sp_count.p, 0, 8 * n, st));
  if (dense) {
    HIPCHK(ctx, hipMemcpyAsync(sh->sp_code.p, code.data(), 4 * n, hipMemcpyHostToDevice, st));
    if (sh->cc_ok && split_cc_on())  // the proof's chunk counts: the bitmap read only at the ranges' ends
      HIPCHK(ctx, launch_split_count_cc(sh->bits.p, sh->bits_begin, sh->cc.p, sh->sp_first.p, sh->sp_E.p,
                                        sh->sp_code.p, n, sh->sp_count.p, st));
    else
      HIPCHK(ctx, launch_split_popcount(sh->bits.p, sh->bits_begin, sh->sp_first.p, sh->sp_E.p, sh->sp_code.p, n,
                                        span, sh->sp_count.p, st));
  } else if (marked) {
    HIPCHK(ctx, hipMemcpyAsync(sh->sp_code.p, code.data(), 4 * n, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, launch_split_cm_count(sh->cm_pos.p, sh->cm_mark.p, sh->cm_mpre.p, sh->cm_n, sh->sp_first.p,
                                      sh->sp_E.p, sh->sp_code.p, n, sh->sp_count.p, st));
    HIPCHK(ctx, hipMemcpyAsync(code.data(), sh->sp_code.p, 4 * n, hipMemcpyDeviceToHost, st));
  } else {
    for (uint64_t i = 0; i < n; ++i)
      if (code[i] == SPLIT_OK && first[i] < E[i]) code[i] = SPLIT_HOST;
  }
  std::vector<unsigned long long> cnt(n);
  HIPCHK(ctx, hipMemcpyAsync(cnt.data(), sh->sp_count.p, 8 * n, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  uint64_t nh = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (code[i] == SPLIT_OK) {
      uint64_t bp = 0;
      uint32_t off = 0;
      rc = sbh_pos_of(sh, first[i], &bp, &off);
      if (rc) return rc;
      first_vpos[i] = (bp << 16) | off;
      counts[i] = first[i] < E[i] ? cnt[i] : 0;
      status[i] = SBH_OK;
      continue;
    }
    if (code[i] == SPLIT_NOREAD) {  // as sbh_split: the split starts at an empty block
      first_vpos[i] = counts[i] = 0;
      status[i] = SBH_E_NO_READ_FOUND;
      continue;
    }
    ++nh;
    if (hostf) hostf[i] = 1;
    if (env_flag("SBH_SPLIT_DEBUG"))
      fprintf(stderr, "[sbh] split %llu [%llu, %llu) host path: shard [%llu, +%llu) first %llu E %llu dense %d marked %d code %#x\n",
              (unsigned long long)i, (unsigned long long)starts[i], (unsigned long long)ends[i],
              (unsigned long long)sh->file_off, (unsigned long long)sh->n, (unsigned long long)first[i],
              (unsigned long long)E[i], (int)dense, (int)marked, code[i]);
    first_vpos[i] = counts[i] = 0;
    status[i] = sbh_split(sh, starts[i], ends[i], k, rtc, mrs, &first_vpos[i], &counts[i]);
  }
  if (n_host) *n_host = nh;
  return SBH_OK;
}

// check-bam's comparison with the `.records` truth (CheckerApp.scala:65-227) on the device:
// the eager bitmap over the hull of the selected flat ranges, the truth (htsjdk vpos of every
// record) scattered into a second bitmap, and one word-parallel compare.  fp_flat / fn_flat
// (optional) receive up to fp_cap / fn_cap mismatching flat positions, sorted: all of them
// when there are at most that many, otherwise an arbitrary subset (the compaction is in
// atomic order), not the first ones by position.
static int check_records_impl(sbh_shard *sh, const uint64_t *range_begin, const uint64_t *range_end,
                              uint64_t n_ranges, int32_t rtc, const uint64_t *rec_vpos, uint64_t n_rec,
                              bool resident, uint64_t *out, uint64_t *fp_flat, uint64_t fp_cap, uint64_t *fn_flat,
                              uint64_t fn_cap) {
  sbh_ctx *ctx = sh->ctx;
  for (uint64_t r = 0; r < n_ranges; ++r)
    if (range_begin[r] > range_end[r] || (r && range_begin[r] < range_end[r - 1]))
      return fail(ctx, SBH_E_ARG, "ranges must be sorted and disjoint");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!n_ranges) return SBH_OK;
  const uint64_t begin = range_begin[0], end = range_end[n_ranges - 1];
  int rc = need_checkable(sh, begin, end, rtc);
  if (rc) return rc;
  rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  // the eager bitmap over the hull, aligned so its words line up with the truth words
  const uint64_t hb0 = begin & ~31ull;
  if (!(sh->bits_valid && sh->bits_rtc == rtc && sh->bits_begin <= hb0 && end <= sh->bits_end &&
        sh->bits_begin % 32 == 0)) {
    rc = eager_range(sh, hb0, end, rtc, nullptr);
    if (rc) return rc;
  }
  const uint64_t nw = (end - hb0 + 31) / 32;
  HIPCHK(ctx, sh->tbits.ensure(nw + 1));
  HIPCHK(ctx, hipMemsetAsync(sh->tbits.p, 0, 4 * (nw + 1), st));
  if (!resident) {
    HIPCHK(ctx, sh->sp_vpos.ensure(n_rec + 1));
    if (n_rec) HIPCHK(ctx, hipMemcpyAsync(sh->sp_vpos.p, rec_vpos, 8 * n_rec, hipMemcpyHostToDevice, st));
  }
  HIPCHK(ctx, sh->t_rb.ensure(n_ranges));
  HIPCHK(ctx, sh->t_re.ensure(n_ranges));
  HIPCHK(ctx, hipMemcpyAsync(sh->t_rb.p, range_begin, 8 * n_ranges, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(sh->t_re.p, range_end, 8 * n_ranges, hipMemcpyHostToDevice, st));
  const uint64_t cap_fp = fp_flat ? fp_cap : 0, cap_fn = fn_flat ? fn_cap : 0;
  HIPCHK(ctx, sh->t_fp.ensure(cap_fp + 1));
  HIPCHK(ctx, sh->t_fn.ensure(cap_fn + 1));
  unsigned long long *acc = sh->ctr.p + ctr::TRUTH;  // tp, fp, fn, fp slots, fn slots, unknown
  constexpr size_t acc_bytes = (ctr::TRUTH_END - ctr::TRUTH) * 8;
  HIPCHK(ctx, hipMemsetAsync(acc, 0, acc_bytes, st));
  HIPCHK(ctx, launch_truth_scatter(sh->sp_vpos.p, n_rec, sh->b_cstart.p, sh->b_ustart.p, sh->nblocks, sh->file_off,
                                   hb0, end, sh->tbits.p, acc + (ctr::TRUTH_UNKNOWN - ctr::TRUTH), st));
  HIPCHK(ctx, launch_truth_compare(sh->bits.p, sh->bits_begin, sh->tbits.p, hb0, end, sh->t_rb.p, sh->t_re.p,
                                   n_ranges, acc, sh->t_fp.p, cap_fp, sh->t_fn.p, cap_fn, st));
  HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::TRUTH, acc, acc_bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  out[0] = sh->h_ctr[ctr::TRUTH_TP];
  out[1] = sh->h_ctr[ctr::TRUTH_FP];
  out[2] = sh->h_ctr[ctr::TRUTH_FN];
  out[3] = sh->h_ctr[ctr::TRUTH_UNKNOWN];
  // the mismatch lists arrive in atomic order and are sorted here; when there are more
  // mismatches than the cap, the listed ones are a (sorted) subset
  auto fetch = [&](uint64_t *dst, const uint64_t *src, uint64_t cap, uint64_t total) -> int {
    const uint64_t k = std::min(cap, total);
    if (!dst || !k) return SBH_OK;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, 8 * k, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    std::sort(dst, dst + k);
    return SBH_OK;
  };
  rc = fetch(fp_flat, sh->t_fp.p, cap_fp, out[1]);
  if (!rc) rc = fetch(fn_flat, sh->t_fn.p, cap_fn, out[2]);
  return rc;
}

extern "C" {

int sbh_check_records(sbh_shard *sh, const uint64_t *range_begin, const uint64_t *range_end, uint64_t n_ranges,
                      int32_t rtc, const uint64_t *rec_vpos, uint64_t n_rec, uint64_t *out /*tp, fp, fn, unknown*/,
                      uint64_t *fp_flat, uint64_t fp_cap, uint64_t *fn_flat, uint64_t fn_cap) {
  if (!sh || !out || (n_ranges && (!range_begin || !range_end)) || (n_rec && !rec_vpos)) return SBH_E_ARG;
  return check_records_impl(sh, range_begin, range_end, n_ranges, rtc, rec_vpos, n_rec, false, out, fp_flat, fp_cap,
                            fn_flat, fn_cap);
}

}  // extern "C"

int sbh::check_records_resident(sbh_shard *sh, const uint64_t *range_begin, const uint64_t *range_end,
                                uint64_t n_ranges, int32_t rtc, uint64_t n_rec, uint64_t *out, uint64_t *fp_flat,
                                uint64_t fp_cap, uint64_t *fn_flat, uint64_t fn_cap) {
  if (!sh || !out || (n_ranges && (!range_begin || !range_end)) || (n_rec && sh->sp_vpos.cap < n_rec))
    return SBH_E_ARG;
  return check_records_impl(sh, range_begin, range_end, n_ranges, rtc, nullptr, n_rec, true, out, fp_flat, fp_cap,
                            fn_flat, fn_cap);
}
