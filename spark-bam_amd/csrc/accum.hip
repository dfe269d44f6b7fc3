// accum.hip -- the host frame the four accumulators share (depth.hip, pileup.hip, tally.hip, stats.hip;
// declared at the end of sbh_host.h, behind the row frame it stands on): the reset, the refusals and the
// round trip of an add, the span table of depth and pileup.  No kernel lives here.
#define SBH_HD __host__ __device__
#include "depth_core.h"
#include "sbh_host.h"

namespace sbh {

int Accum::reset(void *p, uint64_t bytes) {
  int rc = set_device(ctx);
  if (rc) return rc;
  HIPCHK(ctx, hipMemsetAsync(p, 0, bytes, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return SBH_OK;
}

int add_begin(sbh_shard *sh, const Accum *a, const char *name, const char *closed, const sbh_record_filter *filter,
              sbh_bam::Filter *F) {
  sbh_ctx *ctx = sh->ctx;
  if (a->ctx != ctx) return fail(ctx, SBH_E_ARG, "%s: the shard and the accumulator belong to different contexts", name);
  if (!sh->rec.valid) return fail(ctx, SBH_E_STATE, "%s without a records scan", name);
  if (closed) return fail(ctx, SBH_E_STATE, "%s %s", name, closed);
  return row_filter(ctx, filter, F);
}

static_assert(ctr::ADD_BAD == 0 && ctr::ADD_PAST == 1 && ctr::ADD_A == 2 && ctr::ADD_B == 3 && ctr::ADD_HEAD == 4,
              "two memsets, one copy back: bad and past side by side, a and b behind them");

int AddTrip::open(sbh_bam::Filter *F, DBuf<uint64_t> *keep, uint64_t zeroed) const {
  sbh_ctx *ctx = sh->ctx;
  int rc = set_device(ctx);
  if (rc) return rc;
  if (keep) HIPCHK(ctx, keep->ensure((sh->rec.sz.n + 63) / 64));
  HIPCHK(ctx, stage_row_ranges(sh, F));
  HIPCHK(ctx, hipMemsetAsync(head, 0xff, 16, sh->st));
  HIPCHK(ctx, hipMemsetAsync(head + ctr::ADD_A, 0, 8 * zeroed, sh->st));
  return SBH_OK;
}

int AddTrip::verdict(const char *also) const {
  const unsigned long long *h = sh->h_ctr + mirror;
  HIPCHK(sh->ctx, hipMemcpyAsync(sh->h_ctr + mirror, head, 8 * ctr::ADD_HEAD, hipMemcpyDeviceToHost, sh->st));
  HIPCHK(sh->ctx, hipStreamSynchronize(sh->st));
  return rows_verdict(sh, h[ctr::ADD_BAD], h[ctr::ADD_PAST], also);
}

// ---- the span table ------------------------------------------------------------------------------
int spans_refused(sbh_ctx *ctx, const char *stage, const sbh_depth_span *sp, uint32_t n_spans, int32_t n_ref) {
  static_assert(sizeof(sbh_depth_span) == sizeof(sbh_dep::Span), "depth_core.h restates the header's layout");
  if (sbh_dep::spans_ok(reinterpret_cast<const sbh_dep::Span *>(sp), n_spans, n_ref)) return SBH_OK;
  return fail(ctx, SBH_E_ARG, "%s spans: at least one, ref_id in [0, n_ref) strictly ascending, 0 <= beg < end <= 2^31 - 1",
              stage);
}

void SpanTable::assign(const sbh_depth_span *sp, uint32_t n_spans, uint32_t extra) {
  spans.assign(sp, sp + n_spans);
  off.assign(n_spans + 1, 0);
  for (uint32_t k = 0; k < n_spans; ++k) off[k + 1] = off[k] + (uint64_t)(sp[k].end - sp[k].beg) + extra;
  S = off[n_spans];
}

hipError_t SpanTable::upload(uint64_t n_tiles, hipStream_t st) {
  const uint64_t ns = spans.size();
  if (n_tiles >= 0x7fffffffull) return hipErrorOutOfMemory;
  hipError_t e = d_spans.ensure(ns);
  if (e == hipSuccess) e = d_off.ensure(ns + 1);
  if (e == hipSuccess) e = hipMemcpyAsync(d_spans.p, spans.data(), ns * sizeof(sbh_depth_span), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_off.p, off.data(), 8 * (ns + 1), hipMemcpyHostToDevice, st);
  return e;
}

int SpanTable::range(sbh_ctx *ctx, const char *what, uint32_t span, uint64_t from, uint64_t n) const {
  if (span >= spans.size()) return fail(ctx, SBH_E_ARG, "%s: span %u of %zu", what, span, spans.size());
  const uint64_t len = (uint64_t)(spans[span].end - spans[span].beg);
  if (from > len || n > len - from) return fail(ctx, SBH_E_ARG, "%s past the span", what);
  return SBH_OK;
}

}  // namespace sbh
