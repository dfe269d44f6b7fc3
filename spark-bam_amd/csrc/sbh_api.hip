// sbh_api.hip -- the C-ABI (include/sparkbam.h), the shard and its bytes: version, context, last
// error, shard lifetime and loading, the window prefetch threads, FindBlockStart, the block index,
// inflate and the position maps, and the whole-shard runs (run_pipelined, sbh_run_shard, the two
// streaming runs).  The other entry points sit with their stage: api_check.hip (checkers, chain,
// splits), api_records.hip (record decode), and behind the kernels of bai.hip, sam.hip,
// bam_gather.hip, depth.hip and zdeflate.hip.  What they share is in sbh_host.h.
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "sbh_host.h"

using namespace sbh;

namespace {
// the calling thread's last failed call: which context it was on, the message, the status and the
// fields the reference's exception is constructed from (e.g. HeaderParseException(idx, actual,
// expected)); sbh_last_error / sbh_last_error_detail read it back on the same thread
struct ErrRec {
  const sbh_ctx *ctx = nullptr;
  std::string msg;
  int32_t code = 0, n = 0;
  int64_t fields[4] = {0, 0, 0, 0};
};
thread_local ErrRec t_err;
}  // namespace

static int vfail(sbh_ctx *ctx, int code, std::initializer_list<int64_t> fields, const char *fmt, va_list ap) {
  if (ctx) {
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    ErrRec &E = t_err;
    E.ctx = ctx;
    E.msg = buf;
    E.code = code;
    E.n = 0;
    for (int64_t f : fields)
      if (E.n < 4) E.fields[E.n++] = f;
  }
  return code;
}

int sbh::fail(sbh_ctx *ctx, int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfail(ctx, code, {}, fmt, ap);
  va_end(ap);
  return code;
}

// fail() with the fields the reference's exception takes (sbh_last_error_detail)
int sbh::fail_with(sbh_ctx *ctx, int code, std::initializer_list<int64_t> fields, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfail(ctx, code, fields, fmt, ap);
  va_end(ap);
  return code;
}

void sbh::mark(sbh_shard *sh, int i) {
  if (!sh->timing) return;
  if (!sh->ev_ok) {
    sh->ev_ok = true;
    for (hipEvent_t &e : sh->ev)
      if (hipEventCreate(&e) != hipSuccess) sh->ev_ok = false;
  }
  if (sh->ev_ok) (void)hipEventRecord(sh->ev[i], sh->st);
}

int sbh::set_device(sbh_ctx *ctx) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return SBH_OK;
}

// The shard's resident bytes are now [file_off, file_off + n) of the file (sbh_shard_load, a
// prefetched window taken into use): every state derived from the old bytes is void.
void sbh::resident_changed(sbh_shard *sh, uint64_t file_off, uint64_t n) {
  sh->file_off = file_off;
  sh->n = n;
  sh->at_eof = file_off + n == sh->file_size;
  sh->indexed = sh->inflated = sh->bits_valid = sh->chain_ok = sh->cm_valid = false;
  sh->rec.valid = false;
  sh->bai.valid = false;
  sh->sam.valid = false;
  sh->bam.valid = false;
  sh->fq.valid = false;
  sh->ncand = 0;
  sh->scan_from = ~0ull;
  sh->hb.clear();
  sh->nblocks = sh->utotal = 0;
}

extern "C" {

const char *sbh_version(void) { return "sparkbam-hip 0.1 (gfx950)"; }

int sbh_ctx_create(int device, sbh_ctx **out) {
  if (!out) return SBH_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SBH_E_HIP;
  sbh_ctx *c = new sbh_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess) {
    delete c;
    return SBH_E_HIP;
  }
  // SBH_SCHED=spin|yield|block: how a host thread waits in hipStreamSynchronize (the path's
  // host round trips -- index sizes, block table, statuses -- each leave the GPU idle until the
  // host thread wakes); unset: the runtime's default
  if (const char *e = env_str("SBH_SCHED")) {
    const unsigned f = !std::strcmp(e, "spin")    ? hipDeviceScheduleSpin
                       : !std::strcmp(e, "yield") ? hipDeviceScheduleYield
                       : !std::strcmp(e, "block") ? hipDeviceScheduleBlockingSync
                                                  : hipDeviceScheduleAuto;
    // the flag only takes before the device's primary context is active; a refusal is reported
    // (stderr) rather than silently ignored, so an A/B of wait modes shows whether it applied
    const hipError_t fe = hipSetDeviceFlags(f);
    std::fprintf(stderr, "sparkbam-hip: SBH_SCHED=%s %s (%s)\n", e, fe == hipSuccess ? "applied" : "NOT applied",
                 hipGetErrorString(fe));
  }
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return SBH_E_HIP;
  }
  c->own_stream = true;
  *out = c;
  return SBH_OK;
}

int sbh_ctx_destroy(sbh_ctx *ctx) {
  if (!ctx) return SBH_OK;
  if (!ctx->sc_free.empty()) {
    (void)hipSetDevice(ctx->device);
    for (StreamCache *sc : ctx->sc_free) delete sc;
    ctx->sc_free.clear();
  }
  if (ctx->own_stream && ctx->stream) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamDestroy(ctx->stream);
  }
  delete ctx;
  return SBH_OK;
}

const char *sbh_last_error(const sbh_ctx *ctx) {
  if (!ctx) return "no context";
  return t_err.ctx == ctx ? t_err.msg.c_str() : "";
}

int32_t sbh_last_error_detail(const sbh_ctx *ctx, int32_t *code, int64_t *fields, int32_t cap) {
  if (!ctx) return 0;
  const ErrRec &E = t_err;
  const bool mine = E.ctx == ctx;
  if (code) *code = mine ? E.code : 0;
  if (!mine) return 0;
  const int32_t n = fields ? std::min(E.n, std::max(cap, 0)) : 0;
  for (int32_t i = 0; i < n; ++i) fields[i] = E.fields[i];
  return E.n;
}

int sbh_host_alloc(uint64_t n, void **out) {
  if (!out) return SBH_E_ARG;
  *out = nullptr;
  return hipHostMalloc(out, std::max<uint64_t>(n, 1), hipHostMallocDefault) == hipSuccess ? SBH_OK : SBH_E_NOMEM;
}

int sbh_host_free(void *p) { return p && hipHostFree(p) != hipSuccess ? SBH_E_HIP : SBH_OK; }

int sbh_ctx_set_stream(sbh_ctx *ctx, void *hip_stream) {
  if (!ctx) return SBH_E_ARG;
  (void)hipSetDevice(ctx->device);
  {
    // the idle window caches hold shards with streams of their own: let them go, so that every
    // shard built from here on -- sbh_run_stream2's window shard included -- is on the caller's stream
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (StreamCache *sc : ctx->sc_free) delete sc;
    ctx->sc_free.clear();
  }
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);  // (null: the null stream)
  ctx->own_stream = false;
  return SBH_OK;
}

int sbh_ctx_synchronize(sbh_ctx *ctx) {
  if (!ctx) return SBH_E_ARG;
  int rc = set_device(ctx);
  if (rc) return rc;
  // the context's work is on its stream (its own or the caller's) and on the streams of its shards
  // and accumulators: wait for the stream, then for the device
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipDeviceSynchronize());
  return SBH_OK;
}

// Header.make (bgzf/.../block/Header.scala:48-83)
int sbh_header_make(const uint8_t *b, uint64_t avail, int32_t *hsize, int32_t *csize) {
  if (!b || avail < 18) return SBH_E_TRUNCATED;
  if (b[0] != 31 || b[1] != 139 || b[2] != 8 || b[3] != 4) return SBH_E_HEADER_PARSE;
  if (b[12] != 66 || b[13] != 67 || b[14] != 2) return SBH_E_HEADER_PARSE;
  const int32_t xlen = (int32_t)b[10] | ((int32_t)b[11] << 8);
  if (hsize) *hsize = 18 + xlen - 6;
  if (csize) *csize = ((int32_t)b[16] | ((int32_t)b[17] << 8)) + 1;
  return SBH_OK;
}

int sbh_shard_create(sbh_ctx *ctx, const void *src, uint64_t n, uint64_t file_offset, uint64_t file_size,
                     int comp_on_device, sbh_shard **out) {
  if (!ctx || !out || (!src && n) || file_offset + n > file_size) return SBH_E_ARG;
  int rc = set_device(ctx);
  if (rc) return rc;
  sbh_shard *sh = new sbh_shard();
  sh->ctx = ctx;
  if (ctx->own_stream) {
    if (hipStreamCreateWithFlags(&sh->st, hipStreamNonBlocking) != hipSuccess) {
      delete sh;
      return fail(ctx, SBH_E_HIP, "shard create: no stream");
    }
    sh->own_st = true;
  } else {
    sh->st = ctx->stream;  // the caller's (sbh_ctx_set_stream): never destroyed here
  }
  sh->file_off = file_offset;
  sh->n = n;
  sh->file_size = file_size;
  sh->at_eof = file_offset + n == file_size;
  hipError_t e = sh->comp.ensure(n + sh->pad);
  if (e == hipSuccess && n)
    e = hipMemcpyAsync(sh->comp.p, src, n, comp_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                       sh->st);
  if (e == hipSuccess) e = hipMemsetAsync(sh->comp.p + n, 0, sh->pad, sh->st);
  if (e == hipSuccess) e = sh->ctr.ensure(CTR_WORDS);
  // (layout: sbh_internal.h; k_eager's true-count slots must start zero, k_fold_true keeps them so)
  if (e == hipSuccess) e = hipMemsetAsync(sh->ctr.p, 0, CTR_WORDS * sizeof(unsigned long long), sh->st);
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&sh->h_ctr), CTR_WORDS * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipStreamSynchronize(sh->st);
  if (e != hipSuccess) {
    sbh_shard_destroy(sh);
    return fail(ctx, SBH_E_HIP, "shard create: %s", hipGetErrorString(e));
  }
  *out = sh;
  return SBH_OK;
}

int sbh_shard_destroy(sbh_shard *sh) {
  delete sh;  // (~sbh_shard; a null shard is fine)
  return SBH_OK;
}

// A copy stream at another priority than the compute streams: its hardware queue then comes from
// another pool, so no compute stream shares it (a copy in flight on a shared queue held the next
// window's kernels behind it: e2e 130 -> 84 GB/s depending on stream creation order).  A device
// with a single priority gets a plain stream.
static hipError_t copy_stream_create(hipStream_t *cs) {
  int least = 0, greatest = 0;
  const hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (e != hipSuccess) return e;
  return greatest != least ? hipStreamCreateWithPriority(cs, hipStreamNonBlocking, greatest)
                           : hipStreamCreateWithFlags(cs, hipStreamNonBlocking);
}

int sbh_shard_load(sbh_shard *sh, const void *src, uint64_t n, uint64_t file_offset, int comp_on_device) {
  if (!sh || (!src && n) || file_offset + n > sh->file_size) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  int rc = set_device(ctx);
  if (rc) return rc;
  // No kernel may still read the old bytes.  On the caller's stream (sbh_ctx_set_stream) this wait
  // is also what orders the copy below, which runs on another stream, behind the work that wrote
  // `src`: nothing else ties the copy stream to the shard's stream before the copy.
  HIPCHK(ctx, hipStreamSynchronize(sh->st));
  HIPCHK(ctx, sh->comp.ensure(n + sh->pad));
  // the copy on the shard's copy stream: its hardware queue is never one another task's kernels
  // wait behind
  if (!sh->cs) HIPCHK(ctx, copy_stream_create(&sh->cs));
  if (n)
    HIPCHK(ctx, hipMemcpyAsync(sh->comp.p, src, n, comp_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                               sh->cs));
  HIPCHK(ctx, hipStreamSynchronize(sh->cs));
  HIPCHK(ctx, hipMemsetAsync(sh->comp.p + n, 0, sh->pad, sh->st));
  HIPCHK(ctx, hipStreamSynchronize(sh->st));
  resident_changed(sh, file_offset, n);
  return SBH_OK;
}

}  // extern "C"

namespace sbh {

// copy threads per prefetch (SBH_PREFETCH_THREADS, default 4), each hipMemcpyAsync-ing its
// part on its own stream, pageable host memory (a mapped file, a numpy array) included.  (Measured
// and removed: staging pageable memory through page-locked chunks of the threads' own, 2.32 s
// against 2.34 s on a 100.9 GiB file and slower on a 5 GiB one -- DESIGN_HISTORY.md.)
static uint32_t prefetch_threads() { return (uint32_t)env_uint("SBH_PREFETCH_THREADS", 4, 1, 16); }

int shard_prefetch(sbh_shard *sh, const void *src, uint64_t n, uint64_t file_offset, const uint64_t *aux,
                   uint64_t n_aux) {
  if (!sh || (!src && n) || (!aux && n_aux) || file_offset + n > sh->file_size || sh->pf_active) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  int rc = set_device(ctx);
  if (rc) return rc;
  // buffers are sized here, on the calling thread (the copy threads only copy)
  HIPCHK(ctx, sh->comp2.ensure(n + sh->pad));
  HIPCHK(ctx, sh->aux2.ensure(n_aux + 1));
  const uint32_t nt = prefetch_threads();
  while (sh->pf_stream.size() < nt) {
    hipStream_t st = nullptr;
    HIPCHK(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    sh->pf_stream.push_back(st);
  }
  sh->pf_active = true;
  sh->pf_off = file_offset, sh->pf_n = n, sh->pf_naux = n_aux;
  sh->pf_err.assign(nt, hipSuccess);
  sh->pf_ms.assign(nt, 0.0);
  sh->pf.clear();
  const int dev = ctx->device;
  uint8_t *dst = sh->comp2.p;
  uint64_t *adst = sh->aux2.p;
  const uint64_t pad = sh->pad, part = (n / nt + 4095) & ~4095ull;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t k = 0; k < nt; ++k) {
    const uint64_t lo = std::min(n, k * part), hi = k + 1 == nt ? n : std::min(n, (k + 1) * part);
    hipStream_t cs = sh->pf_stream[k];
    hipError_t *err = &sh->pf_err[k];
    double *ms = &sh->pf_ms[k];
    sh->pf.emplace_back([=]() {
      // [from, from + len) of host memory to device memory at to
      auto copy = [&](void *to, const void *from, uint64_t len) {
        return len ? hipMemcpyAsync(to, from, len, hipMemcpyHostToDevice, cs) : hipSuccess;
      };
      hipError_t e = hipSetDevice(dev);
      if (e == hipSuccess) e = copy(dst + lo, static_cast<const uint8_t *>(src) + lo, hi - lo);
      if (e == hipSuccess && k == 0) e = hipMemsetAsync(dst + n, 0, pad, cs);
      if (e == hipSuccess && k == 0 && n_aux) e = copy(adst, aux, 8 * n_aux);
      if (e == hipSuccess) e = hipStreamSynchronize(cs);
      *err = e;
      *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    });
  }
  return SBH_OK;
}

bool shard_prefetch_pending(const sbh_shard *sh, uint64_t *file_offset, uint64_t *n) {
  if (!sh || !sh->pf_active) return false;
  if (file_offset) *file_offset = sh->pf_off;
  if (n) *n = sh->pf_n;
  return true;
}

int shard_prefetch_finish(sbh_shard *sh, bool use, double *copy_ms) {
  if (!sh || !sh->pf_active) return SBH_E_STATE;
  sbh_ctx *ctx = sh->ctx;
  for (std::thread &th : sh->pf)
    if (th.joinable()) th.join();
  sh->pf.clear();
  sh->pf_active = false;
  if (copy_ms) *copy_ms = sh->pf_ms.empty() ? 0.0 : *std::max_element(sh->pf_ms.begin(), sh->pf_ms.end());
  for (hipError_t e : sh->pf_err)
    if (e != hipSuccess) return fail(ctx, SBH_E_HIP, "window prefetch: %s", hipGetErrorString(e));
  if (!use) return SBH_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(sh->st));  // (no kernel may still read the old bytes)
  std::swap(sh->comp, sh->comp2);
  std::swap(sh->sp_vpos, sh->aux2);
  resident_changed(sh, sh->pf_off, sh->pf_n);
  return SBH_OK;
}

}  // namespace sbh

extern "C" {

const void *sbh_shard_comp_device_ptr(sbh_shard *sh) { return sh ? sh->comp.p : nullptr; }

// FindBlockStart.apply (bgzf/.../block/FindBlockStart.scala:8-36)
int sbh_find_block_start(sbh_shard *sh, uint64_t start, int32_t k, uint64_t *out) {
  if (!sh || !out || k < 0 || start < sh->file_off) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  int rc = set_device(ctx);
  if (rc) return rc;
  const uint64_t rel = start - sh->file_off;
  unsigned long long *best = sh->ctr.p + ctr::FBS_BEST;
  HIPCHK(ctx, hipMemsetAsync(best, 0xff, 8, sh->st));
  HIPCHK(ctx, launch_find_block_start(sh->comp.p, sh->n, rel, k, sh->at_eof ? 1 : 0, best, sh->st));
  HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::FBS_BEST, best, 8, hipMemcpyDeviceToHost, sh->st));
  HIPCHK(ctx, hipStreamSynchronize(sh->st));
  const unsigned long long b = sh->h_ctr[ctr::FBS_BEST];
  // HeaderSearchFailedException(path, start, positionsAttempted): the search tried every
  // pos < MAX_BLOCK_SIZE (FindBlockStart.scala:18-35)
  if (b == ~0ull)
    return fail_with(ctx, SBH_E_HEADER_SEARCH_FAILED, {(int64_t)start, 65536}, "no BGZF block start in [%llu, %llu)",
                     (unsigned long long)start, (unsigned long long)(start + 65536));
  const uint32_t outcome = (uint32_t)(b & 0xff);
  const uint64_t pos = b >> 8;
  if (outcome == 2) return fail(ctx, SBH_E_TRUNCATED, "truncated BGZF block near %llu", (unsigned long long)(start + pos));
  if (outcome == 3) return fail(ctx, SBH_E_NEED_HALO, "FindBlockStart(%llu) needs bytes past the shard", (unsigned long long)start);
  *out = start + pos;
  return SBH_OK;
}

// SBH_CHAIN_JUMP=1: the index always builds the block chain by pointer jumping (the path a
// chain with false-positive candidates takes), for tests and A/B.
static bool chain_jump_only() { return env_flag("SBH_CHAIN_JUMP"); }

// MetadataStream from `start` (bgzf/.../block/MetadataStream.scala:16-58)
int sbh_index(sbh_shard *sh, uint64_t start, uint64_t *n_blocks, uint64_t *flat_size) {
  if (!sh || start < sh->file_off || start > sh->file_off + sh->n) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  hipStream_t st = sh->st;
  int rc = set_device(ctx);
  if (rc) return rc;
  sh->indexed = sh->inflated = sh->bits_valid = sh->chain_ok = sh->cm_valid = false;
  // a new index rebases every flat offset: the last scan's positions, and what was rendered from
  // them, describe a stream that is no longer there (what resident_changed voids of them)
  sh->rec.valid = sh->rec.decoded = false;
  sh->bai.valid = false;
  sh->sam.valid = false;
  sh->bam.valid = false;
  sh->fq.valid = false;
  sh->ncand = 0;
  const uint64_t rel = start - sh->file_off;
  const uint64_t n = sh->n;
  const uint64_t srel = sh->scan_from >= sh->file_off && sh->scan_from <= start ? sh->scan_from - sh->file_off : 0;
  // the start must itself be a header (its 18 bytes come back with the candidate count)
  uint8_t *h18 = reinterpret_cast<uint8_t *>(sh->h_ctr + ctr::H_INDEX_HDR18);  // pinned
  auto start_is_header = [&]() -> int {
    if (sbh_header_make(h18, 18, nullptr, nullptr) != SBH_OK) {
      // HeaderParseException(idx, actual, expected): the first byte Header.make's checks
      // reject, in its order (Header.scala:48-71)
      static const uint8_t idx[7] = {0, 1, 2, 3, 12, 13, 14}, want[7] = {31, 139, 8, 4, 66, 67, 2};
      int k = 0;
      while (k < 6 && h18[idx[k]] == want[k]) ++k;
      return fail_with(ctx, SBH_E_HEADER_PARSE, {(int64_t)start, idx[k], (int8_t)h18[idx[k]], (int8_t)want[k]},
                       "Position %d: %d != %d (BGZF header at %llu)", idx[k], (int8_t)h18[idx[k]], (int8_t)want[k],
                       (unsigned long long)start);
    }
    return SBH_OK;
  };
  if (rel + 18 <= n) HIPCHK(ctx, hipMemcpyAsync(h18, sh->comp.p + rel, 18, hipMemcpyDeviceToHost, st));
  const uint64_t nchunks = cand_chunks(n);
  uint64_t nc = 0;
  if (rel + 18 <= n && !nchunks) {
    HIPCHK(ctx, hipStreamSynchronize(st));
    if ((rc = start_is_header()) != SBH_OK) return rc;
  }
  if (nchunks && rel + 18 <= n) {
    // (counts[nchunks] = 0, written by k_cand_count: the scan over nchunks + 1 entries leaves the
    // candidate total in offs[nchunks], one word back)
    HIPCHK(ctx, sh->counts.ensure(nchunks + 1));
    HIPCHK(ctx, sh->cfirst.ensure(nchunks));
    HIPCHK(ctx, sh->offs.ensure(nchunks + 1));
    HIPCHK(ctx, sh->tmp.ensure(scan_tmp_words(nchunks + 1) + scan_tmp_words(1 << 24)));
    HIPCHK(ctx, launch_cand_count(sh->comp.p, n, srel, sh->counts.p, sh->cfirst.p, nchunks, st));
    HIPCHK(ctx, scan_exclusive_u64(sh->counts.p, sh->offs.p, nchunks + 1, sh->tmp.p, st));
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_INDEX_NCAND, sh->offs.p + nchunks, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if ((rc = start_is_header()) != SBH_OK) return rc;
    nc = sh->h_ctr[ctr::H_INDEX_NCAND];
  }
  uint64_t nchain = 0;
  // the 18 bytes after the last chain block (the next header, checked below), written by
  // k_chain_emit and copied back with the block table
  uint8_t *next18_dev = reinterpret_cast<uint8_t *>(sh->ctr.p + CTR_NEXT18);
  uint8_t *nx = reinterpret_cast<uint8_t *>(sh->h_ctr + ctr::H_INDEX_NEXT18);  // pinned
  if (nc) {
    HIPCHK(ctx, sh->cand.ensure(nc));
    HIPCHK(ctx, sh->J0.ensure(nc));
    HIPCHK(ctx, sh->J1.ensure(nc));
    HIPCHK(ctx, sh->on.ensure(nc));
    HIPCHK(ctx, sh->v.ensure(nc));
    HIPCHK(ctx, sh->rank.ensure(nc));
    HIPCHK(ctx, sh->tmp.ensure(scan_tmp_words(nc) + scan_tmp_words(nchunks + 1)));
    HIPCHK(ctx, launch_cand_write(sh->comp.p, n, srel, sh->counts.p, sh->cfirst.p, sh->offs.p, sh->cand.p, nchunks, st));
    HIPCHK(ctx, sh->b_cstart.ensure(nc));
    HIPCHK(ctx, sh->b_ustart.ensure(nc));
    HIPCHK(ctx, sh->usz.ensure(nc));
    HIPCHK(ctx, sh->b_csize.ensure(nc));
    HIPCHK(ctx, sh->b_hsize.ensure(nc));
    HIPCHK(ctx, sh->b_usize.ensure(nc));
    HIPCHK(ctx, sh->b_flags.ensure(nc));
    HIPCHK(ctx, sh->b_status.ensure(nc));
    HIPCHK(ctx, sh->b_ntok.ensure(nc));
  }
  sh->ncand = nc;
  sh->cand_from = srel;
  // host copy of the block table (Pos mapping, segments)
  static_assert(sizeof(sbh_block) == 32, "k_pack_blocks writes 32-byte sbh_block records");
  sh->hb.resize(nc + 1);  // (+ the trailer k_pack_blocks leaves after the table)
  if (nc) {
    HIPCHK(ctx, sh->blkpack.ensure(4 * nc + 4));
    // the linear chain first (every candidate from the start on is chained: no pointer jumping);
    // its flag comes back with the table, and a chain that is not linear is rebuilt by jumping
    for (int pass = chain_jump_only() ? 1 : 0; pass < 2; ++pass) {
      HIPCHK(ctx, build_chain(sh->comp.p, n, sh->cand.p, nc, rel, sh->J0.p, sh->J1.p, sh->on.p, sh->v.p, sh->rank.p,
                              sh->tmp.p, sh->dev_blocks(), sh->usz.p, next18_dev,
                              reinterpret_cast<uint64_t *>(sh->ctr.p + CTR_NEXT18 + 3),
                              pass == 0, st));
      // flat offsets over all nc entries (usz is zero past the chain); the chain length comes
      // back with the block table, so the table is packed and copied for all nc candidates and
      // cut after
      HIPCHK(ctx, scan_exclusive_u64(sh->usz.p, sh->b_ustart.p, nc, sh->tmp.p, st));
      // the table with a 32-byte trailer (hb[nc]): the chain length, then the next18 words (+ the
      // not-linear flag and the empty-block count) -- one copy into hb's page-locked storage
      HIPCHK(ctx, launch_pack_blocks(sh->dev_blocks(), nc, sh->file_off, sh->blkpack.p, st, sh->rank.p, sh->v.p,
                                     reinterpret_cast<const uint64_t *>(next18_dev)));
      HIPCHK(ctx, hipMemcpyAsync(sh->hb.data(), sh->blkpack.p, (nc + 1) * 32, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      std::memcpy(nx, reinterpret_cast<const uint64_t *>(sh->hb.data() + nc) + 1, 24);
      if (pass == 1 || !nx[NEXT18_NONLIN]) break;
    }
    nchain = *reinterpret_cast<const uint64_t *>(sh->hb.data() + nc);
  }
  sh->hb.resize(nchain);
  // stream end: a truncated last block is not part of the resident stream
  sh->open_last = !sh->at_eof;
  sh->broken_end = false;
  if (!sh->hb.empty() && (sh->hb.back().flags & SBH_BLOCK_TRUNCATED)) {
    sh->hb.pop_back();
    --nchain;
  } else if (!sh->hb.empty()) {
    const sbh_block &l = sh->hb.back();
    const uint64_t q = l.start - sh->file_off + l.csize;
    if (q + 18 <= n) {  // the next header does not parse: HeaderParseException if read
      if (sbh_header_make(nx, 18, nullptr, nullptr) != SBH_OK) {
        sh->broken_end = true;
        sh->open_last = false;
      }
    }
  }
  // segments: each empty block ends one (the table is walked only when the chain has any: a
  // walk over a 1 GB shard's 46 k blocks took ~85 us of host time per step); the flat end is
  // that of the last block with bytes
  uint64_t total = 0;
  sh->seg_end.clear();
  const uint32_t nempty = nc ? *reinterpret_cast<const uint32_t *>(nx + NEXT18_NEMPTY) : 0u;
  if (nempty)
    for (const sbh_block &b : sh->hb)
      if (b.flags & SBH_BLOCK_EMPTY) sh->seg_end.push_back(b.ustart);
  for (size_t i = sh->hb.size(); i-- > 0;) {
    const sbh_block &b = sh->hb[i];
    if (!(b.flags & SBH_BLOCK_EMPTY) && b.usize <= 65536) {
      total = b.ustart + b.usize;
      break;
    }
  }
  sh->seg_end.push_back(total);
  HIPCHK(ctx, sh->d_seg.ensure(sh->seg_end.size()));
  HIPCHK(ctx, set_words(sh->d_seg.p, sh->seg_end.data(), sh->seg_end.size(), st));
  // (a stream of the shard's own carries that last write to the shard's next call, with no host
  // round trip here; the caller's stream is handed back drained, as after every call)
  if (!sh->own_st) HIPCHK(ctx, hipStreamSynchronize(st));
  sh->nblocks = nchain;
  sh->utotal = total;
  sh->index_start = start;
  sh->indexed = true;
  if (n_blocks) *n_blocks = nchain;
  if (flat_size) *flat_size = total;
  return SBH_OK;
}

int sbh_get_blocks(sbh_shard *sh, uint64_t first, uint64_t count, sbh_block *out) {
  if (!sh || !out) return SBH_E_ARG;
  if (!sh->indexed) return fail(sh->ctx, SBH_E_STATE, "not indexed");
  if (first + count > sh->hb.size()) return SBH_E_ARG;
  std::memcpy(out, sh->hb.data() + first, count * sizeof(sbh_block));
  return SBH_OK;
}

// After the inflate kernels on `st`: the first block whose status is not INF_OK decides the
// error (the reference's exception for that block); 8 bytes come back, not every status.
// `extra`/`extra_dst`/`extra_n` ride along in the same round trip.
// whole_ctr: the caller set ctr[0, CTR_RUN_WORDS) from the run template (fb = ~0 included), and
// those words all come back to h_ctr in one copy (the eager counters, the step tail's answers)
static int inflate_status(sbh_shard *sh, hipStream_t st, uint64_t *bad_block, const void *extra = nullptr,
                          void *extra_dst = nullptr, size_t extra_n = 0, bool whole_ctr = false) {
  sbh_ctx *ctx = sh->ctx;
  unsigned long long *fb = sh->ctr.p + ctr::FIRST_BAD;
  HIPCHK(ctx, launch_first_bad(sh->b_status.p, sh->nblocks, fb, st, !whole_ctr));
  if (whole_ctr) {
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr, sh->ctr.p, CTR_RUN_WORDS * 8, hipMemcpyDeviceToHost, st));
  } else {
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::FIRST_BAD, fb, 8, hipMemcpyDeviceToHost, st));
    if (extra_n) HIPCHK(ctx, hipMemcpyAsync(extra_dst, extra, extra_n, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(ctx, hipStreamSynchronize(st));
  const uint64_t i = sh->h_ctr[ctr::FIRST_BAD];
  if (i == ~0ull) return SBH_OK;
  uint32_t *hs = reinterpret_cast<uint32_t *>(sh->h_ctr + ctr::H_BAD_STATUS);
  HIPCHK(ctx, hipMemcpyAsync(hs, sh->b_status.p + i, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (bad_block) *bad_block = i;
  const sbh_block &b = sh->hb[i];
  if (*hs == INF_SIZE)
    return fail_with(ctx, SBH_E_INFLATE_SIZE, {(int64_t)b.start, b.usize},
                     "Expected %u decompressed bytes (block %llu)", b.usize, (unsigned long long)b.start);
  if (*hs == INF_BAD_ISIZE) return fail(ctx, SBH_E_BAD_ISIZE, "block %llu: ISIZE %u", (unsigned long long)b.start, b.usize);
  return fail_with(ctx, SBH_E_INFLATE_DATA, {(int64_t)b.start}, "block %llu: invalid deflate data",
                   (unsigned long long)b.start);
}

static hipError_t zero_u_pad(sbh_shard *sh, hipStream_t st) {
  if (sh->u_pad_clean == sh->utotal && sh->u_pad_cap == sh->U.cap) return hipSuccess;
  const hipError_t e = hipMemsetAsync(sh->U.p + sh->utotal, 0, sh->pad, st);
  if (e == hipSuccess) {
    sh->u_pad_clean = sh->utotal;
    sh->u_pad_cap = sh->U.cap;
  }
  return e;
}

static DevBlocks blocks_from(DevBlocks d, uint64_t b) {
  return DevBlocks{d.cstart + b, d.csize + b, d.hsize + b, d.usize + b, d.ustart + b, d.flags + b, d.status + b, d.ntok + b};
}

// Token buffer between k_huff and k_lz: 4 B per flat byte of the blocks inflated at once.  A
// shard whose flat bytes exceed the budget (SBH_TOK_BUDGET bytes, default 16 GiB) is inflated in
// consecutive batches of blocks that reuse one buffer, so HBM holds the compressed and flat
// bytes plus a bounded token buffer whatever the shard size.
static uint64_t tok_cap_flat() { return env_uint("SBH_TOK_BUDGET", 16ull << 30) / 4; }

struct TokPlan {
  std::vector<std::pair<uint64_t, uint64_t>> batches;  // blocks [b0, b1)
  bool reuse = false;                                  // batches share tok (base = ustart of b0)
  uint64_t tok_len = 0;                                // tok entries to allocate
};

// Blocks [0, nblocks) in batches of at most max_blocks blocks and (when the whole shard does
// not fit the token budget) at most the budget's flat bytes each (one block at least).
static TokPlan tok_plan(const sbh_shard *sh, uint64_t max_blocks) {
  TokPlan P;
  const uint64_t nb = sh->nblocks, cap = tok_cap_flat();
  P.reuse = sh->utotal + 64 > cap;
  uint64_t b0 = 0;
  while (b0 < nb) {
    const uint64_t u0 = sh->hb[b0].ustart;
    // (no block walk unless the budget binds; max_blocks may be ~0)
    uint64_t b1 = max_blocks >= nb - b0 ? nb : b0 + std::max<uint64_t>(max_blocks, 1);
    if (P.reuse) {
      b1 = b0 + 1;
      while (b1 < nb && b1 - b0 < max_blocks && sh->hb[b1].ustart + sh->hb[b1].usize - u0 <= cap) ++b1;
    }
    P.batches.emplace_back(b0, b1);
    const uint64_t ext = sh->hb[b1 - 1].ustart + sh->hb[b1 - 1].usize - u0;
    P.tok_len = std::max(P.tok_len, ext);
    b0 = b1;
  }
  if (P.batches.empty()) P.batches.emplace_back(0, 0);  // (an empty shard: one empty batch)
  if (!P.reuse) P.tok_len = sh->utotal;
  P.tok_len += 64;
  return P;
}

int sbh_inflate(sbh_shard *sh, uint64_t *bad_block) {
  if (!sh) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  if (!sh->indexed) return fail(ctx, SBH_E_STATE, "inflate before index");
  int rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  HIPCHK(ctx, sh->U.ensure(sh->utotal + sh->pad));
  const TokPlan P = tok_plan(sh, ~0ull);
  HIPCHK(ctx, sh->tok.ensure(P.tok_len));
  HIPCHK(ctx, zero_u_pad(sh, st));
  mark(sh, 2);
  for (const auto &bt : P.batches) {  // (one stream: a batch's k_lz finishes before the next k_huff)
    const DevBlocks d = blocks_from(sh->dev_blocks(), bt.first);
    const uint64_t base = P.reuse ? sh->hb[bt.first].ustart : 0;
    HIPCHK(ctx, launch_huff(sh->comp.p, d, bt.second - bt.first, sh->tok.p, base, st));
    HIPCHK(ctx, launch_lz(sh->comp.p, d, bt.second - bt.first, sh->tok.p, base, sh->U.p, st));
  }
  mark(sh, 3);
  rc = inflate_status(sh, st, bad_block);
  if (rc) return rc;
  sh->inflated = true;
  sh->bits_valid = sh->chain_ok = sh->cm_valid = false;
  return SBH_OK;
}

// BGZF footer CRC32 of every inflated block vs its bytes in U (crc.hip): the full-size
// bit-exactness check of the inflate (the reference itself never checks CRC32).
int sbh_verify_crc(sbh_shard *sh, uint64_t *n_bad, uint64_t *first_bad) {
  if (!sh || !n_bad) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  if (!sh->inflated) return fail(ctx, SBH_E_STATE, "verify_crc before inflate");
  int rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  unsigned long long *nbad = sh->ctr.p + ctr::CRC_BAD_N, *fbad = sh->ctr.p + ctr::CRC_FIRST_BAD;
  HIPCHK(ctx, hipMemsetAsync(nbad, 0, 8, st));
  HIPCHK(ctx, hipMemsetAsync(fbad, 0xff, 8, st));
  HIPCHK(ctx, launch_block_crc(sh->comp.p, sh->dev_blocks(), sh->nblocks, sh->U.p, nbad, fbad, st));
  // (CRC_BAD_N and CRC_FIRST_BAD)
  HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::CRC_BAD_N, nbad, 2 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  *n_bad = sh->h_ctr[ctr::CRC_BAD_N];
  if (first_bad) *first_bad = sh->h_ctr[ctr::CRC_BAD_N] ? sh->hb[sh->h_ctr[ctr::CRC_FIRST_BAD]].start : 0;
  return SBH_OK;
}

// Which decoder produced each block's tokens (a diagnostic).  Nothing on the inflate path records
// it (a mark stored by k_huff_serial measured 0.35 % of config B's step), so it is derived again:
// the lane-parallel stage runs once more over the shard (the same kernels over the same bytes: the
// same decisions), the statuses it leaves say which blocks it hands to the serial decoder and the
// token counts which are stored copies, and the serial stage then puts status and ntok back as
// sbh_inflate left them.  The flat bytes are not touched.
int sbh_inflate_paths(sbh_shard *sh, uint64_t first, uint64_t count, uint8_t *out) {
  if (!sh || (!out && count)) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  if (!sh->inflated) return fail(ctx, SBH_E_STATE, "inflate_paths before inflate");
  if (first > sh->nblocks || count > sh->nblocks - first) return SBH_E_ARG;
  if (!count) return SBH_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  const TokPlan P = tok_plan(sh, ~0ull);
  HIPCHK(ctx, sh->tok.ensure(P.tok_len));
  std::vector<uint32_t> h(2 * sh->nblocks);
  uint32_t *hst = h.data(), *hnt = h.data() + sh->nblocks;
  for (const auto &bt : P.batches) {  // (a batch's statuses are read before the next reuses the tokens)
    const DevBlocks d = blocks_from(sh->dev_blocks(), bt.first);
    const uint64_t base = P.reuse ? sh->hb[bt.first].ustart : 0, nb = bt.second - bt.first;
    if (!nb) continue;
    HIPCHK(ctx, launch_huff(sh->comp.p, d, nb, sh->tok.p, base, st, HUFF_FAST));
    HIPCHK(ctx, hipMemcpyAsync(hst + bt.first, d.status, nb * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(hnt + bt.first, d.ntok, nb * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, launch_huff(sh->comp.p, d, nb, sh->tok.p, base, st, HUFF_SERIAL));
  }
  HIPCHK(ctx, hipStreamSynchronize(st));
  for (uint64_t i = 0; i < count; ++i) {
    const uint64_t b = first + i;
    out[i] = hst[b] == INF_SERIAL ? SBH_PATH_SERIAL : hnt[b] == NTOK_STORED ? SBH_PATH_STORED : SBH_PATH_PARALLEL;
  }
  return SBH_OK;
}

int sbh_read_flat(sbh_shard *sh, uint64_t flat, uint64_t n, uint8_t *out) {
  if (!sh || (!out && n)) return SBH_E_ARG;
  if (!sh->inflated) return fail(sh->ctx, SBH_E_STATE, "not inflated");
  if (flat + n > sh->utotal) return SBH_E_ARG;
  int rc = set_device(sh->ctx);
  if (rc) return rc;
  HIPCHK(sh->ctx, hipMemcpyAsync(out, sh->U.p + flat, n, hipMemcpyDeviceToHost, sh->st));
  HIPCHK(sh->ctx, hipStreamSynchronize(sh->st));
  return SBH_OK;
}

const void *sbh_flat_device_ptr(sbh_shard *sh) { return sh ? sh->U.p : nullptr; }

}  // extern "C"

int64_t sbh::block_index_of(const sbh_shard *sh, uint64_t file_pos) {
  auto it = std::lower_bound(sh->hb.begin(), sh->hb.end(), file_pos,
                             [](const sbh_block &b, uint64_t v) { return b.start < v; });
  if (it == sh->hb.end() || it->start != file_pos) return -1;
  return it - sh->hb.begin();
}

extern "C" {

int sbh_flat_of(sbh_shard *sh, uint64_t block_pos, uint32_t offset, uint64_t *flat) {
  if (!sh || !flat) return SBH_E_ARG;
  if (!sh->indexed) return fail(sh->ctx, SBH_E_STATE, "not indexed");
  const int64_t i = block_index_of(sh, block_pos);
  if (i < 0) return fail(sh->ctx, SBH_E_NOT_FOUND, "%llu is not an indexed block start", (unsigned long long)block_pos);
  *flat = sh->hb[i].ustart + offset;
  return SBH_OK;
}

int sbh_pos_of(sbh_shard *sh, uint64_t flat, uint64_t *block_pos, uint32_t *offset) {
  if (!sh || !block_pos || !offset) return SBH_E_ARG;
  if (!sh->indexed) return fail(sh->ctx, SBH_E_STATE, "not indexed");
  // last block with ustart <= flat and flat < ustart + usize (skips empty blocks)
  auto it = std::upper_bound(sh->hb.begin(), sh->hb.end(), flat,
                             [](uint64_t v, const sbh_block &b) { return v < b.ustart; });
  int64_t i = (it - sh->hb.begin()) - 1;
  while (i >= 0 && (uint64_t)i < sh->hb.size() && sh->hb[i].ustart + sh->hb[i].usize <= flat) ++i;
  if (i < 0 || (uint64_t)i >= sh->hb.size()) {
    // one past the last byte: Pos(next block, 0)
    if (!sh->hb.empty() && flat == sh->utotal) {
      const sbh_block &l = sh->hb.back();
      *block_pos = l.start + l.csize;
      *offset = 0;
      return SBH_OK;
    }
    return fail(sh->ctx, SBH_E_NOT_FOUND, "flat %llu outside the indexed stream", (unsigned long long)flat);
  }
  // skip zero-size blocks sharing this ustart
  while ((uint64_t)i < sh->hb.size() && (sh->hb[i].usize == 0 || (sh->hb[i].flags & SBH_BLOCK_EMPTY))) ++i;
  if ((uint64_t)i >= sh->hb.size()) return SBH_E_NOT_FOUND;
  *block_pos = sh->hb[i].start;
  *offset = (uint32_t)(flat - sh->hb[i].ustart);
  return SBH_OK;
}

int sbh_flat_bound(sbh_shard *sh, uint64_t file_off, uint64_t *flat) {
  if (!sh || !flat) return SBH_E_ARG;
  if (!sh->indexed) return fail(sh->ctx, SBH_E_STATE, "not indexed");
  auto it = std::lower_bound(sh->hb.begin(), sh->hb.end(), file_off,
                             [](const sbh_block &b, uint64_t v) { return b.start < v; });
  *flat = it == sh->hb.end() ? sh->utotal : it->ustart;
  return SBH_OK;
}

// Inflate + eager check of flat [0, E) as one pipeline over batches of blocks, on three
// streams: k_huff of batch i+1 runs beside k_lz of batch i and beside the eager tiles
// whose staged windows batch i completed (k_huff is latency-bound on LDS and VALU, k_lz on
// barriers, k_eager on its chain walks: side by side they fill each other's idle issue
// slots).  An eager position whose exact check needs bytes past the inflated frontier is
// deferred and re-checked at the end.  Same results as sbh_inflate + sbh_check_eager.
static constexpr uint64_t PIPE_MAX_BATCHES = 16;
static constexpr uint64_t DEFER_CAP = 1 << 20;

// Batches of at least SBH_PIPE_MIN_BLOCKS blocks (tests: small batches exercise many
// frontiers on small inputs).  Default: one batch.  Measured on MI355X (1 GiB shard,
// this design): 1 batch 34.7 ms/step, 3 batches 35.2, 16 batches 38.2 -- side by side
// the three kernels contend for the same LDS and issue slots, and k_lz (two 80 KiB
// workgroups per CU) loses the most; the pipeline stays for inputs where it pays.
static uint64_t pipe_min_blocks() { return env_uint("SBH_PIPE_MIN_BLOCKS", ~0ull); }

static hipEvent_t pev(sbh_shard *sh, size_t i) {
  while (sh->pev.size() <= i) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    sh->pev.push_back(e);
  }
  return sh->pev[i];
}

// pre_sync (optional): more work enqueued on the main stream after the eager kernels and before
// the one host round trip that brings back the inflate status and the eager counters (its
// results are only meaningful when this returns SBH_OK without a fallback)
static int run_pipelined(sbh_shard *sh, uint64_t E, int32_t rtc, uint64_t *n_true,
                         const std::function<hipError_t(hipStream_t)> &pre_sync = nullptr) {
  sbh_ctx *ctx = sh->ctx;
  if (!sh->indexed) return fail(ctx, SBH_E_STATE, "inflate before index");
  if (sh->nctg < 0) return fail(ctx, SBH_E_STATE, "contig lengths not set");
  if (rtc < 0 || rtc > 1023) return fail(ctx, SBH_E_ARG, "readsToCheck must be in [0, 1023]");
  hipStream_t sa = sh->st;
  HIPCHK(ctx, sh->U.ensure(sh->utotal + sh->pad));
  const uint64_t nb = sh->nblocks;
  const uint64_t npipe = std::max<uint64_t>(1, std::min<uint64_t>(PIPE_MAX_BATCHES, nb / pipe_min_blocks()));
  const TokPlan P = tok_plan(sh, (nb + npipe - 1) / std::max<uint64_t>(npipe, 1));
  // one batch (the default) of a resident shard: every launch on the shard's stream, no
  // cross-stream event waits (each cost the step ~15 us of idle device between the stages)
  hipStream_t sl = sa, se = sa;
  if (P.batches.size() > 1) {
    if (!sh->s_lz) HIPCHK(ctx, hipStreamCreateWithFlags(&sh->s_lz, hipStreamNonBlocking));
    if (!sh->s_eg) HIPCHK(ctx, hipStreamCreateWithFlags(&sh->s_eg, hipStreamNonBlocking));
    sl = sh->s_lz;
    se = sh->s_eg;
  }
  // s waits for e, recorded on `on` (nothing to wait for on the same stream)
  auto wait = [](hipStream_t s, hipEvent_t e, hipStream_t on) { return s == on ? hipSuccess : hipStreamWaitEvent(s, e, 0); };
  HIPCHK(ctx, sh->tok.ensure(P.tok_len));
  HIPCHK(ctx, sh->bits.ensure((E + 31) / 32 + 1));
  HIPCHK(ctx, sh->defer.ensure(DEFER_CAP));
  HIPCHK(ctx, sh->xq.ensure(2 * XQ_CAP_MAX));
  HIPCHK(ctx, zero_u_pad(sh, sa));
  unsigned long long *c = sh->ctr.p;
  {
    // ctr[0, CTR_RUN_WORDS) in one copy: k_eager's counters (the first need-halo position = ~0),
    // the step tail's FindRecordStart best = ~0 and chain-proof counters = {0, ~0, 0, ~0},
    // k_first_bad's = ~0; the rest (per-call regions) zero
    unsigned long long *tpl = sh->h_ctr + ctr::H_RUN_TPL;  // pinned
    std::memset(tpl, 0, CTR_RUN_WORDS * 8);
    tpl[ctr::EAGER_HALO_FIRST] = tpl[ctr::FRS_BEST] = tpl[ctr::PROOF_FIRST_ANOM] = tpl[ctr::PROOF_EXIT] =
        tpl[ctr::FIRST_BAD] = ~0ull;
    HIPCHK(ctx, set_words(reinterpret_cast<uint64_t *>(c), reinterpret_cast<const uint64_t *>(tpl), CTR_RUN_WORDS, sa));
  }
  sh->inflated = sh->bits_valid = sh->chain_ok = sh->cm_valid = false;
  sh->pipe_fallback = false;
  const uint64_t nbat = P.batches.size();
  // events: per batch [huff start, huff end, lz start, lz end, eager start, eager end]
  for (size_t i = 0; i < 6 * nbat + 4; ++i)
    if (!pev(sh, i)) return fail(ctx, SBH_E_HIP, "hipEventCreate failed");
  hipEvent_t *ev = sh->pev.data();
  HIPCHK(ctx, hipEventRecord(ev[6 * nbat], sa));  // setup done: the other streams start after it
  HIPCHK(ctx, wait(sl, ev[6 * nbat], sa));
  HIPCHK(ctx, wait(se, ev[6 * nbat], sa));
  const DevBlocks all = sh->dev_blocks();
  uint64_t e_done = 0;
  std::vector<int> eager_launched(nbat, 0);
  for (uint64_t i = 0; i < nbat; ++i) {
    const uint64_t b0 = P.batches[i].first, b1 = P.batches[i].second;
    hipEvent_t *e = ev + 6 * i;
    const DevBlocks d = blocks_from(all, b0);
    const uint64_t base = P.reuse ? sh->hb[b0].ustart : 0;
    // a reused token buffer: this batch's k_huff overwrites what the previous k_lz reads
    if (P.reuse && i) HIPCHK(ctx, wait(sa, ev[6 * (i - 1) + 3], sl));
    HIPCHK(ctx, hipEventRecord(e[0], sa));
    HIPCHK(ctx, launch_huff(sh->comp.p, d, b1 - b0, sh->tok.p, base, sa));
    HIPCHK(ctx, hipEventRecord(e[1], sa));
    HIPCHK(ctx, wait(sl, e[1], sa));
    HIPCHK(ctx, hipEventRecord(e[2], sl));
    HIPCHK(ctx, launch_lz(sh->comp.p, d, b1 - b0, sh->tok.p, base, sh->U.p, sl));
    HIPCHK(ctx, hipEventRecord(e[3], sl));
    // eager tiles whose staged windows lie below the inflated frontier
    const bool last = i + 1 == nbat;
    const uint64_t front = last ? ~0ull : sh->hb[b1].ustart;
    uint64_t hi = E;
    if (!last) {
      hi = front + EAGER_TILE >= EAGER_REACH ? (front + EAGER_TILE - EAGER_REACH) / EAGER_TILE * EAGER_TILE : 0;
      hi = std::min(hi, E);
    }
    if (hi > e_done) {
      HIPCHK(ctx, wait(se, e[3], sl));
      HIPCHK(ctx, hipEventRecord(e[4], se));
      HIPCHK(ctx, launch_eager(sh->U.p, sh->utotal + sh->pad, e_done, hi, sh->d_seg.p, (uint32_t)sh->seg_end.size(),
                               sh->open_last ? 1 : 0, sh->ctg.p, sh->nctg, rtc, sh->bits.p + e_done / 32, c, se,
                               front, sh->defer.p, DEFER_CAP, sh->xq.p, XQ_CAP_MAX));
      HIPCHK(ctx, hipEventRecord(e[5], se));
      eager_launched[i] = 1;
      e_done = hi;
    }
  }
  HIPCHK(ctx, wait(se, ev[6 * (nbat - 1) + 3], sl));
  HIPCHK(ctx, launch_eager_defer(sh->U.p, 0, sh->d_seg.p, (uint32_t)sh->seg_end.size(), sh->open_last ? 1 : 0,
                                 sh->ctg.p, sh->nctg, rtc, sh->bits.p, c, sh->defer.p, DEFER_CAP, se));
  HIPCHK(ctx, hipEventRecord(ev[6 * nbat + 2], se));
  HIPCHK(ctx, launch_eager_xq(sh->U.p, 0, sh->d_seg.p, (uint32_t)sh->seg_end.size(), sh->open_last ? 1 : 0,
                              sh->ctg.p, sh->nctg, rtc, sh->bits.p, c, sh->xq.p, XQ_CAP_MAX, se));
  HIPCHK(ctx, hipEventRecord(ev[6 * nbat + 3], se));
  HIPCHK(ctx, hipEventRecord(ev[6 * nbat + 1], se));
  HIPCHK(ctx, wait(sa, ev[6 * nbat + 1], se));
  if (pre_sync) HIPCHK(ctx, pre_sync(sa));
  {
    const int rs = inflate_status(sh, sa, nullptr, nullptr, nullptr, 0, true);
    if (rs) return rs;
  }
  sh->inflated = true;
  if (sh->timing) {
    double hs = 0, ls = 0, es = 0;
    for (uint64_t i = 0; i < nbat; ++i) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ev[6 * i], ev[6 * i + 1]) == hipSuccess) hs += ms;
      if (hipEventElapsedTime(&ms, ev[6 * i + 2], ev[6 * i + 3]) == hipSuccess) ls += ms;
      if (eager_launched[i] && hipEventElapsedTime(&ms, ev[6 * i + 4], ev[6 * i + 5]) == hipSuccess) es += ms;
    }
    sh->pipe_ms[0] = hs;
    sh->pipe_ms[1] = ls;
    float xs = 0;
    if (hipEventElapsedTime(&xs, ev[6 * nbat + 2], ev[6 * nbat + 3]) == hipSuccess) es += xs;  // k_eager_xq
    sh->pipe_ms[2] = es;
  }
  if (env_flag("SBH_XQ_DEBUG"))
    fprintf(stderr, "[sbh] eager: deferred %llu, long-record queue %llu (%llu past the pre-test)\n",
            sh->h_ctr[ctr::EAGER_DEFER_N], sh->h_ctr[ctr::EAGER_XQ_N], sh->h_ctr[ctr::EAGER_XQ_LIVE]);
  if (sh->h_ctr[ctr::EAGER_DEFER_N] > DEFER_CAP) {  // deferral overflow: plain pass
    sh->pipe_fallback = true;
    return eager_range(sh, 0, E, rtc, n_true);
  }
  sh->bits_valid = true;
  sh->bits_begin = 0;
  sh->bits_end = E;
  sh->bits_rtc = rtc;
  if (n_true) *n_true = sh->h_ctr[ctr::EAGER_TRUE];
  if (sh->h_ctr[ctr::EAGER_HALO_N]) {
    sh->bits_valid = false;
    return fail(ctx, SBH_E_NEED_HALO, "%llu positions (first %llu) need bytes past the shard",
                sh->h_ctr[ctr::EAGER_HALO_N], sh->h_ctr[ctr::EAGER_HALO_FIRST]);
  }
  return SBH_OK;
}

int sbh_run_shard(sbh_shard *sh, uint64_t index_start, uint64_t own_end_file, int32_t rtc, int32_t mrs,
                  sbh_shard_result *res) {
  if (!sh || !res) return SBH_E_ARG;
  std::memset(res, 0, sizeof *res);
  sbh_ctx *ctx = sh->ctx;
  (void)hipGetLastError();
  sh->timing = true;
  mark(sh, 0);
  int rc = sbh_index(sh, index_start, &res->n_blocks, nullptr);
  mark(sh, 1);
  if (rc) { sh->timing = false; return res->status = rc; }
  uint64_t E = 0;
  (void)sbh_flat_bound(sh, own_end_file, &E);
  if (!sh->at_eof && E == sh->utotal) {
    sh->timing = false;
    return res->status = fail(ctx, SBH_E_NEED_HALO, "no halo past %llu", (unsigned long long)own_end_file);
  }
  // the blocks starting before own_end_file (the chain is contiguous: each block starts where
  // the one before it ends, so their bytes are one span)
  const uint64_t owned_blocks = (uint64_t)(std::lower_bound(sh->hb.begin(), sh->hb.end(), own_end_file,
                                                           [](const sbh_block &b, uint64_t v) { return b.start < v; }) -
                                           sh->hb.begin());
  const uint64_t cbytes =
      owned_blocks ? sh->hb[owned_blocks - 1].start + sh->hb[owned_blocks - 1].csize - sh->hb[0].start : 0;
  res->n_blocks = owned_blocks;
  res->comp_bytes = cbytes;
  res->flat_bytes = E;
  mark(sh, 2);
  // The step's tail rides in the inflate-status round trip: FindRecordStart from flat 0 (the
  // first set bit of the verified bitmap below min(segment end, maxReadSize, E)) and the chain
  // proof from that record, which k_verify_chain_w reads from the device.  The answers are taken
  // when the record lies in the first segment and the bitmap is exactly the chain; anything else
  // (no bit found, an anomaly, a fallback inside run_pipelined) goes the long way below, as
  // sbh_find_record_start and count_records_impl would on their own.
  const uint64_t total0 = sh->seg_end.empty() ? 0 : sh->seg_end[0];
  const uint64_t hi0 = std::min(std::min<uint64_t>(total0, (uint64_t)std::max(mrs, 0)), E);
  const uint64_t E0 = std::min(E, total0);
  unsigned long long *tbest = sh->ctr.p + ctr::FRS_BEST, *c = sh->ctr.p;
  bool tail = rtc >= 0 && hi0 > 0;
  if (tail && sh->cc.ensure((E + 31) / 32 / VC_CHUNK + 2) != hipSuccess) tail = false;
  // (tbest and the proof counters start as run_pipelined's counter template sets them, and come
  // back to the same words of h_ctr with its one status copy)
  auto tail_launch = [&](hipStream_t s) -> hipError_t {
    hipError_t e = launch_first_set(sh->bits.p, 0, 0, hi0, tbest, s);
    if (e == hipSuccess)
      e = launch_verify_chain_count(sh->U.p, sh->bits.p, 0, E, 0, E0, total0, c + ctr::PROOF_ANOM,
                                    c + ctr::PROOF_FIRST_ANOM, c + ctr::PROOF_EXIT, c + ctr::PROOF_SET, s, tbest,
                                    sh->cc.p);
    return e;
  };
  rc = tail ? run_pipelined(sh, E, rtc, &res->n_true, tail_launch) : run_pipelined(sh, E, rtc, &res->n_true);
  mark(sh, 5);
  if (rc) { sh->timing = false; return res->status = rc; }
  // (a deferral overflow re-ran the eager pass inside run_pipelined: the bitmap is new)
  tail = tail && sh->bits_valid && sh->bits_begin == 0 && sh->bits_end == E && sh->bits_rtc == rtc &&
         !sh->pipe_fallback;
  uint64_t first = 0;
  int32_t delta = 0;
  sh->run_first = ~0ull;
  if (tail && sh->h_ctr[ctr::FRS_BEST] != ~0ull) {
    first = sh->h_ctr[ctr::FRS_BEST];
    sh->run_first = first;
    rc = SBH_OK;
    // (count_records_impl's proof, done)
    if (first < E0 && sh->h_ctr[ctr::PROOF_ANOM] == 0 && sh->h_ctr[ctr::PROOF_EXIT] != ~0ull) {
      sh->cm_valid = false;
      sh->chain_ok = true;
      sh->cc_ok = true;
      sh->chain_first = first;
      sh->chain_E = E0;
      res->count = sh->h_ctr[ctr::PROOF_SET];
      res->anomalies = 0;
      res->exit_flat = sh->h_ctr[ctr::PROOF_EXIT];
    } else {
      // (the tail's proof covered [first, E0) of this bitmap: its counters are reused when first
      // lies in the first segment, which is the range count_records_impl proves)
      rc = count_records_impl(sh, first, E, &res->count, &res->anomalies, &res->exit_flat, first < E0);
    }
    uint64_t bp = 0;
    uint32_t off = 0;
    if (!rc && sbh_pos_of(sh, first, &bp, &off) == SBH_OK) res->first_vpos = (bp << 16) | off;
  } else {
    rc = sbh_find_record_start(sh, 0, rtc, mrs, &first, &delta);
    if (rc == SBH_E_NO_READ_FOUND) {
      res->count = 0;
      rc = SBH_OK;
    } else if (rc == SBH_OK) {
      sh->run_first = first;
      rc = count_records_impl(sh, first, E, &res->count, &res->anomalies, &res->exit_flat);
      uint64_t bp = 0;
      uint32_t off = 0;
      if (!rc && sbh_pos_of(sh, first, &bp, &off) == SBH_OK) res->first_vpos = (bp << 16) | off;
    }
  }
  if (res->count == 0) res->exit_flat = E;
  mark(sh, 6);
  sh->timing = false;
  if (sh->ev_ok) {
    (void)hipEventSynchronize(sh->ev[6]);
    // [index, inflate + eager pipeline, eager (sum of launches), split/count, k_huff, k_lz]
    const int from[2] = {0, 5}, to[2] = {1, 6};
    for (int i = 0; i < 2; ++i) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, sh->ev[from[i]], sh->ev[to[i]]);
      sh->stage_ms[i == 0 ? 0 : 3] = ms;
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, sh->ev[2], sh->ev[5]);
    sh->stage_ms[1] = ms;
    sh->stage_ms[2] = sh->pipe_ms[2];
    sh->stage_ms[4] = sh->pipe_ms[0];
    sh->stage_ms[5] = sh->pipe_ms[1];
  }
  return res->status = rc;
}

int sbh_stage_times(sbh_shard *sh, double *ms, int32_t cap) {
  if (!sh || !ms || cap < 0) return 0;
  int n = cap < 6 ? cap : 6;
  for (int i = 0; i < n; ++i) ms[i] = sh->stage_ms[i];
  return n;
}

// A shard larger than the HBM budget, streamed through it (Stream.scala:80-122 and
// SplitRDD.scala:33-52 bound the reference's memory the same way: per split, a bounded
// block cache).  The owned range [index_start, own_end_file) is cut into windows of about
// `window` compressed bytes; window w owns the blocks starting in [lo_w, hi_w) and loads
// [lo_w, hi_w + halo).  While window w runs the whole per-shard path (sbh_run_shard), the
// bytes of window w+1 move host -> HBM on a copy stream into the other of two buffers, so
// HBM holds two windows of compressed bytes and one window's flat bytes, tokens and bitmap,
// whatever the shard size.  Window w+1 indexes from the first block at/after hi_w (known
// from window w's block table).  Consecutive non-empty windows stitch like ranks (SURVEY
// 8e): the chain leaving window w must enter window w+1 at its first record, else window
// w+1 is re-walked from that exit.  A result that needs bytes past a window's halo grows
// the halo x4 and redoes the window.
int sbh_run_stream(sbh_ctx *ctx, const void *host, uint64_t n, uint64_t file_offset, uint64_t file_size,
                   uint64_t index_start, uint64_t own_end_file, uint64_t window, uint64_t halo, const int32_t *contigs,
                   int32_t n_contigs, int32_t rtc, int32_t mrs, uint8_t *out_bits, uint64_t out_bits_cap,
                   sbh_stream_result *res) {
  sbh_stream_opts o{};
  o.window = window;
  o.halo = halo;
  o.reads_to_check = rtc;
  o.max_read_size = mrs;
  o.bgzf_blocks_to_check = 5;
  o.out_bits = out_bits;
  o.out_bits_cap = out_bits_cap;
  return sbh_run_stream2(ctx, host, n, file_offset, file_size, index_start, own_end_file, contigs, n_contigs, &o, res);
}

// CRC32 of the first nb blocks of the table (a window's owned blocks) against their footers.
static int verify_crc_prefix(sbh_shard *sh, uint64_t nb, uint64_t *n_bad, uint64_t *first_bad, float *ms) {
  sbh_ctx *ctx = sh->ctx;
  hipStream_t st = sh->st;
  unsigned long long *nbad = sh->ctr.p + ctr::CRC_BAD_N, *fbad = sh->ctr.p + ctr::CRC_FIRST_BAD;
  HIPCHK(ctx, hipMemsetAsync(nbad, 0, 8, st));
  HIPCHK(ctx, hipMemsetAsync(fbad, 0xff, 8, st));
  mark(sh, 7);
  HIPCHK(ctx, launch_block_crc(sh->comp.p, sh->dev_blocks(), nb, sh->U.p, nbad, fbad, st));
  mark(sh, 8);
  // (CRC_BAD_N and CRC_FIRST_BAD)
  HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::CRC_BAD_N, nbad, 2 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  *n_bad = sh->h_ctr[ctr::CRC_BAD_N];
  *first_bad = sh->h_ctr[ctr::CRC_BAD_N] ? sh->hb[sh->h_ctr[ctr::CRC_FIRST_BAD]].start : 0;
  *ms = 0.f;
  if (sh->ev_ok) (void)hipEventElapsedTime(ms, sh->ev[7], sh->ev[8]);
  return SBH_OK;
}

int sbh_run_stream2(sbh_ctx *ctx, const void *host, uint64_t n, uint64_t file_offset, uint64_t file_size,
                    uint64_t index_start, uint64_t own_end_file, const int32_t *contigs, int32_t n_contigs,
                    const sbh_stream_opts *opts, sbh_stream_result *res) {
  if (!ctx || !res || !opts || (!host && n) || !opts->window || file_offset + n > file_size ||
      own_end_file > file_offset + n || own_end_file <= file_offset || n_contigs < 0 || (n_contigs && !contigs))
    return SBH_E_ARG;
  const sbh_stream_opts &O = *opts;
  const uint64_t window = O.window;
  uint64_t halo = O.halo;
  const int32_t rtc = O.reads_to_check, mrs = O.max_read_size, kcheck = O.bgzf_blocks_to_check;
  uint8_t *out_bits = O.out_bits;
  const uint64_t out_bits_cap = O.out_bits_cap, ns = O.n_splits;
  std::memset(res, 0, sizeof *res);
  res->first_vpos = res->exit_vpos = ~0ull;
  if (ns) {  // splits: sorted, disjoint, inside the owned range, with their outputs
    if (!O.split_start || !O.split_end || !O.split_first_vpos || !O.split_count || !O.split_status)
      return fail(ctx, SBH_E_ARG, "run_stream2: split arrays missing");
    for (uint64_t i = 0; i < ns; ++i) {
      const uint64_t a = O.split_start[i], e = O.split_end[i];
      if (a < file_offset || a >= own_end_file || e <= a || e > own_end_file || (i + 1 < ns && e > O.split_start[i + 1]))
        return fail(ctx, SBH_E_ARG, "run_stream2: split %llu [%llu, %llu) out of order or outside [%llu, %llu)",
                    (unsigned long long)i, (unsigned long long)a, (unsigned long long)e,
                    (unsigned long long)file_offset, (unsigned long long)own_end_file);
      O.split_first_vpos[i] = O.split_count[i] = 0;
      O.split_status[i] = SBH_OK;
    }
  }
  const auto t_start = std::chrono::steady_clock::now();
  int rc = set_device(ctx);
  if (rc) return res->status = rc;
  const uint8_t *src = static_cast<const uint8_t *>(host);
  hipPointerAttribute_t pa{};
  res->host_pinned = hipPointerGetAttributes(&pa, host) == hipSuccess && pa.type == hipMemoryTypeHost ? 1 : 0;
  (void)hipGetLastError();
  // the window shard, the two window buffers and the copy stream persist in the context (grow-only),
  // so repeated calls allocate nothing; concurrent callers each take their own cache from the pool
  StreamCache *scp = nullptr;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->sc_free.empty()) {
      scp = ctx->sc_free.back();
      ctx->sc_free.pop_back();
    }
  }
  if (!scp) {
    scp = new StreamCache();
    rc = sbh_shard_create(ctx, nullptr, 0, file_offset, file_size, 0, &scp->sh);
    if (rc) {
      delete scp;
      return res->status = rc;
    }
    scp->sh->comp.release();
    hipError_t e = copy_stream_create(&scp->cs);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
      e = hipEventCreate(&scp->done[i]);
      if (e == hipSuccess) e = hipEventCreate(&scp->c0[i]);
    }
    if (e != hipSuccess) {
      delete scp;
      return res->status = fail(ctx, SBH_E_HIP, "run_stream2: %s", hipGetErrorString(e));
    }
  }
  struct Return {  // the cache goes back to the pool on every return path
    sbh_ctx *ctx;
    StreamCache *sc;
    ~Return() {
      std::lock_guard<std::mutex> lk(ctx->mu);
      ctx->sc_free.push_back(sc);
    }
  } give_back{ctx, scp};
  StreamCache &R = *scp;
  struct Detach {  // the window buffers are never the shard's own: detach on every return path
    StreamCache &R;
    ~Detach() {
      if (R.cs) (void)hipStreamSynchronize(R.cs);
      R.sh->comp.unlend();
    }
  } detach{R};
  sbh_shard *sh = R.sh;
  sh->file_size = file_size;
  // (sbh_set_contigs synchronises the shard's stream.  The window copies below run on the cache's
  // copy stream, which no event orders behind the shard's: when that is the caller's stream
  // (sbh_ctx_set_stream) and work on it was still writing `host`, this wait is what puts the first
  // copy behind it -- a reused cache creates no shard, so nothing else would)
  rc = sbh_set_contigs(sh, contigs, n_contigs);
  if (rc) return res->status = rc;
  const uint64_t data_end = file_offset + n, pad = sh->pad;
  // the first window is short: its copy is the only one no kernel overlaps
  const uint64_t first_window = std::max<uint64_t>(std::min<uint64_t>(window, 64ull << 20), window / 8);
  // window ends: the last split start in (lo, lo + window] when splits are given, so a split
  // lies in one window unless it is longer than a window; such a split is cut at lo + window and
  // its chain followed window by window (the straddling split below), so HBM stays bounded
  // whatever the split size (one split per rank included)
  auto win_end = [&](uint64_t lo) {
    const uint64_t want = lo + (lo == file_offset ? first_window : window);
    uint64_t hi = std::min(want, own_end_file);
    if (own_end_file - hi < window / 4) hi = own_end_file;  // no sliver of a last window
    if (ns && hi < own_end_file) {
      const uint64_t *S = O.split_start;
      const uint64_t k = (uint64_t)(std::upper_bound(S, S + ns, hi) - S);  // starts <= hi: [0, k)
      if (k > 0 && S[k - 1] > lo) hi = S[k - 1];
    }
    return hi;
  };
  // the split that runs past its first window: its index, and the htsjdk vpos of the next record
  // of its own chain (from its first record, CanLoadBam.scala:338-355) not yet counted
  int64_t strad = -1;
  uint64_t strad_cur = 0;
  auto load_end = [&](uint64_t hi) { return std::min(hi + halo, data_end); };
  auto size_bufs = [&]() -> hipError_t {  // (enqueue grows a buffer for a longer split-aligned window)
    const uint64_t cap = window + window / 4 + halo + pad;
    for (auto &b : R.buf) {
      hipError_t e = b.ensure(cap);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  };
  auto fit_buf = [&](int b, uint64_t need) -> hipError_t {  // grow buffer b (not in use) to `need` bytes
    hipError_t e = hipStreamSynchronize(R.cs);
    if (e == hipSuccess) e = hipStreamSynchronize(sh->st);
    if (e == hipSuccess) e = R.buf[b].ensure(need);
    return e;
  };
  double h2d_ms = 0;
  bool timed[2] = {false, false};
  auto account = [&](int b) {  // copy time of the last copy into buffer b
    if (!timed[b]) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, R.c0[b], R.done[b]) == hipSuccess) h2d_ms += ms;
    timed[b] = false;
  };
  uint64_t win_len[2] = {0, 0};  // bytes copied into each window buffer
  auto enqueue = [&](int b, uint64_t lo, uint64_t ld) -> hipError_t {
    hipError_t e = hipSuccess;
    if (R.buf[b].cap < ld - lo + pad) {  // an oversized (split-aligned) window
      e = fit_buf(b, ld - lo + pad);
      if (e != hipSuccess) return e;
    }
    // (the copy stream carries the copy alone: the window's zero pad is set on the shard's stream
    // after it waits for the copy -- a fill queued behind the copy on the copy stream would be a
    // kernel waiting on the DMA, and a hardware queue the copy stream shares with a compute
    // stream would hold that stream's kernels behind it)
    e = hipEventRecord(R.c0[b], R.cs);
    if (e == hipSuccess) e = hipMemcpyAsync(R.buf[b].p, src + (lo - file_offset), ld - lo, hipMemcpyHostToDevice, R.cs);
    if (e == hipSuccess) e = hipEventRecord(R.done[b], R.cs);
    win_len[b] = ld - lo;
    timed[b] = e == hipSuccess;
    return e;
  };
  HIPCHK(ctx, size_bufs());
  uint64_t lo = file_offset, hi = win_end(lo), start = index_start;
  int cur = 0;
  HIPCHK(ctx, enqueue(cur, lo, load_end(hi)));
  bool prefetch = true, have_prev = false;
  uint64_t prev_exit = ~0ull, flat_base = 0;
  std::vector<uint32_t> wbits;
  for (;;) {
    const bool more = hi < own_end_file;
    const uint64_t lo2 = hi, hi2 = more ? win_end(lo2) : 0;
    if (prefetch && more) HIPCHK(ctx, enqueue(1 - cur, lo2, load_end(hi2)));
    const uint64_t ld = load_end(hi);
    HIPCHK(ctx, hipStreamWaitEvent(sh->st, R.done[cur], 0));
    HIPCHK(ctx, hipMemsetAsync(R.buf[cur].p + win_len[cur], 0, pad, sh->st));
    sh->comp.lend(R.buf[cur].p, R.buf[cur].cap);
    sh->file_off = lo;
    sh->n = ld - lo;
    sh->at_eof = ld == file_size;
    if (start == ~0ull) {
      rc = sbh_find_block_start(sh, lo, kcheck, &start);  // BGZFBlocksToCheck (bgzf/.../block/package.scala:20)
      if (rc) return res->status = rc;
    }
    sbh_shard_result r{};
    sh->scan_from = lo;  // header candidates from the window's first byte (its first split's FindBlockStart)
    rc = sbh_run_shard(sh, start, hi, rtc, mrs, &r);
    // this window's splits (every one starting in [lo, hi)): the batched per-split path for the
    // ones that end by hi; the last one may run past hi (a split longer than the window)
    uint64_t k0 = 0, k1 = 0, nh = 0;
    double split_ms = 0;
    // the straddling split's progress in this window, committed once the window holds
    int64_t s_idx = strad;
    uint64_t s_cur = strad_cur, s_add = 0, s_first = 0;
    int32_t s_status = SBH_OK;
    bool s_new = false, s_done = false;
    if (!rc && ns) {
      const auto ts0 = std::chrono::steady_clock::now();
      k0 = (uint64_t)(std::lower_bound(O.split_start, O.split_start + ns, lo) - O.split_start);
      k1 = (uint64_t)(std::lower_bound(O.split_start, O.split_start + ns, hi) - O.split_start);
      const bool straddles = k1 > k0 && O.split_end[k1 - 1] > hi;
      const uint64_t kb = straddles ? k1 - 1 : k1;
      if (kb > k0) {
        rc = sbh_split_starts(sh, O.split_start + k0, O.split_end + k0, kb - k0, kcheck, rtc, mrs,
                              O.split_first_vpos + k0, O.split_count + k0, O.split_status + k0, &nh);
        if (!rc)
          for (uint64_t i = k0; i < kb; ++i)
            if (O.split_status[i] == SBH_E_NEED_HALO) rc = SBH_E_NEED_HALO;
      }
      uint64_t E_hi = 0;
      if (!rc) rc = sbh_flat_bound(sh, hi, &E_hi);
      // follow a chain from flat f while its records start before min(Pos(split end, 0), Pos(hi, 0))
      auto follow = [&](uint64_t f, uint64_t split_end) -> int {
        uint64_t E_end = 0, n = 0, x = 0, bp = 0;
        uint32_t off = 0;
        int r = sbh_flat_bound(sh, split_end, &E_end);
        if (!r) r = sbh_chain_from(sh, f, std::min(E_end, E_hi), &n, &x);
        if (!r && x >= sh->utotal && !sh->at_eof) r = SBH_E_NEED_HALO;  // its next record is past the halo
        if (!r) r = sbh_pos_of(sh, x, &bp, &off);
        if (r) return r;
        s_add += n;
        s_cur = bp << 16 | off;
        s_done = E_end <= E_hi || s_cur >= (split_end << 16);
        return SBH_OK;
      };
      if (!rc && s_idx >= 0 && (s_cur >> 16) < hi) {  // a split from an earlier window goes on here
        uint64_t f = 0;
        rc = sbh_flat_of(sh, s_cur >> 16, (uint32_t)(s_cur & 0xffff), &f);
        if (!rc) rc = follow(f, O.split_end[s_idx]);
      }
      if (!rc && straddles) {  // FindBlockStart + FindRecordStart here, then its chain to hi
        const uint64_t a = O.split_start[k1 - 1], e = O.split_end[k1 - 1];
        uint64_t fbs = 0, f0 = 0, first = 0, bp = 0;
        uint32_t off = 0;
        int32_t delta = 0;
        s_idx = (int64_t)(k1 - 1), s_new = true, s_add = 0;
        rc = sbh_find_block_start(sh, a, kcheck, &fbs);
        if (!rc) rc = sbh_flat_of(sh, fbs, 0, &f0);
        if (!rc) rc = sbh_find_record_start(sh, f0, rtc, mrs, &first, &delta);
        if (!rc) rc = sbh_pos_of(sh, first, &bp, &off);
        if (rc == SBH_E_NO_READ_FOUND || rc == SBH_E_HEADER_SEARCH_FAILED) {
          s_status = rc, s_done = true, rc = SBH_OK;
        } else if (!rc) {
          s_first = bp << 16 | off;
          s_cur = s_first;
          if (s_first >= (e << 16)) s_done = true;
          else rc = follow(first, e);
        }
      }
      split_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts0).count();
    }
    if (rc == SBH_E_NEED_HALO && ld < data_end) {  // grow the halo and redo this window
      HIPCHK(ctx, hipStreamSynchronize(R.cs));
      HIPCHK(ctx, hipStreamSynchronize(sh->st));
      account(0);
      account(1);
      halo *= 4;
      sh->comp.unlend();
      for (auto &b : R.buf) b.release();
      HIPCHK(ctx, size_bufs());
      HIPCHK(ctx, enqueue(cur, lo, load_end(hi)));
      prefetch = true;
      continue;
    }
    if (rc) return res->status = rc;
    if (s_idx >= 0) {  // commit the straddling split's progress
      if (s_new) {
        O.split_status[s_idx] = s_status;
        O.split_first_vpos[s_idx] = s_first;
        O.split_count[s_idx] = 0;
      }
      O.split_count[s_idx] += s_add;
      strad = s_done ? -1 : s_idx;
      strad_cur = s_cur;
    }
    res->ms_splits += split_ms;
    res->splits_host += nh;  // (a window redone with a larger halo counts its final attempt only)
    account(cur);
    if (O.verify_crc && r.n_blocks) {  // the owned blocks are the block table's prefix
      uint64_t nbad = 0, fbad = 0;
      float cms = 0.f;
      const bool was = sh->timing;
      sh->timing = true;
      rc = verify_crc_prefix(sh, std::min<uint64_t>(r.n_blocks, sh->nblocks), &nbad, &fbad, &cms);
      sh->timing = was;
      if (rc) return res->status = rc;
      if (nbad && !res->crc_bad_blocks) res->crc_first_bad = fbad;
      res->crc_bad_blocks += nbad;
      res->ms_crc += cms;
    }
    // this window's chain exit, and the stitch with the previous non-empty window
    uint64_t count = r.count, exit_vpos = ~0ull;
    auto vpos_of = [&](uint64_t flat, uint64_t *v) {
      uint64_t bp = 0;
      uint32_t off = 0;
      if (sbh_pos_of(sh, flat, &bp, &off) != SBH_OK) return false;
      *v = (bp << 16) | off;
      return true;
    };
    if (count) {
      uint64_t first_v = r.first_vpos;
      if (have_prev && prev_exit != ~0ull && first_v != prev_exit) {
        uint64_t f = 0, x = 0, E = 0;
        rc = sbh_flat_of(sh, prev_exit >> 16, (uint32_t)(prev_exit & 0xffff), &f);
        if (!rc) rc = sbh_flat_bound(sh, hi, &E);
        if (!rc) rc = sbh_chain_from(sh, f, E, &count, &x);
        if (rc) return res->status = rc;
        r.exit_flat = x;
        first_v = prev_exit;
        ++res->rewalks;
      }
      if (!vpos_of(r.exit_flat, &exit_vpos)) exit_vpos = ~0ull;
      if (res->first_vpos == ~0ull) res->first_vpos = first_v;
      if (count) {
        prev_exit = exit_vpos;
        have_prev = true;
      }
    }
    if (out_bits && r.flat_bytes) {  // this window's owned bits at global flat offset flat_base
      const uint64_t nb = (flat_base + r.flat_bytes + 7) / 8;
      if (nb > out_bits_cap) return res->status = fail(ctx, SBH_E_ARG, "out_bits_cap too small");
      wbits.assign((r.flat_bytes + 31) / 32 + 1, 0);
      HIPCHK(ctx, hipMemcpyAsync(wbits.data(), sh->bits.p, (r.flat_bytes + 7) / 8, hipMemcpyDeviceToHost, sh->st));
      HIPCHK(ctx, hipStreamSynchronize(sh->st));
      for (uint64_t i = 0; i < r.flat_bytes; ++i)
        if ((wbits[i >> 5] >> (i & 31)) & 1u) out_bits[(flat_base + i) >> 3] |= (uint8_t)(1u << ((flat_base + i) & 7));
    }
    ++res->n_windows;
    res->n_blocks += r.n_blocks;
    res->comp_bytes += r.comp_bytes;
    res->flat_bytes += r.flat_bytes;
    res->n_true += r.n_true;
    res->count += count;
    if (count) res->exit_vpos = exit_vpos;
    for (int i = 0; i < 6; ++i) res->stage_ms[i] += sh->stage_ms[i];
    flat_base += r.flat_bytes;
    if (!more) break;
    // the next window indexes from its first block: the first block at/after hi
    auto it = std::lower_bound(sh->hb.begin(), sh->hb.end(), hi,
                               [](const sbh_block &b, uint64_t v) { return b.start < v; });
    if (it == sh->hb.end()) return res->status = fail(ctx, SBH_E_NEED_HALO, "halo %llu holds no block past %llu",
                                                     (unsigned long long)halo, (unsigned long long)hi);
    start = it->start;
    sh->comp.unlend();
    lo = lo2;
    hi = hi2;
    cur = 1 - cur;
    prefetch = true;
  }
  HIPCHK(ctx, hipStreamSynchronize(R.cs));
  account(0);
  account(1);
  res->ms_h2d = h2d_ms;
  res->halo_final = halo;
  res->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  return res->status = SBH_OK;
}

}  // extern "C"
