// bam_gather.hip -- selected rows of a record scan laid out as one BAM stream (sbh_records_bam_scan).
// The row's validity and the predicate are defined in bam_gather_core.h for device and host.
//
//   k_bam_keep   one row per lane: validate, apply the predicate; len[i] = kept ? 4 + block_size : 0
//   k_bam_heads  kh[i] = keep | head << 32: a kept row starts a RUN unless the row before it is kept
//                too and ends exactly where this one starts in U (tested, not assumed from order)
//   (scans)      len -> off, kh -> khpre (kept rows before i | runs before i << 32)
//   k_bam_index  rec_off / rows per kept row, (dst, src) per run, the closing entries
//   k_bam_copy   one 16-byte-aligned granule of the OUTPUT per lane
//
// This file also defines the frame every filtered row stage shares (sbh_host.h; DESIGN "Row stages"):
// bam_filter_of / row_filter, stage_row_ranges and rows_verdict.
#include <algorithm>
#include <cstring>

#define SBH_HD __host__ __device__
#include "bam_gather_core.h"
#include "bam_name_core.h"
#include "bam_sort_core.h"
#include "sbh_host.h"

namespace sbh {
namespace {

constexpr uint32_t COPY_T = 256, COPY_TILE = COPY_T * 16;  // bytes of output per workgroup and pass
constexpr uint32_t COPY_GRID = 2048;             // k_bam_copy: 8 MiB of output a pass

__global__ __launch_bounds__(256) void k_bam_keep(const uint8_t *__restrict__ U, const uint64_t *pos, uint64_t n,
                                                  uint64_t total, sbh_bam::Filter F, uint64_t *len, uint64_t *keep,
                                                  unsigned long long *bad, unsigned long long *past) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const uint64_t p = pos[i];
    uint64_t bytes = 0;
    const int v = sbh_bam::row_check(U, total, p, &bytes);
    bool k = false;
    if (v != sbh_bam::ROW_OK) {
      // (per-row atomics, not RowMinima: the same two minima, and two loop-carried words fewer)
      atomicMin(bad, (unsigned long long)i);
      if (v == sbh_bam::ROW_PAST) atomicMin(past, (unsigned long long)i);
    } else {
      k = sbh_bam::row_keep(U + p, i, F);
    }
    len[i] = k ? bytes : 0;
    keep[i] = k;
  }
}

__global__ __launch_bounds__(256) void k_bam_heads(const uint64_t *pos, const uint64_t *len, uint64_t n,
                                                   uint64_t *kh) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const uint64_t k = kh[i];  // (k_bam_keep's keep flag; a kept row's len is >= 36)
    const bool joined = k && i && len[i - 1] && pos[i - 1] + len[i - 1] == pos[i];
    kh[i] = k | (uint64_t)(k && !joined) << 32;
  }
}

// i == n writes the closing entries: rec_off[n_kept] = run_dst[n_runs] = bytes
__global__ __launch_bounds__(256) void k_bam_index(const uint64_t *pos, const uint64_t *off, const uint64_t *kh,
                                                   const uint64_t *khpre, uint64_t n, uint64_t head_bytes,
                                                   uint64_t *rec_off, uint64_t *rows, uint64_t *run_dst,
                                                   uint64_t *run_src) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += step) {
    const uint64_t k = khpre[i] & 0xffffffffull, r = khpre[i] >> 32, at = head_bytes + off[i];
    if (i == n) {
      rec_off[k] = at;
      run_dst[r] = at;
    } else if (kh[i]) {
      rec_off[k] = at;
      rows[k] = i;
      if (kh[i] >> 32) {
        run_dst[r] = at;
        run_src[r] = pos[i];
      }
    }
  }
}

// Output bytes [head_bytes, bytes) from the runs: run r fills [run_dst[r], run_dst[r + 1]) from
// U[run_src[r] ...]; run_dst[0] == head_bytes, run_dst[n_runs] == bytes.  A workgroup owns the
// COPY_TILE bytes from T0; a run is at least 36 bytes, so at most 1 + 4095 / 36 = 114 runs begin
// inside a tile after the one holding T0: the COPY_T entries staged from that run on cover it.
// A lane whose granule lies inside one run reads the two aligned 16-byte words that hold its 16
// source bytes and funnels them by the byte shift; every other granule (a run edge inside it, the
// head's end, the stream's end) goes bytewise.
__global__ __launch_bounds__(COPY_T) void k_bam_copy(const uint8_t *__restrict__ U, const uint64_t *run_dst,
                                                     const uint64_t *run_src, uint64_t n_runs, uint64_t head_bytes,
                                                     uint64_t bytes, uint8_t *out) {
  __shared__ uint64_t s_dst[COPY_T], s_src[COPY_T];
  const uint32_t t = threadIdx.x;
  const uint64_t g0 = head_bytes / 16;  // the first granule with a run byte
  for (uint64_t T0 = (g0 + (uint64_t)blockIdx.x * COPY_T) * 16; T0 < bytes; T0 += (uint64_t)gridDim.x * COPY_TILE) {
    uint64_t lo = 0, hi = n_runs;  // runs with dst <= T0 (the same search in every lane)
    while (lo < hi) {
      const uint64_t m = (lo + hi) >> 1;
      if (run_dst[m] <= T0) lo = m + 1;
      else hi = m;
    }
    const uint64_t r0 = lo ? lo - 1 : 0;
    __syncthreads();  // (the previous tile's searches are done)
    s_dst[t] = r0 + t <= n_runs ? run_dst[r0 + t] : ~0ull;
    s_src[t] = r0 + t < n_runs ? run_src[r0 + t] : 0;
    __syncthreads();
    const uint64_t x = T0 + 16ull * t;
    if (x >= bytes || x + 16 <= head_bytes) continue;
    uint32_t a = 0, b = COPY_T;  // staged entries with dst <= x
    while (a < b) {
      const uint32_t m = (a + b) >> 1;
      if (s_dst[m] <= x) a = m + 1;
      else b = m;
    }
    uint32_t k = a ? a - 1 : 0;
    if (a && k + 1 < COPY_T && s_dst[k + 1] >= x + 16 && s_dst[k + 1] != ~0ull) {
      const uint64_t src = s_src[k] + (x - s_dst[k]), base = src & ~15ull;
      const uint4 A = *reinterpret_cast<const uint4 *>(U + base), B = *reinterpret_cast<const uint4 *>(U + base + 16);
      const uint32_t sh = (uint32_t)src & 3u;
      uint32_t d0, d1, d2, d3, d4;
      switch (((uint32_t)src >> 2) & 3u) {
        case 0: d0 = A.x, d1 = A.y, d2 = A.z, d3 = A.w, d4 = B.x; break;
        case 1: d0 = A.y, d1 = A.z, d2 = A.w, d3 = B.x, d4 = B.y; break;
        case 2: d0 = A.z, d1 = A.w, d2 = B.x, d3 = B.y, d4 = B.z; break;
        default: d0 = A.w, d1 = B.x, d2 = B.y, d3 = B.z, d4 = B.w; break;
      }
      *reinterpret_cast<uint4 *>(out + x) =
          make_uint4(__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                     __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh));
    } else {
      for (uint32_t j = 0; j < 16; ++j) {
        const uint64_t y = x + j;
        if (y < head_bytes || y >= bytes) continue;
        while (k + 1 < COPY_T && s_dst[k + 1] <= y) ++k;
        out[y] = U[s_src[k] + (y - s_dst[k])];
      }
    }
  }
}

}  // namespace

// len, kh: n + 1 words (the caller zeroes entry n); bad, past preset to ~0: the first invalid row, the
// first row invalid only because the stream ends too early.  F's row ranges are device memory.
static hipError_t launch_bam_keep(const uint8_t *U, const uint64_t *pos, uint64_t n, uint64_t total, const sbh_bam::Filter &F,
                                  uint64_t *len, uint64_t *kh, unsigned long long *bad, unsigned long long *past,
                                  hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_bam_keep, dim3(rows_grid(n)), dim3(256), 0, st, U, pos, n, total, F, len, kh, bad, past);
  hipLaunchKernelGGL(k_bam_heads, dim3(rows_grid(n)), dim3(256), 0, st, pos, len, n, kh);
  return hipGetLastError();
}

// k_bam_heads alone, over rows whose len and keep flags (kh) are already there (the sorted rows)
static hipError_t launch_bam_heads(const uint64_t *pos, const uint64_t *len, uint64_t n, uint64_t *kh, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_bam_heads, dim3(rows_grid(n)), dim3(256), 0, st, pos, len, n, kh);
  return hipGetLastError();
}

// off, khpre: the exclusive scans of len and kh over n + 1 entries (kh = keep | run head << 32, so
// n < 2^32); rec_off, rows, run_dst, run_src: n + 1 words
static hipError_t launch_bam_index(const uint64_t *pos, const uint64_t *off, const uint64_t *kh, const uint64_t *khpre,
                                   uint64_t n, uint64_t head_bytes, uint64_t *rec_off, uint64_t *rows, uint64_t *run_dst,
                                   uint64_t *run_src, hipStream_t st) {
  hipLaunchKernelGGL(k_bam_index, dim3(rows_grid(n + 1)), dim3(256), 0, st, pos, off, kh, khpre, n, head_bytes, rec_off,
                     rows, run_dst, run_src);
  return hipGetLastError();
}

// out[head_bytes, bytes) from the runs; reads U below (the last run's end) + 32
static hipError_t launch_bam_copy(const uint8_t *U, const uint64_t *run_dst, const uint64_t *run_src, uint64_t n_runs,
                                  uint64_t head_bytes, uint64_t bytes, uint8_t *out, hipStream_t st) {
  if (!n_runs || bytes <= head_bytes) return hipSuccess;
  const uint64_t tiles = ((bytes + 15) / 16 - head_bytes / 16 + COPY_T - 1) / COPY_T;
  hipLaunchKernelGGL(k_bam_copy, dim3((uint32_t)std::min<uint64_t>(tiles, COPY_GRID)), dim3(COPY_T), 0, st, U, run_dst,
                     run_src, n_runs, head_bytes, bytes, out);
  return hipGetLastError();
}

bool bam_filter_of(const sbh_record_filter *f, sbh_bam::Filter *F) {
  *F = sbh_bam::Filter{0, 0, 0, nullptr, nullptr, 0};
  if (f) *F = sbh_bam::Filter{f->flag_require, f->flag_exclude, f->min_mapq, f->row_begin, f->row_end, f->n_row_ranges};
  return sbh_bam::filter_ok(*F);
}

int row_filter(sbh_ctx *ctx, const sbh_record_filter *f, sbh_bam::Filter *F) {
  if (bam_filter_of(f, F)) return SBH_OK;
  return fail(ctx, SBH_E_ARG, "record filter: flags < 65536, 0 <= min_mapq <= 255, row ranges sorted, disjoint and non-empty");
}

hipError_t stage_row_ranges(sbh_shard *sh, sbh_bam::Filter *F) {
  const uint64_t nr = F->n_row_ranges;
  hipError_t e = sh->row_ranges.ensure(2 * nr);
  uint64_t *d = sh->row_ranges.p;
  if (e == hipSuccess && nr) e = hipMemcpyAsync(d, F->row_begin, 8 * nr, hipMemcpyHostToDevice, sh->st);
  if (e == hipSuccess && nr) e = hipMemcpyAsync(d + nr, F->row_end, 8 * nr, hipMemcpyHostToDevice, sh->st);
  F->row_begin = d, F->row_end = d + nr;
  return e;
}

int rows_verdict(sbh_shard *sh, uint64_t bad, uint64_t past, const char *also) {
  if (bad == ~0ull) return SBH_OK;
  // only a record that runs past the resident bytes can be cured by more of them
  if (past == bad && !sh->at_eof)
    return fail(sh->ctx, SBH_E_NEED_HALO, "record %llu of the scan may run past the shard", (unsigned long long)bad);
  return fail_with(sh->ctx, SBH_E_BAD_RECORD, {(int64_t)bad}, "record %llu of the scan does not fit its block or the stream%s",
                   (unsigned long long)bad, also);
}

}  // namespace sbh

using namespace sbh;

extern "C" {

// ---- the C-ABI's BAM stream calls (validity and predicate in bam_gather_core.h) ---------------
// Keep pass, two scans, index pass -- all launched before anything is read back, so one round trip
// brings (first invalid row, first row past the end, kept bytes, kept rows | runs << 32); then the
// stream is allocated, the head copied in and the runs copied behind it.
int sbh_records_bam_scan(sbh_shard *sh, const uint8_t *head, uint64_t head_bytes, const sbh_record_filter *filter,
                         sbh_bam_sizes *out) {
  return sbh_records_bam_scan_order(sh, head, head_bytes, filter, SBH_ORDER_SCAN, out);
}

// SBH_ORDER_COORDINATE: the scan-order pipeline runs as it is up to k_bam_index, whose rows[] are the
// kept rows; k_sort_keys follows it, and the one round trip brings its three counters as well.  No
// descent: the scan order is the coordinate order and the call goes on exactly as in scan order.
// Otherwise the passes whose digit differs somewhere (OR & ~AND) run, k_sort_apply lays out the
// permuted starts and lengths, and k_bam_heads, the scans and k_bam_index run over those -- every
// entry kept -- before a second round trip for the run count.
//
// ORDER_NAME (sbh_records_bam_scan_names; bam_name.hip): k_name_scan stands where k_sort_keys
// stands and the same round trip brings its words (nacc::).  No descent: as above.  Otherwise the tie
// stage, then the chunks from the last one the longest name reaches down to chunk 0 -- each k_name_keys
// and the passes whose digit differs somewhere, skipped whole when the chunk is the same in every row
// -- all enqueued with no host read between them; then k_sort_apply and the rest as in coordinate
// order.  k_name_groups runs over the final row array either way, and its four words come back with
// the call's last synchronisation.
static int bam_scan(sbh_shard *sh, const uint8_t *head, uint64_t head_bytes, const sbh_record_filter *filter, int order,
                    sbh_bam_sizes *out) {
  if (!sh || !out || (head_bytes && !head)) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &R = sh->rec;
  auto &B = sh->bam;
  const bool named = order == ORDER_NAME;
  const bool sorted = order == SBH_ORDER_COORDINATE || named;
  if (!R.valid) return fail(ctx, SBH_E_STATE, "records_bam_scan without a records scan");
  sbh_bam::Filter F;
  int rc = row_filter(ctx, filter, &F);
  if (rc) return rc;
  const uint64_t n = R.sz.n;
  if (n >= 0xffffffffull)
    return fail(ctx, SBH_E_ARG, "records_bam_scan: %llu rows in one scan (scan in windows)", (unsigned long long)n);
  rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  B.valid = false;
  uint64_t bytes = head_bytes, n_kept = 0, n_runs = 0;
  for (auto *b : {&B.len, &B.off, &B.kh, &B.khpre, &B.rec_off, &B.rows, &B.run_dst, &B.run_src}) HIPCHK(ctx, b->ensure(n + 1));
  const uint64_t hist_words = 256 * sort_tiles(n) + 1;
  if (sorted && n) {  // (sized for n: the kept count is not known here)
    for (auto *b : {&B.skey[0], &B.skey[1]}) HIPCHK(ctx, b->ensure(n));
    for (auto *b : {&B.srow[0], &B.srow[1]}) HIPCHK(ctx, b->ensure(n));
    for (auto *b : {&B.pos2, &B.len2}) HIPCHK(ctx, b->ensure(n + 1));
    HIPCHK(ctx, B.hist.ensure(2 * hist_words));
    HIPCHK(ctx, sh->tmp.ensure(scan_tmp_words(hist_words)));
    if (named) HIPCHK(ctx, B.nacc.ensure(nacc::WORDS));
  }
  bool already = true;
  sbh_bam_name_info info{};
  unsigned long long *hn = sh->h_ctr + ctr::H_NAME;  // the name words' mirror
  if (n) {
    HIPCHK(ctx, stage_row_ranges(sh, &F));
    HIPCHK(ctx, sh->tmp.ensure(scan_tmp_words(n + 1)));
    HIPCHK(ctx, hipMemsetAsync(B.len.p + n, 0, 8, st));
    HIPCHK(ctx, hipMemsetAsync(B.kh.p + n, 0, 8, st));
    unsigned long long *bad = sh->ctr.p + ctr::BAM_BAD;  // (BAM_PAST is the next word)
    static_assert(ctr::BAM_PAST == ctr::BAM_BAD + 1, "one memset, one copy");
    HIPCHK(ctx, hipMemsetAsync(bad, 0xff, 16, st));
    HIPCHK(ctx, launch_bam_keep(sh->U.p, R.pos.p, n, sh->utotal, F, B.len.p, B.kh.p, bad, bad + 1, st));
    HIPCHK(ctx, scan_exclusive_u64(B.len.p, B.off.p, n + 1, sh->tmp.p, st));
    HIPCHK(ctx, scan_exclusive_u64(B.kh.p, B.khpre.p, n + 1, sh->tmp.p, st));
    HIPCHK(ctx, launch_bam_index(R.pos.p, B.off.p, B.kh.p, B.khpre.p, n, head_bytes, B.rec_off.p, B.rows.p, B.run_dst.p,
                                 B.run_src.p, st));
    unsigned long long *acc = sh->ctr.p + ctr::SORT_DESC;
    static_assert(ctr::SORT_OR == ctr::SORT_DESC + 1 && ctr::SORT_AND == ctr::SORT_DESC + 2, "one copy");
    if (named) {
      HIPCHK(ctx, hipMemsetAsync(B.nacc.p, 0, 8 * nacc::ONES, st));
      HIPCHK(ctx, hipMemsetAsync(B.nacc.p + nacc::ONES, 0xff, 8 * (nacc::WORDS - nacc::ONES), st));
      HIPCHK(ctx, launch_name_scan(sh->U.p, R.pos.p, B.rows.p, B.khpre.p + n, n, B.srow[0].p, B.nacc.p, st));
      HIPCHK(ctx, hipMemcpyAsync(hn, B.nacc.p, 8 * nacc::WORDS, hipMemcpyDeviceToHost, st));
    } else if (sorted) {
      HIPCHK(ctx, hipMemsetAsync(acc, 0, 16, st));
      HIPCHK(ctx, hipMemsetAsync(acc + 2, 0xff, 8, st));
      HIPCHK(ctx, launch_sort_keys(sh->U.p, R.pos.p, B.rows.p, B.khpre.p + n, n, B.skey[0].p, B.srow[0].p, acc, st));
      HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::SORT_DESC, acc, 24, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::BAM_BAD, bad, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_BAM_BYTES, B.off.p + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_BAM_KH, B.khpre.p + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    rc = rows_verdict(sh, sh->h_ctr[ctr::BAM_BAD], sh->h_ctr[ctr::BAM_PAST], "");
    if (rc) return rc;
    bytes += sh->h_ctr[ctr::H_BAM_BYTES];
    n_kept = sh->h_ctr[ctr::H_BAM_KH] & 0xffffffffull;
    n_runs = sh->h_ctr[ctr::H_BAM_KH] >> 32;
    if (named) info.max_name = (uint32_t)hn[nacc::MAX_L];
    if (sorted && (named ? hn[nacc::DESC] : sh->h_ctr[ctr::SORT_DESC])) {
      already = false;
      const uint64_t m = n_kept;
      int cur = 0;
      // the passes of one key fill: every digit that differs somewhere (the same digit in every key:
      // the pass would move nothing)
      auto passes = [&](uint64_t differ) -> hipError_t {
        for (uint32_t shift = 0; shift < 64; shift += 8) {
          if (!((differ >> shift) & 0xff)) continue;
          hipError_t e = launch_sort_pass(B.skey[cur].p, B.srow[cur].p, m, shift, B.hist.p, sh->tmp.p,
                                          B.skey[cur ^ 1].p, B.srow[cur ^ 1].p, st);
          if (e != hipSuccess) return e;
          cur ^= 1;
          ++info.passes_run;
        }
        return hipSuccess;
      };
      if (!named) {
        HIPCHK(ctx, passes(sh->h_ctr[ctr::SORT_OR] & ~sh->h_ctr[ctr::SORT_AND]));
      } else {
        // a chunk the shortest name does not reach is 0 in some row, whatever the waves that reduced it saw
        for (uint32_t c = 0; c < sbh_bam::NAME_CHUNKS; ++c)
          if (8 * c >= hn[nacc::MIN_L]) hn[nacc::AND + c] = 0;
        if (const uint64_t d = hn[nacc::TIE_OR] & ~hn[nacc::TIE_AND]) {
          HIPCHK(ctx, launch_name_keys(sh->U.p, R.pos.p, B.srow[cur].p, m, sbh_bam::NAME_CHUNKS, B.skey[cur].p, st));
          HIPCHK(ctx, passes(d));
        }
        for (uint32_t c = (info.max_name + 7) / 8; c-- > 0;) {
          const uint64_t d = hn[nacc::OR + c] & ~hn[nacc::AND + c];
          if (!d) continue;
          HIPCHK(ctx, launch_name_keys(sh->U.p, R.pos.p, B.srow[cur].p, m, c, B.skey[cur].p, st));
          HIPCHK(ctx, passes(d));
          ++info.chunks_run;
        }
        HIPCHK(ctx, launch_name_groups(sh->U.p, R.pos.p, B.srow[cur].p, m, B.nacc.p + nacc::GROUPS, st));
        HIPCHK(ctx, hipMemcpyAsync(hn + nacc::GROUPS, B.nacc.p + nacc::GROUPS, 32, hipMemcpyDeviceToHost, st));
      }
      HIPCHK(ctx, launch_sort_apply(R.pos.p, B.len.p, B.srow[cur].p, m, B.pos2.p, B.len2.p, B.kh.p, st));
      HIPCHK(ctx, launch_bam_heads(B.pos2.p, B.len2.p, m, B.kh.p, st));
      HIPCHK(ctx, scan_exclusive_u64(B.len2.p, B.off.p, m + 1, sh->tmp.p, st));
      HIPCHK(ctx, scan_exclusive_u64(B.kh.p, B.khpre.p, m + 1, sh->tmp.p, st));
      HIPCHK(ctx, launch_bam_index(B.pos2.p, B.off.p, B.kh.p, B.khpre.p, m, head_bytes, B.rec_off.p, B.rows.p,
                                   B.run_dst.p, B.run_src.p, st));
      HIPCHK(ctx, launch_sort_rows(B.srow[cur].p, m, B.rows.p, st));
      HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_BAM_KH, B.khpre.p + m, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      n_runs = sh->h_ctr[ctr::H_BAM_KH] >> 32;
    } else if (named) {  // in order as scanned: the groups of the kept rows as k_name_scan laid them out
      HIPCHK(ctx, launch_name_groups(sh->U.p, R.pos.p, B.srow[0].p, n_kept, B.nacc.p + nacc::GROUPS, st));
      HIPCHK(ctx, hipMemcpyAsync(hn + nacc::GROUPS, B.nacc.p + nacc::GROUPS, 32, hipMemcpyDeviceToHost, st));
    }
  } else {
    HIPCHK(ctx, hipMemcpyAsync(B.rec_off.p, &head_bytes, 8, hipMemcpyHostToDevice, st));
  }
  HIPCHK(ctx, B.out.ensure(bytes + 16));
  if (head_bytes) HIPCHK(ctx, hipMemcpyAsync(B.out.p, head, head_bytes, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, launch_bam_copy(sh->U.p, B.run_dst.p, B.run_src.p, n_runs, head_bytes, bytes, B.out.p, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  B.sz = sbh_bam_sizes{n, n_kept, bytes};
  B.head_bytes = head_bytes;
  B.order = order;
  B.already = already;
  if (named) {
    if (n) info.n_names = hn[nacc::GROUPS], info.n_single = hn[nacc::GROUPS + 1], info.n_pair = hn[nacc::GROUPS + 2],
           info.n_more = hn[nacc::GROUPS + 3];
    info.already = already ? 1 : 0;
    B.name_info = info;
  }
  B.valid = true;
  *out = B.sz;
  return SBH_OK;
}

int sbh_records_bam_scan_order(sbh_shard *sh, const uint8_t *head, uint64_t head_bytes, const sbh_record_filter *filter,
                               int order, sbh_bam_sizes *out) {
  if (!sh || !out || (head_bytes && !head)) return SBH_E_ARG;
  if (order != SBH_ORDER_SCAN && order != SBH_ORDER_COORDINATE)
    return fail(sh->ctx, SBH_E_ARG, "records_bam_scan: order %d is neither SBH_ORDER_SCAN nor SBH_ORDER_COORDINATE", order);
  return bam_scan(sh, head, head_bytes, filter, order, out);
}

int sbh_records_bam_scan_names(sbh_shard *sh, const uint8_t *head, uint64_t head_bytes, const sbh_record_filter *filter,
                               sbh_bam_sizes *out) {
  return bam_scan(sh, head, head_bytes, filter, ORDER_NAME, out);
}

int sbh_records_bam_name_info(sbh_shard *sh, sbh_bam_name_info *out) {
  if (!sh || !out) return SBH_E_ARG;
  const auto &B = sh->bam;
  if (!B.valid || B.order != ORDER_NAME)
    return fail(sh->ctx, SBH_E_STATE, "records_bam_name_info without a name-order records_bam_scan");
  *out = B.name_info;
  return SBH_OK;
}

int sbh_records_bam_sorted(sbh_shard *sh, int *already) {
  if (!sh || !already) return SBH_E_ARG;
  const auto &B = sh->bam;
  if (!B.valid || B.order != SBH_ORDER_COORDINATE)
    return fail(sh->ctx, SBH_E_STATE, "records_bam_sorted without a coordinate-order records_bam_scan");
  *already = B.already ? 1 : 0;
  return SBH_OK;
}

const void *sbh_records_bam_device_ptr(sbh_shard *sh) { return sh && sh->bam.valid ? sh->bam.out.p : nullptr; }

int sbh_records_bam_fetch(sbh_shard *sh, uint8_t *stream, uint64_t *rec_off, uint64_t *rows) {
  if (!sh) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &B = sh->bam;
  if (!B.valid) return fail(ctx, SBH_E_STATE, "records_bam_fetch without a records_bam_scan");
  int rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  if (stream && B.sz.bytes) HIPCHK(ctx, hipMemcpyAsync(stream, B.out.p, B.sz.bytes, hipMemcpyDeviceToHost, st));
  if (rec_off) HIPCHK(ctx, hipMemcpyAsync(rec_off, B.rec_off.p, 8 * (B.sz.n_kept + 1), hipMemcpyDeviceToHost, st));
  if (rows && B.sz.n_kept) HIPCHK(ctx, hipMemcpyAsync(rows, B.rows.p, 8 * B.sz.n_kept, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return SBH_OK;
}

int sbh_records_bam_read(sbh_shard *sh, uint64_t offset, uint64_t n, uint8_t *out) {
  if (!sh || (n && !out)) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &B = sh->bam;
  if (!B.valid) return fail(ctx, SBH_E_STATE, "records_bam_read without a records_bam_scan");
  if (offset > B.sz.bytes || n > B.sz.bytes - offset) return fail(ctx, SBH_E_ARG, "records_bam_read past the stream");
  int rc = set_device(ctx);
  if (rc) return rc;
  if (n) HIPCHK(ctx, hipMemcpyAsync(out, B.out.p + offset, n, hipMemcpyDeviceToHost, sh->st));
  HIPCHK(ctx, hipStreamSynchronize(sh->st));
  return SBH_OK;
}

int sbh_bam_gather_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n, const uint8_t *head,
                        uint64_t head_bytes, const sbh_record_filter *filter, uint8_t *out, uint64_t out_cap,
                        uint64_t *rec_off, uint64_t *rows, uint64_t *n_kept, uint64_t *bad_row) {
  if ((!flat && flat_size) || (!starts && n) || (!head && head_bytes) || !n_kept) return SBH_E_ARG;
  sbh_bam::Filter F;
  if (!bam_filter_of(filter, &F)) return SBH_E_ARG;
  uint64_t bad = sbh_bam::NO_ROW, bytes = 0;
  const int rc = sbh_bam::gather_host(flat, flat_size, starts, n, head, head_bytes, F, out, out_cap, rec_off, rows, n_kept,
                                      &bytes, &bad);
  if (bad_row) *bad_row = bad;
  return rc == 0 ? SBH_OK : rc == 1 ? SBH_E_BAD_RECORD : SBH_E_ARG;
}

int sbh_bam_sort_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n, uint64_t *perm,
                      uint64_t *bad_row) {
  if ((!flat && flat_size) || (!starts && n) || (!perm && n)) return SBH_E_ARG;
  uint64_t bad = sbh_bam::NO_ROW;
  const int rc = sbh_bam::sort_host(flat, flat_size, starts, n, perm, &bad);
  if (bad_row) *bad_row = bad;
  return rc == 0 ? SBH_OK : SBH_E_BAD_RECORD;
}

int sbh_bam_name_sort_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n, uint64_t *perm,
                           sbh_bam_name_info *info, uint64_t *bad_row) {
  if ((!flat && flat_size) || (!starts && n) || (!perm && n)) return SBH_E_ARG;
  static_assert(sizeof(sbh_bam::NameInfo) == sizeof(sbh_bam_name_info), "bam_name_core.h restates the struct");
  uint64_t bad = sbh_bam::NO_ROW;
  sbh_bam::NameInfo ni{};
  const int rc = sbh_bam::name_sort_host(flat, flat_size, starts, n, perm, info ? &ni : nullptr, &bad);
  if (info)
    *info = sbh_bam_name_info{ni.n_names, ni.n_single, ni.n_pair, ni.n_more, ni.max_name, ni.chunks_run, ni.passes_run,
                              ni.already};
  if (bad_row) *bad_row = bad;
  return rc == 0 ? SBH_OK : SBH_E_BAD_RECORD;
}

int sbh_bam_header_set_so(const uint8_t *head, uint64_t n, const char *so, uint8_t *out, uint64_t cap, uint64_t *out_n) {
  if (!head || !so || !out_n) return SBH_E_ARG;
  return sbh_bam::header_set_so(head, n, so, out, cap, out_n) == 0 ? SBH_OK : SBH_E_ARG;
}

}  // extern "C"
