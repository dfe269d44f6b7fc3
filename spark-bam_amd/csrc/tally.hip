// tally.hip -- flag counts and per-reference read counts of a record scan's rows into an accumulator
// (sbh_records_tally_add, sbh_tally_fetch).  The counts are defined in tally_core.h for device and
// host.
//
//   k_tally_rows    one row per lane, grid-stride: row_check, row_keep, the reference range and the
//                   counting in one pass over each record's fixed bytes.  It counts into the
//                   accumulator's staging words (zero before every add), never into the totals:
//                     the smallest bad row and the smallest row that only runs past the stream
//                       (RowMinima, sbh_internal.h, as every filtered row kernel records them; the
//                       host's rows_verdict reads them);
//                     the 32 flag counters as ballot + popcount into wave-uniform registers over the
//                       whole loop (per row both columns together, and the QC-fail column only in
//                       a round that holds such a row), combined through LDS and sent out once per
//                       workgroup, non-zero counters only;
//                     the per-reference counters: a wave whose kept lanes share one bin adds its two
//                       popcounts to a run (bin, mapped, unmapped) it holds across rounds, flushed
//                       by one lane when the bin changes and behind the loop; in any other wave the
//                       kept lanes add one each -- into an LDS histogram flushed once per
//                       workgroup when 2 (n_ref + 1) counters fit TALLY_LDS_BINS, else straight into
//                       the staging words.
//                   Every counter is a sum over kept rows: the answer does not depend on the path a
//                   wave takes or on the order of the rows.
//   k_tally_commit  totals[i] += staging[i], launched only when the add's one round trip found no
//                   bad row: a failed add leaves the totals as they were.
#include <algorithm>

#define SBH_HD __host__ __device__
#include "tally_core.h"
#include "sbh_host.h"

namespace sbh {
namespace {

using sbh_tal::TALLY_LDS_BINS;
using sbh_tal::TALLY_ROWS;
constexpr uint32_t FLAG_WORDS = 2 * TALLY_ROWS;
// the staging words: bad, past, the flag counters, the per-reference counters
constexpr uint32_t ST_BAD = 0, ST_PAST = 1, ST_FLAG = 2, ST_REF = ST_FLAG + FLAG_WORDS;
static_assert(TALLY_ROWS == SBH_TALLY_ROWS, "tally_core.h restates the header's row count");
static_assert(TALLY_LDS_BINS * 8 + FLAG_WORDS * 4 * 8 <= 160 * 1024 / 8, "eight workgroups' LDS fit a CU");

// stage: ST_BAD, ST_PAST preset ~0, everything behind them 0; 2 + FLAG_WORDS + n_slots words, n_slots =
// 2 (n_ref + 1).
__global__ __launch_bounds__(256) void k_tally_rows(const uint8_t *__restrict__ U, const uint64_t *pos, uint64_t n,
                                                    uint64_t total, sbh_bam::Filter F, int32_t n_ref, uint64_t n_slots,
                                                    unsigned long long *stage) {
  __shared__ unsigned long long s_hist[TALLY_LDS_BINS];
  __shared__ unsigned long long s_flag[4][FLAG_WORDS];
  const bool in_lds = n_slots <= TALLY_LDS_BINS;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long *ref = stage + ST_REF;
  // a wave's mixed rounds and its run go to s_hist[j] or ref[j], j < n_slots
  auto count = [&](uint64_t j, unsigned long long v) {
    if (in_lds) atomicAdd(&s_hist[j], v);
    else atomicAdd(ref + j, v);
  };
  if (in_lds) {
    for (uint32_t j = threadIdx.x; j < (uint32_t)n_slots; j += 256) s_hist[j] = 0;
    __syncthreads();
  }
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  RowMinima m;
  // wave-uniform: per row the kept rows of both columns, and those of the QC-fail column.  32 bits
  // hold them: a wave sees at most 64 rows a pass of 262144, and the launcher refuses n >= 2^43
  uint32_t all[TALLY_ROWS], fail[TALLY_ROWS];
#pragma unroll
  for (uint32_t c = 0; c < TALLY_ROWS; ++c) all[c] = fail[c] = 0;
  uint64_t run_bin = 0, run_m = 0, run_u = 0;  // wave-uniform: the run, empty while run_m + run_u == 0
  // (the loop is uniform in the workgroup: the ballots run with every lane of the wave)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += step) {
    const uint64_t i = base + threadIdx.x;
    bool k = false;
    uint32_t fl = 0, rows = 0;
    int32_t tid = -1;
    if (i < n) {
      const uint64_t p = pos[i];
      uint64_t bytes = 0;
      const int v = sbh_bam::row_check(U, total, p, &bytes);
      if (v != sbh_bam::ROW_OK) {
        m.refused(i, v == sbh_bam::ROW_PAST);
      } else if (sbh_bam::row_keep(U + p, i, F)) {
        const uint8_t *r = U + p;
        tid = (int32_t)sbh_bam::ld32(r + 4);
        if (tid >= n_ref) {
          m.rejected(i);
        } else {
          k = true;
          fl = sbh_bam::ld32(r + 16) >> 16;
          rows = sbh_tal::rows_of(fl, r[13], tid, (int32_t)sbh_bam::ld32(r + 24));
        }
      }
    }
    const uint64_t km = __ballot(k);
    if (!km) continue;  // (uniform)
    // a lane that is not kept has rows == 0 and fl == 0: it is in no ballot below
    const uint64_t qm = __ballot(sbh_tal::qc_col(fl) != 0);
#pragma unroll
    for (uint32_t row = 0; row < TALLY_ROWS; ++row) all[row] += (uint32_t)__popcll(__ballot((rows >> row) & 1u));
    if (qm) {  // (uniform) QC-fail rows are rare
#pragma unroll
      for (uint32_t row = 0; row < TALLY_ROWS; ++row) fail[row] += (uint32_t)__popcll(__ballot((rows >> row) & 1u) & qm);
    }
    // the per-reference counter of a kept lane: below n_slots, since tid < n_ref was tested above
    const uint64_t slot = sbh_tal::ref_slot(fl, tid, n_ref);
    const uint32_t bin = (uint32_t)(slot >> 1);
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, __builtin_ctzll(km));  // a kept lane's bin
    if (__ballot(k && bin == b0) == km) {  // (uniform) every kept lane of the wave sits on bin b0
      if ((run_m | run_u) && run_bin != b0) {
        if (lane == 0) {
          if (run_m) count(2 * run_bin, run_m);
          if (run_u) count(2 * run_bin + 1, run_u);
        }
        run_m = run_u = 0;
      }
      const uint64_t um = __ballot(k && (slot & 1));
      run_bin = b0;
      run_m += (uint64_t)__popcll(km & ~um);
      run_u += (uint64_t)__popcll(um);
    } else if (k && slot < n_slots) {
      count(slot, 1ull);
    }
  }
  if (lane == 0) {  // run_bin is a kept lane's bin: 2 run_bin + 1 < n_slots
    if (run_m) count(2 * run_bin, run_m);
    if (run_u) count(2 * run_bin + 1, run_u);
  }
  m.send(stage + ST_BAD, stage + ST_PAST);
  if (lane == 0) {
#pragma unroll
    for (uint32_t c = 0; c < TALLY_ROWS; ++c) s_flag[wave][2 * c] = all[c] - fail[c], s_flag[wave][2 * c + 1] = fail[c];
  }
  __syncthreads();  // s_flag is whole, and every wave's adds into s_hist are done
  if (threadIdx.x < FLAG_WORDS) {
    const unsigned long long t = s_flag[0][threadIdx.x] + s_flag[1][threadIdx.x] + s_flag[2][threadIdx.x] + s_flag[3][threadIdx.x];
    if (t) atomicAdd(stage + ST_FLAG + threadIdx.x, t);
  }
  if (in_lds) {
    for (uint32_t j = threadIdx.x; j < (uint32_t)n_slots; j += 256) {
      const unsigned long long t = s_hist[j];
      if (t) atomicAdd(ref + j, t);
    }
  }
}

// totals[i] += staged[i] for i < m: one lane per word, no word is touched by two
__global__ __launch_bounds__(256) void k_tally_commit(unsigned long long *totals, const unsigned long long *staged,
                                                      uint64_t m) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x)
    totals[i] += staged[i];
}

}  // namespace

// stage: the accumulator's 2 + words staging words, preset by the caller (~0, ~0, then zeros)
static hipError_t launch_tally_rows(const uint8_t *U, const uint64_t *pos, uint64_t n, uint64_t total, const sbh_bam::Filter &F,
                                    int32_t n_ref, unsigned long long *stage, hipStream_t st) {
  if (!n) return hipSuccess;
  if (n >> 43) return hipErrorInvalidValue;  // (k_tally_rows' 32-bit wave counters; no memory holds 2^43 records)
  hipLaunchKernelGGL(k_tally_rows, dim3(rows_grid(n)), dim3(256), 0, st, U, pos, n, total, F, n_ref, 2 * ((uint64_t)n_ref + 1), stage);
  return hipGetLastError();
}

static hipError_t launch_tally_commit(unsigned long long *totals, const unsigned long long *staged, uint64_t m,
                                      hipStream_t st) {
  hipLaunchKernelGGL(k_tally_commit, dim3(rows_grid(m)), dim3(256), 0, st, totals, staged, m);
  return hipGetLastError();
}

}  // namespace sbh

using namespace sbh;

extern "C" {

// ---- the C-ABI's tally calls (the definition in tally_core.h) ---------------------------------
int sbh_tally_create(sbh_ctx *ctx, int32_t n_ref, sbh_tally **out) {
  if (!ctx || !out) return SBH_E_ARG;
  *out = nullptr;
  if (n_ref < 0) return fail(ctx, SBH_E_ARG, "tally: n_ref %d is negative", n_ref);
  int rc = set_device(ctx);
  if (rc) return rc;
  sbh_tally *t = new sbh_tally();
  t->ctx = ctx;
  t->n_ref = n_ref;
  t->words = FLAG_WORDS + 2 * ((uint64_t)n_ref + 1);
  char nomem[80];
  std::snprintf(nomem, sizeof nomem, "tally: no memory for the counters of %d references", n_ref);
  return accum_open(t, out, nomem, "tally create", [t] {
    hipError_t e = t->stage.ensure(ST_FLAG + t->words);
    if (e == hipSuccess) e = t->totals.ensure(t->words);
    if (e == hipSuccess) e = hipMemsetAsync(t->totals.p, 0, 8 * t->words, t->st);
    return e;
  });
}

int sbh_tally_destroy(sbh_tally *t) {
  delete t;  // (~sbh_tally; a null accumulator is fine)
  return SBH_OK;
}

int sbh_tally_reset(sbh_tally *t) { return t ? t->reset(t->totals.p, 8 * t->words) : SBH_E_ARG; }

// Two memsets, k_tally_rows, one round trip (bad row, past row, the two totals of kept rows), then
// k_tally_commit only when no row is bad: a failed add has written nothing into the totals.
int sbh_records_tally_add(sbh_shard *sh, sbh_tally *t, const sbh_record_filter *filter, sbh_tally_add_result *out) {
  if (!sh || !t || !out) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &R = sh->rec;
  sbh_bam::Filter F;
  int rc = add_begin(sh, t, "records_tally_add", nullptr, filter, &F);
  if (rc) return rc;
  const uint64_t n = R.sz.n;
  *out = sbh_tally_add_result{n, 0};
  if (!n) return SBH_OK;
  hipStream_t st = sh->st;
  // the head: bad, past, total[QC-pass], total[QC-fail] -- the first two flag counters
  static_assert(ST_BAD == ctr::ADD_BAD && ST_PAST == ctr::ADD_PAST && ST_FLAG == ctr::ADD_A, "the staging words open with the head");
  const AddTrip trip{sh, t->stage.p, ctr::H_STAGE_HEAD};
  rc = trip.open(&F, nullptr, t->words);
  if (rc) return rc;
  HIPCHK(ctx, launch_tally_rows(sh->U.p, R.pos.p, n, sh->utotal, F, t->n_ref, t->stage.p, st));
  rc = trip.verdict(", or its reference is out of range");
  if (rc) return rc;
  out->n_kept = trip.a() + trip.b();
  if (out->n_kept) {
    HIPCHK(ctx, launch_tally_commit(t->totals.p, t->stage.p + ST_FLAG, t->words, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  return SBH_OK;
}

int sbh_tally_fetch(sbh_tally *t, uint64_t *flag, uint64_t first_bin, uint64_t n_bins, uint64_t *ref) {
  if (!t) return SBH_E_ARG;
  sbh_ctx *ctx = t->ctx;
  const uint64_t bins = (uint64_t)t->n_ref + 1;
  if (first_bin > bins || n_bins > bins - first_bin)
    return fail(ctx, SBH_E_ARG, "sbh_tally_fetch: bins [%llu, +%llu) of %llu", (unsigned long long)first_bin,
                (unsigned long long)n_bins, (unsigned long long)bins);
  int rc = set_device(ctx);
  if (rc) return rc;
  if (flag) HIPCHK(ctx, hipMemcpyAsync(flag, t->totals.p, 8 * FLAG_WORDS, hipMemcpyDeviceToHost, t->st));
  if (ref && n_bins)
    HIPCHK(ctx, hipMemcpyAsync(ref, t->totals.p + FLAG_WORDS + 2 * first_bin, 16 * n_bins, hipMemcpyDeviceToHost, t->st));
  HIPCHK(ctx, hipStreamSynchronize(t->st));
  return SBH_OK;
}

int sbh_tally_add_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                       const sbh_record_filter *filter, int32_t n_ref, uint64_t *flag, uint64_t *ref,
                       sbh_tally_add_result *out, uint64_t *bad_row) {
  static_assert(sizeof(sbh_tally_add_result) == sizeof(sbh_tal::AddResult), "tally_core.h restates the header's layout");
  if ((!flat && flat_size) || (!starts && n) || n_ref < 0 || !flag || !ref || !out) return SBH_E_ARG;
  sbh_bam::Filter F;
  if (!bam_filter_of(filter, &F)) return SBH_E_ARG;
  uint64_t bad = sbh_bam::NO_ROW;
  const int rc = sbh_tal::add_host(flat, flat_size, starts, n, F, n_ref, flag, ref, reinterpret_cast<sbh_tal::AddResult *>(out), &bad);
  return host_rows_status(rc, bad, bad_row);
}

}  // extern "C"
