// stats.hip -- read-level statistics of a record scan's rows into an accumulator
// (sbh_records_stats_add, sbh_stats_fetch).  The tables are defined in stats_core.h for device and
// host.
//
//   k_stats_rows    one row per lane, grid-stride, opened as k_tally_rows is: row_check, row_keep, then
//                   everything that needs only the fixed fields and QUAL[0] -- sn (all of it but
//                   sum_quality), read_len, isize, mapq.  The counters that count rows are ballot +
//                   popcount into wave-uniform registers over the whole loop; the length sums and the
//                   maximum are kept per lane and reduced behind it; the three histograms go to u32 LDS
//                   cells (the bins below STAT_LDS_LENGTHS / STAT_LDS_INSERTS; the others straight to
//                   the staging words), flushed once per workgroup, non-zero cells only.
//   k_stats_bases   the per-base tables -- qual, base -- and what needs every SEQ / QUAL byte anyway: gc
//                   and sn[sum_quality].  (The GC count is the base pass's: the row lane never reads
//                   SEQ.)  A wave takes 64 rows at a time: one row per lane for the verdict, the filter and
//                   the read's descriptor, then one read at a time, consecutive lanes on consecutive
//                   bases -- a wave's adds go to distinct cycles -- with the next read's bytes loaded
//                   before this one's are counted; workgroups of 16 waves gather the adds in a
//                   window of u32 LDS cells (rows below STAT_LDS_CYCLES, quality bins below
//                   STAT_LDS_QUALS) and flush the non-zero cells once.  An add outside the window, and
//                   every add of a read of STAT_LDS_MAX_READ bases or more, goes straight to the
//                   staging words: the answer does not depend on the path a base took.  A row that
//                   fails row_check is skipped here (k_stats_rows reports it, and nothing is committed).
//   k_stats_commit  totals[i] += staging[i] (max for sn[max_length]), launched only when the add's one
//                   round trip found no bad row: a failed add leaves the totals as they were.
//
// No u32 cell wraps within an add.  k_stats_rows: a workgroup sees fewer than 2^32 rows (the
// launcher refuses n >= 2^40) and adds one per row to a cell.  k_stats_bases: a launch covers at most
// STATS_BASE_ROWS = 2^25 rows over STATS_GRID = 512 workgroups -- 64 passes of 16 waves x 64 rows, 2^16
// rows a workgroup; a read in the window
// adds at most STAT_LDS_MAX_READ - 1 < 2^16 to one cell (the overflow row takes every base past C).
// The staging words and the totals are u64.
#include <algorithm>

#define SBH_HD __host__ __device__
#include "stats_core.h"
#include "sbh_host.h"

namespace sbh {
namespace {

using namespace sbh_stat;
// the staging words: bad, past, kept rows, then the tables (sn first: sequences is the counted rows)
constexpr uint32_t ST_BAD = 0, ST_PAST = 1, ST_KEPT = 2, ST_TAB = 3;
constexpr uint32_t STATS_GRID = 512, STATS_WAVES = 16;
constexpr uint64_t STATS_BASE_ROWS = 1ull << 25;
static_assert(STAT_SN == SBH_STATS_SN && STAT_QUALS == SBH_STATS_QUALS, "stats_core.h restates the header's sizes");
static_assert(STATS_BASE_ROWS / STATS_GRID * (STAT_LDS_MAX_READ - 1) < (1ull << 32), "no LDS cell of k_stats_bases wraps");
constexpr uint32_t LDS_QUAL = 2 * STAT_LDS_CYCLES * STAT_LDS_QUALS, LDS_BASE = STAT_LDS_CYCLES * STAT_BASES;
constexpr uint32_t LDS_GC = 2 * STAT_GC_BINS;
static_assert((LDS_QUAL + LDS_BASE + LDS_GC) * 4 <= 65536 && 2 * (LDS_QUAL + LDS_BASE + LDS_GC) * 4 <= 160 * 1024,
              "two workgroups of k_stats_bases -- every wave slot of a CU -- fit its LDS");
// the counters of sn that count rows (sn_rows_of's bits)
constexpr uint32_t SN_ROW_MASK = 0xfffu | 1u << SN_DIFF_CHR;
static_assert(SN_SUPPLEMENTARY == 11, "sn[0 .. 11] count rows");

__global__ __launch_bounds__(256) void k_stats_rows(const uint8_t *__restrict__ U, const uint64_t *pos, uint64_t n,
                                                    uint64_t total, sbh_bam::Filter F, Params P, Layout lay,
                                                    unsigned long long *stage) {
  __shared__ uint32_t s_len[STAT_LDS_LENGTHS], s_ins[3 * STAT_LDS_INSERTS], s_mapq[STAT_MAPQS];
  __shared__ uint64_t s_red[4];
  unsigned long long *tab = stage + ST_TAB;
  for (uint32_t j = threadIdx.x; j < STAT_LDS_LENGTHS; j += 256) s_len[j] = 0;
  for (uint32_t j = threadIdx.x; j < 3 * STAT_LDS_INSERTS; j += 256) s_ins[j] = 0;
  s_mapq[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, C = P.cycles;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  RowMinima m;
  // wave-uniform: 32 bits hold them, as k_tally_rows' (a wave sees at most 64 rows a pass of 262144)
  uint32_t cnt[STAT_SN];
#pragma unroll
  for (uint32_t c = 0; c < STAT_SN; ++c) cnt[c] = 0;
  uint32_t kept = 0;
  uint64_t len_all = 0, len_last = 0, len_mapped = 0, len_max = 0;  // per lane
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += step) {
    const uint64_t i = base + threadIdx.x;
    bool k = false;
    uint32_t rows = 0;
    if (i < n) {
      const uint64_t p = pos[i];
      uint64_t bytes = 0;
      const int v = sbh_bam::row_check(U, total, p, &bytes);
      if (v != sbh_bam::ROW_OK) {
        m.refused(i, v == sbh_bam::ROW_PAST);
      } else if (sbh_bam::row_keep(U + p, i, F)) {
        const uint8_t *r = U + p;
        k = true;
        const uint32_t fl = sbh_bam::ld32(r + 16) >> 16, mapq = r[13];
        const int32_t tid = (int32_t)sbh_bam::ld32(r + 4), mtid = (int32_t)sbh_bam::ld32(r + 24);
        rows = sn_rows_of(fl, mapq, tid, mtid);
        if (counted(fl)) {
          const uint64_t L = (uint64_t)sbh_pile::l_seq_of(r);
          len_all += L;
          if (which_of(fl)) len_last += L;
          len_max = L > len_max ? L : len_max;
          if (!(fl & 0x4u)) {
            len_mapped += L;
            atomicAdd(&s_mapq[mapq], 1u);
          }
          const uint64_t lb = L <= C ? L : (uint64_t)C + 1;  // <= C + 1: inside read_len
          if (lb < STAT_LDS_LENGTHS) atomicAdd(&s_len[lb], 1u);
          else atomicAdd(tab + lay.read_len + lb, 1ull);
          uint32_t bin = 0, col = 0;
          if (isize_slot(fl, tid, mtid, (int32_t)sbh_bam::ld32(r + 8), (int32_t)sbh_bam::ld32(r + 28),
                         (int32_t)sbh_bam::ld32(r + 32), P.max_insert, &bin, &col)) {  // bin <= I, col < 3
            rows |= 1u << (SN_INWARD + col);
            if (bin < STAT_LDS_INSERTS) atomicAdd(&s_ins[3 * bin + col], 1u);
            else atomicAdd(tab + lay.isize + 3 * (uint64_t)bin + col, 1ull);
          }
          if (!L || qual_of(r)[0] == 0xff) rows |= 1u << SN_NO_QUAL;  // (QUAL[0] lies inside the record when L > 0)
        }
      }
    }
    const uint64_t km = __ballot(k);
    if (!km) continue;  // (uniform)
    kept += (uint32_t)__popcll(km);
#pragma unroll
    for (uint32_t c = 0; c < STAT_SN; ++c)
      if ((SN_ROW_MASK | 1u << SN_NO_QUAL | 7u << SN_INWARD) >> c & 1u) cnt[c] += (uint32_t)__popcll(__ballot((rows >> c) & 1u));
  }
  m.send(stage + ST_BAD, stage + ST_PAST);
  if (lane == 0) {
    if (kept) atomicAdd(stage + ST_KEPT, (unsigned long long)kept);
#pragma unroll
    for (uint32_t c = 0; c < STAT_SN; ++c)
      if (cnt[c]) atomicAdd(tab + c, (unsigned long long)cnt[c]);
  }
  block_add(len_all, s_red, tab + SN_TOTAL_LEN);
  block_add(len_all - len_last, s_red, tab + SN_FIRST_LEN);
  block_add(len_last, s_red, tab + SN_LAST_LEN);
  block_add(len_mapped, s_red, tab + SN_BASES_MAPPED);
  for (int s = 1; s < 64; s <<= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)len_max, s);
    len_max = o > len_max ? o : len_max;
  }
  if (lane == 0 && len_max) atomicMax(tab + SN_MAX_LEN, (unsigned long long)len_max);
  __syncthreads();  // every wave's adds into the LDS cells are done
  const uint64_t n_len = (uint64_t)C + 2 < STAT_LDS_LENGTHS ? (uint64_t)C + 2 : STAT_LDS_LENGTHS;
  const uint64_t n_ins = (uint64_t)P.max_insert + 1 < STAT_LDS_INSERTS ? (uint64_t)P.max_insert + 1 : STAT_LDS_INSERTS;
  for (uint32_t j = threadIdx.x; j < n_len; j += 256)
    if (s_len[j]) atomicAdd(tab + lay.read_len + j, (unsigned long long)s_len[j]);
  for (uint32_t j = threadIdx.x; j < 3 * n_ins; j += 256)
    if (s_ins[j]) atomicAdd(tab + lay.isize + j, (unsigned long long)s_ins[j]);
  if (s_mapq[threadIdx.x]) atomicAdd(tab + lay.mapq + threadIdx.x, (unsigned long long)s_mapq[threadIdx.x]);
}

// What a wave of k_stats_bases holds of one read while the read before it is counted: the SEQ byte and
// the quality of bases lane and lane + 64 (a read of up to 128 bases is whole in it).
struct BaseRegs {
  uint32_t s0, q0, s1, q1;
};
__device__ __forceinline__ BaseRegs base_regs(const uint8_t *seq, uint64_t L, uint32_t lane) {
  BaseRegs b{0, 0, 0, 0};
  const uint8_t *qual = seq + (L + 1) / 2;  // row_check: SEQ's (L + 1) / 2 bytes and QUAL's L bytes lie inside the record
  if (lane < L) b.s0 = seq[lane >> 1], b.q0 = qual[lane];
  if ((uint64_t)lane + 64 < L) b.s1 = seq[(lane + 64) >> 1], b.q1 = qual[lane + 64];
  return b;
}

// rows [row0, row1) of the scan, row1 - row0 <= STATS_BASE_ROWS.  A wave takes 64 rows at a time: first
// one row per lane -- the verdict, the filter, and the read's descriptor (where SEQ starts, L, strand,
// fragment, whether QUAL[0] is 0xff), 64 reads' fixed fields in flight at once -- then the reads one
// after another, lane j % 64 on base j, the next read's bytes loaded (base_regs) before this one's are
// counted.
__global__ __launch_bounds__(64 * STATS_WAVES) __attribute__((amdgpu_waves_per_eu(8))) void k_stats_bases(const uint8_t *__restrict__ U, const uint64_t *pos,
                                                                  uint64_t row0, uint64_t row1, uint64_t total,
                                                                  sbh_bam::Filter F, Params P, Layout lay,
                                                                  unsigned long long *stage) {
  __shared__ uint32_t s_qual[LDS_QUAL], s_base[LDS_BASE], s_gc[LDS_GC];
  unsigned long long *tab = stage + ST_TAB;
  for (uint32_t j = threadIdx.x; j < LDS_QUAL; j += 64 * STATS_WAVES) s_qual[j] = 0;
  for (uint32_t j = threadIdx.x; j < LDS_BASE; j += 64 * STATS_WAVES) s_base[j] = 0;
  for (uint32_t j = threadIdx.x; j < LDS_GC; j += 64 * STATS_WAVES) s_gc[j] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, C = P.cycles;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t step = (uint64_t)gridDim.x * STATS_WAVES * 64;
  uint64_t sum_q = 0;  // per lane
  // one base of a read: table row `row` <= C, code < 16, quality q; in_lds: the read is short enough for the window
  auto count = [&](uint32_t row, uint32_t code, uint32_t q, bool rev, uint32_t w, bool has_qual, bool in_lds) {
    const uint32_t ch = base_channel(code, rev);  // < STAT_BASES
    const bool row_in = in_lds && row < STAT_LDS_CYCLES;
    if (row_in) atomicAdd(&s_base[row * STAT_BASES + ch], 1u);
    else atomicAdd(tab + lay.base + (uint64_t)row * STAT_BASES + ch, 1ull);
    if (has_qual) {
      const uint32_t qb = q < STAT_QUALS - 1 ? q : STAT_QUALS - 1;
      sum_q += q;
      if (row_in && qb < STAT_LDS_QUALS) atomicAdd(&s_qual[(w * STAT_LDS_CYCLES + row) * STAT_LDS_QUALS + qb], 1u);
      else atomicAdd(tab + lay.qual + ((uint64_t)w * ((uint64_t)C + 1) + row) * STAT_QUALS + qb, 1ull);
    }
  };
  for (uint64_t batch = row0 + ((uint64_t)blockIdx.x * STATS_WAVES + wave) * 64; batch < row1; batch += step) {  // (wave-uniform)
    // ---- one row per lane: the descriptor of a counted read with L > 0, or len == 0
    const uint64_t i = batch + lane;
    uint64_t at = 0, len = 0;  // SEQ's offset in U, L
    uint32_t meta = 0;         // rev, which << 1, has_qual << 2
    if (i < row1) {
      const uint64_t p = pos[i];
      uint64_t bytes = 0;
      if (sbh_bam::row_check(U, total, p, &bytes) == sbh_bam::ROW_OK && sbh_bam::row_keep(U + p, i, F)) {
        const uint8_t *r = U + p;
        const uint32_t fl = sbh_bam::ld32(r + 16) >> 16;
        const uint64_t L = (uint64_t)sbh_pile::l_seq_of(r);
        if (counted(fl) && L) {
          const uint8_t *seq = sbh_pile::seq_of(r);
          at = (uint64_t)(seq - U), len = L;
          meta = ((fl & 0x10u) ? 1u : 0u) | which_of(fl) << 1 | (seq[(L + 1) / 2] != 0xff ? 4u : 0u);  // (QUAL[0]: L > 0)
        }
      }
    }
    uint64_t todo = __ballot(len != 0);
    if (!todo) continue;  // (uniform)
    // ---- the reads of the batch, one after another; k: the lane that holds the read's descriptor
    auto desc = [&](uint32_t k, uint64_t *a, uint64_t *l, uint32_t *m) {
      *a = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)at, (int)k) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(at >> 32), (int)k) << 32;
      *l = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)len, (int)k);  // (L < 2^31)
      *m = (uint32_t)__builtin_amdgcn_readlane((int)meta, (int)k);
    };
    uint64_t a_cur, L_cur;
    uint32_t m_cur;
    desc((uint32_t)__builtin_ctzll(todo), &a_cur, &L_cur, &m_cur);
    todo &= todo - 1;
    BaseRegs cur = base_regs(U + a_cur, L_cur, lane);
    for (;;) {
      uint64_t a_nxt = 0, L_nxt = 0;
      uint32_t m_nxt = 0;
      BaseRegs nxt{0, 0, 0, 0};
      const bool more = todo != 0;  // (uniform)
      if (more) {
        desc((uint32_t)__builtin_ctzll(todo), &a_nxt, &L_nxt, &m_nxt);
        todo &= todo - 1;
        nxt = base_regs(U + a_nxt, L_nxt, lane);
      }
      const uint64_t L = L_cur;
      const bool rev = m_cur & 1u, has_qual = m_cur & 4u, in_lds = L < STAT_LDS_MAX_READ;
      const uint32_t w = (m_cur >> 1) & 1u;
      // bases lane and lane + 64 from the registers (lane is even exactly when the base index is)
      bool gc0 = false, gc1 = false;
      if (lane < L) {
        const uint32_t code = (lane & 1) ? (cur.s0 & 15u) : (cur.s0 >> 4);
        gc0 = is_gc(code);
        count(cycle_row(lane, L, rev, C), code, cur.q0, rev, w, has_qual, in_lds);
      }
      if ((uint64_t)lane + 64 < L) {
        const uint32_t code = (lane & 1) ? (cur.s1 & 15u) : (cur.s1 >> 4);
        gc1 = is_gc(code);
        count(cycle_row((uint64_t)lane + 64, L, rev, C), code, cur.q1, rev, w, has_qual, in_lds);
      }
      uint64_t g = (uint64_t)__popcll(__ballot(gc0)) + (uint64_t)__popcll(__ballot(gc1));
      if (L > 128) {  // (uniform) the rest of a longer read, from memory
        const uint8_t *seq = U + a_cur, *qual = seq + (L + 1) / 2;
        uint32_t gl = 0;  // per lane: fewer than 2^31 / 64 + 1 bases
        for (uint64_t j = (uint64_t)lane + 128; j < L; j += 64) {
          const uint32_t code = seq_code(seq, j);
          gl += is_gc(code);
          count(cycle_row(j, L, rev, C), code, has_qual ? qual[j] : 0u, rev, w, has_qual, in_lds);
        }
        g += wave_sum((uint64_t)gl);
      }
      if (lane == 0) atomicAdd(&s_gc[w * STAT_GC_BINS + gc_bin(g, L)], 1u);  // g <= L: a bin below STAT_GC_BINS
      if (!more) break;
      a_cur = a_nxt, L_cur = L_nxt, m_cur = m_nxt, cur = nxt;
    }
  }
  sum_q = wave_sum(sum_q);
  if (lane == 0 && sum_q) atomicAdd(tab + SN_SUM_QUAL, (unsigned long long)sum_q);
  __syncthreads();  // every wave's adds into the LDS cells are done
  for (uint32_t j = threadIdx.x; j < LDS_QUAL; j += 64 * STATS_WAVES) {
    const uint32_t v = s_qual[j];
    if (!v) continue;
    const uint32_t qb = j % STAT_LDS_QUALS, wr = j / STAT_LDS_QUALS, row = wr % STAT_LDS_CYCLES, w = wr / STAT_LDS_CYCLES;
    // a non-zero cell was added to by a base of table row `row` <= C
    atomicAdd(tab + lay.qual + ((uint64_t)w * ((uint64_t)C + 1) + row) * STAT_QUALS + qb, (unsigned long long)v);
  }
  for (uint32_t j = threadIdx.x; j < LDS_BASE; j += 64 * STATS_WAVES)
    if (s_base[j]) atomicAdd(tab + lay.base + j, (unsigned long long)s_base[j]);  // (the same row-major order)
  for (uint32_t j = threadIdx.x; j < LDS_GC; j += 64 * STATS_WAVES)
    if (s_gc[j]) atomicAdd(tab + lay.gc + j, (unsigned long long)s_gc[j]);
}

// totals[i] += staged[i] for i < m (sn[max_length]: the larger): one lane per word, no word is
// touched by two
__global__ __launch_bounds__(256) void k_stats_commit(unsigned long long *totals, const unsigned long long *staged,
                                                      uint64_t m) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long v = staged[i];
    if (i == SN_MAX_LEN) totals[i] = v > totals[i] ? v : totals[i];
    else if (v) totals[i] += v;
  }
}

}  // namespace

// stage: the accumulator's ST_TAB + words staging words, preset by the caller (~0, ~0, then zeros)
static hipError_t launch_stats_add(const uint8_t *U, const uint64_t *pos, uint64_t n, uint64_t total, const sbh_bam::Filter &F,
                                   const Params &P, unsigned long long *stage, hipStream_t st) {
  if (!n) return hipSuccess;
  if (n >> 40) return hipErrorInvalidValue;  // (k_stats_rows' 32-bit cells; no memory holds 2^40 records)
  const Layout lay = layout_of(P);
  hipLaunchKernelGGL(k_stats_rows, dim3(rows_grid(n)), dim3(256), 0, st, U, pos, n, total, F, P, lay, stage);
  hipError_t e = hipGetLastError();
  for (uint64_t a = 0; a < n && e == hipSuccess; a += STATS_BASE_ROWS) {
    const uint64_t b = std::min(n, a + STATS_BASE_ROWS), g = (b - a + STATS_WAVES * 64 - 1) / (STATS_WAVES * 64);
    hipLaunchKernelGGL(k_stats_bases, dim3((uint32_t)std::min<uint64_t>(g, STATS_GRID)), dim3(64 * STATS_WAVES), 0, st, U, pos,
                       a, b, total, F, P, lay, stage);
    e = hipGetLastError();
  }
  return e;
}

static hipError_t launch_stats_commit(unsigned long long *totals, const unsigned long long *staged, uint64_t m,
                                      hipStream_t st) {
  hipLaunchKernelGGL(k_stats_commit, dim3(rows_grid(m)), dim3(256), 0, st, totals, staged, m);
  return hipGetLastError();
}

}  // namespace sbh

using namespace sbh;

extern "C" {

// ---- the C-ABI's stats calls (the definition in stats_core.h) ---------------------------------
int sbh_stats_create(sbh_ctx *ctx, const sbh_stats_params *params, sbh_stats **out) {
  static_assert(sizeof(sbh_stats_params) == sizeof(sbh_stat::Params), "stats_core.h restates the header's layout");
  if (!ctx || !out) return SBH_E_ARG;
  *out = nullptr;
  if (!params) return fail(ctx, SBH_E_ARG, "stats: no parameters");
  const sbh_stat::Params P{params->cycles, params->max_insert};
  if (!sbh_stat::params_ok(P))
    return fail(ctx, SBH_E_ARG, "stats: cycles %u outside [1, %u] or max_insert %u outside [1, %u]", P.cycles,
                sbh_stat::STAT_CYCLES_MAX, P.max_insert, sbh_stat::STAT_INSERT_MAX);
  int rc = set_device(ctx);
  if (rc) return rc;
  sbh_stats *s = new sbh_stats();
  s->ctx = ctx;
  s->params = *params;
  s->words = sbh_stat::layout_of(P).words;
  char nomem[80];
  std::snprintf(nomem, sizeof nomem, "stats: no memory for the tables of %u cycles", P.cycles);
  return accum_open(s, out, nomem, "stats create", [s] {
    hipError_t e = s->stage.ensure(ST_TAB + s->words);
    if (e == hipSuccess) e = s->totals.ensure(s->words);
    if (e == hipSuccess) e = hipMemsetAsync(s->totals.p, 0, 8 * s->words, s->st);
    return e;
  });
}

int sbh_stats_destroy(sbh_stats *s) {
  delete s;  // (~sbh_stats; a null accumulator is fine)
  return SBH_OK;
}

int sbh_stats_reset(sbh_stats *s) { return s ? s->reset(s->totals.p, 8 * s->words) : SBH_E_ARG; }

// Two memsets, k_stats_rows, k_stats_bases (one launch per 2^25 rows), one round trip (bad row, past
// row, kept rows, counted rows), then k_stats_commit only when no row is bad: a failed add has
// written nothing into the totals.
int sbh_records_stats_add(sbh_shard *sh, sbh_stats *s, const sbh_record_filter *filter, sbh_stats_add_result *out) {
  if (!sh || !s || !out) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &R = sh->rec;
  sbh_bam::Filter F;
  int rc = add_begin(sh, s, "records_stats_add", nullptr, filter, &F);
  if (rc) return rc;
  const uint64_t n = R.sz.n;
  *out = sbh_stats_add_result{n, 0, 0};
  if (!n) return SBH_OK;
  hipStream_t st = sh->st;
  // the head: bad, past, kept, counted -- sn[sequences], the first word of the tables
  static_assert(ST_BAD == ctr::ADD_BAD && ST_PAST == ctr::ADD_PAST && ST_KEPT == ctr::ADD_A &&
                    ST_TAB + sbh_stat::SN_SEQUENCES == ctr::ADD_B,
                "the staging words open with the head");
  const sbh_stat::Params P{s->params.cycles, s->params.max_insert};
  const AddTrip trip{sh, s->stage.p, ctr::H_STAGE_HEAD};
  rc = trip.open(&F, nullptr, 1 + s->words);
  if (rc) return rc;
  HIPCHK(ctx, launch_stats_add(sh->U.p, R.pos.p, n, sh->utotal, F, P, s->stage.p, st));
  rc = trip.verdict("");
  if (rc) return rc;
  out->n_kept = trip.a();
  out->n_counted = trip.b();
  if (out->n_kept) {
    HIPCHK(ctx, launch_stats_commit(s->totals.p, s->stage.p + ST_TAB, s->words, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  return SBH_OK;
}

int sbh_stats_fetch(sbh_stats *s, uint64_t *sn, uint64_t *read_len, uint64_t *qual, uint64_t *base, uint64_t *gc,
                    uint64_t *isize, uint64_t *mapq) {
  if (!s) return SBH_E_ARG;
  sbh_ctx *ctx = s->ctx;
  int rc = set_device(ctx);
  if (rc) return rc;
  const sbh_stat::Layout l = sbh_stat::layout_of(sbh_stat::Params{s->params.cycles, s->params.max_insert});
  const struct {
    uint64_t *dst, at, end;
  } part[7] = {{sn, 0, l.read_len}, {read_len, l.read_len, l.qual}, {qual, l.qual, l.base}, {base, l.base, l.gc},
               {gc, l.gc, l.isize}, {isize, l.isize, l.mapq}, {mapq, l.mapq, l.words}};
  for (const auto &p : part)
    if (p.dst) HIPCHK(ctx, hipMemcpyAsync(p.dst, s->totals.p + p.at, 8 * (p.end - p.at), hipMemcpyDeviceToHost, s->st));
  HIPCHK(ctx, hipStreamSynchronize(s->st));
  return SBH_OK;
}

int sbh_stats_add_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                       const sbh_record_filter *filter, const sbh_stats_params *params, uint64_t *sn, uint64_t *read_len,
                       uint64_t *qual, uint64_t *base, uint64_t *gc, uint64_t *isize, uint64_t *mapq,
                       sbh_stats_add_result *out, uint64_t *bad_row) {
  static_assert(sizeof(sbh_stats_add_result) == sizeof(sbh_stat::AddResult), "stats_core.h restates the header's layout");
  if ((!flat && flat_size) || (!starts && n) || !params || !sn || !read_len || !qual || !base || !gc || !isize || !mapq || !out)
    return SBH_E_ARG;
  const sbh_stat::Params P{params->cycles, params->max_insert};
  sbh_bam::Filter F;
  if (!sbh_stat::params_ok(P) || !bam_filter_of(filter, &F)) return SBH_E_ARG;
  uint64_t bad = sbh_bam::NO_ROW;
  const int rc = sbh_stat::add_host(flat, flat_size, starts, n, F, P, sbh_stat::Tables{sn, read_len, qual, base, gc, isize, mapq},
                                    reinterpret_cast<sbh_stat::AddResult *>(out), &bad);
  return host_rows_status(rc, bad, bad_row);
}

}  // extern "C"
