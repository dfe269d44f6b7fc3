// depth.hip -- per-base depth of a record scan's rows over the spans of an accumulator
// (sbh_records_depth_add, sbh_depth_finish).  Events, validity and runs are defined in depth_core.h
// for device and host.
//
//   k_depth_check      one row per lane: row_check, row_keep and, for kept rows, the reference range
//                      and every op code; a keep bit per row (one ballot word per wave and pass), the
//                      smallest bad row and the smallest row that only runs past the stream (RowMinima,
//                      sbh_internal.h; the host's rows_verdict reads them), n_kept, n_unplaced (block_add:
//                      one atomic per workgroup and counter)
//   k_depth_events     kept rows only, one row per lane: +1 / -1 into the slots by no-return integer
//                      atomics.  A lane walks up to DEPTH_LANE_OPS ops itself; a row with more is
//                      handed to its wave by ballot, and the wave takes such rows one at a time, 64
//                      ops a round, each op's start from a 64-bit wave prefix sum of the advancing
//                      lengths (two 32-bit scans: the low 16 bits and the rest).  n_counted, cov_bases.
//   k_depth_tile_sums  per tile of DEPTH_TILE slots, their sum
//   (scan)             tile sums -> tile bases
//   k_depth_apply      the same tile cut: in-tile scan + base, depth written in place; per tile its
//                      heads, max, covered, sum (k_depth_stats folds the last three: at most 64
//                      workgroups' atomics meet in the three counters)
//   (scan)             heads per tile -> the tile's first run
//   k_depth_runs       the same tile cut over the finished depth: every head writes its run's
//                      (ref_id, depth, beg) and closes the run before it when that lies in its span;
//                      a span's extra slot closes the span's last run
//
// A finish is three launches and two small scans over the slots (histogram, scan, scatter in the
// shape of DESIGN 15): no workgroup waits on another inside a kernel.
//
// Slot s of a tile belongs to (wave, round, lane, e) with s = tile * DEPTH_TILE + wave * 1024 +
// round * 256 + lane * 4 + e: a lane reads 16 aligned bytes, a wave 1 KiB in a row, and the order
// (wave, round, lane, e) ascends with s, so prefix sums nest: e within the lane, lanes by a DPP wave
// scan, rounds by the wave's running total, waves through LDS.
#include <algorithm>
#include <vector>

#define SBH_HD __host__ __device__
#include "depth_core.h"
#include "sbh_host.h"

namespace sbh {
namespace {

using sbh_dep::DEPTH_LANE_OPS;
using sbh_dep::DEPTH_TILE;
using sbh_dep::Span;
constexpr uint32_t TILE_T = 256, TILE_ROUNDS = 4;
static_assert(DEPTH_TILE == TILE_T * TILE_ROUNDS * 4, "a tile is 4 waves x 4 rounds x 64 lanes x 4 slots");

// keep: one u64 per 64 rows, bit (i & 63) of word i >> 6; every word below ceil(n / 64) is written.
// acc: bad, past (preset ~0), n_kept, n_unplaced (preset 0).
__global__ __launch_bounds__(256) void k_depth_check(const uint8_t *__restrict__ U, const uint64_t *pos, uint64_t n,
                                                     uint64_t total, sbh_bam::Filter F, int32_t n_ref, uint64_t *keep,
                                                     unsigned long long *acc) {
  __shared__ uint64_t s_red[4];
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  uint64_t kept = 0, unplaced = 0;
  RowMinima m;
  // (the loop is uniform in the workgroup: the ballot runs with every lane of the wave)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += step) {
    const uint64_t i = base + threadIdx.x;
    bool k = false;
    if (i < n) {
      const uint64_t p = pos[i];
      uint64_t bytes = 0;
      const int v = sbh_bam::row_check(U, total, p, &bytes);
      if (v != sbh_bam::ROW_OK) {
        m.refused(i, v == sbh_bam::ROW_PAST);
      } else if (sbh_bam::row_keep(U + p, i, F)) {
        const uint8_t *r = U + p;
        const int32_t ref_id = (int32_t)sbh_bam::ld32(r + 4);
        if (ref_id >= n_ref || !sbh_dep::ops_ok(r)) {
          m.rejected(i);
        } else {
          k = true;
          ++kept;
          if (ref_id < 0) ++unplaced;
        }
      }
    }
    const uint64_t word = __ballot(k);
    if ((threadIdx.x & 63) == 0 && i < n) keep[i >> 6] = word;
  }
  m.send(acc + 0, acc + 1);
  block_add(kept, s_red, acc + 2);
  block_add(unplaced, s_red, acc + 3);
}

// +1 at slot off + a - beg, -1 at slot off + b - beg for [x, x + len) cut to [beg, end).  Both
// indices are re-tested against S whatever the record says.
__device__ __forceinline__ uint64_t emit(int32_t *slots, uint64_t S, uint64_t off, int64_t beg, int64_t end, int64_t x,
                                         int64_t len) {
  int64_t a, b;
  if (!sbh_dep::clip(x, len, beg, end, &a, &b)) return 0;
  const uint64_t ia = off + (uint64_t)(a - beg), ib = off + (uint64_t)(b - beg);
  if (ia < S) atomicAdd(slots + ia, 1);
  if (ib < S) atomicAdd(slots + ib, -1);
  return (uint64_t)(b - a);
}

// Runs only after k_depth_check found no bad row: every kept row is valid, its CIGAR words lie
// inside its record and its ref_id is below n_ref.  acc: n_counted, cov_bases.
__global__ __launch_bounds__(256) void k_depth_events(const uint8_t *__restrict__ U, const uint64_t *pos, uint64_t n,
                                                      const uint64_t *keep, const Span *sp, const uint64_t *off,
                                                      uint32_t n_spans, uint32_t flags, int32_t *slots, uint64_t S,
                                                      unsigned long long *acc) {
  __shared__ uint64_t s_red[4];
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t lane = threadIdx.x & 63;
  uint64_t counted = 0, cov = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += step) {
    const uint64_t i = base + threadIdx.x;
    const uint8_t *r = U;
    uint32_t nc = 0;
    uint64_t o = 0;
    int64_t beg = 0, end = 0, x = 0;
    bool go = false;
    if (i < n && ((keep[i >> 6] >> (i & 63)) & 1)) {
      r = U + pos[i];
      const int32_t ref_id = (int32_t)sbh_bam::ld32(r + 4);
      const uint32_t k = ref_id < 0 ? n_spans : sbh_dep::span_of(sp, n_spans, ref_id);
      if (k < n_spans) {
        go = true;
        ++counted;
        nc = sbh_dep::n_cigar_of(r);
        o = off[k], beg = sp[k].beg, end = sp[k].end;
        x = (int32_t)sbh_bam::ld32(r + 8);
      }
    }
    const bool is_long = go && nc > DEPTH_LANE_OPS;
    if (go && !is_long) {
      const uint8_t *c = sbh_dep::cigar_of(r);
      for (uint32_t j = 0; j < nc; ++j) {
        const uint32_t w = sbh_bam::ld32(c + 4 * j), op = w & 15u;
        const int64_t l = w >> 4;
        if (sbh_dep::op_covers(op, flags)) cov += emit(slots, S, o, beg, end, x, l);
        if (sbh_dep::op_advances(op)) x += l;
      }
    }
    // the wave's long rows, one at a time (the mask is the same in every lane: uniform loops)
    for (uint64_t todo = __ballot(is_long); todo; todo &= todo - 1) {
      const int src = __builtin_ctzll(todo);
      const uint8_t *c = sbh_dep::cigar_of(U + (uint64_t)__shfl((unsigned long long)(r - U), src));
      const uint32_t wnc = (uint32_t)__shfl((int)nc, src);
      const uint64_t wo = (uint64_t)__shfl((unsigned long long)o, src);
      const int64_t wbeg = (int64_t)__shfl((long long)beg, src), wend = (int64_t)__shfl((long long)end, src);
      int64_t wx = (int64_t)__shfl((long long)x, src);
      for (uint32_t b0 = 0; b0 < wnc; b0 += 64) {
        const uint32_t j = b0 + lane;
        const uint32_t w = j < wnc ? sbh_bam::ld32(c + 4 * (uint64_t)j) : 0u, op = w & 15u;
        const uint32_t l = w >> 4, adv = sbh_dep::op_advances(op) ? l : 0u;
        const uint64_t incl = wave_incl_scan64(adv);  // (64 lengths below 2^28)
        if (j < wnc && sbh_dep::op_covers(op, flags))
          cov += emit(slots, S, wo, wbeg, wend, wx + (int64_t)(incl - adv), (int64_t)l);
        wx += (int64_t)__shfl((unsigned long long)incl, 63);
      }
    }
  }
  block_add(counted, s_red, acc + 0);
  block_add(cov, s_red, acc + 1);
}

// ---- the tile kernels ---------------------------------------------------------------------------
// the first slot of (wave, round, lane) in its tile
__device__ __forceinline__ uint32_t tile_slot(uint32_t wave, uint32_t round, uint32_t lane) {
  return wave * (DEPTH_TILE / 4) + round * 256 + lane * 4;
}
// v[e] = slot first + e of the tile, 0 at and behind `count` (a slot is read only below the tile's count)
__device__ __forceinline__ void load4(const int32_t *tile, uint32_t first, uint32_t count, uint32_t v[4]) {
  if (first + 4 <= count) {
    const int4 q = *reinterpret_cast<const int4 *>(tile + first);
    v[0] = (uint32_t)q.x, v[1] = (uint32_t)q.y, v[2] = (uint32_t)q.z, v[3] = (uint32_t)q.w;
  } else {
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) v[e] = first + e < count ? (uint32_t)tile[first + e] : 0u;
  }
}
__device__ __forceinline__ uint32_t tile_count(uint64_t tile, uint64_t S) {
  const uint64_t base = tile * DEPTH_TILE;
  return (uint32_t)(S - base < DEPTH_TILE ? S - base : DEPTH_TILE);
}

// x[r]: this lane's total of round r.  Returns in x[r] the sum of everything before (wave, r, lane)
// in the tile (32-bit wrapping), in *total the tile's.  Every lane of the workgroup calls.
__device__ __forceinline__ void tile_excl_scan(uint32_t x[TILE_ROUNDS], uint32_t *s_wave, uint32_t *total) {
  const uint32_t wave = threadIdx.x >> 6;
  uint32_t run = 0;
#pragma unroll
  for (uint32_t r = 0; r < TILE_ROUNDS; ++r) {
    const uint32_t incl = wave_incl_scan(x[r]);
    const uint32_t excl = run + incl - x[r];
    run += (uint32_t)__shfl((int)incl, 63);
    x[r] = excl;
  }
  __syncthreads();  // (s_wave may still be read from the call before)
  if ((threadIdx.x & 63) == 0) s_wave[wave] = run;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t w = 0; w < 4; ++w) {
    if (w < wave) before += s_wave[w];
    all += s_wave[w];
  }
#pragma unroll
  for (uint32_t r = 0; r < TILE_ROUNDS; ++r) x[r] += before;
  *total = all;
}

// grid = tiles.  sums[tile] = the tile's slots added up, sign-extended (the scan adds modulo 2^64).
__global__ __launch_bounds__(TILE_T) void k_depth_tile_sums(const int32_t *slots, uint64_t S, uint64_t *sums) {
  __shared__ uint64_t s_red[4];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t count = tile_count(blockIdx.x, S);
  const int32_t *tile = slots + (uint64_t)blockIdx.x * DEPTH_TILE;
  int64_t sum = 0;
#pragma unroll
  for (uint32_t r = 0; r < TILE_ROUNDS; ++r) {
    uint32_t v[4];
    load4(tile, tile_slot(wave, r, lane), count, v);
    sum += (int64_t)(int32_t)v[0] + (int32_t)v[1] + (int32_t)v[2] + (int32_t)v[3];
  }
  const uint64_t w = wave_sum((uint64_t)sum);
  if (lane == 0) s_red[wave] = w;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// What a lane needs about the spans of its 4 slots is a SpanCursor (sbh_internal.h): a span's last slot
// (s + 1 == next) is its extra slot, and a span may be 2 slots short.
// base: the exclusive scan of the tile sums.  Depth in place; heads[tile]; tstat: 3 n_tiles words,
// the tile's max depth, covered positions and sum of depth at [tile], [n_tiles + tile], [2 n_tiles +
// tile] (k_depth_stats folds them: no workgroup of this kernel touches a word another one does).
__global__ __launch_bounds__(TILE_T) void k_depth_apply(int32_t *slots, uint64_t S, const uint64_t *base,
                                                        const uint64_t *off, uint32_t n_spans, uint64_t *heads,
                                                        uint64_t *tstat) {
  __shared__ uint32_t s_wave[4];
  __shared__ uint64_t s_red[4][4];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t count = tile_count(blockIdx.x, S);
  const uint64_t t0 = (uint64_t)blockIdx.x * DEPTH_TILE;
  int32_t *tile = slots + t0;
  uint32_t v[TILE_ROUNDS][4], x[TILE_ROUNDS];
#pragma unroll
  for (uint32_t r = 0; r < TILE_ROUNDS; ++r) {
    load4(tile, tile_slot(wave, r, lane), count, v[r]);
    x[r] = v[r][0] + v[r][1] + v[r][2] + v[r][3];
  }
  uint32_t total;
  tile_excl_scan(x, s_wave, &total);
  const uint32_t tb = (uint32_t)base[blockIdx.x];  // (depth is the prefix modulo 2^32)
  uint32_t n_heads = 0, covered = 0, mx = 0;  // (at most 16 slots a lane)
  uint64_t sum = 0;
#pragma unroll
  for (uint32_t r = 0; r < TILE_ROUNDS; ++r) {
    const uint32_t first = tile_slot(wave, r, lane);
    if (first >= count) continue;
    const uint64_t s0 = t0 + first;
    SpanCursor q = SpanCursor::span_at(off, n_spans, s0);
    uint32_t d = tb + x[r], out[4];
    if (first + 4 <= count && q.first < s0 && s0 + 4 < q.next) {
      // the four slots lie inside one span, none of them its first or its extra slot
#pragma unroll
      for (uint32_t e = 0; e < 4; ++e) {
        d += v[r][e];
        out[e] = d;
        n_heads += v[r][e] != 0;
        mx = d > mx ? d : mx;
        covered += d != 0;
        sum += d;
      }
    } else {
#pragma unroll
      for (uint32_t e = 0; e < 4; ++e) {
        const uint64_t s = s0 + e;
        d += v[r][e];
        out[e] = d;
        if (first + e >= count) continue;
        q.span_to(off, n_spans, s);
        if (s + 1 == q.next) continue;  // the extra slot
        n_heads += s == q.first || v[r][e] != 0;
        mx = d > mx ? d : mx;
        covered += d != 0;
        sum += d;
      }
    }
    if (first + 4 <= count) {
      *reinterpret_cast<int4 *>(tile + first) = make_int4((int)out[0], (int)out[1], (int)out[2], (int)out[3]);
    } else {
#pragma unroll
      for (uint32_t e = 0; e < 4; ++e)
        if (first + e < count) tile[first + e] = (int32_t)out[e];
    }
  }
  for (int m = 1; m < 64; m <<= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)mx, m);
    mx = o > mx ? o : mx;
  }
  const uint64_t wh = wave_sum(n_heads), wc = wave_sum(covered), ws = wave_sum(sum);
  if (lane == 0) s_red[wave][0] = wh, s_red[wave][1] = wc, s_red[wave][2] = ws, s_red[wave][3] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t h = 0, c = 0, t = 0, m = 0;
    for (uint32_t w = 0; w < 4; ++w) h += s_red[w][0], c += s_red[w][1], t += s_red[w][2], m = s_red[w][3] > m ? s_red[w][3] : m;
    heads[blockIdx.x] = h;
    tstat[blockIdx.x] = m;
    tstat[(uint64_t)gridDim.x + blockIdx.x] = c;
    tstat[2 * (uint64_t)gridDim.x + blockIdx.x] = t;
  }
}

// tstat: k_depth_apply's per-tile max, covered and sum (3 nt words) -> acc: max, covered, sum
// (preset 0), one atomic per workgroup and counter.
__global__ __launch_bounds__(256) void k_depth_stats(const uint64_t *tstat, uint64_t nt, unsigned long long *acc) {
  __shared__ uint64_t s_red[4];
  __shared__ uint64_t s_max[4];
  uint64_t mx = 0, covered = 0, sum = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t m = tstat[t];
    mx = m > mx ? m : mx;
    covered += tstat[nt + t];
    sum += tstat[2 * nt + t];
  }
  for (int m = 1; m < 64; m <<= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)mx, m);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < 4; ++w) mx = s_max[w] > mx ? s_max[w] : mx;
    if (mx) atomicMax(acc + 0, (unsigned long long)mx);
  }
  block_add(covered, s_red, acc + 1);
  block_add(sum, s_red, acc + 2);
}

// depth: the finished array; hbase: the exclusive scan of heads (the tile's first run); n_runs: its
// total.  Every store index is hbase[tile] + (heads before the slot in the tile) [- 1], a rank below
// n_runs by construction; the test against n_runs keeps a store inside runs[] whatever the scans hold.
__global__ __launch_bounds__(TILE_T) void k_depth_runs(const int32_t *depth, uint64_t S, const uint64_t *hbase,
                                                       const Span *sp, const uint64_t *off, uint32_t n_spans,
                                                       uint64_t n_runs, sbh_depth_run *runs) {
  __shared__ uint32_t s_wave[4];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t count = tile_count(blockIdx.x, S);
  const uint64_t t0 = (uint64_t)blockIdx.x * DEPTH_TILE;
  const int32_t *tile = depth + t0;
  uint32_t v[TILE_ROUNDS][4], prev[TILE_ROUNDS], x[TILE_ROUNDS], hd[TILE_ROUNDS];
#pragma unroll
  for (uint32_t r = 0; r < TILE_ROUNDS; ++r) {
    const uint32_t first = tile_slot(wave, r, lane);
    load4(tile, first, count, v[r]);
    // the depth before the lane's first slot: the lane below holds it, lane 0 reads it (slot t0 +
    // first - 1 >= 0 is below S; the array is no longer written)
    prev[r] = (uint32_t)__shfl_up((int)v[r][3], 1);
    if (lane == 0) prev[r] = t0 + first && first < count ? (uint32_t)depth[t0 + first - 1] : 0u;
    hd[r] = 0;
    if (first < count) {
      SpanCursor q = SpanCursor::span_at(off, n_spans, t0 + first);
      uint32_t p = prev[r];
      if (first + 4 <= count && q.first < t0 + first && t0 + first + 4 < q.next) {
        // inside one span, none of the four its first or its extra slot: a head is a change of depth
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
          if (v[r][e] != p) hd[r] |= 1u << e;
          p = v[r][e];
        }
      } else {
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
          const uint64_t s = t0 + first + e;
          if (first + e < count) {
            q.span_to(off, n_spans, s);
            if (s + 1 != q.next && (s == q.first || v[r][e] != p)) hd[r] |= 1u << e;
          }
          p = v[r][e];
        }
      }
    }
    x[r] = (uint32_t)__popc(hd[r]);
  }
  uint32_t total;
  tile_excl_scan(x, s_wave, &total);
  const uint64_t hb = hbase[blockIdx.x];
#pragma unroll
  for (uint32_t r = 0; r < TILE_ROUNDS; ++r) {
    const uint32_t first = tile_slot(wave, r, lane);
    if (first >= count) continue;
    SpanCursor q = SpanCursor::span_at(off, n_spans, t0 + first);
    uint64_t rank = hb + x[r];  // heads before the slot
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
      const uint64_t s = t0 + first + e;
      if (first + e >= count) continue;
      q.span_to(off, n_spans, s);
      const int64_t at = sp[q.k].beg + (int64_t)(s - q.first);
      if (s + 1 == q.next) {  // the extra slot: at == the span's end
        if (rank && rank - 1 < n_runs) runs[rank - 1].end = at;
      } else if ((hd[r] >> e) & 1u) {
        if (s != q.first && rank && rank - 1 < n_runs) runs[rank - 1].end = at;
        if (rank < n_runs) {
          runs[rank].ref_id = sp[q.k].ref_id;
          runs[rank].depth = v[r][e];
          runs[rank].beg = at;
        }
        ++rank;
      }
    }
  }
}

}  // namespace

// The launchers, in the order the entry points below use them.  launch_depth_events: off has
// n_spans + 1 entries, off[n_spans] == S (a SpanTable's d_off, sbh_host.h).  The finish: tile sums
// (depth_tiles(S) words), their exclusive scan as base, launch_depth_apply (heads: depth_tiles(S) + 1
// words, the caller zeroes the last), the scan of heads as hbase, launch_depth_runs.
static uint64_t depth_tiles(uint64_t S) { return (S + DEPTH_TILE - 1) / DEPTH_TILE; }

// keep: ceil(n / 64) words; acc: the head at ctr::DEPTH_BAD (preset ~0, ~0, 0, 0).  F's row ranges
// are device memory.
static hipError_t launch_depth_check(const uint8_t *U, const uint64_t *pos, uint64_t n, uint64_t total, const sbh_bam::Filter &F,
                                     int32_t n_ref, uint64_t *keep, unsigned long long *acc, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_depth_check, dim3(rows_grid(n)), dim3(256), 0, st, U, pos, n, total, F, n_ref, keep, acc);
  return hipGetLastError();
}

// acc: ctr::DEPTH_COUNTED, DEPTH_COV (preset 0)
static hipError_t launch_depth_events(const uint8_t *U, const uint64_t *pos, uint64_t n, const uint64_t *keep,
                                      const sbh_depth_span *spans, const uint64_t *off, uint32_t n_spans, uint32_t flags,
                                      int32_t *slots, uint64_t S, unsigned long long *acc, hipStream_t st) {
  if (!n) return hipSuccess;
  static_assert(sizeof(sbh_depth_span) == sizeof(Span), "one layout");
  hipLaunchKernelGGL(k_depth_events, dim3(rows_grid(n)), dim3(256), 0, st, U, pos, n, keep,
                     reinterpret_cast<const Span *>(spans), off, n_spans, flags, slots, S, acc);
  return hipGetLastError();
}

static hipError_t launch_depth_tile_sums(const int32_t *slots, uint64_t S, uint64_t *sums, hipStream_t st) {
  hipLaunchKernelGGL(k_depth_tile_sums, dim3((uint32_t)depth_tiles(S)), dim3(TILE_T), 0, st, slots, S, sums);
  return hipGetLastError();
}

// tstat: 3 depth_tiles(S) words, every one written; acc: max, covered, sum (preset 0)
static hipError_t launch_depth_apply(int32_t *slots, uint64_t S, const uint64_t *base, const uint64_t *off, uint32_t n_spans,
                                     uint64_t *heads, uint64_t *tstat, unsigned long long *acc, hipStream_t st) {
  const uint64_t nt = depth_tiles(S);
  hipLaunchKernelGGL(k_depth_apply, dim3((uint32_t)nt), dim3(TILE_T), 0, st, slots, S, base, off, n_spans, heads, tstat);
  hipLaunchKernelGGL(k_depth_stats, dim3((uint32_t)std::min<uint64_t>((nt + 255) / 256, 64)), dim3(256), 0, st, tstat, nt,
                     acc);
  return hipGetLastError();
}

static hipError_t launch_depth_runs(const int32_t *depth, uint64_t S, const uint64_t *hbase, const sbh_depth_span *spans,
                                    const uint64_t *off, uint32_t n_spans, uint64_t n_runs, sbh_depth_run *runs,
                                    hipStream_t st) {
  hipLaunchKernelGGL(k_depth_runs, dim3((uint32_t)depth_tiles(S)), dim3(TILE_T), 0, st, depth, S, hbase,
                     reinterpret_cast<const Span *>(spans), off, n_spans, n_runs, runs);
  return hipGetLastError();
}

}  // namespace sbh

using namespace sbh;

extern "C" {

// ---- the C-ABI's per-base depth calls (the definition in depth_core.h) ------------------------
static const sbh_dep::Span *depth_spans(const sbh_depth_span *s) {
  static_assert(sizeof(sbh_depth_span) == sizeof(sbh_dep::Span) && sizeof(sbh_depth_run) == sizeof(sbh_dep::Run) &&
                    sizeof(sbh_depth_sizes) == sizeof(sbh_dep::Sizes) &&
                    sizeof(sbh_depth_add_result) == sizeof(sbh_dep::AddResult),
                "depth_core.h restates the header's layouts");
  return reinterpret_cast<const sbh_dep::Span *>(s);
}

int sbh_depth_create(sbh_ctx *ctx, const sbh_depth_span *spans, uint32_t n_spans, int32_t n_ref, uint32_t flags,
                     sbh_depth **out) {
  if (!ctx || !out) return SBH_E_ARG;
  *out = nullptr;
  if (flags & ~SBH_DEPTH_DEL) return fail(ctx, SBH_E_ARG, "depth: unknown flag bits 0x%x", flags & ~SBH_DEPTH_DEL);
  int rc = spans_refused(ctx, "depth", spans, n_spans, n_ref);
  if (rc) return rc;
  rc = set_device(ctx);
  if (rc) return rc;
  sbh_depth *d = new sbh_depth();
  d->ctx = ctx;
  d->n_ref = n_ref;
  d->flags = flags;
  d->assign(spans, n_spans, 1);
  char nomem[80];
  std::snprintf(nomem, sizeof nomem, "depth: no memory for %llu slots (4 bytes each)", (unsigned long long)d->S);
  return accum_open(d, out, nomem, "depth create", [d] {
    const uint64_t nt = depth_tiles(d->S);
    hipError_t e = d->upload(nt, d->st);
    if (e == hipSuccess) e = d->slots.ensure(d->S);
    for (auto *b : {&d->tsum, &d->tbase, &d->heads, &d->hbase})
      if (e == hipSuccess) e = b->ensure(nt + 1);
    if (e == hipSuccess) e = d->tstat.ensure(3 * nt);
    if (e == hipSuccess) e = d->tmp.ensure(scan_tmp_words(nt + 1));
    if (e == hipSuccess) e = d->acc.ensure(3);
    if (e == hipSuccess) e = hipMemsetAsync(d->slots.p, 0, 4 * d->S, d->st);
    return e;
  });
}

int sbh_depth_destroy(sbh_depth *d) {
  delete d;  // (~sbh_depth; a null accumulator is fine)
  return SBH_OK;
}

int sbh_depth_reset(sbh_depth *d) {
  if (!d) return SBH_E_ARG;
  int rc = d->reset(d->slots.p, 4 * d->S);
  if (rc) return rc;
  d->finished = false;
  d->sz = sbh_depth_sizes{};
  return SBH_OK;
}

// k_depth_check, one round trip (bad row, past row, kept, unplaced), then k_depth_events only when
// no row is bad: a failed add has written nothing into the slots.
int sbh_records_depth_add(sbh_shard *sh, sbh_depth *d, const sbh_record_filter *filter, sbh_depth_add_result *out) {
  if (!sh || !d || !out) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &R = sh->rec;
  auto &D = sh->dep;
  sbh_bam::Filter F;
  int rc = add_begin(sh, d, "records_depth_add", d->finished ? "after sbh_depth_finish (sbh_depth_reset reopens)" : nullptr,
                     filter, &F);
  if (rc) return rc;
  const uint64_t n = R.sz.n;
  *out = sbh_depth_add_result{n, 0, 0, 0, 0};
  if (!n) return SBH_OK;
  hipStream_t st = sh->st;
  unsigned long long *acc = sh->ctr.p + ctr::DEPTH_BAD;
  const AddTrip trip{sh, acc, ctr::DEPTH_BAD};
  rc = trip.open(&F, &D.keep, ctr::DEPTH_END - ctr::DEPTH_BAD - ctr::ADD_A);
  if (rc) return rc;
  HIPCHK(ctx, launch_depth_check(sh->U.p, R.pos.p, n, sh->utotal, F, d->n_ref, D.keep.p, acc, st));
  rc = trip.verdict(", or its CIGAR or reference is out of range");
  if (rc) return rc;
  out->n_kept = trip.a();
  out->n_unplaced = trip.b();
  if (out->n_kept > out->n_unplaced) {
    static_assert(ctr::DEPTH_COV == ctr::DEPTH_COUNTED + 1, "one copy");
    unsigned long long *ev = sh->ctr.p + ctr::DEPTH_COUNTED;
    HIPCHK(ctx, launch_depth_events(sh->U.p, R.pos.p, n, D.keep.p, d->d_spans.p, d->d_off.p, (uint32_t)d->spans.size(),
                                    d->flags, d->slots.p, d->S, ev, st));
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::DEPTH_COUNTED, ev, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    out->n_counted = sh->h_ctr[ctr::DEPTH_COUNTED];
    out->cov_bases = sh->h_ctr[ctr::DEPTH_COV];
  }
  return SBH_OK;
}

int sbh_depth_finish(sbh_depth *d, sbh_depth_sizes *out) {
  if (!d || !out) return SBH_E_ARG;
  sbh_ctx *ctx = d->ctx;
  if (d->finished) return fail(ctx, SBH_E_STATE, "sbh_depth_finish twice (sbh_depth_reset reopens)");
  int rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = d->st;
  const uint64_t S = d->S, nt = depth_tiles(S);
  const uint32_t ns = (uint32_t)d->spans.size();
  unsigned long long h[4] = {0, 0, 0, 0};
  HIPCHK(ctx, hipMemsetAsync(d->acc.p, 0, 24, st));
  HIPCHK(ctx, hipMemsetAsync(d->heads.p + nt, 0, 8, st));
  HIPCHK(ctx, launch_depth_tile_sums(d->slots.p, S, d->tsum.p, st));
  HIPCHK(ctx, scan_exclusive_u64(d->tsum.p, d->tbase.p, nt, d->tmp.p, st));
  HIPCHK(ctx, launch_depth_apply(d->slots.p, S, d->tbase.p, d->d_off.p, ns, d->heads.p, d->tstat.p, d->acc.p, st));
  HIPCHK(ctx, scan_exclusive_u64(d->heads.p, d->hbase.p, nt + 1, d->tmp.p, st));
  HIPCHK(ctx, hipMemcpyAsync(h, d->acc.p, 24, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(h + 3, d->hbase.p + nt, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  // from here on the slots hold depth: whatever fails below, no add may follow without a reset
  d->finished = true;
  d->sz = sbh_depth_sizes{S, h[3], h[1], h[2], (uint32_t)h[0], 0};
  const hipError_t e = d->runs.ensure(d->sz.n_runs);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    d->sz.n_runs = 0;
    return fail(ctx, SBH_E_NOMEM, "depth finish: no memory for %llu runs", (unsigned long long)h[3]);
  }
  HIPCHK(ctx, launch_depth_runs(d->slots.p, S, d->hbase.p, d->d_spans.p, d->d_off.p, ns, d->sz.n_runs, d->runs.p, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  *out = d->sz;
  return SBH_OK;
}

int sbh_depth_fetch(sbh_depth *d, uint32_t span, uint64_t from, uint64_t n, uint32_t *depth) {
  if (!d || (n && !depth)) return SBH_E_ARG;
  sbh_ctx *ctx = d->ctx;
  if (!d->finished) return fail(ctx, SBH_E_STATE, "sbh_depth_fetch before sbh_depth_finish");
  int rc = d->range(ctx, "sbh_depth_fetch", span, from, n);
  if (rc) return rc;
  rc = set_device(ctx);
  if (rc) return rc;
  if (n) HIPCHK(ctx, hipMemcpyAsync(depth, d->slots.p + d->off[span] + from, 4 * n, hipMemcpyDeviceToHost, d->st));
  HIPCHK(ctx, hipStreamSynchronize(d->st));
  return SBH_OK;
}

int sbh_depth_runs_fetch(sbh_depth *d, uint64_t first, uint64_t count, sbh_depth_run *runs) {
  if (!d || (count && !runs)) return SBH_E_ARG;
  sbh_ctx *ctx = d->ctx;
  if (!d->finished) return fail(ctx, SBH_E_STATE, "sbh_depth_runs_fetch before sbh_depth_finish");
  if (first > d->sz.n_runs || count > d->sz.n_runs - first) return fail(ctx, SBH_E_ARG, "sbh_depth_runs_fetch past the runs");
  int rc = set_device(ctx);
  if (rc) return rc;
  if (count)
    HIPCHK(ctx, hipMemcpyAsync(runs, d->runs.p + first, count * sizeof(sbh_depth_run), hipMemcpyDeviceToHost, d->st));
  HIPCHK(ctx, hipStreamSynchronize(d->st));
  return SBH_OK;
}

const void *sbh_depth_device_ptr(sbh_depth *d, uint32_t span) {
  return d && d->finished && span < d->spans.size() ? d->slots.p + d->off[span] : nullptr;
}

uint64_t sbh_depth_slots(const sbh_depth_span *spans, uint32_t n_spans) {
  if (!sbh_dep::spans_ok(depth_spans(spans), n_spans, 0x7fffffff)) return 0;
  return sbh_dep::slots_of(depth_spans(spans), n_spans);
}

int sbh_depth_add_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                       const sbh_record_filter *filter, const sbh_depth_span *spans, uint32_t n_spans, int32_t n_ref,
                       uint32_t flags, int32_t *slots, sbh_depth_add_result *out, uint64_t *bad_row) {
  if ((!flat && flat_size) || (!starts && n) || !slots || !out || (flags & ~SBH_DEPTH_DEL)) return SBH_E_ARG;
  sbh_bam::Filter F;
  if (!bam_filter_of(filter, &F) || !sbh_dep::spans_ok(depth_spans(spans), n_spans, n_ref)) return SBH_E_ARG;
  uint64_t bad = sbh_bam::NO_ROW;
  const int rc = sbh_dep::add_host(flat, flat_size, starts, n, F, depth_spans(spans), n_spans, n_ref, flags, slots,
                                     reinterpret_cast<sbh_dep::AddResult *>(out), &bad);
  return host_rows_status(rc, bad, bad_row);
}

int sbh_depth_finish_host(int32_t *slots, const sbh_depth_span *spans, uint32_t n_spans, sbh_depth_run *runs,
                          uint64_t run_cap, sbh_depth_sizes *out) {
  if (!slots || !out || (run_cap && !runs)) return SBH_E_ARG;
  if (!sbh_dep::spans_ok(depth_spans(spans), n_spans, 0x7fffffff)) return SBH_E_ARG;
  sbh_dep::finish_host(slots, depth_spans(spans), n_spans, reinterpret_cast<sbh_dep::Run *>(runs), run_cap,
                         reinterpret_cast<sbh_dep::Sizes *>(out));
  return SBH_OK;
}

}  // extern "C"
