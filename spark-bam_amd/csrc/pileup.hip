// pileup.hip -- per-base allele counts of a record scan's rows over the spans of an accumulator
// (sbh_records_pileup_add, sbh_pileup_finish).  Channels, the walk, validity, the call byte and
// intervals are defined in pileup_core.h for device and host.
//
//   k_pile_check      one row per lane: row_check, row_keep and, for kept rows, the reference range,
//                     every op code and the query-length sum; a row with more than PILE_LANE_OPS ops
//                     is handed to its wave by ballot (lanes stride the ops, one wave sum).  A keep bit
//                     per row (one ballot word per wave and pass), the smallest bad row and the
//                     smallest row that only runs past the stream (RowMinima, sbh_internal.h; the
//                     host's rows_verdict reads them), n_kept, n_unplaced (block_add: one atomic per
//                     workgroup and counter)
//   k_pile_events     kept rows only.  A lane reads its row's fixed fields, first CIGAR word and span (64
//                     rows at once, handed on by v_readlane as scalars); the wave then takes
//                     its rows one at a time (PILE_GROUP = 64 lanes per read): 64 ops a round, each op's
//                     start on the reference and in the query from a 64-bit wave prefix sum (two 32-bit
//                     DPP scans each), then op by op the lanes take consecutive positions.  The adds of
//                     a workgroup's pass meet in an LDS window of PILE_WINDOW positions (ds_add on
//                     u16 halves) and leave it as one no-return integer atomic per non-zero counter;
//                     what falls outside the window is a global atomic of its own, 64 consecutive
//                     positions a wave-instruction.  The channel totals by ballot counts per wave, one
//                     atomic per workgroup and counter
//   k_pile_calls      one tile of PILE_TILE positions per workgroup: two 16-byte loads per position,
//                     the call bytes (through LDS, stored as u32), and per tile its interval heads,
//                     max depth, nonzero, covered, called and eight channel sums (k_pile_fold folds
//                     them: no workgroup touches a word another one does)
//   (scan)            heads per tile -> the tile's first interval
//   k_pile_intervals  the same tile cut over the call bytes only: a head writes its interval's ref_id
//                     and beg, a tail its end; every beg and end has exactly one writer
#include <algorithm>
#include <vector>

#define SBH_HD __host__ __device__
#include "pileup_core.h"
#include "sbh_host.h"

namespace sbh {
namespace {

using sbh_dep::Span;
using sbh_pile::NCH;
using sbh_pile::PILE_LANE_OPS;
using sbh_pile::PILE_TILE;
constexpr uint32_t TILE_T = 256;
constexpr uint32_t TSTAT = 12;  // per tile: max depth, nonzero, covered, called, eight channel sums
static_assert(PILE_TILE == TILE_T * 4, "a tile is 256 lanes x 4 positions");
static_assert(sbh_pile::PILE_GROUP == 64, "k_pile_events gives a wave to a read");

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
  for (int m = 1; m < 64; m <<= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, m);
    v = o > v ? o : v;
  }
  return v;
}
// v of lane src, src the same in every lane: a scalar, so what is computed from it is uniform
__device__ __forceinline__ uint32_t lane_u32(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }
__device__ __forceinline__ uint64_t lane_u64(uint64_t v, int src) {
  return (uint64_t)lane_u32((uint32_t)v, src) | (uint64_t)lane_u32((uint32_t)(v >> 32), src) << 32;
}

// keep: one u64 per 64 rows, every word below ceil(n / 64) written.  acc: bad, past (preset ~0),
// n_kept, n_unplaced (preset 0).
__global__ __launch_bounds__(256) void k_pile_check(const uint8_t *__restrict__ U, const uint64_t *pos, uint64_t n,
                                                    uint64_t total, sbh_bam::Filter F, int32_t n_ref, uint64_t *keep,
                                                    unsigned long long *acc) {
  __shared__ uint64_t s_red[4];
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t lane = threadIdx.x & 63;
  uint64_t kept = 0, unplaced = 0;
  RowMinima m;
  // (the loop is uniform in the workgroup: the ballots run with every lane of the wave)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += step) {
    const uint64_t i = base + threadIdx.x;
    const uint8_t *r = U;
    bool k = false, is_long = false;
    int32_t ref_id = 0;
    if (i < n) {
      const uint64_t p = pos[i];
      uint64_t bytes = 0;
      const int v = sbh_bam::row_check(U, total, p, &bytes);
      if (v != sbh_bam::ROW_OK) {
        m.refused(i, v == sbh_bam::ROW_PAST);
      } else if (sbh_bam::row_keep(U + p, i, F)) {
        r = U + p;
        ref_id = (int32_t)sbh_bam::ld32(r + 4);
        if (ref_id >= n_ref) m.rejected(i);
        else if (sbh_dep::n_cigar_of(r) > PILE_LANE_OPS) is_long = true;
        else if (sbh_pile::walk_ok(r)) k = true;
        else m.rejected(i);
      }
    }
    // the wave's long rows, one at a time (the mask is the same in every lane: uniform loops)
    for (uint64_t todo = __ballot(is_long); todo; todo &= todo - 1) {
      const int src = __builtin_ctzll(todo);
      const uint8_t *wr = U + (uint64_t)__shfl((unsigned long long)(r - U), src);
      const uint8_t *c = sbh_dep::cigar_of(wr);
      const uint32_t wnc = sbh_dep::n_cigar_of(wr);
      const int64_t ls = sbh_pile::l_seq_of(wr);
      uint64_t qsum = 0;
      bool bad_op = false;
      for (uint32_t j = lane; j < wnc; j += 64) {
        const uint32_t w = sbh_bam::ld32(c + 4 * (uint64_t)j), op = w & 15u;
        bad_op |= op > 8;
        if (sbh_pile::op_query(op)) qsum += w >> 4;
      }
      qsum = wave_sum(qsum);
      const bool ok = __ballot(bad_op) == 0 && (ls == 0 || qsum == (uint64_t)ls);
      if ((int)lane == src) {
        if (ok) k = true;
        else m.rejected(i);
      }
    }
    if (k) {
      ++kept;
      if (ref_id < 0) ++unplaced;
    }
    const uint64_t word = __ballot(k);
    if (lane == 0 && i < n) keep[i >> 6] = word;
  }
  m.send(acc + 0, acc + 1);
  block_add(kept, s_red, acc + 2);
  block_add(unplaced, s_red, acc + 3);
}

// Runs only after k_pile_check found no bad row: every kept row is valid, its CIGAR, SEQ and QUAL
// lie inside its record, its ref_id is below n_ref and its query lengths sum to l_seq.
// counts: 8 S words.  acc: n_counted, then the eight channel totals.
//
// The window.  A workgroup's pass takes 256 consecutive rows; on coordinate-sorted input they pile
// onto a few hundred positions, tens of adds each.  Those adds go to LDS first: PILE_WINDOW
// positions from the pass's first counted row on (its first position inside its span, as an index
// into counts: the window may cross from one span into the next), seven channels as u16 halves of
// four u32 planes s_win[plane][position] (plane = channel / 2; consecutive lanes, consecutive words,
// no bank shared).  An aligned or deleted base adds at most once per row and position, so a half
// holds at most 256 before the flush: no carry into its neighbour.  After the pass every thread
// flushes eight positions: the non-zero halves by global atomics, the words zeroed.  A base outside
// the window (rows far apart: unsorted input, long skips) and every insertion go straight to
// global atomics.
__global__ __launch_bounds__(256) void k_pile_events(const uint8_t *__restrict__ U, const uint64_t *pos, uint64_t n,
                                                     const uint64_t *keep, const Span *sp, const uint64_t *off,
                                                     uint32_t n_spans, uint32_t min_baseq, uint32_t *counts, uint64_t S,
                                                     unsigned long long *acc) {
  constexpr uint32_t W = sbh_pile::PILE_WINDOW;
  static_assert(W % 256 == 0 && W % 64 == 0, "256 threads flush the window; a plane is a multiple of the banks");
  __shared__ uint32_t s_win[4 * W];
  __shared__ uint64_t s_first[4];
  __shared__ uint64_t s_red[4];
  __shared__ uint64_t s_tot[4][NCH];
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t counted = 0, ins = 0;
  uint64_t tot[NCH] = {0, 0, 0, 0, 0, 0, 0, 0};  // the wave's, the same in every lane (INS: see ins)
  for (uint32_t k = threadIdx.x; k < 4 * W; k += 256) s_win[k] = 0;
  // (the loop is uniform in the workgroup: its barriers are met by every wave)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += step) {
    const uint64_t i = base + threadIdx.x;
    const uint8_t *r = U;
    uint64_t o = 0, idx0 = 0;
    int64_t beg = 0, end = 0;
    uint32_t x0 = 0, nc = 0, ls32 = 0, l_name = 0, w0 = 0;  // the row's fixed fields and first CIGAR word
    bool go = false;
    if (i < n && ((keep[i >> 6] >> (i & 63)) & 1)) {
      r = U + pos[i];
      const int32_t ref_id = (int32_t)sbh_bam::ld32(r + 4);
      const uint32_t k = ref_id < 0 ? n_spans : sbh_dep::span_of(sp, n_spans, ref_id);
      if (k < n_spans) {
        go = true;
        ++counted;
        o = off[k], beg = sp[k].beg, end = sp[k].end;
        x0 = sbh_bam::ld32(r + 8), nc = sbh_dep::n_cigar_of(r), ls32 = sbh_bam::ld32(r + 20), l_name = r[12];
        if (nc) w0 = sbh_bam::ld32(sbh_dep::cigar_of(r));
        const int64_t p0 = (int32_t)x0;
        idx0 = o + (uint64_t)((p0 < beg ? beg : p0 < end ? p0 : end - 1) - beg);
      }
    }
    // the window's first position: that of the pass's first counted row (~0: the pass has none)
    const uint64_t todo0 = __ballot(go);
    const uint64_t first = lane_u64(idx0, todo0 ? __builtin_ctzll(todo0) : 0);
    if (lane == 0) s_first[wave] = todo0 ? first : ~0ull;
    __syncthreads();  // (and the window is zero: the loop's head, or the flush before)
    uint64_t wbase = ~0ull;
    for (uint32_t w = 4; w-- > 0;)
      if (s_first[w] != ~0ull) wbase = s_first[w];
    // the wave's rows, one at a time (the mask is the same in every lane: uniform loops)
    for (uint64_t todo = todo0; todo; todo &= todo - 1) {
      const int src = __builtin_ctzll(todo);
      const uint8_t *wr = U + lane_u64((uint64_t)(r - U), src);
      const uint64_t wo = lane_u64(o, src);
      const int64_t wbeg = (int64_t)lane_u64((uint64_t)beg, src), wend = (int64_t)lane_u64((uint64_t)end, src);
      const uint32_t wnc = lane_u32(nc, src), ww0 = lane_u32(w0, src);
      const int64_t ls = (int32_t)lane_u32(ls32, src), pos0 = (int32_t)lane_u32(x0, src);
      const uint8_t *c = wr + 36 + lane_u32(l_name, src), *seq = c + 4 * (uint64_t)wnc, *qual = seq + (ls + 1) / 2;
      int64_t wx = pos0;
      uint64_t wq = 0;
      for (uint32_t b0 = 0; b0 < wnc; b0 += 64) {
        const uint32_t j = b0 + lane;
        // (word 0 came with the row's fixed fields: a one-op row reads no CIGAR here)
        const uint32_t w = j == 0 ? ww0 : j < wnc ? sbh_bam::ld32(c + 4 * (uint64_t)j) : 0u, op = w & 15u, l = w >> 4;
        const uint32_t advx = sbh_dep::op_advances(op) ? l : 0u, advq = sbh_pile::op_query(op) ? l : 0u;
        const uint64_t inclx = wave_incl_scan64(advx), inclq = wave_incl_scan64(advq);
        const int64_t xs = wx + (int64_t)(inclx - advx);
        const uint64_t qs = wq + (inclq - advq);
        // an insertion is its lane's own: one add at the position before it
        if (op == 1 && l >= 1 && xs > pos0 && xs - 1 >= wbeg && xs - 1 < wend) {
          const uint64_t idx = wo + (uint64_t)(xs - 1 - wbeg);
          if (idx < S) {
            atomicAdd(counts + NCH * idx + sbh_pile::CH_INS, 1u);
            ++ins;
          }
        }
        // aligned and deleted stretches, op by op, the lanes on consecutive positions
        for (uint64_t ops = __ballot(l > 0 && (sbh_pile::op_aligned(op) || op == 2)); ops; ops &= ops - 1) {
          const int so = __builtin_ctzll(ops);
          const uint32_t oop = lane_u32(op, so);
          const int64_t ol = (int64_t)lane_u32(l, so), oxs = (int64_t)lane_u64((uint64_t)xs, so);
          const uint64_t oqs = lane_u64(qs, so);
          int64_t a, b;
          if (!sbh_dep::clip(oxs, ol, wbeg, wend, &a, &b)) continue;
          for (int64_t p0 = a; p0 < b; p0 += 64) {
            const int64_t p = p0 + (int64_t)lane;
            uint32_t ch = NCH;  // none
            if (p < b) {
              const uint64_t idx = wo + (uint64_t)(p - wbeg), qi = oqs + (uint64_t)(p - oxs);
              if (oop == 2) ch = sbh_pile::CH_DEL;
              else if (ls == 0) ch = sbh_pile::CH_N;
              else if (qi < (uint64_t)ls) ch = sbh_pile::base_channel(seq, qual, qi, min_baseq);
              const uint64_t rel = idx - wbase;  // (below wbase: wraps to a huge value)
              if (ch >= NCH || idx >= S) ch = NCH;
              else if (rel < W) atomicAdd(&s_win[(ch >> 1) * W + (uint32_t)rel], 1u << (16 * (ch & 1)));
              else atomicAdd(counts + NCH * idx + ch, 1u);
            }
#pragma unroll
            for (uint32_t k = 0; k < NCH; ++k)
              if (k != sbh_pile::CH_INS) tot[k] += (uint64_t)__popcll(__ballot(ch == k));
          }
        }
        wx += (int64_t)lane_u64(inclx, 63);
        wq += lane_u64(inclq, 63);
      }
    }
    __syncthreads();
    // the flush: position wbase + q of the window is counts row wbase + q, tested against S again
    if (wbase != ~0ull) {
      for (uint32_t q = threadIdx.x; q < W; q += 256) {
        const uint32_t v[4] = {s_win[q], s_win[W + q], s_win[2 * W + q], s_win[3 * W + q]};
        if (!(v[0] | v[1] | v[2] | v[3])) continue;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
          if (!v[k]) continue;
          s_win[k * W + q] = 0;
          if (wbase + q >= S) continue;
          if (v[k] & 0xffffu) atomicAdd(counts + NCH * (wbase + q) + 2 * k, v[k] & 0xffffu);
          if (v[k] >> 16) atomicAdd(counts + NCH * (wbase + q) + 2 * k + 1, v[k] >> 16);
        }
      }
    }
    // (the next pass's first barrier orders the zeroed words and s_first's readers before its writers)
    __syncthreads();
  }
  tot[sbh_pile::CH_INS] = wave_sum(ins);
  if (lane == 0) {
#pragma unroll
    for (uint32_t k = 0; k < NCH; ++k) s_tot[wave][k] = tot[k];
  }
  block_add(counted, s_red, acc + 0);  // (its barriers order s_tot as well)
  if (threadIdx.x < NCH) {
    const uint64_t t = s_tot[0][threadIdx.x] + s_tot[1][threadIdx.x] + s_tot[2][threadIdx.x] + s_tot[3][threadIdx.x];
    if (t) atomicAdd(acc + 1 + threadIdx.x, (unsigned long long)t);
  }
}

// ---- the tile kernels ---------------------------------------------------------------------------
// (what a lane needs about the span of a position is a SpanCursor, sbh_internal.h)
__device__ __forceinline__ void load_pos(const uint4 *counts, uint64_t s, uint32_t c[NCH]) {
  const uint4 a = counts[2 * s], b = counts[2 * s + 1];
  c[0] = a.x, c[1] = a.y, c[2] = a.z, c[3] = a.w, c[4] = b.x, c[5] = b.y, c[6] = b.z, c[7] = b.w;
}

// grid = tiles.  counts: 2 S uint4; calls: tiles * PILE_TILE bytes, every one written (0 behind S);
// heads[tile]; tstat: TSTAT n_tiles words, statistic j of the tile at [j n_tiles + tile].
__global__ __launch_bounds__(TILE_T) void k_pile_calls(const uint4 *__restrict__ counts, uint64_t S, const uint64_t *off,
                                                       uint32_t n_spans, uint32_t min_depth, uint32_t call_pct,
                                                       uint8_t *calls, uint64_t *heads, uint64_t *tstat) {
  __shared__ uint32_t s_w[1 + TILE_T];  // byte 3: the call before the tile; bytes 4 ..: the tile's calls
  __shared__ uint64_t s_red[4][TSTAT + 1];
  uint8_t *sb = reinterpret_cast<uint8_t *>(s_w);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t t0 = (uint64_t)blockIdx.x * PILE_TILE;
  uint64_t mx = 0, st[TSTAT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) {
    const uint64_t s = t0 + r * TILE_T + threadIdx.x;
    uint8_t call = 0;
    if (s < S) {
      uint32_t c[NCH];
      load_pos(counts, s, c);
      call = sbh_pile::call_of(c, min_depth, call_pct);
      const uint64_t d = sbh_pile::depth_of(c);
      mx = d > mx ? d : mx;
      st[1] += call != 0;
      st[2] += d != 0;
      st[3] += sbh_pile::is_called(call);
#pragma unroll
      for (uint32_t k = 0; k < NCH; ++k) st[4 + k] += c[k];
    }
    sb[4 + r * TILE_T + threadIdx.x] = call;
  }
  if (threadIdx.x == 0) {
    uint8_t before = 0;
    if (t0) {  // (position t0 - 1 < S: the tile exists)
      uint32_t c[NCH];
      load_pos(counts, t0 - 1, c);
      before = sbh_pile::call_of(c, min_depth, call_pct);
    }
    sb[3] = before;
  }
  __syncthreads();
  const uint32_t word = s_w[1 + threadIdx.x];
  reinterpret_cast<uint32_t *>(calls)[(t0 >> 2) + threadIdx.x] = word;
  uint32_t prev = sb[3 + 4 * threadIdx.x];
  uint64_t nh = 0;
  const uint64_t s0 = t0 + 4 * threadIdx.x;
  if (s0 < S) {
    SpanCursor q = SpanCursor::span_at(off, n_spans, s0);
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
      const uint32_t cb = (word >> (8 * e)) & 0xffu;
      if (s0 + e < S) {
        q.span_to(off, n_spans, s0 + e);
        nh += cb && (s0 + e == q.first || !prev);
      }
      prev = cb;
    }
  }
  st[0] = wave_max(mx);
#pragma unroll
  for (uint32_t k = 1; k < TSTAT; ++k) st[k] = wave_sum(st[k]);
  nh = wave_sum(nh);
  if (lane == 0) {
#pragma unroll
    for (uint32_t k = 0; k < TSTAT; ++k) s_red[wave][k] = st[k];
    s_red[wave][TSTAT] = nh;
  }
  __syncthreads();
  if (threadIdx.x <= TSTAT) {
    const uint32_t k = threadIdx.x;
    uint64_t v = s_red[0][k];
    for (uint32_t w = 1; w < 4; ++w) v = k == 0 ? (s_red[w][k] > v ? s_red[w][k] : v) : v + s_red[w][k];
    if (k == TSTAT) heads[blockIdx.x] = v;
    else tstat[(uint64_t)k * gridDim.x + blockIdx.x] = v;
  }
}

// tstat: k_pile_calls' per-tile statistics (TSTAT nt words) -> acc[TSTAT] (preset 0): the max by
// atomicMax, the rest summed, one atomic per workgroup and counter.
__global__ __launch_bounds__(256) void k_pile_fold(const uint64_t *tstat, uint64_t nt, unsigned long long *acc) {
  __shared__ uint64_t s_red[4];
  __shared__ uint64_t s_max[4];
  uint64_t v[TSTAT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t m = tstat[t];
    v[0] = m > v[0] ? m : v[0];
#pragma unroll
    for (uint32_t k = 1; k < TSTAT; ++k) v[k] += tstat[k * nt + t];
  }
  const uint64_t mx = wave_max(v[0]);
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t m = s_max[0];
    for (uint32_t w = 1; w < 4; ++w) m = s_max[w] > m ? s_max[w] : m;
    if (m) atomicMax(acc + 0, (unsigned long long)m);
  }
#pragma unroll
  for (uint32_t k = 1; k < TSTAT; ++k) block_add(v[k], s_red, acc + k);
}

// calls: the finished bytes (tiles * PILE_TILE of them, 0 behind S); hbase: the exclusive scan of
// heads (the tile's first interval); n_iv: its total.  A head's index is hbase[tile] + (heads before
// it in the tile), a tail's that of the last head at or before it: both below n_iv by construction;
// the test against n_iv keeps a store inside ivals[] whatever the scans hold.
__global__ __launch_bounds__(TILE_T) void k_pile_intervals(const uint8_t *__restrict__ calls, uint64_t S,
                                                           const uint64_t *hbase, const Span *sp, const uint64_t *off,
                                                           uint32_t n_spans, uint64_t n_iv, sbh_depth_span *ivals) {
  __shared__ uint32_t s_w[TILE_T];
  __shared__ uint32_t s_wave[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t t0 = (uint64_t)blockIdx.x * PILE_TILE, s0 = t0 + 4 * threadIdx.x;
  const uint32_t word = reinterpret_cast<const uint32_t *>(calls)[(t0 >> 2) + threadIdx.x];
  s_w[threadIdx.x] = word;
  __syncthreads();
  // the bytes before and behind the lane's four (both inside calls[]: t0 - 1 when t0 > 0, the next
  // tile's first byte when there is a next tile)
  const uint32_t before = threadIdx.x ? s_w[threadIdx.x - 1] >> 24 : (t0 ? calls[t0 - 1] : 0u);
  const uint32_t behind = threadIdx.x + 1 < TILE_T ? s_w[threadIdx.x + 1] & 0xffu
                                                   : (blockIdx.x + 1 < gridDim.x ? calls[t0 + PILE_TILE] : 0u);
  uint32_t hd = 0, tl = 0;
  if (s0 < S) {
    SpanCursor q = SpanCursor::span_at(off, n_spans, s0);
    uint32_t prev = before;
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
      const uint32_t cb = (word >> (8 * e)) & 0xffu, nb = e < 3 ? (word >> (8 * e + 8)) & 0xffu : behind;
      if (s0 + e < S && cb) {
        q.span_to(off, n_spans, s0 + e);
        if (s0 + e == q.first || !prev) hd |= 1u << e;
        if (s0 + e + 1 == q.next || !nb) tl |= 1u << e;
      }
      prev = cb;
    }
  }
  const uint32_t nh = (uint32_t)__popc(hd), incl = wave_incl_scan(nh);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  uint32_t before_waves = 0;
  for (uint32_t w = 0; w < wave; ++w) before_waves += s_wave[w];
  uint64_t rank = hbase[blockIdx.x] + before_waves + incl - nh;  // heads before the lane's positions
  if (hd | tl) {
    SpanCursor q = SpanCursor::span_at(off, n_spans, s0);
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
      if (!(((hd | tl) >> e) & 1u)) continue;
      q.span_to(off, n_spans, s0 + e);
      const int64_t at = sp[q.k].beg + (int64_t)(s0 + e - q.first);
      if ((hd >> e) & 1u) {
        if (rank < n_iv) {
          ivals[rank].ref_id = sp[q.k].ref_id;
          ivals[rank].pad = 0;
          ivals[rank].beg = at;
        }
        ++rank;
      }
      if (((tl >> e) & 1u) && rank && rank - 1 < n_iv) ivals[rank - 1].end = at + 1;
    }
  }
}

uint64_t pile_tiles(uint64_t S) { return (S + PILE_TILE - 1) / PILE_TILE; }

const sbh_dep::Span *pile_spans(const sbh_depth_span *s) {
  static_assert(sizeof(sbh_depth_span) == sizeof(sbh_dep::Span) &&
                    sizeof(sbh_pileup_sizes) == sizeof(sbh_pile::Sizes) &&
                    sizeof(sbh_pileup_add_result) == sizeof(sbh_pile::AddResult),
                "pileup_core.h restates the header's layouts");
  return reinterpret_cast<const sbh_dep::Span *>(s);
}

}  // namespace
}  // namespace sbh

using namespace sbh;

extern "C" {

// ---- the C-ABI's pileup calls (the definition in pileup_core.h) --------------------------------
int sbh_pileup_create(sbh_ctx *ctx, const sbh_depth_span *spans, uint32_t n_spans, int32_t n_ref, int32_t min_baseq,
                      sbh_pileup **out) {
  if (!ctx || !out) return SBH_E_ARG;
  *out = nullptr;
  if (min_baseq < 0 || min_baseq > 255) return fail(ctx, SBH_E_ARG, "pileup: min_baseq %d outside [0, 255]", min_baseq);
  int rc = spans_refused(ctx, "pileup", spans, n_spans, n_ref);
  if (rc) return rc;
  rc = set_device(ctx);
  if (rc) return rc;
  sbh_pileup *p = new sbh_pileup();
  p->ctx = ctx;
  p->n_ref = n_ref;
  p->min_baseq = (uint32_t)min_baseq;
  p->assign(spans, n_spans, 0);
  char nomem[80];
  std::snprintf(nomem, sizeof nomem, "pileup: no memory for %llu positions (33 bytes each)", (unsigned long long)p->S);
  return accum_open(p, out, nomem, "pileup create", [p] {
    const uint64_t nt = pile_tiles(p->S);
    hipError_t e = p->upload(nt, p->st);
    if (e == hipSuccess) e = p->counts.ensure(2 * p->S);
    if (e == hipSuccess) e = p->calls.ensure(nt * PILE_TILE);
    if (e == hipSuccess) e = p->heads.ensure(nt + 1);
    if (e == hipSuccess) e = p->hbase.ensure(nt + 1);
    if (e == hipSuccess) e = p->tstat.ensure(TSTAT * nt);
    if (e == hipSuccess) e = p->tmp.ensure(scan_tmp_words(nt + 1));
    if (e == hipSuccess) e = p->acc.ensure(TSTAT);
    if (e == hipSuccess) e = hipMemsetAsync(p->counts.p, 0, 32 * p->S, p->st);
    return e;
  });
}

int sbh_pileup_destroy(sbh_pileup *p) {
  delete p;  // (~sbh_pileup; a null accumulator is fine)
  return SBH_OK;
}

int sbh_pileup_reset(sbh_pileup *p) {
  if (!p) return SBH_E_ARG;
  int rc = p->reset(p->counts.p, 32 * p->S);
  if (rc) return rc;
  p->finished = false;
  p->sz = sbh_pileup_sizes{};
  return SBH_OK;
}

// k_pile_check, one round trip (bad row, past row, kept, unplaced), then k_pile_events only when no
// row is bad: a failed add has written nothing into the counts.
int sbh_records_pileup_add(sbh_shard *sh, sbh_pileup *p, const sbh_record_filter *filter, sbh_pileup_add_result *out) {
  if (!sh || !p || !out) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &R = sh->rec;
  auto &D = sh->dep;  // (the keep bits of the last depth or pileup add)
  sbh_bam::Filter F;
  int rc = add_begin(sh, p, "records_pileup_add", p->finished ? "after sbh_pileup_finish (sbh_pileup_reset reopens)" : nullptr,
                     filter, &F);
  if (rc) return rc;
  const uint64_t n = R.sz.n;
  *out = sbh_pileup_add_result{};
  out->n = n;
  if (!n) return SBH_OK;
  hipStream_t st = sh->st;
  unsigned long long *acc = sh->ctr.p + ctr::PILE_BAD;
  const AddTrip trip{sh, acc, ctr::PILE_BAD};
  rc = trip.open(&F, &D.keep, ctr::PILE_END - ctr::PILE_BAD - ctr::ADD_A);
  if (rc) return rc;
  hipLaunchKernelGGL(k_pile_check, dim3(rows_grid(n)), dim3(256), 0, st, sh->U.p, R.pos.p, n, sh->utotal, F, p->n_ref,
                     D.keep.p, acc);
  HIPCHK(ctx, hipGetLastError());
  rc = trip.verdict(", or its CIGAR, query length or reference is out of range");
  if (rc) return rc;
  out->n_kept = trip.a();
  out->n_unplaced = trip.b();
  if (out->n_kept > out->n_unplaced) {
    static_assert(ctr::PILE_TOTALS == ctr::PILE_COUNTED + 1 && ctr::PILE_END == ctr::PILE_TOTALS + NCH, "one copy");
    unsigned long long *ev = sh->ctr.p + ctr::PILE_COUNTED;
    hipLaunchKernelGGL(k_pile_events, dim3(rows_grid(n)), dim3(256), 0, st, sh->U.p, R.pos.p, n, D.keep.p,
                       reinterpret_cast<const Span *>(p->d_spans.p), p->d_off.p, (uint32_t)p->spans.size(), p->min_baseq,
                       reinterpret_cast<uint32_t *>(p->counts.p), p->S, ev);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::PILE_COUNTED, ev, 8 * (1 + NCH), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    out->n_counted = sh->h_ctr[ctr::PILE_COUNTED];
    for (uint32_t k = 0; k < NCH; ++k) out->totals[k] = sh->h_ctr[ctr::PILE_TOTALS + k];
  }
  return SBH_OK;
}

int sbh_pileup_finish(sbh_pileup *p, uint32_t min_depth, uint32_t call_pct, sbh_pileup_sizes *out) {
  if (!p || !out) return SBH_E_ARG;
  sbh_ctx *ctx = p->ctx;
  if (min_depth < 1 || call_pct < 1 || call_pct > 100)
    return fail(ctx, SBH_E_ARG, "pileup finish: min_depth >= 1 and call_pct in [1, 100]");
  if (p->finished) return fail(ctx, SBH_E_STATE, "sbh_pileup_finish twice (sbh_pileup_reset reopens)");
  int rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = p->st;
  const uint64_t S = p->S, nt = pile_tiles(S);
  const uint32_t ns = (uint32_t)p->spans.size();
  unsigned long long h[TSTAT + 1] = {};
  HIPCHK(ctx, hipMemsetAsync(p->acc.p, 0, 8 * TSTAT, st));
  HIPCHK(ctx, hipMemsetAsync(p->heads.p + nt, 0, 8, st));
  hipLaunchKernelGGL(k_pile_calls, dim3((uint32_t)nt), dim3(TILE_T), 0, st, p->counts.p, S, p->d_off.p, ns, min_depth,
                     call_pct, p->calls.p, p->heads.p, p->tstat.p);
  hipLaunchKernelGGL(k_pile_fold, dim3((uint32_t)std::min<uint64_t>((nt + 255) / 256, 64)), dim3(256), 0, st, p->tstat.p, nt,
                     p->acc.p);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, scan_exclusive_u64(p->heads.p, p->hbase.p, nt + 1, p->tmp.p, st));
  HIPCHK(ctx, hipMemcpyAsync(h, p->acc.p, 8 * TSTAT, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(h + TSTAT, p->hbase.p + nt, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  // from here on the accumulator is finished: whatever fails below, no add may follow without a reset
  p->finished = true;
  p->sz = sbh_pileup_sizes{};
  p->sz.positions = S, p->sz.n_intervals = h[TSTAT], p->sz.nonzero = h[1], p->sz.covered = h[2], p->sz.n_called = h[3];
  for (uint32_t k = 0; k < NCH; ++k) p->sz.totals[k] = h[4 + k];
  p->sz.max_depth = h[0] > 0xffffffffull ? 0xffffffffu : (uint32_t)h[0];
  const hipError_t e = p->ivals.ensure(p->sz.n_intervals);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    p->sz.n_intervals = 0;
    return fail(ctx, SBH_E_NOMEM, "pileup finish: no memory for %llu intervals", (unsigned long long)h[TSTAT]);
  }
  hipLaunchKernelGGL(k_pile_intervals, dim3((uint32_t)nt), dim3(TILE_T), 0, st, p->calls.p, S, p->hbase.p,
                     reinterpret_cast<const Span *>(p->d_spans.p), p->d_off.p, ns, p->sz.n_intervals, p->ivals.p);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(st));
  *out = p->sz;
  return SBH_OK;
}

int sbh_pileup_counts_fetch(sbh_pileup *p, uint32_t span, uint64_t from, uint64_t n, uint32_t *out) {
  if (!p || (n && !out)) return SBH_E_ARG;
  sbh_ctx *ctx = p->ctx;
  int rc = p->range(ctx, "sbh_pileup_counts_fetch", span, from, n);
  if (rc) return rc;
  rc = set_device(ctx);
  if (rc) return rc;
  // (the device layout is the output's: position-major, eight u32 per position)
  if (n) HIPCHK(ctx, hipMemcpyAsync(out, p->counts.p + 2 * (p->off[span] + from), 32 * n, hipMemcpyDeviceToHost, p->st));
  HIPCHK(ctx, hipStreamSynchronize(p->st));
  return SBH_OK;
}

int sbh_pileup_calls_fetch(sbh_pileup *p, uint32_t span, uint64_t from, uint64_t n, uint8_t *out) {
  if (!p || (n && !out)) return SBH_E_ARG;
  sbh_ctx *ctx = p->ctx;
  if (!p->finished) return fail(ctx, SBH_E_STATE, "sbh_pileup_calls_fetch before sbh_pileup_finish");
  int rc = p->range(ctx, "sbh_pileup_calls_fetch", span, from, n);
  if (rc) return rc;
  rc = set_device(ctx);
  if (rc) return rc;
  if (n) HIPCHK(ctx, hipMemcpyAsync(out, p->calls.p + p->off[span] + from, n, hipMemcpyDeviceToHost, p->st));
  HIPCHK(ctx, hipStreamSynchronize(p->st));
  return SBH_OK;
}

int sbh_pileup_intervals_fetch(sbh_pileup *p, uint64_t first, uint64_t count, sbh_depth_span *out) {
  if (!p || (count && !out)) return SBH_E_ARG;
  sbh_ctx *ctx = p->ctx;
  if (!p->finished) return fail(ctx, SBH_E_STATE, "sbh_pileup_intervals_fetch before sbh_pileup_finish");
  if (first > p->sz.n_intervals || count > p->sz.n_intervals - first)
    return fail(ctx, SBH_E_ARG, "sbh_pileup_intervals_fetch past the intervals");
  int rc = set_device(ctx);
  if (rc) return rc;
  if (count)
    HIPCHK(ctx, hipMemcpyAsync(out, p->ivals.p + first, count * sizeof(sbh_depth_span), hipMemcpyDeviceToHost, p->st));
  HIPCHK(ctx, hipStreamSynchronize(p->st));
  return SBH_OK;
}

const void *sbh_pileup_device_ptr(sbh_pileup *p, uint32_t span) {
  return p && span < p->spans.size() ? p->counts.p + 2 * p->off[span] : nullptr;
}

int sbh_pileup_budget(sbh_ctx *ctx, uint64_t *max_positions) {
  if (!ctx || !max_positions) return SBH_E_ARG;
  int rc = set_device(ctx);
  if (rc) return rc;
  size_t free_b = 0, total_b = 0;
  HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
  *max_positions = (uint64_t)free_b / 4 * 3 / 33;
  return SBH_OK;
}

int sbh_pileup_add_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                        const sbh_record_filter *filter, const sbh_depth_span *spans, uint32_t n_spans, int32_t n_ref,
                        int32_t min_baseq, uint32_t *counts, sbh_pileup_add_result *out, uint64_t *bad_row) {
  if ((!flat && flat_size) || (!starts && n) || !counts || !out || min_baseq < 0 || min_baseq > 255) return SBH_E_ARG;
  sbh_bam::Filter F;
  if (!bam_filter_of(filter, &F) || !sbh_dep::spans_ok(pile_spans(spans), n_spans, n_ref)) return SBH_E_ARG;
  uint64_t bad = sbh_bam::NO_ROW;
  const int rc = sbh_pile::add_host(flat, flat_size, starts, n, F, pile_spans(spans), n_spans, n_ref, (uint32_t)min_baseq,
                                    counts, reinterpret_cast<sbh_pile::AddResult *>(out), &bad);
  return host_rows_status(rc, bad, bad_row);
}

int sbh_pileup_finish_host(const uint32_t *counts, const sbh_depth_span *spans, uint32_t n_spans, uint32_t min_depth,
                           uint32_t call_pct, uint8_t *calls, sbh_depth_span *intervals, uint64_t interval_cap,
                           sbh_pileup_sizes *out) {
  if (!counts || !calls || !out || (interval_cap && !intervals)) return SBH_E_ARG;
  if (min_depth < 1 || call_pct < 1 || call_pct > 100) return SBH_E_ARG;
  if (!sbh_dep::spans_ok(pile_spans(spans), n_spans, 0x7fffffff)) return SBH_E_ARG;
  sbh_pile::finish_host(counts, pile_spans(spans), n_spans, min_depth, call_pct, calls,
                        reinterpret_cast<sbh_dep::Span *>(intervals), interval_cap, reinterpret_cast<sbh_pile::Sizes *>(out));
  return SBH_OK;
}

}  // extern "C"
