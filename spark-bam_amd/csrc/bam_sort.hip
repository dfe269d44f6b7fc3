// bam_sort.hip -- the kept rows of a record scan in coordinate order (sbh_records_bam_scan_order with
// SBH_ORDER_COORDINATE): a stable LSD radix sort of (key u64, row u32) pairs, 8 bits a pass.  The
// key is defined in bam_sort_core.h for device and host.
//
//   k_sort_keys     one kept row per lane: key[k], row[k] of the k-th kept row (k_bam_index's rows);
//                   the descents key[k - 1] > key[k], the OR and the AND of all keys into ctr::SORT_*
//   k_sort_hist     per tile of SORT_TILE elements, the count of each digit, digit-major
//                   (cnt[d * n_tiles + tile]): its exclusive scan is every (digit, tile)'s base
//   k_sort_scatter  per tile: a stable rank of each element among the tile's elements of its digit,
//                   then (key, row) to base[d][tile] + rank
//   k_sort_apply    pos'[k] = pos[row[k]], len'[k] = len[row[k]], kh'[k] = 1; entry m closes them
//   k_sort_rows     rows[k] = row[k]: the scan row of the k-th output record
//
// One pass is three launches (histogram, scan_exclusive_u64, scatter); no workgroup waits on
// another inside a kernel.  Both kernels of a pass cut tiles the same way (tile_range).
//
// Stability inside a tile: wave w owns the contiguous slice [w * 64 * SORT_ITEMS, + 64 * SORT_ITEMS)
// of the tile and walks it 64 elements a round, so (wave, round, lane) ascends with the element's
// index.  In a round a lane finds the lanes with its digit by eight ballots; its rank is the
// wave's count of that digit so far (s_cnt[w][d]) + the peers in lower lanes, and the lowest peer
// adds the round's peers to the count.  After the rounds one scan across the waves per digit turns
// s_cnt[w][d] into the elements of digit d in lower waves.
#include <algorithm>

#define SBH_HD __host__ __device__
#include "bam_sort_core.h"
#include "sbh_internal.h"

namespace sbh {
namespace {

using sbh_bam::SORT_ITEMS;
using sbh_bam::SORT_TILE;
using sbh_bam::SORT_WAVES;
constexpr uint32_t SORT_T = SORT_WAVES * 64;  // lanes of a sort workgroup

__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
  for (int m = 1; m < 64; m <<= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, m);
  return v;
}

// rows: k_bam_index's kept rows; kh_total: khpre[n], whose low 32 bits are their count m.  Every
// rows[k], k < m, is a row k_bam_keep found valid, so its 36 fixed bytes lie inside U.
__global__ __launch_bounds__(256) void k_sort_keys(const uint8_t *__restrict__ U, const uint64_t *pos,
                                                   const uint64_t *rows, const uint64_t *kh_total, uint64_t *key,
                                                   uint32_t *row, unsigned long long *acc) {
  __shared__ uint64_t s_red[3][4];
  const uint64_t m = *kh_total & 0xffffffffull;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t desc = 0, any = 0, all = ~0ull;
  // (the loop is uniform in the workgroup, so the shuffle below runs with every lane of the wave)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += step) {
    const uint64_t k = base + threadIdx.x;
    const bool live = k < m;
    uint64_t i = 0, v = 0;
    if (live) {
      i = rows[k], v = sbh_bam::sort_key(U + pos[i]);
      key[k] = v;
      row[k] = (uint32_t)i;
      any |= v;
      all &= v;
    }
    // the key before this one: the lane below holds it, except for a wave's first lane
    uint64_t before = (uint64_t)__shfl_up((unsigned long long)v, 1);
    if (live && k && lane == 0) before = sbh_bam::sort_key(U + pos[rows[k - 1]]);
    if (live && k && before > v) ++desc;
  }
  for (int s = 1; s < 64; s <<= 1) desc += (uint64_t)__shfl_xor((unsigned long long)desc, s);
  any = wave_or(any);
  all = ~wave_or(~all);
  if (lane == 0) s_red[0][wave] = desc, s_red[1][wave] = any, s_red[2][wave] = all;
  __syncthreads();
  if (threadIdx.x == 0) {  // one set of atomics per workgroup: they all meet in three words
    for (uint32_t w = 1; w < 4; ++w) desc += s_red[0][w], any |= s_red[1][w], all &= s_red[2][w];
    if (desc) atomicAdd(acc + 0, (unsigned long long)desc);
    if (any) atomicOr(acc + 1, (unsigned long long)any);
    if (all != ~0ull) atomicAnd(acc + 2, (unsigned long long)all);
  }
}

struct TileRange {
  uint64_t base;
  uint32_t count;
};
__device__ __forceinline__ TileRange tile_range(uint64_t tile, uint64_t m) {
  const uint64_t base = tile * SORT_TILE;
  return TileRange{base, (uint32_t)(m - base < SORT_TILE ? m - base : SORT_TILE)};
}
// the element of (wave, round, lane) within its tile
__device__ __forceinline__ uint32_t tile_slot(uint32_t wave, uint32_t round, uint32_t lane) {
  return wave * 64 * SORT_ITEMS + round * 64 + lane;
}

// grid = n_tiles (tile * SORT_TILE < m).  cnt: 256 * n_tiles words, every one written.
__global__ __launch_bounds__(SORT_T) void k_sort_hist(const uint64_t *key, uint64_t m, uint32_t shift,
                                                     uint64_t n_tiles, uint64_t *cnt) {
  __shared__ uint32_t s_cnt[256];
  const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const TileRange T = tile_range(blockIdx.x, m);
  s_cnt[t] = 0;
  static_assert(SORT_T == 256, "one counter per lane");
  __syncthreads();
  for (uint32_t r = 0; r < SORT_ITEMS; ++r) {
    const uint32_t e = tile_slot(wave, r, lane);
    if (e < T.count) atomicAdd(&s_cnt[(uint32_t)(key[T.base + e] >> shift) & 255u], 1u);
  }
  __syncthreads();
  cnt[(uint64_t)t * n_tiles + blockIdx.x] = s_cnt[t];
}

// base: the exclusive scan of cnt.  Every store index is base[d][tile] + (elements of digit d in
// this tile before this one) < base[d][tile] + cnt[d][tile] <= m; the test against m keeps a store
// inside the arrays whatever the histogram holds.
__global__ __launch_bounds__(SORT_T) void k_sort_scatter(const uint64_t *key, const uint32_t *row, uint64_t m,
                                                        uint32_t shift, uint64_t n_tiles, const uint64_t *base,
                                                        uint64_t *key_out, uint32_t *row_out) {
  __shared__ uint32_t s_cnt[SORT_WAVES * 256];
  __shared__ uint64_t s_base[256];
  const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const TileRange T = tile_range(blockIdx.x, m);
  const uint64_t below = (1ull << lane) - 1;
  for (uint32_t w = 0; w < SORT_WAVES; ++w) s_cnt[w * 256 + t] = 0;
  s_base[t] = base[(uint64_t)t * n_tiles + blockIdx.x];
  __syncthreads();
  uint64_t k[SORT_ITEMS];
  uint32_t rw[SORT_ITEMS], rank[SORT_ITEMS];
  uint32_t *my = s_cnt + wave * 256;  // this wave's counters: no other wave touches them before the barrier
#pragma unroll
  for (uint32_t r = 0; r < SORT_ITEMS; ++r) {
    const uint32_t e = tile_slot(wave, r, lane);
    const bool live = e < T.count;
    k[r] = live ? key[T.base + e] : 0;
    rw[r] = live ? row[T.base + e] : 0;
    const uint32_t d = (uint32_t)(k[r] >> shift) & 255u;
    uint64_t peers = __ballot(live);
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
      const uint64_t has = __ballot((d >> b) & 1u);
      peers &= (d >> b) & 1u ? has : ~has;
    }
    // (a dead lane's peers are the live lanes of digit 0; it neither counts nor stores)
    const uint32_t before = my[d];
    rank[r] = before + (uint32_t)__popcll(peers & below);
    __builtin_amdgcn_wave_barrier();  // every lane has read the count ...
    if (live && !(peers & below)) my[d] = before + (uint32_t)__popcll(peers);
    __builtin_amdgcn_wave_barrier();  // ... and the next round reads what the lowest peer wrote
  }
  __syncthreads();
  {  // digit t: counts per wave -> elements of the digit in lower waves
    uint32_t run = 0;
    for (uint32_t w = 0; w < SORT_WAVES; ++w) {
      const uint32_t c = s_cnt[w * 256 + t];
      s_cnt[w * 256 + t] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < SORT_ITEMS; ++r) {
    const uint32_t e = tile_slot(wave, r, lane);
    const uint32_t d = (uint32_t)(k[r] >> shift) & 255u;
    const uint64_t at = s_base[d] + my[d] + rank[r];
    if (e < T.count && at < m) {
      key_out[at] = k[r];
      row_out[at] = rw[r];
    }
  }
}

// k < m: the permuted starts and lengths, every entry kept; k == m: the closing entries the scans
// and k_bam_heads' caller expect (len'[m] = kh'[m] = 0).  row[k] < n is a row of the scan.
__global__ __launch_bounds__(256) void k_sort_apply(const uint64_t *pos, const uint64_t *len, const uint32_t *row,
                                                    uint64_t m, uint64_t *pos2, uint64_t *len2, uint64_t *kh) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= m; k += step) {
    if (k == m) {
      pos2[k] = 0, len2[k] = 0, kh[k] = 0;
    } else {
      const uint32_t i = row[k];
      pos2[k] = pos[i], len2[k] = len[i], kh[k] = 1;
    }
  }
}

__global__ __launch_bounds__(256) void k_sort_rows(const uint32_t *row, uint64_t m, uint64_t *rows) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += step) rows[k] = row[k];
}

}  // namespace

uint64_t sort_tiles(uint64_t m) { return (m + SORT_TILE - 1) / SORT_TILE; }

// n: the scan's rows (the grid covers that many; only the first khpre[n] & 0xffffffff kept rows are
// touched).  acc: ctr::SORT_DESC, _OR, _AND, preset to 0, 0, ~0.
hipError_t launch_sort_keys(const uint8_t *U, const uint64_t *pos, const uint64_t *rows, const uint64_t *kh_total,
                            uint64_t n, uint64_t *key, uint32_t *row, unsigned long long *acc, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_sort_keys, dim3(rows_grid(n)), dim3(256), 0, st, U, pos, rows, kh_total, key, row, acc);
  return hipGetLastError();
}

// One pass over digit `shift / 8`: hist holds 2 (256 sort_tiles(m) + 1) words, the counts and
// behind them their scan.
hipError_t launch_sort_pass(const uint64_t *key, const uint32_t *row, uint64_t m, uint32_t shift, uint64_t *hist,
                            uint64_t *tmp, uint64_t *key_out, uint32_t *row_out, hipStream_t st) {
  if (!m) return hipSuccess;
  const uint64_t nt = sort_tiles(m), words = 256 * nt + 1;
  uint64_t *cnt = hist, *base = hist + words;
  hipError_t e = hipMemsetAsync(cnt + words - 1, 0, 8, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sort_hist, dim3((uint32_t)nt), dim3(SORT_T), 0, st, key, m, shift, nt, cnt);
  e = scan_exclusive_u64(cnt, base, words, tmp, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sort_scatter, dim3((uint32_t)nt), dim3(SORT_T), 0, st, key, row, m, shift, nt, base, key_out,
                     row_out);
  return hipGetLastError();
}

hipError_t launch_sort_apply(const uint64_t *pos, const uint64_t *len, const uint32_t *row, uint64_t m, uint64_t *pos2,
                             uint64_t *len2, uint64_t *kh, hipStream_t st) {
  hipLaunchKernelGGL(k_sort_apply, dim3(rows_grid(m + 1)), dim3(256), 0, st, pos, len, row, m, pos2, len2, kh);
  return hipGetLastError();
}

hipError_t launch_sort_rows(const uint32_t *row, uint64_t m, uint64_t *rows, hipStream_t st) {
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_sort_rows, dim3(rows_grid(m)), dim3(256), 0, st, row, m, rows);
  return hipGetLastError();
}

}  // namespace sbh
