// bam_name.hip -- the kept rows of a record scan in read-name order (sbh_records_bam_scan_names): the
// key is the name padded to 256 bytes, 32 chunks of 8 bytes, then a 4-bit tie (bam_name_core.h holds
// the definition for device and host).  The sort is LSD over chunks: the tie first, then the chunks
// from the last one a name reaches down to chunk 0, each a run of bam_sort.hip's stable 8-bit passes
// over (key u64, row u32) -- so the chunk sorted last is the most significant.  The row array
// travels through the scatters; only the key array is refilled between chunks.
//
//   k_name_scan    one kept row per lane: row[k] of the k-th kept row (k_bam_index's rows); the
//                  descents name_cmp(row k - 1, row k) > 0, the OR and the AND of every chunk and of the
//                  tie, the longest and the shortest name -- into the shard's name words (nacc::)
//   k_name_keys    key[k] = name_chunk(U + pos[row[k]], c) in the current order (c == NAME_CHUNKS: the tie)
//   k_name_groups  over the rows in their final order: groups of one name, and those of 1, 2, more rows
//
// Bounds of every index: k < m <= n (m = the kept rows, khpre[n] & 0xffffffff); rows[k] and row[k]
// < n are rows k_bam_keep found valid, so with r = U + pos[row] the 36 fixed bytes and the name bytes
// at < r + 36 + l_read_name <= r + 4 + block_size <= U + utotal are resident; a chunk index is < 32
// (8 c < L <= 254), the LDS words are [wave < 4][chunk < 32].  No workgroup waits on another.
#define SBH_HD __host__ __device__
#include "bam_name_core.h"
#include "sbh_internal.h"

namespace sbh {
namespace {

using sbh_bam::NAME_CHUNKS;

__device__ __forceinline__ uint64_t wave_or64(uint64_t v) {
  for (int m = 1; m < 64; m <<= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, m);
  return v;
}
__device__ __forceinline__ uint32_t wave_max32(uint32_t v) {
  for (int m = 1; m < 64; m <<= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, m);
    v = v > o ? v : o;
  }
  return v;
}

// rows, kh_total: as k_sort_keys takes them.  acc: the nacc:: words, preset (0 below nacc::ONES, ~0
// from there).  A chunk's AND is reduced over the rows of the waves whose longest name of that round
// reaches the chunk; every other row is shorter than 8 c + 1 bytes, its chunk is 0, and the host
// clears the AND of every chunk the shortest name does not reach (name_and_fix) -- which covers them.
__global__ __launch_bounds__(256) void k_name_scan(const uint8_t *__restrict__ U, const uint64_t *pos,
                                                   const uint64_t *rows, const uint64_t *kh_total, uint32_t *row,
                                                   unsigned long long *acc) {
  __shared__ uint64_t s_or[4][NAME_CHUNKS], s_and[4][NAME_CHUNKS], s_misc[4][5];
  const uint64_t m = *kh_total & 0xffffffffull;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < NAME_CHUNKS) s_or[wave][lane] = 0, s_and[wave][lane] = ~0ull;  // (its own wave's words)
  uint64_t desc = 0;
  uint32_t max_l = 0, min_l = ~0u, tie_or = 0, tie_and = ~0u;
  // (the loop is uniform in the workgroup, so the shuffles below run with every lane of the wave)
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += step) {
    const uint64_t k = base + threadIdx.x;
    const bool live = k < m;
    uint64_t i = 0;
    uint32_t L = 0;
    const uint8_t *r = U;
    if (live) {
      i = rows[k], r = U + pos[i];
      row[k] = (uint32_t)i;
      L = sbh_bam::name_len(r);
      const uint32_t t = sbh_bam::name_tie(r);
      tie_or |= t, tie_and &= t;
      max_l = max_l > L ? max_l : L;
      min_l = min_l < L ? min_l : L;
    }
    // the row before this one: the lane below holds it, except for a wave's first lane
    uint64_t before = (uint64_t)__shfl_up((unsigned long long)i, 1);
    if (live && k && lane == 0) before = rows[k - 1];
    if (live && k && sbh_bam::name_cmp(U + pos[before], r) > 0) ++desc;
    const uint32_t n_chunks = (wave_max32(L) + 7) / 8;  // <= 32; the same in every lane of the wave
    for (uint32_t c = 0; c < n_chunks; ++c) {
      const uint64_t v = live ? sbh_bam::name_chunk(r, c) : 0;
      const uint64_t any = wave_or64(v), all = ~wave_or64(live ? ~v : 0);
      if (lane == 0) s_or[wave][c] |= any, s_and[wave][c] &= all;
    }
  }
  desc = wave_sum(desc);
  max_l = wave_max32(max_l);
  min_l = ~wave_max32(~min_l);
  tie_or = (uint32_t)wave_or64(tie_or);
  tie_and = ~(uint32_t)wave_or64((uint32_t)~tie_and);
  if (lane == 0)
    s_misc[wave][0] = desc, s_misc[wave][1] = max_l, s_misc[wave][2] = min_l, s_misc[wave][3] = tie_or,
    s_misc[wave][4] = tie_and;
  __syncthreads();
  // one set of atomics per workgroup, and only for the chunks below its own longest name
  for (uint32_t w = 0; w < 4; ++w) max_l = max_l > (uint32_t)s_misc[w][1] ? max_l : (uint32_t)s_misc[w][1];
  if (threadIdx.x < NAME_CHUNKS && 8 * threadIdx.x < max_l) {
    const uint32_t c = threadIdx.x;
    uint64_t any = 0, all = ~0ull;
    for (uint32_t w = 0; w < 4; ++w) any |= s_or[w][c], all &= s_and[w][c];
    if (any) atomicOr(acc + nacc::OR + c, (unsigned long long)any);
    if (all != ~0ull) atomicAnd(acc + nacc::AND + c, (unsigned long long)all);
  }
  if (threadIdx.x == 64) {
    desc = 0, min_l = ~0u, tie_or = 0, tie_and = ~0u;
    for (uint32_t w = 0; w < 4; ++w) {
      desc += s_misc[w][0];
      min_l = min_l < (uint32_t)s_misc[w][2] ? min_l : (uint32_t)s_misc[w][2];
      tie_or |= (uint32_t)s_misc[w][3], tie_and &= (uint32_t)s_misc[w][4];
    }
    if (desc) atomicAdd(acc + nacc::DESC, (unsigned long long)desc);
    if (max_l) atomicMax(acc + nacc::MAX_L, (unsigned long long)max_l);
    if (min_l != ~0u) atomicMin(acc + nacc::MIN_L, (unsigned long long)min_l);
    if (tie_or) atomicOr(acc + nacc::TIE_OR, (unsigned long long)tie_or);
    if (tie_and != ~0u) atomicAnd(acc + nacc::TIE_AND, (unsigned long long)tie_and);
  }
}

// c < NAME_CHUNKS: that chunk; c == NAME_CHUNKS: the tie.  row[k] < n, k < m.
__global__ __launch_bounds__(256) void k_name_keys(const uint8_t *__restrict__ U, const uint64_t *pos,
                                                   const uint32_t *row, uint64_t m, uint32_t c, uint64_t *key) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += step) {
    const uint8_t *r = U + pos[row[k]];
    key[k] = c < NAME_CHUNKS ? sbh_bam::name_chunk(r, c) : (uint64_t)sbh_bam::name_tie(r);
  }
}

// row k starts a group when k == 0 or its name differs from row k - 1's; k >= m counts as a start
__device__ __forceinline__ bool group_head(const uint8_t *U, const uint64_t *pos, const uint32_t *row, uint64_t m,
                                           uint64_t k) {
  return k >= m || k == 0 || sbh_bam::name_cmp_names(U + pos[row[k - 1]], U + pos[row[k]]) != 0;
}

// A head at k owns a group of 1 when k + 1 is a start, of 2 when k + 2 is the next start, of more
// otherwise: the two starts after a lane come from the wave's ballot, and the wave's last two lanes
// compare for themselves.  out: n_names, n_single, n_pair, n_more (zero before the launch).
__global__ __launch_bounds__(256) void k_name_groups(const uint8_t *__restrict__ U, const uint64_t *pos,
                                                     const uint32_t *row, uint64_t m, unsigned long long *out) {
  __shared__ uint64_t s_red[4];
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t lane = threadIdx.x & 63;
  uint64_t names = 0, single = 0, pair = 0, more = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += step) {
    const uint64_t k = base + threadIdx.x;
    const bool h = group_head(U, pos, row, m, k);
    const uint64_t heads = __ballot(h);
    if (k < m && h) {
      const bool h1 = lane < 63 ? (heads >> (lane + 1)) & 1 : group_head(U, pos, row, m, k + 1);
      const bool h2 = h1 || (lane < 62 ? (heads >> (lane + 2)) & 1 : group_head(U, pos, row, m, k + 2));
      ++names;
      if (h1) ++single;
      else if (h2) ++pair;
      else ++more;
    }
  }
  block_add(names, s_red, out + 0);
  block_add(single, s_red, out + 1);
  block_add(pair, s_red, out + 2);
  block_add(more, s_red, out + 3);
}

}  // namespace

// n: the scan's rows (the grid covers that many; only the first khpre[n] & 0xffffffff kept rows are touched)
hipError_t launch_name_scan(const uint8_t *U, const uint64_t *pos, const uint64_t *rows, const uint64_t *kh_total,
                            uint64_t n, uint32_t *row, unsigned long long *acc, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_name_scan, dim3(rows_grid(n)), dim3(256), 0, st, U, pos, rows, kh_total, row, acc);
  return hipGetLastError();
}

hipError_t launch_name_keys(const uint8_t *U, const uint64_t *pos, const uint32_t *row, uint64_t m, uint32_t c,
                            uint64_t *key, hipStream_t st) {
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_name_keys, dim3(rows_grid(m)), dim3(256), 0, st, U, pos, row, m, c, key);
  return hipGetLastError();
}

hipError_t launch_name_groups(const uint8_t *U, const uint64_t *pos, const uint32_t *row, uint64_t m,
                              unsigned long long *out, hipStream_t st) {
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_name_groups, dim3(rows_grid(m)), dim3(256), 0, st, U, pos, row, m, out);
  return hipGetLastError();
}

}  // namespace sbh
