// bam_gather.hip -- selected rows of a record scan laid out as one BAM stream (sbh_records_bam_scan).
// The row's validity and the predicate are defined in bam_gather_core.h for device and host.
//
//   k_bam_keep   one row per lane: validate, apply the predicate; len[i] = kept ? 4 + block_size : 0
//   k_bam_heads  kh[i] = keep | head << 32: a kept row starts a RUN unless the row before it is kept
//                too and ends exactly where this one starts in U (tested, not assumed from order)
//   (scans)      len -> off, kh -> khpre (kept rows before i | runs before i << 32)
//   k_bam_index  rec_off / rows per kept row, (dst, src) per run, the closing entries
//   k_bam_copy   one 16-byte-aligned granule of the OUTPUT per lane
#include <algorithm>

#define SBH_HD __host__ __device__
#include "bam_gather_core.h"
#include "sbh_internal.h"

namespace sbh {
namespace {

constexpr uint32_t KEEP_GRID = 1024;             // k_bam_keep / _heads / _index: 262144 rows a pass
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

uint32_t rows_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + 255) / 256, KEEP_GRID); }

}  // namespace

// len, kh: n + 1 words (the caller zeroes entry n); bad, past preset to ~0
hipError_t launch_bam_keep(const uint8_t *U, const uint64_t *pos, uint64_t n, uint64_t total, uint32_t flag_require,
                           uint32_t flag_exclude, int32_t min_mapq, const uint64_t *row_begin, const uint64_t *row_end,
                           uint64_t n_row_ranges, uint64_t *len, uint64_t *kh, unsigned long long *bad,
                           unsigned long long *past, hipStream_t st) {
  if (!n) return hipSuccess;
  const sbh_bam::Filter F{flag_require, flag_exclude, min_mapq, row_begin, row_end, n_row_ranges};
  hipLaunchKernelGGL(k_bam_keep, dim3(rows_grid(n)), dim3(256), 0, st, U, pos, n, total, F, len, kh, bad, past);
  hipLaunchKernelGGL(k_bam_heads, dim3(rows_grid(n)), dim3(256), 0, st, pos, len, n, kh);
  return hipGetLastError();
}

// k_bam_heads alone, over rows whose len and keep flags (kh) are already there (the sorted rows)
hipError_t launch_bam_heads(const uint64_t *pos, const uint64_t *len, uint64_t n, uint64_t *kh, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_bam_heads, dim3(rows_grid(n)), dim3(256), 0, st, pos, len, n, kh);
  return hipGetLastError();
}

// off, khpre: the exclusive scans of len and kh over n + 1 entries
hipError_t launch_bam_index(const uint64_t *pos, const uint64_t *off, const uint64_t *kh, const uint64_t *khpre,
                            uint64_t n, uint64_t head_bytes, uint64_t *rec_off, uint64_t *rows, uint64_t *run_dst,
                            uint64_t *run_src, hipStream_t st) {
  hipLaunchKernelGGL(k_bam_index, dim3(rows_grid(n + 1)), dim3(256), 0, st, pos, off, kh, khpre, n, head_bytes, rec_off,
                     rows, run_dst, run_src);
  return hipGetLastError();
}

hipError_t launch_bam_copy(const uint8_t *U, const uint64_t *run_dst, const uint64_t *run_src, uint64_t n_runs,
                           uint64_t head_bytes, uint64_t bytes, uint8_t *out, hipStream_t st) {
  if (!n_runs || bytes <= head_bytes) return hipSuccess;
  const uint64_t tiles = ((bytes + 15) / 16 - head_bytes / 16 + COPY_T - 1) / COPY_T;
  hipLaunchKernelGGL(k_bam_copy, dim3((uint32_t)std::min<uint64_t>(tiles, COPY_GRID)), dim3(COPY_T), 0, st, U, run_dst,
                     run_src, n_runs, head_bytes, bytes, out);
  return hipGetLastError();
}

}  // namespace sbh
