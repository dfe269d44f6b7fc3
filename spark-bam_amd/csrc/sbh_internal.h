// sbh_internal.h -- device-side layouts shared by the HIP kernels and the C-ABI layer.
// CDNA4 (gfx950) only: 64-lane waves, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sparkbam.h"

namespace sbh {

constexpr int WAVE = 64;

// Inclusive prefix sum over the 64 lanes of a wave in DPP steps (no LDS round trips):
// row_shr 1/2/4/8 within each 16-lane row, then row_bcast:15 and row_bcast:31 carry
// the row totals across rows (gfx9 DPP).  Inactive lanes must contribute 0.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return x;
}

// The same for 64 values below 2^28, whose sum needs more than 32 bits: two scans, the low 16 bits
// (which sum below 2^22) and the rest (below 2^18).
__device__ __forceinline__ uint64_t wave_incl_scan64(uint32_t v) {
  return (uint64_t)wave_incl_scan(v & 0xffffu) + ((uint64_t)wave_incl_scan(v >> 16) << 16);
}

// v summed over the 64 lanes of a wave, in every lane
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
  for (int m = 1; m < 64; m <<= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, m);
  return v;
}

// One value per workgroup of 256 into *dst: v summed over the 4 waves (every lane calls; s_red: 4 words).
__device__ __forceinline__ void block_add(uint64_t v, uint64_t *s_red, unsigned long long *dst) {
  v = wave_sum(v);
  __syncthreads();  // (s_red may still be read from the call before)
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t t = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    if (t) atomicAdd(dst, (unsigned long long)t);
  }
}

// The opening of a filtered row kernel (bam_gather.hip, depth.hip, pileup.hip, tally.hip, fastq.hip,
// stats.hip):
// a lane's smallest bad row and its smallest row that is bad only because it runs past the stream,
// kept over the lane's whole loop and sent out once behind it.  The host's rows_verdict reads the
// two words: they are equal exactly when more resident bytes may cure the first bad row.
struct RowMinima {
  uint64_t bad = ~0ull, past = ~0ull;
  // row i failed row_check; only_past: its verdict was ROW_PAST
  __device__ __forceinline__ void refused(uint64_t i, bool only_past) {
    bad = bad < i ? bad : i;
    if (only_past) past = past < i ? past : i;
  }
  // row i is valid and kept, but the stage itself refuses it (reference or CIGAR out of range)
  __device__ __forceinline__ void rejected(uint64_t i) { bad = bad < i ? bad : i; }
  // bad_out, past_out: preset ~0 by the caller
  __device__ __forceinline__ void send(unsigned long long *bad_out, unsigned long long *past_out) const {
    if (bad != ~0ull) atomicMin(bad_out, (unsigned long long)bad);
    if (past != ~0ull) atomicMin(past_out, (unsigned long long)past);
  }
};

// Where a slot of a span table stands (depth.hip's slots, pileup.hip's positions): span k owns
// [off[k], off[k + 1]), off has n_spans + 1 ascending entries, off[0] == 0, and s < off[n_spans].  Slot s
// is its span's first when s == first and its last when s + 1 == next.
struct SpanCursor {
  uint32_t k;
  uint64_t first, next;  // off[k], off[k + 1]
  // the span holding slot s: the last k with off[k] <= s (below n_spans, so off[k + 1] exists)
  static __device__ __forceinline__ SpanCursor span_at(const uint64_t *off, uint32_t n_spans, uint64_t s) {
    uint32_t lo = 0, hi = n_spans;  // first k with off[k] > s, in [1, n_spans]
    while (lo < hi) {
      const uint32_t m = (lo + hi) >> 1;
      if (off[m] <= s) lo = m + 1;
      else hi = m;
    }
    const uint32_t k = lo ? lo - 1 : 0;
    return SpanCursor{k, off[k], off[k + 1]};
  }
  // on to the span of slot s, from the span of a slot before it (spans may be 1 slot long: a loop)
  __device__ __forceinline__ void span_to(const uint64_t *off, uint32_t n_spans, uint64_t s) {
    while (s >= next && k + 1 < n_spans) ++k, first = next, next = off[k + 1];
  }
};

// The grid of a kernel that takes one row per lane, grid-stride, in workgroups of 256: 262144 rows a pass.
constexpr uint32_t ROWS_GRID = 1024;
inline uint32_t rows_grid(uint64_t n) {
  const uint64_t g = (n + 255) / 256;
  return (uint32_t)(g < ROWS_GRID ? g : ROWS_GRID);
}

// v from lane ^ M: quad DPP for 1 and 2, ds_swizzle (bit mode, within 32 lanes) for 4..16,
// ds_bpermute for 32.
template <uint32_t M>
__device__ __forceinline__ uint32_t xor_lane(uint32_t v) {
  if constexpr (M == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, false);
  else if constexpr (M == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, false);
  else if constexpr (M < 32) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (int)((M << 10) | 0x1f));
  else return (uint32_t)__shfl_xor((int)v, (int)M);
}
template <uint32_t SIZE, uint32_t STRIDE>
__device__ __forceinline__ uint32_t bitonic_step(uint32_t k, uint32_t lane) {
  const uint32_t o = xor_lane<STRIDE>(k);
  const bool up = (lane & SIZE) == 0, lower = (lane & STRIDE) == 0;
  return (lower == up) ? (k < o ? k : o) : (k > o ? k : o);
}
// ascending sort of one key per lane across the wave
__device__ __forceinline__ uint32_t bitonic64(uint32_t k, uint32_t lane) {
  k = bitonic_step<2, 1>(k, lane);
  k = bitonic_step<4, 2>(k, lane), k = bitonic_step<4, 1>(k, lane);
  k = bitonic_step<8, 4>(k, lane), k = bitonic_step<8, 2>(k, lane), k = bitonic_step<8, 1>(k, lane);
  k = bitonic_step<16, 8>(k, lane), k = bitonic_step<16, 4>(k, lane), k = bitonic_step<16, 2>(k, lane);
  k = bitonic_step<16, 1>(k, lane);
  k = bitonic_step<32, 16>(k, lane), k = bitonic_step<32, 8>(k, lane), k = bitonic_step<32, 4>(k, lane);
  k = bitonic_step<32, 2>(k, lane), k = bitonic_step<32, 1>(k, lane);
  k = bitonic_step<64, 32>(k, lane), k = bitonic_step<64, 16>(k, lane), k = bitonic_step<64, 8>(k, lane);
  k = bitonic_step<64, 4>(k, lane), k = bitonic_step<64, 2>(k, lane), k = bitonic_step<64, 1>(k, lane);
  return k;
}

// Block table (struct of arrays, one entry per BGZF block of the chain, in file
// order).  Mirrors bgzf Metadata(start, compressedSize, uncompressedSize)
// (bgzf/.../block/Metadata.scala:6-8) plus the header size and flat start.
struct DevBlocks {
  uint64_t *cstart;  // compressed offset relative to the shard's first byte
  uint32_t *csize;   // BSIZE + 1
  uint32_t *hsize;   // 18 + XLEN - 6
  uint32_t *usize;   // ISIZE (0 for an empty block)
  uint64_t *ustart;  // flat offset of the block's first uncompressed byte
  uint32_t *flags;   // BLK_* bits
  uint32_t *status;  // inflate status per block (INF_*)
  uint32_t *ntok;    // LZ77 tokens k_huff emitted for the block (k_lz input)
};

constexpr uint32_t BLK_EMPTY = 1u;     // dataLength == 2: the stream ends here
constexpr uint32_t BLK_TRUNCATED = 2u;  // block runs past the resident bytes

// Inflate status codes per block (written by k_huff).
constexpr uint32_t INF_OK = 0;
constexpr uint32_t INF_SIZE = 1;      // fewer than ISIZE bytes produced
constexpr uint32_t INF_DATA = 2;      // DataFormatException (zlib Z_DATA_ERROR)
constexpr uint32_t INF_BAD_ISIZE = 3; // ISIZE outside [0, 65536]
constexpr uint32_t INF_SERIAL = 0xffu; // (inside inflate only) left to the serial decoder
constexpr uint32_t NTOK_STORED = 0xffffffffu;  // ntok of a block whose payload is one stored deflate block

// Eager tile geometry (check.hip): a workgroup decides ETILE positions and stages those
// plus a look-ahead; EAGER_REACH bounds the flat bytes past a tile's first position
// that its staged window touches (the pipelined run launches a tile only once they are
// inflated; reads beyond, by the exact path, defer the position instead).
#ifndef SBH_ETILE
#define SBH_ETILE 16384
#endif
constexpr uint64_t EAGER_TILE = SBH_ETILE;
constexpr uint64_t EAGER_REACH = SBH_ETILE + 4096 + 512 + 64;
// Bitmap set-bit prefix (launch_rec_positions_bits): one u64 per group of WPRE_GROUP
// consecutive words of [first, E) -- the set bits before the group; a lookup adds the
// popcounts of the group's earlier words (one 64-byte read).
constexpr uint32_t WPRE_GROUP = 16;

// Launchers that one .hip file defines and another calls: this header is the only place such a
// function is declared.  (A launcher whose callers all sit in its own file is static there; the
// host side's structs and helpers are in sbh_host.h.)

// Exclusive scan of n u64 (bgzf_index.hip; out != in); tmp holds scan_tmp_words(n) words.
uint64_t scan_tmp_words(uint64_t n);
hipError_t scan_exclusive_u64(const uint64_t *in, uint64_t *out, uint64_t n, uint64_t *tmp, hipStream_t st);
// Block index (bgzf_index.hip): FindBlockStart's best, the header candidates per scan chunk
// (cand_chunks(n) of them: counts, then the scan, then the write), the chain over the
// candidates (build_chain, described there) and the table packed as sbh_block records.
hipError_t launch_find_block_start(const uint8_t *comp, uint64_t n, uint64_t start, int32_t k, int at_eof,
                                   unsigned long long *best, hipStream_t st);
uint64_t cand_chunks(uint64_t n);
hipError_t launch_cand_count(const uint8_t *comp, uint64_t n, uint64_t from, uint64_t *counts, uint32_t *first,
                             uint64_t nchunks, hipStream_t st);
hipError_t launch_cand_write(const uint8_t *comp, uint64_t n, uint64_t from, const uint64_t *counts,
                             const uint32_t *first, const uint64_t *offs, uint64_t *cand, uint64_t nchunks,
                             hipStream_t st);
hipError_t launch_pack_blocks(DevBlocks bl, uint64_t n, uint64_t file_off, uint64_t *out, hipStream_t st,
                              const uint64_t *rank = nullptr, const uint64_t *v = nullptr,
                              const uint64_t *next18 = nullptr);
hipError_t build_chain(const uint8_t *comp, uint64_t n, const uint64_t *cand, uint64_t nc, uint64_t start_rel,
                       int64_t *J0, int64_t *J1, uint8_t *on, uint64_t *v, uint64_t *rank, uint64_t *tmp,
                       DevBlocks bl, uint64_t *usz, uint8_t *next18, uint64_t *sidx, bool linear, hipStream_t st);

// Inflate = k_huff (Huffman decode -> LZ77 tokens, block status) then k_lz (tokens ->
// flat bytes; a block that is one stored deflate block is copied from comp).  tok_buf: >= 4 B
// of token scratch per flat byte of the launched blocks, tok_buf[0] standing for flat offset
// tok_base (block b's tokens at tok_buf[ustart_b - tok_base ...]), so a shard can be inflated
// in batches of blocks that reuse one bounded token buffer.
// stages: the lane-parallel kernels, which leave INF_SERIAL in the status of a block they do not
// finish, and the serial decoder behind them (sbh_inflate_paths runs the two apart).
constexpr uint32_t HUFF_FAST = 1u, HUFF_SERIAL = 2u;
hipError_t launch_huff(const uint8_t *comp, DevBlocks blocks, uint64_t nblocks, uint32_t *tok_buf, uint64_t tok_base,
                       hipStream_t stream, uint32_t stages = HUFF_FAST | HUFF_SERIAL);
hipError_t launch_lz(const uint8_t *comp, DevBlocks blocks, uint64_t nblocks, const uint32_t *tok_buf,
                     uint64_t tok_base, uint8_t *U, hipStream_t stream);
// *first = the first block of [0, n) whose status is not INF_OK (~0 if none).
// (init: set *first to ~0 first; false when the caller already did)
hipError_t launch_first_bad(const uint32_t *status, uint64_t n, unsigned long long *first, hipStream_t stream,
                            bool init = true);

// Checkers and the record chain (check.hip; each launcher's buffers are described at its
// definition).  counters: the shard's counter buffer, slots in namespace ctr below.
hipError_t launch_eager(const uint8_t *U, uint64_t u_pad, uint64_t begin, uint64_t end, const uint64_t *seg_end,
                        uint32_t nseg, uint32_t open_last, const int32_t *ctg, int32_t nctg, int32_t rtc,
                        uint32_t *bits, unsigned long long *counters, hipStream_t st, uint64_t front,
                        uint64_t *defer_pos, uint64_t defer_cap, uint64_t *xq_pos, uint64_t xq_cap);
hipError_t launch_eager_xq(const uint8_t *U, uint64_t begin, const uint64_t *seg_end, uint32_t nseg,
                           uint32_t open_last, const int32_t *ctg, int32_t nctg, int32_t rtc, uint32_t *bits,
                           unsigned long long *counters, uint64_t *xq_pos, uint64_t cap, hipStream_t st);
hipError_t launch_eager_defer(const uint8_t *U, uint64_t begin, const uint64_t *seg_end, uint32_t nseg,
                              uint32_t open_last, const int32_t *ctg, int32_t nctg, int32_t rtc, uint32_t *bits,
                              unsigned long long *counters, const uint64_t *defer_pos, uint64_t cap,
                              hipStream_t st);
hipError_t launch_full(const uint8_t *U, uint64_t u_pad, uint64_t begin, uint64_t end, const uint64_t *seg_end,
                       uint32_t nseg, uint32_t open_last, const int32_t *ctg, int32_t nctg, int32_t rtc,
                       uint32_t *words, unsigned long long *counters, uint64_t *close_pos, uint32_t *close_word,
                       uint64_t close_cap, uint32_t *op_words, uint64_t op_cap_words, hipStream_t st);
hipError_t launch_first_set(const uint32_t *bits, uint64_t begin, uint64_t from, uint64_t to,
                            unsigned long long *best, hipStream_t st);
hipError_t launch_verify_chain_count(const uint8_t *U, const uint32_t *bits, uint64_t begin, uint64_t bits_end,
                                     uint64_t from, uint64_t E, uint64_t total, unsigned long long *n_anom,
                                     unsigned long long *first_anom, unsigned long long *exit_pos,
                                     unsigned long long *n_set, hipStream_t st,
                                     const unsigned long long *from_dev = nullptr, uint32_t *chunk_cnt = nullptr);
hipError_t launch_chain_walk(const uint8_t *U, uint64_t first, uint64_t E, uint64_t total,
                             unsigned long long *count, unsigned long long *last, hipStream_t st);
hipError_t launch_chain_mark(const uint8_t *U, const uint32_t *bits, uint64_t begin, uint64_t from, uint64_t E,
                             uint64_t total, const uint64_t *pos, const uint64_t *wpre, uint64_t n, uint32_t *J,
                             uint32_t *J2, uint32_t *J0, uint64_t *mark, unsigned long long *exit_pos,
                             uint32_t *final_code, bool doubling, hipStream_t st);

// Record field extraction (records.hip): device columns of a decoded batch (the host
// view is sbh_records_out in sparkbam.h).
struct RecCols {
  int32_t *ref_id, *pos, *next_ref_id, *next_pos, *tlen;
  uint16_t *flag, *bin;
  uint8_t *mapq;
  char *names;
  uint32_t *cigar;
  char *seq;
  uint8_t *qual, *aux;
};
hipError_t launch_rec_positions_bits(const uint32_t *bits, uint64_t begin, uint64_t first, uint64_t E, uint64_t *cnt,
                                     uint64_t *wpre, uint64_t *tmp, uint64_t *pos, hipStream_t st);
hipError_t launch_rec_positions_chain(const uint8_t *U, uint64_t first, uint64_t E, uint64_t total, uint64_t cap,
                                      uint64_t *pos, hipStream_t st);
// record starts of n sorted, disjoint ranges [first[i], E[i]) inside the union [U0, U1) in one
// launch set: pos[off[i] + r] = the range's r-th set bit, off[0..n] the exclusive prefix of the
// ranges' counts + reserve[i] (rows left free behind range i's own)
hipError_t launch_rec_positions_ranges(const uint32_t *bits, uint64_t begin, uint64_t U0, uint64_t U1,
                                       const uint64_t *first, const uint64_t *E, const uint64_t *reserve, uint64_t n,
                                       uint64_t *cnt, uint64_t *wpre, uint64_t *tmp, uint64_t *rbase, uint64_t *rcnt,
                                       uint64_t *off, uint64_t cap, uint64_t *pos, hipStream_t st);
// bad = min row of a record that runs over the end of its stream segment
hipError_t launch_rec_seg_check(const uint8_t *U, const uint64_t *pos, uint64_t n, const uint64_t *seg_end,
                                uint32_t nseg, unsigned long long *bad, hipStream_t st);
hipError_t launch_rec_sizes(const uint8_t *U, const uint64_t *pos, uint64_t n, uint64_t total, uint64_t *nm,
                            uint64_t *cg, uint64_t *sq, uint64_t *ax, unsigned long long *bad, hipStream_t st);
hipError_t launch_rec_fields(const uint8_t *U, const uint64_t *pos, uint64_t n, const uint64_t *nm_off,
                             const uint64_t *cg_off, const uint64_t *sq_off, const uint64_t *ax_off, const RecCols &c,
                             hipStream_t st);
hipError_t launch_region_keep(const uint8_t *U, const uint64_t *pos, uint64_t n, uint64_t total, const int32_t *iv_ref,
                              const int64_t *iv_begin, const int64_t *iv_end, uint32_t n_iv, uint64_t *keep,
                              hipStream_t st);
hipError_t launch_compact_u64(const uint64_t *in, const uint64_t *keep, const uint64_t *kpre, uint64_t n,
                              uint64_t *out, hipStream_t st);
// the chain proof's chunk of bitmap words (k_verify_chain_w: one wave, 4 words per lane)
constexpr uint64_t VC_CHUNK = 256;
// split counts from the proof's per-chunk set-bit counts (splits.hip): counts[i] += set bits of
// [first[i], E[i]) for the SPLIT_OK splits, the bitmap read only in each range's end chunks
// (chain_E != 0: counts are written, not added, and a range outside [chain_first, chain_E) gets
// SPLIT_NOCOUNT)
hipError_t launch_split_count_cc(const uint32_t *bits, uint64_t begin, const uint32_t *chunk_cnt, const uint64_t *first,
                                 const uint64_t *E, const uint32_t *code, uint64_t nsplit, unsigned long long *counts,
                                 hipStream_t st, uint64_t chain_first = 0, uint64_t chain_E = 0);
// record starts (flat) -> htsjdk virtual positions over the device block table
hipError_t launch_rec_vpos(const uint64_t *pos, uint64_t n, DevBlocks bl, uint64_t nblocks, uint64_t file_off,
                           uint64_t *vpos, hipStream_t st);
// Coordinate order of the kept rows (bam_sort.hip; the key in bam_sort_core.h).  launch_sort_keys:
// key / row of the first khpre[n] & 0xffffffff entries of rows (k_bam_index's), acc = ctr::SORT_DESC
// (preset 0, 0, ~0).  launch_sort_pass: one stable 8-bit pass from (key, row) to (key_out, row_out);
// hist: 2 (256 sort_tiles(m) + 1) words, tmp: scan_tmp_words(256 sort_tiles(m) + 1).
// launch_sort_apply: pos2 / len2 / kh over m + 1 entries; launch_sort_rows: rows[k] = row[k].
uint64_t sort_tiles(uint64_t m);
hipError_t launch_sort_keys(const uint8_t *U, const uint64_t *pos, const uint64_t *rows, const uint64_t *kh_total,
                            uint64_t n, uint64_t *key, uint32_t *row, unsigned long long *acc, hipStream_t st);
hipError_t launch_sort_pass(const uint64_t *key, const uint32_t *row, uint64_t m, uint32_t shift, uint64_t *hist,
                            uint64_t *tmp, uint64_t *key_out, uint32_t *row_out, hipStream_t st);
hipError_t launch_sort_apply(const uint64_t *pos, const uint64_t *len, const uint32_t *row, uint64_t m, uint64_t *pos2,
                             uint64_t *len2, uint64_t *kh, hipStream_t st);
hipError_t launch_sort_rows(const uint32_t *row, uint64_t m, uint64_t *rows, hipStream_t st);
// Read-name order of the kept rows (bam_name.hip; the order in bam_name_core.h).  The words k_name_scan
// and k_name_groups reduce into -- a device array of the shard's (sbh_shard::Bam::nacc), not slots of
// the counter buffer: the descents, the longest name, the tie's OR, each chunk's OR, the four group
// counts (all preset 0), then the shortest name, the tie's AND and each chunk's AND (preset ~0).
namespace nacc {
constexpr uint32_t DESC = 0, MAX_L = 1, TIE_OR = 2, OR = 3, GROUPS = OR + 32, ONES = GROUPS + 4;
constexpr uint32_t MIN_L = ONES, TIE_AND = ONES + 1, AND = ONES + 2, WORDS = AND + 32;
}  // namespace nacc
// sbh_shard::Bam::order after sbh_records_bam_scan_names: the library's own word, not a value of
// sbh_records_bam_scan_order's argument (which keeps refusing it)
constexpr int ORDER_NAME = 2;
// launch_name_scan: row[] of the first khpre[n] & 0xffffffff entries of rows, acc = the nacc words
// (preset).  launch_name_keys: key[k] of chunk c (c == 32: the tie) for row[k], k < m.
// launch_name_groups: out = acc + nacc::GROUPS, over row[] in its final order.
hipError_t launch_name_scan(const uint8_t *U, const uint64_t *pos, const uint64_t *rows, const uint64_t *kh_total,
                            uint64_t n, uint32_t *row, unsigned long long *acc, hipStream_t st);
hipError_t launch_name_keys(const uint8_t *U, const uint64_t *pos, const uint32_t *row, uint64_t m, uint32_t c,
                            uint64_t *key, hipStream_t st);
hipError_t launch_name_groups(const uint8_t *U, const uint64_t *pos, const uint32_t *row, uint64_t m,
                              unsigned long long *out, hipStream_t st);
// BGZF footer CRC32 of every inflated, non-truncated block (crc.hip).
hipError_t launch_block_crc(const uint8_t *comp, DevBlocks bl, uint64_t nblocks, const uint8_t *U,
                            unsigned long long *n_bad, unsigned long long *first_bad, hipStream_t st);

// BGZF writer (deflate.hip): members are coded in batches of at most DEFLATE_BATCH 65498-byte
// pieces: k_prev (hash chains into prev), k_deflate (tokens into toks, one 64 KiB slot per
// member and its size), k_footer; k_gather packs the slots at host-computed offsets.
constexpr uint32_t DEFLATE_BATCH = 2048;
constexpr uint64_t DEFLATE_PREV_BYTES = 65536ull * 2;  // prev scratch per member
constexpr uint64_t DEFLATE_TOK_BYTES = 65536ull * 4;   // token scratch per member (256 lanes x 256)
constexpr uint64_t DEFLATE_REC_BYTES = 4096;           // per-member record: token counts, histogram, codes
uint64_t deflate_nblocks(uint64_t n);
hipError_t launch_deflate(const uint8_t *src, uint64_t n, uint64_t b0, uint32_t nbatch, uint16_t *prev,
                          uint32_t *toks, uint8_t *recs, uint8_t *slots, uint32_t *sizes, hipStream_t st);
hipError_t launch_deflate_gather(const uint8_t *slots, uint64_t stride, const uint32_t *sizes, const uint64_t *offs,
                                 uint64_t nblocks, uint8_t *out, hipStream_t st);

// Byte-exact BGZF writer (zdeflate.hip; zlib 1.2.11 deflate_slow at level 4..9, htsjdk's 5 by
// default): members in batches of at most ZDEFLATE_BATCH (env SBH_ZDEFLATE_BATCH overrides),
// per member prev[] (u16), match records (u64), tokens (u32), a record of blocks / trees /
// headers, and an output slot: ~1 MB of scratch per member, 8 GB at 8192 members.  The batch
// is large because k_zparse runs one serial wave per member: 8192 members keep 8 of them per
// SIMD in flight.
constexpr uint32_t ZDEFLATE_BATCH = 8192;
constexpr uint64_t ZDEFLATE_PREV_ENTRIES = 65536;
constexpr uint64_t ZDEFLATE_INFO_ENTRIES = 65536;
constexpr uint64_t ZDEFLATE_TOK_ENTRIES = 65536;
constexpr uint64_t ZDEFLATE_REC_BYTES = 16384;
constexpr uint32_t ZDEFLATE_HDR_BYTES = 640;  // a dynamic block header (<= ~4500 bits)
constexpr uint64_t ZDEFLATE_SLOT = 65536 + 64;  // 18 + (< 65518) + 8 bytes, a multiple of 16
hipError_t launch_member_footer(const uint8_t *src, uint64_t n, uint64_t b0, uint64_t nblocks, uint32_t nbatch,
                                uint8_t *slots, uint64_t stride, const uint32_t *sizes, hipStream_t st);

// The shard's counter buffer (sbh_shard::ctr, device, CTR_WORDS u64, zeroed by
// sbh_shard_create) and its pinned host mirror h_ctr (same size, same indices).  Entry points
// run one at a time on the shard's stream and copy their results out before returning, so
// regions used within one call may share words with another call's; the one persistent
// region may overlap nothing.
constexpr uint32_t CTR_WORDS = 4096;
// persistent [CTR_TRUE_SPREAD, +CTR_TRUE_WORDS): k_eager's per-wave true counts, zero before
// every k_eager launch; k_fold_true folds them into the true count and zeroes them again
constexpr uint32_t CTR_TRUE_SPREAD = 2048, CTR_TRUE_WORDS = 64 * 16;
// per call [CTR_NEXT18, +4): the 18 bytes after an index's last chained block, at byte
// NEXT18_NONLIN the linear chain's "not linear" flag (u8), at byte NEXT18_NEMPTY the chain's
// empty-block count (u32), then the linear chain's start index (u64, device only)
constexpr uint32_t CTR_NEXT18 = CTR_TRUE_SPREAD + CTR_TRUE_WORDS;
constexpr uint32_t NEXT18_NONLIN = 18, NEXT18_NEMPTY = 20;
// sbh_run_shard sets ctr[0, CTR_RUN_WORDS) from one template (h_ctr + H_RUN_TPL) and brings
// the same words back in one copy with the inflate status
constexpr uint32_t CTR_RUN_WORDS = 101;

// The slots of [0, CTR_CALL_END), by owner.  A name without H_ is a word a kernel writes (its
// result lands at the same index of h_ctr); an H_ name exists only in h_ctr.
namespace ctr {
// eager checker (launch_eager, _defer, _xq; eager_range, run_pipelined)
constexpr uint32_t EAGER_TRUE = 0, EAGER_HALO_N = 1, EAGER_HALO_FIRST = 2;  // need-halo: count, min position
constexpr uint32_t EAGER_DEFER_N = 3, EAGER_XQ_N = 4, EAGER_XQ_LIVE = 5;    // xq: queued, past the pre-test
constexpr uint32_t EAGER_END = 6;
// full checker (launch_full, sbh_check_full): Counts[nnz][flag] and the reads-before-error
// histogram [nnz][rbe] behind four scalars.  Shares [0, FULL_END) with everything below:
// sbh_check_full zeroes it, runs and copies it out within the call.
constexpr uint32_t FULL_NNZ = SBH_NNZ_MAX, FULL_FLAGS = 19, FULL_RBE = SBH_RBE_MAX;
constexpr uint32_t FULL_SUCCESS = 0, FULL_UNKNOWN_N = 1, FULL_UNKNOWN_MIN = 2, FULL_CLOSE_N = 3;
constexpr uint32_t FULL_COUNTS = 4, FULL_COUNTS_N = FULL_NNZ * FULL_FLAGS;
constexpr uint32_t FULL_RBE_HIST = FULL_COUNTS + FULL_COUNTS_N, FULL_RBE_N = FULL_NNZ * FULL_RBE;
constexpr uint32_t FULL_END = FULL_RBE_HIST + FULL_RBE_N;
// FindBlockStart's best (sbh_find_block_start); sbh_index lands its candidate count in the
// same word of the mirror (h_ctr only)
constexpr uint32_t FBS_BEST = 0, H_INDEX_NCAND = 0;
// FindRecordStart's best (sbh_find_record_start, sbh_run_shard's tail)
constexpr uint32_t FRS_BEST = 8;
// chain proof (k_verify_chain_w).  Not only per call: sbh_run_shard's tail writes these and its
// status copy leaves them in h_ctr, where count_records_impl(known = true) -- called by
// sbh_run_shard next, nothing else having run on the shard -- reads them instead of proving again.
constexpr uint32_t PROOF_ANOM = 16, PROOF_FIRST_ANOM = 17, PROOF_SET = 18, PROOF_EXIT = 19, PROOF_END = 20;
// chain walk (k_chain_walk): records, exit
constexpr uint32_t WALK_COUNT = 20, WALK_EXIT = 21;
// chain mark (launch_chain_mark): the exit and, in the word behind it, the verdict (u32) on
// the device; h_ctr only: the verdict's landing place, the marked count, the first node and
// the exit's copy
constexpr uint32_t MARK_EXIT = 22, MARK_CODE = 23;
constexpr uint32_t H_MARK_CODE = 22, H_MARK_COUNT = 23, H_MARK_FIRST = 24, H_MARK_EXIT = 25;
// records: first malformed row of the size pass (records_finish) and of the batch's segment
// check.  They share H_MARK_FIRST / H_MARK_EXIT: count_records_impl has read those before it
// returns.
constexpr uint32_t REC_BAD = 24, REC_SEG_BAD = 25;
// block CRC (launch_block_crc): bad blocks, first bad block
constexpr uint32_t CRC_BAD_N = 32, CRC_FIRST_BAD = 33;
// check-records (launch_truth_scatter / _compare): tp, fp, fn, fp slots, fn slots, unknown
constexpr uint32_t TRUTH = 40, TRUTH_TP = 40, TRUTH_FP = 41, TRUTH_FN = 42, TRUTH_UNKNOWN = 45;
constexpr uint32_t TRUTH_END = 46;
// BAI scan (sbh_bai_scan): three error rows on the device; h_ctr only: the run count, the
// scan's three aux words (the edges are the last two) and the bad row's virtual offset.  Shares
// [40, 48) with check-records: per call.
constexpr uint32_t BAI_ERR = 40, BAI_UNFIT = 40, BAI_UNSORTED = 41, BAI_OFF_REF = 42, BAI_ERR_END = 43;
constexpr uint32_t H_BAI_NRUNS = 43, H_BAI_AUX = 44, H_BAI_FIRST_EDGE = 45, H_BAI_LAST_EDGE = 46;
constexpr uint32_t H_BAI_BAD_VPOS = 47;
// SAM scan (sbh_records_sam_scan): first malformed row; h_ctr only: host rows, text bytes
constexpr uint32_t SAM_BAD = 48, H_SAM_NHOST = 49, H_SAM_TOTAL = 50;
// BAM scan (sbh_records_bam_scan): first invalid row, first row that only runs past the stream's
// end; h_ctr only: the kept records' bytes, kept rows | runs << 32
constexpr uint32_t BAM_BAD = 51, BAM_PAST = 52, H_BAM_BYTES = 53, H_BAM_KH = 54;
// coordinate order (k_sort_keys): descents key[k - 1] > key[k], the OR and the AND of all keys
constexpr uint32_t SORT_DESC = 55, SORT_OR = 56, SORT_AND = 57, SORT_END = 58;
// The head of an accumulator add's counters, the four words of its one round trip (sbh::AddTrip,
// sbh_host.h): first bad row, first row that only runs past the stream's end, then two counters of the
// stage's own.  Every add's row kernel writes them in this order and reads nothing else back.
constexpr uint32_t ADD_BAD = 0, ADD_PAST = 1, ADD_A = 2, ADD_B = 3, ADD_HEAD = 4;
// depth add: the head (k_depth_check: kept rows, kept rows without a reference); (k_depth_events):
// rows walked, bases covered
constexpr uint32_t DEPTH_BAD = SORT_END, DEPTH_COUNTED = DEPTH_BAD + ADD_HEAD, DEPTH_COV = DEPTH_COUNTED + 1;
constexpr uint32_t DEPTH_END = DEPTH_COV + 1;
// tally and stats adds, h_ctr only -- the device words are the accumulator's staging words: the head
// (k_tally_rows: kept rows QC-pass, QC-fail; k_stats_rows: kept rows, counted rows)
constexpr uint32_t H_STAGE_HEAD = DEPTH_END, STAGE_END = H_STAGE_HEAD + ADD_HEAD;
// FASTQ scan (sbh_records_fastq_scan): first invalid row, first row that only runs past the stream's
// end; h_ctr only: the parts' bytes (3 words), then their lines (3 words)
constexpr uint32_t FASTQ_BAD = STAGE_END, FASTQ_PAST = FASTQ_BAD + 1, H_FASTQ_SUMS = FASTQ_BAD + 2;
constexpr uint32_t FASTQ_END = H_FASTQ_SUMS + 6;
// pileup add: the head (k_pile_check: kept rows, kept rows without a reference); (k_pile_events):
// rows walked, then what went into each of the eight channels
constexpr uint32_t PILE_BAD = FASTQ_END, PILE_COUNTED = PILE_BAD + ADD_HEAD, PILE_TOTALS = PILE_COUNTED + 1;
constexpr uint32_t PILE_END = PILE_TOTALS + 8;
// inflate status (launch_first_bad): the first block whose status is not INF_OK
constexpr uint32_t FIRST_BAD = 100;
// h_ctr only: that block's status (u32), fetched after the run's copy of [0, CTR_RUN_WORDS)
constexpr uint32_t H_BAD_STATUS = 101;
// h_ctr only: where a name-order BAM scan's nacc:: words land (the device words are the shard's own array)
constexpr uint32_t H_NAME = 128;
// h_ctr only, host scratch under the full checker's mirror (each written and read within one
// call): the 18 bytes at an index's start and its next18 words (sbh_index); the proof
// counters' initial values, an H2D source, and the bitmap word of the proof's first position
// (count_records_impl); the run template
constexpr uint32_t H_INDEX_HDR18 = 512, H_INDEX_NEXT18 = 516;
constexpr uint32_t H_PROOF_INIT = 600, H_PROOF_FIRST_WORD = 604;
constexpr uint32_t H_RUN_TPL = 1024;
}  // namespace ctr
constexpr uint32_t CTR_CALL_END = 4 + ctr::FULL_NNZ * ctr::FULL_FLAGS + ctr::FULL_NNZ * ctr::FULL_RBE;
static_assert(CTR_CALL_END <= CTR_TRUE_SPREAD && CTR_NEXT18 + 4 <= CTR_WORDS, "counter buffer layout");
static_assert(ctr::FULL_END == CTR_CALL_END, "the full checker's counters end the per-call region");
static_assert(ctr::DEPTH_END <= ctr::FIRST_BAD, "the depth counters end before the first bad block");
static_assert(ctr::STAGE_END <= ctr::FIRST_BAD, "the tally and stats adds' mirror words end before the first bad block");
static_assert(ctr::FASTQ_END <= ctr::FIRST_BAD, "the FASTQ scan's words end before the first bad block");
static_assert(ctr::PILE_END <= ctr::FIRST_BAD, "the pileup add's counters end before the first bad block");
// what the run template presets (the eager counters, FindRecordStart's best, the proof
// counters, the first bad block) travels in the run's one copy each way ...
static_assert(ctr::EAGER_END <= CTR_RUN_WORDS && ctr::FRS_BEST < CTR_RUN_WORDS &&
                  ctr::PROOF_END <= CTR_RUN_WORDS && ctr::FIRST_BAD == CTR_RUN_WORDS - 1,
              "the run template covers every slot it presets, the first bad block last");
// ... and that copy must not land on the status word fetched after it
static_assert(ctr::H_BAD_STATUS >= CTR_RUN_WORDS, "the bad block's status lies behind the run's copy");
static_assert(ctr::H_RUN_TPL + CTR_RUN_WORDS <= CTR_WORDS, "the run template fits the mirror");
static_assert(ctr::H_NAME > ctr::H_BAD_STATUS && ctr::H_NAME + nacc::WORDS <= ctr::H_INDEX_HDR18,
              "the name words' mirror lies between the run's words and the index's host scratch");
static_assert(ctr::H_INDEX_HDR18 + 3 <= ctr::H_INDEX_NEXT18 && ctr::H_INDEX_NEXT18 + 3 <= ctr::H_PROOF_INIT &&
                  ctr::H_PROOF_INIT + 4 <= ctr::H_PROOF_FIRST_WORD && ctr::H_PROOF_FIRST_WORD < ctr::H_RUN_TPL,
              "host scratch regions are disjoint");

// Batched splits and check-bam truth comparison (splits.hip).
constexpr uint32_t SPLIT_OK = 0;    // first record and flat end decided on the device
constexpr uint32_t SPLIT_HOST = 1;  // off the common path: the exact per-split host path decides
constexpr uint32_t SPLIT_NOREAD = 2;  // FindBlockStart lands on an empty block: NoReadFoundException (no records)
constexpr unsigned long long SPLIT_NOCOUNT = ~0ull;  // (sbh_split_starts fast path) the count is the host's to decide
struct SplitArgs {
  const uint8_t *comp;
  uint64_t n;
  int at_eof;
  const uint64_t *cand;
  uint64_t ncand, cand_from;
  int32_t k_check;
  const uint64_t *cstart, *ustart;
  const uint32_t *flags;
  uint64_t nblocks, utotal, last_start;
  const uint64_t *seg_end;
  uint32_t nseg;
  const uint32_t *bits;
  uint64_t bits_begin, bits_end;
  int64_t mrs;
};
// n host words to dst on st: up to 128 as a kernel's arguments (no DMA), more by a copy
hipError_t set_words(uint64_t *dst, const uint64_t *src, uint64_t n, hipStream_t st);
hipError_t launch_split_prologue(const SplitArgs &a, const uint64_t *starts, const uint64_t *ends, uint64_t nsplit,
                                 uint64_t *first, uint64_t *E, uint32_t *code, hipStream_t st);
hipError_t launch_split_popcount(const uint32_t *bits, uint64_t begin, const uint64_t *first, const uint64_t *E,
                                 const uint32_t *code, uint64_t nsplit, uint64_t max_span,
                                 unsigned long long *counts, hipStream_t st);
hipError_t launch_split_cm_count(const uint64_t *pos, const uint64_t *mark, const uint64_t *mpre, uint64_t n,
                                 const uint64_t *first, const uint64_t *E, uint32_t *code, uint64_t nsplit,
                                 unsigned long long *counts, hipStream_t st);
hipError_t launch_truth_scatter(const uint64_t *vpos, uint64_t n, const uint64_t *cstart, const uint64_t *ustart,
                                uint64_t nblocks, uint64_t file_off, uint64_t begin, uint64_t end, uint32_t *tbits,
                                unsigned long long *bad, hipStream_t st);
hipError_t launch_truth_compare(const uint32_t *ebits, uint64_t ebegin, const uint32_t *tbits, uint64_t begin,
                                uint64_t end, const uint64_t *rb, const uint64_t *re, uint64_t nr,
                                unsigned long long *acc, uint64_t *fp_pos, uint64_t fp_cap, uint64_t *fn_pos,
                                uint64_t fn_cap, hipStream_t st);

// Host-side streaming over a shard (sbh_check_stream, check_stream.hip): the next window's
// compressed bytes -- and optionally a host array of u64 riding with it (check-bam's truth
// slice) -- copied into the shard's spare device buffers by a host thread while the current
// window's kernels run.  shard_prefetch starts the copy; shard_prefetch_finish waits for it and,
// with `use`, makes it the shard's bytes exactly as sbh_shard_load(src, n, file_offset) would
// (the u64 array becomes the resident truth of check_records_resident); without, drops it.
int shard_prefetch(sbh_shard *sh, const void *src, uint64_t n, uint64_t file_offset, const uint64_t *aux,
                   uint64_t n_aux);
int shard_prefetch_finish(sbh_shard *sh, bool use, double *copy_ms = nullptr);
bool shard_prefetch_pending(const sbh_shard *sh, uint64_t *file_offset, uint64_t *n);
// sbh_check_records with the truth already on the device (the prefetched u64 array, n_rec of it)
int check_records_resident(sbh_shard *sh, const uint64_t *range_begin, const uint64_t *range_end, uint64_t n_ranges,
                           int32_t rtc, uint64_t n_rec, uint64_t *out, uint64_t *fp_flat, uint64_t fp_cap,
                           uint64_t *fn_flat, uint64_t fn_cap);

}  // namespace sbh
