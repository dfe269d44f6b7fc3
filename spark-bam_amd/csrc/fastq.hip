// fastq.hip -- FASTQ / FASTA text of a record scan's rows on CDNA4 (sbh_records_fastq_scan): size
// pass -> scans -> index pass -> emit pass.  The line a record becomes is defined in fastq_core.h,
// which the host renderer shares.
//
//   k_fastq_sizes  one row per lane, grid-stride: row_check, row_keep, the name's length, the class.
//                  Part p of the text (fastq_core.h: one part, or class 1 / 2 / 0 with
//                  SBH_FASTQ_SPLIT) has its own columns len[p][i] and keep[p][i]: the row's line
//                  length and 1 in the column of its part, 0 in every other column and for a row
//                  the filter drops.  cls[i] = the class byte.  The first bad row and the first row
//                  that only runs past the stream go out as per-lane minima behind the loop
//                  (RowMinima, sbh_internal.h; the host's rows_verdict reads them).
//   (scans)        len[p] -> lpre[p], keep[p] -> kpre[p], over n + 1 entries (entry n is 0, so
//                  entry n of a scan is the column's total)
//   k_fastq_index  off[i] = (bytes of the parts before p) + lpre[p][i]; the line's place in layout
//                  order j = (lines of the parts before p) + kpre[p][i]; rec_off[j] = off[i],
//                  rows[j] = i; i == n closes rec_off and writes the parts' totals
//   k_fastq_emit   a wave per row: the record's used bytes go to the wave's LDS slot (longer records
//                  are read in U), then the lanes stride over the aligned 4-byte words of
//                  text[off[i], off[i] + len[i]), each byte line_byte(line, k) of fastq_core.h; a word
//                  wholly inside the line is one store, the two edge words go bytewise.
//
// Bounds.
//  * Reads.  k_fastq_sizes reads a row's fixed bytes and name only after row_check has proven
//    [p, p + 4 + block_size) to lie inside the stream and to hold 36 + l_name + 4 n_cigar +
//    (l_seq + 1) / 2 + l_seq bytes.  k_fastq_emit visits only rows with len != 0, which are rows
//    the size pass of the same call accepted; line_of clamps the name's length to l_name, and
//    line_byte reads name[k] for k < name_len, packed bases at (j >> 1) for j < l_seq and
//    qualities at j < l_seq: all inside the parts row_check counted, whatever len says.  The LDS
//    slot holds the aligned words around exactly those `used` bytes at the same offsets (used <=
//    STAGE, lead <= 3: at most STAGE / 4 + 1 of the slot's STAGE / 4 + 2 words), so the same indices
//    bound the LDS reads; the copy itself reads U from 3 bytes before the record at the most to 3
//    bytes behind its used bytes, inside the stream or the zeroed pad every U carries behind it.
//  * Stores.  k_fastq_emit writes text[y] only for off[i] <= y < off[i] + len[i], and skips a row
//    unless off[i] + len[i] <= total (the text's size): nothing lands outside the row's range or
//    at or past the total even if the passes disagreed.  k_fastq_index writes rec_off[j] and
//    rows[j] for j = a sum of keep totals and prefixes < n_kept <= n (both have n + 1 entries).
#include <algorithm>

#define SBH_HD __host__ __device__
#include "fastq_core.h"
#include "sbh_host.h"

namespace sbh {
namespace {

using sbh_fq::PARTS;
constexpr uint32_t EMIT_GRID = 16384;  // k_fastq_emit: 65536 rows a pass
static_assert(sizeof(sbh_fastq_sizes) == sizeof(sbh_fq::Sizes), "fastq_core.h restates the header's layout");
static_assert(SBH_FASTQ_FASTA == sbh_fq::MODE_FASTA && SBH_FASTQ_SUFFIX == sbh_fq::MODE_SUFFIX &&
                  SBH_FASTQ_SUFFIX_ALWAYS == sbh_fq::MODE_SUFFIX_ALWAYS && SBH_FASTQ_SPLIT == sbh_fq::MODE_SPLIT,
              "fastq_core.h restates the header's mode bits");

// len, keep: n_parts(mode) columns of `stride` = n + 1 words
__global__ __launch_bounds__(256) void k_fastq_sizes(const uint8_t *__restrict__ U, const uint64_t *pos, uint64_t n,
                                                     uint64_t total, sbh_bam::Filter F, uint32_t mode, uint64_t stride,
                                                     uint64_t *len, uint64_t *keep, uint8_t *cls, unsigned long long *bad,
                                                     unsigned long long *past) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t np = sbh_fq::n_parts(mode);
  RowMinima m;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const uint64_t p = pos[i];
    uint64_t bytes = 0, l = 0;
    uint32_t c = 0;
    const int v = sbh_bam::row_check(U, total, p, &bytes);
    if (v != sbh_bam::ROW_OK) {
      m.refused(i, v == sbh_bam::ROW_PAST);
    } else if (sbh_bam::row_keep(U + p, i, F)) {
      const uint8_t *r = U + p;
      c = sbh_fq::class_of(sbh_sam::ld16(r + 18), mode);
      l = sbh_fq::line_len(sbh_sam::qname_len(r + 36, r[12]), (uint64_t)(int32_t)sbh_sam::ld32(r + 20),
                           sbh_fq::suffix_of(c, mode), mode);
    }
    const uint32_t mine = sbh_fq::part_of(c, mode);
    for (uint32_t q = 0; q < np; ++q) {
      len[q * stride + i] = q == mine ? l : 0;
      keep[q * stride + i] = q == mine && l;
    }
    cls[i] = (uint8_t)c;
  }
  m.send(bad, past);
}

// sums: part_bytes[3], part_rows[3] (parts the mode does not have: 0)
__global__ __launch_bounds__(256) void k_fastq_index(const uint64_t *len, const uint64_t *lpre, const uint64_t *kpre,
                                                     const uint8_t *cls, uint64_t n, uint32_t mode, uint64_t stride,
                                                     uint64_t *off, uint64_t *rec_off, uint64_t *rows, uint64_t *sums) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t np = sbh_fq::n_parts(mode);
  uint64_t pb[PARTS + 1] = {0, 0, 0, 0}, pr[PARTS + 1] = {0, 0, 0, 0};  // bytes and lines before each part
  for (uint32_t q = 0; q < np; ++q) {
    pb[q + 1] = pb[q] + lpre[q * stride + n];
    pr[q + 1] = pr[q] + kpre[q * stride + n];
  }
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += step) {
    if (i == n) {
      rec_off[pr[np]] = pb[np];
      for (uint32_t q = 0; q < PARTS; ++q) {
        sums[q] = q < np ? pb[q + 1] - pb[q] : 0;
        sums[PARTS + q] = q < np ? pr[q + 1] - pr[q] : 0;
      }
      continue;
    }
    const uint32_t q = sbh_fq::part_of(cls[i], mode);
    uint64_t o = 0;
    if (len[q * stride + i]) {
      o = pb[q] + lpre[q * stride + i];
      const uint64_t j = pr[q] + kpre[q * stride + i];
      if (j < n) {
        rec_off[j] = o;
        rows[j] = i;
      }
    }
    off[i] = o;
  }
}

// A record whose used bytes -- fixed fields, name, CIGAR, bases, qualities -- are at most STAGE is
// copied into its wave's LDS slot first, as aligned 4-byte words (every lane's load is independent:
// one trip to memory), and line_byte then reads it there: made on U directly, the reads of a line
// sit in divergent branches and each waits for memory on its own (measured over config B: k_fastq_emit
// 13.4 ms on U).  The copy starts at the aligned word that holds the record's first
// byte and ends with the one that holds its last used byte: at most 3 bytes before the record (the
// stream's earlier bytes) and 3 behind it (U's zeroed pad behind the stream at the worst).  The
// slot is the wave's own and LDS instructions of a wave execute in order, so a wave-scope fence is
// all that separates the copy from the reads and the reads from the next copy (sam.hip's staging).
// (A four-byte form of line_byte with branch-free paths for words wholly inside the bases or the
// qualities was built and measured: slower, 13.8 against 10.2 ms -- a wave's lanes sit in different
// parts of the line, so it runs every path)
constexpr uint32_t STAGE = 1024;
constexpr uint32_t SLOT_WORDS = STAGE / 4 + 2;

// the aligned words of text[o, o + L.len), strided over the lanes
__device__ __forceinline__ void emit_line(const sbh_fq::Line &L, uint64_t o, uint32_t lane, char *text) {
  const uint64_t end = o + L.len;
  for (uint64_t w = (o & ~3ull) + 4ull * lane; w < end; w += 4ull * WAVE) {
    if (w >= o && w + 4 <= end) {
      const uint64_t k = w - o;
      const uint32_t v = (uint32_t)sbh_fq::line_byte(L, k) | (uint32_t)sbh_fq::line_byte(L, k + 1) << 8 |
                         (uint32_t)sbh_fq::line_byte(L, k + 2) << 16 | (uint32_t)sbh_fq::line_byte(L, k + 3) << 24;
      *reinterpret_cast<uint32_t *>(text + w) = v;  // (text is a hipMalloc'd base: w is its alignment)
    } else {
      for (uint32_t b = 0; b < 4; ++b) {
        const uint64_t y = w + b;
        if (y >= o && y < end) text[y] = (char)sbh_fq::line_byte(L, y - o);
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_fastq_emit(const uint8_t *__restrict__ U, const uint64_t *pos, uint64_t n,
                                                    const uint64_t *len, const uint64_t *off, const uint8_t *cls,
                                                    uint32_t mode, int32_t def_qual, uint64_t stride, uint64_t total,
                                                    char *text) {
  __shared__ uint32_t stage[256 / WAVE][SLOT_WORDS];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x / WAVE);
  for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; i < n; i += nw) {
    const uint32_t c = cls[i];
    const uint64_t l = len[sbh_fq::part_of(c, mode) * stride + i], o = off[i];
    if (!l || o > total || l > total - o) continue;  // (wave-uniform)
    const uint64_t p = pos[i];
    const uint8_t *g = U + p;
    const uint64_t ls = (uint64_t)(int32_t)sbh_sam::ld32(g + 20);
    const uint64_t used = 36 + (uint64_t)g[12] + 4ull * sbh_sam::ld16(g + 16) + (ls + 1) / 2 + ls;
    if (used <= STAGE) {
      uint32_t *slot = stage[threadIdx.x / WAVE];
      const uint32_t lead = (uint32_t)(p & 3), words = (lead + (uint32_t)used + 3) / 4;  // <= SLOT_WORDS - 1
      const uint32_t *src = reinterpret_cast<const uint32_t *>(U + (p - lead));  // (U is a hipMalloc'd base)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      for (uint32_t k = lane; k < words; k += WAVE) slot[k] = src[k];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      emit_line(sbh_fq::line_of_len(reinterpret_cast<const uint8_t *>(slot) + lead, l, c, mode, def_qual), o, lane, text);
    } else {
      emit_line(sbh_fq::line_of_len(g, l, c, mode, def_qual), o, lane, text);
    }
  }
}

}  // namespace

// len, keep: n_parts(mode) x (n + 1) words, entry n of each column zeroed by the caller; bad, past preset ~0
static hipError_t launch_fastq_sizes(const uint8_t *U, const uint64_t *pos, uint64_t n, uint64_t total, const sbh_bam::Filter &F,
                                     uint32_t mode, uint64_t *len, uint64_t *keep, uint8_t *cls, unsigned long long *bad,
                                     unsigned long long *past, hipStream_t st) {
  hipLaunchKernelGGL(k_fastq_sizes, dim3(rows_grid(n)), dim3(256), 0, st, U, pos, n, total, F, mode, n + 1, len, keep, cls,
                     bad, past);
  return hipGetLastError();
}

// off: n words; rec_off, rows: n + 1 words; sums: 2 PARTS words
static hipError_t launch_fastq_index(const uint64_t *len, const uint64_t *lpre, const uint64_t *kpre, const uint8_t *cls,
                                     uint64_t n, uint32_t mode, uint64_t *off, uint64_t *rec_off, uint64_t *rows,
                                     uint64_t *sums, hipStream_t st) {
  hipLaunchKernelGGL(k_fastq_index, dim3(rows_grid(n + 1)), dim3(256), 0, st, len, lpre, kpre, cls, n, mode, n + 1, off,
                     rec_off, rows, sums);
  return hipGetLastError();
}

// text: `total` bytes from a hipMalloc'd base
static hipError_t launch_fastq_emit(const uint8_t *U, const uint64_t *pos, uint64_t n, const uint64_t *len, const uint64_t *off,
                                    const uint8_t *cls, uint32_t mode, int32_t def_qual, uint64_t total, char *text,
                                    hipStream_t st) {
  if (!total) return hipSuccess;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 3) / 4, EMIT_GRID);
  hipLaunchKernelGGL(k_fastq_emit, dim3(grid), dim3(256), 0, st, U, pos, n, len, off, cls, mode, def_qual, n + 1, total,
                     text);
  return hipGetLastError();
}

}  // namespace sbh

using namespace sbh;

static bool fastq_args_ok(uint32_t mode, int32_t def_qual) {
  return !(mode & ~sbh_fq::MODE_ALL) && def_qual >= 0 && def_qual <= sbh_fq::QUAL_MAX;
}

extern "C" {

// ---- the C-ABI's FASTQ / FASTA calls (the line is defined in fastq_core.h) ---------------------
// Size pass, the scans and the index pass are launched before anything is read back, so one round
// trip brings (first bad row, first row past the end, the parts' bytes and lines); then the text is
// allocated and written.
int sbh_records_fastq_scan(sbh_shard *sh, const sbh_record_filter *filter, uint32_t mode, int32_t def_qual,
                           sbh_fastq_sizes *out) {
  if (!sh || !out) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &R = sh->rec;
  auto &Q = sh->fq;
  if (!R.valid) return fail(ctx, SBH_E_STATE, "records_fastq_scan without a records scan");
  if (!fastq_args_ok(mode, def_qual))
    return fail(ctx, SBH_E_ARG, "records_fastq_scan: mode 0x%x has unknown bits, or def_qual %d is outside [0, 93]", mode, def_qual);
  sbh_bam::Filter F;
  int rc = row_filter(ctx, filter, &F);
  if (rc) return rc;
  const uint64_t n = R.sz.n, np = sbh_fq::n_parts(mode);
  rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  Q.valid = false;
  sbh_fastq_sizes sz{n, 0, 0, {0, 0, 0}, {0, 0, 0}};
  HIPCHK(ctx, Q.rec_off.ensure(n + 1));
  HIPCHK(ctx, Q.text.ensure(16));  // (a text of no bytes has a pointer too)
  if (!n) {
    HIPCHK(ctx, hipMemsetAsync(Q.rec_off.p, 0, 8, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  } else {
    for (auto *b : {&Q.len, &Q.keep, &Q.lpre, &Q.kpre}) HIPCHK(ctx, b->ensure(np * (n + 1)));
    for (auto *b : {&Q.off, &Q.rows}) HIPCHK(ctx, b->ensure(n + 1));
    HIPCHK(ctx, Q.cls.ensure(n));
    HIPCHK(ctx, Q.sums.ensure(2 * sbh_fq::PARTS));
    HIPCHK(ctx, sh->tmp.ensure(scan_tmp_words(n + 1)));
    HIPCHK(ctx, stage_row_ranges(sh, &F));
    for (uint64_t q = 0; q < np; ++q) {
      HIPCHK(ctx, hipMemsetAsync(Q.len.p + q * (n + 1) + n, 0, 8, st));
      HIPCHK(ctx, hipMemsetAsync(Q.keep.p + q * (n + 1) + n, 0, 8, st));
    }
    unsigned long long *bad = sh->ctr.p + ctr::FASTQ_BAD;  // (FASTQ_PAST is the next word)
    static_assert(ctr::FASTQ_PAST == ctr::FASTQ_BAD + 1, "one memset, one copy");
    HIPCHK(ctx, hipMemsetAsync(bad, 0xff, 16, st));
    HIPCHK(ctx, launch_fastq_sizes(sh->U.p, R.pos.p, n, sh->utotal, F, mode, Q.len.p, Q.keep.p, Q.cls.p, bad, bad + 1, st));
    for (uint64_t q = 0; q < np; ++q) {
      HIPCHK(ctx, scan_exclusive_u64(Q.len.p + q * (n + 1), Q.lpre.p + q * (n + 1), n + 1, sh->tmp.p, st));
      HIPCHK(ctx, scan_exclusive_u64(Q.keep.p + q * (n + 1), Q.kpre.p + q * (n + 1), n + 1, sh->tmp.p, st));
    }
    HIPCHK(ctx, launch_fastq_index(Q.len.p, Q.lpre.p, Q.kpre.p, Q.cls.p, n, mode, Q.off.p, Q.rec_off.p, Q.rows.p, Q.sums.p, st));
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::FASTQ_BAD, bad, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_FASTQ_SUMS, Q.sums.p, 8 * 2 * sbh_fq::PARTS, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    rc = rows_verdict(sh, sh->h_ctr[ctr::FASTQ_BAD], sh->h_ctr[ctr::FASTQ_PAST], "");
    if (rc) return rc;
    for (uint32_t q = 0; q < sbh_fq::PARTS; ++q) {
      sz.part_bytes[q] = sh->h_ctr[ctr::H_FASTQ_SUMS + q];
      sz.part_rows[q] = sh->h_ctr[ctr::H_FASTQ_SUMS + sbh_fq::PARTS + q];
      sz.text_bytes += sz.part_bytes[q], sz.n_kept += sz.part_rows[q];
    }
    HIPCHK(ctx, Q.text.ensure(sz.text_bytes + 16));  // (the compressor reads whole aligned words)
    HIPCHK(ctx, launch_fastq_emit(sh->U.p, R.pos.p, n, Q.len.p, Q.off.p, Q.cls.p, mode, def_qual, sz.text_bytes, Q.text.p, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  Q.sz = sz;
  Q.valid = true;
  *out = sz;
  return SBH_OK;
}

const void *sbh_records_fastq_device_ptr(sbh_shard *sh) { return sh && sh->fq.valid ? sh->fq.text.p : nullptr; }

int sbh_records_fastq_fetch(sbh_shard *sh, char *text, uint64_t *rec_off, uint64_t *rows) {
  if (!sh) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &Q = sh->fq;
  if (!Q.valid) return fail(ctx, SBH_E_STATE, "records_fastq_fetch without a records_fastq_scan");
  int rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  if (text && Q.sz.text_bytes) HIPCHK(ctx, hipMemcpyAsync(text, Q.text.p, Q.sz.text_bytes, hipMemcpyDeviceToHost, st));
  if (rec_off) HIPCHK(ctx, hipMemcpyAsync(rec_off, Q.rec_off.p, 8 * (Q.sz.n_kept + 1), hipMemcpyDeviceToHost, st));
  if (rows && Q.sz.n_kept) HIPCHK(ctx, hipMemcpyAsync(rows, Q.rows.p, 8 * Q.sz.n_kept, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return SBH_OK;
}

int sbh_fastq_render_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                          const sbh_record_filter *filter, uint32_t mode, int32_t def_qual, char *text, uint64_t text_cap,
                          uint64_t *rec_off, uint64_t *rows, sbh_fastq_sizes *sizes, uint64_t *bad_row) {
  if ((!flat && flat_size) || (!starts && n) || !sizes || !fastq_args_ok(mode, def_qual)) return SBH_E_ARG;
  sbh_bam::Filter F;
  if (!bam_filter_of(filter, &F)) return SBH_E_ARG;
  uint64_t bad = sbh_bam::NO_ROW;
  const int rc = sbh_fq::render_host(flat, flat_size, starts, n, F, mode, def_qual, text, text_cap, rec_off, rows,
                                     reinterpret_cast<sbh_fq::Sizes *>(sizes), &bad);
  if (bad_row) *bad_row = bad;
  return rc == 0 ? SBH_OK : rc == 1 ? SBH_E_BAD_RECORD : SBH_E_ARG;
}

}  // extern "C"
