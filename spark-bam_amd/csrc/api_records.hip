// api_records.hip -- the C-ABI's record stage (host only): record starts by the chain and the
// column decode (records.hip) for a range, one split, a batch of splits and BAI chunks with a
// region filter; the fetch of the decoded columns.
#include <algorithm>
#include <cstring>
#include <vector>

#include "sbh_host.h"

using namespace sbh;

extern "C" {

// RecordStream + BAMRecordCodec.decode over [first, end) (check/.../iterator/RecordStream.scala:16-41,
// load/.../CanLoadBam.scala:244-264): record starts by the chain, sizes -> prefix offsets,
// then one wave per record decodes into the columns.
int sbh_records_scan(sbh_shard *sh, uint64_t first, uint64_t end_flat, sbh_records_sizes *out) {
  if (!sh || !out) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  if (!sh->inflated) return fail(ctx, SBH_E_STATE, "records before inflate");
  if (first > sh->utotal) return SBH_E_ARG;
  int rc = set_device(ctx);
  if (rc) return rc;
  auto &R = sh->rec;
  R.valid = false;
  sh->sam.valid = false;
  sh->bam.valid = false;
  sh->fq.valid = false;
  const uint64_t total = seg_end_of(sh, first);
  const uint64_t E = std::min(std::min(end_flat, sh->utotal), total);
  uint64_t n = 0;
  int32_t anomalies = 0;
  rc = count_records_impl(sh, first, E, &n, &anomalies);
  if (rc) return rc;
  HIPCHK(ctx, R.pos.ensure(n));
  rc = records_positions(sh, first, E, total, n, anomalies, R.pos.p);
  if (rc) return rc;
  return records_finish(sh, n, total, out);
}

// One FileSplit of loadReadsAndPositions (load/.../CanLoadBam.scala:316-356) in one call:
// FindBlockStart(start) (FindBlockStart.scala:8-36), then sbh_run_shard's step from that block --
// MetadataStream + inflate + the eager check at every position of [Pos(blockStart, 0), Pos(end, 0))
// + FindRecordStart from Pos(blockStart, 0) (FindRecordStart.scala:11-30) + the chain proof of the
// records while pos < Pos(end, 0) (RecordStream.takeWhile, :338-355) -- then the record starts (and
// with decode, BAMRecordCodec.decode's columns) for sbh_records_fetch.  The per-split facade
// (jni/Native.scala GpuSplitPartition) made seven calls with a host round trip each.
int sbh_split_records(sbh_shard *sh, uint64_t start, uint64_t end, int32_t k, int32_t rtc, int32_t mrs, int32_t decode,
                      sbh_split_records_result *out) {
  if (!sh || !out || end <= start) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  std::memset(out, 0, sizeof *out);
  int rc = set_device(ctx);
  if (rc) return rc;
  auto &R = sh->rec;
  R.valid = R.decoded = false;
  sh->sam.valid = false;
  sh->bam.valid = false;
  sh->fq.valid = false;
  uint64_t b = 0;
  rc = sbh_find_block_start(sh, start, k, &b);
  if (rc) return rc;
  out->block_start = b;
  sbh_shard_result r{};
  rc = sbh_run_shard(sh, b, end, rtc, mrs, &r);
  if (rc) return rc;
  out->n_blocks = sh->nblocks;
  out->flat_size = sh->utotal;
  out->owned_flat = r.flat_bytes;
  out->n_true = r.n_true;
  uint64_t first = sh->run_first;
  if (r.count == 0) {
    // no record of the chain below Pos(end, 0): FindRecordStart's own answer decides between an
    // empty split and NoReadFoundException(path, blockStart, maxReadSize)
    int32_t delta = 0;
    rc = sbh_find_record_start(sh, 0, rtc, mrs, &first, &delta);
    if (rc == SBH_E_NO_READ_FOUND)
      return fail_with(ctx, SBH_E_NO_READ_FOUND, {(int64_t)b, mrs},
                       "Failed to find a valid read-start in %d attempts from %llu", mrs, (unsigned long long)b);
    if (rc) return rc;
    out->first_flat = first;
    R.sz = sbh_records_sizes{0, 0, 0, 0, 0};
    R.valid = true;
    R.decoded = decode != 0;
    return SBH_OK;
  }
  out->first_flat = first;
  out->first_vpos = r.first_vpos;
  const uint64_t total = seg_end_of(sh, first);
  const uint64_t E = std::min(std::min(r.flat_bytes, sh->utotal), total);
  HIPCHK(ctx, R.pos.ensure(r.count));
  rc = records_positions(sh, first, E, total, r.count, r.anomalies, R.pos.p);
  if (rc) return rc;
  if (!decode) {
    HIPCHK(ctx, hipStreamSynchronize(sh->st));
    R.sz = sbh_records_sizes{r.count, 0, 0, 0, 0};
    R.valid = true;
    out->sizes = R.sz;
    return SBH_OK;
  }
  rc = records_finish(sh, r.count, total, &out->sizes);
  // the split's last record runs past the resident bytes: more halo, not a malformed record
  if (rc == SBH_E_BAD_RECORD && !sh->at_eof)
    return fail(ctx, SBH_E_NEED_HALO, "a record of the split runs past the shard");
  return rc;
}

// sbh_split from block bi on, for a split whose FindBlockStart lands on an empty block.  sbh_split
// answers NoReadFoundException there (the stream from an empty block ends at once);
// sbh_split_records, indexing from that block, searches on in the segment behind it.  The batch
// answers as sbh_split_records does: the search starts at the empty block's flat position.
static int split_behind_empty_block(sbh_shard *sh, int64_t bi, uint64_t end, int32_t rtc, int32_t mrs,
                                    uint64_t *first_vpos, uint64_t *count) {
  uint64_t first = 0, E = 0;
  int32_t delta = 0;
  int rc = sbh_find_record_start(sh, sh->hb[bi].ustart, rtc, mrs, &first, &delta);
  if (rc) return rc;
  (void)sbh_flat_bound(sh, end, &E);
  if (!sh->at_eof && E == sh->utotal)
    return fail(sh->ctx, SBH_E_NEED_HALO, "split end %llu past the resident blocks", (unsigned long long)end);
  rc = count_records_impl(sh, first, E, count, nullptr);
  if (rc) return rc;
  uint64_t bp = 0;
  uint32_t off = 0;
  rc = sbh_pos_of(sh, first, &bp, &off);
  if (rc) return rc;
  *first_vpos = (bp << 16) | off;
  return SBH_OK;
}

// Many FileSplits of one shard in one call: sbh_split_records' answer for every split [starts[i],
// ends[i]) from ONE pass over their bytes -- FindBlockStart(starts[0]), sbh_run_shard from that
// block to the last end, sbh_split_starts for all splits, the record starts of every split in one
// launch set (launch_rec_positions_ranges over the verified bitmap), one records_finish.  The
// batch's rows are the splits' records in split order; split i owns rows [rec_begin, + rec_count).
int sbh_split_records_batch(sbh_shard *sh, const uint64_t *starts, const uint64_t *ends, uint64_t n, int32_t k,
                            int32_t rtc, int32_t mrs, int32_t decode, sbh_batch_split *splits,
                            sbh_split_batch_result *out) {
  if (!sh || !out || !n || !starts || !ends || !splits || k < 0) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  std::memset(out, 0, sizeof *out);
  std::memset(splits, 0, n * sizeof *splits);
  for (uint64_t i = 0; i < n; ++i)
    if (starts[i] >= ends[i] || (i + 1 < n && ends[i] > starts[i + 1]))
      return fail(ctx, SBH_E_ARG, "splits must be ascending and disjoint (split %llu)", (unsigned long long)i);
  if (starts[0] < sh->file_off || starts[0] >= sh->file_off + sh->n)
    return fail(ctx, SBH_E_ARG, "the first split starts outside the shard");
  int rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  auto &R = sh->rec;
  R.valid = R.decoded = false;
  sh->sam.valid = false;
  sh->bam.valid = false;
  sh->fq.valid = false;
  // the chain starts at the first split whose FindBlockStart succeeds; a split before it keeps
  // its own failure (HeaderSearchFailedException(path, start, positionsAttempted))
  uint64_t j0 = 0, b = 0;
  for (; j0 < n; ++j0) {
    rc = starts[j0] < sh->file_off + sh->n ? sbh_find_block_start(sh, starts[j0], k, &b) : SBH_E_NEED_HALO;
    if (rc == SBH_OK) break;
    if (rc == SBH_E_ARG || rc == SBH_E_HIP || rc == SBH_E_NOMEM) return rc;
    splits[j0].status = rc;
  }
  if (j0 == n) {
    R.sz = sbh_records_sizes{0, 0, 0, 0, 0};
    R.valid = true;
    R.decoded = decode != 0;
    return SBH_OK;
  }
  out->block_start = b;
  sbh_shard_result r{};
  rc = sbh_run_shard(sh, b, ends[n - 1], rtc, mrs, &r);
  if (rc == SBH_E_NEED_HALO) {
    // the last end has no block behind it in the resident bytes (or an answer of the step needs
    // the halo): index and inflate what is there; sbh_split_starts runs the eager check over it
    // and every split decides alone, NEED_HALO where its own answer needs the missing bytes
    rc = sbh_index(sh, b, nullptr, nullptr);
    if (!rc) rc = sbh_inflate(sh, nullptr);
    r = sbh_shard_result{};
  }
  if (rc) return rc;
  out->n_blocks = sh->nblocks;
  out->flat_size = sh->utotal;
  out->n_true = r.n_true;
  const uint64_t m = n - j0;
  std::vector<uint64_t> fv(m, 0), cnt(m, 0);
  std::vector<int32_t> stat(m, 0);
  std::vector<uint8_t> hostf(m, 0);
  rc = split_starts_impl(sh, starts + j0, ends + j0, m, k, rtc, mrs, fv.data(), cnt.data(), stat.data(), &out->n_host,
                         hostf.data());
  if (rc) return rc;
  // per split: FindBlockStart's block, the flat range of its records, its rows
  std::vector<uint64_t> in(3 * n, 0);  // [first, E, reserve] x n, normalised: sorted, empty = [cursor, cursor)
  uint64_t *hf = in.data(), *hE = hf + n, *hres = hE + n;
  uint64_t rows = 0, U0 = ~0ull, U1 = 0;
  for (uint64_t i = j0; i < n; ++i) {
    sbh_batch_split &s = splits[i];
    s.status = stat[i - j0];
    s.host_path = hostf[i - j0];
    s.rec_begin = rows;
    if (s.status != SBH_OK && s.status != SBH_E_NO_READ_FOUND) continue;
    if (s.host_path) {
      if (sbh_find_block_start(sh, starts[i], k, &s.block_start) != SBH_OK) s.block_start = 0;
    } else {
      auto it = std::lower_bound(sh->hb.begin(), sh->hb.end(), starts[i],
                                 [](const sbh_block &bl, uint64_t v) { return bl.start < v; });
      s.block_start = it == sh->hb.end() ? 0 : it->start;
    }
    const int64_t bi = block_index_of(sh, s.block_start);
    if (s.status == SBH_E_NO_READ_FOUND && bi >= 0 && (sh->hb[bi].flags & SBH_BLOCK_EMPTY)) {
      s.status = split_behind_empty_block(sh, bi, ends[i], rtc, mrs, &fv[i - j0], &cnt[i - j0]);
      if (s.status == SBH_E_ARG || s.status == SBH_E_HIP || s.status == SBH_E_NOMEM) return s.status;
      if (!s.host_path) ++out->n_host;
      s.host_path = 1;
      if (s.status != SBH_OK && s.status != SBH_E_NO_READ_FOUND) continue;
    }
    (void)sbh_flat_bound(sh, ends[i], &s.owned_flat);
    if (s.status != SBH_OK || !cnt[i - j0]) continue;
    rc = sbh_flat_of(sh, fv[i - j0] >> 16, (uint32_t)(fv[i - j0] & 0xffff), &s.first_flat);
    if (rc) return rc;
    s.first_vpos = fv[i - j0];
    s.rec_count = cnt[i - j0];
    rows += s.rec_count;
  }
  uint64_t cursor = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const sbh_batch_split &s = splits[i];
    hf[i] = hE[i] = cursor;
    if (!s.rec_count) continue;
    const uint64_t E = std::min(std::min(s.owned_flat, sh->utotal), seg_end_of(sh, s.first_flat));
    if (s.host_path || s.first_flat < cursor || s.first_flat >= E) {  // (its records by the chain walk)
      hres[i] = s.rec_count;
      continue;
    }
    hf[i] = s.first_flat;
    hE[i] = cursor = E;
    U0 = std::min(U0, hf[i]);
    U1 = E;
  }
  HIPCHK(ctx, R.pos.ensure(rows + 1));
  std::vector<uint64_t> off(n + 1, 0);
  const bool covered = U0 < U1 && sh->bits_valid && sh->bits_begin <= U0 && U1 <= sh->bits_end;
  if (U0 < U1 && !covered)  // no bitmap over the ranges: every split by the chain walk
    for (uint64_t i = 0; i < n; ++i) {
      hf[i] = hE[i] = 0;
      hres[i] = splits[i].rec_count;
    }
  if (covered) {
    for (uint64_t i = 0; i < n; ++i)  // (empty ranges before the first live one: inside the union)
      if (hf[i] < U0) hf[i] = hE[i] = U0;
    const uint64_t nw = (U1 - sh->bits_begin + 31) / 32 - (U0 - sh->bits_begin) / 32;
    HIPCHK(ctx, R.wcnt.ensure(nw + 2));
    HIPCHK(ctx, R.wpre.ensure(nw));
    HIPCHK(ctx, sh->tmp.ensure(std::max(scan_tmp_words(nw), scan_tmp_words(n + 1))));
    HIPCHK(ctx, R.bt_in.ensure(3 * n));
    HIPCHK(ctx, R.bt_rbase.ensure(n));
    HIPCHK(ctx, R.bt_cnt.ensure(n + 1));
    HIPCHK(ctx, R.bt_off.ensure(n + 1));
    HIPCHK(ctx, hipMemcpyAsync(R.bt_in.p, in.data(), 24 * n, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, launch_rec_positions_ranges(sh->bits.p, sh->bits_begin, U0, U1, R.bt_in.p, R.bt_in.p + n,
                                            R.bt_in.p + 2 * n, n, R.wcnt.p, R.wpre.p, sh->tmp.p, R.bt_rbase.p,
                                            R.bt_cnt.p, R.bt_off.p, rows, R.pos.p, st));
    HIPCHK(ctx, hipMemcpyAsync(off.data(), R.bt_off.p, 8 * (n + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  // the layout the splits' counts give; where the bitmap's agrees the rows are in place
  bool moved = false;
  for (uint64_t i = 0; i < n && !moved; ++i)
    moved = covered && (off[i] != splits[i].rec_begin || off[i + 1] - off[i] != splits[i].rec_count);
  uint64_t *dst = R.pos.p;
  if (moved) {
    // set bits off the chain inside a range (false positives): the splits whose bitmap count
    // is their record count keep their rows (copied to their place), the others walk the chain
    HIPCHK(ctx, R.pos2.ensure(rows + 1));
    dst = R.pos2.p;
  }
  for (uint64_t i = 0; i < n; ++i) {
    const sbh_batch_split &s = splits[i];
    if (!s.rec_count) continue;
    const bool by_bits = covered && !hres[i] && off[i + 1] - off[i] == s.rec_count && off[i + 1] <= rows;
    if (by_bits && !moved) continue;
    if (by_bits) {
      HIPCHK(ctx, hipMemcpyAsync(dst + s.rec_begin, R.pos.p + off[i], 8 * s.rec_count, hipMemcpyDeviceToDevice, st));
      continue;
    }
    const uint64_t total = seg_end_of(sh, s.first_flat);
    HIPCHK(ctx, launch_rec_positions_chain(sh->U.p, s.first_flat, std::min(std::min(s.owned_flat, sh->utotal), total),
                                           total, s.rec_count, dst + s.rec_begin, st));
  }
  if (moved) std::swap(R.pos, R.pos2);
  out->sizes = sbh_records_sizes{rows, 0, 0, 0, 0};
  // A record over the end of its stream segment.  Starts only: the batch's last record against
  // an open shard end, so decode = 0 asks for the halo where decode = 1 does.  Decoding: the size
  // pass below measures every record against the resident bytes' end; where empty blocks cut
  // the stream into segments, each record against its own segment's end first (sbh_split_records
  // measures a split's records against the end of the segment its first record lies in).
  unsigned long long *bad = sh->ctr.p + ctr::REC_SEG_BAD;
  if (rows && (decode ? sh->seg_end.size() > 1 : !sh->at_eof)) {
    HIPCHK(ctx, hipMemsetAsync(bad, 0xff, 8, st));
    HIPCHK(ctx, launch_rec_seg_check(sh->U.p, decode ? R.pos.p : R.pos.p + rows - 1, decode ? rows : 1, sh->d_seg.p,
                                     (uint32_t)sh->seg_end.size(), bad, st));
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::REC_SEG_BAD, bad, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (sh->h_ctr[ctr::REC_SEG_BAD] != ~0ull)
      return sh->at_eof ? fail(ctx, SBH_E_BAD_RECORD, "a record of the batch runs over the end of the stream")
                        : fail(ctx, SBH_E_NEED_HALO, "a record of the batch runs past the shard");
  }
  if (!decode) {
    HIPCHK(ctx, hipStreamSynchronize(st));
    R.sz = out->sizes;
    R.valid = true;
    return SBH_OK;
  }
  rc = records_finish(sh, rows, sh->utotal, &out->sizes);
  if (rc == SBH_E_BAD_RECORD && !sh->at_eof)
    return fail(ctx, SBH_E_NEED_HALO, "a record of the batch runs past the shard");
  return rc;
}

}  // extern "C"

// Record starts of the chain from first while the start is < E, written at pos (cap n).
int sbh::records_positions(sbh_shard *sh, uint64_t first, uint64_t E, uint64_t total, uint64_t n, int32_t anomalies,
                           uint64_t *pos) {
  sbh_ctx *ctx = sh->ctx;
  hipStream_t st = sh->st;
  auto &R = sh->rec;
  const bool covered = sh->bits_valid && sh->bits_begin <= first && E <= sh->bits_end && anomalies == 0;
  if (n && covered) {
    const uint64_t nw = (E - sh->bits_begin + 31) / 32 - (first - sh->bits_begin) / 32;
    HIPCHK(ctx, R.wcnt.ensure(nw + 2));  // (chunk sums + prefix: 2 per 4096 words)
    HIPCHK(ctx, R.wpre.ensure(nw));
    HIPCHK(ctx, sh->tmp.ensure(scan_tmp_words(nw)));
    HIPCHK(ctx, launch_rec_positions_bits(sh->bits.p, sh->bits_begin, first, E, R.wcnt.p, R.wpre.p, sh->tmp.p, pos, st));
  } else if (n && sh->cm_valid && sh->cm_first == first && sh->cm_E == E) {
    // the chain marked by count_records_impl's pointer doubling: compact its nodes
    HIPCHK(ctx, launch_compact_u64(sh->cm_pos.p, sh->cm_mark.p, sh->cm_mpre.p, sh->cm_n, pos, st));
  } else if (n) {
    HIPCHK(ctx, launch_rec_positions_chain(sh->U.p, first, E, total, n, pos, st));
  }
  return SBH_OK;
}

// Sizes -> prefix offsets -> columns for the n record starts in R.pos.
int sbh::records_finish(sbh_shard *sh, uint64_t n, uint64_t total, sbh_records_sizes *out) {
  sbh_ctx *ctx = sh->ctx;
  hipStream_t st = sh->st;
  auto &R = sh->rec;
  // per-record sizes (a trailing zero makes the exclusive scan's last entry the total)
  DBuf<uint64_t> *sz[4] = {&R.nm, &R.cg, &R.sq, &R.ax}, *of[4] = {&R.nmo, &R.cgo, &R.sqo, &R.axo};
  for (int k = 0; k < 4; ++k) {
    HIPCHK(ctx, sz[k]->ensure(n + 1));
    HIPCHK(ctx, of[k]->ensure(n + 1));
    HIPCHK(ctx, hipMemsetAsync(sz[k]->p + n, 0, 8, st));
  }
  unsigned long long *bad = sh->ctr.p + ctr::REC_BAD;
  HIPCHK(ctx, hipMemsetAsync(bad, 0xff, 8, st));
  HIPCHK(ctx, launch_rec_sizes(sh->U.p, R.pos.p, n, total, R.nm.p, R.cg.p, R.sq.p, R.ax.p, bad, st));
  HIPCHK(ctx, sh->tmp.ensure(scan_tmp_words(n + 1)));
  for (int k = 0; k < 4; ++k) HIPCHK(ctx, scan_exclusive_u64(sz[k]->p, of[k]->p, n + 1, sh->tmp.p, st));
  uint64_t tot[4] = {0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) HIPCHK(ctx, hipMemcpyAsync(&tot[k], of[k]->p + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::REC_BAD, bad, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (sh->h_ctr[ctr::REC_BAD] != ~0ull)
    return fail(ctx, SBH_E_BAD_RECORD, "record %llu of the range is malformed",
                (unsigned long long)sh->h_ctr[ctr::REC_BAD]);
  HIPCHK(ctx, R.ref_id.ensure(n)); HIPCHK(ctx, R.p0.ensure(n)); HIPCHK(ctx, R.nref.ensure(n));
  HIPCHK(ctx, R.npos.ensure(n)); HIPCHK(ctx, R.tlen.ensure(n)); HIPCHK(ctx, R.flag.ensure(n));
  HIPCHK(ctx, R.bin.ensure(n)); HIPCHK(ctx, R.mapq.ensure(n));
  HIPCHK(ctx, R.names.ensure(tot[0])); HIPCHK(ctx, R.cigar.ensure(tot[1]));
  HIPCHK(ctx, R.seq.ensure(tot[2])); HIPCHK(ctx, R.qual.ensure(tot[2])); HIPCHK(ctx, R.aux.ensure(tot[3]));
  const RecCols cols{R.ref_id.p, R.p0.p, R.nref.p, R.npos.p, R.tlen.p, R.flag.p, R.bin.p, R.mapq.p,
                     R.names.p, R.cigar.p, R.seq.p, R.qual.p, R.aux.p};
  HIPCHK(ctx, launch_rec_fields(sh->U.p, R.pos.p, n, R.nmo.p, R.cgo.p, R.sqo.p, R.axo.p, cols, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  R.sz = sbh_records_sizes{n, tot[0], tot[1], tot[2], tot[3]};
  R.valid = true;
  R.decoded = true;
  *out = R.sz;
  return SBH_OK;
}

extern "C" {

// loadBamIntervals (load/.../CanLoadBam.scala:78-154): for each BAI chunk, the records from
// chunk.start while the start is < chunk.end (records.seek(chunk.start) + takeWhile), then the
// region filter on the device, then the same column decode as sbh_records_scan.
int sbh_records_scan_regions(sbh_shard *sh, const uint64_t *chunk_begin, const uint64_t *chunk_end, uint64_t n_chunks,
                             const int32_t *iv_ref, const int64_t *iv_begin, const int64_t *iv_end, uint32_t n_iv,
                             sbh_records_sizes *out) {
  if (!sh || !out || (n_chunks && (!chunk_begin || !chunk_end)) || (n_iv && (!iv_ref || !iv_begin || !iv_end)))
    return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  if (!sh->inflated) return fail(ctx, SBH_E_STATE, "records before inflate");
  for (uint32_t k = 0; k < n_iv; ++k) {
    if (iv_begin[k] >= iv_end[k]) return fail(ctx, SBH_E_ARG, "interval %u is empty", k);
    if (k && (iv_ref[k] < iv_ref[k - 1] || (iv_ref[k] == iv_ref[k - 1] && iv_begin[k] < iv_end[k - 1])))
      return fail(ctx, SBH_E_ARG, "intervals must be sorted by (ref, begin) and disjoint");
  }
  int rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  auto &R = sh->rec;
  R.valid = false;
  sh->sam.valid = false;
  sh->bam.valid = false;
  sh->fq.valid = false;
  std::vector<uint64_t> cn(n_chunks, 0), cfirst(n_chunks, 0), cE(n_chunks, 0), ctot(n_chunks, 0);
  std::vector<int32_t> can(n_chunks, 0);
  uint64_t n = 0;
  for (uint64_t c = 0; c < n_chunks; ++c) {
    const uint64_t first = chunk_begin[c];
    if (first > sh->utotal) return fail(ctx, SBH_E_ARG, "chunk %llu starts past the stream", (unsigned long long)c);
    ctot[c] = seg_end_of(sh, first);
    cE[c] = std::min(std::min(chunk_end[c], sh->utotal), ctot[c]);
    cfirst[c] = first;
    if (first < cE[c]) {
      rc = count_records_impl(sh, first, cE[c], &cn[c], &can[c]);
      if (rc) return rc;
    }
    n += cn[c];
  }
  HIPCHK(ctx, R.pos2.ensure(n + 1));
  uint64_t o = 0;
  for (uint64_t c = 0; c < n_chunks; ++c) {
    rc = records_positions(sh, cfirst[c], cE[c], ctot[c], cn[c], can[c], R.pos2.p + o);
    if (rc) return rc;
    o += cn[c];
  }
  HIPCHK(ctx, R.keep.ensure(n + 1));
  HIPCHK(ctx, R.kpre.ensure(n + 1));
  HIPCHK(ctx, R.iv_ref.ensure(n_iv + 1));
  HIPCHK(ctx, R.iv_b.ensure(n_iv + 1));
  HIPCHK(ctx, R.iv_e.ensure(n_iv + 1));
  if (n_iv) {
    HIPCHK(ctx, hipMemcpyAsync(R.iv_ref.p, iv_ref, 4ull * n_iv, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(R.iv_b.p, iv_begin, 8ull * n_iv, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(R.iv_e.p, iv_end, 8ull * n_iv, hipMemcpyHostToDevice, st));
  }
  HIPCHK(ctx, hipMemsetAsync(R.keep.p + n, 0, 8, st));
  HIPCHK(ctx, launch_region_keep(sh->U.p, R.pos2.p, n, sh->utotal, R.iv_ref.p, R.iv_b.p, R.iv_e.p, n_iv, R.keep.p, st));
  HIPCHK(ctx, sh->tmp.ensure(scan_tmp_words(n + 1)));
  HIPCHK(ctx, scan_exclusive_u64(R.keep.p, R.kpre.p, n + 1, sh->tmp.p, st));
  uint64_t kept = 0;
  HIPCHK(ctx, hipMemcpyAsync(&kept, R.kpre.p + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, R.pos.ensure(kept + 1));
  HIPCHK(ctx, launch_compact_u64(R.pos2.p, R.keep.p, R.kpre.p, n, R.pos.p, st));
  return records_finish(sh, kept, sh->utotal, out);
}

int sbh_records_fetch(sbh_shard *sh, const sbh_records_out *o) {
  if (!sh || !o) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &R = sh->rec;
  if (!R.valid) return fail(ctx, SBH_E_STATE, "records_fetch without a records_scan");
  if (!R.decoded && (o->ref_id || o->pos || o->next_ref_id || o->next_pos || o->tlen || o->flag || o->bin || o->mapq ||
                     o->name_off || o->cigar_off || o->seq_off || o->aux_off || o->names || o->cigar || o->seq ||
                     o->qual || o->aux))
    return fail(ctx, SBH_E_STATE, "records_fetch: only the starts were scanned (sbh_split_records, decode = 0)");
  int rc = set_device(ctx);
  if (rc) return rc;
  const uint64_t n = R.sz.n;
  if (o->vpos && n) {  // the starts' virtual positions, computed on the device from the block table
    HIPCHK(ctx, R.vpos.ensure(n));
    HIPCHK(ctx, launch_rec_vpos(R.pos.p, n, sh->dev_blocks(), sh->nblocks, sh->file_off, R.vpos.p, sh->st));
    HIPCHK(ctx, hipMemcpyAsync(o->vpos, R.vpos.p, 8 * n, hipMemcpyDeviceToHost, sh->st));
  }
  // (every column is copied on the shard's stream, then one wait)
  auto cp = [&](void *dst, const void *src, uint64_t bytes) -> hipError_t {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, sh->st) : hipSuccess;
  };
  HIPCHK(ctx, cp(o->flat, R.pos.p, 8 * n));
  HIPCHK(ctx, cp(o->ref_id, R.ref_id.p, 4 * n));
  HIPCHK(ctx, cp(o->pos, R.p0.p, 4 * n));
  HIPCHK(ctx, cp(o->next_ref_id, R.nref.p, 4 * n));
  HIPCHK(ctx, cp(o->next_pos, R.npos.p, 4 * n));
  HIPCHK(ctx, cp(o->tlen, R.tlen.p, 4 * n));
  HIPCHK(ctx, cp(o->flag, R.flag.p, 2 * n));
  HIPCHK(ctx, cp(o->bin, R.bin.p, 2 * n));
  HIPCHK(ctx, cp(o->mapq, R.mapq.p, n));
  HIPCHK(ctx, cp(o->name_off, R.nmo.p, 8 * (n + 1)));
  HIPCHK(ctx, cp(o->cigar_off, R.cgo.p, 8 * (n + 1)));
  HIPCHK(ctx, cp(o->seq_off, R.sqo.p, 8 * (n + 1)));
  HIPCHK(ctx, cp(o->aux_off, R.axo.p, 8 * (n + 1)));
  HIPCHK(ctx, cp(o->names, R.names.p, R.sz.name_bytes));
  HIPCHK(ctx, cp(o->cigar, R.cigar.p, 4 * R.sz.cigar_ops));
  HIPCHK(ctx, cp(o->seq, R.seq.p, R.sz.bases));
  HIPCHK(ctx, cp(o->qual, R.qual.p, R.sz.bases));
  HIPCHK(ctx, cp(o->aux, R.aux.p, R.sz.aux_bytes));
  HIPCHK(ctx, hipStreamSynchronize(sh->st));
  return SBH_OK;
}

}  // extern "C"
