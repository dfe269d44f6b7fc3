// sbh_host.h -- the host side's private header: the context, the shard and the other structs
// behind the opaque handles of include/sparkbam.h, the error helpers, and the host helpers that
// one file's entry points (sbh_api.hip, api_check.hip, api_records.hip, and the output stages' calls
// behind the kernels of bai.hip, sam.hip, bam_gather.hip, depth.hip, pileup.hip, tally.hip, stats.hip,
// fastq.hip, zdeflate.hip) borrow from another's.  Launchers are declared in sbh_internal.h; nothing
// here is seen by device code.
//
// The stages that run over the rows of the last records scan under an sbh_record_filter
// (bam_gather.hip, depth.hip, pileup.hip, tally.hip, fastq.hip, stats.hip) share one frame, declared at the end
// of this header and defined in bam_gather.hip: row_filter (the filter and its one message),
// stage_row_ranges (the device copy of the row ranges, sbh_shard::row_ranges) and rows_verdict (bad
// row, past row -> SBH_OK / SBH_E_NEED_HALO / SBH_E_BAD_RECORD).  The four accumulators share sbh::Accum
// and, behind the row frame, the frame of accum.hip: accum_open, Accum::reset, add_begin, AddTrip, SpanTable.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <mutex>
#include <thread>
#include <vector>

#include "sbh_internal.h"

namespace sbh {
// Pinned host storage for the host copy of the block table: the device writes it in the
// sbh_block layout and one DMA lands it in place (no staging copy, no per-block host loop);
// elements are default-initialised (resize() does not zero what the copy overwrites).
template <class T>
struct PinnedAlloc {
  using value_type = T;
  PinnedAlloc() = default;
  template <class U>
  PinnedAlloc(const PinnedAlloc<U> &) {}
  T *allocate(size_t n) {
    void *p = nullptr;
    if (hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) != hipSuccess) {
      std::fprintf(stderr, "sparkbam: pinned host allocation of %zu bytes failed\n", n * sizeof(T));
      std::abort();
    }
    return static_cast<T *>(p);
  }
  void deallocate(T *p, size_t) { (void)hipHostFree(p); }
  template <class U>
  void construct(U *p) { ::new (static_cast<void *>(p)) U; }
  template <class U, class... A>
  void construct(U *p, A &&...a) { ::new (static_cast<void *>(p)) U(static_cast<A &&>(a)...); }
  bool operator==(const PinnedAlloc &) const { return true; }
  bool operator!=(const PinnedAlloc &) const { return false; }
};

template <typename T>
struct DBuf {  // grow-only device buffer, freed with its owner (movable, not copyable)
  T *p = nullptr;
  uint64_t cap = 0;
  bool lent = false;  // p is another buffer's memory (lend): never freed or regrown through this one
  DBuf() = default;
  DBuf(const DBuf &) = delete;
  DBuf &operator=(const DBuf &) = delete;
  DBuf(DBuf &&o) noexcept : p(o.p), cap(o.cap), lent(o.lent) { o.forget(); }
  DBuf &operator=(DBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap, lent = o.lent;
      o.forget();
    }
    return *this;
  }
  ~DBuf() { release(); }
  hipError_t ensure(uint64_t n) {
    if (n <= cap) return hipSuccess;
    if (lent) return hipErrorInvalidValue;  // (the lender sizes its memory)
    release();
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), std::max<uint64_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
  // frees now what the destructor would free later (a lent pointer is only dropped)
  void release() {
    if (p && !lent) (void)hipFree(p);
    forget();
  }
  // borrow q[0, c) from its owner, which must outlive the loan; unlend() ends it
  void lend(T *q, uint64_t c) {
    release();
    p = q, cap = c, lent = true;
  }
  void unlend() {
    if (lent) forget();
  }

 private:
  void forget() { p = nullptr, cap = 0, lent = false; }
};

// ---- run-time knobs ----------------------------------------------------------------------------
// The environment is read through these three and nowhere else under csrc/; INTEGRATION.md
// ("Run-time knobs") lists every name they are given.  A knob is read again at each call, never
// cached: tests change them between calls in one process.
// The value, or nullptr when the variable is unset or empty.
inline const char *env_str(const char *name) {
  const char *e = std::getenv(name);
  return e && *e ? e : nullptr;
}
// 0 / 1: off / on; unset: dflt.
inline bool env_flag(const char *name, bool dflt = false) {
  const char *e = env_str(name);
  return e ? e[0] != '0' : dflt;
}
// A positive integer clamped to [lo, hi]; unset or not positive: dflt.
inline uint64_t env_uint(const char *name, uint64_t dflt, uint64_t lo = 1, uint64_t hi = ~0ull) {
  const char *e = env_str(name);
  const long long v = e ? std::atoll(e) : 0;
  return v > 0 ? std::min(std::max<uint64_t>((uint64_t)v, lo), hi) : dflt;
}

}  // namespace sbh

struct StreamCache;  // sbh_run_stream's window shard, buffers and copy stream (kept between calls)

// Threading (include/sparkbam.h): one context serves every thread of its process on its device
// -- a Spark executor's concurrent tasks share it (jni/Native.scala Device).  What a context holds
// is therefore either immutable after creation (device, the context stream used by context-level
// calls) or guarded by `mu` (the pool of streaming-window caches).  Each shard has its own HIP
// stream (sbh_shard_create), so two tasks' shards run concurrently on the device and a task's
// hipStreamSynchronize waits for its own work only; a shard itself belongs to one thread at a time.
// A context that was given the caller's stream (sbh_ctx_set_stream, before any other thread uses the
// context) puts every later shard on that one stream: the tasks then share it, each call still
// drains it before it returns, and no shard ever destroys it.
// The last error (message, status, the reference exception's fields) is kept per thread and per
// context (t_err in sbh_api.hip), so one task's failure never overwrites what another task reads back.
struct sbh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::mutex mu;                       // guards sc_free
  std::vector<StreamCache *> sc_free;  // idle sbh_run_stream2 window caches (one per concurrent caller)
};

struct sbh_shard {
  sbh_ctx *ctx = nullptr;
  // the shard's own stream (every device call on the shard is enqueued here), or the caller's
  // stream when the context was given one (sbh_ctx_set_stream)
  hipStream_t st = nullptr;
  bool own_st = false;
  uint64_t file_off = 0, n = 0, file_size = 0;
  bool at_eof = false;
  sbh::DBuf<uint8_t> comp;
  // index
  bool indexed = false;
  uint64_t index_start = 0, nblocks = 0, utotal = 0;
  sbh::DBuf<uint64_t> b_cstart, b_ustart, usz;
  sbh::DBuf<uint32_t> b_csize, b_hsize, b_usize, b_flags, b_status, b_ntok;
  sbh::DBuf<uint64_t> counts, offs, cand, v, rank, tmp, blkpack;
  sbh::DBuf<uint32_t> cfirst;  // per scan chunk: offset of its first candidate
  uint64_t ncand = 0, cand_from = 0;  // header candidates in cand[] (shard-relative, >= cand_from)
  // sbh_index scans for header candidates from this file offset when it lies in
  // [file_off, start] (~0: from the shard's first byte), so that every split starting in the
  // resident bytes -- a rank's or a streamed window's first one included -- has its
  // FindBlockStart candidates on the device; the block chain still starts at `start`
  uint64_t scan_from = ~0ull;
  sbh::DBuf<int64_t> J0, J1;
  sbh::DBuf<uint8_t> on;
  std::vector<sbh_block, sbh::PinnedAlloc<sbh_block>> hb;
  std::vector<uint64_t> seg_end;
  bool open_last = false, broken_end = false;
  sbh::DBuf<uint64_t> d_seg;
  // inflate
  bool inflated = false;
  sbh::DBuf<uint8_t> U;
  // U's pad [utotal, + pad) is zero for this utotal and allocation (only k_lz writes U, and only
  // below utotal): a step over the same shard skips the memset (an unaligned one is 3 fills)
  uint64_t u_pad_clean = ~0ull, u_pad_cap = 0;
  sbh::DBuf<uint32_t> tok;  // LZ77 tokens between k_huff and k_lz (4 B per flat byte)
  // checker
  sbh::DBuf<int32_t> ctg;
  int32_t nctg = -1;
  sbh::DBuf<uint32_t> bits;
  bool pipe_fallback = false;  // run_pipelined redid the eager pass (a deferral overflow)
  // chain marking (pointer doubling) over the set bits of [cm_first, cm_E) when the bitmap
  // is not the chain: node positions, per-word prefix counts, jumps, marks and their prefix
  sbh::DBuf<uint64_t> cm_pos, cm_wcnt, cm_wpre, cm_mark, cm_mpre;
  sbh::DBuf<uint32_t> cm_j, cm_j2, cm_j0;
  uint64_t cm_first = 0, cm_E = 0, cm_n = 0;
  bool cm_valid = false;
  // the bitmap verified equal to the record chain over [chain_first, chain_E) (k_verify_chain)
  bool chain_ok = false;
  uint64_t chain_first = 0, chain_E = 0;
  // that proof's set bits per VC_CHUNK bitmap words (chunk k = words [VC_CHUNK k, ...) from
  // bits_begin), valid with chain_ok for the same range (cc_ok): the split counts' inner chunks
  sbh::DBuf<uint32_t> cc;
  bool cc_ok = false;
  bool bits_valid = false;
  uint64_t bits_begin = 0, bits_end = 0;
  uint64_t run_first = ~0ull;  // sbh_run_shard's first record (flat), ~0: none found
  int32_t bits_rtc = 0;
  sbh::DBuf<uint32_t> words;
  sbh::DBuf<uint32_t> opix;  // the full checker's bad-CIGAR-op index (launch_full)
  sbh::DBuf<uint64_t> close_pos;
  sbh::DBuf<uint32_t> close_word;
  // the device copy of the row ranges of the filtered row stage under way (stage_row_ranges): the
  // begins, then the ends.  One buffer serves every such stage: each of them synchronises the shard's
  // stream before it returns and a shard belongs to one thread at a time, so no kernel still reads
  // the ranges of the call before when the next call overwrites them.
  sbh::DBuf<uint64_t> row_ranges;
  sbh::DBuf<unsigned long long> ctr;  // scratch counters
  unsigned long long *h_ctr = nullptr;  // pinned mirror
  uint64_t pad = 4096;
  // pipelined run (run_pipelined): extra streams, per-batch events, deferred positions
  hipStream_t s_lz = nullptr, s_eg = nullptr;
  hipStream_t cs = nullptr;  // sbh_shard_load's copy stream (created on first use)
  std::vector<hipEvent_t> pev;
  sbh::DBuf<uint64_t> defer;
  sbh::DBuf<uint64_t> xq;  // long-record eager candidates for the wave-cooperative exact pass
  // record field extraction (sbh_records_scan / fetch): positions, sizes -> offsets, columns
  struct Recs {
    sbh::DBuf<uint64_t> pos, wcnt, wpre, nm, cg, sq, ax, nmo, cgo, sqo, axo, keep, kpre, pos2, vpos;
    // sbh_split_records_batch: [first, E, reserve] x n in, each range's base, count and prefix
    sbh::DBuf<uint64_t> bt_in, bt_rbase, bt_cnt, bt_off;
    sbh::DBuf<int64_t> iv_b, iv_e;
    sbh::DBuf<int32_t> iv_ref;
    sbh::DBuf<int32_t> ref_id, p0, nref, npos, tlen;
    sbh::DBuf<uint16_t> flag, bin;
    sbh::DBuf<uint8_t> mapq, qual, aux;
    sbh::DBuf<char> names, seq;
    sbh::DBuf<uint32_t> cigar;
    sbh_records_sizes sz{};
    bool valid = false;
    bool decoded = false;  // the columns were decoded (else only the starts, sbh_split_records decode = 0)
  } rec;
  // BAI construction (sbh_bai_scan / fetch): per-record keys, windows, starts, the scan's input and
  // prefix, the runs and the linear-index minima of the last scan
  struct Bai {
    sbh::DBuf<uint64_t> pos, key, win, vbeg, flg, pre, ridx, lin, lin_off, aux;
    sbh::DBuf<sbh_bai_run> runs;
    sbh_bai_sizes sz{};
    int32_t edges[4] = {-1, 0, -1, 0};
    bool valid = false;
    bool off_ok = false;  // lin_off holds the window prefix of the current contig lengths
  } bai;
  // SAM text of the last decoded scan (sbh_records_sam_scan / fetch): per-row line lengths and
  // their prefix, the host-row flags and their prefix, the text; the reference names; the host
  // rows (indices, record bytes packed) and their lines as the host rendered them
  struct Sam {
    sbh::DBuf<uint64_t> len, off, hostf, hpre, rows, rbytes, goff, ref_off;
    sbh::DBuf<char> text, refs;
    sbh::DBuf<uint8_t> gbuf;
    std::vector<uint64_t> h_rows, h_off;
    std::vector<char> h_text;
    sbh_sam_sizes sz{};
    bool valid = false;
  } sam;
  // BAM stream of the last scan's selected rows (sbh_records_bam_scan / fetch): per-row lengths and
  // their prefix, keep | run head << 32 and its prefix, the kept rows' offsets and indices, the
  // runs' (output, U) offsets, the stream
  struct Bam {
    sbh::DBuf<uint64_t> len, off, kh, khpre, rec_off, rows, run_dst, run_src;
    sbh::DBuf<uint8_t> out;
    // coordinate order (bam_sort.hip; sizes in bam_sort_core.h): the two (key, row) arrays the passes
    // alternate between, the digit counts with their scan, the permuted starts and lengths
    sbh::DBuf<uint64_t> skey[2], hist, pos2, len2;
    sbh::DBuf<uint32_t> srow[2];
    // read-name order (bam_name.hip) borrows all of those; its own: the words k_name_scan and
    // k_name_groups reduce into (sbh::nacc) and the summary of the last name-order scan
    sbh::DBuf<unsigned long long> nacc;
    sbh_bam_name_info name_info{};
    sbh_bam_sizes sz{};
    uint64_t head_bytes = 0;
    int order = SBH_ORDER_SCAN;  // SBH_ORDER_SCAN, SBH_ORDER_COORDINATE or sbh::ORDER_NAME
    bool already = false;  // a coordinate- or name-order scan found its kept rows in order (no pass ran)
    bool valid = false;
  } bam;
  // per-base depth and pileup (sbh_records_depth_add, sbh_records_pileup_add): the keep bits of the
  // last add of either (a ballot word per 64 rows); the slots live in the sbh_depth or sbh_pileup
  struct Depth {
    sbh::DBuf<uint64_t> keep;
  } dep;
  // FASTQ / FASTA text of the last scan's selected rows (sbh_records_fastq_scan / fetch): per part of
  // the text (fastq_core.h) the rows' line lengths and keep flags with their prefixes, the class byte,
  // each row's offset, the lines' offsets and rows in layout order, the parts' totals, the text
  struct Fastq {
    sbh::DBuf<uint64_t> len, keep, lpre, kpre, off, rec_off, rows, sums;
    sbh::DBuf<uint8_t> cls;
    sbh::DBuf<char> text;
    sbh_fastq_sizes sz{};
    bool valid = false;
  } fq;
  std::vector<int32_t> h_ctg;  // host copy of the contig lengths (sbh_set_contigs)
  // batched splits (sbh_split_starts) and check-bam truth (sbh_check_records)
  sbh::DBuf<uint64_t> sp_start, sp_end, sp_first, sp_E, sp_vpos;
  sbh::DBuf<uint32_t> sp_code;
  sbh::DBuf<unsigned long long> sp_count;
  // sbh_split_starts' fast path: [start, end, first, E, count] x n + code x n in one device
  // buffer and its page-locked mirror (one copy each way)
  sbh::DBuf<uint64_t> sp_pack;
  uint64_t *sp_pin = nullptr;
  uint64_t sp_pin_cap = 0;
  sbh::DBuf<uint32_t> tbits;
  sbh::DBuf<uint64_t> t_rb, t_re, t_fp, t_fn;
  // the next window prefetched by a host thread (shard_prefetch): spare compressed bytes and
  // a u64 array riding with them (check-bam's truth slice; sp_vpos once used)
  sbh::DBuf<uint8_t> comp2;
  sbh::DBuf<uint64_t> aux2;
  std::vector<std::thread> pf;
  std::vector<hipStream_t> pf_stream;
  std::vector<hipError_t> pf_err;
  bool pf_active = false;
  uint64_t pf_off = 0, pf_n = 0, pf_naux = 0;
  std::vector<double> pf_ms;  // each copy thread's wall time
  hipEvent_t ev[9] = {};
  bool ev_ok = false, timing = false;
  double stage_ms[6] = {0, 0, 0, 0, 0, 0};
  double pipe_ms[3] = {0, 0, 0};  // k_huff, k_lz, k_eager summed over the pipelined launches

  sbh::DevBlocks dev_blocks() {
    return sbh::DevBlocks{b_cstart.p, b_csize.p, b_hsize.p, b_usize.p, b_ustart.p, b_flags.p, b_status.p, b_ntok.p};
  }

  // What is not a DBuf is let go here; the DBuf members (and rec, bai, sam, bam) free themselves after
  // this body, in their own destructors -- that is, after the streams below are gone.  That order
  // is sound only because the shard's stream is synchronised first (every entry point joins the
  // other streams into it before it returns), so nothing on the device still uses the memory;
  // the extra streams are drained as well for a call that failed between its launches.
  ~sbh_shard() {
    if (pf_active) (void)sbh::shard_prefetch_finish(this, false);  // (joins the copy threads)
    if (ctx) (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(st);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : pev)
      if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : pf_stream) (void)hipStreamDestroy(s);
    for (hipStream_t s : {s_lz, s_eg, cs})
      if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
      }
    if (sp_pin) (void)hipHostFree(sp_pin);
    if (h_ctr) (void)hipHostFree(h_ctr);
    if (own_st && st) (void)hipStreamDestroy(st);
  }
};

namespace sbh {
// What the accumulators (sbh_depth, sbh_pileup, sbh_tally, sbh_stats) share: the owning context and a stream of
// the accumulator's own.  The adds run on the adding shard's stream and synchronise it before they
// return; reset, finish and the fetches run on `st` and synchronise that -- so no two of them ever
// overlap on the device, and a shard may be destroyed right after its add.
// drain() is the one destructor body of them all.  The derived destructors call it; it is not
// ~Accum, because a base is destroyed after the derived struct's members and the DBufs must be freed
// only once the stream is drained.
struct Accum {
  sbh_ctx *ctx = nullptr;
  hipStream_t st = nullptr;
  int reset(void *p, uint64_t bytes);  // sbh_*_reset: `bytes` at p zeroed on st, st synchronised (accum.hip)
  void drain() {
    if (ctx) (void)hipSetDevice(ctx->device);
    if (st) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
      st = nullptr;
    }
  }
};

// The spans of a depth or pileup accumulator, host and device (accum.hip).  Span k owns the slots
// [off[k], off[k + 1]): its end - beg positions and `extra` (depth: 1, pileup: 0) behind them.
struct SpanTable {
  std::vector<sbh_depth_span> spans;
  std::vector<uint64_t> off;  // n_spans + 1: the first slot of each span, then S
  uint64_t S = 0;
  DBuf<sbh_depth_span> d_spans;
  DBuf<uint64_t> d_off;
  void assign(const sbh_depth_span *sp, uint32_t n_spans, uint32_t extra);  // (spans_refused has judged them)
  // the device copies, on st (the caller synchronises it); hipErrorOutOfMemory for 2^31 - 1 tiles or
  // more: the tile kernels run one workgroup per tile
  hipError_t upload(uint64_t n_tiles, hipStream_t st);
  // positions [from, from + n) of `span`: SBH_OK, or SBH_E_ARG in the words of `what`, the fetch's name
  int range(sbh_ctx *ctx, const char *what, uint32_t span, uint64_t from, uint64_t n) const;
};
}  // namespace sbh

// A depth accumulator (sbh_depth_create): owned by a context, fed by any number of its shards.
struct sbh_depth : sbh::Accum, sbh::SpanTable {
  int32_t n_ref = 0;
  uint32_t flags = 0;
  sbh::DBuf<int32_t> slots;  // S; after finish the depth (u32)
  sbh::DBuf<uint64_t> tsum, tbase, heads, hbase, tstat, tmp;
  sbh::DBuf<unsigned long long> acc;  // max, covered, sum
  sbh::DBuf<sbh_depth_run> runs;
  sbh_depth_sizes sz{};
  bool finished = false;
  ~sbh_depth() { drain(); }
};

// A pileup accumulator (sbh_pileup_create): eight u32 channels per position, owned by a context, fed
// by any number of its shards.  An add borrows the adding shard's depth scratch (the keep bits).
struct sbh_pileup : sbh::Accum, sbh::SpanTable {
  int32_t n_ref = 0;
  uint32_t min_baseq = 0;
  sbh::DBuf<uint4> counts;  // 2 S: position s is counts[2 s], counts[2 s + 1] (A C G T | N DEL INS LOWQ)
  sbh::DBuf<uint8_t> calls;  // S, after finish
  sbh::DBuf<sbh_depth_span> ivals;
  sbh::DBuf<uint64_t> heads, hbase, tstat, tmp;
  sbh::DBuf<unsigned long long> acc;  // the folded tile stats
  sbh_pileup_sizes sz{};
  bool finished = false;
  ~sbh_pileup() { drain(); }
};

// A tally accumulator (sbh_tally_create): flag counts and per-reference counts, owned by a context,
// fed by any number of its shards.
struct sbh_tally : sbh::Accum {
  int32_t n_ref = 0;
  uint64_t words = 0;  // 2 SBH_TALLY_ROWS flag counters, then 2 (n_ref + 1) per-reference counters
  // stage: bad row, past row, then `words` counters of the add under way (k_tally_rows); totals:
  // `words` counters of every add that succeeded (k_tally_commit)
  sbh::DBuf<unsigned long long> stage, totals;
  ~sbh_tally() { drain(); }
};

// A stats accumulator (sbh_stats_create): the tables of csrc/stats_core.h one behind another, owned
// by a context, fed by any number of its shards.
struct sbh_stats : sbh::Accum {
  sbh_stats_params params{};
  uint64_t words = 0;  // sbh_stat::layout_of(params).words
  // stage: bad row, past row, kept rows, then `words` counters of the add under way (k_stats_rows,
  // k_stats_bases); totals: `words` counters of every add that succeeded (k_stats_commit)
  sbh::DBuf<unsigned long long> stage, totals;
  ~sbh_stats() { drain(); }
};

struct StreamCache {
  sbh_shard *sh = nullptr;  // the window shard: its comp is lent one of buf[] while a call runs
  sbh::DBuf<uint8_t> buf[2];
  hipStream_t cs = nullptr;
  hipEvent_t done[2] = {nullptr, nullptr}, c0[2] = {nullptr, nullptr};
  // (the caller has set the device; buf[] free themselves after the copy stream has drained)
  ~StreamCache() {
    if (cs) (void)hipStreamSynchronize(cs);
    if (sh) {
      sh->comp.unlend();
      delete sh;
    }
    for (int i = 0; i < 2; ++i) {
      if (done[i]) (void)hipEventDestroy(done[i]);
      if (c0[i]) (void)hipEventDestroy(c0[i]);
    }
    if (cs) (void)hipStreamDestroy(cs);
  }
};

namespace sbh_bam {
struct Filter;  // bam_gather_core.h
}

namespace sbh {

// ---- errors, device, timing (sbh_api.hip) ------------------------------------------------------
// Records msg (printf style) and code as the calling thread's last error on ctx; returns code.
int fail(sbh_ctx *ctx, int code, const char *fmt, ...);
// fail() with the fields the reference's exception takes (sbh_last_error_detail)
int fail_with(sbh_ctx *ctx, int code, std::initializer_list<int64_t> fields, const char *fmt, ...);
// Makes the context's device current for the calling thread.
int set_device(sbh_ctx *ctx);
// With sh->timing: records the shard's stage event i on its stream (sbh_stage_times).
void mark(sbh_shard *sh, int i);
// The shard's resident bytes are now [file_off, file_off + n) of the file: every state derived
// from the old bytes is void.
void resident_changed(sbh_shard *sh, uint64_t file_off, uint64_t n);

// ---- index (sbh_api.hip) ----------------------------------------------------------------------
// Index in the host block table of the block that starts at file_pos, or -1.
int64_t block_index_of(const sbh_shard *sh, uint64_t file_pos);

// ---- checkers, chain, splits (api_check.hip) ---------------------------------------------------
// Capacity of the long-record eager queue (sbh_shard::xq holds 2 XQ_CAP_MAX entries), which every
// launch is given.
constexpr uint64_t XQ_CAP_MAX = 1 << 22;  // queued long-record eager candidates (2 x 32 MiB)
// The eager bitmap of flat [begin, end) into sh->bits (then bits_valid, bits_begin, bits_end,
// bits_rtc); *n_true (optional) = its set bits.  SBH_E_NEED_HALO when a position needs bytes past
// the shard.  The caller has checked the arguments and set the device.
int eager_range(sbh_shard *sh, uint64_t begin, uint64_t end, int32_t rtc, uint64_t *n_true);
// Flat end of the stream segment (empty block to empty block) that holds p.
uint64_t seg_end_of(const sbh_shard *sh, uint64_t p);
// Records of the chain from first whose start is < E (clamped to first's segment); *anomalies
// (optional) = 0 when the eager bitmap is exactly that chain, else how many positions disagree;
// *exit_flat (optional) = the first chain record at/after E.  known: the proof's counters are
// already in h_ctr (sbh_run_shard's tail).
int count_records_impl(sbh_shard *sh, uint64_t first, uint64_t E, uint64_t *count, int32_t *anomalies,
                       uint64_t *exit_flat = nullptr, bool known = false);
// sbh_split_starts; hostf (optional, zeroed by the caller): hostf[i] = 1 for every split the
// per-split path decided.
int split_starts_impl(sbh_shard *sh, const uint64_t *starts, const uint64_t *ends, uint64_t n, int32_t k,
                      int32_t rtc, int32_t mrs, uint64_t *first_vpos, uint64_t *counts, int32_t *status,
                      uint64_t *n_host, uint8_t *hostf);

// ---- records (api_records.hip) -----------------------------------------------------------------
// Record starts of the chain from first while the start is < E, written at pos (cap n); n and
// anomalies as count_records_impl returned them for the same range.
int records_positions(sbh_shard *sh, uint64_t first, uint64_t E, uint64_t total, uint64_t n, int32_t anomalies,
                      uint64_t *pos);
// Sizes -> prefix offsets -> columns for the n record starts in sh->rec.pos; SBH_E_BAD_RECORD when
// a record is malformed or runs past total.
int records_finish(sbh_shard *sh, uint64_t n, uint64_t total, sbh_records_sizes *out);

// ---- the filtered row stages' shared frame (bam_gather.hip) ------------------------------------
// *F = the filter f describes (nullptr: keep every row); false when it is not a valid one.  (The
// *_host entry points call it directly: they have no context to leave a message in.)
bool bam_filter_of(const sbh_record_filter *f, sbh_bam::Filter *F);
// bam_filter_of for a call on a context: SBH_OK, or SBH_E_ARG with the one message of every stage.
int row_filter(sbh_ctx *ctx, const sbh_record_filter *f, sbh_bam::Filter *F);
// Copies the host row ranges of *F to sh->row_ranges on the shard's stream (two copies; none without
// ranges) and points F->row_begin / row_end at the copy.  The caller synchronises the stream before
// it returns: until then its arrays are the copies' source.
hipError_t stage_row_ranges(sbh_shard *sh, sbh_bam::Filter *F);
// What a stage returns for the two words its row kernel sent back (sbh::RowMinima): bad = the first
// row refused (~0: none, SBH_OK), past = the first row refused only because it runs past the stream.
// `also` ends the SBH_E_BAD_RECORD message with what the stage refuses beyond row_check ("": nothing).
int rows_verdict(sbh_shard *sh, uint64_t bad, uint64_t past, const char *also);
// The tail of the four *_add_host: rc 0 or 1 and the bad row, as the core header's add_host gave them.
inline int host_rows_status(int rc, uint64_t bad, uint64_t *bad_row) {
  if (bad_row) *bad_row = bad;
  return rc == 0 ? SBH_OK : SBH_E_BAD_RECORD;
}

// ---- the accumulators' shared frame (accum.hip) ------------------------------------------------
// The tail of every sbh_*_create.  a: the new accumulator, its ctx and fields set.  Gives it its stream,
// runs fill() -- the stage's allocations, copies and memsets on a->st -- and synchronises; *out = a.  A
// failure deletes a: SBH_E_NOMEM with `nomem`, the whole message, when memory or the stream was not to be
// had, else SBH_E_HIP "<what>: <HIP's text>".
template <class A, class Fill>
int accum_open(A *a, A **out, const char *nomem, const char *what, Fill fill) {
  sbh_ctx *ctx = a->ctx;
  hipError_t e = hipStreamCreateWithFlags(&a->st, hipStreamNonBlocking);
  const bool have_stream = e == hipSuccess;
  if (e == hipSuccess) e = fill();
  if (e == hipSuccess) e = hipStreamSynchronize(a->st);
  if (e == hipSuccess) {
    *out = a;
    return SBH_OK;
  }
  delete a;
  if (e == hipErrorOutOfMemory || !have_stream) {
    (void)hipGetLastError();
    return fail(ctx, SBH_E_NOMEM, "%s", nomem);
  }
  return fail(ctx, SBH_E_HIP, "%s: %s", what, hipGetErrorString(e));
}
// SBH_OK, or SBH_E_ARG with the one message of sbh_depth_create ("depth") and sbh_pileup_create ("pileup").
int spans_refused(sbh_ctx *ctx, const char *stage, const sbh_depth_span *sp, uint32_t n_spans, int32_t n_ref);

// The refusals of every sbh_records_*_add (sh and a are not null) in the words of `name`, the call's, and
// in this order: the shard of another context, a shard without a records scan, `closed` (null, or what a
// finished accumulator says behind the name), the filter (row_filter: *F, its row ranges still the
// caller's).  The caller then presets its result and returns SBH_OK for a scan without rows.
int add_begin(sbh_shard *sh, const Accum *a, const char *name, const char *closed, const sbh_record_filter *filter,
              sbh_bam::Filter *F);
// The one round trip of an add, on the shard's stream.  head: the device words bad, past, a, b
// (ctr::ADD_BAD ..) and whatever else the stage counts behind them; mirror: where in h_ctr the four land.
struct AddTrip {
  sbh_shard *sh;
  unsigned long long *head;
  uint32_t mirror;
  // the device made current, keep (null: none) grown to a bit per row, F's row ranges staged; then two
  // memsets: bad and past ~0, the `zeroed` words from a on 0
  int open(sbh_bam::Filter *F, DBuf<uint64_t> *keep, uint64_t zeroed) const;
  // behind the stage's launches: the head copied back, the stream synchronised, rows_verdict(bad, past, also)
  int verdict(const char *also) const;
  uint64_t a() const { return sh->h_ctr[mirror + ctr::ADD_A]; }
  uint64_t b() const { return sh->h_ctr[mirror + ctr::ADD_B]; }
};

}  // namespace sbh

#define HIPCHK(ctx, x)                                                                              \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) return sbh::fail((ctx), SBH_E_HIP, "%s: %s", #x, hipGetErrorString(e_));  \
  } while (0)
