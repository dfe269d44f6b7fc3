// bai.hip -- BAI index construction on CDNA4: what htslib's hts_idx_push does record by record
// (bins, chunks, the linear index, the per-reference metadata), restated as data-parallel passes
// over the record starts sbh_records_scan already produces, and the host-side finisher
// (hts_idx_finish: compress_binning, chunk merging, the linear index's backward fill) plus the
// BAI serialisation.
//
// Device passes (one lane per record, workgroups of BAI_T):
//   k_bai_keys   the 36 fixed bytes and the CIGAR's reference length -> key (ref_id, bin), the
//                linear-index windows [w0, w1], the start's virtual offset, the unmapped bit; the
//                ordering / malformed checks against record i - 1.  A record with more than
//                BAI_COOP_OPS CIGAR ops is summed by the whole wave (ballot loop), so one long
//                CIGAR does not hold 63 lanes idle for thousands of iterations.
//   k_bai_heads  head flag (key[i] != key[i - 1]) into the scan input, and the linear index:
//                atomicMin(lin[w], vbeg) only for windows record i - 1 does not already cover.
//   (one exclusive scan of head | unmapped << 32: run index and unmapped prefix together)
//   k_bai_ridx   run r's head record index, scattered at the heads
//   k_bai_runs   one lane per run: sbh_bai_run from its head, the next run's head and the prefixes.
// Runs are formed without atomics.  Records without a reference (ref_id < 0) carry the key ~0:
// in a sorted file they are one trailing run, which sbh_bai_scan turns into n_no_coor.
#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "sbh_host.h"

namespace sbh {
namespace {

constexpr uint32_t BAI_T = 256;        // workgroup of every kernel here (4 waves)
constexpr uint32_t BAI_COOP_OPS = 32;  // more CIGAR ops than this: the wave sums them together
constexpr uint64_t KEY_NONE = ~0ull;   // key of a record without a reference

__device__ __forceinline__ uint32_t rd_u32(const uint8_t *U, uint64_t p) {
  return (uint32_t)U[p] | (uint32_t)U[p + 1] << 8 | (uint32_t)U[p + 2] << 16 | (uint32_t)U[p + 3] << 24;
}

// htslib hts_reg2bin(beg, end, 14, 5)
__device__ __forceinline__ uint32_t reg2bin(int64_t beg, int64_t end) {
  --end;
  int s = 14;
  int64_t t = 4681;
  for (int l = 5; l > 0; s += 3) {
    if (beg >> s == end >> s) return (uint32_t)(t + (beg >> s));
    --l;
    t -= 1ll << (3 * l);
  }
  return 0;
}

__device__ __forceinline__ int64_t ref_len_of(uint32_t op) {
  const uint32_t t = op & 15;
  return (t == 0 || t == 2 || t == 3 || t == 7 || t == 8) ? (int64_t)(op >> 4) : 0;
}

// Flat position -> virtual offset as htslib's bgzf_tell reports it: canonical inside the stream
// (k_rec_vpos), and a position at the end of the last non-empty block is the address of the
// member after it (the EOF member, or the next window's first block), offset 0.
__device__ __forceinline__ uint64_t vpos_of(uint64_t f, const uint64_t *ustart, const uint64_t *cstart,
                                            const uint32_t *csize, const uint32_t *usize, uint64_t nblocks,
                                            uint64_t file_off) {
  uint64_t lo = 0, hi = nblocks;  // first block with ustart > f
  while (lo < hi) {
    const uint64_t m = (lo + hi) / 2;
    if (ustart[m] <= f) lo = m + 1;
    else hi = m;
  }
  uint64_t k = lo ? lo - 1 : 0;
  while (k > 0 && usize[k] == 0) --k;
  const uint64_t off = f - ustart[k];
  if (off >= usize[k]) return (file_off + cstart[k] + csize[k]) << 16;
  return (file_off + cstart[k]) << 16 | off;
}

// aux[0] the last record's end (virtual offset), aux[1] / aux[2] the first record's and the last
// coordinate record's (ref_id << 32 | pos); err[0] / err[1] / err[2] the smallest row that does not
// fit the stream (more resident bytes may cure it) / is out of order / is off its reference
// (ref_id >= n_ref, or pos < 0 on a reference).
__global__ __launch_bounds__(BAI_T) void k_bai_keys(const uint8_t *__restrict__ U, const uint64_t *pos, uint64_t n,
                                                    uint64_t total, const int32_t *ctg, int32_t nctg,
                                                    const uint64_t *ustart, const uint64_t *cstart,
                                                    const uint32_t *csize, const uint32_t *usize, uint64_t nblocks,
                                                    uint64_t file_off, uint64_t *key, uint64_t *win, uint64_t *vbeg,
                                                    uint64_t *flg, uint64_t *aux, unsigned long long *err) {
  const uint64_t i = (uint64_t)blockIdx.x * BAI_T + threadIdx.x;
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const bool live = i < n;
  const uint64_t p = live ? pos[i] : 0;
  bool ok = live && p + 36 <= total;
  int32_t ref = -1, rp = 0;
  uint32_t ncig = 0, flag = 0;
  uint64_t q = 0;
  int64_t bsz = 0;
  if (ok) {
    bsz = (int32_t)rd_u32(U, p);
    ref = (int32_t)rd_u32(U, p + 4);
    rp = (int32_t)rd_u32(U, p + 8);
    const uint32_t fnc = rd_u32(U, p + 16);
    ncig = fnc & 0xffff;
    flag = fnc >> 16;
    const uint32_t l_name = U[p + 12];
    q = p + 36 + l_name;
    if (bsz < 32 + (int64_t)l_name + 4 * (int64_t)ncig || p + 4 + (uint64_t)bsz > total) ok = false;
  }
  const bool off_ref = ok && (ref >= nctg || (ref >= 0 && rp < 0));
  if (off_ref) ok = false;
  const bool coord = ok && ref >= 0;
  // reference length: short CIGARs in the lane, long ones by the wave
  int64_t reflen = 0;
  const bool big = coord && ncig > BAI_COOP_OPS;
  if (coord && !big)
    for (uint32_t c = 0; c < ncig; ++c) reflen += ref_len_of(rd_u32(U, q + 4ull * c));
  unsigned long long todo = __ballot(big);
  while (todo) {
    const int src = __builtin_ctzll(todo);
    todo &= todo - 1;
    const uint64_t q0 = (uint64_t)__shfl((unsigned long long)q, src);
    const uint32_t nc0 = (uint32_t)__shfl((int)ncig, src);
    long long part = 0;
    for (uint32_t c = lane; c < nc0; c += WAVE) part += ref_len_of(rd_u32(U, q0 + 4ull * c));
    for (int off = WAVE / 2; off > 0; off >>= 1) part += __shfl_down(part, off);
    part = __shfl(part, 0);
    if ((int)lane == src) reflen = part;
  }
  if (!live) return;
  if (!ok) atomicMin(err + (off_ref ? 2 : 0), (unsigned long long)i);
  uint64_t k = KEY_NONE, w = 0, um = 0;
  if (coord) {
    const int64_t beg = rp;
    const int64_t end = (!(flag & 4) && reflen > 0) ? beg + reflen : beg + 1;
    const int64_t wmax = ((int64_t)ctg[ref] >> 14) + 1;  // the reference's last linear-index slot
    const int64_t b14 = beg >> 14, e14 = (end - 1) >> 14;
    const int64_t w0 = b14 < wmax ? b14 : wmax, w1 = e14 < wmax ? e14 : wmax;
    k = (uint64_t)(uint32_t)ref << 32 | reg2bin(beg, end);
    w = (uint64_t)w0 << 32 | (uint64_t)w1;
    um = (flag & 4) ? 1 : 0;
  }
  key[i] = k;
  win[i] = w;
  flg[i] = um << 32;
  vbeg[i] = vpos_of(p, ustart, cstart, csize, usize, nblocks, file_off);
  // ordering against the record before (hts_idx_push refuses unsorted input)
  if (coord && i > 0) {
    const uint64_t pp = pos[i - 1];
    if (pp + 12 <= total) {
      const int32_t pref = (int32_t)rd_u32(U, pp + 4), ppos = (int32_t)rd_u32(U, pp + 8);
      if (pref < 0 || ref < pref || (ref == pref && rp < ppos)) atomicMin(err + 1, (unsigned long long)i);
    }
  }
  if (i == 0) aux[1] = (uint64_t)(uint32_t)(ok ? ref : -1) << 32 | (uint32_t)rp;
  if (coord) {
    bool last = i + 1 == n;
    if (!last) {
      const uint64_t np = pos[i + 1];
      last = np + 8 > total || (int32_t)rd_u32(U, np + 4) < 0;
    }
    if (last) aux[2] = (uint64_t)(uint32_t)ref << 32 | (uint32_t)rp;
  }
  if (i + 1 == n)
    aux[0] = ok ? vpos_of(p + 4 + (uint64_t)bsz, ustart, cstart, csize, usize, nblocks, file_off) : 0;
}

// Head flags and the linear index.  Window w of record i needs no atomicMin when record i - 1
// lies on the same reference and covers w: that record's start is the smaller virtual offset and
// (by induction along the run of covering records) some record before it has written w.  In a
// coordinate-sorted file this removes nearly every same-address atomic.
__global__ __launch_bounds__(BAI_T) void k_bai_heads(const uint64_t *key, const uint64_t *win, const uint64_t *vbeg,
                                                     uint64_t n, const uint64_t *lin_off, uint64_t *flg,
                                                     unsigned long long *lin) {
  const uint64_t i = (uint64_t)blockIdx.x * BAI_T + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    flg[n] = 0;  // (the scan's last entry is then the total)
    return;
  }
  const uint64_t k = key[i], pk = i ? key[i - 1] : 0;
  if (i == 0 || k != pk) flg[i] |= 1;
  if (k == KEY_NONE) return;
  const uint32_t ref = (uint32_t)(k >> 32);
  const uint64_t w = win[i];
  uint64_t w0 = w >> 32;
  const uint64_t w1 = w & 0xffffffffu;
  if (i && pk != KEY_NONE && (uint32_t)(pk >> 32) == ref) {
    const uint64_t pw = win[i - 1];
    const uint64_t after = (pw & 0xffffffffu) + 1;
    if ((pw >> 32) <= w0 && after > w0) w0 = after;
  }
  const uint64_t v = vbeg[i], base = lin_off[ref];
  for (uint64_t x = w0; x <= w1; ++x) atomicMin(lin + base + x, (unsigned long long)v);
}

__global__ __launch_bounds__(BAI_T) void k_bai_ridx(const uint64_t *flg, const uint64_t *pre, uint64_t n,
                                                    uint64_t *ridx) {
  const uint64_t i = (uint64_t)blockIdx.x * BAI_T + threadIdx.x;
  if (i < n && (flg[i] & 1)) ridx[pre[i] & 0xffffffffu] = i;
}

__global__ __launch_bounds__(BAI_T) void k_bai_runs(const uint64_t *ridx, uint64_t nruns, uint64_t n,
                                                    const uint64_t *key, const uint64_t *vbeg, const uint64_t *pre,
                                                    const uint64_t *aux, sbh_bai_run *runs) {
  const uint64_t r = (uint64_t)blockIdx.x * BAI_T + threadIdx.x;
  if (r >= nruns) return;
  const uint64_t i0 = ridx[r], i1 = r + 1 < nruns ? ridx[r + 1] : n;
  const uint64_t k = key[i0];
  const uint64_t um = (pre[i1] >> 32) - (pre[i0] >> 32);
  sbh_bai_run o;
  o.ref_id = k == KEY_NONE ? -1 : (int32_t)(k >> 32);
  o.bin = (uint32_t)k;
  o.vbeg = vbeg[i0];
  o.vend = i1 < n ? vbeg[i1] : aux[0];
  o.n_mapped = (i1 - i0) - um;
  o.n_unmapped = um;
  runs[r] = o;
}

}  // namespace

// key / win / vbeg: n u64 each, flg: n + 1 (the scan's input, head | unmapped << 32), aux: 3 words,
// err: 3 (preset to ~0).
static hipError_t launch_bai_keys(const uint8_t *U, const uint64_t *pos, uint64_t n, uint64_t total, const int32_t *ctg,
                                  int32_t nctg, DevBlocks bl, uint64_t nblocks, uint64_t file_off, uint64_t *key,
                                  uint64_t *win, uint64_t *vbeg, uint64_t *flg, uint64_t *aux, unsigned long long *err,
                                  hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_bai_keys, dim3((uint32_t)((n + BAI_T - 1) / BAI_T)), dim3(BAI_T), 0, st, U, pos, n, total, ctg,
                     nctg, bl.ustart, bl.cstart, bl.csize, bl.usize, nblocks, file_off, key, win, vbeg, flg, aux, err);
  return hipGetLastError();
}

static hipError_t launch_bai_heads(const uint64_t *key, const uint64_t *win, const uint64_t *vbeg, uint64_t n,
                                   const uint64_t *lin_off, uint64_t *flg, uint64_t *lin, hipStream_t st) {
  hipLaunchKernelGGL(k_bai_heads, dim3((uint32_t)((n + 1 + BAI_T - 1) / BAI_T)), dim3(BAI_T), 0, st, key, win, vbeg, n,
                     lin_off, flg, reinterpret_cast<unsigned long long *>(lin));
  return hipGetLastError();
}

// pre: the exclusive scan of flg[0..n]; ridx: nruns words; runs: nruns entries
static hipError_t launch_bai_runs(const uint64_t *flg, const uint64_t *pre, uint64_t n, uint64_t nruns, const uint64_t *key,
                                  const uint64_t *vbeg, const uint64_t *aux, uint64_t *ridx, sbh_bai_run *runs,
                                  hipStream_t st) {
  if (!n || !nruns) return hipSuccess;
  hipLaunchKernelGGL(k_bai_ridx, dim3((uint32_t)((n + BAI_T - 1) / BAI_T)), dim3(BAI_T), 0, st, flg, pre, n, ridx);
  hipLaunchKernelGGL(k_bai_runs, dim3((uint32_t)((nruns + BAI_T - 1) / BAI_T)), dim3(BAI_T), 0, st, ridx, nruns, n, key,
                     vbeg, pre, aux, runs);
  return hipGetLastError();
}

}  // namespace sbh

using namespace sbh;

extern "C" {

// ---- the C-ABI's scan calls (htslib hts_idx_push over the record chain) ----------------------
int sbh_bai_scan(sbh_shard *sh, uint64_t first, uint64_t end_flat, sbh_bai_sizes *out) {
  if (!sh || !out) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  if (!sh->inflated) return fail(ctx, SBH_E_STATE, "bai scan before inflate");
  if (sh->nctg < 0) return fail(ctx, SBH_E_STATE, "contig lengths not set");
  if (first > sh->utotal) return SBH_E_ARG;
  int rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  auto &B = sh->bai;
  B.valid = false;
  const int32_t nref = sh->nctg;
  if (!B.off_ok) {  // the linear index's layout: reference r owns (l_ref >> 14) + 2 slots
    std::vector<uint64_t> off((size_t)nref + 1, 0);
    for (int32_t r = 0; r < nref; ++r) {
      if (sh->h_ctg[r] < 0) return fail(ctx, SBH_E_ARG, "contig %d has a negative length", r);
      off[r + 1] = off[r] + ((uint64_t)sh->h_ctg[r] >> 14) + 2;
    }
    HIPCHK(ctx, B.lin_off.ensure((uint64_t)nref + 1));
    HIPCHK(ctx, hipMemcpyAsync(B.lin_off.p, off.data(), 8 * ((uint64_t)nref + 1), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    B.sz.lin_size = off[nref];
    B.off_ok = true;
  }
  const uint64_t lin_size = B.sz.lin_size;
  const uint64_t total = seg_end_of(sh, first);
  const uint64_t E = std::min(std::min(end_flat, sh->utotal), total);
  uint64_t n = 0;
  int32_t anomalies = 0;
  rc = count_records_impl(sh, first, E, &n, &anomalies);
  if (rc) return rc;
  if (n >= 0xffffffffull) return fail(ctx, SBH_E_ARG, "bai scan: %llu records in one scan (scan in windows)",
                                      (unsigned long long)n);
  HIPCHK(ctx, B.pos.ensure(n));
  rc = records_positions(sh, first, E, total, n, anomalies, B.pos.p);
  if (rc) return rc;
  for (auto *b : {&B.key, &B.win, &B.vbeg}) HIPCHK(ctx, b->ensure(n));
  HIPCHK(ctx, B.flg.ensure(n + 1));
  HIPCHK(ctx, B.pre.ensure(n + 1));
  HIPCHK(ctx, B.lin.ensure(lin_size));
  HIPCHK(ctx, B.aux.ensure(8));
  HIPCHK(ctx, sh->tmp.ensure(scan_tmp_words(n + 1)));
  unsigned long long *err = sh->ctr.p + ctr::BAI_ERR;  // rows: does not fit, unsorted, off its reference
  constexpr size_t err_bytes = (ctr::BAI_ERR_END - ctr::BAI_ERR) * 8;
  HIPCHK(ctx, hipMemsetAsync(err, 0xff, err_bytes, st));
  HIPCHK(ctx, hipMemsetAsync(B.aux.p, 0xff, 24, st));
  if (lin_size) HIPCHK(ctx, hipMemsetAsync(B.lin.p, 0xff, 8 * lin_size, st));
  uint64_t nruns = 0, no_coor = 0;
  B.edges[0] = B.edges[2] = -1;
  B.edges[1] = B.edges[3] = 0;
  if (n) {
    HIPCHK(ctx, launch_bai_keys(sh->U.p, B.pos.p, n, total, sh->ctg.p, nref, sh->dev_blocks(), sh->nblocks,
                                sh->file_off, B.key.p, B.win.p, B.vbeg.p, B.flg.p, B.aux.p, err, st));
    HIPCHK(ctx, launch_bai_heads(B.key.p, B.win.p, B.vbeg.p, n, B.lin_off.p, B.flg.p, B.lin.p, st));
    HIPCHK(ctx, scan_exclusive_u64(B.flg.p, B.pre.p, n + 1, sh->tmp.p, st));
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::BAI_ERR, err, err_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_BAI_NRUNS, B.pre.p + n, 8, hipMemcpyDeviceToHost, st));
    // (aux's three words: the edges are the last two)
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_BAI_AUX, B.aux.p, 3 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint64_t unfit = sh->h_ctr[ctr::BAI_UNFIT], uns = sh->h_ctr[ctr::BAI_UNSORTED],
                   off_ref = sh->h_ctr[ctr::BAI_OFF_REF];
    const uint64_t bad = std::min(unfit, off_ref);
    if (bad != ~0ull || uns != ~0ull) {
      const uint64_t row = std::min(bad, uns);
      HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_BAI_BAD_VPOS, B.vbeg.p + row, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      const uint64_t v = sh->h_ctr[ctr::H_BAI_BAD_VPOS];
      if (bad <= uns) {
        // only a record that does not fit can be cured by more resident bytes
        if (unfit < off_ref && !sh->at_eof)
          return fail(ctx, SBH_E_NEED_HALO, "record %llu of the scan may run past the shard", (unsigned long long)row);
        return fail(ctx, SBH_E_BAD_RECORD, "record %llu of the scan (%llu:%u) is malformed or off its reference",
                    (unsigned long long)row, (unsigned long long)(v >> 16), (unsigned)(v & 0xffff));
      }
      return fail_with(ctx, SBH_E_UNSORTED, {(int64_t)v},
                       "record %llu of the scan (%llu:%u) is out of coordinate order", (unsigned long long)row, (unsigned long long)(v >> 16), (unsigned)(v & 0xffff));
    }
    nruns = sh->h_ctr[ctr::H_BAI_NRUNS] & 0xffffffffull;
    HIPCHK(ctx, B.ridx.ensure(nruns));
    HIPCHK(ctx, B.runs.ensure(nruns));
    HIPCHK(ctx, launch_bai_runs(B.flg.p, B.pre.p, n, nruns, B.key.p, B.vbeg.p, B.aux.p, B.ridx.p, B.runs.p, st));
    sbh_bai_run last{};
    HIPCHK(ctx, hipMemcpyAsync(&last, B.runs.p + (nruns - 1), sizeof last, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (last.ref_id < 0) {  // the trailing run of records without a reference
      no_coor = last.n_mapped + last.n_unmapped;
      --nruns;
    }
    B.edges[0] = (int32_t)(sh->h_ctr[ctr::H_BAI_FIRST_EDGE] >> 32);
    B.edges[1] = (int32_t)(uint32_t)sh->h_ctr[ctr::H_BAI_FIRST_EDGE];
    if (sh->h_ctr[ctr::H_BAI_LAST_EDGE] != ~0ull) {
      B.edges[2] = (int32_t)(sh->h_ctr[ctr::H_BAI_LAST_EDGE] >> 32);
      B.edges[3] = (int32_t)(uint32_t)sh->h_ctr[ctr::H_BAI_LAST_EDGE];
    }
  }
  B.sz = sbh_bai_sizes{n, nruns, no_coor, lin_size};
  B.valid = true;
  *out = B.sz;
  return SBH_OK;
}

int sbh_bai_fetch(sbh_shard *sh, sbh_bai_run *runs, uint64_t *lin) {
  if (!sh) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &B = sh->bai;
  if (!B.valid) return fail(ctx, SBH_E_STATE, "bai_fetch without a bai_scan");
  int rc = set_device(ctx);
  if (rc) return rc;
  if (runs && B.sz.n_runs)
    HIPCHK(ctx, hipMemcpyAsync(runs, B.runs.p, B.sz.n_runs * sizeof(sbh_bai_run), hipMemcpyDeviceToHost, sh->st));
  if (lin && B.sz.lin_size)
    HIPCHK(ctx, hipMemcpyAsync(lin, B.lin.p, 8 * B.sz.lin_size, hipMemcpyDeviceToHost, sh->st));
  HIPCHK(ctx, hipStreamSynchronize(sh->st));
  return SBH_OK;
}

int sbh_bai_edges(sbh_shard *sh, int32_t *first_ref, int32_t *first_pos, int32_t *last_ref, int32_t *last_pos) {
  if (!sh) return SBH_E_ARG;
  if (!sh->bai.valid) return fail(sh->ctx, SBH_E_STATE, "bai_edges without a bai_scan");
  const int32_t *e = sh->bai.edges;
  if (first_ref) *first_ref = e[0];
  if (first_pos) *first_pos = e[1];
  if (last_ref) *last_ref = e[2];
  if (last_pos) *last_pos = e[3];
  return SBH_OK;
}

}  // extern "C"

// ---- host-only finisher (no context, no device) ---------------------------------------------
namespace {

struct Chunk {
  uint64_t u, v;
  bool operator<(const Chunk &o) const { return u != o.u ? u < o.u : v < o.v; }
};
struct RefIdx {
  std::map<uint32_t, std::vector<Chunk>> bins;
  uint64_t first = 0, last = 0, n_mapped = 0, n_unmapped = 0;
  bool any = false;
};

constexpr uint32_t BAI_META_BIN = 37450;

// htslib compress_binning for one reference
void compress_binning(RefIdx &R) {
  for (int l = 5; l > 0; --l) {
    const uint32_t first = ((1u << (3 * l)) - 1) / 7, end = ((1u << (3 * (l + 1))) - 1) / 7;
    for (auto it = R.bins.lower_bound(first); it != R.bins.end() && it->first < end;) {
      std::vector<Chunk> &c = it->second;
      if (l < 5) std::sort(c.begin(), c.end());
      if ((c.back().v >> 16) - (c.front().u >> 16) < 0x10000) {
        std::vector<Chunk> &par = R.bins[(it->first - 1) >> 3];  // (a smaller key: `it` stays valid)
        par.insert(par.end(), c.begin(), c.end());
        it = R.bins.erase(it);
      } else {
        ++it;
      }
    }
  }
  auto z = R.bins.find(0);
  if (z != R.bins.end()) std::sort(z->second.begin(), z->second.end());
  for (auto &kv : R.bins) {  // merge chunks that meet in one BGZF block
    std::vector<Chunk> &c = kv.second;
    size_t m = 0;
    for (size_t l = 1; l < c.size(); ++l) {
      if (c[m].v >> 16 >= c[l].u >> 16) {
        if (c[m].v < c[l].v) c[m].v = c[l].v;
      } else {
        c[++m] = c[l];
      }
    }
    c.resize(m + 1);
  }
}

void put32(std::vector<uint8_t> &o, uint32_t v) {
  for (int k = 0; k < 4; ++k) o.push_back((uint8_t)(v >> (8 * k)));
}
void put64(std::vector<uint8_t> &o, uint64_t v) {
  for (int k = 0; k < 8; ++k) o.push_back((uint8_t)(v >> (8 * k)));
}

}  // namespace

extern "C" {

uint64_t sbh_bai_bound(uint64_t n_runs, uint64_t lin_size, int32_t n_ref) {
  // magic, n_ref, n_no_coor; per reference n_bin, n_intv and the metadata bin; per run at most
  // one bin header and one chunk (a fold never adds bins or chunks); the linear index
  return 16 + 56 * (uint64_t)std::max(n_ref, 0) + 24 * n_runs + 8 * lin_size;
}

int sbh_bai_build(const sbh_bai_run *runs, uint64_t n_runs, const uint64_t *lin, const int32_t *contig_len,
                  int32_t n_ref, uint64_t n_no_coor, uint8_t *out, uint64_t cap, uint64_t *size) {
  if (n_ref < 0 || (n_ref && !contig_len) || (n_runs && !runs) || !out || !size) return SBH_E_ARG;
  std::vector<uint64_t> lin_off((size_t)n_ref + 1, 0);
  for (int32_t r = 0; r < n_ref; ++r) {
    if (contig_len[r] < 0) return SBH_E_ARG;
    lin_off[r + 1] = lin_off[r] + ((uint64_t)contig_len[r] >> 14) + 2;
  }
  if (lin_off[n_ref] && !lin) return SBH_E_ARG;
  std::vector<RefIdx> refs((size_t)n_ref);
  // hts_idx_push's chunks: adjacent runs with one (ref_id, bin) are one run cut at a window seam
  const sbh_bai_run *prev = nullptr;
  for (uint64_t i = 0; i < n_runs; ++i) {
    const sbh_bai_run &r = runs[i];
    if (r.ref_id < 0 || r.ref_id >= n_ref) return SBH_E_BAD_RECORD;
    if (prev && r.ref_id < prev->ref_id) return SBH_E_UNSORTED;
    RefIdx &R = refs[r.ref_id];
    if (r.bin >= BAI_META_BIN) return SBH_E_ARG;
    if (prev && prev->ref_id == r.ref_id && prev->bin == r.bin) {
      if (prev->vend != r.vbeg) return SBH_E_ARG;  // (not one run cut in two: a gap or an overlap)
      R.bins[r.bin].back().v = r.vend;
    } else {
      R.bins[r.bin].push_back(Chunk{r.vbeg, r.vend});
    }
    if (!R.any) R.first = r.vbeg;
    R.any = true;
    R.last = r.vend;
    R.n_mapped += r.n_mapped;
    R.n_unmapped += r.n_unmapped;
    prev = &r;
  }
  std::vector<uint8_t> o;
  o.reserve(sbh_bai_bound(n_runs, lin_off[n_ref], n_ref));
  o.insert(o.end(), {'B', 'A', 'I', 1});
  put32(o, (uint32_t)n_ref);
  for (int32_t r = 0; r < n_ref; ++r) {
    RefIdx &R = refs[r];
    if (!R.any) {
      put32(o, 0);
      put32(o, 0);
      continue;
    }
    compress_binning(R);
    put32(o, (uint32_t)R.bins.size() + 1);
    for (const auto &kv : R.bins) {  // ascending bin id (htslib: hash order), the metadata bin last
      put32(o, kv.first);
      put32(o, (uint32_t)kv.second.size());
      for (const Chunk &c : kv.second) put64(o, c.u), put64(o, c.v);
    }
    put32(o, BAI_META_BIN);
    put32(o, 2);
    put64(o, R.first), put64(o, R.last), put64(o, R.n_mapped), put64(o, R.n_unmapped);
    // linear index: up to the last touched window, gaps filled from the next touched one
    const uint64_t *L = lin + lin_off[r];
    uint64_t n_intv = lin_off[r + 1] - lin_off[r];
    while (n_intv && L[n_intv - 1] == UINT64_MAX) --n_intv;
    put32(o, (uint32_t)n_intv);
    std::vector<uint64_t> fill(L, L + n_intv);
    for (uint64_t k = n_intv; k-- > 1;)
      if (fill[k - 1] == UINT64_MAX) fill[k - 1] = fill[k];
    for (uint64_t v : fill) put64(o, v);
  }
  put64(o, n_no_coor);
  *size = o.size();
  if (o.size() > cap) return SBH_E_ARG;
  std::memcpy(out, o.data(), o.size());
  return SBH_OK;
}

}  // extern "C"
