// sam.hip -- SAM text of the decoded records on CDNA4: size pass -> scan -> emit pass.
//
// Input is what a decoded scan leaves resident (records.hip, records_finish): the flat bytes U,
// the record starts pos[], and the exclusive prefix offsets of the validated per-record sizes
// (name bytes, CIGAR ops, bases, tag bytes).  The line a record becomes is defined in sam_core.h,
// which the host renderer shares.
//
//   k_sam_sizes  one wave per record (grid-stride, four waves per workgroup, as k_rec_fields):
//                len[i] = the line's bytes; rows with an f / B:f value get hostf[i] = 1 and
//                len[i] = 0 (the host renders them: Float.toString needs strtof); a malformed
//                CIGAR op or tag area does atomicMin(bad, i).
//   scan_exclusive_u64 over len[0..n] (len[n] = 0) gives line_off[0..n], line_off[n] the total.
//   k_sam_emit   the same walk, writing each field at text + line_off[i] + the running offset.
//
// Inside a wave everything that steers control flow -- the sizes, the fixed fields, the tag
// cursor -- is loaded from one address by all 64 lanes, so the lanes never diverge on it: they
// follow the same tag, find a Z / H value's NUL by ballot over 64 bytes per step, and stride
// over CIGAR ops, bases, qualities and B elements, whose text positions come from a wave prefix sum.
//
// Bounds.
//  * Reads.  A record's bytes are [p, p + 4 + block_size), which k_rec_sizes has proven to lie
//    inside the stream and to hold 36 + l_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq bytes before
//    the tag area of l_aux bytes; the offsets arrays carry exactly those validated sizes.  Name,
//    CIGAR, bases and qualities are read at indices below their sizes.  In the tag area the cursor
//    is checked against l_aux before every read of a type byte, a count or a value (tag_head; the
//    NUL search and the element loops stop at l_aux resp. at the count tag_head admitted).
//    A record of at most STAGE bytes is walked in its wave's LDS slot of STAGE bytes, a copy of
//    exactly those bytes at the same offsets, so the same indices bound the LDS reads.
//  * Stores.  A wave writes only inside [line_off[i], line_off[i + 1]): every store is guarded by
//    the line's length, so nothing goes at or past line_off[n] even if the two passes disagreed.
//    Host rows (len 0 in the size pass, their lengths scattered in before the scan) are skipped.
//  * Reference names are read inside [off[k], off[k + 1]) for 0 <= k < n_ref only.
#include <algorithm>
#include <cstring>
#include <vector>

#define SBH_HD __host__ __device__
#include "sam_core.h"
#include "sbh_host.h"

namespace sbh {
namespace {

using namespace sbh_sam;

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
  for (int m = WAVE / 2; m > 0; m >>= 1) x += (uint32_t)__shfl_xor((int)x, m);
  return x;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t x) {
  for (int m = WAVE / 2; m > 0; m >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, m), hi = (uint32_t)__shfl_xor((int)(x >> 32), m);
    x += (uint64_t)hi << 32 | lo;
  }
  return x;
}
__device__ __forceinline__ uint32_t first_lane(unsigned long long m) { return (uint32_t)__builtin_ctzll(m); }

// The validated sizes of record i (records_finish's offsets) and the bytes they add up to: the
// record is [p, p + bytes), bytes == 4 + block_size.
struct RecSizes {
  uint32_t l_name, n_cig, l_aux;
  uint64_t l_seq, bytes;
};
__device__ __forceinline__ RecSizes sizes_of(const uint64_t *nm_off, const uint64_t *cg_off, const uint64_t *sq_off,
                                             const uint64_t *ax_off, uint64_t i) {
  RecSizes z;
  z.l_name = (uint32_t)(nm_off[i + 1] - nm_off[i]);
  z.n_cig = (uint32_t)(cg_off[i + 1] - cg_off[i]);
  z.l_seq = sq_off[i + 1] - sq_off[i];
  z.l_aux = (uint32_t)(ax_off[i + 1] - ax_off[i]);
  z.bytes = 36 + z.l_name + 4ull * z.n_cig + (z.l_seq + 1) / 2 + z.l_seq + z.l_aux;
  return z;
}

// A record of up to STAGE bytes is copied into its wave's LDS slot first -- every lane's loads are
// independent, one trip to memory -- and both passes then walk it there: the tag walk is a chain of
// dependent reads (type byte, then the value, then the next type byte), each a trip to HBM or L2
// when made on U directly (measured over config B: the whole call 74.4 ms walking U, 68.4 ms
// staged).  Longer records are walked in U.  The slot is the wave's
// own and LDS instructions of a wave execute in order, so a wave-scope fence (no reordering by
// the compiler) is all that separates the copy from the reads and the reads from the next copy.
constexpr uint32_t STAGE = 1024;
__device__ __forceinline__ void stage_record(uint8_t *slot, const uint8_t *g, uint32_t nb, uint32_t lane) {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  for (uint32_t k = lane; k < nb; k += WAVE) slot[k] = g[k];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// What both passes know of a record before they walk it (r: its bytes, in LDS or in U).
struct RecView {
  const uint8_t *r, *aux;
  Fixed f;
  uint32_t l_name, n_cig, l_aux, name_len;
  uint64_t l_seq, q_cig, q_seq, q_qual;
};

__device__ __forceinline__ RecView view_of(const uint8_t *r, const RecSizes &z, uint32_t lane) {
  RecView v;
  v.r = r;
  v.f = fixed_of(v.r);
  v.l_name = z.l_name;
  v.n_cig = z.n_cig;
  v.l_seq = z.l_seq;
  v.l_aux = z.l_aux;
  v.q_cig = 36 + v.l_name;
  v.q_seq = v.q_cig + 4ull * v.n_cig;
  v.q_qual = v.q_seq + (v.l_seq + 1) / 2;
  v.aux = v.r + v.q_qual + v.l_seq;
  // the name ends at its first NUL (l_name <= 255: at most four steps)
  v.name_len = v.l_name;
  for (uint32_t k0 = 0; k0 < v.l_name; k0 += WAVE) {
    const uint32_t k = k0 + lane;
    const unsigned long long m = __ballot(k < v.l_name && v.r[36 + k] == 0);
    if (m) {
      v.name_len = k0 + first_lane(m);
      break;
    }
  }
  return v;
}

// first NUL of aux[from, l_aux), or l_aux when there is none
__device__ __forceinline__ uint32_t find_nul(const uint8_t *aux, uint32_t from, uint32_t l_aux, uint32_t lane) {
  for (uint32_t k0 = from; k0 < l_aux; k0 += WAVE) {
    const uint32_t k = k0 + lane;
    const unsigned long long m = __ballot(k < l_aux && aux[k] == 0);
    if (m) return k0 + first_lane(m);
  }
  return l_aux;
}

__device__ __forceinline__ void size_record(const uint8_t *r, const RecSizes &z, const Refs &R, uint64_t i,
                                            uint32_t lane, uint64_t *len, uint64_t *hostf, unsigned long long *bad) {
  {
    const RecView v = view_of(r, z, lane);
    bool ok = true, has_f = false;
    // CIGAR: digits(len) + 1 per op, strided over the lanes
    uint64_t cigar = 1;
    if (v.n_cig) {
      uint32_t s = 0, bad_op = 0;
      for (uint32_t k = lane; k < v.n_cig; k += WAVE) {
        const uint32_t op = ld32(v.r + v.q_cig + 4ull * k);
        bad_op |= !cigar_op_ok(op);
        s += cigar_op_len(op);
      }
      cigar = wave_sum(s);
      ok = !__any((int)bad_op);
    }
    // tags: a wave-uniform cursor
    uint64_t tags = 0;
    for (uint32_t cur = 0; ok && cur < v.l_aux;) {
      Tag t;
      if (!tag_head(v.aux, v.l_aux, cur, &t)) {
        ok = false;
        break;
      }
      const uint8_t *val = v.aux + t.val;
      if (t.type == 'Z' || t.type == 'H') {
        const uint32_t nul = find_nul(v.aux, t.val, v.l_aux, lane);
        if (nul == v.l_aux) {
          ok = false;
          break;
        }
        tags += TAG_PREFIX + (nul - t.val);
        cur = nul + 1;
        continue;
      }
      uint64_t vl = 1;  // A; B: the sub-type letter
      if (t.type == 'f' || t.sub == 'f') {
        has_f = true;
      } else if (t.type == 'B') {
        uint64_t s = 0;  // (up to 2^31 one-byte elements of up to 5 bytes of text: past 32 bits)
        for (uint32_t k = lane; k < t.count; k += WAVE) s += 1 + sdec_len(tag_int(t.sub, val + (uint64_t)k * t.esz));
        vl += wave_sum64(s);
      } else if (t.type != 'A') {
        vl = sdec_len(tag_int(t.type, val));
      }
      tags += TAG_PREFIX + vl;
      cur = t.val + t.size;
    }
    if (lane == 0) {
      uint64_t l = 0;
      if (!ok) atomicMin(bad, (unsigned long long)i);
      else if (!has_f)
        l = line_len(v.name_len, fixed_text_len(v.f, R), cigar, v.l_seq ? v.l_seq : 1,
                     v.l_seq == 0 || v.r[v.q_qual] == 0xFF ? 1 : v.l_seq, tags);
      len[i] = l;
      hostf[i] = ok && has_f;
    }
  }
}

__global__ __launch_bounds__(256) void k_sam_sizes(const uint8_t *__restrict__ U, const uint64_t *pos, uint64_t n,
                                                   const uint64_t *nm_off, const uint64_t *cg_off,
                                                   const uint64_t *sq_off, const uint64_t *ax_off, Refs R,
                                                   uint64_t *len, uint64_t *hostf, unsigned long long *bad) {
  __shared__ uint8_t stage[256 / WAVE][STAGE];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x / WAVE);
  for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; i < n; i += nw) {
    const RecSizes z = sizes_of(nm_off, cg_off, sq_off, ax_off, i);
    const uint8_t *g = U + pos[i];
    if (z.bytes <= STAGE) {
      uint8_t *slot = stage[threadIdx.x / WAVE];
      stage_record(slot, g, (uint32_t)z.bytes, lane);
      size_record(slot, z, R, i, lane, len, hostf, bad);
    } else {
      size_record(g, z, R, i, lane, len, hostf, bad);
    }
  }
}

// The emit pass's cursor in one line: dst[0, lim) is the line, o the running offset (wave-uniform).
struct Line {
  char *dst;
  uint64_t lim, o;
  uint32_t lane;
  __device__ __forceinline__ bool room(uint64_t n) const { return o + n <= lim; }
  // n consecutive bytes from src, strided over the lanes: one run of stores per 64 bytes
  __device__ __forceinline__ void copy(const void *src, uint64_t n) {
    if (room(n))
      for (uint64_t k = lane; k < n; k += WAVE) dst[o + k] = ((const char *)src)[k];
    o += n;
  }
  __device__ __forceinline__ void ch(char c) {
    if (lane == 0 && room(1)) dst[o] = c;
    ++o;
  }
  __device__ __forceinline__ void dec(int64_t v) {
    const uint32_t n = sdec_len(v);
    if (lane == 0 && room(n)) put_sdec(dst + o, v);
    o += n;
  }
  __device__ __forceinline__ void ref(const Refs &R, int32_t k) {
    if (k == REF_STAR) ch('*');
    else if (k == REF_EQ) ch('=');
    else copy(R.names + R.off[k], R.off[k + 1] - R.off[k]);
  }
};

// (Putting a line together in LDS and writing it out in aligned 4-byte stores was built and
// measured: no change, 68.8 against 68.4 ms for the two passes -- the passes are bound by the
// instructions a whole wave issues for one record's serial walk, not by their stores)
__device__ __forceinline__ void emit_record(const uint8_t *r, const RecSizes &z, const Refs &R, Line L) {
  {
    const uint32_t lane = L.lane;
    const RecView v = view_of(r, z, lane);
    L.copy(v.r + 36, v.name_len);
    L.ch('\t');
    L.dec(v.f.flag);
    L.ch('\t');
    L.ref(R, rname_ref(v.f, R.n));
    L.ch('\t');
    L.dec((int64_t)v.f.pos + 1);
    L.ch('\t');
    L.dec(v.f.mapq);
    L.ch('\t');
    if (!v.n_cig) L.ch('*');
    for (uint32_t k0 = 0; k0 < v.n_cig; k0 += WAVE) {  // 64 ops per step, placed by a prefix sum
      const uint32_t k = k0 + lane;
      const uint32_t op = k < v.n_cig ? ld32(v.r + v.q_cig + 4ull * k) : 0;
      const uint32_t mine = k < v.n_cig ? cigar_op_len(op) : 0;
      const uint32_t incl = wave_incl_scan(mine);
      const uint64_t at = L.o + incl - mine;
      if (mine && at + mine <= L.lim) put_cigar_op(L.dst + at, op);
      L.o += (uint32_t)__shfl((int)incl, WAVE - 1);
    }
    L.ch('\t');
    L.ref(R, rnext_ref(v.f, R.n));
    L.ch('\t');
    L.dec((int64_t)v.f.next_pos + 1);
    L.ch('\t');
    L.dec(v.f.tlen);
    L.ch('\t');
    if (!v.l_seq) L.ch('*');
    else {
      if (L.room(v.l_seq))
        for (uint64_t k = lane; k < v.l_seq; k += WAVE) L.dst[L.o + k] = seq_letter(v.r + v.q_seq, k);
      L.o += v.l_seq;
    }
    L.ch('\t');
    if (v.l_seq == 0 || v.r[v.q_qual] == 0xFF) L.ch('*');
    else {
      if (L.room(v.l_seq))
        for (uint64_t k = lane; k < v.l_seq; k += WAVE) L.dst[L.o + k] = (char)(uint8_t)(v.r[v.q_qual + k] + 33);
      L.o += v.l_seq;
    }
    for (uint32_t cur = 0; cur < v.l_aux;) {
      Tag t;
      if (!tag_head(v.aux, v.l_aux, cur, &t)) break;  // (the size pass has refused such a row)
      if (lane == 0 && L.room(TAG_PREFIX)) put_tag_prefix(L.dst + L.o, v.aux, cur, t.type);
      L.o += TAG_PREFIX;
      const uint8_t *val = v.aux + t.val;
      if (t.type == 'Z' || t.type == 'H') {
        const uint32_t nul = find_nul(v.aux, t.val, v.l_aux, lane);
        if (nul == v.l_aux) break;
        L.copy(val, nul - t.val);
        cur = nul + 1;
        continue;
      }
      if (t.type == 'A') L.ch((char)val[0]);
      else if (t.type == 'B') {
        L.ch((char)t.sub);
        if (t.sub != 'f')  // (a row with floats is the host's)
          for (uint32_t k0 = 0; k0 < t.count; k0 += WAVE) {
            const uint32_t k = k0 + lane;
            const int64_t x = k < t.count ? tag_int(t.sub, val + (uint64_t)k * t.esz) : 0;
            const uint32_t mine = k < t.count ? 1 + sdec_len(x) : 0;
            const uint32_t incl = wave_incl_scan(mine);
            const uint64_t at = L.o + incl - mine;
            if (mine && at + mine <= L.lim) {
              L.dst[at] = ',';
              put_sdec(L.dst + at + 1, x);
            }
            L.o += (uint32_t)__shfl((int)incl, WAVE - 1);
          }
      } else if (t.type != 'f') {
        L.dec(tag_int(t.type, val));
      }
      cur = t.val + t.size;
    }
    L.ch('\n');
  }
}

__global__ __launch_bounds__(256) void k_sam_emit(const uint8_t *__restrict__ U, const uint64_t *pos, uint64_t n,
                                                  const uint64_t *nm_off, const uint64_t *cg_off,
                                                  const uint64_t *sq_off, const uint64_t *ax_off, Refs R,
                                                  const uint64_t *line_off, const uint64_t *hostf, char *text) {
  __shared__ uint8_t stage[256 / WAVE][STAGE];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x / WAVE);
  for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; i < n; i += nw) {
    if (hostf[i]) continue;
    const RecSizes z = sizes_of(nm_off, cg_off, sq_off, ax_off, i);
    const uint8_t *g = U + pos[i];
    const Line L{text + line_off[i], line_off[i + 1] - line_off[i], 0, lane};
    if (z.bytes <= STAGE) {
      uint8_t *slot = stage[threadIdx.x / WAVE];
      stage_record(slot, g, (uint32_t)z.bytes, lane);
      emit_record(slot, z, R, L);
    } else {
      emit_record(g, z, R, L);
    }
  }
}

// The host rows: row j of the compacted list is record rows[j]; its start and its bytes (4 +
// block_size) go to the host with it.
__global__ void k_sam_host_rows(const uint8_t *__restrict__ U, const uint64_t *pos, const uint64_t *hostf,
                                const uint64_t *hpre, uint64_t n, uint64_t *rows, uint64_t *rec_bytes) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !hostf[i]) return;
  rows[hpre[i]] = i;
  rec_bytes[hpre[i]] = 4 + (uint64_t)ld32(U + pos[i]);
}

// The host rows' record bytes packed one after another (goff: their prefix offsets), a wave per record.
__global__ __launch_bounds__(256) void k_sam_gather(const uint8_t *__restrict__ U, const uint64_t *pos,
                                                    const uint64_t *rows, const uint64_t *goff, uint64_t m,
                                                    uint8_t *out) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x / WAVE);
  for (uint64_t j = (uint64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; j < m; j += nw) {
    const uint8_t *src = U + pos[rows[j]];
    const uint64_t nb = goff[j + 1] - goff[j];
    for (uint64_t k = lane; k < nb; k += WAVE) out[goff[j] + k] = src[k];
  }
}

// len[rows[j]] = vals[j]: the host-rendered lines' lengths into their holes, before the second scan
__global__ void k_sam_scatter(const uint64_t *rows, const uint64_t *vals, uint64_t m, uint64_t n, uint64_t *len) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m && rows[j] < n) len[rows[j]] = vals[j];
}

uint32_t wave_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + 3) / 4, 65536); }  // 4 waves per workgroup

}  // namespace

// len / hostf: n + 1 words (the caller zeroes entry n); names / name_off: the packed reference names
// on the device.
static hipError_t launch_sam_sizes(const uint8_t *U, const uint64_t *pos, uint64_t n, const uint64_t *nm_off,
                                   const uint64_t *cg_off, const uint64_t *sq_off, const uint64_t *ax_off, const char *names,
                                   const uint64_t *name_off, int32_t n_ref, uint64_t *len, uint64_t *hostf,
                                   unsigned long long *bad, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_sam_sizes, dim3(wave_grid(n)), dim3(256), 0, st, U, pos, n, nm_off, cg_off, sq_off, ax_off,
                     Refs{names, name_off, n_ref}, len, hostf, bad);
  return hipGetLastError();
}

static hipError_t launch_sam_emit(const uint8_t *U, const uint64_t *pos, uint64_t n, const uint64_t *nm_off,
                                  const uint64_t *cg_off, const uint64_t *sq_off, const uint64_t *ax_off, const char *names,
                                  const uint64_t *name_off, int32_t n_ref, const uint64_t *line_off, const uint64_t *hostf,
                                  char *text, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_sam_emit, dim3(wave_grid(n)), dim3(256), 0, st, U, pos, n, nm_off, cg_off, sq_off, ax_off,
                     Refs{names, name_off, n_ref}, line_off, hostf, text);
  return hipGetLastError();
}

// the rows with hostf set (hpre: its exclusive scan), compacted: their indices and record sizes
static hipError_t launch_sam_host_rows(const uint8_t *U, const uint64_t *pos, const uint64_t *hostf, const uint64_t *hpre,
                                       uint64_t n, uint64_t *rows, uint64_t *rec_bytes, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_sam_host_rows, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, U, pos, hostf, hpre, n, rows,
                     rec_bytes);
  return hipGetLastError();
}

// those m rows' record bytes packed at goff
static hipError_t launch_sam_gather(const uint8_t *U, const uint64_t *pos, const uint64_t *rows, const uint64_t *goff,
                                    uint64_t m, uint8_t *out, hipStream_t st) {
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_sam_gather, dim3(wave_grid(m)), dim3(256), 0, st, U, pos, rows, goff, m, out);
  return hipGetLastError();
}

// their lines' lengths (vals) back into len
static hipError_t launch_sam_scatter(const uint64_t *rows, const uint64_t *vals, uint64_t m, uint64_t n, uint64_t *len,
                                     hipStream_t st) {
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_sam_scatter, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, rows, vals, m, n, len);
  return hipGetLastError();
}

}  // namespace sbh

using namespace sbh;

extern "C" {

// ---- the C-ABI's SAM text calls (the line is defined in sam_core.h) --------------------------
// Size pass, scan, emit pass over the rows of the last decoded scan.  Both scans (line lengths,
// host-row flags) are launched before anything is read back, so the common case -- no row with
// a float tag -- costs one round trip for (bad row, n_host, total) before the text is allocated
// and written.  With host rows: their indices and record bytes come to the host, sam_core.h's
// renderer writes their lines, the lengths go back into len[] and the scan runs again; the lines
// themselves are put into their holes by sbh_records_sam_fetch.
int sbh_records_sam_scan(sbh_shard *sh, const char *ref_names, const uint64_t *ref_name_off, int32_t n_ref,
                         sbh_sam_sizes *out) {
  if (!sh || !out || n_ref < 0 || (n_ref && (!ref_names || !ref_name_off))) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &R = sh->rec;
  auto &S = sh->sam;
  if (!R.valid || !R.decoded) return fail(ctx, SBH_E_STATE, "records_sam_scan without a decoded records scan");
  for (int32_t k = 0; k < n_ref; ++k)
    if (ref_name_off[k + 1] < ref_name_off[k]) return fail(ctx, SBH_E_ARG, "reference name offsets must not decrease");
  int rc = set_device(ctx);
  if (rc) return rc;
  hipStream_t st = sh->st;
  S.valid = false;
  S.h_rows.clear();
  S.h_off.assign(1, 0);
  S.h_text.clear();
  const uint64_t n = R.sz.n;
  if (!n) {
    S.sz = sbh_sam_sizes{0, 0, 0};
    S.valid = true;
    *out = S.sz;
    return SBH_OK;
  }
  const uint64_t name_bytes = n_ref ? ref_name_off[n_ref] - ref_name_off[0] : 0;
  std::vector<uint64_t> roff((size_t)n_ref + 1, 0);  // rebased to the first name
  for (int32_t k = 0; k <= n_ref && n_ref; ++k) roff[k] = ref_name_off[k] - ref_name_off[0];
  HIPCHK(ctx, S.refs.ensure(name_bytes + 1));
  HIPCHK(ctx, S.ref_off.ensure((uint64_t)n_ref + 1));
  if (name_bytes)
    HIPCHK(ctx, hipMemcpyAsync(S.refs.p, ref_names + ref_name_off[0], name_bytes, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(S.ref_off.p, roff.data(), 8 * ((uint64_t)n_ref + 1), hipMemcpyHostToDevice, st));
  for (auto *b : {&S.len, &S.off, &S.hostf, &S.hpre}) HIPCHK(ctx, b->ensure(n + 1));
  HIPCHK(ctx, sh->tmp.ensure(scan_tmp_words(n + 1)));
  HIPCHK(ctx, hipMemsetAsync(S.len.p + n, 0, 8, st));
  HIPCHK(ctx, hipMemsetAsync(S.hostf.p + n, 0, 8, st));
  unsigned long long *bad = sh->ctr.p + ctr::SAM_BAD;  // first malformed row
  HIPCHK(ctx, hipMemsetAsync(bad, 0xff, 8, st));
  HIPCHK(ctx, launch_sam_sizes(sh->U.p, R.pos.p, n, R.nmo.p, R.cgo.p, R.sqo.p, R.axo.p, S.refs.p, S.ref_off.p, n_ref,
                               S.len.p, S.hostf.p, bad, st));
  HIPCHK(ctx, scan_exclusive_u64(S.hostf.p, S.hpre.p, n + 1, sh->tmp.p, st));
  HIPCHK(ctx, scan_exclusive_u64(S.len.p, S.off.p, n + 1, sh->tmp.p, st));  // (speculative: right when n_host == 0)
  HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::SAM_BAD, bad, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_SAM_NHOST, S.hpre.p + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_SAM_TOTAL, S.off.p + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (sh->h_ctr[ctr::SAM_BAD] != ~0ull)
    return fail_with(ctx, SBH_E_BAD_RECORD, {(int64_t)sh->h_ctr[ctr::SAM_BAD]},
                     "record %llu of the scan has a malformed CIGAR or tag area",
                     (unsigned long long)sh->h_ctr[ctr::SAM_BAD]);
  const uint64_t n_host = sh->h_ctr[ctr::H_SAM_NHOST];
  uint64_t total = sh->h_ctr[ctr::H_SAM_TOTAL];
  if (n_host) {
    for (auto *b : {&S.rows, &S.rbytes}) HIPCHK(ctx, b->ensure(n_host));
    HIPCHK(ctx, S.goff.ensure(n_host + 1));
    HIPCHK(ctx, launch_sam_host_rows(sh->U.p, R.pos.p, S.hostf.p, S.hpre.p, n, S.rows.p, S.rbytes.p, st));
    S.h_rows.resize(n_host);
    std::vector<uint64_t> goff(n_host + 1, 0), hlen(n_host);
    HIPCHK(ctx, hipMemcpyAsync(S.h_rows.data(), S.rows.p, 8 * n_host, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(hlen.data(), S.rbytes.p, 8 * n_host, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (uint64_t j = 0; j < n_host; ++j) goff[j + 1] = goff[j] + hlen[j];
    std::vector<uint8_t> recs(goff[n_host]);
    HIPCHK(ctx, S.gbuf.ensure(goff[n_host]));
    HIPCHK(ctx, hipMemcpyAsync(S.goff.p, goff.data(), 8 * (n_host + 1), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, launch_sam_gather(sh->U.p, R.pos.p, S.rows.p, S.goff.p, n_host, S.gbuf.p, st));
    HIPCHK(ctx, hipMemcpyAsync(recs.data(), S.gbuf.p, goff[n_host], hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const sbh_sam::Refs refs{ref_names + ref_name_off[0], roff.data(), n_ref};
    S.h_off.assign(n_host + 1, 0);
    uint64_t bad_row = 0;
    int hr = sbh_sam::render_host(recs.data(), recs.size(), goff.data(), n_host, refs, nullptr, 0, S.h_off.data(), &bad_row);
    if (!hr) {
      S.h_text.resize(S.h_off[n_host]);
      hr = sbh_sam::render_host(recs.data(), recs.size(), goff.data(), n_host, refs, S.h_text.data(), S.h_text.size(),
                                S.h_off.data(), &bad_row);
    }
    if (hr)
      return fail_with(ctx, SBH_E_BAD_RECORD, {(int64_t)S.h_rows[bad_row]}, "record %llu of the scan has a malformed CIGAR or tag area",
                       (unsigned long long)S.h_rows[bad_row]);
    for (uint64_t j = 0; j < n_host; ++j) hlen[j] = S.h_off[j + 1] - S.h_off[j];
    HIPCHK(ctx, hipMemcpyAsync(S.rbytes.p, hlen.data(), 8 * n_host, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, launch_sam_scatter(S.rows.p, S.rbytes.p, n_host, n, S.len.p, st));
    HIPCHK(ctx, scan_exclusive_u64(S.len.p, S.off.p, n + 1, sh->tmp.p, st));
    HIPCHK(ctx, hipMemcpyAsync(sh->h_ctr + ctr::H_SAM_TOTAL, S.off.p + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    total = sh->h_ctr[ctr::H_SAM_TOTAL];
  }
  HIPCHK(ctx, S.text.ensure(total));
  HIPCHK(ctx, launch_sam_emit(sh->U.p, R.pos.p, n, R.nmo.p, R.cgo.p, R.sqo.p, R.axo.p, S.refs.p, S.ref_off.p, n_ref,
                              S.off.p, S.hostf.p, S.text.p, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  S.sz = sbh_sam_sizes{n, total, n_host};
  S.valid = true;
  *out = S.sz;
  return SBH_OK;
}

int sbh_records_sam_fetch(sbh_shard *sh, char *text, uint64_t *line_off) {
  if (!sh) return SBH_E_ARG;
  sbh_ctx *ctx = sh->ctx;
  auto &S = sh->sam;
  if (!S.valid) return fail(ctx, SBH_E_STATE, "records_sam_fetch without a records_sam_scan");
  const uint64_t n = S.sz.n;
  if (!n) {
    if (line_off) line_off[0] = 0;
    return SBH_OK;
  }
  int rc = set_device(ctx);
  if (rc) return rc;
  std::vector<uint64_t> own;  // the holes' offsets when the caller does not want line_off
  if (!line_off && text && S.sz.n_host) {
    own.resize(n + 1);
    line_off = own.data();
  }
  if (text && S.sz.text_bytes) HIPCHK(ctx, hipMemcpyAsync(text, S.text.p, S.sz.text_bytes, hipMemcpyDeviceToHost, sh->st));
  if (line_off) HIPCHK(ctx, hipMemcpyAsync(line_off, S.off.p, 8 * (n + 1), hipMemcpyDeviceToHost, sh->st));
  HIPCHK(ctx, hipStreamSynchronize(sh->st));
  if (text)
    for (uint64_t j = 0; j < S.sz.n_host; ++j)
      std::memcpy(text + line_off[S.h_rows[j]], S.h_text.data() + S.h_off[j], S.h_off[j + 1] - S.h_off[j]);
  return SBH_OK;
}

int sbh_sam_render_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                        const char *ref_names, const uint64_t *ref_name_off, int32_t n_ref, char *text,
                        uint64_t text_cap, uint64_t *line_off, uint64_t *bad_row) {
  if ((!flat && flat_size) || (!starts && n) || !line_off || n_ref < 0 || (n_ref && (!ref_names || !ref_name_off)))
    return SBH_E_ARG;
  for (int32_t k = 0; k < n_ref; ++k)
    if (ref_name_off[k + 1] < ref_name_off[k]) return SBH_E_ARG;
  uint64_t bad = sbh_sam::NO_ROW;
  const int rc = sbh_sam::render_host(flat, flat_size, starts, n, sbh_sam::Refs{ref_names, ref_name_off, n_ref}, text,
                                      text_cap, line_off, &bad);
  if (bad_row) *bad_row = bad;
  return rc == 0 ? SBH_OK : rc == 1 ? SBH_E_BAD_RECORD : SBH_E_ARG;
}

}  // extern "C"
