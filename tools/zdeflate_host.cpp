// Host build of spark-bam_amd/csrc/zdeflate_core.h for the CPU test suite only: the serial
// definition of the byte-exact (zlib 1.2.11 level 5) BGZF writer, checked against the
// container's zlib by tests/test_zdeflate_cpu.py.  Not part of the product library.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../spark-bam_amd/csrc/zdeflate_core.h"

using namespace sbh_zlib;

static ZTreeState g_st;

extern "C" {

// raw deflate of src[0, n) (n <= 65536) as zlib writes it at level 4..9; returns its size
uint32_t sbh_host_zdeflate_raw(const uint8_t *src, uint32_t n, int level, uint8_t *out, uint32_t cap) {
  std::vector<uint16_t> prev(n + 1), head(HASH_MASK + 1);
  std::vector<uint32_t> tok(n + 1);
  std::vector<uint64_t> info(n + 1);
  return z_deflate_serial(src, n, level, out, cap, prev.data(), head.data(), tok.data(), info.data(), g_st);
}

// The stages' intermediate results for one member, for assertions zlib's bytes cannot show (which
// chain a position was searched with, what the search saw): prev[n], the z_info records info[n]
// (with their byte), the positions z_parse visited and the prev_length it had there
// (visit[2 * i], visit[2 * i + 1]), the tokens tok[n + 1], and per block eight words (tok0, tok1,
// byte0, byte1, nobuf, ZB_* type, and _tr_flush_block's opt_lenb and static_lenb before it takes
// the smaller).  counts = {visits, tokens, blocks}.
void sbh_host_zdeflate_trace(const uint8_t *src, uint32_t n, int level, uint16_t *prev, uint64_t *info,
                             uint32_t *visit, uint32_t *tok, uint32_t *blocks, uint32_t *counts) {
  const ZCfg cf = z_config(level);
  std::vector<uint16_t> head(HASH_MASK + 1), pv(n + 1);
  z_prev_serial(src, n, pv.data(), head.data());
  for (uint32_t p = 0; p < n; ++p) prev[p] = p + MIN_MATCH <= n ? pv[p] : 0;
  auto prv = [&](uint32_t i) -> uint32_t { return pv[i]; };
  auto cmp = [&](uint32_t a, uint32_t b, uint32_t lim) -> uint32_t {
    uint32_t l = 0;
    while (l < lim && src[a + l] == src[b + l]) ++l;
    return l;
  };
  for (uint32_t p = 0; p < n; ++p) info[p] = z_rec_with_byte(z_info(prv, cmp, p, n, cf), src[p]);
  // z_parse reads info(p) once per position it visits; prev_length there follows from the
  // records alone (deflate_slow's match_length after the previous iteration), shadowed here
  uint32_t nv = 0, ml = MIN_MATCH - 1;
  auto inf = [&](uint32_t p) -> uint64_t {
    const uint64_t r = info[p];
    const uint32_t pl = ml;
    visit[2 * nv] = p, visit[2 * nv + 1] = pl, ++nv;
    ml = MIN_MATCH - 1;
    if (pl < cf.lazy) {
      const uint32_t M = z_rec_len(r, pl >= cf.good), S = z_rec_start(r, pl >= cf.good);
      if (M > pl && !(M == MIN_MATCH && p - S > TOO_FAR)) ml = M;
    }
    if (pl >= MIN_MATCH && ml <= pl) ml = MIN_MATCH - 1;  // the previous match is emitted
    return r;
  };
  ZBlock zb[MAX_BLOCKS];
  uint32_t ntok = 0;
  const uint32_t nb = z_parse(n, cf, inf, [&](uint32_t k, uint32_t t) { tok[k] = t; }, zb, &ntok);
  for (uint32_t i = 0; i < nb; ++i) {
    int32_t mbl = 0;
    const uint32_t type = z_block_trees(g_st, [&](uint32_t k) { return tok[k]; }, zb[i], &mbl);
    const uint32_t w[8] = {zb[i].tok0, zb[i].tok1, zb[i].byte0, zb[i].byte1, zb[i].nobuf, type,
                           (uint32_t)((g_st.opt_len + 3 + 7) >> 3), (uint32_t)((g_st.static_len + 3 + 7) >> 3)};
    memcpy(blocks + 8 * i, w, sizeof w);
  }
  counts[0] = nv, counts[1] = ntok, counts[2] = nb;
}

}  // extern "C"
