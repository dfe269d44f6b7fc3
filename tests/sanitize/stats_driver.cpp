// stats_driver.cpp -- the host add and the renderer of csrc/stats_core.h under the sanitizers
// (tests/test_stats_sanitize_cpu.py builds this with -fsanitize=address,undefined and runs it).
//
// Input file (little endian, written by stats_corpus.driver_input): u64 flat_size, the flat bytes,
// u64 n, n u64 record starts, u32 cycles, u32 max_insert, u32 flag_require, u32 flag_exclude, i32
// min_mapq, u64 n_ranges, the ranges' begins, their ends.  Every buffer is heap-allocated at its exact
// size -- each of the seven tables on its own, at exactly the words the definition gives it -- so a read
// or write one word past any of them is an ASan report.
// Prints
//   "<status> <bad_row> <n> <n_kept> <n_counted> <h sn> <h read_len> <h qual> <h base> <h gc> <h isize>
//    <h mapq> <h text>"
// h of a table: fnv1a64 over (index u64, value u64) of its non-zero words in order; h text: fnv1a64 of
// the report's bytes.  status 0 ok, 1 a bad row (bad_row names it; the tables must still hold their
// preset: 5 if not), 2 bad parameters or a bad filter.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "stats_core.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static uint64_t fnv(uint64_t h, const void *p, size_t n) {
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
  return h;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t flat_size = 0, n = 0, n_ranges = 0;
  int32_t min_mapq = 0;
  uint32_t cycles = 0, max_insert = 0, require = 0, exclude = 0;
  if (!rd(f, &flat_size, 8)) return 2;
  std::vector<uint8_t> flat(flat_size);
  if (!rd(f, flat.data(), flat_size) || !rd(f, &n, 8)) return 2;
  std::vector<uint64_t> starts(n);
  if (!rd(f, starts.data(), 8 * n) || !rd(f, &cycles, 4) || !rd(f, &max_insert, 4) || !rd(f, &require, 4) ||
      !rd(f, &exclude, 4) || !rd(f, &min_mapq, 4) || !rd(f, &n_ranges, 8))
    return 2;
  std::vector<uint64_t> rb(n_ranges), re(n_ranges);
  if (!rd(f, rb.data(), 8 * n_ranges) || !rd(f, re.data(), 8 * n_ranges)) return 2;
  fclose(f);

  const uint64_t h0 = 0xcbf29ce484222325ull;
  uint64_t bad = 0, h[8] = {h0, h0, h0, h0, h0, h0, h0, h0};
  sbh_stat::AddResult add{n, 0, 0};
  int status = 0;
  const sbh_bam::Filter F{require, exclude, min_mapq, rb.data(), re.data(), n_ranges};
  const sbh_stat::Params P{cycles, max_insert};
  if (!sbh_bam::filter_ok(F) || !sbh_stat::params_ok(P)) {
    status = 2;
  } else {
    // preset to a value no add leaves behind by chance: a failed add must not have written
    const uint64_t preset = 0x5a5a5a5a5a5a5a5aull;
    const sbh_stat::Layout l = sbh_stat::layout_of(P);
    const uint64_t size[7] = {l.read_len, l.qual - l.read_len, l.base - l.qual, l.gc - l.base, l.isize - l.gc, l.mapq - l.isize,
                              l.words - l.mapq};
    std::vector<std::vector<uint64_t>> t;
    for (uint64_t s : size) t.emplace_back((size_t)s, preset);
    const sbh_stat::Tables T{t[0].data(), t[1].data(), t[2].data(), t[3].data(), t[4].data(), t[5].data(), t[6].data()};
    t[0][sbh_stat::SN_MAX_LEN] = 0;  // (a maximum, not a sum: its preset is what an add has to beat)
    status = sbh_stat::add_host(flat.data(), flat_size, starts.data(), n, F, P, T, &add, &bad);
    if (status == 1) {
      for (size_t k = 0; k < t.size(); ++k)
        for (size_t i = 0; i < t[k].size(); ++i)
          if (t[k][i] != (k == 0 && i == sbh_stat::SN_MAX_LEN ? 0 : preset)) status = 5;
    } else {
      t[0][sbh_stat::SN_MAX_LEN] += preset;
      for (auto &v : t)
        for (uint64_t &x : v) x -= preset;
      for (int k = 0; k < 7; ++k)
        for (uint64_t i = 0; i < t[k].size(); ++i)
          if (t[k][i]) {
            const uint64_t pair[2] = {i, t[k][i]};
            h[k] = fnv(h[k], pair, 16);
          }
      const std::string text = sbh_stat::stats_text(P, T);
      h[7] = fnv(h[7], text.data(), text.size());
    }
  }
  printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64, status, bad, add.n, add.n_kept, add.n_counted);
  for (uint64_t x : h) printf(" %016" PRIx64, x);
  printf("\n");
  return 0;
}
