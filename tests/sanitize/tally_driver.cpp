// tally_driver.cpp -- the host add and the two renderers of csrc/tally_core.h under the sanitizers
// (tests/test_tally_sanitize_cpu.py builds this with -fsanitize=address,undefined and runs it).
//
// Input file (little endian, written by tally_corpus.driver_input): u64 flat_size, the flat bytes,
// u64 n, n u64 record starts, i32 n_ref, u32 flag_require, u32 flag_exclude, i32 min_mapq, u64
// n_ranges, the ranges' begins, their ends.  Every buffer is heap-allocated at its exact size -- the
// flag counters at exactly 32 words, the per-reference counters at exactly 2 (n_ref + 1), the names and
// lengths at exactly n_ref -- so a read or write one word past any of them is an ASan report.
// Prints
//   "<status> <bad_row> <n> <n_kept> <fnv1a64 of flag[]> <fnv1a64 of ref[]> <fnv1a64 of the flagstat
//    text> <fnv1a64 of the idxstats text>"
// status 0 ok, 1 a bad row (bad_row names it; the counters must still hold their preset: 5 if not),
// 2 a bad filter or n_ref.  Reference k is named "ref<k>" and is 1000 + k long.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "tally_core.h"

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
  int32_t n_ref = 0, min_mapq = 0;
  uint32_t require = 0, exclude = 0;
  if (!rd(f, &flat_size, 8)) return 2;
  std::vector<uint8_t> flat(flat_size);
  if (!rd(f, flat.data(), flat_size) || !rd(f, &n, 8)) return 2;
  std::vector<uint64_t> starts(n);
  if (!rd(f, starts.data(), 8 * n) || !rd(f, &n_ref, 4) || !rd(f, &require, 4) || !rd(f, &exclude, 4) ||
      !rd(f, &min_mapq, 4) || !rd(f, &n_ranges, 8))
    return 2;
  std::vector<uint64_t> rb(n_ranges), re(n_ranges);
  if (!rd(f, rb.data(), 8 * n_ranges) || !rd(f, re.data(), 8 * n_ranges)) return 2;
  fclose(f);

  const uint64_t h0 = 0xcbf29ce484222325ull;
  uint64_t bad = 0, hf = h0, hr = h0, hft = h0, hit = h0;
  sbh_tal::AddResult add{n, 0};
  int status = 0;
  const sbh_bam::Filter F{require, exclude, min_mapq, rb.data(), re.data(), n_ranges};
  if (!sbh_bam::filter_ok(F) || n_ref < 0) {
    status = 2;
  } else {
    // preset to a value no add leaves behind by chance: a failed add must not have written
    const uint64_t preset = 0x5a5a5a5a5a5a5a5aull;
    std::vector<uint64_t> flag(2 * sbh_tal::TALLY_ROWS, preset), ref(2 * ((size_t)n_ref + 1), preset);
    status = sbh_tal::add_host(flat.data(), flat_size, starts.data(), n, F, n_ref, flag.data(), ref.data(), &add, &bad);
    if (status == 1) {
      for (uint64_t v : flag)
        if (v != preset) status = 5;
      for (uint64_t v : ref)
        if (v != preset) status = 5;
    } else {
      for (uint64_t &v : flag) v -= preset;
      for (uint64_t &v : ref) v -= preset;
      std::vector<std::string> names((size_t)n_ref);
      std::vector<int32_t> lengths((size_t)n_ref);
      for (int32_t k = 0; k < n_ref; ++k) names[k] = "ref" + std::to_string(k), lengths[k] = 1000 + k;
      const std::string ft = sbh_tal::flagstat_text(flag.data());
      const std::string it = sbh_tal::idxstats_text(ref.data(), names.data(), lengths.data(), n_ref);
      hf = fnv(hf, flag.data(), 8 * flag.size());
      hr = fnv(hr, ref.data(), 8 * ref.size());
      hft = fnv(hft, ft.data(), ft.size());
      hit = fnv(hit, it.data(), it.size());
    }
  }
  printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", status, bad,
         add.n, add.n_kept, hf, hr, hft, hit);
  return 0;
}
