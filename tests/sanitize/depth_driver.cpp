// depth_driver.cpp -- the host add and finish of csrc/depth_core.h under the sanitizers
// (tests/test_depth_sanitize_cpu.py builds this with -fsanitize=address,undefined and runs it).
//
// Input file (little endian, written by depth_corpus.driver_input): u64 flat_size, the flat bytes,
// u64 n, n u64 record starts, u64 n_spans, the spans (sbh_depth_span's 24 bytes each), i32 n_ref,
// u32 flags, u32 flag_require, u32 flag_exclude, i32 min_mapq, u64 n_ranges, the ranges' begins,
// their ends.  Every buffer is heap-allocated at its exact size -- the slots at exactly the spans'
// slots, the runs at exactly n_runs -- so a read or write one slot past either is an ASan report.
// Adds, finishes twice (sizes only on a copy, then with the runs) and prints
//   "<status> <bad_row> <n> <n_kept> <n_counted> <n_unplaced> <cov_bases> <slots> <n_runs> <covered>
//    <sum> <max_depth> <fnv1a64 of the depth array> <fnv1a64 of the runs>"
// status 0 ok, 1 a bad row (bad_row names it; the slots must still be zero: 5 if not), 2 bad
// spans or filter, 3 the two finishes disagreed.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "depth_core.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static uint64_t fnv(uint64_t h, const void *p, size_t n) {
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
  return h;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t flat_size = 0, n = 0, n_spans = 0, n_ranges = 0;
  int32_t n_ref = 0, min_mapq = 0;
  uint32_t flags = 0, require = 0, exclude = 0;
  if (!rd(f, &flat_size, 8)) return 2;
  std::vector<uint8_t> flat(flat_size);
  if (!rd(f, flat.data(), flat_size) || !rd(f, &n, 8)) return 2;
  std::vector<uint64_t> starts(n);
  if (!rd(f, starts.data(), 8 * n) || !rd(f, &n_spans, 8)) return 2;
  std::vector<sbh_dep::Span> spans(n_spans);
  static_assert(sizeof(sbh_dep::Span) == 24 && sizeof(sbh_dep::Run) == 24, "the layouts the test hashes");
  if (!rd(f, spans.data(), 24 * n_spans) || !rd(f, &n_ref, 4) || !rd(f, &flags, 4) || !rd(f, &require, 4) ||
      !rd(f, &exclude, 4) || !rd(f, &min_mapq, 4) || !rd(f, &n_ranges, 8))
    return 2;
  std::vector<uint64_t> rb(n_ranges), re(n_ranges);
  if (!rd(f, rb.data(), 8 * n_ranges) || !rd(f, re.data(), 8 * n_ranges)) return 2;
  fclose(f);

  const uint64_t h0 = 0xcbf29ce484222325ull;
  uint64_t bad = 0, hd = h0, hr = h0;
  sbh_dep::AddResult add{n, 0, 0, 0, 0};
  sbh_dep::Sizes sz{0, 0, 0, 0, 0, 0};
  int status = 0;
  const sbh_bam::Filter F{require, exclude, min_mapq, rb.data(), re.data(), n_ranges};
  if (!sbh_bam::filter_ok(F) || !sbh_dep::spans_ok(spans.data(), (uint32_t)n_spans, n_ref)) {
    status = 2;
  } else {
    std::vector<int32_t> slots(sbh_dep::slots_of(spans.data(), (uint32_t)n_spans), 0);
    status = sbh_dep::add_host(flat.data(), flat_size, starts.data(), n, F, spans.data(), (uint32_t)n_spans, n_ref,
                               flags, slots.data(), &add, &bad);
    if (status == 1) {
      for (int32_t v : slots)
        if (v) status = 5;
    } else {
      std::vector<int32_t> probe(slots);
      sbh_dep::Sizes first{};
      sbh_dep::finish_host(probe.data(), spans.data(), (uint32_t)n_spans, nullptr, 0, &first);
      std::vector<sbh_dep::Run> runs(first.n_runs);
      sbh_dep::finish_host(slots.data(), spans.data(), (uint32_t)n_spans, runs.data(), runs.size(), &sz);
      if (sz.n_runs != first.n_runs || sz.sum != first.sum || probe != slots) status = 3;
      hd = fnv(hd, slots.data(), 4 * slots.size());
      hr = fnv(hr, runs.data(), 24 * runs.size());
    }
  }
  printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
         " %" PRIu64 " %u %016" PRIx64 " %016" PRIx64 "\n",
         status, bad, add.n, add.n_kept, add.n_counted, add.n_unplaced, add.cov_bases, sz.slots, sz.n_runs, sz.covered,
         sz.sum, sz.max_depth, hd, hr);
  return 0;
}
