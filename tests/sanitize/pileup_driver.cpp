// pileup_driver.cpp -- the host add and finish of csrc/pileup_core.h under the sanitizers
// (tests/test_pileup_sanitize_cpu.py builds this with -fsanitize=address,undefined and runs it).
//
// Input file (little endian, written by pileup_corpus.driver_input): u64 flat_size, the flat bytes,
// u64 n, n u64 record starts, u64 n_spans, the spans (sbh_depth_span's 24 bytes each), i32 n_ref,
// u32 min_baseq, u32 min_depth, u32 call_pct, u32 flag_require, u32 flag_exclude, i32 min_mapq, u64
// n_ranges, the ranges' begins, their ends.  The flat bytes are copied into a heap block of exactly
// flat_size bytes and the counts, calls and intervals are allocated at exactly positions * 8,
// positions and n_intervals -- so a nibble, a quality byte, a counter or an interval one past
// either end is an ASan report.
// Adds, finishes twice (sizes only, then with the intervals) and prints
//   "<status> <bad_row> <n> <n_kept> <n_counted> <n_unplaced> <8 add totals> <positions>
//    <n_intervals> <nonzero> <n_called> <covered> <max_depth> <8 finish totals> <fnv1a64 of the
//    counts> <of the calls> <of the intervals>"
// status 0 ok, 1 a bad row (bad_row names it; the counts must still be zero: 5 if not), 2 bad
// spans, filter or parameters, 3 the two finishes disagreed.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "pileup_core.h"

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
  uint32_t min_baseq = 0, min_depth = 0, call_pct = 0, require = 0, exclude = 0;
  if (!rd(f, &flat_size, 8)) return 2;
  std::unique_ptr<uint8_t[]> flat(new uint8_t[flat_size]);  // (exactly flat_size: no vector slack)
  if (!rd(f, flat.get(), flat_size) || !rd(f, &n, 8)) return 2;
  std::vector<uint64_t> starts(n);
  if (!rd(f, starts.data(), 8 * n) || !rd(f, &n_spans, 8)) return 2;
  std::vector<sbh_dep::Span> spans(n_spans);
  static_assert(sizeof(sbh_dep::Span) == 24, "the layout the test hashes");
  if (!rd(f, spans.data(), 24 * n_spans) || !rd(f, &n_ref, 4) || !rd(f, &min_baseq, 4) || !rd(f, &min_depth, 4) ||
      !rd(f, &call_pct, 4) || !rd(f, &require, 4) || !rd(f, &exclude, 4) || !rd(f, &min_mapq, 4) || !rd(f, &n_ranges, 8))
    return 2;
  std::vector<uint64_t> rb(n_ranges), re(n_ranges);
  if (!rd(f, rb.data(), 8 * n_ranges) || !rd(f, re.data(), 8 * n_ranges)) return 2;
  fclose(f);

  const uint64_t h0 = 0xcbf29ce484222325ull;
  uint64_t bad = 0, hc = h0, hk = h0, hi = h0;
  sbh_pile::AddResult add{};
  add.n = n;
  sbh_pile::Sizes sz{};
  int status = 0;
  const sbh_bam::Filter F{require, exclude, min_mapq, rb.data(), re.data(), n_ranges};
  if (!sbh_bam::filter_ok(F) || !sbh_dep::spans_ok(spans.data(), (uint32_t)n_spans, n_ref) || min_baseq > 255 ||
      min_depth < 1 || call_pct < 1 || call_pct > 100) {
    status = 2;
  } else {
    const uint64_t S = sbh_pile::positions_of(spans.data(), (uint32_t)n_spans);
    std::unique_ptr<uint32_t[]> counts(new uint32_t[8 * S]());
    status = sbh_pile::add_host(flat.get(), flat_size, starts.data(), n, F, spans.data(), (uint32_t)n_spans, n_ref,
                                min_baseq, counts.get(), &add, &bad);
    if (status == 1) {
      for (uint64_t i = 0; i < 8 * S; ++i)
        if (counts[i]) status = 5;
    } else {
      std::unique_ptr<uint8_t[]> probe(new uint8_t[S]), calls(new uint8_t[S]);
      sbh_pile::Sizes first{};
      sbh_pile::finish_host(counts.get(), spans.data(), (uint32_t)n_spans, min_depth, call_pct, probe.get(), nullptr, 0,
                            &first);
      std::unique_ptr<sbh_dep::Span[]> ivals(new sbh_dep::Span[first.n_intervals]);
      sbh_pile::finish_host(counts.get(), spans.data(), (uint32_t)n_spans, min_depth, call_pct, calls.get(), ivals.get(),
                            first.n_intervals, &sz);
      if (sz.n_intervals != first.n_intervals || sz.nonzero != first.nonzero || memcmp(probe.get(), calls.get(), S))
        status = 3;
      hc = fnv(hc, counts.get(), 32 * S);
      hk = fnv(hk, calls.get(), S);
      hi = fnv(hi, ivals.get(), 24 * sz.n_intervals);
    }
  }
  printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64, status, bad, add.n, add.n_kept, add.n_counted,
         add.n_unplaced);
  for (int k = 0; k < 8; ++k) printf(" %" PRIu64, add.totals[k]);
  printf(" %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u", sz.positions, sz.n_intervals, sz.nonzero,
         sz.n_called, sz.covered, sz.max_depth);
  for (int k = 0; k < 8; ++k) printf(" %" PRIu64, sz.totals[k]);
  printf(" %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", hc, hk, hi);
  return 0;
}
