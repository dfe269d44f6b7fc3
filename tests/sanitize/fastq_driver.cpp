// fastq_driver.cpp -- the host renderer of csrc/fastq_core.h under the sanitizers
// (tests/test_fastq_sanitize_cpu.py builds this with -fsanitize=address,undefined and runs it).
//
// Input file (little endian, written by fastq_corpus.driver_input): u64 flat_size, the flat bytes,
// u64 n, n u64 record starts, u32 mode, i32 def_qual, u32 flag_require, u32 flag_exclude, i32
// min_mapq, u64 n_ranges, the ranges' begins, their ends.  A sizes-only call comes first; then every
// buffer is heap-allocated at its exact size -- the text at exactly text_bytes, rec_off at exactly
// n_kept + 1, rows at exactly n_kept -- so a read or write one byte past any of them is an ASan
// report.  Prints
//   "<status> <bad_row> <n> <n_kept> <text_bytes> <part bytes x 3> <part rows x 3> <fnv1a64 of the
//    text> <fnv1a64 of rec_off[]> <fnv1a64 of rows[]>"
// status 0 ok, 1 a bad row (bad_row names it), 2 a bad filter, mode or def_qual, 5 the two calls
// disagree, 6 a text one byte short was not refused.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fastq_core.h"

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
  int32_t def_qual = 0, min_mapq = 0;
  uint32_t mode = 0, require = 0, exclude = 0;
  if (!rd(f, &flat_size, 8)) return 2;
  std::vector<uint8_t> flat(flat_size);
  if (!rd(f, flat.data(), flat_size) || !rd(f, &n, 8)) return 2;
  std::vector<uint64_t> starts(n);
  if (!rd(f, starts.data(), 8 * n) || !rd(f, &mode, 4) || !rd(f, &def_qual, 4) || !rd(f, &require, 4) ||
      !rd(f, &exclude, 4) || !rd(f, &min_mapq, 4) || !rd(f, &n_ranges, 8))
    return 2;
  std::vector<uint64_t> rb(n_ranges), re(n_ranges);
  if (!rd(f, rb.data(), 8 * n_ranges) || !rd(f, re.data(), 8 * n_ranges)) return 2;
  fclose(f);

  const uint64_t h0 = 0xcbf29ce484222325ull;
  uint64_t bad = 0, ht = h0, ho = h0, hr = h0;
  sbh_fq::Sizes sz{n, 0, 0, {0, 0, 0}, {0, 0, 0}};
  int status = 0;
  const sbh_bam::Filter F{require, exclude, min_mapq, rb.data(), re.data(), n_ranges};
  if (!sbh_bam::filter_ok(F) || (mode & ~sbh_fq::MODE_ALL) || def_qual < 0 || def_qual > sbh_fq::QUAL_MAX) {
    status = 2;
  } else {
    status = sbh_fq::render_host(flat.data(), flat_size, starts.data(), n, F, mode, def_qual, nullptr, 0, nullptr, nullptr, &sz,
                                 &bad);
    if (status == 0) {
      std::vector<char> text(sz.text_bytes);
      std::vector<uint64_t> rec_off(sz.n_kept + 1), rows(sz.n_kept);
      sbh_fq::Sizes again{};
      if (sz.text_bytes &&
          sbh_fq::render_host(flat.data(), flat_size, starts.data(), n, F, mode, def_qual, text.data(), sz.text_bytes - 1, nullptr,
                              nullptr, &again, &bad) != 2)
        status = 6;
      const int rc = sbh_fq::render_host(flat.data(), flat_size, starts.data(), n, F, mode, def_qual, text.data(), text.size(),
                                         rec_off.data(), rows.data(), &again, &bad);
      if (rc != 0 || memcmp(&again, &sz, sizeof sz) != 0) status = status ? status : 5;
      ht = fnv(ht, text.data(), text.size());
      ho = fnv(ho, rec_off.data(), 8 * rec_off.size());
      hr = fnv(hr, rows.data(), 8 * rows.size());
    }
  }
  printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64, status, bad, sz.n, sz.n_kept, sz.text_bytes);
  for (uint32_t p = 0; p < sbh_fq::PARTS; ++p) printf(" %" PRIu64, sz.part_bytes[p]);
  for (uint32_t p = 0; p < sbh_fq::PARTS; ++p) printf(" %" PRIu64, sz.part_rows[p]);
  printf(" %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", ht, ho, hr);
  return 0;
}
