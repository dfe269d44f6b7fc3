// bam_gather_driver.cpp -- the host BAM gatherer of csrc/bam_gather_core.h under the sanitizers
// (tests/test_bam_gather_sanitize_cpu.py builds this with -fsanitize=address,undefined and runs it).
//
// Input file (little endian, written by bam_gather_corpus.driver_input): u64 flat_size, the flat
// bytes, u64 n, n u64 record starts, u64 head_bytes, the head, u32 flag_require, u32 flag_exclude,
// i32 min_mapq, u32 pad, u64 n_row_ranges, the range begins, the range ends.  Every buffer is
// heap-allocated at its exact size, so a read or write one byte past it is an ASan report.
// Gathers twice (sizes only, then into a buffer of exactly the stream's bytes) and prints
//   "<status> <bad_row> <n_kept> <bytes> <fnv1a64 of the stream> <fnv1a64 of rec_off and rows>"
// status 0 ok, 1 malformed record (bad_row names it), 2 capacity, 5 bad filter.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bam_gather_core.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static uint64_t fnv(uint64_t h, const void *p, size_t n) {
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
  return h;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t flat_size = 0, n = 0, head_bytes = 0, nr = 0;
  uint32_t fl[4] = {0, 0, 0, 0};
  if (!rd(f, &flat_size, 8)) return 2;
  std::vector<uint8_t> flat(flat_size);
  if (!rd(f, flat.data(), flat_size) || !rd(f, &n, 8)) return 2;
  std::vector<uint64_t> starts(n);
  if (!rd(f, starts.data(), 8 * n) || !rd(f, &head_bytes, 8)) return 2;
  std::vector<uint8_t> head(head_bytes);
  if (!rd(f, head.data(), head_bytes) || !rd(f, fl, 16) || !rd(f, &nr, 8)) return 2;
  std::vector<uint64_t> rb(nr), re(nr);
  if (!rd(f, rb.data(), 8 * nr) || !rd(f, re.data(), 8 * nr)) return 2;
  fclose(f);
  const sbh_bam::Filter F{fl[0], fl[1], (int32_t)fl[2], rb.data(), re.data(), nr};
  uint64_t n_kept = 0, bytes = 0, bad = 0, h = 0xcbf29ce484222325ull, hi = h;
  int rc = 5;
  if (sbh_bam::filter_ok(F)) {
    std::vector<uint64_t> off(n + 1, 0), rows(n, 0);
    rc = sbh_bam::gather_host(flat.data(), flat_size, starts.data(), n, head.data(), head_bytes, F, nullptr, 0,
                              off.data(), rows.data(), &n_kept, &bytes, &bad);
    if (rc == 0) {
      std::vector<uint8_t> out(bytes);
      std::vector<uint64_t> off2(n_kept + 1, 0), rows2(n_kept, 0);  // exactly what is written
      uint64_t k2 = 0, b2 = 0;
      rc = sbh_bam::gather_host(flat.data(), flat_size, starts.data(), n, head.data(), head_bytes, F, out.data(), bytes,
                                off2.data(), rows2.data(), &k2, &b2, &bad);
      off.resize(n_kept + 1);
      rows.resize(n_kept);
      if (rc == 0 && (k2 != n_kept || b2 != bytes || off2 != off || rows2 != rows)) rc = 3;
      h = fnv(h, out.data(), out.size());
      hi = fnv(fnv(hi, off.data(), 8 * off.size()), rows.data(), 8 * rows.size());
      if (rc == 0 && bytes) {  // one byte short: refused, nothing written past the buffer
        std::vector<uint8_t> small(bytes - 1);
        if (sbh_bam::gather_host(flat.data(), flat_size, starts.data(), n, head.data(), head_bytes, F, small.data(),
                                 bytes - 1, nullptr, nullptr, &k2, &b2, &bad) != 2)
          rc = 4;
        bad = sbh_bam::NO_ROW;
      }
    }
  }
  printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %016" PRIx64 " %016" PRIx64 "\n", rc, bad, n_kept, bytes, h, hi);
  return 0;
}
