// bam_sort_driver.cpp -- the host sorter and the header rewrite of csrc/bam_sort_core.h under the
// sanitizers (tests/test_bam_sort_sanitize_cpu.py builds this with -fsanitize=address,undefined and
// runs it).
//
// Input file (little endian, written by bam_sort_corpus.driver_input): u64 flat_size, the flat
// bytes, u64 n, n u64 record starts, u64 head_bytes, the header bytes, u64 so_bytes, the sort-order
// value.  Every buffer is heap-allocated at its exact size, so a read or write one byte past it is
// an ASan report.  Sorts, then rewrites the header twice (sizes only, then into a buffer of exactly
// the result's bytes, then into one a byte short) and prints
//   "<status> <bad_row> <fnv1a64 of perm> <header status> <header bytes> <fnv1a64 of the header>"
// status 0 ok, 1 malformed record (bad_row names it); header status 0 ok, 1 refused, 3 / 4 the
// second or the short call disagreed.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bam_sort_core.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static uint64_t fnv(uint64_t h, const void *p, size_t n) {
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
  return h;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t flat_size = 0, n = 0, head_bytes = 0, so_bytes = 0;
  if (!rd(f, &flat_size, 8)) return 2;
  std::vector<uint8_t> flat(flat_size);
  if (!rd(f, flat.data(), flat_size) || !rd(f, &n, 8)) return 2;
  std::vector<uint64_t> starts(n);
  if (!rd(f, starts.data(), 8 * n) || !rd(f, &head_bytes, 8)) return 2;
  std::vector<uint8_t> head(head_bytes);
  if (!rd(f, head.data(), head_bytes) || !rd(f, &so_bytes, 8)) return 2;
  std::vector<char> so(so_bytes + 1, 0);
  if (!rd(f, so.data(), so_bytes)) return 2;
  fclose(f);

  const uint64_t h0 = 0xcbf29ce484222325ull;
  uint64_t bad = 0, hp = h0, hh = h0, out_n = 0;
  std::vector<uint64_t> perm(n, 0);
  const int rc = sbh_bam::sort_host(flat.data(), flat_size, starts.data(), n, perm.data(), &bad);
  if (rc == 0) hp = fnv(hp, perm.data(), 8 * perm.size());

  int hrc = sbh_bam::header_set_so(head.data(), head_bytes, so.data(), nullptr, 0, &out_n);
  if (hrc == 2) {
    std::vector<uint8_t> out(out_n);
    uint64_t n2 = 0;
    hrc = sbh_bam::header_set_so(head.data(), head_bytes, so.data(), out.data(), out_n, &n2);
    if (hrc == 0 && n2 != out_n) hrc = 3;
    hh = fnv(hh, out.data(), out.size());
    if (hrc == 0 && out_n) {  // one byte short: refused, nothing written past the buffer
      std::vector<uint8_t> small(out_n - 1);
      if (sbh_bam::header_set_so(head.data(), head_bytes, so.data(), small.data(), out_n - 1, &n2) != 2) hrc = 4;
    }
  }
  printf("%d %" PRIu64 " %016" PRIx64 " %d %" PRIu64 " %016" PRIx64 "\n", rc, bad, hp, hrc, out_n, hh);
  return 0;
}
