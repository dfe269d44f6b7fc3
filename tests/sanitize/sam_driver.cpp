// sam_driver.cpp -- the host SAM renderer of csrc/sam_core.h under the sanitizers
// (tests/test_sam_sanitize_cpu.py builds this with -fsanitize=address,undefined and runs it).
//
// Input file (little endian, written by the test): u64 flat_size, the flat bytes, u64 n, n u64
// record starts, u64 n_ref, n_ref + 1 u64 name offsets, the packed names.  Every buffer is
// heap-allocated at its exact size, so a read or write one byte past it is an ASan report.
// Renders twice (sizes only, then the text into a buffer of exactly line_off[n] bytes) and prints
//   "<status> <bad_row> <n> <text_bytes> <fnv1a64 of the text>"
// status 0 ok, 1 malformed record (bad_row names it), 2 capacity.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sam_core.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t flat_size = 0, n = 0, n_ref = 0;
  if (!rd(f, &flat_size, 8)) return 2;
  std::vector<uint8_t> flat(flat_size);
  if (!rd(f, flat.data(), flat_size) || !rd(f, &n, 8)) return 2;
  std::vector<uint64_t> starts(n);
  if (!rd(f, starts.data(), 8 * n) || !rd(f, &n_ref, 8)) return 2;
  std::vector<uint64_t> off(n_ref + 1);
  if (!rd(f, off.data(), 8 * (n_ref + 1))) return 2;
  std::vector<char> names(off[n_ref]);
  if (!rd(f, names.data(), names.size())) return 2;
  fclose(f);
  const sbh_sam::Refs refs{names.data(), off.data(), (int32_t)n_ref};
  std::vector<uint64_t> line_off(n + 1, 0);
  uint64_t bad = 0;
  int rc = sbh_sam::render_host(flat.data(), flat_size, starts.data(), n, refs, nullptr, 0, line_off.data(), &bad);
  uint64_t h = 0xcbf29ce484222325ull, total = 0;
  if (rc == 0) {
    total = line_off[n];
    std::vector<char> text(total);
    std::vector<uint64_t> again(n + 1, 0);
    rc = sbh_sam::render_host(flat.data(), flat_size, starts.data(), n, refs, text.data(), total, again.data(), &bad);
    if (rc == 0 && again != line_off) rc = 3;
    for (char c : text) h = (h ^ (uint8_t)c) * 0x100000001b3ull;
    if (rc == 0 && total) {  // one byte short: refused, nothing written past the buffer
      std::vector<char> small(total - 1);
      if (sbh_sam::render_host(flat.data(), flat_size, starts.data(), n, refs, small.data(), total - 1, again.data(),
                               &bad) != 2)
        rc = 4;
      bad = sbh_sam::NO_ROW;
    }
  }
  printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %016" PRIx64 "\n", rc, bad, n, total, h);
  return 0;
}
