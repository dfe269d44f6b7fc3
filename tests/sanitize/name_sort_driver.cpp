// name_sort_driver.cpp -- the host name sorter of csrc/bam_name_core.h under the sanitizers
// (tests/test_name_sort_sanitize_cpu.py builds this with -fsanitize=address,undefined and runs it).
//
// Input file (little endian, written by name_sort_corpus.driver_input): u64 flat_size, the flat
// bytes, u64 n, n u64 record starts.  Every buffer is heap-allocated at its exact size, so a read
// or write one byte past it -- a name byte past the stream, say -- is an ASan report.  Sorts with
// the summary and once more without, and prints
//   "<status> <bad_row> <fnv1a64 of perm> <n_names> <n_single> <n_pair> <n_more> <max_name> <already>"
// status 0 ok, 1 malformed record (bad_row names it), 3 the call without a summary disagreed.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bam_name_core.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static uint64_t fnv(uint64_t h, const void *p, size_t n) {
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
  return h;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t flat_size = 0, n = 0;
  if (!rd(f, &flat_size, 8)) return 2;
  std::vector<uint8_t> flat(flat_size);
  if (!rd(f, flat.data(), flat_size) || !rd(f, &n, 8)) return 2;
  std::vector<uint64_t> starts(n);
  if (!rd(f, starts.data(), 8 * n)) return 2;
  fclose(f);

  uint64_t bad = 0, bad2 = 0, hp = 0xcbf29ce484222325ull;
  std::vector<uint64_t> perm(n, 0), perm2(n, 0);
  sbh_bam::NameInfo info{};
  int rc = sbh_bam::name_sort_host(flat.data(), flat_size, starts.data(), n, perm.data(), &info, &bad);
  const int rc2 = sbh_bam::name_sort_host(flat.data(), flat_size, starts.data(), n, perm2.data(), nullptr, &bad2);
  if (rc2 != rc || bad2 != bad || (rc == 0 && perm2 != perm)) rc = 3;
  if (rc == 0) hp = fnv(hp, perm.data(), 8 * perm.size());
  printf("%d %" PRIu64 " %016" PRIx64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %d\n", rc, bad, hp, info.n_names,
         info.n_single, info.n_pair, info.n_more, info.max_name, info.already);
  return 0;
}
