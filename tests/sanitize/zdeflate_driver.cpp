// ASan/UBSan driver for the byte-exact writer's host restatement (csrc/zdeflate_core.h): deflates
// every record of the corpus files given on the command line with z_deflate_serial, the source and
// every scratch array allocated at exactly the size the header promises to stay within, and prints
// each stream's size and FNV-1a hash (tests/test_zdeflate_sanitize_cpu.py compares them with
// libz's).  Test infrastructure only.
//
// File format: records of { u32 level, u32 n, n bytes }, little endian, until the end of the file.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

#include "zdeflate_core.h"

using namespace sbh_zlib;

int main(int argc, char **argv) {
  auto st = std::make_unique<ZTreeState>();
  for (int k = 1; k < argc; ++k) {
    std::ifstream f(argv[k], std::ios::binary);
    const std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t o = 0;
    while (o + 8 <= d.size()) {
      uint32_t level, n;
      std::memcpy(&level, &d[o], 4);
      std::memcpy(&n, &d[o + 4], 4);
      o += 8;
      if (n > MAX_MEMBER || o + n > d.size()) {
        std::fprintf(stderr, "%s: bad record at %zu\n", argv[k], o - 8);
        return 2;
      }
      // exact sizes: an access past what the header allows is a heap-buffer-overflow
      const std::vector<uint8_t> src(d.begin() + o, d.begin() + o + n);
      std::vector<uint16_t> prev(n), head(HASH_MASK + 1);
      std::vector<uint32_t> tok(n);
      std::vector<uint64_t> info(n);
      const uint32_t cap = 2 * n + 1024;
      std::vector<uint8_t> out(cap);
      const uint32_t size = z_deflate_serial(src.data(), n, (int)level, out.data(), cap, prev.data(), head.data(),
                                             tok.data(), info.data(), *st);
      if (size > cap) {
        std::fprintf(stderr, "%s: stream of %u bytes does not fit %u\n", argv[k], size, cap);
        return 2;
      }
      uint64_t h = 0xcbf29ce484222325ull;
      for (uint32_t i = 0; i < size; ++i) h = (h ^ out[i]) * 0x100000001b3ull;
      std::printf("%u %016llx\n", size, (unsigned long long)h);
      o += n;
    }
    if (o != d.size()) {
      std::fprintf(stderr, "%s: %zu trailing bytes\n", argv[k], d.size() - o);
      return 2;
    }
  }
  return 0;
}
