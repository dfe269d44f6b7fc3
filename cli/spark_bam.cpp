// spark-bam CLI on MI355X: the reference's commands (cli/.../Main.scala:19-28) over the
// C-ABI in include/sparkbam.h.  Host side in C++ (the reference's Scala/JVM toolchain
// is not part of this build); all byte work runs in libsparkbam_hip.so on the GPU.
//
//   spark-bam compute-splits [-s] [-m SIZE] [-l N] BAM      (ComputeSplits.scala:18-156)
//   spark-bam count-reads   [-s] [-m SIZE] BAM              (compare/CountReads.scala:21-213)
//   spark-bam check-bam -s  [-m SIZE] [-i RANGES] [-r RECORDS] BAM  (check/eager/CheckBam.scala)
//   spark-bam full-check    [-m SIZE] [-i RANGES] [-l N] BAM       (check/full/FullCheck.scala)
//   spark-bam index-blocks  BAM [OUT]                        (bgzf/index/IndexBlocks.scala)
//   spark-bam index-records BAM [OUT]                        (check/index/IndexRecords.scala)
//   spark-bam index-bai     BAM [OUT]                        (the .bai samtools index writes; htslib hts.c)
//   spark-bam view [-h] [-o FILE] BAM                        (the records as SAM text: htsjdk getSAMString)
//   spark-bam view -b -o OUT [-f INT] [-F INT] [-q INT] [-r ROWS] [--level N] [--index-bai] [--sort|--sort-name] BAM
//   spark-bam sort [-N] [-o OUT] [--level N] [--index-bai] BAM [OUT]  (coordinate order, as samtools sort;
//                                                             -N: read-name order, as samtools sort -N)
//                                                            (the records that pass, as a BAM gathered on the GPU)
//   spark-bam check-blocks -s [-r RECORDS] [-l N] BAM        (cli/.../check/blocks/CheckBlocks.scala)
//   spark-bam htsjdk-rewrite [-r READS] [-b] [-i] [--index-bai] BAM OUT  (cli/.../rewrite/HTSJDKRewrite.scala)
//
// The hadoop-bam ("seqdoop", -u) comparisons are out of scope: hadoop-bam's
// BAMSplitGuesser is a competitor's algorithm, not part of spark-bam's path.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../include/sparkbam.h"
#include "../spark-bam_amd/csrc/stats_core.h"  // stats' report (host functions only)
#include "../spark-bam_amd/csrc/tally_core.h"  // flagstat's and idxstats' text (host functions only)
#include "../spark-bam_amd/csrc/fastq_core.h"  // fastq's mode bits, the quality bound and the parts' order

namespace {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

sbh_ctx *g_ctx = nullptr;

void chk(int rc, const char *what) {
  if (rc != SBH_OK) throw Error(rc, std::string(what) + ": " + sbh_last_error(g_ctx));
}

// hammerlab Bytes parser: integers or shorthands (k = 1024, "230k" = 235520)
uint64_t parse_bytes(const std::string &s) {
  size_t i = 0;
  while (i < s.size() && (isdigit((unsigned char)s[i]) || s[i] == '.')) ++i;
  double v = std::stod(s.substr(0, i));
  std::string u = s.substr(i);
  for (auto &c : u) c = (char)tolower(c);
  if (!u.empty() && u.back() == 'b') u.pop_back();
  double m = 1;
  if (u == "k") m = 1024.0;
  else if (u == "m") m = 1024.0 * 1024;
  else if (u == "g") m = 1024.0 * 1024 * 1024;
  else if (u == "t") m = 1024.0 * 1024 * 1024 * 1024;
  else if (!u.empty()) throw Error(SBH_E_ARG, "bad byte size: " + s);
  return (uint64_t)(v * m);
}

// ByteRanges (check/.../args/ByteRanges.scala, Range.scala): a-b | a+len | pos
std::vector<std::pair<uint64_t, uint64_t>> parse_ranges(const std::string &s) {
  std::vector<std::pair<uint64_t, uint64_t>> out;
  size_t p = 0;
  while (p <= s.size()) {
    size_t q = s.find(',', p);
    std::string t = s.substr(p, q == std::string::npos ? std::string::npos : q - p);
    size_t d = t.find('-'), pl = t.find('+');
    if (d != std::string::npos) out.push_back({parse_bytes(t.substr(0, d)), parse_bytes(t.substr(d + 1))});
    else if (pl != std::string::npos) {
      uint64_t a = parse_bytes(t.substr(0, pl));
      out.push_back({a, a + parse_bytes(t.substr(pl + 1))});
    } else {
      uint64_t a = parse_bytes(t);
      out.push_back({a, a + 1});
    }
    if (q == std::string::npos) break;
    p = q + 1;
  }
  return out;
}

std::vector<uint8_t> read_file(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw Error(SBH_E_ARG, "cannot open " + path);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Pos {
  uint64_t block = 0;
  uint32_t off = 0;
  std::string str() const { return std::to_string(block) + ":" + std::to_string(off); }
  double minus(const Pos &o, double ratio = 3.0) const {  // Pos.- (Pos.scala:17-22)
    int64_t v = (int64_t)block - (int64_t)o.block + (int64_t)(((int64_t)off - (int64_t)o.off) / ratio);
    return (double)std::max<int64_t>(0, v);
  }
};

struct BamHeader {
  std::vector<std::string> names;
  std::vector<int32_t> lens;
  uint64_t end = 0;
};

int32_t rd32(const uint8_t *p) { return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24); }

// header.Header.apply (check/.../header/Header.scala:26-60)
BamHeader parse_header(sbh_shard *sh, uint64_t flat_size) {
  uint64_t n = std::min<uint64_t>(flat_size, 1 << 16);
  for (;;) {
    std::vector<uint8_t> b(n);
    chk(sbh_read_flat(sh, 0, n, b.data()), "read header");
    BamHeader h;
    bool ok = n >= 12 && std::memcmp(b.data(), "BAM\1", 4) == 0;
    if (!ok) throw Error(SBH_E_ARG, "not a BAM file");
    uint64_t c = 8 + (uint64_t)rd32(&b[4]);
    bool done = false;
    if (c + 4 <= n) {
      int32_t nref = rd32(&b[c]);
      c += 4;
      done = true;
      for (int32_t i = 0; i < nref; ++i) {
        if (c + 4 > n) { done = false; break; }
        int32_t l = rd32(&b[c]);
        if (c + 8 + (uint64_t)l > n) { done = false; break; }
        h.names.emplace_back((const char *)&b[c + 4], strnlen((const char *)&b[c + 4], l));
        h.lens.push_back(rd32(&b[c + 4 + l]));
        c += 8 + l;
      }
    }
    if (done) { h.end = c; return h; }
    if (n >= flat_size) throw Error(SBH_E_TRUNCATED, "truncated BAM header");
    n = std::min<uint64_t>(flat_size, n * 4);
  }
}

struct Loaded {
  std::vector<uint8_t> data;
  sbh_shard *sh = nullptr;
  uint64_t nblocks = 0, flat = 0;
  BamHeader hdr;
  std::vector<sbh_block> blocks;
  explicit Loaded(const std::string &path) : data(read_file(path)) {
    chk(sbh_shard_create(g_ctx, data.data(), data.size(), 0, data.size(), 0, &sh), "shard");
    chk(sbh_index(sh, 0, &nblocks, &flat), "index");
    chk(sbh_inflate(sh, nullptr), "inflate");
    hdr = parse_header(sh, flat);
    chk(sbh_set_contigs(sh, hdr.lens.data(), (int32_t)hdr.lens.size()), "contigs");
    blocks.resize(nblocks);
    if (nblocks) chk(sbh_get_blocks(sh, 0, nblocks, blocks.data()), "blocks");
  }
  ~Loaded() { sbh_shard_destroy(sh); }
  uint64_t seg_end() const {  // the flat end of the stream's first segment: an empty block ends it
    for (const sbh_block &b : blocks)
      if (b.flags & SBH_BLOCK_EMPTY) return b.ustart;
    return flat;
  }
  Pos pos(uint64_t flat_pos) const {
    Pos p;
    chk(sbh_pos_of(sh, flat_pos, &p.block, &p.off), "pos");
    return p;
  }
};

std::vector<std::pair<uint64_t, uint64_t>> file_splits(uint64_t size, uint64_t split) {
  std::vector<std::pair<uint64_t, uint64_t>> out;
  uint64_t rem = size;
  while ((double)rem / (double)split > 1.1) {
    out.push_back({size - rem, size - rem + split});
    rem -= split;
  }
  if (rem) out.push_back({size - rem, size});
  return out;
}

// hammerlab stats number rendering (as in the reference's golden outputs)
std::string num(double v) {
  char b[64];
  if (std::fabs(v) >= 1e5) {
    snprintf(b, sizeof b, "%.1e", v);
    std::string s(b);
    size_t e = s.find('e');
    std::string mant = s.substr(0, e), ex = s.substr(e + 1);
    int x = std::stoi(ex);
    return mant + "e" + std::to_string(x);
  }
  if (std::fabs(v - std::round(v)) < 1e-9 || std::fabs(v) >= 100) {
    snprintf(b, sizeof b, "%.0f", v);
    return b;
  }
  snprintf(b, sizeof b, "%.1f", v);
  return b;
}

std::string stats_lines(const std::vector<double> &xs) {
  std::string out;
  size_t n = xs.size();
  if (!n) return "(empty)\n";
  double mean = 0;
  for (double x : xs) mean += x;
  mean /= n;
  double var = 0;
  for (double x : xs) var += (x - mean) * (x - mean);
  double sd = std::sqrt(var / n);
  auto median = [](std::vector<double> v) {
    std::sort(v.begin(), v.end());
    size_t m = v.size();
    return m % 2 ? v[m / 2] : (v[m / 2 - 1] + v[m / 2]) / 2;
  };
  double med = median(xs);
  std::vector<double> dev;
  for (double x : xs) dev.push_back(std::fabs(x - med));
  double mad = median(dev);
  out += "N: " + std::to_string(n) + ", μ/σ: " + num(mean) + "/" + num(sd) + ", med/mad: " + num(med) + "/" + num(mad) + "\n";
  std::string el = " elems:", so = "sorted:";
  std::vector<double> s = xs;
  std::sort(s.begin(), s.end());
  for (double x : xs) el += " " + std::to_string((long long)x);
  for (double x : s) so += " " + std::to_string((long long)x);
  out += el + "\n" + so + "\n";
  return out;
}

// hammerlab Bytes.format: 583K, 25.6K, 1.2M ...
std::string bytes_fmt(uint64_t b) {
  const char *u[] = {"B", "K", "M", "G", "T"};
  double v = (double)b;
  int i = 0;
  while (v >= 1024 && i < 4) { v /= 1024; ++i; }
  char buf[64];
  if (i == 0) snprintf(buf, sizeof buf, "%lluB", (unsigned long long)b);
  else if (v >= 100) snprintf(buf, sizeof buf, "%.0f%s", std::floor(v + 0.5 - 1e-9), u[i]);
  else snprintf(buf, sizeof buf, "%.1f%s", v, u[i]);
  return buf;
}

struct Args {
  std::string cmd, path, out, records, blocks_path;
  uint64_t split = 0;
  bool has_split = false, s = false, u = false;
  long limit = 1000000;
  std::vector<std::pair<uint64_t, uint64_t>> ranges;
  bool has_ranges = false;
  int reads_to_check = 10, max_read_size = 100000000, blocks_to_check = 5;
  // htsjdk-rewrite: -r record-index ranges (IntRanges), -b / -i / --index-bai write OUT.blocks /
  // OUT.records / OUT.bai
  std::vector<std::pair<uint64_t, uint64_t>> read_ranges;
  bool has_read_ranges = false, idx_blocks = false, idx_records = false, idx_bai = false;
  bool sam_header = false;  // view -h: the BAM header text first
  // view -b: BAM output of the records with (flag & -f) == -f, (flag & -F) == 0, mapq >= -q and an
  // index in -r (read_ranges); --level as sbh_bgzf_compress_level; --index-bai (idx_bai) writes OUT.bai
  // view -b --sort, sort: the kept records in coordinate order (sbh_records_bam_scan_order), SO:coordinate
  // view -b --sort-name, sort -N: in read-name order (sbh_records_bam_scan_names), SO:queryname; no --index-bai
  bool bam_out = false, sort = false, sort_name = false;
  uint32_t flag_require = 0, flag_exclude = 0;
  int min_mapq = 0, level = SBH_LEVEL_HTSJDK;
  // depth: -a every position of the spans, -r REGION, -J D ops cover, --bedgraph; -F defaults to 1796
  bool depth_all = false, count_del = false, bedgraph = false, has_exclude = false;
  std::string region;
  // pileup, consensus: -a / -r / -f / -F / -q as depth's, -H a header line, -Q the least base quality a
  // letter needs, -d / -c consensus's least depth and percentage, --max-positions the accumulator's budget
  bool pile_header = false;
  int min_baseq = 0, min_depth = 1, call_pct = 75;
  long long max_positions = -1;  // (-1: sbh_pileup_budget's)
  bool count_only = false;  // view -c: the number of records that pass -f / -F / -q, nothing else
  // fastq, fasta: -1 / -2 / -0 the sinks of read 1, read 2 and the others (any of them: the output is split),
  // -n no /1 /2 suffixes, -N always, -v the quality of a record without qualities; -F defaults to 0x900;
  // --level, or a sink ending in .gz: BGZF members compressed from device memory
  std::string out_part[3];
  bool suffix_never = false, suffix_always = false, has_level = false;
  int def_qual = 1;
  long stat_cycles = 1024, stat_insert = 8000;  // stats: --cycles, -i
};

// decimal or 0x hex
long parse_int(const std::string &s) {
  size_t used = 0;
  long v = 0;
  try {
    v = std::stol(s, &used, 0);
  } catch (const std::exception &) {
    used = 0;
  }
  if (!used || used != s.size()) throw Error(SBH_E_ARG, "bad integer: " + s);
  return v;
}

// The record commands: which of the shared options each takes, whether it rejects a dash-option it does
// not know, and the synopsis that the rejection shows.
enum : unsigned { O_FILTER = 1, O_OUT = 2, O_REGION = 4, O_LEVEL = 8, O_BAI = 16 };  // -f -F -q | -o | -r REGION | --level | --index-bai
struct Command {
  const char *name;
  unsigned opts;
  bool strict;
  const char *synopsis;
};
const char *const TALLY_SYNOPSIS = "[-f INT] [-F INT] [-q INT] [-o FILE] <bam>";
const char *const FASTQ_SYNOPSIS = "[-o FILE] [-1 FILE] [-2 FILE] [-0 FILE] [-n|-N] [-f INT] [-F INT] [-q INT] [-v INT] [--level N] <bam>";
const Command COMMANDS[] = {
    {"view", O_FILTER | O_OUT | O_LEVEL | O_BAI, false, nullptr},
    {"sort", O_OUT | O_LEVEL | O_BAI, false, nullptr},
    {"htsjdk-rewrite", O_BAI, false, nullptr},
    {"depth", O_FILTER | O_OUT | O_REGION, false, nullptr},
    {"pileup", O_FILTER | O_OUT | O_REGION, true, "[-a] [-H] [-r REGION] [-f INT] [-F INT] [-q INT] [-Q INT] [-o FILE] <bam>"},
    {"consensus", O_FILTER | O_OUT | O_REGION, true, "[-r REGION] [-f INT] [-F INT] [-q INT] [-Q INT] [-d MIN_DEPTH] [-c PCT] [-o FILE] <bam>"},
    {"flagstat", O_FILTER | O_OUT, true, TALLY_SYNOPSIS},
    {"idxstats", O_FILTER | O_OUT, true, TALLY_SYNOPSIS},
    {"stats", O_FILTER | O_OUT, true, "[-f INT] [-F INT] [-q INT] [--cycles N] [-i MAX_INSERT] [-o FILE] <bam>"},
    {"fastq", O_FILTER | O_OUT | O_LEVEL, true, FASTQ_SYNOPSIS},
    {"fasta", O_FILTER | O_OUT | O_LEVEL, true, FASTQ_SYNOPSIS},
};

Args parse(int argc, char **argv) {
  Args a;
  if (argc < 2)
    throw Error(SBH_E_ARG,
                "usage: spark-bam <command> [options] <bam>\n"
                "  commands: compute-splits count-reads check-bam full-check index-blocks index-records index-bai\n"
                "            check-blocks htsjdk-rewrite view sort depth pileup consensus flagstat idxstats stats fastq\n"
                "            fasta\n"
                "  view [-h|--header] [-o FILE] <bam>: the records as SAM text (-h: the header text first)\n"
                "  view -b -o OUT [-f INT] [-F INT] [-q INT] [-r ROWS] [--level N] [--index-bai] [--sort|--sort-name] <bam>:\n"
                "       the records with\n"
                "       (flag & f) == f, (flag & F) == 0, mapq >= q and an index in ROWS (a-b,c-d: htsjdk-rewrite's -r)\n"
                "       as a BAM at deflate level N (5: htsjdk's bytes; -1: the fast coder); --index-bai writes OUT.bai;\n"
                "       --sort: in coordinate order (reference, position, strand; unplaced last), header SO:coordinate\n"
                "       --sort-name: in read-name order (bytes of the name, a prefix first; then read 1, read 2; primary,\n"
                "       secondary, supplementary), header SO:queryname; not with --index-bai (a BAI needs coordinate order)\n"
                "  sort [-N] [-o OUT] [--level N] [--index-bai] <bam> [OUT]: every record, coordinate-sorted on the GPU;\n"
                "       -N: sorted by read name instead (samtools sort -N's byte order), not with --index-bai\n"
                "  depth [-a] [-r REGION] [-f INT] [-F INT] [-q INT] [-J] [--bedgraph] [-o FILE] <bam>: per-base depth as\n"
                "       RNAME POS DEPTH lines (samtools depth; -a: zero-depth positions too) or, with --bedgraph, RNAME BEG END\n"
                "       DEPTH runs (genomecov -bg); REGION is NAME or NAME:BEG-END (1-based, inclusive); -F defaults to 1796;\n"
                "       -J: deletions count\n"
                "  pileup [-a] [-H] [-r REGION] [-f INT] [-F INT] [-q INT] [-Q INT] [-o FILE] <bam>: per-base allele counts as\n"
                "       NAME POS A C G T N DEL INS LOWQ lines (POS 1-based) for every position any kept read touches (-a: every\n"
                "       position of the region; -H: a header line first); -Q: bases of lower quality count as LOWQ (0; samtools\n"
                "       mpileup's is 13); -F defaults to 1796; 33 bytes of device memory per position: without -r a genome that\n"
                "       does not fit is refused (--max-positions N overrides the budget)\n"
                "  consensus [-r REGION] [-f INT] [-F INT] [-q INT] [-Q INT] [-d MIN_DEPTH] [-c PCT] [-o FILE] <bam>: FASTA of the\n"
                "       base at least PCT percent (75) of at least MIN_DEPTH (1) reads agree on, N elsewhere, deletions dropped\n"
                "  flagstat [-f INT] [-F INT] [-q INT] [-o FILE] <bam>: samtools flagstat's sixteen lines of the records that pass\n"
                "  idxstats [-f INT] [-F INT] [-q INT] [-o FILE] <bam>: NAME LENGTH MAPPED UNMAPPED per reference, then the `*` line\n"
                "       (samtools idxstats), counted from the records: no index is read, any order will do\n"
                "  stats [-f INT] [-F INT] [-q INT] [--cycles N] [-i MAX_INSERT] [-o FILE] <bam>: the read-level sections of samtools\n"
                "       stats (SN, FFQ, LFQ, GCF, GCL, GCC, IS, RL, MAPQ) of the records that pass: read lengths, qualities and bases\n"
                "       per cycle (N rows, 1024; longer reads share a last row), GC content, insert sizes (up to MAX_INSERT, 8000)\n"
                "  view -c [-f INT] [-F INT] [-q INT] <bam>: how many records pass (samtools view -c)\n"
                "  fastq [-o FILE] [-1 FILE] [-2 FILE] [-0 FILE] [-n|-N] [-f INT] [-F INT] [-q INT] [-v INT] [--level N] <bam>:\n"
                "       the records as FASTQ (samtools fastq): @NAME[/1|/2], bases, +, qualities; reverse-strand reads\n"
                "       reverse-complemented; -1 / -2 / -0: read 1, read 2 and the others to their own files (a class without\n"
                "       one goes to -o, or nowhere); -n: no /1 /2 suffixes, -N: always; -v: the quality of reads without\n"
                "       qualities (1); -F defaults to 0x900; --level N, or a FILE ending in .gz: BGZF-compressed on the GPU\n"
                "  fasta: the same flags, >NAME and the bases only (samtools fasta)");
  a.cmd = argv[1];
  static const Command plain{"", 0, false, nullptr};
  const Command *c = &plain;
  for (const Command &k : COMMANDS)
    if (a.cmd == k.name) c = &k;
  const bool view = a.cmd == "view", rewrite = a.cmd == "htsjdk-rewrite", tally = a.cmd == "flagstat" || a.cmd == "idxstats";
  const bool fq = a.cmd == "fastq" || a.cmd == "fasta", pile = a.cmd == "pileup" || a.cmd == "consensus";
  std::vector<std::string> pos;
  for (int i = 2; i < argc; ++i) {
    std::string t = argv[i];
    auto next = [&]() -> std::string {
      if (i + 1 >= argc) throw Error(SBH_E_ARG, "missing value for " + t);
      return argv[++i];
    };
    auto is = [&](unsigned opt, const char *brief, const char *full) { return (c->opts & opt) && (t == brief || t == full); };
    // the shared options, where the command's row has them
    if (is(O_FILTER, "-f", "--require-flags")) a.flag_require = (uint32_t)parse_int(next());
    else if (is(O_FILTER, "-F", "--exclude-flags")) { a.flag_exclude = (uint32_t)parse_int(next()); a.has_exclude = true; }
    else if (is(O_FILTER, "-q", "--min-mapq")) a.min_mapq = (int)parse_int(next());
    else if (is(O_OUT, "-o", "--output")) a.out = next();
    else if (is(O_REGION, "-r", "--region")) a.region = next();
    else if (is(O_LEVEL, "-l", "--level")) { a.level = (int)parse_int(next()); a.has_level = true; }
    else if (is(O_BAI, "--index-bai", "--index-bai")) a.idx_bai = true;
    // each command's own
    else if ((rewrite || view) && (t == "-r" || t == "--read-ranges")) { a.read_ranges = parse_ranges(next()); a.has_read_ranges = true; }
    else if (rewrite && (t == "-b" || t == "--index-blocks")) a.idx_blocks = true;
    else if (rewrite && (t == "-i" || t == "--index-records")) a.idx_records = true;
    else if (view && (t == "-h" || t == "--header")) a.sam_header = true;
    else if (view && (t == "-b" || t == "--bam")) a.bam_out = true;
    else if (view && t == "--sort") a.sort = true;
    else if (view && t == "--sort-name") a.sort_name = true;
    else if (a.cmd == "sort" && t == "-N") a.sort_name = true;
    else if (view && (t == "-c" || t == "--count")) a.count_only = true;
    else if (a.cmd == "stats" && t == "--cycles") a.stat_cycles = parse_int(next());
    else if (a.cmd == "stats" && (t == "-i" || t == "--insert-size")) a.stat_insert = parse_int(next());
    else if (fq && t == "-1") a.out_part[0] = next();
    else if (fq && t == "-2") a.out_part[1] = next();
    else if (fq && t == "-0") a.out_part[2] = next();
    else if (fq && t == "-n") a.suffix_never = true;
    else if (fq && t == "-N") a.suffix_always = true;
    else if (fq && t == "-v") a.def_qual = (int)parse_int(next());
    else if ((a.cmd == "depth" || a.cmd == "pileup") && t == "-a") a.depth_all = true;
    else if (a.cmd == "depth" && t == "-J") a.count_del = true;
    else if (a.cmd == "depth" && t == "--bedgraph") a.bedgraph = true;
    else if (a.cmd == "pileup" && t == "-H") a.pile_header = true;
    else if (pile && (t == "-Q" || t == "--min-baseq")) a.min_baseq = (int)parse_int(next());
    else if (a.cmd == "consensus" && t == "-d") a.min_depth = (int)parse_int(next());
    else if (a.cmd == "consensus" && t == "-c") a.call_pct = (int)parse_int(next());
    else if (pile && t == "--max-positions") a.max_positions = parse_int(next());
    else if (c->strict && t.size() > 1 && t[0] == '-')
      throw Error(SBH_E_ARG, "usage: " + a.cmd + " " + c->synopsis + " (unknown option " + t + ")");
    // the reference's commands' options, wherever no row above claims the letter
    else if (t == "-m" || t == "--max-split-size") { a.split = parse_bytes(next()); a.has_split = true; }
    else if (t == "-s" || t == "--spark-bam") a.s = true;
    else if (t == "-u" || t == "--upstream" || t == "--hadoop-bam") a.u = true;
    else if (t == "-l" || t == "--print-limit") a.limit = std::stol(next());
    else if (t == "-i" || t == "--intervals") { a.ranges = parse_ranges(next()); a.has_ranges = true; }
    else if (t == "-r" || t == "--records-path") a.records = next();
    else if (t == "-b" || t == "--blocks-path") a.blocks_path = next();
    else if (t == "--reads-to-check") a.reads_to_check = std::stoi(next());
    else if (t == "--max-read-size") a.max_read_size = std::stoi(next());
    else if (t == "-z" || t == "--bgzf-blocks-to-check") a.blocks_to_check = std::stoi(next());
    else if (t == "-w" || t == "--warn") {}
    else pos.push_back(t);
  }
  if (pos.empty()) throw Error(SBH_E_ARG, "missing BAM path");
  a.path = pos[0];
  if (a.count_only) {
    if (a.bam_out || a.sam_header || a.has_read_ranges || a.idx_bai || a.sort || a.sort_name || !a.out.empty() || pos.size() != 1 ||
        (pos[0].size() > 1 && pos[0][0] == '-'))
      throw Error(SBH_E_ARG, "usage: view -c [-f INT] [-F INT] [-q INT] <bam>");
  }
  if (pos.size() > 1 && a.cmd != "depth" && a.cmd != "stats" && !tally && !fq && !pile) a.out = pos[1];
  if (fq && !a.has_exclude) a.flag_exclude = 0x900;  // SECONDARY, SUPPLEMENTARY: samtools fastq's
  if (fq && a.suffix_never && a.suffix_always) throw Error(SBH_E_ARG, "usage: " + a.cmd + " takes -n or -N, not both");
  if ((a.cmd == "depth" || pile) && !a.has_exclude) a.flag_exclude = 1796;  // UNMAP, SECONDARY, QCFAIL, DUP: samtools depth's
  if (a.sort && a.sort_name) throw Error(SBH_E_ARG, "usage: view -b takes --sort or --sort-name, not both");
  if (a.sort_name && a.idx_bai)
    throw Error(SBH_E_ARG, std::string(a.cmd == "sort" ? "sort -N" : "view --sort-name") +
                               " with --index-bai: a BAI indexes by position and needs coordinate order, not read-name order");
  if (a.cmd == "sort") {
    a.bam_out = true;
    a.sort = !a.sort_name;
    if (a.out.empty()) throw Error(SBH_E_ARG, "usage: sort needs -o OUT (a BAM is not written to the terminal)");
  }
  if (a.cmd == "view" && a.bam_out && a.out.empty())
    throw Error(SBH_E_ARG, "usage: view -b needs -o OUT (a BAM is not written to the terminal)");
  return a;
}

// The frame of the record commands: the eager calls and the record scan over the records of the
// stream's first segment, the -f / -F / -q filter, an accumulator's handle, and the sink.

// The eager calls over the records; false: the file has none, and nothing ran.
bool eager_calls(Loaded &L, const Args &a) {
  const uint64_t end = L.seg_end();
  if (end <= L.hdr.end) return false;
  uint64_t n = 0;
  chk(sbh_check_eager(L.sh, L.hdr.end, end, a.reads_to_check, nullptr, &n), "eager");
  return true;
}

// eager_calls, then sbh_records_scan -- over no records too when `always` (view -b: its gather then
// finds the scan of no rows); false: the file has no records.
bool scan_records(Loaded &L, const Args &a, bool always = false) {
  const bool any = eager_calls(L, a);
  sbh_records_sizes rs{};
  if (any || always) chk(sbh_records_scan(L.sh, L.hdr.end, L.seg_end(), &rs), "records scan");
  return any;
}

sbh_record_filter filter_of(const Args &a) {
  sbh_record_filter f{};
  f.flag_require = a.flag_require;
  f.flag_exclude = a.flag_exclude;
  f.min_mapq = a.min_mapq;
  return f;
}

template <class T, int (*Destroy)(T *)>
struct Owned {  // a library handle, destroyed on the way out
  T *p = nullptr;
  ~Owned() { Destroy(p); }
};

// -o FILE, or the terminal.  Text gathers in `text` and goes out whenever 1 MiB of it has (spill) and
// at the end (close), which throws when any write fell short.
struct Sink {
  std::string path, text;  // (path "": the terminal)
  FILE *f;
  bool ok = true;
  explicit Sink(const std::string &p) : path(p), f(p.empty() ? stdout : fopen(p.c_str(), "wb")) {
    if (!f) throw Error(SBH_E_ARG, "cannot write " + path);
  }
  Sink(const Sink &) = delete;
  ~Sink() {
    if (f && f != stdout) fclose(f);
  }
  void write(const void *p, size_t n) { ok = ok && fwrite(p, 1, n, f) == n; }
  void spill(bool all = false) {
    if (all || text.size() >= (1u << 20)) {
      write(text.data(), text.size());
      text.clear();
    }
  }
  void close() {
    spill(true);
    ok = ok && fflush(f) == 0;
    if (f != stdout) fclose(f);
    f = nullptr;
    if (!ok) throw Error(SBH_E_ARG, "short write to " + (path.empty() ? std::string("stdout") : path));
  }
};

// a command's whole output at once
void write_out(const std::string &path, const void *p, size_t n) {
  Sink out(path);
  out.write(p, n);
  out.close();
}

void no_hadoop_bam() {
  throw Error(SBH_E_ARG, "hadoop-bam (seqdoop) comparison is not part of the MI355X build; use -s");
}

struct SplitsResult {
  std::vector<std::pair<Pos, Pos>> splits;
  std::vector<uint64_t> counts;
};

SplitsResult splits_from(const std::vector<std::pair<uint64_t, uint64_t>> &sp, const std::vector<uint64_t> &v,
                         const std::vector<uint64_t> &cnt, const std::vector<int32_t> &status, uint64_t file_size) {
  SplitsResult r;
  std::vector<Pos> firsts;
  for (uint64_t i = 0; i < sp.size(); ++i) {
    if (status[i]) throw Error(status[i], "split " + std::to_string(sp[i].first) + "-" + std::to_string(sp[i].second));
    r.counts.push_back(cnt[i]);
    if (cnt[i]) firsts.push_back(Pos{v[i] >> 16, (uint32_t)(v[i] & 0xffff)});
  }
  for (size_t i = 0; i < firsts.size(); ++i)
    r.splits.push_back({firsts[i], i + 1 < firsts.size() ? firsts[i + 1] : Pos{file_size, 0}});
  return r;
}

// CanLoadBam.loadSplitsAndReads (load/.../CanLoadBam.scala:268-302)
SplitsResult spark_bam_splits(Loaded &L, const Args &a, uint64_t split_size) {
  // every split in one batch: FindBlockStart + FindRecordStart + counts on the device
  const auto sp = file_splits(L.data.size(), split_size);
  const uint64_t n = sp.size();
  std::vector<uint64_t> st(n), en(n), v(n), cnt(n);
  std::vector<int32_t> status(n);
  for (uint64_t i = 0; i < n; ++i) st[i] = sp[i].first, en[i] = sp[i].second;
  chk(sbh_split_starts(L.sh, st.data(), en.data(), n, a.blocks_to_check, a.reads_to_check, a.max_read_size,
                       v.data(), cnt.data(), status.data(), nullptr),
      "splits");
  return splits_from(sp, v, cnt, status, L.data.size());
}

uint64_t default_split(const Args &a) { return a.has_split ? a.split : 32ull << 20; }

// A file larger than this many compressed bytes (SBH_RESIDENT_MAX, default 24 GiB) is not held
// resident: it is memory-mapped and streamed through HBM in windows cut at split starts
// (sbh_run_stream2), each split decided in its window -- the same per-split answer in bounded
// HBM, as the reference bounds its memory per split (SplitRDD.scala:33-52, Stream.scala:80-122).
uint64_t resident_max() {
  const char *e = std::getenv("SBH_RESIDENT_MAX");
  return e && *e ? std::strtoull(e, nullptr, 10) : 24ull << 30;
}

struct Mapped {  // read-only mapping of a whole file
  const uint8_t *p = nullptr;
  uint64_t n = 0;
  explicit Mapped(const std::string &path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) throw Error(SBH_E_ARG, "cannot open " + path);
    struct stat st;
    if (fstat(fd, &st) != 0) {
      close(fd);
      throw Error(SBH_E_ARG, "cannot stat " + path);
    }
    n = (uint64_t)st.st_size;
    void *m = n ? mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
    close(fd);
    if (n && m == MAP_FAILED) throw Error(SBH_E_ARG, "cannot map " + path);
    p = static_cast<const uint8_t *>(m);
  }
  ~Mapped() {
    if (p) munmap(const_cast<uint8_t *>(p), n);
  }
};

// Header(path) from the file's leading bytes (grown x4 until the header fits)
BamHeader header_of(const uint8_t *data, uint64_t size) {
  for (uint64_t m = std::min<uint64_t>(size, 1 << 20);; m = std::min<uint64_t>(size, m * 4)) {
    sbh_shard *sh = nullptr;
    chk(sbh_shard_create(g_ctx, data, m, 0, size, 0, &sh), "shard");
    uint64_t nb = 0, flat = 0;
    int rc = sbh_index(sh, 0, &nb, &flat);
    if (!rc) rc = sbh_inflate(sh, nullptr);
    try {
      if (rc) throw Error(rc, "header blocks");
      BamHeader h = parse_header(sh, flat);
      sbh_shard_destroy(sh);
      return h;
    } catch (const Error &) {
      sbh_shard_destroy(sh);
      if (m >= size) throw;
    }
  }
}

// loadSplitsAndReads over a file streamed through HBM (sbh_run_stream2 with every split)
SplitsResult spark_bam_splits_streamed(const std::string &path, const Args &a, uint64_t split_size) {
  Mapped f(path);
  const BamHeader h = header_of(f.p, f.n);
  const auto sp = file_splits(f.n, split_size);
  const uint64_t n = sp.size();
  std::vector<uint64_t> st(n), en(n), v(n), cnt(n);
  std::vector<int32_t> status(n);
  for (uint64_t i = 0; i < n; ++i) st[i] = sp[i].first, en[i] = sp[i].second;
  sbh_stream_opts o{};
  o.window = 1ull << 30;
  o.halo = 4ull << 20;
  o.reads_to_check = a.reads_to_check;
  o.max_read_size = a.max_read_size;
  o.bgzf_blocks_to_check = a.blocks_to_check;
  o.split_start = st.data(), o.split_end = en.data(), o.n_splits = n;
  o.split_first_vpos = v.data(), o.split_count = cnt.data(), o.split_status = status.data();
  sbh_stream_result res;
  chk(sbh_run_stream2(g_ctx, f.p, f.n, 0, f.n, UINT64_MAX, f.n, h.lens.data(), (int32_t)h.lens.size(), &o, &res),
      "stream");
  return splits_from(sp, v, cnt, status, f.n);
}

// the resident path for files that fit, the streamed one otherwise
SplitsResult spark_bam_splits_any(const Args &a, uint64_t split_size) {
  struct stat st;
  if (stat(a.path.c_str(), &st) == 0 && (uint64_t)st.st_size > resident_max())
    return spark_bam_splits_streamed(a.path, a, split_size);
  Loaded L(a.path);
  return spark_bam_splits(L, a, split_size);
}

int compute_splits(const Args &a) {
  if (a.u && !a.s) no_hadoop_bam();
  auto t0 = std::chrono::steady_clock::now();
  SplitsResult r = spark_bam_splits_any(a, default_split(a));
  long ms = (long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
  printf("Get spark-bam splits: %ldms\n\n", ms);
  std::vector<double> lens;
  for (auto &s : r.splits) lens.push_back((double)(int64_t)s.second.minus(s.first));
  printf("Split-size distribution:\n%s\n", stats_lines(lens).c_str());
  size_t n = r.splits.size();
  if ((long)n <= a.limit) printf("%zu splits:\n", n);
  else printf("First %ld of %zu splits:\n", a.limit, n);
  for (size_t i = 0; i < n && (long)i < a.limit; ++i)
    printf("\t%s-%s\n", r.splits[i].first.str().c_str(), r.splits[i].second.str().c_str());
  if ((long)n > a.limit) printf("\t…\n");
  printf("\n");
  return 0;
}

int count_reads(const Args &a) {
  auto t0 = std::chrono::steady_clock::now();
  SplitsResult r = spark_bam_splits_any(a, default_split(a));
  uint64_t total = 0;
  for (uint64_t c : r.counts) total += c;
  long ms = (long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
  printf("spark-bam read-count time: %ld\n\n", ms);
  printf("spark-bam found %llu reads, hadoop-bam threw exception:\n", (unsigned long long)total);
  printf("\thadoop-bam is not part of the MI355X build\n");
  return 0;
}

std::vector<Pos> read_records_file(const std::string &p) {
  std::ifstream f(p);
  if (!f) throw Error(SBH_E_ARG, "no records file " + p + " (run index-records first)");
  std::vector<Pos> out;
  std::string line;
  while (std::getline(f, line)) {
    size_t c = line.find(',');
    if (c == std::string::npos) continue;
    out.push_back(Pos{std::stoull(line.substr(0, c)), (uint32_t)std::stoul(line.substr(c + 1))});
  }
  return out;
}

// Set bits of an LSB-first bitmap as positions base + i (64 positions per step).
std::vector<uint64_t> bits_to_positions(const std::vector<uint8_t> &bits, uint64_t base, uint64_t n) {
  std::vector<uint64_t> out;
  for (uint64_t i = 0; i < n; i += 64) {
    uint64_t w = 0;
    std::memcpy(&w, bits.data() + i / 8, std::min<uint64_t>(8, bits.size() - i / 8));
    if (n - i < 64) w &= (1ull << (n - i)) - 1;
    for (; w; w &= w - 1) out.push_back(base + i + (uint64_t)__builtin_ctzll(w));
  }
  return out;
}

// Blocks.apply (check/src/main/scala/org/hammerlab/bam/check/Blocks.scala:47-208): the blocks the
// all-positions modes examine, per partition.  With a `.blocks` file (-b, default BAM.blocks): its
// blocks whose start is in -i, partitioned by cumulative compressed size / split size (:86-139);
// without one: the file cut every split size, the splits meeting -i, each one's blocks found on
// the device (FindBlockStart, then MetadataStream while start < split end: sbh_find_blocks,
// :141-206).  The split size is -m, default 2 MB (:74-78).
struct BlockMeta {
  uint64_t start;
  uint32_t csize, usize;
};
struct BlocksPartitions {
  std::vector<std::vector<BlockMeta>> parts;
  std::vector<std::pair<uint64_t, uint64_t>> bounds;
  std::vector<uint64_t> starts() const {
    std::vector<uint64_t> v;
    for (auto &p : parts)
      for (auto &m : p) v.push_back(m.start);
    return v;
  }
};

bool in_ranges(const Args &a, uint64_t x) {
  if (!a.has_ranges) return true;
  for (auto &r : a.ranges)
    if (r.first <= x && x < r.second) return true;
  return false;
}

BlocksPartitions blocks_apply(const Args &a, const uint8_t *data, uint64_t size) {
  const uint64_t split = a.has_split ? a.split : 2ull << 20;
  const std::string bp = a.blocks_path.empty() ? a.path + ".blocks" : a.blocks_path;
  BlocksPartitions R;
  std::ifstream f(bp);
  if (f) {
    std::vector<BlockMeta> metas;
    std::string line;
    while (std::getline(f, line)) {
      if (line.empty()) continue;
      const size_t c1 = line.find(','), c2 = c1 == std::string::npos ? c1 : line.find(',', c1 + 1);
      if (c2 == std::string::npos) throw Error(SBH_E_ARG, "Bad blocks-index line: " + line);
      BlockMeta m{std::stoull(line.substr(0, c1)), (uint32_t)std::stoul(line.substr(c1 + 1, c2 - c1 - 1)),
                  (uint32_t)std::stoul(line.substr(c2 + 1))};
      if (in_ranges(a, m.start)) metas.push_back(m);
    }
    // partition = (compressed bytes of the blocks before it) / split; the partition count is the last
    // block's partition + 1 (as BlocksTest's "block boundaries" case pins it)
    uint64_t off = 0;
    for (auto &m : metas) {
      const uint64_t k = off / split;
      if (R.parts.size() <= k) R.parts.resize(k + 1);
      R.parts[k].push_back(m);
      off += m.csize;
    }
    for (uint64_t i = 0; i < R.parts.size(); ++i) R.bounds.push_back({i * split, (i + 1) * split});
    return R;
  }
  std::vector<uint64_t> idx, st, en;
  for (uint64_t i = 0; i * split < size; ++i) {
    bool meets = !a.has_ranges;
    for (auto &r : a.ranges) meets |= r.first < r.second && r.first < (i + 1) * split && r.second > i * split;
    if (!meets) continue;
    idx.push_back(i);
    st.push_back(i * split);
    en.push_back(std::min(size, (i + 1) * split));
    R.bounds.push_back({i * split, (i + 1) * split});
  }
  R.parts.resize(idx.size());
  std::vector<sbh_block> out(size / 16384 + 4096);  // BAM blocks average 15-25 KB; regrown if short
  uint64_t n = 0;
  for (;;) {
    chk(sbh_find_blocks(g_ctx, data, size, st.data(), en.data(), st.size(), a.blocks_to_check, 1ull << 30, out.data(),
                        out.size(), &n),
        "find blocks");
    if (n <= out.size()) break;
    out.resize(n);
  }
  for (uint64_t i = 0; i < n; ++i)
    if (in_ranges(a, out[i].start)) R.parts[out[i].ustart].push_back(BlockMeta{out[i].start, out[i].csize, out[i].usize});
  return R;
}

uint64_t stream_window() {
  const char *e = std::getenv("SBH_STREAM_WINDOW");
  return e && *e ? std::strtoull(e, nullptr, 10) : 1ull << 30;
}

// The file's record at/after a vpos, for PosMetadata (a few KB of the file around it inflated on
// the device; grown x4 while the search needs more bytes).
struct NextRecord {
  bool found = false;
  int32_t delta = 0, ref = 0, pos = 0, lseq = 0;
  uint32_t flag = 0;
  std::string name;
};
NextRecord next_record(const uint8_t *data, uint64_t size, const BamHeader &h, const Args &a, uint64_t vpos) {
  NextRecord r;
  const uint64_t blk = vpos >> 16;
  for (uint64_t span = 4ull << 20;; span *= 4) {
    const uint64_t n = std::min(size - blk, span);
    sbh_shard *sh = nullptr;
    chk(sbh_shard_create(g_ctx, data + blk, n, blk, size, 0, &sh), "shard");
    uint64_t nb = 0, flat = 0, nxt = 0;
    int rc = sbh_index(sh, blk, &nb, &flat);
    if (!rc) rc = sbh_inflate(sh, nullptr);
    if (!rc) rc = sbh_set_contigs(sh, h.lens.data(), (int32_t)h.lens.size());
    if (!rc) rc = sbh_find_record_start(sh, vpos & 0xffff, a.reads_to_check, a.max_read_size, &nxt, &r.delta);
    if (rc == SBH_E_NEED_HALO && blk + n < size) {
      sbh_shard_destroy(sh);
      continue;
    }
    if (!rc && nxt + 36 <= flat) {
      uint8_t f[36];
      chk(sbh_read_flat(sh, nxt, 36, f), "read record");
      r.ref = rd32(f + 4), r.pos = rd32(f + 8), r.lseq = rd32(f + 20);
      const uint32_t rnl = (uint32_t)rd32(f + 12) & 0xff;
      r.flag = (uint32_t)rd32(f + 16) >> 16;
      std::vector<uint8_t> name(rnl ? rnl : 1, 0);
      if (rnl && nxt + 36 + rnl <= flat) chk(sbh_read_flat(sh, nxt + 36, rnl, name.data()), "read name");
      r.name.assign((const char *)name.data(), strnlen((const char *)name.data(), rnl));
      r.found = true;
    }
    sbh_shard_destroy(sh);
    return r;
  }
}

// check-bam -s and full-check's pass over Blocks.apply's blocks: sbh_check_stream moves the file
// through HBM in windows, so any file size runs in bounded HBM.
struct AllPositions {
  sbh_check_result res{};
  std::vector<uint64_t> fp, fn, close_v, counts, rbe;
  std::vector<uint32_t> close_w;
};
AllPositions all_positions(const Args &a, const Mapped &f, const BamHeader &h, const std::vector<uint64_t> *truth,
                           bool full, uint64_t cap) {
  const BlocksPartitions B = blocks_apply(a, f.p, f.n);
  const std::vector<uint64_t> starts = B.starts();
  AllPositions R;
  sbh_check_opts o{};
  o.window = stream_window();
  o.halo = 4ull << 20;
  o.reads_to_check = a.reads_to_check;
  o.blocks = starts.data();
  o.n_blocks = starts.size();
  if (truth) {
    R.fp.resize(cap + 1);
    R.fn.resize(cap + 1);
    o.truth_vpos = truth->data();
    o.n_truth = truth->size();
    o.fp_vpos = R.fp.data(), o.fn_vpos = R.fn.data();
    o.fp_cap = o.fn_cap = cap;
  }
  if (full) {
    const uint64_t ccap = 1 << 22;
    R.counts.resize(21 * 19);
    R.rbe.resize(21 * 64);
    R.close_v.resize(ccap);
    R.close_w.resize(ccap);
    o.full = 1;
    o.counts = R.counts.data(), o.rbe_hist = R.rbe.data();
    o.close_vpos = R.close_v.data(), o.close_word = R.close_w.data(), o.close_cap = ccap;
  }
  chk(sbh_check_stream(g_ctx, f.p, f.n, h.lens.data(), (int32_t)h.lens.size(), &o, &R.res), "check");
  R.fp.resize(std::min<uint64_t>(R.res.fp, cap));
  R.fn.resize(std::min<uint64_t>(R.res.fn, cap));
  if (full) {
    R.close_v.resize(std::min<uint64_t>(R.res.n_close, R.close_v.size()));
    R.close_w.resize(R.close_v.size());
  }
  return R;
}

Pos pos_of_vpos(uint64_t v) { return Pos{v >> 16, (uint32_t)(v & 0xffff)}; }

// CheckerApp's summary (CheckerApp.scala:150-227) of the eager calls vs the `.records` truth
void print_check_summary(const Args &a, const AllPositions &R) {
  const uint64_t tp = R.res.tp, fp = R.res.fp, fn = R.res.fn, positions = R.res.positions, comp = R.res.comp_bytes;
  if (R.res.unknown)
    throw Error(SBH_E_NOT_FOUND, std::to_string(R.res.unknown) + " records-file positions are not block starts");
  printf("%llu uncompressed positions\n%s compressed\nCompression ratio: %.2f\n%llu reads\n",
         (unsigned long long)positions, bytes_fmt(comp).c_str(), (double)positions / (double)comp,
         (unsigned long long)(tp + fn));
  if (!fp && !fn) {
    printf("All calls matched!\n");
    return;
  }
  printf("%llu false positives, %llu false negatives\n\n", (unsigned long long)fp, (unsigned long long)fn);
  if (fp) {
    printf("False positives:\n");
    for (uint64_t v : R.fp) printf("\t%s\n", pos_of_vpos(v).str().c_str());
  }
  if (fn) {
    printf("%llu false negatives:\n", (unsigned long long)fn);
    for (uint64_t v : R.fn) printf("\t%s\n", pos_of_vpos(v).str().c_str());
  }
}

std::vector<uint64_t> truth_of(const Args &a) {
  std::vector<Pos> recs = read_records_file(a.records.empty() ? a.path + ".records" : a.records);
  std::vector<uint64_t> truth(recs.size());
  for (size_t i = 0; i < recs.size(); ++i) truth[i] = recs[i].block << 16 | recs[i].off;
  std::sort(truth.begin(), truth.end());
  return truth;
}

int check_bam(const Args &a) {
  if (!a.s) no_hadoop_bam();
  Mapped f(a.path);
  const BamHeader h = header_of(f.p, f.n);
  const std::vector<uint64_t> truth = truth_of(a);
  const AllPositions R = all_positions(a, f, h, &truth, false, (uint64_t)std::max(a.limit, 0L));
  print_check_summary(a, R);
  return 0;
}

const char *FLAG_NAMES[19] = {
    "tooFewFixedBlockBytes", "negativeReadIdx", "tooLargeReadIdx", "negativeReadPos", "tooLargeReadPos",
    "negativeNextReadIdx", "tooLargeNextReadIdx", "negativeNextReadPos", "tooLargeNextReadPos",
    "tooFewBytesForReadName", "nonNullTerminatedReadName", "nonASCIIReadName", "noReadName", "emptyReadName",
    "tooFewBytesForCigarOps", "invalidCigarOp", "emptyMappedCigar", "emptyMappedSeq",
    "tooFewRemainingBytesImplied"};

std::string flags_str(uint32_t w) {
  std::string s;
  for (int i = 0; i < 19; ++i)
    if (w & (1u << i)) s += (s.empty() ? "" : ",") + std::string(FLAG_NAMES[i]);
  return s;
}

// PosMetadata show (check/.../PosMetadata.scala:20-53) with htsjdk SAMRecord.toString
std::string pos_metadata(const Mapped &f, const BamHeader &h, const Args &a, uint64_t vpos, uint32_t word) {
  std::string rec = "no next record";
  const NextRecord r = next_record(f.p, f.n, h, a, vpos);
  if (r.found) {
    std::string s = std::to_string(r.delta) + " before " + r.name;
    if (r.flag & 1) s += (r.flag & 0x40) ? " 1/2" : " 2/2";
    s += " " + std::to_string(r.lseq) + "b";
    const bool unmapped = r.flag & 4;
    s += unmapped ? " unmapped read" : " aligned read";
    auto where = [&]() { return h.names[r.ref] + ":" + std::to_string(r.pos + 1); };
    if (unmapped && r.pos + 1 >= 0 && r.ref >= 0 && r.ref < (int32_t)h.names.size()) s += " (placed at " + where() + ")";
    else if (!unmapped && r.ref >= 0 && r.ref < (int32_t)h.names.size()) s += " @ " + where();
    rec = s;
  }
  return pos_of_vpos(vpos).str() + ":\t" + rec + ". Failing checks: " + flags_str(word & SBH_FULL_FLAGS_MASK);
}

std::vector<std::string> counts_lines(const std::vector<uint64_t> &c, const std::map<uint32_t, uint64_t> &rbe,
                                      bool include_zeros, bool hide_first) {
  std::vector<std::pair<std::string, uint64_t>> kv;
  for (int i = 0; i < 19; ++i) kv.push_back({FLAG_NAMES[i], c[i]});
  std::stable_sort(kv.begin(), kv.end(), [](auto &x, auto &y) { return x.second > y.second; });
  std::vector<std::pair<std::string, std::string>> pairs;
  for (auto &p : kv) {
    if ((p.second > 0 || include_zeros) && (p.first != "tooFewFixedBlockBytes" || !hide_first))
      pairs.push_back({p.first, std::to_string(p.second)});
  }
  if (!rbe.empty()) {
    std::string v;
    for (auto &r : rbe) v += (v.empty() ? "" : " ") + std::to_string(r.first) + "ⅹ" + std::to_string(r.second);
    pairs.push_back({"readsBeforeError", v});
  }
  size_t mk = 0, mv = 0;
  for (auto &p : pairs) { mk = std::max(mk, p.first.size()); mv = std::max(mv, p.second.size()); }
  std::vector<std::string> out;
  for (auto &p : pairs)
    out.push_back(std::string(mk - p.first.size(), ' ') + p.first + ":\t" + std::string(mv - p.second.size(), ' ') + p.second);
  return out;
}

int full_check(const Args &a) {
  Mapped f(a.path);
  const BamHeader h = header_of(f.p, f.n);
  // records file, if present: the indexed comparison summary first (FullCheck.scala:94-106), from
  // the same pass over the blocks
  const std::string rp = a.records.empty() ? a.path + ".records" : a.records;
  const bool have_records = (bool)std::ifstream(rp);
  std::vector<uint64_t> truth;
  if (have_records) {
    Args e = a;
    e.records = rp;
    truth = truth_of(e);
  }
  const AllPositions R = all_positions(a, f, h, have_records ? &truth : nullptr, true, (uint64_t)std::max(a.limit, 0L));
  if (have_records) {
    print_check_summary(a, R);
    printf("\n");
  }
  const std::vector<uint64_t> &counts = R.counts, &rbe = R.rbe;
  std::vector<std::pair<uint64_t, uint32_t>> close;
  for (size_t i = 0; i < R.close_v.size(); ++i) close.push_back({R.close_v[i], R.close_w[i]});
  auto nnz_of = [](uint32_t w) { return __builtin_popcount(w & SBH_FULL_FLAGS_MASK) + (((w >> SBH_FULL_N_SHIFT) & 0x3FF) > 0); };
  auto per = [&](int k) {
    std::vector<uint64_t> c(19);
    for (int i = 0; i < 19; ++i) c[i] = counts[k * 19 + i];
    std::map<uint32_t, uint64_t> r;
    for (int j = 1; j < 64; ++j)
      if (rbe[k * 64 + j]) r[j] = rbe[k * 64 + j];
    return std::make_pair(c, r);
  };
  std::vector<std::pair<uint64_t, uint32_t>> ones, twos;
  for (auto &c : close) (nnz_of(c.second) == 1 ? ones : twos).push_back(c);
  if (ones.empty()) {
    printf("No positions where only one check failed\n");
  } else {
    auto pc = per(1);
    printf("Critical error counts (true negatives where only one check failed):\n");
    for (auto &l : counts_lines(pc.first, pc.second, false, false)) printf("\t%s\n", l.c_str());
    printf("\n");
    if ((long)ones.size() <= a.limit) printf("%zu critical positions:\n", ones.size());
    else printf("%ld of %zu critical positions:\n", a.limit, ones.size());
    for (size_t i = 0; i < ones.size() && (long)i < a.limit; ++i)
      printf("\t%s\n", pos_metadata(f, h, a, ones[i].first, ones[i].second).c_str());
    if ((long)ones.size() > a.limit) printf("\t…\n");
  }
  printf("\n");
  if (twos.empty()) {
    printf("No positions where exactly two checks failed\n\n");
  } else {
    if ((long)twos.size() <= a.limit) printf("%zu positions where exactly two checks failed:\n", twos.size());
    else printf("%ld of %zu positions where exactly two checks failed:\n", a.limit, twos.size());
    for (size_t i = 0; i < twos.size() && (long)i < a.limit; ++i)
      printf("\t%s\n", pos_metadata(f, h, a, twos[i].first, twos[i].second).c_str());
    if ((long)twos.size() > a.limit) printf("\t…\n");
    printf("\n");
    std::map<uint32_t, uint64_t> hist;
    for (auto &t : twos) hist[t.second & SBH_FULL_FLAGS_MASK]++;
    std::vector<std::pair<uint64_t, uint32_t>> h;
    for (auto &x : hist) h.push_back({x.second, x.first});
    std::stable_sort(h.begin(), h.end(), [](auto &x, auto &y) { return x.first > y.first; });
    if (h.front().first > 1) {
      printf("\tHistogram:\n");
      for (size_t i = 0; i < h.size() && (long)i < a.limit; ++i)
        printf("\t\t%llu:\t%s\n", (unsigned long long)h[i].first, flags_str(h[i].second).c_str());
      printf("\n");
    }
    auto pc = per(2);
    printf("\tPer-flag totals:\n");
    for (auto &l : counts_lines(pc.first, pc.second, false, false)) printf("\t\t%s\n", l.c_str());
    printf("\n");
  }
  std::vector<uint64_t> tot(19, 0);
  std::map<uint32_t, uint64_t> trbe;
  for (int k = 0; k < 21; ++k) {
    for (int i = 0; i < 19; ++i) tot[i] += counts[k * 19 + i];
    for (int j = 1; j < 64; ++j)
      if (rbe[k * 64 + j]) trbe[j] += rbe[k * 64 + j];
  }
  printf("Total error counts:\n");
  for (auto &l : counts_lines(tot, trbe, true, true)) printf("\t%s\n", l.c_str());
  printf("\n");
  return 0;
}

int index_blocks(const Args &a) {
  Loaded L(a.path);
  std::string out = a.out.empty() ? a.path + ".blocks" : a.out;
  FILE *f = fopen(out.c_str(), "w");
  if (!f) throw Error(SBH_E_ARG, "cannot write " + out);
  for (const sbh_block &b : L.blocks) {
    if (b.flags & SBH_BLOCK_EMPTY) break;  // MetadataStream ends at the first empty block
    fprintf(f, "%llu,%u,%u\n", (unsigned long long)b.start, b.csize, b.usize);
  }
  fclose(f);
  return 0;
}

int index_records(const Args &a) {
  Loaded L(a.path);
  const uint64_t seg_end = L.seg_end();
  std::vector<uint8_t> bits((seg_end - L.hdr.end + 7) / 8);
  uint64_t n = 0, chain = 0;
  chk(sbh_check_eager(L.sh, L.hdr.end, seg_end, a.reads_to_check, bits.data(), &n), "eager");
  chk(sbh_count_records(L.sh, L.hdr.end, seg_end, &chain), "records");
  if (chain != n) throw Error(SBH_E_STATE, "record chain and eager calls disagree; refusing to write .records");
  std::string out = a.out.empty() ? a.path + ".records" : a.out;
  FILE *f = fopen(out.c_str(), "w");
  if (!f) throw Error(SBH_E_ARG, "cannot write " + out);
  for (uint64_t p : bits_to_positions(bits, L.hdr.end, seg_end - L.hdr.end)) {
    Pos q = L.pos(p);
    fprintf(f, "%llu,%u\n", (unsigned long long)q.block, q.off);
  }
  fclose(f);
  return 0;
}

// The .bai of a coordinate-sorted BAM (what samtools index writes), whole file resident: the
// eager calls give the record starts in parallel, sbh_bai_scan turns the records into runs of
// equal (ref_id, bin) and linear-index minima on the device, sbh_bai_build finishes on the host.
int index_bai(const Args &a) {
  Loaded L(a.path);
  eager_calls(L, a);
  sbh_bai_sizes sz{};
  chk(sbh_bai_scan(L.sh, L.hdr.end, L.seg_end(), &sz), "bai scan");
  std::vector<sbh_bai_run> runs(sz.n_runs);
  std::vector<uint64_t> lin(sz.lin_size);
  chk(sbh_bai_fetch(L.sh, runs.data(), lin.data()), "bai fetch");
  const int32_t n_ref = (int32_t)L.hdr.lens.size();
  std::vector<uint8_t> bai(sbh_bai_bound(sz.n_runs, sz.lin_size, n_ref));
  uint64_t size = 0;
  const int rc = sbh_bai_build(runs.data(), runs.size(), lin.data(), L.hdr.lens.data(), n_ref, sz.n_no_coor, bai.data(),
                               bai.size(), &size);
  if (rc) throw Error(rc, "bai build failed (status " + std::to_string(rc) + ")");
  write_out(a.out.empty() ? a.path + ".bai" : a.out, bai.data(), size);
  return 0;
}

// The records as SAM text (one line per record, htsjdk SAMRecord.getSAMString), whole file
// resident as index-bai holds it: the eager calls give the record starts, sbh_records_scan
// decodes from the header's end, sbh_records_sam_scan renders on the device, the fetch brings the
// text back.  -h: the BAM header text (the l_text bytes after the magic) first, verbatim.
int view_bam(const Args &a);

int tally(const Args &a);

int view(const Args &a) {
  if (a.count_only) return tally(a);
  if (a.bam_out) return view_bam(a);
  if (a.has_read_ranges || a.flag_require || a.flag_exclude || a.min_mapq || a.idx_bai || a.sort || a.sort_name)
    throw Error(SBH_E_ARG, "view: -f / -F / -q / -r / --index-bai / --sort / --sort-name select records for BAM output: they need -b");
  Loaded L(a.path);
  std::vector<char> text;
  uint64_t head = 0;
  if (a.sam_header) {
    uint8_t lt[4];
    chk(sbh_read_flat(L.sh, 4, 4, lt), "read header");
    const int32_t l_text = rd32(lt);
    if (l_text < 0 || 8 + (uint64_t)l_text > L.hdr.end) throw Error(SBH_E_ARG, "bad BAM header text length");
    head = (uint64_t)l_text;
    text.resize(head);
    if (head) chk(sbh_read_flat(L.sh, 8, head, (uint8_t *)text.data()), "read header text");
  }
  if (scan_records(L, a)) {
    std::string names;
    std::vector<uint64_t> off(1, 0);
    for (const std::string &s : L.hdr.names) {
      names += s;
      off.push_back(names.size());
    }
    sbh_sam_sizes sz{};
    chk(sbh_records_sam_scan(L.sh, names.data(), off.data(), (int32_t)L.hdr.names.size(), &sz), "sam scan");
    text.resize(head + sz.text_bytes);
    chk(sbh_records_sam_fetch(L.sh, text.data() + head, nullptr), "sam fetch");
  }
  write_out(a.out, text.data(), text.size());
  return 0;
}

// view -b: the records that pass the filters as a BAM, whole file resident.  The records are
// selected and laid out behind the header on the device (sbh_records_bam_scan) and compressed
// from device memory: only the header and the finished file cross to the host.
int view_bam(const Args &a) {
  if (a.out.empty()) throw Error(SBH_E_ARG, "usage: view -b needs -o OUT (a BAM is not written to the terminal)");
  std::vector<uint8_t> out;
  uint64_t size = 0, nb = 0;
  {
    Loaded L(a.path);
    std::vector<uint8_t> head(L.hdr.end);
    if (L.hdr.end) chk(sbh_read_flat(L.sh, 0, L.hdr.end, head.data()), "read header");
    if (a.sort || a.sort_name) {
      std::vector<uint8_t> so(head.size() + 64);
      uint64_t so_n = 0;
      chk(sbh_bam_header_set_so(head.data(), head.size(), a.sort_name ? "queryname" : "coordinate", so.data(), so.size(), &so_n),
          "header SO");
      so.resize(so_n);
      head.swap(so);
    }
    scan_records(L, a, true);
    // -r as given -> sorted, disjoint ranges
    std::vector<std::pair<uint64_t, uint64_t>> rr = a.read_ranges;
    std::sort(rr.begin(), rr.end());
    std::vector<uint64_t> rb, re;
    for (auto &r : rr) {
      if (!re.empty() && r.first <= re.back()) re.back() = std::max(re.back(), r.second);
      else { rb.push_back(r.first); re.push_back(r.second); }
    }
    sbh_record_filter f = filter_of(a);
    f.row_begin = rb.data();
    f.row_end = re.data();
    f.n_row_ranges = rb.size();
    sbh_bam_sizes bs{};
    if (a.sort_name)
      chk(sbh_records_bam_scan_names(L.sh, head.data(), head.size(), &f, &bs), "bam scan");
    else
      chk(sbh_records_bam_scan_order(L.sh, head.data(), head.size(), &f, a.sort ? SBH_ORDER_COORDINATE : SBH_ORDER_SCAN, &bs),
          "bam scan");
    out.resize(sbh_bgzf_compress_bound(bs.bytes));
    chk(sbh_bgzf_compress_level(g_ctx, sbh_records_bam_device_ptr(L.sh), bs.bytes, 1, a.level, out.data(), out.size(), &size,
                                &nb, nullptr),
        "bgzf compress");
  }
  write_out(a.out, out.data(), size);
  if (a.idx_bai) {
    Args ix = a;
    ix.path = a.out;
    ix.out.clear();
    index_bai(ix);
  }
  return 0;
}

// The spans of -r REGION over the file's references: a reference name, or NAME:BEG-END with 1-based
// inclusive positions; none: every reference whole.  cmd names the command in the error messages.
template <class Header>
std::vector<sbh_depth_span> region_spans(const Header &hdr, const std::string &region, const std::string &cmd) {
  const int32_t n_ref = (int32_t)hdr.lens.size();
  std::vector<sbh_depth_span> spans;
  if (region.empty()) {
    for (int32_t k = 0; k < n_ref; ++k)
      if (hdr.lens[k] > 0) spans.push_back(sbh_depth_span{k, 0, 0, hdr.lens[k]});
    return spans;
  }
  auto find = [&](const std::string &name) {
    for (int32_t k = 0; k < n_ref; ++k)
      if (hdr.names[k] == name) return k;
    return (int32_t)-1;
  };
  int32_t k = find(region);
  int64_t beg = 0, end = k >= 0 ? hdr.lens[k] : 0;
  if (k < 0) {
    const size_t c = region.rfind(':'), d = c == std::string::npos ? c : region.find('-', c);
    auto digits = [](const std::string &t) { return !t.empty() && t.size() < 11 && t.find_first_not_of("0123456789") == std::string::npos; };
    if (c == std::string::npos || d == std::string::npos || (k = find(region.substr(0, c))) < 0 ||
        !digits(region.substr(c + 1, d - c - 1)) || !digits(region.substr(d + 1)))
      throw Error(SBH_E_ARG, cmd + ": unknown reference in region " + region);
    beg = std::stoll(region.substr(c + 1, d - c - 1)) - 1;
    end = std::min<int64_t>(std::stoll(region.substr(d + 1)), hdr.lens[k]);
  }
  if (beg < 0 || beg >= end) throw Error(SBH_E_ARG, cmd + ": empty region " + region);
  spans.push_back(sbh_depth_span{k, 0, beg, end});
  return spans;
}

// depth: per-base depth of the records that pass the filters, whole file resident as view holds
// it.  The records are scanned, their CIGARs walked and the depth scanned into runs on the device
// (sbh_records_depth_add, sbh_depth_finish); the runs come back and are printed here -- samtools
// depth's lines (RNAME, 1-based POS, DEPTH; zero depth only with -a) or, with --bedgraph,
// genomecov -bg's (RNAME, 0-based BEG, END, DEPTH; depth > 0 only).  REGION: a reference name, or
// NAME:BEG-END with 1-based inclusive positions; none: every reference whole.
int depth(const Args &a) {
  Loaded L(a.path);
  const int32_t n_ref = (int32_t)L.hdr.lens.size();
  const std::vector<sbh_depth_span> spans = region_spans(L.hdr, a.region, "depth");
  Owned<sbh_depth, sbh_depth_destroy> acc;
  chk(sbh_depth_create(g_ctx, spans.data(), (uint32_t)spans.size(), n_ref, a.count_del ? SBH_DEPTH_DEL : 0u, &acc.p),
      "depth create");
  if (scan_records(L, a)) {
    const sbh_record_filter f = filter_of(a);
    sbh_depth_add_result ar{};
    chk(sbh_records_depth_add(L.sh, acc.p, &f, &ar), "depth add");
  }
  sbh_depth_sizes sz{};
  chk(sbh_depth_finish(acc.p, &sz), "depth finish");
  std::vector<sbh_depth_run> runs(sz.n_runs);
  chk(sbh_depth_runs_fetch(acc.p, 0, sz.n_runs, runs.data()), "depth runs");
  Sink out(a.out);
  std::string &text = out.text;
  for (const sbh_depth_run &r : runs) {
    if (!r.depth && !(a.depth_all && !a.bedgraph)) continue;
    const std::string &name = L.hdr.names[r.ref_id];
    if (a.bedgraph) {
      text += name + "\t" + std::to_string(r.beg) + "\t" + std::to_string(r.end) + "\t" + std::to_string(r.depth) + "\n";
    } else {
      const std::string tail = "\t" + std::to_string(r.depth) + "\n";
      for (int64_t p = r.beg + 1; p <= r.end; ++p) {
        text += name;
        text += '\t';
        text += std::to_string(p);
        text += tail;
        out.spill();
      }
    }
  }
  out.close();
  return 0;
}

// pileup, consensus: per-base allele counts of the records that pass the filters, whole file resident
// as depth holds it.  The records are scanned and their CIGARs, bases and qualities walked into eight
// counters per position on the device (sbh_records_pileup_add); the finish leaves a call byte per
// position and the intervals any kept read touches (sbh_pileup_finish).  pileup prints the counters of
// the intervals' positions (-a: of every position), consensus the call bytes as FASTA.
int pileup(const Args &a) {
  Loaded L(a.path);
  const int32_t n_ref = (int32_t)L.hdr.lens.size();
  const std::vector<sbh_depth_span> spans = region_spans(L.hdr, a.region, a.cmd);
  uint64_t positions = 0, budget = 0;
  for (const sbh_depth_span &s : spans) positions += (uint64_t)(s.end - s.beg);
  if (a.max_positions >= 0) budget = (uint64_t)a.max_positions;
  else chk(sbh_pileup_budget(g_ctx, &budget), "pileup budget");
  if (positions > budget)
    throw Error(SBH_E_ARG, a.cmd + ": " + std::to_string(positions) + " positions at 33 bytes each do not fit the device memory budget of " +
                               std::to_string(budget) + " positions: give a region with -r");
  Owned<sbh_pileup, sbh_pileup_destroy> acc;
  chk(sbh_pileup_create(g_ctx, spans.data(), (uint32_t)spans.size(), n_ref, a.min_baseq, &acc.p), "pileup create");
  if (scan_records(L, a)) {
    const sbh_record_filter f = filter_of(a);
    sbh_pileup_add_result ar{};
    chk(sbh_records_pileup_add(L.sh, acc.p, &f, &ar), "pileup add");
  }
  sbh_pileup_sizes sz{};
  chk(sbh_pileup_finish(acc.p, (uint32_t)std::max(a.min_depth, 0), (uint32_t)std::max(a.call_pct, 0), &sz), "pileup finish");
  Sink out(a.out);
  std::string &text = out.text;
  constexpr uint64_t CHUNK = 1 << 16;  // positions fetched at a time
  if (a.cmd == "consensus") {
    std::vector<uint8_t> calls(CHUNK);
    for (uint32_t k = 0; k < spans.size(); ++k) {
      const sbh_depth_span &s = spans[k];
      const std::string &name = L.hdr.names[s.ref_id];
      text += ">" + name;
      if (s.beg != 0 || s.end != L.hdr.lens[s.ref_id]) text += ":" + std::to_string(s.beg + 1) + "-" + std::to_string(s.end);
      text += '\n';
      uint64_t col = 0;
      for (uint64_t from = 0, len = (uint64_t)(s.end - s.beg); from < len; from += CHUNK) {
        const uint64_t m = std::min(CHUNK, len - from);
        chk(sbh_pileup_calls_fetch(acc.p, k, from, m, calls.data()), "pileup calls");
        for (uint64_t i = 0; i < m; ++i) {
          if (calls[i] == '*') continue;
          text += calls[i] ? (char)calls[i] : 'N';
          if (++col == 60) text += '\n', col = 0;
        }
        out.spill();
      }
      if (col) text += '\n';
    }
  } else {
    if (a.pile_header) text += "#chrom\tpos\tA\tC\tG\tT\tN\tdel\tins\tlowq\n";
    std::vector<sbh_depth_span> ivals(sz.n_intervals);
    chk(sbh_pileup_intervals_fetch(acc.p, 0, sz.n_intervals, ivals.data()), "pileup intervals");
    std::vector<uint32_t> counts(8 * CHUNK);
    size_t iv = 0;
    for (uint32_t k = 0; k < spans.size(); ++k) {
      const sbh_depth_span &s = spans[k];
      const std::string &name = L.hdr.names[s.ref_id];
      // the stretches to print: the span, or its intervals (they come in span and position order)
      std::vector<std::pair<int64_t, int64_t>> cut;
      if (a.depth_all) cut.emplace_back(s.beg, s.end);
      for (; iv < ivals.size() && ivals[iv].ref_id == s.ref_id; ++iv)
        if (!a.depth_all) cut.emplace_back(ivals[iv].beg, ivals[iv].end);
      for (const auto &c : cut)
        for (int64_t x = c.first; x < c.second; x += (int64_t)CHUNK) {
          const uint64_t m = std::min<uint64_t>(CHUNK, (uint64_t)(c.second - x));
          chk(sbh_pileup_counts_fetch(acc.p, k, (uint64_t)(x - s.beg), m, counts.data()), "pileup counts");
          for (uint64_t i = 0; i < m; ++i) {
            text += name;
            text += '\t';
            text += std::to_string(x + (int64_t)i + 1);
            for (int ch = 0; ch < 8; ++ch) {
              text += '\t';
              text += std::to_string(counts[8 * i + ch]);
            }
            text += '\n';
            out.spill();
          }
        }
    }
  }
  out.close();
  return 0;
}

// flagstat, idxstats, view -c: one pass over the records that pass -f / -F / -q, whole file resident as
// depth holds it, counted on the device (sbh_records_tally_add); the counts come back and are printed
// here by tally_core.h's renderers -- samtools flagstat's sixteen lines, samtools idxstats' line per
// reference and its `*` line, or (view -c) the number of records kept.
int tally(const Args &a) {
  Loaded L(a.path);
  const int32_t n_ref = (int32_t)L.hdr.lens.size();
  Owned<sbh_tally, sbh_tally_destroy> acc;
  chk(sbh_tally_create(g_ctx, n_ref, &acc.p), "tally create");
  sbh_tally_add_result ar{};
  if (scan_records(L, a)) {
    const sbh_record_filter f = filter_of(a);
    chk(sbh_records_tally_add(L.sh, acc.p, &f, &ar), "tally add");
  }
  std::vector<uint64_t> flag(2 * SBH_TALLY_ROWS), ref(2 * ((size_t)n_ref + 1));
  chk(sbh_tally_fetch(acc.p, flag.data(), 0, (uint64_t)n_ref + 1, ref.data()), "tally fetch");
  std::string text;
  if (a.count_only) text = std::to_string(ar.n_kept) + "\n";
  else if (a.cmd == "flagstat") text = sbh_tal::flagstat_text(flag.data());
  else text = sbh_tal::idxstats_text(ref.data(), L.hdr.names.data(), L.hdr.lens.data(), n_ref);
  write_out(a.out, text.data(), text.size());
  return 0;
}

// stats: one pass over the records that pass -f / -F / -q, whole file resident as depth holds it,
// counted on the device (sbh_records_stats_add); the tables come back and stats_core.h's renderer
// prints them.
int stats(const Args &a) {
  if (a.stat_cycles < 1 || a.stat_cycles > (long)sbh_stat::STAT_CYCLES_MAX || a.stat_insert < 1 || a.stat_insert > (long)sbh_stat::STAT_INSERT_MAX)
    throw Error(SBH_E_ARG, "stats: --cycles takes 1.." + std::to_string(sbh_stat::STAT_CYCLES_MAX) + ", -i 1.." + std::to_string(sbh_stat::STAT_INSERT_MAX));
  Loaded L(a.path);
  Owned<sbh_stats, sbh_stats_destroy> acc;
  const sbh_stats_params prm{(uint32_t)a.stat_cycles, (uint32_t)a.stat_insert};
  chk(sbh_stats_create(g_ctx, &prm, &acc.p), "stats create");
  if (scan_records(L, a)) {
    const sbh_record_filter f = filter_of(a);
    sbh_stats_add_result ar{};
    chk(sbh_records_stats_add(L.sh, acc.p, &f, &ar), "stats add");
  }
  const sbh_stat::Params P{prm.cycles, prm.max_insert};
  const sbh_stat::Layout lay = sbh_stat::layout_of(P);
  std::vector<uint64_t> w(lay.words);
  const sbh_stat::Tables T{w.data(), w.data() + lay.read_len, w.data() + lay.qual, w.data() + lay.base, w.data() + lay.gc,
                           w.data() + lay.isize, w.data() + lay.mapq};
  chk(sbh_stats_fetch(acc.p, T.sn, T.read_len, T.qual, T.base, T.gc, T.isize, T.mapq), "stats fetch");
  const std::string text = sbh_stat::stats_text(P, T);
  write_out(a.out, text.data(), text.size());
  return 0;
}

// fastq, fasta: the records that pass -f / -F / -q as FASTQ or FASTA text, whole file resident as depth
// holds it, rendered on the device (sbh_records_fastq_scan).  One sink (-o, or the terminal) takes the
// text in file order; with any of -1 / -2 / -0 the text comes in three parts -- read 1, read 2, the
// others -- and each part goes to its own sink, to -o without one, or nowhere.  A sink ending in
// .gz, and every sink with --level, receives BGZF members compressed from device memory.
int fastq(const Args &a) {
  static_assert(SBH_FASTQ_SPLIT == sbh_fq::MODE_SPLIT && SBH_FASTQ_FASTA == sbh_fq::MODE_FASTA, "fastq_core.h restates the header's bits");
  if (a.def_qual < 0 || a.def_qual > sbh_fq::QUAL_MAX) throw Error(SBH_E_ARG, a.cmd + ": -v takes 0.." + std::to_string(sbh_fq::QUAL_MAX));
  const bool split = !a.out_part[0].empty() || !a.out_part[1].empty() || !a.out_part[2].empty();
  const uint32_t mode = (a.cmd == "fasta" ? SBH_FASTQ_FASTA : 0u) | (split ? SBH_FASTQ_SPLIT : 0u) |
                        (a.suffix_always ? SBH_FASTQ_SUFFIX_ALWAYS : a.suffix_never ? 0u : SBH_FASTQ_SUFFIX);
  Loaded L(a.path);
  sbh_fastq_sizes sz{};
  if (scan_records(L, a)) {
    const sbh_record_filter f = filter_of(a);
    chk(sbh_records_fastq_scan(L.sh, &f, mode, a.def_qual, &sz), "fastq scan");
  }
  // the sink of each part (a path; "": the terminal), a sink named twice opened once
  struct PartSink {
    std::string path;
    FILE *f = nullptr;
    bool gz = false;
  };
  std::vector<PartSink> sinks;
  int of_part[sbh_fq::PARTS] = {-1, -1, -1};
  auto sink_of = [&](const std::string &path) {
    for (size_t k = 0; k < sinks.size(); ++k)
      if (sinks[k].path == path) return (int)k;
    PartSink s;
    s.path = path;
    s.gz = a.has_level || (path.size() > 3 && path.compare(path.size() - 3, 3, ".gz") == 0);
    s.f = path.empty() ? stdout : fopen(path.c_str(), "wb");
    if (!s.f) throw Error(SBH_E_ARG, "cannot write " + path);
    sinks.push_back(s);
    return (int)sinks.size() - 1;
  };
  if (!split) of_part[0] = sink_of(a.out);
  else
    for (uint32_t p = 0; p < sbh_fq::PARTS; ++p)
      if (!a.out_part[p].empty()) of_part[p] = sink_of(a.out_part[p]);
      else if (!a.out.empty()) of_part[p] = sink_of(a.out);
  const char *dev = (const char *)sbh_records_fastq_device_ptr(L.sh);
  std::vector<char> text;
  bool plain = false;
  for (uint32_t p = 0; p < sbh_fq::PARTS; ++p) plain |= of_part[p] >= 0 && !sinks[of_part[p]].gz && sz.part_bytes[p];
  if (plain) {
    text.resize(sz.text_bytes);
    chk(sbh_records_fastq_fetch(L.sh, text.data(), nullptr, nullptr), "fastq fetch");
  }
  bool ok = true;
  uint64_t at = 0;
  std::vector<uint8_t> comp;
  for (uint32_t p = 0; p < sbh_fq::PARTS; ++p) {
    const uint64_t nb = sz.part_bytes[p];
    if (nb && of_part[p] >= 0) {
      PartSink &s = sinks[of_part[p]];
      if (!s.gz) {
        ok = ok && fwrite(text.data() + at, 1, nb, s.f) == nb;
      } else {
        comp.resize(sbh_bgzf_compress_bound(nb));
        uint64_t size = 0, members = 0;
        chk(sbh_bgzf_compress_level(g_ctx, dev + at, nb, 1, a.level, comp.data(), comp.size(), &size, &members, nullptr),
            "bgzf compress");
        ok = ok && size >= 28 && fwrite(comp.data(), 1, size - 28, s.f) == size - 28;  // (its EOF member comes once, below)
      }
    }
    at += nb;
  }
  static const uint8_t eof_member[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (PartSink &s : sinks) {
    if (s.gz) ok = ok && fwrite(eof_member, 1, 28, s.f) == 28;
    ok = ok && fflush(s.f) == 0;
    if (s.f != stdout) fclose(s.f);
  }
  if (!ok) throw Error(SBH_E_ARG, "short write");
  return 0;
}

// HTSJDKRewrite (cli/.../rewrite/HTSJDKRewrite.scala:40-92): the BAM's uncompressed stream --
// header, then every record, or only the records whose index is in -r (:48-58) -- re-cut into
// 65498-byte BGZF members on the GPU (sbh_bgzf_compress) plus the EOF member; -b / -i then
// index the output like IndexBlocks / IndexRecords (:72-90).  Records pass through byte for
// byte (htsjdk's decode/re-encode is the identity on a BAM it wrote), and each member is
// deflated exactly as htsjdk's Deflater(5) does (zlib 1.2.11 deflate_slow, include/sparkbam.h),
// so the output and its .blocks / .records equal htsjdk's (HTSJDKRewriteTest's dirMatch).
int htsjdk_rewrite(const Args &a) {
  if (a.out.empty()) throw Error(SBH_E_ARG, "htsjdk-rewrite: missing output path");
  std::vector<uint8_t> payload;
  {
    Loaded L(a.path);
    const uint64_t seg_end = L.seg_end();
    std::vector<uint8_t> flat(seg_end);
    if (seg_end) chk(sbh_read_flat(L.sh, 0, seg_end, flat.data()), "read stream");
    if (!a.has_read_ranges) {
      payload.swap(flat);
    } else {
      // record starts: the eager calls over the records, proven equal to the record chain
      std::vector<uint8_t> bits((seg_end - L.hdr.end + 7) / 8);
      uint64_t n = 0, chain = 0;
      chk(sbh_check_eager(L.sh, L.hdr.end, seg_end, a.reads_to_check, bits.data(), &n), "eager");
      chk(sbh_count_records(L.sh, L.hdr.end, seg_end, &chain), "records");
      if (chain != n) throw Error(SBH_E_STATE, "record chain and eager calls disagree");
      const std::vector<uint64_t> st = bits_to_positions(bits, L.hdr.end, seg_end - L.hdr.end);
      payload.assign(flat.begin(), flat.begin() + (ptrdiff_t)L.hdr.end);
      for (uint64_t i = 0; i < st.size(); ++i) {
        bool in = false;
        for (auto &r : a.read_ranges) in |= r.first <= i && i < r.second;
        if (!in) continue;
        const uint64_t e = i + 1 < st.size() ? st[i + 1] : seg_end;
        payload.insert(payload.end(), flat.begin() + (ptrdiff_t)st[i], flat.begin() + (ptrdiff_t)e);
      }
    }
  }
  std::vector<uint8_t> out(sbh_bgzf_compress_bound(payload.size()));
  uint64_t size = 0, nb = 0;
  chk(sbh_bgzf_compress(g_ctx, payload.data(), payload.size(), 0, out.data(), out.size(), &size, &nb, nullptr),
      "bgzf compress");
  write_out(a.out, out.data(), size);
  Args ix = a;
  ix.path = a.out;
  ix.out.clear();
  if (a.idx_blocks) index_blocks(ix);
  if (a.idx_records) index_records(ix);
  if (a.idx_bai) index_bai(ix);
  return 0;
}

// hammerlab Stats.fromHist rendered with the truncating Show[Double] CheckBlocks installs
// (CheckBlocks.scala:123-131): N, mean / population sigma, median / MAD, the histogram's
// first and last 10 runs ("v" or "v×n", "…" between), and the percentiles whose
// interpolation index (N + 1) p - 1 lies inside [0, N - 1].
std::string stats_hist(const std::map<long long, uint64_t> &hist) {
  std::vector<double> v;
  for (auto &kv : hist) v.insert(v.end(), kv.second, (double)kv.first);
  const size_t n = v.size();
  if (!n) return "(empty)\n";
  auto rnd = [](double x) { return std::to_string((long long)std::floor(x + 0.5)); };
  auto pct = [&](const std::vector<double> &s, double p) {  // s sorted
    const double idx = (double)(s.size() + 1) * p - 1;
    const size_t lo = (size_t)std::floor(idx);
    const double f = idx - (double)lo;
    return lo + 1 < s.size() ? s[lo] + f * (s[lo + 1] - s[lo]) : s[lo];
  };
  double mean = 0, var = 0;
  for (double x : v) mean += x;
  mean /= (double)n;
  for (double x : v) var += (x - mean) * (x - mean);
  const double sd = std::sqrt(var / (double)n), med = pct(v, 0.5);
  std::vector<double> dev;
  for (double x : v) dev.push_back(std::fabs(x - med));
  std::sort(dev.begin(), dev.end());
  std::string out = "N: " + std::to_string(n) + ", μ/σ: " + rnd(mean) + "/" + rnd(sd) + ", med/mad: " + rnd(med) +
                    "/" + rnd(pct(dev, 0.5)) + "\n";
  std::vector<std::string> runs;
  for (auto &kv : hist)
    runs.push_back(std::to_string(kv.first) + (kv.second > 1 ? "×" + std::to_string(kv.second) : ""));
  out += " elems:";
  for (size_t i = 0; i < runs.size(); ++i) {
    if (runs.size() > 20 && i == 10) {
      out += " …";
      i = runs.size() - 10;
    }
    out += " " + runs[i];
  }
  out += "\n";
  const double ps[] = {0.01, 0.05, 0.10, 0.25, 0.50, 0.75, 0.90, 0.95, 0.99};
  for (double p : ps) {
    const double idx = (double)(n + 1) * p - 1;
    if (idx < 0 || idx > (double)(n - 1)) continue;
    char lab[16];
    snprintf(lab, sizeof lab, "%.2f", p);
    out += std::string("  ") + (lab + 1) + ":\t" + rnd(pct(v, p)) + "\n";
  }
  return out;
}

// java.lang.Double.toString for 1e-3 <= |x| < 1e7: the shortest digits that read back
std::string jdouble(double x) {
  char b[64];
  for (int p = 1; p <= 17; ++p) {
    snprintf(b, sizeof b, "%.*g", p, x);
    if (std::strtod(b, nullptr) == x) break;
  }
  std::string s(b);
  if (s.find('.') == std::string::npos && s.find('e') == std::string::npos) s += ".0";
  return s;
}

// CheckBlocks (cli/.../check/blocks/CheckBlocks.scala:30-195), -s mode: for every BGZF
// block, the next read start from Pos(start, 0) by the indexed checker (the .records
// ground truth) and by the eager checker; blocks where they differ are reported with the
// compressed positions whose splits they would break.
int check_blocks(const Args &a) {
  if (!a.s || a.u) no_hadoop_bam();
  Loaded L(a.path);
  std::vector<uint64_t> truth;
  for (auto &r : read_records_file(a.records.empty() ? a.path + ".records" : a.records)) {
    uint64_t f = 0;
    chk(sbh_flat_of(L.sh, r.block, r.off, &f), "records file position");
    truth.push_back(f);
  }
  std::sort(truth.begin(), truth.end());
  uint64_t seg_end = L.flat;
  std::vector<const sbh_block *> blocks;
  for (const sbh_block &b : L.blocks) {
    if (b.flags & SBH_BLOCK_EMPTY) { seg_end = b.ustart; break; }  // the stream (and the block list) ends
    blocks.push_back(&b);
  }
  std::vector<uint8_t> bits((seg_end + 7) / 8);
  uint64_t ncalled = 0;
  if (seg_end) chk(sbh_check_eager(L.sh, 0, seg_end, a.reads_to_check, bits.data(), &ncalled), "eager");
  auto next_set = [&](uint64_t f) -> int64_t {  // eager nextReadStart: first call in [f, f + maxReadSize)
    const uint64_t lim = std::min<uint64_t>(seg_end, f + (uint64_t)a.max_read_size);
    for (uint64_t i = f; i < lim; ++i)
      if (bits[i >> 3] & (1u << (i & 7))) return (int64_t)i;
    return -1;
  };
  auto show = [&](int64_t f) { return f < 0 ? std::string("-") : L.pos((uint64_t)f).str(); };
  std::map<long long, uint64_t> offsets;  // first read's offset in its block -> blocks
  uint64_t no_read = 0, wrong_pos = 0;
  std::vector<std::string> bad;
  for (size_t i = 0; i < blocks.size(); ++i) {
    const sbh_block &b = *blocks[i];
    auto it = std::lower_bound(truth.begin(), truth.end(), b.ustart);
    const int64_t p1 = it == truth.end() ? -1 : (int64_t)*it;
    const int64_t p2 = next_set(b.ustart);
    if (p1 >= 0 && L.pos((uint64_t)p1).block == b.start) ++offsets[(long long)L.pos((uint64_t)p1).off];
    else ++no_read;
    if (p1 != p2) {
      const uint64_t prev = i ? blocks[i - 1]->csize : 1;
      wrong_pos += prev;
      bad.push_back(std::to_string(b.start) + " (prev block size: " + std::to_string(prev) + "):\t" + show(p1) +
                    "\t" + show(p2));
    }
  }
  const uint64_t total = L.data.size();
  auto offsets_info = [&]() {
    if (no_read && offsets.size() == 1 && offsets.count(0))
      printf("\n%llu blocks start with a read, %llu blocks didn't contain a read\n",
             (unsigned long long)offsets[0], (unsigned long long)no_read);
    else if (!no_read && offsets.size() == 1 && offsets.count(0))
      printf("\nAll blocks start with reads\n");
    else
      printf("\nOffsets of blocks' first reads (%llu blocks didn't contain a read start):\n%s",
             (unsigned long long)no_read, stats_hist(offsets).c_str());
  };
  if (bad.empty()) {
    printf("First read-position matched in %zu BGZF blocks totaling %sB (compressed)\n", blocks.size(),
           bytes_fmt(total).c_str());
    offsets_info();
  } else {
    printf("First read-position mismatched in %zu of %zu BGZF blocks\n\n", bad.size(), blocks.size());
    printf("%llu of %llu (%s) compressed positions would lead to bad splits\n", (unsigned long long)wrong_pos,
           (unsigned long long)total, jdouble((double)wrong_pos / (double)total).c_str());
    offsets_info();
    printf("\n");
    if ((long)bad.size() <= a.limit) printf("%zu mismatched blocks:\n", bad.size());
    else printf("%ld of %zu mismatched blocks:\n", a.limit, bad.size());
    for (size_t i = 0; i < bad.size() && (long)i < a.limit; ++i) printf("\t%s\n", bad[i].c_str());
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  try {
    Args a = parse(argc, argv);
    chk(sbh_ctx_create(0, &g_ctx), "context");
    int rc;
    if (a.cmd == "compute-splits") rc = compute_splits(a);
    else if (a.cmd == "count-reads") rc = count_reads(a);
    else if (a.cmd == "check-bam") rc = check_bam(a);
    else if (a.cmd == "full-check") rc = full_check(a);
    else if (a.cmd == "index-blocks") rc = index_blocks(a);
    else if (a.cmd == "index-records") rc = index_records(a);
    else if (a.cmd == "index-bai") rc = index_bai(a);
    else if (a.cmd == "check-blocks") rc = check_blocks(a);
    else if (a.cmd == "htsjdk-rewrite") rc = htsjdk_rewrite(a);
    else if (a.cmd == "view" || a.cmd == "sort") rc = view(a);
    else if (a.cmd == "depth") rc = depth(a);
    else if (a.cmd == "pileup" || a.cmd == "consensus") rc = pileup(a);
    else if (a.cmd == "flagstat" || a.cmd == "idxstats") rc = tally(a);
    else if (a.cmd == "stats") rc = stats(a);
    else if (a.cmd == "fastq" || a.cmd == "fasta") rc = fastq(a);
    else throw Error(SBH_E_ARG, "unknown command " + a.cmd);
    sbh_ctx_destroy(g_ctx);
    return rc;
  } catch (const Error &e) {
    fprintf(stderr, "spark-bam: %s\n", e.what());
    if (g_ctx) sbh_ctx_destroy(g_ctx);
    return 1;
  } catch (const std::exception &e) {
    fprintf(stderr, "spark-bam: %s\n", e.what());
    return 1;
  }
}
