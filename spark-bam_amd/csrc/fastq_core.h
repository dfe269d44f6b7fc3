// fastq_core.h -- the FASTQ / FASTA text of a record scan's rows (samtools fastq, samtools fasta),
// written once for both sides: the device kernels (fastq.hip: k_fastq_sizes, k_fastq_emit) and the
// host renderer below (sbh_fastq_render_host, tests/sanitize/fastq_driver.cpp).
// SBH_HD is __host__ __device__ under hipcc, empty otherwise.
//
// Fields of one record (r = its first byte): l_name = r[12], n_cig = ld16(r + 16),
// flag = ld32(r + 16) >> 16, l_seq = ld32(r + 20); the name at r + 36, the packed bases at
// r + 36 + l_name + 4 n_cig, the qualities behind the (l_seq + 1) / 2 base bytes.
//
// Every row, kept or not, passes row_check; a row the filter keeps (bam_gather_core.h; no filter:
// every row) renders as
//     @NAME[/1|/2]\nSEQ\n+\nQUAL\n        (FASTQ)
//     >NAME[/1|/2]\nSEQ\n                 (MODE_FASTA)
//   NAME    sam_core.h's QNAME: the name bytes up to the first NUL
//   suffix  MODE_SUFFIX: /1 when flag & 0x1 and (flag & 0xC0) == 0x40, /2 when flag & 0x1 and
//           (flag & 0xC0) == 0x80, else none; MODE_SUFFIX_ALWAYS: the same without the 0x1 condition
//           (it wins when both bits are given); neither bit: none
//   SEQ     base j is "=ACMGRSVTWYHKDBN"[code(j)], code(j) the high nibble of byte j / 2 for even j,
//           the low nibble for odd j; with flag & 0x10 the reverse complement: base j is
//           comp(code(l_seq - 1 - j)), comp the reversal of the four bits (A<>T C<>G M<>K R<>Y V<>B
//           H<>D; = S W N stay).  l_seq == 0: an empty line
//   QUAL    byte j is min(q, 93) + 33, q read from the other end with flag & 0x10 (SAM text's
//           (q + 33) & 0xFF would print q = 233 as a newline); a first quality byte 0xFF: every
//           byte is def_qual + 33, def_qual in [0, 93].  l_seq == 0: an empty line
//   len     1 + name + suffix + 1 + l_seq + 1 [+ 2 + l_seq + 1], in 64 bits
// MODE_SPLIT: a kept row's class is 1 or 2 by the /1 and /2 conditions (MODE_SUFFIX_ALWAYS drops
// the 0x1 condition here too, so class and suffix agree), else 0.  The text is three parts one
// after another -- class 1, class 2, class 0 -- each in row order; without the bit, one part in
// row order.
//
// The bytes of a line are a function of (record, position in the line): line_byte below.  The
// emit kernel and the host renderer both call it for every byte they write, so the index
// arithmetic of the reverse strand (where an odd l_seq flips the nibble parity between source and
// destination) exists once.
#pragma once
#include <stdint.h>

#include "bam_gather_core.h"
#include "sam_core.h"

namespace sbh_fq {

constexpr uint32_t MODE_FASTA = 1u, MODE_SUFFIX = 2u, MODE_SUFFIX_ALWAYS = 4u, MODE_SPLIT = 8u;  // SBH_FASTQ_*
constexpr uint32_t MODE_ALL = 15u;
constexpr int32_t QUAL_MAX = 93;  // '~' - 33
constexpr uint32_t PARTS = 3;

// 1, 2 or 0 (see the head of the file)
SBH_HD inline uint32_t class_of(uint32_t flag, uint32_t mode) {
  if (!(flag & 0x1u) && !(mode & MODE_SUFFIX_ALWAYS)) return 0;
  return (flag & 0xC0u) == 0x40u ? 1u : (flag & 0xC0u) == 0x80u ? 2u : 0u;
}
// the digit behind the '/', 0: no suffix
SBH_HD inline uint32_t suffix_of(uint32_t cls, uint32_t mode) {
  return (mode & (MODE_SUFFIX | MODE_SUFFIX_ALWAYS)) && cls ? (uint32_t)'0' + cls : 0u;
}
// where a class's lines go: its part of the text (1, 2, 0 in that order; one part without MODE_SPLIT)
SBH_HD inline uint32_t part_of(uint32_t cls, uint32_t mode) { return (mode & MODE_SPLIT) ? (cls + 2u) % 3u : 0u; }
SBH_HD inline uint32_t n_parts(uint32_t mode) { return (mode & MODE_SPLIT) ? PARTS : 1u; }

// what a line has besides its name
SBH_HD inline uint64_t fixed_len(uint64_t l_seq, uint32_t suffix, uint32_t mode) {
  return 1 + (suffix ? 2 : 0) + 1 + l_seq + 1 + ((mode & MODE_FASTA) ? 0 : 2 + l_seq + 1);
}
SBH_HD inline uint64_t line_len(uint64_t name_len, uint64_t l_seq, uint32_t suffix, uint32_t mode) {
  return name_len + fixed_len(l_seq, suffix, mode);
}

// "=ACMGRSVTWYHKDBN"[c] without a table in memory: eight letters to a word
constexpr uint64_t LETTERS_LO = 0x565352474D43413Dull, LETTERS_HI = 0x4E42444B48595754ull;
SBH_HD constexpr uint8_t base_letter(uint32_t c) { return (uint8_t)(((c & 8u) ? LETTERS_HI : LETTERS_LO) >> (8u * (c & 7u))); }
constexpr bool letters_ok() {
  for (uint32_t c = 0; c < 16; ++c)
    if (base_letter(c) != (uint8_t)"=ACMGRSVTWYHKDBN"[c]) return false;
  return true;
}
static_assert(letters_ok(), "base_letter spells =ACMGRSVTWYHKDBN");
SBH_HD inline uint32_t comp4(uint32_t c) { return (c & 1u) << 3 | (c & 2u) << 1 | (c & 4u) >> 1 | (c & 8u) >> 3; }
SBH_HD inline uint32_t code_at(const uint8_t *seq, uint64_t j) {
  const uint32_t b = seq[j >> 1];
  return (j & 1) ? (b & 15u) : (b >> 4);
}

// One kept record's line.  name_len <= l_name and every read index is below l_name resp. l_seq,
// whatever `len` says.
struct Line {
  const uint8_t *name, *seq, *qual;
  uint64_t l_seq, len;
  uint32_t name_len, suffix, defq;  // defq: def_qual + 33 when the qualities are missing, else 0
  bool rev, fasta;
};

// r = the first byte of a record row_check accepts; name_len as the size pass found it
SBH_HD inline Line line_of(const uint8_t *r, uint32_t name_len, uint32_t cls, uint32_t mode, int32_t def_qual) {
  const uint32_t l_name = r[12], n_cig = sbh_sam::ld16(r + 16), flag = sbh_sam::ld16(r + 18);
  Line L;
  L.l_seq = (uint64_t)(int32_t)sbh_sam::ld32(r + 20);
  L.name = r + 36;
  L.seq = L.name + l_name + 4ull * n_cig;
  L.qual = L.seq + (L.l_seq + 1) / 2;
  L.name_len = name_len < l_name ? name_len : l_name;
  L.suffix = suffix_of(cls, mode);
  L.defq = L.l_seq && L.qual[0] == 0xFF ? (uint32_t)def_qual + 33u : 0u;
  L.rev = flag & 0x10u;
  L.fasta = mode & MODE_FASTA;
  L.len = line_len(L.name_len, L.l_seq, L.suffix, mode);
  return L;
}
// the same from the line's length (the emit pass reads the size pass's): the name is what the
// fixed parts leave, never more than l_name
SBH_HD inline Line line_of_len(const uint8_t *r, uint64_t len, uint32_t cls, uint32_t mode, int32_t def_qual) {
  const uint64_t ls = (uint64_t)(int32_t)sbh_sam::ld32(r + 20);
  const uint64_t fixed = fixed_len(ls, suffix_of(cls, mode), mode);
  const uint64_t name = len > fixed ? len - fixed : 0;
  return line_of(r, name < 255 ? (uint32_t)name : 255u, cls, mode, def_qual);
}

// byte k of the line, k < L.len
SBH_HD inline uint8_t line_byte(const Line &L, uint64_t k) {
  if (k == 0) return L.fasta ? '>' : '@';
  k -= 1;
  if (k < L.name_len) return L.name[k];
  k -= L.name_len;
  if (L.suffix) {
    if (k == 0) return '/';
    if (k == 1) return (uint8_t)L.suffix;
    k -= 2;
  }
  if (k == 0) return '\n';
  k -= 1;
  if (k < L.l_seq) {
    const uint32_t c = L.rev ? comp4(code_at(L.seq, L.l_seq - 1 - k)) : code_at(L.seq, k);
    return base_letter(c);
  }
  k -= L.l_seq;
  if (k == 0 || L.fasta) return '\n';
  if (k == 1) return '+';
  if (k == 2) return '\n';
  k -= 3;
  if (k < L.l_seq) {
    if (L.defq) return (uint8_t)L.defq;
    const uint32_t q = L.qual[L.rev ? L.l_seq - 1 - k : k];
    return (uint8_t)((q < (uint32_t)QUAL_MAX ? q : (uint32_t)QUAL_MAX) + 33u);
  }
  return '\n';
}

}  // namespace sbh_fq

// ---- the host renderer (plain host functions under hipcc too) -----------------------------------
namespace sbh_fq {

struct Sizes {  // sbh_fastq_sizes' layout
  uint64_t n, n_kept, text_bytes, part_bytes[PARTS], part_rows[PARTS];
};

// The text of the records at starts[0..n) that F keeps.  rec_off (n_kept + 1 written: the lines'
// offsets in layout order, then text_bytes) and rows (n_kept written: the row of each line) may be
// nullptr, and so may text (sizes only).  Returns 0, 1 (a bad row: *bad_row, nothing else written) or
// 2 (text_cap too small; *sz is set).
inline int render_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n,
                       const sbh_bam::Filter &F, uint32_t mode, int32_t def_qual, char *text, uint64_t text_cap,
                       uint64_t *rec_off, uint64_t *rows, Sizes *sz, uint64_t *bad_row) {
  *bad_row = sbh_bam::NO_ROW;
  *sz = Sizes{n, 0, 0, {0, 0, 0}, {0, 0, 0}};
  uint64_t bytes = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (sbh_bam::row_check(flat, flat_size, starts[i], &bytes) != sbh_bam::ROW_OK) {
      *bad_row = i;
      return 1;
    }
  auto line = [&](uint64_t i) {
    const uint8_t *r = flat + starts[i];
    return line_of(r, sbh_sam::qname_len(r + 36, r[12]), class_of(sbh_sam::ld16(r + 18), mode), mode, def_qual);
  };
  auto part = [&](uint64_t i) { return part_of(class_of(sbh_sam::ld16(flat + starts[i] + 18), mode), mode); };
  for (uint64_t i = 0; i < n; ++i) {
    if (!sbh_bam::row_keep(flat + starts[i], i, F)) continue;
    const uint32_t p = part(i);
    sz->part_bytes[p] += line(i).len;
    ++sz->part_rows[p];
  }
  uint64_t at[PARTS], k[PARTS];  // each part's next byte and next line
  for (uint32_t p = 0; p < PARTS; ++p) {
    at[p] = sz->text_bytes, k[p] = sz->n_kept;
    sz->text_bytes += sz->part_bytes[p], sz->n_kept += sz->part_rows[p];
  }
  if (text && text_cap < sz->text_bytes) return 2;
  for (uint64_t i = 0; i < n; ++i) {
    if (!sbh_bam::row_keep(flat + starts[i], i, F)) continue;
    const uint32_t p = part(i);
    const Line L = line(i);
    if (rec_off) rec_off[k[p]] = at[p];
    if (rows) rows[k[p]] = i;
    if (text)
      for (uint64_t b = 0; b < L.len; ++b) text[at[p] + b] = (char)line_byte(L, b);
    at[p] += L.len, ++k[p];
  }
  if (rec_off) rec_off[sz->n_kept] = sz->text_bytes;
  return 0;
}

}  // namespace sbh_fq
