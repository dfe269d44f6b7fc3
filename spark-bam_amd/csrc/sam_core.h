// sam_core.h -- the definition of a BAM record's SAM text line, written once for both sides:
// the device kernels (sam.hip: k_sam_sizes, k_sam_emit) and the host renderer below
// (sbh_sam_render_host, the rows with float tags, tests/sanitize/sam_driver.cpp).
// SBH_HD is __host__ __device__ under hipcc, empty otherwise.
//
// A line is what records.py's Reads.sam_line produces (htsjdk SAMRecord.getSAMString, the format
// of the reference's test_bams/*.sam) plus a final '\n': eleven tab-separated fields
//   QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL
// then one "\tTG:T:VALUE" per tag.
//   QNAME   the name bytes up to the first NUL (may be empty)
//   RNAME   the reference name for 0 <= ref_id < n_ref, else "*"
//   POS     pos + 1, PNEXT next_pos + 1 (64-bit: 2^31 - 1 prints 2147483648)
//   RNEXT   "*" for next_ref_id < 0, "=" for next_ref_id == ref_id, the name below n_ref, else "*"
//   CIGAR   "*" for no ops, else <len><op> per op with MIDNSHP=X; an op code above 8 is malformed
//   SEQ     "*" for l_seq == 0, else the "=ACMGRSVTWYHKDBN" letters
//   QUAL    "*" for l_seq == 0 or a first quality byte 0xFF, else each byte (q + 33) & 0xFF
//   tags    A: the byte; c C s S i I: ":i:" and the decimal value; Z H: the bytes up to the NUL;
//           B: ":B:<sub>" then ",<value>" per element; f and B:f: Java's Float.toString (host only)
// The tag area is malformed when a type (or B sub-type) byte is unknown, a value runs past the
// record's tag bytes, a Z / H has no NUL inside them, a B count is negative, or 1 or 2 bytes are
// left after the last tag.
#pragma once
#include <stdint.h>

#ifndef SBH_HD
#define SBH_HD
#endif

namespace sbh_sam {

SBH_HD inline uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
SBH_HD inline uint32_t ld32(const uint8_t *p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// ---- decimal text ----
SBH_HD inline uint32_t dec_digits(uint32_t v) {
  return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6
       : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}
// v's dec_digits(v) digits at dst
SBH_HD inline uint32_t put_dec(char *dst, uint32_t v) {
  const uint32_t n = dec_digits(v);
  for (uint32_t k = n; k-- > 0;) {
    dst[k] = (char)('0' + v % 10u);
    v /= 10u;
  }
  return n;
}
// signed values of magnitude < 2^32: every integer a record holds (int32 fields + 1, u32 tags)
SBH_HD inline uint32_t sdec_len(int64_t v) { return v < 0 ? 1 + dec_digits((uint32_t)(-v)) : dec_digits((uint32_t)v); }
SBH_HD inline uint32_t put_sdec(char *dst, int64_t v) {
  if (v < 0) {
    *dst = '-';
    return 1 + put_dec(dst + 1, (uint32_t)(-v));
  }
  return put_dec(dst, (uint32_t)v);
}

// ---- the fixed fields (r = the record's first byte, its block_size word) ----
struct Fixed {
  int32_t ref_id, pos, next_ref, next_pos, tlen, l_seq;
  uint32_t l_name, mapq, n_cigar, flag;
};
SBH_HD inline Fixed fixed_of(const uint8_t *r) {
  Fixed f;
  f.ref_id = (int32_t)ld32(r + 4);
  f.pos = (int32_t)ld32(r + 8);
  f.l_name = r[12];
  f.mapq = r[13];
  f.n_cigar = ld16(r + 16);
  f.flag = ld16(r + 18);
  f.l_seq = (int32_t)ld32(r + 20);
  f.next_ref = (int32_t)ld32(r + 24);
  f.next_pos = (int32_t)ld32(r + 28);
  f.tlen = (int32_t)ld32(r + 32);
  return f;
}

// QNAME: the l_name name bytes up to the first NUL (may be empty).  Sixteen bytes a step, each read
// at an index clamped below l_name: the reads of a step do not depend on one another, so a lane
// waits for memory once per step and not once per byte.
SBH_HD inline uint32_t qname_len(const uint8_t *name, uint32_t l_name) {
  for (uint32_t base = 0; base < l_name; base += 16) {
    uint32_t nul = 0;
    for (uint32_t j = 0; j < 16; ++j) {
      const uint32_t k = base + j < l_name ? base + j : l_name - 1;
      nul |= (uint32_t)(name[k] == 0) << j;
    }
    if (nul) {
      uint32_t j = 0;
      while (!((nul >> j) & 1u)) ++j;
      return base + j < l_name ? base + j : l_name;
    }
  }
  return l_name;
}

// reference names packed: name k = names[off[k] .. off[k + 1])
struct Refs {
  const char *names;
  const uint64_t *off;
  int32_t n;
};
constexpr int32_t REF_STAR = -1, REF_EQ = -2;
SBH_HD inline int32_t rname_ref(const Fixed &f, int32_t n_ref) { return f.ref_id >= 0 && f.ref_id < n_ref ? f.ref_id : REF_STAR; }
SBH_HD inline int32_t rnext_ref(const Fixed &f, int32_t n_ref) {
  if (f.next_ref < 0) return REF_STAR;
  if (f.next_ref == f.ref_id) return REF_EQ;
  return f.next_ref < n_ref ? f.next_ref : REF_STAR;
}
SBH_HD inline uint64_t ref_len(const Refs &R, int32_t k) { return k < 0 ? 1 : R.off[k + 1] - R.off[k]; }

// ---- CIGAR ----
SBH_HD inline bool cigar_op_ok(uint32_t op) { return (op & 15u) <= 8u; }
SBH_HD inline uint32_t cigar_op_len(uint32_t op) { return dec_digits(op >> 4) + 1; }
SBH_HD inline uint32_t put_cigar_op(char *dst, uint32_t op) {
  const uint32_t n = put_dec(dst, op >> 4);
  dst[n] = "MIDNSHP=X"[op & 15u];
  return n + 1;
}
SBH_HD inline char seq_letter(const uint8_t *seq, uint64_t k) {
  const uint8_t b = seq[k >> 1];
  return "=ACMGRSVTWYHKDBN"[(k & 1) ? (b & 15) : (b >> 4)];
}

// ---- the line-length formula ----
// FLAG RNAME POS MAPQ RNEXT PNEXT TLEN
SBH_HD inline uint64_t fixed_text_len(const Fixed &f, const Refs &R) {
  return dec_digits(f.flag) + ref_len(R, rname_ref(f, R.n)) + sdec_len((int64_t)f.pos + 1) + dec_digits(f.mapq) +
         ref_len(R, rnext_ref(f, R.n)) + sdec_len((int64_t)f.next_pos + 1) + sdec_len(f.tlen);
}
SBH_HD inline uint64_t seq_text_len(const Fixed &f) { return f.l_seq ? (uint64_t)f.l_seq : 1; }
SBH_HD inline uint64_t qual_text_len(const Fixed &f, uint8_t first_qual) {
  return f.l_seq == 0 || first_qual == 0xFF ? 1 : (uint64_t)f.l_seq;
}
// name + the seven fixed fields + CIGAR + SEQ + QUAL + tags (each tag with its leading tab) + the ten
// tabs between the eleven fields + '\n'
SBH_HD inline uint64_t line_len(uint64_t name, uint64_t fixed, uint64_t cigar, uint64_t seq, uint64_t qual,
                                uint64_t tags) {
  return name + fixed + cigar + seq + qual + tags + 11;
}

// ---- the tag area ----
constexpr uint32_t TAG_PREFIX = 6;  // "\tTG:T:"
// bytes of a fixed-size value of this type (A c C s S i I f), 0 for every other type byte
SBH_HD inline uint32_t tag_value_size(uint8_t t) {
  switch (t) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    default: return 0;
  }
}
SBH_HD inline uint32_t tag_elem_size(uint8_t sub) { return sub == 'A' ? 0 : tag_value_size(sub); }  // B sub-types
SBH_HD inline int64_t tag_int(uint8_t t, const uint8_t *p) {  // c C s S i I
  switch (t) {
    case 'c': return (int8_t)p[0];
    case 'C': return p[0];
    case 's': return (int16_t)ld16(p);
    case 'S': return ld16(p);
    case 'i': return (int32_t)ld32(p);
    default: return ld32(p);
  }
}
// The tag at aux[cur ..] of a tag area of l_aux bytes (cur < l_aux): its type, where its value begins,
// and for the fixed-size types and B how many bytes it has (B: sub-type, element count and size; val
// is the first element).  A Z / H value ends at the first NUL of [val, l_aux), which the caller
// finds.  false: malformed (see the head of the file); every byte read lies below l_aux.
struct Tag {
  uint8_t type, sub;
  uint32_t val, size, count, esz;
};
SBH_HD inline bool tag_head(const uint8_t *aux, uint32_t l_aux, uint32_t cur, Tag *t) {
  if (l_aux - cur < 3) return false;  // 1 or 2 bytes left over
  t->type = aux[cur + 2];
  t->sub = 0;
  t->val = cur + 3;
  t->count = t->esz = 0;
  t->size = tag_value_size(t->type);
  if (t->size) return t->size <= l_aux - t->val;
  if (t->type == 'Z' || t->type == 'H') return true;
  if (t->type != 'B' || l_aux - t->val < 5) return false;
  t->sub = aux[t->val];
  t->esz = tag_elem_size(t->sub);
  const int32_t cnt = (int32_t)ld32(aux + t->val + 1);
  t->val += 5;
  if (!t->esz || cnt < 0 || (uint64_t)cnt * t->esz > (uint64_t)(l_aux - t->val)) return false;
  t->count = (uint32_t)cnt;
  t->size = t->count * t->esz;
  return true;
}
// "\tTG:T:" of a tag (the integer types all print as i)
SBH_HD inline void put_tag_prefix(char *dst, const uint8_t *aux, uint32_t cur, uint8_t type) {
  dst[0] = '\t';
  dst[1] = (char)aux[cur];
  dst[2] = (char)aux[cur + 1];
  dst[3] = ':';
  dst[4] = (type == 'A' || type == 'f' || type == 'Z' || type == 'H' || type == 'B') ? (char)type : 'i';
  dst[5] = ':';
}

}  // namespace sbh_sam

// ---- the host renderer (plain host functions under hipcc too) -----------------------------------
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace sbh_sam {

// java.lang.Float.toString: NaN, Infinity, -Infinity, 0.0, -0.0 as those words; otherwise the
// fewest decimal digits, but at least two, that read back as the same float32 ("%.{p-1}e" for
// p = 2..9 until strtof round-trips; a trailing zero of the two is dropped again), as plain
// decimal when the decimal exponent is in [-3, 6] (1e-3 <= |x| < 1e7), else d.dddE<exp>; at least
// one digit after the point either way.  Two places follow the JDK's FloatingDecimal rather than
// "shortest that reads back".  At least two digits are generated: the smallest denormal is
// 1.4E-45 in Java, not 1.0E-45, though "1e-45" reads back as it.  And for an exact power of two,
// whose lower neighbour is half as far away, FloatingDecimal halves its tolerance on both sides
// ("the next smallest number is only half as far away as we think"): the digits must lie within a
// quarter of the spacing above x, so FLT_MIN is 1.17549435E-38, not the 1.1754944E-38 that also
// reads back.  dst: >= 24 bytes.
inline uint32_t put_float(char *dst, float x) {
  uint32_t bits;
  memcpy(&bits, &x, 4);
  const bool neg = bits >> 31;
  const char *word = nullptr;
  if ((bits & 0x7f800000u) == 0x7f800000u) word = (bits & 0x007fffffu) ? "NaN" : neg ? "-Infinity" : "Infinity";
  else if (!(bits & 0x7fffffffu)) word = neg ? "-0.0" : "0.0";
  if (word) {
    const uint32_t n = (uint32_t)strlen(word);
    memcpy(dst, word, n);
    return n;
  }
  char buf[32], dig[12];
  const float ax = neg ? -x : x;
  const uint32_t ex = (bits >> 23) & 0xffu, mant = bits & 0x007fffffu;
  const bool pow2 = ex ? mant == 0 : (mant & (mant - 1)) == 0;
  const double quarter_ulp = ldexp(1.0, (ex ? (int)ex - 150 : -149) - 2);
  for (int p = 2; p <= 9; ++p) {
    snprintf(buf, sizeof buf, "%.*e", p - 1, (double)ax);
    if (pow2 ? fabs(strtod(buf, nullptr) - (double)ax) < quarter_ulp : strtof(buf, nullptr) == ax) break;
  }
  // buf = d<point>ddd e<sign>XX
  uint32_t nd = 0;
  const char *c = buf;
  for (; *c && *c != 'e' && *c != 'E'; ++c)
    if (*c >= '0' && *c <= '9') dig[nd++] = *c;
  const int e = atoi(c + 1);
  while (nd > 1 && dig[nd - 1] == '0') --nd;
  uint32_t o = 0;
  if (neg) dst[o++] = '-';
  if (e >= -3 && e <= 6) {
    if (e >= 0) {
      for (int k = 0; k <= e; ++k) dst[o++] = (uint32_t)k < nd ? dig[k] : '0';
      dst[o++] = '.';
      if ((uint32_t)e + 1 >= nd) dst[o++] = '0';
      for (uint32_t k = (uint32_t)e + 1; k < nd; ++k) dst[o++] = dig[k];
    } else {
      dst[o++] = '0';
      dst[o++] = '.';
      for (int k = -1; k > e; --k) dst[o++] = '0';
      for (uint32_t k = 0; k < nd; ++k) dst[o++] = dig[k];
    }
  } else {
    dst[o++] = dig[0];
    dst[o++] = '.';
    if (nd == 1) dst[o++] = '0';
    for (uint32_t k = 1; k < nd; ++k) dst[o++] = dig[k];
    dst[o++] = 'E';
    o += put_sdec(dst + o, e);
  }
  return o;
}

constexpr uint64_t NO_ROW = ~0ull;

// One record's line: its length, and with dst != nullptr its bytes (dst has room for them: the
// caller sized it by a first call).  r = the record (block_size word first), rec_bytes = 4 +
// block_size, already checked to hold the fixed fields, name, CIGAR, bases and qualities.
// 0: malformed (a line is never empty: it ends in '\n').
inline uint64_t render_record(const uint8_t *r, uint64_t rec_bytes, const Refs &R, char *dst) {
  const Fixed f = fixed_of(r);
  const uint8_t *name = r + 36, *cig = name + f.l_name, *seq = cig + 4ull * f.n_cigar;
  const uint8_t *qual = seq + ((uint64_t)f.l_seq + 1) / 2, *aux = qual + f.l_seq;
  const uint32_t l_aux = (uint32_t)(r + rec_bytes - aux);
  uint64_t o = 0;
  char num[24];
  auto bytes = [&](const void *src, uint64_t n) {
    if (dst && n) memcpy(dst + o, src, n);
    o += n;
  };
  auto ch = [&](char c) {
    if (dst) dst[o] = c;
    ++o;
  };
  auto ref = [&](int32_t k) {
    if (k == REF_STAR) ch('*');
    else if (k == REF_EQ) ch('=');
    else bytes(R.names + R.off[k], R.off[k + 1] - R.off[k]);
  };
  const uint32_t name_len = qname_len(name, f.l_name);
  bytes(name, name_len);
  ch('\t');
  bytes(num, put_dec(num, f.flag));
  ch('\t');
  ref(rname_ref(f, R.n));
  ch('\t');
  bytes(num, put_sdec(num, (int64_t)f.pos + 1));
  ch('\t');
  bytes(num, put_dec(num, f.mapq));
  ch('\t');
  if (!f.n_cigar) ch('*');
  for (uint32_t k = 0; k < f.n_cigar; ++k) {
    const uint32_t op = ld32(cig + 4ull * k);
    if (!cigar_op_ok(op)) return 0;
    bytes(num, put_cigar_op(num, op));
  }
  ch('\t');
  ref(rnext_ref(f, R.n));
  ch('\t');
  bytes(num, put_sdec(num, (int64_t)f.next_pos + 1));
  ch('\t');
  bytes(num, put_sdec(num, f.tlen));
  ch('\t');
  if (!f.l_seq) ch('*');
  for (uint64_t k = 0; k < (uint64_t)f.l_seq; ++k) ch(seq_letter(seq, k));
  ch('\t');
  if (f.l_seq == 0 || qual[0] == 0xFF) ch('*');
  else
    for (uint64_t k = 0; k < (uint64_t)f.l_seq; ++k) ch((char)(uint8_t)(qual[k] + 33));
  for (uint32_t cur = 0; cur < l_aux;) {
    Tag t;
    if (!tag_head(aux, l_aux, cur, &t)) return 0;
    put_tag_prefix(num, aux, cur, t.type);
    bytes(num, TAG_PREFIX);
    const uint8_t *v = aux + t.val;
    if (t.type == 'Z' || t.type == 'H') {
      const void *nul = memchr(v, 0, l_aux - t.val);
      if (!nul) return 0;
      t.size = (uint32_t)((const uint8_t *)nul - v);
      bytes(v, t.size);
      cur = t.val + t.size + 1;
      continue;
    }
    if (t.type == 'A') ch((char)v[0]);
    else if (t.type == 'f') {
      float x;
      memcpy(&x, v, 4);
      bytes(num, put_float(num, x));
    } else if (t.type == 'B') {
      ch((char)t.sub);
      for (uint32_t k = 0; k < t.count; ++k) {
        ch(',');
        if (t.sub == 'f') {
          float x;
          memcpy(&x, v + 4ull * k, 4);
          bytes(num, put_float(num, x));
        } else {
          bytes(num, put_sdec(num, tag_int(t.sub, v + (uint64_t)k * t.esz)));
        }
      }
    } else {
      bytes(num, put_sdec(num, tag_int(t.type, v)));
    }
    cur = t.val + t.size;
  }
  ch('\n');
  return o;
}

// The lines of the records at starts[0..n) of a flat BAM stream, one after another: line_off[0..n]
// their prefix offsets (always filled up to the first malformed row), text (may be nullptr: sizes
// only) their bytes when text_cap holds them all.  Returns 0, 1 when a record is malformed
// (*bad_row = the first such row: it does not fit the stream or its own block_size, as
// k_rec_sizes judges, or its CIGAR / tag area is malformed) or 2 when text_cap is too small.
inline int render_host(const uint8_t *flat, uint64_t flat_size, const uint64_t *starts, uint64_t n, const Refs &R,
                       char *text, uint64_t text_cap, uint64_t *line_off, uint64_t *bad_row) {
  *bad_row = NO_ROW;
  line_off[0] = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t p = starts[i];
    uint64_t len = 0;
    if (p <= flat_size && flat_size - p >= 36) {
      const int64_t bsz = (int32_t)ld32(flat + p), ls = (int32_t)ld32(flat + p + 20);
      const int64_t need = 32 + (int64_t)flat[p + 12] + 4 * (int64_t)ld16(flat + p + 16) + (ls + 1) / 2 + ls;
      if (ls >= 0 && bsz >= need && (uint64_t)bsz <= flat_size - p - 4)
        len = render_record(flat + p, 4 + (uint64_t)bsz, R, nullptr);
    }
    if (!len) {
      *bad_row = i;
      return 1;
    }
    line_off[i + 1] = line_off[i] + len;
  }
  if (!text) return 0;
  if (line_off[n] > text_cap) return 2;
  for (uint64_t i = 0; i < n; ++i)
    render_record(flat + starts[i], 4 + (uint64_t)ld32(flat + starts[i]), R, text + line_off[i]);
  return 0;
}

}  // namespace sbh_sam
