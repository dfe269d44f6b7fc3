"""Hand-built probes for the eager and full checkers (test infrastructure; plain Python, no GPU).

Every probe is a candidate record whose header fields are free (l_read_name independent of
the name bytes, block_size of what follows), laid into streams so that the device kernels meet
it at every tile edge, with the checkers' answers at its first byte written down BY HAND from
the Scala.  Nothing here is computed from the oracle or from the library.

The rules the literals restate (paths under check/src/main/scala/org/hammerlab/bam/check/):

* full/Checker.scala:27-28      n == readsToCheck: Success(readsToCheck).
* full/Checker.scala:30-48      36 fixed bytes not there: Success(n) when the channel stands
                                exactly at the record's nominal start and n > 0, else
                                tooFewFixedBlockBytes with readsBeforeError = n.
* full/Checker.scala:53         nextOffset = startPos + 4 + remainingBytes: the NOMINAL start of
                                the next record; the cursor may be past it (an "abnormal" record)
                                and the next record is then READ at the cursor, COUNTED from nominal.
* PosChecker.scala:43-63        getRefPosError: idx < -1 (with pos < -1: both bits), idx >= n
                                (with pos < -1: both bits), pos < -1, idx >= 0 && pos > len(idx).
* full/Checker.scala:68-71      tooFewRemainingBytesImplied: remainingBytes < 32 + l_read_name +
                                4 * n_cigar + (l_seq + 1) / 2 + l_seq, in Java int arithmetic.
* full/Checker.scala:81-109     l_read_name 0: noReadName, 1: emptyReadName (neither reads a name
                                byte: the CIGAR is read straight after the fixed fields); else the
                                last byte != 0: nonNullTerminatedReadName, else a byte outside
                                '!'..'?' ++ 'A'..'~' (Checker.scala:12-17): nonASCIIReadName.
* full/Checker.scala:111-136    the first op with (op & 0xf) > 8: invalidCigarOp; the stream ends
                                inside the ops before one: tooFewBytesForCigarOps; else a mapped
                                read (flag & 4 == 0) with l_seq == 0 or n_cigar == 0:
                                EmptyMapped(emptySeq, emptyCigar) -- whose FIELDS are
                                (emptyMappedCigar, emptyMappedSeq), full/error/CigarOpsError.scala:22-24:
                                l_seq == 0 sets emptyMappedCigar, n_cigar == 0 sets emptyMappedSeq.
* full/Checker.scala:140-143    the stream ends inside the name: tooFewBytesForReadName, and the
                                CIGAR is not tested.
* full/Checker.scala:158-183    no flag: skip to nextOffset when it lies ahead (the skip clamps at
                                the stream's end), next record with n + 1; else Flags(..., n).
* full/error/Flags.scala:203-221  the bit of each flag.
* eager/Checker.scala:24-126    the same tests, false at the first that fails: the eager answer
                                is true exactly where the full answer is a Success.

A probe's expectation is written as (records that pass before the chain is decided, how it is
decided): `word(p, rtc)` turns that into the result word for a readsToCheck by the two rules at
full/Checker.scala:27-28 and :30-48 alone.
"""
import functools
import struct
from collections import namedtuple

import numpy as np

from deflate_build import EOF_MEMBER
from record_corpus import PAYLOADS, bgzf

# kernel constants of check.hip the layouts and the GPU tests aim at (named here so that a change
# of one of them in the kernel shows up as a failed coverage assertion, not as a silent miss)
ETILE, ELA, EW, ESTAGE = 16384, 4096, 20480, 20992
FTILE, FSN, FULL_FAST_REACH = 8192, 12288, 262435
CIG_WAVE, XQ_MIN_OPS, XQ_MIN_REC = 16, 32, 2048
SLOWCAP, FCCAP, FCTG, EQ_CHUNK = 512, 256, 1024, 4096
SEGCAP = EQ_CHUNK // 4          # k_eager: refID survivors a wave lists for its quarter (EW / 4) of the window

SUCCESS, N_SHIFT = 0x80000000, 20
FLAGS = ("tooFewFixedBlockBytes", "negativeReadIdx", "tooLargeReadIdx", "negativeReadPos", "tooLargeReadPos",
         "negativeNextReadIdx", "tooLargeNextReadIdx", "negativeNextReadPos", "tooLargeNextReadPos",
         "tooFewBytesForReadName", "nonNullTerminatedReadName", "nonASCIIReadName", "noReadName", "emptyReadName",
         "tooFewBytesForCigarOps", "invalidCigarOp", "emptyMappedCigar", "emptyMappedSeq",
         "tooFewRemainingBytesImplied")
(FIXED, NEG_IDX, BIG_IDX, NEG_POS, BIG_POS, NEG_NIDX, BIG_NIDX, NEG_NPOS, BIG_NPOS, NAME_EOF, NO_NUL, NON_ASCII,
 NO_NAME, EMPTY_NAME, CIGAR_EOF, BAD_OP, MAPPED_CIGAR, MAPPED_SEQ, IMPLIED) = (1 << i for i in range(19))

I32_MAX = 2 ** 31 - 1
SMALL = (16571, 1000, I32_MAX)
BIG = tuple(1000 + i for i in range(1500))
DICTS = {"SMALL": SMALL, "BIG": BIG}


def raw(bs=None, ref=-1, pos=-1, rnl=None, mapq=0, bin=0, nc=None, flag=4, lseq=0, nref=-1, npos=-1, tlen=0,
        name=b"A\0", ops=(), extra=b""):
    """A record's bytes with every header field free.  name: the name bytes as they lie in the
    stream (the NUL is the caller's business); ops: raw 32-bit op words; extra: bytes after the
    ops.  rnl / nc / bs default to what the bytes say (bs: everything after the first 4 bytes)."""
    tail = bytes(name) + b"".join(struct.pack("<I", o & 0xffffffff) for o in ops) + bytes(extra)
    rnl = len(name) if rnl is None else rnl
    nc = len(ops) if nc is None else nc
    bs = 32 + len(tail) if bs is None else bs
    u = lambda v: v & 0xffffffff
    return struct.pack("<9I", u(bs), u(ref), u(pos), (bin & 0xffff) << 16 | (mapq & 0xff) << 8 | (rnl & 0xff),
                       (flag & 0xffff) << 16 | (nc & 0xffff), u(lseq), u(nref), u(npos), u(tlen)) + tail


MIN = raw()                     # block_size 34, -1, -1, l_read_name 2, flag 4, 'A\0': 38 bytes
assert len(MIN) == 38 and MIN[:4] == struct.pack("<i", 34)
RUNWAY = MIN * 10               # minimal records: enough for readsToCheck 10 after any probe
FILL = 0xEE                     # filler between probes: refID 0xEEEEEEEE < -1 fails every dictionary

# How a probe's chain is decided, after `n` records passed:
#   ("flags", f)  record n + 1 fails with flag bits f         -> f | n << 20
#   ("more",)     records keep passing (a runway follows)     -> Success(readsToCheck)
#   ("end",)      the stream ends exactly at a nominal start  -> Success(n)   (n > 0)
Probe = namedtuple("Probe", "label data follow ctg n how tags")
PROBES = []
END_CASES = []


def word(p, rtc):
    """The full checker's word at the probe's first byte for a readsToCheck (0 <= rtc < 1024)."""
    if rtc <= p.n or p.how[0] == "more":
        return SUCCESS | rtc << N_SHIFT          # :27-28
    if p.how[0] == "end":
        return SUCCESS | p.n << N_SHIFT          # :34-37
    return p.how[1] | p.n << N_SHIFT


def eager(p, rtc):
    return bool(word(p, rtc) & SUCCESS)


def _fail(label, data, flags, ctg="BIG", n=0, follow=b"", **tags):
    PROBES.append(Probe(label, data, follow, ctg, n, ("flags", flags), tags))


def _pass(label, data, ctg="BIG", **tags):
    PROBES.append(Probe(label, data, RUNWAY, ctg, 1, ("more",), tags))


def _end(label, data, n, how, **tags):
    END_CASES.append(Probe(label, data, b"", "BIG", n, how, tags))


# ----------------------------------------------------------------------------- getRefPosError
# (idx, pos, error bits: 1 negativeRefIdx, 2 tooLargeRefIdx, 4 negativeRefPos, 8 tooLargeRefPos)
REFPOS = {
    "SMALL": (
        (-2, -2, 1 | 4), (-2, -1, 1), (-2, 0, 1), (-2, I32_MAX, 1), (-0x80000000, -0x80000000, 1 | 4),
        (3, -2, 2 | 4), (3, -1, 2), (3, 0, 2), (I32_MAX, -2, 2 | 4), (I32_MAX, 5, 2),
        (-1, -2, 4), (0, -2, 4), (2, -2, 4), (2, -0x80000000, 4),
        (-1, -1, 0), (-1, 0, 0), (-1, I32_MAX, 0),
        (0, -1, 0), (0, 0, 0), (0, 16571, 0), (0, 16572, 8), (0, I32_MAX, 8),
        (1, 1000, 0), (1, 1001, 8), (2, -1, 0), (2, I32_MAX, 0),
    ),
    "BIG": (
        (-2, -2, 1 | 4), (-2, 0, 1), (1500, -2, 2 | 4), (1500, 0, 2), (-1, -2, 4), (-1, I32_MAX, 0),
        (0, 1000, 0), (0, 1001, 8), (1023, 2023, 0), (1023, 2024, 8), (1024, 2024, 0), (1024, 2025, 8),
        (1025, 2025, 0), (1025, 2026, 8), (1499, 2499, 0), (1499, 2500, 8), (1499, -1, 0), (1499, -2, 4),
    ),
}
for _ctg, _rows in REFPOS.items():
    for _idx, _pos, _e in _rows:
        for _pair, _shift in (("read", 1), ("mate", 5)):
            _kw = dict(ref=_idx, pos=_pos) if _pair == "read" else dict(nref=_idx, npos=_pos)
            _lab = f"refpos_{_ctg}_{_pair}_{_idx}_{_pos}"
            if _e:
                _fail(_lab, raw(**_kw), _e << _shift, _ctg, refpos=(_pair, _e, _idx, _pos))
            else:
                _pass(_lab, raw(**_kw), _ctg, refpos=(_pair, 0, _idx, _pos))
# both pairs wrong at once; the read pair's error does not hide the mate's
_fail("refpos_both", raw(ref=-2, pos=-2, nref=1500, npos=-2), NEG_IDX | NEG_POS | BIG_NIDX | NEG_NPOS)
_fail("refpos_both_small", raw(ref=3, pos=0, nref=0, npos=16572), BIG_IDX | BIG_NPOS, "SMALL")

# ----------------------------------------------------------------------------- read name
NAME_LENGTHS = (0, 1, 2, 17, 32, 33, 34, 48, 49, 50, 255)      # l_read_name
BAD_AT = (0, 3, 4, 15, 16, 31, 32, 33, 47, 48, 253)
BAD_BYTES = (0x00, 0x20, 0x40, 0x7F, 0x80, 0xFF)
EDGE_OK_BYTES = (0x21, 0x3F, 0x41, 0x7E)


def name_of(rnl, at=None, byte=None, nul=True):
    """rnl name bytes: letters, the NUL last (or 'A' when nul is False), one byte replaced."""
    b = bytearray(0x42 + k % 57 for k in range(rnl - 1)) + (b"\0" if nul else b"A")
    if at is not None:
        b[at] = byte
    return bytes(b)


_fail("name_len0", raw(name=b"", rnl=0), NO_NAME, name_len=0)
_fail("name_len1", raw(name=b"\0", rnl=1), EMPTY_NAME, name_len=1)
# l_read_name 0 / 1 read no name byte: the op is the word right after the fixed fields
_fail("name_len0_bad_op", raw(name=b"", rnl=0, ops=(9,)), NO_NAME | BAD_OP)
_fail("name_len1_bad_op", raw(name=b"", rnl=1, ops=(9,), extra=b"\0"), EMPTY_NAME | BAD_OP)
_fail("name_len1_op_behind_nul", raw(name=b"\0", rnl=1, ops=(9,)), EMPTY_NAME)   # the op read: 00 09 00 00
_fail("name_len0_mapped_empty", raw(name=b"", rnl=0, flag=0), NO_NAME | MAPPED_CIGAR | MAPPED_SEQ)
for _n in NAME_LENGTHS[2:]:
    _pass(f"name_len{_n}", raw(name=name_of(_n)), name_len=_n)
    _fail(f"name_len{_n}_no_nul", raw(name=name_of(_n, nul=False)), NO_NUL, name_len=_n)
    for _k, _at in enumerate(a for a in BAD_AT if a < _n - 1):
        # '@' at every position (it lies inside the allowed range's gap), and the other bad values in turn
        for _b in (0x40, [b for b in BAD_BYTES if b != 0x40][(_k + _n) % 5]):
            _fail(f"name_len{_n}_bad{_b:02x}_at{_at}", raw(name=name_of(_n, _at, _b)), NON_ASCII, name_len=_n,
                  bad_at=_at, bad_byte=_b)
for _b in BAD_BYTES:
    for _at in (0, 32):
        if not any(p.label == f"name_len34_bad{_b:02x}_at{_at}" for p in PROBES):
            _fail(f"name_len34_bad{_b:02x}_at{_at}", raw(name=name_of(34, _at, _b)), NON_ASCII, name_len=34,
                  bad_at=_at, bad_byte=_b)
for _b in EDGE_OK_BYTES:
    for _at in (0, 31, 32, 48):
        _pass(f"name_len50_ok{_b:02x}_at{_at}", raw(name=name_of(50, _at, _b)), ok_byte=_b)
_fail("name_no_nul_and_bad", raw(name=b"@\x7fB"), NO_NUL)                        # else-if: one flag
_fail("name_at", raw(name=b"@A\0"), NON_ASCII)
_fail("name_del", raw(name=b"\x7fA\0"), NON_ASCII)
_fail("name_space", raw(name=b" A\0"), NON_ASCII)
_fail("name_AB", raw(name=b"AB"), NO_NUL)
for _n in (2, 33):
    _pass(f"name_len{_n}_bad_past_nul", raw(name=name_of(_n), extra=b"\x40\x00\xff\x20"), past_nul=_n)
_fail("name_inner_nul", raw(name=b"A\0B\0"), NON_ASCII)                          # a NUL before the last byte

# ----------------------------------------------------------------------------- CIGAR
OP_COUNTS = (0, 1, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 1100, 65535)
BAD_OP_AT = (0, 7, 8, 15, 16, 63, 64)


def op(k, bad=False):
    """Op word k: the low nibble 0..8 (valid) or 9 (bad); every other nibble of the word is above
    8, so a scan that looks at the wrong byte of a word sees an invalid op."""
    return 0x9A9BFC00 | ((k * 7) & 0xF) << 4 | (9 if bad else k % 9)


def ops_of(n, bad_at=None):
    return tuple(op(k, k == bad_at) for k in range(n))


HEAVY = []   # probes too long for the layouts without a tail
for _n in OP_COUNTS[:-2]:
    _pass(f"cigar{_n}", raw(ops=ops_of(_n)), n_ops=_n, bad_op=None)
    for _at in sorted(set(a for a in BAD_OP_AT if a < _n) | ({_n - 1} if _n else set())):
        _fail(f"cigar{_n}_bad_at{_at}", raw(ops=ops_of(_n, _at)), BAD_OP, n_ops=_n, bad_op=_at, last=_at == _n - 1)
# 1100 ops (4.4 KB a probe), with names that put the end of name + CIGAR on the 16-byte grid the
# staged windows end on: 36 + 252 + 4400 = 4688 = 16 * 293, 4689 one past it, 36 + 240 + 4400 = 4676
_pass("cigar1100", raw(name=name_of(252), ops=ops_of(1100)), n_ops=1100, bad_op=None)
_pass("cigar1100_name253", raw(name=name_of(253), ops=ops_of(1100)), n_ops=1100, bad_op=None)
_fail("cigar1100_bad_at1099", raw(name=name_of(240), ops=ops_of(1100, 1099)), BAD_OP, n_ops=1100, bad_op=1099, last=True)
_fail("cigar65535_bad_last", raw(ops=ops_of(65535, 65534)), BAD_OP, n_ops=65535, bad_op=65534, last=True)
HEAVY.append(PROBES.pop())
_pass("cigar_op_nibble8", raw(ops=(0x18,)), nibble=8)
_fail("cigar_op_nibble9", raw(ops=(0x19,)), BAD_OP, nibble=9)
_pass("cigar_op_ffffff08", raw(ops=(0xFFFFFF08,)), high_ff=8)
_fail("cigar_op_ffffff09", raw(ops=(0xFFFFFF09,)), BAD_OP, high_ff=9)
_fail("cigar_op_0f", raw(ops=(0x0F,)), BAD_OP)
# long_candidate: block_size >= 2048 with >= 32 ops leaves the eager check to a whole wave
for _bs in (2047, 2048):
    for _n in (31, 32, 33):
        _x = b"\x55" * (_bs - 34 - 4 * _n)
        _pass(f"long_bs{_bs}_ops{_n}", raw(ops=ops_of(_n), extra=_x), long_bs=(_bs, _n))
        if _bs == 2048:
            _fail(f"long_bs{_bs}_ops{_n}_bad_last", raw(ops=ops_of(_n, _n - 1), extra=_x), BAD_OP, long_bs=(_bs, _n))
        if _n == 32:
            _fail(f"long_bs{_bs}_ops{_n}_bad_name", raw(name=b"\x40\0", ops=ops_of(_n), extra=_x), NON_ASCII)
assert all(struct.unpack_from("<i", p.data)[0] == int(p.label[7:11]) for p in PROBES if p.label.startswith("long_bs"))
# A long candidate that passes and is abnormal (l_seq -1000: implied 32 + 2 + 2048 - 1499 = 583; 512 ops
# end at 2086, past the nominal end 2052), so the window cannot walk its chain and the eager
# checker's whole-wave walk reads the second record, at the cursor: one bad name byte there (each
# bound of the allowed ranges from outside) is nonASCIIReadName with n = 1
for _b in (0x20, 0x40, 0x7F):
    _fail(f"long_then_name_bad{_b:02x}", raw(bs=2048, lseq=-1000, ops=ops_of(512)) + raw(name=bytes([0x41, _b, 0])),
          NON_ASCII, n=1, follow=RUNWAY, second_name=_b, abnormal=True)
# the mapped / empty rule and its field swap
_fail("mapped_no_cigar_no_seq", raw(flag=0), MAPPED_CIGAR | MAPPED_SEQ, swap="both")
_fail("mapped_no_cigar", raw(flag=0, lseq=5, extra=b"\0" * 8), MAPPED_SEQ, swap="n_cigar == 0")
_fail("mapped_no_seq", raw(flag=0, ops=(0x10,)), MAPPED_CIGAR, swap="l_seq == 0")
_pass("mapped_ok", raw(flag=0, lseq=1, ops=(0x10,), extra=b"\x10\x20"), swap="neither")
_pass("unmapped_no_cigar_no_seq_flag_ffff", raw(flag=0xFFFF), swap="flag 4 set")
_fail("mapped_flag_fffb", raw(flag=0xFFFB), MAPPED_CIGAR | MAPPED_SEQ, swap="flag 4 clear")
_fail("mapped_no_seq_bad_op", raw(flag=0, ops=(0x19,)), BAD_OP)                  # the op error wins

# ----------------------------------------------------------------------------- arithmetic
# implied = 32 + l_read_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq (Java int: / truncates to 0, + wraps)
#   l_seq -1:          0 / 2 - 1 = -1                                   implied 33
#   l_seq -1000:       -999 / 2 - 1000 = -499 - 1000 = -1499            implied -1465
#   l_seq 0x7FFFFFFF:  (-2^31) / 2 + (2^31 - 1) = 2^30 - 1              implied 1073741857
#   l_seq 0x80000000:  (-2^31 + 1) / 2 - 2^31 = -1073741823 - 2^31 -> wraps to 1073741825; implied 1073741859
#   l_seq 0x55555555:  0x2AAAAAAB + 0x55555555 = 0x80000000 -> -2^31    implied negative: every block_size passes
#   l_seq 0x55555520:  0x2AAAAA90 + 0x55555520 = 0x7FFFFFB0             implied 0x7FFFFFD2
_fail("implied_minus_1", raw(bs=33), IMPLIED, arith="block_size implied - 1")
_pass("implied_lseq5", raw(lseq=5, extra=b"\0" * 8), arith="block_size implied")
_fail("implied_lseq5_minus_1", raw(bs=41, lseq=5, extra=b"\0" * 8), IMPLIED, arith="block_size implied - 1")
_pass("lseq_m1", raw(bs=33, lseq=-1), arith="l_seq -1", abnormal=True)
_fail("lseq_m1_short", raw(bs=32, lseq=-1), IMPLIED, arith="l_seq -1")
_pass("lseq_m1000", raw(bs=-1465, lseq=-1000), arith="l_seq -1000", abnormal=True)
_fail("lseq_m1000_short", raw(bs=-1466, lseq=-1000), IMPLIED, arith="l_seq -1000")
# a first record that passes with a nominal end far past the stream: the skip clamps at the
# stream's end, which is not the nominal start: tooFewFixedBlockBytes after one record
_fail("lseq_max", raw(bs=1073741857, lseq=0x7FFFFFFF), FIXED, n=1, arith="l_seq 0x7FFFFFFF")
_fail("lseq_max_short", raw(bs=1073741856, lseq=0x7FFFFFFF), IMPLIED, arith="l_seq 0x7FFFFFFF")
_fail("lseq_max_bs_max", raw(bs=I32_MAX, lseq=0x7FFFFFFF), FIXED, n=1, arith="l_seq 0x7FFFFFFF")
_fail("lseq_min", raw(bs=1073741859, lseq=0x80000000), FIXED, n=1, arith="l_seq 0x80000000")
_fail("lseq_min_short", raw(bs=1073741858, lseq=0x80000000), IMPLIED, arith="l_seq 0x80000000")
_pass("lseq_wrap", raw(lseq=0x55555555), arith="implied wraps negative")
_fail("lseq_no_wrap", raw(lseq=0x55555520), IMPLIED, arith="implied 0x7FFFFFD2")
_fail("bs_max", raw(bs=I32_MAX), FIXED, n=1, arith="block_size 0x7FFFFFFF")
_fail("bs_zero", raw(bs=0), IMPLIED)
_fail("bs_negative", raw(bs=-1), IMPLIED)

# ----------------------------------------------------------------------------- abnormal records
# ABN: l_seq -1, block_size 33: nominal end = start + 37, the cursor after 'A\0' = start + 38.
ABN = raw(bs=33, lseq=-1)
assert len(ABN) == 38
# two of them, then runway: every later record is read where the cursor stands
PROBES.append(Probe("abnormal_two_then_runway", ABN + ABN, RUNWAY, "BIG", 2, ("more",), dict(abnormal=True)))
# the cursor (76) is past the nominal start (74) of a record that fails: flags with n = 2
_fail("abnormal_two_then_bad", ABN + ABN + raw(ref=-2), NEG_IDX, n=2, abnormal=True)

# ----------------------------------------------------------------------------- end of stream
# Each is laid at the end of a first segment (an empty BGZF member and more data behind it) and at
# the end of the file.  Byte counts from the probe's first byte:
_end("end_clean_1", MIN, 1, ("end",), clean=1)
_end("end_clean_2", MIN * 2, 2, ("end",), clean=2)
_end("end_clean_9", MIN * 9, 9, ("end",), clean=9)
_end("end_1_past", MIN + b"\0", 1, ("flags", FIXED), past=1)
_end("end_35_past", MIN + MIN[:35], 1, ("flags", FIXED), past=35)
_end("end_cut_fixed", MIN[:20], 0, ("flags", FIXED), cut="fixed")
_end("end_cut_fixed_35", MIN[:35], 0, ("flags", FIXED), cut="fixed")
_end("end_minimal_one_short", MIN[:37], 0, ("flags", NAME_EOF), cut="name")
_end("end_cut_name", raw(name=b"ABCD\0", ops=(0x19,))[:38], 0, ("flags", NAME_EOF), cut="name")
# tooFewBytesForReadName: the CIGAR tests (mapped / empty among them) are not made
_end("end_cut_name_mapped_empty", raw(flag=0, name=b"ABCD\0")[:39], 0, ("flags", NAME_EOF), cut="name")
_end("end_cut_name_refpos", raw(ref=-2, bs=0, name=b"ABCD\0")[:36], 0, ("flags", NEG_IDX | IMPLIED | NAME_EOF), cut="name")
_end("end_cut_between_ops", raw(ops=(0x10, 0x10))[:42], 0, ("flags", CIGAR_EOF), cut="between ops")
_end("end_cut_inside_op", raw(ops=(0x10, 0x10))[:44], 0, ("flags", CIGAR_EOF), cut="inside op")
# the ops are tested in order: a bad op before the cut is invalidCigarOp, one behind it is not reached
_end("end_bad_op_then_cut", raw(ops=(0x19, 0x10))[:44], 0, ("flags", BAD_OP), order="bad op first")
_end("end_cut_then_bad_op", raw(ops=(0x10, 0x19))[:45], 0, ("flags", CIGAR_EOF), order="cut first")
_end("end_no_name_cut_op", raw(bs=36, name=b"", rnl=0, nc=1), 0, ("flags", NO_NAME | CIGAR_EOF), order="noReadName, cut op")
_end("end_empty_name_cut_op", raw(bs=37, name=b"\0\0", rnl=1, nc=1), 0, ("flags", EMPTY_NAME | CIGAR_EOF))
# abnormal chains.  ABN + MIN: MIN is read at 38 and counted from 37, its nominal end 75, the
# cursor 76 = the stream's end: not the nominal start -> tooFewFixedBlockBytes, n = 2
_end("end_abnormal_min", ABN + MIN, 2, ("flags", FIXED), abnormal=True)
# ABN + a record one byte longer by its block_size (35): read at 38, nominal end 37 + 39 = 76 =
# the cursor: the chain is in step again and the stream ends there -> Success(2)
_end("end_abnormal_resync", ABN + raw(bs=35), 2, ("end",), abnormal=True)
# ABN, ABN (read at 38, counted from 37: nominal end 74, cursor 76), then block_size 36: read at
# 76, nominal end 74 + 40 = 114 = the cursor -> Success(3); with block_size 34: nominal 112, the
# cursor 114 -> tooFewFixedBlockBytes, n = 3
_end("end_abnormal_chain_clean", ABN + ABN + raw(bs=36), 3, ("end",), abnormal=True)
_end("end_abnormal_chain_unclean", ABN + ABN + MIN, 3, ("flags", FIXED), abnormal=True)

# ----------------------------------------------------------------------------- dense sections
# PASS16: with BIG, every 16th position is a record that passes (block_size 0x40000, refID 65,
# pos 0, l_read_name 2, flag 4, l_seq 65, mate 0 / 2, name 'A\0') and whose nominal end lies
# 262148 bytes on: 4 bytes into a later period, where refID 0 / pos 2, l_read_name 0
# (noReadName), flag 0, 65 valid ops, l_seq 0 (emptyMappedCigar), mate refID 2 / pos 0x40000 >
# 1002 (tooLargeNextReadPos) and block_size 65 < 292 (tooFewRemainingBytesImplied) fail with n = 1.
PASS16_UNIT = struct.pack("<IIII", 0x00040000, 0x41, 0, 2)
PASS16_WORD_RTC10 = 1 << N_SHIFT | BIG_NPOS | NO_NAME | MAPPED_CIGAR | IMPLIED
assert PASS16_WORD_RTC10 == 0x151100
PASS16_LEN = 262148 + 3 * FTILE + 1024        # three full tiles whose landing points are PASS16 too, and slack
# CLOSE16: the same with refID 64, so that the name is '@\0': every 16th position fails with
# nonASCIIReadName alone (a close call: one non-zero field), 512 in a tile, twice FCCAP.
CLOSE16_UNIT = struct.pack("<IIII", 0x00040000, 0x40, 0, 2)
CLOSE16_WORD = NON_ASCII
CLOSE16_LEN = FTILE + 512
# OPS11: bytes 0x11 (refID 0x11111111: tooLargeReadIdx and ...NextReadIdx, l_read_name 17 with no
# NUL, n_cigar 4369 of a mapped read, block_size below implied) with single bytes 0x19.
OPS11_WORD, OPS11_OPS, OPS11_CIGAR_AT = BIG_IDX | BIG_NIDX | NO_NUL | IMPLIED, 4369, 36 + 17
assert OPS11_WORD == 0x40444
OPS11_LEN = 288 * 1024                       # >= 3 * FTILE + 270000, whole 1 KiB lines
OPS11_GROUP = 26 * 1024                      # bad bytes this far apart never share a CIGAR (17476 bytes)
OPS11_LINE_OFFSETS = (30, 31, 32, 33, 1023, 1024, 1025, 1026, FSN - 1, FSN)  # relative to a 1 KiB line


def ops11_bad(start):
    """Flats of the 0x19 bytes of an OPS11 section starting at `start`."""
    line = (start + 20480 + 1023) & ~1023
    return tuple(line + k * OPS11_GROUP + o for k, o in enumerate(OPS11_LINE_OFFSETS))


def ops11_word(p, bad):
    """The literal rule at an OPS11 position p none of whose 53 header / name bytes is a bad byte."""
    hit = any(0 <= b - (p + OPS11_CIGAR_AT) < 4 * OPS11_OPS and (b - (p + OPS11_CIGAR_AT)) % 4 == 0 for b in bad)
    return OPS11_WORD | (BAD_OP if hit else 0)


# ----------------------------------------------------------------------------- layouts
Layout = namedtuple("Layout", "kind ctg shift flat segments probes sections contigs")
# segments: (begin, end) flat ranges; probes: (Probe, flat of its first byte); sections: name -> (begin, end)


def bam_header(contigs):
    out = b"BAM\1" + struct.pack("<ii", 0, len(contigs))
    for i, ln in enumerate(contigs):
        nm = b"%x\0" % i
        out += struct.pack("<i", len(nm)) + nm + struct.pack("<i", ln)
    return out


def _pad16(n):
    return bytes([FILL]) * (-n % 16)


@functools.lru_cache(maxsize=None)
def layout(kind, ctg, shift=0):
    """kind 'long' | 'short' | 'segmented'; ctg 'SMALL' | 'BIG'; shift: extra bytes (0..15) before the
    first probe, so that every probe starts at flat = shift (mod 16)."""
    hdr = bam_header(DICTS[ctg])
    out = bytearray(hdr)
    out += MIN * (EW // 38 + 1)                         # front pad of at least EW: a chain from the header
    out += _pad16(len(out)) + bytes([FILL]) * shift
    probes, sections = [], {}
    mine = [p for p in PROBES if p.ctg == ctg] + (HEAVY if kind == "long" and ctg == "BIG" and shift == 0 else [])
    for p in mine:
        assert len(out) % 16 == shift
        probes.append((p, len(out)))
        out += p.data + p.follow
        out += _pad16(len(out) - shift)
    segments = None
    if ctg == "BIG" and shift == 0:
        a = len(out)
        out += CLOSE16_UNIT * (CLOSE16_LEN // 16)
        sections["CLOSE16"] = (a, len(out))
    if kind == "long":
        if ctg == "BIG" and shift == 0:
            out += bytes([FILL]) * (-len(out) % 1024)
            a = len(out)
            body = bytearray(b"\x11" * OPS11_LEN)
            for b in ops11_bad(a):
                body[b - a] = 0x19
            out += body
            sections["OPS11"] = (a, len(out))
        a = len(out)
        out += PASS16_UNIT * (PASS16_LEN // 16)         # the tail every tile before it is fast against
        sections["PASS16"] = (a, len(out))
        out += RUNWAY
    elif kind == "segmented":
        segments = [(0, len(out)), (len(out), len(out) + 300 * len(MIN))]
        out += MIN * 300
    return Layout(kind, ctg, shift, bytes(out), segments or [(0, len(out))], tuple(probes), sections,
                  DICTS[ctg])


def compress(lay, payload, level=6, cuts=()):
    """The layout as BGZF members of `payload` bytes; an empty member closes each segment.  cuts:
    flat offsets where a member must end as well."""
    out = []
    for a, b in lay.segments:
        edges = sorted({a, b} | {c for c in cuts if a < c < b})
        out += [bgzf(lay.flat[x:y], payload, level)[:-len(EOF_MEMBER)] for x, y in zip(edges, edges[1:])]
        out.append(EOF_MEMBER)
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def end_layout(label):
    """An end case twice: at the end of a first segment (empty member, then more data) and at the
    end of the file.  Runway records lead up to it in both, so that positions before it chain in."""
    p = next(c for c in END_CASES if c.label == label)
    seg1 = bam_header(BIG) + MIN * 20
    seg1 += _pad16(len(seg1))
    seg2 = MIN * 7 + bytes([FILL]) * 3
    probes = ((p, len(seg1)), (p, len(seg1) + len(p.data) + len(seg2)))
    flat = seg1 + p.data + seg2 + p.data
    cut = len(seg1) + len(p.data)
    return Layout("end", "BIG", 0, flat, [(0, cut), (cut, len(flat))], probes, {}, BIG)


def fast_tile(lay, s0):
    """k_full's fast-tile condition for the tile at s0, for a call whose range holds the tile."""
    end = next(e for b, e in lay.segments if b <= s0 < e)
    return s0 + FTILE + FULL_FAST_REACH <= end


assert PAYLOADS == (65280, 4096, 97) and EOF_MEMBER


# ----------------------------------------------------------------------------- test helpers
def oracles(lay, payload=65280, level=6):
    """One CPU-oracle stream per segment of the layout: [(OracleFile, first flat of the segment)].
    (For the tests that compare with the oracle; no literal above comes from it.)"""
    from oracle_lib import OracleFile
    data = np.frombuffer(compress(lay, payload, level), np.uint8)
    out, start = [], 0
    for a, b in lay.segments:
        of = OracleFile(data, start=start)
        assert of.flat_size == b - a and bytes(of.uncompressed()) == lay.flat[a:b]
        of.contig_len = np.asarray(lay.contigs, np.int32)     # (a later segment has no header to parse)
        out.append((of, a))
        start = of.blocks[-1][0] + of.blocks[-1][1] + len(EOF_MEMBER)   # past the empty member that closes it
    return out


def tally(words, begin):
    """Counts, reads-before-error histogram, successes and close calls of a run of full words, as
    FullCheck.scala:142-192 aggregates them (test_checker_corpus_cpu.py holds it to the oracle's sums)."""
    pos = np.arange(begin, begin + words.size, dtype=np.uint64)
    ok = (words & SUCCESS) != 0
    w, pos = words[~ok], pos[~ok]
    f, n = w & 0x7FFFF, (w >> 20) & 0x3FF
    keep = ~((f == 1) & (n == 0))
    w, pos, f, n = w[keep], pos[keep], f[keep], n[keep]
    nnz = sum(((f >> b) & 1).astype(np.int64) for b in range(19)) + (n > 0)
    counts, rbe = np.zeros((21, 19), np.int64), np.zeros((21, 64), np.int64)
    for b in range(19):
        np.add.at(counts[:, b], nnz[((f >> b) & 1) == 1], 1)
    m = (n > 0) & (n < 64)
    np.add.at(rbe, (nnz[m], n[m].astype(np.int64)), 1)
    close = set(zip(pos[nnz <= 2].tolist(), w[nnz <= 2].tolist()))
    return counts, rbe, int(ok.sum()), close
