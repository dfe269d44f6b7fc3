"""A token-level writer for raw DEFLATE (RFC 1951) streams and BGZF members -- TEST INFRASTRUCTURE.

Tests build compressed streams symbol by symbol with it, valid and invalid, so that a decoder is
fed inputs no compressor writes.  Nothing here checks validity: invalid streams are wanted.

Tokens (a list per deflate block):
  int                       a literal byte
  (length, distance)        a match, coded the way RFC 1951 3.2.5 prescribes (258 is code 285)
  ("L", lsym, lx, dsym, dx) a match by its codes: length symbol lsym (257..) with extra-bit value
                            lx, distance symbol dsym with extra-bit value dx
  ("S", sym)                a bare literal/length symbol's code and nothing else
A symbol that has no code in the block's alphabet is written as one 0 bit.
"""
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163,
            195, 227, 258, 0, 0]  # (286, 287: no base)
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0, 0, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049,
             3073, 4097, 6145, 8193, 12289, 16385, 24577, 0, 0]  # (30, 31: no base)
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13,
              0, 0]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class Bits:
    """An LSB-first bit writer; `n` is the number of bits written so far."""

    def __init__(self):
        self._buf, self._acc, self._k = bytearray(), 0, 0

    @property
    def n(self):
        return len(self._buf) * 8 + self._k

    def put(self, value, nbits):  # LSB first
        self._acc |= (value & ((1 << nbits) - 1)) << self._k
        self._k += nbits
        if self._k >= 64:
            nb = self._k >> 3
            self._buf += (self._acc & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
            self._acc >>= 8 * nb
            self._k -= 8 * nb

    def code(self, c, nbits):  # Huffman codes go most significant bit first
        if nbits:
            self.put(int(format(c & ((1 << nbits) - 1), f"0{nbits}b")[::-1], 2), nbits)

    def align(self):
        self.put(0, -self.n & 7)

    def bytes(self):
        return bytes(self._buf) + self._acc.to_bytes((self._k + 7) // 8, "little")


def canon(lens):
    """Canonical codes (RFC 1951 3.2.2) of a code-length array: (code, length) per symbol, None for
    length 0.  An over-subscribed array gives codes that overflow their length (kept modulo)."""
    cnt = [0] * 17
    for ln in lens:
        cnt[ln] += 1
    cnt[0] = 0
    nxt, c = [0] * 17, 0
    for b in range(1, 16):
        c = (c + cnt[b - 1]) << 1
        nxt[b] = c
    out = []
    for ln in lens:
        if ln:
            out.append((nxt[ln], ln))
            nxt[ln] += 1
        else:
            out.append(None)
    return out


def kraft(lens):
    """Sum of 2^-len over the used symbols, in units of 2^-15 (32768 = complete)."""
    return sum(1 << (15 - ln) for ln in lens if ln)


def _sym(w, codes, s):
    c = codes[s] if s < len(codes) else None
    if c is None:
        w.put(0, 1)
    else:
        w.code(*c)


def len_code(ln):
    return max(i for i in range(29) if LEN_BASE[i] <= ln)


def dist_code(d):
    return max(i for i in range(30) if DIST_BASE[i] <= d)


def write_tokens(w, lc, dc, tokens, eob=True):
    """The tokens (and the end-of-block symbol) in the codes lc (literal/length) and dc (distance)."""
    for t in tokens:
        if isinstance(t, tuple):
            if t[0] == "S":
                _sym(w, lc, t[1])
                continue
            if t[0] == "L":
                _, ls, lx, ds, dx = t
            else:
                ln, d = t
                c, ds = len_code(ln), dist_code(d)
                ls, lx, dx = 257 + c, ln - LEN_BASE[c], d - DIST_BASE[ds]
            _sym(w, lc, ls)
            w.put(lx, LEN_EXTRA[ls - 257])
            _sym(w, dc, ds)
            w.put(dx, DIST_EXTRA[ds])
        else:
            _sym(w, lc, t)
    if eob:
        _sym(w, lc, 256)


def fixed_block(w, tokens, final, eob=True):
    """A block in the fixed code (BTYPE 01)."""
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    write_tokens(w, canon(FIXED_LIT_LENS), canon(FIXED_DIST_LENS), tokens, eob)


def default_cl_lens(used):
    """Lengths of a complete code-length code over the symbols `used` (at most 5 bits)."""
    used = sorted(set(used))
    cl = [0] * 19
    n = len(used)
    if n == 1:
        cl[used[0]] = 1
        cl[(used[0] + 1) % 19] = 1
        return cl
    k = (n - 1).bit_length()
    short = (1 << k) - n  # symbols one bit shorter
    for i, s in enumerate(used):
        cl[s] = k - 1 if i < short else k
    return cl


def dynamic_block(w, lit_lens, dist_lens, tokens, final, *, hlit=None, hdist=None, cl_syms=None, cl_lens=None,
                  hclen=None, eob=True):
    """A block with its own codes (BTYPE 10) from explicit code-length arrays.

    cl_syms: the exact code-length-symbol sequence -- ints 0..15, or (16 | 17 | 18, extra-bit value)
    (default: every length on its own); cl_lens: the 19 code-length-code lengths (default: a
    complete code over the symbols used).  No validity checks.  Returns {"start", "symbols"}: the
    bit positions of the block's first bit and of its first literal/length symbol."""
    start = w.n
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    if hlit is None:
        hlit = max(257, max([i for i, ln in enumerate(lit_lens) if ln] + [0]) + 1)
    if hdist is None:
        hdist = max(1, max([i for i, ln in enumerate(dist_lens) if ln] + [0]) + 1)
    if cl_syms is None:
        cl_syms = (lit_lens + [0] * 320)[:hlit] + (dist_lens + [0] * 32)[:hdist]
    cl_syms = [(s, 0) if isinstance(s, int) else tuple(s) for s in cl_syms]
    if cl_lens is None:
        cl_lens = default_cl_lens(s for s, _ in cl_syms)
    if hclen is None:
        hclen = max(4, max([i for i in range(19) if cl_lens[CL_ORDER[i]]] + [0]) + 1)
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_lens[CL_ORDER[i]], 3)
    clc = canon(cl_lens)
    for s, x in cl_syms:
        _sym(w, clc, s)
        w.put(x, CL_EXTRA.get(s, 0))
    symbols = w.n
    write_tokens(w, canon((lit_lens + [0] * 288)[:288]), canon((dist_lens + [0] * 32)[:32]), tokens, eob)
    return {"start": start, "symbols": symbols}


def stored_block(w, data, final, *, nlen=None):
    """A stored block (BTYPE 00): LEN, NLEN (default: LEN's complement; pass one to make them
    disagree) and the bytes."""
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    for b in bytes(data):
        w.put(b, 8)


def raw_bits(w, value, nbits):
    """Any bits (reserved block types, hand-made corruption)."""
    w.put(value, nbits)


def expand(tokens, out=None):
    """The bytes the tokens stand for, independent of zlib (None when a distance reaches before
    the first byte)."""
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, tuple):
            if t[0] == "L":
                ln, d = LEN_BASE[t[1] - 257] + t[2], DIST_BASE[t[3]] + t[4]
            else:
                ln, d = t
            if d > len(out):
                return None
            if d == 1:
                out += out[-1:] * ln
            else:
                for _ in range(ln):
                    out.append(out[-d])
        else:
            out.append(t)
    return out


def member(raw, isize, crc):
    """The BGZF member around a raw deflate stream, with the footer given."""
    total = 18 + len(raw) + 8
    assert total <= 65536, total
    hdr = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", total - 1)
    return hdr + bytes(raw) + struct.pack("<II", crc & 0xffffffff, isize & 0xffffffff)


def member_of(raw, data):
    """The BGZF member of a stream that inflates to `data`."""
    return member(raw, len(data), zlib.crc32(bytes(data)))


def filler(phase, at=0):
    """A stored-block member placed at file offset `at`, sized so that the first deflate byte of
    the member after it lies at a file offset = phase (mod 4); returns (member, its bytes)."""
    # the filler is 18 + 5 + k + 8 bytes and the next member's deflate bytes start 18 further on
    k = 4 + (phase - (at + 49)) % 4
    data = bytes(range(1, k + 1))
    w = Bits()
    stored_block(w, data, True)
    return member_of(w.bytes(), data), data


def place(members, phase, at=0):
    """The members behind a filler member (at file offset `at`) that puts the first one's first
    deflate byte at a file offset = phase (mod 4): the decoder's bit offset into its first dword."""
    return filler(phase, at)[0] + b"".join(members)


def fixed_member(blocks, isize):
    """A BGZF member of fixed-code deflate blocks (lists of tokens): (member, raw stream, bytes or
    None).  An invalid stream gets ISIZE `isize` and CRC 0 (nothing reads them before the error)."""
    w = Bits()
    for i, toks in enumerate(blocks):
        fixed_block(w, toks, i == len(blocks) - 1)
    raw = w.bytes()
    u = expand([t for b in blocks for t in b])
    data = member(raw, len(u) if u is not None else isize, zlib.crc32(bytes(u)) if u is not None else 0)
    return data, raw, u
