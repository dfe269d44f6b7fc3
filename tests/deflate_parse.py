"""A token-level reader for raw DEFLATE (RFC 1951) streams -- TEST INFRASTRUCTURE, the inverse of
deflate_build.py: raw bytes -> [Block].  It shows what a compressor did with an input (which
block types it chose, which matches it took, how wide its codes came out), so that a test case
built to reach one edge of the writer can prove that it does.

Tokens are deflate_build's: an int is a literal byte, (length, distance) a match; a stored block's
bytes are its tokens too, so deflate_build.expand(all tokens) is the stream's payload.
"""
from deflate_build import (CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_DIST_LENS, FIXED_LIT_LENS, LEN_BASE, LEN_EXTRA,
                           canon)

STORED, FIXED, DYNAMIC = "stored", "fixed", "dynamic"


class Block:
    """One deflate block.  kind: STORED / FIXED / DYNAMIC; final: BFINAL; tokens; start / end: bit
    offsets of the block's first bit and of the first bit after it; data_byte: a stored block's
    first payload byte offset in the stream.  Dynamic blocks also carry hlit / hdist / hclen (the
    counts, not the header fields), cl_lens (19), cl_syms (the code-length symbols as sent, 0..18),
    lit_lens (hlit), dist_lens (hdist), header_bits
    (everything before the first symbol) and widths (bits of each token, extra bits included)."""

    def __init__(self, kind, final, start):
        self.kind, self.final, self.start, self.end = kind, final, start, start
        self.tokens, self.widths = [], []
        self.hlit = self.hdist = self.hclen = None
        self.cl_lens = self.cl_syms = self.lit_lens = self.dist_lens = None
        self.header_bits = 3
        self.eob_bits = 0
        self.data_byte = None

    @property
    def nsyms(self):
        return len(self.tokens)

    def matches(self):
        return [t for t in self.tokens if isinstance(t, tuple)]


class _Reader:
    def __init__(self, raw):
        self.raw, self.pos = bytes(raw) + bytes(8), 0
        self.nbits = 8 * len(raw)

    def peek(self, n):
        i = self.pos >> 3
        return (int.from_bytes(self.raw[i:i + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def get(self, n):
        v = self.peek(n)
        self.pos += n
        if self.pos > self.nbits:
            raise ValueError("deflate stream ends inside a block")
        return v


def _table(lens):
    """LSB-first lookup of a canonical code: (table of (symbol, length) indexed by the next
    `width` bits, width).  Incomplete codes leave None entries."""
    width = max(lens) if any(lens) else 1
    tab = [None] * (1 << width)
    for s, c in enumerate(canon(list(lens))):
        if c is None:
            continue
        code, ln = c
        rev = int(format(code & ((1 << ln) - 1), "0%db" % ln)[::-1], 2)
        for hi in range(1 << (width - ln)):
            tab[rev | hi << ln] = (s, ln)
    return tab, width


def _sym(r, tab):
    e = tab[0][r.peek(tab[1])]
    if e is None:
        raise ValueError("no such code at bit %d" % r.pos)
    r.pos += e[1]
    if r.pos > r.nbits:
        raise ValueError("deflate stream ends inside a block")
    return e[0]


_FIXED = None


def _tokens(r, b, lt, dt):
    tokens, widths = b.tokens, b.widths
    while True:
        p0 = r.pos
        s = _sym(r, lt)
        if s < 256:
            tokens.append(s)
        elif s == 256:
            b.eob_bits = r.pos - p0
            return
        else:
            if s > 285:
                raise ValueError("length symbol %d" % s)
            ln = LEN_BASE[s - 257] + r.get(LEN_EXTRA[s - 257])
            ds = _sym(r, dt)
            if ds > 29:
                raise ValueError("distance symbol %d" % ds)
            tokens.append((ln, DIST_BASE[ds] + r.get(DIST_EXTRA[ds])))
        widths.append(r.pos - p0)


def parse(raw, max_blocks=None):
    """Every block of the raw deflate stream `raw` (or its first max_blocks), which must end with
    its final block's last byte (ValueError otherwise, or on any invalid code)."""
    global _FIXED
    r, out = _Reader(raw), []
    while True:
        start = r.pos
        final, kind = r.get(1), r.get(2)
        if kind == 0:
            b = Block(STORED, bool(final), start)
            r.pos = (r.pos + 7) & ~7
            n, nn = r.get(16), r.get(16)
            if n ^ nn != 0xffff:
                raise ValueError("stored LEN / NLEN disagree")
            b.header_bits = r.pos - start
            b.data_byte = r.pos >> 3
            b.tokens = list(r.raw[b.data_byte:b.data_byte + n])
            r.pos += 8 * n
            if r.pos > r.nbits:
                raise ValueError("stored block past the end")
        elif kind == 1:
            b = Block(FIXED, bool(final), start)
            if _FIXED is None:
                _FIXED = _table(FIXED_LIT_LENS), _table(FIXED_DIST_LENS)
            _tokens(r, b, *_FIXED)
        elif kind == 2:
            b = Block(DYNAMIC, bool(final), start)
            b.hlit, b.hdist, b.hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
            b.cl_lens = [0] * 19
            for i in range(b.hclen):
                b.cl_lens[CL_ORDER[i]] = r.get(3)
            ct = _table(b.cl_lens)
            lens, b.cl_syms = [], []
            while len(lens) < b.hlit + b.hdist:
                s = _sym(r, ct)
                b.cl_syms.append(s)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    if not lens:
                        raise ValueError("repeat with no previous length")
                    lens += [lens[-1]] * (3 + r.get(2))
                elif s == 17:
                    lens += [0] * (3 + r.get(3))
                else:
                    lens += [0] * (11 + r.get(7))
            if len(lens) != b.hlit + b.hdist:
                raise ValueError("code lengths overrun")
            b.lit_lens, b.dist_lens = lens[:b.hlit], lens[b.hlit:]
            b.header_bits = r.pos - start
            _tokens(r, b, _table(b.lit_lens), _table(b.dist_lens))
        else:
            raise ValueError("reserved block type")
        b.end = r.pos
        out.append(b)
        if final:
            break
        if max_blocks is not None and len(out) >= max_blocks:
            return out
    if (r.pos + 7) >> 3 != len(raw):
        raise ValueError("%d bytes after the final block" % (len(raw) - ((r.pos + 7) >> 3)))
    return out


def all_tokens(blocks):
    return [t for b in blocks for t in b.tokens]


def payload(blocks):
    """The bytes the blocks stand for, independent of zlib (deflate_build.expand's result, copied a
    match at a time; ValueError when a distance reaches before the first byte)."""
    out = bytearray()
    for b in blocks:
        if b.kind == STORED:
            out += bytes(b.tokens)
            continue
        for t in b.tokens:
            if isinstance(t, tuple):
                ln, d = t
                if d > len(out):
                    raise ValueError("distance %d at offset %d" % (d, len(out)))
                if d >= ln:
                    out += out[len(out) - d:len(out) - d + ln]
                else:
                    out += (bytes(out[-d:]) * (ln // d + 1))[:ln]
            else:
                out.append(t)
    return bytes(out)


def positions(blocks):
    """[(payload offset, token)] of every token."""
    out, p = [], 0
    for t in all_tokens(blocks):
        out.append((p, t))
        p += t[0] if isinstance(t, tuple) else 1
    return out
