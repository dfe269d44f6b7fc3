"""A hand-built record stream replayed behind a gap of zeros, so that its records lie across a
chosen flat offset -- 2^31 or 2^32 (test infrastructure; plain Python, no GPU).

The record stages are translation invariant: what they produce for a set of records does not
depend on where in the flat stream the records lie; only flat starts, virtual positions and BAI
chunk offsets do.  shift() lays a corpus out as

    the header in its own member(s) | whole 65280-byte zero members, one compressed once and
    replicated | one shorter zero member for the rest | the records in members of a chosen
    payload | the EOF member

with byte `d` of record `k` at flat offset exactly `B`.  The gap is never materialised: a 65280-byte
zero member compresses to about a hundred bytes, so a file whose flat size is 4 GiB is a few MB, and
the member table (compressed offset, compressed length, flat offset, payload length per member) is
arithmetic.  Virtual offsets are remapped on the host through that table (vpos_of, flat_of_vpos,
remap_vpos), so the existing references serve unchanged.

combine() lays several corpora that share a header one after another, each at its own row range,
so that one gap serves them all.
"""
import struct
import zlib
from collections import namedtuple

import numpy as np

from deflate_build import EOF_MEMBER, member_of
import record_corpus as rc

GAP_PAYLOAD = 65280
U64_MAX = (1 << 64) - 1

# data: the file (numpy uint8); shift: new start - old start; starts: the shifted record starts;
# members: int64 [n, 4] rows (compressed offset, compressed length, flat offset, payload length),
# the EOF member included; first: flat start of the first record; flat_size; rec_member: the row
# of `members` that holds the first record byte
Shifted = namedtuple("Shifted", "data shift starts members first flat_size rec_member")


def _member(chunk, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return member_of(c.compress(chunk) + c.flush(), chunk)


def _cut(data, payload, level):
    """[(member bytes, payload length)] of data cut every `payload` bytes."""
    return [(_member(data[o:o + payload], level), len(data[o:o + payload])) for o in range(0, len(data), payload)]


def shift(flat, first, starts, B, k, d, payload=GAP_PAYLOAD, level=6):
    """flat[:first] (the header), a gap of zeros, flat[first:] (the records), laid out so that byte
    d of the record at starts[k] lies at flat offset B.  Returns a Shifted."""
    flat = bytes(flat)
    starts = [int(s) for s in starts]
    P = B - d - starts[k]
    if P < 0:
        raise ValueError("record %d + %d lies past %d already" % (k, d, B))
    n_full, rest = divmod(P, GAP_PAYLOAD)
    head = _cut(flat[:first], GAP_PAYLOAD, level)
    full = _member(bytes(GAP_PAYLOAD), level)
    tail = [(_member(bytes(rest), level), rest)] if rest else []
    recs = _cut(flat[first:], payload, level)
    small = head + tail + recs + [(EOF_MEMBER, 0)]
    at = len(head)  # the whole zero members go in after the header's
    clen = np.asarray([len(m) for m, _ in small], np.int64)
    ulen = np.asarray([u for _, u in small], np.int64)
    clen = np.concatenate((clen[:at], np.full(n_full, len(full), np.int64), clen[at:]))
    ulen = np.concatenate((ulen[:at], np.full(n_full, GAP_PAYLOAD, np.int64), ulen[at:]))
    members = np.stack((np.cumsum(clen) - clen, clen, np.cumsum(ulen) - ulen, ulen), axis=1)
    data = b"".join([m for m, _ in small[:at]] + [full * n_full] + [m for m, _ in small[at:]])
    assert len(data) == int(clen.sum()) and int(ulen.sum()) == len(flat) + P
    return Shifted(np.frombuffer(data, np.uint8), P, [s + P for s in starts], members, first + P, len(flat) + P,
                   len(head) + n_full + len(tail))


def shift_stream(s, B, k, d, payload=GAP_PAYLOAD, level=6):
    """shift() of a record_corpus.Stream."""
    return shift(s.flat, s.first, s.starts, B, k, d, payload, level)


def unshifted(flat, first, starts, payload=GAP_PAYLOAD, level=6):
    """The same layout without a gap: the header's members, then the records' members -- member for
    member the tail of every shift() of the same stream at the same payload."""
    return shift(flat, first, starts, int(starts[0]), 0, 0, payload, level)


def walk(data):
    """The member table from a walk of the file: BSIZE from each member's header, ISIZE from its
    footer; nothing is inflated."""
    data = memoryview(np.ascontiguousarray(data)).cast("B")
    rows, p, f = [], 0, 0
    while p < len(data):
        assert bytes(data[p:p + 4]) == b"\x1f\x8b\x08\x04" and bytes(data[p + 12:p + 14]) == b"BC"
        csize = struct.unpack_from("<H", data, p + 16)[0] + 1
        usize = struct.unpack_from("<I", data, p + csize - 4)[0]
        rows.append((p, csize, f, usize))
        p, f = p + csize, f + usize
    assert p == len(data)
    return np.asarray(rows, np.int64).reshape(-1, 4)


def vpos_of(members, flats):
    """Canonical virtual offsets (uint64) of flat positions: a position at a member's end is (next
    member, 0), empty members hold none, and the end of the stream is the start of what follows the
    last non-empty member."""
    live = members[members[:, 3] > 0]
    f = np.asarray(flats, np.int64).reshape(-1)
    assert f.size == 0 or (f.min() >= 0 and f.max() <= live[-1, 2] + live[-1, 3])
    i = np.searchsorted(live[:, 2], f, side="right") - 1
    within = f - live[i, 2]
    at_end = within == live[i, 3]  # (only past the last byte of the last non-empty member)
    c = np.where(at_end, live[i, 0] + live[i, 1], live[i, 0])
    return (c.astype(np.uint64) << np.uint64(16)) | np.where(at_end, 0, within).astype(np.uint64)


def flat_of_vpos(members, v):
    """Flat positions (int64) of virtual offsets whose member offsets are member starts."""
    v = np.asarray(v, np.uint64).reshape(-1)
    c = (v >> np.uint64(16)).astype(np.int64)
    i = np.searchsorted(members[:, 0], c, side="left")
    assert np.array_equal(members[i, 0], c)
    return members[i, 2] + (v & np.uint64(0xFFFF)).astype(np.int64)


def remap_vpos(old, new, shift_by, v):
    """Virtual offsets of the unshifted file `old` (a member table) as the shifted file `new` has
    them; UINT64_MAX (an untouched linear-index window) stays."""
    v = np.asarray(v, np.uint64)
    out = v.copy().reshape(-1)
    real = out != np.uint64(U64_MAX)
    out[real] = vpos_of(new, flat_of_vpos(old, out[real]) + shift_by)
    return out.reshape(v.shape)


def combine(streams):
    """Streams that share record_corpus.header(), their records laid one after another behind it:
    (the Stream, [(first row, one past the last row)] per input)."""
    hdr = rc.header()
    body, starts, rows = [], [], []
    at = len(hdr)
    for s in streams:  # (anything with .flat and .starts: a Stream, or a corpus module's Case)
        flat = bytes(s.flat)
        assert flat[:len(hdr)] == hdr and list(s.starts) == sorted(set(s.starts))
        rows.append((len(starts), len(starts) + len(s.starts)))
        starts += [int(p) - len(hdr) + at for p in s.starts]
        body.append(flat[len(hdr):])
        at += len(flat) - len(hdr)
    return rc.Stream(hdr + b"".join(body), len(hdr), starts), rows
