"""Deflate writer conformance on the GPU: the hand-built corpus (tests/zdeflate_corpus.py, one case
per named edge of k_zprev / k_zinfo / k_zparse / k_ztrees / k_zemit) through sbh_bgzf_compress_level,
byte for byte against libz 1.2.11 driven like htsjdk's Deflater (test_zdeflate_cpu.htsjdk_member) --
never against the project's own host build.  tests/test_zdeflate_corpus_cpu.py proves on the CPU
that every case reaches the edge it is named for.

Also: every full-size case as the middle member of three (its base b * 65498 is not dword-aligned
and its neighbours share the batch's scratch), compression from device pointers at every byte
alignment, and the library's own FAST coder (level -1) over the same corpus.  FAST has no external
byte reference: it is held to the host build of the same coder (test_deflate_cpu.compress) and to
every member inflating back to its payload with zlib, and to nothing more."""
import numpy as np
import pytest

import zdeflate_corpus as zc
from deflate_build import Bits, member_of, stored_block
from pkg import sb
from test_deflate_cpu import compress as fast_host, parse_members
from test_zdeflate_cpu import EOF_MEMBER, PAYLOAD, htsjdk_bgzf, htsjdk_member

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


def guarded(f, *a, **k):
    try:
        return f(*a, **k)
    except sb.SparkBamError as e:
        if e.code == 2:  # SBH_E_HIP: a device error -- nothing more runs on this GPU
            pytest.exit("HIP error: %s" % e, returncode=3)
        raise


def gpu(ctx, data, level, nbytes=None):
    src = data if isinstance(data, int) else np.frombuffer(bytes(data), dtype=np.uint8)
    got, nb, _ = guarded(ctx.bgzf_compress, src, nbytes, level)
    return got.tobytes(), nb


@pytest.mark.parametrize("p", zc.pairs(), ids=zc.pair_id)
def test_case(ctx, p):
    c, level = p
    got, nb = gpu(ctx, c.data, level)
    assert nb == 1 and got == htsjdk_member(c.data, level) + EOF_MEMBER


@pytest.mark.parametrize("p", [(c, lv) for c in zc.FULL for lv in c.levels], ids=zc.pair_id)
def test_placement(ctx, p):
    """The case as member 1 of three: its bytes start at offset 65498 (2 mod 4) of the input."""
    c, level = p
    data = bytes(zc.noisy(70, PAYLOAD)) + c.data + bytes(zc.noisy(71, 30001))
    got, nb = gpu(ctx, data, level)
    assert nb == 3 and got == htsjdk_bgzf(data, level)


def stored_bgzf(data):
    """`data` as a BGZF file of stored-block members (inflating it leaves `data` in the shard)."""
    out = b""
    for o in range(0, len(data), 60000):
        w = Bits()
        stored_block(w, data[o:o + 60000], True)
        out += member_of(w.bytes(), data[o:o + 60000])
    return out + EOF_MEMBER


@pytest.fixture(scope="module")
def flat(ctx):
    """slide_32768 and m258_dst_0 back to back, inflated into a shard: (device pointer, bytes)."""
    data = zc.BY_NAME["slide_32768"].data + zc.BY_NAME["m258_dst_0"].data
    sh = ctx.shard(np.frombuffer(stored_bgzf(data), dtype=np.uint8).copy())
    try:
        _, n = guarded(sh.index, 0)
        guarded(sh.inflate)
        assert n == len(data) and bytes(sh.read_flat(0, n)) == data
        yield sh.flat_ptr(), data
    finally:
        sh.close()


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("end", [0, 1, 2, 3])
def test_device_pointer_alignment(ctx, flat, k, end):
    """Two members compressed from flat_ptr() + k, with ptr + n at residue `end` (mod 4): k_zinfo
    re-aligns the source dwords by ptr & 3 and guards its last read by the buffer's end."""
    ptr, data = flat
    n = len(data) - k - 4
    n += (end - (ptr + k + n)) % 4
    assert (ptr + k + n) % 4 == end and k + n <= len(data) and n > PAYLOAD
    got, nb = gpu(ctx, ptr + k, 5, nbytes=n)
    assert nb == 2 and got == htsjdk_bgzf(data[k:k + n], 5)


@pytest.mark.parametrize("c", zc.CASES, ids=lambda c: c.name)
def test_fast_coder(ctx, c):
    """level -1, the library's own coder: equal to its host build, and every member inflates (zlib)
    to its payload with a sound frame, CRC32 and ISIZE."""
    got, nb = gpu(ctx, c.data, -1)
    assert nb == 1 and got == fast_host(c.data)
    ms = parse_members(got)
    assert len(ms) == 2 and ms[0][3] == c.data and ms[1][2] == 0
