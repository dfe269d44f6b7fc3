"""The deflate writer's conformance corpus (tests/zdeflate_corpus.py) pinned with no GPU: on every
case and level the host definition (zdeflate_core.h, tools/libzdeflate_host.so) gives libz's bytes
-- through java.util.zip.Deflater's single call and through compress() + flush() -- the parsed
tokens expand to the payload, and the case's structural property holds: read from zlib's parsed
stream (tests/deflate_parse.py) or, where zlib's bytes cannot show it, from the host definition's
trace.  A case that stops reaching its edge after a generator is edited fails here.
tests/test_zdeflate_conformance_gpu.py runs the kernels over the same corpus."""
import zlib

import pytest

import deflate_parse as dp
import zdeflate_corpus as zc
from conftest import golden_bam
from deflate_build import expand
from test_zdeflate_cpu import host_lib, host_raw, jdk_deflate, members, zlib_raw


@pytest.mark.parametrize("name", ["2.bam", "1.bam", "2.100-1000.bam", "1.2203053-2211029.bam", "5k.bam",
                                  "1.block-aligned.bam"])
def test_parser_on_golden_members(name):
    """deflate_parse's own check: every member of the golden BAMs parses, and its tokens expand to
    what zlib inflates."""
    for i, (u, raw) in enumerate(members(golden_bam(name))):
        blocks = dp.parse(raw)
        assert dp.payload(blocks) == u == zlib.decompress(raw, -15), (name, i)
        assert blocks[-1].final and not any(b.final for b in blocks[:-1])
        for b in blocks:
            assert b.end - b.start == b.header_bits + sum(b.widths) + b.eob_bits or b.kind == dp.STORED


def test_parser_agrees_with_expand():
    """payload() copies a match at a time; deflate_build.expand goes byte by byte."""
    for name in ("dist_cap15", "window_jumps", "final_empty"):
        blocks = dp.parse(zlib_raw(zc.BY_NAME[name].data, 5))
        assert dp.payload(blocks) == bytes(expand(dp.all_tokens(blocks))) == zc.BY_NAME[name].data


@pytest.mark.parametrize("p", zc.pairs(), ids=zc.pair_id)
def test_case(p):
    c, level = p
    host_lib()
    v = zc.View(c, level)
    h = host_raw(c.data, level)
    assert h == zlib_raw(c.data, level) == v.raw
    d, done = jdk_deflate(c.data, level, out_cap=2 * len(c.data) + 1024)
    assert done and d == h
    assert dp.payload(v.blocks) == c.data
    c.check(v)
    # the trace is the host definition's: its tokens are zlib's wherever zlib's stream shows them
    t, k = v.trace.tokens(), 0
    assert len(v.trace.blocks) == len(v.blocks)
    for b, row in zip(v.blocks, v.trace.blocks):
        assert {dp.STORED: zc.ZB_STORED, dp.FIXED: zc.ZB_STATIC, dp.DYNAMIC: zc.ZB_DYN}[b.kind] == row[5]
        if b.kind != dp.STORED:
            assert b.tokens == t[row[0]:row[1]]


REQUIRED = """len_1 len_2 len_3 len_4 len_66 len_67 len_130 step_one_hash pair_63_64 hash_every_step same_hash_cmp
m258_dst_-258 m258_dst_-257 m258_dst_-1 m258_dst_0 m258_dst_-100 m258_src_-258 m258_src_-257 m258_src_-1 m258_src_0
m258_src_-100 dist_head_a dist_head_b chain_cut two_nice end_lookahead chain_positions quarter_chain defer3 max_lazy
too_far window_jumps tokens_1 tokens_63 tokens_64 tokens_65 tokens_128 tokens_255 tokens_256 tokens_257 tokens_16447
sym16383_match final_empty slide_32767 slide_32768 slide_32769 pending_literal no_match_block one_dist_code static_tie
dsd_phase_0 dsd_phase_1 dsd_phase_2 dsd_phase_3 dsd_phase_4 dsd_phase_5 dsd_phase_6 dsd_phase_7 dist_cap15
bl_cap7 lit_cap15 fallback_65516 fallback_65517 fallback_65518""".split()


def test_corpus_is_complete():
    """Every case the suite was written for is there, once, under the member size, with its levels;
    what the bounded searches did not find is stated, not faked."""
    assert not [n for n in REQUIRED if n not in zc.BY_NAME]
    for c in zc.CASES:
        assert c.why and 0 < len(c.data) <= zc.PAYLOAD
        assert set(c.levels) <= {4, 5, 6, 7, 8, 9} and (len(c.data) < zc.SMALL or not {8, 9} & set(c.levels))
    assert [c.name for c in zc.FULL] == ["slide_32767", "slide_32768", "slide_32769", "fallback_65516",
                                         "fallback_65518"]
    # no level-5 stream of 65519 bytes exists (see the corpus docstring for why)
    assert zc.FALLBACK_MISSING == [65519]
