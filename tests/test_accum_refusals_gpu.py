"""What the four accumulators (sbh_tally, sbh_stats, sbh_depth, sbh_pileup) refuse, as (status code,
exact text of sbh_last_error): the argument refusals of each create; the refusals every add shares --
a shard of another context, a shard without a records scan, a bad filter -- and, for depth and pileup,
an add after finish; an empty scan, which is SBH_OK with the result preset and the totals untouched;
finish twice, each fetch before finish and each fetch past its span.  Every text is the library's
own, byte for byte; the input is four hand-built records on one span of 50 positions."""
import ctypes as C

import numpy as np
import pytest

from pkg import sb
import pileup_corpus as pc
import record_corpus as rc
from test_depth_gpu import scanned
from test_record_conformance_gpu import call

pytestmark = pytest.mark.gpu

L = sb._lib
OK, E_ARG, E_STATE = L.SBH_OK, L.SBH_E_ARG, L.SBH_E_STATE
N_REF = pc.N_REF
SPANS = [(0, 5, 55)]
LEN = 50
STAGES = ("tally", "stats", "depth", "pileup")
RESULT = {"tally": L.SbhTallyAddResult, "stats": L.SbhStatsAddResult, "depth": L.SbhDepthAddResult,
          "pileup": L.SbhPileupAddResult}
FILTER_TEXT = b"record filter: flags < 65536, 0 <= min_mapq <= 255, row ranges sorted, disjoint and non-empty"
SPANS_TEXT = b" spans: at least one, ref_id in [0, n_ref) strictly ascending, 0 <= beg < end <= 2^31 - 1"


def records():
    return [pc.read(3, [(6, pc.M)]), pc.read(10, [(4, pc.M), (2, pc.D), (3, pc.M)], flag=0x10, seed=1),
            pc.read(20, [(2, pc.S), (5, pc.M), (1, pc.I), (2, pc.M)], seed=2), pc.read(52, [(8, pc.M)], flag=0x4, seed=3)]


def make(ctx, stage):
    return {"tally": lambda: ctx.tally(N_REF), "stats": lambda: ctx.stats(cycles=16, max_insert=32),
            "depth": lambda: ctx.depth(SPANS, N_REF), "pileup": lambda: ctx.pileup(SPANS, N_REF)}[stage]()


def last_error(ctx):
    return bytes(sb.lib().sbh_last_error(ctx.h))


def raw_add(stage, sh, acc, f=None):
    """sbh_records_<stage>_add through ctypes: (status, the result struct's bytes), every byte of the
    struct 0xff before the call."""
    res = RESULT[stage]()
    C.memset(C.byref(res), 0xff, C.sizeof(res))
    rc = getattr(sb.lib(), "sbh_records_%s_add" % stage)(sh.h, acc.h, f, C.byref(res))
    if rc == L.SBH_E_HIP:
        pytest.exit("HIP error: %s" % last_error(sh.ctx), returncode=3)
    return rc, bytes(res)


def refused(ctx, f, *a):
    """(status, text) of a call through the Python wrappers that the library refuses."""
    with pytest.raises(sb.SparkBamError) as e:
        call(f, *a)
    return e.value.code, last_error(ctx)


def totals(stage, acc):
    """What the accumulator holds, as a list of arrays (depth: the slots cannot be read before finish --
    test_empty_scan finishes it instead)."""
    if stage == "tally":
        return list(call(acc.counts))
    if stage == "stats":
        t = call(acc.counts)
        return [t[k] for k in sorted(t)]
    return [call(acc.counts)] if stage == "pileup" else []


@pytest.fixture(scope="module")
def ctx():
    c = sb.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def stream():
    c = pc.case(records(), SPANS)
    return np.frombuffer(bytes(c.flat), np.uint8), list(c.starts)


@pytest.fixture(scope="module")
def shard(ctx, stream):
    """The four records scanned."""
    flat, starts = stream
    sh = scanned(ctx, flat, starts[0], len(starts))
    yield sh
    sh.close()


@pytest.mark.parametrize("stage", STAGES)
def test_shard_of_another_context(ctx, shard, stage):
    other = sb.Context(0)
    acc = make(other, stage)
    try:
        rc, res = raw_add(stage, shard, acc)
        # (the message is left in the shard's context)
        assert (rc, last_error(ctx)) == (E_ARG, b"records_%s_add: the shard and the accumulator belong to different contexts"
                                         % stage.encode())
        assert res == b"\xff" * len(res)
    finally:
        acc.close()
        other.close()


@pytest.mark.parametrize("stage", STAGES)
def test_shard_without_a_scan(ctx, stream, stage):
    flat, _ = stream
    raw = ctx.shard(np.frombuffer(rc.bgzf(flat, 65280), np.uint8).copy())  # resident, inflated below, never scanned
    acc = make(ctx, stage)
    try:
        call(raw.index, 0)
        call(raw.inflate)
        assert refused(ctx, acc.add, raw) == (E_STATE, b"records_%s_add without a records scan" % stage.encode())
        # the scan check comes before the filter's
        assert refused(ctx, acc.add, raw, {"min_mapq": 256})[1] == b"records_%s_add without a records scan" % stage.encode()
    finally:
        acc.close()
        raw.close()


@pytest.mark.parametrize("stage", STAGES)
def test_bad_filter(ctx, shard, stage):
    acc = make(ctx, stage)
    try:
        for bad in ({"min_mapq": 256}, {"flag_require": 65536}, {"rows": [(2, 2)]}, {"rows": [(1, 3), (2, 4)]}):
            assert refused(ctx, acc.add, shard, bad) == (E_ARG, FILTER_TEXT)
    finally:
        acc.close()


@pytest.mark.parametrize("stage", STAGES)
def test_empty_scan(ctx, stream, shard, stage):
    flat, starts = stream
    empty = scanned(ctx, flat, len(flat), 0)
    acc = make(ctx, stage)
    try:
        first = call(acc.add, shard)
        assert first["n"] == 4 and first["n_kept"] == 4
        before = totals(stage, acc)
        rc, res = raw_add(stage, empty, acc)
        assert rc == OK and res == bytes(len(res))  # n = 0 and every other word of the result 0
        # a filter with row ranges stages nothing either
        f, keep = sb.records.record_filter({"rows": [(0, 2)]})
        assert raw_add(stage, empty, acc, C.byref(f)) == (OK, bytes(len(res)))
        del keep
        for got, want in zip(totals(stage, acc), before):
            assert np.array_equal(got, want)
        if stage == "depth":
            add, depth, _, sizes = sb.depth_host(flat, starts, SPANS, N_REF)
            assert first == add and call(acc.finish) == sizes
            assert np.array_equal(call(acc.depth, 0), depth[:LEN])
    finally:
        acc.close()
        empty.close()


FINISH = {"depth": "sbh_depth_finish", "pileup": "sbh_pileup_finish"}
RESET = {"depth": "sbh_depth_reset", "pileup": "sbh_pileup_reset"}
# (function, whether it needs a finish: the pileup's counts may be read between adds)
SPAN_FETCHES = {"depth": (("sbh_depth_fetch", True),),
                "pileup": (("sbh_pileup_counts_fetch", False), ("sbh_pileup_calls_fetch", True))}
LIST_FETCHES = {"depth": ("sbh_depth_runs_fetch", "runs", "n_runs"),
                "pileup": ("sbh_pileup_intervals_fetch", "intervals", "n_intervals")}


def status(ctx, rc):
    if rc == L.SBH_E_HIP:
        pytest.exit("HIP error: %s" % last_error(ctx), returncode=3)
    return (rc, last_error(ctx)) if rc else (rc, b"")


@pytest.mark.parametrize("stage", ("depth", "pileup"))
def test_finish_and_fetch_refusals(ctx, shard, stage):
    lib = sb.lib()
    acc = make(ctx, stage)
    buf = np.zeros(32 * (LEN + 1), np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    list_fetch, what, count = LIST_FETCHES[stage]
    try:
        call(acc.add, shard)
        # before finish
        for fn, needs_finish in SPAN_FETCHES[stage]:
            want = (E_STATE, b"%s before %s" % (fn.encode(), FINISH[stage].encode())) if needs_finish else (OK, b"")
            assert status(ctx, getattr(lib, fn)(acc.h, 0, 0, LEN, p)) == want
        assert status(ctx, getattr(lib, list_fetch)(acc.h, 0, 0, None)) == (
            E_STATE, b"%s before %s" % (list_fetch.encode(), FINISH[stage].encode()))
        if stage == "pileup":
            for bad in ((0, 75), (1, 0), (1, 101)):
                assert refused(ctx, acc.finish, *bad) == (E_ARG, b"pileup finish: min_depth >= 1 and call_pct in [1, 100]")
        sizes = call(acc.finish)
        # finish twice, add after finish
        assert refused(ctx, acc.finish) == (E_STATE, b"%s twice (%s reopens)" % (FINISH[stage].encode(), RESET[stage].encode()))
        assert refused(ctx, acc.add, shard) == (
            E_STATE, b"records_%s_add after %s (%s reopens)" % (stage.encode(), FINISH[stage].encode(), RESET[stage].encode()))
        # ... which is tested after the scan and before the filter
        assert refused(ctx, acc.add, shard, {"min_mapq": 256})[0] == E_STATE
        # past the spans, past the span
        for fn, _ in SPAN_FETCHES[stage]:
            f = getattr(lib, fn)
            assert status(ctx, f(acc.h, 1, 0, 0, p)) == (E_ARG, b"%s: span 1 of 1" % fn.encode())
            assert status(ctx, f(acc.h, 0xffffffff, 0, 1, p)) == (E_ARG, b"%s: span 4294967295 of 1" % fn.encode())
            past = (E_ARG, b"%s past the span" % fn.encode())
            assert status(ctx, f(acc.h, 0, LEN + 1, 0, p)) == past       # from past the length
            assert status(ctx, f(acc.h, 0, 0, LEN + 1, p)) == past       # n past the length
            assert status(ctx, f(acc.h, 0, LEN - 3, 4, p)) == past       # n past the remainder
            assert status(ctx, f(acc.h, 0, 1, 2 ** 64 - 1, p)) == past   # from + n wraps
            assert status(ctx, f(acc.h, 0, LEN, 0, None)) == (OK, b"")   # the empty tail is inside
            assert status(ctx, f(acc.h, 0, LEN - 3, 3, p)) == (OK, b"")
        n = sizes[count]
        f = getattr(lib, list_fetch)
        past = (E_ARG, b"%s past the %s" % (list_fetch.encode(), what.encode()))
        assert status(ctx, f(acc.h, n + 1, 0, None)) == past and status(ctx, f(acc.h, 0, n + 1, p)) == past
        assert status(ctx, f(acc.h, n, 0, None)) == (OK, b"")
        # reset reopens
        call(acc.reset)
        assert call(acc.add, shard)["n_kept"] == 4 and call(acc.finish) == sizes
    finally:
        acc.close()


def create(ctx, fn, *a):
    """(status, text, the handle left in *out) of a create call, *out a non-null value before it."""
    h = C.c_void_p(0xdead)
    rc = getattr(sb.lib(), fn)(ctx.h, *a, C.byref(h))
    return status(ctx, rc) + (h.value,)


def test_create_refusals(ctx):
    good = pc.span_array(SPANS)
    sp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    assert create(ctx, "sbh_tally_create", -1) == (E_ARG, b"tally: n_ref -1 is negative", None)
    assert create(ctx, "sbh_tally_create", -2 ** 31) == (E_ARG, b"tally: n_ref -2147483648 is negative", None)
    assert create(ctx, "sbh_stats_create", None) == (E_ARG, b"stats: no parameters", None)
    for cycles, ins in ((0, 8000), (65537, 8000), (1024, 0), (1024, 2 ** 20 + 1)):
        assert create(ctx, "sbh_stats_create", C.byref(L.SbhStatsParams(cycles, ins))) == (
            E_ARG, b"stats: cycles %d outside [1, 65536] or max_insert %d outside [1, 1048576]" % (cycles, ins), None)
    for flags, text in ((2, b"0x2"), (3, b"0x2"), (0x80000001, b"0x80000000")):
        assert create(ctx, "sbh_depth_create", sp(good), 1, N_REF, flags) == (E_ARG, b"depth: unknown flag bits " + text, None)
    for q in (-1, 256):
        assert create(ctx, "sbh_pileup_create", sp(good), 1, N_REF, q) == (
            E_ARG, b"pileup: min_baseq %d outside [0, 255]" % q, None)
    bad_spans = ([], [(1, 0, 10), (0, 0, 10)], [(1, 0, 10), (1, 20, 30)], [(0, 10, 10)], [(0, -1, 5)], [(0, 0, 2 ** 31)],
                 [(-1, 0, 10)], [(N_REF, 0, 10)])
    for stage, fn, arg in (("depth", "sbh_depth_create", 0), ("pileup", "sbh_pileup_create", 0)):
        for spans in bad_spans:
            a = pc.span_array(spans)
            assert create(ctx, fn, sp(a), len(spans), N_REF, arg) == (E_ARG, stage.encode() + SPANS_TEXT, None)
        for n_ref in (-1, 0):  # a negative n_ref, and none: no span's reference is below it
            assert create(ctx, fn, sp(good), 1, n_ref, arg) == (E_ARG, stage.encode() + SPANS_TEXT, None)
        # the flag and the quality are judged before the spans
        worse = 2 if stage == "depth" else 256
        assert create(ctx, fn, None, 0, N_REF, worse)[1].startswith(stage.encode() + b": ")
    # no context, no place for the handle: SBH_E_ARG and no message to leave
    assert sb.lib().sbh_tally_create(None, 1, C.byref(C.c_void_p())) == E_ARG
    assert sb.lib().sbh_tally_create(ctx.h, 1, None) == E_ARG
