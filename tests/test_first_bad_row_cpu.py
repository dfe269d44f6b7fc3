"""The opening every *_add_host shares (csrc/bam_gather_core.h: first_bad_row), through the four
accumulators' host entry points, no GPU: every row is validated, kept or not; a kept row must also
pass the stage's own test -- the reference range (tally), the range and the op codes (depth), the range
and the query lengths (pileup), nothing (stats); the first such row is reported and the output arrays
are left as they were.  Four hand-built rows per case."""
import sys

import numpy as np
import pytest

from pkg import sb
import pileup_corpus as pc
import record_corpus as rc

SBH_E_BAD_RECORD = sb._lib.SBH_E_BAD_RECORD
stm = sys.modules["spark_bam_amd.stats"]  # (sb.stats is api.stats, the function)
M = pc.M
N_REF = pc.N_REF
SPANS = [(0, 0, 60)]
STAGES = ("tally", "stats", "depth", "pileup")
DUP = 0x400


def good(i, flag=0):
    return pc.read(10 + i, [(4, M)], flag=flag, seed=i)


def malformed(flag=0):
    """A record whose block_size is too small for its own parts: row_check refuses it."""
    r = bytearray(good(9, flag))
    r[0:4] = (40).to_bytes(4, "little")
    return bytes(r)


# a kept row that fails the named stage's own test; REFUSES: every stage whose test it fails
OWN = {
    "tally": lambda flag=0: pc.read(10, [(4, M)], ref=N_REF, flag=flag),      # depth and pileup refuse it as well
    "depth": lambda flag=0: pc.read(10, [(4, M), (4, 9)], codes=(1,) * 4, qual=bytes(4), flag=flag),  # op code 9: pileup too
    "pileup": lambda flag=0: pc.read(10, [(9, M)], codes=(1,) * 10, qual=bytes(10), flag=flag),       # 9 != l_seq 10
}
REFUSES = {"tally": ("tally", "depth", "pileup"), "depth": ("depth", "pileup"), "pileup": ("pileup",)}


def add(stage, records, filter=None):
    """The stage's host add over the records, every output word 7 before it: (bad row, None) with the
    outputs verified untouched, or (None, n_kept)."""
    s = rc.lay(records)
    flat = np.frombuffer(s.flat, np.uint8)
    if stage == "tally":
        out = [np.full((16, 2), 7, np.uint64), np.full((N_REF + 1, 2), 7, np.uint64)]
        go = lambda: sb.tally_host(flat, s.starts, N_REF, filter, flag=out[0], ref=out[1])[2]  # noqa: E731
    elif stage == "stats":
        t = stm.empty_tables(16, 32)
        for a in t.values():
            a[...] = 7
        out = list(t.values())
        go = lambda: sb.stats_host(flat, s.starts, 16, 32, filter, tables=t)[1]  # noqa: E731
    elif stage == "depth":
        out = [np.full(61, 7, np.int32)]
        go = lambda: sb.depth_host(flat, s.starts, SPANS, N_REF, filter, slots=out[0], finish=False)[0]["n_kept"]  # noqa: E731
    else:
        out = [np.full((60, 8), 7, np.uint32)]
        go = lambda: sb.pileup_host(flat, s.starts, SPANS, N_REF, filter, counts=out[0], finish=False)[0]["n_kept"]  # noqa: E731
    try:
        return None, go()
    except sb.SparkBamError as e:
        assert e.code == SBH_E_BAD_RECORD and len(e.fields) == 1
        assert all((a == 7).all() for a in out)
        return e.fields[0], None


@pytest.mark.parametrize("stage", STAGES)
def test_a_malformed_row_first_last_and_dropped_by_the_filter(stage):
    assert add(stage, [good(0), good(1), good(2), good(3)]) == (None, 4)
    assert add(stage, [malformed(), good(1), good(2), good(3)]) == (0, None)
    assert add(stage, [good(0), good(1), good(2), malformed()]) == (3, None)
    # the filter would drop the row: it is judged all the same
    drop = {"flag_exclude": DUP}
    assert add(stage, [good(0), good(1), good(2, DUP), good(3)], drop) == (None, 3)
    assert add(stage, [good(0), good(1), malformed(DUP), good(3)], drop) == (2, None)
    assert add(stage, [good(0), good(1), good(2), malformed()], {"rows": [(0, 2)]}) == (3, None)
    # two of them: the first
    assert add(stage, [good(0), malformed(), good(2), malformed()]) == (1, None)


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("own", sorted(OWN))
def test_a_kept_row_the_stage_itself_refuses(stage, own):
    row = OWN[own]
    refuses = stage in REFUSES[own]
    assert add(stage, [good(0), row(), good(2), good(3)]) == ((1, None) if refuses else (None, 4))
    assert add(stage, [good(0), good(1), good(2), row()]) == ((3, None) if refuses else (None, 4))
    # before a malformed row it is the first bad row; behind one it is not
    assert add(stage, [good(0), row(), good(2), malformed()]) == ((1, None) if refuses else (3, None))
    assert add(stage, [malformed(), row(), good(2), good(3)]) == (0, None)
    # dropped by the filter it is no bad row for anyone
    assert add(stage, [good(0), row(DUP), good(2), good(3)], {"flag_exclude": DUP}) == (None, 3)
    assert add(stage, [good(0), good(1), good(2), row()], {"rows": [(0, 3)]}) == (None, 3)
