"""tests/interval_join_reference.py against itself and against the contract's worked vectors: the
element-at-a-time simulation and the closed form agree, and both give what include/gpuwin.h
states for the boundary cases.  No library, no device."""
import numpy as np
import pytest

from flink_amd import windowing as W
from tests import interval_join_reference as R

L, RT = R.LEFT, R.RIGHT


def _cols(key, ts, pay=None):
    ts = np.asarray(ts, np.int64)
    pay = ts * 10 if pay is None else np.asarray(pay, np.int64)
    return np.full(len(ts), key, np.int64), ts, pay


def _run(lower, upper, events):
    """The simulation over `events`: per ingest call (rows, late records of the call)."""
    sim = R.IntervalJoinSim(lower, upper)
    out = []
    for ev in events:
        if ev[0] == "watermark":
            sim.advance_watermark(ev[1])
        else:
            late0 = sim.late_dropped
            rows = sim.ingest(*ev[1:])
            out.append((rows, sim.late_dropped - late0))
    return out


def _row_set(rows):
    return sorted(zip(*[c.tolist() for c in rows]))


BOUNDS = [(-1, 1), (0, 2), (-3, -1), (2, 7), (0, 0), (-5, -5), (4, 4), (-12, 9), (-40, 40)]


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("lower,upper", BOUNDS)
def test_simulation_and_closed_form_agree(seed, lower, upper):
    events = R.make_stream(seed * 31 + (lower + 50) * 101 + upper)
    sim, closed = _run(lower, upper, events), R.closed_form(lower, upper, events)
    assert len(sim) == len(closed) == sum(e[0] == "ingest" for e in events)
    for (rows_s, late_s), (rows_c, late_c) in zip(sim, closed):
        assert late_s == late_c
        assert _row_set(rows_s) == _row_set(rows_c)  # as sets per call
        R.check(rows_s, rows_c)                      # and in the specified order


def test_the_grid_is_not_vacuous():
    """Over the grid: rows, late records, and pairs inside the bounds lost to a cleanup."""
    rows = late = lost = 0
    for lower, upper in BOUNDS:
        for seed in range(6):
            events = R.make_stream(seed * 31 + (lower + 50) * 101 + upper)
            got = _run(lower, upper, events)
            rows += sum(len(r[0]) for r, _ in got)
            late += sum(l for _, l in got)
            # the same records and watermarks' lateness, but no cleanup: the watermarks come last
            # for the buffers, i.e. the closed form without its third condition
            sim = R.IntervalJoinSim(lower, upper)
            wm, n_all = R.I64_MIN, 0
            for ev in events:
                if ev[0] == "watermark":
                    wm = max(wm, ev[1])
                    continue
                _, side, key, ts, pay = ev
                keep = np.ones(len(ts), bool) if wm == R.I64_MIN else ts >= wm
                n_all += len(sim.ingest(side, key[keep], ts[keep], pay[keep])[0])
            lost += n_all - sum(len(r[0]) for r, _ in got)
    # (a pair is lost only on the exact boundary: the later record's ts == the watermark == the
    # earlier one's cleanup time, so these are few)
    assert rows > 1000 and late > 100 and lost >= 10


def test_vector_1_symmetric_bounds():
    """lower = -1, upper = 1, key 7: left ts 1..4 in one call, then right ts 1..4."""
    sim = R.IntervalJoinSim(-1, 1)
    assert len(sim.ingest(L, *_cols(7, [1, 2, 3, 4]))[0]) == 0  # records of one call never pair
    rows = sim.ingest(RT, *_cols(7, [1, 2, 3, 4]))
    assert len(rows[0]) == 10
    partners = {r: sorted(rows[1][rows[2] == r].tolist()) for r in (1, 2, 3, 4)}
    assert partners == {1: [1, 2], 2: [1, 2, 3], 3: [2, 3, 4], 4: [3, 4]}
    assert rows[0].tolist() == [7] * 10
    assert rows[2].tolist() == [1, 1, 2, 2, 2, 3, 3, 3, 4, 4]      # the call's records in arrival order
    assert rows[1].tolist() == [1, 2, 1, 2, 3, 2, 3, 4, 3, 4]      # partners by ascending ts
    assert rows[3].tolist() == [t * 10 for t in rows[1].tolist()] and rows[4].tolist() == [t * 10 for t in rows[2].tolist()]
    closed = R.closed_form(-1, 1, [("ingest", L, *_cols(7, [1, 2, 3, 4])), ("ingest", RT, *_cols(7, [1, 2, 3, 4]))])
    R.check(closed[1][0], rows)


@pytest.mark.parametrize("wm,right_ts,rows,late", [(7, 7, 0, 0), (6, 7, 1, 0), (7, 6, 0, 1)])
def test_vector_2_the_cleanup_boundary(wm, right_ts, rows, late):
    """lower = 0, upper = 2, left ts 5 (cleaned at 7): a right record at ts 7 arriving on watermark
    7 is not late but its partner is gone; on watermark 6 it pairs; ts 6 after watermark 7 is late."""
    events = [("ingest", L, *_cols(1, [5])), ("watermark", wm), ("ingest", RT, *_cols(1, [right_ts]))]
    for got in (_run(0, 2, events), R.closed_form(0, 2, events)):
        assert (len(got[1][0][0]), got[1][1]) == (rows, late)
    if rows:
        assert [c.tolist() for c in _run(0, 2, events)[1][0]] == [[1], [5], [7], [50], [70]]


def test_vector_3_negative_bounds():
    """lower = -3, upper = -1: right ts 10, then left ts 12 pairs (12 - 3 <= 10 <= 12 - 1).  The
    right record is cleaned at 10 + 3 = 13, the left one at its own ts."""
    assert R.cleanup_time(RT, 10, -3, -1) == 13 and R.cleanup_time(L, 12, -3, -1) == 12
    for wm, rows in ((12, 1), (13, 0)):
        events = [("ingest", RT, *_cols(4, [10])), ("watermark", wm), ("ingest", L, *_cols(4, [12 if wm == 12 else 13]))]
        for got in (_run(-3, -1, events), R.closed_form(-3, -1, events)):
            assert len(got[1][0][0]) == rows
    sim = R.IntervalJoinSim(-3, -1)
    sim.ingest(RT, *_cols(4, [10]))
    sim.ingest(L, *_cols(4, [12]))
    sim.advance_watermark(12)
    assert (sim.live(L), sim.live(RT)) == (0, 1)
    sim.advance_watermark(13)
    assert sim.live(RT) == 0


@pytest.mark.parametrize("lower,upper,left_ts,right_ts", [
    (-9, -2, 20, [10, 11, 18, 19]),   # all negative: the right record is the older one
    (2, 9, 20, [21, 22, 29, 30]),     # all positive
    (5, 5, 20, [24, 25, 26]),         # lower == upper: one timestamp
    (0, 0, 20, [19, 20, 21]),
    (-5, -5, 20, [14, 15, 16]),
])
def test_bounds_all_negative_all_positive_and_equal(lower, upper, left_ts, right_ts):
    want = [t for t in right_ts if left_ts + lower <= t <= left_ts + upper]
    assert 1 <= len(want) < len(right_ts)
    for first in (L, RT):  # either side arriving first
        sim = R.IntervalJoinSim(lower, upper)
        calls = [(L, _cols(3, [left_ts])), (RT, _cols(3, right_ts))]
        if first == RT:
            calls.reverse()
        assert len(sim.ingest(calls[0][0], *calls[0][1])[0]) == 0
        rows = sim.ingest(calls[1][0], *calls[1][1])
        assert rows[2].tolist() == want and rows[1].tolist() == [left_ts] * len(want)


def test_exclusive_bounds():
    assert R.exclusive_bounds(-2, 3, lower_exclusive=True) == (-1, 3)
    assert R.exclusive_bounds(-2, 3, upper_exclusive=True) == (-2, 2)
    assert R.exclusive_bounds(4, 6, True, True) == (5, 5)
    for lo, hi, le, ue in ((4, 4, True, False), (4, 4, False, True), (4, 5, True, True), (5, 4, False, False)):
        with pytest.raises(ValueError):
            R.exclusive_bounds(lo, hi, le, ue)
    # the rows: (0, 2] and [0, 2) and (0, 2)
    for le, ue, want in ((True, False, [6, 7]), (False, True, [5, 6]), (True, True, [6])):
        sim = R.IntervalJoinSim(*R.exclusive_bounds(0, 2, le, ue))
        sim.ingest(L, *_cols(1, [5]))
        assert sim.ingest(RT, *_cols(1, [4, 5, 6, 7, 8]))[2].tolist() == want


def test_api_mirror_bounds_follow_the_reference():
    """IntervalJoined.between / lower_bound_exclusive / upper_bound_exclusive (no library call)."""
    env = W.StreamExecutionEnvironment.get_execution_environment()
    a = env.from_elements([]).key_by(lambda v: v)
    b = env.from_elements([]).key_by(lambda v: v)
    j = a.interval_join(b).between(-2, 3).lower_bound_exclusive().upper_bound_exclusive()
    assert (j.lower, j.upper) == R.exclusive_bounds(-2, 3, True, True) == (-1, 2)
    with pytest.raises(ValueError):
        a.interval_join(b).between(3, 2)
    with pytest.raises(ValueError):
        a.interval_join(b).between(4, 4).lower_bound_exclusive()
    with pytest.raises(ValueError):
        a.interval_join(b).between(4, 5).lower_bound_exclusive().upper_bound_exclusive()
    with pytest.raises(ValueError):
        a.interval_join(b).lower_bound_exclusive()
    with pytest.raises(ValueError):
        W.GpuIntervalJoinOperator(1, 0)
    with pytest.raises(ValueError):
        W.GpuIntervalJoinOperator(0, (1 << 62) + 1)


def test_errors_leave_nothing_and_kill_the_operator():
    sim = R.IntervalJoinSim(-1, 1)
    sim.ingest(L, *_cols(1, [5]))
    with pytest.raises(R.NoTimestamp):
        sim.ingest(RT, *_cols(1, [5, R.I64_MIN]))
    assert sim.live(RT) == 0 and sim.rows_emitted == 0
    with pytest.raises(R.Failed):
        sim.ingest(RT, *_cols(1, [5]))
    with pytest.raises(R.Failed):
        sim.advance_watermark(3)
    # the range check is for the records that are not late; Long.MIN_VALUE is checked before
    sim = R.IntervalJoinSim(0, 10)
    sim.advance_watermark(0)
    assert len(sim.ingest(RT, *_cols(1, [R.I64_MIN + 3]))[0]) == 0 and sim.late_dropped == 1  # late: no range check
    with pytest.raises(R.NoTimestamp):
        sim.ingest(RT, *_cols(1, [R.I64_MIN]))
    for side, ts in ((L, R.I64_MAX - 9), (RT, R.I64_MIN + 9)):
        sim = R.IntervalJoinSim(0, 10)
        with pytest.raises(R.BoundRange):
            sim.ingest(side, *_cols(1, [ts]))
        sim = R.IntervalJoinSim(0, 10)
        sim.ingest(side, *_cols(1, [ts + (-1 if side == L else 1)]))


def test_watermark_that_does_not_advance_is_ignored():
    sim = R.IntervalJoinSim(0, 5)
    sim.advance_watermark(10)
    sim.advance_watermark(4)
    assert sim.wm == 10
    assert len(sim.ingest(L, *_cols(1, [9]))[0]) == 0 and sim.late_dropped == 1
