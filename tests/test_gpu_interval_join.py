"""Event-time interval join on the device (gw_ijoin.hip; gw_interval_join_device, gw_ijoin_*): the
stateless call and the operator against tests/interval_join_reference.py, exactly, in order and
values.

Shapes hit the wave (64), the scan tile (1024 records) and several expand tiles (1024 output
rows); one key gives long partner ranges, as many keys as records leaves most probes without a
partner.  Every case that is not named empty must have rows by the reference alone.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from flink_amd import _native as N
from flink_amd import windowing as W
from tests import interval_join_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 64
MAX_ROWS = 2_200_000


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0xffffffff


def _dev(cols):
    # (one element when empty: an empty tensor has no pointer; the length travels separately)
    return [torch.from_numpy(np.resize(np.ascontiguousarray(c), max(len(c), 1))).cuda() for c in cols]


# a thinned product: every n on each side, every n with itself, and per (shape, keys) two of the
# eight (bounds, probe side) combinations in rotation, so that every one meets every key distribution
_NS = [0, 1, 63, 64, 65, 1024, 1025, 20_011]
SHAPES = sorted({(n, _NS[(3 * i + 1) % 8]) for i, n in enumerate(_NS)} | {(n, n) for n in _NS} |
                {(20_011, 1025), (65, 20_011)})
KEYS = ["one", "seven", "many"]
BOUNDS = [(-1, 1), (0, 2), (-3, -1), (2, 2)]
_COMBOS = [(b, s) for b in BOUNDS for s in (R.LEFT, R.RIGHT)]
CASES = []
for _i, (_np, _nb) in enumerate(SHAPES):
    for _j, _k in enumerate(KEYS):
        for _t in range(2):
            CASES.append((_np, _nb, _k) + _COMBOS[(2 * (_i + _j) + 3 * _t) % 8])
CASES = sorted(set(CASES))

_ref = {}


def _inputs(n_p, n_b, keys, bounds, probe_side):
    """Seeded inputs and their reference, made once; the seed is the first whose reference has
    rows (unless a side is empty)."""
    case = (n_p, n_b, keys, bounds, probe_side)
    if case in _ref:
        return _ref[case]
    if keys == "one":      # one key in a span of 100: partner ranges of tens of records, many expand tiles
        n_p, n_b = min(n_p, 1500), min(n_b, 1500)
        kw = dict(num_keys=1, ts_span=100)
    elif keys == "seven":
        kw = dict(num_keys=7, ts_span=max(100, max(n_p, n_b) // 2))
    else:
        kw = dict(num_keys=max(n_p + n_b, 1), ts_span=40)
    for t in range(2000):
        probe = R.make_records(_seed(case, t, 0), n_p, **kw)
        build = R.make_records(_seed(case, t, 1), n_b, **kw)
        want = R.reference_call(probe_side, probe, build, *bounds)
        if len(want[0]) > 0 or n_p == 0 or n_b == 0:
            break
    _ref[case] = (probe, build, want)
    return _ref[case]


def _ids(v):
    return "%d_%d" % v if isinstance(v, tuple) else None


@pytest.mark.parametrize("n_p,n_b,keys,bounds,probe_side", CASES, ids=_ids)
def test_device_matches_reference(n_p, n_b, keys, bounds, probe_side):
    probe, build, want = _inputs(n_p, n_b, keys, bounds, probe_side)
    if n_p > 0 and n_b > 0:
        assert 1 <= len(want[0]) <= MAX_ROWS  # not vacuous
    else:
        assert len(want[0]) == 0
    dp, db = _dev(probe), _dev(build)
    got = W.interval_join_device(probe_side, *[t[:len(probe[0])] for t in dp], *[t[:len(build[0])] for t in db], *bounds)
    R.check([g.cpu().numpy() for g in got], want)


def test_case_list_covers_the_contract():
    assert {c[0] for c in CASES} == set(_NS) and {c[1] for c in CASES} == set(_NS)
    assert {(c[2], c[3], c[4]) for c in CASES} == {(k, b, s) for k in KEYS for b in BOUNDS for s in (R.LEFT, R.RIGHT)}
    assert (20_011, 20_011) in {c[:2] for c in CASES}
    assert any(lo == hi for lo, hi in BOUNDS) and any(hi < 0 for _, hi in BOUNDS)


def _call(probe_side, probe, build, lower, upper, cap, shift=(0, 0, 0, 0, 0)):
    """gw_interval_join_device into sentinel-filled columns of cap + GUARD rows, column c starting
    shift[c] words into its tensor.  (rc, n_out, the columns from their start, as numpy)."""
    dp, db = _dev(probe), _dev(build)
    out = [torch.full((cap + GUARD + 4,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(5)]
    n_out = ctypes.c_int64(-7)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    rc = N.lib().gw_interval_join_device(probe_side, len(probe[0]), *[P(t) for t in dp], len(build[0]), *[P(t) for t in db],
                                         lower, upper, *[ctypes.c_void_p(o.data_ptr() + 8 * s) for o, s in zip(out, shift)],
                                         cap, ctypes.byref(n_out), None)
    return rc, n_out.value, [o.cpu().numpy()[s:] for o, s in zip(out, shift)]


def _cols(key, ts, pay_base=0):
    key, ts = np.asarray(key, np.int64), np.asarray(ts, np.int64)
    return key, ts, np.arange(len(key), dtype=np.int64) + pay_base


@pytest.mark.parametrize("probe_side", [R.LEFT, R.RIGHT], ids=["left", "right"])
def test_one_probe_with_5000_partners(probe_side):
    """One descriptor spans five expand tiles; the partners come by ascending (ts, arrival)."""
    rng = np.random.default_rng(5)
    bkey = np.concatenate([np.full(5000, 3, np.int64), rng.integers(4, 40, 2000)])
    bts = np.concatenate([rng.integers(-1, 2, 5000), rng.integers(-1, 2, 2000)])
    order = rng.permutation(7000)
    build = _cols(bkey[order], bts[order], 1000)
    probe = _cols([2, 3, 50], [0, 0, 0])
    want = R.reference_call(probe_side, probe, build, -1, 1)
    assert len(want[0]) == 5000
    rc, n, out = _call(probe_side, probe, build, -1, 1, 5000)
    assert (rc, n) == (N.GW_OK, 5000)
    R.check([o[:5000] for o in out], want)
    assert all((o[5000:] == SENTINEL).all() for o in out)


def test_3000_probes_without_a_partner_between_two_with():
    """Without the compaction the tile's descriptors would not fit: the two probes with partners
    are 3000 records apart and their rows are neighbours."""
    build = _cols(np.full(700, 9), np.arange(700) % 3)
    probe = _cols(np.concatenate([[9], np.arange(100, 3100), [9]]), np.concatenate([[1], np.zeros(3000, np.int64), [2]]))
    want = R.reference_call(R.LEFT, probe, build, -1, 0)
    assert len(want[0]) == 2 * 700 - 233 - 234 and set(want[3].tolist()) == {0, 3001}
    rc, n, out = _call(R.LEFT, probe, build, -1, 0, len(want[0]))
    assert (rc, n) == (N.GW_OK, len(want[0]))
    R.check([o[:n] for o in out], want)


@pytest.mark.parametrize("n", [1024, 1025])
def test_a_tile_of_single_row_descriptors(n):
    """1024 descriptors of one row each fill a tile's LDS exactly; 1025 leave one row to a second tile."""
    rng = np.random.default_rng(n)
    probe = _cols(rng.permutation(n) - 500, np.zeros(n))
    build = _cols(rng.permutation(n + 300) - 500, np.full(n + 300, 7), 5000)
    want = R.reference_call(R.RIGHT, probe, build, -7, -7)
    assert len(want[0]) == n
    rc, got_n, out = _call(R.RIGHT, probe, build, -7, -7, n)
    assert (rc, got_n) == (N.GW_OK, n)
    R.check([o[:n] for o in out], want)


def test_extreme_keys_and_negative_timestamps():
    rng = np.random.default_rng(11)
    table = np.array([R.I64_MIN, R.I64_MIN + 1, -2, -1, 0, 1, R.I64_MAX - 1, R.I64_MAX], np.int64)
    sides = []
    for n in (900, 1100):
        sides.append((table[rng.integers(0, 8, n)], rng.integers(-(1 << 40), -(1 << 40) + 50, n).astype(np.int64),
                      rng.integers(R.I64_MIN, R.I64_MAX, n, dtype=np.int64, endpoint=True)))
    for probe_side in (R.LEFT, R.RIGHT):
        want = R.reference_call(probe_side, sides[0], sides[1], -2, 3)
        assert 1000 < len(want[0]) <= MAX_ROWS and {R.I64_MIN, R.I64_MAX} <= set(want[0].tolist())
        rc, n, out = _call(probe_side, sides[0], sides[1], -2, 3, len(want[0]))
        assert (rc, n) == (N.GW_OK, len(want[0]))
        R.check([o[:n] for o in out], want)


@pytest.mark.parametrize("shift", [(0,) * 5, (1,) * 5, (2,) * 5, (3,) * 5, (0, 1, 0, 1, 0)],
                         ids=["0", "1", "2", "3", "mixed"])
@pytest.mark.parametrize("odd", [False, True], ids=["even", "odd"])
def test_output_row_offsets_against_the_16_byte_stores(shift, odd):
    """Columns 8 bytes past a 16-byte boundary give the two-rows-per-lane store a head, an odd
    total a tail, and columns of different alignment take the 8-byte stores."""
    probe, build, want = _inputs(1025, 1024, "one", (-1, 1), R.LEFT)
    if odd != bool(len(want[0]) & 1):
        probe = tuple(c[:-1] for c in probe)
        while bool(len(R.reference_call(R.LEFT, probe, build, -1, 1)[0]) & 1) != odd:
            probe = tuple(c[:-1] for c in probe)
        want = R.reference_call(R.LEFT, probe, build, -1, 1)
    need = len(want[0])
    assert need > 2048 and bool(need & 1) == odd
    rc, n, out = _call(R.LEFT, probe, build, -1, 1, need, shift)
    assert (rc, n) == (N.GW_OK, need)
    R.check([o[:need] for o in out], want)
    assert all((o[need:] == SENTINEL).all() for o in out)


def test_cap_exact_and_one_short():
    probe, build, want = _inputs(1025, 1025, "one", (0, 2), R.RIGHT)
    need = len(want[0])
    assert need > 2048
    rc, n, out = _call(R.RIGHT, probe, build, 0, 2, need)
    assert (rc, n) == (N.GW_OK, need)
    R.check([o[:need] for o in out], want)
    assert all((o[need:] == SENTINEL).all() for o in out)
    for cap in (need - 1, 0):
        rc, n, out = _call(R.RIGHT, probe, build, 0, 2, cap)
        assert (rc, n) == (N.GW_E_OUTPUT_FULL, need)
        assert all((o == SENTINEL).all() for o in out)


def test_device_errors():
    one = (np.array([1], np.int64), np.array([5], np.int64), np.array([9], np.int64))
    many = R.make_records(3, 3000, 7)
    big = 1 << 62
    for probe_side in (R.LEFT, R.RIGHT):
        for where in ("probe", "build"):
            side = probe_side if where == "probe" else 1 - probe_side
            over = R.I64_MAX - 9 if side == R.LEFT else R.I64_MIN + 9  # ts + 10 / ts - 10 leaves int64
            for bad, code in (([R.I64_MIN], N.GW_E_NO_TIMESTAMP), ([over], N.GW_E_RANGE), ([over, R.I64_MIN], N.GW_E_NO_TIMESTAMP)):
                cols = (many[0], many[1].copy(), many[2])
                cols[1][2900:2900 + len(bad)] = bad
                args = (cols, one) if where == "probe" else (one, cols)
                rc, n, out = _call(probe_side, *args, 0, 10, 64)
                assert (rc, n) == (code, 0)
                assert all((o == SENTINEL).all() for o in out)
            ok = (many[0], many[1].copy(), many[2])
            ok[1][2900] = over + (-1 if side == R.LEFT else 1)  # just inside
            args = (ok, one) if where == "probe" else (one, ok)
            assert _call(probe_side, *args, 0, 10, 64)[0] == N.GW_OK
    assert _call(R.LEFT, one, one, 2, 1, 4)[0] == N.GW_E_INVALID
    assert _call(R.LEFT, one, one, 0, big + 1, 4)[0] == N.GW_E_INVALID
    assert _call(R.LEFT, one, one, -big - 1, 0, 4)[0] == N.GW_E_INVALID
    assert _call(R.LEFT, one, one, -big, big, 4)[:2] == (N.GW_OK, 1)
    assert _call(2, one, one, 0, 0, 4)[0] == N.GW_E_INVALID
    assert _call(R.LEFT, one, one, 0, 0, -1)[0] == N.GW_E_INVALID
    L = N.lib()
    n_out = ctypes.c_int64(-7)
    d = torch.zeros(8, dtype=torch.int64, device="cuda")
    p = ctypes.c_void_p(d.data_ptr())
    for n_p, n_b in ((1 << 30, 1), (1, 1 << 30)):  # refused before any column is read
        assert L.gw_interval_join_device(0, n_p, p, p, p, n_b, p, p, p, 0, 0, p, p, p, p, p, 1, ctypes.byref(n_out),
                                         None) == N.GW_E_UNSUPPORTED
    assert L.gw_interval_join_device(0, 1, None, p, p, 1, p, p, p, 0, 0, p, p, p, p, p, 1, ctypes.byref(n_out), None) == N.GW_E_INVALID
    assert L.gw_interval_join_device(0, 1, p, p, p, 1, p, p, p, 0, 0, p, p, p, p, p, 1, None, None) == N.GW_E_INVALID
    ms = ctypes.c_double(-1)
    assert L.gw_interval_join_device_timed(0, 1, p, p, p, 1, p, p, p, 0, 0, p, p, p, p, p, 1, ctypes.byref(n_out), None,
                                           None) == N.GW_E_INVALID
    assert L.gw_interval_join_device_timed(0, 1, p, p, p, 1, p, p, p, 0, 0, p, p, p, p, p, 1, ctypes.byref(n_out), None,
                                           ctypes.byref(ms)) == N.GW_OK
    assert n_out.value == 1 and ms.value >= 0


# ---- the operator ------------------------------------------------------------------------------
def _drive(op, sim, events, device=False):
    """Every ingest call and every watermark through the operator and the simulation: the call's
    rows (exact), the late count and the live records per side after each step."""
    stream = torch.cuda.Stream() if device else None
    for ev in events:
        if ev[0] == "watermark":
            op.advance_watermark(ev[1])
            sim.advance_watermark(ev[1])
        else:
            _, side, key, ts, pay = ev
            want = sim.ingest(side, key, ts, pay)
            if device:
                with torch.cuda.stream(stream):
                    d = _dev((key, ts, pay))
                    n = op.process_batch_device(side, *[t[:len(key)] for t in d])
            else:
                n = op.process_batch(side, key, ts, pay)
            assert n == len(want[0]) == op.pending() == op.stats()["last_call_rows"]
            R.check(op.drain(), want)
        st = op.stats()
        assert (st["live_left"], st["live_right"]) == (sim.live(R.LEFT), sim.live(R.RIGHT))
        assert op.num_late_records_dropped() == sim.late_dropped
    assert op.stats()["rows_emitted"] == sim.rows_emitted


def _log_view(op, sim, side):
    """The order of a side's log, seen through a probe of the other side that meets every record
    of each key: the partners come in log order.  (The probe records join the other log.)"""
    log = sim.log(side)
    keys = np.unique(log[0])
    ts = np.full(len(keys), 0, np.int64)
    want = sim.ingest(1 - side, keys, ts, keys)
    assert len(want[0]) == len(log[0])
    op.process_batch(1 - side, keys, ts, keys)
    R.check(op.drain(), want)


@pytest.mark.parametrize("device_ingest", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("bounds", [(-1, 1), (0, 2), (-3, -1), (-12, 9), (4, 4)], ids=_ids)
@pytest.mark.parametrize("seed", [1, 2])
def test_operator_matches_simulation(seed, bounds, device_ingest):
    for t in range(200):  # the first stream with rows and late records by the simulation alone
        events = R.make_stream(_seed(seed, bounds, t), calls=16)
        ref = R.IntervalJoinSim(*bounds)
        for e in events:
            if e[0] == "ingest":
                ref.ingest(*e[1:])
            else:
                ref.advance_watermark(e[1])
        if ref.rows_emitted >= 20 and ref.late_dropped >= 1:
            break
    assert ref.rows_emitted >= 20 and ref.late_dropped >= 1  # not vacuous
    with W.GpuIntervalJoinOperator(*bounds, capacity_hint=16, max_batch=16) as op:
        _drive(op, R.IntervalJoinSim(*bounds), events, device_ingest)
        assert op.stats()["live_left"] == op.stats()["live_right"] == 0  # the last watermark is the end of input


def _one_key(ts, key=7):
    ts = np.asarray(ts, np.int64)
    return np.full(len(ts), key, np.int64), ts, ts * 10


def test_vector_1_symmetric_bounds():
    with W.GpuIntervalJoinOperator(-1, 1) as op:
        assert op.process_batch(op.LEFT, *_one_key([1, 2, 3, 4])) == 0  # records of one call never pair
        assert op.process_batch(op.RIGHT, *_one_key([1, 2, 3, 4])) == 10
        k, lt, rt, lp, rp = op.drain()
        assert k.tolist() == [7] * 10
        assert rt.tolist() == [1, 1, 2, 2, 2, 3, 3, 3, 4, 4] and lt.tolist() == [1, 2, 1, 2, 3, 2, 3, 4, 3, 4]
        assert lp.tolist() == [t * 10 for t in lt.tolist()] and rp.tolist() == [t * 10 for t in rt.tolist()]


@pytest.mark.parametrize("wm,right_ts,rows,late", [(7, 7, 0, 0), (6, 7, 1, 0), (7, 6, 0, 1)])
def test_vector_2_the_cleanup_boundary(wm, right_ts, rows, late):
    events = [("ingest", R.LEFT, *_one_key([5])), ("watermark", wm), ("ingest", R.RIGHT, *_one_key([right_ts]))]
    sim = R.IntervalJoinSim(0, 2)
    with W.GpuIntervalJoinOperator(0, 2) as op:
        _drive(op, sim, events)
        assert (sim.rows_emitted, sim.late_dropped) == (rows, late)
        assert (op.stats()["rows_emitted"], op.num_late_records_dropped()) == (rows, late)


def test_vector_3_negative_bounds():
    with W.GpuIntervalJoinOperator(-3, -1) as op:
        op.process_batch(op.RIGHT, *_one_key([10]))
        assert op.process_batch(op.LEFT, *_one_key([12])) == 1
        assert [c.tolist() for c in op.drain()] == [[7], [12], [10], [120], [100]]
        op.advance_watermark(12)   # the left record is cleaned at its own ts, the right one at 10 + 3
        assert (op.stats()["live_left"], op.stats()["live_right"]) == (0, 1)
        op.advance_watermark(13)
        assert op.stats()["live_right"] == 0


def test_merges_before_after_interleaved_and_ties():
    """The batch sorts wholly before, wholly after and in between the log's records, and ties with
    them on (key, ts): the partner order of a wide probe is the log's order, old before new."""
    sim = R.IntervalJoinSim(-1000, 1000)
    with W.GpuIntervalJoinOperator(-1000, 1000, capacity_hint=16) as op:
        pay = iter(range(0, 10 ** 6, 1000))

        def ingest(side, key, ts):
            key, ts = np.asarray(key, np.int64), np.asarray(ts, np.int64)
            p = np.arange(len(key), dtype=np.int64) + next(pay)
            want = sim.ingest(side, key, ts, p)
            assert op.process_batch(side, key, ts, p) == len(want[0])
            R.check(op.drain(), want)

        ingest(R.LEFT, [5, 5, 6, 5], [10, 12, 3, 10])             # the first batch, with a tie of its own
        ingest(R.LEFT, [7, 8, 6], [0, 0, 9])                      # wholly after (6 @ 9 follows 6 @ 3)
        ingest(R.LEFT, [-3, R.I64_MIN, 4], [50, 50, 50])          # wholly before
        ingest(R.LEFT, [5, 6, 5, 7, 5, -3], [11, 1, 10, 0, 12, 50])  # interleaved, four ties with the log
        ingest(R.LEFT, np.full(300, 5), np.arange(300) % 4 + 9)   # a large batch of ties
        assert sim.live(R.LEFT) == 316 and op.stats()["merges"] == 5
        _log_view(op, sim, R.LEFT)
        # the right log, probed by the left side
        ingest(R.RIGHT, [5] * 40, np.arange(40) % 3)
        ingest(R.RIGHT, [5] * 40, np.arange(40) % 3)
        _log_view(op, sim, R.RIGHT)


def test_eviction_followed_by_a_merge():
    sim = R.IntervalJoinSim(-2, 5)
    rng = np.random.default_rng(8)
    events = []
    for step in range(6):
        for side in (R.LEFT, R.RIGHT):
            n = 150
            events.append(("ingest", side, rng.integers(0, 6, n), rng.integers(0, 30, n) + 10 * step,
                           np.arange(n, dtype=np.int64) + 1000 * (2 * step + side)))
        events.append(("watermark", 10 * step + 12))
    with W.GpuIntervalJoinOperator(-2, 5, capacity_hint=64) as op:
        _drive(op, sim, events)
        # every call after the first watermark merged into a log that an eviction had compacted,
        # and the calls after it probed that log
        assert sim.late_dropped > 50 and 0 < sim.live(R.LEFT) < 900 and sim.rows_emitted > 1000
        assert op.stats()["merges"] == 12


def test_log_grows_past_capacity_hint():
    sim = R.IntervalJoinSim(0, 3)
    rng = np.random.default_rng(4)
    events = [("ingest", s % 2, rng.integers(0, 50, 700), rng.integers(0, 40, 700), np.arange(700, dtype=np.int64) + 700 * s)
              for s in range(8)]
    with W.GpuIntervalJoinOperator(0, 3, capacity_hint=100) as op:
        _drive(op, sim, events)
        st = op.stats()
        assert st["live_left"] == st["live_right"] == 2800 and sim.rows_emitted > 10_000
        assert st["log_growths"] >= 6 and st["log_capacity_left"] >= 2800 and st["log_capacity_right"] >= 2800


def test_max_batch_passes_equal_one_pass():
    rng = np.random.default_rng(21)
    build = (rng.integers(0, 40, 2500), rng.integers(0, 60, 2500), np.arange(2500, dtype=np.int64))
    probe = (rng.integers(0, 40, 2500), rng.integers(0, 60, 2500), np.arange(2500, dtype=np.int64) + 5000)
    got = []
    for max_batch in (1000, 0):
        with W.GpuIntervalJoinOperator(-2, 2, max_batch=max_batch) as op:
            op.advance_watermark(5)  # some of either call are late
            assert op.process_batch(op.LEFT, *build) == 0
            n = op.process_batch(op.RIGHT, *probe)
            got.append((n, op.drain(), op.num_late_records_dropped(), op.stats()["merges"]))
    sim = R.IntervalJoinSim(-2, 2)
    sim.advance_watermark(5)
    sim.ingest(R.LEFT, *build)
    want = sim.ingest(R.RIGHT, *probe)
    assert len(want[0]) > 5000 and sim.late_dropped > 100
    for n, rows, late, merges in got:
        assert n == len(want[0]) and late == sim.late_dropped
        R.check(rows, want)
    assert (got[0][3], got[1][3]) == (6, 2)


def test_rows_accumulate_drain_in_parts_rows_device_and_clear():
    sim = R.IntervalJoinSim(-1, 1)
    a, b, c = (R.make_records(s, 400, 3, ts_span=30) for s in (1, 2, 3))
    with W.GpuIntervalJoinOperator(-1, 1) as op:
        sim.ingest(R.LEFT, *a)
        op.process_batch(op.LEFT, *a)
        w1, w2 = sim.ingest(R.RIGHT, *b), sim.ingest(R.LEFT, *c)
        n1, n2 = op.process_batch(op.RIGHT, *b), op.process_batch(op.LEFT, *c)
        assert (n1, n2) == (len(w1[0]), len(w2[0])) and n1 > 1000 and n2 > 1000
        want = tuple(np.concatenate([x, y]) for x, y in zip(w1, w2))
        assert op.pending() == n1 + n2
        ptrs, n = op.rows_device()
        assert n == n1 + n2 and all(ptrs)
        # drain in two parts through the C entry point: the first leaves rows behind
        first = n1 + 3
        out = [np.empty(n1 + n2, np.int64) for _ in range(5)]
        got = ctypes.c_int64(0)
        rc = N.lib().gw_ijoin_drain(op._h, *[ctypes.c_void_p(o.ctypes.data) for o in out], first, ctypes.byref(got))
        assert (rc, got.value) == (N.GW_E_OUTPUT_FULL, first) and op.pending() == n2 - 3
        ptrs2, m = op.rows_device()
        assert m == n2 - 3 and ptrs2[0] == ptrs[0] + 8 * first
        rc = N.lib().gw_ijoin_drain(op._h, *[ctypes.c_void_p(o.ctypes.data + 8 * first) for o in out], n2, ctypes.byref(got))
        assert (rc, got.value) == (N.GW_OK, n2 - 3) and op.pending() == 0
        R.check(out, want)
        assert op.rows_device() == ([None] * 5, 0)
        # the rows of a later call start the buffer again; clear_rows drops them
        w3 = sim.ingest(R.RIGHT, *a)
        assert op.process_batch(op.RIGHT, *a) == len(w3[0]) > 0
        op.clear_rows()
        assert op.pending() == 0 and len(op.drain()[0]) == 0
        w4 = sim.ingest(R.LEFT, *b)
        op.process_batch(op.LEFT, *b)
        R.check(op.drain(cap=777), w4)


@pytest.mark.parametrize("bad,code", [(R.I64_MIN, N.GW_E_NO_TIMESTAMP), (R.I64_MAX - 1, N.GW_E_RANGE)])
@pytest.mark.parametrize("max_batch", [0, 100], ids=["one_pass", "passes"])
@pytest.mark.parametrize("device_ingest", [False, True], ids=["host", "device"])
def test_state_after_an_error(bad, code, max_batch, device_ingest):
    """The bad record is in the call's last pass: nothing of the call is taken, and the handle is dead."""
    key, ts, pay = R.make_records(9, 450, 3)
    ts = ts.copy()
    ts[440] = bad
    with W.GpuIntervalJoinOperator(0, 5, max_batch=max_batch) as op:
        op.process_batch(op.RIGHT, *R.make_records(10, 50, 3))
        with pytest.raises(N.GpuWinError) as e:
            if device_ingest:
                d = _dev((key, ts, pay))
                op.process_batch_device(op.LEFT, *d)
            else:
                op.process_batch(op.LEFT, key, ts, pay)
        assert e.value.code == code
        st = op.stats()
        assert (st["live_left"], st["live_right"], st["rows_emitted"], st["merges"]) == (0, 50, 0, 1)
        for call in (lambda: op.process_batch(op.LEFT, key[:3], ts[:3], pay[:3]), lambda: op.advance_watermark(5),
                     op.end_input, op.pending, op.drain, op.rows_device, op.clear_rows, op.last_times):
            with pytest.raises(N.GpuWinError) as e:
                call()
            assert e.value.code == N.GW_E_STATE


def test_late_records_are_not_range_checked_and_invalid_calls_keep_the_handle():
    with W.GpuIntervalJoinOperator(0, 10) as op:
        op.advance_watermark(0)
        assert op.process_batch(op.RIGHT, [1], [R.I64_MIN + 3], [0]) == 0  # late: ts - 10 is never computed
        assert op.num_late_records_dropped() == 1
        with pytest.raises(N.GpuWinError) as e:
            op.process_batch(2, [1], [5], [0])
        assert e.value.code == N.GW_E_INVALID
        assert op.process_batch(op.RIGHT, [1], [5], [0]) == 0  # the handle goes on
        assert op.process_batch(op.LEFT, [1, 1], [0, 5], [1, 2]) == 2
        probe_ms, merge_ms = op.last_times()
        assert probe_ms >= 0 and merge_ms >= 0
    with pytest.raises(ValueError):
        W.GpuIntervalJoinOperator(3, 2)


def test_api_mirror():
    """keyedA.interval_join(keyedB).between().process() with the documented schedule: the sources
    in turn, each up to its next Watermark; the operator's watermark is the minimum of the two."""
    rng = np.random.default_rng(6)

    def source(name, n):
        out, clock = [], 0
        for i in range(n):
            clock += int(rng.integers(0, 4))
            out.append(W.StreamRecord((name, "k%d" % rng.integers(0, 4), i), clock - int(rng.integers(0, 9))))
            if i % 11 == 10:
                out.append(W.Watermark(clock - 3))
        return out

    lefts, rights = source("a", 90), source("b", 70)
    env = W.StreamExecutionEnvironment.get_execution_environment()
    a = env.from_elements(lefts).key_by(lambda v: v[1])
    b = env.from_elements(rights).key_by(lambda v: v[1])
    got = (a.interval_join(b).between(-3, 2).upper_bound_exclusive()
           .process(lambda l, r, ctx: (l, r, ctx.left_timestamp, ctx.right_timestamp, ctx.timestamp)).execute_and_collect())
    # the same schedule through the simulation
    sim = R.IntervalJoinSim(-3, 1)
    ids = {}
    srcs, at, wm_in, want, side = (lefts, rights), [0, 0], [R.I64_MIN, R.I64_MIN], [], 0
    recs = [[e for e in s if isinstance(e, W.StreamRecord)] for s in srcs]
    seen = [0, 0]
    while at[0] < len(lefts) or at[1] < len(rights):
        if at[side] < len(srcs[side]):
            batch, mark = [], None
            while at[side] < len(srcs[side]) and mark is None:
                e = srcs[side][at[side]]
                at[side] += 1
                if isinstance(e, W.Watermark):
                    mark = e.timestamp
                else:
                    batch.append(e)
            rows = sim.ingest(side, [ids.setdefault(e.value[1], len(ids)) for e in batch], [e.timestamp for e in batch],
                              list(range(seen[side], seen[side] + len(batch))))
            seen[side] += len(batch)
            for _, lt, rt, lp, rp in zip(*[c.tolist() for c in rows]):
                want.append(W.StreamRecord((recs[0][lp].value, recs[1][rp].value, lt, rt, max(lt, rt)), max(lt, rt)))
            if mark is not None:
                wm_in[side] = max(wm_in[side], mark)
            if at[side] >= len(srcs[side]):
                wm_in[side] = R.I64_MAX
            sim.advance_watermark(min(wm_in))
        side = 1 - side
    assert len(want) >= 20 and sim.late_dropped > 0  # not vacuous
    assert got == want
    assert all(r.value[0][1] == r.value[1][1] and -3 <= r.value[3] - r.value[2] <= 1 for r in got)
