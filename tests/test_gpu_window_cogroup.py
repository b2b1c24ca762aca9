"""coGroup and outer window joins on the device (gw_join.hip; gw_window_join_outer_device,
gw_window_cogroup_device, gw_join_set_mode and the accessors that go with it) against
tests/cogroup_reference.py, exactly: order, values and `present`.

Shapes are built group by group, so each case names the edge it sits on: the expand tile (1024
output slots, at most 1024 descriptors), the scan tile (1024 groups), a wave (64), a lane's two
rows falling into two descriptors of every kind, and the alignments of the int64 columns and of
the present bytes.  The largest case has about 12,000 tuples.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from flink_amd import _native as N
from flink_amd import windowing as W
from tests import cogroup_reference as C
from tests import join_reference as R
from tests.gpu_helpers import random_stream

pytestmark = pytest.mark.gpu

GEOMETRIES = {"tumbling": (10, 10, 0), "sliding": (10, 5, 0), "sliding_3_1": (10, 3, 1)}
INTERVALS = {"all": (R.I64_MIN, R.I64_MAX), "partial": (-3, 27)}
ALL = INTERVALS["all"]
SENTINEL = 0x5A5A5A5A5A5A5A5A
PSENT = 0x5A
GUARD = 64
MODE_NAMES = list(C.MODES)


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0xffffffff


def assigner(size, slide, offset):
    return W.TumblingEventTimeWindows.of(size, offset) if size == slide else W.SlidingEventTimeWindows.of(size, slide, offset)


def _dev(cols):
    # (one element when empty: an empty tensor has no pointer; the length travels separately)
    return [torch.from_numpy(np.resize(np.ascontiguousarray(c), max(len(c), 1))).cuda() for c in cols]


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _outer(left, right, geom, interval, mode, cap, at=0, pat=None, present=True):
    """gw_window_join_outer_device into sentinel-filled columns of cap + GUARD rows, the int64
    columns starting `at` rows and the present bytes `pat` (default: at) bytes into their
    tensors.  (rc, n_out, the six columns from their start, as numpy)."""
    pat = at if pat is None else pat
    dl, dr = _dev(left), _dev(right)
    out = [torch.full((cap + GUARD + at,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(5)]
    pres = torch.full((cap + GUARD + pat,), PSENT, dtype=torch.uint8, device="cuda")
    n_out = ctypes.c_int64(-7)
    torch.cuda.synchronize()
    rc = N.lib().gw_window_join_outer_device(len(left[0]), *[_P(t) for t in dl], len(right[0]), *[_P(t) for t in dr], *geom,
                                             *interval, mode, C.NULL, *[ctypes.c_void_p(o.data_ptr() + 8 * at) for o in out],
                                             ctypes.c_void_p(pres.data_ptr() + pat) if present else None, cap,
                                             ctypes.byref(n_out), None)
    return rc, n_out.value, [o.cpu().numpy()[at:] for o in out] + [pres.cpu().numpy()[pat:]]


def _check_outer(left, right, geom, interval, mode, want, at=0, pat=None):
    need = len(want[0])
    rc, n, out = _outer(left, right, geom, interval, mode, need, at, pat)
    assert (rc, n) == (N.GW_OK, need)
    C.check_rows([o[:need] for o in out], want)
    assert all((o[need:] == SENTINEL).all() for o in out[:5]) and (out[5][need:] == PSENT).all()


def _cogroup(left, right, geom, interval, caps):
    """gw_window_cogroup_device into sentinel-filled columns.  (rc, n_out[3], the seven columns)."""
    dl, dr = _dev(left), _dev(right)
    F = lambda k: torch.full((k + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    g = [F(caps[0]) for _ in range(3)] + [F(caps[0] + 1) for _ in range(2)]
    le, re = F(caps[1]), F(caps[2])
    n = (ctypes.c_int64 * 3)(-7, -7, -7)
    torch.cuda.synchronize()
    rc = N.lib().gw_window_cogroup_device(len(left[0]), *[_P(t) for t in dl], len(right[0]), *[_P(t) for t in dr], *geom,
                                          *interval, *[_P(x) for x in g], _P(le), caps[1], _P(re), caps[2], caps[0], n, None)
    return rc, tuple(n), [x.cpu().numpy() for x in g + [le, re]]


def _check_cogroup(left, right, geom, interval, want):
    need = (len(want[0]), len(want[5]), len(want[6]))
    rc, n, out = _cogroup(left, right, geom, interval, need)
    assert rc == N.GW_OK and n == need
    ends = (n[0], n[0], n[0], n[0] + 1, n[0] + 1, n[1], n[2])
    C.check_csr([o[:k] for o, k in zip(out, ends)], want)
    assert all((o[k:] == SENTINEL).all() for o, k in zip(out, ends))


# ---- shapes built group by group ---------------------------------------------------------------
def _from_groups(spec, seed=0):
    """spec: per key 0, 1, .. its (L, R) in one tumbling window [0, 10); arrival shuffled, payloads
    distinct.  (left, right) columns."""
    rng = np.random.default_rng(seed)
    sides = []
    for sd in (0, 1):
        key = np.repeat(np.arange(len(spec), dtype=np.int64), [g[sd] for g in spec])
        key = key[rng.permutation(len(key))]
        ts = rng.integers(0, 10, len(key)).astype(np.int64)
        pay = (np.arange(len(key), dtype=np.int64) * 2 + sd) * 1_000_003 + 17
        sides.append((key, ts, pay))
    return sides[0], sides[1]


def _spec(kind, t):
    if kind == "mixed":      # left only, right only, 1 x 1 in turn: a row each in full outer, and a lane's
        return [((1, 0), (0, 1), (1, 1))[i % 3] for i in range(t)]          # two rows of every two kinds
    if kind == "mixed_rev":  # the same transitions in the other direction
        return [((1, 1), (0, 1), (1, 0))[i % 3] for i in range(t)]
    if kind == "one_sided":  # every descriptor one-sided with a single row
        return [((1, 0), (0, 1))[i % 2] for i in range(t)]
    if kind == "left_wide":  # one left-only descriptor over the whole output
        return [(t, 0)]
    if kind == "right_wide":
        return [(0, t)]
    if kind == "runs":       # one-sided groups of several rows next to products
        return [((3, 0), (2, 2), (0, 5), (1, 3), (4, 0), (0, 1))[i % 6] for i in range(t)]
    raise KeyError(kind)


TOTALS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049]
TUMBLING = GEOMETRIES["tumbling"]
_shape_ref = {}


def _shape(kind, t):
    if (kind, t) not in _shape_ref:
        left, right = _from_groups(_spec(kind, t), _seed(kind, t))
        _shape_ref[(kind, t)] = (left, right, C.fired_groups(left, right, *TUMBLING))
    return _shape_ref[(kind, t)]


@pytest.mark.parametrize("t", TOTALS)
@pytest.mark.parametrize("kind", ["mixed", "mixed_rev", "one_sided", "left_wide", "right_wide", "runs"])
def test_group_shapes_in_every_mode(kind, t):
    """t groups (or one group of t records): t rows in full outer for the single-row kinds, so
    the totals sit around the expand tile, its descriptor limit, the scan tile and a wave."""
    left, right, groups = _shape(kind, t)
    full = C.emit_rows(groups, 10, C.FULL_OUTER)
    if kind != "runs":
        assert len(full[0]) == t
    for name, mode in C.MODES.items():
        _check_outer(left, right, TUMBLING, ALL, mode, C.emit_rows(groups, 10, mode))
    _check_cogroup(left, right, TUMBLING, ALL, C.emit_csr(groups, 10))


# ---- one large group among singles, at every alignment -----------------------------------------
_skew_ref = {}


def _skew(singles):
    """One group of 4096 x 64 on key 2500 among `singles` groups of one record per side at most:
    even keys 1 x 1, odd keys left only and right only in turn."""
    if singles not in _skew_ref:
        spec = [(1, 1) if k % 2 == 0 else ((1, 0), (0, 1))[(k // 2) % 2] for k in range(singles + 1)]
        spec[2500] = (4096, 64)
        left, right = _from_groups(spec, singles)
        groups = C.fired_groups(left, right, *TUMBLING)
        _skew_ref[singles] = (left, right, {m: C.emit_rows(groups, 10, m) for m in C.MODES.values()}, C.emit_csr(groups, 10))
    return _skew_ref[singles]


@pytest.mark.parametrize("singles", [5000, 4999])
@pytest.mark.parametrize("at,pat", [(0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (1, 0)])
def test_skew_full_outer_at_every_alignment(singles, at, pat):
    """Tile boundaries fall inside the large group and between the singles, half of them
    unmatched.  Row offsets 0 .. 3 give the int64 columns both 16-byte phases and the present
    bytes their aligned 2-byte stores; (0, 1) and (1, 0) give the present bytes the other parity
    (byte stores).  5000 singles: an even total; 4999: an odd one, a tail of one row."""
    left, right, want, _ = _skew(singles)
    need = 4096 * 64 + singles
    assert len(want[C.FULL_OUTER][0]) == need and int((want[C.FULL_OUTER][5] != 3).sum()) in (2499, 2500)
    _check_outer(left, right, TUMBLING, ALL, C.FULL_OUTER, want[C.FULL_OUTER], at, pat)


@pytest.mark.parametrize("name", ["inner", "left_outer", "right_outer"])
def test_skew_other_modes_and_csr(name):
    left, right, want, csr = _skew(4999)
    _check_outer(left, right, TUMBLING, ALL, C.MODES[name], want[C.MODES[name]], at=1)
    if name == "inner":
        _check_cogroup(left, right, TUMBLING, ALL, csr)


# ---- seeded records: key distributions, geometries, intervals ----------------------------------
_ref = {}


def _inputs(keys, geometry, interval):
    case = (keys, geometry, interval)
    if case not in _ref:
        if keys == "one":      # one group per window, spanning expand tiles
            left, right = R.make_records(_seed(case), 120, 90, num_keys=1, ts_lo=0, ts_span=10)
        elif keys == "seven":
            left, right = R.make_records(_seed(case), 1025, 700, num_keys=7, ts_span=200)
        else:                  # as many keys as records: nearly every group one-sided
            left, right = R.make_records(_seed(case), 1500, 1300, num_keys=2800)
        _ref[case] = (left, right, C.fired_groups(left, right, *GEOMETRIES[geometry], *INTERVALS[interval]))
    return _ref[case]


@pytest.mark.parametrize("interval", list(INTERVALS))
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("keys", ["one", "seven", "many"])
def test_device_matches_reference(keys, geometry, interval):
    left, right, groups = _inputs(keys, geometry, interval)
    geom, iv = GEOMETRIES[geometry], INTERVALS[interval]
    full = C.emit_rows(groups, geom[0], C.FULL_OUTER)
    assert len(full[0]) > 0 and (full[5] == 3).any()
    assert keys != "many" or ((full[5] == 1).any() and (full[5] == 2).any())
    for name, mode in C.MODES.items():
        _check_outer(left, right, geom, iv, mode, C.emit_rows(groups, geom[0], mode))
    _check_cogroup(left, right, geom, iv, C.emit_csr(groups, geom[0]))
    # the Python wrappers
    dl, dr = _dev(left), _dev(right)
    got = W.window_join_outer_device(*dl, *dr, assigner(*geom), "full_outer", C.NULL, *iv)
    C.check_rows([g.cpu().numpy() for g in got], full)
    got = W.window_cogroup_device(*dl, *dr, assigner(*geom), *iv)
    C.check_csr([g.cpu().numpy() for g in got], C.emit_csr(groups, geom[0]))


@pytest.mark.parametrize("name", MODE_NAMES)
def test_one_side_empty(name):
    """A call with one empty side is not empty where the mode keeps the other side."""
    mode = C.MODES[name]
    left, right = R.make_records(9, 700, 900, 7)
    none = tuple(np.empty(0, np.int64) for _ in range(3))
    for l, r in ((none, right), (left, none), (none, none)):
        groups = C.fired_groups(l, r, 10, 5, 0)
        want = C.emit_rows(groups, 10, mode)
        kept = (len(r[0]) if mode & 2 and not len(l[0]) else 0) + (len(l[0]) if mode & 1 and not len(r[0]) else 0)
        assert len(want[0]) == 2 * kept  # every record in its two windows
        _check_outer(l, r, (10, 5, 0), ALL, mode, want)
        if name == "inner":
            _check_cogroup(l, r, (10, 5, 0), ALL, C.emit_csr(groups, 10))


def test_present_may_be_null():
    left, right, groups = _shape("runs", 1025)
    want = C.emit_rows(groups, 10, C.FULL_OUTER)
    need = len(want[0])
    rc, n, out = _outer(left, right, TUMBLING, ALL, C.FULL_OUTER, need, present=False)
    assert (rc, n) == (N.GW_OK, need)
    C.check_rows([o[:need] for o in out[:5]], want)
    assert (out[5] == PSENT).all()


def test_inner_mode_is_the_inner_join():
    """mode 0 against gw_window_join_device's own output, present all 3."""
    left, right, groups = _inputs("seven", "sliding_3_1", "all")
    dl, dr = _dev(left), _dev(right)
    a = assigner(*GEOMETRIES["sliding_3_1"])
    inner = [t.cpu().numpy() for t in W.window_join_device(*dl, *dr, a)]
    assert len(inner[0]) > 2048
    got = [t.cpu().numpy() for t in W.window_join_outer_device(*dl, *dr, a, "inner", C.NULL)]
    R.check(got[:5], inner)
    assert (got[5] == 3).all()
    R.check(C.expand_csr([t.cpu().numpy() for t in W.window_cogroup_device(*dl, *dr, a)]), inner)


def test_caps_exact_and_one_short():
    left, right, groups = _shape("runs", 1025)
    want = C.emit_rows(groups, 10, C.FULL_OUTER)
    need = len(want[0])
    for cap in (need - 1, 0):
        rc, n, out = _outer(left, right, TUMBLING, ALL, C.FULL_OUTER, cap)
        assert (rc, n) == (N.GW_E_OUTPUT_FULL, need)
        assert all((o == SENTINEL).all() for o in out[:5]) and (out[5] == PSENT).all()
    csr = C.emit_csr(groups, 10)
    need3 = (len(csr[0]), len(csr[5]), len(csr[6]))
    for short in range(3):
        caps = tuple(need3[i] - (i == short) for i in range(3))
        rc, n, out = _cogroup(left, right, TUMBLING, ALL, caps)
        assert rc == N.GW_E_OUTPUT_FULL and n == need3
        assert all((o == SENTINEL).all() for o in out)
    _check_cogroup(left, right, TUMBLING, ALL, csr)


def test_device_errors():
    one = (np.array([1], np.int64), np.array([5], np.int64), np.array([9], np.int64))
    none = tuple(np.empty(0, np.int64) for _ in range(3))
    many = R.make_records(3, 3000, 3000, 7)[0]
    for bad_ts, code in ((R.I64_MIN, N.GW_E_NO_TIMESTAMP), (R.I64_MAX - 2, N.GW_E_RANGE)):
        bad = (many[0], many[1].copy(), many[2])
        bad[1][2900] = bad_ts
        assert _outer(bad, none, TUMBLING, ALL, C.LEFT_OUTER, 64)[0] == code
        assert _outer(one, bad, TUMBLING, ALL, C.FULL_OUTER, 64)[0] == code
        assert _cogroup(none, bad, TUMBLING, ALL, (64, 64, 64))[0] == code
    for mode in (-1, 4):
        assert _outer(one, one, TUMBLING, ALL, mode, 16)[0] == N.GW_E_INVALID
    assert _outer(one, none, (65, 1, 0), ALL, C.LEFT_OUTER, 128)[0] == N.GW_E_UNSUPPORTED
    rc, n, out = _outer(none, one, (64, 1, 0), ALL, C.RIGHT_OUTER, 128)
    assert (rc, n) == (N.GW_OK, 64) and out[1][:64].tolist() == list(range(-58, 6)) and (out[5][:64] == 2).all()
    assert _cogroup(one, one, (10, 5, 5), ALL, (16, 16, 16))[0] == N.GW_E_INVALID
    rc, n, out = _cogroup(one, one, TUMBLING, (20, 20), (4, 4, 4))
    assert rc == N.GW_OK and n == (0, 0, 0) and out[3][0] == 0 and out[4][0] == 0


# ---- the operator ------------------------------------------------------------------------------
def _streams(seed, geometry):
    """Two seeded streams over different key ranges that overlap (keys 0 .. 4 left, 2 .. 6 right),
    bounded disorder beyond the watermark lag (some records late), cut into 6 and 7 batches."""
    size = GEOMETRIES[geometry][0]
    sides = []
    for sd, nb in ((0, 6), (1, 7)):
        keys, ts, _, batches = random_stream(seed * 2 + sd, 420, 5, nb, ts_step=1, disorder=6 * size, wm_lag=size // 2,
                                             key_offset=2 * sd)
        pay = np.arange(len(keys), dtype=np.int64) * 2 + sd + 1000 * (seed + 1)
        sides.append((keys, ts, pay, batches))
    return sides


@pytest.mark.parametrize("device_ingest", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("name", MODE_NAMES + ["cogroup"])
def test_operator_matches_reference(name, geometry, device_ingest):
    size, slide, offset = GEOMETRIES[geometry]
    mode = C.COGROUP if name == "cogroup" else C.MODES[name]
    sides = _streams(1, geometry)
    ref = C.ReferenceCoGroupOperator(size, slide, offset, mode=mode)
    want, got_csr = [], []
    side_stream = torch.cuda.Stream() if device_ingest else None
    with W.GpuWindowJoinOperator(assigner(size, slide, offset), capacity_hint=16, max_batch=16, mode=name,
                                 null_payload=C.NULL) as op:
        wm_in = [R.I64_MIN, R.I64_MIN]
        for b in range(7):
            for sd, (keys, ts, pay, batches) in enumerate(sides):
                if b >= len(batches):
                    continue
                lo, hi, wm = batches[b]
                cols = (keys[lo:hi], ts[lo:hi], pay[lo:hi])
                ref.ingest(sd, *cols)
                if device_ingest:
                    with torch.cuda.stream(side_stream):
                        d = [torch.from_numpy(np.ascontiguousarray(c)).cuda(non_blocking=False) for c in cols]
                        op.process_batch_device(sd, *d)
                        del d  # freed in stream order: the operator made the stream wait for its reads
                else:
                    op.process_batch(sd, *cols)
                wm_in[sd] = wm
            wm = min(wm_in)
            out = ref.advance_watermark(wm)
            want.append(out)
            assert op.advance_watermark(wm) == len(out[0])
            assert op.advance_watermark(wm) == 0       # does not advance: ignored
            assert op.num_late_records_dropped() == ref.late_dropped
            st = op.stats()
            assert (st["live_left"], st["live_right"]) == (ref.live_records(0), ref.live_records(1))
            if mode == C.COGROUP and b % 3 == 2:       # three watermarks' groups in one CSR, drained once
                assert op.cogroup_pending() == tuple(sum(len(w[c]) for w in want) for c in (0, 5, 6))
                got_csr.append(op.cogroup_drain())
                C.check_csr(got_csr[-1], C.concat_csr(want))
                assert op.cogroup_pending() == (0, 0, 0)
                want = []
        out = ref.end_input()
        want.append(out)
        assert op.end_input() == len(out[0])
        st = op.stats()
        assert (st["live_left"], st["live_right"]) == (0, 0)
        assert st["pairs_fired"] == ref.fired and ref.fired > 100 and ref.late_dropped > 0
        assert st["log_growths"] >= 5
        if mode == C.COGROUP:
            assert len(got_csr) == 2 and all(len(g[0]) > 0 for g in got_csr)
            ptrs, n = op.cogroup_rows_device()
            assert n == op.cogroup_pending() and all(p for p in ptrs[:5])
            C.check_csr(op.cogroup_drain(), C.concat_csr(want))
            assert op.cogroup_pending() == (0, 0, 0)
            sizes = [np.diff(g[3]) + np.diff(g[4]) for g in got_csr]
            assert all((s > 0).all() for s in sizes)
        else:
            assert op.pending() == ref.fired
            all_rows = [np.concatenate([w[c] for w in want]) for c in range(6)]
            if name != "inner":
                assert (all_rows[5] != 3).any()
            # rows of every fire accumulated; drained 37 at a time (GW_E_OUTPUT_FULL until the last)
            C.check_rows(op.drain_outer(cap=37), all_rows)
            assert op.pending() == 0
    if side_stream is not None:
        side_stream.synchronize()


def test_operator_drain_without_present_and_device_view():
    left, right, groups = _shape("runs", 64)
    want = C.emit_rows(groups, 10, C.FULL_OUTER)
    with W.GpuWindowJoinOperator(assigner(*TUMBLING), mode="full_outer", null_payload=C.NULL) as op:
        op.process_batch(0, *left)
        op.process_batch(1, *right)
        assert op.end_input() == len(want[0])
        ptrs, n = op.rows_device_outer()
        assert n == len(want[0]) and all(ptrs)
        assert ptrs[:5] == op.rows_device()[0]
        C.check_rows(op.drain(), want)         # the five columns alone
        assert op.pending() == 0
        ptrs, n = op.rows_device_outer()
        assert n == 0 and not any(ptrs)
        op.clear_rows()


def test_operator_mode_errors():
    one = np.array([1], np.int64)
    a = W.TumblingEventTimeWindows.of(10)
    with W.GpuWindowJoinOperator(a) as op:       # untouched: inner
        op.set_mode("left_outer", 5)
        op.set_mode("inner")
        op.process_batch(0, one, one, one)
        with pytest.raises(N.GpuWinError) as e:
            op.set_mode("full_outer")
        assert e.value.code == N.GW_E_STATE
        assert op.end_input() == 0                # it goes on as an inner join
        for call in (op.cogroup_pending, op.cogroup_drain, op.cogroup_rows_device):
            with pytest.raises(N.GpuWinError) as e:
                call()
            assert e.value.code == N.GW_E_INVALID
        assert op.pending() == 0
    with W.GpuWindowJoinOperator(a) as op:
        op.advance_watermark(5)
        with pytest.raises(N.GpuWinError) as e:
            op.set_mode("cogroup")
        assert e.value.code == N.GW_E_STATE
    with W.GpuWindowJoinOperator(a, mode="cogroup") as op:
        op.process_batch(1, one, one, one)
        assert op.end_input() == 1
        for call in (op.pending, op.drain, op.drain_outer, op.rows_device, op.rows_device_outer):
            with pytest.raises(N.GpuWinError) as e:
                call()
            assert e.value.code == N.GW_E_INVALID
        assert op.cogroup_pending() == (1, 0, 1)
        op.clear_rows()
        assert op.cogroup_pending() == (0, 0, 0)
        key, start, end, loff, roff, le, re = op.cogroup_drain()
        assert len(key) == 0 and loff.tolist() == [0] and roff.tolist() == [0]
        with pytest.raises(N.GpuWinError) as e:
            N.check(N.lib().gw_join_set_mode(op._h, 5, 0))
        assert e.value.code == N.GW_E_INVALID
    with pytest.raises(ValueError):
        W.GpuWindowJoinOperator(a, mode="outer")


def test_cogroup_drain_is_all_or_nothing():
    left, right, groups = _shape("runs", 64)
    want = C.emit_csr(groups, 10)
    need = (len(want[0]), len(want[5]), len(want[6]))
    with W.GpuWindowJoinOperator(assigner(*TUMBLING), mode="cogroup") as op:
        op.process_batch(0, *left)
        op.process_batch(1, *right)
        assert op.end_input() == need[0]
        for short in range(3):
            caps = [need[i] - (i == short) for i in range(3)]
            g = [np.full(caps[0] + 1, SENTINEL, np.int64) for _ in range(5)]
            le, re = np.full(caps[1] + 1, SENTINEL, np.int64), np.full(caps[2] + 1, SENTINEL, np.int64)
            n = (ctypes.c_int64 * 3)()
            rc = N.lib().gw_join_cogroup_drain(op._h, *[x.ctypes.data for x in g], le.ctypes.data, caps[1], re.ctypes.data,
                                               caps[2], caps[0], n)
            assert rc == N.GW_E_OUTPUT_FULL and tuple(n) == need
            assert all((x == SENTINEL).all() for x in g + [le, re])
            assert op.cogroup_pending() == need
        C.check_csr(op.cogroup_drain(), want)


# ---- composition: full-outer rows -> network-buffer bytes --------------------------------------
def test_full_outer_rows_encode_as_tuple3_rows():
    """rows_device() columns of a full outer join into gw_encode_rows_device as Tuple3<Long, Long,
    Long>(key, left payload, right payload), decoded again: the rows come back, each stamped
    end - 1, the lacking sides as null_payload."""
    left, right = R.make_records(11, 500, 400, 40)
    want = C.reference_rows(left, right, 10, 5, 0, C.FULL_OUTER)
    n = len(want[0])
    assert n > 1000 and (want[5] == 1).any() and (want[5] == 2).any()
    with W.GpuWindowJoinOperator(W.SlidingEventTimeWindows.of(10, 5), mode="full_outer", null_payload=C.NULL) as op:
        op.process_batch(0, *left)
        op.process_batch(1, *right)
        assert op.end_input() == n
        ptrs, got_n = op.rows_device()
        assert got_n == n
        lay = N.row_layout("JJJ", (N.GW_ROW_KEY, N.GW_ROW_RESULT, N.GW_ROW_PAYLOAD))
        row = N.lib().gw_row_encoded_bytes(ctypes.byref(lay))
        buf = torch.full((n * row + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        off, nb = np.zeros(1, np.int64), np.zeros(1, np.int64)
        V = ctypes.c_void_p
        rc = N.lib().gw_encode_rows_device(n, V(ptrs[0]), V(ptrs[1]), V(ptrs[2]), V(ptrs[3]), V(ptrs[4]), ctypes.byref(lay),
                                           0, 1, 128, N.NO_WATERMARK, V(buf.data_ptr()), buf.numel(), off.ctypes.data,
                                           nb.ctypes.data, V(op.stream))
        assert rc == N.GW_OK and nb[0] == n * row
        op.clear_rows()
    fields = []
    for value_field in (1, 2):
        k, t, v = (torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(3))
        wp, wv = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(2))
        res = N.GwDecodeResult()
        rl = N.record_layout("JJJ", 0, value_field)
        rc = N.lib().gw_decode_serialized(_P(buf), int(nb[0]), ctypes.byref(rl), _P(k), _P(t), _P(v), n + 1, _P(wp), _P(wv), 4,
                                          ctypes.byref(res), None)
        assert rc == N.GW_OK and res.records == n and res.consumed == nb[0]
        fields.append((k[:n].cpu().numpy(), t[:n].cpu().numpy(), v[:n].cpu().numpy()))
    assert np.array_equal(fields[0][0], want[0]) and np.array_equal(fields[0][1], want[2] - 1)
    assert np.array_equal(fields[0][2], want[3]) and np.array_equal(fields[1][2], want[4])
    assert (fields[0][2][want[5] == 2] == C.NULL).all() and (fields[1][2][want[5] == 1] == C.NULL).all()


# ---- the API mirror ----------------------------------------------------------------------------
SR = W.StreamRecord
PERSONS = [SR(("p", 1, "ann"), 1), SR(("p", 2, "bob"), 3), SR(("p", 3, "cy"), 12), SR(("p", 1, "ann2"), 14),
           SR(("p", 9, "zed"), 15), W.Watermark(9)]
AUCTIONS = [SR(("a", 100, 2), 2), SR(("a", 101, 1), 5), SR(("a", 102, 1), 9), SR(("a", 103, 3), 8),
            SR(("a", 104, 1), 11), SR(("a", 105, 3), 19), SR(("a", 106, 7), 13)]


def _co_group():
    env_p = W.StreamExecutionEnvironment.get_execution_environment()
    env_a = W.StreamExecutionEnvironment.get_execution_environment()
    return (env_p.from_elements(PERSONS).co_group(env_a.from_elements(AUCTIONS))
            .where(lambda p: p[1]).equal_to(lambda a: a[2]).window(W.TumblingEventTimeWindows.of(10)))


def test_co_group_api_mirror():
    """Sellers with their auctions per window, those without auctions included (a Q8 variant)."""
    out = _co_group().apply(lambda ps, as_: [([p[2] for p in ps], [a[1] for a in as_])]).execute_and_collect()
    assert [(r.value, r.timestamp) for r in out] == [
        ((["ann"], [101, 102]), 9), ((["bob"], [100]), 9), (([], [103]), 9),
        ((["ann2"], [104]), 19), ((["cy"], [105]), 19), (([], [106]), 19), ((["zed"], []), 19)]
    # a function that emits nothing for some groups and several outputs for others
    out = _co_group().apply(lambda ps, as_: [a[1] for a in as_] if ps else []).execute_and_collect()
    assert [r.value for r in out] == [101, 102, 100, 104, 105]


def test_outer_join_api_mirror():
    f = lambda p, a: (p[2] if p else None, a[1] if a else None)
    full = _co_group().apply(W.OuterJoin("full", f)).execute_and_collect()
    assert [(r.value, r.timestamp) for r in full] == [
        (("ann", 101), 9), (("ann", 102), 9), (("bob", 100), 9), ((None, 103), 9),
        (("ann2", 104), 19), (("cy", 105), 19), ((None, 106), 19), (("zed", None), 19)]
    left = _co_group().apply(W.OuterJoin("left", f)).execute_and_collect()
    assert [r.value for r in left] == [("ann", 101), ("ann", 102), ("bob", 100), ("ann2", 104), ("cy", 105), ("zed", None)]
    right = _co_group().apply(W.OuterJoin("right", f)).execute_and_collect()
    assert [r.value for r in right] == [("ann", 101), ("ann", 102), ("bob", 100), (None, 103), ("ann2", 104), ("cy", 105),
                                        (None, 106)]
