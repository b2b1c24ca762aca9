"""gw_window_join_outer_host and gw_window_cogroup_host: the coGroup / outer-join contract
(include/gpuwin.h) as plain host code through the C ABI, against tests/cogroup_reference.py
exactly, in order and values.  Runs without a GPU."""
import ctypes
import zlib

import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import windowing as W
from tests import cogroup_reference as C
from tests import join_reference as R

GEOMETRIES = {"tumbling": (10, 10, 0), "sliding": (10, 5, 0), "sliding_3_1": (10, 3, 1)}
INTERVALS = {"all": (R.I64_MIN, R.I64_MAX), "partial": (-3, 27)}
SENTINEL = 0x5A5A5A5A5A5A5A5A
NONE = tuple(np.empty(0, np.int64) for _ in range(3))
ONE = (np.array([1], np.int64), np.array([5], np.int64), np.array([9], np.int64))


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0xffffffff


def assigner(size, slide, offset):
    return W.TumblingEventTimeWindows.of(size, offset) if size == slide else W.SlidingEventTimeWindows.of(size, slide, offset)


def _P(a):
    return ctypes.c_void_p(a.ctypes.data) if len(a) else None


def _outer(left, right, size, slide, offset, w0, w1, mode, cap, present=True):
    """(rc, n_out, six sentinel-filled output columns of max(cap, 1) + 8 rows)."""
    out = [np.full(max(cap, 1) + 8, SENTINEL, np.int64) for _ in range(5)] + [np.full(max(cap, 1) + 8, 0x5A, np.uint8)]
    n_out = ctypes.c_int64(-7)
    rc = N.lib().gw_window_join_outer_host(len(left[0]), *[_P(c) for c in left], len(right[0]), *[_P(c) for c in right],
                                           size, slide, offset, w0, w1, mode, C.NULL, *[o.ctypes.data for o in out[:5]],
                                           out[5].ctypes.data if present else None, cap, ctypes.byref(n_out))
    return rc, n_out.value, out


def _cogroup(left, right, size, slide, offset, w0, w1, caps):
    """(rc, n_out[3], seven sentinel-filled output columns); caps = (groups, left, right)."""
    g = [np.full(caps[0] + 8, SENTINEL, np.int64) for _ in range(3)] + [np.full(caps[0] + 9, SENTINEL, np.int64) for _ in range(2)]
    le, re = np.full(caps[1] + 8, SENTINEL, np.int64), np.full(caps[2] + 8, SENTINEL, np.int64)
    n = (ctypes.c_int64 * 3)(-7, -7, -7)
    rc = N.lib().gw_window_cogroup_host(len(left[0]), *[_P(c) for c in left], len(right[0]), *[_P(c) for c in right],
                                        size, slide, offset, w0, w1, *[x.ctypes.data for x in g], le.ctypes.data, caps[1],
                                        re.ctypes.data, caps[2], caps[0], n)
    return rc, tuple(n), g + [le, re]


@pytest.mark.parametrize("interval", list(INTERVALS))
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("num_keys", [1, 7, 500])
@pytest.mark.parametrize("n_r", [0, 1, 64, 300])
@pytest.mark.parametrize("n_l", [0, 1, 64, 300])
def test_host_matches_reference(n_l, n_r, num_keys, geometry, interval):
    size, slide, offset = GEOMETRIES[geometry]
    w0, w1 = INTERVALS[interval]
    left, right = R.make_records(_seed(n_l, n_r, num_keys, geometry), n_l, n_r, num_keys)
    groups = C.fired_groups(left, right, size, slide, offset, w0, w1)
    a = assigner(size, slide, offset)
    for name, mode in C.MODES.items():
        want = C.emit_rows(groups, size, mode)
        C.check_rows(W.window_join_outer_host(*left, *right, a, name, C.NULL, w0, w1), want)
        if mode == C.INNER:
            R.check(W.window_join_host(*left, *right, a, w0, w1), want[:5])
            assert (want[5] == 3).all()
    C.check_csr(W.window_cogroup_host(*left, *right, a, w0, w1), C.emit_csr(groups, size))
    if n_l + n_r >= 64 and interval == "all":
        assert len(groups) > 0


def test_one_side_empty_per_mode():
    left, right = R.make_records(9, 40, 50, 7)
    for l, r in ((NONE, right), (left, NONE), (NONE, NONE)):
        groups = C.fired_groups(l, r, 10, 5, 0)
        for mode in C.MODES.values():
            want = C.emit_rows(groups, 10, mode)
            rc, n, out = _outer(l, r, 10, 5, 0, R.I64_MIN, R.I64_MAX, mode, 200)
            assert (rc, n) == (N.GW_OK, len(want[0]))
            C.check_rows([o[:n] for o in out], want)
        rc, n, out = _cogroup(l, r, 10, 5, 0, R.I64_MIN, R.I64_MAX, (200, 200, 200))
        want = C.emit_csr(groups, 10)
        assert rc == N.GW_OK and n == (len(want[0]), len(want[5]), len(want[6]))
        C.check_csr([out[0][:n[0]], out[1][:n[0]], out[2][:n[0]], out[3][:n[0] + 1], out[4][:n[0] + 1], out[5][:n[1]],
                     out[6][:n[2]]], want)
    assert len(C.reference_rows(NONE, right, 10, 5, 0, C.RIGHT_OUTER)[0]) == 100  # every right tuple, two windows each
    assert len(C.reference_rows(NONE, right, 10, 5, 0, C.LEFT_OUTER)[0]) == 0


def test_all_groups_one_sided():
    """Disjoint keys: the inner join is empty, each outer mode gives its side's tuples."""
    left, right = R.make_records(4, 70, 90, 7)
    right = (right[0] ^ 0x100, right[1], right[2])
    a = assigner(10, 5, 0)
    got = {name: W.window_join_outer_host(*left, *right, a, name, C.NULL) for name in C.MODES}
    assert len(got["inner"][0]) == 0
    assert len(got["left_outer"][0]) == 140 and len(got["right_outer"][0]) == 180 and len(got["full_outer"][0]) == 320
    for name, mode in C.MODES.items():
        C.check_rows(got[name], C.reference_rows(left, right, 10, 5, 0, mode))
    csr = W.window_cogroup_host(*left, *right, a)
    C.check_csr(csr, C.reference_csr(left, right, 10, 5, 0))
    assert ((np.diff(csr[3]) == 0) | (np.diff(csr[4]) == 0)).all()


def test_present_may_be_null():
    left, right = R.make_records(6, 64, 64, 20)
    want = C.reference_rows(left, right, 10, 5, 0, C.FULL_OUTER)
    rc, n, out = _outer(left, right, 10, 5, 0, R.I64_MIN, R.I64_MAX, C.FULL_OUTER, len(want[0]), present=False)
    assert (rc, n) == (N.GW_OK, len(want[0]))
    C.check_rows([o[:n] for o in out[:5]], want)
    assert (out[5] == 0x5A).all()


def test_outer_output_full_reports_the_count_and_writes_nothing():
    left, right = R.make_records(5, 64, 64, 20)
    want = C.reference_rows(left, right, 10, 5, 0, C.FULL_OUTER)
    need = len(want[0])
    assert need > 10 and 0 < int((want[5] != 3).sum()) < need
    for cap in (0, 1, need - 1):
        rc, n, out = _outer(left, right, 10, 5, 0, R.I64_MIN, R.I64_MAX, C.FULL_OUTER, cap)
        assert (rc, n) == (N.GW_E_OUTPUT_FULL, need)
        assert all((o == SENTINEL).all() for o in out[:5]) and (out[5] == 0x5A).all()
    rc, n, out = _outer(left, right, 10, 5, 0, R.I64_MIN, R.I64_MAX, C.FULL_OUTER, need)
    assert (rc, n) == (N.GW_OK, need)
    C.check_rows([o[:need] for o in out], want)
    assert all((o[need:] == SENTINEL).all() for o in out[:5]) and (out[5][need:] == 0x5A).all()


def test_cogroup_output_full_for_each_of_the_three_caps():
    left, right = R.make_records(5, 64, 80, 20)
    want = C.reference_csr(left, right, 10, 5, 0)
    need = (len(want[0]), len(want[5]), len(want[6]))
    assert min(need) > 10
    for short in range(3):
        for cut in (1, need[short]):
            caps = tuple(need[i] - cut if i == short else need[i] for i in range(3))
            rc, n, out = _cogroup(left, right, 10, 5, 0, R.I64_MIN, R.I64_MAX, caps)
            assert rc == N.GW_E_OUTPUT_FULL and n == need
            assert all((o == SENTINEL).all() for o in out)
    rc, n, out = _cogroup(left, right, 10, 5, 0, R.I64_MIN, R.I64_MAX, need)
    assert rc == N.GW_OK and n == need
    C.check_csr([out[0][:n[0]], out[1][:n[0]], out[2][:n[0]], out[3][:n[0] + 1], out[4][:n[0] + 1], out[5][:n[1]],
                 out[6][:n[2]]], want)
    assert all((o[k:] == SENTINEL).all() for o, k in zip(out, (n[0], n[0], n[0], n[0] + 1, n[0] + 1, n[1], n[2])))


def test_errors():
    no_ts = (ONE[0], np.array([R.I64_MIN], np.int64), ONE[2])
    far = (ONE[0], np.array([R.I64_MAX - 2], np.int64), ONE[2])
    A = (R.I64_MIN, R.I64_MAX)
    for bad, code in ((no_ts, N.GW_E_NO_TIMESTAMP), (far, N.GW_E_RANGE)):
        for left, right in ((bad, ONE), (ONE, bad), (bad, NONE), (NONE, bad)):
            assert _outer(left, right, 10, 10, 0, *A, C.FULL_OUTER, 16)[0] == code
            assert _cogroup(left, right, 10, 10, 0, *A, (16, 16, 16))[0] == code
    # an unknown mode; the coGroup mode is the operator's alone
    for mode in (-1, 4, 5):
        assert _outer(ONE, ONE, 10, 10, 0, *A, mode, 16)[0] == N.GW_E_INVALID
    # 65 windows per record; 64 are fine
    assert _outer(ONE, NONE, 65, 1, 0, *A, C.LEFT_OUTER, 128)[0] == N.GW_E_UNSUPPORTED
    assert _cogroup(ONE, NONE, 65, 1, 0, *A, (128, 128, 128))[0] == N.GW_E_UNSUPPORTED
    rc, n, _ = _outer(ONE, NONE, 64, 1, 0, *A, C.LEFT_OUTER, 128)
    assert (rc, n) == (N.GW_OK, 64)
    rc, n, _ = _cogroup(ONE, NONE, 64, 1, 0, *A, (128, 128, 128))
    assert rc == N.GW_OK and n == (64, 64, 0)
    for size, slide, offset in ((0, 1, 0), (10, 0, 0), (10, 5, 5), (10, 5, -5)):
        assert _outer(ONE, ONE, size, slide, offset, *A, C.FULL_OUTER, 16)[0] == N.GW_E_INVALID
        assert _cogroup(ONE, ONE, size, slide, offset, *A, (16, 16, 16))[0] == N.GW_E_INVALID
    with pytest.raises(N.GpuWinError):
        W.window_cogroup_host(*ONE, *ONE, W.EventTimeSessionWindows.with_gap(5))
    with pytest.raises(ValueError):
        W.window_join_outer_host(*ONE, *ONE, W.TumblingEventTimeWindows.of(10), "cogroup")
    # an interval that fires nothing
    rc, n, out = _cogroup(ONE, ONE, 10, 10, 0, 20, 20, (4, 4, 4))
    assert rc == N.GW_OK and n == (0, 0, 0) and out[3][0] == 0 and out[4][0] == 0


def test_names_are_exported_and_the_abi_stands():
    names = ["gw_window_join_outer_device", "gw_window_join_outer_host", "gw_window_cogroup_device",
             "gw_window_cogroup_host", "gw_join_set_mode", "gw_join_drain_outer", "gw_join_rows_device_outer",
             "gw_join_cogroup_pending", "gw_join_cogroup_drain", "gw_join_cogroup_rows_device"]
    for name in names:
        assert name in N.EXPORTS
        assert getattr(N.lib(), name) is not None
    assert N.lib().gw_abi_version() == 3
    assert ctypes.sizeof(N.GwJoinConfig) == 56 and ctypes.sizeof(N.GwJoinStats) == 64
    assert (N.JOIN_MODE_INNER, N.JOIN_MODE_LEFT_OUTER, N.JOIN_MODE_RIGHT_OUTER, N.JOIN_MODE_FULL_OUTER,
            N.JOIN_MODE_COGROUP) == (0, 1, 2, 3, 4)


def test_co_group_api_rejects_session_and_count_windows():
    env = W.StreamExecutionEnvironment.get_execution_environment()
    a = env.from_elements([W.StreamRecord((1, 2), 3)])
    b = W.StreamExecutionEnvironment.get_execution_environment().from_elements([W.StreamRecord((1, 5), 4)])
    j = a.co_group(b).where(lambda v: v[0]).equal_to(lambda v: v[0])
    assert isinstance(j, W.CoGroupedStreams)
    for bad in (W.EventTimeSessionWindows.with_gap(5), W.CountWindows.of(3)):
        with pytest.raises(N.GpuWinError) as e:
            j.window(bad)
        assert e.value.code == N.GW_E_UNSUPPORTED
    with pytest.raises(ValueError):
        W.OuterJoin("inner", lambda l, r: (l, r))
