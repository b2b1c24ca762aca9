"""gw_window_join_host: the window-join contract (include/gpuwin.h) as plain host code through
the C ABI, against tests/join_reference.py exactly, in order and values.  Runs without a GPU."""
import ctypes
import zlib

import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import windowing as W
from tests import join_reference as R

GEOMETRIES = {"tumbling": (10, 10, 0), "sliding": (10, 5, 0), "sliding_3_1": (10, 3, 1)}
INTERVALS = {"all": (R.I64_MIN, R.I64_MAX), "partial": (-3, 27)}
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0xffffffff


def assigner(size, slide, offset):
    return W.TumblingEventTimeWindows.of(size, offset) if size == slide else W.SlidingEventTimeWindows.of(size, slide, offset)


def _call(left, right, size, slide, offset, w0, w1, cap):
    """(rc, n_out, the five output columns of max(cap, 1) + 8 sentinel-filled rows)."""
    out = [np.full(max(cap, 1) + 8, SENTINEL, np.int64) for _ in range(5)]
    n_out = ctypes.c_int64(-7)
    P = lambda a: ctypes.c_void_p(a.ctypes.data) if len(a) else None
    rc = N.lib().gw_window_join_host(len(left[0]), *[P(c) for c in left], len(right[0]), *[P(c) for c in right],
                                     size, slide, offset, w0, w1, *[o.ctypes.data for o in out], cap,
                                     ctypes.byref(n_out))
    return rc, n_out.value, out


@pytest.mark.parametrize("interval", list(INTERVALS))
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("num_keys", [1, 7, 500])
@pytest.mark.parametrize("n_r", [0, 1, 64, 1000])
@pytest.mark.parametrize("n_l", [0, 1, 64, 1000])
def test_host_matches_reference(n_l, n_r, num_keys, geometry, interval):
    size, slide, offset = GEOMETRIES[geometry]
    w0, w1 = INTERVALS[interval]
    left, right = R.make_records(_seed(n_l, n_r, num_keys, geometry), n_l, n_r, num_keys)
    want = R.reference(left, right, size, slide, offset, w0, w1)
    got = W.window_join_host(*left, *right, assigner(size, slide, offset), w0, w1)
    R.check(got, want)
    if n_l >= 64 and n_r >= 64 and num_keys <= 7:
        assert len(want[0]) > 0


def test_output_full_reports_the_count_and_writes_nothing():
    left, right = R.make_records(5, 64, 64, 7)
    want = R.reference(left, right, 10, 5, 0)
    need = len(want[0])
    assert need > 10
    for cap in (0, 1, need - 1):
        rc, n, out = _call(left, right, 10, 5, 0, R.I64_MIN, R.I64_MAX, cap)
        assert (rc, n) == (N.GW_E_OUTPUT_FULL, need)
        assert all((o == SENTINEL).all() for o in out)
    rc, n, out = _call(left, right, 10, 5, 0, R.I64_MIN, R.I64_MAX, need)
    assert (rc, n) == (N.GW_OK, need)
    R.check([o[:need] for o in out], want)
    assert all((o[need:] == SENTINEL).all() for o in out)


def test_errors():
    one = (np.array([1], np.int64), np.array([5], np.int64), np.array([9], np.int64))
    no_ts = (one[0], np.array([R.I64_MIN], np.int64), one[2])
    far = (one[0], np.array([R.I64_MAX - 2], np.int64), one[2])
    for bad, code in ((no_ts, N.GW_E_NO_TIMESTAMP), (far, N.GW_E_RANGE)):
        for left, right in ((bad, one), (one, bad)):
            assert _call(left, right, 10, 10, 0, R.I64_MIN, R.I64_MAX, 16)[0] == code
    assert b"timestamp" in N.lib().gw_last_error(None) or b"int64" in N.lib().gw_last_error(None)
    # 65 windows per record; 64 are fine
    assert _call(one, one, 65, 1, 0, R.I64_MIN, R.I64_MAX, 128)[0] == N.GW_E_UNSUPPORTED
    rc, n, _ = _call(one, one, 64, 1, 0, R.I64_MIN, R.I64_MAX, 128)
    assert (rc, n) == (N.GW_OK, 64)
    for size, slide, offset in ((0, 1, 0), (10, 0, 0), (10, 5, 5), (10, 5, -5)):
        assert _call(one, one, size, slide, offset, R.I64_MIN, R.I64_MAX, 16)[0] == N.GW_E_INVALID
    with pytest.raises(N.GpuWinError):
        W.window_join_host(*one, *one, W.EventTimeSessionWindows.with_gap(5))


def test_empty_sides():
    one = (np.array([1], np.int64), np.array([5], np.int64), np.array([9], np.int64))
    none = tuple(np.empty(0, np.int64) for _ in range(3))
    for left, right in ((none, one), (one, none), (none, none)):
        rc, n, _ = _call(left, right, 10, 10, 0, R.I64_MIN, R.I64_MAX, 4)
        assert (rc, n) == (N.GW_OK, 0)


def test_names_are_exported():
    names = ["gw_window_join_device", "gw_window_join_host", "gw_join_create", "gw_join_destroy", "gw_join_last_error",
             "gw_join_ingest", "gw_join_ingest_device", "gw_join_advance_watermark", "gw_join_end_input",
             "gw_join_pending", "gw_join_drain", "gw_join_rows_device", "gw_join_clear_rows", "gw_join_late_dropped",
             "gw_join_get_stats", "gw_join_stream"]
    for name in names:
        assert name in N.EXPORTS
        assert getattr(N.lib(), name) is not None
    assert N.lib().gw_abi_version() == 3
    assert ctypes.sizeof(N.GwJoinConfig) == 56 and ctypes.sizeof(N.GwJoinStats) == 64


def test_join_api_rejects_session_and_count_windows():
    env = W.StreamExecutionEnvironment.get_execution_environment()
    a = env.from_elements([W.StreamRecord((1, 2), 3)])
    b = W.StreamExecutionEnvironment.get_execution_environment().from_elements([W.StreamRecord((1, 5), 4)])
    j = a.join(b).where(lambda v: v[0]).equal_to(lambda v: v[0])
    for bad in (W.EventTimeSessionWindows.with_gap(5), W.CountWindows.of(3)):
        with pytest.raises(N.GpuWinError) as e:
            j.window(bad)
        assert e.value.code == N.GW_E_UNSUPPORTED
