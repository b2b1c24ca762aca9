"""gw_interval_join_host (plain host code, no device) against tests/interval_join_reference.py,
exactly, in order and values; every error of the stateless contract; the new symbols."""
import ctypes
import zlib

import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import windowing as W
from tests import interval_join_reference as R

SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 16

BOUNDS = [(-1, 1), (0, 2), (-7, -2), (3, 9), (4, 4), (0, 0), (-30, 30)]
SHAPES = [(0, 0), (0, 5), (5, 0), (1, 1), (1, 300), (300, 1), (64, 65), (257, 300), (1500, 1200)]
KEYS = {"one": 1, "seven": 7, "many": 600}


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0xffffffff


@pytest.mark.parametrize("probe_side", [R.LEFT, R.RIGHT], ids=["left", "right"])
@pytest.mark.parametrize("keys", list(KEYS))
@pytest.mark.parametrize("n_p,n_b", SHAPES)
def test_host_matches_reference(n_p, n_b, keys, probe_side):
    total = 0
    for lower, upper in BOUNDS:
        probe = R.make_records(_seed(n_p, n_b, keys, lower, 0), n_p, KEYS[keys])
        build = R.make_records(_seed(n_p, n_b, keys, lower, 1), n_b, KEYS[keys])
        want = R.reference_call(probe_side, probe, build, lower, upper)
        got = W.interval_join_host(probe_side, *probe, *build, lower, upper)
        R.check(got, want)
        total += len(want[0])
    if n_p == 0 or n_b == 0:
        assert total == 0
    elif n_p * n_b >= 300 and (keys != "many" or n_p * n_b >= 10_000):
        assert total >= 1  # not vacuous


def _call(probe_side, probe, build, lower, upper, cap, null=()):
    """gw_interval_join_host into sentinel-filled columns of cap + GUARD rows: (rc, n_out, columns)."""
    cols = [np.ascontiguousarray(c, np.int64) for c in (*probe, *build)]
    out = [np.full(cap + GUARD, SENTINEL, np.int64) for _ in range(5)]
    n_out = ctypes.c_int64(-7)
    P = lambda i, a: None if i in null else ctypes.c_void_p(a.ctypes.data)
    rc = N.lib().gw_interval_join_host(probe_side, len(cols[0]), *[P(i, c) for i, c in enumerate(cols[:3])], len(cols[3]),
                                       *[P(3 + i, c) for i, c in enumerate(cols[3:])], lower, upper,
                                       *[P(6 + i, o) for i, o in enumerate(out)], cap, ctypes.byref(n_out))
    return rc, n_out.value, out


def test_output_full_writes_nothing_and_reports_the_need():
    probe, build = R.make_records(1, 200, 3), R.make_records(2, 300, 3)
    want = R.reference_call(R.LEFT, probe, build, -10, 10)
    need = len(want[0])
    assert need > 1000
    rc, n, out = _call(R.LEFT, probe, build, -10, 10, need)
    assert (rc, n) == (N.GW_OK, need)
    R.check([o[:need] for o in out], want)
    assert all((o[need:] == SENTINEL).all() for o in out)
    for cap in (need - 1, 0):
        rc, n, out = _call(R.LEFT, probe, build, -10, 10, cap)
        assert (rc, n) == (N.GW_E_OUTPUT_FULL, need)
        assert all((o == SENTINEL).all() for o in out)


def test_every_error():
    one = (np.array([1], np.int64), np.array([5], np.int64), np.array([9], np.int64))
    many = R.make_records(3, 500, 7)
    big = 1 << 62
    # bounds
    assert _call(R.LEFT, one, one, 2, 1, 4)[0] == N.GW_E_INVALID
    assert _call(R.LEFT, one, one, 0, big + 1, 4)[0] == N.GW_E_INVALID
    assert _call(R.LEFT, one, one, -big - 1, 0, 4)[0] == N.GW_E_INVALID
    assert _call(R.LEFT, one, one, -big, big, 4)[:2] == (N.GW_OK, 1)
    # arguments
    assert _call(2, one, one, 0, 0, 4)[0] == N.GW_E_INVALID
    assert _call(-1, one, one, 0, 0, 4)[0] == N.GW_E_INVALID
    assert _call(R.LEFT, one, one, 0, 0, -1)[0] == N.GW_E_INVALID
    assert N.lib().gw_interval_join_host(0, 0, None, None, None, 0, None, None, None, 0, 0, None, None, None, None, None, 0,
                                         None) == N.GW_E_INVALID
    for i in (0, 1, 2, 3, 4, 5, 6, 10):
        assert _call(R.LEFT, one, one, 0, 0, 4, null=(i,))[0] == N.GW_E_INVALID
    L = N.lib()
    n_out = ctypes.c_int64(-7)
    p = ctypes.c_void_p(one[0].ctypes.data)
    for n_p, n_b in ((-1, 1), (1, -1)):
        assert L.gw_interval_join_host(0, n_p, p, p, p, n_b, p, p, p, 0, 0, p, p, p, p, p, 1, ctypes.byref(n_out)) == N.GW_E_INVALID
    for n_p, n_b in ((1 << 30, 1), (1, 1 << 30)):  # refused before any column is read
        assert L.gw_interval_join_host(0, n_p, p, p, p, n_b, p, p, p, 0, 0, p, p, p, p, p, 1, ctypes.byref(n_out)) == N.GW_E_UNSUPPORTED
    # an empty side: no rows, whatever the other side holds
    assert _call(R.LEFT, (one[0][:0],) * 3, many, 0, 0, 4)[:2] == (N.GW_OK, 0)
    assert _call(R.RIGHT, many, (one[0][:0],) * 3, 0, 0, 4)[:2] == (N.GW_OK, 0)
    # Long.MIN_VALUE and the range check on either side, the former first
    for probe_side in (R.LEFT, R.RIGHT):
        for where in ("probe", "build"):
            side = probe_side if where == "probe" else 1 - probe_side
            over = R.I64_MAX - 9 if side == R.LEFT else R.I64_MIN + 9  # ts + 10 / ts - 10 leaves int64
            for bad, code in (([R.I64_MIN], N.GW_E_NO_TIMESTAMP), ([over], N.GW_E_RANGE), ([over, R.I64_MIN], N.GW_E_NO_TIMESTAMP)):
                cols = (many[0], many[1].copy(), many[2])
                cols[1][400:400 + len(bad)] = bad
                args = (cols, one) if where == "probe" else (one, cols)
                rc, n, out = _call(probe_side, *args, 0, 10, 64)
                assert (rc, n) == (code, 0)
                assert all((o == SENTINEL).all() for o in out)
            ok = (many[0], many[1].copy(), many[2])
            ok[1][400] = over + (-1 if side == R.LEFT else 1)  # just inside
            args = (ok, one) if where == "probe" else (one, ok)
            assert _call(probe_side, *args, 0, 10, 64)[0] == N.GW_OK
    msg = L.gw_last_error(None).decode()
    assert "interval join" in msg or "timestamp" in msg


def test_extreme_keys_and_timestamps():
    key = np.array([R.I64_MIN, R.I64_MAX, -1, 0, R.I64_MIN, R.I64_MAX], np.int64)
    ts = np.array([-5, R.I64_MAX - 3, -7, 0, -6, R.I64_MAX - 2], np.int64)
    pay = np.arange(6, dtype=np.int64)
    left, right = (key, ts, pay), (key[::-1].copy(), ts[::-1].copy(), pay[::-1].copy() + 100)
    for probe_side, probe, build in ((R.LEFT, left, right), (R.RIGHT, right, left)):
        want = R.reference_call(probe_side, probe, build, -2, 2)
        assert len(want[0]) >= 8
        R.check(W.interval_join_host(probe_side, *probe, *build, -2, 2), want)


def test_symbols_and_abi_version():
    L = N.lib()
    names = [n for n in N.EXPORTS if n.startswith(("gw_interval_join_", "gw_ijoin_"))]
    assert len(names) == 3 + 15
    assert all(hasattr(L, n) for n in names)
    assert L.gw_abi_version() == 3
    # gw_ijoin_config: 2 x int64, int32 (+ padding), 2 x int64; gw_ijoin_stats: 8 x int64
    assert ctypes.sizeof(N.GwIJoinConfig) == 40 and N.GwIJoinConfig.capacity_hint.offset == 24
    assert ctypes.sizeof(N.GwIJoinStats) == 64
