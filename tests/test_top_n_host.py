"""gw_top_n_host: the per-window top-N contract (include/gpuwin.h) as pure host code -- the
non-keyed stage behind the keyed window aggregate in Nexmark Q5 / Q7, and how a job at
parallelism > 1 combines its subtasks' lists.  Against the numpy reference of
tests/topn_reference.py, exactly.  Runs without a GPU.
"""
import ctypes
import zlib

import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import windowing as W
from tests import topn_reference as R


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0xffffffff


@pytest.mark.parametrize("smallest", [False, True], ids=["largest", "smallest"])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("windows", [1, 3, 17, 300])
@pytest.mark.parametrize("top", [1, 5, 64])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 5000])
def test_host_matches_reference(n, top, windows, kind, smallest):
    key, start, end, res = R.make_rows(_seed(n, top, windows, kind), n, windows, kind)
    f64 = kind == "f64"
    col = res.view(np.float64) if f64 else res
    got = W.top_n_host(key, start, end, col, top, smallest=smallest)
    want = R.reference(key, start, end, res, top, smallest=smallest, f64=f64)
    R.check(got, want, f64)
    assert got[3].dtype == (np.float64 if f64 else np.int64)


def test_order_key_reference_is_double_compare():
    """The reference's own order key, on the values the contract names."""
    v = np.array([-np.inf, -1.5, -0.0, 0.0, 1.5, np.inf], np.float64).view(np.int64)
    k = R.f64_order_key(np.concatenate([v, [R.NAN_A, R.NAN_B]]))
    assert (np.diff(k[:7]) > 0).all() and k[6] == k[7]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("smallest", [False, True], ids=["largest", "smallest"])
def test_merge_of_partial_lists_is_global(kind, smallest):
    """Rows split into 4 parts by key (as key groups split them over subtasks): the top-N of
    the concatenated per-part top-Ns is the top-N of all rows."""
    key, start, end, res = R.make_rows(_seed("merge", kind), 5000, 17, kind)
    f64 = kind == "f64"
    col = res.view(np.float64) if f64 else res
    parts = []
    for p in range(4):
        m = (key % 4) == p
        parts.append(W.top_n_host(key[m], start[m], end[m], col[m], 5, smallest=smallest))
    cat = [np.concatenate([p[c] for p in parts]) for c in range(4)]
    got = W.top_n_host(*cat, 5, smallest=smallest)
    want = R.reference(key, start, end, res, 5, smallest=smallest, f64=f64)
    for c in range(3):
        assert np.array_equal(got[c], want[c])
    R.check((got[0], got[1], got[2], got[3], want[4]), want, f64)  # win_rows counts list rows here


def _call(key, start, end, res, top, cap, mode=0):
    out = [np.zeros(max(cap, 1), np.int64) for _ in range(5)]
    n_out = ctypes.c_int64(-7)
    rc = N.lib().gw_top_n_host(len(key), *[x.ctypes.data for x in (key, start, end, res)], top, mode,
                               *[o.ctypes.data for o in out], cap, ctypes.byref(n_out))
    return rc, n_out.value


@pytest.mark.parametrize("top", [0, 65, -1])
def test_top_out_of_range_is_invalid(top):
    a = np.arange(4, dtype=np.int64)
    assert _call(a, a * 0, a * 0 + 10, a, top, 64)[0] == N.GW_E_INVALID


def test_two_starts_under_one_end_is_invalid():
    key = np.arange(6, dtype=np.int64)
    end = np.array([10, 20, 10, 20, 10, 20], np.int64)
    start = np.array([0, 10, 0, 10, 1, 10], np.int64)
    assert _call(key, start, end, key, 2, 64)[0] == N.GW_E_INVALID
    start[4] = 0
    assert _call(key, start, end, key, 2, 64) == (N.GW_OK, 4)


def test_too_many_windows_is_unsupported():
    end = np.arange(1025, dtype=np.int64)
    z = np.zeros(1025, np.int64)
    assert _call(z, end - 1, end, z, 1, 2048)[0] == N.GW_E_UNSUPPORTED
    assert _call(z[:1024], end[:1024] - 1, end[:1024], z[:1024], 1, 2048) == (N.GW_OK, 1024)


def test_small_output_reports_needed_size():
    key, start, end, res = R.make_rows(3, 500, 3, "ties")
    need = len(R.reference(key, start, end, res, 5)[0])
    assert need == 15
    assert _call(key, start, end, res, 5, need - 1) == (N.GW_E_OUTPUT_FULL, need)
    assert _call(key, start, end, res, 5, need) == (N.GW_OK, need)


def test_empty_input():
    z = np.zeros(0, np.int64)
    assert _call(z, z, z, z, 3, 0) == (N.GW_OK, 0)


def test_names_are_exported():
    for name in ("gw_top_n_device", "gw_top_n_rows", "gw_top_n_host"):
        assert name in N.EXPORTS
        assert getattr(N.lib(), name) is not None
    assert N.lib().gw_abi_version() == 3
