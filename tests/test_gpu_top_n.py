"""Per-window top-N over fired rows on the device (gw_topn.hip; gw_top_n_device, gw_top_n_rows):
the non-keyed stage behind the keyed window aggregate in Nexmark Q5 ("hot items") and Q7.

Against the numpy reference of tests/topn_reference.py, exactly (NaN bits as "both NaN"); end
to end against the reference applied to the oracle's rows of every watermark.  Shapes hit the
wave (64), tile (1024 rows) and grid-stride edges of the kernels, 17 windows are one more than
one selection pass ranks, 300 need several passes.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from flink_amd import _native as N
from flink_amd import windowing as W
from tests import topn_reference as R
from tests.gpu_helpers import compare, gpu_operator, random_stream, run_oracle

pytestmark = pytest.mark.gpu


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0xffffffff


def _dev(*cols):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]


def _run_device(key, start, end, res, top, smallest, f64):
    out = W.top_n_device(*_dev(key, start, end, res), top, smallest=smallest, f64=f64)
    return [o.cpu().numpy() for o in out]


# a thinned product: every n, every top and every window count, each n with two (top, windows)
# pairs, the largest n with every window count
_NS = [1, 63, 64, 65, 4095, 4097, 200_003]
_TOPS = [1, 5, 64]
_WINS = [1, 3, 17, 300]
SHAPES = sorted({(n, _TOPS[i % 3], _WINS[i % 4]) for i, n in enumerate(_NS)} |
                {(n, _TOPS[(i + 1) % 3], _WINS[(i + 2) % 4]) for i, n in enumerate(_NS)} |
                {(200_003, _TOPS[i % 3], w) for i, w in enumerate(_WINS)})


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n,top,windows", SHAPES)
def test_device_matches_reference(n, top, windows, kind):
    key, start, end, res = R.make_rows(_seed(n, top, windows, kind), n, windows, kind)
    f64 = kind == "f64"
    for smallest in (False, True):
        got = _run_device(key, start, end, res, top, smallest, f64)
        R.check(got, R.reference(key, start, end, res, top, smallest=smallest, f64=f64), f64)


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_sorted_input_one_window(order):
    """Ascending results: every row beats the block's threshold, so every row goes through the
    candidate buffer and its merge -- where a lost or duplicated entry would show."""
    n = 100_000
    res = np.arange(n, dtype=np.int64) * 3 - 1000
    if order == "descending":
        res = res[::-1].copy()
    key = np.random.default_rng(11).permutation(n).astype(np.int64)
    start, end = np.full(n, 5, np.int64), np.full(n, 15, np.int64)
    got = _run_device(key, start, end, res, 64, False, False)
    R.check(got, R.reference(key, start, end, res, 64))


def test_window_smaller_than_top():
    key = np.array([7, 3, 9, 1, 4, 2], np.int64)
    end = np.array([20, 10, 20, 10, 20, 20], np.int64)
    start = end - 10
    res = np.array([5, 8, 5, -1, 6, 5], np.int64)
    k, s, e, r, w = _run_device(key, start, end, res, 5, False, False)
    assert k.tolist() == [3, 1, 4, 2, 7, 9]
    assert s.tolist() == [0, 0, 10, 10, 10, 10]
    assert e.tolist() == [10, 10, 20, 20, 20, 20]
    assert r.tolist() == [8, -1, 6, 5, 5, 5]
    assert w.tolist() == [2, 2, 4, 4, 4, 4]


def _call(key, start, end, res, top, cap, mode=0):
    cols = _dev(key, start, end, res)
    out = [torch.zeros(max(cap, 1), dtype=torch.int64, device="cuda") for _ in range(5)]
    n_out = ctypes.c_int64(-7)
    rc = N.lib().gw_top_n_device(len(key), *[c.data_ptr() for c in cols], top, mode, *[o.data_ptr() for o in out],
                                 cap, ctypes.byref(n_out), None)
    return rc, n_out.value


def test_device_errors():
    a = np.arange(4, dtype=np.int64)
    for top in (0, 65):
        assert _call(a, a * 0, a * 0 + 10, a, top, 64)[0] == N.GW_E_INVALID
    key = np.arange(6, dtype=np.int64)
    end = np.array([10, 20, 10, 20, 10, 20], np.int64)
    start = np.array([0, 10, 0, 10, 1, 10], np.int64)
    assert _call(key, start, end, key, 2, 64)[0] == N.GW_E_INVALID
    start[4] = 0
    assert _call(key, start, end, key, 2, 64) == (N.GW_OK, 4)
    # the disagreeing start far from the window's other rows (another block finds it)
    n = 50_000
    big_end = np.where(np.arange(n) % 2 == 0, 10, 20).astype(np.int64)
    big_start = big_end - 10
    big_start[n - 3] += 1
    z = np.zeros(n, np.int64)
    assert _call(z, big_start, big_end, z, 2, 64)[0] == N.GW_E_INVALID
    ends = np.arange(1025, dtype=np.int64)
    z = np.zeros(1025, np.int64)
    assert _call(z, ends - 1, ends, z, 1, 2048)[0] == N.GW_E_UNSUPPORTED
    assert _call(z[:1024], ends[:1024] - 1, ends[:1024], z[:1024], 1, 2048) == (N.GW_OK, 1024)
    key, start, end, res = R.make_rows(3, 500, 3, "ties")
    assert _call(key, start, end, res, 5, 14) == (N.GW_E_OUTPUT_FULL, 15)
    assert _call(key, start, end, res, 5, 15) == (N.GW_OK, 15)
    e = np.zeros(0, np.int64)
    assert _call(e, e, e, e, 3, 0) == (N.GW_OK, 0)


# ---- through a handle, against the oracle ------------------------------------------------
def _skewed_stream(seed, agg, n=200_000, num_keys=3000, n_batches=20):
    keys, ts, vals, batches = random_stream(seed, n, num_keys, n_batches, ts_step=1, agg=agg)
    rng = np.random.default_rng(seed + 1)
    keys = np.floor(num_keys * rng.random(n) ** 3).astype(np.int64)  # a few hot keys
    if agg == "avg_f64":
        # multiples of 1/4 with small sums: every summation order gives the same double, so the
        # device's averages are the oracle's to the bit and the ranks compare exactly
        vals = (rng.integers(-4000, 4000, n) / 4.0).astype(np.float64)
    return keys, ts, vals, batches


_HANDLES = {
    "count": (dict(assigner="sliding", size=10_000, slide=2_000, agg="count"), 0),
    "sum": (dict(assigner="sliding", size=10_000, slide=2_000, agg="sum_i64"), 0),
    "sum-region": (dict(assigner="sliding", size=10_000, slide=2_000, agg="sum_i64"), N.FLAG_FORCE_REGION),
    "sum-direct": (dict(assigner="sliding", size=10_000, slide=2_000, agg="sum_i64"), N.FLAG_NO_REGION),
    "window-classes": (dict(assigner="sliding", size=70_000, slide=1_000, agg="sum_i64"), 0),  # n + m > 64
    "avg-f64": (dict(assigner="sliding", size=10_000, slide=2_000, agg="avg_f64"), 0),
}


@pytest.mark.parametrize("variant", list(_HANDLES))
def test_handle_top_n_matches_oracle(oracle_lib, variant):
    kw, flags = _HANDLES[variant]
    agg = kw["agg"]
    keys, ts, vals, batches = _skewed_stream(_seed(variant) & 0xffff, agg)
    ora, _ = run_oracle(oracle_lib, kw, keys, ts, vals, batches)
    f64 = agg in N.DOUBLE_RESULT
    op = gpu_operator(kw, capacity_hint=4096, flags=flags)
    drained, fired = [], 0
    try:
        for b, (lo, hi, wm) in enumerate(batches + [(0, 0, W.LONG_MAX)]):
            if hi > lo:
                op.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi])
            op.advance_watermark(wm)
            top = op.top_n_rows(3)
            k, s, e, r = op.drain()  # top_n_rows consumed nothing: the rows are all still there
            drained.append((k, s, e, r.view(np.int64)))
            ok, os_, oe, orr = ora[b]
            R.check(top, R.reference(ok, os_, oe, orr, 3, f64=f64), f64)
            assert top[3].dtype == (np.float64 if f64 else np.int64)
            fired += len(ok) > 0
            if b == 5:
                low = op.top_n_rows(2, smallest=True)
                op.clear_rows()  # nothing pending after the drain: still fine
                assert len(low[0]) == 0
    finally:
        op.close()
    assert fired >= 10
    assert compare(drained, ora, f64) == []


def test_handle_smallest_and_pending_rows_kept(oracle_lib):
    kw = dict(assigner="tumbling", size=5_000, agg="sum_i64")
    keys, ts, vals, batches = _skewed_stream(77, "sum_i64", n=40_000, num_keys=500, n_batches=4)
    ora, _ = run_oracle(oracle_lib, kw, keys, ts, vals, batches, final_wm=None)
    op = gpu_operator(kw, capacity_hint=1024)
    try:
        for lo, hi, wm in batches:  # rows of several watermarks stay pending
            op.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi])
            op.advance_watermark(wm)
        allrows = [np.concatenate([o[c] for o in ora]) for c in range(4)]
        R.check(op.top_n_rows(64, smallest=True), R.reference(*allrows, 64, smallest=True))
        assert op.pending_rows() == len(allrows[0])
    finally:
        op.close()


def test_session_handle_is_unsupported():
    op = gpu_operator(dict(assigner="session", gap=100, agg="sum_i64"))
    try:
        op.process_batch(np.array([1, 2], np.int64), np.array([10, 20], np.int64), np.array([5, 6], np.int64))
        op.advance_watermark(10_000)
        out = [np.zeros(16, np.int64) for _ in range(5)]
        n = ctypes.c_int64(0)
        rc = N.lib().gw_top_n_rows(op.handle, 3, 0, *[o.ctypes.data for o in out], 16, ctypes.byref(n))
        assert rc == N.GW_E_UNSUPPORTED
        assert len(op.drain()[0]) == 2
    finally:
        op.close()


def test_window_all_top_n():
    SR, WM = W.StreamRecord, W.Watermark
    elements = [
        SR((1, 1), 1), SR((2, 5), 2), SR((3, 5), 3), SR((1, 3), 4), WM(9),            # [0,10): 1:4 2:5 3:5
        SR((3, 7), 11), SR((1, 2), 12), SR((2, 2), 13), SR((1, 1), 15), WM(12),      # [10,20): 3:7 1:3 2:2
        SR((5, 9), 21),                                                              # [20,30): 5:9
        SR((4, -1), 31), SR((6, -1), 32), SR((2, -5), 33),                           # [30,40): 4:-1 6:-1 2:-5
    ]
    env = W.StreamExecutionEnvironment.get_execution_environment()
    out = env.from_elements(elements).key_by(lambda v: v[0]).window(W.TumblingEventTimeWindows.of(10)) \
        .sum(1).window_all_top_n(2).execute_and_collect()
    got = [(tuple(int(x) for x in r.value), r.timestamp) for r in out]
    assert got == [
        ((2, 0, 10, 5), 9), ((3, 0, 10, 5), 9),
        ((3, 10, 20, 7), 19), ((1, 10, 20, 3), 19),
        ((5, 20, 30, 9), 29),
        ((4, 30, 40, -1), 39), ((6, 30, 40, -1), 39),
    ]
    low = env.from_elements(elements).key_by(lambda v: v[0]).window(W.TumblingEventTimeWindows.of(10)) \
        .sum(1).window_all_top_n(1, smallest=True).execute_and_collect()
    assert [tuple(int(x) for x in r.value) for r in low] == [(1, 0, 10, 4), (2, 10, 20, 2), (5, 20, 30, 9),
                                                             (2, 30, 40, -5)]
