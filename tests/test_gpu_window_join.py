"""Event-time window join on the device (gw_join.hip; gw_window_join_device, gw_join_*): the
stateless call and the operator against tests/join_reference.py, exactly, in order and values.

Shapes hit the wave (64), the scan tile (1024 records) and several expand tiles (1024 output
slots); one key makes one group span many expand tiles, as many keys as records leaves most
groups one-sided.  Every case that is not named empty must have pairs by the reference alone.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from flink_amd import _native as N
from flink_amd import windowing as W
from tests import join_reference as R
from tests.gpu_helpers import random_stream

pytestmark = pytest.mark.gpu

GEOMETRIES = {"tumbling": (10, 10, 0), "sliding": (10, 5, 0), "sliding_3_1": (10, 3, 1)}
INTERVALS = {"all": (R.I64_MIN, R.I64_MAX), "partial": (-3, 27)}
SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 64


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0xffffffff


def assigner(size, slide, offset):
    return W.TumblingEventTimeWindows.of(size, offset) if size == slide else W.SlidingEventTimeWindows.of(size, slide, offset)


def _dev(cols):
    # (one element when empty: an empty tensor has no pointer; the length travels separately)
    return [torch.from_numpy(np.resize(np.ascontiguousarray(c), max(len(c), 1))).cuda() for c in cols]


# a thinned product: every n on each side, the largest with itself, and per (shape, keys) two of the
# six (geometry, interval) combinations in rotation, so that every one meets every key distribution
_NS = [0, 1, 63, 64, 65, 1025, 20_011]
SHAPES = sorted({(n, _NS[(3 * i + 1) % 7]) for i, n in enumerate(_NS)} | {(n, n) for n in _NS} |
                {(20_011, 1025), (65, 20_011)})
KEYS = ["one", "seven", "many"]
_COMBOS = [(g, iv) for g in GEOMETRIES for iv in INTERVALS]
CASES = []
for _i, (_nl, _nr) in enumerate(SHAPES):
    for _j, _k in enumerate(KEYS):
        for _t in range(2):
            CASES.append((_nl, _nr, _k) + _COMBOS[(2 * (_i + _j) + 3 * _t) % 6])
CASES = sorted(set(CASES))

_ref = {}


def _inputs(n_l, n_r, keys, geometry, interval):
    """Seeded inputs and their reference, made once; the seed is the first whose reference has
    pairs (unless a side is empty)."""
    case = (n_l, n_r, keys, geometry, interval)
    if case in _ref:
        return _ref[case]
    size, slide, offset = GEOMETRIES[geometry]
    w0, w1 = INTERVALS[interval]
    if keys == "one":      # one key, every record in [0, 10): one group per window, many expand tiles
        n_l, n_r = min(n_l, 300), min(n_r, 257)
        kw = dict(num_keys=1, ts_lo=0, ts_span=10)
    elif keys == "seven":  # groups of a few hundred records at most
        kw = dict(num_keys=7, ts_span=max(100, max(n_l, n_r) // 20))
    else:
        kw = dict(num_keys=max(n_l + n_r, 1))
    for t in range(2000):
        left, right = R.make_records(_seed(case, t), n_l, n_r, **kw)
        want = R.reference(left, right, size, slide, offset, w0, w1)
        if len(want[0]) > 0 or n_l == 0 or n_r == 0:
            break
    _ref[case] = (left, right, want)
    return _ref[case]


@pytest.mark.parametrize("n_l,n_r,keys,geometry,interval", CASES)
def test_device_matches_reference(n_l, n_r, keys, geometry, interval):
    left, right, want = _inputs(n_l, n_r, keys, geometry, interval)
    if n_l > 0 and n_r > 0:
        assert len(want[0]) >= 1          # not vacuous
        assert len(want[0]) <= 2_200_000
    else:
        assert len(want[0]) == 0
    w0, w1 = INTERVALS[interval]
    n_dl, n_dr = len(left[0]), len(right[0])
    dl, dr = _dev(left), _dev(right)
    got = W.window_join_device(*[t[:n_dl] for t in dl], *[t[:n_dr] for t in dr], assigner(*GEOMETRIES[geometry]), w0, w1)
    R.check([g.cpu().numpy() for g in got], want)


def test_case_list_covers_the_contract():
    assert {c[0] for c in CASES} == set(_NS) and {c[1] for c in CASES} == set(_NS)
    assert {(c[2], c[3], c[4]) for c in CASES} == {(k, g, i) for k in KEYS for g in GEOMETRIES for i in INTERVALS}
    assert (20_011, 20_011) in {c[:2] for c in CASES}


def _call(left, right, size, slide, offset, w0, w1, cap, shift=(0, 0, 0, 0, 0)):
    """gw_window_join_device into sentinel-filled columns of cap + GUARD rows, column c starting
    shift[c] words into its tensor.  (rc, n_out, the columns from their start, as numpy)."""
    dl, dr = _dev(left), _dev(right)
    out = [torch.full((cap + GUARD + 2,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(5)]
    n_out = ctypes.c_int64(-7)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    rc = N.lib().gw_window_join_device(len(left[0]), *[P(t) for t in dl], len(right[0]), *[P(t) for t in dr], size, slide,
                                       offset, w0, w1, *[ctypes.c_void_p(o.data_ptr() + 8 * s) for o, s in zip(out, shift)],
                                       cap, ctypes.byref(n_out), None)
    return rc, n_out.value, [o.cpu().numpy()[s:] for o, s in zip(out, shift)]


def _skew(singles):
    """One group of 4096 x 64 on key 2500 among `singles` groups of 1 x 1 (keys 0 .., the hot key's
    own single pair left out), one tumbling window, arrival shuffled."""
    rng = np.random.default_rng(singles)
    others = np.array([k for k in range(singles + 1) if k != 2500], np.int64)
    sides = []
    for hot in (4096, 64):
        key = np.concatenate([np.full(hot, 2500, np.int64), others])
        key = key[rng.permutation(len(key))]
        ts = rng.integers(0, 10, len(key)).astype(np.int64)
        pay = rng.integers(R.I64_MIN, R.I64_MAX, len(key), dtype=np.int64, endpoint=True)
        sides.append((key, ts, pay))
    return sides


@pytest.mark.parametrize("singles", [5000, 4999])
@pytest.mark.parametrize("shift", [(0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (0, 1, 0, 1, 0)], ids=["aligned", "odd", "mixed"])
def test_skew_one_large_group_among_singles(singles, shift):
    """The expand tiles' boundaries fall inside the large group and between the small ones; an odd
    total leaves the two-pairs-per-lane store a tail, columns 8 bytes off a 16-byte boundary give
    it a head, and columns of different alignment take the 8-byte stores."""
    left, right = _skew(singles)
    want = R.reference(left, right, 10, 10, 0)
    need = 4096 * 64 + singles
    assert len(want[0]) == need
    rc, n, out = _call(left, right, 10, 10, 0, R.I64_MIN, R.I64_MAX, need, shift)
    assert (rc, n) == (N.GW_OK, need)
    R.check([o[:need] for o in out], want)
    assert all((o[need:] == SENTINEL).all() for o in out)


def test_cap_exact_and_one_short():
    left, right, want = _inputs(1025, 1025, "seven", "sliding", "all")
    need = len(want[0])
    assert need > 2048
    rc, n, out = _call(left, right, 10, 5, 0, R.I64_MIN, R.I64_MAX, need)
    assert (rc, n) == (N.GW_OK, need)
    R.check([o[:need] for o in out], want)
    assert all((o[need:] == SENTINEL).all() for o in out)
    for cap in (need - 1, 0):
        rc, n, out = _call(left, right, 10, 5, 0, R.I64_MIN, R.I64_MAX, cap)
        assert (rc, n) == (N.GW_E_OUTPUT_FULL, need)
        assert all((o == SENTINEL).all() for o in out)


def test_device_errors():
    one = (np.array([1], np.int64), np.array([5], np.int64), np.array([9], np.int64))
    many = R.make_records(3, 3000, 3000, 7)[0]
    for bad_ts, code in ((R.I64_MIN, N.GW_E_NO_TIMESTAMP), (R.I64_MAX - 2, N.GW_E_RANGE)):
        bad = (many[0], many[1].copy(), many[2])
        bad[1][2900] = bad_ts
        assert _call(bad, one, 10, 10, 0, R.I64_MIN, R.I64_MAX, 64)[0] == code
        assert _call(one, bad, 10, 10, 0, R.I64_MIN, R.I64_MAX, 64)[0] == code
    assert _call(one, one, 65, 1, 0, R.I64_MIN, R.I64_MAX, 128)[0] == N.GW_E_UNSUPPORTED
    rc, n, out = _call(one, one, 64, 1, 0, R.I64_MIN, R.I64_MAX, 128)
    assert (rc, n) == (N.GW_OK, 64) and out[1][:64].tolist() == list(range(-58, 6))
    assert _call(one, one, 10, 5, 5, R.I64_MIN, R.I64_MAX, 16)[0] == N.GW_E_INVALID


# ---- the operator ------------------------------------------------------------------------------
def _streams(seed, geometry):
    """Two seeded streams with bounded disorder beyond the watermark lag (some records late), cut
    into 6 and 7 batches; the two-input operator's watermark is the minimum of its inputs'."""
    size = GEOMETRIES[geometry][0]
    sides = []
    for sd, nb in ((0, 6), (1, 7)):
        keys, ts, _, batches = random_stream(seed * 2 + sd, 420, 5, nb, ts_step=1, disorder=6 * size, wm_lag=size // 2)
        pay = np.arange(len(keys), dtype=np.int64) * 2 + sd + 1000 * (seed + 1)
        sides.append((keys, ts, pay, batches))
    return sides


@pytest.mark.parametrize("device_ingest", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("seed", [1, 2])
def test_operator_matches_reference(seed, geometry, device_ingest):
    size, slide, offset = GEOMETRIES[geometry]
    sides = _streams(seed, geometry)
    ref = R.ReferenceJoinOperator(size, slide, offset)
    want = []
    side_stream = torch.cuda.Stream() if device_ingest else None
    with W.GpuWindowJoinOperator(assigner(size, slide, offset), capacity_hint=16, max_batch=16) as op:
        wm_in = [R.I64_MIN, R.I64_MIN]
        fires = 0
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
            fires += wm > ref.wm
            out = ref.advance_watermark(wm)
            want.append(out)
            assert op.advance_watermark(wm) == len(out[0])
            assert op.advance_watermark(wm) == 0       # does not advance: ignored
            assert op.num_late_records_dropped() == ref.late_dropped
            st = op.stats()
            # the records left are exactly those with an unfired window
            assert (st["live_left"], st["live_right"]) == (ref.live_records(0), ref.live_records(1))
        out = ref.end_input()
        want.append(out)
        assert op.end_input() == len(out[0])
        st = op.stats()
        assert (st["live_left"], st["live_right"]) == (0, 0)
        assert st["pairs_fired"] == ref.pairs_fired == op.pending() and ref.pairs_fired > 100
        assert ref.late_dropped > 0
        # each side's first batch (70 left and 60 right records, none late) goes 16 at a time into
        # a log of 16 rows, which doubles three times for the 70 and twice for the 60
        assert st["log_growths"] >= 5 and st["log_capacity_left"] >= 128 and st["log_capacity_right"] >= 64
        assert st["fires"] == fires + 1 and st["last_fire_tuples"] >= 0
        # pairs of every fire accumulated; drained 37 at a time (GW_E_OUTPUT_FULL until the last)
        got = op.drain(cap=37)
        R.check(got, [np.concatenate([w[c] for w in want]) for c in range(5)])
        assert op.pending() == 0
    if side_stream is not None:
        side_stream.synchronize()


def test_empty_device_batch_on_a_side_stream_between_two_batches():
    """process_batch_device with no records on a producer stream that is not the operator's: the
    operator launches nothing, and the batches before and after it join as if it had not come."""
    size, slide, offset = GEOMETRIES["sliding"]
    sides = _streams(3, "sliding")
    ref = R.ReferenceJoinOperator(size, slide, offset)
    side_stream = torch.cuda.Stream()
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    want = []
    with W.GpuWindowJoinOperator(assigner(size, slide, offset), capacity_hint=16, max_batch=16) as op:
        assert side_stream.cuda_stream != op.stream
        for b in range(2):
            for sd, (keys, ts, pay, batches) in enumerate(sides):
                lo, hi, _ = batches[b]
                cols = (keys[lo:hi], ts[lo:hi], pay[lo:hi])
                ref.ingest(sd, *cols)
                with torch.cuda.stream(side_stream):
                    d = [torch.from_numpy(np.ascontiguousarray(c)).cuda(non_blocking=False) for c in cols]
                    op.process_batch_device(sd, *d)
                    del d
                    op.process_batch_device(sd, empty, empty, empty)  # between this batch and the next
            wm = min(sides[0][3][b][2], sides[1][3][b][2])
            out = ref.advance_watermark(wm)
            want.append(out)
            assert op.advance_watermark(wm) == len(out[0])
        want.append(ref.end_input())
        assert op.end_input() == len(want[-1][0])
        st = op.stats()
        assert (st["live_left"], st["live_right"]) == (0, 0)
        assert op.pending() == ref.pairs_fired and ref.pairs_fired > 20
        R.check(op.drain(), [np.concatenate([w[c] for w in want]) for c in range(5)])
    side_stream.synchronize()


def test_operator_errors():
    with pytest.raises(N.GpuWinError) as e:
        W.GpuWindowJoinOperator(W.EventTimeSessionWindows.with_gap(5))
    assert e.value.code == N.GW_E_UNSUPPORTED
    with pytest.raises(N.GpuWinError) as e:
        W.GpuWindowJoinOperator(W.SlidingEventTimeWindows.of(65, 1)).open()
    assert e.value.code == N.GW_E_UNSUPPORTED
    one = np.array([1], np.int64)
    with W.GpuWindowJoinOperator(W.TumblingEventTimeWindows.of(10)) as op:
        op.process_batch(0, one, one, one)
        with pytest.raises(N.GpuWinError) as e:
            op.process_batch(1, one, np.array([R.I64_MIN], np.int64), one)
        assert e.value.code == N.GW_E_NO_TIMESTAMP
        with pytest.raises(N.GpuWinError) as e:
            op.advance_watermark(100)
        assert e.value.code == N.GW_E_STATE


# ---- composition: pairs -> network-buffer bytes ------------------------------------------------
def test_pairs_encode_as_tuple3_rows():
    """rows_device() columns into gw_encode_rows_device as Tuple3<Long, Long, Long>(key, left
    payload, right payload), decoded again with gw_decode_serialized: the pairs come back, each
    stamped end - 1."""
    left, right = R.make_records(11, 500, 400, 7)
    want = R.reference(left, right, 10, 5, 0)
    n = len(want[0])
    assert n > 1000
    with W.GpuWindowJoinOperator(W.SlidingEventTimeWindows.of(10, 5)) as op:
        op.process_batch(0, *left)
        op.process_batch(1, *right)
        assert op.end_input() == n
        ptrs, got_n = op.rows_device()
        assert got_n == n
        lay = N.row_layout("JJJ", (N.GW_ROW_KEY, N.GW_ROW_RESULT, N.GW_ROW_PAYLOAD))
        row = N.lib().gw_row_encoded_bytes(ctypes.byref(lay))
        assert row == 4 + 1 + 8 + 24
        buf = torch.full((n * row + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        off, nb = np.zeros(1, np.int64), np.zeros(1, np.int64)
        V = ctypes.c_void_p
        rc = N.lib().gw_encode_rows_device(n, V(ptrs[0]), V(ptrs[1]), V(ptrs[2]), V(ptrs[3]), V(ptrs[4]), ctypes.byref(lay),
                                           0, 1, 128, N.NO_WATERMARK, V(buf.data_ptr()), buf.numel(), off.ctypes.data,
                                           nb.ctypes.data, V(op.stream))
        assert rc == N.GW_OK and nb[0] == n * row
        op.clear_rows()
        assert op.pending() == 0
    fields = []
    for value_field in (1, 2):
        k, t, v = (torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(3))
        wp, wv = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(2))
        res = N.GwDecodeResult()
        rl = N.record_layout("JJJ", 0, value_field)
        P = lambda x: ctypes.c_void_p(x.data_ptr())
        rc = N.lib().gw_decode_serialized(P(buf), int(nb[0]), ctypes.byref(rl), P(k), P(t), P(v), n + 1, P(wp), P(wv), 4,
                                          ctypes.byref(res), None)
        assert rc == N.GW_OK and res.records == n and res.consumed == nb[0]
        fields.append((k[:n].cpu().numpy(), t[:n].cpu().numpy(), v[:n].cpu().numpy()))
    assert np.array_equal(fields[0][0], want[0]) and np.array_equal(fields[0][1], want[2] - 1)
    assert np.array_equal(fields[0][2], want[3]) and np.array_equal(fields[1][2], want[4])


# ---- the API mirror ----------------------------------------------------------------------------
def test_join_api_mirror():
    """persons join auctions on person.id = auction.seller, tumbling 10 (Nexmark Q8's shape)."""
    SR = W.StreamRecord
    persons = [SR(("p", 1, "ann"), 1), SR(("p", 2, "bob"), 3), SR(("p", 3, "cy"), 12), SR(("p", 1, "ann2"), 14),
               SR(("p", 9, "zed"), 15), W.Watermark(9)]
    auctions = [SR(("a", 100, 2), 2), SR(("a", 101, 1), 5), SR(("a", 102, 1), 9), SR(("a", 103, 3), 8),
                SR(("a", 104, 1), 11), SR(("a", 105, 3), 19), SR(("a", 106, 7), 13)]
    env_p = W.StreamExecutionEnvironment.get_execution_environment()
    env_a = W.StreamExecutionEnvironment.get_execution_environment()
    out = (env_p.from_elements(persons).join(env_a.from_elements(auctions))
           .where(lambda p: p[1]).equal_to(lambda a: a[2])
           .window(W.TumblingEventTimeWindows.of(10))
           .apply(lambda p, a: (p[2], a[1]))
           .execute_and_collect())
    assert [(r.value, r.timestamp) for r in out] == [
        (("ann", 101), 9), (("ann", 102), 9), (("bob", 100), 9),
        (("ann2", 104), 19), (("cy", 105), 19)]
    with pytest.raises(N.GpuWinError):
        env_p.from_elements(persons).join(env_a.from_elements(auctions)).where(lambda p: p[1]) \
            .equal_to(lambda a: a[2]).window(W.CountWindows.of(3))
