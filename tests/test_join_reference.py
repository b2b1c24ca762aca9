"""tests/join_reference.py against hand-written vectors of the window-join contract
(include/gpuwin.h), and against the existing CPU oracle: a window join is union -> keyBy ->
window, so per fired (key, window) the reference's L + R must be the oracle's `count` row over
the union of both sides under the same watermarks, and its late count the oracle's.  No GPU."""
import numpy as np
import pytest

from tests import join_reference as R
from tests.gpu_helpers import random_stream


def cols(*recs):
    """(key, ts, payload) triples -> three int64 columns."""
    a = np.array(recs, np.int64).reshape(-1, 3)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def rows(out):
    return list(zip(*[c.tolist() for c in out]))


def test_tumbling_cross_product_is_left_major():
    left = cols((7, 1, 100), (7, 5, 101))
    right = cols((7, 2, 200), (7, 3, 201), (7, 9, 202))
    assert rows(R.reference(left, right, 10, 10, 0)) == [
        (7, 0, 10, 100, 200), (7, 0, 10, 100, 201), (7, 0, 10, 100, 202),
        (7, 0, 10, 101, 200), (7, 0, 10, 101, 201), (7, 0, 10, 101, 202)]


def test_key_on_one_side_only_emits_nothing():
    left = cols((1, 1, 100), (2, 1, 101))
    right = cols((3, 2, 200))
    assert rows(R.reference(left, right, 10, 10, 0)) == []
    assert rows(R.reference(left, cols(), 10, 10, 0)) == []


def test_sliding_record_joins_in_both_its_windows():
    left, right = cols((4, 7, 1)), cols((4, 8, 2))
    assert rows(R.reference(left, right, 10, 5, 0)) == [(4, 0, 10, 1, 2), (4, 5, 15, 1, 2)]
    # only the window whose end - 1 lies in (w0, w1]
    assert rows(R.reference(left, right, 10, 5, 0, w0=9, w1=14)) == [(4, 5, 15, 1, 2)]
    assert rows(R.reference(left, right, 10, 5, 0, w0=R.I64_MIN, w1=9)) == [(4, 0, 10, 1, 2)]
    assert rows(R.reference(left, right, 10, 5, 0, w0=14, w1=R.I64_MAX)) == []


def test_slide_not_dividing_size_with_offset():
    # starts are 1 (mod 3): ts 7 -> 7, 4, 1, -2; ts 5 -> 4, 1, -2
    assert R.window_starts(7, 10, 3, 1) == (7, [7, 4, 1, -2])
    assert R.window_starts(5, 10, 3, 1) == (4, [4, 1, -2])
    out = rows(R.reference(cols((0, 7, 1)), cols((0, 5, 2)), 10, 3, 1))
    assert out == [(0, -2, 8, 1, 2), (0, 1, 11, 1, 2), (0, 4, 14, 1, 2)]


def test_negative_timestamps_and_keys():
    left = cols((3, -5, 10), (-5, -5, 11), (3, -11, 12))
    right = cols((-5, -1, 20), (3, -10, 21), (3, -20, 22))
    assert rows(R.reference(left, right, 10, 10, 0)) == [
        (3, -20, -10, 12, 22), (-5, -10, 0, 11, 20), (3, -10, 0, 10, 21)]


def test_errors():
    with pytest.raises(R.NoTimestamp):
        R.reference(cols((1, R.I64_MIN, 0)), cols((1, 0, 0)), 10, 10, 0)
    with pytest.raises(R.WindowRange):
        R.reference(cols((1, R.I64_MAX - 2, 0)), cols((1, 0, 0)), 10, 10, 0)
    with pytest.raises(R.Unsupported):
        R.reference(cols((1, 0, 0)), cols((1, 0, 0)), 65, 1, 0)
    R.reference(cols((1, 0, 0)), cols((1, 0, 0)), 64, 1, 0)


def test_late_record_is_dropped_and_counted():
    op = R.ReferenceJoinOperator(10, 10)
    op.ingest(0, *cols((1, 5, 100)))
    op.ingest(1, *cols((1, 6, 200)))
    assert rows(op.advance_watermark(9)) == [(1, 0, 10, 100, 200)]
    op.ingest(0, *cols((1, 7, 101), (1, 12, 102)))  # ts 7: its only window [0, 10) has passed
    assert op.late_dropped == 1
    op.ingest(1, *cols((1, 13, 201)))
    assert rows(op.advance_watermark(9)) == []       # does not advance
    assert rows(op.end_input()) == [(1, 10, 20, 102, 201)]
    assert op.late_dropped == 1 and op.pairs_fired == 2


def test_record_after_its_earlier_window_passed_joins_only_later():
    op = R.ReferenceJoinOperator(10, 5)
    op.ingest(1, *cols((2, 6, 200)))                 # windows [0, 10) and [5, 15)
    assert rows(op.advance_watermark(9)) == []       # [0, 10) fires with the right side only
    op.ingest(0, *cols((2, 7, 100)))                 # [0, 10) has passed, [5, 15) has not: not late
    assert op.late_dropped == 0
    assert rows(op.advance_watermark(14)) == [(2, 5, 15, 100, 200)]


def test_arrival_order_across_ingest_calls():
    op = R.ReferenceJoinOperator(10, 10)
    op.ingest(0, *cols((1, 1, 100)))
    op.ingest(1, *cols((1, 2, 200)))
    op.ingest(0, *cols((1, 0, 101)))
    op.ingest(1, *cols((1, 1, 201)))
    assert [r[3:] for r in rows(op.end_input())] == [(100, 200), (100, 201), (101, 200), (101, 201)]


GEOMETRIES = [dict(assigner="tumbling", size=100), dict(assigner="sliding", size=100, slide=50),
              dict(assigner="sliding", size=100, slide=30, offset=10)]


@pytest.mark.parametrize("seed", range(21))
def test_union_matches_the_oracle_count(oracle_lib, seed):
    geo = GEOMETRIES[seed % 3]
    size, slide, offset = geo["size"], geo.get("slide", geo["size"]), geo.get("offset", 0)
    # disorder up to 600 against a watermark lag of 50 and windows of 100: a record displaced by
    # more than 250 behind a batch's newest is late for every geometry
    keys, ts, _, batches = random_stream(seed, 600, 9, 6, disorder=600, wm_lag=50, agg="count")
    side = np.random.default_rng(1000 + seed).integers(0, 2, len(keys))
    pay = np.arange(len(keys), dtype=np.int64)
    ora = oracle_lib.OracleOperator(oracle_lib.make_config(agg="count", **geo))
    ref = R.ReferenceJoinOperator(size, slide, offset)
    fired = 0
    for lo, hi, wm in batches + [(len(keys), len(keys), R.I64_MAX)]:
        sl = slice(lo, hi)
        ora.process_batch(keys[sl], ts[sl], np.zeros(hi - lo, np.int64))
        for sd in (0, 1):
            m = side[sl] == sd
            ref.ingest(sd, keys[sl][m], ts[sl][m], pay[sl][m])
        ora.process_watermark(wm)
        out = ref.advance_watermark(wm)
        k, s, e, r = ora.drain()
        want = {(int(s[i]), int(k[i])): int(r[i]) for i in range(len(k))}
        assert all(int(e[i]) == int(s[i]) + size for i in range(len(k)))
        assert {g: l + r_ for g, (l, r_) in ref.last_fired.items()} == want
        assert len(out[0]) == sum(l * r_ for l, r_ in ref.last_fired.values())
        fired += len(want)
    assert fired > 0 and ref.late_dropped == ora.late_dropped and ref.late_dropped > 0
