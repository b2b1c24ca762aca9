"""The fused fire (gw_runtime.cpp fast_fire, gw_pane.hip k_rgn_apply_nar<AGG, true, true>): the
apply kernel of a firing nar2 flush emits the window's rows itself, a guard behind it revokes
them when the flush left something the host has to see first, and k_fire_retire retires the
panes.  Every case compares every watermark's rows and the late count with the oracle; the
cases differ in whether the fused path must be taken, must be revoked or must not be tried.

Reference: WindowOperator.onEventTime (RS/runtime/operators/windowing/WindowOperator.java:
439-494): the rows of every watermark are the oracle's, whichever kernel wrote them.
"""
import zlib

import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import windowing as W
from gpu_helpers import compare, gpu_operator, random_stream, run_oracle

pytestmark = pytest.mark.gpu

SLIDING = dict(assigner="sliding", size=30_000, slide=10_000)
TWO_PASS = dict(flags=N.FLAG_FORCE_REGION, capacity_hint=600_000)  # the two-pass nar2 table


def run_gpu(kw, keys, ts, vals, batches, **opkw):
    """gpu_helpers.run_gpu with the fused fires (gw_kernel_time_ms selector 4) and the revoked
    ones (selector 5) counted; stats["fused_at"][i]: watermark i's rows came from a fused fire."""
    op = gpu_operator(kw, **opkw)
    outs, fused_at = [], []
    try:
        for lo, hi, wm in list(batches) + [(0, 0, W.LONG_MAX)]:
            if hi > lo:
                op.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi])
            before = op.kernel_time_ms(4)[1]
            op.advance_watermark(wm)
            fused_at.append(op.kernel_time_ms(4)[1] > before)
            k, s, e, r = op.drain()
            outs.append((k, s, e, r.view(np.int64)))
        late = op.num_late_records_dropped
        stats = op.stats()
        stats["fast_fires"] = op.kernel_time_ms(3)[1]
        stats["fused_fires"] = op.kernel_time_ms(4)[1]
        stats["fused_revoked"] = op.kernel_time_ms(5)[1]
        stats["fused_at"] = fused_at
    finally:
        op.close()
    return outs, late, stats


def _run(oracle_lib, kw, stream, **opkw):
    keys, ts, vals, batches = stream
    g, glate, stats = run_gpu(kw, keys, ts, vals, batches, **opkw)
    o, olate = run_oracle(oracle_lib, kw, keys, ts, vals, batches)
    assert glate == olate
    assert compare(g, o, kw["agg"].endswith("f64")) == []
    assert stats["fused_fires"] <= stats["fast_fires"] <= stats["fires"], stats
    return stats, g


def _no_row_twice(outs):
    k = np.concatenate([x[0] for x in outs])
    s = np.concatenate([x[1] for x in outs])
    rows = np.stack([k, s], axis=1)
    assert len(np.unique(rows, axis=0)) == len(rows)


@pytest.mark.parametrize("agg", ["sum_i64", "count"])
def test_fused_fire_taken_and_exact(oracle_lib, agg):
    """The stream of test_gpu_fast_fire.test_fast_fire_taken_and_exact[region-buffered] (same
    seed): there `fast_fires` meets this bound without the fused path, the cold first fires
    being the allowance."""
    kw = dict(SLIDING, agg=agg)
    stream = random_stream(seed=zlib.crc32(f"ff{agg}{N.FLAG_FORCE_REGION}{600_000}".encode()) & 0xffff, n=200_000,
                           num_keys=20_000, n_batches=60, ts_step=1, agg=agg)
    stats, _ = _run(oracle_lib, kw, stream, **TWO_PASS)
    assert stats["fires"] >= 10
    assert stats["fused_fires"] >= stats["fires"] // 2, stats


def _interval_stream(seed, counts, keyfn):
    """Slide intervals of 10 000 ms, interval i holding counts[i] records evenly spread with the
    keys keyfn(i, rng, count), three batches per interval.  Disorder within the watermark lag:
    no record is late."""
    rng = np.random.default_rng(seed)
    tss, ks, cuts = [], [], [0]
    for i, cnt in enumerate(counts):
        tss.append(i * 10_000 + (np.arange(cnt, dtype=np.int64) * 10_000) // cnt)
        ks.append(keyfn(i, rng, cnt).astype(np.int64))
        start = cuts[-1]
        cuts += [start + cnt * j // 3 for j in (1, 2, 3)]
    ts = np.concatenate(tss)
    ts = ts - rng.integers(0, 301, len(ts))
    keys = np.concatenate(ks)
    vals = rng.integers(-(10 ** 6), 10 ** 6, len(ts)).astype(np.int64)
    batches = [(cuts[b], cuts[b + 1], int(ts[:cuts[b + 1]].max()) - 301) for b in range(len(cuts) - 1)]
    assert batches[-1][1] == len(ts)
    return keys, ts, vals, batches


def test_fused_fire_sentinel_key(oracle_lib):
    """The key Long.MIN_VALUE lives in the sentinel slot, which belongs to no super-region:
    workgroup 0 emits its row beside the rows of its super-region.  No narrow record holds
    that key, so its records go the deferred way and the fire behind their flush falls back;
    they arrive in one pane in mid-stream only, and the next fires, whose window still covers
    that pane, are fused."""
    kw = dict(SLIDING, agg="sum_i64")
    keys, ts, vals, batches = random_stream(seed=61, n=200_000, num_keys=20_000, n_batches=60, ts_step=1)
    keys = np.where((ts >= 100_500) & (ts < 109_000) & (np.arange(len(ts)) % 97 == 0), W.LONG_MIN, keys)
    stats, g = _run(oracle_lib, kw, (keys, ts, vals, batches), **TWO_PASS)
    assert stats["fused_fires"] >= stats["fires"] // 2, stats
    with_row = [int((x[0] == W.LONG_MIN).sum()) for x in g]
    assert sum(with_row) == 3 and max(with_row) == 1, with_row  # the three windows over that pane
    assert any(f and c for f, c in zip(stats["fused_at"], with_row)), (stats["fused_at"], with_row)


def _idle_stream(num_keys=20_000, per=10_000, n_int=20, sparse=(9, 14), stop_after=7):
    """`per` records per interval, but ~50 in the `sparse` ones; the keys below num_keys / 3
    stop arriving after interval `stop_after` (batch 21)."""
    def keyfn(i, rng, cnt):
        k = rng.integers(0, num_keys, cnt)
        return k if i < stop_after else num_keys // 3 + k % (num_keys - num_keys // 3)
    return _interval_stream(21, [50 if i in sparse else per for i in range(n_int)], keyfn)


@pytest.mark.parametrize("agg", ["sum_i64", "count"])
def test_fused_fire_idle_super_regions(oracle_lib, agg):
    """Flushes of ~50 records leave most super-regions without a record: their workgroups
    still emit the rows of keys whose records sit in the window's older panes (and of the keys
    that stopped arriving, until their last window has fired)."""
    kw = dict(SLIDING, agg=agg)
    stats, _ = _run(oracle_lib, kw, _idle_stream(), **TWO_PASS)
    assert stats["fused_fires"] >= stats["fires"] // 2, stats


def test_fused_fire_table_growth(oracle_lib):
    """A table sized for 2000 keys gets 300k (the stream of test_fast_fire_guard_table_growth):
    it is single-pass, so no fire is fused, until its last growth; from then on fires may be.
    Rows stay exact across the change of path and no row appears twice."""
    kw = dict(assigner="sliding", size=400_000, slide=200_000, agg="sum_i64")
    stream = random_stream(seed=5, n=1_200_000, num_keys=300_000, n_batches=12, ts_step=1)
    stats, g = _run(oracle_lib, kw, stream, flags=N.FLAG_FORCE_REGION, capacity_hint=2000)
    assert stats["rehashes"] > 0
    _no_row_twice(g)


def test_fused_fire_revoked_row_buffer(oracle_lib):
    """The rows of one fused fire exceed the row buffer.  The two-pass table hinted at 600 000
    keys has 1 048 576 slots (it grows past 734 003 keys, at the next ingest) and a row buffer of
    750 000 rows.  After eight intervals of 20 000 keys one interval brings 740 000 new ones:
    the guard before the launch sees room (20 001 rows wanted), the apply inserts the keys
    without a spill, and the window's 760 000 rows do not fit: the workgroups whose
    reservation passes the end write nothing and revoke the fire, the guard behind puts the
    row cursor back, the exact path grows the buffer and fires.  A row of the revoked fire left
    in the buffer, or a missing one, breaks the parity of that watermark."""
    kw = dict(SLIDING, agg="sum_i64")
    burst = 8

    def keyfn(i, rng, cnt):
        return 20_000 + np.arange(cnt) % 740_000 if i == burst else rng.integers(0, 20_000, cnt)
    stream = _interval_stream(23, [800_000 if i == burst else 10_000 for i in range(14)], keyfn)
    stats, g = _run(oracle_lib, kw, stream, **TWO_PASS)
    assert max(len(x[0]) for x in g) > 750_000
    assert stats["fused_revoked"] >= 1, stats
    assert stats["fused_fires"] >= 4, stats  # before the burst and after it
    _no_row_twice(g)


def _foreign_stream(seed, t_lo, t_hi):
    """~0.5% of the keys >= 2^32 and ~0.5% of the values >= 2^27 among the records with
    t_lo <= ts < t_hi (below the 1/64 that turns narrow records off)."""
    keys, ts, vals, batches = random_stream(seed=seed, n=200_000, num_keys=20_000, n_batches=60, ts_step=1)
    rng = np.random.default_rng(seed + 1)
    inr = (ts >= t_lo) & (ts < t_hi)
    big_k = inr & (rng.random(len(ts)) < 0.005)
    big_v = inr & (rng.random(len(ts)) < 0.005)
    keys = np.where(big_k, keys + (1 << 32) + (keys << 20), keys)
    vals = np.where(big_v, vals + (1 << 40), vals)
    return keys, ts, vals, batches


def test_fused_fire_foreign_and_wide_everywhere(oracle_lib):
    """Records no narrow record holds go the deferred way, so the fires behind their flushes
    fall back to the exact path."""
    kw = dict(SLIDING, agg="sum_i64")
    stats, _ = _run(oracle_lib, kw, _foreign_stream(31, 0, 1 << 40), **TWO_PASS)
    assert stats["region_format"] == 2, stats  # narrow records stayed on
    # every fire cycle (~10 000 records) carries ~50 such keys and ~50 such values: pass 1 defers
    # them, so no fire may keep fused rows (the guard before the launch sees the deferred entries)
    assert stats["fires"] >= 10
    assert stats["fused_fires"] == 0, stats


def test_fused_fire_foreign_slots_under_fused_fires(oracle_lib):
    """Large keys in one pane in mid-stream only: the fire behind their flush falls back, the
    following fires are fused while the window still covers that pane -- the rows of slots
    whose key has no 32-bit form take the key from the table.  (Not in the first window: the
    first fires of a stream are cold and take the exact path whatever they hold, so foreign
    slots there would meet no fused fire; a pane in mid-stream is followed by two warm fires
    whose window still covers it.)"""
    kw = dict(SLIDING, agg="sum_i64")
    stats, g = _run(oracle_lib, kw, _foreign_stream(33, 100_500, 109_000), **TWO_PASS)
    assert stats["fused_fires"] >= stats["fires"] // 2, stats
    big = [int((x[0] >= (1 << 32)).sum()) for x in g]
    assert any(f and c for f, c in zip(stats["fused_at"], big)), (stats["fused_at"], big)


@pytest.mark.parametrize("kw,n_batches", [
    (dict(SLIDING, agg="sum_i64", lateness=5_000), 60),
    (dict(SLIDING, agg="max_f64"), 60),
    (dict(SLIDING, agg="avg_f64"), 60),
    (dict(SLIDING, agg="sum_i64"), 10),  # every watermark completes two windows
], ids=["lateness", "max_f64", "avg_f64", "two-windows"])
def test_fused_fire_not_taken(oracle_lib, kw, n_batches):
    stream = random_stream(seed=41, n=200_000, num_keys=20_000, n_batches=n_batches, ts_step=1, agg=kw["agg"])
    stats, _ = _run(oracle_lib, kw, stream, **TWO_PASS)
    assert stats["fires"] >= 5
    assert stats["fused_fires"] == 0, stats


def test_fused_fire_state_snapshot(oracle_lib):
    """Right after a fused fire the state is the oracle's (heap-layout blobs compared as
    test_gpu_restore does), and both sides continue alike from it."""
    from test_gpu_restore import feed_gpu, feed_oracle, resume, same_state
    kw = dict(SLIDING, agg="sum_i64")
    keys, ts, vals, batches = random_stream(seed=51, n=200_000, num_keys=20_000, n_batches=60, ts_step=1)
    op = gpu_operator(kw, **TWO_PASS)
    ora = oracle_lib.OracleOperator(oracle_lib.make_config(**kw))
    go, oo = [], []
    cut = None
    try:
        for b in range(45):
            before = op.kernel_time_ms(4)[1]
            feed_gpu(op, keys, ts, vals, batches[b:b + 1], go)
            feed_oracle(ora, keys, ts, vals, batches[b:b + 1], oo)
            if b >= 30 and op.kernel_time_ms(4)[1] > before:
                cut = b + 1
                break
        assert cut is not None, "no fused fire between batches 30 and 45"
        blob = op.snapshot_state()
        same_state(blob, ora.snapshot(), kw["agg"])
    finally:
        op.close()
        ora.close()
    assert compare(go, oo, False) == []
    none = np.zeros(0, np.int64)
    g, glate, _ = resume("gpu", oracle_lib, kw, blob, keys, ts, vals, batches[cut:cut + 10], none)
    r, rlate, _ = resume("oracle", oracle_lib, kw, blob, keys, ts, vals, batches[cut:cut + 10], none)
    assert glate == rlate
    assert compare(g, r, False) == []
