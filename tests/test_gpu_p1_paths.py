"""Pass 1 of the region ingest (gw_pane.hip k_rgn_p1_lean / k_rgn_p1) against the oracle, at the
places where its two record paths meet: the lean classification of the unrolled pass (in ring,
or late and merely counted; 32-bit pane arithmetic) and the full classify of the rare pass
(everything else, with the counts the lean pass leaves to it).

* tile edges: batches of 1, 511, 512, 513, 4095, 4096, 4097 and 2 * 4096 + 1 records; 4096
  records of one key (one bucket counter reaches 4096) beside batches whose every record is
  special;
* time origin and width: timestamps from 0, 1.7e12 and -5e9; pane widths 1, 3, 7, 1000 and
  86 400 000 and a tumbling size beyond 2^32 ms; records at t_late - 1, t_late,
  t_late + 2^32 - 1 and t_late + 2^32; far-future records inside one 64-record stretch;
* special records among ordinary ones: a Long.MIN_VALUE timestamp, the sentinel key, late
  records with and without the side output, allowed lateness with re-fires, window classes,
  a gapped assigner (the general kernel), keys and values just beyond the narrow and the
  compact records;
* count, sum_i64, min_i64 and avg_f64; narrow and compact records; packed exchange words once.
Rows are compared per watermark (bit-exact; averages 1e-6 relative), with
num_late_records_dropped and the side output's rows."""
import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import windowing as W
from gpu_helpers import compare, make_assigner

pytestmark = pytest.mark.gpu

AGGS = ["count", "sum_i64", "min_i64", "avg_f64"]
FMTS = [(0, "narrow"), (N.FLAG_NO_NARROW, "compact")]


def make_stream(seed, sizes, num_keys, ts0=0, step=5, disorder=300, wm_lag=300, agg="sum_i64", key_hi=None):
    """Batches of the given sizes; timestamps advance by `step` per record from ts0 with bounded
    disorder; the watermark after a batch is maxTs - wm_lag - 1 (no late record while
    disorder <= wm_lag)."""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    pool = rng.integers(0, key_hi or (1 << 27), num_keys).astype(np.int64)
    keys = pool[rng.integers(0, num_keys, n)]
    ts = ts0 + np.arange(n, dtype=np.int64) * step - rng.integers(0, disorder + 1, n).astype(np.int64)
    if agg == "avg_f64":
        vals = rng.uniform(-1000.0, 1000.0, n).astype(np.float64)
    else:
        vals = rng.integers(-(10 ** 6), 10 ** 6, n).astype(np.int64)
    cuts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    batches = [(int(cuts[b]), int(cuts[b + 1]), int(ts[:cuts[b + 1]].max()) - wm_lag - 1) for b in range(len(sizes))]
    return keys, ts, vals, batches


def run_both(oracle_lib, kw, keys, ts, vals, batches, cap=1 << 14, flags=0, side=False, lean="all"):
    """Operator and oracle over the same batches: rows per watermark, the late count, the side
    output.  lean: which pass-1 launches must have taken k_rgn_p1_lean (gw_kernel_time_ms
    selectors 9 and 10 count the lean and the general launches): "all", "none", or None where
    the handle is a composite of window classes.  Returns the record formats the region path used."""
    extra = N.FLAG_LATE_SIDE_OUTPUT if side else 0
    op = W.GpuWindowOperator(make_assigner(kw), kw["agg"], kw.get("lateness", 0), capacity_hint=cap,
                             flags=N.FLAG_FORCE_REGION | flags | extra).open()
    ora = oracle_lib.OracleOperator(oracle_lib.make_config(**kw, flags=extra) if side else oracle_lib.make_config(**kw))
    if kw["agg"] == "count":
        vals = np.zeros(len(keys), np.int64)  # COUNT takes no value column: the side output's values are 0
    vb = vals.view(np.int64) if vals.dtype == np.float64 else vals
    g, o, fmts, n_side = [], [], [], 0
    try:
        for b, (lo, hi, wm) in enumerate(list(batches) + [(0, 0, W.LONG_MAX)]):
            if hi > lo:
                op.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi] if kw["agg"] != "count" else None)
                fmts.append(op.stats()["region_format"])
                ora.process_batch(keys[lo:hi], ts[lo:hi], vb[lo:hi])
            op.advance_watermark(wm)
            ora.process_watermark(wm)
            k, s, e, r = op.drain()
            g.append((k, s, e, r.view(np.int64)))
            o.append(ora.drain())
            if side:
                got = sorted(zip(*[c.tolist() for c in op.drain_late()]))
                exp = sorted(zip(*[c.tolist() for c in ora.drain_late()]))
                assert got == exp, f"side output differs at watermark #{b}"
                n_side += len(exp)
        assert op.num_late_records_dropped == ora.late_dropped
        late = ora.late_dropped
        n_lean, n_general = op.kernel_time_ms(9)[1], op.kernel_time_ms(10)[1]
    finally:
        op.close()
        ora.close()
    if lean is not None:
        # (a batch may take no pass 1 at all: few keys go through the pre-aggregation path)
        assert (n_general == 0 and n_lean > 0) if lean == "all" else (n_lean == 0 and n_general > 0), (n_lean, n_general)
    assert compare(g, o, kw["agg"].startswith("avg")) == []
    assert sum(len(x[0]) for x in o) > 0
    return fmts, late, n_side


# ------------------------------------------------------------------ tile edges
EDGE_SIZES = [1, 511, 512, 513, 4095, 4096, 4097, 2 * 4096 + 1]


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("flags", [f for f, _ in FMTS], ids=[i for _, i in FMTS])
@pytest.mark.parametrize("cap", [1 << 14, 1 << 19], ids=["single-pass", "two-pass"])
def test_tile_edges(oracle_lib, agg, flags, cap):
    kw = dict(assigner="sliding", size=2000, slide=500, agg=agg)
    keys, ts, vals, batches = make_stream(3, EDGE_SIZES, 3000, agg=agg)
    fmts, _, _ = run_both(oracle_lib, kw, keys, ts, vals, batches, cap, flags,
                          lean="none" if agg == "avg_f64" else "all")  # wide records: the general kernel
    if agg != "avg_f64":
        assert set(fmts) == ({1} if flags else {2})


@pytest.mark.parametrize("agg", ["count", "sum_i64"])
@pytest.mark.parametrize("flags", [f for f, _ in FMTS], ids=[i for _, i in FMTS])
def test_one_key_tile_beside_all_special_batches(oracle_lib, agg, flags):
    """A tile of one key (its bucket counter reaches 4096, every rank atomic of the tile on one
    address), a tile in which no record has a bucket (all far in the future: deferred), and a
    tile of keys beyond the narrow record (special for narrow records, ordinary for compact)."""
    kw = dict(assigner="sliding", size=2000, slide=500, agg=agg)
    keys, ts, vals, batches = make_stream(5, [4096, 4096, 4096, 4096, 3000], 500)
    keys[0:4096] = 77
    ts[4096:8192] += 10 ** 9                  # beyond the ring: the deferred list
    keys[8192:12288] += 1 << 33               # beyond 32 bits
    near = np.ones(len(ts), bool)
    near[4096:8192] = False                   # the far-future batch does not move the watermark
    batches = [(lo, hi, int(ts[:hi][near[:hi]].max()) - 301) for lo, hi, _ in batches]
    run_both(oracle_lib, kw, keys, ts, vals, batches, 1 << 14, flags)


# ------------------------------------------------------------------ time origin and width
@pytest.mark.parametrize("ts0", [0, 1_700_000_000_000, -5_000_000_000], ids=["epoch0", "now", "negative"])
@pytest.mark.parametrize("width", [1, 3, 7, 1000, 86_400_000])
def test_origins_and_pane_widths(oracle_lib, ts0, width):
    """Pane width = gcd(size, slide) = slide; the stream spans ~12 panes, with records up to
    three panes behind (late: both of their windows have fired)."""
    kw = dict(assigner="sliding", size=2 * width, slide=width, agg="sum_i64")
    n, lag = 9000, max(1, width // 3)
    keys, _, vals, _ = make_stream(width % 97 + 1, [n], 700)
    ts = ts0 + (np.arange(n, dtype=np.int64) * 12 * width) // n - np.random.default_rng(1).integers(0, 3 * width + 2 * lag + 1, n)
    cuts = [b * (n // 6) for b in range(7)]
    batches = [(cuts[b], cuts[b + 1], int(ts[:cuts[b + 1]].max()) - lag - 1) for b in range(6)]
    fmts, late, _ = run_both(oracle_lib, kw, keys, ts, vals, batches)
    assert late > 0 and set(fmts) == {2}


@pytest.mark.parametrize("agg", ["sum_i64", "count"])
def test_tumbling_size_beyond_32_bits(oracle_lib, agg):
    size = (1 << 32) + 1000
    kw = dict(assigner="tumbling", size=size, slide=size, agg=agg)
    n = 8000
    keys, ts, vals, batches = make_stream(11, [n // 16] * 16, 300, step=3 * size // n, disorder=size // 4, wm_lag=size // 16)
    _, late, _ = run_both(oracle_lib, kw, keys, ts, vals, batches, lean="none")  # the ring ends beyond 2^32 ms
    assert late > 0


@pytest.mark.parametrize("flags", [f for f, _ in FMTS], ids=[i for _, i in FMTS])
@pytest.mark.parametrize("ts0", [0, -5_000_000_000], ids=["epoch0", "negative"])
def test_records_around_t_late_and_its_32_bit_horizon(oracle_lib, flags, ts0):
    """Tumbling 1000 ms from an origin that is a window start: after the watermark t0 + 4999,
    t_late = t0 + 5000.  Records at t_late - 1 (late), t_late, t_late + 2^32 - 1 (the last the
    32-bit division takes) and t_late + 2^32 (special), and three far-future records within one
    64-record stretch of ordinary ones: deferred, fired at the end."""
    kw = dict(assigner="tumbling", size=1000, slide=1000, agg="sum_i64")
    keys, ts, vals, _ = make_stream(13, [6000], 200, ts0=ts0, step=1, disorder=0)
    t_late = ts0 + 5000
    first = np.nonzero(ts >= t_late)[0][0]
    hits = {first + 3: t_late - 1, first + 4: t_late, first + 5: t_late + (1 << 32) - 1, first + 6: t_late + (1 << 32),
            first + 100: t_late + 10 ** 12, first + 131: t_late + 10 ** 12 + 1, first + 163: t_late + (1 << 40)}
    for i, t in hits.items():
        ts[i] = t
    batches = [(0, int(first), t_late - 1), (int(first), 6000, t_late + 400)]
    _, late, _ = run_both(oracle_lib, kw, keys, ts, vals, batches, 1 << 14, flags)
    assert late == 1


# ------------------------------------------------------------------ special kinds among ordinary records
def test_no_timestamp_record_fails_the_operator():
    keys, ts, vals, _ = make_stream(17, [5000], 100)
    ts[2345] = W.LONG_MIN
    op = W.GpuWindowOperator(W.TumblingEventTimeWindows.of(1000), "sum_i64", capacity_hint=1 << 14,
                             flags=N.FLAG_FORCE_REGION).open()
    try:
        with pytest.raises(N.GpuWinError) as ei:
            op.process_batch(keys, ts, vals)
            op.advance_watermark(W.LONG_MAX)
        assert ei.value.code == N.GW_E_NO_TIMESTAMP
    finally:
        op.close()


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("flags", [f for f, _ in FMTS], ids=[i for _, i in FMTS])
def test_sentinel_key(oracle_lib, agg, flags):
    kw = dict(assigner="sliding", size=2000, slide=500, agg=agg)
    keys, ts, vals, batches = make_stream(19, [5000, 4097, 3000], 400, agg=agg)
    keys[::61] = W.LONG_MIN
    run_both(oracle_lib, kw, keys, ts, vals, batches, 1 << 14, flags, lean="none" if agg == "avg_f64" else "all")


@pytest.mark.parametrize("side", [False, True], ids=["dropped", "side-output"])
@pytest.mark.parametrize("kw", [dict(assigner="tumbling", size=1000, slide=1000),
                                dict(assigner="sliding", size=1500, slide=500, lateness=300),   # re-fires
                                dict(assigner="sliding", size=1000, slide=10),                  # window classes
                                dict(assigner="sliding", size=300, slide=1000)],                # gapped: the general P1
                         ids=["tumbling", "lateness", "classes", "gapped"])
@pytest.mark.parametrize("agg", ["sum_i64", "count"])
def test_late_records(oracle_lib, kw, side, agg):
    kw = dict(kw, agg=agg)
    keys, ts, vals, batches = make_stream(23, [4000, 4097, 513, 5000, 3000], 300, step=1, disorder=3000, wm_lag=200)
    which = {10: None, 1000: "none"}.get(kw.get("slide"), "all") if kw["assigner"] == "sliding" else "all"
    _, late, n_side = run_both(oracle_lib, kw, keys, ts, vals, batches, side=side, lean=which)
    assert (n_side > 0 and late == 0) if side else late > 0


@pytest.mark.parametrize("agg", ["sum_i64", "min_i64", "count"])
def test_keys_and_values_just_beyond_the_narrow_record(oracle_lib, agg):
    kw = dict(assigner="sliding", size=2000, slide=500, agg=agg)
    keys, ts, vals, batches = make_stream(29, [6000, 4097, 4000], 2000, key_hi=(1 << 28) - 1)
    rng = np.random.default_rng(2)
    m = rng.random(len(keys)) < 0.008  # few enough for the handle to keep narrow records
    keys[m] = rng.choice(np.array([(1 << 32) - 3, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 28) - 1, 1 << 28, -1], np.int64), int(m.sum()))
    m = rng.random(len(keys)) < 0.008
    vals[m] = rng.choice(np.array([(1 << 27) - 1, 1 << 27, -(1 << 27), -(1 << 27) - 1], np.int64), int(m.sum()))
    fmts, _, _ = run_both(oracle_lib, kw, keys, ts, vals, batches)
    assert set(fmts) == {2}


@pytest.mark.parametrize("agg", ["sum_i64", "min_i64"])
def test_values_just_beyond_the_compact_record(oracle_lib, agg):
    kw = dict(assigner="sliding", size=2000, slide=500, agg=agg)
    keys, ts, vals, batches = make_stream(31, [6000, 4097, 4000], 2000, key_hi=1 << 40)
    rng = np.random.default_rng(3)
    m = rng.random(len(keys)) < 0.008
    vals[m] = rng.choice(np.array([(1 << 31) - 1, 1 << 31, -(1 << 31), -(1 << 31) - 1], np.int64), int(m.sum()))
    fmts, _, _ = run_both(oracle_lib, kw, keys, ts, vals, batches, flags=N.FLAG_NO_NARROW)
    assert set(fmts) == {1}


# ------------------------------------------------------------------ packed exchange words (the general P1 decodes them)
def test_packed_words_once(oracle_lib):
    import torch
    kw = dict(assigner="sliding", size=1000, slide=250, agg="sum_i64")
    keys, ts, vals, batches = make_stream(37, [5000, 4097, 4000, 3000], 800, step=1, disorder=300, wm_lag=300)
    op = W.GpuWindowOperator(make_assigner(kw), "sum_i64", capacity_hint=1 << 14, flags=N.FLAG_FORCE_REGION).open()
    ora = oracle_lib.OracleOperator(oracle_lib.make_config(**kw))
    g, o, last, packed, n_plain = [], [], W.LONG_MIN, 0, 0
    s = torch.cuda.current_stream().cuda_stream
    try:
        for lo, hi, wm in batches:
            k, t, v = keys[lo:hi], ts[lo:hi], vals[lo:hi]
            geom = N.pack_geom(1000, 250, 0, last)
            if geom is None:
                op.process_batch(k, t, v)
                n_plain += 1
            else:
                w, fits = N.pack_records(k, t, v, geom)
                rest = ~fits
                dk, dt, dv = (torch.from_numpy(np.ascontiguousarray(x[rest])).cuda() for x in (k, t, v))
                dw = torch.from_numpy(np.ascontiguousarray(w[fits]).view(np.int64)).cuda()
                torch.cuda.synchronize()
                some = bool(rest.any())
                op.process_batch_packed_device_ptr(int(rest.sum()), dk.data_ptr() if some else None,
                                                   dt.data_ptr() if some else None, dv.data_ptr() if some else None,
                                                   int(fits.sum()), dw.data_ptr() if fits.any() else None, geom, stream=s)
                torch.cuda.synchronize()
                packed += int(fits.sum())
            ora.process_batch(k, t, v)
            for wmk in (wm,) if hi < len(keys) else (wm, W.LONG_MAX):
                op.advance_watermark(wmk)
                kk, ss, ee, rr = op.drain()
                g.append((kk, ss, ee, rr.view(np.int64)))
                ora.process_watermark(wmk)
                o.append(ora.drain())
            last = wm
        assert op.num_late_records_dropped == ora.late_dropped
        # launches with packed words take the general kernel, the others the lean one
        assert op.kernel_time_ms(9)[1] == n_plain and op.kernel_time_ms(10)[1] > 0
    finally:
        op.close()
        ora.close()
    assert packed > 0.5 * len(keys)
    assert compare(g, o, False) == []
