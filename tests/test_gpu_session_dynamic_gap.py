"""Session windows with a per-element gap (GW_SESSION_DYNAMIC, gw_ingest_gap*: the DYN
instantiations of k_sess_prep / k_sess_segment / k_sess_wide in gw_session.hip) on the device.

* a constant gap column through the dynamic handle equals the C oracle's constant-gap run;
* varying gaps equal tests/session_dynamic_reference.py (pinned to that oracle by
  tests/test_session_dynamic_reference.py): rows per watermark, late count, side output and
  the merge count, on streams that reach the hard paths -- each test first asserts on the
  reference's own counters that its stream has late records, session-to-session merges, keys
  with many sessions, windows fired on element; S2 also that the GPU punted records of keys
  without a slot (the fourth punt column), S4 runs on a 2^25-slot table with grouped slots;
* the hand-written vectors of what only varying gaps produce;
* device columns, the error paths, snapshots (byte-equal body, restore, key-group slices, key
  tables, refusal across the two session assigners).
Parity: bit-exact for integer aggregates and f64 min / max, 1e-6 relative for f64 averages."""
import ctypes

import numpy as np
import pytest

import session_dynamic_reference as R
from flink_amd import _native as N
from flink_amd import windowing as W
from gpu_helpers import compare, gpu_operator, random_stream
from test_gpu_session_deferred import colliding_keys

pytestmark = pytest.mark.gpu

AGGS = ["count", "sum_i64", "avg_f64", "max_f64", "min_i64"]  # test_gpu_session_scenarios.AGGS


def dyn_operator(agg, lateness=0, trigger="event_time", side=False, capacity_hint=1024, max_batch=1 << 22):
    trig = W.PurgingTrigger.of(W.EventTimeTrigger.create()) if trigger == "purging_event_time" \
        else W.EventTimeTrigger.create()
    return W.GpuWindowOperator(W.DynamicEventTimeSessionWindows.with_dynamic_gap(lambda v: v[2]), agg, lateness, trig,
                               capacity_hint=capacity_hint, max_batch=max_batch,
                               flags=N.FLAG_LATE_SIDE_OUTPUT if side else 0).open()


def feed(op, keys, ts, vals, gaps, lo, hi, device=False):
    if hi <= lo:
        return
    if device:
        import torch
        cols = [torch.from_numpy(np.ascontiguousarray(x[lo:hi])).cuda() for x in (keys, ts, vals, gaps)]
        op.process_batch_device(cols[0], cols[1], cols[2], gaps=cols[3])
    else:
        op.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi], gaps=gaps[lo:hi])


def drain_into(op, outs):
    k, s, e, r = op.drain()
    outs.append((k, s, e, r.view(np.int64)))


def run_dynamic(op, keys, ts, vals, gaps, batches, device=False, final_wm=W.LONG_MAX):
    """-> per-watermark rows, late count, sorted side output, stats; closes the operator."""
    outs = []
    try:
        for lo, hi, wm in batches:
            feed(op, keys, ts, vals, gaps, lo, hi, device)
            op.advance_watermark(wm)
            drain_into(op, outs)
        if final_wm is not None:
            op.advance_watermark(final_wm)
            drain_into(op, outs)
        late = op.num_late_records_dropped
        side = sorted(zip(*[x.tolist() for x in op.drain_late()]))
        stats = op.stats()
    finally:
        op.close()
    return outs, late, side, stats


def check_against_reference(ref_out, ref, gpu, agg):
    outs, late, side, stats = gpu
    assert compare(outs, ref_out, agg == "avg_f64") == []
    assert late == ref.late_dropped
    assert side == sorted(zip(*[x.tolist() for x in ref.drain_late()]))
    assert stats["session_merges"] == ref.merges
    return stats


# ------------------------------------------------------------------------ streams S1 - S4
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def s1(agg="sum_i64"):
    return cached(("S1", agg in R.DOUBLE_INPUT), lambda: R.stream_s1("sum_f64" if agg in R.DOUBLE_INPUT else "sum_i64"))


def s1_gaps():
    return cached("S1g", lambda: R.gap_column(s1()[0], 12, [200, 5000, 30000, 100000], 1, 400000))


def s3(agg, lateness):
    return cached(("S3", agg in R.DOUBLE_INPUT, lateness), lambda: random_stream(
        seed=5, n=240_000, num_keys=6000, n_batches=2, ts_step=1, disorder=800 + lateness, wm_lag=400,
        agg="sum_f64" if agg in R.DOUBLE_INPUT else "sum_i64"))


# ------------------------------------------------- 1. constant column against the C oracle
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("gap,lateness", [(100, 0), (300, 1500)])
@pytest.mark.parametrize("name", ["S1", "S3"])
def test_constant_gap_column_equals_the_c_oracle(oracle_lib, name, gap, lateness, agg):
    keys, ts, vals, batches = s1(agg) if name == "S1" else s3(agg, lateness)
    gaps = np.full(len(keys), gap, np.int64)
    op = dyn_operator(agg, lateness, capacity_hint=1024 if name == "S1" else 2048)
    outs, late, _, _ = run_dynamic(op, keys, ts, vals, gaps, batches)
    ora = oracle_lib.OracleOperator(oracle_lib.make_config(assigner="session", gap=gap, agg=agg, lateness=lateness))
    vb = vals.view(np.int64) if vals.dtype == np.float64 else vals
    exp = []
    for lo, hi, wm in batches + [(0, 0, W.LONG_MAX)]:
        if hi > lo:
            ora.process_batch(keys[lo:hi], ts[lo:hi], vb[lo:hi])
        ora.process_watermark(wm)
        exp.append(ora.drain())
    olate = ora.late_dropped
    ora.close()
    assert late == olate
    assert compare(outs, exp, agg == "avg_f64") == []


# --------------------------------------- 2. varying gaps against the pinned Python reference
@pytest.mark.parametrize("lateness,side,trigger", [(0, False, "event_time"), (20_000, False, "event_time"),
                                                   (20_000, True, "event_time"), (20_000, False, "purging_event_time")])
def test_s1_many_sessions_per_key(lateness, side, trigger):
    keys, ts, vals, batches = s1()
    gaps = s1_gaps()
    ref_out, ref = R.run_reference(keys, ts, vals, gaps, batches, "sum_i64", lateness, trigger, side)
    c = ref.counters()
    assert c["late"] >= 5 and c["merges"] >= 20 and c["peak_sessions"] > 3, c
    if lateness:
        assert c["fired_on_element"] >= 20, c
    op = dyn_operator("sum_i64", lateness, trigger, side, capacity_hint=1024)
    check_against_reference(ref_out, ref, run_dynamic(op, keys, ts, vals, gaps, batches), "sum_i64")


def test_s2_more_keys_than_slots():
    keys, ts, vals, batches = random_stream(seed=9, n=120_000, num_keys=4000, n_batches=6, ts_step=1, disorder=300,
                                            wm_lag=100)
    keys[::97] = W.LONG_MIN
    # Uniform keys alone never lose a slot (the host grows the table for a batch's possible new
    # keys before the prep), so the stream as first drawn punted nothing.  A fifth of the records
    # go to 300 keys whose slot hashes agree in their low 16 bits: more than kMaxProbe (128) of
    # them share one home slot at every table size the batches start with
    # (test_gpu_session_deferred builds its punting streams the same way).
    rng = np.random.default_rng(72)
    hot = colliding_keys(300, low_bits=16)
    pick = rng.random(keys.size) < 0.2
    keys[pick] = hot[rng.integers(0, hot.size, int(pick.sum()))]
    gaps = R.gap_column(keys, 13, [5, 30, 200, 2000], 1, 20000)
    ref_out, ref = R.run_reference(keys, ts, vals, gaps, batches, "sum_i64")
    c = ref.counters()
    assert c["late"] >= 5 and c["peak_sessions"] > 3, c
    op = dyn_operator("sum_i64", capacity_hint=1024)
    stats = check_against_reference(ref_out, ref, run_dynamic(op, keys, ts, vals, gaps, batches), "sum_i64")
    assert stats["session_punted"] > 0  # records of keys without a slot took the punt columns, gap included


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("lateness", [0, 1500])
def test_s3_large_batches_table_grown_under_the_batch(agg, lateness):
    keys, ts, vals, batches = s3(agg, lateness)
    gaps = cached(("S3g", lateness), lambda: R.gap_column(keys, 14, [5, 30, 200, 2000], 1, 20000))
    ref_out, ref = R.run_reference(keys, ts, vals, gaps, batches, agg, lateness)
    c = ref.counters()
    assert c["late"] >= 5 and c["merges"] >= 20, c
    if lateness:
        assert c["fired_on_element"] >= 20, c
    op = dyn_operator(agg, lateness, capacity_hint=2048)
    stats = check_against_reference(ref_out, ref, run_dynamic(op, keys, ts, vals, gaps, batches), agg)
    assert stats["rehashes"] > 0


def test_s4_large_table_grouped_slots(monkeypatch):
    # 2^25 slots are 26 sorted slot bits; a sort over 24 of them leaves groups of four slots
    # whose runs one thread separates (seg_run with gshift > 0)
    monkeypatch.setenv("GW_SESSION_SORT_BITS", "24")
    keys, ts, vals, batches = random_stream(seed=21, n=120_000, num_keys=30_000, n_batches=4, ts_step=1,
                                            disorder=300, wm_lag=300)
    gaps = R.gap_column(keys, 15, [50, 300, 2000, 20000], 1, 100000)
    ref_out, ref = R.run_reference(keys, ts, vals, gaps, batches, "sum_i64")
    assert ref.counters()["peak_sessions"] > 3, ref.counters()
    op = dyn_operator("sum_i64", capacity_hint=20_000_000)
    stats = check_against_reference(ref_out, ref, run_dynamic(op, keys, ts, vals, gaps, batches), "sum_i64")
    assert stats["table_capacity"] == 1 << 25


# -------------------------------------------------------------- 3. the hand-written vectors
@pytest.mark.parametrize("name,lateness,steps,exp", R.VECTORS, ids=[v[0] for v in R.VECTORS])
def test_hand_written_vectors(name, lateness, steps, exp):
    op = dyn_operator("count", lateness)
    one = lambda x: np.array([x], np.int64)
    rows = []
    try:
        for s in steps:
            if s[0] == "w":
                op.advance_watermark(s[1])
            else:
                op.process_batch(one(R.VECTOR_KEY), one(s[1]), one(1), gaps=one(s[2]))
            k, a, b, r = op.drain()
            assert set(k.tolist()) <= {R.VECTOR_KEY}
            rows += list(zip(a.tolist(), b.tolist(), r.tolist()))
        assert rows == exp["rows"]
        assert op.num_late_records_dropped == exp["late"]
        assert op.stats()["session_merges"] == exp["merges"]
        op.advance_watermark(W.LONG_MAX)  # the sessions in flight (a fired one that is kept does not fire again)
        _, a, b, _ = op.drain()
        fired_before = {(x, y) for x, y, _ in exp["rows"]}
        assert sorted(zip(a.tolist(), b.tolist())) == [w for w in exp["sessions"] if w not in fired_before]
    finally:
        op.close()


def test_process_element_evaluates_the_extractor():
    op = W.GpuWindowOperator(W.DynamicEventTimeSessionWindows.with_dynamic_gap(lambda v: v[2]), "sum_i64").open()
    try:
        for k, v, g, t in [(1, 5, 10, 0), (1, 6, 10, 30), (1, 7, 30, 5), (2, 1, 3, 0)]:
            op.process_element(W.StreamRecord((k, v, g), t))
        op.process_watermark(W.MAX_WATERMARK)
        rows = sorted(r.value for r in op.get_output() if isinstance(r, W.StreamRecord))
        assert rows == [(1, 0, 40, 18), (2, 0, 3, 1)]
    finally:
        op.close()


# ---------------------------------------------------------------------- 4. device columns
def test_device_columns_equal_host_columns():
    keys, ts, vals, batches = s1()
    gaps = s1_gaps()
    host = run_dynamic(dyn_operator("sum_i64", 20_000, side=True), keys, ts, vals, gaps, batches)
    dev = run_dynamic(dyn_operator("sum_i64", 20_000, side=True), keys, ts, vals, gaps, batches, device=True)
    assert compare(dev[0], host[0], False) == []
    assert sum(len(x[0]) for x in host[0]) > 1000
    assert dev[1:3] == host[1:3] and len(host[2]) >= 5
    assert dev[3]["session_merges"] == host[3]["session_merges"]


# ------------------------------------------------------------------------------ 5. errors
def _one(x):
    return np.array([x], np.int64)


@pytest.mark.parametrize("lateness", [0, 10])  # deferred ingest (the error surfaces at the next call) / synchronous
@pytest.mark.parametrize("gap", [0, -5])
def test_a_gap_that_is_not_positive_fails_the_operator(gap, lateness):
    op = dyn_operator("count", lateness)
    try:
        k = np.arange(100, dtype=np.int64)
        g = np.full(100, 50, np.int64)
        g[37] = gap
        with pytest.raises(N.GpuWinError) as ei:
            op.process_batch(k, k * 3, k, gaps=g)
            op.advance_watermark(1000)
        assert ei.value.code == N.GW_E_INVALID
        assert "Dynamic session time gap must satisfy 0 < gap" in str(ei.value)
        with pytest.raises(N.GpuWinError) as ei:
            op.process_batch(k, k * 3, k, gaps=np.full(100, 50, np.int64))
        assert ei.value.code == N.GW_E_STATE
    finally:
        op.close()


@pytest.mark.parametrize("lateness", [0, 10])
def test_window_end_beyond_int64_is_a_range_error(lateness):
    op = dyn_operator("count", lateness)
    try:
        with pytest.raises(N.GpuWinError) as ei:
            op.process_batch(_one(1), _one(W.LONG_MAX - 5), _one(1), gaps=_one(10))
            op.advance_watermark(1000)
        assert ei.value.code == N.GW_E_RANGE
        with pytest.raises(N.GpuWinError) as ei:
            op.process_batch(_one(1), _one(5), _one(1), gaps=_one(10))
        assert ei.value.code == N.GW_E_STATE
    finally:
        op.close()


def _err(h):
    return N.lib().gw_last_error(h).decode()


def test_cross_use_is_invalid():
    L = N.lib()
    k = _one(1)
    p = k.ctypes.data
    dyn = dyn_operator("count")
    ses = gpu_operator(dict(assigner="session", gap=10, agg="count"))
    tum = gpu_operator(dict(assigner="tumbling", size=10, agg="count"))
    try:
        assert L.gw_ingest(dyn.handle, 1, p, None, p, p) == N.GW_E_INVALID and "gap column" in _err(dyn.handle)
        assert L.gw_ingest_device(dyn.handle, 1, p, None, p, p, None) == N.GW_E_INVALID
        assert "gap column" in _err(dyn.handle)
        for op in (ses, tum):
            assert L.gw_ingest_gap(op.handle, 1, p, None, p, p, p) == N.GW_E_INVALID
            assert "not a GW_SESSION_DYNAMIC handle" in _err(op.handle)
            assert L.gw_ingest_gap_device(op.handle, 1, p, None, p, p, p, None) == N.GW_E_INVALID
            assert "not a GW_SESSION_DYNAMIC handle" in _err(op.handle)
        assert L.gw_ingest_gap(dyn.handle, 1, p, None, p, p, None) == N.GW_E_INVALID and "null gap" in _err(dyn.handle)
        assert L.gw_ingest_gap_device(dyn.handle, 1, p, None, p, p, None, None) == N.GW_E_INVALID
        assert "null gap" in _err(dyn.handle)
        assert L.gw_ingest_gap(dyn.handle, 0, None, None, None, None, None) == N.GW_OK  # no records, no columns
        # none of this failed the operators
        dyn.process_batch(k, k, k, gaps=_one(5))
        ses.process_batch(k, k, k)
        assert dyn.advance_watermark(W.LONG_MAX) == 1 and ses.advance_watermark(W.LONG_MAX) == 1
    finally:
        for op in (dyn, ses, tum):
            op.close()


def test_unsupported_on_a_dynamic_handle():
    import torch
    L = N.lib()
    op = dyn_operator("sum_i64")
    try:
        def unsupported(call):
            with pytest.raises(N.GpuWinError) as ei:
                call()
            assert ei.value.code == N.GW_E_UNSUPPORTED
            assert "GW_SESSION_DYNAMIC" in str(ei.value) or "session" in str(ei.value)
        lay = N.record_layout("JJ", 0, 1)
        unsupported(lambda: op.stage_alloc(2, 1024))
        unsupported(lambda: op.process_serialized(b"\x00" * 32, lay))
        unsupported(lambda: op.process_serialized_device(torch.zeros(32, dtype=torch.uint8, device="cuda"), lay))
        g = N.GwPackGeom()
        unsupported(lambda: op.process_batch_packed_device_ptr(0, None, None, None, 0, None, g))
        op.process_batch(_one(1), _one(1), _one(1), gaps=_one(5))
        op.advance_watermark(W.LONG_MAX)
        unsupported(lambda: op.top_n_rows(1))
        assert op.pending_rows() == 1  # the handle still works
    finally:
        op.close()


# --------------------------------------------------------------------------- 6. snapshots
def test_blob_body_equals_the_constant_gap_handles():
    keys, ts, vals, batches = s1()
    G, late = 30_000, 1500  # ten times the watermark's lag: most keys hold sessions at the snapshot
    dyn = dyn_operator("sum_i64", late, capacity_hint=1024)
    ses = gpu_operator(dict(assigner="session", gap=G, agg="sum_i64", lateness=late), capacity_hint=1024)
    try:
        for lo, hi, wm in batches[:3]:
            dyn.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi], gaps=np.full(hi - lo, G, np.int64))
            ses.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi])
            dyn.advance_watermark(wm)
            ses.advance_watermark(wm)
        a, b = dyn.snapshot_state(), ses.snapshot_state()
        assert len(a) > 20_000 and a[96:] == b[96:]
        # the header: the dynamic assigner, gap 0; everything else as the constant-gap blob's
        import struct
        fa, fb = (struct.unpack_from("<4sIii5q4i3q", x, 0) for x in (a, b))
        assert fa[3] == N.ASSIGNERS["session_dynamic"] and fb[3] == N.ASSIGNERS["session"]
        assert fa[7] == 0 and fb[7] == G
        assert fa[:3] + fa[8:] == fb[:3] + fb[8:]
        # a blob of the one session assigner is not state of the other
        for op, blob in ((ses, a), (dyn, b)):
            fresh = gpu_operator(dict(assigner="session", gap=G, agg="sum_i64", lateness=late)) if op is ses \
                else dyn_operator("sum_i64", late)
            try:
                with pytest.raises(N.GpuWinError) as ei:
                    fresh.initialize_state(blob)
                assert ei.value.code == N.GW_E_INVALID and "snapshot of a different window" in str(ei.value)
            finally:
                fresh.close()
    finally:
        dyn.close()
        ses.close()


def _key_groups(keys, maxp=128):
    L = N.lib()
    u = np.unique(keys)
    kg = {int(k): L.gw_key_group_for_hash(L.gw_java_long_hash(int(k)), maxp) for k in u}
    return np.array([kg[int(k)] for k in keys], np.int32)


@pytest.mark.parametrize("split", [False, True], ids=["one_handle", "two_key_group_slices"])
def test_snapshot_restore_continues_as_the_reference(split):
    keys, ts, vals, batches = s1()
    gaps = s1_gaps()
    late = 20_000
    ref = R.DynamicSessionOperator("sum_i64", late)
    op = dyn_operator("sum_i64", late, capacity_hint=1024)
    for lo, hi, wm in batches[:3]:
        ref.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi], gaps[lo:hi])
        ref.process_watermark(wm)
        op.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi], gaps=gaps[lo:hi])
        op.advance_watermark(wm)
    op.drain()
    ref.drain()
    blob = op.snapshot_state()
    op.close()
    live = sorted(k for k, m in ref.sets.items() if m)
    assert len(live) > 100 and N.snapshot_keys(blob).tolist() == live  # gw_snapshot_keys on a dynamic blob
    late0, merges0 = ref.late_dropped, ref.merges
    ref.restore()
    if split:  # per-key-group slices of the blob, the lower key groups into one handle, the rest into another
        ops = [dyn_operator("sum_i64", late, capacity_hint=1024) for _ in range(2)]
        for kg in range(128):
            ops[kg >= 64].initialize_state(N.snapshot_slice(blob, kg))
        owner = (_key_groups(keys) >= 64).astype(np.int64)
    else:
        ops = [dyn_operator("sum_i64", late, capacity_hint=1024)]
        ops[0].initialize_state(blob)
        owner = np.zeros(len(keys), np.int64)
    gout, rout = [], []
    try:
        for lo, hi, wm in batches[3:] + [(0, 0, W.LONG_MAX)]:
            rows = []
            for i, o in enumerate(ops):
                m = owner[lo:hi] == i
                if m.any():
                    o.process_batch(keys[lo:hi][m], ts[lo:hi][m], vals[lo:hi][m], gaps=gaps[lo:hi][m])
                o.advance_watermark(wm)
                k, s, e, r = o.drain()
                rows.append((k, s, e, r.view(np.int64)))
            gout.append(tuple(np.concatenate([x[c] for x in rows]) for c in range(4)))
            if hi > lo:
                ref.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi], gaps[lo:hi])
            ref.process_watermark(wm)
            rout.append(ref.drain())
        assert compare(gout, rout, False) == []
        assert sum(len(x[0]) for x in rout) > 1000
        assert sum(o.num_late_records_dropped for o in ops) == ref.late_dropped - late0
        assert sum(o.stats()["session_merges"] for o in ops) == ref.merges - merges0
    finally:
        for o in ops:
            o.close()


def test_key_remap_on_a_dynamic_blob():
    op = dyn_operator("count")
    fresh = dyn_operator("count")
    try:
        k = np.array([3, 9, 3, 5], np.int64)
        op.process_batch(k, np.array([0, 0, 4, 7], np.int64), k, gaps=np.array([10, 2, 1, 100], np.int64))
        blob = op.snapshot_state()
        assert N.snapshot_keys(blob).tolist() == [3, 5, 9]
        moved = N.snapshot_remap_keys(blob, {3: 1003, 9: 1009})
        assert N.snapshot_keys(moved).tolist() == [5, 1003, 1009]
        fresh.initialize_state(moved)
        fresh.advance_watermark(W.LONG_MAX)
        kk, s, e, r = fresh.drain()
        assert sorted(zip(kk.tolist(), s.tolist(), e.tolist(), r.tolist())) == [(5, 7, 107, 1), (1003, 0, 10, 2),
                                                                                (1009, 0, 2, 1)]
    finally:
        op.close()
        fresh.close()
