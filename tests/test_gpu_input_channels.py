"""An operator that reads several input channels (gw_set_input_channels, gw_ingest_channels*):
one segmented decode per call, the handle's valve on the host, the records between two emitted
watermarks as one batch.

The reference is the CPU oracle operator driven by the Python valve (tests/valve_reference.py):
every range decoded by itself (tests/netbuf_channels.py reference), its events fed to the valve
in order, its records to the oracle, the oracle advanced at every watermark the valve emits.
All rows bit-exact (as multisets), late_dropped equal."""
import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import netbuf as NB
from flink_amd import windowing as W
from tests.gpu_helpers import compare, gpu_operator, random_stream
from tests.netbuf_channels import reference
from tests.valve_reference import ReferenceValve

pytestmark = pytest.mark.gpu

LAY = ("JJ", 0, 1)
IDLE, ACTIVE = NB.stream_status(False), NB.stream_status(True)


class Reference:
    """The oracle operator behind a ReferenceValve, fed the same calls as the GPU operator."""

    def __init__(self, oracle_lib, kw, n, layout=LAY):
        self.op = oracle_lib.OracleOperator(oracle_lib.make_config(**kw))
        self.valve, self.layout, self.carry = ReferenceValve(n), layout, {}
        self.emitted = []

    def call(self, parts):
        """parts: [(channel, bytes)]; each channel's unconsumed tail waits for its next bytes."""
        data = [(c, self.carry.get(c, b"") + bytes(d)) for c, d in parts]
        ref = reference([d for _, d in data], *self.layout)
        assert ref.code == 0
        vb = ref.val
        done, first = 0, 0
        for (c, d), used, ne in zip(data, ref.consumed, ref.ev_count):
            self.carry[c] = d[used:]
            for i in range(first, first + ne):
                for what, x in self.valve.event(c, int(ref.ev_kind[i]), int(ref.ev_val[i])):
                    self.emitted.append((what, x))
                    if what != "W":
                        continue
                    p = int(ref.ev_pos[i])
                    if p > done:
                        self.op.process_batch(ref.key[done:p], ref.ts[done:p], vb[done:p])
                        done = p
                    self.op.process_watermark(x)
            first += ne
        if len(ref.key) > done:
            self.op.process_batch(ref.key[done:], ref.ts[done:], vb[done:])

    def finish(self):
        self.op.process_watermark(W.LONG_MAX)
        return self.op.drain(), self.op.late_dropped


def finish_gpu(op):
    op.advance_watermark(W.LONG_MAX)
    k, s, e, r = op.drain()
    return (k, s, e, r.view(np.int64)), op.num_late_records_dropped


def channel_streams(kw, n_channels, seed, n=6000, nb=10, n_keys=60, statuses=False):
    """A seeded keyed stream dealt to the channels record by record; every channel serializes its
    share batch by batch, a watermark behind each batch (its own bounded-out-of-orderness one)."""
    keys, ts, vals, batches = random_stream(seed, n, n_keys, nb, ts_step=3, disorder=150, wm_lag=150,
                                            agg="sum_i64")
    rng = np.random.default_rng(seed + 1)
    owner = rng.integers(0, n_channels, n)
    out = []
    for c in range(n_channels):
        parts = []
        for b, (lo, hi, _) in enumerate(batches):
            m = np.nonzero(owner[lo:hi] == c)[0] + lo
            if len(m):
                parts.append(NB.serialize_batches("JJ", 0, 1, [(keys[m], ts[m], vals[m])],
                                                  [int(ts[m].max()) - 151 - 7 * c]))
            if statuses and (b + c) % 4 == 1:
                parts.append(IDLE if (b // 4) % 2 == 0 else ACTIVE)
        out.append(b"".join(parts))
    return out


def polls(streams, bufsize):
    """Call i holds buffer i of every channel that still has one, channels in a rotating order."""
    bufs = [NB.split_buffers(s, bufsize) for s in streams]
    calls = []
    for i in range(max(len(b) for b in bufs)):
        order = [(c + i) % len(bufs) for c in range(len(bufs))]
        calls.append([(c, bufs[c][i]) for c in order if i < len(bufs[c])])
    return calls


def run_both(oracle_lib, kw, n_channels, calls, device=False):
    import torch
    ref = Reference(oracle_lib, kw, n_channels)
    op = gpu_operator(kw)
    lay = N.record_layout(*LAY)
    try:
        op.set_input_channels(n_channels)
        fired, carry = 0, {}
        for parts in calls:
            ref.call(parts)
            if not device:
                fired += op.process_channel_buffers(parts, lay)
                continue
            data = [(c, carry.get(c, b"") + bytes(d)) for c, d in parts]
            tensors = [(c, torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() if d
                        else torch.empty(0, dtype=torch.uint8, device="cuda")) for c, d in data]
            used, f = op.process_channels_device(tensors, lay)
            fired += f
            for (c, d), u in zip(data, used):
                carry[c] = d[u:]
        status = op.input_status()
        got, late = finish_gpu(op)
    finally:
        op.close()
    exp, exp_late = ref.finish()
    assert compare([got], [exp], kw["agg"] in N.DOUBLE_RESULT) == []
    assert late == exp_late
    return ref, status, fired, len(exp[0])


CONFIGS = {
    "tumbling-sum": dict(assigner="tumbling", size=500, agg="sum_i64"),
    "sliding-count": dict(assigner="sliding", size=900, slide=300, offset=-50, agg="count"),
    "session-sum": dict(assigner="session", gap=40, agg="sum_i64"),
}


@pytest.mark.parametrize("n_channels", [2, 3, 8])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_channels_match_the_oracle_behind_the_reference_valve(oracle_lib, name, n_channels):
    kw = CONFIGS[name]
    streams = channel_streams(kw, n_channels, seed=50 + n_channels, statuses=(n_channels == 3))
    calls = polls(streams, 4093)  # records span the buffers: every channel carries a tail
    assert len(calls) >= 4
    ref, status, fired, rows = run_both(oracle_lib, kw, n_channels, calls, device=(n_channels == 8))
    wms = [x for what, x in ref.emitted if what == "W"]
    assert len(wms) >= 5 and fired > 0 and rows > 0
    assert status == (ref.valve.last_wm, ref.valve.last_status != 0)


def test_a_watermark_in_the_middle_of_a_call_fires_and_makes_later_records_late(oracle_lib):
    """Channel 0: records, W(100).  Channel 1: a record at 50 (on time), W(100) -- the valve emits
    100 and the window [0, 100) fires -- then a record at 60: late, dropped."""
    kw = dict(assigner="tumbling", size=100, agg="sum_i64")
    R = lambda k, t, v: NB.record((k, v), "JJ", t)  # noqa: E731
    c0 = R(1, 10, 5) + R(2, 20, 7) + NB.watermark(100)
    c1 = R(1, 50, 100) + NB.watermark(100) + R(1, 60, 1000) + R(2, 150, 1)
    ref = Reference(oracle_lib, kw, 2)
    ref.call([(0, c0), (1, c1)])
    op = gpu_operator(kw)
    try:
        op.set_input_channels(2)
        used, fired = op.process_channels([(0, c0), (1, c1)], N.record_layout(*LAY))
        assert used == [len(c0), len(c1)] and fired == 2
        assert op.input_status() == (100, False)
        k, s, e, r = op.drain()
        assert sorted(zip(k.tolist(), s.tolist(), e.tolist(), r.view(np.int64).tolist())) == [(1, 0, 100, 105),
                                                                                             (2, 0, 100, 7)]
        assert op.num_late_records_dropped == 1
        got, late = finish_gpu(op)
    finally:
        op.close()
    exp, exp_late = ref.finish()
    assert late == exp_late == 1
    assert sorted(zip(*[x.tolist() for x in got])) == [(2, 100, 200, 1)]
    assert sorted(zip(*[x.tolist() for x in exp])) == [(1, 0, 100, 105), (2, 0, 100, 7), (2, 100, 200, 1)]


def test_idle_channels_do_not_hold_the_watermark_back(oracle_lib):
    """Channel 2 is idle from the start: channels 0 and 1 drive the watermark.  It returns (its
    records count, its old watermark does not until it has caught up).  At the end every channel
    goes idle: the valve flushes the maximum and reports idle."""
    kw = dict(assigner="tumbling", size=200, agg="sum_i64")
    streams = channel_streams(kw, 3, seed=77, n=3000, nb=8)
    half = [NB.split_buffers(s, len(s) // 2 + 1) for s in streams]
    # (the cut falls inside an element: the tail is carried)
    calls = [[(2, IDLE), (0, half[0][0]), (1, half[1][0])],
             [(1, half[1][1]), (2, ACTIVE + half[2][0]), (0, half[0][1])],
             [(2, half[2][1])],
             [(0, IDLE), (2, IDLE), (1, NB.watermark(1 << 40) + IDLE)]]
    ref = Reference(oracle_lib, kw, 3)
    op = gpu_operator(kw)
    lay = N.record_layout(*LAY)
    try:
        op.set_input_channels(3)
        seen = []
        for parts in calls:
            ref.call(parts)
            op.process_channel_buffers(parts, lay)
            seen.append(op.input_status())
            assert seen[-1] == (ref.valve.last_wm, ref.valve.last_status != 0)
        assert op.channel_tails() == {}
        got, late = finish_gpu(op)
    finally:
        op.close()
    exp, exp_late = ref.finish()
    assert seen[0][0] > W.LONG_MIN and not seen[0][1]  # the two active channels drove it
    assert seen[-1] == (1 << 40, True)                 # max flush, then idle
    assert ("S", -1) in ref.emitted
    assert compare([got], [exp], False) == [] and late == exp_late


def test_window_class_composite_decodes_once_at_the_parent(oracle_lib):
    kw = dict(assigner="sliding", size=1000, slide=10, agg="sum_i64")  # 100 panes: two window classes
    streams = channel_streams(kw, 3, seed=91, n=2500, nb=6, n_keys=12)
    ref, status, fired, rows = run_both(oracle_lib, kw, 3, polls(streams, 16384))
    assert fired > 0 and rows > 1000


def test_two_stage_loop_with_the_row_encoder(oracle_lib):
    """Two upstream operators (parallelism 2) each write their fired rows as one byte range per
    downstream channel (gw_rows_serialized_device, channels = 2, the watermark behind the rows);
    downstream operator j ingests range j of both upstream buffers, on the device, and equals
    the oracle fed the same rows."""
    import torch
    up_kw = dict(assigner="tumbling", size=100, agg="count")
    down_kw = dict(assigner="tumbling", size=1000, agg="sum_i64")
    keys, ts, vals, batches = random_stream(3, 8000, 300, 8, ts_step=1, disorder=30, wm_lag=30)
    owner = np.asarray([W.compute_operator_index_for_key_group(128, 2, W.assign_to_key_group(int(k), 128))
                        for k in range(300)])[keys]
    rows = N.row_layout("JJ", (N.GW_ROW_KEY, N.GW_ROW_RESULT))
    lay = N.record_layout("JJ", 0, 1)
    mk = lambda kw, i: W.GpuWindowOperator(W.TumblingEventTimeWindows.of(kw["size"]), kw["agg"], capacity_hint=1024,  # noqa: E731
                                           max_parallelism=128, parallelism=2, operator_index=i).open()
    ups, downs = [mk(up_kw, i) for i in range(2)], [mk(down_kw, j) for j in range(2)]
    refs = [Reference(oracle_lib, down_kw, 2) for _ in range(2)]
    try:
        for d in downs:
            d.set_input_channels(2)
        for lo, hi, wm in batches:
            bufs = []
            for i, u in enumerate(ups):
                m = np.nonzero(owner[lo:hi] == i)[0] + lo
                u.process_batch(keys[m], ts[m], vals[m])
                u.advance_watermark(wm - 13 * i)
                bufs.append(u.rows_serialized_device(rows, channels=2, max_parallelism=128, watermark=wm - 13 * i))
                u.clear_rows()
            for j, d in enumerate(downs):
                parts = [(i, bufs[i][0][bufs[i][1][j][0]:bufs[i][1][j][0] + bufs[i][1][j][1]]) for i in range(2)]
                used, _ = d.process_channels_device(parts, lay)
                assert used == [p.numel() for _, p in parts]
                refs[j].call([(i, p.cpu().numpy().tobytes()) for i, p in parts])
        torch.cuda.synchronize()
        total = 0
        for j, d in enumerate(downs):
            got, late = finish_gpu(d)
            exp, exp_late = refs[j].finish()
            assert compare([got], [exp], False) == [] and late == exp_late
            total += len(exp[0])
        assert total > 300
    finally:
        for o in ups + downs:
            o.close()


def test_argument_errors(oracle_lib):
    import torch
    lay = N.record_layout(*LAY)
    rec = NB.record((1, 2), "JJ", 3)
    op = gpu_operator(dict(assigner="tumbling", size=100, agg="sum_i64"))
    try:
        with pytest.raises(N.GpuWinError) as e:  # no channels set yet
            op.process_channels([(0, rec)], lay)
        assert e.value.code == N.GW_E_STATE
        for n in (0, N.MAX_INPUT_CHANNELS + 1):
            with pytest.raises(N.GpuWinError) as e:
                op.set_input_channels(n)
            assert e.value.code == N.GW_E_INVALID
        op.set_input_channels(3)
        for parts in ([(1, rec), (1, rec)], [(3, rec)], [(-1, rec)]):  # twice in a call; outside [0, n)
            with pytest.raises(N.GpuWinError) as e:
                op.process_channels(parts, lay)
            assert e.value.code == N.GW_E_INVALID
        dev = torch.zeros(32, dtype=torch.uint8, device="cuda")
        for call in (lambda: op.process_serialized(rec, lay), lambda: op.process_serialized_device(dev, lay)):
            with pytest.raises(N.GpuWinError) as e:  # the single-channel valve would bypass this one
                call()
            assert e.value.code == N.GW_E_INVALID
        # none of these failed the operator or reached its state
        assert op.process_channels([(2, rec), (0, b"")], lay) == ([len(rec), 0], 0)
        # a status that is neither 0 nor -1: the stream is corrupt, the task fails
        bad = rec + b"\0\0\0\5\4" + (3).to_bytes(4, "big")
        with pytest.raises(N.GpuWinError) as e:
            op.process_channels([(1, bad)], lay)
        assert e.value.code == N.GW_E_INVALID
        with pytest.raises(N.GpuWinError):  # the operator has failed
            op.advance_watermark(1000)
    finally:
        op.close()
    # a corrupt range fails the operator and the message names the range
    op = gpu_operator(dict(assigner="tumbling", size=100, agg="sum_i64"))
    try:
        op.set_input_channels(2)
        with pytest.raises(N.GpuWinError) as e:
            op.process_channels([(1, rec), (0, rec + b"\0\0\0\x09\x09" + b"\0" * 8)], lay)
        assert e.value.code == N.GW_E_INVALID and "range 1" in str(e.value)
    finally:
        op.close()
    first = W.GpuWindowOperator(W.TumblingEventTimeWindows.of(100), "sum_i64", flags=N.FLAG_FIRST_ELEMENT).open()
    dyn = W.GpuWindowOperator(W.DynamicEventTimeSessionWindows.with_dynamic_gap(lambda r: 10), "sum_i64").open()
    try:
        for o in (first, dyn):
            with pytest.raises(N.GpuWinError) as e:
                o.set_input_channels(2)
            assert e.value.code == N.GW_E_UNSUPPORTED
            with pytest.raises(N.GpuWinError) as e:
                o.process_channels([(0, rec)], lay)
            assert e.value.code == N.GW_E_UNSUPPORTED
    finally:
        first.close()
        dyn.close()


def test_restore_resets_the_valve(oracle_lib):
    """The valve is not part of the state: after gw_restore every channel is back at
    Long.MIN_VALUE, so a watermark another channel sent before the restore no longer counts."""
    kw = dict(assigner="tumbling", size=100, agg="sum_i64")
    lay = N.record_layout(*LAY)
    a, b = gpu_operator(kw), gpu_operator(kw)
    try:
        a.process_batch(np.asarray([1]), np.asarray([150]), np.asarray([2]))
        blob = a.snapshot_state()
        b.set_input_channels(2)
        b.process_channels([(0, NB.watermark(50))], lay)
        assert b.input_status() == (W.LONG_MIN, False)
        b.initialize_state([blob])
        b.process_channels([(1, NB.watermark(300))], lay)
        assert b.input_status() == (W.LONG_MIN, False)  # channel 0's 50 is forgotten
        b.process_channels([(0, NB.watermark(250))], lay)
        assert b.input_status() == (250, False)
        k, s, e, r = b.drain()
        assert list(zip(k.tolist(), s.tolist(), r.view(np.int64).tolist())) == [(1, 100, 2)]
    finally:
        a.close()
        b.close()
