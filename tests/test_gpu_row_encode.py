"""Fired rows as network-buffer bytes on the device (gw_encode_rows_device, gw_drain_serialized,
gw_rows_serialized_device): the device encoder against the host encoder byte for byte inside
every reported range (tests/test_row_encode_host.py pins the host encoder to the sender-side
writer and the reference's bytes), the handle calls against netbuf.record over the rows the
handle shows, and two operators chained through device bytes against the oracle."""
import ctypes

import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import netbuf as NB
from flink_amd import windowing as W
from tests import row_encode_cases as C
from tests.gpu_helpers import gpu_operator, random_stream, run_oracle

pytestmark = pytest.mark.gpu

# head / tail handling (n mod 4, n mod 16 bytes), one tile and its neighbours (512 rows), several
# tiles, and channels that end up empty
SIZES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099, 100003]
CHANNELS = [1, 2, 3, 16, 128]
GUARD = 256
_cols = {}


class DeviceColumns(list):
    """The five device tensors of n rows."""
    def __init__(self, n, tensors):
        super().__init__(tensors)
        self.n = n

    def clone(self):
        return DeviceColumns(self.n, [t.clone() for t in self])


def columns(n, int_keys):
    """Host columns and their device copies, made once per size."""
    import torch
    if (n, int_keys) not in _cols:
        host = C.rows(n, seed=n, int_keys=int_keys)
        # (one element when n = 0: an empty tensor has no pointer, and a null payload column means
        # "no payload")
        _cols[(n, int_keys)] = (host, DeviceColumns(n, [torch.from_numpy(np.resize(c, max(n, 1))).cuda() for c in host]))
    return _cols[(n, int_keys)]


def call_device(dev, lay, channels=1, max_parallelism=128, watermark=None, mode=0, cap=0, base=0, payload=True):
    """gw_encode_rows_device into a 0xFF-filled buffer: `base` bytes, cap bytes for the call,
    GUARD bytes behind them.  (rc, the whole buffer as numpy, chan_off, chan_bytes)."""
    import torch
    out = torch.full((base + cap + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    off, nb = np.full(channels, -1, np.int64), np.full(channels, -1, np.int64)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    rc = N.lib().gw_encode_rows_device(dev.n, P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]),
                                       P(dev[4]) if payload else None, ctypes.byref(lay), mode, channels,
                                       max_parallelism, N.NO_WATERMARK if watermark is None else watermark,
                                       ctypes.c_void_p(out.data_ptr() + base), cap, off.ctypes.data, nb.ctypes.data, None)
    return rc, out.cpu().numpy(), off, nb


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("name", list(C.LAYOUTS))
def test_device_matches_host(name, channels):
    lay = C.layout(name)
    for n in SIZES:
        host, dev = columns(n, name == "I")
        for wm in (None, 1234567890123):
            rc, hbuf, hoff, hnb = C.call_host(host, lay, channels=channels, watermark=wm)
            assert rc == N.GW_OK
            need = C.check_ranges(hoff, hnb, len(hbuf))
            for base in (0, 16):
                rc, buf, off, nb = call_device(dev, lay, channels=channels, watermark=wm, cap=need, base=base)
                where = f"n={n} watermark={wm} base={base}"
                assert rc == N.GW_OK, where
                assert off.tolist() == hoff.tolist() and nb.tolist() == hnb.tolist(), where
                assert (buf[:base] == 0xFF).all() and (buf[base + need:] == 0xFF).all(), where
                for c in range(channels):
                    lo = int(off[c])
                    assert np.array_equal(buf[base + lo:base + lo + int(nb[c])], hbuf[lo:lo + int(hnb[c])]), \
                        f"{where} channel {c}"


def test_device_global_window_and_max_parallelism():
    host, dev = columns(4099, False)
    lay = C.layout("JJ")
    for kw in (dict(mode=N.ENCODE_GLOBAL_WINDOW), dict(channels=3, max_parallelism=4096)):
        rc, hbuf, hoff, hnb = C.call_host(host, lay, watermark=7, **kw)
        need = C.check_ranges(hoff, hnb, len(hbuf))
        rc, buf, off, nb = call_device(dev, lay, watermark=7, cap=need, **kw)
        assert rc == N.GW_OK and C.slices(buf, off, nb) == C.slices(hbuf, hoff, hnb)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_device_int_field_out_of_range(where):
    n = 1025
    host, dev = columns(n, False)
    i = {"first": 0, "middle": 600, "last": n - 1}[where]
    bad = dev.clone()
    bad[C.P][i] = C.I32_MAX + 1
    for channels in (1, 3):
        assert call_device(dev, C.layout("JJI"), channels=channels, cap=n * 33 + 64)[0] == N.GW_OK
        rc = call_device(bad, C.layout("JJI"), channels=channels, cap=n * 33 + 64)[0]
        assert rc == N.GW_E_RANGE and b"Java int" in N.lib().gw_last_error(None)


@pytest.mark.parametrize("channels", [1, 3])
def test_device_output_full(channels):
    host, dev = columns(1025, False)
    lay = C.layout("JJ")
    rc, hbuf, hoff, hnb = C.call_host(host, lay, channels=channels, watermark=1)
    need = C.check_ranges(hoff, hnb, len(hbuf))
    for cap in (0, 16, need // 2, need - 1):
        rc, buf, off, nb = call_device(dev, lay, channels=channels, watermark=1, cap=cap)
        assert rc == N.GW_E_OUTPUT_FULL and off[0] == need
        assert (buf == 0xFF).all()


def test_device_rejections():
    host, dev = columns(5, False)
    lay = C.layout("JJ")
    assert call_device(dev, lay, cap=4096, base=8)[0] == N.GW_E_INVALID          # 16-byte alignment
    assert call_device(dev, lay, cap=4096, channels=129, max_parallelism=4096)[0] == N.GW_E_UNSUPPORTED
    assert call_device(dev, C.layout("JJI"), cap=4096, payload=False)[0] == N.GW_E_INVALID
    assert call_device(dev, N.row_layout("D", (C.K,)), cap=4096)[0] == N.GW_E_INVALID


def test_device_round_trip_through_the_decoder():
    """channel 0 of 100003 "JJ" rows back through gw_decode_serialized: key, end - 1, result and
    the watermark behind the last record."""
    import torch
    n = 100003
    host, dev = columns(n, False)
    out = torch.full((n * 29 + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    off, nb = np.zeros(1, np.int64), np.zeros(1, np.int64)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    lay = C.layout("JJ")
    rc = N.lib().gw_encode_rows_device(n, P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), None, ctypes.byref(lay), 0, 1,
                                       128, 555, P(out), out.numel(), off.ctypes.data, nb.ctypes.data, None)
    assert rc == N.GW_OK and off[0] == 0 and nb[0] == n * 29 + 13
    k, t, v = (torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(3))
    wp, wv = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(2))
    res = N.GwDecodeResult()
    rl = N.record_layout("JJ", 0, 1)
    rc = N.lib().gw_decode_serialized(P(out), int(nb[0]), ctypes.byref(rl), P(k), P(t), P(v), n + 1, P(wp), P(wv), 4,
                                      ctypes.byref(res), None)
    assert rc == N.GW_OK and res.records == n and res.watermarks == 1 and res.consumed == nb[0]
    assert np.array_equal(k[:n].cpu().numpy(), host[C.K])
    assert np.array_equal(t[:n].cpu().numpy(), host[C.E] - 1)  # (int64 wrap-around, as Java's)
    assert np.array_equal(v[:n].cpu().numpy(), host[C.R])
    assert wp[:1].tolist() == [n] and wv[:1].tolist() == [555]


# ---- handles ---------------------------------------------------------------------------------
def _d2h(ptr, n):
    """n int64 words at a device pointer -> numpy (hipMemcpy of the runtime torch loaded)."""
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    hip = ctypes.CDLL("libamdhip64.so.7")
    out = np.empty(n, np.int64)
    if n:
        assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(n * 8), 2) == 0
    return out


def pending(op):
    ptrs, n = op.rows_device()
    op.synchronize()
    return [_d2h(p, n) for p in ptrs]


def expected(rows, types, sources, channels, max_parallelism, wm, global_window=False, payload=None):
    import struct
    cols = list(rows) + [payload]
    out = [[] for _ in range(channels)]
    for i in range(len(rows[0])):
        f = [struct.unpack(">d", struct.pack(">q", int(cols[s][i])))[0] if t == "D" else int(cols[s][i])
             for t, s in zip(types, sources)]
        ts = C.I64_MAX if global_window else int(rows[2][i]) - 1
        out[0 if channels == 1 else C.channel_of(rows[0][i], max_parallelism, channels)].append(NB.record(f, types, ts))
    return [b"".join(x) + (b"" if wm is None else NB.watermark(wm)) for x in out]


HANDLES = [
    ("tumbling sum", dict(assigner="tumbling", size=1000, agg="sum_i64"), "JJ", (C.K, C.R)),
    ("window classes", dict(assigner="sliding", size=2000, slide=20, agg="count"), "JJJJ", (C.K, C.S, C.E, C.R)),
    ("session avg", dict(assigner="session", gap=40, agg="avg_f64"), "JJD", (C.K, C.S, C.R)),
    ("count windows", dict(assigner="count_tumbling", size=5, agg="sum_i64"), "JIJ", (C.K, C.E, C.R)),
]


@pytest.mark.parametrize("what,kw,types,sources", HANDLES, ids=[h[0] for h in HANDLES])
def test_drain_serialized(what, kw, types, sources):
    keys, ts, vals, batches = random_stream(seed=3, n=6000, num_keys=40, n_batches=4, ts_step=5, disorder=100,
                                            wm_lag=150, agg=kw["agg"])
    lay = N.row_layout(types, sources)
    glob = kw["assigner"].startswith("count")
    op = gpu_operator(kw)
    total = 0
    try:
        for b, (lo, hi, wm) in enumerate(batches):
            op.process_batch(keys[lo:hi], ts[lo:hi], None if kw["agg"] == "count" else vals[lo:hi])
            op.advance_watermark(wm)
            channels, wm_out = [(1, None), (3, wm), (1, wm), (16, None)][b]
            rows = pending(op)
            got = op.drain_serialized(lay, channels=channels, watermark=wm_out)
            assert got == expected(rows, types, sources, channels, 128, wm_out, glob), f"batch {b}"
            assert op.pending_rows() == 0
            total += len(rows[0])
        assert total > 0
        assert op.drain_serialized(lay, channels=2, watermark=9) == [NB.watermark(9)] * 2  # nothing pending
    finally:
        op.close()


def test_drain_serialized_first_element_payload():
    size = 100
    kw = dict(assigner="tumbling", size=size, agg="sum_i64")
    keys, ts, vals, batches = random_stream(seed=4, n=4000, num_keys=30, n_batches=4, ts_step=3, disorder=50, wm_lag=60)
    payload = keys * 1000003 + ts // size  # one payload per (key, window): whichever element came first
    lay = N.row_layout("JJI", (C.K, C.R, C.P))
    op = gpu_operator(kw, flags=N.FLAG_FIRST_ELEMENT)
    try:
        with pytest.raises(N.GpuWinError):  # GW_ROW_PAYLOAD on a handle without payloads
            plain = gpu_operator(kw)
            try:
                plain.drain_serialized(lay)
            finally:
                plain.close()
        total = 0
        for lo, hi, wm in batches:
            op.process_batch_payload(keys[lo:hi], ts[lo:hi], vals[lo:hi], payload[lo:hi])
            op.advance_watermark(wm)
            rows = pending(op)
            pay = rows[0] * 1000003 + rows[1] // size
            got = op.drain_serialized(lay, channels=2, watermark=wm)
            assert got == expected(rows, "JJI", (C.K, C.R, C.P), 2, 128, wm, payload=pay)
            assert op.pending_rows() == 0
            total += len(rows[0])
        assert total > 0
    finally:
        op.close()


def test_rows_serialized_device_leaves_the_rows():
    kw = dict(assigner="tumbling", size=1000, agg="sum_i64")
    keys, ts, vals, batches = random_stream(seed=5, n=3000, num_keys=40, n_batches=1, ts_step=5)
    lay = N.row_layout("JJ", (C.K, C.R))
    op = gpu_operator(kw)
    try:
        op.process_batch(keys, ts, vals * 10 ** 5)  # sums beyond the Java int range
        op.advance_watermark(batches[0][2])
        rows = pending(op)
        n = len(rows[0])
        assert n > 0 and np.abs(rows[3]).max() > C.I32_MAX
        data, ranges = op.rows_serialized_device(lay, channels=3, watermark=77)
        host = data.cpu().numpy()
        assert [host[o:o + b].tobytes() for o, b in ranges] == expected(rows, "JJ", (C.K, C.R), 3, 128, 77)
        assert op.pending_rows() == n
        # an 'I' field that does not fit: the call fails, the rows and the operator stay
        with pytest.raises(N.GpuWinError) as err:
            op.drain_serialized(N.row_layout("JI", (C.K, C.R)))
        assert err.value.code == N.GW_E_RANGE and op.pending_rows() == n
        k, s, e, r = op.drain()
        assert np.array_equal(k, rows[0]) and np.array_equal(r, rows[3])
    finally:
        op.close()


def test_key_hash_fed_handle():
    kw = dict(assigner="tumbling", size=1000, agg="sum_i64")
    keys, ts, vals, batches = random_stream(seed=6, n=2000, num_keys=20, n_batches=1, ts_step=5)
    hashes = (keys * 31 + 7).astype(np.int32)
    lay = N.row_layout("JJ", (C.K, C.R))
    op = gpu_operator(kw)
    try:
        op.process_batch(keys, ts, vals, key_hashes=hashes)
        op.advance_watermark(batches[0][2])
        rows = pending(op)
        assert len(rows[0]) > 0
        with pytest.raises(N.GpuWinError) as err:
            op.drain_serialized(lay, channels=2)
        assert err.value.code == N.GW_E_UNSUPPORTED and op.pending_rows() == len(rows[0])
        with pytest.raises(N.GpuWinError) as err:
            op.rows_serialized_device(lay, channels=2)
        assert err.value.code == N.GW_E_UNSUPPORTED
        assert op.drain_serialized(lay, channels=1, watermark=3) == expected(rows, "JJ", (C.K, C.R), 1, 128, 3)
        op.process_batch(keys, ts + 100000, vals, key_hashes=hashes)  # the handle still works
        op.advance_watermark(W.LONG_MAX)
        assert op.pending_rows() > 0
    finally:
        op.close()


def test_two_operators_chained_on_the_device(oracle_lib):
    """A (tumbling sum) fires; its rows go as device bytes, watermark appended, into B (tumbling
    max over a 5x longer window, same key); B's rows equal the oracle's B fed the oracle's A rows."""
    kw_a = dict(assigner="tumbling", size=200, agg="sum_i64")
    kw_b = dict(assigner="tumbling", size=1000, agg="max_i64")
    keys, ts, vals, batches = random_stream(seed=8, n=60000, num_keys=3000, n_batches=6, ts_step=1, disorder=100,
                                            wm_lag=120)
    a, b = gpu_operator(kw_a, capacity_hint=4096), gpu_operator(kw_b, capacity_hint=4096)
    lay_out, lay_in = N.row_layout("JJ", (C.K, C.R)), N.record_layout("JJ", 0, 1)
    got = []
    try:
        for lo, hi, wm in batches + [(0, 0, W.LONG_MAX)]:
            if hi > lo:
                a.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi])
            a.advance_watermark(wm)
            data, ((o, nbytes),) = a.rows_serialized_device(lay_out, watermark=wm)
            a.clear_rows()
            consumed, fired = b.process_serialized_device(data[o:o + nbytes], lay_in)
            assert consumed == nbytes
            k, s, e, r = b.drain()
            got.append((k, s, e, r.view(np.int64)))
    finally:
        a.close()
        b.close()
    ora_a, _ = run_oracle(oracle_lib, kw_a, keys, ts, vals, batches)
    ob = oracle_lib.OracleOperator(oracle_lib.make_config(**kw_b))
    exp = []
    for (k, s, e, r), (lo, hi, wm) in zip(ora_a, batches + [(0, 0, W.LONG_MAX)]):
        if len(k):
            ob.process_batch(k, e - 1, r)
        ob.process_watermark(wm)
        exp.append(ob.drain())
    from tests.gpu_helpers import compare
    assert sum(len(x[0]) for x in got) > 3000
    assert compare(got, exp, False) == []
