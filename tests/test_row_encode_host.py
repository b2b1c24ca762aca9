"""Fired rows as network-buffer bytes, host side (gw_row_encoded_bytes, gw_encode_rows_host):
the layout rules, the bytes against the sender-side writer (flink_amd/netbuf.py) element by
element, the reference's own serializer bytes (tests/golden/serializer/), the channel of every
row against the Python restatement of KeyGroupRangeAssignment, and the oracle's sequential decoder
reading the stream back."""
import ctypes
import os

import numpy as np
import pytest

from tests import row_encode_cases as C
from flink_amd import _native as N
from flink_amd import netbuf as NB


@pytest.fixture(scope="module")
def lib():
    return N.lib()


def test_encoded_bytes(lib):
    for name, (types, sources, nbytes) in C.LAYOUTS.items():
        assert lib.gw_row_encoded_bytes(ctypes.byref(C.layout(name))) == nbytes == 13 + sum(4 if t == "I" else 8 for t in types)
    assert lib.gw_row_encoded_bytes(None) == N.GW_E_INVALID


def bad_layouts():
    yield "no fields", N.row_layout("", ())
    nine = N.row_layout("J" * 8, (C.K,) * 8)
    nine.nfields = 9
    yield "nine fields", nine
    neg = N.row_layout("J", (C.K,))
    neg.nfields = -1
    yield "negative field count", neg
    yield "unknown source", N.row_layout("J", (5,))
    yield "negative source", N.row_layout("J", (-1,))
    for t in "FSBZjx":
        yield f"type {t}", N.row_layout("J" + t, (C.K, C.R))
    for s in (C.K, C.S, C.E, C.P):
        yield f"double from source {s}", N.row_layout("D", (s,))


@pytest.mark.parametrize("what,lay", list(bad_layouts()), ids=[w for w, _ in bad_layouts()])
def test_layout_rejections(lib, what, lay):
    assert lib.gw_row_encoded_bytes(ctypes.byref(lay)) == N.GW_E_INVALID
    rc, buf, off, nb = C.call_host(C.rows(3), lay)
    assert rc == N.GW_E_INVALID and lib.gw_last_error(None)
    assert (buf == 0xFF).all()


def test_payload_needs_its_column(lib):
    cols = C.rows(3)
    assert C.call_host(cols, C.layout("JJI"), payload=False)[0] == N.GW_E_INVALID
    assert C.call_host(cols, C.layout("JJI"), payload=True)[0] == N.GW_OK
    assert C.call_host(cols, C.layout("JJ"), payload=False)[0] == N.GW_OK


def test_argument_rejections(lib):
    cols, lay = C.rows(3), C.layout("JJ")
    assert C.call_host(cols, lay, channels=0)[0] == N.GW_E_INVALID
    assert C.call_host(cols, lay, channels=129, max_parallelism=4096)[0] == N.GW_E_UNSUPPORTED
    assert C.call_host(cols, lay, channels=16, max_parallelism=8)[0] == N.GW_E_INVALID
    assert C.call_host(cols, lay, mode=2)[0] == N.GW_E_INVALID


@pytest.mark.parametrize("wm", [None, 123456789012, C.I64_MAX, -1])
@pytest.mark.parametrize("name", list(C.LAYOUTS))
def test_bytes_match_the_writer(lib, name, wm):
    cols = C.rows(67, seed=len(name), int_keys=name == "I")
    rc, buf, off, nb = C.call_host(cols, C.layout(name), watermark=wm)
    assert rc == N.GW_OK
    assert off[0] == 0 and nb[0] == 67 * C.LAYOUTS[name][2] + (0 if wm is None else 13)
    assert C.slices(buf, off, nb) == C.reference(cols, name, watermark=wm)
    assert (buf[nb[0]:] == 0xFF).all()


def test_global_window_timestamp(lib):
    cols = C.rows(9)
    rc, buf, off, nb = C.call_host(cols, C.layout("JJ"), mode=N.ENCODE_GLOBAL_WINDOW, watermark=5)
    assert rc == N.GW_OK and C.slices(buf, off, nb) == C.reference(cols, "JJ", watermark=5, global_window=True)


def test_no_rows(lib):
    z = [np.empty(0, np.int64)] * 5
    rc, buf, off, nb = C.call_host(z, C.layout("JJ"), channels=3)
    assert rc == N.GW_OK and nb.tolist() == [0, 0, 0] and (buf == 0xFF).all()
    rc, buf, off, nb = C.call_host(z, C.layout("JJ"), channels=3, watermark=77)
    assert rc == N.GW_OK and C.slices(buf, off, nb) == [NB.watermark(77)] * 3
    assert off.tolist() == [0, 16, 32]


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("value", [C.I32_MAX + 1, C.I32_MIN - 1, C.I64_MIN, 1 << 32])
def test_int_field_out_of_range(lib, where, value):
    cols = [c.copy() for c in C.rows(41)]
    i = {"first": 0, "middle": 20, "last": 40}[where]
    assert C.call_host(cols, C.layout("JJI"))[0] == N.GW_OK
    cols[C.P][i] = value
    for channels in (1, 3):
        rc = C.call_host(cols, C.layout("JJI"), channels=channels)[0]
        assert rc == N.GW_E_RANGE and b"Java int" in lib.gw_last_error(None)


def key_patterns(channels, max_parallelism):
    """(name, keys): every channel empty but one; one row per channel; random keys."""
    by_channel = {}
    k = 0
    while len(by_channel) < channels:
        by_channel.setdefault(C.channel_of(k, max_parallelism, channels), []).append(k)
        k += 1
    target = channels // 2
    yield "one channel", np.array((by_channel[target] * 40)[:37], np.int64)
    yield "one row per channel", np.array([by_channel[c][0] for c in reversed(range(channels))], np.int64)
    yield "random", np.random.default_rng(channels).integers(C.I64_MIN, C.I64_MAX, 500, dtype=np.int64)


@pytest.mark.parametrize("max_parallelism", [128, 4096])
@pytest.mark.parametrize("channels", [1, 2, 3, 16, 128])
def test_channels(lib, channels, max_parallelism):
    for what, keys in key_patterns(channels, max_parallelism):
        cols = list(C.rows(len(keys), seed=3))
        cols[C.K] = keys
        for wm in (None, 42):
            rc, buf, off, nb = C.call_host(cols, C.layout("JJ"), channels=channels,
                                           max_parallelism=max_parallelism, watermark=wm)
            assert rc == N.GW_OK, what
            C.check_ranges(off, nb, len(buf) - 64)
            exp = C.reference(cols, "JJ", channels, max_parallelism, wm)
            assert C.slices(buf, off, nb) == exp, what
            for c in range(channels):  # the C restatement of the same assignment
                own = [k for k in keys.tolist() if lib.gw_operator_for_key_group(
                    max_parallelism, channels, lib.gw_key_group_for_hash(lib.gw_java_long_hash(k), max_parallelism)) == c]
                assert nb[c] == 29 * len(own) + (0 if wm is None else 13)


@pytest.mark.parametrize("channels", [1, 3])
def test_output_full_reports_the_size_and_writes_nothing_past_cap(lib, channels):
    cols = C.rows(50, seed=9)
    rc, buf, off, nb = C.call_host(cols, C.layout("JJ"), channels=channels, watermark=1)
    assert rc == N.GW_OK
    need = C.check_ranges(off, nb, len(buf))
    for cap in (0, 1, need // 2, need - 1):
        rc, small, off2, nb2 = C.call_host(cols, C.layout("JJ"), channels=channels, watermark=1, cap=cap)
        assert rc == N.GW_E_OUTPUT_FULL and off2[0] == need
        assert (small[cap:] == 0xFF).all()
    rc, exact, off2, nb2 = C.call_host(cols, C.layout("JJ"), channels=channels, watermark=1, cap=need)
    assert rc == N.GW_OK and (exact[need:] == 0xFF).all()
    assert C.slices(exact, off2, nb2) == C.slices(buf, off, nb)


def test_reference_serializer_bytes(lib):
    """The reference's own bytes (StreamElementSerializerUpgradeTest's tag + timestamp,
    LongSerializer's Long): the row (1234567890) of a window ending at 123457 under "J"."""
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "serializer")
    rec = open(os.path.join(d, "stream-element-serializer.test-data"), "rb").read()
    lng = open(os.path.join(d, "long-serializer.test-data"), "rb").read()
    one = lambda v: np.array([v], np.int64)
    cols = [one(1234567890), one(0), one(123457), one(0), one(0)]
    rc, buf, off, nb = C.call_host(cols, C.layout("J"))
    assert rc == N.GW_OK and nb[0] == 21
    got = buf[:21].tobytes()
    assert got[:4] == (17).to_bytes(4, "big") and got[4:] == rec[:9] + lng


@pytest.mark.parametrize("name,kf,vf", [("JJ", 0, 1), ("JJJD", 0, 3), ("J8", 0, 3), ("J", 0, -1)])
def test_oracle_decoder_reads_it_back(oracle_lib, name, kf, vf):
    cols = C.rows(300, seed=11)
    rc, buf, off, nb = C.call_host(cols, C.layout(name), watermark=991)
    assert rc == N.GW_OK
    rc, k, t, v, wp, wv, res = oracle_lib.decode_stream(buf[:nb[0]].tobytes(), C.LAYOUTS[name][0], kf, vf)
    assert rc == 0 and res.records == 300 and res.consumed == nb[0]
    assert (k == cols[C.K]).all() and (t == cols[C.E] - 1).all()  # (int64 wrap-around, as Java's)
    if vf >= 0:
        assert (np.asarray(v).view(np.int64) == cols[C.R]).all()
    assert list(wp) == [300] and list(wv) == [991]
