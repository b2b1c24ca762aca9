"""gw_valve (include/gpuwin.h; host code, no device) against the vectors that pin
StatusWatermarkValve's behaviour and against tests/valve_reference.py over seeded random
sequences of watermarks, idle and active statuses."""
import ctypes

import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import windowing as W
from tests.valve_reference import ACTIVE, IDLE, LONG_MIN, ReferenceValve

S_IDLE, S_ACTIVE = ("S", IDLE), ("S", ACTIVE)


def Wm(c, t, *out):
    return ("W", c, t, [("W", o) for o in out])


def I(c, *out):  # noqa: E743
    return ("I", c, None, list(out))


def A(c, *out):
    return ("A", c, None, list(out))


VECTORS = {
    "V1": (3, [Wm(0, 10), Wm(1, 5), Wm(2, 7, 5), Wm(1, 20, 7), Wm(2, 8, 8), Wm(2, 6), Wm(0, 9)]),
    "V2": (3, [Wm(0, 10), Wm(1, 5), I(2, ("W", 5)), I(1, ("W", 10)), I(0, S_IDLE), Wm(0, 50), A(1, S_ACTIVE),
               Wm(1, 8), Wm(1, 12, 12)]),
    "V3": (2, [Wm(0, 10), Wm(1, 20, 10), I(1), I(0, ("W", 20), S_IDLE)]),
    "V3b": (2, [Wm(0, 10), Wm(1, 20, 10), I(0, ("W", 20)), I(1, S_IDLE)]),
    "V4": (2, [Wm(0, 10), Wm(1, 10, 10), I(1), Wm(0, 30, 30), A(1), Wm(0, 40, 40), Wm(1, 35), Wm(1, 45),
               Wm(0, 50, 45)]),
    "one-channel": (1, [Wm(0, 3, 3), Wm(0, 3), Wm(0, 2), Wm(0, 9, 9), Wm(0, LONG_MIN), Wm(0, 10, 10)]),
}


class NativeValve:
    """gw_valve through the C ABI, emissions in valve_reference's form."""

    def __init__(self, n):
        self.v = ctypes.c_void_p()
        N.check(N.lib().gw_valve_create(n, ctypes.byref(self.v)))

    def event(self, c, kind, value):
        o = N.GwValveOutput()
        N.check(N.lib().gw_valve_input(self.v, c, kind, value, ctypes.byref(o)))
        out = [("W", o.watermark)] if o.has_watermark else []
        return out + ([("S", o.status)] if o.has_status else [])

    def close(self):
        N.lib().gw_valve_destroy(self.v)


def feed(valve, step):
    what, c, t, _ = step
    if what == "W":
        return valve.event(c, N.EVENT_WATERMARK, t)
    return valve.event(c, N.EVENT_STATUS, IDLE if what == "I" else ACTIVE)


@pytest.mark.parametrize("name", sorted(VECTORS))
def test_vectors(name):
    n, steps = VECTORS[name]
    nat, ref = NativeValve(n), ReferenceValve(n)
    for i, step in enumerate(steps):
        assert feed(nat, step) == step[3], (name, i, step)
        assert feed(ref, step) == step[3], (name, i, step)
    nat.close()


def random_inputs(rng, n, count):
    """W / I / A over n channels: watermarks mostly advance a slowly growing clock with jitter (so
    some do not advance their channel and some jump ahead), statuses flip often enough that all
    channels are idle now and then: the mix changes every 250 inputs between mostly watermarks,
    mostly idle and mostly active."""
    clock, out = 0, []
    mixes = [(0.70, 0.87), (0.15, 0.95), (0.30, 0.35)]  # P(watermark), P(watermark or idle)
    for i in range(count):
        p_wm, p_idle = mixes[(i // 250) % 3]
        c = int(rng.integers(0, n))
        u = rng.random()
        if u < p_wm:
            clock += int(rng.integers(0, 4))
            out.append((c, N.EVENT_WATERMARK, clock + int(rng.integers(-6, 7))))
        elif u < p_idle:
            out.append((c, N.EVENT_STATUS, IDLE))
        else:
            out.append((c, N.EVENT_STATUS, ACTIVE))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 17])
def test_random_sequences_match_the_reference(n):
    rng = np.random.default_rng(100 + n)
    nat, ref = NativeValve(n), ReferenceValve(n)
    emitted = {"W": 0, ("S", IDLE): 0, ("S", ACTIVE): 0, "both": 0}
    for i, (c, kind, value) in enumerate(random_inputs(rng, n, 4000)):
        got, exp = nat.event(c, kind, value), ref.event(c, kind, value)
        assert got == exp, (n, i, c, kind, value)
        for e in got:
            emitted["W" if e[0] == "W" else e] += 1
        emitted["both"] += len(got) == 2
    nat.close()
    # the sequences reach every kind of emission (n = 1: a lone channel's idle never flushes)
    assert emitted["W"] > 100 and emitted[("S", IDLE)] > 0 and emitted[("S", ACTIVE)] > 0
    assert n == 1 or emitted["both"] > 0


def test_extreme_watermarks():
    nat, ref = NativeValve(2), ReferenceValve(2)
    top = (1 << 63) - 1
    for c, t in [(0, LONG_MIN), (0, LONG_MIN + 1), (1, top), (0, top), (1, top)]:
        assert nat.event(c, N.EVENT_WATERMARK, t) == ref.event(c, N.EVENT_WATERMARK, t)
    assert ref.last_wm == top
    nat.close()


def test_argument_errors():
    L = N.lib()
    v = ctypes.c_void_p()
    for n in (0, -1, N.MAX_INPUT_CHANNELS + 1):
        assert L.gw_valve_create(n, ctypes.byref(v)) == N.GW_E_INVALID
    assert L.gw_valve_create(N.MAX_INPUT_CHANNELS, ctypes.byref(v)) == 0
    o = N.GwValveOutput()
    assert L.gw_valve_input(v, N.MAX_INPUT_CHANNELS, N.EVENT_WATERMARK, 1, ctypes.byref(o)) == N.GW_E_INVALID
    assert L.gw_valve_input(v, -1, N.EVENT_WATERMARK, 1, ctypes.byref(o)) == N.GW_E_INVALID
    assert L.gw_valve_input(v, 0, 2, 1, ctypes.byref(o)) == N.GW_E_INVALID
    for bad in (1, -2, 1 << 32):  # a status is 0 or -1 as written; nothing is truncated to fit
        assert L.gw_valve_input(v, 0, N.EVENT_STATUS, bad, ctypes.byref(o)) == N.GW_E_INVALID
    assert L.gw_valve_input(v, 0, N.EVENT_STATUS, IDLE, ctypes.byref(o)) == 0
    L.gw_valve_destroy(v)


def test_python_wrapper():
    v = W.StatusWatermarkValve(2)
    assert v.input_watermark(0, 10) == []
    assert v.input_watermark(1, 20) == [("watermark", 10)]
    assert v.input_status(1, True) == []
    assert v.input_status(0, True) == [("watermark", 20), ("status", True)]
    assert v.input_status(0, False) == [("status", False)]
    v.close()
    with pytest.raises(ValueError):
        W.StatusWatermarkValve(0)
