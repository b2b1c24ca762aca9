"""Shared by the row-encoder tests (test_row_encode_host.py, test_gpu_row_encode.py,
test_jni_row_encode.py): the layouts, row columns with the awkward values in them, and the
reference bytes built element by element with the sender-side writer (flink_amd/netbuf.py)."""
import struct

import numpy as np

from flink_amd import _native as N
from flink_amd import netbuf as NB
from flink_amd import windowing as W

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
NAN_PAYLOAD = 0x7FF8000000000123      # a quiet NaN with payload bits
NAN_NEGATIVE = 0xFFF0000000000001 - (1 << 64)  # a signalling NaN with the sign set
NEG_ZERO = -(1 << 63)                 # the bits of -0.0

K, S, E, R, P = N.GW_ROW_KEY, N.GW_ROW_START, N.GW_ROW_END, N.GW_ROW_RESULT, N.GW_ROW_PAYLOAD
# name -> (types, sources, encoded bytes).  'I' fields read the key (LAYOUTS["I"]) or the payload,
# which rows() keeps inside the Java int range.
LAYOUTS = {
    "I": ("I", (K,), 17),
    "J": ("J", (K,), 21),
    "JJ": ("JJ", (K, R), 29),
    "JJI": ("JJI", (K, R, P), 33),
    "JJJD": ("JJJD", (K, S, E, R), 45),
    "J8": ("JJJJJJJJ", (K, S, E, R, P, K, E, R), 77),
}


def layout(name):
    types, sources, _ = LAYOUTS[name]
    return N.row_layout(types, sources)


def rows(n, seed=0, int_keys=False, key_space=None):
    """Columns (key, start, end, result, payload) of n rows: uniform over all of int64, the first
    rows carrying INT64_MIN / MAX, -1, 0, NaNs with payload bits and -0.0 in every column that may
    hold them; payload (and key when int_keys) inside the Java int range, limits included."""
    rng = np.random.default_rng(seed)
    full = lambda: rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    small = lambda: rng.integers(I32_MIN, I32_MAX, n, dtype=np.int64, endpoint=True)
    key = small() if int_keys else full()
    if key_space is not None:
        key = rng.integers(0, key_space, n).astype(np.int64)
    start, end, result, payload = full(), full(), full(), small()
    special = [I64_MIN, I64_MAX, -1, 0, NAN_PAYLOAD, NAN_NEGATIVE, NEG_ZERO]
    for i, v in enumerate(special[:n]):
        result[i] = v
        end[(i + 1) % n] = v          # end = INT64_MIN: the timestamp end - 1 wraps like Java's
        start[(i + 2) % n] = v
        if not int_keys and key_space is None:
            key[(i + 3) % n] = v
    for i, v in enumerate([I32_MIN, I32_MAX, -1, 0][:n]):
        payload[(i + 4) % n] = v
        if int_keys:
            key[(i + 5) % n] = v
    return key, start, end, result, payload


def channel_of(key, max_parallelism, channels):
    """KeyGroupStreamPartitioner.selectChannel through the Python restatement of
    KeyGroupRangeAssignment (flink_amd/windowing.py)."""
    kg = W.assign_to_key_group(int(key), max_parallelism)
    return W.compute_operator_index_for_key_group(max_parallelism, channels, kg)


def wrap64(v):
    return (int(v) + (1 << 63)) % (1 << 64) - (1 << 63)


def reference(cols, name, channels=1, max_parallelism=128, watermark=None, global_window=False):
    """One bytes object per channel: netbuf.record per row in input order, then the watermark."""
    types, sources, nbytes = LAYOUTS[name]
    out = [[] for _ in range(channels)]
    for i in range(len(cols[0])):
        fields = []
        for t, s in zip(types, sources):
            v = int(cols[s][i])
            fields.append(struct.unpack(">d", struct.pack(">q", v))[0] if t == "D" else v)
        ts = I64_MAX if global_window else wrap64(int(cols[E][i]) - 1)
        rec = NB.record(fields, types, ts)  # (struct keeps a NaN's payload bits through a float)
        assert len(rec) == nbytes
        out[0 if channels == 1 else channel_of(cols[K][i], max_parallelism, channels)].append(rec)
    tail = b"" if watermark is None else NB.watermark(watermark)
    return [b"".join(x) + tail for x in out]


def call_host(cols, lay, channels=1, max_parallelism=128, watermark=None, mode=0, cap=None, guard=64,
              payload=True):
    """gw_encode_rows_host into a 0xFF-filled buffer of cap bytes with `guard` more behind them:
    (rc, buffer, chan_off, chan_bytes)."""
    import ctypes
    cols = [np.ascontiguousarray(c, np.int64) for c in cols]
    n = len(cols[0])
    if cap is None:
        cap = n * 77 + channels * 32
    buf = np.full(cap + guard, 0xFF, np.uint8)
    off, nb = np.full(channels, -1, np.int64), np.full(channels, -1, np.int64)
    rc = N.lib().gw_encode_rows_host(n, *[c.ctypes.data for c in cols[:4]], cols[4].ctypes.data if payload else None,
                                     ctypes.byref(lay), mode, channels, max_parallelism,
                                     N.NO_WATERMARK if watermark is None else watermark, buf.ctypes.data, cap,
                                     off.ctypes.data, nb.ctypes.data)
    return rc, buf, off, nb


def slices(buf, off, nb):
    return [buf[o:o + b].tobytes() for o, b in zip(off.tolist(), nb.tolist())]


def check_ranges(off, nb, cap):
    """Ranges in channel order, 16-byte aligned starts, padding below 16 bytes, inside cap."""
    end = 0
    for o, b in zip(off.tolist(), nb.tolist()):
        assert o % 16 == 0 and 0 <= o - end < 16 and b >= 0
        end = o + b
    assert end <= cap
    return end
