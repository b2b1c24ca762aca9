"""Row encoder measurements (profiles/row_encode/): one JSON line per figure.

    python scripts/row_encode_bench.py [--rows 10000000] [--reps 5]

encode: gw_encode_rows_device over uniform keys, layout "JJ" (key, result), channels 1 and 8,
        timed with HIP events on the stream around the call (warm; the span covers the call's
        4-byte flag clear and read-back next to its kernels, and for channels > 1 the partition
        passes and the host's wait for the row counts).
drain:  a tumbling sum_i64 operator fires `rows` rows; gw_drain into pinned columns against
        gw_drain_serialized into a pinned byte buffer, wall time of the call."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flink_amd import _native as N  # noqa: E402
from flink_amd import windowing as W  # noqa: E402


def encode(rows, reps):
    import torch
    g = torch.Generator(device="cuda").manual_seed(1)
    key = torch.randint(0, 1 << 40, (rows,), dtype=torch.int64, device="cuda", generator=g)
    start = torch.zeros(rows, dtype=torch.int64, device="cuda")
    end = start + 1000
    res = torch.randint(0, 1 << 30, (rows,), dtype=torch.int64, device="cuda", generator=g)
    lay = N.row_layout("JJ", (N.GW_ROW_KEY, N.GW_ROW_RESULT))
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    s = torch.cuda.current_stream()
    for channels in (1, 8):
        cap = rows * 29 + channels * 32
        out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        off, nb = np.zeros(channels, np.int64), np.zeros(channels, np.int64)
        ms = []
        for r in range(reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            N.check(N.lib().gw_encode_rows_device(rows, P(key), P(start), P(end), P(res), None, ctypes.byref(lay), 0,
                                                  channels, 128, 5, P(out), cap, off.ctypes.data, nb.ctypes.data,
                                                  ctypes.c_void_p(s.cuda_stream)))
            b.record(s)
            b.synchronize()
            if r >= 2:
                ms.append(a.elapsed_time(b))
        # read: key, result and end (the timestamp), 24 B per row
        moved = rows * 24 + int(nb.sum())
        best = min(ms)
        print(json.dumps(dict(what="encode", rows=rows, layout="JJ", channels=channels, ms=[round(x, 4) for x in ms],
                              ms_min=round(best, 4), bytes_read=rows * 24, bytes_written=int(nb.sum()),
                              tb_per_s=round(moved / best / 1e9, 3))), flush=True)


def drain(rows, reps):
    import torch
    op = W.GpuWindowOperator(W.TumblingEventTimeWindows.of(1000), "sum_i64", capacity_hint=rows, max_batch=rows).open()
    key = torch.arange(rows, dtype=torch.int64, device="cuda")
    ts = torch.zeros(rows, dtype=torch.int64, device="cuda")
    val = torch.ones(rows, dtype=torch.int64, device="cuda")
    cols = [torch.empty(rows, dtype=torch.int64).pin_memory().numpy() for _ in range(4)]
    cap = rows * 29 + 64
    pinned = torch.empty(cap, dtype=torch.uint8).pin_memory().numpy()
    lay = N.row_layout("JJ", (N.GW_ROW_KEY, N.GW_ROW_RESULT))
    off, nb, got = np.zeros(1, np.int64), np.zeros(1, np.int64), ctypes.c_int64(0)
    t_cols, t_ser = [], []
    for r in range(2 * (reps + 1)):
        ts.fill_(r * 1000)
        op.process_batch_device(key, ts, val)
        assert op.advance_watermark(r * 1000 + 999) == rows
        op.synchronize()
        t0 = time.perf_counter()
        if r % 2 == 0:
            op.drain(out=cols)
        else:
            N.check(N.lib().gw_drain_serialized(op.handle, ctypes.byref(lay), 1, 128, r * 1000 + 999,
                                                pinned.ctypes.data, cap, off.ctypes.data, nb.ctypes.data,
                                                ctypes.byref(got)), op.handle)
            assert got.value == rows
        dt = (time.perf_counter() - t0) * 1e3
        if r >= 2:
            (t_cols if r % 2 == 0 else t_ser).append(dt)
    op.close()
    print(json.dumps(dict(what="drain", rows=rows, bytes=rows * 32, ms=[round(x, 3) for x in t_cols],
                          ms_min=round(min(t_cols), 3))), flush=True)
    print(json.dumps(dict(what="drain_serialized", rows=rows, layout="JJ", bytes=int(nb[0]),
                          ms=[round(x, 3) for x in t_ser], ms_min=round(min(t_ser), 3))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    encode(args.rows, args.reps)
    drain(args.rows, args.reps)
