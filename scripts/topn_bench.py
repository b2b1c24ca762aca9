"""Per-window top-N over a headline-shaped fire (gw_top_n_rows, gw_topn.hip) against its two
yardsticks: a sliding 10 s / 2 s sum_i64 operator over --keys keys is fed until a fire leaves
its rows pending, then three things are timed with events on the handle's stream, each after
one untimed warm-up call:

    (a) top_n_rows(--top)                        the winners alone come to the host
    (b) a device-to-device copy of the four row columns   the streaming yardstick: the kernels
                                                 read at most what the copy reads
    (c) drain() into pinned host arrays          what a caller without the top-N has to do

One JSON line on stdout and in --out.  Under rocprofv3 --kernel-trace --stats the per-kernel
split is k_topn_discover / k_topn_select / k_topn_merge.

    python scripts/topn_bench.py [--keys 10000000] [--windows 1] [--top 10] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flink_amd import windowing as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=10_000_000)
    ap.add_argument("--windows", type=int, default=1, help="windows the timed fire completes (1..5)")
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "topn", "topn_bench.json"))
    a = ap.parse_args()
    import torch
    K, slide = a.keys, 2_000
    hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime torch loaded
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    op = W.GpuWindowOperator(W.SlidingEventTimeWindows.of(10_000, slide), "sum_i64", capacity_hint=K,
                             max_batch=max(K, 1 << 20)).open()
    try:
        stream = torch.cuda.ExternalStream(op.stream())
        g = torch.Generator(device="cuda").manual_seed(5)
        keys = torch.randperm(K, device="cuda", generator=g)
        vals = torch.randint(0, 1_000_000, (K,), device="cuda", generator=g)
        ts = torch.randint(0, slide, (K,), device="cuda", generator=g)
        torch.cuda.synchronize()
        op.process_batch_device(keys, ts, vals)
        op.advance_watermark(a.windows * slide - 1)  # completes the windows ending at 2 s .. windows * 2 s
        n = op.pending_rows()
        (pk, ps, pe, pr), _ = op.rows_device()
        copy = torch.empty((4, n), dtype=torch.int64, device="cuda")
        pinned = [torch.empty(n, dtype=torch.int64, pin_memory=True).numpy() for _ in range(4)]

        def timed(fn, iters):
            best = []
            for i in range(iters + 1):  # the first call is the warm-up
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if i:
                    best.append(e0.elapsed_time(e1))
            return sorted(best)[len(best) // 2]

        def d2d():
            for c, p in enumerate((pk, ps, pe, pr)):
                hip.hipMemcpyAsync(copy[c].data_ptr(), p, n * 8, 3, op.stream())

        winners = op.top_n_rows(a.top)
        t_top = timed(lambda: op.top_n_rows(a.top), a.iters)
        t_copy = timed(d2d, a.iters)
        # drain consumes the rows: warm up on the pinned arrays with a copy of the same size,
        # then time the one drain
        for c, p in enumerate((pk, ps, pe, pr)):
            hip.hipMemcpyAsync(pinned[c].ctypes.data, p, n * 8, 2, op.stream())
        op.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        k, s, e, r = op.drain(out=pinned)
        e1.record(stream)
        e1.synchronize()
        t_drain = e0.elapsed_time(e1)
        want = W.top_n_host(k, s, e, r, a.top)
        ok = all((x == y).all() for x, y in zip(winners, want))
        res = {"rows": int(n), "windows": int(len(np.unique(e))),
               "top": a.top, "top_n_rows_ms": round(t_top, 4), "d2d_copy_ms": round(t_copy, 4),
               "drain_pinned_ms": round(t_drain, 4), "winners": int(len(winners[0])),
               "winners_match_host_top_n": bool(ok)}
    finally:
        op.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
