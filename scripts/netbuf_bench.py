"""Decode throughput of the network-buffer ingest (gw_decode_serialized) on a Q5-shaped
channel: Tuple2<Long, Long> (auction, price) records with timestamps, a watermark every
1M records.  Prints GB/s of serialized bytes; run under rocprofv3 --kernel-trace --stats
for the per-kernel split (k_nb_walk / k_nb_resolve / k_nb_scan / k_nb_decode).

    python scripts/netbuf_bench.py [--records 10000000] [--iters 10]

--compare-lib PATH: the same decode through a second build of the library (the parent commit's,
say), alternated with this one in one process, --repeats times each; prints every repeat's time
so the repeat-to-repeat spread shows beside the difference.

--channels C: the records dealt to C input channels (contiguous shares, each serialized as a
stream of its own); one gw_decode_channels_device call over the C ranges against C sequential
gw_decode_serialized calls over the same bytes, alternated, --repeats times each.  With
--buffer-bytes B every channel's range is the first B bytes of its stream (one network buffer per
channel, the shape a task sees per poll; it may end inside an element).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flink_amd import _native as N  # noqa: E402
from flink_amd import netbuf as NB  # noqa: E402


def timed(f, iters, torch):
    """ms per call of f, a host clock around calls that end in a synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def channels_mode(a, torch):
    n, C = a.records, a.channels
    rng = np.random.default_rng(1)
    k = rng.integers(0, 10_000_000, n)
    t = np.arange(n) // 50
    v = rng.integers(0, 1_000_000, n)
    cuts = np.linspace(0, n, C + 1).astype(np.int64)
    if a.buffer_bytes:  # only the head of each share is needed
        per = a.buffer_bytes // 29 + 2
        cuts = np.arange(C + 1, dtype=np.int64) * per
        assert cuts[-1] <= n, "--records too small for --channels x --buffer-bytes"
    parts = []
    for c in range(C):
        lo, hi = int(cuts[c]), int(cuts[c + 1])
        s = NB.serialize_batches("JJ", 0, 1, [(k[lo:hi], t[lo:hi], v[lo:hi])], [int(t[hi - 1]) - 100])
        parts.append(s[:a.buffer_bytes] if a.buffer_bytes else s)
    tens = [torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda() for s in parts]  # separate allocations
    total = sum(len(s) for s in parts)
    rec_cap = total // 29 + C
    cols = torch.empty((3, rec_cap), dtype=torch.int64, device="cuda")
    ev = torch.empty((2, 2 * C + 8), dtype=torch.int64, device="cuda")
    kind = torch.empty(2 * C + 8, dtype=torch.int32, device="cuda")
    lay = N.record_layout("JJ", 0, 1)
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    L = N.lib()
    ptrs = (ctypes.c_void_p * C)(*[x.data_ptr() for x in tens])
    lens = (ctypes.c_int64 * C)(*[len(s) for s in parts])
    consumed, recs = (ctypes.c_int64 * C)(), (ctypes.c_int64 * C)()
    out, res = N.GwDecodeChannelsResult(), N.GwDecodeResult()

    def segmented():
        N.check(L.gw_decode_channels_device(C, ptrs, lens, ctypes.byref(lay), P(cols[0]), P(cols[1]), P(cols[2]),
                                            rec_cap, P(ev[0]), P(kind), P(ev[1]), ev.shape[1], consumed, recs, None,
                                            ctypes.byref(out), None))

    def sequential():
        at = 0
        for c in range(C):
            N.check(L.gw_decode_serialized(P(tens[c]), len(parts[c]), ctypes.byref(lay), P(cols[0][at:]),
                                           P(cols[1][at:]), P(cols[2][at:]), rec_cap - at, P(ev[0]), P(ev[1]),
                                           ev.shape[1], ctypes.byref(res), None))
            at += res.records
        return at

    segmented()
    seg_cols = cols.clone()
    assert sequential() == out.records and torch.equal(seg_cols[:, :out.records], cols[:, :out.records])
    ms = {"segmented": [], "sequential": []}
    for r in range(a.repeats):  # (the order swaps every repeat)
        for name, f in (("sequential", sequential), ("segmented", segmented))[::1 if r % 2 == 0 else -1]:
            ms[name].append(timed(f, a.iters, torch))
    seg, seq = float(np.median(ms["segmented"])), float(np.median(ms["sequential"]))
    print(json.dumps({"mode": "channels", "channels": C, "buffer_bytes": a.buffer_bytes, "bytes": total,
                      "records": int(out.records), "iters": a.iters, "segmented_ms": ms["segmented"],
                      "sequential_ms": ms["sequential"], "segmented_median_ms": seg, "sequential_median_ms": seq,
                      "sequential_over_segmented": seq / seg}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--mode", choices=["decode", "operator"], default="decode",
                    help="decode: gw_decode_serialized alone; operator: gw_ingest_serialized_device into a "
                         "sliding 10s/2s sum operator (decode + ingest + fires)")
    ap.add_argument("--repeats", type=int, default=5, help="timed repeats of --iters calls (--compare-lib, --channels)")
    ap.add_argument("--compare-lib", default=None, help="a second libgpuwin.so to alternate with this one")
    ap.add_argument("--channels", type=int, default=0, help="segmented decode of C ranges against C single decodes")
    ap.add_argument("--buffer-bytes", type=int, default=0, help="with --channels: bytes per channel (0: an even split)")
    a = ap.parse_args()
    import torch
    if a.channels > 0:
        return channels_mode(a, torch)
    n = a.records
    rng = np.random.default_rng(1)
    k = rng.integers(0, 10_000_000, n)
    t = np.arange(n) // 50
    v = rng.integers(0, 1_000_000, n)
    step = 1_000_000
    data = NB.serialize_batches("JJ", 0, 1, [(k[i:i + step], t[i:i + step], v[i:i + step]) for i in range(0, n, step)],
                                [int(t[min(i + step, n) - 1]) - 100 for i in range(0, n, step)])
    d = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cols = torch.empty((3, n), dtype=torch.int64, device="cuda")
    wm = torch.empty((2, n // step + 1), dtype=torch.int64, device="cuda")
    lay = N.record_layout("JJ", 0, 1)
    res = N.GwDecodeResult()
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    L = N.lib()

    def once():
        N.check(L.gw_decode_serialized(P(d), len(data), ctypes.byref(lay), P(cols[0]), P(cols[1]), P(cols[2]), n,
                                       P(wm[0]), P(wm[1]), wm.shape[1], ctypes.byref(res), None))

    if a.mode == "operator":
        from flink_amd import windowing as W
        op = W.GpuWindowOperator(W.SlidingEventTimeWindows.of(10_000, 2_000), "sum_i64",
                                 capacity_hint=10_000_000, max_batch=2_000_000).open()

        def once():  # noqa: F811  (each call: the same bytes, the clock moved on by shifting watermarks)
            used, _ = op.process_serialized_device(d, lay)
            assert used == len(data)
            op.clear_rows()

    once()
    if a.mode == "operator":
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            once()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.iters
        print(json.dumps({"mode": "operator", "records": n, "bytes": len(data), "ms_per_call": dt * 1e3,
                          "records_per_s": n / dt, "stats": {k: v for k, v in op.stats().items()}
                          if isinstance(op.stats(), dict) else None}))
        op.close()
        return
    assert res.records == n and res.consumed == len(data)
    assert torch.equal(cols[0].cpu(), torch.from_numpy(k)) and torch.equal(cols[2].cpu(), torch.from_numpy(v))
    torch.cuda.synchronize()
    if a.compare_lib:
        other = ctypes.CDLL(os.path.abspath(a.compare_lib))
        other.gw_decode_serialized.restype = ctypes.c_int
        other.gw_decode_serialized.argtypes = L.gw_decode_serialized.argtypes

        def once_other():
            rc = other.gw_decode_serialized(P(d), len(data), ctypes.byref(lay), P(cols[0]), P(cols[1]), P(cols[2]), n,
                                            P(wm[0]), P(wm[1]), wm.shape[1], ctypes.byref(res), None)
            assert rc == 0 and res.records == n

        once_other()
        ms = {"this": [], "other": []}
        for r in range(a.repeats):  # (the order swaps every repeat: neither is always the second)
            for name, f in (("other", once_other), ("this", once))[::1 if r % 2 == 0 else -1]:
                ms[name].append(timed(f, a.iters, torch))
        print(json.dumps({"mode": "compare-lib", "records": n, "bytes": len(data), "iters": a.iters,
                          "this_ms": ms["this"], "other_ms": ms["other"], "other": a.compare_lib,
                          "this_median_ms": float(np.median(ms["this"])),
                          "other_median_ms": float(np.median(ms["other"])),
                          "other_spread_ms": max(ms["other"]) - min(ms["other"])}))
        return
    t0 = time.perf_counter()
    for _ in range(a.iters):
        once()
    dt = (time.perf_counter() - t0) / a.iters
    out = {"records": n, "bytes": len(data), "ms_per_call_incl_alloc_sync": dt * 1e3,
           "GBps_serialized_in": len(data) / dt / 1e9, "records_per_s": n / dt,
           "algorithmic_bytes": len(data) + 24 * n}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
