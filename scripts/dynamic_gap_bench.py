"""What the per-element gap column costs: the sessions config's stream (scripts/configs_bench.py:
event-time sessions, avg(f64) over 12.5M keys, 10M records per watermark batch) through a
DynamicEventTimeSessionWindows handle with gap == 10 s on every record, and through the
EventTimeSessionWindows.withGap(10 s) handle, in one process on the same columns.

Each handle runs the stream twice: once untimed for events/s (host clock over the timed steps),
once with kernel timing on for the device split per batch -- gw_kernel_time_ms 0 (ingest), 6 / 7
/ 8 (its prep, sort and segment) and 1 (fire).  Both fire the same rows (checked).  The DYN prep
writes a 32-B (ts, value, gap, 0) record where the constant prep writes a 16-B (ts, value) pair,
and the segment gathers it from the same 64-B sector.

One JSON line on stdout and in --out.

    python scripts/dynamic_gap_bench.py [--steps 100] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def run(kind, timing, cols, wms, nb, warmup, steps):
    import torch
    from flink_amd import windowing as W
    keys, ts, vals, gaps = cols
    assigner = W.EventTimeSessionWindows.with_gap(10_000) if kind == "constant" \
        else W.DynamicEventTimeSessionWindows.with_dynamic_gap(lambda v: 10_000)
    op = W.GpuWindowOperator(assigner, "avg_f64", capacity_hint=12_500_000, max_batch=nb * 2).open()
    rows = 0

    def step(b):
        nonlocal rows
        lo, hi = b * nb, (b + 1) * nb
        op.process_batch_device(keys[lo:hi], ts[lo:hi], vals[lo:hi], stream=op.stream(),
                                gaps=gaps[lo:hi] if kind == "dynamic" else None)
        rows += op.advance_watermark(wms[b])
        op.clear_rows()

    try:
        for b in range(warmup):
            step(b)
        op.synchronize()
        torch.cuda.synchronize()
        rows = 0
        if timing:
            op.enable_kernel_timing(2)  # with the ingest's prep / sort / segment split
            for w in (0, 1, 6, 7, 8):
                op.kernel_time_ms(w)  # reset
        t0 = time.perf_counter()
        for b in range(warmup, warmup + steps):
            step(b)
        op.synchronize()
        dt = time.perf_counter() - t0
        out = {"events_per_s": nb * steps / dt, "ms_per_step": dt * 1e3 / steps, "rows_fired": rows,
               "session_merges": op.stats()["session_merges"]}
        if timing:
            out = {"rows_fired": rows}
            for name, w in (("ingest_ms", 0), ("prep_ms", 6), ("sort_ms", 7), ("segment_ms", 8), ("fire_ms", 1)):
                out[name] = op.kernel_time_ms(w)[0]
        return out
    finally:
        op.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="timed steps (100: 20 s of event time, sessions fire)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "dynamic_gap", "gap_column_cost.json"))
    a = ap.parse_args()
    import torch
    from configs_bench import gen
    dev = torch.device("cuda:0")
    nb = 10_000_000
    kw, agg, keys, ts, vals, wms = gen("sessions", nb, a.warmup + a.steps, dev)
    assert kw == dict(assigner="session", gap=10_000) and agg == "avg_f64"
    gaps = torch.full_like(ts, 10_000)
    torch.cuda.synchronize()
    cols = (keys, ts, vals, gaps)
    res = {"config": "sessions", "events_per_step": nb, "steps": a.steps, "warmup": a.warmup, "gap_ms": 10_000}
    for kind in ("constant", "dynamic", "constant", "dynamic"):  # alternating, two untimed runs each
        res.setdefault(kind, {"runs": []})["runs"].append(run(kind, False, cols, wms, nb, a.warmup, a.steps))
    for kind in ("constant", "dynamic"):
        res[kind]["device_split"] = run(kind, True, cols, wms, nb, a.warmup, a.steps)
        res[kind]["events_per_s"] = max(r["events_per_s"] for r in res[kind]["runs"])
    rows = {r["rows_fired"] for k in ("constant", "dynamic") for r in res[k]["runs"]}
    assert len(rows) == 1, f"the two handles fired different rows: {rows}"
    res["dynamic_over_constant_events_per_s"] = res["dynamic"]["events_per_s"] / res["constant"]["events_per_s"]
    for part in ("ingest_ms", "prep_ms", "sort_ms", "segment_ms"):
        c = res["constant"]["device_split"][part]
        res["dynamic_over_constant_" + part] = res["dynamic"]["device_split"][part] / c if c else None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
