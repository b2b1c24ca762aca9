"""The interval join (gw_interval_join_device, gw_ijoin_*; gw_ijoin.hip) on two shapes, timestamps
uniform in a 10 s span:

    q8     Nexmark-Q8-like: --left records (one per key) and --right records with keys uniform over
           them, bounds (-10 s, 10 s): every same-key pair is inside, about one row per right record
    skew   the same sizes with 1% of each side's records on one key and bounds of --skew-bound ms
           either way, so the hot key's partner ranges are long but its rows stay near the q8 count

Stateless call: the right side probes a buffer of the left side.  Per shape, after one untimed
warm-up call, --iters calls are timed: the whole call with a host clock (it ends in a stream
synchronise) and its expand kernel alone between two HIP events (gw_interval_join_device_timed).
Reported: medians, rows/s of the call, and the expand kernel's written bytes/s (40 B per row: five
int64 columns), to hold against the rate of a streaming copy and against scripts/join_bench.py.
The row count is checked against a count made with torch.searchsorted over (key, ts) words.

Operator (--operator): per iteration a fresh handle takes the whole right side as its log (untimed),
then two timed calls: `probe`, one call of the left side against that log (its merge goes into an
empty log), and `merge`, one call of --left more right records into that log (its probe meets the
left log).  Per call: the host clock around it plus a wait for the handle's stream, and the device
times of its probe stage (probe, two scans, descriptors) and of its merge kernel
(gw_ijoin_last_times).  The merge's bytes are from shapes: 24 B read and 24 B written per record
of the log and the batch.  One JSON line per run on stdout and in --out.

    python scripts/ijoin_bench.py [--left 1000000] [--right 10000000] [--iters 5] [--shapes q8,skew]
                                  [--operator] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flink_amd import _native as N  # noqa: E402
from flink_amd import windowing as W  # noqa: E402

SPAN = 10_000


def make(shape, n_l, n_r, torch):
    g = torch.Generator(device="cuda").manual_seed(8)
    lkey = torch.randperm(n_l, device="cuda", generator=g)
    rkey = torch.randint(0, n_l, (n_r,), device="cuda", generator=g)
    if shape == "skew":  # 1% of each side on key 0, spread over the arrival order
        lkey[torch.randperm(n_l, device="cuda", generator=g)[:n_l // 100]] = 0
        rkey[torch.randperm(n_r, device="cuda", generator=g)[:n_r // 100]] = 0
    cols = []
    for key in (lkey, rkey):
        ts = torch.randint(0, SPAN, (key.numel(),), device="cuda", generator=g)
        pay = torch.arange(key.numel(), device="cuda", dtype=torch.int64)
        cols += [key, ts, pay]
    return cols


def count_rows(lkey, lts, rkey, rts, lower, upper, torch):
    """Rows of left ⋈ right and the longest partner range of a right record: the left side as sorted
    key * 4 SPAN + ts words (ts and the bounds stay inside one key's stripe), two searches per right."""
    stripe = 4 * SPAN
    lw = torch.sort(lkey * stripe + lts + SPAN)[0]
    lo = torch.searchsorted(lw, rkey * stripe + torch.clamp(rts - upper, -SPAN, 2 * SPAN) + SPAN, right=False)
    hi = torch.searchsorted(lw, rkey * stripe + torch.clamp(rts - lower, -SPAN, 2 * SPAN) + SPAN, right=True)
    return int((hi - lo).sum().item()), int((hi - lo).max().item())


def med(v):
    return sorted(v)[len(v) // 2]


def stats(res, prefix, v, digits):
    res[prefix] = round(med(v), digits)
    res[prefix + "_min_max"] = [round(min(v), digits), round(max(v), digits)]
    return med(v)


def run_stateless(shape, n_l, n_r, bound, iters, torch):
    cols = make(shape, n_l, n_r, torch)
    want, longest = count_rows(cols[0], cols[1], cols[3], cols[4], -bound, bound, torch)
    out = [torch.empty(max(want, 1), dtype=torch.int64, device="cuda") for _ in range(5)]
    torch.cuda.synchronize()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    n_out, ms = ctypes.c_int64(0), ctypes.c_double(0)
    call, expand = [], []
    for i in range(iters + 1):  # the first call is the warm-up
        t0 = time.perf_counter()
        rc = N.lib().gw_interval_join_device_timed(N.JOIN_RIGHT, n_r, P(cols[3]), P(cols[4]), P(cols[5]), n_l, P(cols[0]),
                                                   P(cols[1]), P(cols[2]), -bound, bound, *[P(o) for o in out], want,
                                                   ctypes.byref(n_out), None, ctypes.byref(ms))
        t1 = time.perf_counter()
        N.check(rc)
        if i:
            call.append((t1 - t0) * 1e3)
            expand.append(ms.value)
    rows = n_out.value
    # spot check: every row inside the bounds on one key
    inside = bool(((out[2][:rows] - out[1][:rows]).abs() <= bound).all().item()) if rows else True
    res = {"shape": shape, "run": "stateless", "probe": "right", "left": n_l, "right": n_r, "bounds": [-bound, bound],
           "rows": rows, "rows_match": rows == want and inside, "longest_partner_range": longest}
    c = stats(res, "call_ms", call, 3)
    e = stats(res, "expand_ms", expand, 4)
    res["rows_per_s"] = round(rows / (c * 1e-3))
    res["expand_written_bytes_per_s"] = round(rows * 40 / (e * 1e-3)) if e > 0 else None
    return res, res["rows_match"]


def run_operator(shape, n_l, n_r, bound, iters, torch):
    cols = make(shape, n_l, n_r, torch)
    extra = make(shape, n_l, n_l, torch)[3:]  # n_l more right records for the timed merge
    want_probe, _ = count_rows(cols[0], cols[1], cols[3], cols[4], -bound, bound, torch)
    want_merge, _ = count_rows(cols[0], cols[1], extra[0], extra[1], -bound, bound, torch)
    torch.cuda.synchronize()
    t = {k: [] for k in ("probe_call", "probe_probe", "merge_call", "merge_probe", "merge_merge")}
    ok = True
    for i in range(iters + 1):  # the first round is the warm-up
        with W.GpuIntervalJoinOperator(-bound, bound, capacity_hint=n_r + n_l, max_batch=1 << 24) as op:
            op.process_batch_device(op.RIGHT, *cols[3:])
            op.last_times()  # (waits for the stream)
            t0 = time.perf_counter()
            rows_p = op.process_batch_device(op.LEFT, *cols[:3])
            p_ms, _ = op.last_times()
            t1 = time.perf_counter()
            op.clear_rows()
            rows_m = op.process_batch_device(op.RIGHT, *extra)
            p2_ms, m_ms = op.last_times()
            t2 = time.perf_counter()
            st = op.stats()
            ok = ok and rows_p == want_probe and rows_m == want_merge and st["live_right"] == n_r + n_l and st["live_left"] == n_l
            if i:
                for k, v in zip(t, ((t1 - t0) * 1e3, p_ms, (t2 - t1) * 1e3, p2_ms, m_ms)):
                    t[k].append(v)
    res = {"shape": shape, "run": "operator", "log_right": n_r, "left_call": n_l, "right_call": n_l, "bounds": [-bound, bound],
           "probe_call_rows": want_probe, "merge_call_rows": want_merge, "counts_match": ok}
    stats(res, "probe_call_ms", t["probe_call"], 3)
    stats(res, "probe_call_probe_stage_ms", t["probe_probe"], 4)
    stats(res, "merge_call_ms", t["merge_call"], 3)
    stats(res, "merge_call_probe_stage_ms", t["merge_probe"], 4)
    m = stats(res, "merge_call_merge_ms", t["merge_merge"], 4)
    res["merge_read_plus_written_bytes_per_s"] = round((n_r + n_l) * 48 / (m * 1e-3)) if m > 0 else None
    return res, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--left", type=int, default=1_000_000)
    ap.add_argument("--right", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--shapes", default="q8,skew")
    ap.add_argument("--skew-bound", type=int, default=50)
    ap.add_argument("--operator", action="store_true", help="also the operator's probe and merge calls")
    ap.add_argument("--out", default=os.path.join("profiles", "ijoin", "ijoin_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("ijoin_bench needs a GPU", file=sys.stderr)
        return 2
    lines, ok = [], True
    for shape in a.shapes.split(","):
        if shape not in ("q8", "skew"):
            print(f"unknown shape {shape}", file=sys.stderr)
            return 2
        bound = SPAN if shape == "q8" else a.skew_bound
        runs = [run_stateless] + ([run_operator] if a.operator else [])
        for run in runs:
            res, good = run(shape, a.left, a.right, bound, a.iters, torch)
            ok = ok and good
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
