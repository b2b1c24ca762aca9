"""The stateless window join (gw_window_join_device, gw_join.hip) on two shapes, one tumbling 10 s
window each:

    q8     Nexmark Q8: --persons persons (one per seller id) join --auctions auctions with sellers
           uniform over the persons, so most groups are 1 x ~10
    skew   the same sizes with 1% of each side's records on one key: one group holds most pairs

Per shape, after one untimed warm-up call, --iters calls are timed: the whole call with a host
clock (the call ends in a stream synchronise) and its expand kernel alone between two HIP events
(gw_window_join_device_timed).  Reported: medians, pairs/s of the call, and the expand kernel's
written bytes/s (40 B per pair: five int64 columns), to hold against the rate of a streaming copy.
The pair count is checked against sum over keys of L_k * R_k.  One JSON line per shape on stdout
and in --out.

--modes adds, per shape, runs of the other outputs of the same groups:

    full_outer   gw_window_join_outer_device_timed in GW_JOIN_MODE_FULL_OUTER with the present
                 column: the pairs plus one row per record without a partner (41 B per row)
    cogroup      gw_window_cogroup_device_timed: the groups as a CSR; timed between the events are
                 its two writer kernels (groups and elements), and the bytes are from shapes:
                 written 40 B per group + 8 B per element, read 36 B per group by the group
                 writer and 20 B per element + 24 B per group by the element pass

Their row, group and element counts are checked against the per-key counts as well.

    python scripts/join_bench.py [--persons 1000000] [--auctions 10000000] [--iters 5]
                                 [--modes inner,full_outer,cogroup] [--out FILE]
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

SIZE = 10_000


def make(shape, n_l, n_r, torch):
    g = torch.Generator(device="cuda").manual_seed(8)
    lkey = torch.randperm(n_l, device="cuda", generator=g)
    rkey = torch.randint(0, n_l, (n_r,), device="cuda", generator=g)
    if shape == "skew":  # 1% of each side on key 0, spread over the arrival order
        lkey[torch.randperm(n_l, device="cuda", generator=g)[:n_l // 100]] = 0
        rkey[torch.randperm(n_r, device="cuda", generator=g)[:n_r // 100]] = 0
    cols = []
    for key in (lkey, rkey):
        ts = torch.randint(0, SIZE, (key.numel(),), device="cuda", generator=g)
        pay = torch.arange(key.numel(), device="cuda", dtype=torch.int64)
        cols += [key, ts, pay]
    return cols


def run(shape, n_l, n_r, iters, torch):
    cols = make(shape, n_l, n_r, torch)
    lc = torch.bincount(cols[0], minlength=n_l).to(torch.int64)
    rc = torch.bincount(cols[3], minlength=n_l).to(torch.int64)
    want = int((lc * rc).sum().item())
    out = [torch.empty(want, dtype=torch.int64, device="cuda") for _ in range(5)]
    torch.cuda.synchronize()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    n_out, ms = ctypes.c_int64(0), ctypes.c_double(0)
    call, expand = [], []
    for i in range(iters + 1):  # the first call is the warm-up
        t0 = time.perf_counter()
        rc_ = N.lib().gw_window_join_device_timed(n_l, P(cols[0]), P(cols[1]), P(cols[2]), n_r, P(cols[3]), P(cols[4]),
                                                  P(cols[5]), SIZE, SIZE, 0, -(1 << 63), (1 << 63) - 1, *[P(o) for o in out],
                                                  want, ctypes.byref(n_out), None, ctypes.byref(ms))
        t1 = time.perf_counter()
        N.check(rc_)
        if i:
            call.append((t1 - t0) * 1e3)
            expand.append(ms.value)
    med = lambda v: sorted(v)[len(v) // 2]
    pairs = n_out.value
    res = {"shape": shape, "left": n_l, "right": n_r, "pairs": pairs, "pairs_match": pairs == want,
           "largest_group_pairs": int((lc * rc).max().item()),
           "call_ms": round(med(call), 3), "call_ms_min_max": [round(min(call), 3), round(max(call), 3)],
           "expand_ms": round(med(expand), 4), "expand_ms_min_max": [round(min(expand), 4), round(max(expand), 4)],
           "pairs_per_s": round(pairs / (med(call) * 1e-3)),
           "expand_written_bytes_per_s": round(pairs * 40 / (med(expand) * 1e-3)) if med(expand) > 0 else None}
    return res


def _timed(call, iters):
    """iters timed calls after one warm-up: (call ms, device ms between the events) lists."""
    ms = ctypes.c_double(0)
    host, dev = [], []
    for i in range(iters + 1):
        t0 = time.perf_counter()
        rc_ = call(ctypes.byref(ms))
        t1 = time.perf_counter()
        N.check(rc_)
        if i:
            host.append((t1 - t0) * 1e3)
            dev.append(ms.value)
    return host, dev


def _stats(res, prefix, v, digits):
    med = sorted(v)[len(v) // 2]
    res[prefix] = round(med, digits)
    res[prefix + "_min_max"] = [round(min(v), digits), round(max(v), digits)]
    return med


def run_full_outer(shape, n_l, n_r, iters, torch):
    cols = make(shape, n_l, n_r, torch)
    lc = torch.bincount(cols[0], minlength=n_l).to(torch.int64)
    rc = torch.bincount(cols[3], minlength=n_l).to(torch.int64)
    pairs = int((lc * rc).sum().item())
    left_only, right_only = int(lc[rc == 0].sum().item()), int(rc[lc == 0].sum().item())
    want = pairs + left_only + right_only
    out = [torch.empty(want, dtype=torch.int64, device="cuda") for _ in range(5)]
    pres = torch.empty(want, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    n_out = ctypes.c_int64(0)
    call, expand = _timed(lambda ms: N.lib().gw_window_join_outer_device_timed(
        n_l, P(cols[0]), P(cols[1]), P(cols[2]), n_r, P(cols[3]), P(cols[4]), P(cols[5]), SIZE, SIZE, 0, -(1 << 63),
        (1 << 63) - 1, N.JOIN_MODE_FULL_OUTER, -1, *[P(o) for o in out], P(pres), want, ctypes.byref(n_out), None, ms), iters)
    kinds = torch.bincount(pres.to(torch.int64), minlength=4).tolist()
    res = {"shape": shape, "mode": "full_outer", "left": n_l, "right": n_r, "rows": n_out.value,
           "rows_match": n_out.value == want and kinds[1:] == [left_only, right_only, pairs],
           "left_only_rows": left_only, "right_only_rows": right_only}
    c = _stats(res, "call_ms", call, 3)
    e = _stats(res, "expand_ms", expand, 4)
    res["rows_per_s"] = round(want / (c * 1e-3))
    res["expand_written_bytes_per_s"] = round(want * 41 / (e * 1e-3)) if e > 0 else None
    return res, res["rows_match"]


def run_cogroup(shape, n_l, n_r, iters, torch):
    cols = make(shape, n_l, n_r, torch)
    lc = torch.bincount(cols[0], minlength=n_l)
    rc = torch.bincount(cols[3], minlength=n_l)
    groups = int(((lc + rc) > 0).sum().item())
    g = [torch.empty(groups + 1, dtype=torch.int64, device="cuda") for _ in range(5)]
    le = torch.empty(n_l, dtype=torch.int64, device="cuda")
    re = torch.empty(n_r, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    n3 = (ctypes.c_int64 * 3)()
    call, write = _timed(lambda ms: N.lib().gw_window_cogroup_device_timed(
        n_l, P(cols[0]), P(cols[1]), P(cols[2]), n_r, P(cols[3]), P(cols[4]), P(cols[5]), SIZE, SIZE, 0, -(1 << 63),
        (1 << 63) - 1, *[P(x) for x in g], P(le), n_l, P(re), n_r, groups, n3, None, ms), iters)
    present = (lc + rc) > 0
    ok = (tuple(n3) == (groups, n_l, n_r) and bool((torch.diff(g[3]) == lc[present]).all().item())
          and bool((torch.diff(g[4]) == rc[present]).all().item()) and int(le.sum().item()) == n_l * (n_l - 1) // 2
          and int(re.sum().item()) == n_r * (n_r - 1) // 2)
    res = {"shape": shape, "mode": "cogroup", "left": n_l, "right": n_r, "groups": n3[0], "left_elements": n3[1],
           "right_elements": n3[2], "csr_match": ok}
    c = _stats(res, "call_ms", call, 3)
    w = _stats(res, "write_ms", write, 4)
    written = groups * 40 + (n_l + n_r) * 8
    read = groups * 36 + (n_l + n_r) * 20 + groups * 24
    res["elements_per_s"] = round((n_l + n_r) / (c * 1e-3))
    res["write_written_bytes_per_s"] = round(written / (w * 1e-3)) if w > 0 else None
    res["write_read_plus_written_bytes_per_s"] = round((written + read) / (w * 1e-3)) if w > 0 else None
    return res, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--persons", type=int, default=1_000_000)
    ap.add_argument("--auctions", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--shapes", default="q8,skew")
    ap.add_argument("--modes", default="inner", help="inner, full_outer, cogroup (comma separated)")
    ap.add_argument("--out", default=os.path.join("profiles", "join", "join_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("join_bench needs a GPU", file=sys.stderr)
        return 2
    lines, ok = [], True
    for shape in a.shapes.split(","):
        for mode in a.modes.split(","):
            if mode == "inner":
                res = run(shape, a.persons, a.auctions, a.iters, torch)
                good = res["pairs_match"]
            elif mode == "full_outer":
                res, good = run_full_outer(shape, a.persons, a.auctions, a.iters, torch)
            elif mode == "cogroup":
                res, good = run_cogroup(shape, a.persons, a.auctions, a.iters, torch)
            else:
                print(f"unknown mode {mode}", file=sys.stderr)
                return 2
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
