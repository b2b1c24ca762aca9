"""Numpy restatement of the per-window top-N contract (include/gpuwin.h, gw_top_n_*), and the
seeded inputs the CPU and GPU tests share.

Reference: a lexsort on (end, order key in the wanted direction, key), then the first `top` rows
of every window.  The order key of a double is computed here from its bits, independently of the
library: Double.compare order (-0.0 < 0.0, every NaN equal and above +inf).
"""
import numpy as np

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
NAN_A = np.array([0x7ff8000000000000], np.uint64).view(np.int64)[0]   # the canonical NaN
NAN_B = np.array([0xfff0000000000123], np.uint64).view(np.int64)[0]   # sign bit set, another payload


def f64_order_key(bits):
    """int64 whose signed order is Double.compare's, from the IEEE bits."""
    b = np.asarray(bits, np.int64).copy()
    u = b.view(np.uint64)
    nan = ((u >> np.uint64(52)) & np.uint64(0x7ff)) == np.uint64(0x7ff)
    nan &= (u & np.uint64(0xfffffffffffff)) != 0
    b[nan] = NAN_A
    neg = b < 0
    b[neg] ^= np.int64(0x7fffffffffffffff)
    return b


def reference(key, start, end, result, top, smallest=False, f64=False):
    """(key, start, end, result bits, win_rows) of the contract; raises ValueError where the
    library returns GW_E_INVALID for two starts under one end."""
    key, start, end = (np.asarray(x, np.int64) for x in (key, start, end))
    bits = np.asarray(result).view(np.int64)
    o = f64_order_key(bits) if f64 else bits
    # descending order without negating (INT64_MIN has no negative): the complement reverses it
    d = o if smallest else ~o
    idx = np.lexsort((key, d, end))
    e = end[idx]
    first = np.r_[True, e[1:] != e[:-1]] if len(e) else np.zeros(0, bool)
    wid = np.cumsum(first) - 1
    starts = np.nonzero(first)[0]
    sizes = np.diff(np.r_[starts, len(e)])
    if len(e) and (start[idx] != start[idx][starts][wid]).any():
        raise ValueError("two starts under one end")
    rank = np.arange(len(e)) - starts[wid] if len(e) else np.zeros(0, np.int64)
    keep = idx[rank < top]
    return key[keep], start[keep], end[keep], bits[keep], sizes[wid][rank < top].astype(np.int64)


def check(got, want, f64=False):
    """Exact comparison of (key, start, end, result, win_rows); NaN bits compare as 'both NaN'."""
    names = ("key", "start", "end", "result", "win_rows")
    assert len(got[0]) == len(want[0]), f"{len(got[0])} rows, reference {len(want[0])}"
    for c in (0, 1, 2, 4):
        g, w = np.asarray(got[c]), np.asarray(want[c])
        assert np.array_equal(g, w), f"{names[c]} differs at row {int(np.nonzero(g != w)[0][0])}"
    g, w = np.asarray(got[3]).view(np.int64), np.asarray(want[3]).view(np.int64)
    same = g == w
    if f64:
        same |= np.isnan(g.view(np.float64)) & np.isnan(w.view(np.float64))
    assert same.all(), f"result differs at row {int(np.nonzero(~same)[0][0])}"


KINDS = ("ties", "full", "f64")


def make_rows(seed, n, windows, kind):
    """n rows in `windows` windows interleaved at random (fewer when n < windows).  kind: 'ties'
    int64 results from a 7-value domain (ties decide most ranks), 'full' the whole int64 range
    with both extremes, 'f64' doubles with +-0.0, +-inf and NaNs of two payloads.  Keys repeat and
    include negative ones and both extremes."""
    rng = np.random.default_rng(seed)
    wends = rng.choice(np.arange(-5 * windows, 5 * windows + 1), size=windows, replace=False).astype(np.int64) * 1000
    if windows >= 3:
        wends[0], wends[1] = I64_MIN, I64_MAX  # the library's own empty mark must be a usable end
    w = rng.integers(0, windows, n)
    end = wends[w]
    start = end - np.int64(10_000)  # wraps for the extreme ends: still one start per end
    key = rng.integers(-50, max(n // 2, 2), n).astype(np.int64)
    if n >= 4:
        key[rng.integers(0, n)] = I64_MIN
        key[rng.integers(0, n)] = I64_MAX
    if kind == "ties":
        res = rng.integers(-3, 4, n).astype(np.int64)
    elif kind == "full":
        res = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
        if n >= 2:
            res[rng.integers(0, n)] = I64_MIN
            res[rng.integers(0, n)] = I64_MAX
    else:
        vals = rng.normal(0.0, 100.0, n)
        vals = np.where(rng.random(n) < 0.3, np.round(vals), vals)  # some ties
        res = vals.view(np.int64).copy()
        special = np.array([0.0, -0.0, np.inf, -np.inf], np.float64).view(np.int64)
        special = np.concatenate([special, [NAN_A, NAN_B]])
        hit = rng.random(n) < 0.25
        res[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    return key, start, end, res
