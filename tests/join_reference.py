"""The window-join contract of include/gpuwin.h (gw_window_join_*, gw_join_*) restated in plain
Python, from the contract's text: Flink's stream.join(other).where().equalTo().window().apply(),
i.e. union -> keyBy -> WindowOperator with ListState -> JoinCoGroupFunction's nested loop.

Python integers do not wrap, so "beyond int64" is tested on the true value.
"""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MAX_WINDOWS = 64


class NoTimestamp(Exception):
    pass


class WindowRange(Exception):
    pass


class Unsupported(Exception):
    pass


def check_geometry(size, slide, offset):
    if size <= 0 or slide <= 0 or abs(offset) >= slide:
        raise ValueError("size > 0, slide > 0, |offset| < slide")
    if -(-size // slide) > MAX_WINDOWS:
        raise Unsupported("more than 64 windows per record")


def _i64(v):
    if not I64_MIN <= v <= I64_MAX:
        raise WindowRange(v)
    return v


def last_start(ts, slide, offset):
    """TimeWindow.getWindowStartWithOffset(ts, offset, slide)."""
    if ts == I64_MIN:
        raise NoTimestamp()
    return _i64(ts - (_i64(ts - offset) % slide))  # Python's % is the floor modulus


def window_starts(ts, size, slide, offset):
    """SlidingEventTimeWindows.assignWindows: lastStart, lastStart - slide, ... while start > ts - size
    (newest first), with lastStart itself."""
    ls = last_start(ts, slide, offset)
    _i64(ls + size)
    starts = []
    s = ls
    while s > ts - size:
        starts.append(_i64(s))
        s -= slide
    return ls, starts


def _emit(groups, size):
    """groups: {(start, key): ([left payloads], [right payloads])} -> the five columns, windows by
    ascending end, keys ascending, left-major."""
    cols = [[], [], [], [], []]
    for (start, key) in sorted(groups):
        l, r = groups[(start, key)]
        if not l or not r:
            continue
        n = len(l) * len(r)
        cols[0].append(np.full(n, key, np.int64))
        cols[1].append(np.full(n, start, np.int64))
        cols[2].append(np.full(n, start + size, np.int64))
        cols[3].append(np.repeat(np.array(l, np.int64), len(r)))
        cols[4].append(np.tile(np.array(r, np.int64), len(l)))
    return tuple(np.concatenate(c) if c else np.empty(0, np.int64) for c in cols)


def reference(left, right, size, slide, offset, w0=I64_MIN, w1=I64_MAX):
    """left / right: (key, ts, payload) columns in arrival order.  The pairs of the windows with
    w0 < end - 1 <= w1 as five int64 columns (key, start, end, left payload, right payload)."""
    check_geometry(size, slide, offset)
    if len(left[0]) == 0 or len(right[0]) == 0:
        return _emit({}, size)
    groups = {}
    for side, (key, ts, pay) in enumerate((left, right)):
        for k, t, p in zip(key.tolist(), ts.tolist(), pay.tolist()):
            _, starts = window_starts(t, size, slide, offset)
            for s in starts:
                if w0 < s + size - 1 <= w1:
                    groups.setdefault((s, k), ([], []))[side].append(p)
    return _emit(groups, size)


class ReferenceJoinOperator:
    """The stateful contract: a list per (key, window) and side, late records dropped and counted,
    windows fired by the watermark in the specified order."""

    def __init__(self, size, slide, offset=0):
        check_geometry(size, slide, offset)
        self.size, self.slide, self.offset = size, slide, offset
        self.wm = I64_MIN
        self.state = {}
        self.late_dropped = 0
        self.pairs_fired = 0

    def ingest(self, side, key, ts, pay):
        for k, t, p in zip(np.asarray(key).tolist(), np.asarray(ts).tolist(), np.asarray(pay).tolist()):
            ls, starts = window_starts(t, self.size, self.slide, self.offset)
            if ls + self.size - 1 <= self.wm:
                self.late_dropped += 1
                continue
            for s in starts:
                if s + self.size - 1 > self.wm:  # a window that has passed never sees the record
                    self.state.setdefault((s, k), ([], []))[side].append(p)

    def advance_watermark(self, wm):
        """The pairs fired (five columns); a watermark that does not advance fires nothing."""
        self.last_fired = {}
        if wm <= self.wm:
            return _emit({}, self.size)
        fire = {g: v for g, v in self.state.items() if self.wm < g[0] + self.size - 1 <= wm}
        for g in fire:
            del self.state[g]
        # the group table of this fire, one-sided groups included: (start, key) -> (L, R)
        self.last_fired = {g: (len(v[0]), len(v[1])) for g, v in fire.items()}
        self.wm = wm
        out = _emit(fire, self.size)
        self.pairs_fired += len(out[0])
        return out

    def end_input(self):
        return self.advance_watermark(I64_MAX)

    def live_records(self, side):
        """Distinct records (by payload) of `side` still held by some window."""
        return len({p for v in self.state.values() for p in v[side]})


SPECIAL_KEYS = [I64_MIN, -1, 0, I64_MAX]


def key_table(rng, n):
    """n distinct keys: the four the contract names, then random int64s."""
    extra = rng.integers(I64_MIN, I64_MAX, max(0, n - 4), dtype=np.int64, endpoint=True)
    return np.concatenate([np.array(SPECIAL_KEYS, np.int64), extra])[:max(n, 1)]


def make_records(seed, n_l, n_r, num_keys, ts_lo=-40, ts_span=100):
    """Seeded inputs: per side (key, ts, payload) with keys drawn from num_keys distinct values
    (INT64_MIN, -1, 0 and INT64_MAX among them), timestamps uniform in [ts_lo, ts_lo + ts_span)
    and distinct random payloads."""
    rng = np.random.default_rng(seed)
    table = key_table(rng, num_keys)
    sides = []
    for n in (n_l, n_r):
        key = table[rng.integers(0, len(table), n)]
        ts = rng.integers(ts_lo, ts_lo + ts_span, n).astype(np.int64)
        pay = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
        sides.append((key, ts, pay))
    return sides[0], sides[1]


def check(got, want):
    """Exact, in order and values."""
    assert len(got) == 5
    for c, name in enumerate(("key", "start", "end", "left payload", "right payload")):
        g, w = np.asarray(got[c]), np.asarray(want[c])
        assert len(g) == len(w), f"{len(g)} pairs, expected {len(w)}"
        if not np.array_equal(g, w):
            i = int(np.nonzero(g != w)[0][0])
            raise AssertionError(f"{name} differs at pair {i}: {int(g[i])} vs {int(w[i])}")
