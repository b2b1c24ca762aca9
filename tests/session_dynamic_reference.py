"""Pure-Python, record-by-record restatement of Flink's merging WindowOperator over
DynamicEventTimeSessionWindows.withDynamicGap: every element brings its own gap and is assigned
the window [ts, ts + gap) (DynamicEventTimeSessionWindows.assignWindows).  TEST INFRASTRUCTURE
ONLY: the checker of the GPU's dynamic-gap session path, which the C oracle (constant gap only)
cannot check.  tests/test_session_dynamic_reference.py pins it to that oracle with a constant
gap column and to hand-written vectors.

Structure follows the reference, not the GPU code (paths relative to the Flink tree, RS/ =
flink-runtime/src/main/java/org/apache/flink/streaming/):
  MergingWindowSet.addWindow      RS/runtime/operators/windowing/MergingWindowSet.java:153-224
                                  (mapping window -> state window, TimeWindow.mergeWindows
                                  with the inclusive TimeWindow.intersects)
  WindowOperator.processElement   merging branch, WindowOperator.java:303-403; the late check
                                  isWindowLate :609-612; the side output / numLateRecordsDropped
                                  :440-446; the merge callback :314-366 (trigger.onMerge, clear of
                                  the merged windows' timers, mergeNamespaces)
  WindowOperator.onEventTime      :450-494, clearAllState :560-571, cleanupTime :670-677
  EventTimeTrigger / PurgingTrigger   fire on element when maxTimestamp <= watermark, timer
                                  otherwise; FIRE -> FIRE_AND_PURGE
  state                           AggregatingState / ReducingState per (key, state window)

Beside the rows it keeps counters of the hard paths (late records, session-to-session merges,
peak sessions per key, windows fired on element) so that a test can assert it reaches them."""
import heapq
import struct

import numpy as np

LONG_MIN = -(1 << 63)
LONG_MAX = (1 << 63) - 1

AGGS = ("count", "sum_i64", "sum_f64", "min_i64", "max_i64", "min_f64", "max_f64", "avg_i64", "avg_f64", "sum_i32")
DOUBLE_INPUT = {"sum_f64", "min_f64", "max_f64", "avg_f64"}
BAD_GAP = "Dynamic session time gap must satisfy 0 < gap"


def _wrap64(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def _wrap32(x):
    return (x + (1 << 31)) % (1 << 32) - (1 << 31)


def _dbits(d):
    return struct.unpack("<q", struct.pack("<d", d))[0]


def _double_compare(a, b):
    """Double.compare: numeric order, then doubleToLongBits (NaN canonical and largest, -0.0 < 0.0)."""
    if a < b:
        return -1
    if a > b:
        return 1
    x = 0x7ff8000000000000 if a != a else _dbits(a)
    y = 0x7ff8000000000000 if b != b else _dbits(b)
    return 0 if x == y else (-1 if x < y else 1)


class _Agg:
    """createAccumulator + add / the first reduced value, add, merge and getResult of one
    aggregate.  v: the int64 value (integer aggregates) or the double (floating ones)."""

    def __init__(self, name):
        if name not in AGGS:
            raise ValueError(f"unknown aggregate {name!r}")
        self.name = name
        self.double_in = name in DOUBLE_INPUT

    def first(self, v):
        n = self.name
        if n == "count":
            return 1
        if n == "avg_i64":
            return (v, 1)
        if n == "avg_f64":
            return (0.0 + v, 1)
        if n == "sum_i32":
            return _wrap32(v)
        return v

    def merge(self, a, b):
        """mergeState(a, b) / ReduceFunction.reduce(a, b); add(v) is merge(a, first(v))."""
        n = self.name
        if n == "count":
            return a + b
        if n == "sum_i64":
            return _wrap64(a + b)
        if n == "sum_i32":
            return _wrap32(a + b)
        if n == "sum_f64":
            return a + b
        if n == "min_i64":
            return a if a < b else b
        if n == "max_i64":
            return a if a > b else b
        if n == "min_f64":
            return a if _double_compare(a, b) < 0 else b
        if n == "max_f64":
            return a if _double_compare(a, b) > 0 else b
        if n == "avg_i64":
            return (_wrap64(a[0] + b[0]), a[1] + b[1])
        return (a[0] + b[0], a[1] + b[1])  # avg_f64

    def result_bits(self, a):
        n = self.name
        if n == "avg_i64":
            return _dbits(float(a[0]) / float(a[1]))
        if n == "avg_f64":
            return _dbits(a[0] / float(a[1]))
        if n in ("sum_f64", "min_f64", "max_f64"):
            return _dbits(a)
        return a


class DynamicSessionOperator:
    """One keyed WindowOperator subtask over DynamicEventTimeSessionWindows."""

    def __init__(self, agg="count", lateness=0, trigger="event_time", side_output=False):
        if lateness < 0:
            raise ValueError("The allowed lateness cannot be negative.")
        if trigger not in ("event_time", "purging_event_time"):
            raise ValueError("unknown trigger")
        self.agg = _Agg(agg)
        self.lateness = int(lateness)
        self.purging = trigger == "purging_event_time"
        self.side_output = side_output
        self.wm = LONG_MIN
        self.sets = {}        # key -> {window: state window}       (MergingWindowSet.mapping)
        self.state = {}       # (key, state window) -> accumulator   (windowMergingState)
        self.timers = set()   # (time, key, window)                  (the event-time timer queue)
        self.heap = []
        self.rows = []        # (key, start, end, result bits) since the last drain
        self.late_out = []    # the side output: (key, ts, value bits)
        self.late_dropped = 0
        # coverage counters
        self.late_records = 0      # skipped late elements (dropped or sent to the side output)
        self.merges = 0            # sessions merged away into another session
        self.peak_sessions = 0     # most in-flight sessions one key held at once
        self.fired_on_element = 0  # windows EventTimeTrigger.onElement fired at once

    # ---- timers ----
    def _register(self, time, key, w):
        t = (time, key, w)
        if t not in self.timers:  # HeapPriorityQueueSet.add dedups
            self.timers.add(t)
            heapq.heappush(self.heap, t)

    def _delete(self, time, key, w):
        self.timers.discard((time, key, w))  # skipped when popped

    def _cleanup_time(self, end):
        ct = end - 1 + self.lateness
        return ct if ct <= LONG_MAX else LONG_MAX  # WindowOperator.cleanupTime: overflow -> Long.MAX_VALUE

    def _is_window_late(self, w):
        return self._cleanup_time(w[1]) <= self.wm

    # ---- MergingWindowSet.addWindow ----
    def _add_window(self, key, mapping, new):
        # The in-flight windows of a key never intersect each other (they would have merged), so
        # a merge group of more than one window always holds the new one: when the new window
        # intersects nothing, mergeWindows reports no merge and the window maps to itself.
        ns, ne = new
        for w in mapping:
            if w[0] <= ne and w[1] >= ns:
                break
        else:
            mapping[new] = new
            return new
        windows = list(mapping)
        if new not in mapping:
            windows.append(new)
        windows.sort(key=lambda w: w[0])  # TimeWindow.mergeWindows: stable sort by start, sweep
        groups = []
        for w in windows:
            if groups and groups[-1][0][0] <= w[1] and groups[-1][0][1] >= w[0]:  # intersects (inclusive)
                c = groups[-1][0]
                groups[-1][0] = (min(c[0], w[0]), max(c[1], w[1]))  # cover
                groups[-1][1].append(w)
            else:
                groups.append([w, [w]])
        result, merged_new, any_merge = new, False, False
        for cover, members in groups:
            if len(members) <= 1:
                continue
            any_merge = True
            if new in members:
                members.remove(new)
                merged_new = True
                result = cover
            state_window = mapping[members[0]]
            merged_state = [mapping.pop(w) for w in members]
            mapping[cover] = state_window
            merged_state.remove(state_window)
            self.merges += len(members) - 1
            if not (cover in members and len(members) == 1):
                self._merge(key, cover, members, state_window, merged_state)
        if not any_merge or (result == new and not merged_new):
            mapping[result] = result
        return result

    # the MergeFunction of WindowOperator.processElement
    def _merge(self, key, result, merged_windows, state_window, merged_state_windows):
        if self._cleanup_time(result[1]) <= self.wm:
            raise RuntimeError("The end timestamp of an event-time window cannot become earlier than the "
                               "current watermark by merging.")
        if result[1] - 1 > self.wm:  # EventTimeTrigger.onMerge
            self._register(result[1] - 1, key, result)
        for w in merged_windows:
            self._delete(w[1] - 1, key, w)                    # trigger.clear
            ct = self._cleanup_time(w[1])
            if ct != LONG_MAX:
                self._delete(ct, key, w)                      # deleteCleanupTimer
        merged = None  # AbstractHeapMergingState.mergeNamespaces
        for sw in merged_state_windows:
            src = self.state.pop((key, sw), None)
            if src is None:
                continue
            merged = src if merged is None else self.agg.merge(merged, src)
        if merged is not None:
            tgt = self.state.get((key, state_window))
            self.state[(key, state_window)] = merged if tgt is None else self.agg.merge(tgt, merged)

    def _emit(self, key, w, acc):
        self.rows.append((key, w[0], w[1], self.agg.result_bits(acc)))

    # ---- WindowOperator.processElement, merging branch ----
    def process_element(self, key, ts, value, value_bits, gap):
        if ts == LONG_MIN:
            raise ValueError("Record has Long.MIN_VALUE timestamp (= no timestamp marker).")
        if gap <= 0:
            raise ValueError(BAD_GAP)
        if ts + gap > LONG_MAX:
            raise OverflowError("session window end overflows int64")
        mapping = self.sets.setdefault(key, {})
        actual = self._add_window(key, mapping, (ts, ts + gap))
        if self._is_window_late(actual):
            del mapping[actual]  # retireWindow
            # isSkippedElement && isElementLate (ts + lateness <= wm follows from the late window)
            self.late_records += 1
            if self.side_output:
                self.late_out.append((key, ts, value_bits))
            else:
                self.late_dropped += 1
            return
        if len(mapping) > self.peak_sessions:
            self.peak_sessions = len(mapping)
        sk = (key, mapping[actual])
        acc = self.state.get(sk)
        one = self.agg.first(value)
        self.state[sk] = one if acc is None else self.agg.merge(acc, one)
        if actual[1] - 1 <= self.wm:  # EventTimeTrigger.onElement: FIRE
            self.fired_on_element += 1
            self._emit(key, actual, self.state[sk])
            if self.purging:
                del self.state[sk]
        else:
            self._register(actual[1] - 1, key, actual)
        ct = self._cleanup_time(actual[1])
        if ct != LONG_MAX:
            self._register(ct, key, actual)

    def process_batch(self, keys, ts, value_bits, gaps):
        keys = np.asarray(keys, dtype=np.int64)
        n = len(keys)
        ts = np.asarray(ts, dtype=np.int64)
        gaps = np.asarray(gaps, dtype=np.int64)
        if value_bits is None:
            bits = np.zeros(n, np.int64)
        else:
            bits = np.ascontiguousarray(value_bits).view(np.int64)
        vals = bits.view(np.float64).tolist() if self.agg.double_in else bits.tolist()
        bl = bits.tolist()
        for k, t, v, b, g in zip(keys.tolist(), ts.tolist(), vals, bl, gaps.tolist()):
            self.process_element(k, t, v, b, g)

    # ---- WindowOperator.onEventTime ----
    def process_watermark(self, wm):
        if wm <= self.wm:
            return
        self.wm = wm
        while self.heap and self.heap[0][0] <= wm:
            t = heapq.heappop(self.heap)
            if t not in self.timers:
                continue
            self.timers.discard(t)
            time, key, w = t
            mapping = self.sets.get(key)
            if not mapping or w not in mapping:
                continue  # a timer of a window that no longer exists
            sk = (key, mapping[w])
            if time == w[1] - 1:  # EventTimeTrigger.onEventTime: FIRE
                acc = self.state.get(sk)
                if acc is not None:
                    self._emit(key, w, acc)
                if self.purging:
                    self.state.pop(sk, None)
            if time == self._cleanup_time(w[1]):  # clearAllState
                self.state.pop(sk, None)
                self._delete(w[1] - 1, key, w)
                del mapping[w]

    def restore(self):
        """A restore from a snapshot taken now: all keyed state (sessions, accumulators, timers)
        stays, the watermark is not part of the state and starts again at Long.MIN_VALUE."""
        self.wm = LONG_MIN

    # ---- output ----
    def drain(self):
        rows, self.rows = self.rows, []
        cols = [np.array([r[c] for r in rows], dtype=np.int64) for c in range(4)]
        return tuple(cols)

    def drain_late(self):
        out, self.late_out = self.late_out, []
        return tuple(np.array([r[c] for r in out], dtype=np.int64) for c in range(3))

    def sessions(self, key):
        """The key's in-flight windows, ascending."""
        return sorted(self.sets.get(key, {}))

    def counters(self):
        return dict(late=self.late_records, merges=self.merges, peak_sessions=self.peak_sessions,
                    fired_on_element=self.fired_on_element)


# ---- the streams and vectors shared by the CPU pin and the GPU tests ----
def gap_column(keys, seed, base, short, long, p=0.15):
    """base[key % 4] per record; a fraction p of the records gets `short`, another p `long`."""
    keys = np.asarray(keys, dtype=np.int64)
    g = np.asarray(base, dtype=np.int64)[keys % 4]
    r = np.random.default_rng(seed).random(len(keys))
    g = np.where(r < p, np.int64(short), g)
    g = np.where(r > 1 - p, np.int64(long), g)
    return g.astype(np.int64)


def stream_s1(agg="sum_i64"):
    """S1, many sessions per key: 60 000 records over 500 keys in six batches, each followed by
    the watermark (max ts so far) - 3001."""
    rng = np.random.default_rng(11)
    n = 60_000
    keys = rng.integers(0, 500, n).astype(np.int64)
    ts = np.sort(rng.integers(0, 3_000_000, n)).astype(np.int64) - rng.integers(0, 40_000, n)
    vals = values_for(rng, n, agg)
    batches = [(lo, lo + 10_000, int(ts[:lo + 10_000].max()) - 3001) for lo in range(0, n, 10_000)]
    return keys, ts, vals, batches


def values_for(rng, n, agg):
    if agg in DOUBLE_INPUT:
        return rng.uniform(0.0, 1000.0, n).astype(np.float64)
    return rng.integers(-(10 ** 6), 10 ** 6, n).astype(np.int64)


def run_reference(keys, ts, vals, gaps, batches, agg, lateness=0, trigger="event_time", side_output=False,
                  final_wm=LONG_MAX, restore_after=None):
    """Per-watermark rows of the reference over the batches (and the final watermark), the
    operator itself for its counters.  restore_after: restore() after that batch's watermark."""
    op = DynamicSessionOperator(agg, lateness, trigger, side_output)
    vb = None if vals is None else (vals.view(np.int64) if vals.dtype == np.float64 else vals)
    outs = []
    for b, (lo, hi, wm) in enumerate(batches):
        op.process_batch(keys[lo:hi], ts[lo:hi], None if vb is None else vb[lo:hi], gaps[lo:hi])
        op.process_watermark(wm)
        outs.append(op.drain())
        if restore_after is not None and b == restore_after:
            op.restore()
    if final_wm is not None:
        op.process_watermark(final_wm)
        outs.append(op.drain())
    return outs, op


# (name, lateness, steps, expected) -- steps: ("e", ts, gap) an element of key 7 with value 1,
# ("w", watermark); expected: the rows (start, end, count) fired in order, the late count and
# the key's in-flight sessions at the end.
VECTORS = [
    # one long-gap element bridges two sessions
    ("bridging", 0, [("e", 0, 10), ("e", 30, 10), ("e", 5, 30)],
     dict(rows=[], late=0, sessions=[(0, 40)], merges=1)),
    # an element's window lies strictly inside a session and extends nothing
    ("contained", 0, [("e", 0, 100), ("e", 10, 1)],
     dict(rows=[], late=0, sessions=[(0, 100)], merges=0)),
    # TimeWindow.intersects is inclusive: touching windows merge
    ("touching", 0, [("e", 0, 10), ("e", 10, 5)],
     dict(rows=[], late=0, sessions=[(0, 15)], merges=0)),
    # same timestamp, late by the gap alone: [90, 95) has max timestamp 94 <= 100, [90, 140) not
    ("late_by_gap_alone", 0, [("w", 100), ("e", 90, 5), ("e", 90, 50)],
     dict(rows=[], late=1, sessions=[(90, 140)], merges=0)),
    # under lateness 20 the fired session [80, 100) is kept until 119: (90, 5) merges into it
    # and the merged window fires at once
    ("merge_into_fired_kept", 20, [("e", 80, 20), ("w", 100), ("e", 90, 5)],
     dict(rows=[(80, 100, 1), (80, 100, 2)], late=0, sessions=[(80, 100)], merges=0)),
]
VECTOR_KEY = 7
