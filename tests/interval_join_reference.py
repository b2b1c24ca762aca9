"""The interval-join contract of include/gpuwin.h (gw_interval_join_*, gw_ijoin_*) restated twice
in plain Python, from the contract's text: Flink's keyedA.intervalJoin(keyedB).between(lower,
upper).process(), i.e. IntervalJoinOperator.

  IntervalJoinSim   element at a time, as the operator is written: per side and key a map
                    ts -> list, processElement's scan of the other side's map, the late test, and
                    the cleanup timers run by the watermark;
  closed_form       no buffers and no timers: a pair is emitted iff it is inside the bounds, both
                    records were not late, and the watermark at the later arrival is below the
                    earlier record's cleanup time -- or is still the watermark the earlier record
                    arrived on: a timer registered at or below the current watermark fires at the
                    next watermark that advances (InternalTimerServiceImpl.advanceWatermark), so
                    a record with ts == w and cleanup time w stays until then.

Python integers do not wrap, so "beyond int64" is tested on the true value.
"""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MAX_BOUND = 1 << 62
LEFT, RIGHT = 0, 1
COLUMNS = ("key", "left ts", "right ts", "left payload", "right payload")


class NoTimestamp(Exception):
    pass


class BoundRange(Exception):
    pass


class Failed(Exception):
    """A call on an operator after one of its calls failed."""


def check_bounds(lower, upper):
    if lower > upper or lower < -MAX_BOUND or upper > MAX_BOUND:
        raise ValueError("-2^62 <= lower <= upper <= 2^62")


def exclusive_bounds(lower, upper, lower_exclusive=False, upper_exclusive=False):
    """IntervalJoined.lowerBoundExclusive / upperBoundExclusive: lower + 1 / upper - 1, checked
    afterwards."""
    lower, upper = lower + bool(lower_exclusive), upper - bool(upper_exclusive)
    check_bounds(lower, upper)
    return lower, upper


def relative(side, lower, upper):
    """The other side's timestamps a record of `side` at ts meets: [ts + lo, ts + hi]."""
    return (lower, upper) if side == LEFT else (-upper, -lower)


def cleanup_time(side, ts, lower, upper):
    """processElement1 / 2's cleanup timer."""
    if side == LEFT:
        return ts + upper if upper > 0 else ts
    return ts - lower if lower < 0 else ts


def _empty():
    return tuple(np.empty(0, np.int64) for _ in range(5))


def _rows(side, probe, probe_ids, counts, other, partner_ids):
    """Rows of probes (ids into the `probe` columns, `counts` partners each) and their partners
    (ids into the `other` columns, concatenated)."""
    if not partner_ids:
        return _empty()
    pi = np.repeat(np.asarray(probe_ids, np.int64), np.asarray(counts, np.int64))
    oi = np.asarray(partner_ids, np.int64)
    pk, pt, pp = (np.asarray(c, np.int64)[pi] for c in probe)
    _, ot, op = (np.asarray(c, np.int64)[oi] for c in other)
    return (pk, pt, ot, pp, op) if side == LEFT else (pk, ot, pt, op, pp)


class IntervalJoinSim:
    """IntervalJoinOperator, element at a time.  ingest() returns the call's rows as five int64
    columns: the call's records in arrival order, each one's partners by ascending (ts, arrival)."""

    def __init__(self, lower, upper):
        check_bounds(lower, upper)
        self.lower, self.upper = lower, upper
        self.wm = I64_MIN
        self.late_dropped = 0
        self.rows_emitted = 0
        self.failed = False
        self.buf = ({}, {})                       # per side: key -> {ts: [record ids, arrival order]}
        self.rec = ([[], [], []], [[], [], []])   # per side: key, ts, payload by record id

    def _alive(self):
        if self.failed:
            raise Failed()

    def ingest(self, side, key, ts, pay):
        self._alive()
        key, ts, pay = (np.asarray(c).tolist() for c in (key, ts, pay))
        lo, hi = relative(side, self.lower, self.upper)
        # the whole call is checked before any of it is taken
        try:
            if any(t == I64_MIN for t in ts):
                raise NoTimestamp()
            for t in ts:
                if not self._late(t) and not (I64_MIN <= t + lo and t + hi <= I64_MAX):
                    raise BoundRange(t)
        except (NoTimestamp, BoundRange):
            self.failed = True
            raise
        own, other = self.buf[side], self.buf[1 - side]
        rk, rt, rp = self.rec[side]
        probe_ids, counts, partner_ids = [], [], []
        for k, t, p in zip(key, ts, pay):
            if self._late(t):
                self.late_dropped += 1
                continue
            rid = len(rk)
            rk.append(k); rt.append(t); rp.append(p)
            own.setdefault(k, {}).setdefault(t, []).append(rid)
            bucket = other.get(k)
            if not bucket:
                continue
            # Flink walks the map's entries; a HashMap's order is unspecified, the contract's is
            # ascending ts (the lists are in arrival order)
            if hi - lo + 1 < len(bucket):
                hits = [t2 for t2 in range(t + lo, t + hi + 1) if t2 in bucket]
            else:
                hits = sorted(t2 for t2 in bucket if t + lo <= t2 <= t + hi)
            n0 = len(partner_ids)
            for t2 in hits:
                partner_ids.extend(bucket[t2])
            if len(partner_ids) > n0:
                probe_ids.append(rid)
                counts.append(len(partner_ids) - n0)
        out = _rows(side, self.rec[side], probe_ids, counts, self.rec[1 - side], partner_ids)
        self.rows_emitted += len(out[0])
        return out

    def _late(self, t):
        return self.wm != I64_MIN and t < self.wm

    def advance_watermark(self, wm):
        """onEventTime for every cleanup timer <= wm; a watermark that does not advance is ignored."""
        self._alive()
        if wm <= self.wm:
            return
        for side in (LEFT, RIGHT):
            for k in list(self.buf[side]):
                bucket = self.buf[side][k]
                for t in [t for t in bucket if cleanup_time(side, t, self.lower, self.upper) <= wm]:
                    del bucket[t]
                if not bucket:
                    del self.buf[side][k]
        self.wm = wm

    def end_input(self):
        self.advance_watermark(I64_MAX)

    def live(self, side):
        return sum(len(ids) for bucket in self.buf[side].values() for ids in bucket.values())

    def log(self, side):
        """The live records of `side` as the device keeps them: by (key, ts), equal ones in
        arrival order; three columns."""
        ids = sorted((k, t, rid) for k, bucket in self.buf[side].items() for t, rids in bucket.items() for rid in rids)
        ids = [rid for _, _, rid in ids]
        return tuple(np.asarray(c, np.int64)[ids] if ids else np.empty(0, np.int64) for c in self.rec[side])


def closed_form(lower, upper, events):
    """events: ("ingest", side, key, ts, payload) and ("watermark", w) in order (valid inputs: no
    Long.MIN_VALUE timestamp, nothing beyond int64).  Per ingest call its rows as five columns and
    the number of late records, from the closed form alone."""
    check_bounds(lower, upper)
    wm = I64_MIN
    seen = ([], [])  # per side: (key, ts, payload, cleanup time) of the earlier calls' records that were not late
    out = []
    for ev in events:
        if ev[0] == "watermark":
            wm = max(wm, ev[1])
            continue
        _, side, key, ts, pay = ev
        key, ts, pay = (np.asarray(c, np.int64) for c in (key, ts, pay))
        on_time = np.ones(len(ts), bool) if wm == I64_MIN else ts >= wm
        key, ts, pay = key[on_time], ts[on_time], pay[on_time]
        if seen[1 - side]:
            ok, ot, op, oc, ow = (np.concatenate(c) for c in zip(*seen[1 - side]))
        else:
            ok = ot = op = oc = ow = np.empty(0, np.int64)
        # (Python integers: the cleanup times and arrival watermarks are objects)
        alive = np.array([c > wm or w == wm for c, w in zip(oc.tolist(), ow.tolist())], bool)
        lo, hi = relative(side, lower, upper)
        rows = [[], [], [], [], []]
        for k, t, p in zip(key.tolist(), ts.tolist(), pay.tolist()):
            m = np.nonzero((ok == k) & (ot >= max(t + lo, I64_MIN)) & (ot <= min(t + hi, I64_MAX)) & alive)[0]
            m = m[np.argsort(ot[m], kind="stable")]  # candidates are in arrival order
            for j in m.tolist():
                l, r = ((t, p), (int(ot[j]), int(op[j])))[::1 if side == LEFT else -1]
                for c, v in zip(rows, (k, l[0], r[0], l[1], r[1])):
                    c.append(v)
        clean = np.array([cleanup_time(side, t, lower, upper) for t in ts.tolist()], object)
        seen[side].append((key, ts, pay, clean, np.array([wm] * len(ts), object)))
        out.append((tuple(np.array(c, np.int64) for c in rows), int((~on_time).sum())))
    return out


def reference_call(probe_side, probe, build, lower, upper):
    """The stateless contract: one ingest call of `probe` against a buffer holding `build` (the
    other side's records in arrival order), no watermark."""
    sim = IntervalJoinSim(lower, upper)
    if len(build[0]) == 0 or len(probe[0]) == 0:
        return _empty()
    sim.ingest(1 - probe_side, *build)
    return sim.ingest(probe_side, *probe)


SPECIAL_KEYS = [I64_MIN, -1, 0, I64_MAX]


def key_table(rng, n):
    """n distinct keys: the four the contract names, then random int64s."""
    extra = rng.integers(I64_MIN, I64_MAX, max(0, n - 4), dtype=np.int64, endpoint=True)
    return np.concatenate([np.array(SPECIAL_KEYS, np.int64), extra])[:max(n, 1)]


def make_records(seed, n, num_keys, ts_lo=-40, ts_span=100):
    """Seeded (key, ts, payload) columns: keys drawn from num_keys distinct values (INT64_MIN, -1,
    0 and INT64_MAX among them), timestamps uniform in [ts_lo, ts_lo + ts_span), random payloads."""
    rng = np.random.default_rng(seed)
    table = key_table(np.random.default_rng(num_keys), num_keys)  # one table per num_keys: both sides draw from it
    key = table[rng.integers(0, len(table), n)]
    ts = rng.integers(ts_lo, ts_lo + ts_span, n).astype(np.int64)
    pay = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    return key, ts, pay


def make_stream(seed, calls=14, num_keys=5, max_batch=40, step=8, disorder=16, lag=12):
    """A seeded two-input schedule: ingest calls of random side and size whose timestamps follow a
    clock advancing `step` per call with `disorder` behind it, and after about half of the calls a
    watermark `lag` behind the clock -- so some records are late, some partners already cleaned."""
    rng = np.random.default_rng(seed)
    table = key_table(rng, num_keys)
    events, clock, serial = [], 0, 0
    for _ in range(calls):
        side = int(rng.integers(0, 2))
        n = int(rng.integers(0, max_batch + 1))
        key = table[rng.integers(0, len(table), n)]
        ts = (clock - rng.integers(0, disorder + 1, n)).astype(np.int64)
        pay = np.arange(serial, serial + n, dtype=np.int64) * 2 + side
        serial += n
        events.append(("ingest", side, key, ts, pay))
        clock += int(rng.integers(0, step + 1))
        if rng.random() < 0.5:
            events.append(("watermark", clock - int(rng.integers(0, 2 * lag + 1))))  # (may not advance)
    events.append(("watermark", I64_MAX))
    return events


def check(got, want):
    """Exact, in order and values."""
    assert len(got) == 5
    for c, name in enumerate(COLUMNS):
        g, w = np.asarray(got[c]), np.asarray(want[c])
        assert len(g) == len(w), f"{len(g)} rows, expected {len(w)}"
        if not np.array_equal(g, w):
            i = int(np.nonzero(g != w)[0][0])
            raise AssertionError(f"{name} differs at row {i}: {int(g[i])} vs {int(w[i])}")
