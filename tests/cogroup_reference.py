"""The coGroup / outer-join contract of include/gpuwin.h (gw_window_join_outer_*,
gw_window_cogroup_*, gw_join_set_mode) restated in plain Python, from the contract's text:
CoGroupedStreams is union -> keyBy -> WindowOperator with ListState, and at the fire
CoGroupFunction.coGroup sees every (key, window) with a record on either side.  The outer modes
are the CoGroupFunctions "cross product, or the kept side alone with a null partner".
"""
import numpy as np

from tests.join_reference import (I64_MAX, I64_MIN, NoTimestamp, Unsupported, WindowRange,  # noqa: F401
                                  check_geometry, make_records, window_starts)

INNER, LEFT_OUTER, RIGHT_OUTER, FULL_OUTER, COGROUP = 0, 1, 2, 3, 4
MODES = {"inner": INNER, "left_outer": LEFT_OUTER, "right_outer": RIGHT_OUTER, "full_outer": FULL_OUTER}
NULL = -7_777_777_777  # the null_payload the tests pass (`present`, not this value, tells the rows apart)


def fired_groups(left, right, size, slide, offset, w0=I64_MIN, w1=I64_MAX):
    """{(start, key): ([left payloads], [right payloads])} of the windows with w0 < end - 1 <= w1,
    each side in arrival order."""
    check_geometry(size, slide, offset)
    groups = {}
    for side, (key, ts, pay) in enumerate((left, right)):
        for k, t, p in zip(np.asarray(key).tolist(), np.asarray(ts).tolist(), np.asarray(pay).tolist()):
            _, starts = window_starts(t, size, slide, offset)
            for s in starts:
                if w0 < s + size - 1 <= w1:
                    groups.setdefault((s, k), ([], []))[side].append(p)
    return groups


def _i64(rows):
    return np.array(rows, np.int64) if rows else np.empty(0, np.int64)


def emit_rows(groups, size, mode, null=NULL):
    """The rows of `mode`: (key, start, end, left payload, right payload, present), windows by
    ascending end, keys ascending, left-major; a one-sided group's rows in arrival order."""
    assert mode in (INNER, LEFT_OUTER, RIGHT_OUTER, FULL_OUTER)
    cols = [[], [], [], [], [], []]

    def row(key, start, lp, rp, pres):
        for c, v in zip(cols, (key, start, start + size, lp, rp, pres)):
            c.append(v)

    for (start, key) in sorted(groups):
        l, r = groups[(start, key)]
        if l and r:
            for x in l:
                for y in r:
                    row(key, start, x, y, 3)
        elif l and mode & 1:
            for x in l:
                row(key, start, x, null, 1)
        elif r and mode & 2:
            for y in r:
                row(key, start, null, y, 2)
    return tuple(_i64(c) for c in cols[:5]) + (np.array(cols[5], np.uint8),)


def emit_csr(groups, size):
    """(key, start, end, loff, roff, lelem, relem): every group, one-sided ones included."""
    key, start, end, loff, roff, le, re = [], [], [], [0], [0], [], []
    for (s, k) in sorted(groups):
        l, r = groups[(s, k)]
        key.append(k)
        start.append(s)
        end.append(s + size)
        le += l
        re += r
        loff.append(len(le))
        roff.append(len(re))
    return tuple(_i64(c) for c in (key, start, end, loff, roff, le, re))


def reference_rows(left, right, size, slide, offset, mode, null=NULL, w0=I64_MIN, w1=I64_MAX):
    return emit_rows(fired_groups(left, right, size, slide, offset, w0, w1), size, mode, null)


def reference_csr(left, right, size, slide, offset, w0=I64_MIN, w1=I64_MAX):
    return emit_csr(fired_groups(left, right, size, slide, offset, w0, w1), size)


def expand_csr(csr):
    """The CSR expanded by JoinCoGroupFunction's nested loop: the inner join's five columns."""
    key, start, end, loff, roff, le, re = csr
    cols = [[], [], [], [], []]
    for g in range(len(key)):
        for x in le[loff[g]:loff[g + 1]].tolist():
            for y in re[roff[g]:roff[g + 1]].tolist():
                for c, v in zip(cols, (int(key[g]), int(start[g]), int(end[g]), x, y)):
                    c.append(v)
    return tuple(_i64(c) for c in cols)


def concat_csr(parts):
    """Several fires' CSRs as the one an operator accumulates: offsets rebased by the totals."""
    out = [np.concatenate([p[c] for p in parts]) if parts else np.empty(0, np.int64) for c in (0, 1, 2)]
    loff, roff, nl, nr = [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], 0, 0
    for p in parts:
        loff.append(p[3][1:] + nl)
        roff.append(p[4][1:] + nr)
        nl += len(p[5])
        nr += len(p[6])
    le = np.concatenate([p[5] for p in parts]) if parts else np.empty(0, np.int64)
    re = np.concatenate([p[6] for p in parts]) if parts else np.empty(0, np.int64)
    return tuple(out) + (np.concatenate(loff), np.concatenate(roff), le, re)


class ReferenceCoGroupOperator:
    """The stateful contract with a mode: a list per (key, window) and side, late records dropped
    and counted whatever the mode, windows fired by the watermark.  advance_watermark returns the
    mode's rows (six columns), or in COGROUP mode the fire's CSR (offsets from 0)."""

    def __init__(self, size, slide, offset=0, mode=INNER, null=NULL):
        check_geometry(size, slide, offset)
        self.size, self.slide, self.offset, self.mode, self.null = size, slide, offset, mode, null
        self.wm = I64_MIN
        self.state = {}
        self.late_dropped = 0
        self.fired = 0  # rows, or groups in COGROUP mode

    def ingest(self, side, key, ts, pay):
        for k, t, p in zip(np.asarray(key).tolist(), np.asarray(ts).tolist(), np.asarray(pay).tolist()):
            ls, starts = window_starts(t, self.size, self.slide, self.offset)
            if ls + self.size - 1 <= self.wm:
                self.late_dropped += 1
                continue
            for s in starts:
                if s + self.size - 1 > self.wm:  # a window that has passed never sees the record
                    self.state.setdefault((s, k), ([], []))[side].append(p)

    def _emit(self, groups):
        if self.mode == COGROUP:
            return emit_csr(groups, self.size)
        return emit_rows(groups, self.size, self.mode, self.null)

    def advance_watermark(self, wm):
        self.last_fired = {}
        if wm <= self.wm:
            return self._emit({})
        fire = {g: v for g, v in self.state.items() if self.wm < g[0] + self.size - 1 <= wm}
        for g in fire:
            del self.state[g]
        self.last_fired = {g: (len(v[0]), len(v[1])) for g, v in fire.items()}
        self.wm = wm
        out = self._emit(fire)
        self.fired += len(out[0])
        return out

    def end_input(self):
        return self.advance_watermark(I64_MAX)

    def live_records(self, side):
        return len({p for v in self.state.values() for p in v[side]})


ROW_NAMES = ("key", "start", "end", "left payload", "right payload", "present")
CSR_NAMES = ("key", "start", "end", "loff", "roff", "left elements", "right elements")


def _check(got, want, names):
    assert len(got) == len(want) == len(names)
    for c, name in enumerate(names):
        g, w = np.asarray(got[c]), np.asarray(want[c])
        assert len(g) == len(w), f"{name}: {len(g)} entries, expected {len(w)}"
        if not np.array_equal(g, w):
            i = int(np.nonzero(g != w)[0][0])
            raise AssertionError(f"{name} differs at {i}: {int(g[i])} vs {int(w[i])}")


def check_rows(got, want):
    """Exact, in order and values; `present` too when got has it."""
    n = len(got)
    assert n in (5, 6)
    _check(got, want[:n], ROW_NAMES[:n])


def check_csr(got, want):
    _check(got, want, CSR_NAMES)
