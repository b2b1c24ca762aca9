"""Host-side mirror of the reference's keyed event-time window operator interface.

Names, argument meaning and error behaviour follow Flink's DataStream windowing API
so a job (or a harness test) reads the same:

  * assigners   TumblingEventTimeWindows.of / SlidingEventTimeWindows.of /
                EventTimeSessionWindows.with_gap / DynamicEventTimeSessionWindows.with_dynamic_gap
                (flink-runtime/.../streaming/api/windowing/assigners/*.java,
                 flink-streaming-java/.../EventTimeSessionWindows.java)
  * triggers    EventTimeTrigger.create(), PurgingTrigger.of(...)
  * operator    GpuWindowOperator — the OneInputStreamOperator slot of WindowOperator
                (RS/runtime/operators/windowing/WindowOperator.java:102): open,
                process_element, process_watermark, end_input, close.  Records between
                two watermarks are batched into columns and handed to libgpuwin.so in one
                gw_ingest call; process_watermark fires through gw_advance_watermark.
  * errors      invalid configurations raise ValueError (IllegalArgumentException in
                the reference), runtime failures raise GpuWinError (the task fails).

Every call goes to the HIP library; there is no CPU path here.
"""
from __future__ import annotations

import contextlib
import ctypes
import struct
import time
from dataclasses import dataclass
from typing import Any, Callable, Iterable, List, Optional

import numpy as np

from . import _native as N

LONG_MIN = -(1 << 63)
LONG_MAX = (1 << 63) - 1


# --------------------------------------------------------------------------- time
class Duration:
    """java.time.Duration stand-in: milliseconds."""

    @staticmethod
    def of_millis(ms: int) -> int:
        return int(ms)

    @staticmethod
    def of_seconds(s: int) -> int:
        return int(s) * 1000

    @staticmethod
    def of_minutes(m: int) -> int:
        return int(m) * 60_000


# ---------------------------------------------------------------------- assigners
class WindowAssigner:
    kind = ""

    def config(self) -> dict:
        raise NotImplementedError


class WindowStagger:
    """WindowStagger (RS/api/windowing/assigners/WindowStagger.java:27-60): ALIGNED (0), RANDOM
    (U(0, size)) or NATURAL (the processing time's offset into its window), drawn at the first
    element; gw_window_stagger_offset computes the resulting window offset."""
    ALIGNED, RANDOM, NATURAL = 0, 1, 2

    @staticmethod
    def window_offset(stagger: int, processing_time: int, size: int, global_offset: int,
                      random01: Optional[float] = None) -> int:
        """(global_offset + stagger offset) % size, as TumblingEventTimeWindows.assignWindows
        uses it (TumblingEventTimeWindows.java:72-79)."""
        import random
        r = random.random() if random01 is None else float(random01)
        out = ctypes.c_int64(0)
        N.check(N.lib().gw_window_stagger_offset(int(stagger), int(processing_time), r, int(size), int(global_offset),
                                                 ctypes.byref(out)))
        return out.value


class TumblingEventTimeWindows(WindowAssigner):
    """TumblingEventTimeWindows.of(size[, offset[, stagger]])."""
    kind = "tumbling"

    def __init__(self, size: int, offset: int = 0, stagger: int = WindowStagger.ALIGNED):
        if abs(offset) >= size:  # TumblingEventTimeWindows.java:55-62
            raise ValueError("TumblingEventTimeWindows parameters must satisfy abs(offset) < size")
        self.size, self.offset, self.stagger = int(size), int(offset), int(stagger)

    @staticmethod
    def of(size: int, offset: int = 0, stagger: int = WindowStagger.ALIGNED) -> "TumblingEventTimeWindows":
        return TumblingEventTimeWindows(size, offset, stagger)

    def config(self):
        return dict(assigner="tumbling", size=self.size, slide=self.size, offset=self.offset)


class SlidingEventTimeWindows(WindowAssigner):
    kind = "sliding"
    MAX_WINDOW_NUM = 10_000_000

    def __init__(self, size: int, slide: int, offset: int = 0):
        if abs(offset) >= slide or size <= 0:  # SlidingEventTimeWindows.java:57-70
            raise ValueError("SlidingEventTimeWindows parameters must satisfy abs(offset) < slide and size > 0")
        if size // slide > self.MAX_WINDOW_NUM:
            raise ValueError(f"SlidingEventTimeWindows parameters must satisfy size / slide <= {self.MAX_WINDOW_NUM}")
        self.size, self.slide, self.offset = int(size), int(slide), int(offset)

    @staticmethod
    def of(size: int, slide: int, offset: int = 0) -> "SlidingEventTimeWindows":
        return SlidingEventTimeWindows(size, slide, offset)

    def config(self):
        return dict(assigner="sliding", size=self.size, slide=self.slide, offset=self.offset)


class EventTimeSessionWindows(WindowAssigner):
    kind = "session"

    def __init__(self, gap: int):
        if gap <= 0:  # EventTimeSessionWindows.java:52-53
            raise ValueError("EventTimeSessionWindows parameters must satisfy 0 < size")
        self.gap = int(gap)

    @staticmethod
    def with_gap(gap: int) -> "EventTimeSessionWindows":
        return EventTimeSessionWindows(gap)

    withGap = with_gap

    def config(self):
        return dict(assigner="session", gap=self.gap)


class DynamicEventTimeSessionWindows(WindowAssigner):
    """DynamicEventTimeSessionWindows.withDynamicGap(extractor): the element's window is
    [timestamp, timestamp + extractor(element)) (flink-streaming-java/.../assigners/
    DynamicEventTimeSessionWindows.java).  The operator evaluates the extractor per element
    (process_element) or takes the gaps as a column (process_batch(..., gaps=))."""
    kind = "session_dynamic"

    def __init__(self, extractor: Callable[[Any], int]):
        if extractor is None:
            raise ValueError("a session gap extractor is required")
        self.extractor = extractor

    @staticmethod
    def with_dynamic_gap(extractor: Callable[[Any], int]) -> "DynamicEventTimeSessionWindows":
        return DynamicEventTimeSessionWindows(extractor)

    withDynamicGap = with_dynamic_gap

    def config(self):
        return dict(assigner="session_dynamic")


class CountWindows(WindowAssigner):
    """KeyedStream.countWindow(size[, slide]) — GlobalWindows with
    PurgingTrigger(CountTrigger(size)), or CountEvictor(size) + CountTrigger(slide)
    (RS/api/datastream/KeyedStream.java:676-690).  Rows are (key, first element ordinal,
    end ordinal, result) and come out of process_batch itself."""
    kind = "count"

    def __init__(self, size: int, slide: Optional[int] = None):
        if size <= 0 or (slide is not None and slide <= 0):
            raise ValueError("count windows need size > 0 and slide > 0")
        self.size, self.slide = int(size), (int(slide) if slide is not None else None)

    @staticmethod
    def of(size: int, slide: Optional[int] = None) -> "CountWindows":
        return CountWindows(size, slide)

    def config(self):
        if self.slide is None:
            return dict(assigner="count_tumbling", size=self.size, slide=self.size)
        return dict(assigner="count_sliding", size=self.size, slide=self.slide)


# ----------------------------------------------------------------------- triggers
class EventTimeTrigger:
    name = "event_time"

    @staticmethod
    def create() -> "EventTimeTrigger":
        return EventTimeTrigger()


class PurgingTrigger:
    def __init__(self, nested):
        if not isinstance(nested, EventTimeTrigger):
            raise ValueError("only PurgingTrigger.of(EventTimeTrigger) is on the GPU path")
        self.name = "purging_event_time"

    @staticmethod
    def of(nested) -> "PurgingTrigger":
        return PurgingTrigger(nested)


# ------------------------------------------------------------------ stream elements
@dataclass
class StreamRecord:
    value: Any
    timestamp: int


@dataclass
class Watermark:
    timestamp: int


MAX_WATERMARK = Watermark(LONG_MAX)


def java_string_hash(s: str) -> int:
    """JDK String.hashCode (UTF-16 code units, int arithmetic)."""
    h = 0
    data = s.encode("utf-16-le")
    for i in range(0, len(data), 2):
        h = (31 * h + (data[i] | (data[i + 1] << 8))) & 0xFFFFFFFF
    return h - (1 << 32) if h >= (1 << 31) else h


def java_hash(key) -> int:
    """key.hashCode() for the key types the path supports."""
    if isinstance(key, bool):
        return 1231 if key else 1237
    if isinstance(key, int):
        if -(1 << 31) <= key < (1 << 31):
            return key  # Integer.hashCode
        return N.lib().gw_java_long_hash(key)
    if isinstance(key, str):
        return java_string_hash(key)
    raise TypeError(f"unsupported key type {type(key).__name__}")


def assign_to_key_group(key, max_parallelism: int) -> int:
    """KeyGroupRangeAssignment.assignToKeyGroup (bit-exact, via libgpuwin.so)."""
    return N.lib().gw_key_group_for_hash(java_hash(key), max_parallelism)


def compute_operator_index_for_key_group(max_parallelism: int, parallelism: int, key_group: int) -> int:
    return N.lib().gw_operator_for_key_group(max_parallelism, parallelism, key_group)


def compute_key_group_range_for_operator_index(max_parallelism: int, parallelism: int, index: int):
    """KeyGroupRangeAssignment.computeKeyGroupRangeForOperatorIndex (:93-106)."""
    start = (index * max_parallelism + parallelism - 1) // parallelism
    end = ((index + 1) * max_parallelism - 1) // parallelism
    return start, end


def compute_default_max_parallelism(parallelism: int) -> int:
    return N.lib().gw_default_max_parallelism(parallelism)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def select_lookup_device(sel, sel_value: int, idx, dictionary, ts, key_out, ts_out, stream) -> int:
    """gw_select_lookup_device over device tensors (int64): the records with sel == sel_value,
    in arrival order, as (dictionary[idx], ts) into key_out / ts_out; returns their number.  The
    filter + projection + static-table join a job chains ahead of keyBy (YSB's view filter
    and ad -> campaign join), fused on the device."""
    n_out = ctypes.c_int64(0)
    N.check(N.lib().gw_select_lookup_device(sel.numel(), sel.data_ptr(), int(sel_value), idx.data_ptr(),
                                             dictionary.data_ptr(), dictionary.numel(), ts.data_ptr(),
                                             key_out.data_ptr(), ts_out.data_ptr(), ctypes.byref(n_out), stream))
    return int(n_out.value)


def _top_n_mode(smallest: bool, f64: bool) -> int:
    return (N.TOPN_SMALLEST if smallest else 0) | (N.TOPN_F64 if f64 else 0)


def top_n_device(key, start, end, result, top: int, smallest: bool = False, f64: bool = False, stream=None):
    """gw_top_n_device over torch device tensors (8-byte columns of n rows in any order): per
    window (rows sharing `end`) the `top` rows with the largest result (smallest=True: the
    smallest; f64=True: result bits are doubles in Double.compare order), ties to the smaller key,
    windows in ascending end, best first.  Returns device tensors (key, start, end, result,
    win_rows); result has the dtype it came in.  The windowAll top-N stage of Nexmark Q5 / Q7
    behind the keyed window aggregate.  Waits on `stream` (default: torch's current)."""
    import torch
    n = key.numel()
    if stream is None:
        stream = torch.cuda.current_stream(key.device).cuda_stream
    mode = _top_n_mode(smallest, f64)
    n_out = ctypes.c_int64(0)
    cap = min(n, 4096)  # top * windows at most; a retry with the needed size when it is more
    while True:
        out = [torch.empty(cap, dtype=torch.int64, device=key.device) for _ in range(5)]
        rc = N.lib().gw_top_n_device(n, key.data_ptr(), start.data_ptr(), end.data_ptr(), result.data_ptr(), int(top),
                                     mode, *[o.data_ptr() for o in out], cap, ctypes.byref(n_out),
                                     ctypes.c_void_p(stream) if stream else None)
        if rc == N.GW_E_OUTPUT_FULL and n_out.value > cap:
            cap = n_out.value
            continue
        N.check(rc)
        break
    k, s, e, r, w = (o[:n_out.value] for o in out)
    return k, s, e, r.view(result.dtype), w


def top_n_host(key, start, end, result, top: int, smallest: bool = False, f64: bool = False):
    """gw_top_n_host over numpy columns: the contract of top_n_device as pure host code.  A job
    at parallelism > 1 combines its subtasks' top-N lists with it (the keys are partitioned, so
    the top-N of the concatenated lists is the global one).  result: int64 or float64 (f64
    follows from a float64 dtype)."""
    key, start, end = (np.ascontiguousarray(x, dtype=np.int64) for x in (key, start, end))
    result = np.ascontiguousarray(result)
    is_f = result.dtype == np.float64
    bits = result.view(np.int64) if is_f else result.astype(np.int64, copy=False)
    n = len(key)
    if not (len(start) == len(end) == len(bits) == n):
        raise ValueError("column lengths differ")
    mode = _top_n_mode(smallest, f64 or is_f)
    n_out = ctypes.c_int64(0)
    cap = min(n, 4096)
    while True:
        out = [np.empty(cap, np.int64) for _ in range(5)]
        rc = N.lib().gw_top_n_host(n, _ptr(key), _ptr(start), _ptr(end), _ptr(bits), int(top), mode,
                                   *[_ptr(o) for o in out], cap, ctypes.byref(n_out))
        if rc == N.GW_E_OUTPUT_FULL and n_out.value > cap:
            cap = n_out.value
            continue
        N.check(rc)
        break
    k, s, e, r, w = (o[:n_out.value] for o in out)
    return k, s, e, (r.view(np.float64) if is_f else r), w


def _join_geometry(assigner: WindowAssigner):
    """(assigner id, size, slide, offset) of a window join's assigner; session and count windows
    raise as an unsupported configuration does (GW_E_UNSUPPORTED)."""
    a = assigner.config()
    if a["assigner"] not in ("tumbling", "sliding"):
        raise N.GpuWinError(N.GW_E_UNSUPPORTED,
                            "window join: only tumbling and sliding event-time windows (no session or count windows)")
    size = a["size"]
    return N.ASSIGNERS[a["assigner"]], size, a.get("slide", size) if a["assigner"] == "sliding" else size, a.get("offset", 0)


def window_join_device(lkey, lts, lpay, rkey, rts, rpay, assigner: WindowAssigner, w0: int = LONG_MIN,
                       w1: int = LONG_MAX, stream=None):
    """gw_window_join_device over torch device tensors (int64): the left and right records in
    arrival order, the windows firing for a watermark going from w0 to w1.  Returns device tensors
    (key, start, end, left payload, right payload): per fired (window, key) the cross product of
    the two sides, windows by ascending end, keys ascending, left-major in arrival order -- the
    window join of Nexmark Q8.  Waits on `stream` (default: torch's current)."""
    import torch
    _, size, slide, offset = _join_geometry(assigner)
    if stream is None:
        stream = torch.cuda.current_stream(lkey.device).cuda_stream
    n_out = ctypes.c_int64(0)
    cap = max(lkey.numel(), rkey.numel(), 1)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    while True:
        out = [torch.empty(cap, dtype=torch.int64, device=lkey.device) for _ in range(5)]
        rc = N.lib().gw_window_join_device(lkey.numel(), P(lkey), P(lts), P(lpay), rkey.numel(), P(rkey), P(rts), P(rpay),
                                           size, slide, offset, int(w0), int(w1), *[o.data_ptr() for o in out], cap,
                                           ctypes.byref(n_out), ctypes.c_void_p(stream) if stream else None)
        if rc == N.GW_E_OUTPUT_FULL and n_out.value > cap:
            cap = n_out.value
            continue
        N.check(rc)
        break
    return tuple(o[:n_out.value] for o in out)


def window_join_host(lkey, lts, lpay, rkey, rts, rpay, assigner: WindowAssigner, w0: int = LONG_MIN,
                     w1: int = LONG_MAX):
    """gw_window_join_host over numpy columns: the contract of window_join_device as plain host
    code (no device), for a fire of a few records."""
    _, size, slide, offset = _join_geometry(assigner)
    cols = [np.ascontiguousarray(x, dtype=np.int64) for x in (lkey, lts, lpay, rkey, rts, rpay)]
    if not (len(cols[0]) == len(cols[1]) == len(cols[2]) and len(cols[3]) == len(cols[4]) == len(cols[5])):
        raise ValueError("column lengths differ")
    n_out = ctypes.c_int64(0)
    cap = max(len(cols[0]), len(cols[3]), 1)
    while True:
        out = [np.empty(cap, np.int64) for _ in range(5)]
        rc = N.lib().gw_window_join_host(len(cols[0]), *[_ptr(c) for c in cols[:3]], len(cols[3]),
                                         *[_ptr(c) for c in cols[3:]], size, slide, offset, int(w0), int(w1),
                                         *[_ptr(o) for o in out], cap, ctypes.byref(n_out))
        if rc == N.GW_E_OUTPUT_FULL and n_out.value > cap:
            cap = n_out.value
            continue
        N.check(rc)
        break
    return tuple(o[:n_out.value] for o in out)


def _join_mode(mode, cogroup_ok=False) -> int:
    """A GW_JOIN_MODE_* from its number or its name ("inner", "left_outer", "right_outer",
    "full_outer", and for the operator "cogroup")."""
    m = N.JOIN_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= (N.JOIN_MODE_COGROUP if cogroup_ok else 3):
        raise ValueError(f"unknown join mode {mode!r}")
    return m


def window_join_outer_device(lkey, lts, lpay, rkey, rts, rpay, assigner: WindowAssigner, mode="full_outer",
                             null_payload: int = 0, w0: int = LONG_MIN, w1: int = LONG_MAX, stream=None,
                             present: bool = True):
    """gw_window_join_outer_device over torch device tensors: window_join_device in an outer mode.
    Per fired (window, key) the cross product of the two sides, or where one side is empty and the
    mode keeps the other, that side's records with null_payload in the lacking column.  Returns
    (key, start, end, left payload, right payload, present); present (uint8: 1 left only, 2 right
    only, 3 both) is None with present=False."""
    import torch
    _, size, slide, offset = _join_geometry(assigner)
    mode = _join_mode(mode)
    dev = lkey.device if lkey.numel() else rkey.device
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    n_out = ctypes.c_int64(0)
    cap = max(lkey.numel(), rkey.numel(), 1)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    while True:
        out = [torch.empty(cap, dtype=torch.int64, device=dev) for _ in range(5)]
        pres = torch.empty(cap, dtype=torch.uint8, device=dev) if present else None
        rc = N.lib().gw_window_join_outer_device(lkey.numel(), P(lkey), P(lts), P(lpay), rkey.numel(), P(rkey), P(rts),
                                                 P(rpay), size, slide, offset, int(w0), int(w1), mode, int(null_payload),
                                                 *[o.data_ptr() for o in out], pres.data_ptr() if present else None, cap,
                                                 ctypes.byref(n_out), ctypes.c_void_p(stream) if stream else None)
        if rc == N.GW_E_OUTPUT_FULL and n_out.value > cap:
            cap = n_out.value
            continue
        N.check(rc)
        break
    return tuple(o[:n_out.value] for o in out) + (pres[:n_out.value] if present else None,)


def window_join_outer_host(lkey, lts, lpay, rkey, rts, rpay, assigner: WindowAssigner, mode="full_outer",
                           null_payload: int = 0, w0: int = LONG_MIN, w1: int = LONG_MAX):
    """gw_window_join_outer_host over numpy columns: window_join_outer_device as plain host code."""
    _, size, slide, offset = _join_geometry(assigner)
    mode = _join_mode(mode)
    cols = [np.ascontiguousarray(x, dtype=np.int64) for x in (lkey, lts, lpay, rkey, rts, rpay)]
    if not (len(cols[0]) == len(cols[1]) == len(cols[2]) and len(cols[3]) == len(cols[4]) == len(cols[5])):
        raise ValueError("column lengths differ")
    n_out = ctypes.c_int64(0)
    cap = max(len(cols[0]), len(cols[3]), 1)
    while True:
        out = [np.empty(cap, np.int64) for _ in range(5)]
        pres = np.empty(cap, np.uint8)
        rc = N.lib().gw_window_join_outer_host(len(cols[0]), *[_ptr(c) for c in cols[:3]], len(cols[3]),
                                               *[_ptr(c) for c in cols[3:]], size, slide, offset, int(w0), int(w1), mode,
                                               int(null_payload), *[_ptr(o) for o in out], _ptr(pres), cap,
                                               ctypes.byref(n_out))
        if rc == N.GW_E_OUTPUT_FULL and n_out.value > cap:
            cap = n_out.value
            continue
        N.check(rc)
        break
    return tuple(o[:n_out.value] for o in out) + (pres[:n_out.value],)


def window_cogroup_device(lkey, lts, lpay, rkey, rts, rpay, assigner: WindowAssigner, w0: int = LONG_MIN,
                          w1: int = LONG_MAX, stream=None):
    """gw_window_cogroup_device over torch device tensors: every fired (window, key) with a record
    on either side as a CSR.  Returns device tensors (key, start, end, loff, roff, lelem, relem):
    group g's left payloads are lelem[loff[g]:loff[g + 1]] in arrival order, likewise right; what
    CoGroupFunction.coGroup is called with, in the join's order."""
    import torch
    _, size, slide, offset = _join_geometry(assigner)
    dev = lkey.device if lkey.numel() else rkey.device
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    n = (ctypes.c_int64 * 3)()
    caps = [max(lkey.numel() + rkey.numel(), 1), max(lkey.numel(), 1), max(rkey.numel(), 1)]
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    while True:
        E = lambda k: torch.empty(k, dtype=torch.int64, device=dev)
        g = [E(caps[0]) for _ in range(3)] + [E(caps[0] + 1) for _ in range(2)]
        le, re = E(caps[1]), E(caps[2])
        rc = N.lib().gw_window_cogroup_device(lkey.numel(), P(lkey), P(lts), P(lpay), rkey.numel(), P(rkey), P(rts), P(rpay),
                                              size, slide, offset, int(w0), int(w1), *[x.data_ptr() for x in g],
                                              le.data_ptr(), caps[1], re.data_ptr(), caps[2], caps[0], n,
                                              ctypes.c_void_p(stream) if stream else None)
        if rc == N.GW_E_OUTPUT_FULL and any(n[i] > caps[i] for i in range(3)):
            caps = [max(caps[i], n[i]) for i in range(3)]
            continue
        N.check(rc)
        break
    return (g[0][:n[0]], g[1][:n[0]], g[2][:n[0]], g[3][:n[0] + 1], g[4][:n[0] + 1], le[:n[1]], re[:n[2]])


def window_cogroup_host(lkey, lts, lpay, rkey, rts, rpay, assigner: WindowAssigner, w0: int = LONG_MIN,
                        w1: int = LONG_MAX):
    """gw_window_cogroup_host over numpy columns: window_cogroup_device as plain host code."""
    _, size, slide, offset = _join_geometry(assigner)
    cols = [np.ascontiguousarray(x, dtype=np.int64) for x in (lkey, lts, lpay, rkey, rts, rpay)]
    if not (len(cols[0]) == len(cols[1]) == len(cols[2]) and len(cols[3]) == len(cols[4]) == len(cols[5])):
        raise ValueError("column lengths differ")
    n = (ctypes.c_int64 * 3)()
    caps = [max(len(cols[0]) + len(cols[3]), 1), max(len(cols[0]), 1), max(len(cols[3]), 1)]
    while True:
        g = [np.empty(caps[0], np.int64) for _ in range(3)] + [np.empty(caps[0] + 1, np.int64) for _ in range(2)]
        le, re = np.empty(caps[1], np.int64), np.empty(caps[2], np.int64)
        rc = N.lib().gw_window_cogroup_host(len(cols[0]), *[_ptr(c) for c in cols[:3]], len(cols[3]),
                                            *[_ptr(c) for c in cols[3:]], size, slide, offset, int(w0), int(w1),
                                            *[_ptr(x) for x in g], _ptr(le), caps[1], _ptr(re), caps[2], caps[0], n)
        if rc == N.GW_E_OUTPUT_FULL and any(n[i] > caps[i] for i in range(3)):
            caps = [max(caps[i], n[i]) for i in range(3)]
            continue
        N.check(rc)
        break
    return (g[0][:n[0]], g[1][:n[0]], g[2][:n[0]], g[3][:n[0] + 1], g[4][:n[0] + 1], le[:n[1]], re[:n[2]])


def interval_join_device(probe_side: int, pkey, pts, ppay, bkey, bts, bpay, lower: int, upper: int, stream=None):
    """gw_interval_join_device over torch device tensors (int64): the rows of one ingest call of
    `probe_side` (0 left, 1 right) against a buffer of the other side's records in arrival order.
    A left l and a right r pair when l.key == r.key and l.ts + lower <= r.ts <= l.ts + upper (both
    inclusive, relative to the left record whichever side probes).  Returns device tensors (key,
    left ts, right ts, left payload, right payload): the probes in arrival order, each one's
    partners by ascending (ts, arrival).  No late filtering.  Waits on `stream` (default: torch's
    current)."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(pkey.device).cuda_stream
    n_out = ctypes.c_int64(0)
    cap = max(pkey.numel(), bkey.numel(), 1)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    while True:
        out = [torch.empty(cap, dtype=torch.int64, device=pkey.device) for _ in range(5)]
        rc = N.lib().gw_interval_join_device(int(probe_side), pkey.numel(), P(pkey), P(pts), P(ppay), bkey.numel(), P(bkey),
                                             P(bts), P(bpay), int(lower), int(upper), *[o.data_ptr() for o in out], cap,
                                             ctypes.byref(n_out), ctypes.c_void_p(stream) if stream else None)
        if rc == N.GW_E_OUTPUT_FULL and n_out.value > cap:
            cap = n_out.value
            continue
        N.check(rc)
        break
    return tuple(o[:n_out.value] for o in out)


def interval_join_host(probe_side: int, pkey, pts, ppay, bkey, bts, bpay, lower: int, upper: int):
    """gw_interval_join_host over numpy columns: the contract of interval_join_device as plain
    host code (no device)."""
    cols = [np.ascontiguousarray(x, dtype=np.int64) for x in (pkey, pts, ppay, bkey, bts, bpay)]
    if not (len(cols[0]) == len(cols[1]) == len(cols[2]) and len(cols[3]) == len(cols[4]) == len(cols[5])):
        raise ValueError("column lengths differ")
    n_out = ctypes.c_int64(0)
    cap = max(len(cols[0]), len(cols[3]), 1)
    while True:
        out = [np.empty(cap, np.int64) for _ in range(5)]
        rc = N.lib().gw_interval_join_host(int(probe_side), len(cols[0]), *[_ptr(c) for c in cols[:3]], len(cols[3]),
                                           *[_ptr(c) for c in cols[3:]], int(lower), int(upper), *[_ptr(o) for o in out],
                                           cap, ctypes.byref(n_out))
        if rc == N.GW_E_OUTPUT_FULL and n_out.value > cap:
            cap = n_out.value
            continue
        N.check(rc)
        break
    return tuple(o[:n_out.value] for o in out)


# ------------------------------------------------------------------------ operator
class StatusWatermarkValve:
    """The valve of an input gate with n channels (gw_valve; host code, no device): feed it each
    channel's watermarks and watermark statuses, act on what it emits.  Every input returns a
    list of at most two emissions, ("watermark", t) before ("status", idle)."""

    def __init__(self, n: int):
        v = ctypes.c_void_p()
        rc = N.lib().gw_valve_create(int(n), ctypes.byref(v))
        if rc == N.GW_E_INVALID:
            raise ValueError(N.lib().gw_last_error(None).decode())
        N.check(rc)
        self._v, self.n = v, int(n)

    def _input(self, channel: int, kind: int, value: int) -> list:
        o = N.GwValveOutput()
        N.check(N.lib().gw_valve_input(self._v, int(channel), kind, int(value), ctypes.byref(o)))
        out = []
        if o.has_watermark:
            out.append(("watermark", o.watermark))
        if o.has_status:
            out.append(("status", o.status == N.STATUS_IDLE))
        return out

    def input_watermark(self, channel: int, timestamp: int) -> list:
        return self._input(channel, N.EVENT_WATERMARK, timestamp)

    def input_status(self, channel: int, idle: bool) -> list:
        return self._input(channel, N.EVENT_STATUS, N.STATUS_IDLE if idle else N.STATUS_ACTIVE)

    def input_event(self, channel: int, kind: int, value: int) -> list:
        """kind / value as the decoder writes them (N.EVENT_*; a status value as serialized)."""
        return self._input(channel, kind, value)

    def close(self):
        if self._v:
            N.lib().gw_valve_destroy(self._v)
            self._v = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GpuWindowOperator:
    """Keyed event-time window operator on one MI355X (one Flink subtask).

    aggregate: one of count, sum_i64, sum_i32, sum_f64, min_i64, max_i64, min_f64,
    max_f64, avg_i64, avg_f64 (the closed set of include/gpuwin.h).
    key_selector / value_selector extract key and aggregated field from a record
    value (defaults: value[0] and value[1], i.e. Tuple2 f0 / f1).
    """

    def __init__(self, assigner: WindowAssigner, aggregate: str, allowed_lateness: int = 0,
                 trigger=None, key_selector: Callable = None, value_selector: Callable = None,
                 max_parallelism: int = 128, parallelism: int = 1, operator_index: int = 0,
                 device: int = 0, capacity_hint: int = 0, max_batch: int = 1 << 22, flags: int = 0,
                 window_function: Optional[Callable] = None, processing_time: Optional[Callable[[], int]] = None):
        if aggregate not in N.AGGS:
            raise ValueError(f"unknown aggregate {aggregate!r}")
        if allowed_lateness < 0:
            raise ValueError("The allowed lateness cannot be negative.")
        self.assigner = assigner
        self.aggregate = aggregate
        self.trigger = trigger or EventTimeTrigger.create()
        self.key_selector = key_selector or (lambda v: v[0])
        self.value_selector = value_selector or (lambda v: v[1])
        self.is_double_out = aggregate in N.DOUBLE_RESULT
        self.is_double_in = aggregate in N.DOUBLE_INPUT
        c = N.GwConfig()
        a = assigner.config()
        c.assigner = N.ASSIGNERS[a["assigner"]]
        c.trigger = N.TRIGGERS[self.trigger.name]
        c.size, c.slide, c.offset = a.get("size", 0), a.get("slide", 0), a.get("offset", 0)
        c.gap = a.get("gap", 0)
        c.allowed_lateness = allowed_lateness
        c.agg = N.AGGS[aggregate]
        c.max_parallelism, c.parallelism, c.operator_index = max_parallelism, parallelism, operator_index
        c.device, c.flags, c.capacity_hint, c.max_batch = device, flags, capacity_hint, max_batch
        self.cfg = c
        self._h = None
        self._keys_in: dict = {}
        self._keys_out: list = []
        self._hash_out: list = []  # key.hashCode() per dictionary id (gw_ingest key_hash)
        self._int_keys = True
        self._buf_k: List[int] = []
        self._buf_t: List[int] = []
        self._buf_v: List = []
        # payload handles (FLAG_FIRST_ELEMENT / FLAG_BY_FIELD) on the record-at-a-time surface:
        # each element is kept on the host and its index travels as the payload
        self._payload = bool(flags & (N.FLAG_FIRST_ELEMENT | N.FLAG_BY_FIELD))
        self._by = bool(flags & N.FLAG_BY_FIELD)
        self._elems: list = []
        self._buf_p: List[int] = []
        # per-element session gaps (DynamicEventTimeSessionWindows): the extractor's value per record
        self._dynamic = a["assigner"] == "session_dynamic"
        self._buf_g: List[int] = []
        self.output: list = []
        # reduce / aggregate(..., ProcessWindowFunction): window_function(key, (start, end), [result],
        # out) per fired window, out a list the emitted values go to (InternalSingleValueProcess-
        # WindowFunction: a one-element Iterable of the pre-aggregated result, output stamped
        # window.maxTimestamp())
        self.window_function = window_function
        # processing-time clock in ms (ProcessingTimeService.getCurrentProcessingTime): a staggered
        # tumbling assigner draws its stagger at the first element
        self.processing_time = processing_time or (lambda: time.time_ns() // 1_000_000)
        self._stagger = getattr(assigner, "stagger", WindowStagger.ALIGNED)
        self._deferred = False        # staggered: the handle is created at the first element
        self._deferred_wm = LONG_MIN  # watermarks seen before it
        self._stagger_time = None

    # lifecycle -------------------------------------------------------------
    def open(self):
        if self._stagger != WindowStagger.ALIGNED:
            # TumblingEventTimeWindows draws its stagger at the first element (:72-79): the
            # handle, whose windows need the offset, is created then
            WindowStagger.window_offset(self._stagger, 0, self.cfg.size, self.cfg.offset, 0.0)  # validates
            self._deferred = True
            return self
        return self._create()

    def _create(self):
        h = ctypes.c_void_p()
        rc = N.lib().gw_create(ctypes.byref(self.cfg), ctypes.byref(h))
        if rc == -1:
            raise ValueError(N.lib().gw_last_error(None).decode())
        N.check(rc, None)
        self._h = h
        return self

    def _ensure_handle(self):
        """A staggered operator's first element: draw the stagger at the processing time the
        first element arrived, create the handle with (offset + stagger) % size, replay the
        watermark seen so far (no state yet: it fires nothing)."""
        if not self._deferred:
            return
        now = self._stagger_time if self._stagger_time is not None else self.processing_time()
        self.cfg.offset = WindowStagger.window_offset(self._stagger, now, self.cfg.size, self.cfg.offset)
        self._deferred = False
        self._create()
        if self._deferred_wm != LONG_MIN:
            self.advance_watermark(self._deferred_wm)

    def close(self):
        if self._h:
            N.lib().gw_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self.open() if self._h is None else self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # keys --------------------------------------------------------------------
    def _encode_key(self, key) -> int:
        """Long keys go to the GPU as they are (the device computes Long.hashCode); any
        other key type gets a dictionary id, and its key.hashCode() travels in the key_hash
        column so key groups, snapshots and rescaling follow the key's own hash."""
        if isinstance(key, int) and not isinstance(key, bool) and LONG_MIN <= key <= LONG_MAX and self._int_keys \
                and not self._keys_out:
            return key
        self._int_keys = False
        kid = self._keys_in.get(key)
        if kid is None:
            kid = len(self._keys_out)
            self._keys_in[key] = kid
            self._keys_out.append(key)
            self._hash_out.append(java_hash(key))
        return kid

    def _decode_key(self, kid: int):
        return kid if self._int_keys else self._keys_out[kid]

    # record-at-a-time surface (StreamRecord / Watermark) ----------------------
    def process_element(self, record: StreamRecord):
        if self._deferred and self._stagger_time is None:
            self._stagger_time = self.processing_time()  # the stagger is drawn at the first element
        v = record.value
        self._buf_k.append(self._encode_key(self.key_selector(v)))
        self._buf_t.append(int(record.timestamp))
        self._buf_v.append(self.value_selector(v) if self.aggregate != "count" else 0)
        if self._dynamic:
            self._buf_g.append(int(self.assigner.extractor(v)))
        if self._payload:
            self._buf_p.append(len(self._elems))
            self._elems.append(v)

    def _flush(self):
        if not self._buf_k:
            return
        k = np.asarray(self._buf_k, dtype=np.int64)
        t = np.asarray(self._buf_t, dtype=np.int64)
        if self.is_double_in:
            v = np.asarray(self._buf_v, dtype=np.float64).view(np.int64)
        else:
            v = np.asarray(self._buf_v, dtype=np.int64)
        self._buf_k, self._buf_t, self._buf_v = [], [], []
        h = None if self._int_keys else np.asarray(self._hash_out, dtype=np.int32)[k]
        if self._payload:
            p = np.asarray(self._buf_p, dtype=np.int64)
            self._buf_p = []
            self.process_batch_payload(k, t, v, p, key_hashes=h)
        elif self._dynamic:
            g = np.asarray(self._buf_g, dtype=np.int64)
            self._buf_g = []
            self.process_batch(k, t, v, key_hashes=h, gaps=g)
        else:
            self.process_batch(k, t, v, key_hashes=h)

    def process_watermark(self, wm):
        ts = wm.timestamp if isinstance(wm, Watermark) else int(wm)
        self._flush()
        self.advance_watermark(ts)
        if self._payload:
            # minBy / maxBy emit the element itself (ComparableAggregator.java:88-95); positional
            # aggregates the first element beside the result
            k, s, e, r, pl = self.drain_payload()
            for i in range(len(k)):
                el = self._elems[int(pl[i])]
                val = el if self._by else (self._decode_key(int(k[i])), int(s[i]), int(e[i]), r[i], el)
                self.output.append(StreamRecord(val, int(e[i]) - 1))
            self.output.append(Watermark(ts))
            return
        k, s, e, r = self.drain()
        for i in range(len(k)):
            res = r[i]
            key, start, end = self._decode_key(int(k[i])), int(s[i]), int(e[i])
            if self.window_function is not None:
                out: list = []
                self.window_function(key, (start, end), [res], out)
                self.output.extend(StreamRecord(x, end - 1) for x in out)
            else:
                self.output.append(StreamRecord((key, start, end, res), end - 1))
        self.output.append(Watermark(ts))

    def end_input(self):
        """BoundedOneInput.endInput followed by MAX_WATERMARK."""
        self.process_watermark(MAX_WATERMARK)

    def get_output(self):
        out, self.output = self.output, []
        return out

    # columnar surface ------------------------------------------------------------
    def _check_gaps(self, gaps):
        if self._dynamic and gaps is None:
            raise ValueError("a DynamicEventTimeSessionWindows operator needs the gap column (gaps=)")
        if not self._dynamic and gaps is not None:
            raise ValueError("gaps= is for DynamicEventTimeSessionWindows operators")

    def process_batch(self, keys: np.ndarray, timestamps: np.ndarray, values: Optional[np.ndarray] = None,
                      key_hashes: Optional[np.ndarray] = None, gaps: Optional[np.ndarray] = None):
        """gaps: the per-element session gaps in ms (DynamicEventTimeSessionWindows operators)."""
        self._check_gaps(gaps)
        self._ensure_handle()
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        timestamps = np.ascontiguousarray(timestamps, dtype=np.int64)
        if values is not None:
            values = np.ascontiguousarray(values)
            if values.dtype == np.float64:
                values = values.view(np.int64)
            values = values.astype(np.int64, copy=False)
        if key_hashes is not None:
            key_hashes = np.ascontiguousarray(key_hashes, dtype=np.int32)
        if len(keys) != len(timestamps) or (values is not None and len(values) != len(keys)):
            raise ValueError("column lengths differ")
        if gaps is not None:
            gaps = np.ascontiguousarray(gaps, dtype=np.int64)
            if len(gaps) != len(keys):
                raise ValueError("column lengths differ")
            rc = N.lib().gw_ingest_gap(self._h, len(keys), _ptr(keys), _ptr(key_hashes), _ptr(timestamps),
                                       _ptr(values), _ptr(gaps))
        else:
            rc = N.lib().gw_ingest(self._h, len(keys), _ptr(keys), _ptr(key_hashes), _ptr(timestamps), _ptr(values))
        N.check(rc, self._h)

    # first-element rows (flags=FLAG_FIRST_ELEMENT) ------------------------------------
    def process_batch_payload(self, keys, timestamps, values, payload, key_hashes=None):
        """Records with a 64-bit payload each (the Tuple's non-aggregated fields, packed by the
        caller); rows carry the payload of their window's first element in arrival order, as
        SumAggregator / ComparableAggregator keep it (gw_ingest_payload)."""
        self._ensure_handle()
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        timestamps = np.ascontiguousarray(timestamps, dtype=np.int64)
        values = np.ascontiguousarray(values)
        values = values.view(np.int64) if values.dtype == np.float64 else values.astype(np.int64, copy=False)
        payload = np.ascontiguousarray(payload, dtype=np.int64)
        if key_hashes is not None:
            key_hashes = np.ascontiguousarray(key_hashes, dtype=np.int32)
        if not (len(keys) == len(timestamps) == len(values) == len(payload)):
            raise ValueError("column lengths differ")
        N.check(N.lib().gw_ingest_payload(self._h, len(keys), _ptr(keys), _ptr(key_hashes), _ptr(timestamps),
                                          _ptr(values), _ptr(payload)), self._h)

    def process_batch_payload_device(self, keys, timestamps, values, payload, stream=None):
        """Same, with torch device columns produced on `stream` (default: torch's current)."""
        self._ensure_handle()
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(keys.device).cuda_stream
        p = [ctypes.c_void_p(x.data_ptr()) for x in (keys, timestamps, values, payload)]
        N.check(N.lib().gw_ingest_payload_device(self._h, keys.numel(), p[0], None, p[1], p[2], p[3],
                                                 ctypes.c_void_p(stream) if stream else None), self._h)

    def drain_payload(self):
        """All pending rows as numpy (key, start, end, result, payload) columns."""
        n = self.pending_rows()
        k, s, e, r, pl = (np.empty(n, np.int64) for _ in range(5))
        got = ctypes.c_int64(0)
        if n:
            N.check(N.lib().gw_drain_payload(self._h, _ptr(k), _ptr(s), _ptr(e), _ptr(r), _ptr(pl), n,
                                             ctypes.byref(got)), self._h)
            assert got.value == n
        if self.is_double_out:
            r = r.view(np.float64)
        return k, s, e, r, pl

    # network-buffer surface -----------------------------------------------------------
    def process_serialized(self, data: bytes, layout: "N.GwRecordLayout") -> tuple:
        """Decode and process one input channel's serialized elements (records and
        watermarks) on the GPU (gw_ingest_serialized).  Returns (consumed, rows_fired):
        bytes past `consumed` belong to an element spanning into the next buffer and must
        be passed again, prepended to it."""
        self._ensure_handle()
        consumed, fired = ctypes.c_int64(0), ctypes.c_int64(0)
        buf = ctypes.create_string_buffer(bytes(data), len(data)) if data else None
        N.check(N.lib().gw_ingest_serialized(self._h, buf, len(data), ctypes.byref(layout), ctypes.byref(consumed),
                                             ctypes.byref(fired)), self._h)
        return consumed.value, fired.value

    def process_serialized_device(self, data, layout: "N.GwRecordLayout", stream=None) -> tuple:
        """Same, with the bytes in a device uint8 tensor."""
        self._ensure_handle()
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(data.device).cuda_stream
        consumed, fired = ctypes.c_int64(0), ctypes.c_int64(0)
        N.check(N.lib().gw_ingest_serialized_device(self._h, ctypes.c_void_p(data.data_ptr()), data.numel(),
                                                    ctypes.byref(layout),
                                                    ctypes.c_void_p(stream) if stream else None,
                                                    ctypes.byref(consumed), ctypes.byref(fired)), self._h)
        return consumed.value, fired.value

    def process_buffers(self, buffers, layout: "N.GwRecordLayout") -> int:
        """Feed network buffers in order, carrying a spanning record's bytes over to the next
        buffer (SpanningWrapper).  Returns the rows fired."""
        carry = b""
        fired = 0
        for b in buffers:
            data = carry + bytes(b)
            used, f = self.process_serialized(data, layout)
            carry = data[used:]
            fired += f
        if carry:
            raise N.GpuWinError(-1, f"{len(carry)} bytes of an incomplete element at the end of the input")
        return fired

    # several input channels (gw_set_input_channels, gw_ingest_channels*) -----------------------
    def set_input_channels(self, n: int):
        """The operator reads n input channels through a StatusWatermarkValve of its own: what it
        acts on is the minimum watermark over the active, aligned channels."""
        self._ensure_handle()
        N.check(N.lib().gw_set_input_channels(self._h, int(n)), self._h)
        self._channel_carry = {}
        return self

    def process_channels(self, parts, layout: "N.GwRecordLayout") -> tuple:
        """parts: [(channel, bytes)], each channel at most once; processed as if the parts had
        arrived in list order (gw_ingest_channels: one decode, one synchronisation).  Returns
        (consumed per part, rows_fired)."""
        self._ensure_handle()
        n = len(parts)
        chan = (ctypes.c_int32 * max(n, 1))(*[int(c) for c, _ in parts])
        bufs = [ctypes.create_string_buffer(bytes(d), len(d)) if len(d) else None for _, d in parts]
        ptrs = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(b, ctypes.c_void_p) if b is not None else None
                                               for b in bufs])
        lens = (ctypes.c_int64 * max(n, 1))(*[len(d) for _, d in parts])
        consumed = (ctypes.c_int64 * max(n, 1))()
        fired = ctypes.c_int64(0)
        N.check(N.lib().gw_ingest_channels(self._h, n, chan, ptrs, lens, ctypes.byref(layout), consumed,
                                           ctypes.byref(fired)), self._h)
        return list(consumed)[:n], fired.value

    def process_channels_device(self, parts, layout: "N.GwRecordLayout", stream=None) -> tuple:
        """Same, with each part's bytes in a device uint8 tensor (4-byte aligned; separate
        allocations allowed), produced on `stream`."""
        self._ensure_handle()
        n = len(parts)
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        chan = (ctypes.c_int32 * max(n, 1))(*[int(c) for c, _ in parts])
        ptrs = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() if t.numel() else None for _, t in parts])
        lens = (ctypes.c_int64 * max(n, 1))(*[t.numel() for _, t in parts])
        consumed = (ctypes.c_int64 * max(n, 1))()
        fired = ctypes.c_int64(0)
        N.check(N.lib().gw_ingest_channels_device(self._h, n, chan, ptrs, lens, ctypes.byref(layout),
                                                  ctypes.c_void_p(stream) if stream else None, consumed,
                                                  ctypes.byref(fired)), self._h)
        return list(consumed)[:n], fired.value

    def process_channel_buffers(self, parts, layout: "N.GwRecordLayout") -> int:
        """One poll of the input gate: parts = [(channel, bytes)] as process_channels takes them.
        Each channel's unconsumed tail (an element spanning into its next buffer) is kept and
        prepended to the channel's next bytes, as process_buffers does for one channel.  Returns
        the rows fired."""
        carry = self._channel_carry = getattr(self, "_channel_carry", None) or {}
        data = [(c, carry.get(c, b"") + bytes(d)) for c, d in parts]
        used, fired = self.process_channels(data, layout)
        for (c, d), u in zip(data, used):
            carry[c] = d[u:]
        return fired

    def channel_tails(self) -> dict:
        """Bytes of incomplete elements waiting per channel (process_channel_buffers)."""
        return {c: len(t) for c, t in (getattr(self, "_channel_carry", None) or {}).items() if t}

    def input_status(self) -> tuple:
        """(watermark, idle): the last output of the handle's valve (gw_input_status), which the
        operator forwards downstream."""
        wm, idle = ctypes.c_int64(0), ctypes.c_int32(0)
        N.check(N.lib().gw_input_status(self._h, ctypes.byref(wm), ctypes.byref(idle)), self._h)
        return wm.value, bool(idle.value)

    # staged host ingest (gw_stage_*): pinned library-owned columns filled in place ------------
    def stage_alloc(self, slots: int, cap: int):
        """`slots` pinned column slots of `cap` records (gw_stage_alloc)."""
        self._ensure_handle()
        N.check(N.lib().gw_stage_alloc(self._h, int(slots), int(cap)), self._h)
        self._stage_cap = int(cap)

    def stage_columns(self, slot: int):
        """Slot `slot`'s (key int64, key_hash int32, ts int64, value int64) columns as numpy arrays
        over the pinned memory, once the slot's previous transfer has read it."""
        p = [ctypes.c_void_p() for _ in range(4)]
        N.check(N.lib().gw_stage_columns(self._h, int(slot), *[ctypes.byref(x) for x in p]), self._h)
        cap = self._stage_cap

        def arr(ptr, ct):
            return np.ctypeslib.as_array(ctypes.cast(ptr.value, ctypes.POINTER(ct)), shape=(cap,))
        return arr(p[0], ctypes.c_int64), arr(p[1], ctypes.c_int32), arr(p[2], ctypes.c_int64), arr(p[3], ctypes.c_int64)

    def ingest_stage(self, slot: int, n: int, with_value: bool = True, with_key_hash: bool = False):
        """The slot's first n records (gw_ingest_stage)."""
        cols = (N.STAGE_VALUE if with_value else 0) | (N.STAGE_KEY_HASH if with_key_hash else 0)
        N.check(N.lib().gw_ingest_stage(self._h, int(slot), int(n), cols), self._h)

    def stage_send(self, slot: int, n: int, with_value: bool = True, with_key_hash: bool = False):
        """Send the slot's first n records over PCIe ahead of their gw_ingest_stage (gw_stage_send):
        up to two batches ahead (three device buffers); ingest_stage calls must follow the send
        order."""
        cols = (N.STAGE_VALUE if with_value else 0) | (N.STAGE_KEY_HASH if with_key_hash else 0)
        N.check(N.lib().gw_stage_send(self._h, int(slot), int(n), cols), self._h)

    def process_batch_device(self, keys, timestamps, values=None, stream=None, gaps=None):
        """Columns already in HBM (torch tensors or raw device pointers); gaps: the per-element
        session gaps of a DynamicEventTimeSessionWindows operator."""
        self._check_gaps(gaps)
        self._ensure_handle()
        def p(x):
            if x is None:
                return None
            return ctypes.c_void_p(x if isinstance(x, int) else x.data_ptr())
        n = keys if isinstance(keys, int) else keys.numel()
        if isinstance(keys, int):
            raise ValueError("pass tensors, or use process_batch_device_ptr for raw pointers")
        if stream is None:  # the columns were produced on PyTorch's current stream
            import torch
            stream = torch.cuda.current_stream(keys.device).cuda_stream
        if gaps is not None:
            if gaps.numel() != n:
                raise ValueError("column lengths differ")
            rc = N.lib().gw_ingest_gap_device(self._h, n, p(keys), None, p(timestamps), p(values), p(gaps),
                                              ctypes.c_void_p(stream) if stream else None)
        else:
            rc = N.lib().gw_ingest_device(self._h, n, p(keys), None, p(timestamps), p(values),
                                          ctypes.c_void_p(stream) if stream else None)
        N.check(rc, self._h)

    def process_batch_device_ptr(self, n: int, key_ptr: int, ts_ptr: int, val_ptr: Optional[int], stream=None):
        self._ensure_handle()
        rc = N.lib().gw_ingest_device(self._h, n, ctypes.c_void_p(key_ptr), None, ctypes.c_void_p(ts_ptr),
                                      ctypes.c_void_p(val_ptr) if val_ptr else None,
                                      ctypes.c_void_p(stream) if stream else None)
        N.check(rc, self._h)

    def process_batch_packed_device_ptr(self, n_other: int, key_ptr, ts_ptr, val_ptr, n_words: int, words_ptr,
                                        geom, stream=None):
        """gw_ingest_packed_device: n_other column records followed by n_words packed exchange
        words (NativeKeyByExchange.last_words)."""
        self._ensure_handle()
        vp = lambda x: ctypes.c_void_p(x) if x else None
        rc = N.lib().gw_ingest_packed_device(self._h, n_other, vp(key_ptr), vp(ts_ptr), vp(val_ptr), n_words,
                                             vp(words_ptr), ctypes.byref(geom), vp(stream))
        N.check(rc, self._h)

    def advance_watermark(self, wm: int) -> int:
        if self._deferred:  # staggered, no element yet: nothing can fire
            self._deferred_wm = max(self._deferred_wm, int(wm))
            return 0
        fired = ctypes.c_int64(0)
        N.check(N.lib().gw_advance_watermark(self._h, int(wm), ctypes.byref(fired)), self._h)
        return fired.value

    def flush(self):
        """Apply every buffered record to the window state (gw_flush); firing does this
        by itself, a snapshot or a timing boundary calls it explicitly."""
        if self._deferred:
            return
        N.check(N.lib().gw_flush(self._h), self._h)

    # checkpointing ----------------------------------------------------------------
    def snapshot_state(self, key_group_range=None) -> bytes:
        """Keyed window state of the key groups [lo, hi] (default: all), as one blob
        (StreamOperator.snapshotState; restore with initialize_state)."""
        lo, hi = key_group_range if key_group_range is not None else (0, self.cfg.max_parallelism - 1)
        if self._deferred:  # staggered, no element yet: no window state
            tmp = GpuWindowOperator(TumblingEventTimeWindows.of(self.cfg.size, self.cfg.offset), self.aggregate,
                                    self.cfg.allowed_lateness, self.trigger, max_parallelism=self.cfg.max_parallelism,
                                    device=self.cfg.device, capacity_hint=16, max_batch=16,
                                    flags=self.cfg.flags).open()
            try:
                return tmp.snapshot_state(key_group_range)
            finally:
                tmp.close()
        n = ctypes.c_int64(0)
        N.check(N.lib().gw_snapshot(self._h, lo, hi, None, 0, ctypes.byref(n)), self._h)
        buf = ctypes.create_string_buffer(n.value)
        N.check(N.lib().gw_snapshot(self._h, lo, hi, buf, n.value, ctypes.byref(n)), self._h)
        return buf.raw[:n.value]

    def initialize_state(self, blobs):
        """Restore one or more snapshot blobs (e.g. the key-group ranges of several
        subtasks after rescaling) before processing (StreamOperator.initializeState).
        A keyed snapshot (snapshot_state_keyed) gets its keys re-encoded through this
        operator's dictionary first."""
        if isinstance(blobs, (bytes, bytearray)):
            blobs = [blobs]
        if self._deferred:
            self._adopt_restored_stagger(blobs)
        if self._deferred:  # no restored window state: the stagger is drawn at the first element
            return
        for b in blobs:
            b = bytes(b)
            if b[:4] == KEYED_MAGIC:
                b = self._rekey(b)
            N.check(N.lib().gw_restore(self._h, b, len(b)), self._h)

    def _adopt_restored_stagger(self, blobs):
        """A staggered tumbling operator restored from window state keeps the stagger the state
        was written under: the blobs' window offset (header), which is (offset + stagger) %
        size of the operator that wrote them.  The reference draws a new stagger after a restore
        (TumblingEventTimeWindows.java:72-79: staggerOffset starts out null) and keeps the
        restored windows at their old alignment beside it; one handle holds one alignment, so
        the old draw is reused -- for RANDOM a valid draw of the same distribution, for NATURAL
        the first element's processing time of the run that wrote the state.  Blobs without
        state leave the operator to draw at its first element; blobs of one restore carrying
        different staggers (subtasks' independent draws merged by a rescale) are refused."""
        offs = set()
        for b in blobs:
            b = bytes(b)
            if b[:4] == KEYED_MAGIC:
                b = unpack_keyed_snapshot(b)[0]
            hdr = struct.unpack_from("<4sIii5q4i3q", b, 0)
            nk = hdr[11] - hdr[10] + 1
            if hdr[15] > 12 * nk:  # payload beyond the empty sections (n = m = t = 0) of each key group
                offs.add(int(hdr[6]))
        if len(offs) > 1:
            raise N.GpuWinError(N.GW_E_UNSUPPORTED, "restoring window state of staggered tumbling operators "
                                f"drawn with different staggers (window offsets {sorted(offs)}) into one")
        if offs:
            self.cfg.offset = offs.pop()
            self._deferred = False
            self._create()

    def snapshot_state_keyed(self, key_group_range=None) -> bytes:
        """snapshot_state plus the real keys behind the dictionary ids its entries name, as
        GpuWindowOperator.snapshotState writes them through the key serializer: any
        operator (another process, another dictionary) restores it."""
        blob = self.snapshot_state(key_group_range)
        ids = N.snapshot_keys(blob)
        return pack_keyed_snapshot(blob, {int(i): self._decode_key(int(i)) for i in ids})

    def _rekey(self, wrapped: bytes) -> bytes:
        blob, keys = unpack_keyed_snapshot(wrapped)
        if self._int_keys and all(isinstance(k, int) for k in keys.values()) and not self._keys_out:
            return N.snapshot_remap_keys(blob, {i: k for i, k in keys.items()})
        if not self._keys_out:
            self._int_keys = False
        return N.snapshot_remap_keys(blob, {i: self._encode_key(k) for i, k in keys.items()})

    def pending_rows(self) -> int:
        if self._deferred:
            return 0
        n = ctypes.c_int64(0)
        N.check(N.lib().gw_pending_rows(self._h, ctypes.byref(n)), self._h)
        return n.value

    def drain(self, out=None):
        """All pending fired rows as numpy (key, start, end, result) columns.  `out`: four int64
        numpy arrays to fill (e.g. over pinned memory, which the D2H then writes directly);
        views of their first n entries are returned."""
        n = self.pending_rows()
        if out is not None:
            if any(len(x) < n for x in out):
                raise ValueError(f"drain: out arrays hold fewer than the {n} pending rows")
            k, s, e, r = (x[:n] for x in out)
        else:
            k = np.empty(n, np.int64)
            s = np.empty(n, np.int64)
            e = np.empty(n, np.int64)
            r = np.empty(n, np.int64)
        got = ctypes.c_int64(0)
        if n:
            rc = N.lib().gw_drain(self._h, _ptr(k), _ptr(s), _ptr(e), _ptr(r), n, ctypes.byref(got))
            N.check(rc, self._h)
            assert got.value == n
        if self.is_double_out:
            r = r.view(np.float64)
        return k, s, e, r

    def clear_rows(self):
        if self._deferred:
            return
        N.check(N.lib().gw_clear_rows(self._h), self._h)

    def top_n_rows(self, top: int, smallest: bool = False):
        """Per window, the `top` pending rows with the largest (smallest=True: smallest) result,
        ties to the smaller key, ranked on the device (gw_top_n_rows): numpy (key, start, end,
        result, win_rows), windows in ascending end, best first; win_rows = the pending rows of
        the row's window.  The rows stay pending: follow with clear_rows() or drain().  The
        non-keyed top-N stage of Nexmark Q5 / Q7 without draining one row per key."""
        if self._deferred:
            return tuple(np.empty(0, np.float64 if (self.is_double_out and i == 3) else np.int64) for i in range(5))
        mode = N.TOPN_SMALLEST if smallest else 0
        n = ctypes.c_int64(0)
        cap = 4096
        while True:
            out = [np.empty(cap, np.int64) for _ in range(5)]
            rc = N.lib().gw_top_n_rows(self._h, int(top), mode, *[_ptr(o) for o in out], cap, ctypes.byref(n))
            if rc == N.GW_E_OUTPUT_FULL and n.value > cap:
                cap = n.value
                continue
            N.check(rc, self._h)
            break
        k, s, e, r, w = (o[:n.value] for o in out)
        return k, s, e, (r.view(np.float64) if self.is_double_out else r), w

    def rows_device(self):
        p = [ctypes.c_void_p() for _ in range(4)]
        n = ctypes.c_int64(0)
        rc = N.lib().gw_rows_device(self._h, *[ctypes.byref(x) for x in p], ctypes.byref(n))
        N.check(rc, self._h)
        return [x.value for x in p], n.value

    # network-buffer output ------------------------------------------------------------
    def _serialized_cap(self, layout, channels: int) -> int:
        rb = N.lib().gw_row_encoded_bytes(ctypes.byref(layout))
        if rb < 0:
            N.check(int(rb))
        return self.pending_rows() * rb + channels * 32  # a watermark and alignment padding per channel

    def _no_rows_serialized(self, layout, channels, max_parallelism, watermark):
        z = np.empty(0, np.int64)
        return N.encode_rows_host(z, z, z, z, layout, payload=z if self._payload else None, channels=channels,
                                  max_parallelism=max_parallelism, watermark=watermark)

    def drain_serialized(self, layout: "N.GwRowLayout", channels: int = 1, max_parallelism: int = 128,
                         watermark: Optional[int] = None) -> list:
        """All pending rows as the serialized stream elements a Flink task would have written for
        them (gw_drain_serialized; netbuf.record per row, timestamp = window end - 1), encoded on
        the GPU: one bytes object per downstream channel (channels > 1: keyBy on the row key),
        each ending with Watermark(watermark) when one is given.  The rows are removed."""
        if self._deferred:  # staggered and no element yet: no rows
            return self._no_rows_serialized(layout, channels, max_parallelism, watermark)
        cap = self._serialized_cap(layout, channels)
        buf = np.empty(max(cap, 1), np.uint8)
        off, nb = np.zeros(channels, np.int64), np.zeros(channels, np.int64)
        N.check(N.lib().gw_drain_serialized(self._h, ctypes.byref(layout), channels, max_parallelism,
                                            N.NO_WATERMARK if watermark is None else int(watermark), _ptr(buf), cap,
                                            _ptr(off), _ptr(nb), None), self._h)
        return [buf[o:o + b].tobytes() for o, b in zip(off.tolist(), nb.tolist())]

    def rows_serialized_device(self, layout: "N.GwRowLayout", channels: int = 1, max_parallelism: int = 128,
                               watermark: Optional[int] = None, stream=None):
        """Same, into device memory (gw_rows_serialized_device): (bytes, ranges) with bytes a
        torch.uint8 tensor on the operator's device and ranges a list of (offset, length) per
        channel, e.g. for another operator's process_serialized_device(bytes[o:o + n], ...).  The
        rows stay pending: follow with clear_rows()."""
        import torch
        dev = f"cuda:{self.cfg.device}"
        if self._deferred:
            parts = self._no_rows_serialized(layout, channels, max_parallelism, watermark)
            data = np.frombuffer(b"".join(parts), np.uint8).copy()
            ends = np.cumsum([len(x) for x in parts]).tolist()
            return torch.from_numpy(data).to(dev), [(e - len(x), len(x)) for e, x in zip(ends, parts)]
        cap = self._serialized_cap(layout, channels)
        out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(out.device).cuda_stream
        off, nb = np.zeros(channels, np.int64), np.zeros(channels, np.int64)
        N.check(N.lib().gw_rows_serialized_device(self._h, ctypes.byref(layout), channels, max_parallelism,
                                                  N.NO_WATERMARK if watermark is None else int(watermark),
                                                  ctypes.c_void_p(out.data_ptr()), cap, _ptr(off), _ptr(nb), None,
                                                  ctypes.c_void_p(stream) if stream else None), self._h)
        return out, list(zip(off.tolist(), nb.tolist()))

    def drain_late(self):
        """The late-data side output (flags=FLAG_LATE_SIDE_OUTPUT, WindowedStream.sideOutputLateData):
        the late records since the last call, as (key, timestamp, value bits) numpy columns."""
        if self._deferred:
            return tuple(np.empty(0, np.int64) for _ in range(3))
        n = ctypes.c_int64(0)
        N.check(N.lib().gw_pending_late(self._h, ctypes.byref(n)), self._h)
        k, t, v = (np.empty(n.value, np.int64) for _ in range(3))
        got = ctypes.c_int64(0)
        if n.value:
            N.check(N.lib().gw_drain_late(self._h, _ptr(k), _ptr(t), _ptr(v), n.value, ctypes.byref(got)), self._h)
            assert got.value == n.value
        return k, t, v

    @property
    def num_late_records_dropped(self) -> int:
        return 0 if self._deferred else N.lib().gw_late_dropped(self._h)

    def stats(self) -> dict:
        s = N.GwStats()
        if self._deferred:
            return s.as_dict()
        N.check(N.lib().gw_get_stats(self._h, ctypes.byref(s)), self._h)
        return s.as_dict()

    def stream(self) -> int:
        return N.lib().gw_stream(self._h)

    def enable_kernel_timing(self, on=True):
        """True / 1: time every launch; k > 1: time region pass 1 on every k-th batch only."""
        k = int(on) if not isinstance(on, bool) else (1 if on else 0)
        N.check(N.lib().gw_enable_kernel_timing(self._h, k), self._h)

    def kernel_time_ms(self, which: int = 0):
        ms = ctypes.c_double(0)
        n = ctypes.c_int64(0)
        N.check(N.lib().gw_kernel_time_ms(self._h, which, ctypes.byref(ms), ctypes.byref(n)), self._h)
        return ms.value, n.value

    def synchronize(self):
        if self._deferred:
            return
        N.check(N.lib().gw_synchronize(self._h), self._h)


# -------------------------------------------------------------- DataStream surface
class _TwoStreamOperator:
    """What the two-stream operators share around their C handles, whose entry points differ only
    in the prefix (gw_join_*, gw_ijoin_*): the handle's life, the error check, ingest of host and
    device columns, and the pending rows (five int64 columns; drain, view, clear).  A subclass
    sets _prefix and _stats_type and builds self.cfg."""

    _prefix, _stats_type = "", None

    def _fn(self, name: str):
        return getattr(N.lib(), f"{self._prefix}_{name}")

    def open(self):
        h = ctypes.c_void_p()
        rc = self._fn("create")(ctypes.byref(self.cfg), ctypes.byref(h))
        if rc == N.GW_E_INVALID:
            raise ValueError(N.lib().gw_last_error(None).decode())
        N.check(rc, None)
        self._h = h
        return self

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = None

    def __enter__(self):
        return self.open() if self._h is None else self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != N.GW_OK:
            msg = self._fn("last_error")(self._h)
            raise N.GpuWinError(rc, msg.decode() if msg else "")
        return rc

    def _ingest(self, side: int, keys, ts, payload, *extra):
        keys, ts, payload = (np.ascontiguousarray(x, dtype=np.int64) for x in (keys, ts, payload))
        if not (len(keys) == len(ts) == len(payload)):
            raise ValueError("column lengths differ")
        self._check(self._fn("ingest")(self._h, int(side), len(keys), _ptr(keys), _ptr(ts), _ptr(payload), *extra))

    def _ingest_device(self, side: int, keys, ts, payload, stream, *extra):
        if not (keys.numel() == ts.numel() == payload.numel()):
            raise ValueError("column lengths differ")
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(keys.device).cuda_stream
        P = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
        self._check(self._fn("ingest_device")(self._h, int(side), keys.numel(), P(keys), P(ts), P(payload),
                                              ctypes.c_void_p(stream) if stream else None, *extra))

    def pending(self) -> int:
        n = ctypes.c_int64(0)
        self._check(self._fn("pending")(self._h, ctypes.byref(n)))
        return n.value

    def _drain(self, fn, byte_column: bool, cap: Optional[int]):
        """All pending rows through fn (a drain entry point), cap rows per call (default: all at
        once): five int64 numpy columns, and a uint8 one behind them where fn takes one."""
        n = self.pending()
        out = [np.empty(n, np.int64) for _ in range(5)]
        if byte_column:
            out.append(np.empty(n, np.uint8))
        step = n if cap is None else max(1, int(cap))
        at = 0
        got = ctypes.c_int64(0)
        while at < n:
            rc = fn(self._h, *[ctypes.c_void_p(o.ctypes.data + o.itemsize * at) for o in out], step, ctypes.byref(got))
            if rc != N.GW_E_OUTPUT_FULL:
                self._check(rc)
            at += got.value
            if rc == N.GW_OK:
                break
        assert at == n
        return tuple(out)

    def rows_device(self):
        """Zero-copy view of the pending rows: five device pointers and their number."""
        p = [ctypes.c_void_p() for _ in range(5)]
        n = ctypes.c_int64(0)
        self._check(self._fn("rows_device")(self._h, *[ctypes.byref(x) for x in p], ctypes.byref(n)))
        return [x.value for x in p], n.value

    def clear_rows(self):
        self._check(self._fn("clear_rows")(self._h))

    def num_late_records_dropped(self) -> int:
        return int(self._fn("late_dropped")(self._h))

    def stats(self) -> dict:
        s = self._stats_type()
        self._fn("get_stats")(self._h, ctypes.byref(s))
        return s.as_dict()

    @property
    def stream(self) -> int:
        return self._fn("stream")(self._h) or 0


class GpuWindowJoinOperator(_TwoStreamOperator):
    """Event-time window join of two keyed streams on one MI355X (gw_join): Flink's
    stream.join(other).where().equalTo().window(assigner).apply(), i.e. union -> keyBy ->
    WindowOperator with ListState -> JoinCoGroupFunction.  Records are (key, ts, payload) int64
    columns per side (payload: the element as the caller numbers or packs it); a fire leaves
    (key, start, end, left payload, right payload) pairs, windows by ascending end, keys ascending,
    left-major in arrival order.  Tumbling and sliding event-time windows, allowed lateness 0.
    mode: "inner" (default), "left_outer", "right_outer", "full_outer" -- the unmatched records of
    the kept sides come as rows with null_payload in the lacking column, drain_outer() adds the
    present column -- or "cogroup": a fire leaves the groups themselves, one-sided ones included,
    as a CSR (cogroup_drain, cogroup_rows_device)."""

    LEFT, RIGHT = N.JOIN_LEFT, N.JOIN_RIGHT
    _prefix, _stats_type = "gw_join", N.GwJoinStats

    def __init__(self, assigner: WindowAssigner, device: int = 0, capacity_hint: int = 0, max_batch: int = 0,
                 mode="inner", null_payload: int = 0):
        self.assigner = assigner
        self.mode = _join_mode(mode, cogroup_ok=True)
        self.null_payload = int(null_payload)
        c = N.GwJoinConfig()
        c.assigner, c.size, c.slide, c.offset = _join_geometry(assigner)
        c.device, c.capacity_hint, c.max_batch = device, capacity_hint, max_batch
        self.cfg = c
        self._h = None

    def open(self):
        super().open()
        if self.mode != N.JOIN_MODE_INNER:
            self.set_mode(self.mode, self.null_payload)
        return self

    def set_mode(self, mode, null_payload: int = 0):
        """gw_join_set_mode: only before the first batch or watermark (GW_E_STATE afterwards)."""
        m = _join_mode(mode, cogroup_ok=True)
        self._check(N.lib().gw_join_set_mode(self._h, m, int(null_payload)))
        self.mode, self.null_payload = m, int(null_payload)

    def process_batch(self, side: int, keys, ts, payload):
        self._ingest(side, keys, ts, payload)

    def process_batch_device(self, side: int, keys, ts, payload, stream=None):
        """Columns already in HBM (torch int64 tensors), produced on `stream` (default: torch's
        current): the operator reads them behind that stream's work, and the stream waits for
        the reads."""
        self._ingest_device(side, keys, ts, payload, stream)

    def advance_watermark(self, wm: int) -> int:
        fired = ctypes.c_int64(0)
        self._check(N.lib().gw_join_advance_watermark(self._h, int(wm), ctypes.byref(fired)))
        return fired.value

    def end_input(self) -> int:
        fired = ctypes.c_int64(0)
        self._check(N.lib().gw_join_end_input(self._h, ctypes.byref(fired)))
        return fired.value

    def drain(self, cap: Optional[int] = None):
        """All pending pairs as numpy (key, start, end, left payload, right payload), copied cap
        pairs per call (default: all at once)."""
        return self._drain(N.lib().gw_join_drain, False, cap)

    def drain_outer(self, cap: Optional[int] = None):
        """drain() with the present column (uint8: 1 left only, 2 right only, 3 both) as a sixth."""
        return self._drain(N.lib().gw_join_drain_outer, True, cap)

    def rows_device_outer(self):
        """rows_device() with the present column's pointer as a sixth."""
        p = [ctypes.c_void_p() for _ in range(6)]
        n = ctypes.c_int64(0)
        self._check(N.lib().gw_join_rows_device_outer(self._h, *[ctypes.byref(x) for x in p], ctypes.byref(n)))
        return [x.value for x in p], n.value

    def cogroup_pending(self):
        """(groups, left elements, right elements) pending in coGroup mode."""
        n = (ctypes.c_int64 * 3)()
        self._check(N.lib().gw_join_cogroup_pending(self._h, n))
        return tuple(n)

    def cogroup_drain(self):
        """The pending groups of every fire since the last drain as one CSR, numpy (key, start,
        end, loff, roff, lelem, relem): group g's left payloads are lelem[loff[g]:loff[g + 1]]."""
        ng, nl, nr = self.cogroup_pending()
        g = [np.empty(ng, np.int64) for _ in range(3)] + [np.empty(ng + 1, np.int64) for _ in range(2)]
        le, re = np.empty(nl, np.int64), np.empty(nr, np.int64)
        n = (ctypes.c_int64 * 3)()
        self._check(N.lib().gw_join_cogroup_drain(self._h, *[_ptr(x) for x in g], _ptr(le), nl, _ptr(re), nr, ng, n))
        return tuple(g) + (le, re)

    def cogroup_rows_device(self):
        """Zero-copy view of the pending CSR: seven device pointers (key, start, end, loff, roff,
        lelem, relem) and (groups, left elements, right elements)."""
        p = [ctypes.c_void_p() for _ in range(7)]
        n = (ctypes.c_int64 * 3)()
        self._check(N.lib().gw_join_cogroup_rows_device(self._h, *[ctypes.byref(x) for x in p], n))
        return [x.value for x in p], tuple(n)


class JoinedStreams:
    """stream.join(other) -- JoinedStreams (RS/api/datastream/JoinedStreams.java): where(k1)
    .equal_to(k2).window(assigner).apply(join_function).execute_and_collect()."""

    def __init__(self, left: "DataStream", right: "DataStream"):
        self.left, self.right = left, right
        self._k1 = self._k2 = None
        self.assigner = None
        self._fn = None

    def where(self, key_selector) -> "JoinedStreams":
        self._k1 = key_selector
        return self

    def equal_to(self, key_selector) -> "JoinedStreams":
        if self._k1 is None:
            raise ValueError("where() before equal_to()")
        self._k2 = key_selector
        return self

    equalTo = equal_to

    def window(self, assigner: WindowAssigner) -> "JoinedStreams":
        if self._k2 is None:
            raise ValueError("where().equal_to() before window()")
        _join_geometry(assigner)  # session and count windows: unsupported
        self.assigner = assigner
        return self

    def apply(self, join_function: Callable) -> "JoinedStreams":
        if self.assigner is None:
            raise ValueError("window() before apply()")
        self._fn = join_function
        return self

    def execute_and_collect(self) -> list:
        """Both bounded sources through one join operator, the left source first (the interleaving
        of the sides does not matter to a window join); returns join_function(left, right) per
        pair as StreamRecords with timestamp end - 1, in the operator's order.  Non-integer keys
        get ids in their sorted order, so "keys ascending" is the keys' own order."""
        if self._fn is None:
            raise ValueError("apply() before execute_and_collect()")
        out = []
        with self._run() as (op, lefts, rights):
            _, _, e, lp, rp = op.drain()
            for i in range(len(e)):
                out.append(StreamRecord(self._fn(lefts[int(lp[i])].value, rights[int(rp[i])].value), int(e[i]) - 1))
        return out

    @contextlib.contextmanager
    def _run(self, **mode):
        """Both bounded sources through one operator to the end of input: yields (operator, left
        records, right records); a record's payload is its index in its side's list."""
        lefts = [e for e in self.left.elements if isinstance(e, StreamRecord)]
        rights = [e for e in self.right.elements if isinstance(e, StreamRecord)]
        keys_in, keys_out = {}, []

        def kid(key):
            if key not in keys_in:
                keys_in[key] = len(keys_out)
                keys_out.append(key)
            return keys_in[key]

        # keys ordered as the operator orders them: ids follow the sorted distinct keys
        allk = [self._k1(e.value) for e in lefts] + [self._k2(e.value) for e in rights]
        int_keys = all(isinstance(k, int) and not isinstance(k, bool) and LONG_MIN <= k <= LONG_MAX for k in allk)
        if not int_keys:
            for k in sorted(set(allk), key=lambda k: (type(k).__name__, k)):
                kid(k)
        enc = (lambda k: k) if int_keys else kid
        kw = {k: v for k, v in self.left.env.op_kwargs.items() if k in ("device", "capacity_hint", "max_batch")}
        with GpuWindowJoinOperator(self.assigner, **kw, **mode) as op:
            # the two-input operator's watermark is the minimum of its inputs' (AbstractStreamOperator
            # .processWatermark1/2): with each bounded source fed whole, the first one is end of input
            for side, elems, sel in ((op.LEFT, lefts, self._k1), (op.RIGHT, rights, self._k2)):
                if elems:
                    op.process_batch(side, [enc(sel(e.value)) for e in elems], [int(e.timestamp) for e in elems],
                                     list(range(len(elems))))
            op.end_input()
            yield op, lefts, rights


class OuterJoin:
    """A CoGroupFunction of the closed set that runs wholly on the device: the left, right or full
    outer join.  CoGroupedStreams.apply(OuterJoin(kind, fn)) runs the operator in that outer mode
    and calls fn(left_or_None, right_or_None) per row, so no per-group lists are built."""

    KINDS = {"left": N.JOIN_MODE_LEFT_OUTER, "right": N.JOIN_MODE_RIGHT_OUTER, "full": N.JOIN_MODE_FULL_OUTER}

    def __init__(self, kind: str, join_function: Callable):
        if kind not in self.KINDS:
            raise ValueError("OuterJoin kind: 'left', 'right' or 'full'")
        self.kind, self.mode, self.fn = kind, self.KINDS[kind], join_function


class CoGroupedStreams(JoinedStreams):
    """stream.co_group(other) -- CoGroupedStreams (RS/api/datastream/CoGroupedStreams.java): where(k1)
    .equal_to(k2).window(assigner).apply(co_group_function).execute_and_collect().
    co_group_function(lefts, rights) is called once per fired (window, key) with a record on either
    side, one list possibly empty, and returns an iterable of outputs; an OuterJoin runs as rows."""

    def execute_and_collect(self) -> list:
        """The outputs as StreamRecords with timestamp end - 1, groups in the operator's order
        (windows by ascending end, keys ascending), each side's elements in arrival order."""
        if self._fn is None:
            raise ValueError("apply() before execute_and_collect()")
        out = []
        if isinstance(self._fn, OuterJoin):
            with self._run(mode=self._fn.mode, null_payload=-1) as (op, lefts, rights):
                _, _, e, lp, rp, pres = op.drain_outer()
                for i in range(len(e)):
                    l = lefts[int(lp[i])].value if pres[i] & 1 else None
                    r = rights[int(rp[i])].value if pres[i] & 2 else None
                    out.append(StreamRecord(self._fn.fn(l, r), int(e[i]) - 1))
            return out
        with self._run(mode="cogroup") as (op, lefts, rights):
            _, _, e, loff, roff, le, re = op.cogroup_drain()
            for g in range(len(e)):
                ls = [lefts[int(i)].value for i in le[loff[g]:loff[g + 1]]]
                rs = [rights[int(i)].value for i in re[roff[g]:roff[g + 1]]]
                for v in self._fn(ls, rs):
                    out.append(StreamRecord(v, int(e[g]) - 1))
        return out


class GpuIntervalJoinOperator(_TwoStreamOperator):
    """Event-time interval join of two keyed streams on one MI355X (gw_ijoin): Flink's
    keyedA.intervalJoin(keyedB).between(lower, upper).process(), i.e. IntervalJoinOperator.  A left
    l and a right r pair when l.key == r.key and l.ts + lower <= r.ts <= l.ts + upper (inclusive).
    Records are (key, ts, payload) int64 columns per side; process_batch joins a batch against the
    other side's buffer as it stands and returns the number of rows it made: (key, left ts, right
    ts, left payload, right payload), the batch's records in arrival order, each one's partners by
    ascending (ts, arrival).  A watermark emits nothing; it drops the late records of later
    batches and removes the buffered records whose cleanup time has passed."""

    LEFT, RIGHT = N.JOIN_LEFT, N.JOIN_RIGHT
    _prefix, _stats_type = "gw_ijoin", N.GwIJoinStats

    def __init__(self, lower: int, upper: int, device: int = 0, capacity_hint: int = 0, max_batch: int = 0):
        lower, upper = int(lower), int(upper)
        if lower > upper:
            raise ValueError("interval join: lower bound must not be greater than the upper bound")
        if lower < -N.IJOIN_MAX_BOUND or upper > N.IJOIN_MAX_BOUND:
            raise ValueError("interval join: bounds beyond +-2^62")
        c = N.GwIJoinConfig()
        c.lower, c.upper, c.device, c.capacity_hint, c.max_batch = lower, upper, device, capacity_hint, max_batch
        self.lower, self.upper = lower, upper
        self.cfg = c
        self._h = None

    def process_batch(self, side: int, keys, ts, payload) -> int:
        rows = ctypes.c_int64(0)
        self._ingest(side, keys, ts, payload, ctypes.byref(rows))
        return rows.value

    def process_batch_device(self, side: int, keys, ts, payload, stream=None) -> int:
        """Columns already in HBM (torch int64 tensors), produced on `stream` (default: torch's
        current): the operator reads them behind that stream's work, and the stream waits for
        the reads."""
        rows = ctypes.c_int64(0)
        self._ingest_device(side, keys, ts, payload, stream, ctypes.byref(rows))
        return rows.value

    def advance_watermark(self, wm: int):
        self._check(N.lib().gw_ijoin_advance_watermark(self._h, int(wm)))

    def end_input(self):
        self._check(N.lib().gw_ijoin_end_input(self._h))

    def drain(self, cap: Optional[int] = None):
        """All pending rows as numpy (key, left ts, right ts, left payload, right payload), copied
        cap rows per call (default: all at once)."""
        return self._drain(N.lib().gw_ijoin_drain, False, cap)

    def last_times(self):
        """(probe stage ms, merge ms) of the last ingest pass on the device; waits for the stream."""
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        self._check(N.lib().gw_ijoin_last_times(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value


@dataclass
class IntervalJoinContext:
    """ProcessJoinFunction.Context: the two records' timestamps and the result's (their maximum)."""
    left_timestamp: int
    right_timestamp: int
    timestamp: int


class IntervalJoined:
    """keyedA.interval_join(keyedB) -- KeyedStream.IntervalJoin / IntervalJoined
    (RS/api/datastream/KeyedStream.java): between(lower, upper)[.lower_bound_exclusive()]
    [.upper_bound_exclusive()].process(fn).execute_and_collect()."""

    def __init__(self, left: "KeyedStream", right: "KeyedStream"):
        self.left, self.right = left, right
        self.lower = self.upper = None
        self._fn = None

    def between(self, lower, upper) -> "IntervalJoined":
        lower, upper = int(lower), int(upper)
        if lower > upper:
            raise ValueError("between(): lower bound must not be greater than the upper bound")
        self.lower, self.upper = lower, upper
        return self

    def _bounds_set(self):
        if self.lower is None:
            raise ValueError("between() first")

    def lower_bound_exclusive(self) -> "IntervalJoined":
        """IntervalJoined.lowerBoundExclusive: the lower bound plus one (checked afterwards)."""
        self._bounds_set()
        if self.lower + 1 > self.upper:
            raise ValueError("lower_bound_exclusive(): the interval would be empty")
        self.lower += 1
        return self

    def upper_bound_exclusive(self) -> "IntervalJoined":
        """IntervalJoined.upperBoundExclusive: the upper bound minus one (checked afterwards)."""
        self._bounds_set()
        if self.lower > self.upper - 1:
            raise ValueError("upper_bound_exclusive(): the interval would be empty")
        self.upper -= 1
        return self

    lowerBoundExclusive, upperBoundExclusive = lower_bound_exclusive, upper_bound_exclusive

    def process(self, process_join_function: Callable) -> "IntervalJoined":
        self._bounds_set()
        self._fn = process_join_function
        return self

    def execute_and_collect(self) -> list:
        """Both bounded sources through one interval join operator.  Unlike a window join, here
        the interleaving of the two inputs decides the result (a record meets only what the other
        side's buffer holds when it arrives, and a watermark cleans buffers and makes later
        records late), so the schedule is fixed: the sources are consumed in turn, the left up to
        and including its next Watermark, then the right up to its next, and so on; a source that
        has run out is skipped.  The records of one turn are one ingest call.  The operator's
        watermark is the minimum of the two inputs' last watermarks (Long.MIN_VALUE before an
        input's first), a finished source counting as Long.MAX_VALUE.  Returns fn(left, right,
        ctx) per pair as StreamRecords stamped max(left ts, right ts), turns in order, within a
        turn the operator's order."""
        if self._fn is None:
            raise ValueError("process() before execute_and_collect()")
        sides = (self.left, self.right)
        elems = [list(s.elements) for s in sides]
        recs = [[e for e in el if isinstance(e, StreamRecord)] for el in elems]
        keys_in = {}
        allk = [sides[sd].key_selector(e.value) for sd in (0, 1) for e in recs[sd]]
        int_keys = all(isinstance(k, int) and not isinstance(k, bool) and LONG_MIN <= k <= LONG_MAX for k in allk)
        enc = (lambda k: k) if int_keys else (lambda k: keys_in.setdefault(k, len(keys_in)))
        kw = {k: v for k, v in self.left.env.op_kwargs.items() if k in ("device", "capacity_hint", "max_batch")}
        out = []
        with GpuIntervalJoinOperator(self.lower, self.upper, **kw) as op:
            at, seen = [0, 0], [0, 0]
            wm_in = [LONG_MIN if el else LONG_MAX for el in elems]
            side = 0
            while at[0] < len(elems[0]) or at[1] < len(elems[1]):
                if at[side] < len(elems[side]):
                    batch, mark = [], None
                    while at[side] < len(elems[side]) and mark is None:
                        e = elems[side][at[side]]
                        at[side] += 1
                        if isinstance(e, Watermark):
                            mark = e.timestamp
                        else:
                            batch.append(e)
                    if batch:
                        sel = sides[side].key_selector
                        op.process_batch(side, [enc(sel(e.value)) for e in batch], [int(e.timestamp) for e in batch],
                                         list(range(seen[side], seen[side] + len(batch))))
                        seen[side] += len(batch)
                        _, lt, rt, lp, rp = op.drain()
                        for i in range(len(lt)):
                            ts = max(int(lt[i]), int(rt[i]))
                            ctx = IntervalJoinContext(int(lt[i]), int(rt[i]), ts)
                            out.append(StreamRecord(self._fn(recs[0][int(lp[i])].value, recs[1][int(rp[i])].value, ctx), ts))
                    if mark is not None:
                        wm_in[side] = max(wm_in[side], int(mark))
                    if at[side] >= len(elems[side]):
                        wm_in[side] = LONG_MAX
                    op.advance_watermark(min(wm_in))
                side = 1 - side
        return out


class WindowedStream:
    """keyBy(...).window(assigner) — WindowedStream (RS/api/datastream/WindowedStream.java:84-96)."""

    def __init__(self, keyed: "KeyedStream", assigner: WindowAssigner):
        self.keyed = keyed
        self.assigner = assigner
        self._lateness = 0
        self._trigger = None

    def allowed_lateness(self, ms: int) -> "WindowedStream":
        if ms < 0:
            raise ValueError("The allowed lateness cannot be negative.")
        self._lateness = ms
        return self

    allowedLateness = allowed_lateness

    def trigger(self, trig) -> "WindowedStream":
        self._trigger = trig
        return self

    def _op(self, agg, field, flags=0, window_function=None):
        kw = dict(self.keyed.env.op_kwargs)
        kw["flags"] = kw.get("flags", 0) | flags
        if window_function is not None:
            kw["window_function"] = window_function
        return GpuWindowOperator(self.assigner, agg, self._lateness, self._trigger, self.keyed.key_selector,
                                 (lambda v: v[field]) if field is not None else (lambda v: 0), **kw)

    # WindowedStream.sum / min / max (:660, :687, :788) on a typed field, aggregate (:310)
    def sum(self, field: int, kind: str = "i64") -> "DataStreamResult":
        return DataStreamResult(self, self._op(f"sum_{kind}", field))

    def min(self, field: int, kind: str = "i64") -> "DataStreamResult":
        return DataStreamResult(self, self._op(f"min_{kind}", field))

    def max(self, field: int, kind: str = "i64") -> "DataStreamResult":
        return DataStreamResult(self, self._op(f"max_{kind}", field))

    # reduce / aggregate with a window function (WindowedStream.java:224-276, 342-526): the
    # pre-aggregated result of each fired window goes through window_function(key, (start, end),
    # [result], out); `reduce` names the built-in ReduceFunction of the closed set ("sum_i64", ...)
    def reduce(self, function: str, field: int, window_function: Optional[Callable] = None) -> "DataStreamResult":
        return DataStreamResult(self, self._op(function, field, window_function=window_function))

    def process(self, function: str, field: Optional[int], window_function: Callable) -> "DataStreamResult":
        """aggregate(AggregateFunction, ProcessWindowFunction) with the closed-set aggregate."""
        return DataStreamResult(self, self._op(function, field, window_function=window_function))

    # WindowedStream.minBy / maxBy (:725-771): the element with the smallest / largest field,
    # the first of equal ones (first=True) or the last
    def min_by(self, field: int, first: bool = True, kind: str = "i64") -> "DataStreamResult":
        return DataStreamResult(self, self._op(f"min_{kind}", field, N.FLAG_BY_FIELD | (0 if first else N.FLAG_BY_LAST)))

    def max_by(self, field: int, first: bool = True, kind: str = "i64") -> "DataStreamResult":
        return DataStreamResult(self, self._op(f"max_{kind}", field, N.FLAG_BY_FIELD | (0 if first else N.FLAG_BY_LAST)))

    minBy = min_by
    maxBy = max_by

    def aggregate(self, function: str, field: Optional[int] = None,
                  window_function: Optional[Callable] = None) -> "DataStreamResult":
        return DataStreamResult(self, self._op(function, field, window_function=window_function))

    def count(self) -> "DataStreamResult":
        return DataStreamResult(self, self._op("count", None))


class DataStreamResult:
    def __init__(self, ws: WindowedStream, op: GpuWindowOperator):
        self.ws, self.op = ws, op

    def execute_and_collect(self) -> list:
        """Run the bounded source through the operator, like env.execute() on a MiniCluster
        with parallelism 1; returns the fired StreamRecords (watermarks dropped)."""
        env = self.ws.keyed.env
        out = []
        with self.op:
            for el in env.elements:
                if isinstance(el, Watermark):
                    self.op.process_watermark(el)
                else:
                    self.op.process_element(el)
            self.op.end_input()
            out = [r for r in self.op.get_output() if isinstance(r, StreamRecord)]
        return out

    def window_all_top_n(self, n: int, smallest: bool = False) -> "WindowAllTopN":
        """...aggregate(...) followed by a windowAll per-window top-N (Nexmark Q5's "hot items",
        Q7's highest bid): per fired window the n rows with the largest (smallest) result."""
        return WindowAllTopN(self, n, smallest)

    windowAllTopN = window_all_top_n


class WindowAllTopN:
    """keyBy().window().aggregate(...) -> windowAll top-N in one call: at every watermark the
    fired rows are ranked on the device (GpuWindowOperator.top_n_rows) and only the winners come
    to the host, as the StreamRecords the operator emits for a fired row ((key, start, end,
    result), timestamp end - 1), windows in ascending end, best first."""

    def __init__(self, result: DataStreamResult, n: int, smallest: bool = False):
        op = result.op
        if op._payload or op.window_function is not None:
            raise ValueError("window_all_top_n ranks plain aggregate rows (no minBy / first-element / window function)")
        if not 1 <= n <= N.TOPN_MAX_N:
            raise ValueError(f"top-N size must be in [1, {N.TOPN_MAX_N}]")
        self.result, self.n, self.smallest = result, n, smallest

    def execute_and_collect(self) -> list:
        op = self.result.op
        out = []

        def watermark(ts):
            op._flush()
            op.advance_watermark(ts)
            if op.pending_rows() == 0:
                return
            k, s, e, r, _ = op.top_n_rows(self.n, self.smallest)
            op.clear_rows()
            for i in range(len(k)):
                end = int(e[i])
                out.append(StreamRecord((op._decode_key(int(k[i])), int(s[i]), end, r[i]), end - 1))

        with op:
            for el in self.result.ws.keyed.env.elements:
                if isinstance(el, Watermark):
                    watermark(el.timestamp)
                else:
                    op.process_element(el)
            watermark(MAX_WATERMARK.timestamp)  # BoundedOneInput.endInput
        return out


class KeyedStream:
    def __init__(self, env, key_selector, elements=None):
        self.env, self.key_selector = env, key_selector
        self.elements = env.elements if elements is None else elements  # this stream's own source

    def interval_join(self, other: "KeyedStream") -> IntervalJoined:
        """KeyedStream.intervalJoin (RS/api/datastream/KeyedStream.java): this stream is the left
        side, `other` the right."""
        return IntervalJoined(self, other)

    intervalJoin = interval_join

    def window(self, assigner: WindowAssigner) -> WindowedStream:
        return WindowedStream(self, assigner)

    def count_window(self, size: int, slide: Optional[int] = None) -> WindowedStream:
        """KeyedStream.countWindow (KeyedStream.java:676-690)."""
        return WindowedStream(self, CountWindows(size, slide))

    countWindow = count_window


class DataStream:
    def __init__(self, env, elements=None):
        self.env = env
        self.elements = env.elements if elements is None else elements  # this stream's own source

    def key_by(self, key_selector) -> KeyedStream:
        return KeyedStream(self.env, key_selector, self.elements)

    keyBy = key_by

    def join(self, other: "DataStream") -> JoinedStreams:
        """DataStream.join (RS/api/datastream/DataStream.java): a window join with `other`."""
        return JoinedStreams(self, other)

    def co_group(self, other: "DataStream") -> "CoGroupedStreams":
        """DataStream.coGroup (RS/api/datastream/DataStream.java): a window coGroup with `other`."""
        return CoGroupedStreams(self, other)

    coGroup = co_group


class StreamExecutionEnvironment:
    """Minimal local environment: a bounded, timestamped source (list of StreamRecord and
    Watermark elements) feeding one GPU window operator."""

    def __init__(self, **op_kwargs):
        self.elements: list = []
        self.op_kwargs = op_kwargs

    @staticmethod
    def get_execution_environment(**op_kwargs) -> "StreamExecutionEnvironment":
        return StreamExecutionEnvironment(**op_kwargs)

    def from_elements(self, elements: Iterable) -> DataStream:
        self.elements = list(elements)
        return DataStream(self, self.elements)


# Keyed snapshot: a gw_snapshot blob plus its key table (id -> key), what the Java operator
# writes per key group (the blob, then the keys through the key serializer).
KEYED_MAGIC = b"GWK1"


def pack_keyed_snapshot(blob: bytes, keys: dict) -> bytes:
    out = [KEYED_MAGIC, struct.pack("<qq", len(blob), len(keys)), blob]
    for kid, key in sorted(keys.items()):
        if isinstance(key, str):
            tag, body = b"s", key.encode("utf-8")
        elif isinstance(key, bool):
            tag, body = b"z", b"\x01" if key else b"\x00"
        elif isinstance(key, int):
            tag, body = b"j", struct.pack("<q", key)
        else:
            raise TypeError(f"unsupported key type {type(key).__name__}")
        out.append(struct.pack("<q", kid) + tag + struct.pack("<i", len(body)) + body)
    return b"".join(out)


def unpack_keyed_snapshot(data: bytes):
    if data[:4] != KEYED_MAGIC:
        raise ValueError("not a keyed snapshot")
    nb, nk = struct.unpack_from("<qq", data, 4)
    p = 20
    blob = data[p:p + nb]
    p += nb
    keys = {}
    for _ in range(nk):
        kid, = struct.unpack_from("<q", data, p)
        tag = data[p + 8:p + 9]
        ln, = struct.unpack_from("<i", data, p + 9)
        body = data[p + 13:p + 13 + ln]
        p += 13 + ln
        keys[kid] = body.decode("utf-8") if tag == b"s" else (body == b"\x01" if tag == b"z" else
                                                               struct.unpack("<q", body)[0])
    if p != len(data):
        raise ValueError("trailing bytes in a keyed snapshot")
    return blob, keys


def result_value(bits: int, is_double: bool):
    if is_double:
        return struct.unpack("<d", struct.pack("<q", int(bits)))[0]
    return int(bits)
