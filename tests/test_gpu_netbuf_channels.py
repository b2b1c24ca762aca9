"""The segmented network-buffer decode (flink_amd/csrc/gw_netbuf.hip, NbSeg geometry): many byte
ranges, one per input channel, in one pipeline run.  Driven through gw::launch_nb_decode_seg on
buffers the test owns (tests/netbuf_channels.py: poisoned output rows and guard rows, scratch
that starts as 0xFF with a guard behind it) and through the C ABI's gw_decode_channels_device.

The reference is every range decoded by itself (tests/test_netbuf_oracle.py py_decode_full, which
the CPU suite holds against the oracle's wo_decode_stream), the watermark statuses from a Python
parse of the same bytes, concatenated in range order: the three columns, (ev_pos, ev_kind,
ev_val) with ev_pos counting the records of the whole call, and consumed / records / events per
range, all exact."""
import ctypes
import functools
import struct

import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import netbuf as NB
from tests import netbuf_streams as S
from tests.netbuf_channels import SegDecoder, check_against, reference
from tests.netbuf_native import PATTERN
from tests.test_netbuf_oracle import random_elements

pytestmark = pytest.mark.gpu

# narrow (29-byte records), 65-byte and 77-byte elements (the two-candidates-per-lane walk)
LAYOUTS = {"narrow": ("JJ", 0, 1), "wide65": ("JJJJJJI", 1, 6), "wide77": ("JJJJJJJJ", 3, 7)}
KIB = 1024


@functools.lru_cache(maxsize=None)
def decoder():
    return SegDecoder(arena_bytes=512 * KIB, rec_rows=24000, ev_rows=8192, max_ranges=256, max_chunks=640)


def elements(seed, types, kf, vf, min_bytes, p_status=0.06):
    """Whole elements of every kind, idle and active statuses among them, at least min_bytes."""
    rng = np.random.default_rng(seed)
    out = b""
    while len(out) < min_bytes:
        out += random_elements(rng, 3, types, kf, vf, p_wm=0.12, p_other=0.1, p_nots=0.1)
        if rng.random() < p_status * 3:
            out += NB.stream_status(bool(rng.integers(0, 2)))
    return out


def cut(seed, types, kf, vf, nbytes):
    """A range of exactly nbytes bytes that starts on an element and ends wherever the cut falls."""
    return elements(seed, types, kf, vf, nbytes)[:nbytes]


def run(ranges, layout, gap=0, filler=0xFF, start=0, **caps):
    types, kf, vf = layout
    D = decoder()
    D.fill(filler)
    res = D.decode(D.place(ranges, gap=gap, start=start), types, kf, vf, **caps)
    return res, reference(ranges, types, kf, vf)


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_range_lengths_and_cuts_inside_the_last_element(name):
    """Ranges of 0, 3, one element, 1023, 1024 and 1025 bytes, and a range cut at every offset of
    its last element (after a few whole ones, and as its only element), all in one call."""
    layout = LAYOUTS[name]
    types, kf, vf = layout
    one = NB.record([7] * len(types), types, 1234)
    ranges = [b"", cut(1, *layout, 3), one] + [cut(2 + n, *layout, n) for n in (1023, 1024, 1025)]
    head = elements(9, *layout, 200)
    last = NB.record(list(range(len(types))), types, 77)
    for k in range(len(last) + 1):
        ranges.append(head + last[:k])
        ranges.append(last[:k])
    ranges.append(b"")
    res, ref = run(ranges, layout)
    assert ref.code == 0 and ref.consumed[-2] == len(last) and ref.consumed[-4] == 0
    check_against(res, ref, name)


def test_truncated_element_whose_length_reaches_into_the_next_range():
    """Range 0 ends 5 bytes into a record whose length word claims 29 bytes: they would come out of
    range 1, which lies right behind it.  Range 0 reports consumed before that element, range 1
    decodes from its first byte."""
    layout = LAYOUTS["narrow"]
    rec = [NB.record((i, 10 * i), "JJ", 100 + i) for i in range(8)]
    r0 = b"".join(rec[:3]) + rec[3][:5]
    assert len(r0) % 4 == 0  # back to back: range 1 starts where range 0 ends
    r1 = NB.watermark(5) + b"".join(rec[4:])
    res, ref = run([r0, r1], layout, gap=0)
    assert ref.consumed == [87, len(r1)] and ref.rec_count == [3, 4]
    check_against(res, ref)
    assert res.key[:7].tolist() == [0, 1, 2, 4, 5, 6, 7] and res.ev_pos[0] == 3


@pytest.mark.parametrize("gap", [0, 4, 1500])
@pytest.mark.parametrize("name", ["narrow", "wide77"])
def test_bytes_outside_the_ranges_do_not_matter(name, gap):
    """Back to back and with gaps; everything outside the ranges 0xFF in one variant, a stream of
    valid elements in the other: the same result, the reference's."""
    layout = LAYOUTS[name]
    ranges = [cut(20 + i, *layout, n) for i, n in enumerate((700, 1024, 2049, 40, 3000, 1))]
    valid = elements(99, *layout, 4096)
    got = []
    for filler in (0xFF, valid):
        res, ref = run(ranges, layout, gap=gap, filler=filler, start=len(valid) // 2 & ~3)
        check_against(res, ref, (name, gap, isinstance(filler, int)))
        got.append(res)
    n, m = got[0].status.records, got[0].status.watermarks
    assert n > 0 and m > 0
    for col in ("key", "ts", "val", "ev_pos", "ev_val", "ev_kind"):
        assert np.array_equal(getattr(got[0], col), getattr(got[1], col)), col
    assert got[0].consumed == got[1].consumed


@pytest.mark.parametrize("kib", [(100, 156, 40), (101, 156, 40), (100, 155, 41)])
def test_range_boundaries_and_scan_blocks(kib):
    """More than 256 chunks (several blocks of k_nb_resolve's scan): a range boundary exactly on a
    scan-block boundary (100 + 156 KiB), the same shifted by one chunk either way (inside a
    block), ranges ending on a chunk boundary and a few bytes before and behind one."""
    layout = LAYOUTS["narrow"]
    for delta in (0, -5, 3):
        lens = [kib[0] * KIB + delta, kib[1] * KIB - delta, kib[2] * KIB]
        ranges = [cut(40 + i, *layout, n) for i, n in enumerate(lens)]
        res, ref = run(ranges, layout)
        assert res.nchunks > 256 + 32
        check_against(res, ref, (kib, delta))


def test_many_tiny_ranges():
    """128 ranges, most shorter than a chunk, some empty, a few of several chunks."""
    layout = LAYOUTS["narrow"]
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 900, 128)
    lens[rng.integers(0, 128, 12)] = 0
    lens[[0, 127]] = 0
    lens[rng.integers(1, 127, 6)] = rng.integers(1025, 5000, 6)
    ranges = [cut(200 + i, *layout, int(n)) for i, n in enumerate(lens)]
    for gap in (0, 64):
        res, ref = run(ranges, layout, gap=gap)
        assert sum(1 for c in ref.rec_count if c) > 90 and ref.consumed.count(0) >= 10
        check_against(res, ref, gap)


def test_status_events_and_positions_across_ranges():
    """Watermarks and watermark statuses keep their order, kinds and values; ev_pos counts the
    records of the whole call; latency markers and record attributes stay skipped."""
    R = lambda k: NB.record((k, -k), "JJ", 10 * k)  # noqa: E731
    r0 = R(1) + NB.stream_status(False) + R(2) + NB.watermark(15) + NB.latency_marker(1, 2, 3, 4)
    r1 = NB.stream_status(True) + NB.internal_watermark(-7, 3) + NB.record_attributes(True)
    r2 = b""
    r3 = R(3) + R(4) + R(5) + struct.pack(">i", 5) + bytes([4]) + struct.pack(">i", 7) + NB.watermark(1 << 62)
    res, ref = run([r0, r1, r2, r3], LAYOUTS["narrow"])
    check_against(res, ref)
    assert res.ev_pos[:6].tolist() == [1, 2, 2, 2, 5, 5]
    assert res.ev_kind[:6].tolist() == [1, 0, 1, 0, 1, 0]
    assert res.ev_val[:6].tolist() == [-1, 15, 0, -7, 7, 1 << 62]  # (a status value is passed on as written)
    assert res.status.skipped == 2 and ref.ev_count == [2, 2, 0, 2]


def channels_device(ranges, layout, rec_cap, ev_cap, tensors=None):
    """gw_decode_channels_device over ranges in separate allocations -> (rc, result, consumed,
    rec_count, ev_count, columns)."""
    import torch
    types, kf, vf = layout
    tensors = tensors or [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() if d else None for d in ranges]
    n = len(ranges)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in tensors])
    lens = (ctypes.c_int64 * n)(*[len(d) for d in ranges])
    cols = torch.full((3 * rec_cap + 2 * ev_cap + 8,), -1, dtype=torch.int64, device="cuda")
    kind = torch.full((ev_cap + 8,), -1, dtype=torch.int32, device="cuda")
    at = [cols.data_ptr() + 8 * o for o in (0, rec_cap, 2 * rec_cap, 3 * rec_cap, 3 * rec_cap + ev_cap)]
    consumed, rc_, ec_ = ((ctypes.c_int64 * n)() for _ in range(3))
    out = N.GwDecodeChannelsResult()
    lay = N.record_layout(types, kf, vf)
    rc = N.lib().gw_decode_channels_device(n, ptrs, lens, ctypes.byref(lay), at[0], at[1], at[2], rec_cap, at[3],
                                           kind.data_ptr(), at[4], ev_cap, consumed, rc_, ec_, ctypes.byref(out),
                                           None)
    return rc, out, list(consumed), list(rc_), list(ec_), cols.cpu().numpy(), kind.cpu().numpy()


def test_separate_allocations_through_the_c_abi():
    layout = LAYOUTS["wide65"]
    ranges = [cut(60 + i, *layout, n) for i, n in enumerate((5000, 0, 333, 1024, 12))]
    ref = reference(ranges, *layout)
    n, m = len(ref.key), len(ref.ev_pos)
    rc, out, consumed, recs, evs, cols, kind = channels_device(ranges, layout, n, m)
    assert rc == 0 and (out.records, out.events, out.skipped, out.error_range) == (n, m, ref.skipped, -1)
    assert consumed == ref.consumed and recs == ref.rec_count and evs == ref.ev_count
    assert np.array_equal(cols[:n], ref.key) and np.array_equal(cols[n:2 * n], ref.ts)
    assert np.array_equal(cols[2 * n:3 * n], ref.val)
    assert np.array_equal(cols[3 * n:3 * n + m], ref.ev_pos) and np.array_equal(cols[3 * n + m:3 * n + 2 * m], ref.ev_val)
    assert np.array_equal(kind[:m], ref.ev_kind) and (kind[m:] == -1).all() and (cols[3 * n + 2 * m:] == -1).all()


def test_earliest_error_in_range_then_byte_order():
    """The call reports the earliest error in (range, byte position): a range's late error wins
    over a later range's early one, whatever their kinds; the message names the range."""
    layout = LAYOUTS["narrow"]
    good = elements(70, *layout, 6000)
    whole = lambda n: good[:reference([good[:n]], *layout).consumed[0]]  # noqa: E731
    late_tag = whole(5000) + S.UNKNOWN_TAG + good[:200]
    late_long = whole(5000) + S.TOO_LONG + good[:200]
    early_tag = whole(100) + S.UNKNOWN_TAG + good[:200]
    early_long = whole(100) + S.TOO_LONG + good[:200]
    for ranges, code, where in [([good, late_tag, early_long], N.GW_E_INVALID, 1),
                                ([good, late_long, early_tag], N.GW_E_UNSUPPORTED, 1),
                                ([early_long, late_tag], N.GW_E_UNSUPPORTED, 0),
                                ([good, b"", good[:64], early_tag], N.GW_E_INVALID, 3)]:
        res, ref = run(ranges, layout)
        assert (ref.code, ref.error_range) == (code, where)
        check_against(res, ref, where)
        rc, out, *_ = channels_device(ranges, layout, 1000, 1000)
        assert rc == code and out.error_range == where
        assert f"range {where}" in N.lib().gw_last_error(None).decode()


def test_output_capacity_exact_and_one_short():
    layout = LAYOUTS["narrow"]
    ranges = [cut(80 + i, *layout, n) for i, n in enumerate((1500, 700, 2100))]
    ref = reference(ranges, *layout)
    n, m = len(ref.key), len(ref.ev_pos)
    res, _ = run(ranges, layout, rec_cap=n, ev_cap=m)
    check_against(res, ref, "exact")
    for caps in (dict(rec_cap=n - 1, ev_cap=m), dict(rec_cap=n, ev_cap=m - 1)):
        res, _ = run(ranges, layout, **caps)
        assert res.code == N.GW_E_OUTPUT_FULL and res.scratch_ok and res.rng_guard_ok
        # nothing is written past the capacity
        assert (res.key[caps["rec_cap"]:] == PATTERN).all() and (res.ev_pos[caps["ev_cap"]:] == PATTERN).all()


def test_argument_errors():
    import torch
    layout = LAYOUTS["narrow"]
    data = cut(90, *layout, 100)
    t = torch.frombuffer(bytearray(b"\0" + data), dtype=torch.uint8).cuda()
    rc, *_ = channels_device([data], layout, 10, 10, tensors=[t[1:]])  # not 4-byte aligned
    assert rc == N.GW_E_INVALID
    out = N.GwDecodeChannelsResult()
    lay = N.record_layout("JJ", 0, 1)
    lens = (ctypes.c_int64 * 1)(-1)
    ptrs = (ctypes.c_void_p * 1)(t.data_ptr())
    assert N.lib().gw_decode_channels_device(1, ptrs, lens, ctypes.byref(lay), None, None, None, 0, None, None, None,
                                             0, None, None, None, ctypes.byref(out), None) == N.GW_E_INVALID
    # no ranges, or only empty ones: nothing decoded, no error
    rc, out, consumed, recs, evs, _, _ = channels_device([b"", b""], layout, 4, 4)
    assert rc == 0 and (out.records, out.events) == (0, 0) and consumed == [0, 0] and recs == [0, 0]
