"""Buffers that grow while they hold live contents (gw_devmem.h DevCols::reserve_keep behind
ensure_output, ensure_late, ensure_refire, the composite's and the first-element handle's
waiting rows, the payload log, and the session path's ensure_rows / ensure_late).

The row, late and re-fire columns start at 1 << 16 entries, so every case here is the smallest
that needs more than that while earlier rows are still pending: nothing is drained between
the step that fills the buffer and the step that outgrows it.  What is drained afterwards must
equal the oracle's output for the same stream, the rows from before the growth included.  Each
test first asserts, from the oracle's own counts, that its stream does cross the capacity.

Growth from empty or after a drain is what every other GPU test does; the payload log's ring
re-layout without a growth is covered by test_gpu_first_element.py."""
import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import windowing as W
from tests.gpu_helpers import compare, gpu_operator, random_stream

pytestmark = pytest.mark.gpu

FLOOR = 1 << 16  # smallest capacity of the row / late / re-fire columns (gw_runtime.cpp, gw_session.hip)
NKEY = 40_000


def _cat(parts, ncol=4):
    return tuple(np.concatenate([np.asarray(p[c]).view(np.int64) for p in parts]) for c in range(ncol))


def _late_multiset(cols):
    return sorted(zip(*[c.tolist() for c in cols]))


class Pair:
    """The GPU operator and the oracle, fed alike."""

    def __init__(self, o, kw, flags=0, capacity_hint=1 << 17):
        self.op = gpu_operator(kw, flags=flags, capacity_hint=capacity_hint)
        self.ora = o.OracleOperator(o.make_config(**kw, flags=flags))

    def batch(self, keys, ts, vals):
        self.op.process_batch(keys, ts, vals)
        self.ora.process_batch(keys, ts, vals)

    def watermark(self, wm):
        self.op.advance_watermark(wm)
        self.ora.process_watermark(wm)

    def close(self):
        self.op.close()
        self.ora.close()


def _two_rounds(o, kw):
    """NKEY keys with one record each in two consecutive windows / sessions, a watermark behind
    each round that fires it, one drain at the end."""
    p = Pair(o, kw)
    keys = np.arange(NKEY, dtype=np.int64)
    exp = []
    for r, (t, wm) in enumerate([(10, 999), (1010, 1999)]):
        p.batch(keys, np.full(NKEY, t, np.int64), keys * 3 + r)
        p.watermark(wm)
        exp.append(p.ora.drain())
        assert len(exp[-1][0]) == NKEY
        assert p.op.pending_rows() == NKEY * (r + 1)  # nothing drained: round 1's rows wait
    assert 2 * NKEY > FLOOR > NKEY  # the second fire outgrows the columns that hold the first one's rows
    k, s, e, res = p.op.drain()
    assert compare([(k, s, e, res.view(np.int64))], [_cat(exp)], False) == []
    p.close()


def test_pane_rows_grow_with_rows_pending(oracle_lib):
    _two_rounds(oracle_lib, dict(assigner="tumbling", size=1000, agg="sum_i64"))


def test_session_rows_grow_with_rows_pending(oracle_lib):
    _two_rounds(oracle_lib, dict(assigner="session", gap=100, agg="sum_i64"))


def _late_batches(sizes, late_ts, ok_ts):
    """Batches of distinct keys in which every 4th record carries late_ts, the others ok_ts."""
    out, k0 = [], 1000
    for n in sizes:
        i = np.arange(n, dtype=np.int64)
        out.append((k0 + i, np.where(i % 4 == 0, late_ts, ok_ts).astype(np.int64), i * 7 + 1))
        k0 += n
    return out


def _late_side_output(o, kw, sizes, need_of):
    """An on-time batch and a watermark, then `sizes` batches with every 4th record late and
    no drain of the side output until the end.  need_of(late so far, batch size): the
    capacity the operator asks for before that batch."""
    p = Pair(o, kw, flags=N.FLAG_LATE_SIDE_OUTPUT)
    first = np.arange(100, dtype=np.int64)
    p.batch(first, np.full(100, 500, np.int64), first)
    p.watermark(999)
    rows_g, rows_o = [p.op.drain()], [p.ora.drain()]
    assert len(p.op.drain_late()[0]) == 0 and len(p.ora.drain_late()[0]) == 0
    late, side_o, needs = 0, [], []
    for keys, ts, vals in _late_batches(sizes, late_ts=10, ok_ts=1500):
        needs.append(need_of(late, len(keys)))
        p.batch(keys, ts, vals)
        side_o.append(p.ora.drain_late())
        assert len(side_o[-1][0]) == len(keys) // 4
        late += len(keys) // 4
    # the last batch outgrows the columns that hold the earlier batches' late records
    assert max(needs[:-1]) <= FLOOR < needs[-1] and late > len(side_o[-1][0])
    got = p.op.drain_late()
    assert len(got[0]) == late
    assert _late_multiset(got) == _late_multiset(_cat(side_o, 3))
    assert p.op.num_late_records_dropped == p.ora.late_dropped
    p.watermark(W.LONG_MAX)
    rows_g.append(p.op.drain())
    rows_o.append(p.ora.drain())
    assert compare([_cat(rows_g)], [_cat(rows_o)], False) == []
    p.close()
    return late


def test_pane_late_output_grows_with_records_pending(oracle_lib):
    # asked for: every record since the side output was last emptied (lo_bound) + the batch
    late = _late_side_output(oracle_lib, dict(assigner="tumbling", size=1000, agg="sum_i64"), [NKEY, NKEY],
                             lambda late, n: 100 + 4 * late + n)
    assert late == 20_000


def test_session_late_output_grows_with_records_pending(oracle_lib):
    """The session path asks for the late records so far + the batch, so the two batches of the
    pane case (10 000 late + 40 000) stay within 1 << 16: a third batch of 50 000 crosses it
    with 20 000 late records pending."""
    late = _late_side_output(oracle_lib, dict(assigner="session", gap=100, agg="sum_i64"), [NKEY, NKEY, 50_000],
                             lambda late, n: late + n)
    assert late == 32_500


def test_refire_list_grows_with_records_pending(oracle_lib):
    """Lateness > 0: every 4th record of two batches belongs to the fired, not yet cleaned
    window [0, 1000); they wait on the re-fire list until the next watermark."""
    p = Pair(oracle_lib, dict(assigner="tumbling", size=1000, agg="sum_i64", lateness=5000))
    first = np.arange(100, dtype=np.int64)
    p.batch(first, np.full(100, 500, np.int64), first)
    p.watermark(999)
    assert compare([p.op.drain()], [p.ora.drain()], False) == []
    for keys, ts, vals in _late_batches([NKEY, NKEY], late_ts=10, ok_ts=1500):
        p.batch(keys, ts, vals)
    assert NKEY <= FLOOR < 2 * NKEY  # asked for: the records since the last watermark + the batch
    p.watermark(1999)
    exp = p.ora.drain()
    assert int((exp[1] == 0).sum()) == 20_000 and int((exp[1] == 1000).sum()) == 60_000
    k, s, e, r = p.op.drain()
    assert compare([(k, s, e, r.view(np.int64))], [exp], False) == []
    assert p.op.num_late_records_dropped == p.ora.late_dropped == 0
    p.watermark(W.LONG_MAX)
    assert compare([p.op.drain()], [p.ora.drain()], False) == []
    p.close()


def test_composite_rows_grow_with_rows_pending(oracle_lib):
    """Window classes (ring > 64 panes): gw_rows_device gathers the children's rows behind the
    ones still waiting, so the second call outgrows a buffer sized for the first."""
    kw = dict(assigner="sliding", size=70_000, slide=1_000, agg="sum_i64")
    keys, ts, vals, batches = random_stream(seed=41, n=20_000, num_keys=200, n_batches=2, ts_step=5, disorder=100,
                                            wm_lag=150)
    p = Pair(oracle_lib, kw, capacity_hint=1024)
    exp, seen = [], []
    for lo, hi, wm in batches:
        p.batch(keys[lo:hi], ts[lo:hi], vals[lo:hi])
        p.watermark(wm)
        exp.append(p.ora.drain())
        seen.append(p.op.rows_device()[1])
    n1, n2 = len(exp[0][0]), len(exp[1][0])
    assert n1 > 0 and n2 > 0  # the buffer holds the first call's rows exactly: the second has to grow it
    assert seen == [n1, n1 + n2]
    k, s, e, r = p.op.drain()
    assert compare([(k, s, e, r.view(np.int64))], [_cat(exp)], False) == []
    p.close()


def _first_element(o, kw, keys, ts, vals, payload, script):
    """script: (lo, hi) batches and watermarks (ints), no drain before the end.  The payload of
    a row is that of its window's first element: the oracle run as MIN over arrival sequences."""
    op = gpu_operator(kw, flags=N.FLAG_FIRST_ELEMENT)
    agg = o.OracleOperator(o.make_config(**kw))
    seq = o.OracleOperator(o.make_config(**dict(kw, agg="min_i64")))
    order = np.arange(len(keys), dtype=np.int64)
    fired = []
    for step in script:
        if isinstance(step, tuple):
            lo, hi = step
            op.process_batch_payload(keys[lo:hi], ts[lo:hi], vals[lo:hi], payload[lo:hi])
            agg.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi])
            seq.process_batch(keys[lo:hi], ts[lo:hi], order[lo:hi])
        else:
            op.advance_watermark(step)
            agg.process_watermark(step)
            seq.process_watermark(step)
            fired.append(op.pending_rows())
    a, q = agg.drain(), seq.drain()
    ia, iq = np.lexsort((a[2], a[1], a[0])), np.lexsort((q[2], q[1], q[0]))
    assert all(np.array_equal(a[c][ia], q[c][iq]) for c in range(3))
    k, s, e, r, pay = op.drain_payload()
    ig = np.lexsort((e, s, k))
    assert compare([(k, s, e, r.view(np.int64))], [a], False) == []
    assert np.array_equal(pay[ig], payload[q[3][iq]])
    for x in (op, agg, seq):
        x.close()
    return fired


def test_first_element_rows_grow_with_rows_pending(oracle_lib):
    kw = dict(assigner="tumbling", size=100, agg="min_i64")
    keys, ts, vals, batches = random_stream(seed=43, n=20_000, num_keys=80, n_batches=2, ts_step=3, disorder=250,
                                            wm_lag=250, agg="min_i64")
    payload = np.random.default_rng(44).integers(-(1 << 62), 1 << 62, len(keys)).astype(np.int64)
    script = [s for lo, hi, wm in batches for s in ((int(lo), int(hi)), wm)]
    n1, n2 = _first_element(oracle_lib, kw, keys, ts, vals, payload, script)
    assert n2 > n1 > 0  # the buffer holds the first join's rows exactly: the second has to grow it


def test_payload_log_grows_with_sequences_live(oracle_lib):
    """1.1M records before the first watermark: the payload log (1 << 20 sequences at first)
    grows at the fourth batch, with the first three batches' sequences live."""
    n, part = 1_100_000, 275_000
    assert 3 * part <= 1 << 20 < n
    rng = np.random.default_rng(45)
    keys = rng.integers(0, 1000, n).astype(np.int64)
    ts = np.arange(n, dtype=np.int64)
    vals = rng.integers(-(10 ** 6), 10 ** 6, n).astype(np.int64)
    payload = rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64)
    kw = dict(assigner="tumbling", size=100_000, agg="min_i64")
    script = [(lo, lo + part) for lo in range(0, n, part)] + [W.LONG_MAX]
    assert _first_element(oracle_lib, kw, keys, ts, vals, payload, script) == [11 * 1000]
