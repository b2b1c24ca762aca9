"""tests/cogroup_reference.py against hand-written vectors of the coGroup / outer-join contract
(include/gpuwin.h), against tests/join_reference.py on the seeded grid, and against the CPU
oracle: a coGroup is union -> keyBy -> window, so the fired groups with their L + R are exactly
the oracle's `count` rows over the union of both sides, one-sided groups included.  No GPU."""
import zlib

import numpy as np
import pytest

from tests import cogroup_reference as C
from tests import join_reference as R
from tests.gpu_helpers import random_stream

X = C.NULL


def cols(*recs):
    a = np.array(recs, np.int64).reshape(-1, 3)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def rows(out):
    return list(zip(*[c.tolist() for c in out]))


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0xffffffff


# key 1 left only, key 2 two-sided (2 x 1), key 3 right only (two records), one tumbling window
LEFT = cols((2, 1, 100), (1, 2, 101), (2, 3, 102))
RIGHT = cols((3, 4, 200), (2, 5, 201), (3, 0, 202))


def test_one_window_with_a_left_only_a_two_sided_and_a_right_only_group():
    both = [(2, 0, 10, 100, 201, 3), (2, 0, 10, 102, 201, 3)]
    lo, ro = [(1, 0, 10, 101, X, 1)], [(3, 0, 10, X, 200, 2), (3, 0, 10, X, 202, 2)]
    assert rows(C.reference_rows(LEFT, RIGHT, 10, 10, 0, C.INNER)) == both
    assert rows(C.reference_rows(LEFT, RIGHT, 10, 10, 0, C.LEFT_OUTER)) == lo + both
    assert rows(C.reference_rows(LEFT, RIGHT, 10, 10, 0, C.RIGHT_OUTER)) == both + ro
    assert rows(C.reference_rows(LEFT, RIGHT, 10, 10, 0, C.FULL_OUTER)) == lo + both + ro
    assert rows(C.reference_rows(LEFT, RIGHT, 10, 10, 0, C.FULL_OUTER, null=0))[0] == (1, 0, 10, 101, 0, 1)


def test_csr_of_the_same_window():
    key, start, end, loff, roff, le, re = C.reference_csr(LEFT, RIGHT, 10, 10, 0)
    assert key.tolist() == [1, 2, 3] and start.tolist() == [0, 0, 0] and end.tolist() == [10, 10, 10]
    assert loff.tolist() == [0, 1, 3, 3] and roff.tolist() == [0, 0, 1, 3]
    assert le.tolist() == [101, 100, 102] and re.tolist() == [201, 200, 202]
    empty = C.reference_csr(cols(), cols(), 10, 10, 0)
    assert [len(c) for c in empty] == [0, 0, 0, 1, 1, 0, 0] and empty[3][0] == 0 and empty[4][0] == 0


def test_sliding_record_unmatched_in_one_window_and_matched_in_another():
    # left ts 7: windows [0, 10) and [5, 15); right ts 12: [5, 15) and [10, 20)
    left, right = cols((4, 7, 1)), cols((4, 12, 2))
    assert rows(C.reference_rows(left, right, 10, 5, 0, C.FULL_OUTER)) == [
        (4, 0, 10, 1, X, 1), (4, 5, 15, 1, 2, 3), (4, 10, 20, X, 2, 2)]
    assert rows(C.reference_rows(left, right, 10, 5, 0, C.LEFT_OUTER)) == [(4, 0, 10, 1, X, 1), (4, 5, 15, 1, 2, 3)]
    assert rows(C.reference_rows(left, right, 10, 5, 0, C.RIGHT_OUTER)) == [(4, 5, 15, 1, 2, 3), (4, 10, 20, X, 2, 2)]
    # only the windows whose end - 1 lies in (w0, w1]
    assert rows(C.reference_rows(left, right, 10, 5, 0, C.FULL_OUTER, w0=9, w1=14)) == [(4, 5, 15, 1, 2, 3)]
    assert C.reference_csr(left, right, 10, 5, 0)[3].tolist() == [0, 1, 2, 2]


def test_one_empty_side_is_not_empty():
    none = cols()
    assert rows(C.reference_rows(none, RIGHT, 10, 10, 0, C.FULL_OUTER)) == [
        (2, 0, 10, X, 201, 2), (3, 0, 10, X, 200, 2), (3, 0, 10, X, 202, 2)]
    assert rows(C.reference_rows(none, RIGHT, 10, 10, 0, C.LEFT_OUTER)) == []
    assert len(C.reference_rows(LEFT, none, 10, 10, 0, C.LEFT_OUTER)[0]) == 3
    assert rows(C.reference_rows(none, none, 10, 10, 0, C.FULL_OUTER)) == []


def test_signed_key_order_and_errors():
    out = C.reference_rows(cols((-1, 1, 5), (R.I64_MIN, 1, 6)), cols((R.I64_MAX, 1, 7), (0, 1, 8)), 10, 10, 0, C.FULL_OUTER)
    assert out[0].tolist() == [R.I64_MIN, -1, 0, R.I64_MAX] and out[5].tolist() == [1, 1, 2, 2]
    with pytest.raises(R.NoTimestamp):
        C.reference_rows(cols(), cols((1, R.I64_MIN, 0)), 10, 10, 0, C.RIGHT_OUTER)
    with pytest.raises(R.WindowRange):
        C.reference_csr(cols((1, R.I64_MAX - 2, 0)), cols(), 10, 10, 0)
    with pytest.raises(R.Unsupported):
        C.reference_csr(cols((1, 0, 0)), cols(), 65, 1, 0)


def test_operator_modes_fire_one_sided_groups_and_count_late_records():
    for mode, want9 in ((C.INNER, []), (C.RIGHT_OUTER, [(2, 0, 10, X, 200, 2)]), (C.FULL_OUTER, [(2, 0, 10, X, 200, 2)])):
        op = C.ReferenceCoGroupOperator(10, 5, mode=mode)
        op.ingest(1, *cols((2, 6, 200)))                 # windows [0, 10) and [5, 15)
        assert rows(op.advance_watermark(9)) == want9    # [0, 10) fires with the right side only
        op.ingest(0, *cols((2, 7, 100), (2, 3, 101)))    # ts 3: its last window [0, 10) has passed
        assert op.late_dropped == 1
        assert rows(op.advance_watermark(9)) == []       # does not advance
        assert rows(op.end_input()) == [(2, 5, 15, 100, 200, 3)]
    op = C.ReferenceCoGroupOperator(10, 10, mode=C.COGROUP)
    op.ingest(0, *LEFT)
    assert C.expand_csr(op.advance_watermark(9))[0].tolist() == [] and op.fired == 2
    op.ingest(1, *cols((1, 12, 9)))
    csr = op.end_input()
    assert csr[0].tolist() == [1] and csr[3].tolist() == [0, 0] and csr[4].tolist() == [0, 1] and op.fired == 3


GEOMETRIES = {"tumbling": (10, 10, 0), "sliding": (10, 5, 0), "sliding_3_1": (10, 3, 1)}
INTERVALS = {"all": (R.I64_MIN, R.I64_MAX), "partial": (-3, 27)}
GRID = [(n_l, n_r, k, g, i) for n_l in (0, 1, 64, 300) for n_r in (0, 1, 64, 300) for k in (1, 7, 500)
        for g in GEOMETRIES for i in INTERVALS]


@pytest.mark.parametrize("n_l,n_r,num_keys,geometry,interval", GRID)
def test_modes_and_csr_against_the_join_reference(n_l, n_r, num_keys, geometry, interval):
    size, slide, offset = GEOMETRIES[geometry]
    w0, w1 = INTERVALS[interval]
    left, right = R.make_records(_seed(n_l, n_r, num_keys, geometry), n_l, n_r, num_keys)
    inner = R.reference(left, right, size, slide, offset, w0, w1)
    got = C.reference_rows(left, right, size, slide, offset, C.INNER, C.NULL, w0, w1)
    R.check(got[:5], inner)
    assert (got[5] == 3).all()
    # the CSR expanded by the nested loop is the inner join
    csr = C.reference_csr(left, right, size, slide, offset, w0, w1)
    R.check(C.expand_csr(csr), inner)
    # full outer = inner plus exactly the unmatched records, each once per fired window of its own
    full = C.reference_rows(left, right, size, slide, offset, C.FULL_OUTER, C.NULL, w0, w1)
    both = full[5] == 3
    R.check([c[both] for c in full[:5]], inner)
    matched = [set(zip(inner[1].tolist(), inner[3].tolist())), set(zip(inner[1].tolist(), inner[4].tolist()))]
    for side, (recs, pres, col) in enumerate(((left, 1, 3), (right, 2, 4))):
        want = []
        for k, t, p in zip(*[c.tolist() for c in recs]):
            for s in R.window_starts(t, size, slide, offset)[1]:
                if w0 < s + size - 1 <= w1 and (s, p) not in matched[side]:
                    want.append((k, s, s + size, p))
        m = full[5] == pres
        have = list(zip(full[0][m].tolist(), full[1][m].tolist(), full[2][m].tolist(), full[col][m].tolist()))
        assert sorted(have) == sorted(want) and len(set(have)) == len(have)
        assert (full[7 - col][m] == C.NULL).all()
        one = C.reference_rows(left, right, size, slide, offset, pres, C.NULL, w0, w1)
        keep = both | m
        C.check_rows(one, [c[keep] for c in full])
    assert len(full[0]) == int(both.sum()) + int((full[5] == 1).sum()) + int((full[5] == 2).sum())


ORACLE_GEOMETRIES = [dict(assigner="tumbling", size=100), dict(assigner="sliding", size=100, slide=50),
                     dict(assigner="sliding", size=100, slide=30, offset=10)]


@pytest.mark.parametrize("seed", range(21))
def test_groups_match_the_oracle_count(oracle_lib, seed):
    geo = ORACLE_GEOMETRIES[seed % 3]
    size, slide, offset = geo["size"], geo.get("slide", geo["size"]), geo.get("offset", 0)
    keys, ts, _, batches = random_stream(seed, 600, 9, 6, disorder=600, wm_lag=50, agg="count")
    side = np.random.default_rng(1000 + seed).integers(0, 2, len(keys))
    pay = np.arange(len(keys), dtype=np.int64)
    ora = oracle_lib.OracleOperator(oracle_lib.make_config(agg="count", **geo))
    ref = C.ReferenceCoGroupOperator(size, slide, offset, mode=C.COGROUP)
    fired = one_sided = 0
    for lo, hi, wm in batches + [(len(keys), len(keys), R.I64_MAX)]:
        sl = slice(lo, hi)
        ora.process_batch(keys[sl], ts[sl], np.zeros(hi - lo, np.int64))
        for sd in (0, 1):
            m = side[sl] == sd
            ref.ingest(sd, keys[sl][m], ts[sl][m], pay[sl][m])
        ora.process_watermark(wm)
        key, start, end, loff, roff, le, re = ref.advance_watermark(wm)
        k, s, e, r = ora.drain()
        want = {(int(s[i]), int(k[i])): int(r[i]) for i in range(len(k))}
        sizes = (np.diff(loff) + np.diff(roff)).tolist()
        got = {(int(start[g]), int(key[g])): sizes[g] for g in range(len(key))}
        assert got == want and len(got) == len(key)
        assert (end == start + size).all()
        one_sided += int(((np.diff(loff) == 0) | (np.diff(roff) == 0)).sum())
        fired += len(want)
    assert fired > 0 and one_sided > 0 and ref.fired == fired
    assert ref.late_dropped == ora.late_dropped and ref.late_dropped > 0
