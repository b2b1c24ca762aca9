"""The grouping sort's numpy reference (tests/sort_reference.py) against pure Python, the
comparison helper's sight of an unstable result, and the input generators' claimed properties.
No GPU: tests/test_gpu_sort.py runs gw_sort.hip against this reference."""
import numpy as np
import pytest

from tests import sort_reference as R

U32, U64 = np.uint32, np.uint64
RANGES = {U32: [(0, 1), (0, 9), (0, 26), (0, 32), (4, 30), (31, 32), (5, 5)],
          U64: [(0, 1), (0, 40), (0, 64), (20, 61), (63, 64), (5, 5)]}
TILE = 96  # small, so n <= 2000 spans many tiles, the last one partial


def py_digit(k, lo, hi):
    return (int(k) >> lo) & ((1 << (hi - lo)) - 1)


@pytest.mark.parametrize("gen", sorted(R.GENERATORS))
@pytest.mark.parametrize("dtype", [U32, U64], ids=["u32", "u64"])
def test_reference_equals_pure_python(gen, dtype):
    for lo, hi in RANGES[dtype]:
        for n in (0, 1, 2, 65, 777, 2000):
            keys = R.make_keys(gen, n, dtype, lo, hi, seed=n + hi, tile=TILE)
            vals = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint32)
            klist = keys.tolist()
            perm = sorted(range(n), key=lambda i: py_digit(klist[i], lo, hi))  # sorted() is stable
            assert R.digits(keys, lo, hi).tolist() == [py_digit(k, lo, hi) for k in klist]
            ek, ev = R.stable_sort_reference(keys, vals, lo, hi)
            assert ek.dtype == dtype and ev.dtype == np.uint32
            assert ek.tolist() == [klist[i] for i in perm], (gen, lo, hi, n)
            assert ev.tolist() == [int(vals[i]) for i in perm], (gen, lo, hi, n)
            ik, iv = R.stable_sort_reference(keys, None, lo, hi)
            assert iv.dtype == np.uint32 and iv.tolist() == perm and np.array_equal(ik, ek)


def test_digit_plan_is_the_sorts():
    assert R.digit_plan(5, 5) == []
    assert R.digit_plan(0, 1) == [(0, 1)]
    assert R.digit_plan(0, 10) == [(0, 5), (5, 5)]
    assert R.digit_plan(0, 19) == [(0, 7), (7, 6), (13, 6)]
    assert R.digit_plan(0, 26) == [(0, 9), (9, 9), (18, 8)]
    assert R.digit_plan(4, 30) == [(4, 9), (13, 9), (22, 8)]
    assert R.digit_plan(0, 32) == [(8 * i, 8) for i in range(4)]
    assert R.digit_plan(0, 64) == [(8 * i, 8) for i in range(8)]
    assert R.digit_plan(0, 63) == [(9 * i, 9) for i in range(7)]
    for lo, hi in [(0, 37), (20, 61), (23, 32), (3, 64)]:
        p = R.digit_plan(lo, hi)
        assert p[0][0] == lo and p[-1][0] + p[-1][1] == hi and all(0 < w <= 9 for _, w in p)
        assert all(a[0] + a[1] == b[0] for a, b in zip(p, p[1:]))


def test_comparison_reports_an_unstable_result():
    """A permutation that keeps the keys sorted but swaps two values inside one run of equal digits
    is what an unstable sort produces; the helper the GPU test uses must call it a mismatch and
    say where."""
    n, lo, hi, tile = 1500, 3, 6, 512
    rng = np.random.default_rng(11)
    keys = (rng.integers(0, 8, n, dtype=np.uint32) << np.uint32(lo)) | np.uint32(0x40000001)
    ek, ev = R.stable_sort_reference(keys, None, lo, hi)
    assert R.first_mismatch(ek, ev, ek.copy(), ev.copy(), tile) is None
    assert R.first_mismatch(ek, None, ek.copy(), None, tile) is None
    d = R.digits(ek, lo, hi)
    i = 700 + int(np.argmax(d[700:-1] == d[701:]))
    assert i < 1000 and d[i] == d[i + 1] and ev[i] != ev[i + 1]  # inside one run of equal digits
    gv = ev.copy()
    gv[[i, i + 1]] = gv[[i + 1, i]]
    assert np.array_equal(np.sort(gv), np.arange(n))  # still a permutation, keys still sorted
    msg = R.first_mismatch(ek, ev, ek, gv, tile)
    assert msg is not None
    assert f"first at index {i} (tile 1, offset {i - tile})" in msg
    assert f"expected key {int(ek[i]):#x} value {int(ev[i])}, got key {int(ek[i]):#x} value {int(gv[i])}" in msg
    assert msg.startswith("2 of 1500 records differ")
    # keys only cannot see it (the keys are equal), which is why the matrix carries values
    assert R.first_mismatch(ek, None, ek, None, tile) is None
    # an altered bit outside [lo, hi) is a mismatch
    gk = ek.copy()
    gk[3] ^= np.uint32(1 << 20)
    assert "first at index 3 (tile 0, offset 3)" in R.first_mismatch(ek, None, gk, None, tile)


@pytest.mark.parametrize("dtype", [U32, U64], ids=["u32", "u64"])
def test_generator_properties(dtype):
    width = 8 * np.dtype(dtype).itemsize
    n = 2000
    for lo, hi in RANGES[dtype]:
        mk = lambda g, seed=1: R.make_keys(g, n, dtype, lo, hi, seed, TILE)
        plan = R.digit_plan(lo, hi)
        # seeded
        for g in R.GENERATORS:
            assert np.array_equal(mk(g), mk(g))
        assert not np.array_equal(mk("uniform", 1), mk("uniform", 2))
        # uniform: noise over the whole width, outside [lo, hi) too
        u = mk("uniform").astype(np.uint64)
        for b in range(width):
            assert 0.4 < float(((u >> np.uint64(b)) & np.uint64(1)).mean()) < 0.6, b
        assert len(np.unique(mk("equal"))) == 1
        # two: exactly the top sorted bit differs, records alternate, the first has it set
        t = mk("two").astype(np.uint64)
        top = max(hi - 1, lo) % width
        assert int(t[0] ^ t[1]) == 1 << top and (int(t[0]) >> top) & 1 == 1
        assert np.array_equal(t[2:], t[:-2])
        # sorted / reversed by the sorted bits only; the other bits stay noise
        s, r = R.digits(mk("sorted"), lo, hi), R.digits(mk("reversed"), lo, hi)
        assert (s[1:] >= s[:-1]).all() and (r[1:] <= r[:-1]).all()
        if hi - lo < width:
            out = mk("sorted").astype(np.uint64) & ~np.uint64(((1 << (hi - lo)) - 1) << lo)
            assert (out[1:] > out[:-1]).sum() > n // 4 and (out[1:] < out[:-1]).sum() > n // 4
        # skew: ~90 % one key, and whole aligned runs of 64 of it
        k = mk("skew")
        vals, cnt = np.unique(k, return_counts=True)
        hot = vals[np.argmax(cnt)]
        assert 0.85 < cnt.max() / n < 0.95
        blocks = (k[:n // 64 * 64] == hot).reshape(-1, 64)
        assert blocks.all(axis=1).sum() >= n // 64 // 2
        assert (~blocks.all(axis=1) & blocks.any(axis=1)).sum() >= 4  # mixed waves too
        if not plan:
            continue
        sh, w = plan[0]
        # distinct_lanes: any 64 consecutive records, aligned or not, have min(64, 2^w) low digits
        d = R.digits(mk("distinct_lanes"), sh, sh + w)
        for at in list(range(0, 200)) + [n - 64]:
            assert len(np.unique(d[at:at + 64])) == min(64, 1 << w), (lo, hi, at)
        if w >= 7:
            assert len(np.unique(d)) > 64  # steps through the pass's range
        # one_bin_per_tile
        d = R.digits(mk("one_bin_per_tile"), sh, sh + w)
        bins = min(5, 1 << w)
        assert np.array_equal(d, (np.arange(n) // TILE) % bins)
        assert n // TILE > 2 * bins  # tiles share bins: look-back sums are not all zero
