"""Numpy restatement of the grouping sort's contract (flink_amd/csrc/gw_sort.h), the comparison
the CPU and GPU tests share, and their seeded inputs.

Contract: a stable sort of (key, uint32 value) pairs by the key bits [lo, hi).  The keys come out
whole: bits outside [lo, hi) neither influence the order nor change.  In iota mode the values are
the arrival indices 0..n-1, so the value column of the result is the permutation itself.
"""
import numpy as np

MAX_DIGIT_BITS = 9  # kOsCfgs' maxw in gw_sort.hip
WAVE = 64


def digit_plan(lo, hi, maxw=MAX_DIGIT_BITS):
    """[(shift, width)] of the passes, lowest first: gw_sort.hip's plan_for -- the fewest digits of
    <= maxw bits (at most 8), the bits spread evenly, the wider digits first."""
    bits = max(0, hi - lo)
    npass = min(8, -(-bits // maxw))
    plan, at = [], lo
    for i in range(npass):
        w = -(-(bits - (at - lo)) // (npass - i))
        plan.append((at, w))
        at += w
    return plan


def digits(keys, lo, hi):
    """(key >> lo) & ((1 << (hi - lo)) - 1) in unsigned 64-bit arithmetic; never shifts by 64."""
    k = np.asarray(keys).astype(np.uint64)
    w = hi - lo
    if w <= 0:
        return np.zeros(k.shape, np.uint64)
    d = k >> np.uint64(lo)  # w > 0 and hi <= 64, so lo <= 63
    if w < 64:
        d &= np.uint64((1 << w) - 1)
    return d


def stable_sort_reference(keys, values, lo, hi):
    """(keys[perm], values[perm]) for the stable order by digits(keys, lo, hi); values None is iota
    mode: the second array is perm itself as uint32."""
    keys = np.asarray(keys)
    perm = np.argsort(digits(keys, lo, hi), kind="stable")
    return keys[perm], (perm.astype(np.uint32) if values is None else np.asarray(values)[perm])


def first_mismatch(exp_keys, exp_values, got_keys, got_values, tile):
    """None if the result equals the expectation bit for bit, else a message naming the first
    differing index, its tile and offset in the tile, and the expected and actual pair.
    exp_values / got_values None: keys only."""
    if got_keys.shape != exp_keys.shape or got_keys.dtype != exp_keys.dtype:
        return f"keys are {got_keys.dtype}{got_keys.shape}, expected {exp_keys.dtype}{exp_keys.shape}"
    bad = got_keys != exp_keys
    if exp_values is not None:
        if got_values is None or got_values.shape != exp_values.shape:
            return f"values are {None if got_values is None else got_values.shape}, expected {exp_values.shape}"
        bad |= got_values != exp_values
    if not bad.any():
        return None
    i = int(np.argmax(bad))

    def pair(k, v):
        return f"key {int(k[i]):#x}" + ("" if exp_values is None else f" value {int(v[i])}")

    return (f"{int(bad.sum())} of {bad.size} records differ, first at index {i} (tile {i // tile}, offset "
            f"{i % tile}): expected {pair(exp_keys, exp_values)}, got {pair(got_keys, got_values)}")


# ---- inputs ------------------------------------------------------------------------------------
# gen(n, dtype, lo, hi, seed, tile) -> n keys of dtype (uint32 / uint64).  Unless a generator says
# otherwise the bits outside [lo, hi) are noise.

def _noise(rng, n, dtype):
    return rng.integers(0, np.iinfo(dtype).max, n, dtype=dtype, endpoint=True)


def _with_low_digit(keys, d, lo, w):
    """keys with the w-bit field at lo replaced by d."""
    k = keys.astype(np.uint64)
    field = np.uint64(((1 << w) - 1) << lo)
    return ((k & ~field) | (np.asarray(d).astype(np.uint64) << np.uint64(lo))).astype(keys.dtype)


def uniform(n, dtype, lo, hi, seed, tile):
    return _noise(np.random.default_rng(seed), n, dtype)


def equal(n, dtype, lo, hi, seed, tile):
    return np.full(n, _noise(np.random.default_rng(seed), 1, dtype)[0], dtype)


def two(n, dtype, lo, hi, seed, tile):
    """Two keys differing in the top sorted bit only, alternating; the first has the bit set, so
    every even record moves behind every odd one.  (hi == lo: the bit at lo, which sorts nothing.)"""
    bit = dtype(1) << dtype(max(hi - 1, lo) % (8 * np.dtype(dtype).itemsize))
    a = _noise(np.random.default_rng(seed), 1, dtype)[0] | bit
    k = np.full(n, a, dtype)
    k[1::2] = a ^ bit
    return k


def sorted_(n, dtype, lo, hi, seed, tile):
    k = _noise(np.random.default_rng(seed), n, dtype)
    return k[np.argsort(digits(k, lo, hi), kind="stable")]


def reversed_(n, dtype, lo, hi, seed, tile):
    return sorted_(n, dtype, lo, hi, seed, tile)[::-1].copy()


def skew(n, dtype, lo, hi, seed, tile):
    """About 90 % one key, the rest uniform.  By aligned blocks of 64 records (what a wave ranks
    at once): every 16th block is all uniform, every fourth has the hot key with 15 % uniform
    records scattered in, the others are all the hot key (one ballot group of 64)."""
    rng = np.random.default_rng(seed)
    k = _noise(rng, n, dtype)
    hot = _noise(rng, 1, dtype)[0]
    block = np.arange(n) // WAVE
    cold = (block % 16 == 0) | ((block % 4 == 1) & (rng.random(n) < 0.15))
    k[~cold] = hot
    return k


def distinct_lanes(n, dtype, lo, hi, seed, tile):
    """Any 64 consecutive records have 64 different digits in the lowest pass (2^width if the
    pass is narrower than 6 bits): every lane is its own ballot group.  The digits step through
    the pass's whole range and rotate from one run of 64 to the next."""
    k = _noise(np.random.default_rng(seed), n, dtype)
    plan = digit_plan(lo, hi)
    if not plan:
        return k
    w = plan[0][1]
    m = min(WAVE, 1 << w)
    g = (1 << w) // m
    i = np.arange(n)
    return _with_low_digit(k, (i % m) * g + (i // m) % g, lo, w)


def one_bin_per_tile(n, dtype, lo, hi, seed, tile, bins=5):
    """Every record of tile t has the lowest pass's digit t mod bins, so a tile contributes to one
    bin and publishes zero counts for the others.  bins is small (5, or 2^width if that is less) so
    that tiles share bins even at ten tiles: with one bin per tile and no sharing every look-back
    sum would be zero, and a look-back that returned zero would pass."""
    k = _noise(np.random.default_rng(seed), n, dtype)
    plan = digit_plan(lo, hi)
    if not plan:
        return k
    w = plan[0][1]
    return _with_low_digit(k, (np.arange(n) // tile) % min(bins, 1 << w), lo, w)


GENERATORS = {"uniform": uniform, "equal": equal, "two": two, "sorted": sorted_, "reversed": reversed_,
              "skew": skew, "distinct_lanes": distinct_lanes, "one_bin_per_tile": one_bin_per_tile}


def make_keys(gen, n, dtype, lo, hi, seed, tile):
    k = GENERATORS[gen](n, dtype, lo, hi, seed, tile)
    assert k.dtype == dtype and k.shape == (n,)
    return k
