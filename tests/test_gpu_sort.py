"""The grouping radix sort (flink_amd/csrc/gw_sort.hip) by itself, against the stable numpy
reference of tests/sort_reference.py: every result is compared bit for bit (keys and values: an
integer permutation has no tolerance), read from the pair result_in_alt names.

What the cases are for:
* sizes around a wave's share of a tile, a tile, four and eight tiles (the look-back reads four
  predecessors per round trip) with a partial last tile, and 1,000,003 records (163 / 245 tiles:
  tiles publish out of order and the look-back's re-read loop runs);
* bit ranges from 0 and 1 bit to the 4 x 8 plan of 32 bits and the 8 x 8 plan of 64, with lo > 0,
  over inputs whose bits outside [lo, hi) are noise: they must not order anything and must come
  out unchanged;
* explicit values (carried, not regenerated), arrival indices over a dirty v0, keys only;
* every buffer, the scratch of exactly sort_scratch_bytes(n) bytes included, between two 4-KiB
  guard bands that must come out untouched; the scratch starts filled with 0x80000000, an
  "inclusive prefix 0" look-back word, so a word the sort fails to zero gives a wrong position
  inside the output and not a wait or a stray address (the head of the scratch -- histograms and
  tile counters -- is covered by sort_pairs_impl's memset together with the first pass's words).
"""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

from tests import sort_reference as R
from tests.sort_native import sort_entry_points

pytestmark = pytest.mark.gpu

# Records per tile (one workgroup): kOsCfgs' defaults in gw_sort.hip, {512, 12} for 4-byte keys
# and {512, 8} for 8-byte keys (os_cfg; GW_SORT_CFG is not set here).  A wave ranks T / 8 of them.
TILE = {"u32": 512 * 12, "u64": 512 * 8}
DTYPE = {"u32": np.uint32, "u64": np.uint64}
BIG = 1_000_003

GUARD_WORDS = 1024  # 4 KiB on each side of every buffer
SENTINEL = 0x5AA55AA5
INCLUSIVE_ZERO = -(1 << 31)  # 0x80000000 in int32 storage


def sizes(d):
    t, w = TILE[d], TILE[d] // 8
    return [0, 1, 2, 63, 64, 65, w - 1, w, w + 1, t - 1, t, t + 1, 2 * t, 4 * t + 1, 5 * t, 8 * t + 1,
            9 * t + w + 3, BIG]


def two_sizes(d):
    t = TILE[d]
    return [t + 1, 9 * t + t // 8 + 3]


RANGES = {"u32": [(0, 1), (0, 9), (0, 10), (0, 19), (0, 26), (0, 32), (4, 30), (23, 32), (31, 32), (5, 5)],
          "u64": [(0, 1), (0, 37), (0, 40), (0, 63), (0, 64), (20, 61), (32, 33), (63, 64), (7, 7)]}
MODES = ["explicit", "iota", "keys"]


class Guarded:
    """nbytes of device memory (int32 storage; torch has no unsigned arithmetic to rely on, numpy
    views the words) between two guard bands of the sentinel."""

    def __init__(self, nbytes, fill=SENTINEL):
        assert nbytes % 4 == 0
        self.words = nbytes // 4
        self.t = torch.full((2 * GUARD_WORDS + self.words,), SENTINEL, dtype=torch.int32, device="cuda")
        if fill != SENTINEL:
            self.payload().fill_(fill)
        self.ptr = self.t.data_ptr() + 4 * GUARD_WORDS
        assert self.ptr % 8 == 0

    def payload(self):
        return self.t[GUARD_WORDS:GUARD_WORDS + self.words]

    def write(self, arr):
        assert arr.nbytes == 4 * self.words
        self.payload().copy_(torch.from_numpy(np.ascontiguousarray(arr).view(np.int32).copy()))
        return self

    def read(self, dtype):
        """(payload as dtype, both guard bands untouched)"""
        h = self.t.cpu().numpy()
        ok = (h[:GUARD_WORDS] == SENTINEL).all() and (h[GUARD_WORDS + self.words:] == SENTINEL).all()
        return h[GUARD_WORDS:GUARD_WORDS + self.words].view(dtype), bool(ok)


@functools.lru_cache(maxsize=None)
def entry_points():
    return sort_entry_points()


class Case:
    """Seeded keys and values and their reference orders; computed once, read-only."""

    def __init__(self, gen, d, n, lo, hi):
        seed = zlib.crc32(f"{gen}/{d}/{n}/{lo}/{hi}".encode())
        self.d, self.n, self.lo, self.hi = d, n, lo, hi
        self.keys = R.make_keys(gen, n, DTYPE[d], lo, hi, seed, TILE[d])
        self.values = np.random.default_rng(seed + 1).integers(0, 1 << 32, n, dtype=np.uint32)
        self.keys.flags.writeable = self.values.flags.writeable = False
        self._ref = {}

    def expected(self, mode):
        """(keys, values or None) of the contract."""
        kind = "explicit" if mode == "explicit" else "iota"
        if kind not in self._ref:
            self._ref[kind] = R.stable_sort_reference(self.keys, self.values if kind == "explicit" else None,
                                                      self.lo, self.hi)
            for a in self._ref[kind]:
                a.flags.writeable = False
        ek, ev = self._ref[kind]
        return ek, (ev if mode in ("explicit", "iota") else None)


@functools.lru_cache(maxsize=4)
def case(gen, d, n, lo, hi):
    return Case(gen, d, n, lo, hi)


def run_sort(c, mode, scratch=None, stream=None, fn=None):
    """One sort of c's keys on the device, checked against the reference.  mode: explicit values,
    iota over a dirty v0, keys (null values) or iota_null (iota asked for with null values).
    scratch: a Guarded to reuse as it is (default: exactly sort_scratch_bytes(n) bytes of
    "inclusive prefix 0" words).  fn(k0, v0, k1, v1, n, scratch, stream, alt): another entry point
    to call instead of sort_pairs_*.  Returns (keys, values) as read from the device."""
    S = entry_points()
    n, isz = c.n, np.dtype(DTYPE[c.d]).itemsize
    k0, k1 = Guarded(n * isz).write(c.keys), Guarded(n * isz)
    v0 = v1 = None
    if mode == "explicit":
        v0, v1 = Guarded(n * 4).write(c.values), Guarded(n * 4)
    elif mode == "iota":
        v0, v1 = Guarded(n * 4).write(~c.values), Guarded(n * 4)  # v0's contents are not read
    if scratch is None:
        scratch = Guarded(S.sort_scratch_bytes(n), fill=INCLUSIVE_ZERO)
    bufs = {"k0": k0, "k1": k1, "scratch": scratch}
    if v0 is not None:
        bufs.update(v0=v0, v1=v1)
    torch.cuda.synchronize()
    handle = stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream
    alt = ctypes.c_int(-1)
    ptr = lambda b: b.ptr if b is not None else None
    if fn is None:
        f = S.sort_pairs_u32 if c.d == "u32" else S.sort_pairs_u64
        rc = f(k0.ptr, ptr(v0), k1.ptr, ptr(v1), n, c.lo, c.hi, scratch.ptr, handle, ctypes.byref(alt),
               mode in ("iota", "iota_null"))
    else:
        rc = fn(k0.ptr, ptr(v0), k1.ptr, ptr(v1), n, scratch.ptr, handle, ctypes.byref(alt))
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    assert rc == 0, f"hipError_t {rc}"
    assert alt.value in (0, 1)
    if c.hi == c.lo or n <= 1:
        assert alt.value == 0, "nothing to sort: the result stays in (k0, v0)"
    host = {name: b.read(DTYPE[c.d] if name[0] == "k" else np.uint32) for name, b in bufs.items()}
    gk = host["k1" if alt.value else "k0"][0]
    gv = host["v1" if alt.value else "v0"][0] if v0 is not None else None
    ek, ev = c.expected(mode)
    msg = R.first_mismatch(ek, ev, gk, gv, TILE[c.d])
    assert msg is None, f"{c.d} n={n} bits [{c.lo}, {c.hi}) {mode}, result_in_alt={alt.value}: {msg}"
    touched = [name for name, (_, ok) in host.items() if not ok]
    assert touched == [], f"guard bands written: {touched}"
    return gk, gv


def matrix():
    """(gen, dtype, n, lo, hi, mode), in an order that keeps a Case's uses together."""
    cases = []
    for d, lo, hi in [("u32", 0, 26), ("u64", 0, 40), ("u64", 0, 64)]:  # every size, the three modes
        for n in sizes(d):
            cases += [("uniform", d, n, lo, hi, m) for m in MODES]
    for d in ("u32", "u64"):  # every bit range, every generator
        for lo, hi in RANGES[d]:
            for n in two_sizes(d):
                cases += [(g, d, n, lo, hi, "explicit") for g in R.GENERATORS]
    for d, lo, hi in [("u32", 0, 26), ("u64", 0, 64)]:  # many tiles in flight
        cases += [(g, d, BIG, lo, hi, "explicit") for g in ("uniform", "skew", "one_bin_per_tile")]
    return list(dict.fromkeys(cases))


def case_id(p):
    gen, d, n, lo, hi, mode = p
    return f"{d}-{lo}_{hi}-n{n}-{gen}-{mode}"


@pytest.mark.parametrize("p", matrix(), ids=case_id)
def test_sort_matches_reference(p):
    gen, d, n, lo, hi, mode = p
    run_sort(case(gen, d, n, lo, hi), mode)


@pytest.mark.parametrize("d", ["u32", "u64"])
def test_iota_with_null_values_is_keys_only(d):
    lo, hi = (0, 26) if d == "u32" else (0, 40)
    for n in (1, TILE[d] + 1, two_sizes(d)[1]):
        run_sort(case("uniform", d, n, lo, hi), "iota_null")


@pytest.mark.parametrize("d", ["u32", "u64"])
def test_scratch_reuse_across_sizes_and_pass_counts(d):
    """What production does every batch: another n and another number of passes in the same
    scratch, nothing cleared in between.  The one memset per sort and "each pass zeroes the next
    pass's look-back words" have to cope with what the sort before left behind."""
    t = TILE[d]
    seq = [(9 * t + t // 8 + 3, 0, 26), (t + 1, 0, 9), (5 * t, 0, 10), (9 * t + t // 8 + 3, 0, 26)]
    assert [len(R.digit_plan(lo, hi)) for _, lo, hi in seq] == [3, 1, 2, 3]
    scratch = Guarded(entry_points().sort_scratch_bytes(max(n for n, _, _ in seq)), fill=INCLUSIVE_ZERO)
    for n, lo, hi in seq:
        run_sort(case("uniform", d, n, lo, hi), "explicit", scratch=scratch)


@pytest.mark.parametrize("d", ["u32", "u64"])
def test_dirty_scratch_from_a_cold_start(d):
    """Every word of the scratch is 0x80000000 before the sort (run_sort's default, asserted here):
    three passes, so both look-back regions are used and the second one twice."""
    n = two_sizes(d)[1]
    scratch = Guarded(entry_points().sort_scratch_bytes(n), fill=INCLUSIVE_ZERO)
    words, _ = scratch.read(np.uint32)
    assert words.size * 4 == entry_points().sort_scratch_bytes(n) and (words == 0x80000000).all()
    run_sort(case("skew", d, n, 0, 26), "iota", scratch=scratch)


def test_sort_on_a_non_default_stream():
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.default_stream().cuda_stream
    run_sort(case("uniform", "u32", two_sizes("u32")[1], 0, 26), "iota", stream=s)


@pytest.mark.parametrize("bits", [1, 40, 64])
def test_radix_sort_pairs_is_sort_pairs_u64_from_bit_zero(bits):
    S = entry_points()
    for n in two_sizes("u64"):
        c = case("uniform", "u64", n, 0, bits)
        fn = lambda k0, v0, k1, v1, n, scratch, stream, alt: S.radix_sort_pairs(k0, v0, k1, v1, n, bits, scratch,
                                                                                stream, alt)
        rk, rv = run_sort(c, "explicit", fn=fn)
        sk, sv = run_sort(c, "explicit")
        assert np.array_equal(rk, sk) and np.array_equal(rv, sv)


def test_scratch_bytes():
    """radix_sort_scratch_bytes is sort_scratch_bytes; it never shrinks as n grows.  (That it covers
    what the sort addresses is the guard bands' check, at every size above.)"""
    S = entry_points()
    ns = sorted(set(sizes("u32")) | set(sizes("u64")) | set(range(0, 60_000, 61)) | {1 << 20, 1 << 27, (1 << 30) - 1})
    b = [S.sort_scratch_bytes(n) for n in ns]
    assert [S.radix_sort_scratch_bytes(n) for n in ns] == b
    assert all(x > 0 and x % 4 == 0 for x in b)
    assert all(x <= y for x, y in zip(b, b[1:]))


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4096 * 256 + 1])
def test_launch_iota(n):
    """4096 * 256 + 1 is one record more than the capped grid of 4096 blocks covers in one step."""
    v = Guarded(4 * n)
    rc = entry_points().launch_iota(v.ptr, n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    got, ok = v.read(np.uint32)
    assert np.array_equal(got, np.arange(n, dtype=np.uint32))
    assert ok, "guard bands written"
