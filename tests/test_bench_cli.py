"""bench.py's command line and the --dump-outputs file writer (CPU only; the GPU side:
tests/test_gpu_bench_outputs.py)."""
import os

import numpy as np


def test_full_and_dump_outputs_default_off():
    import bench

    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    assert a.stretch_steps is None
    a = bench.parse(["--full", "--dump-outputs", "d", "--stretch-steps", "30"])
    assert a.full is True and a.dump_outputs == "d" and a.stretch_steps == 30


def test_watermarks_of_a_stretch_are_the_streams_own():
    import bench

    whole = bench.watermarks(10_000_000, 0, 2000, 100_000_000, 2000, 100, t_shift=800)
    assert bench.watermarks(10_000_000, 1230, 100, 100_000_000, 2000, 100, t_shift=800) == whole[1230:1330]
    assert all(b - a == 200 for a, b in zip(whole, whole[1:]))  # one watermark interval per batch


def test_dump_rows_ignores_row_order_and_keeps_within_the_size_limit(tmp_path):
    import bench

    n = bench.DUMP_MAX_ROWS + 100_000  # more rows than are written whole: a sample by key
    k = np.arange(n, dtype=np.int64) * 7
    s = 1_700_000_000_000 + (k % 5) * 2000
    rows = (k, s, s + 10_000, k * 3 + 1)
    p = np.random.default_rng(3).permutation(n)
    for d, r in (("a", rows), ("b", tuple(c[p] for c in rows))):
        os.makedirs(tmp_path / d)
        bench.dump_rows(str(tmp_path / d), "x", "", r)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == [f"x_{c}.npy" for c in ("count", "end", "key", "result", "start")]
    for f in names:
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read()
    key, res = np.load(tmp_path / "a" / "x_key.npy"), np.load(tmp_path / "a" / "x_result.npy")
    fired, kept = np.load(tmp_path / "a" / "x_count.npy")
    assert key.dtype == np.float64 and fired == n and kept == len(key)
    assert 0.5 * n / bench.DUMP_KEY_MOD < kept < 2 * n / bench.DUMP_KEY_MOD  # one key in DUMP_KEY_MOD
    assert np.all(np.diff(key) > 0) and np.array_equal(res, key * 3 + 1)
    # two row sets of four float64 columns at the cap stay below 64 MB
    assert 2 * 4 * 8 * bench.DUMP_MAX_ROWS + 1024 <= 64 * 1000 * 1000

    os.makedirs(tmp_path / "s")
    bench.dump_rows(str(tmp_path / "s"), "x", "", tuple(c[p][:1000] for c in rows))  # few rows: all of them
    assert np.array_equal(np.load(tmp_path / "s" / "x_count.npy"), [1000, 1000])
    assert np.array_equal(np.load(tmp_path / "s" / "x_key.npy"), np.sort(k[p][:1000]))

    os.makedirs(tmp_path / "e")
    for r in (None, tuple(c[:0] for c in rows)):  # nothing fired: the count alone, no empty column
        bench.dump_rows(str(tmp_path / "e"), "x", ".rank1", r)
        assert os.listdir(tmp_path / "e") == ["x_count.rank1.npy"]
        assert np.array_equal(np.load(tmp_path / "e" / "x_count.rank1.npy"), [0, 0])
