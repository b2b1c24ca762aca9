"""bench.py --dump-outputs and the plain / --full split, on a small Q5-shaped stream.

bench.main runs in-process over 5,000 keys and 20,000-event watermark batches (2 warmup + 20
timed steps: the watermarks of timed steps 10 and 20 each fire a whole set of windows):

* the plain result line holds the headline fields and none of the --full legs;
* two runs with the same arguments write byte-identical files;
* a --checksum run (every step drains its rows inside the step) writes the same files as the
  plain run (the newest fired rows left pending and drained after the clock);
* so does a run whose stream is generated a stretch of 10 batches at a time (--stretch-steps);
* the files equal the CPU oracle's rows of the same watermarks: last_fired_* = the rows of the
  newest timed watermark that fired any, end_of_input_* = the rows MAX_WATERMARK fires
  afterwards (integer sums: bit-exact);
* with 17 timed steps, whose last 7 watermarks fire nothing, last_fired_* holds the rows of timed
  step 10, pending through the steps after it: no file is empty.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WARMUP, STEPS = 2, 20
ARGS = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--keys", "5000",
        "--events-per-pane", "200000"]
FILES = [f"{s}_{c}.npy" for s in ("last_fired", "end_of_input") for c in ("key", "start", "end", "result", "count")]


def _run(bench, capsys, extra, out_dir):
    capsys.readouterr()
    bench.main(ARGS + extra + ["--dump-outputs", str(out_dir)])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    return json.loads(line)


def _bytes(d, files=FILES):
    return {f: open(os.path.join(str(d), f), "rb").read() for f in files}


def test_dump_outputs_repeat_and_match_the_oracle(oracle_lib, tmp_path, capsys):
    import torch

    import bench

    res = _run(bench, capsys, [], tmp_path / "a")
    assert sorted(os.listdir(tmp_path / "a")) == sorted(FILES)
    assert res["steps"] == STEPS and res["warmup"] == WARMUP and res["ms_per_step"] > 0
    assert res["unit"] == "events/s" and res["higher_is_better"] is True and res["dtype"] == "int64"
    assert res["value"] == pytest.approx(STEPS * 20_000 / (res["ms_per_step"] * STEPS / 1e3))
    assert res["full"] is False and res["cpu_baseline"] is None and res["host_fed"] is None
    assert "frac" not in res["roofline"]
    a = _bytes(tmp_path / "a")
    assert sum(map(len, a.values())) <= 64 << 20
    for f in FILES:
        x = np.load(tmp_path / "a" / f)
        assert x.dtype == np.float64 and x.size > 0

    _run(bench, capsys, [], tmp_path / "b")
    assert _bytes(tmp_path / "b") == a, "two runs with the same arguments wrote different files"
    _run(bench, capsys, ["--checksum"], tmp_path / "c")
    assert _bytes(tmp_path / "c") == a, "rows drained inside the step differ from the rows held to the end"
    # the stream generated 10 batches at a time (batches 0-1, 2-11, 12-21: two stops of the clock
    # inside the run) is the same stream
    res = _run(bench, capsys, ["--stretch-steps", "10"], tmp_path / "d")
    assert res["stretch_steps"] == 10 and res["steps"] == STEPS and res["rows_fired"] > 0
    assert [c["steps"] for c in res["fire_cycles"]] == [10, 10]
    assert _bytes(tmp_path / "d") == a, "a stream generated in stretches gave other rows"
    # 17 timed steps: the newest rows are those of timed step 10 (batch 11)
    res = _run(bench, capsys, ["--steps", "17"], tmp_path / "e")
    assert res["steps"] == 17 and [c["steps"] for c in res["fire_cycles"]] == [10, 7]
    assert sorted(os.listdir(tmp_path / "e")) == sorted(FILES)
    _run(bench, capsys, ["--steps", "17", "--checksum"], tmp_path / "f")
    assert _bytes(tmp_path / "f") == _bytes(tmp_path / "e")

    # the oracle over the same stream and watermarks
    args = bench.parse(ARGS)
    nb = args.events_per_pane * args.wm_interval_ms // args.slide_ms
    total = WARMUP + STEPS
    keys, ts, vals, wms = bench.make_stream(nb, total, args.keys, args.events_per_pane, args.slide_ms,
                                            args.disorder_ms, args.agg, torch.device("cuda", 0),
                                            t_shift=(WARMUP - 1) * args.wm_interval_ms)
    cfg = oracle_lib.make_config(assigner="sliding", size=args.size_ms, slide=args.slide_ms, agg=args.agg,
                                 max_parallelism=128)
    ok, os_, oe, orr, ow, _ = oracle_lib.run_parallel_rows(cfg, 4, np.full(total, nb, np.int64),
                                                           np.array(wms, np.int64), keys.cpu().numpy(),
                                                           ts.cpu().numpy(), vals.cpu().numpy(), 1 << 20)
    assert sorted(set(ow[ow >= WARMUP].tolist())) == [WARMUP + 9, WARMUP + 19, total]  # the timed fires
    for d in ("o", "o17"):
        os.makedirs(tmp_path / d)
    for d, name, i in (("o", "last_fired", total - 1), ("o", "end_of_input", total), ("o17", "last_fired", WARMUP + 9)):
        sel = ow == i
        bench.dump_rows(str(tmp_path / d), name, "", (ok[sel], os_[sel], oe[sel], orr[sel]))
    n_last, kept_last = np.load(tmp_path / "o" / "last_fired_count.npy")
    assert n_last > 0.9 * args.keys and kept_last == n_last  # the watermark fires ~every key's window
    assert a == _bytes(tmp_path / "o"), "dumped rows differ from the oracle's"
    last = [f for f in FILES if f.startswith("last_fired")]
    assert _bytes(tmp_path / "e", last) == _bytes(tmp_path / "o17", last), "17 steps: rows differ from the oracle's"
