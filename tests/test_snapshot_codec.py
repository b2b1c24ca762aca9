"""The checkpoint blob codec (flink_amd/csrc/gw_snapshot.h) on the CPU, on its own.

Every reader and writer of the runtime goes through this header-only codec: the bounds-checked
Cursor, open(), the two version-4 key-group walkers and the Writer.  tests/native/
snapshot_codec.cpp is compiled here with g++ under AddressSanitizer and UBSan (a stand-alone
program; without the sanitizers when their runtimes are missing, which the output says) and
run once over every input: the oracle's blobs of test_snapshot_fuzz.CFGS, their damaged
forms and those of the v1-v3 entry blobs.  Each blob sits in a heap block of its exact
length, so a read past a damaged blob's end stops the program.

The oracle's blobs: the walkers see what tests/heapsnap.py decodes and what gw_snapshot_keys
names, and the Writer rebuilds them byte for byte.  Damaged blobs: the codec rejects exactly
what gw_snapshot_keys rejects and names the same keys otherwise."""
import os
import struct
import subprocess

import numpy as np
import pytest

import heapsnap
from flink_amd import _native as N
from test_snapshot_fuzz import CFGS, mutants, oracle_blob
from test_snapshot_slice import make_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
N_MUTANTS = 400


def compile_codec(tmp):
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    linked = subprocess.run(["g++", *SANITIZE, probe, "-o", os.path.join(tmp, "probe")], capture_output=True)
    flags = SANITIZE if linked.returncode == 0 else []
    if not flags:
        print("snapshot_codec: the sanitizer runtimes are missing, compiled without -fsanitize")
    exe = os.path.join(tmp, "snapshot_codec")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "flink_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "snapshot_codec.cpp"), "-o", exe], check=True)
    return exe


def read_line(ln):
    """-> None (invalid) or dict(version, rt, counts = [(a, b, c), ...] or None, keys)."""
    if ln == "invalid":
        return None
    v, rt, counts, keys = ln.split(" ")
    counts = counts[len("counts="):]
    keys = keys[len("keys="):]
    return dict(version=int(v[1:]), rt=rt == "rt=1",
                counts=None if counts == "-" else [tuple(int(x) for x in g.split(":")) for g in counts.split(",")],
                keys=[int(k) for k in keys.split(",")] if keys else [])


@pytest.fixture(scope="module")
def run(oracle_lib, tmp_path_factory):
    """One process over every input: ([oracle blob per CFGS], its results, [damaged blobs], their results)."""
    tmp = str(tmp_path_factory.mktemp("codec"))
    oracle = [oracle_blob(oracle_lib, kw, 11) for kw in CFGS]
    damaged = [m for i, b in enumerate(oracle) for m in mutants(b, 7 + i, N_MUTANTS)]
    for version, words in [(1, 4), (2, 6), (3, 8)]:
        blob, _, _ = make_blob(version, words, 8, 23, lambda k: (k * 5) % 4, seed=version)
        damaged += [blob] + list(mutants(blob, version, N_MUTANTS))
    path = os.path.join(tmp, "blobs.bin")
    with open(path, "wb") as f:
        for b in oracle + damaged:
            f.write(struct.pack("<q", len(b)) + b)
    r = subprocess.run([compile_codec(tmp), path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]  # a sanitizer report ends the program
    lines = [read_line(ln) for ln in r.stdout.splitlines()]
    assert len(lines) == len(oracle) + len(damaged)
    return oracle, lines[:len(oracle)], damaged, lines[len(oracle):]


@pytest.mark.parametrize("i", range(3), ids=[c["assigner"] for c in CFGS[:3]])
def test_window_walker_counts_match_the_decoder(run, i):
    oracle, got, _, _ = run
    want = heapsnap.parse(oracle[i], CFGS[i]["agg"])
    assert got[i]["version"] == 4
    assert got[i]["counts"] == [(len(s["state"]), len(s["sets"]), len(s["timers"])) for _, s in sorted(want.items())]
    assert sum(c[0] for c in got[i]["counts"]) > 0 and sum(c[2] for c in got[i]["counts"]) > 0
    assert (sum(c[1] for c in got[i]["counts"]) > 0) == (CFGS[i]["assigner"] == "session")


@pytest.mark.parametrize("i", range(4), ids=[c["assigner"] for c in CFGS])
def test_keys_and_writer_round_trip(run, i):
    oracle, got, _, _ = run
    assert got[i]["keys"] == N.snapshot_keys(oracle[i]).tolist() and got[i]["keys"]
    assert got[i]["rt"], "the Writer rebuilt other bytes"
    if CFGS[i]["assigner"] == "count_tumbling":  # contents and their CountTrigger counts, no timers
        assert all(a == b and c == 0 for a, b, c in got[i]["counts"]) and sum(a for a, _, _ in got[i]["counts"]) > 0


def test_damaged_blobs_are_rejected_or_read_alike(run):
    _, _, damaged, got = run
    valid = 0
    for blob, g in zip(damaged, got):
        try:
            want = N.snapshot_keys(blob).tolist()
        except N.GpuWinError:
            want = None
        if want is None:
            assert g is None
        else:
            assert g is not None and g["keys"] == want
            valid += 1
    assert 0 < valid < len(damaged)  # both outcomes occur
