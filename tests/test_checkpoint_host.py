"""What a checkpoint blob's entries mean for an operator (flink_amd/csrc/gw_checkpoint.h) on the
CPU, on its own: the layer between the byte codec (gw_snapshot.h, test_snapshot_codec.py) and
the handle -- WindowOperator.cleanupTime, trigger and cleanup timers, the MergingWindowSet
mapping, count-window purge, the window-class cut and the first-element split.

tests/native/checkpoint.cpp includes the real header over tests/native/fake_hip and is
compiled here with g++ under AddressSanitizer and UBSan (a stand-alone program; without the
sanitizers when their runtimes are missing, which the output says) and run once over every
case; each input blob sits in a heap block of its exact length.  Nothing is loaded into Python
and nothing needs a GPU.

* the oracle's blobs of test_snapshot_fuzz.CFGS: decode, encode as a restore leaves the state,
  decode again; the encoded blob holds what the oracle's holds (state, sets and timers per key
  group; sessions filed under their windows, heapsnap.normalize_sessions, since the oracle
  keeps a merged session's state under an original window; the count-window layout by
  parse_count below, heapsnap.parse reads the window layout only) and a second encoding gives
  the first one's bytes;
* the 16 reference-written migration snapshots as test_gpu_refsnap.py feeds them: the decoded
  windows are the reference's (window, key id, sum), the key hashes String.hashCode, the timer
  flag on exactly the windows with an event timer at end - 1;
* a hand-made pane case of encode_windows against state and timers written out below;
* the sliding blob cut into 3 window classes and merged; a first-element blob split and joined;
* damaged blobs: the program ends clean, every accepted one round-trips (the program checks
  it), the tools agree with the library's gw_snapshot_keys and gw_snapshot_slice on reject and
  accept.  The loaded library has no reader without a handle that checks more than a blob's
  structure, so the decoders' verdicts are pinned from both sides of that: what the operator's
  own decoder accepts, gw_snapshot_keys accepts, and what gw_snapshot_keys accepts and the
  decoder refuses is refused by a rule of the operator's own (OPERATOR_RULES), never by a
  structural reason.

The program takes 3 s under the sanitizers for its 2,827 cases (2,803 damaged blobs at 400
per source), measured on the CPU before the count was fixed."""
import os
import struct
import subprocess

import pytest

import heapsnap
import refsnap
from flink_amd import _native as N
from flink_amd import windowing as W
from test_snapshot_fuzz import CFGS, mutants, oracle_blob
from test_snapshot_slice import HDR, make_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
N_MUTANTS = 400
IDS = {"key1": 0, "key2": 1}  # test_gpu_refsnap.py's
GEOMETRY = {"tumbling": (1, 1, 0), "sliding": (3, 1, 0), "session": (1, 1, 6), "count_tumbling": (1, 1, 2 + 2)}  # n, m, ew


def compile_checkpoint(tmp):
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    linked = subprocess.run(["g++", *SANITIZE, probe, "-o", os.path.join(tmp, "probe")], capture_output=True)
    flags = SANITIZE if linked.returncode == 0 else []
    print("checkpoint: compiled with " + " ".join(flags) if flags else
          "checkpoint: the sanitizer runtimes are missing, compiled without -fsanitize")
    exe = os.path.join(tmp, "checkpoint")
    # the stand-in hip/hip_runtime.h comes before any ROCm include path; the HIP function
    # attributes of gw_common.h's GW_HD mean nothing to g++
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags,
                    "-D__host__=", "-D__device__=", "-D__forceinline__=inline",
                    "-I", os.path.join(ROOT, "tests", "native", "fake_hip"), "-I", os.path.join(ROOT, "flink_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "checkpoint.cpp"), "-o", exe], check=True)
    return exe


def spec(kw, max_parallelism):
    """ckpt::Spec's fields of the operator of one CFGS entry."""
    size, slide = kw.get("size", 0), kw.get("slide", 0)
    n, m, ew = GEOMETRY[kw["assigner"]]
    return [N.AGGS[kw["agg"]], N.ASSIGNERS[kw["assigner"]], N.TRIGGERS["event_time"], max_parallelism, size,
            size if kw["assigner"] == "tumbling" else slide, slide, 0, kw.get("gap", 0), kw.get("lateness", 0), n, m, ew]


def case(kind, params, blob=b""):
    return struct.pack(f"<qq{len(params)}qq", kind, len(params), *params, len(blob)) + blob


def parse_count(blob):
    """The count-window layout (gw_snapshot.h walk_count_windows) of an avg_f64 blob without
    key hashes: kg -> (contents [(key, sum bits, n)], counts [(key, count)]), sorted."""
    h = HDR.unpack(blob[:96])
    nk = h[11] - h[10] + 1
    offs = struct.unpack(f"<{nk + 1}q", blob[96:96 + 8 * (nk + 1)])
    pay = blob[96 + 8 * (nk + 1):]
    out = {}
    for g in range(nk):
        p = offs[g]
        n, = struct.unpack_from(">i", pay, p)
        contents = [struct.unpack_from(">bqqq", pay, p + 4 + 25 * i) for i in range(n)]
        p += 4 + 25 * n
        m, = struct.unpack_from(">i", pay, p)
        counts = [struct.unpack_from(">bqq", pay, p + 4 + 17 * i) for i in range(m)]
        p += 4 + 17 * m
        assert struct.unpack_from(">i", pay, p) == (0,) and p + 4 == offs[g + 1]
        out[h[10] + g] = (sorted(contents), sorted(counts))
    return out


def two_keys():
    """Two keys in different key groups of 4."""
    a = 1
    b = next(k for k in range(2, 100) if W.assign_to_key_group(k, 4) != W.assign_to_key_group(a, 4))
    return a, b


# what a decoder checks beyond the blob's structure (gw_checkpoint.h); a window outside the
# assigner is refused with its bounds in the text
OPERATOR_RULES = {
    "snapshot of a different window / aggregate / max parallelism",
    "snapshot: a key with two different key hashes",
    "merging window set in a tumbling / sliding snapshot",
    "two state entries of one (key, window) in a snapshot key group",
    "empty session window in a snapshot",
    "overlapping sessions of one key in a snapshot",
    "two sessions share one state window",
    "a session without state whose timer has not fired (a trigger other than EventTimeTrigger / PurgingTrigger)",
    "a state entry outside every merging window set",
    "count-window contents without their CountTrigger count",
    "corrupt count-window snapshot entry",
}
PANE_RUNS = [(-(1 << 40), -(1 << 40), 0), (0, 0, 0), (0, -1, 600)]  # fired_k, state_lo, lateness


@pytest.fixture(scope="module")
def run(oracle_lib, tmp_path_factory):
    """One process over every case -> dict of what went in and what came out."""
    tmp = str(tmp_path_factory.mktemp("checkpoint"))
    oracle = [oracle_blob(oracle_lib, kw, 11) for kw in CFGS]
    specs = [spec(kw, HDR.unpack(b[:96])[9]) for kw, b in zip(CFGS, oracle)]
    cases = [case(0, s + [3 if kw["assigner"] == "sliding" else 0], b) for kw, s, b in zip(CFGS, specs, oracle)]
    ref = {}
    for ver, path in sorted(refsnap.migration_fixtures().items()):
        ref[ver] = refsnap.parse(open(path, "rb").read())
        blob = refsnap.to_gpuwin_blob(ref[ver], IDS, W.java_string_hash, N.AGGS["sum_i32"], N.ASSIGNERS["tumbling"], 3000, 3000)
        cases.append(case(1, spec(dict(assigner="tumbling", size=3000, slide=3000, agg="sum_i32"), 1), blob))
    a, b = two_keys()
    cases += [case(3, [a, b, fired_k, state_lo, lateness]) for fired_k, state_lo, lateness in PANE_RUNS]
    cases.append(case(4, []))
    damaged = []  # (blob, its source's spec, a key group of the source)
    for i, blob in enumerate(oracle):
        damaged += [(m, specs[i], HDR.unpack(blob[:96])[10]) for m in mutants(blob, 7 + i, N_MUTANTS)]
    for version, words in [(1, 4), (2, 6), (3, 8)]:
        blob, _, _ = make_blob(version, words, 8, 23, lambda k: (k * 5) % 4, seed=version)
        s = spec(dict(assigner="sliding", size=1000, slide=200, agg="sum_i64"), 128)
        damaged += [(m, s, 8) for m in [blob] + list(mutants(blob, version, N_MUTANTS))]
    cases += [case(2, s + [kg], m) for m, s, kg in damaged]
    src, dst = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "blobs.bin")
    with open(src, "wb") as f:
        f.write(b"".join(cases))
    r = subprocess.run([compile_checkpoint(tmp), src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])  # a failed check or a sanitizer report
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    data, blobs = open(dst, "rb").read(), []
    while data:
        n, = struct.unpack_from("<q", data)
        blobs.append(data[8:8 + n])
        data = data[8 + n:]
    assert len(blobs) == len(oracle) + 1 + len(PANE_RUNS)
    no = len(oracle)
    return dict(oracle=oracle, oracle_lines=lines[:no], encoded=blobs[:2] + blobs[3:5], merged=blobs[2], ref=ref,
                ref_lines=lines[no:no + len(ref)], keys=(a, b), panes=blobs[5:], pane_lines=lines[no + len(ref):][:3],
                fe_line=lines[no + len(ref) + 3], damaged=damaged, damaged_lines=lines[no + len(ref) + 4:])


@pytest.mark.parametrize("i", range(4), ids=[c["assigner"] for c in CFGS])
def test_oracle_blob_round_trips(run, i):
    kw, want, got = CFGS[i], run["oracle"][i], run["encoded"][i]
    assert run["oracle_lines"][i].startswith("ok ") and int(run["oracle_lines"][i][3:]) > 0
    if kw["assigner"] == "count_tumbling":
        assert parse_count(got) == parse_count(want) and any(c for c, _ in parse_count(want).values())
        return
    g, o = heapsnap.parse(got, kw["agg"]), heapsnap.parse(want, kw["agg"])
    assert sorted(g) == sorted(o)
    assert sum(len(s["state"]) for s in o.values()) > 0 and sum(len(s["timers"]) for s in o.values()) > 0
    for kg in o:
        assert g[kg]["timers"] == o[kg]["timers"], kg
        if kw["assigner"] == "session":
            assert heapsnap.normalize_sessions(g[kg]) == heapsnap.normalize_sessions(o[kg]), kg
        else:
            assert g[kg]["state"] == o[kg]["state"] and g[kg]["sets"] == o[kg]["sets"] == [], kg


def test_window_classes_cut_and_merge(run):
    i = next(i for i, c in enumerate(CFGS) if c["assigner"] == "sliding")
    assert heapsnap.parse(run["merged"], CFGS[i]["agg"]) == heapsnap.parse(run["oracle"][i], CFGS[i]["agg"])


def test_reference_snapshots_decode_to_the_reference_entries(run):
    assert len(run["ref"]) == 16
    for (ver, ref), line in zip(sorted(run["ref"].items()), run["ref_lines"]):
        windows, hashes = (part.split("=")[1] for part in line.split(" "))
        got = sorted(tuple(int(x) for x in w.split(":")) for w in windows.split(",") if w)
        want = sorted((IDS[k], s // 3000, v[1], int((e - 1, k, s, e) in sec["event"]))
                      for sec in ref.values() for s, e, k, v in sec["state"])
        assert got == want and want, ver
        keys = {k for sec in ref.values() for _, _, k, _ in sec["state"]}
        assert hashes == "".join(f"{i}:{W.java_string_hash(k)}," for i, k in sorted((IDS[k], k) for k in keys)), ver


def _expected_panes(a, b, fired_k, state_lo, lateness):
    """Sliding 900 / 300, sum_i64: window k = [300 k, 300 k + 900) covers panes k .. k + 2.
    Key A: pane 0 = 5, pane 1 = 7 + 11; key B: pane 5 = 100, restored window 4 = 1000 with a
    pending timer.  State: the windows >= state_lo; timers: end - 1 for the windows >= fired_k,
    end - 1 + lateness for every window with state when lateness > 0."""
    windows = [(a, -2, 5), (a, -1, 5 + 18), (a, 0, 5 + 18), (a, 1, 18), (b, 3, 100), (b, 4, 100 + 1000), (b, 5, 100)]
    out = {kg: {"state": [], "sets": [], "timers": []} for kg in range(4)}
    for key, k, total in windows:
        if k < state_lo:
            continue
        sec = out[W.assign_to_key_group(key, 4)]
        start, end = 300 * k, 300 * k + 900
        sec["state"].append((start, end, key, total))
        if k >= fired_k:
            sec["timers"].append((end - 1, key, start, end))
        if lateness:
            sec["timers"].append((end - 1 + lateness, key, start, end))
    return {kg: {name: sorted(v) for name, v in sec.items()} for kg, sec in out.items()}


@pytest.mark.parametrize("i", range(3), ids=["nothing-fired", "fired-below-0", "lateness-600"])
def test_pane_cells_fold_into_windows_and_timers(run, i):
    a, b = run["keys"]
    assert run["pane_lines"][i] == "ok"
    got = heapsnap.parse(run["panes"][i], "sum_i64")
    assert got == _expected_panes(a, b, *PANE_RUNS[i])
    counts = [(len(s["state"]), len(s["timers"])) for s in got.values()]
    assert sorted(c for c in counts if c != (0, 0)) == [[(3, 3), (4, 4)], [(2, 2), (3, 3)], [(3, 5), (3, 6)]][i]


def test_first_element_blob_splits_and_joins(run):
    assert run["fe_line"] == "ok"


def test_damaged_blobs_are_rejected_or_read_alike(run):
    accepted = valid = 0
    reasons = set()
    for (blob, _, kg), line in zip(run["damaged"], run["damaged_lines"]):
        dec, sl, keys, why = (part.split("=", 1)[1] for part in line.split(" ", 3))
        try:
            want = N.snapshot_keys(blob).tolist()
        except N.GpuWinError:
            want = None
        assert (None if keys == "invalid" else [int(k) for k in keys.split(",") if k]) == want
        try:
            N.snapshot_slice(blob, kg)
            sliced = True
        except N.GpuWinError:
            sliced = False
        assert (sl == "0") == sliced
        if dec == "1":
            assert want is not None  # what a restore accepts, the key reader accepts
            accepted += 1
        elif want is not None:  # the structure is whole: only a rule of the operator's own may refuse it
            assert why in OPERATOR_RULES or why.endswith("is not a window of this assigner"), why
            reasons.add(why if why in OPERATOR_RULES else "window")
        valid += want is not None
    assert len(reasons) >= 4, reasons  # the operator's kind, its windows, the session rules, the count rule
    assert 0 < valid < len(run["damaged"]) and 0 < accepted < valid  # both outcomes occur
