"""The network-buffer decoder's rare paths (flink_amd/csrc/gw_netbuf.hip), driven directly
through gw::launch_nb_decode (tests/netbuf_native.py) with streams built to force each path
(tests/netbuf_streams.py) and the decoder's own counters as proof that the path ran:
NbStatus.fallback counts the chunks whose candidates disagreed after the sync window (the
full-chunk walk of k_nb_walk), NbStatus.walkback the chunk steps k_nb_resolve walked back over
chunks that never converged.

Every decode is compared exactly with tests/test_netbuf_oracle.py py_decode_full (which the CPU
suite holds against the oracle's decoder on these same streams): records, watermarks, consumed,
skipped, the three columns, wm_pos and wm_val.  Every output row past the decoded ones, the
guard rows past the capacity included, must still hold its fill pattern, and so must the bytes
behind the nb_scratch_bytes(n) bytes of scratch.  The scratch starts as 0xFF bytes: device
memory is not zeroed in production either.

* ghost chains (a): runs of hundreds of non-converged chunks, across the 256-chunk resolve
  blocks, narrow (NL = 64) and wide (NL = 128) walks;
* a dictionary of payload words that read as element heads (b): wrong candidates die as
  corrupt, over-long or negative and must not be reported;
* real errors inside ghost runs, and output capacities that are exactly enough and one short (c);
* every prefix length of a three-chunk stream, with the stream's continuation and then 0xFF
  behind the prefix (d);
* every entry lane of 64-, 65- and 77-byte elements (e);
* grids of one block (GW_NB_GRID=1 GW_NB_TAIL_GRID=1, a child process): every wave loops over
  hundreds of chunks, the tail block takes several turns (f)."""
import functools
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from flink_amd import netbuf as NB
from tests import netbuf_streams as S
from tests.netbuf_native import PATTERN, STATUS_FIELDS, NbDecoder
from tests.test_gpu_netbuf import gpu_decode
from tests.test_netbuf_oracle import py_decode_full

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def big():
    return NbDecoder(1 << 20, 30000, 2048)


@functools.lru_cache(maxsize=None)
def small():
    return NbDecoder(8192, 256, 256)


@functools.lru_cache(maxsize=None)
def reference(data, types, kf, vf):
    return py_decode_full(data, types, kf, vf)


def counters(res):
    return {f: int(getattr(res.status, f)) for f in STATUS_FIELDS}


def check(res, ref, n=None):
    """A decode of the first n bytes of ref's stream with status 0, exactly the reference's."""
    nr, nw, sk, consumed = ref.prefix(ref.consumed if n is None else n)
    got = counters(res)
    assert (res.code, got["corrupt"], got["unsupported"], got["full"]) == (0, 0, 0, 0), (n, got)
    assert (got["records"], got["watermarks"], got["consumed"], got["skipped"]) == (nr, nw, consumed, sk), (n, got)
    for name, m in (("key", nr), ("ts", nr), ("val", nr), ("wm_pos", nw), ("wm_val", nw)):
        col = getattr(res, name)
        assert np.array_equal(col[:m], getattr(ref, name)[:m]), (n, name)
        assert (col[m:] == PATTERN).all(), (n, name, "a row past the decoded ones was written")
    assert res.scratch_ok, (n, "a byte behind the scratch was written")


def check_guards(res):
    """No row at or past a capacity, and no byte behind the scratch, was written."""
    for name, cap in (("key", res.rec_cap), ("ts", res.rec_cap), ("val", res.rec_cap), ("wm_pos", res.wm_cap),
                      ("wm_val", res.wm_cap)):
        assert (getattr(res, name)[cap:] == PATTERN).all(), name
    assert res.scratch_ok


def decode_whole(data, types, kf, vf, dec=None):
    dec = dec or big()
    dec.upload(data)
    res = dec.decode(len(data), types, kf, vf)
    check(res, reference(data, types, kf, vf))
    return counters(res)


# ---- (a) ghost chains: resolution over many chunks ---------------------------------------------

@pytest.mark.parametrize("name", ["A", "A2", "B", "B2"])
def test_ghost_chains_resolve_over_long_runs(name):
    types, kf, vf, data = S.ghost(name)
    model = S.walk_model(data, types)
    nch = model["nch"]
    # the stream's construction reaches the path (the CPU suite holds the model to the same numbers)
    assert model["runs"] == S.MODEL[name]["runs"] and nch == S.MODEL[name]["nch"]
    got = decode_whole(data, types, kf, vf)
    print(name, "fallback", got["fallback"], "walkback", got["walkback"], "chunks", nch)
    if name == "A":
        assert got["walkback"] >= 257 * nch  # some run is longer than a resolve block
    elif name in ("A2", "B"):
        assert got["fallback"] >= nch / 2 and got["walkback"] >= 256
    assert (got["fallback"], got["walkback"]) == (model["fallback"], model["walkback"])


@pytest.mark.parametrize("name", ["A2", "B"])
def test_ghost_chains_with_watermarks_and_skipped_elements(name):
    """Counts and watermark positions come from the true lane only: the ghost chain steps over
    the same chunks and counts other elements."""
    types, kf, vf, data = S.ghost(name, True)
    ref = reference(data, types, kf, vf)
    assert ref.rc == 0 and ref.watermarks >= 20 and ref.skipped >= 30
    model = S.walk_model(data, types)
    assert max(model["runs"]) >= 8 and len(model["runs"]) >= 20  # still ghost runs, now many of them
    got = decode_whole(data, types, kf, vf)
    assert (got["fallback"], got["walkback"]) == (model["fallback"], model["walkback"])


# ---- (b) ghosts that end badly must not be reported ---------------------------------------------

def test_dictionary_of_element_heads_reports_no_error():
    data = S.dictionary_stream()
    ref = reference(data, "JJ", 0, 1)
    assert ref.rc == 0 and ref.consumed == len(data)
    model = S.walk_model(data, "JJ")
    got = decode_whole(data, "JJ", 0, 1)
    print("dictionary fallback", got["fallback"], "walkback", got["walkback"], "chunks", model["nch"])
    assert got["fallback"] >= 1
    assert (got["fallback"], got["walkback"]) == (model["fallback"], model["walkback"])


# ---- (c) real errors inside the rare paths, output capacities -----------------------------------

@pytest.mark.parametrize("name", ["A2", "B"])
def test_errors_inside_ghost_runs_give_the_reference_status(name):
    types, kf, vf, _ = S.ghost(name)
    dec = big()
    want = {"tag": -1, "len": -1, "long": -2, "long-then-tag": -2, "tag-then-long": -1, "long-then-len": -2,
            "long-then-tag-same-run": -2, "tag-then-long-same-run": -1, "long-then-len-same-run": -2}
    seen = {}
    for label, data in S.error_streams(name).items():
        ref = reference(data, types, kf, vf)
        assert ref.rc == want[label], label  # the reference's first error, in its order of checks
        at = ref.consumed // S.CHUNK  # the chunk of the failing element: inside a non-converged run
        nonconv = S.walk_model(data, types)["nonconv"]
        assert nonconv[at - 3:at].all(), label
        dec.upload(data)
        res = dec.decode(len(data), types, kf, vf)
        check_guards(res)
        seen[label] = res.code
        if "then" in label:  # and through the C ABI's own mapping of the status (nb_status_code)
            assert gpu_decode(data, types, kf, vf)[0] == want[label], label
    assert seen == want


@pytest.mark.parametrize("name", ["A2", "B"])
def test_output_capacity_exact_and_one_short(name):
    types, kf, vf, data = S.ghost(name, True)
    ref = reference(data, types, kf, vf)
    dec = big()
    dec.upload(data)
    n = len(data)
    check(dec.decode(n, types, kf, vf, rec_cap=ref.records, wm_cap=ref.watermarks), ref)
    for caps in (dict(rec_cap=ref.records - 1), dict(wm_cap=ref.watermarks - 1)):
        res = dec.decode(n, types, kf, vf, **caps)
        assert res.code == -5 and res.status.full, caps  # GW_E_OUTPUT_FULL
        check_guards(res)


# ---- (d) every prefix length ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["narrow", "wide"])
@pytest.mark.parametrize("behind", ["continuation", "ones"])
def test_every_prefix_length(name, behind):
    """The stream is uploaded once and a prefix is decoded by passing n, so the bytes behind n
    are the stream's own continuation (or, n descending, 0xFF): a kernel that looks past nbytes
    decodes something else than the reference."""
    types, kf, vf, data = S.prefix_stream(name)
    ref = reference(data, types, kf, vf)
    total = len(data)
    assert ref.rc == 0 and ref.consumed == total and total >= S.PREFIX_STREAMS[name][3]
    assert {0, 1, 2} <= set(np.diff(ref.cum, axis=1).argmax(axis=0).tolist())  # every class of element
    dec = small()
    dec.upload(data)
    for n in range(total, -1, -1):
        if behind == "ones":
            dec.poison_from(n)
        check(dec.decode(n, types, kf, vf), ref, n)


# ---- (e) every entry lane --------------------------------------------------------------------------

def entry_offsets(ref):
    """Offset into its chunk of the first element that starts in each chunk after the first."""
    first = {}
    for s in ref.starts.tolist():
        first.setdefault(s // S.CHUNK, s % S.CHUNK)
    return {o for c, o in first.items() if c > 0}


@pytest.mark.parametrize("vf", [6, 7])
def test_every_entry_lane_of_64_byte_elements(vf):
    """Elements of 64 bytes keep their phase against the 1-KB chunks: s leading 17-byte watermarks
    put the chunks' first elements on lane 17 s mod 64, up to lane 63 of the narrow walk."""
    types, kf = "JJJJJJSB", 0
    rng = np.random.default_rng(51)
    assert len(NB.record([0] * 8, types, 1)) == 64 and S.lanes(types) == 64
    dec = small()
    seen = set()
    for s in range(64):
        cols = [S.ordinary(rng, t, 40) for t in types]
        data = b"".join(NB.internal_watermark(100 + j, j) for j in range(s)) + \
            b"".join(NB.record([c[i] for c in cols], types, 1000 + i) for i in range(40))
        ref = reference(data, types, kf, vf)
        assert ref.rc == 0 and ref.records == 40
        seen |= entry_offsets(ref)
        dec.upload(data)
        check(dec.decode(len(data), types, kf, vf), ref)
    assert seen >= set(range(64))


@pytest.mark.parametrize("types,kf,vf,size", [("JJJJJJI", 1, 6, 65), ("JJJJJJJJ", 3, 7, 77)])
def test_every_entry_lane_of_wide_elements(types, kf, vf, size):
    """65 bytes is the smallest element that needs the wide walk (entry lane 64); elements of 65
    and 77 bytes drift through every entry lane by themselves."""
    rng = np.random.default_rng(size)
    assert len(NB.record([0] * len(types), types, 1)) == size and S.lanes(types) == 128
    cols = [S.ordinary(rng, t, 1100) for t in types]
    data = b"".join(NB.record([c[i] for c in cols], types, 1000 + i) for i in range(1100))
    ref = reference(data, types, kf, vf)
    assert entry_offsets(ref) >= set(range(size))
    got = decode_whole(data, types, kf, vf)
    assert got["records"] == 1100


# ---- (f) grids of one block ---------------------------------------------------------------------

def grid_cases():
    """(label, types, kf, vf, stream, prefix lengths)"""
    cases = []
    for name in ("A2", "B"):
        types, kf, vf, data = S.ghost(name)
        cases.append((name, types, kf, vf, data, [len(data)]))
    data = S.dictionary_stream()
    cases.append(("dictionary", "JJ", 0, 1, data, [len(data)]))
    for name in S.PREFIX_STREAMS:
        types, kf, vf, data = S.prefix_stream(name)
        cases.append((name, types, kf, vf, data, S.threshold_prefixes(len(data), types)))
    return cases


def grid_digest():
    """Decodes every grid case, holds each to the reference and folds all outputs, the whole
    status (counters included) and every row's fill pattern into one digest."""
    crc, launches = 0, 0
    for label, types, kf, vf, data, prefixes in grid_cases():
        ref = reference(data, types, kf, vf)
        dec = big() if len(data) > 8192 else small()
        dec.upload(data)
        for n in prefixes:
            res = dec.decode(n, types, kf, vf)
            check(res, ref, n)
            crc = zlib.crc32(res.raw.tobytes(), crc)
            launches += 1
    return {"crc": crc, "launches": launches}


def test_grids_of_one_block_decode_the_same():
    mine = grid_digest()
    assert mine["launches"] > 300
    env = dict(os.environ, GW_NB_GRID="1", GW_NB_TAIL_GRID="1")
    code = ("import json, sys; sys.path.insert(0, %r); sys.path.insert(0, %r); "
            "import test_gpu_netbuf_paths as t; print('RESULT', json.dumps(t.grid_digest()))"
            % (ROOT, os.path.join(ROOT, "tests")))
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=None,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:]
    other = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert other == mine
