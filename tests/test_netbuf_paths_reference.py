"""CPU side of tests/test_gpu_netbuf_paths.py: the prefix-aware Python reference
(tests/test_netbuf_oracle.py py_decode_full) agrees with the oracle's decoder on every stream
the GPU tests decode -- whole, on a handful of prefixes, and on the status code of the streams
that fail -- and the streams' construction gives the chunk runs they were built for
(tests/netbuf_streams.py walk_model)."""
import numpy as np
import pytest

from tests import netbuf_streams as S
from tests.test_netbuf_oracle import py_decode_full


def agree(oracle_lib, data, types, kf, vf, ref, n):
    rc, k, t, v, wp, wv, res = oracle_lib.decode_stream(data[:n], types, kf, vf)
    nr, nw, sk, consumed = ref.prefix(n)
    assert rc == 0
    assert (res.records, res.watermarks, res.skipped, res.consumed) == (nr, nw, sk, consumed)
    assert np.array_equal(k, ref.key[:nr]) and np.array_equal(t, ref.ts[:nr]) and np.array_equal(v, ref.val[:nr])
    assert np.array_equal(wp, ref.wm_pos[:nw]) and np.array_equal(wv, ref.wm_val[:nw])


def streams():
    out = [(name, *S.ghost(name)) for name in S.GHOSTS]
    out += [(name + " sprinkled", *S.ghost(name, True)) for name in ("A2", "B")]
    out.append(("dictionary", "JJ", 0, 1, S.dictionary_stream()))
    out += [(name, *S.prefix_stream(name)) for name in S.PREFIX_STREAMS]
    return out


@pytest.mark.parametrize("case", streams(), ids=lambda c: c[0])
def test_prefix_reference_agrees_with_oracle(oracle_lib, case):
    _, types, kf, vf, data = case
    ref = py_decode_full(data, types, kf, vf)
    total = len(data)
    assert ref.rc == 0 and ref.consumed == total
    some = ref.ends[[len(ref.ends) // 3, len(ref.ends) // 2]].tolist()
    cuts = {total, total - 1, total - 3, total // 2, 4096, 1024, 1023, 72, 5, 3, 0}
    cuts |= {e + d for e in some for d in (-1, 0, 1, 4, 5)}
    for n in sorted(c for c in cuts if 0 <= c <= total):
        agree(oracle_lib, data, types, kf, vf, ref, n)


@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_prefix_reference_agrees_with_oracle_on_every_prefix(oracle_lib, name):
    types, kf, vf, data = S.prefix_stream(name)
    ref = py_decode_full(data, types, kf, vf)
    for n in range(len(data) + 1):
        agree(oracle_lib, data, types, kf, vf, ref, n)


@pytest.mark.parametrize("name", ["A2", "B"])
def test_error_status_agrees_with_oracle(oracle_lib, name):
    types, kf, vf, _ = S.ghost(name)
    for label, data in S.error_streams(name).items():
        ref = py_decode_full(data, types, kf, vf)
        assert ref.rc == oracle_lib.decode_stream(data, types, kf, vf)[0], label
        assert ref.rc == (-2 if label.startswith("long") else -1), label
        # everything before the failing element decodes, and the reference stops there
        agree(oracle_lib, data, types, kf, vf, ref, ref.consumed)


@pytest.mark.parametrize("name", list(S.GHOSTS))
def test_ghost_streams_give_the_runs_they_were_built_for(name):
    types, _, _, data = S.ghost(name)
    m = S.walk_model(data, types)
    for field, want in S.MODEL[name].items():
        assert m[field] == want, field
    if name == "A":  # one run longer than a resolve block: nch (nch - 1) / 2 chunk steps
        assert m["walkback"] == m["nch"] * (m["nch"] - 1) // 2 >= 257 * m["nch"]
    if name in ("A2", "B"):  # the long runs cross resolve-block boundaries
        starts = np.flatnonzero(np.diff(np.concatenate([[0], m["nonconv"].astype(int)])) == 1)
        crossed = {b for s0, r in zip(starts, m["runs"]) for b in range(S.SCAN_BLOCK, m["nch"], S.SCAN_BLOCK)
                   if s0 < b < s0 + r}
        assert crossed == set(range(S.SCAN_BLOCK, m["nch"], S.SCAN_BLOCK))


def test_dictionary_stream_falls_back_and_converges():
    m = S.walk_model(S.dictionary_stream(), "JJ")
    assert m["fallback"] >= m["nch"] // 4 and m["runs"] == []
