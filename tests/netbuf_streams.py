"""Serialized streams built to force the network-buffer decoder's data-dependent paths
(flink_amd/csrc/gw_netbuf.hip), and a small CPU restatement of k_nb_walk's candidate walk that
says which chunks of a stream leave the sync window undecided (fallback) and which never
converge (so k_nb_resolve walks back over them).  The restatement only shows that a stream's
construction reaches the path it was built for; what a decode must return comes from
tests/test_netbuf_oracle.py py_decode_full and the oracle.

Ghost chains.  A record's key field holding (L << 32) | x with L the record's own length word
and x < 2^24 reads, at the key's offset, as "length L, tag 0": a second valid chain that steps
in phase with the true one, one record length at a time, and never merges with it.  Every chunk
starts a candidate on it (the candidates cover the first 64 / 128 bytes), so a chunk made of
such records ends with two live exits."""
import functools
import struct

import numpy as np

from flink_amd import netbuf as NB

CHUNK = 1024         # kNbChunk
SYNC = 80            # GW_NB_SYNC
MAX_ELEMENT = 128    # GW_MAX_ELEMENT
SCAN_BLOCK = 256     # kNbScanBlock: chunks per k_nb_resolve block
WIDTH = {"J": 8, "D": 8, "I": 4, "F": 4, "S": 2, "B": 1, "Z": 1}

UNKNOWN_TAG = struct.pack(">i", 9) + bytes([9]) + b"\0" * 8
TOO_LONG = NB.record(tuple(range(15)), "J" * 15, 1)  # 133 bytes > GW_MAX_ELEMENT


def vbytes(types):
    return sum(WIDTH[t] for t in types)


def lanes(types):
    """NL: candidate entries per chunk (launch_nb_decode's wide switch)."""
    return 128 if 13 + vbytes(types) > 64 else 64


def wrong_length(types):
    """A well-formed record of another layout: its length does not fit its tag under `types`."""
    return NB.record((1, 2), "JJ", 3) if types != "JJ" else NB.record((1, 2, 3), "JJJ", 3)


def ordinary(rng, t, n):
    if t == "J":
        return rng.integers(-(1 << 62), 1 << 62, n).tolist()
    bits = 8 * WIDTH[t] - 1
    return rng.integers(-(1 << bits), 1 << bits, n).tolist()


def ghost_stream(types, kf, n, plain=lambda i: False, seed=1, inserts=None):
    """n records with timestamp whose key field makes a ghost chain, except where plain(i): key i.
    inserts: {i: bytes placed before record i}."""
    rng = np.random.default_rng(seed)
    length_word = 9 + vbytes(types)
    x = rng.integers(0, 1 << 24, n).tolist()
    cols = [ordinary(rng, t, n) for t in types]
    stamp = (1000 + 3 * np.arange(n) + rng.integers(-40, 40, n)).tolist()
    inserts = inserts or {}
    parts = []
    for i in range(n):
        if i in inserts:
            parts.append(inserts[i])
        f = [c[i] for c in cols]
        f[kf] = i if plain(i) else (length_word << 32) | x[i]
        parts.append(NB.record(f, types, stamp[i]))
    return b"".join(parts)


def sprinkles(n, period, seed):
    """Watermarks and the three skipped element kinds before every period-th record or so."""
    rng = np.random.default_rng(seed)
    out = {}
    for i in range(period // 2, n, period):
        j = i + int(rng.integers(0, period // 3))
        kinds = [NB.watermark(3 * j), NB.internal_watermark(3 * j + 1, 2), NB.latency_marker(j, 1, 2, 3),
                 NB.stream_status(bool(j & 1)), NB.record_attributes(bool(j & 2))]
        out[j] = b"".join(kinds[k] for k in rng.permutation(5)[:int(rng.integers(1, 6))])
    return out


def plain_a2(i):
    return 5000 <= i % 10000 < 5040


def plain_b(i):
    return 2000 <= i % 4000 < 2040


# name -> (types, key field, value field, builder)
GHOSTS = {
    "A": ("JJ", 0, 1, lambda ins=None: ghost_stream("JJ", 0, 28250, seed=11, inserts=ins)),
    "A2": ("JJ", 0, 1, lambda ins=None: ghost_stream("JJ", 0, 28250, plain_a2, seed=12, inserts=ins)),
    "B": ("JJJJJJJJ", 3, 7, lambda ins=None: ghost_stream("JJJJJJJJ", 3, 9000, plain_b, seed=13, inserts=ins)),
    "B2": ("JJJJJJI", 1, 6, lambda ins=None: ghost_stream("JJJJJJI", 1, 4000, seed=14, inserts=ins)),
}
GHOST_RECORDS = {"A": 28250, "A2": 28250, "B": 9000, "B2": 4000}
# what the streams were designed to give (walk_model at GW_NB_SYNC 80; the decoder's own
# counters agree on the device): chunks, fallback chunks, runs of non-converged chunks, chunk
# steps walked back
MODEL = {
    "A": dict(nch=801, fallback=800, runs=[801], walkback=320400),
    "A2": dict(nch=801, fallback=796, runs=[141, 281, 282, 91], walkback=93630),
    "B": dict(nch=677, fallback=671, runs=[150, 297, 222], walkback=80109),
    "B2": dict(nch=254, runs=[254]),
}
# record index inside a ghost run (A2: the run of 281 chunks, B: of 297), and one in the next run
ERROR_AT = {"A2": (8000, 8100, 18000), "B": (4000, 4050, 7000)}


def error_streams(name):
    """{label: stream}: one unknown tag, one length that does not fit its tag, one element of 133
    bytes inside a ghost run; and two errors of different kinds, in both orders, in the same run
    and in two runs."""
    types, _, _, build = GHOSTS[name]
    a, b, c = ERROR_AT[name]
    bad = {"tag": UNKNOWN_TAG, "len": wrong_length(types), "long": TOO_LONG}
    out = {k: build({a: v}) for k, v in bad.items()}
    for first, second in (("long", "tag"), ("tag", "long"), ("long", "len")):
        out[f"{first}-then-{second}"] = build({a: bad[first], c: bad[second]})
        out[f"{first}-then-{second}-same-run"] = build({a: bad[first], b: bad[second]})
    return out


DICTIONARY = [(25 << 32) | 25, 25 << 32, (17 << 32) | (1 << 24), (9 << 32) | (2 << 24), (13 << 32) | (6 << 24),
              (29 << 32) | (3 << 24), (5 << 32) | (4 << 24), (2 << 32) | (5 << 24),
              1 << 32, 0, 125 << 32, 124 << 32, 0x7fffffff00000000, -1]


def dictionary_stream(n=20000, seed=21):
    """"JJ" elements whose keys, values and half the timestamps are words that read as element
    heads: (length << 32) | (tag << 24) for every tag, lengths 0, 1, 124, 125, a huge and a
    negative one.  The wrong candidates they start die as corrupt, over-long or negative, or
    merge; the true chain is valid."""
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    w = rng.integers(0, len(DICTIONARY), (n, 3))
    low = rng.integers(0, 1 << 16, n).tolist()
    from_dict = rng.random(n) < 0.5
    parts = []
    for i in range(n):
        if u[i] < 0.03:
            parts.append(NB.watermark(1000 + i))
        elif u[i] < 0.05:
            parts.append(NB.record_attributes(bool(i & 1)))
        else:
            key = DICTIONARY[w[i, 0]] ^ low[i]
            stamp = DICTIONARY[w[i, 2]] if from_dict[i] else 1000 + i
            parts.append(NB.record((key, DICTIONARY[w[i, 1]]), "JJ", None if u[i] < 0.07 else stamp))
    return b"".join(parts)


def walk_model(data, types):
    """k_nb_walk and k_nb_resolve's walk-back restated: -> dict(nch, fallback, walkback, runs,
    nonconv).  fallback counts the windowed chunks whose candidates disagree at the end of the
    sync window, runs lists the lengths of the maximal runs of chunks with more than one live
    exit, walkback sums, over the chunks, the non-converged chunks right before each."""
    n, nl = len(data), lanes(types)
    vb = vbytes(types)
    fits = {0: 9 + vb, 1: 1 + vb, 2: 9, 3: 29, 4: 5, 5: 2, 6: 13}
    ksync = (SYNC if nl == 64 else 2 * SYNC) - 8
    NORMAL, TAIL, DEAD, LONG = 0, 1, 2, 3

    def walk(pos, limit, rlim, memo):
        """from element start pos while pos < limit -> (pos, state)"""
        path = []
        while True:
            if pos in memo:
                res = memo[pos]
                break
            if pos >= limit:
                res = (pos, NORMAL)
                break
            path.append(pos)
            if pos + 4 > rlim:
                res = (pos, TAIL)
                break
            ln = int.from_bytes(data[pos:pos + 4], "big", signed=True)
            if ln < 1:
                res = (pos, DEAD)
            elif ln > MAX_ELEMENT - 4:
                res = (pos, LONG)
            elif pos + 4 + ln > rlim:
                res = (pos, TAIL)
            elif fits.get(data[pos + 4]) != ln:
                res = (pos, DEAD)
            else:
                pos += 4 + ln
                continue
            break
        for p in path:
            memo[p] = res
        return res

    nch = (n + CHUNK - 1) // CHUNK
    nonconv = np.zeros(nch, bool)
    fallback = 0
    for c in range(nch):
        base = c * CHUNK
        left = n - base
        rlim = base + min(left, CHUNK + 4 * nl)
        rend = min(rlim, base + CHUNK)
        windowed = rend - base > ksync
        memo = {}
        cand = [walk(base + i, base + ksync if windowed else rend, rlim, memo) for i in range(nl)]
        if windowed:
            live = [x for x in cand if x[1] in (NORMAL, TAIL)]
            normal = [x for x in cand if x[1] == NORMAL]
            if live and normal and all(x == normal[0] for x in live):
                continue  # synced: k_nb_tail walks the one chain on, its exit is unique
            fallback += 1
            memo = {}
            cand = [walk(p, rend, rlim, memo) if s == NORMAL else (p, s) for p, s in cand]
        live = [x for x in cand if x[1] in (NORMAL, TAIL)]
        nonconv[c] = bool(live) and any(x != live[0] for x in live)
    runs, walkback, run = [], 0, 0
    for c in range(nch):
        walkback += run  # the non-converged chunks right before chunk c
        if nonconv[c]:
            run += 1
        else:
            if run:
                runs.append(run)
            run = 0
    if run:
        runs.append(run)
    return dict(nch=nch, fallback=fallback, walkback=walkback, runs=runs, nonconv=nonconv)


@functools.lru_cache(maxsize=None)
def ghost(name, sprinkled=False):
    """(types, kf, vf, stream) of A, A2, B, B2; sprinkled: with watermarks and skipped elements."""
    types, kf, vf, build = GHOSTS[name]
    n = GHOST_RECORDS[name]
    return types, kf, vf, build(sprinkles(n, n // 40, 31) if sprinkled else None)


def mixed_stream(types, kf, vf, min_bytes, seed):
    """Elements of every kind until the stream is at least min_bytes long."""
    from tests.test_netbuf_oracle import random_elements
    rng = np.random.default_rng(seed)
    data = b""
    while len(data) < min_bytes:
        data += random_elements(rng, 4, types, kf, vf, p_wm=0.15, p_other=0.2, p_nots=0.1)
    return data


# (d): streams of two chunks and a last one that reaches past every threshold of the end handling
PREFIX_STREAMS = {
    "narrow": ("JJ", 0, 1, 2 * CHUNK + 4 * 64 + 64, 41),
    "wide": ("JJJJJJJJ", 3, 7, 2 * CHUNK + 4 * 128 + 128, 42),
}


@functools.lru_cache(maxsize=None)
def prefix_stream(name):
    types, kf, vf, nbytes, seed = PREFIX_STREAMS[name]
    return types, kf, vf, mixed_stream(types, kf, vf, nbytes, seed)


def end_thresholds(types):
    """Bytes left in a chunk at which the decoder's end handling changes: the non-windowed last
    chunk (sync window - 8), fetch_window in range (256), a whole chunk, the chunk's LDS words
    (nb_words), nb_fetch in range (1280), rlim no longer binding (chunk + 4 NL)."""
    nl = lanes(types)
    return sorted({(SYNC if nl == 64 else 2 * SYNC) - 8, 256, CHUNK, CHUNK + nl + 8, 1280, CHUNK + 4 * nl})


def threshold_prefixes(total, types, around=8):
    """Every n within `around` bytes of a threshold of some chunk."""
    ns = set()
    for base in range(0, total + 1, CHUNK):
        for t in [0] + end_thresholds(types):
            ns.update(range(base + t - around, base + t + around + 1))
    return sorted(n for n in ns if 0 <= n <= total)
