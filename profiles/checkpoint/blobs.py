"""Writes the gw_snapshot blobs of a fixed small set into argv[1], with the library GW_LIB_PATH names."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from flink_amd import _native as N  # noqa: E402
from gpu_helpers import gpu_operator, random_stream  # noqa: E402
from test_snapshot_fuzz import CFGS  # noqa: E402

out = sys.argv[1]
os.makedirs(out, exist_ok=True)


def save(name, blob):
    with open(os.path.join(out, name + ".bin"), "wb") as f:
        f.write(blob)
    print(name, len(blob), flush=True)


def feed(op, kw, hashed=False, payload=False):
    keys, ts, vals, batches = random_stream(11, 4000, 200, 6, disorder=600, wm_lag=200, agg=kw["agg"])
    kh = (keys * 2654435761 % (1 << 31)).astype(np.int32)
    pl = (keys * 1000003 + ts).astype(np.int64)
    for lo, hi, wm in batches[:4]:
        if payload:
            op.process_batch_payload(keys[lo:hi], ts[lo:hi], vals[lo:hi], pl[lo:hi])
        else:
            op.process_batch(keys[lo:hi], ts[lo:hi], vals[lo:hi], key_hashes=kh[lo:hi] if hashed else None)
        op.advance_watermark(wm)
        (op.drain_payload if payload else op.drain)()


for kw in CFGS:
    for hashed in (False, True):
        op = gpu_operator(kw)
        feed(op, kw, hashed)
        blob = op.snapshot_state()
        save(f"{kw['assigner']}-{kw['agg']}" + ("-hashed" if hashed else ""), blob)
        op.close()
        if not hashed:  # restored from the blob and snapshotted again before any record
            op = gpu_operator(kw)
            op.initialize_state(blob)
            save(f"{kw['assigner']}-{kw['agg']}-restored", op.snapshot_state())
            op.close()

kw = dict(assigner="sliding", size=1000, slide=10, agg="sum_i64")  # 2 window classes
op = gpu_operator(kw)
feed(op, kw)
blob = op.snapshot_state()
save("window-classes", blob)
op.close()
op = gpu_operator(kw)
op.initialize_state(blob)
save("window-classes-restored", op.snapshot_state())
op.close()

for name, kw, flags in [("first-element", dict(assigner="sliding", size=900, slide=300, agg="sum_i64"), N.FLAG_FIRST_ELEMENT),
                        ("min-by", dict(assigner="tumbling", size=1000, agg="min_i64"), N.FLAG_FIRST_ELEMENT | N.FLAG_BY_FIELD)]:
    op = gpu_operator(kw, flags=flags)
    feed(op, kw, payload=True)
    blob = op.snapshot_state()
    save(name, blob)
    op.close()
    op = gpu_operator(kw, flags=flags)
    op.initialize_state(blob)
    save(name + "-restored", op.snapshot_state())
    op.close()
print("done", flush=True)
