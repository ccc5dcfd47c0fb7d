#!/usr/bin/env python
"""Time btsbot_alert_features (the custom metadata columns of prep_alerts) on one GPU:

    python tools/alert_features_bench.py [N]          # N alerts, default 1,000,000

Object sizes are long-tailed (Pareto: most objects a handful of alerts, a few in the thousands, capped at 4,000) and the
alerts arrive in shuffled order.  Timed with HIP events after >= 0.5 s of the same work, seven blocks, the MEDIAN block reported (as
bench.py does).  Prints one JSON line:
  kernel_ms   the one launch of btsbot_alert_features on grouped input
  call_ms     alert_utils.alert_features end to end: stable sort of the ids, offsets, the launch
  kernel_gbs  the bytes the kernel has to move (perm, offsets, five input columns read once, eight float32 written per
              alert; the per-object re-reads are served on chip and not counted) over kernel_ms
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from btsbot_amd import _lib, alert_utils   # noqa: E402

BLOCKS, WARM_SECONDS = 7, 0.5


def synthetic(n, seed=0):
    rng = np.random.default_rng(seed)
    sizes = []
    left = n
    while left > 0:
        draw = np.minimum((rng.pareto(1.1, 4096) * 4 + 1).astype(np.int64), 4000)
        for s in draw:
            s = int(min(s, left))
            sizes.append(s)
            left -= s
            if left == 0:
                break
    sizes = np.array(sizes)
    oid = np.repeat(rng.permutation(len(sizes)).astype(np.int64) * 977 - 12345, sizes)
    jd = 2459000.5 + rng.uniform(0, 700, n)
    order = rng.permutation(n)
    ndet = rng.integers(1, 60, n).astype(np.int32)
    cols = dict(object_id=oid[order], jd=jd[order], magpsf=np.round(rng.uniform(16, 21, n), 2),
                jdstarthist=2459000.5 + rng.uniform(-30, 30, n), ncovhist=ndet + rng.integers(0, 900, n).astype(np.int32),
                ndethist=ndet)
    return cols, sizes


def timed(fn, steps, dev):
    """median over BLOCKS of the device time of `steps` calls, in ms per call"""
    t_end = time.perf_counter() + WARM_SECONDS
    while time.perf_counter() < t_end:
        fn()
        torch.cuda.synchronize(dev)
    ms = []
    for _ in range(BLOCKS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    ms.sort()
    return ms[len(ms) // 2], ms


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    if not torch.cuda.is_available():
        sys.exit("alert_features_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    cols, sizes = synthetic(n)
    t = {k: torch.from_numpy(v).to(dev) for k, v in cols.items()}
    args = [t[k] for k in ("object_id", "jd", "magpsf", "jdstarthist", "ncovhist", "ndethist")]
    out = alert_utils.alert_features(*args)

    perm, offsets = alert_utils._group_by_object(t["object_id"])
    out2 = torch.empty_like(out)
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = [C.c_void_p(x.data_ptr()) for x in (perm, offsets, *args[1:], out2)]

    def kernel():
        _lib.check(L.btsbot_alert_features(ptr[0], ptr[1], n, n, *ptr[2:], st), "btsbot_alert_features")

    kernel()
    torch.cuda.synchronize(dev)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    steps = max(1, min(50, 20_000_000 // max(n, 1)))
    k_ms, k_all = timed(kernel, steps, dev)
    c_ms, c_all = timed(lambda: alert_utils.alert_features(*args), steps, dev)
    nbytes = 4 * n + 4 * (n + 1) + (3 * 8 + 2 * 4) * n + 32 * n
    print(json.dumps({
        "alerts": n, "objects": int(len(sizes)), "largest_object": int(sizes.max()),
        "median_object": float(np.median(sizes)), "objects_over_64": int((sizes > 64).sum()),
        "objects_over_tile": int((sizes > alert_utils.FEATURE_TILE).sum()),
        "kernel_ms": round(k_ms, 4), "call_ms": round(c_ms, 4), "kernel_bytes": nbytes,
        "kernel_gbs": round(nbytes / (k_ms * 1e-3) / 1e9, 1),
        "blocks_kernel_ms": [round(x, 4) for x in k_all], "blocks_call_ms": [round(x, 4) for x in c_all],
        "steps_per_block": steps, "device": torch.cuda.get_device_name(dev)}))


if __name__ == "__main__":
    main()
