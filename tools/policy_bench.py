#!/usr/bin/env python
"""Time the per-object policy metrics (btsbot_policy_eval, val.policy_performance) on one GPU:

    python tools/policy_bench.py [N]          # N alerts, default 1,000,000

Object sizes are long-tailed (Pareto: most objects a handful of alerts, a few in the thousands, capped at 4,000) and the
alerts arrive in shuffled order.  Timed with HIP events after >= 0.5 s of the same work, seven blocks, the MEDIAN block reported (as
bench.py does).  Prints one JSON line:
  kernel_ms     the one launch of btsbot_policy_eval on grouped input, the reference's four policies
  kernel16_ms   the same launch with 16 policies (a threshold sweep's chunk)
  eval_ms       val.policy_eval end to end: stable sort of the ids, offsets, the launch, the object count (one sync)
  call_ms       val.policy_performance end to end with junk / save / trigger columns: the above without the count, the
                object filter, the counts, the medians and the one host read (host clock around a call that ends in
                that read)
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from btsbot_amd import _lib, alert_utils, val   # noqa: E402

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
    label = np.repeat(rng.integers(0, 2, len(sizes)), sizes)
    score = np.clip(rng.normal(0.25 + 0.5 * label, 0.2), 0, 1).astype(np.float32)      # clustered by label, overlapping
    save = np.repeat(np.where(rng.random(len(sizes)) < 0.5, 2459300.5 + rng.uniform(0, 400, len(sizes)), np.nan), sizes)
    cols = dict(object_id=oid[order], jd=jd[order], magpsf=np.round(rng.uniform(16, 21, n), 2), label=label[order],
                raw_preds=score[order], junk=np.repeat(rng.random(len(sizes)) < 0.02, sizes)[order],
                save_time=save[order], trigger_time=(save - 1.5)[order])
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


def host_timed(fn, steps):
    """median over BLOCKS of the host time of `steps` calls that each end in a host read, in ms per call"""
    t_end = time.perf_counter() + WARM_SECONDS
    while time.perf_counter() < t_end:
        fn()
    ms = []
    for _ in range(BLOCKS):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    ms.sort()
    return ms[len(ms) // 2], ms


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    if not torch.cuda.is_available():
        sys.exit("policy_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    cols, sizes = synthetic(n)
    t = {k: torch.from_numpy(v).to(dev) for k, v in cols.items()}
    args = [t[k] for k in ("object_id", "jd", "magpsf", "label", "raw_preds")]
    extra = {k: t[k] for k in ("junk", "save_time", "trigger_time")}
    sweep = {f"t{i}": (0.05 + 0.055 * i, 19.0, 1, 18.5) for i in range(16)}
    perf = val.policy_performance(*args, **extra)

    perm, offsets = alert_utils._group_by_object(t["object_id"])
    lab32 = t["label"].to(torch.int32)
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = [C.c_void_p(x.data_ptr()) for x in (perm, offsets, t["jd"], t["magpsf"], t["raw_preds"], lab32)]
    pred = torch.empty((n, 16), dtype=torch.int32, device=dev)
    trig = torch.empty((n, 16, 2), dtype=torch.float64, device=dev)
    info = torch.empty((n, 3), dtype=torch.float64, device=dev)
    outs = [C.c_void_p(x.data_ptr()) for x in (pred, trig, info)]
    tables = {m: val._policy_table(p) for m, p in ((4, val.REFERENCE_POLICIES), (16, sweep))}

    def kernel(m):
        tab = C.cast(C.c_void_p(tables[m].data_ptr()), C.POINTER(C.c_double))
        _lib.check(L.btsbot_policy_eval(ptr[0], ptr[1], n, n, *ptr[2:], tab, m, *outs, st), "btsbot_policy_eval")

    kernel(4)
    torch.cuda.synchronize(dev)
    steps = max(1, min(50, 20_000_000 // max(n, 1)))
    k_ms, k_all = timed(lambda: kernel(4), steps, dev)
    k16_ms, k16_all = timed(lambda: kernel(16), steps, dev)
    e_ms, e_all = host_timed(lambda: val.policy_eval(*args), steps)
    c_ms, c_all = host_timed(lambda: val.policy_performance(*args, **extra), steps)
    print(json.dumps({
        "alerts": n, "objects": int(len(sizes)), "largest_object": int(sizes.max()),
        "median_object": float(np.median(sizes)), "objects_over_64": int((sizes > 64).sum()),
        "objects_over_tile": int((sizes > val.POLICY_TILE).sum()),
        "kernel_ms": round(k_ms, 4), "kernel16_ms": round(k16_ms, 4), "eval_ms": round(e_ms, 4), "call_ms": round(c_ms, 4),
        "blocks_kernel_ms": [round(x, 4) for x in k_all], "blocks_kernel16_ms": [round(x, 4) for x in k16_all],
        "blocks_eval_ms": [round(x, 4) for x in e_all], "blocks_call_ms": [round(x, 4) for x in c_all],
        "steps_per_block": steps, "device": torch.cuda.get_device_name(dev),
        "policy_performance": {k: [round(v["policy_recall"], 4), round(v["policy_precision"], 4)] for k, v in perf.items()}}))


if __name__ == "__main__":
    main()
