#!/usr/bin/env python
"""Time the streaming policy triggers (btsbot_trigger_update, btsbot_amd.TriggerState) on one GPU:

    python tools/trigger_bench.py [N]          # N alerts of history, default 1,000,000

The history is policy_bench.py's stream: long-tailed object sizes (Pareto: most objects a handful of alerts, a few in the
thousands, capped at 4,000), shuffled.  Timed with HIP events after >= 0.5 s of the same work, seven blocks, the MEDIAN
block reported (as bench.py does).  Prints one JSON line:
  nightly_kernel_ms   the one launch of btsbot_trigger_update on grouped input for a NIGHTLY batch: 8192 alerts, 1-3 per
                      object (nine objects in ten known to the state), onto a state that holds the N alerts of history
  nightly_update_ms   TriggerState.update for that batch end to end: two stable sorts, the offsets, the launch
  replay_kernel_ms    the launch for a REPLAY batch: the N alerts of history in one call onto an empty state
  replay_update_ms    TriggerState.update for it end to end (the reset before it is not timed)
  policy_eval_ms      val.policy_eval over the N + 8192 accumulated alerts: the way to the same answer after that nightly
                      batch without a state (host clock around a call that ends in its one host read)
  nightly_over_policy_eval = nightly_update_ms / policy_eval_ms
The nightly batch is applied again and again to the same state: from the second call on its objects are all held, its
alerts are late and its policies have fired, so a timed call finds every slot, scans every alert and writes every output,
but stores no new trigger.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from btsbot_amd import TriggerState, _lib, alert_utils, val   # noqa: E402

BLOCKS, WARM_SECONDS, NIGHTLY, NIGHTLY_STEPS = 7, 0.5, 8192, 2000
T_END = 2459000.5 + 700.0


def history(n, seed=0):
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
    ids = rng.permutation(len(sizes)).astype(np.int64) * 977 - 12345
    label = np.repeat(rng.integers(0, 2, len(sizes)), sizes)
    order = rng.permutation(n)
    cols = dict(object_id=np.repeat(ids, sizes)[order], jd=(2459000.5 + rng.uniform(0, 700, n))[order],
                magpsf=np.round(rng.uniform(16, 21, n), 2),
                raw_preds=np.clip(rng.normal(0.25 + 0.5 * label, 0.2), 0, 1).astype(np.float32)[order])
    return cols, sizes, ids


def nightly(ids, seed=1):
    """8192 alerts after the history's last night, 1-3 per object; every tenth object is new to the state."""
    rng = np.random.default_rng(seed)
    per = rng.integers(1, 4, NIGHTLY)
    per = per[:np.searchsorted(np.cumsum(per), NIGHTLY) + 1]
    per[-1] -= per.sum() - NIGHTLY
    objs = rng.choice(ids, len(per), replace=len(per) > len(ids))
    new = rng.random(len(per)) < 0.1
    objs[new] = ids.max() + 1 + np.arange(new.sum())
    oid = np.repeat(objs, per)
    order = rng.permutation(NIGHTLY)
    return dict(object_id=oid[order], jd=(T_END + rng.uniform(0, 1, NIGHTLY))[order],
                magpsf=np.round(rng.uniform(16, 21, NIGHTLY), 2),
                raw_preds=np.clip(rng.normal(0.5, 0.3, NIGHTLY), 0, 1).astype(np.float32)), int(len(per))


def timed(fn, steps, dev, before=None):
    """median over BLOCKS of the device time of `steps` calls of fn (each after an untimed before()), in ms per call"""
    def once(events=None):
        if before is not None:
            before()
        if events is not None:
            events[0].record()
        fn()
        if events is not None:
            events[1].record()

    t_end = time.perf_counter() + WARM_SECONDS
    while time.perf_counter() < t_end:
        once()
        torch.cuda.synchronize(dev)
    ms = []
    for _ in range(BLOCKS):
        if before is None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / steps)
        else:
            pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            torch.cuda.synchronize(dev)
            for pair in pairs:
                once(pair)
            torch.cuda.synchronize(dev)
            ms.append(sum(a.elapsed_time(b) for a, b in pairs) / steps)
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
        sys.exit("trigger_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    keys = ("object_id", "jd", "magpsf", "raw_preds")
    hist, sizes, ids = history(n)
    night, night_objects = nightly(ids)
    h = [torch.from_numpy(hist[k]).to(dev) for k in keys]
    b = [torch.from_numpy(night[k]).to(dev) for k in keys]
    capacity = 1 << max(10, int(np.ceil(np.log2(4 * (len(sizes) + NIGHTLY)))))   # load factor <= 1/4
    state = TriggerState(val.REFERENCE_POLICIES, capacity, dev)
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    table = C.cast(C.c_void_p(state._policy_rows.data_ptr()), C.POINTER(C.c_double))

    def launcher(cols):
        m = cols[0].shape[0]
        perm, offsets = alert_utils._group_by_object(cols[0], then_by=cols[1])
        fired = torch.empty((m, 4), dtype=torch.uint8, device=dev)
        dropped = torch.empty(m, dtype=torch.uint8, device=dev)
        ptr = [C.c_void_p(x.data_ptr()) for x in (perm, offsets, *cols, fired, dropped)]
        keep = (perm, offsets, fired, dropped)

        def launch():
            _lib.check(L.btsbot_trigger_update(C.byref(state._table), table, ptr[0], ptr[1], m, m, *ptr[2:], st),
                       "btsbot_trigger_update")
            return keep
        return launch

    # (b) replay: the whole history in one call onto an empty state
    replay_launch = launcher(h)
    steps_r = max(1, min(50, 20_000_000 // max(n, 1)))
    rk_ms, rk_all = timed(replay_launch, steps_r, dev, before=state.reset)
    ru_ms, ru_all = timed(lambda: state.update(*h), steps_r, dev, before=state.reset)
    # (a) nightly: onto the state that holds the history (the batch's new objects are claimed by the first call)
    state.reset()
    state.update(*h)
    held = state.counters()
    night_launch = launcher(b)
    nk_ms, nk_all = timed(night_launch, NIGHTLY_STEPS, dev)
    nu_ms, nu_all = timed(lambda: state.update(*b), NIGHTLY_STEPS, dev)
    after = state.counters()
    # (c) the same answer without a state: policy_eval over everything seen so far
    acc = [torch.cat([x, y]) for x, y in zip(h, b)]
    label = torch.zeros(n + NIGHTLY, dtype=torch.int64, device=dev)
    pe_ms, pe_all = host_timed(lambda: val.policy_eval(acc[0], acc[1], acc[2], label, acc[3]), steps_r)
    r4 = lambda xs: [round(x, 4) for x in xs]   # noqa: E731
    print(json.dumps({
        "alerts": n, "objects": int(len(sizes)), "largest_object": int(sizes.max()), "median_object": float(np.median(sizes)),
        "capacity": capacity, "nightly_alerts": NIGHTLY, "nightly_objects": night_objects,
        "nightly_kernel_ms": round(nk_ms, 4), "nightly_update_ms": round(nu_ms, 4),
        "replay_kernel_ms": round(rk_ms, 4), "replay_update_ms": round(ru_ms, 4), "policy_eval_ms": round(pe_ms, 4),
        "nightly_over_policy_eval": round(nu_ms / pe_ms, 5),
        "blocks_nightly_kernel_ms": r4(nk_all), "blocks_nightly_update_ms": r4(nu_all),
        "blocks_replay_kernel_ms": r4(rk_all), "blocks_replay_update_ms": r4(ru_all), "blocks_policy_eval_ms": r4(pe_all),
        "steps_per_block": {"nightly": NIGHTLY_STEPS, "replay": steps_r, "policy_eval": steps_r},
        "counters_after_replay": held, "counters_at_end": after, "device": torch.cuda.get_device_name(dev)}))


if __name__ == "__main__":
    main()
