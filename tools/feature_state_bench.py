#!/usr/bin/env python
"""Time the streaming light-curve features (btsbot_feature_update, btsbot_amd.FeatureState) on one GPU:

    python tools/feature_state_bench.py [N]          # N alerts of history, default 1,000,000

The history and the nightly batch are trigger_bench.py's: long-tailed object sizes (Pareto, capped at 4,000), shuffled; a
nightly batch of 8192 alerts, 1-3 per object, nine objects in ten known to the state.  Timed with HIP events after
>= 0.5 s of the same work, seven blocks, the MEDIAN block reported (as bench.py does).  Prints one JSON line:
  nightly_kernel_ms   the one launch of btsbot_feature_update on grouped input for the nightly batch, onto a state that
                      holds the N alerts of history
  nightly_update_ms   FeatureState.update for that batch end to end: two stable sorts, the offsets, the launch
  replay_kernel_ms    the launch for a REPLAY batch: the N alerts of history in one call onto an empty state
  replay_update_ms    FeatureState.update for it end to end (the reset before it is not timed)
  alert_features_ms   alert_utils.alert_features over the N + 8192 accumulated alerts: the way to the same rows after
                      that nightly batch without a state (one stable sort, the offsets, the launch; device time)
  nightly_over_alert_features = nightly_update_ms / alert_features_ms
The nightly batch is applied again and again to the same state: from the second call on its objects are all held and its
alerts are late, so a timed call finds every slot, scans every alert and writes every row.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from btsbot_amd import FeatureState, _lib, alert_utils   # noqa: E402
from trigger_bench import NIGHTLY, NIGHTLY_STEPS, history, nightly, timed   # noqa: E402

KEYS = ("object_id", "jd", "magpsf", "jdstarthist", "ncovhist", "ndethist")


def with_packet_fields(cols, seed):
    """trigger_bench's (object_id, jd, magpsf) with the three packet fields the features need."""
    rng = np.random.default_rng(seed)
    n = len(cols["jd"])
    ndet = rng.integers(1, 60, n).astype(np.int32)
    return dict(object_id=cols["object_id"], jd=cols["jd"], magpsf=cols["magpsf"],
                jdstarthist=2459000.5 - rng.choice([0.0, 2.5, 40.0], n), ndethist=ndet,
                ncovhist=(ndet + rng.integers(0, 900, n)).astype(np.int32))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    if not torch.cuda.is_available():
        sys.exit("feature_state_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    hist, sizes, ids = history(n)
    night, night_objects = nightly(ids)
    hist, night = with_packet_fields(hist, 2), with_packet_fields(night, 3)
    h = [torch.from_numpy(hist[k]).to(dev) for k in KEYS]
    b = [torch.from_numpy(night[k]).to(dev) for k in KEYS]
    capacity = 1 << max(10, int(np.ceil(np.log2(4 * (len(sizes) + NIGHTLY)))))   # load factor <= 1/4
    state = FeatureState(capacity, dev)
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def launcher(cols):
        m = cols[0].shape[0]
        perm, offsets = alert_utils._group_by_object(cols[0], then_by=cols[1])
        out = torch.empty((m, 8), dtype=torch.float32, device=dev)
        dropped = torch.empty(m, dtype=torch.uint8, device=dev)
        ptr = [C.c_void_p(x.data_ptr()) for x in (perm, offsets, *cols, out, dropped)]
        keep = (perm, offsets, out, dropped)

        def launch():
            _lib.check(L.btsbot_feature_update(C.byref(state._table), ptr[0], ptr[1], m, m, *ptr[2:], st),
                       "btsbot_feature_update")
            return keep
        return launch

    # (b) replay: the whole history in one call onto an empty state
    steps_r = max(1, min(50, 20_000_000 // max(n, 1)))
    rk_ms, rk_all = timed(launcher(h), steps_r, dev, before=state.reset)
    ru_ms, ru_all = timed(lambda: state.update(*h), steps_r, dev, before=state.reset)
    # (a) nightly: onto the state that holds the history (the batch's new objects are claimed by the first call)
    state.reset()
    state.update(*h)
    held = state.counters()
    nk_ms, nk_all = timed(launcher(b), NIGHTLY_STEPS, dev)
    nu_ms, nu_all = timed(lambda: state.update(*b), NIGHTLY_STEPS, dev)
    after = state.counters()
    # (c) the same rows without a state: alert_features over everything seen so far
    acc = [torch.cat([x, y]) for x, y in zip(h, b)]
    af_ms, af_all = timed(lambda: alert_utils.alert_features(*acc), steps_r, dev)
    r4 = lambda xs: [round(x, 4) for x in xs]   # noqa: E731
    print(json.dumps({
        "alerts": n, "objects": int(len(sizes)), "largest_object": int(sizes.max()), "median_object": float(np.median(sizes)),
        "capacity": capacity, "nightly_alerts": NIGHTLY, "nightly_objects": night_objects,
        "nightly_kernel_ms": round(nk_ms, 4), "nightly_update_ms": round(nu_ms, 4),
        "replay_kernel_ms": round(rk_ms, 4), "replay_update_ms": round(ru_ms, 4), "alert_features_ms": round(af_ms, 4),
        "nightly_over_alert_features": round(nu_ms / af_ms, 5),
        "blocks_nightly_kernel_ms": r4(nk_all), "blocks_nightly_update_ms": r4(nu_all),
        "blocks_replay_kernel_ms": r4(rk_all), "blocks_replay_update_ms": r4(ru_all), "blocks_alert_features_ms": r4(af_all),
        "steps_per_block": {"nightly": NIGHTLY_STEPS, "replay": steps_r, "alert_features": steps_r},
        "counters_after_replay": held, "counters_at_end": after, "device": torch.cuda.get_device_name(dev)}))


if __name__ == "__main__":
    main()
