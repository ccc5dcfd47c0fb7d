#!/usr/bin/env python
"""Time btsbot_split_labels and splits.label_set (the per-object loop of cut_set_and_assign_splits) on one GPU:

    python tools/splits_bench.py [N]          # N alerts, default 1,000,000

The table is the one of tools/alert_features_bench.py (long-tailed object sizes capped at 4,000, shuffled order) and the
timing is the same: HIP events after >= 0.5 s of the same work, seven blocks, the MEDIAN block reported.  Prints one JSON
line:
  kernel_ms   the one launch of btsbot_split_labels on grouped input
  call_ms     splits.label_set end to end: stable sort of the ids, offsets, the launch, the host read of the distinct
              object sizes, the two RandomState draws on the host and the gathers of N and split
  alert_features_kernel_ms, alert_features_call_ms   the sibling kernel over the same table in the same run, for scale
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from alert_features_bench import synthetic, timed   # noqa: E402
from btsbot_amd import _lib, alert_utils, splits   # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    if not torch.cuda.is_available():
        sys.exit("splits_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    cols, sizes = synthetic(n)
    t = {k: torch.from_numpy(v).to(dev) for k, v in cols.items()}
    args = [t[k] for k in ("object_id", "jd", "magpsf")]
    want = splits.split_labels(*args)
    lab = splits.label_set(*args)
    assert int(lab["object_rank"].max()) + 1 == len(sizes)

    perm, offsets = alert_utils._group_by_object(t["object_id"])
    outs = [torch.empty_like(want[k]) for k in ("pos", "size", "first_row", "later")]
    outs += [torch.empty(n, dtype=torch.uint8, device=dev), torch.empty_like(want["peakmag"])]
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = [C.c_void_p(x.data_ptr()) for x in (perm, offsets, *args[1:], *outs)]

    def kernel():
        _lib.check(L.btsbot_split_labels(ptr[0], ptr[1], n, n, *ptr[2:], st), "btsbot_split_labels")

    kernel()
    torch.cuda.synchronize(dev)
    assert all(torch.equal(a, want[k]) for a, k in zip(outs[:4], ("pos", "size", "first_row", "later")))
    assert torch.equal(outs[4].bool(), want["is_rise"])

    af_args = [t[k] for k in ("object_id", "jd", "magpsf", "jdstarthist", "ncovhist", "ndethist")]
    af_out = torch.empty((n, 8), dtype=torch.float32, device=dev)
    af_ptr = [C.c_void_p(x.data_ptr()) for x in (perm, offsets, *af_args[1:], af_out)]

    def af_kernel():
        _lib.check(L.btsbot_alert_features(af_ptr[0], af_ptr[1], n, n, *af_ptr[2:], st), "btsbot_alert_features")

    steps = max(1, min(50, 20_000_000 // max(n, 1)))
    k_ms, k_all = timed(kernel, steps, dev)
    c_ms, c_all = timed(lambda: splits.label_set(*args), steps, dev)
    afk_ms, _ = timed(af_kernel, steps, dev)
    afc_ms, _ = timed(lambda: alert_utils.alert_features(*af_args), steps, dev)
    print(json.dumps({
        "alerts": n, "objects": int(len(sizes)), "largest_object": int(sizes.max()),
        "distinct_sizes": int(len(np.unique(sizes))), "objects_over_64": int((sizes > 64).sum()),
        "objects_over_tile": int((sizes > alert_utils.FEATURE_TILE).sum()),
        "kernel_ms": round(k_ms, 4), "call_ms": round(c_ms, 4),
        "alert_features_kernel_ms": round(afk_ms, 4), "alert_features_call_ms": round(afc_ms, 4),
        "blocks_kernel_ms": [round(x, 4) for x in k_all], "blocks_call_ms": [round(x, 4) for x in c_all],
        "steps_per_block": steps, "device": torch.cuda.get_device_name(dev)}))


if __name__ == "__main__":
    main()
