#!/usr/bin/env python
"""Time the data of the diagnostic figure (btsbot_alert_histograms, diagnostics.*) on one GPU:

    python tools/diagnostic_bench.py [N]          # N alerts, default 1,000,000

Two score distributions: "uniform", and "trained" -- 45 % of the scores within 0.02 of 0, 45 % within 0.02 of 1, the rest
uniform: what a trained model gives, nearly every alert in the first or the last score bin.  Magnitudes are uniform over
15.5-21.5 in hundredths, labels follow the score loosely, objects are long-tailed as in tools/policy_bench.py.  Timed warm
(>= 0.5 s of the same work first), seven blocks, the MEDIAN block reported.  Prints one JSON line per distribution:
  kernel_ms       the one launch of btsbot_alert_histograms into a buffer that is not cleared (HIP events)
  hist_ms         diagnostics.alert_histograms: conversions, the zeroed buffer, the launch (HIP events; no host read)
  torch_ms        the same counts written with torch ops -- bucketize + bincount per histogram, as a caller without the
                  kernel would -- checked equal to the kernel's once (HIP events around calls that synchronise inside)
  torch_over_kernel, torch_over_hist   the ratios
  roc_ms          diagnostics.roc_points (host clock: the call ends in its host read)
  data_ms         the whole diagnostics.diagnostic_data with junk / save / trigger columns (host clock)
Workgroup size, grid cap and counter layout are build-time choices of csrc/alert_hist.hip (ALERT_HIST_WG, ALERT_HIST_GRID,
ALERT_HIST_LAYOUT); to time another one, build it with tools/build_variant.sh and point the binding at that library.
``library`` in the output names the one that ran.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from btsbot_amd import _lib, diagnostics   # noqa: E402
from policy_bench import host_timed, timed   # noqa: E402


def synthetic(n, dist, seed=0):
    rng = np.random.default_rng(seed)
    sizes = np.minimum((rng.pareto(1.1, n) * 4 + 1).astype(np.int64), 4000)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), n)) + 1]
    oid = np.repeat(np.arange(len(sizes), dtype=np.int64) * 977 - 12345, sizes)[:n]
    u = rng.random(n)
    if dist == "uniform":
        score = u
    else:
        pick = rng.random(n)
        score = np.where(pick < 0.45, 0.02 * u, np.where(pick < 0.9, 1 - 0.02 * u, u))
    label = (rng.random(n) < 0.15 + 0.7 * score).astype(np.int64)
    save = np.where((oid // 977) % 2 == 0, 2459300.5 + (oid % 400), np.nan)
    order = rng.permutation(n)
    cols = dict(object_id=oid, jd=2459000.5 + rng.uniform(0, 700, n), magpsf=np.round(rng.uniform(15.5, 21.5, n), 2),
                label=label, raw_preds=score.astype(np.float32), junk=(oid % 50) == 0, save_time=save,
                trigger_time=save - 1.5)
    return {k: v[order] for k, v in cols.items()}


def torch_histograms(mag, raw, lab, me, se, ce):
    """btsbot_alert_histograms's counts from torch ops: the bin by bucketize (right=True, the last edge folded into the last
    bin, everything outside sent to a spare bin), the counts by bincount."""
    def bins(x, e):
        nb = e.numel() - 1
        idx = (torch.bucketize(x, e, right=True) - 1).clamp(max=nb - 1)
        return torch.where((x >= e[0]) & (x <= e[-1]), idx, torch.full_like(idx, nb)), nb
    s = raw.to(torch.float64)
    (mb, nm), (sb, ns), (cb, nc) = bins(mag, me), bins(s, se), bins(mag, ce)
    pred, pos = s > 0.5, lab != 0
    cls = torch.where(pos, torch.where(pred, 0, 3), torch.where(pred, 1, 2))
    joint = torch.where((mb < nm) & (sb < ns), mb * ns + sb, torch.full_like(mb, nm * ns))
    return torch.cat([torch.bincount(joint, minlength=nm * ns + 1)[:nm * ns], torch.bincount(mb, minlength=nm + 1)[:nm],
                      torch.bincount(sb, minlength=ns + 1)[:ns],
                      torch.bincount(torch.where(cb < nc, cls * nc + cb, torch.full_like(cb, 4 * nc)), minlength=4 * nc + 1)[:4 * nc],
                      torch.bincount(cls, minlength=4)])


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    if not torch.cuda.is_available():
        sys.exit("diagnostic_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    for dist in ("uniform", "trained"):
        t = {k: torch.from_numpy(v).to(dev) for k, v in synthetic(n, dist).items()}
        mag, raw, lab = t["magpsf"], t["raw_preds"], t["label"]
        lab32 = lab.to(torch.int32)
        ref = diagnostics.alert_histograms(mag, raw, lab)
        me, se, ce = (ref[k] for k in ("mag_edges", "score_edges", "class_edges"))
        dev_edges = [torch.from_numpy(e).to(dev) for e in (me, se, ce)]
        same = torch.equal(torch_histograms(mag, raw, lab, *dev_edges), ref["counts"])
        out = torch.zeros_like(ref["counts"])
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def kernel():
            _lib.check(L.btsbot_alert_histograms(C.c_void_p(mag.data_ptr()), C.c_void_p(raw.data_ptr()),
                                                 C.c_void_p(lab32.data_ptr()), n, me.ctypes.data_as(dp), len(me) - 1,
                                                 se.ctypes.data_as(dp), len(se) - 1, ce.ctypes.data_as(dp), len(ce) - 1,
                                                 C.c_void_p(out.data_ptr()), st), "btsbot_alert_histograms")

        steps = max(1, min(50, 20_000_000 // max(n, 1)))
        args = [t[k] for k in ("object_id", "jd", "magpsf", "label", "raw_preds")]
        extra = {k: t[k] for k in ("junk", "save_time", "trigger_time")}
        k_ms, k_all = timed(kernel, steps, dev)
        h_ms, h_all = timed(lambda: diagnostics.alert_histograms(mag, raw, lab), steps, dev)
        t_ms, t_all = timed(lambda: torch_histograms(mag, raw, lab, *dev_edges), steps, dev)
        r_ms, r_all = host_timed(lambda: diagnostics.roc_points(raw, lab), max(1, steps // 4))
        d_ms, d_all = host_timed(lambda: diagnostics.diagnostic_data(*args, **extra), max(1, steps // 4))
        roc = diagnostics.roc_points(raw, lab)
        print(json.dumps({
            "distribution": dist, "alerts": n, "library": os.path.basename(_lib.LIB_PATH), "torch_form_equal": bool(same),
            "first_last_score_bin_share": round(float(ref["score"][0] + ref["score"][-1]) / n, 4),
            "kernel_ms": round(k_ms, 4), "hist_ms": round(h_ms, 4), "torch_ms": round(t_ms, 4),
            "torch_over_kernel": round(t_ms / k_ms, 2), "torch_over_hist": round(t_ms / h_ms, 2),
            "roc_ms": round(r_ms, 4), "data_ms": round(d_ms, 4), "roc_points": len(roc["fpr"]), "auc": round(roc["auc"], 6),
            "blocks_kernel_ms": [round(x, 4) for x in k_all], "blocks_hist_ms": [round(x, 4) for x in h_all],
            "blocks_torch_ms": [round(x, 4) for x in t_all], "blocks_roc_ms": [round(x, 4) for x in r_all],
            "blocks_data_ms": [round(x, 4) for x in d_all], "steps_per_block": steps,
            "device": torch.cuda.get_device_name(dev)}), flush=True)


if __name__ == "__main__":
    main()
