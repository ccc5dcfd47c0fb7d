#!/usr/bin/env python3
"""A broker loop on the MI355X-native package: score the alerts of each night, then ask which objects a scanning policy
fires on NOW.

A synthetic, time-ordered alert stream (long-tailed object sizes: most objects a handful of alerts, a few in the hundreds)
is scored night by night with a seeded ``mm_ConvNeXt`` through ``btsbot.ScoreStream``; the scores go to a
``btsbot.TriggerState``, which keeps each object's history as a few numbers on the device and returns the night's new
triggers.  At the end the state's ``export()`` is compared with ``btsbot.policy_eval`` over the whole stream -- the only
way to get the same answer without the state, at a cost that grows with the history.

    python examples/trigger_example.py [--alerts 4096] [--nights 16] [--precision f16]
"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd as btsbot  # noqa: E402
from btsbot_amd.synthetic import METADATA_COLS, synthetic_batch  # noqa: E402


def synthetic_stream(n, nights, seed=0):
    """object_id int64 [n] and jd float64 [n], sorted by jd: Pareto object sizes (capped at 400), every object's alerts
    spread over a window of the survey, object ids scattered over the int64 range a broker's hashes would use."""
    rng = np.random.default_rng(seed)
    sizes, left = [], n
    while left > 0:
        s = int(min(min(rng.pareto(1.1) * 4 + 1, 400), left))
        sizes.append(s)
        left -= s
    sizes = np.array(sizes)
    ids = rng.integers(-2 ** 62, 2 ** 62, len(sizes), dtype=np.int64)
    start = rng.uniform(0, nights * 0.7, len(sizes))
    jd = 2459000.5 + np.repeat(start, sizes) + rng.uniform(0, nights * 0.3, n)
    order = np.argsort(jd, kind="stable")
    return np.repeat(ids, sizes)[order], jd[order], sizes


def seeded_model(precision):
    cfg = dict(pretrained=False, train_data_version="v11", metadata_cols=METADATA_COLS, meta_fc1_neurons=128,
               meta_fc2_neurons=128, meta_dropout=0.25, comb_fc1_neurons=128, comb_fc2_neurons=32, comb_dropout=0.2,
               model_kind="convnext_pico.d1_in1k")
    torch.manual_seed(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return btsbot.mm_ConvNeXt(cfg, precision=precision)


def main():
    p = argparse.ArgumentParser(description="Streaming policy triggers over a synthetic alert stream (MI355X)")
    p.add_argument("--alerts", type=int, default=4096)
    p.add_argument("--nights", type=int, default=16)
    p.add_argument("--precision", type=str, default="f16", choices=["f32", "bf16", "f16", "f16x2"])
    p.add_argument("--batch", type=int, default=256, help="alerts per forward")
    args = p.parse_args()
    dev = torch.device("cuda:0")

    object_id, jd, sizes = synthetic_stream(args.alerts, args.nights)
    images, metadata, _ = synthetic_batch(args.alerts, seed=5)
    magpsf = metadata[:, METADATA_COLS.index("magpsf")].double()
    object_id, jd = torch.from_numpy(object_id).to(dev), torch.from_numpy(jd).to(dev)
    images, metadata, magpsf = images.to(dev), metadata.to(dev), magpsf.to(dev)
    print(f"{args.alerts} alerts of {len(sizes)} objects (largest {sizes.max()}) over {args.nights} nights")

    scorer = btsbot.ScoreStream(seeded_model(args.precision).to(dev).eval(), depth=2)
    state = btsbot.TriggerState(btsbot.REFERENCE_POLICIES, capacity=1 << 14, device=dev)
    names = list(state.policies)
    night = torch.floor(jd - 2459000.5).long()
    all_scores = []
    for k in range(int(night.max().item()) + 1):
        rows = (night == k).nonzero()[:, 0]
        if rows.numel() == 0:
            continue
        batches = [(images[r], metadata[r]) for r in rows.split(args.batch)]
        with torch.no_grad():
            scores = torch.cat([torch.sigmoid(z).squeeze(1) for z in scorer.map(batches)])
        all_scores.append(scores)
        new = state.new_triggers(object_id[rows], jd[rows], magpsf[rows], scores)
        per_policy = torch.bincount(new["policy"], minlength=len(names)).tolist()
        first = ", ".join(f"{int(o)}:{names[int(q)]}@{float(t):.2f}" for o, q, t in
                          zip(new["object_id"][:2], new["policy"][:2], new["trigger_jd"][:2]))
        print(f"night {k:2d}: {rows.numel():5d} alerts, new triggers {dict(zip(names, per_policy))}" +
              (f"  e.g. {first}" if first else ""))

    print("counters:", state.counters())
    got = state.export()
    want = btsbot.policy_eval(object_id, jd, magpsf, torch.zeros_like(object_id), torch.cat(all_scores))
    for key in ("object_id", "n_alerts", "min_magpsf", "pred", "trigger_jd", "trigger_mag"):
        g, w = got[key], want[key]
        same = g.shape == w.shape and bool(((g == w) | ((g != g) & (w != w))).all())
        if not same:
            raise SystemExit(f"export() differs from policy_eval over the whole stream in {key!r}")
    print(f"export() equals policy_eval over the whole stream: {got['object_id'].numel()} objects, "
          f"{got['pred'].sum(0).tolist()} fired per policy")


if __name__ == "__main__":
    main()
