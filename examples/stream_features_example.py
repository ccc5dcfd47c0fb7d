#!/usr/bin/env python3
"""A broker loop with both per-object states: the metadata a model reads is continued from each object's history, the
scores it returns go to the scanning policies.

The synthetic, time-ordered alert stream of ``trigger_example.py`` is taken night by night.  ``btsbot.FeatureState`` keeps
each object's light curve so far as a few numbers on the device and fills the six model columns that are not packet
fields (``age``, ``days_since_peak``, ``days_to_peak``, ``peakmag_so_far``, ``maxmag_so_far``, ``nnotdet``) for tonight's
alerts; a seeded ``mm_ConvNeXt`` scores them through ``btsbot.ScoreStream``; ``btsbot.TriggerState`` takes the scores.  At
the end the rows of all nights are compared with ``btsbot.alert_features`` over the whole stream -- the only way to the
same metadata without the state, at a cost that grows with the history -- and ``export()`` with its whole-curve columns.

With ``--retain-days D`` both states forget, every night, the objects they have not seen for D days (``expire``: on the
device, no host synchronisation), which is what keeps a long-running service's tables from filling up.  An object that
comes back after that is a new object, so the comparison with the whole stream is not made; the numbers of objects
expired are printed instead.

    python examples/stream_features_example.py [--alerts 4096] [--nights 16] [--precision f16] [--retain-days 5]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd as btsbot  # noqa: E402
from btsbot_amd.synthetic import METADATA_COLS, synthetic_batch  # noqa: E402
from trigger_example import seeded_model, synthetic_stream  # noqa: E402

MODEL_COLS = ("peakmag_so_far", "maxmag_so_far", "age", "days_since_peak", "days_to_peak", "nnotdet")


def same(a, b):
    return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


def main():
    p = argparse.ArgumentParser(description="Streaming light-curve features over a synthetic alert stream (MI355X)")
    p.add_argument("--alerts", type=int, default=4096)
    p.add_argument("--nights", type=int, default=16)
    p.add_argument("--precision", type=str, default="f16", choices=["f32", "bf16", "f16", "f16x2"])
    p.add_argument("--batch", type=int, default=256, help="alerts per forward")
    p.add_argument("--retain-days", type=float, default=None,
                   help="every night, expire the objects not seen for this many days from both states")
    args = p.parse_args()
    dev = torch.device("cuda:0")

    object_id, jd, sizes = synthetic_stream(args.alerts, args.nights)
    images, metadata, _ = synthetic_batch(args.alerts, seed=5)
    rng = np.random.default_rng(3)
    # the packet fields the features are made of: the survey saw each field before the object's first detection
    first = {int(o): jd[object_id == o].min() for o in np.unique(object_id)}
    jdstarthist = np.array([first[int(o)] for o in object_id]) - rng.choice([0.0, 2.5, 40.0], args.alerts)
    ndethist = rng.integers(1, 60, args.alerts).astype(np.int32)
    ncovhist = (ndethist + rng.integers(0, 900, args.alerts)).astype(np.int32)
    magpsf = metadata[:, METADATA_COLS.index("magpsf")].double()
    object_id, jd, jdstarthist, ncovhist, ndethist = (torch.from_numpy(x).to(dev) for x in
                                                      (object_id, jd, jdstarthist, ncovhist, ndethist))
    images, metadata, magpsf = images.to(dev), metadata.to(dev), magpsf.to(dev)
    print(f"{args.alerts} alerts of {len(sizes)} objects (largest {sizes.max()}) over {args.nights} nights")

    dst = torch.tensor([METADATA_COLS.index(c) for c in MODEL_COLS], device=dev)
    src = torch.tensor([btsbot.CUSTOM_COLS.index(c) for c in MODEL_COLS], device=dev)
    scorer = btsbot.ScoreStream(seeded_model(args.precision).to(dev).eval(), depth=2)
    feats = btsbot.FeatureState(capacity=1 << 14, device=dev)
    state = btsbot.TriggerState(btsbot.REFERENCE_POLICIES, capacity=1 << 14, device=dev)
    names = list(state.policies)
    night = torch.floor(jd - 2459000.5).long()
    seen_rows, seen_feats = [], []
    for k in range(int(night.max().item()) + 1):
        if args.retain_days is not None:
            feats.expire(2459000.5 + k - args.retain_days)
            state.expire(2459000.5 + k - args.retain_days)
        rows = (night == k).nonzero()[:, 0]
        if rows.numel() == 0:
            continue
        out = feats.update(object_id[rows], jd[rows], magpsf[rows], jdstarthist[rows], ncovhist[rows], ndethist[rows])
        meta = metadata[rows]
        meta[:, dst] = out["features"][:, src]
        seen_rows.append(rows)
        seen_feats.append(out["features"])
        batches = [(images[r], m) for r, m in zip(rows.split(args.batch), meta.split(args.batch))]
        with torch.no_grad():
            scores = torch.cat([torch.sigmoid(z).squeeze(1) for z in scorer.map(batches)])
        new = state.new_triggers(object_id[rows], jd[rows], magpsf[rows], scores)
        per_policy = torch.bincount(new["policy"], minlength=len(names)).tolist()
        print(f"night {k:2d}: {rows.numel():5d} alerts, median age {float(out['features'][:, 4].median()):6.2f} d, "
              f"new triggers {dict(zip(names, per_policy))}")

    print("feature counters:", feats.counters())
    print("trigger counters:", state.counters())
    if args.retain_days is not None:
        print(f"expired after {args.retain_days:g} quiet days: {feats.n_expired()} objects from the feature state, "
              f"{state.n_expired()} from the trigger state (an object that came back was made afresh)")
        return
    rows, got = torch.cat(seen_rows), torch.cat(seen_feats)
    want = btsbot.alert_features(object_id, jd, magpsf, jdstarthist, ncovhist, ndethist)
    if not same(got[:, 2:], want[rows][:, 2:]):
        raise SystemExit("the nightly rows differ from alert_features over the whole stream in columns 2-7")
    exported = feats.export()
    at = torch.searchsorted(exported["object_id"], object_id)
    final = torch.stack([exported["peakmag"][at], exported["maxmag"][at]], dim=1).float()
    if not same(final, want[:, :2]):
        raise SystemExit("export() differs from alert_features over the whole stream in peakmag / maxmag")
    print(f"columns 2-7 of all nights equal alert_features over the whole stream, and export()'s peakmag / maxmag its "
          f"columns 0-1: {rows.numel()} alerts, {exported['object_id'].numel()} objects")


if __name__ == "__main__":
    main()
