#!/usr/bin/env python3
"""Which cluster of the archive does each of tonight's alerts belong to?

A seeded ``mm_ConvNeXt`` embeds a synthetic archive: ``--kinds`` kinds of sources (a kind is one stamp and one metadata
row; its sources are noisy copies), plus a few sources unlike any kind.  ``btsbot.ClusterModel`` fits HDBSCAN on the
archive's embedding rows once.  A night of new alerts -- further sources of the same kinds, and some strangers -- is then
streamed through ``btsbot.ScoreStream(embed="features")``: the embedding row comes out of the launch that scores the
batch, and ``model.predict`` places it in the fitted clusters from one neighbour search, without a refit.  Each alert's
cluster, membership strength and GLOSH outlier score are printed.

    python examples/cluster_new_alerts_example.py [--kinds 6] [--per-kind 120] [--night 48] [--strangers 4]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd as btsbot  # noqa: E402
from btsbot_amd.synthetic import META_RANGES, synthetic_batch  # noqa: E402
from trigger_example import seeded_model  # noqa: E402


def copies_of(images, meta, kind, seed, noise=0.02):
    """one alert per entry of ``kind``: that kind's stamps and metadata plus noise"""
    gen = torch.Generator().manual_seed(seed)
    img, m = images[kind], meta[kind]
    span = torch.tensor([hi - lo for lo, hi in META_RANGES])
    return (img * (1.0 + noise * torch.randn(img.shape, generator=gen)),
            m + 0.1 * noise * span * torch.randn(m.shape, generator=gen))


def main():
    p = argparse.ArgumentParser(description="Assign a night's alerts to the archive's HDBSCAN clusters (MI355X)")
    p.add_argument("--kinds", type=int, default=6)
    p.add_argument("--per-kind", type=int, default=120, help="archive sources per kind")
    p.add_argument("--night", type=int, default=48)
    p.add_argument("--strangers", type=int, default=4, help="alerts of tonight that are of no archive kind")
    p.add_argument("--min-cluster-size", type=int, default=10)
    p.add_argument("--precision", type=str, default="f16", choices=["f32", "bf16", "f16", "f16x2"])
    p.add_argument("--batch", type=int, default=256, help="alerts per forward")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cluster_new_alerts_example: needs a GPU (btsbot_amd has no CPU fallback)")
    dev = torch.device("cuda:0")
    model = seeded_model(args.precision).to(dev).eval()
    images, meta, _ = synthetic_batch(args.kinds + args.strangers, seed=31)      # the kinds, then the strangers

    def batches(img, m):
        return [(i.to(dev), j.to(dev)) for i, j in zip(img.split(args.batch), m.split(args.batch))]

    stream = btsbot.ScoreStream(model, depth=2, embed="features")
    kind = torch.arange(args.kinds).repeat_interleave(args.per_kind)
    with torch.no_grad():
        index = None
        for _logits, emb in stream.map(batches(*copies_of(images, meta, kind, 32))):
            index = btsbot.EmbeddingIndex(emb) if index is None else index.add(emb)
    fit = btsbot.ClusterModel(index, min_cluster_size=args.min_cluster_size)
    found = int(fit.labels.max()) + 1
    print(f"archive: {len(index)} alerts of {args.kinds} kinds, embedding width {index.dim}; HDBSCAN finds {found} "
          f"clusters, {int((fit.labels < 0).sum())} rows are noise; GLOSH of the archive: median "
          f"{float(fit.outlier_scores.nanmedian()):.3f}, largest {float(fit.outlier_scores.max()):.3f}")

    gen = torch.Generator().manual_seed(33)
    tonight = torch.cat([torch.randint(0, args.kinds, (args.night - args.strangers,), generator=gen),
                         args.kinds + torch.arange(args.strangers)])[torch.randperm(args.night, generator=gen)]
    labels, prob, score = [], [], []
    stats = {}
    with torch.no_grad():
        for _logits, emb in stream.map(batches(*copies_of(images, meta, tonight, 34))):
            lab, pr, det = fit.predict(emb, return_details=True, stats=stats)
            labels.append(lab), prob.append(pr), score.append(det["outlier"])
    labels, prob, score = torch.cat(labels), torch.cat(prob), torch.cat(score)
    print(f"tonight: {args.night} alerts, {int((labels < 0).sum())} in no cluster; the last batch sent "
          f"{stats['unresolved']} rows through the radius tier")
    for i in range(args.night):
        what = f"kind {int(tonight[i])}" if tonight[i] < args.kinds else "stranger"
        where = f"cluster {int(labels[i]):3d}" if labels[i] >= 0 else "no cluster "
        print(f"  alert {i:3d} ({what:>8})  {where}  strength {float(prob[i]):.3f}  GLOSH {float(score[i]):.3f}")


if __name__ == "__main__":
    main()
