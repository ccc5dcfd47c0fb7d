#!/usr/bin/env python3
"""Which labelled alerts of the archive look like tonight's candidates?

A seeded ``mm_ConvNeXt`` embeds a synthetic, labelled archive; ``btsbot.EmbeddingIndex`` packs the rows once.  A night of
new alerts is then streamed through ``btsbot.ScoreStream(embed="features")`` -- the embedding row comes out of the launch
that scores the batch -- and each batch is looked up in the index: the k nearest archive rows, their distances and the
majority label among them, next to the model's own score.  Nothing of size night x archive is ever formed.

    python examples/similar_alerts_example.py [--archive 4096] [--night 512] [--k 7] [--metric cosine]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd as btsbot  # noqa: E402
from btsbot_amd.synthetic import synthetic_batch  # noqa: E402
from trigger_example import seeded_model  # noqa: E402


def main():
    p = argparse.ArgumentParser(description="Nearest labelled archive alerts of a night's candidates (MI355X)")
    p.add_argument("--archive", type=int, default=4096)
    p.add_argument("--night", type=int, default=512)
    p.add_argument("--k", type=int, default=7)
    p.add_argument("--metric", type=str, default="euclidean", choices=list(btsbot.neighbors.METRICS))
    p.add_argument("--precision", type=str, default="f16", choices=["f32", "bf16", "f16", "f16x2"])
    p.add_argument("--batch", type=int, default=256, help="alerts per forward")
    p.add_argument("--show", type=int, default=8, help="alerts printed")
    args = p.parse_args()
    dev = torch.device("cuda:0")
    model = seeded_model(args.precision).to(dev).eval()

    def batches(images, meta):
        return [(i.to(dev), m.to(dev)) for i, m in zip(images.split(args.batch), meta.split(args.batch))]

    images, meta, labels = synthetic_batch(args.archive, seed=11)
    labels = labels.to(dev).reshape(-1) > 0.5
    stream = btsbot.ScoreStream(model, depth=2, embed="features")
    with torch.no_grad():
        index = None
        for _logits, emb in stream.map(batches(images, meta)):      # the archive enters the index batch by batch
            index = btsbot.EmbeddingIndex(emb, args.metric) if index is None else index.add(emb)
    print(f"archive: {len(index)} alerts, {int(labels.sum())} labelled real, embedding width {index.dim}")

    images, meta, truth = synthetic_batch(args.night, seed=12)
    shown = 0
    agree = total = 0
    with torch.no_grad():
        for logits, emb in stream.map(batches(images, meta)):
            idx, dist = index.query(emb, args.k)
            votes = labels[idx.clamp_min(0)] & (idx >= 0)
            majority = votes.sum(1) * 2 > (idx >= 0).sum(1)
            score = torch.sigmoid(logits).reshape(-1)
            agree += int((majority == (score > 0.5)).sum())
            total += int(score.numel())
            for r in range(min(args.show - shown, emb.shape[0])):
                print(f"alert {shown:4d}: score {float(score[r]):.3f}  neighbours {idx[r].tolist()}  "
                      f"nearest {float(dist[r, 0]):.4f} farthest {float(dist[r, -1]):.4f}  "
                      f"majority label {'real' if bool(majority[r]) else 'bogus'}")
                shown += 1
    print(f"{total} alerts of the night: the neighbours' majority label agrees with the model's own call on {agree}")
    del truth


if __name__ == "__main__":
    main()
