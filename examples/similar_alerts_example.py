#!/usr/bin/env python3
"""Which labelled SOURCES of the archive look like tonight's candidates?

A seeded ``mm_ConvNeXt`` embeds a synthetic, labelled archive in which every ``--epochs`` consecutive alerts are one
source (``alert_utils.object_keys`` of their ZTF names); ``btsbot.EmbeddingIndex(..., groups=ids)`` packs the rows once.
A night of new alerts -- further epochs of archive sources -- is then streamed through
``btsbot.ScoreStream(embed="features")`` -- the embedding row comes out of the launch that scores the batch -- and each
batch is looked up in the index with ``one_per_group`` and the alert's own source excluded: the k nearest sources, each by
its nearest alert, their distances and the distance-weighted vote of their labels (``btsbot.neighbor_vote``), next to the
model's own score.  Without the two switches the answer would be the other epochs of the alert's own source.  Nothing of
size night x archive is ever formed.

With ``--ivf N_LISTS`` the labelled archive is a ``btsbot.IvfIndex(..., groups=ids)`` -- the index for archives too large
for the linear search -- asked with the same two switches over the lists of each alert's ``--nprobe`` nearest centroids,
and the recall of its sources against the exact grouped answer of the same run is printed.

    python examples/similar_alerts_example.py [--archive 4096] [--night 512] [--k 7] [--epochs 4] [--metric cosine]
                                              [--ivf N_LISTS] [--nprobe 8]
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
    p.add_argument("--k", type=int, default=7, help="sources per alert (at most 32)")
    p.add_argument("--epochs", type=int, default=4, help="alerts per archive source")
    p.add_argument("--metric", type=str, default="euclidean", choices=list(btsbot.neighbors.METRICS))
    p.add_argument("--precision", type=str, default="f16", choices=["f32", "bf16", "f16", "f16x2"])
    p.add_argument("--batch", type=int, default=256, help="alerts per forward")
    p.add_argument("--show", type=int, default=8, help="alerts printed")
    p.add_argument("--ivf", type=int, default=0, metavar="N_LISTS", help="ask an IvfIndex of this many lists (0: the exact search)")
    p.add_argument("--nprobe", type=int, default=8, help="lists searched per alert with --ivf")
    args = p.parse_args()
    if args.ivf and args.metric != "euclidean":
        p.error("--ivf is built for --metric euclidean only")
    dev = torch.device("cuda:0")
    model = seeded_model(args.precision).to(dev).eval()

    def batches(images, meta):
        return [(i.to(dev), m.to(dev)) for i, m in zip(images.split(args.batch), meta.split(args.batch))]

    images, meta, labels = synthetic_batch(args.archive, seed=11)
    labels = labels.to(dev).reshape(-1) > 0.5
    names = btsbot.alert_utils.object_names(range(21 * 26 ** 7, 21 * 26 ** 7 + -(-args.archive // args.epochs)))
    source = torch.from_numpy(btsbot.alert_utils.object_keys(names)).to(dev)       # one id per source
    groups = source.repeat_interleave(args.epochs)[:args.archive]                  # ... and per archive alert
    labels = labels[::args.epochs].repeat_interleave(args.epochs)[:args.archive]   # a source has one label
    stream = btsbot.ScoreStream(model, depth=2, embed="features")
    with torch.no_grad():
        index = None
        for _logits, emb in stream.map(batches(images, meta)):      # the archive enters the index batch by batch
            g = groups[len(index) if index is not None else 0:][:emb.shape[0]]
            index = btsbot.EmbeddingIndex(emb, args.metric, groups=g) if index is None else index.add(emb, groups=g)
    print(f"archive: {len(index)} alerts of {len(source)} sources, {int(labels.sum())} alerts labelled real, "
          f"embedding width {index.dim}")
    ivf = None
    if args.ivf:
        ivf = btsbot.IvfIndex(index.bank, args.ivf, groups=index.groups)
        nprobe = min(args.nprobe, ivf.n_lists)
        print(f"ivf: {ivf.n_lists} lists, the largest of {int(ivf.list_sizes.max())} alerts; {nprobe} probed per alert")

    images, meta, truth = synthetic_batch(args.night, seed=12)
    own = source[torch.arange(args.night, device=dev) % len(source)]               # tonight's alerts: archive sources
    shown = 0
    agree = total = found = asked = 0
    with torch.no_grad():
        for logits, emb in stream.map(batches(images, meta)):
            kw = dict(query_groups=own[total:total + emb.shape[0]], exclude_same_group=True, one_per_group=True)
            idx, dist = index.query(emb, args.k, **kw)
            if ivf is not None:
                exact = idx
                idx, dist = ivf.query(emb, args.k, nprobe, **kw)
                hit = (groups[idx.clamp(min=0)][:, :, None] == groups[exact.clamp(min=0)][:, None, :]) & (idx >= 0)[:, :, None]
                found += int((hit.any(dim=1) & (exact >= 0)).sum())
                asked += int((exact >= 0).sum())
            majority = btsbot.neighbor_vote(idx, dist, labels, weights="distance") > 0.5
            score = torch.sigmoid(logits).reshape(-1)
            agree += int((majority == (score > 0.5)).sum())
            total += int(score.numel())
            for r in range(min(args.show - shown, emb.shape[0])):
                near = [names[i // args.epochs] for i in idx[r].tolist() if i >= 0]
                print(f"alert {shown:4d} of {names[shown % len(names)]}: score {float(score[r]):.3f}  nearest sources "
                      f"{near}  nearest {float(dist[r, 0]):.4f} farthest {float(dist[r, -1]):.4f}  "
                      f"weighted label {'real' if bool(majority[r]) else 'bogus'}")
                shown += 1
    print(f"{total} alerts of the night: the nearest sources' weighted label agrees with the model's own call on {agree}")
    if ivf is not None:
        print(f"ivf: {found} of the {asked} sources of the exact grouped answer found ({found / max(asked, 1):.4f} recall)")
    del truth


if __name__ == "__main__":
    main()
