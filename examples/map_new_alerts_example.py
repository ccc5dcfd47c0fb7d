#!/usr/bin/env python3
"""Where do tonight's candidates fall on the archive's map?

A seeded ``mm_ConvNeXt`` embeds a synthetic archive of two populations (the second brighter in its stamps and shifted in
its metadata); ``btsbot.EmbeddingMap`` packs the rows and lays them out once.  A night of new alerts is then streamed
through ``btsbot.ScoreStream(embed="features")`` -- the embedding row comes out of the launch that scores the batch -- and
each batch is placed on the map with ``transform``: the archive's points do not move, so yesterday's figure still holds,
and a batch costs a neighbour search in the index plus one launch for the whole epoch schedule.  ``--extend`` also adds
each batch to the map, so that later alerts find it.

    python examples/map_new_alerts_example.py [--archive 4096] [--night 512] [--extend] [--out map_new_alerts.png]
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


def two_populations(n, seed):
    images, meta, _ = synthetic_batch(n, seed=seed)
    labels = torch.arange(n) % 2
    return images * (1.0 + 0.5 * labels)[:, None, None, None], meta + 2.0 * meta.std(dim=0) * labels[:, None], labels


def main():
    p = argparse.ArgumentParser(description="Place a night's alerts on the archive's embedding map (MI355X)")
    p.add_argument("--archive", type=int, default=4096)
    p.add_argument("--night", type=int, default=512)
    p.add_argument("--extend", action="store_true", help="add each batch to the map after placing it")
    p.add_argument("--precision", type=str, default="f16", choices=["f32", "bf16", "f16", "f16x2"])
    p.add_argument("--batch", type=int, default=256, help="alerts per forward")
    p.add_argument("--out", default="map_new_alerts.png")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("map_new_alerts_example: needs a GPU (btsbot_amd has no CPU fallback)")
    dev = torch.device("cuda:0")
    model = seeded_model(args.precision).to(dev).eval()
    stream = btsbot.ScoreStream(model, depth=2, embed="features")

    def batches(images, meta):
        return [(i.to(dev), m.to(dev)) for i, m in zip(images.split(args.batch), meta.split(args.batch))]

    images, meta, archive_labels = two_populations(args.archive, 11)
    with torch.no_grad():
        archive = torch.cat([emb for _logits, emb in stream.map(batches(images, meta))])
    m = btsbot.EmbeddingMap(archive, n_neighbors=15, min_dist=0.1, n_epochs=200, seed=0)
    archive_y = m.embedding_.clone()
    print(f"archive: {len(m)} alerts of embedding width {m.index.dim} laid out once")

    images, meta, night_labels = two_populations(args.night, 12)
    placed = []
    with torch.no_grad():
        for _logits, emb in stream.map(batches(images, meta)):
            placed.append(m.extend(emb) if args.extend else m.transform(emb))
    night_y = torch.cat(placed)
    assert torch.equal(m.embedding_[:args.archive], archive_y)                 # the archive has not moved
    # which population's archive points surround each new alert on the map?
    near = torch.cdist(night_y, archive_y).topk(5, largest=False).indices.cpu()
    purity = float((archive_labels[near] == night_labels[:, None]).float().mean())
    print(f"{args.night} alerts of the night placed; share of their 5 nearest archive points on the map that carry their "
          f"population label: {purity:.3f}; the map now holds {len(m)} points")

    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(figsize=(6, 6))
    a_y, n_y = archive_y.cpu().numpy(), night_y.cpu().numpy()
    for lab, colour in ((0, "tab:blue"), (1, "tab:orange")):
        ax.scatter(*a_y[archive_labels.numpy() == lab].T, s=2, c=colour, alpha=0.3, label=f"archive, label {lab}")
        ax.scatter(*n_y[night_labels.numpy() == lab].T, s=12, c=colour, edgecolors="k", linewidths=0.4,
                   label=f"tonight, label {lab}")
    ax.set_xlabel("umap_emb_1")
    ax.set_ylabel("umap_emb_2")
    ax.legend(markerscale=2)
    fig.savefig(args.out, dpi=150)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
