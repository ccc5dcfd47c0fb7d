#!/usr/bin/env python
"""Map of the embeddings: embed a synthetic labelled set, lay the rows out with btsbot_amd.embedding_layout and save the
scatter.

    python examples/embedding_layout_example.py [--n 4096] [--out embedding_layout.png] [--csv PATH]

Two synthetic populations (the second brighter in its stamps and shifted in its metadata) go through ``model.embed`` of
a seeded mm_ConvNeXt; the map is the 2-D UMAP layout of the rows (kNN graph -> fuzzy graph -> 200 deterministic epochs,
all on the device).  Prints the map's extent and how pure its neighbourhoods are in the population label; --csv writes
the reference's columns ``umap_emb_1, umap_emb_2`` with the label.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402
from btsbot_amd.synthetic import synthetic_batch   # noqa: E402
from trigger_example import seeded_model   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", default="embedding_layout.png")
    ap.add_argument("--csv", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", default="f16", choices=["f32", "bf16", "f16", "f16x2"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("embedding_layout_example: needs a GPU (btsbot_amd has no CPU fallback)")
    dev = torch.device("cuda:0")

    # two populations: the second one brighter in its stamps and shifted in its metadata
    images, meta, _ = synthetic_batch(args.n, seed=args.seed + 11)
    labels = torch.arange(args.n) % 2
    images = images * (1.0 + 0.5 * labels)[:, None, None, None]
    meta = meta + 2.0 * meta.std(dim=0) * labels[:, None]
    labels = labels.numpy()
    model = seeded_model(args.precision).to(dev).eval()
    with torch.no_grad():
        emb = torch.cat([model.embed(image_input=i.to(dev), metadata_input=m.to(dev), layer="features")
                         for i, m in zip(images.split(256), meta.split(256))])

    y = btsbot_amd.embedding_layout(emb, n_neighbors=15, min_dist=0.1, n_epochs=200, seed=args.seed).cpu().numpy()
    idx, _ = btsbot_amd.knn_graph(torch.from_numpy(y).to(dev), 6)
    purity = float((labels[idx[:, 1:].cpu().numpy()] == labels[:, None]).mean())
    print(f"{args.n} rows of width {emb.shape[1]} -> map of extent x [{y[:, 0].min():.1f}, {y[:, 0].max():.1f}], "
          f"y [{y[:, 1].min():.1f}, {y[:, 1].max():.1f}]; 5-neighbour label purity in the map {purity:.3f}")
    q = btsbot_amd.map_quality(emb, torch.from_numpy(y).to(dev), 15)
    print(f"map quality at k = {q['k']} over {q['rows']} rows: trustworthiness {q['trustworthiness']:.4f}, continuity "
          f"{q['continuity']:.4f}, neighbour recall {q['neighbor_recall']:.3f}")
    if args.csv:
        import pandas as pd
        pd.DataFrame({"umap_emb_1": y[:, 0], "umap_emb_2": y[:, 1], "label": labels}).to_csv(args.csv, index=False)
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(figsize=(6, 6))
    for lab, colour in ((0, "tab:blue"), (1, "tab:orange")):
        ax.scatter(*y[labels == lab].T, s=2, c=colour, label=f"label {lab}")
    ax.set_xlabel("umap_emb_1")
    ax.set_ylabel("umap_emb_2")
    ax.legend(markerscale=5)
    fig.savefig(args.out, dpi=150)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
