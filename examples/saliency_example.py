#!/usr/bin/env python3
"""Which pixels and which metadata columns moved this score?

A seeded ``mm_ConvNeXt`` scores a synthetic batch; ``btsbot.saliency`` then attributes every alert's score to its
3 x 63 x 63 triplet and its metadata row with the chosen method (``gradient``, ``gradient_x_input``, ``smoothgrad``,
``integrated_gradients``) -- all of it on the device, through the HIP backward (``model.input_gradients``).  Writes an
``.npz`` with the scores, the maps and the metadata attributions, prints the ten metadata columns with the largest mean
|attribution|, and, where matplotlib is installed, one figure of the science, reference and difference cutouts of the first
alerts beside their maps.

    python examples/saliency_example.py [--alerts 64] [--method integrated_gradients] [--out saliency.npz]
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
from trigger_example import seeded_model  # noqa: E402


def figure(path, images, maps, scores, rows):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("saliency_example: matplotlib is not installed, no figure written")
        return
    names = ("science", "reference", "difference")
    fig, axes = plt.subplots(rows, 6, figsize=(12, 2 * rows), squeeze=False)
    for r in range(rows):
        for c in range(3):
            axes[r][2 * c].imshow(images[r, c], cmap="gray")
            lim = float(np.abs(maps[r, c]).max()) or 1.0
            axes[r][2 * c + 1].imshow(maps[r, c], cmap="seismic", vmin=-lim, vmax=lim)
            if r == 0:
                axes[r][2 * c].set_title(names[c])
                axes[r][2 * c + 1].set_title(names[c] + " map")
        axes[r][0].set_ylabel(f"score {scores[r]:.2f}")
    for ax in axes.flat:
        ax.set_xticks([])
        ax.set_yticks([])
    fig.tight_layout()
    fig.savefig(path, dpi=120)
    print(f"wrote {path}")


def main():
    p = argparse.ArgumentParser(description="Saliency maps of BTSbot scores through the HIP backward (MI355X)")
    p.add_argument("--alerts", type=int, default=64)
    p.add_argument("--method", type=str, default="integrated_gradients", choices=list(btsbot.attribution.METHODS))
    p.add_argument("--target", type=str, default="score", choices=list(btsbot.attribution.TARGETS))
    p.add_argument("--precision", type=str, default="f32", choices=["f32", "bf16", "f16", "f16x2"])
    p.add_argument("--out", type=str, default="saliency.npz")
    p.add_argument("--rows", type=int, default=4, help="alerts in the figure")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("saliency_example: needs a GPU (btsbot_amd has no CPU fallback)")
    dev = torch.device("cuda:0")
    model = seeded_model(args.precision).to(dev).eval()
    images, meta, _ = synthetic_batch(args.alerts, seed=31)
    images, meta = images.to(dev), meta.to(dev)
    with torch.no_grad():
        scores = torch.sigmoid(model(image_input=images, metadata_input=meta)).reshape(-1)
    extra = {}
    if args.method == "integrated_gradients":
        img_attr, meta_attr, delta = btsbot.saliency(model, image_input=images, metadata_input=meta, method=args.method,
                                                     target=args.target, return_delta=True)
        extra["completeness_gap"] = delta.cpu().numpy()
        print(f"integrated gradients: largest completeness gap |sum(attr) - (f(x) - f(baseline))| = {float(delta.abs().max()):.3e}")
    else:
        img_attr, meta_attr = btsbot.saliency(model, image_input=images, metadata_input=meta, method=args.method,
                                              target=args.target)
    mean_abs = meta_attr.abs().mean(dim=0)
    order = mean_abs.argsort(descending=True)[:10].tolist()
    print(f"{args.alerts} alerts, {args.method} of the {args.target}; metadata columns by mean |attribution|:")
    for j in order:
        print(f"  {METADATA_COLS[j]:<16} {float(mean_abs[j]):.4e}")
    np.savez(args.out, scores=scores.cpu().numpy(), image_attribution=img_attr.cpu().numpy(),
             metadata_attribution=meta_attr.cpu().numpy(), metadata_cols=np.array(METADATA_COLS),
             top_columns=np.array([METADATA_COLS[j] for j in order]), **extra)
    print(f"wrote {args.out}")
    rows = min(args.rows, args.alerts)
    figure(os.path.splitext(args.out)[0] + ".png", images[:rows].cpu().numpy(), img_attr[:rows].cpu().numpy(),
           scores[:rows].cpu().numpy(), rows)


if __name__ == "__main__":
    main()
