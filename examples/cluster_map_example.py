#!/usr/bin/env python
"""Clumps of a map, and how new a night is: lay a synthetic archive out, cluster the map with btsbot_amd.dbscan and count,
for the rows of new nights, the archive rows within r of each (btsbot_amd.EmbeddingIndex.count_within).

    python examples/cluster_map_example.py [--n 6000] [--nights 3] [--per-night 8] [--method grid] [--algorithm hdbscan]

The archive is four populations of embedding rows (Gaussian clumps in 32 dimensions) and a thin uniform background; its
map is the 2-D UMAP layout (``embedding_layout``), clustered with DBSCAN at an ``eps`` taken from the map itself (the
median distance to the 10th neighbour).  A night brings rows of the known populations and a few that belong to none:
their count of archive rows within r -- r = the archive's median 15th-neighbour distance -- is the novelty column
(0: nothing like it has been seen).  ``--method grid`` answers the questions about the MAP (its 10th-neighbour distances
and its DBSCAN) on a uniform grid (``btsbot_amd.MapIndex``): the same numbers, in time linear in the rows.
``--algorithm hdbscan`` clusters the map with ``btsbot_amd.hdbscan(y, min_cluster_size=25, min_samples=10)`` instead: no
``eps``, clusters of any density, and a membership strength per row.  Everything runs on the device (HDBSCAN's hierarchy
is a host pass of the library over the spanning tree the device built).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6000)
    ap.add_argument("--nights", type=int, default=3)
    ap.add_argument("--per-night", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--method", choices=("tiles", "grid"), default="tiles")
    ap.add_argument("--algorithm", choices=("dbscan", "hdbscan"), default="dbscan")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cluster_map_example: needs a GPU (btsbot_amd has no CPU fallback)")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(args.seed)

    centres = 6.0 * torch.randn((4, 32), generator=gen, device=dev)
    member = torch.arange(args.n, device=dev) % 5                      # population 4: the background
    rows = torch.randn((args.n, 32), generator=gen, device=dev) + centres[member.clamp(max=3)]
    rows = torch.where((member == 4)[:, None], 12.0 * (torch.rand((args.n, 32), generator=gen, device=dev) - 0.5), rows)
    mean = rows.mean(dim=0)
    rows = rows - mean                                                 # centred rows keep the candidate margin small

    y = btsbot_amd.embedding_layout(rows, n_neighbors=15, n_epochs=200, seed=args.seed)
    if args.algorithm == "hdbscan":
        labels, prob = btsbot_amd.hdbscan(y, 25, 10, method=args.method)
        n_clusters = int(labels.max()) + 1
        print(f"{args.n} rows -> map; HDBSCAN(min_cluster_size = 25, min_samples = 10): {n_clusters} clusters, "
              f"{int((labels < 0).sum())} rows of noise, median membership {float(prob[labels >= 0].median()):.2f}")
    else:
        _, d10 = btsbot_amd.knn_graph(y, 11, method=args.method)
        eps = float(d10[:, 10].median())
        labels, core = btsbot_amd.dbscan(y, eps, min_samples=10, method=args.method)
        n_clusters = int(labels.max()) + 1
        print(f"{args.n} rows -> map; DBSCAN(eps = {eps:.3f}, min_samples = 10): {n_clusters} clusters, "
              f"{int(core.sum())} core rows, {int((labels < 0).sum())} rows of noise")
    for c in range(min(n_clusters, 8)):
        inside = labels == c
        share = torch.bincount(member[inside], minlength=5).float() / inside.sum()
        print(f"  cluster {c}: {int(inside.sum()):5d} rows, populations " + " ".join(f"{s:.2f}" for s in share.tolist()))

    index = btsbot_amd.EmbeddingIndex(rows)
    _, d15 = index.query(rows[:: max(1, args.n // 512)], 16, self_offset=-1)
    r = float(d15[:, 15].median())
    print(f"novelty: archive rows within r = {r:.3f} of each new row (0 = nothing like it)")
    for night in range(args.nights):
        known = torch.randn((args.per_night - 2, 32), generator=gen, device=dev) + centres[night % 4]
        new = 9.0 + torch.randn((2, 32), generator=gen, device=dev)    # two rows far from everything
        batch = torch.cat([known, new]) - mean
        counts = index.count_within(batch, r)
        print(f"  night {night}: " + " ".join(f"{c:5d}" for c in counts.tolist()))
        index.add(batch)                                               # tomorrow they are part of the archive


if __name__ == "__main__":
    main()
