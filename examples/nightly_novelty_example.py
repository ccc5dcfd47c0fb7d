#!/usr/bin/env python3
"""Three nights of an archive that grows, and a novelty fit that follows it without searching the history again.

An archive of embedding rows (synthetic here: Gaussian clusters, every ``--epochs`` consecutive rows one source) carries a
``btsbot.NoveltyModel(index, k, keep_graph=True)``: the model keeps the neighbour graph its fit is computed on.  Each
night the new rows are first scored against the archive as it stands -- with their own source left out --, then appended
with ``index.add(rows, groups=...)``, and ``model.update()`` brings graph and fit to the rows the index holds now: the new
rows' lists by one ``query``, the old rows' lists by one ``radius`` of the old rows against the NEW ones and a merge kernel
(``btsbot.KnnGraph``).  A few rows of the last night lie far from every cluster.  At the end the
model is checked against one fitted from scratch on the same index: the lists are the same up to rows with two candidates
inside the search's selection band at the k-th place, the fit is the same bit for bit wherever the lists are, and the kept
graph serves ``local_outlier_factor(None, k, knn=...)`` as it is.

    python examples/nightly_novelty_example.py [--archive 20000] [--night 2000] [--dim 32] [--k 10] [--epochs 4]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd as btsbot  # noqa: E402


def draw(n, centres, gen, epochs, first_source):
    """n rows around random centres, ``epochs`` consecutive rows per source (near-copies), and their source ids"""
    dev = centres.device
    n_src = -(-n // epochs)
    pick = torch.randint(0, centres.shape[0], (n_src,), generator=gen, device=dev)
    base = centres[pick] + torch.randn((n_src, centres.shape[1]), generator=gen, device=dev)
    rows = base.repeat_interleave(epochs, dim=0)[:n]
    rows = rows + 0.01 * torch.randn(rows.shape, generator=gen, device=dev)
    source = first_source + torch.arange(n_src, device=dev).repeat_interleave(epochs)[:n]
    return rows, source


def main():
    p = argparse.ArgumentParser(description="A novelty fit that follows index.add night by night (MI355X)")
    p.add_argument("--archive", type=int, default=20000)
    p.add_argument("--night", type=int, default=2000)
    p.add_argument("--dim", type=int, default=32)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--epochs", type=int, default=4, help="rows per source")
    p.add_argument("--odd", type=int, default=3, help="rows of the last night far from every cluster")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nightly_novelty_example: needs a GPU (btsbot_amd has no CPU fallback)")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(31)
    centres = 4.0 * torch.randn((20, args.dim), generator=gen, device=dev)

    rows, source = draw(args.archive, centres, gen, args.epochs, 0)
    index = btsbot.EmbeddingIndex(rows, groups=source)
    model = btsbot.NoveltyModel(index, args.k, keep_graph=True)            # group_mode="exclude": no row of the own source
    print(f"archive: {len(index)} rows of {int(source[-1]) + 1} sources, width {index.dim}; LOF median "
          f"{float(model.lof.nanmedian()):.3f}, 99th percentile {model.threshold(0.01):.3f}")

    for night in range(3):
        rows, source = draw(args.night, centres, gen, args.epochs, int(index.groups.max()) + 1)
        if night == 2:
            rows[:args.odd] = 40.0 * torch.randn((args.odd, args.dim), generator=gen, device=dev)
        flag = model.threshold(0.01)
        score = model.score(rows, query_groups=source, exclude_same_group=True)     # against the archive as it stands
        index.add(rows, groups=source)
        stats = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.update(stats)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        print(f"night {night + 1}: {args.night} new rows, {int((score > flag).sum())} above the archive's 99th percentile "
              f"(largest LOF {float(score.max()):.2f}); update() {ms:.1f} ms: {stats['offers']} offers to {stats['touched']} "
              f"old rows, {stats['changed']} lists changed, {stats['candidates']} pairs verified")

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fresh = btsbot.NoveltyModel(index, args.k)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    idx, dist = index.query(index.bank, args.k, self_offset=0, query_groups=index.groups, exclude_same_group=True)
    same = ((idx == model.graph.idx) & (dist == model.graph.dist)).all(dim=1)
    # a row's fit reads its neighbours' lists too: compare where the row and all its neighbours have the same lists
    settled = same & same[model.graph.idx.clamp(min=0)].all(dim=1)
    settled &= settled[model.graph.idx.clamp(min=0)].all(dim=1)
    equal = torch.equal(model.lof[settled].view(torch.int64), fresh.lof[settled].view(torch.int64))
    worst = float(((model.lof - fresh.lof).abs() / fresh.lof).nan_to_num(0.0).max())
    print(f"from scratch: {ms:.1f} ms for {len(index)} rows; {int((~same).sum())} lists differ from the rebuilt graph (two "
          f"candidates inside the selection band); LOF bit-identical on the {int(settled.sum())} settled rows: {equal}; "
          f"largest relative difference anywhere {worst:.2e}")
    again = btsbot.local_outlier_factor(None, args.k, knn=(model.graph.idx, model.graph.dist))
    kept = torch.equal(again.view(torch.int64), model.lof.view(torch.int64))
    print(f"local_outlier_factor(None, k, knn=(graph.idx, graph.dist)) equals the model's fit: {kept}")
    if not (equal and kept):
        sys.exit("nightly_novelty_example: the updated fit and the fit from scratch disagree")


if __name__ == "__main__":
    main()
