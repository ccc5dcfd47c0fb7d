#!/usr/bin/env python3
"""Nights of an archive that grows AND forgets, and a novelty fit that follows both without searching the history again.

``nightly_novelty_example.py`` only adds.  Here every row carries the night it arrived (a per-row array of the caller's,
kept aligned through what ``index.remove`` returns), and each night the rows older than ``--keep`` nights leave:

    index.add(rows, groups=source)            # tonight's rows
    kept = index.remove(night_of < oldest)    # a stable compaction; kept = the old row number of every survivor
    night_of = night_of[kept]                 # the caller's per-row arrays follow
    model.update(stats)                       # graph and fit: one pass over the lists, one query for the damaged rows
    model.score(...)                          # against the archive as it now stands

``model.update()`` renumbers every surviving list in one launch (``btsbot_knn_graph_compact``), searches again only the
rows whose list lost an entry, and merges tonight's rows in as before (``btsbot.KnnGraph``).  At the
end the model is checked against one fitted from scratch on the surviving rows: the lists are the same up to rows with two
candidates inside the search's selection band at the k-th place, and the fit is the same bit for bit wherever the lists are.

    python examples/archive_retention_example.py [--archive 20000] [--night 2000] [--nights 5] [--keep 3] [--dim 32] [--k 10]
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
    p = argparse.ArgumentParser(description="A novelty fit that follows index.add and index.remove night by night (MI355X)")
    p.add_argument("--archive", type=int, default=20000, help="rows at the start, spread over the --keep nights before")
    p.add_argument("--night", type=int, default=2000)
    p.add_argument("--nights", type=int, default=5)
    p.add_argument("--keep", type=int, default=3, help="a row leaves when it is older than this many nights")
    p.add_argument("--dim", type=int, default=32)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--epochs", type=int, default=4, help="rows per source")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("archive_retention_example: needs a GPU (btsbot_amd has no CPU fallback)")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(31)
    centres = 4.0 * torch.randn((20, args.dim), generator=gen, device=dev)

    rows, source = draw(args.archive, centres, gen, args.epochs, 0)
    next_source = int(source[-1]) + 1
    # the starting archive arrived over the nights -keep .. -1, oldest first
    night_of = (torch.arange(args.archive, device=dev) * args.keep // args.archive) - args.keep
    index = btsbot.EmbeddingIndex(rows, groups=source)
    model = btsbot.NoveltyModel(index, args.k, keep_graph=True)            # group_mode="exclude": no row of the own source
    print(f"archive: {len(index)} rows of {next_source} sources, width {index.dim}; LOF median "
          f"{float(model.lof.nanmedian()):.3f}, 99th percentile {model.threshold(0.01):.3f}")

    for night in range(args.nights):
        rows, source = draw(args.night, centres, gen, args.epochs, next_source)
        next_source = int(source[-1]) + 1
        flag = model.threshold(0.01)
        score = model.score(rows, query_groups=source, exclude_same_group=True)     # against the archive as it stands
        index.add(rows, groups=source)
        night_of = torch.cat([night_of, torch.full((args.night,), night, device=dev)])
        first_id = int(index.ids[0])
        kept = index.remove(night_of < night - args.keep + 1)
        night_of = night_of[kept]
        stats = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.update(stats)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        print(f"night {night + 1}: {args.night} new rows, {int((score > flag).sum())} above the archive's 99th percentile; "
              f"{stats.get('removed', 0)} rows left (ids {first_id} .. {int(index.ids[0]) - 1}), {len(index)} stay; update() "
              f"{ms:.1f} ms: {stats.get('damaged', 0)} lists searched again, {stats['offers']} offers to {stats['touched']} "
              f"old rows")
        assert len(model) == len(index) == night_of.shape[0]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fresh = btsbot.NoveltyModel(btsbot.EmbeddingIndex(index.bank.clone(), groups=index.groups.clone()), args.k)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    idx, dist = index.query(index.bank, args.k, self_offset=0, query_groups=index.groups, exclude_same_group=True)
    same = ((idx == model.graph.idx) & (dist == model.graph.dist)).all(dim=1)
    # a row's fit reads its neighbours' lists too: compare where the row and all its neighbours have the same lists
    settled = same & same[model.graph.idx.clamp(min=0)].all(dim=1)
    settled &= settled[model.graph.idx.clamp(min=0)].all(dim=1)
    equal = torch.equal(model.lof[settled].view(torch.int64), fresh.lof[settled].view(torch.int64))
    worst = float(((model.lof - fresh.lof).abs() / fresh.lof).nan_to_num(0.0).max())
    print(f"from scratch on the {len(index)} surviving rows: {ms:.1f} ms; {int((~same).sum())} lists differ from the rebuilt "
          f"graph (two candidates inside the selection band); LOF bit-identical on the {int(settled.sum())} settled rows: "
          f"{equal}; largest relative difference anywhere {worst:.2e}")
    if not equal:
        sys.exit("archive_retention_example: the updated fit and the fit from scratch disagree")


if __name__ == "__main__":
    main()
