#!/usr/bin/env python
"""Time the neighbour questions of a 2-D map on the grid (MapIndex, csrc/grid.hip) and on the tiles (EmbeddingIndex) in the
same run, on one GPU:

    python tools/map_index_bench.py [N ...] [--no-tiles] [--lanes 1,4,8,16,32,64]      # default 100000 1000000

The map: 200 Gaussian clumps in the plane (centres uniform in a 40 x 40 box, unit noise), seeded and centred.  eps = the
median 10th-neighbour distance of a sample of 4,096 rows, from ``MapIndex.query`` in the same run.  HIP events after a
warm-up call, seven blocks, the MEDIAN block.  Prints one JSON line per N:
  build_ms             MapIndex(y): finite flags, bounding box, cells, the stable sort, cell_start, the gathers
  *_graph_ms           radius_graph(y, eps, method=...): index build, count, the sizing read, fill, the ordering sort
  *_count_ms           count_within(y[:8192], eps) on an index built before (grid: the count pass alone, no host read)
  *_knn15_ms           knn_graph(y, 15, method=...)
  *_dbscan_ms          dbscan(y, eps, 10, method=...) end to end (graph, components, labels)
  grid_radius_ms       MapIndex.radius(y, eps) on an index built before
  lanes_<w>_radius_ms  the same with w lanes per query row (the kernel's W; 16 is the library's choice)
  edges, visited, visited_per_edge, pairs   the graph's entries, the pairs whose distance the grid computed (one pass) and N * N
  same_graph, same_labels   the grid's graph / labels equal the tiles' bit for bit (checked at this size, in this run)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402


def timed(fn, blocks=7):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def clumps(n, dev, seed=3):
    gen = torch.Generator(device=dev).manual_seed(seed)
    spots = 40.0 * torch.rand((200, 2), generator=gen, device=dev)
    y = spots[torch.randint(0, 200, (n,), generator=gen, device=dev)] + torch.randn((n, 2), generator=gen, device=dev)
    return y - y.mean(dim=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="*", type=int, default=[100_000, 1_000_000])
    ap.add_argument("--no-tiles", action="store_true")
    ap.add_argument("--lanes", default="1,4,8,16,32,64")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("map_index_bench: needs a GPU")
    dev = torch.device("cuda:0")
    for n in args.n:
        y = clumps(n, dev)
        res = {"N": n, "pairs": n * n}
        mi = btsbot_amd.MapIndex(y)
        res["cells"] = mi.cells
        _, d10 = mi.query(y[:: max(1, n // 4096)], 11)
        eps = float(d10[:, 10].median())
        res["eps"] = eps
        q = y[:8192]
        st = {}
        grid_graph = btsbot_amd.radius_graph(y, eps, method="grid", stats=st)
        res.update(edges=st["total"], visited=st["visited"], visited_per_edge=round(st["visited"] / max(1, st["total"]), 3),
                   error_flag=st["error_flag"])
        res["build_ms"] = timed(lambda: btsbot_amd.MapIndex(y))
        res["grid_radius_ms"] = timed(lambda: mi.radius(y, eps))
        for w in [int(s) for s in args.lanes.split(",") if s]:
            mi._lanes = w
            res[f"lanes_{w}_radius_ms"] = timed(lambda: mi.radius(y, eps))
        mi._lanes = 0
        res["grid_graph_ms"] = timed(lambda: btsbot_amd.radius_graph(y, eps, method="grid"))
        res["grid_count_ms"] = timed(lambda: mi.count_within(q, eps))
        res["grid_knn15_ms"] = timed(lambda: btsbot_amd.knn_graph(y, 15, method="grid"))
        res["grid_dbscan_ms"] = timed(lambda: btsbot_amd.dbscan(y, eps, 10, method="grid"))
        labels, core = btsbot_amd.dbscan(y, eps, 10, method="grid")
        res["clusters"], res["noise"] = int(labels.max()) + 1, int((labels < 0).sum())
        if not args.no_tiles:
            tiles = btsbot_amd.EmbeddingIndex(y)
            tiles_graph = btsbot_amd.radius_graph(y, eps, method="tiles")
            res["same_graph"] = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                b.view(torch.int32) if b.dtype == torch.float32 else b)
                                    for a, b in zip(grid_graph, tiles_graph))
            del tiles_graph
            res["same_counts"] = bool(torch.equal(mi.count_within(q, eps), tiles.count_within(q, eps)))
            res["tiles_graph_ms"] = timed(lambda: btsbot_amd.radius_graph(y, eps, method="tiles"))
            res["tiles_count_ms"] = timed(lambda: tiles.count_within(q, eps))
            res["tiles_knn15_ms"] = timed(lambda: btsbot_amd.knn_graph(y, 15, method="tiles"))
            res["tiles_dbscan_ms"] = timed(lambda: btsbot_amd.dbscan(y, eps, 10, method="tiles"))
            tl, tc = btsbot_amd.dbscan(y, eps, 10, method="tiles")
            res["same_labels"] = bool(torch.equal(tl, labels) and torch.equal(tc, core))
            del tiles
        del grid_graph, mi, y
        torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
