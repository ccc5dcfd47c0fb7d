#!/usr/bin/env python
"""Time HDBSCAN (mutual_reachability_mst, ClusterTree, hdbscan) on one GPU:

    python tools/hdbscan_bench.py [N] [D] [min_cluster_size] [min_samples] [--search-k K] [--sklearn-n M] [--map-n P]
                                                                           # default 100,000  528  10  10

Rows: tools/radius_bench.py's set (50 Gaussian clusters, centres 4 N(0,1), unit noise, seeded), centred.  The 2-D map is
a set of the same kind in the plane (spread 12), P rows.  One warm-up at a sixteenth of the size, then ONE timed run of each
(a run is seconds long; the round counts and the unresolved rows do not vary between runs).  Prints one JSON line:
  tiles / grid          for the tile path at [N, D] and for the grid at [P, 2], each:
    rounds              Boruvka rounds
    components          at the start of each round
    unresolved          rows sent to the radius tier, per round
    radius_total        entries of their radius lists, per round
    ms_search ...       per round: the grouped k-nearest search, the offer kernel (with the host read of the unresolved
    ms_merge            rows), the radius tier with its offer, reduce / hook / relabel (with the read of the edge cursor);
                        the device is synchronised around each step for these, and only for these
    mst_ms              mutual_reachability_mst end to end, untimed steps (core distances included)
    tree_ms             the host pass: ClusterTree(mst).labels(min_cluster_size), copy of the edges included
    hdbscan_ms          hdbscan(...) end to end
  sklearn               scikit-learn's HDBSCAN on the host on the first M rows of each set (0 = skipped), in the same
                        run: seconds, and whether its partition equals this one's on those rows
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402
from radius_bench import clusters   # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def one(rows, method, mcs, ms, search_k):
    btsbot_amd.hdbscan(rows[:max(len(rows) // 16, 4 * ms + 8)], mcs, ms, method=method, search_k=search_k)   # warm-up
    stats = {"time": True}
    btsbot_amd.mutual_reachability_mst(rows, ms, method=method, search_k=search_k, stats=stats)
    stats.pop("time")
    mst, mst_ms = wall(lambda: btsbot_amd.mutual_reachability_mst(rows, ms, method=method, search_k=search_k))
    _, tree_ms = wall(lambda: btsbot_amd.ClusterTree(mst).labels(mcs))
    (labels, _prob), all_ms = wall(lambda: btsbot_amd.hdbscan(rows, mcs, ms, method=method, search_k=search_k))
    out = {k: ([round(x, 3) for x in v] if k.startswith("ms_") else v) for k, v in stats.items()}
    out.update(n=len(rows), d=int(rows.shape[1]), mst_ms=round(mst_ms, 2), tree_ms=round(tree_ms, 2),
               hdbscan_ms=round(all_ms, 2), clusters=int(labels.max()) + 1, noise=int((labels < 0).sum()))
    return out


def same_partition(a, b):
    if not torch.equal(a < 0, b < 0):
        return False
    pairs = torch.unique(torch.stack([a, b], 1), dim=0)
    return len(pairs) == len(pairs[:, 0].unique()) == len(pairs[:, 1].unique())


def against_sklearn(rows, m, method, mcs, ms):
    from sklearn.cluster import HDBSCAN
    sub = rows[:m]
    t = time.perf_counter()
    sk = HDBSCAN(min_cluster_size=mcs, min_samples=ms).fit(sub.double().cpu().numpy())
    secs = time.perf_counter() - t
    (labels, _), ours = wall(lambda: btsbot_amd.hdbscan(sub, mcs, ms, method=method))
    return dict(n=int(m), d=int(rows.shape[1]), sklearn_s=round(secs, 2), hdbscan_ms=round(ours, 2),
                same_partition=same_partition(labels.cpu(), torch.from_numpy(sk.labels_).long()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=100_000)
    ap.add_argument("d", nargs="?", type=int, default=528)
    ap.add_argument("min_cluster_size", nargs="?", type=int, default=10)
    ap.add_argument("min_samples", nargs="?", type=int, default=10)
    ap.add_argument("--search-k", type=int, default=8)
    ap.add_argument("--sklearn-n", type=int, default=20_000, help="rows scikit-learn clusters on the host (0: skip)")
    ap.add_argument("--map-n", type=int, default=None, help="rows of the 2-D map (default N; 0: skip the grid)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hdbscan_bench: needs a GPU")
    dev = torch.device("cuda:0")
    mcs, ms = args.min_cluster_size, args.min_samples
    out = dict(min_cluster_size=mcs, min_samples=ms, search_k=args.search_k)
    sets = {}
    if args.n:
        rows, _ = clusters(args.n, args.d, 1, dev)
        sets["tiles"] = rows - rows.mean(dim=0)
    map_n = args.n if args.map_n is None else args.map_n
    if map_n:
        gen = torch.Generator(device=dev).manual_seed(2)
        centres = 12.0 * torch.randn((50, 2), generator=gen, device=dev)
        sets["grid"] = clusters(map_n, 2, 3, dev, centres)[0]
    for method, rows in sets.items():
        out[method] = one(rows, method, mcs, ms, args.search_k)
    if args.sklearn_n:
        out["sklearn"] = {m: against_sklearn(rows, min(args.sklearn_n, len(rows)), m, mcs, ms) for m, rows in sets.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
