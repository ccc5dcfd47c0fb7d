#!/usr/bin/env python
"""Time KnnGraph.update (btsbot_amd/graph.py, btsbot_knn_graph_merge) against the rebuild on one GPU:

    python tools/knn_graph_bench.py [N] [Q] [D] [k] [--rebuild-blocks 7]      # default 1,000,000  8,192  528  20

Rows: tools/radius_bench.py's set (50 Gaussian clusters, centres 4 N(0,1), unit noise, seeded and centred), N + Q of them;
the graph is built on the first N, the last Q are added.  HIP events after a warm-up call, seven blocks, the MEDIAN block
(``--rebuild-blocks``: fewer blocks for the three searches of all rows among all rows, which take seconds each).  Before
every block of an update or a merge the graph's first N rows are put back (not timed).  Prints one JSON line:
  update_ms           KnnGraph.update() end to end (stats=None)
  forward_ms          its first part: index.query(new, k, self_offset=N), the new rows' lists
  reverse_ms          its second part: the temporary index of the new rows and radius(old rows, r, sort="distance")
  merge_ms            its third part, btsbot_knn_graph_merge alone: every old row visited, a row without offers leaves
                      after two indptr reads
  merge_compact_ms    the same kernel on the touched rows only (rows=), plus compact_ms, the torch ops that list them
  torch_merge_ms      the merge as torch ops over the touched rows (concatenate, stable sort, gather, scatter)
  torch_equals_kernel whether both merges give the same lists, bit for bit
  rebuild_ms          KnnGraph.rebuild(): index.query(bank, k, self_offset=0) over all N + Q rows, the same run
  update_over_rebuild update_ms / rebuild_ms
  model_update_ms     NoveltyModel(keep_graph=True).update(): the graph's update and btsbot_lof_fit over all rows
  model_refit_ms      NoveltyModel.refit() of the same model: the rebuild and the fit
  offers, touched, changed, candidates      the update's stats
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402
from btsbot_amd import novelty   # noqa: E402
from radius_bench import clusters, timed   # noqa: E402


def timed_after(reset, fn, blocks=7):
    """``timed`` with ``reset()`` before every call, outside the events"""
    reset()
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def torch_merge(idx, dist, indptr, off_idx, off_dist, rows, k):
    """The plain merge over ``rows`` as torch ops: a row's list and its first k offers side by side, one stable sort by
    dist (the old entries stand first, so they win a tie), the first k columns written back."""
    cnt = indptr.diff()[rows].clamp(max=k)
    col = torch.arange(k, device=idx.device)
    has = col[None, :] < cnt[:, None]
    src = torch.where(has, indptr[rows][:, None] + col[None, :], torch.zeros_like(has, dtype=torch.int64))
    oi = torch.where(has, off_idx[src], torch.full_like(src, -1))
    od = torch.where(has, off_dist[src], torch.full_like(src, float("inf"), dtype=torch.float32))
    ci, cd = torch.cat([idx[rows], oi], dim=1), torch.cat([dist[rows], od], dim=1)
    order = torch.sort(cd, dim=1, stable=True).indices[:, :k]
    idx[rows] = ci.gather(1, order)
    dist[rows] = cd.gather(1, order)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=1_000_000)
    ap.add_argument("q", nargs="?", type=int, default=8192)
    ap.add_argument("d", nargs="?", type=int, default=528)
    ap.add_argument("k", nargs="?", type=int, default=20)
    ap.add_argument("--rebuild-blocks", type=int, default=7, help="blocks for the searches of all rows among all rows")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_graph_bench: needs a GPU")
    dev = torch.device("cuda:0")
    n, nq, k = args.n, args.q, args.k
    res = {"N": n, "Q": nq, "D": args.d, "k": k, "rebuild_blocks": args.rebuild_blocks}

    rows, _ = clusters(n + nq, args.d, 1, dev)
    rows -= rows.mean(dim=0)
    index = btsbot_amd.EmbeddingIndex(rows[:n])
    g = btsbot_amd.KnnGraph(index, k)
    index.add(rows[n:])
    del rows
    idx0, dist0 = g.idx.clone(), g.dist.clone()
    g._reserve(n + nq)                                   # (the one move of the storage happens outside the blocks)

    def reset():
        g._n = n
        g._idx[:n].copy_(idx0)
        g._dist[:n].copy_(dist0)

    stats = {}
    reset()
    g.update(stats)
    res.update(stats)
    res["update_ms"] = timed_after(reset, g.update)
    res["forward_ms"] = timed(lambda: index.query(index.bank[n:], k, self_offset=n))
    reset()
    res["reverse_ms"] = timed(lambda: g._offers(n, n + nq))
    indptr, off_idx, off_dist = g._offers(n, n + nq)
    res["merge_ms"] = timed_after(reset, lambda: g._merge(n, indptr, off_idx, off_dist))
    kernel_i, kernel_d = g._idx[:n].clone(), g._dist[:n].clone()
    res["compact_ms"] = timed(lambda: (indptr.diff() > 0).nonzero().view(-1))
    touched = (indptr.diff() > 0).nonzero().view(-1)
    res["merge_compact_ms"] = timed_after(reset, lambda: g._merge(n, indptr, off_idx, off_dist, rows=touched))
    same_compact = torch.equal(g._idx[:n], kernel_i) and torch.equal(g._dist[:n].view(torch.int32), kernel_d.view(torch.int32))
    res["torch_merge_ms"] = timed_after(reset, lambda: torch_merge(g._idx, g._dist, indptr, off_idx, off_dist, touched, k))
    res["torch_equals_kernel"] = bool(same_compact and torch.equal(g._idx[:n], kernel_i)
                                      and torch.equal(g._dist[:n].view(torch.int32), kernel_d.view(torch.int32)))
    res["torch_over_kernel"] = res["torch_merge_ms"] / res["merge_ms"]
    del kernel_i, kernel_d, indptr, off_idx, off_dist, touched

    model = btsbot_amd.NoveltyModel.__new__(btsbot_amd.NoveltyModel)      # the graph above, without another search
    model.index, model.n_neighbors, model.metric, model.group_mode, model.device, model.graph = index, k, "euclidean", \
        "exclude", dev, g
    res["model_update_ms"] = timed_after(reset, model.update)
    res["fit_ms"] = timed(lambda: novelty._fit(g.idx, g.dist))
    res["rebuild_ms"] = timed(g.rebuild, args.rebuild_blocks)
    res["model_refit_ms"] = timed(model.refit, args.rebuild_blocks)
    res["update_over_rebuild"] = res["update_ms"] / res["rebuild_ms"]
    res["model_update_over_refit"] = res["model_update_ms"] / res["model_refit_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
