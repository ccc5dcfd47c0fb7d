#!/usr/bin/env python
"""Time EmbeddingIndex.remove and the KnnGraph.update that follows it (btsbot_amd/graph.py, btsbot_knn_graph_compact)
against the rebuild on one GPU:

    python tools/knn_graph_remove_bench.py [N] [Q] [D] [k] [f] [--order random|oldest] [--blocks 7] [--rebuild-blocks 3]
                                                                            # default 1,000,000  0  528  20  0.01  random

Rows: tools/knn_graph_bench.py's set (50 Gaussian clusters, centres 4 N(0,1), unit noise, seeded and centred), N + Q of
them; the graph is built on the first N, a share f of these is removed (uniformly at random, or the oldest), and the last Q
are added in the same update.  HIP events after a warm-up call, the MEDIAN block.  Before every block the index and the
graph are put back (not timed): both compact out of place, so the arrays from before are still whole.  Prints one JSON line:
  remove_ms           index.remove(mask): the survivor scan, the gathers of rows / records / ids, the swap
  update_ms           KnnGraph.update() end to end after remove (and add), stats=None
  compact_ms          its first part, btsbot_knn_graph_compact alone: every list renumbered, the damaged rows marked
  requery_ms          its last part: index.query(bank[rows], k, self_rows=rows) for the damaged rows
  grow_ms             with Q > 0, the add half: the new rows' lists, the reverse radius search, the merge
  torch_compact_ms    the compaction as torch ops on the same lists (gather, mask, stable sort of the mask, gather)
  torch_equals_kernel whether both give the same lists and the same damaged rows, bit for bit
  rebuild_ms          KnnGraph.rebuild() on the index after the removal, the same run
  scratch_ms          the only route without remove: EmbeddingIndex(bank[keep]) and KnnGraph(index, k), the same run
  model_update_ms     NoveltyModel(keep_graph=True).update(): the graph's update and btsbot_lof_fit over all rows
  damaged, damaged_share, uniform_share       rows searched again, their share of the survivors, and 1 - (1 - f)^k
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402
from btsbot_amd import _lib   # noqa: E402
from btsbot_amd._lib import ptr, stream   # noqa: E402
from knn_graph_bench import timed_after   # noqa: E402
from radius_bench import clusters, timed   # noqa: E402


def kernel_compact(idx, dist, new_of_old, s, k):
    n = idx.shape[0]
    out_i = torch.empty((s, k), dtype=torch.int64, device=idx.device)
    out_d = torch.empty((s, k), dtype=torch.float32, device=idx.device)
    damaged = torch.empty(s, dtype=torch.uint8, device=idx.device)
    _lib.check(_lib.lib().btsbot_knn_graph_compact(ptr(idx), ptr(dist), k, k, n, ptr(new_of_old), ptr(out_i), ptr(out_d), k, s,
                                                   0, ptr(damaged), None, stream(idx.device)), "btsbot_knn_graph_compact")
    return out_i, out_d, damaged


def torch_compact(idx, dist, new_of_old, kept, k):
    """The same lists by torch ops: the survivors' rows gathered, every entry mapped, the surviving entries moved to the
    front by a stable sort of the mask, the tail filled."""
    li, ld = idx[kept], dist[kept]
    mapped = torch.where(li >= 0, new_of_old[li.clamp(min=0)], torch.full_like(li, -1))
    lives = mapped >= 0
    order = torch.sort((~lives).to(torch.uint8), dim=1, stable=True).indices
    lives = lives.gather(1, order)
    out_i = torch.where(lives, mapped.gather(1, order), torch.full_like(li, -1))
    out_d = torch.where(lives, ld.gather(1, order), torch.full_like(ld, float("inf")))
    nan = torch.isnan(ld[:, 0])
    out_i, out_d = torch.where(nan[:, None], li, out_i), torch.where(nan[:, None], ld, out_d)
    damaged = ((li >= 0) & (mapped < 0)).any(dim=1) & (li[:, k - 1] >= 0) & ~nan
    return out_i, out_d, damaged.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=1_000_000)
    ap.add_argument("q", nargs="?", type=int, default=0)
    ap.add_argument("d", nargs="?", type=int, default=528)
    ap.add_argument("k", nargs="?", type=int, default=20)
    ap.add_argument("f", nargs="?", type=float, default=0.01)
    ap.add_argument("--order", choices=("random", "oldest"), default="random")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--rebuild-blocks", type=int, default=3, help="blocks for the searches of all rows among all rows")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_graph_remove_bench: needs a GPU")
    dev = torch.device("cuda:0")
    n, nq, k, f = args.n, args.q, args.k, args.f
    res = {"N": n, "Q": nq, "D": args.d, "k": k, "f": f, "order": args.order, "blocks": args.blocks,
           "rebuild_blocks": args.rebuild_blocks}

    rows, _ = clusters(n + nq, args.d, 1, dev)
    rows -= rows.mean(dim=0)
    new_rows = rows[n:].clone()
    index = btsbot_amd.EmbeddingIndex(rows[:n])
    del rows
    g = btsbot_amd.KnnGraph(index, k)
    n_gone = int(round(f * n))
    if args.order == "oldest":
        gone = torch.arange(n, device=dev) < n_gone
    else:
        gone = torch.zeros(n, dtype=torch.bool, device=dev)
        gone[torch.randperm(n, generator=torch.Generator(device=dev).manual_seed(2), device=dev)[:n_gone]] = True
    s = n - n_gone
    whole = (index._bank, index._packed, index._ids, index._n, index._cap, index._next_id, index.generation)
    graph = (g._idx, g._dist, g._n, g._ids, g._generation)

    def put_back():
        index._bank, index._packed, index._ids, index._n, index._cap, index._next_id, index.generation = whole
        g._idx, g._dist, g._n, g._ids, g._generation = graph

    def removed():
        put_back()
        index.remove(gone)
        if nq:
            index.add(new_rows)

    res["remove_ms"] = timed_after(put_back, lambda: index.remove(gone), args.blocks)
    stats = {}
    removed()
    g.update(stats)
    res.update(stats)
    res["damaged_share"] = stats["damaged"] / max(s, 1)
    res["uniform_share"] = 1.0 - (1.0 - f) ** k
    res["update_ms"] = timed_after(removed, g.update, args.blocks)
    updated = (g.idx.clone(), g.dist.clone())

    # the parts, on the state update() meets
    removed()
    idx0, dist0 = graph[0][:n], graph[1][:n]
    kept = (~gone).nonzero().view(-1)
    new_of_old = torch.where(gone, torch.full((n,), -1, dtype=torch.int64, device=dev),
                             torch.cumsum(~gone, 0, dtype=torch.int64) - 1)
    res["compact_ms"] = timed(lambda: kernel_compact(idx0, dist0, new_of_old, s, k), args.blocks)
    res["torch_compact_ms"] = timed(lambda: torch_compact(idx0, dist0, new_of_old, kept, k), args.blocks)
    a, b = kernel_compact(idx0, dist0, new_of_old, s, k), torch_compact(idx0, dist0, new_of_old, kept, k)
    res["torch_equals_kernel"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
                                      and torch.equal(a[2], b[2]))
    res["torch_over_kernel"] = res["torch_compact_ms"] / res["compact_ms"]
    damaged = a[2].nonzero().view(-1)
    del a, b
    if damaged.numel():
        res["requery_ms"] = timed(lambda: index.query(index.bank[damaged], k, self_rows=damaged), args.blocks)
    if nq:
        g._idx = torch.empty((s + nq, k), dtype=torch.int64, device=dev)
        g._dist = torch.empty((s + nq, k), dtype=torch.float32, device=dev)
        lists = kernel_compact(idx0, dist0, new_of_old, s, k)

        def compacted():
            g._idx[:s].copy_(lists[0])
            g._dist[:s].copy_(lists[1])
        res["grow_ms"] = timed_after(compacted, lambda: g._grow(s, s + nq, None, lists[2]), args.blocks)
        del lists

    model = btsbot_amd.NoveltyModel.__new__(btsbot_amd.NoveltyModel)      # the graph above, without another search
    model.index, model.n_neighbors, model.metric, model.group_mode, model.device, model.graph = index, k, "euclidean", \
        "exclude", dev, g
    res["model_update_ms"] = timed_after(removed, model.update, args.blocks)

    removed()
    g.update()
    res["update_equals_first"] = bool(torch.equal(g.idx, updated[0]) and torch.equal(g.dist.view(torch.int32),
                                                                                  updated[1].view(torch.int32)))
    res["rebuild_ms"] = timed(g.rebuild, args.rebuild_blocks)
    res["lists_differing_from_rebuild"] = int(((g.idx != updated[0]) | (g.dist != updated[1])).any(dim=1).sum())
    bank = whole[0][:n]

    def scratch():
        btsbot_amd.KnnGraph(btsbot_amd.EmbeddingIndex(torch.cat([bank[kept], new_rows]) if nq else bank[kept]), k)
    res["scratch_ms"] = timed(scratch, args.rebuild_blocks)
    res["update_over_rebuild"] = res["update_ms"] / res["rebuild_ms"]
    res["remove_update_over_scratch"] = (res["remove_ms"] + res["update_ms"]) / res["scratch_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
