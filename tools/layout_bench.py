#!/usr/bin/env python
"""Time the embedding layout (btsbot_layout_*, btsbot_amd.embedding_layout) on one GPU against the torch-op form of an epoch:

    python tools/layout_bench.py [N] [D] [k] [epochs]      # default 100,000  528  15  200

Rows: 50 Gaussian clusters (centres 4 N(0,1), unit noise), seeded.  HIP events after a warm-up call, seven blocks, the
MEDIAN block reported (three blocks for the whole call, which the neighbour search dominates).  Prints one JSON line:
  knn_ms          knn_graph(emb, k, include_self=True), for scale (tools/neighbors_bench.py measures it properly)
  graph_ms        fuzzy_graph(idx, dist): smooth_knn, the sort, merge, scan and CSR fill, with its allocations
  epoch_ms        optimize_layout over all `epochs` epochs of the schedule, divided by `epochs`
  whole_ms        embedding_layout(emb, n_neighbors=k, n_epochs=epochs) end to end (init="pca": one host read)
  torch_epoch_ms  the same epochs written with torch ops on the same graph in the same run: the firing mask, gathers of the
                  fired slots, index_add_ of the attractive terms and of negative_sample_rate rounds of repulsive terms
                  (torch.randint targets: it is a timing comparator, not the same samples), divided by `epochs`
  edges, firings_per_epoch, gathers_per_epoch
                  CSR slots; the mean number of slots that fire in an epoch; positions gathered at random per epoch,
                  firings * (1 + negative_sample_rate)
  gather_gbps     8 bytes * gathers_per_epoch over epoch_ms: the USEFUL bytes of the random gathers
  line_gbps       the same gathers counted as the 128-byte lines they touch, to set beside the measured HBM rate (about
                  6,300 GB/s) and the L2 rate (about 17,000 GB/s): N positions are 8 N bytes, so up to N = 500,000 the
                  table fits one XCD's 4 MiB L2
  stream_gbps     the bytes an epoch streams in order (CSR slots 8 E, indptr 8 N, positions in and out 16 N) over epoch_ms
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402

BLOCKS = 7
RATE = 5


def timed(fn, blocks=BLOCKS):
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


def fire_mask(g, n):
    r = (g.weights / g.w_max).double()
    return torch.floor(n * r) > torch.floor((n - 1) * r)


def torch_epochs(g, rows, y, n_epochs, a, b, rate=RATE):
    n_v = y.shape[0]
    cols = g.indices.long()
    for n in range(1, n_epochs + 1):
        slot = fire_mask(g, n).nonzero().squeeze(1)
        v, u = rows[slot], cols[slot]
        acc = torch.zeros_like(y)
        diff = y[v] - y[u]
        d2 = (diff * diff).sum(dim=1, keepdim=True)
        coeff = torch.where(d2 > 0, -2.0 * a * b * d2 ** (b - 1.0) / (1.0 + a * d2 ** b), torch.zeros_like(d2))
        acc.index_add_(0, v, 2.0 * (coeff * diff).clamp(-4.0, 4.0))
        for _ in range(rate):
            t = torch.randint(n_v, v.shape, device=y.device)
            diff = y[v] - y[t]
            d2 = (diff * diff).sum(dim=1, keepdim=True)
            term = (2.0 * b / ((0.001 + d2) * (1.0 + a * d2 ** b)) * diff).clamp(-4.0, 4.0)
            acc.index_add_(0, v, torch.where((t != v)[:, None], torch.where(d2 > 0, term, torch.full_like(term, 4.0)),
                                             torch.zeros_like(term)))
        y = y + (1.0 - (n - 1) / n_epochs) * acc
    return y


def main():
    args = [int(x) for x in sys.argv[1:5]]
    n, d, k, epochs = args + [100_000, 528, 15, 200][len(args):]
    if not torch.cuda.is_available():
        sys.exit("layout_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    centres = 4.0 * torch.randn((50, d), generator=gen, device=dev)
    emb = centres[torch.arange(n, device=dev) % 50] + torch.randn((n, d), generator=gen, device=dev)
    a, b = btsbot_amd.find_ab_params(1.0, 0.1)

    knn_ms = timed(lambda: btsbot_amd.knn_graph(emb, k), blocks=3)
    idx, dist = btsbot_amd.knn_graph(emb, k)
    graph_ms = timed(lambda: btsbot_amd.fuzzy_graph(idx, dist))
    g = btsbot_amd.fuzzy_graph(idx, dist)
    y0 = btsbot_amd.embedding_layout(emb, n_neighbors=k, n_epochs=1, knn=(idx, dist), learning_rate=1e-30)
    epochs_ms = timed(lambda: btsbot_amd.optimize_layout(g, y0, epochs, a, b, negative_sample_rate=RATE))
    whole_ms = timed(lambda: btsbot_amd.embedding_layout(emb, n_neighbors=k, n_epochs=epochs), blocks=3)
    rows = torch.repeat_interleave(torch.arange(n, device=dev), g.indptr.diff())
    torch_ms = timed(lambda: torch_epochs(g, rows, y0, epochs, a, b), blocks=3)

    fired = sum(int(fire_mask(g, e).sum()) for e in range(1, epochs + 1)) / epochs
    epoch_ms = epochs_ms / epochs
    gathers = fired * (1 + RATE)
    degree = g.indptr.diff()
    out = dict(n=n, dim=d, k=k, epochs=epochs, negative_sample_rate=RATE, device=torch.cuda.get_device_name(0), blocks=BLOCKS,
               knn_ms=round(knn_ms, 2), graph_ms=round(graph_ms, 3), epoch_ms=round(epoch_ms, 4), epochs_ms=round(epochs_ms, 2),
               whole_ms=round(whole_ms, 1), torch_epoch_ms=round(torch_ms / epochs, 4),
               torch_over_kernel=round(torch_ms / epochs_ms, 1), edges=g.n_edges, max_degree=int(degree.max()),
               mean_degree=round(g.n_edges / n, 2), firings_per_epoch=round(fired), gathers_per_epoch=round(gathers),
               gather_gbps=round(8 * gathers / (epoch_ms * 1e-3) / 1e9, 1),
               line_gbps=round(128 * gathers / (epoch_ms * 1e-3) / 1e9, 1),
               stream_gbps=round((8 * g.n_edges + 24 * n) / (epoch_ms * 1e-3) / 1e9, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
