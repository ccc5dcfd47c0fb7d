#!/usr/bin/env python
"""Time the radius search (btsbot_knn_radius_*, EmbeddingIndex.radius / count_within) and DBSCAN on one GPU:

    python tools/radius_bench.py [N] [Q] [D] [--maps 100000,1000000]      # default 1,000,000  8,192  528

Rows: 50 Gaussian clusters (centres 4 N(0,1), unit noise), seeded and centred.  r = the median 15th-neighbour distance
of the queries, from ``index.query(k=15)`` in the same run.  HIP events after a warm-up call, seven blocks, the MEDIAN
block.  Prints one JSON line:
  query_k15_ms     index.query(queries, 15): unchanged code, the yardstick
  radius_ms        index.radius(queries, r): both tile passes, the verification, the sort, its two host reads
  count_within_ms  index.count_within(queries, r)
  count_pass_ms    btsbot_knn_radius_count alone (query pack + the counting tile pass)
  torch_ms         the torch form: cdist over query chunks of at most 4 GiB of distances, <= r, nonzero
  *_peak_mib       torch.cuda.max_memory_allocated over the timed calls, above what the inputs hold
  candidates, total   pairs verified in the direct form / pairs returned
  lists_differing  of 256 sampled queries, how many lists differ from the float64 brute force outside the free band
                   (tests/radius_ref.py: a pair within (D + 4) u of r may go either way)
  map_<n>_graph_ms, map_<n>_dbscan_ms   radius_graph(y, eps) and dbscan(y, eps, 10, graph=...) on a 2-D map of n rows
                   (Gaussian clumps; eps = the median 10th-neighbour distance of a sample)
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402
from btsbot_amd import _lib   # noqa: E402

U = 2.0 ** -24


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


def timed_peak(fn, blocks=7):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = timed(fn, blocks)
    return ms, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def clusters(n, d, seed, dev, centres=None):
    gen = torch.Generator(device=dev).manual_seed(seed)
    if centres is None:
        centres = 4.0 * torch.randn((50, d), generator=gen, device=dev)
    rows = torch.empty((n, d), device=dev)
    for a in range(0, n, 1 << 18):                   # in slices: the generator's temporaries stay small
        m = min(1 << 18, n - a)
        pick = torch.randint(0, centres.shape[0], (m,), generator=gen, device=dev)
        rows[a:a + m] = centres[pick] + torch.randn((m, d), generator=gen, device=dev)
    return rows, centres


def torch_form(q, bank, r):
    chunk = max(1, (4 << 30) // (4 * bank.shape[0]))
    out = []
    for a in range(0, q.shape[0], chunk):
        out.append((torch.cdist(q[a:a + chunk], bank) <= r).nonzero())
    return out


def count_pass(index, q, r):
    L = _lib.lib()
    nq, n = q.shape[0], len(index)
    splits = int(L.btsbot_knn_splits(nq, n, index.dim, 1))
    rad = torch.full((nq,), r, device=q.device)
    counts = torch.zeros((nq, splits), dtype=torch.int32, device=q.device)
    need = int(L.btsbot_knn_radius_workspace(nq, index.dim))
    ws = torch.empty(need, dtype=torch.uint8, device=q.device)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def go():
        _lib.check(L.btsbot_knn_radius_count(p(q), nq, p(index._packed), n, index.dim, index._metric_id, p(rad), -1, splits,
                                             None, None, 0, p(counts), p(ws), need, _lib.stream(index.device)), "count")
    return go


def lists_differing(index, q, r, sample=256):
    """float64 on the device: the expansion form decides all pairs but those within 1e-3 of r, which are redone direct"""
    bank = index.bank
    d = bank.shape[1]
    pick = torch.arange(0, q.shape[0], max(1, q.shape[0] // sample), device=q.device)[:sample]
    ip, ii, _ = index.radius(q[pick], r)
    q64 = q[pick].double()
    bb = torch.zeros(bank.shape[0], dtype=torch.float64, device=q.device)
    dot = torch.empty((len(pick), bank.shape[0]), dtype=torch.float64, device=q.device)
    for a in range(0, bank.shape[0], 1 << 17):
        b64 = bank[a:a + (1 << 17)].double()
        bb[a:a + (1 << 17)] = (b64 * b64).sum(1)
        dot[:, a:a + (1 << 17)] = q64 @ b64.T
    dist = ((q64 * q64).sum(1)[:, None] + bb[None, :] - 2 * dot).clamp_(min=0).sqrt_()
    near = ((dist - r).abs() <= 1e-3 * r).nonzero()
    dist[near[:, 0], near[:, 1]] = ((q64[near[:, 0]] - bank[near[:, 1]].double()) ** 2).sum(1).sqrt()
    band = (d + 4) * U
    must_in, must_out = dist * (1 + band) <= r, dist * (1 - band) > r
    got = torch.zeros_like(must_in)
    rows = torch.repeat_interleave(torch.arange(len(pick), device=q.device), ip.diff())
    got[rows, ii] = True
    wrong = (must_in & ~got) | (must_out & got)
    return int(wrong.any(dim=1).sum()), int((~must_in & ~must_out).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=1_000_000)
    ap.add_argument("q", nargs="?", type=int, default=8192)
    ap.add_argument("d", nargs="?", type=int, default=528)
    ap.add_argument("--maps", default="100000,1000000")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("radius_bench: needs a GPU")
    dev = torch.device("cuda:0")
    res = {"N": args.n, "Q": args.q, "D": args.d}

    bank, centres = clusters(args.n, args.d, 1, dev)
    q, _ = clusters(args.q, args.d, 2, dev, centres)
    mean = bank.mean(dim=0)
    bank -= mean
    q -= mean
    index = btsbot_amd.EmbeddingIndex(bank)
    del bank
    _, d15 = index.query(q, 15)
    r = float(d15[:, 14].median())
    res["r"] = r
    stats = {}
    index.radius(q, r, stats=stats)
    res.update(candidates=stats["candidates"], total=stats["total"], error_flag=stats["error_flag"])
    res["query_k15_ms"], res["query_k15_peak_mib"] = timed_peak(lambda: index.query(q, 15))
    res["radius_ms"], res["radius_peak_mib"] = timed_peak(lambda: index.radius(q, r))
    res["count_within_ms"], _ = timed_peak(lambda: index.count_within(q, r))
    res["count_pass_ms"] = timed(count_pass(index, q, r))
    if not args.no_torch:
        res["torch_ms"], res["torch_peak_mib"] = timed_peak(lambda: torch_form(q, index.bank, r), blocks=3)
    res["lists_differing"], res["pairs_in_free_band"] = lists_differing(index, q, r)
    del index
    torch.cuda.empty_cache()

    for n in [int(s) for s in args.maps.split(",") if s]:
        gen = torch.Generator(device=dev).manual_seed(3)
        spots = 40.0 * torch.rand((200, 2), generator=gen, device=dev)
        y = spots[torch.randint(0, 200, (n,), generator=gen, device=dev)] + torch.randn((n, 2), generator=gen, device=dev)
        y -= y.mean(dim=0)
        sample = y[:: max(1, n // 4096)]
        _, d10 = btsbot_amd.EmbeddingIndex(y).query(sample, 11)
        eps = float(d10[:, 10].median())
        st = {}
        graph = btsbot_amd.radius_graph(y, eps, stats=st)
        res[f"map_{n}_eps"] = eps
        res[f"map_{n}_edges"], res[f"map_{n}_candidates"] = st["total"], st["candidates"]
        res[f"map_{n}_graph_ms"], res[f"map_{n}_graph_peak_mib"] = timed_peak(lambda: btsbot_amd.radius_graph(y, eps), blocks=3)
        res[f"map_{n}_dbscan_ms"], _ = timed_peak(lambda: btsbot_amd.dbscan(y, eps, 10, graph=graph[:2]), blocks=3)
        labels, core = btsbot_amd.dbscan(y, eps, 10, graph=graph[:2])
        res[f"map_{n}_clusters"], res[f"map_{n}_noise"] = int(labels.max()) + 1, int((labels < 0).sum())
        del graph, y
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
