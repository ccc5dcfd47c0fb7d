#!/usr/bin/env python
"""Time the neighbour ranks (btsbot_knn_rank_*, EmbeddingIndex.rank_of) and the map quality on one GPU:

    python tools/rank_bench.py [N] [Q] [D] [--quality-n 100000] [--no-torch]      # default 1,000,000  8,192  528

Rows: tools/radius_bench.py's set (50 Gaussian clusters, centres 4 N(0,1), unit noise, seeded and centred).  The map is
``embedding_layout(rows, 15)`` of all N rows, laid out once; the Q query rows are every (N / Q)-th row of the bank and
their t = 15 targets are their 15 nearest neighbours ON THE MAP (``MapIndex.query``, the row itself dropped).  HIP events
after a warm-up call, seven blocks, the MEDIAN block.  Prints one JSON line:
  rank_of_ms          index.rank_of(queries, targets): query pack, thresholds, both tile passes, the band verification,
                      its two host reads
  query_k15_ms        index.query(queries, 15): unchanged code, the yardstick
  count_pass_ms       btsbot_knn_radius_count alone at r = the median 15th-neighbour distance (the counting tile pass)
  count_within_ms     the route through the lists for ONE column: index.count_within(queries, dist[:, 7])
  torch_ms            the torch form: cdist over query chunks of at most 4 GiB of distances, compare with each
                      target's distance and sum
  *_peak_mib          torch.cuda.max_memory_allocated over the timed calls, above what the inputs hold
  band_pairs, band_per_threshold   band entries of the call (pairs decided in the direct form), and per (q, c)
  rank_median, rank_p99, rank_max  of the targets' ranks
  ranks_differing     of 256 sampled queries x 15 targets, how many ranks lie outside the float64 interval
  trust_rows_ms       trustworthiness(rows, y, 15, rows=the Q rows) at N
  quality_<n>_*       at n = --quality-n rows (their own layout): trustworthiness of all rows / of 8,192 rows, ms
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402
from radius_bench import clusters, count_pass, timed, timed_peak   # noqa: E402

U = 2.0 ** -24


def map_targets(y, rows, t):
    """int64 [len(rows), t]: the rows' t nearest map neighbours, the row itself dropped"""
    idx = btsbot_amd.MapIndex(y).query(y[rows], t + 1)[0]
    own = idx == rows[:, None]
    pos = torch.where(own.any(dim=1), own.to(torch.int64).argmax(dim=1), torch.full_like(rows, t))
    cols = torch.arange(t, device=y.device)[None, :]
    return torch.gather(idx, 1, cols + (cols >= pos[:, None]).to(torch.int64)).contiguous()


def torch_form(q, bank, targets):
    chunk = max(1, (4 << 30) // (4 * bank.shape[0]))
    out = []
    for a in range(0, q.shape[0], chunk):
        d = torch.cdist(q[a:a + chunk], bank)
        dt = torch.gather(d, 1, targets[a:a + chunk])
        out.append(torch.stack([(d < dt[:, c:c + 1]).sum(dim=1) for c in range(targets.shape[1])], dim=1))
    return torch.cat(out)


def ranks_differing(index, q, targets, rank, sample=256):
    """float64 on the device, expansion form; a pair within the band of the target's distance may go either way"""
    bank = index.bank
    d = bank.shape[1]
    pick = torch.arange(0, q.shape[0], max(1, q.shape[0] // sample), device=q.device)[:sample]
    q64 = q[pick].double()
    dist = torch.empty((len(pick), bank.shape[0]), dtype=torch.float64, device=q.device)
    for a in range(0, bank.shape[0], 1 << 17):
        b64 = bank[a:a + (1 << 17)].double()
        dist[:, a:a + (1 << 17)] = ((q64 * q64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :] - 2 * q64 @ b64.T)
    dist.clamp_(min=0).sqrt_()
    band = (d + 4) * U
    tg, rk = targets[pick], rank[pick]
    wrong = 0
    for c in range(tg.shape[1]):
        dt = torch.gather(dist, 1, tg[:, c:c + 1])
        lo = (dist * (1 + band) < dt * (1 - band)).sum(dim=1)
        hi = (~(dist * (1 - band) > dt * (1 + band))).sum(dim=1) - 1       # (the target itself is in its own band)
        wrong += int(((rk[:, c] < lo) | (rk[:, c] > hi)).sum())
    return wrong


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=1_000_000)
    ap.add_argument("q", nargs="?", type=int, default=8192)
    ap.add_argument("d", nargs="?", type=int, default=528)
    ap.add_argument("--quality-n", type=int, default=100_000)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rank_bench: needs a GPU")
    dev = torch.device("cuda:0")
    t = 15
    res = {"N": args.n, "Q": args.q, "D": args.d, "t": t}

    bank, centres = clusters(args.n, args.d, 1, dev)
    bank -= bank.mean(dim=0)
    index = btsbot_amd.EmbeddingIndex(bank)
    del bank
    y = btsbot_amd.embedding_layout(index.bank, 15)
    rows = torch.arange(0, args.n, max(1, args.n // args.q), device=dev)[:args.q]
    q = index.bank[rows].contiguous()
    targets = map_targets(y, rows, t)
    stats = {}
    rank, dist = index.rank_of(q, targets, stats=stats)
    res.update(band_pairs=stats["band"], band_per_threshold=stats["band"] / max(1, targets.numel()),
               error_flag=stats["error_flag"])
    rk = rank[rank >= 0].double()
    res.update(rank_median=float(rk.median()), rank_p99=float(rk.quantile(0.99)), rank_max=float(rk.max()))
    res["rank_of_ms"], res["rank_of_peak_mib"] = timed_peak(lambda: index.rank_of(q, targets))
    res["query_k15_ms"], res["query_k15_peak_mib"] = timed_peak(lambda: index.query(q, 15))
    _, d15 = index.query(q, 16)
    res["count_pass_ms"] = timed(count_pass(index, q, float(d15[:, 15].median())))
    col = dist[:, 7].contiguous()
    res["count_within_ms"], res["count_within_peak_mib"] = timed_peak(lambda: index.count_within(q, col))
    if not args.no_torch:
        res["torch_ms"], res["torch_peak_mib"] = timed_peak(lambda: torch_form(q, index.bank, targets), blocks=3)
    res["ranks_differing"] = ranks_differing(index, q, targets, rank)
    res["trust_rows_ms"], res["trust_rows_peak_mib"] = timed_peak(
        lambda: btsbot_amd.trustworthiness(index.bank, y, 15, rows=rows), blocks=3)
    res["trust_rows"] = btsbot_amd.trustworthiness(index.bank, y, 15, rows=rows)
    del index, y, q
    torch.cuda.empty_cache()

    n = args.quality_n
    if n:
        emb, _ = clusters(n, args.d, 1, dev, centres)
        emb -= emb.mean(dim=0)
        y = btsbot_amd.embedding_layout(emb, 15)
        rows = torch.arange(0, n, max(1, n // 8192), device=dev)[:8192]
        res[f"quality_{n}_all_ms"], res[f"quality_{n}_all_peak_mib"] = timed_peak(
            lambda: btsbot_amd.trustworthiness(emb, y, 15), blocks=3)
        res[f"quality_{n}_rows_ms"], _ = timed_peak(lambda: btsbot_amd.trustworthiness(emb, y, 15, rows=rows), blocks=3)
        res[f"quality_{n}_trust_all"] = btsbot_amd.trustworthiness(emb, y, 15)
        res[f"quality_{n}_trust_rows"] = btsbot_amd.trustworthiness(emb, y, 15, rows=rows)
        res[f"quality_{n}_continuity_rows"] = btsbot_amd.continuity(emb, y, 15, rows=rows)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
