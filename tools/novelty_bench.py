#!/usr/bin/env python
"""Time the local outlier factor (btsbot_lof_fit / btsbot_lof_score, NoveltyModel) on one GPU:

    python tools/novelty_bench.py [N] [Q] [D] [k] [--no-end-to-end]      # default 1,000,000  8,192  528  20

Rows: tools/radius_bench.py's set (50 Gaussian clusters, centres 4 N(0,1), unit noise, seeded and centred); the Q new rows
are every (N / Q)-th bank row plus N(0, 0.5).  HIP events after a warm-up call, seven blocks, the MEDIAN block.  Prints
one JSON line:
  fit_ms              btsbot_lof_fit alone on the bank's graph [N, k]: kdist, lrd and lof, three launches
  score_ms            btsbot_lof_score alone on the new rows' lists [Q, k]: one launch
  torch_fit_ms        the same formulas as torch ops (gather, maximum, mean) on the same graph in the same run
  torch_score_ms      ... and for the new rows
  fit_gbs             bytes the fit must move at least (the graph read three times, 16 N k gathered bytes counted as
                      such, the outputs) per second
  model_ms            NoveltyModel(index, k) end to end: the neighbour search of all rows among all rows, then the fit
  score_call_ms       model.score(queries) end to end: index.query, then the launch
  query_ms            index.query(queries, k) alone, the yardstick
  lanes               lanes per row of this k in this build (BTSBOT_AMD_LIB names another build: tools/build_variant.sh
                      lof64 -DBTSBOT_LOF_LANES=64 lof.hip is the one-wave-per-row form)
  torch_vs_kernel_*   the largest relative difference of the torch form's lof (its sums run in another order)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402
from btsbot_amd import _lib, novelty   # noqa: E402
from radius_bench import clusters, timed   # noqa: E402


def torch_fit(idx, dist):
    """complete rows only (the bench's graphs have no tail)"""
    d = dist.double()
    kdist = d[:, -1].contiguous()
    lrd = 1.0 / (torch.maximum(d, kdist[idx]).mean(dim=1) + 1e-10)
    return kdist, lrd, (lrd[idx] / lrd[:, None]).mean(dim=1)


def torch_score(idx, dist, kdist, lrd):
    own = 1.0 / (torch.maximum(dist.double(), kdist[idx]).mean(dim=1) + 1e-10)
    return own, (lrd[idx] / own[:, None]).mean(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=1_000_000)
    ap.add_argument("q", nargs="?", type=int, default=8192)
    ap.add_argument("d", nargs="?", type=int, default=528)
    ap.add_argument("k", nargs="?", type=int, default=20)
    ap.add_argument("--no-end-to-end", action="store_true", help="skip model_ms (eight neighbour searches of all rows)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("novelty_bench: needs a GPU")
    dev = torch.device("cuda:0")
    n, nq, k = args.n, args.q, args.k
    forced = "lof64" in os.path.basename(_lib.LIB_PATH)
    res = {"N": n, "Q": nq, "D": args.d, "k": k, "library": os.path.basename(_lib.LIB_PATH),
           "lanes": 64 if forced else 16 if k <= 16 else 32 if k <= 32 else 64}

    bank, _ = clusters(n, args.d, 1, dev)
    bank -= bank.mean(dim=0)
    index = btsbot_amd.EmbeddingIndex(bank)
    del bank
    rows = torch.arange(0, n, max(1, n // nq), device=dev)[:nq]
    gen = torch.Generator(device=dev).manual_seed(2)
    q = index.bank[rows] + 0.5 * torch.randn((len(rows), args.d), generator=gen, device=dev)

    idx, dist = index.query(index.bank, k, self_offset=0)
    qi, qd = index.query(q, k)
    kdist, lrd, lof = novelty._fit(idx, dist)
    res["rows_with_a_tail"] = int((idx < 0).any(dim=1).sum()) + int((qi < 0).any(dim=1).sum())
    res["fit_ms"] = timed(lambda: novelty._fit(idx, dist))
    res["score_ms"] = timed(lambda: novelty._score(qi, qd, kdist, lrd))
    res["fit_gbs"] = (3 * 12 * n * k + 16 * n * k + 5 * 8 * n) / res["fit_ms"] / 1e6
    res["torch_fit_ms"] = timed(lambda: torch_fit(idx, dist))
    res["torch_score_ms"] = timed(lambda: torch_score(qi, qd, kdist, lrd))
    res["torch_over_kernel_fit"] = res["torch_fit_ms"] / res["fit_ms"]
    res["torch_over_kernel_score"] = res["torch_score_ms"] / res["score_ms"]
    t_lof = torch_fit(idx, dist)[2]
    res["torch_vs_kernel_fit"] = float(((t_lof - lof).abs() / lof).max())
    s_lof = novelty._score(qi, qd, kdist, lrd)[1]
    res["torch_vs_kernel_score"] = float(((torch_score(qi, qd, kdist, lrd)[1] - s_lof).abs() / s_lof).max())
    res["lof_median"], res["lof_max"] = float(lof.median()), float(lof.max())
    res["score_median"], res["score_max"] = float(s_lof.median()), float(s_lof.max())
    del idx, dist, t_lof

    res["query_ms"] = timed(lambda: index.query(q, k))
    if not args.no_end_to_end:
        res["model_ms"] = timed(lambda: btsbot_amd.NoveltyModel(index, k))
    model = btsbot_amd.NoveltyModel.__new__(btsbot_amd.NoveltyModel)      # the fit above, without another search
    model.index, model.n_neighbors, model.kdist, model.lrd, model.lof = index, k, kdist, lrd, lof
    res["score_call_ms"] = timed(lambda: model.score(q))
    res["threshold_1pct"] = model.threshold(0.01)
    res["flagged_at_1pct"] = int((s_lof > res["threshold_1pct"]).sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
