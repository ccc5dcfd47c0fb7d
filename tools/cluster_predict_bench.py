#!/usr/bin/env python
"""Time ClusterModel.predict (btsbot_cluster_offer_knn / _csr / _assign) on one GPU:

    python tools/cluster_predict_bench.py [N] [Q] [D] [min_samples] [--no-refit]     # default 100,000  8,192  528  10

Rows: tools/radius_bench.py's set (50 Gaussian clusters, centres 4 N(0,1), unit noise, seeded and centred); the Q new rows
are every (N / Q)-th bank row plus N(0, 0.5).  min_cluster_size = min_samples.  HIP events after a warm-up call, seven
blocks, the MEDIAN block.  Prints one JSON line:
  fit_ms              ClusterModel(index, ...) once (not a median): the spanning tree, the host pass, the tables
  predict_ms          model.predict(queries) end to end: index.query, the offer kernel, the read of the unresolved rows,
                      their radius tier, the assign kernel
  query_ms            index.query(queries, k_s) alone, the yardstick
  kernels_ms          the offer and the assign kernel alone on the lists, slack included (two launches; no radius tier)
  unresolved          rows of the call sent to the radius tier, radius_total the entries of their lists
  torch_ms            the same rule as torch ops on the same lists (gather, maximum, argmin on the keys, a masked climb
                      loop), for the rows the lists resolve
  torch_agrees        labels, clusters and lambda of the torch form equal the kernels' on the resolved rows
  refit_ms            hdbscan(bank + new rows) end to end, the only way to such labels without predict
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402
from radius_bench import clusters, timed   # noqa: E402


def torch_form(m, idx, dist):
    """the rule on the lists alone, in torch: (labels, cluster, lambda)"""
    t, ms = m.tables, m.min_samples
    core = m.mst.core
    present = idx >= 0
    safe = idx.clamp(min=0)
    core_q = dist[:, ms - 2] if ms > 1 else torch.zeros_like(dist[:, 0])
    w = torch.maximum(torch.maximum(dist, core_q[:, None]), core[safe]).clamp(min=0)
    key = (w.view(torch.int32).to(torch.int64) << 32) | safe
    key = torch.where(present, key, torch.full_like(key, torch.iinfo(torch.int64).max))
    best = key.min(dim=1).values
    b = best & 0xffffffff
    w_best = (best >> 32).to(torch.int32).view(torch.float32)
    lam = torch.where(w_best == 0, torch.full_like(w_best, m.lam_zero, dtype=torch.float64), 1.0 / w_best.double())
    c = t["row_cluster"][b].to(torch.int64)
    parent, birth = t["parent"].to(torch.int64), t["birth"]
    go = t["row_lambda"][b] > lam
    for _ in range(int(parent.shape[0])):
        go = go & (parent[c] >= 0) & (birth[c] >= lam)
        if not bool(go.any()):                       # (one host read per level, as a torch form has to)
            break
        c = torch.where(go, parent[c].clamp(min=0), c)
    return t["label"][c].to(torch.int64), c, lam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=100_000)
    ap.add_argument("q", nargs="?", type=int, default=8192)
    ap.add_argument("d", nargs="?", type=int, default=528)
    ap.add_argument("min_samples", nargs="?", type=int, default=10)
    ap.add_argument("--no-refit", action="store_true", help="skip refit_ms (eight fits of bank plus new rows)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cluster_predict_bench: needs a GPU")
    dev = torch.device("cuda:0")
    n, nq, ms = args.n, args.q, args.min_samples
    res = {"N": n, "Q": nq, "D": args.d, "min_samples": ms, "min_cluster_size": ms}

    bank, _ = clusters(n, args.d, 1, dev)
    bank -= bank.mean(dim=0)
    index = btsbot_amd.EmbeddingIndex(bank)
    del bank
    rows = torch.arange(0, n, max(1, n // nq), device=dev)[:nq]
    gen = torch.Generator(device=dev).manual_seed(2)
    q = index.bank[rows] + 0.5 * torch.randn((len(rows), args.d), generator=gen, device=dev)

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    m = btsbot_amd.ClusterModel(index, ms, ms)
    b.record()
    b.synchronize()
    res["fit_ms"] = a.elapsed_time(b)
    res["clusters"] = int(m.labels.max()) + 1
    res["bank_noise_share"] = float((m.labels < 0).double().mean())

    stats = {}
    labels, prob, det = m.predict(q, return_details=True, stats=stats)
    res.update(stats)
    res["unresolved_share"] = stats["unresolved"] / max(nq, 1)
    res["query_noise_share"] = float((labels < 0).double().mean())
    res["outlier_median"], res["outlier_max"] = float(det["outlier"].median()), float(det["outlier"].max())
    k_s = max(min(64, max(8, 2 * ms)), ms - 1, 1)
    res["k_s"] = k_s
    res["predict_ms"] = timed(lambda: m.predict(q))
    res["query_ms"] = timed(lambda: index.query(q, k_s))
    idx, dist = index.query(q, k_s)

    def kernels():
        _core_q, best_w, best_j, _unres = m._offer(idx, dist, q)
        return m._assign(best_w, best_j)

    res["kernels_ms"] = timed(kernels)
    res["torch_ms"] = timed(lambda: torch_form(m, idx, dist))
    res["torch_over_kernels"] = res["torch_ms"] / res["kernels_ms"]
    unres = m._offer(idx, dist, q)[3] != 0
    t_lab, t_c, t_lam = torch_form(m, idx, dist)
    ok = ~unres
    res["torch_agrees"] = bool(torch.equal(t_lab[ok], labels[ok]) and torch.equal(t_c[ok], det["cluster"][ok])
                               and torch.equal(t_lam[ok].view(torch.int64), det["lambda"][ok].view(torch.int64)))
    if not args.no_refit:
        both = torch.cat([index.bank, q])
        res["refit_ms"] = timed(lambda: btsbot_amd.hdbscan(both, ms, ms))
        res["refit_over_predict"] = res["refit_ms"] / res["predict_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
