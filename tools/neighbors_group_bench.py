#!/usr/bin/env python
"""Time the grouped embedding neighbours (btsbot_knn_query_grouped: EmbeddingIndex(groups=...).query(...,
exclude_same_group / one_per_group)) on one GPU against the ungrouped query of the same run and the torch-op form:

    python tools/neighbors_group_bench.py [N] [Q] [D] [k]      # default 1,000,000  8,192  528  15

The bank is an archive of objects: long-tailed object sizes (tools/splits_bench.py's: 4 Pareto(1.1) + 1, capped at 4,000),
every alert its object's centre (N(0,1)) plus a jitter of 0.05 N(0,1), rows in shuffled order; a query is one more alert of
a random object of the bank and carries that object's id -- so the ungrouped answer is the object's own epochs, the case the
modes are for.  HIP events after a warm-up call, seven blocks, the MEDIAN block reported.  Prints one JSON line:
  ungrouped_ms, exclude_ms, one_ms, both_ms
                 index.query end to end (query pack, selection, merge, allocations) without groups and in the three modes
  *_select_ms, *_merge_ms
                 the two kernels of one call, from torch.profiler's device-side kernel records in a separate, untimed
                 call (null when the profiler reports no such kernels)
  one_distinct_ms, one_distinct_select_ms
                 one_per_group where every bank row is its own group: the answer (and every list) is the ungrouped one, so
                 what this costs over ungrouped_ms is the same-group scan in offer_one() alone; what
                 one_ms costs over it is what same-group candidates add (replacements in place, bucket rounds)
  ungrouped_k17_ms, ungrouped_k8_ms, one_k8_ms
                 what occupancy and a smaller k are worth: the ungrouped query at k = 17 (lists of more than 16 KB: one
                 workgroup per CU, not two), and both forms at k = 8.  These decided where one_per_group keeps the groups
                 of its list entries (the workspace, not LDS: DESIGN.md section 4m)
  torch_one_ms, torch_one_peak_gib, torch_blocks
                 the form a user has today for one_per_group: torch.cdist over query chunks, scatter_reduce(amin) into
                 [chunk, n_groups], topk; chunks sized so that a chunk's [rows, N] fp32 matrix stays under 4 GiB; its
                 peak device memory above the inputs (torch_blocks: 7, or 3 where one call takes over 2 s)
  knn_peak_gib   the same peak for index.query(..., one_per_group=True)
  one_groups_differ
                 of a 256-query sample, the rows whose set of returned GROUPS differs from the torch form's
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402
from neighbors_bench import BLOCKS, CHUNK_BYTES, peak_gib, timed   # noqa: E402


def object_sizes(n, seed=0):
    rng = np.random.default_rng(seed)
    sizes = np.minimum((rng.pareto(1.1, n) * 4 + 1).astype(np.int64), 4000)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), n)) + 1]
    sizes[-1] -= sizes.sum() - n
    return sizes[sizes > 0]


def archive(n, nq, d, dev, seed=0):
    sizes = object_sizes(n, seed)
    g = torch.Generator(device=dev).manual_seed(7 + seed)
    centres = torch.randn((len(sizes), d), generator=g, device=dev)
    rank = torch.repeat_interleave(torch.arange(len(sizes), device=dev), torch.from_numpy(sizes).to(dev))
    rank = rank[torch.randperm(n, generator=g, device=dev)]
    bank = centres[rank] + 0.05 * torch.randn((n, d), generator=g, device=dev)
    qrank = torch.randint(0, len(sizes), (nq,), generator=g, device=dev)
    q = centres[qrank] + 0.05 * torch.randn((nq, d), generator=g, device=dev)
    ids = lambda r: r * 977 - 12345 + ((r % 3) << 40)          # ids as wide as alert_utils.object_keys'
    return bank, ids(rank), rank, q, ids(qrank), sizes


def torch_one_per_group(q, bank, rank, n_groups, k):
    rows = max(1, min(q.shape[0], CHUNK_BYTES // (4 * bank.shape[0])))
    idx, dist = [], []
    for i in range(0, q.shape[0], rows):
        dm = torch.cdist(q[i:i + rows], bank)
        best = torch.full((dm.shape[0], n_groups), float("inf"), device=q.device)
        best.scatter_reduce_(1, rank.expand(dm.shape[0], -1), dm, "amin")
        d, j = best.topk(k, dim=1, largest=False)
        idx.append(j)
        dist.append(d)
    return torch.cat(idx), torch.cat(dist)


def kernel_times(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        got = {}
        for ev in prof.events():
            for name in ("knn_select_kernel", "knn_merge_kernel"):
                if name in ev.name:
                    t = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
                    got[name] = got.get(name, 0.0) + t / 1000.0
        return got
    except Exception as e:   # the profiler is optional: the end-to-end figures do not depend on it
        print(f"neighbors_group_bench: kernel times not measured ({type(e).__name__}: {e})", file=sys.stderr)
        return {}


def main():
    args = [int(a) for a in sys.argv[1:5]]
    n, nq, d, k = args + [1_000_000, 8192, 528, 15][len(args):]
    if not torch.cuda.is_available():
        sys.exit("neighbors_group_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    bank, bg, rank, q, qg, sizes = archive(n, nq, d, dev)
    index = btsbot_amd.EmbeddingIndex(bank, groups=bg)
    distinct = btsbot_amd.EmbeddingIndex(bank, groups=torch.arange(n, device=dev))
    calls = {
        "ungrouped": lambda: index.query(q, k),
        "exclude": lambda: index.query(q, k, query_groups=qg, exclude_same_group=True),
        "one": lambda: index.query(q, k, one_per_group=True),
        "both": lambda: index.query(q, k, query_groups=qg, exclude_same_group=True, one_per_group=True),
        "one_distinct": lambda: distinct.query(q, k, one_per_group=True),
    }
    out = dict(n_bank=n, n_query=nq, dim=d, k=k, objects=int(len(sizes)), largest_object=int(sizes.max()),
               splits=int(btsbot_amd._lib.lib().btsbot_knn_splits(nq, n, d, k)), device=torch.cuda.get_device_name(0),
               blocks=BLOCKS)
    for name, fn in calls.items():
        out[f"{name}_ms"] = round(timed(fn), 3)
    for name, fn in calls.items():
        kt = kernel_times(fn)
        for kern in ("select", "merge"):
            t = kt.get(f"knn_{kern}_kernel")
            out[f"{name}_{kern}_ms"] = None if t is None else round(t, 3)
    for name in ("exclude", "one", "both", "one_distinct"):
        out[f"{name}_over_ungrouped"] = round(out[f"{name}_ms"] / out["ungrouped_ms"], 3)
    out["ungrouped_k17_ms"] = round(timed(lambda: index.query(q, 17)), 3)       # one workgroup per CU
    out["ungrouped_k8_ms"] = round(timed(lambda: index.query(q, 8)), 3)
    out["one_k8_ms"] = round(timed(lambda: index.query(q, 8, one_per_group=True)), 3)
    out["knn_peak_gib"] = round(peak_gib(calls["one"]), 3)

    torch_fn = lambda: torch_one_per_group(q, bank, rank, len(sizes), k)
    once = timed(torch_fn, 1)
    out["torch_blocks"] = BLOCKS if once <= 2000.0 else 3
    out["torch_one_ms"] = round(timed(torch_fn, out["torch_blocks"]), 3)
    out["torch_one_peak_gib"] = round(peak_gib(torch_fn), 3)
    out["torch_over_one"] = round(out["torch_one_ms"] / out["one_ms"], 2)

    sample = slice(0, min(256, nq))
    knn_i, _ = index.query(q[sample], k, one_per_group=True)
    torch_g, _ = torch_one_per_group(q[sample], bank, rank, len(sizes), k)
    out["one_groups_differ"] = int((rank[knn_i].sort(1).values != torch_g.sort(1).values).any(dim=1).sum())
    out["sample"] = int(knn_i.shape[0])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
