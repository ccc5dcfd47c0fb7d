#!/usr/bin/env python
"""Time the partitioned index (btsbot_amd.IvfIndex, btsbot_amd.kmeans; csrc/ivf.hip) on one GPU against the exact search:

    python tools/ivf_bench.py [N] [Q] [D] [k] [n_lists]      # default 1,000,000  8,192  528  15  1,024

50 Gaussian clusters (centres 2 N(0,1), rows N(0,1) around them), seeded; the queries are fresh draws.  HIP events after a
warm-up call, seven blocks, the MEDIAN block reported.  Prints one JSON line:
  fit            assign_ms / update_ms per Lloyd iteration (update_ms with the stable sort of the labels, sort_ms of it),
                 update_kernels_ms and update_gbs: btsbot_kmeans_update alone on a given order, in GB/s of fp32 rows read;
                 index_add_ms / index_add_gbs: the same means by zeros.index_add_(0, labels, rows) / counts in this run;
                 layout_ms: the list image and its row maps (btsbot_ivf_layout with the sort of the labels);
                 index_select_ms: torch's index_select of the packed records by the image's row map alone (no padding
                 records, no maps: a lower bound of that route); fit_ms: IvfIndex(bank, n_lists) end to end, once
  lists          largest, mean, empty; the work items of the nprobe = 8 call: their number, the longest (in 128-row bank
                 tiles) against the mean
  exact_ms       index.query(queries, k) in this run
  query          per nprobe in 1 2 4 8 16 32: ms of ivf.query end to end (with the probes), probes_ms of it, select_ms and
                 merge_ms from torch.profiler's kernel records in a separate call, recall (recall@k over all Q against
                 index.query of this run), over_exact = ms / exact_ms
  graph          ivf.knn_graph(k, nprobe=8) over all N rows, once: ms, and recall of its neighbour columns against the
                 exact search on a sample of 8,192 rows
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd                      # noqa: E402
from btsbot_amd import ivf as ivf_mod  # noqa: E402

BLOCKS = 7
NPROBES = (1, 2, 4, 8, 16, 32)


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


def once(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def kernel_times(fn, names):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        got = {}
        for ev in prof.events():
            for name in names:
                if name in ev.name:
                    t = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
                    got[name] = got.get(name, 0.0) + t / 1000.0
        return got
    except Exception as e:   # the profiler is optional: the end-to-end figures do not depend on it
        print(f"ivf_bench: kernel times not measured ({type(e).__name__}: {e})", file=sys.stderr)
        return {}


def recall(got, want):
    """The fraction of want's valid entries that the same row of got holds."""
    hit = ((got[:, :, None] == want[:, None, :]) & (want[:, None, :] >= 0)).any(dim=1).sum()
    return float(hit) / max(int((want >= 0).sum()), 1)


def clusters(n, d, centres, g):
    which = torch.randint(0, centres.shape[0], (n,), generator=g, device=centres.device)
    return centres[which] + torch.randn((n, d), generator=g, device=centres.device)


def main():
    args = [int(a) for a in sys.argv[1:6]]
    n, nq, d, k, nl = args + [1_000_000, 8192, 528, 15, 1024][len(args):]
    if not torch.cuda.is_available():
        sys.exit("ivf_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    centres = 2.0 * torch.randn((50, d), generator=g, device=dev)
    bank, q = clusters(n, d, centres, g), clusters(nq, d, centres, g)
    r2 = lambda x: round(x, 3)   # noqa: E731

    ivf, fit_ms = once(lambda: btsbot_amd.IvfIndex(bank, nl, n_iter=10, seed=0))
    rows, cen, labels = ivf.index.bank, ivf.centroids, ivf.labels
    order = torch.sort(labels, stable=True).indices
    scratch = cen.clone()
    valid = labels >= 0
    lv, rv = labels[valid], rows[valid]

    def by_index_add():
        sums = torch.zeros_like(cen).index_add_(0, lv, rv)
        return sums / torch.bincount(lv, minlength=nl).clamp(min=1)[:, None]

    rec = ivf.index._record_bytes()
    src = ivf._row_of.clamp(min=0).to(torch.int64)
    gbs = lambda ms: round(n * d * 4 / (ms * 1e-3) / 1e9, 1)   # noqa: E731
    upd = timed(lambda: ivf_mod.kmeans_update(rows, labels, scratch, order))
    add = timed(by_index_add)
    fit = dict(fit_ms=r2(fit_ms), n_iter=10,
               assign_ms=r2(timed(lambda: ivf_mod._assign(cen, rows))),
               update_ms=r2(timed(lambda: ivf_mod.kmeans_update(rows, labels, scratch))),
               sort_ms=r2(timed(lambda: torch.sort(labels, stable=True))),
               update_kernels_ms=r2(upd), update_gbs=gbs(upd), index_add_ms=r2(add), index_add_gbs=gbs(add),
               update_vs_index_add_max_abs=float((scratch - by_index_add()).abs().max()),
               layout_ms=r2(timed(ivf._layout)),
               index_select_ms=r2(timed(lambda: ivf.index._packed[:n * rec].view(n, rec).index_select(0, src))),
               list_image_gib=round(ivf._list_packed.numel() / 2 ** 30, 3))

    sizes = ivf.list_sizes
    tiles = (sizes + 127) // 128
    pr = ivf.probes(q, min(8, nl))
    per_list = torch.bincount(pr[pr >= 0].view(-1), minlength=nl)
    items = (per_list + 127) // 128
    item_tiles = torch.repeat_interleave(tiles, items)
    lists = dict(largest=int(sizes.max()), mean=round(float(sizes.float().mean()), 1), empty=int((sizes == 0).sum()),
                 items=int(items.sum()), longest_item_tiles=int(item_tiles.max()) if item_tiles.numel() else 0,
                 mean_item_tiles=round(float(item_tiles.float().mean()), 2) if item_tiles.numel() else 0.0)

    exact_ms = timed(lambda: ivf.index.query(q, k))
    want = ivf.index.query(q, k)[0]
    query = {}
    for nprobe in NPROBES:
        if nprobe > min(nl, 32):
            continue
        ms = timed(lambda: ivf.query(q, k, nprobe))
        kt = kernel_times(lambda: ivf.query(q, k, nprobe), ("ivf_select_kernel", "ivf_merge_kernel"))
        query[str(nprobe)] = dict(ms=r2(ms), probes_ms=r2(timed(lambda: ivf.probes(q, nprobe))),
                                  select_ms=None if "ivf_select_kernel" not in kt else r2(kt["ivf_select_kernel"]),
                                  merge_ms=None if "ivf_merge_kernel" not in kt else r2(kt["ivf_merge_kernel"]),
                                  recall=round(recall(ivf.query(q, k, nprobe)[0], want), 4),
                                  over_exact=round(ms / exact_ms, 3))

    graph = None
    if nl >= 8 and k > 1:
        (gi, _gd), graph_ms = once(lambda: ivf.knn_graph(k, nprobe=8))
        sample = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:min(8192, n)].to(dev)
        truth = ivf.index.query(rows[sample], k - 1, self_rows=sample)[0]
        graph = dict(ms=r2(graph_ms), nprobe=8, sample=int(sample.shape[0]),
                     recall=round(recall(gi[sample][:, 1:].contiguous(), truth), 4))

    print(json.dumps(dict(n_bank=n, n_query=nq, dim=d, k=k, n_lists=nl, device=torch.cuda.get_device_name(0),
                          blocks=BLOCKS, fit=fit, lists=lists, exact_ms=r2(exact_ms), query=query, graph=graph)))


if __name__ == "__main__":
    main()
