#!/usr/bin/env python
"""Time the embedding neighbours (btsbot_knn_query, btsbot_amd.EmbeddingIndex) on one GPU against the torch-op form:

    python tools/neighbors_bench.py [N] [Q] [D] [k]      # default 1,000,000  8,192  528  15

N(0,1) rows, seeded.  HIP events after a warm-up call, seven blocks, the MEDIAN block reported.  Prints one JSON line:
  pack_ms        EmbeddingIndex(bank): the one-off pack of the bank (with the copy of the rows into the index)
  query_ms       index.query(queries, k) end to end: the query pack, the selection, the merge, the allocations
  select_ms, merge_ms, query_pack_ms
                 the three kernels of one query call, from torch.profiler's device-side kernel records in a separate,
                 untimed call (null when the profiler reports no such kernels)
  select_tflops  the products the selection needs, 2 * Q * N * D FLOP (three times as many f16 MFMA FLOP are issued on the
                 split operands), over select_ms
  torch_ms       the form a user would otherwise write: torch.cdist(chunk, bank).topk(k, largest=False) over query chunks
                 sized so that a chunk's [rows, N] fp32 matrix stays under 4 GiB
  torch_peak_gib, knn_peak_gib
                 peak device memory allocated during one call of either form, above what the inputs hold
  torch_rows_differ, knn_rows_differ
                 of a 256-query sample, the rows whose index list differs from the float64 brute force (direct-form
                 float64 distances on the device, ties by index).  Both forms return fp32 distances: two neighbours whose
                 float64 distances round to the same fp32 value come out in index order, which counts as a difference
  torch_sets_differ, knn_sets_differ
                 the same count for the index SETS (the order inside a row ignored)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd   # noqa: E402

BLOCKS = 7
CHUNK_BYTES = 4 << 30


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


def peak_gib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 30


def torch_form(q, bank, k):
    rows = max(1, min(q.shape[0], CHUNK_BYTES // (4 * bank.shape[0])))
    idx, dist = [], []
    for i in range(0, q.shape[0], rows):
        d, j = torch.cdist(q[i:i + rows], bank).topk(k, dim=1, largest=False)
        idx.append(j)
        dist.append(d)
    return torch.cat(idx), torch.cat(dist)


def float64_answer(q, bank, k, rows=16):
    """Index lists of the float64 brute force, direct form, ties by index (a stable sort of the k + 8 best)."""
    b64 = bank.double()
    out = []
    for i in range(0, q.shape[0], rows):
        d = torch.cdist(q[i:i + rows].double(), b64, compute_mode="donot_use_mm_for_euclid_dist")
        dd, j = d.topk(min(k + 8, bank.shape[0]), dim=1, largest=False)
        key = torch.argsort(j, dim=1, stable=True)
        dd, j = dd.gather(1, key), j.gather(1, key)
        key = torch.argsort(dd, dim=1, stable=True)
        out.append(j.gather(1, key)[:, :k])
    return torch.cat(out)


def kernel_times(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        got = {}
        for ev in prof.events():
            for name in ("knn_select_kernel", "knn_merge_kernel", "knn_pack_kernel"):
                if name in ev.name:
                    t = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
                    got[name] = got.get(name, 0.0) + t / 1000.0
        return got
    except Exception as e:   # the profiler is optional: the end-to-end figures do not depend on it
        print(f"neighbors_bench: kernel times not measured ({type(e).__name__}: {e})", file=sys.stderr)
        return {}


def main():
    args = [int(a) for a in sys.argv[1:5]]
    n, nq, d, k = args + [1_000_000, 8192, 528, 15][len(args):]
    if not torch.cuda.is_available():
        sys.exit("neighbors_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    bank = torch.randn((n, d), generator=g, device=dev)
    q = torch.randn((nq, d), generator=g, device=dev)

    pack_ms = timed(lambda: btsbot_amd.EmbeddingIndex(bank))
    index = btsbot_amd.EmbeddingIndex(bank)
    query_ms = timed(lambda: index.query(q, k))
    kt = kernel_times(lambda: index.query(q, k))
    knn_peak = peak_gib(lambda: index.query(q, k))
    torch_ms = timed(lambda: torch_form(q, bank, k))
    torch_peak = peak_gib(lambda: torch_form(q, bank, k))

    sample = q[:min(256, nq)]
    want = float64_answer(sample, bank, k)
    knn_i, _ = index.query(sample, k)
    torch_i, _ = torch_form(sample, bank, k)
    sel = kt.get("knn_select_kernel")
    out = dict(n_bank=n, n_query=nq, dim=d, k=k, splits=int(btsbot_amd._lib.lib().btsbot_knn_splits(nq, n, d, k)),
               device=torch.cuda.get_device_name(0), blocks=BLOCKS,
               pack_ms=round(pack_ms, 3), query_ms=round(query_ms, 3),
               select_ms=None if sel is None else round(sel, 3),
               merge_ms=None if "knn_merge_kernel" not in kt else round(kt["knn_merge_kernel"], 3),
               query_pack_ms=None if "knn_pack_kernel" not in kt else round(kt["knn_pack_kernel"], 3),
               select_tflops=None if not sel else round(2.0 * nq * n * d / (sel * 1e-3) / 1e12, 1),
               torch_ms=round(torch_ms, 3), torch_over_knn=round(torch_ms / query_ms, 2),
               torch_peak_gib=round(torch_peak, 3), knn_peak_gib=round(knn_peak, 3),
               torch_rows_differ=int((torch_i != want).any(dim=1).sum()),
               knn_rows_differ=int((knn_i != want).any(dim=1).sum()),
               torch_sets_differ=int((torch_i.sort(1).values != want.sort(1).values).any(dim=1).sum()),
               knn_sets_differ=int((knn_i.sort(1).values != want.sort(1).values).any(dim=1).sum()),
               sample=int(sample.shape[0]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
