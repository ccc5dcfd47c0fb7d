#!/usr/bin/env python
"""Time the placement of new rows on an existing map (btsbot_layout_transform, btsbot_amd.layout_transform) on one GPU
against the torch-op form of the same epochs:

    python tools/layout_transform_bench.py [N] [Q] [D] [k] [epochs]      # default 1,000,000  8,192  528  15  100

Bank and queries: draws of 50 Gaussian clusters (centres 4 N(0,1), unit noise), seeded.  The bank's map is NOT laid out
(at 10^6 rows that is the 8.9 s of DESIGN.md section 4n): its positions are the rows projected on two random directions
and scaled to max |y| = 10, which gives the transform the same kind of input -- clustered positions in a box of 20.  HIP
events after a warm-up call, seven blocks, the MEDIAN block reported.  Prints one JSON line:
  query_ms        EmbeddingIndex.query(queries, k) on the packed bank
  memberships_ms  query_memberships(idx, dist): one launch
  transform_ms    layout_transform over all `epochs` epochs with the memberships' launch, the start's and the ONE launch of
                  the schedule; epoch_us = transform_ms / epochs
  torch_ms        the same epochs written with torch ops on the same inputs in the same run: the firing mask, gathers of
                  the fired slots, index_add_ of the attractive terms and of negative_sample_rate rounds of repulsive terms
                  (torch.randint targets: a timing comparator, not the same samples)
  firings_per_epoch, gathers_per_epoch
                  slots that fire in an epoch (mean); bank positions gathered at random per epoch, firings *
                  negative_sample_rate (the neighbours' positions stay in registers)
  line_gbps       those gathers counted as the 128-byte lines they touch, over epoch time
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


def fire_mask(r, n):
    return torch.floor(n * r) > torch.floor((n - 1) * r)


def torch_transform(idx, w, bank_y, n_epochs, a, b, rate=RATE):
    present = idx >= 0
    safe = idx.clamp(min=0)
    wsum = w.sum(dim=1, keepdim=True)
    y = (w[:, :, None] * bank_y[safe]).sum(dim=1) / wsum
    r = torch.where(present, w / w.max(dim=1, keepdim=True).values, torch.zeros_like(w)).double()
    n_bank = bank_y.shape[0]
    for n in range(1, n_epochs + 1):
        v, j = fire_mask(r, n).nonzero(as_tuple=True)
        acc = torch.zeros_like(y)
        diff = y[v] - bank_y[safe[v, j]]
        d2 = (diff * diff).sum(dim=1, keepdim=True)
        coeff = torch.where(d2 > 0, -2.0 * a * b * d2 ** (b - 1.0) / (1.0 + a * d2 ** b), torch.zeros_like(d2))
        acc.index_add_(0, v, (coeff * diff).clamp(-4.0, 4.0))
        for _ in range(rate):
            t = torch.randint(n_bank, v.shape, device=y.device)
            diff = y[v] - bank_y[t]
            d2 = (diff * diff).sum(dim=1, keepdim=True)
            term = (2.0 * b / ((0.001 + d2) * (1.0 + a * d2 ** b)) * diff).clamp(-4.0, 4.0)
            acc.index_add_(0, v, torch.where(d2 > 0, term, torch.full_like(term, 4.0)))
        y = y + 0.25 * (1.0 - (n - 1) / n_epochs) * acc
    return y


def main():
    args = [int(x) for x in sys.argv[1:6]]
    n, q, d, k, epochs = args + [1_000_000, 8192, 528, 15, 100][len(args):]
    if not torch.cuda.is_available():
        sys.exit("layout_transform_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    centres = 4.0 * torch.randn((50, d), generator=gen, device=dev)
    bank = centres[torch.arange(n, device=dev) % 50] + torch.randn((n, d), generator=gen, device=dev)
    queries = centres[torch.arange(q, device=dev) % 50] + torch.randn((q, d), generator=gen, device=dev)
    proj = bank @ torch.randn((d, 2), generator=gen, device=dev)
    bank_y = (proj * (10.0 / proj.abs().max())).contiguous()
    a, b = btsbot_amd.find_ab_params(1.0, 0.1)

    index = btsbot_amd.EmbeddingIndex(bank)
    query_ms = timed(lambda: index.query(queries, k))
    idx, dist = index.query(queries, k)
    memberships_ms = timed(lambda: btsbot_amd.query_memberships(idx, dist))
    w, _sigma = btsbot_amd.query_memberships(idx, dist)
    transform_ms = timed(lambda: btsbot_amd.layout_transform(idx, dist, bank_y, epochs, a=a, b=b, negative_sample_rate=RATE))
    torch_ms = timed(lambda: torch_transform(idx, w, bank_y, epochs, a, b), blocks=3)

    r = torch.where(idx >= 0, w / w.max(dim=1, keepdim=True).values, torch.zeros_like(w)).double()
    fired = sum(int(fire_mask(r, e).sum()) for e in range(1, epochs + 1)) / epochs
    gathers = fired * RATE
    epoch_ms = transform_ms / epochs
    out = dict(n_bank=n, q=q, dim=d, k=k, epochs=epochs, negative_sample_rate=RATE, device=torch.cuda.get_device_name(0),
               blocks=BLOCKS, query_ms=round(query_ms, 3), memberships_ms=round(memberships_ms, 4),
               transform_ms=round(transform_ms, 4), epoch_us=round(1e3 * epoch_ms, 3), torch_ms=round(torch_ms, 2),
               torch_over_kernel=round(torch_ms / transform_ms, 1), firings_per_epoch=round(fired),
               gathers_per_epoch=round(gathers), line_gbps=round(128 * gathers / (epoch_ms * 1e-3) / 1e9, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
