#!/usr/bin/env python3
"""A night's candidates against a partitioned archive: how much of the exact answer do a few lists give, and how fast?

A seeded ``mm_ConvNeXt`` embeds a synthetic archive through ``btsbot.ScoreStream(embed="features")``; the rows go into a
``btsbot.IvfIndex`` -- k-means centroids fitted on the device, the rows cut into lists around them.  A night of new alerts
is streamed through the same ``ScoreStream`` and every batch is looked up twice: ``ivf.query(emb, k, nprobe)``, which
walks only the lists of the ``nprobe`` nearest centroids, and ``ivf.index.query(emb, k)``, the exact search over the whole
archive.  Printed: the recall of the probed answer against the exact one and the time of both (HIP events; the first batch
warms both up and is not timed).  The probed answer is exact over the lists it looks at -- its distances are the exact
search's, bit for bit -- so recall is its only approximation.

    python examples/ivf_example.py [--archive 16384] [--night 2048] [--k 10] [--lists 128] [--nprobe 8]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd as btsbot  # noqa: E402
from btsbot_amd.synthetic import synthetic_batch  # noqa: E402
from trigger_example import seeded_model  # noqa: E402


def main():
    p = argparse.ArgumentParser(description="Probed against exact nearest archive alerts of a night's candidates (MI355X)")
    p.add_argument("--archive", type=int, default=16384)
    p.add_argument("--night", type=int, default=2048)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--lists", type=int, default=0, help="0: round(sqrt(archive))")
    p.add_argument("--nprobe", type=int, default=8)
    p.add_argument("--precision", type=str, default="f16", choices=["f32", "bf16", "f16", "f16x2"])
    p.add_argument("--batch", type=int, default=256, help="alerts per forward")
    args = p.parse_args()
    dev = torch.device("cuda:0")
    model = seeded_model(args.precision).to(dev).eval()

    def batches(images, meta):
        return [(i.to(dev), m.to(dev)) for i, m in zip(images.split(args.batch), meta.split(args.batch))]

    stream = btsbot.ScoreStream(model, depth=2, embed="features")
    images, meta, _ = synthetic_batch(args.archive, seed=11)
    with torch.no_grad():
        archive = torch.cat([emb for _logits, emb in stream.map(batches(images, meta))])
    ivf = btsbot.IvfIndex(archive, args.lists or None, n_iter=10, seed=0)
    sizes = ivf.list_sizes
    nprobe = min(args.nprobe, ivf.n_lists, 32)
    print(f"archive: {len(ivf)} alerts, embedding width {ivf.dim}, {ivf.n_lists} lists (largest {int(sizes.max())}, mean "
          f"{float(sizes.float().mean()):.1f}, empty {int((sizes == 0).sum())})")

    images, meta, _ = synthetic_batch(args.night, seed=12)
    hit = total = 0
    ms = [0.0, 0.0]
    same_bits = True
    with torch.no_grad():
        for b, (_logits, emb) in enumerate(stream.map(batches(images, meta))):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            idx, dist = ivf.query(emb, args.k, nprobe)
            ev[1].record()
            want, wdist = ivf.index.query(emb, args.k)
            ev[2].record()
            ev[2].synchronize()
            if b:
                ms[0] += ev[0].elapsed_time(ev[1])
                ms[1] += ev[1].elapsed_time(ev[2])
            found = (idx[:, :, None] == want[:, None, :]) & (want[:, None, :] >= 0)
            hit += int(found.any(dim=1).sum())
            total += int((want >= 0).sum())
            # a row both answers hold has the same distance in both, bit for bit
            at = found.float().argmax(dim=2)
            both = found.any(dim=2)
            same_bits &= bool((dist.view(torch.int32)[both] == wdist.view(torch.int32).gather(1, at)[both]).all())
    print(f"{args.night} alerts of the night, k = {args.k}, nprobe = {nprobe} of {ivf.n_lists}: recall {hit / max(total, 1):.4f} "
          f"against the exact search; probed {ms[0]:.2f} ms, exact {ms[1]:.2f} ms after the first batch; shared rows carry "
          f"the same distance bits: {same_bits}")


if __name__ == "__main__":
    main()
