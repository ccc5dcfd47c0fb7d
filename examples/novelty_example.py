#!/usr/bin/env python3
"""Which of tonight's sources look like nothing in the archive?

A seeded ``mm_ConvNeXt`` embeds a synthetic archive of multi-epoch objects: every ``--epochs`` consecutive alerts are one
source, near-copies of one another, and a few ``--odd`` sources are unlike all the others (a double source in the stamps,
metadata beyond the usual ranges) -- but they, too, are in the archive with all their epochs.  Two fits of the local
outlier factor: ``btsbot.NoveltyModel(index, k)`` on the index that carries ``groups`` leaves a row's own source out,
``btsbot.NoveltyModel(index.bank, k)`` knows no sources.  A night of further epochs of archive sources is then streamed
through ``btsbot.ScoreStream(embed="features")`` -- the embedding row comes out of the launch that scores the batch -- and
each batch is scored by both: without sources an odd object is as dense as its own earlier epochs and scores about 1
(as long as ``k`` is below ``--epochs``); with ``exclude_same_group`` it stands alone.  Tonight's most novel sources are
listed by the second score.

    python examples/novelty_example.py [--sources 600] [--epochs 5] [--odd 4] [--night 512] [--k 4]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd as btsbot  # noqa: E402
from btsbot_amd.synthetic import META_RANGES, synthetic_batch  # noqa: E402
from trigger_example import seeded_model  # noqa: E402


def epochs_of(images, meta, source, seed):
    """one alert per entry of ``source``: that source's stamps and metadata plus a little noise"""
    gen = torch.Generator().manual_seed(seed)
    img, m = images[source], meta[source]
    span = torch.tensor([hi - lo for lo, hi in META_RANGES])
    return (img * (1.0 + 0.01 * torch.randn(img.shape, generator=gen)),
            m + 1e-3 * span * torch.randn(m.shape, generator=gen))


def odd_sources(images, meta, n):
    """the first n sources become unlike all others, each in its own way: a double source off the centre at its own
    angle, and metadata beyond the ranges the others fill, in its own corner"""
    yy, xx = torch.meshgrid(torch.arange(63.0), torch.arange(63.0), indexing="ij")
    lo = torch.tensor([r[0] for r in META_RANGES])
    hi = torch.tensor([r[1] for r in META_RANGES])
    cols = torch.arange(len(META_RANGES))
    for i in range(n):
        a = torch.tensor(3.14159265 * i / max(n, 1))
        dy, dx = 14.0 * torch.sin(a), 14.0 * torch.cos(a)
        pair = (torch.exp(-((yy - 31 - dy) ** 2 + (xx - 31 - dx) ** 2) / 18.0)
                + torch.exp(-((yy - 31 + dy) ** 2 + (xx - 31 + dx) ** 2) / 18.0))
        img = images[i] + 0.5 * pair
        images[i] = img / img.flatten(1).norm(dim=1).reshape(3, 1, 1)
        corner = ((cols >> (i % 5)) & 1).float()                          # which columns go above, which below
        meta[i] = lo + (hi - lo) * (2.0 * corner - 0.5)


def main():
    p = argparse.ArgumentParser(description="Local outlier factor of a night's alerts against an archive (MI355X)")
    p.add_argument("--sources", type=int, default=600)
    p.add_argument("--epochs", type=int, default=5, help="alerts per archive source")
    p.add_argument("--odd", type=int, default=4, help="sources unlike all others")
    p.add_argument("--night", type=int, default=512)
    p.add_argument("--k", type=int, default=4, help="neighbours; below --epochs the masking is complete")
    p.add_argument("--precision", type=str, default="f16", choices=["f32", "bf16", "f16", "f16x2"])
    p.add_argument("--batch", type=int, default=256, help="alerts per forward")
    p.add_argument("--show", type=int, default=8, help="sources printed")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("novelty_example: needs a GPU (btsbot_amd has no CPU fallback)")
    dev = torch.device("cuda:0")
    model = seeded_model(args.precision).to(dev).eval()

    images, meta, _ = synthetic_batch(args.sources, seed=21)              # one alert per source, the others copy it
    gen = torch.Generator().manual_seed(22)
    odd_sources(images, meta, args.odd)
    names = btsbot.alert_utils.object_names(range(21 * 26 ** 7, 21 * 26 ** 7 + args.sources))
    ids = torch.from_numpy(btsbot.alert_utils.object_keys(names)).to(dev)

    def batches(img, m):
        return [(i.to(dev), j.to(dev)) for i, j in zip(img.split(args.batch), m.split(args.batch))]

    source = torch.arange(args.sources).repeat_interleave(args.epochs)
    stream = btsbot.ScoreStream(model, depth=2, embed="features")
    with torch.no_grad():
        index = None
        for _logits, emb in stream.map(batches(*epochs_of(images, meta, source, 23))):
            at = len(index) if index is not None else 0
            g = ids[source[at:at + emb.shape[0]].to(dev)]
            index = btsbot.EmbeddingIndex(emb, groups=g) if index is None else index.add(emb, groups=g)
    novelty = btsbot.NoveltyModel(index, args.k)                          # the fit: every row without its own source
    blind = btsbot.NoveltyModel(index.bank, args.k)                       # ... and the fit that knows no sources
    flag = novelty.threshold(0.01)
    print(f"archive: {len(index)} alerts of {args.sources} sources ({args.odd} odd), embedding width {index.dim}; "
          f"LOF of the archive: median {float(novelty.lof.nanmedian()):.3f}, 99th percentile {flag:.3f}")

    tonight = torch.cat([torch.arange(args.odd), torch.randint(args.odd, args.sources, (args.night - args.odd,),
                                                               generator=gen)])[torch.randperm(args.night, generator=gen)]
    plain, own_out = [], []
    with torch.no_grad():
        done = 0
        for _logits, emb in stream.map(batches(*epochs_of(images, meta, tonight, 24))):
            g = ids[tonight[done:done + emb.shape[0]].to(dev)]
            plain.append(blind.score(emb))
            own_out.append(novelty.score(emb, query_groups=g, exclude_same_group=True))
            done += emb.shape[0]
    plain, own_out = torch.cat(plain), torch.cat(own_out)
    # a source's score tonight: the largest of its alerts'
    per_source = torch.full((args.sources,), float("-inf"), dtype=torch.float64, device=dev)
    per_source.scatter_reduce_(0, tonight.to(dev), own_out, reduce="amax")
    per_plain = torch.full_like(per_source, float("-inf")).scatter_reduce_(0, tonight.to(dev), plain, reduce="amax")
    order = per_source.argsort(descending=True)[:args.show].tolist()
    print(f"tonight: {args.night} alerts; {int((own_out > flag).sum())} score above the archive's 99th percentile with "
          f"their own source left out, {int((plain > blind.threshold(0.01)).sum())} above the sourceless fit's")
    for s in order:
        print(f"  {names[s]}{' (odd)' if s < args.odd else '      '}  LOF without its own epochs {float(per_source[s]):8.3f}   "
              f"without sources {float(per_plain[s]):6.3f}")


if __name__ == "__main__":
    main()
