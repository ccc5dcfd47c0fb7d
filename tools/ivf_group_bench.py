#!/usr/bin/env python
"""Time the partitioned index by source (btsbot_ivf_query_grouped: IvfIndex(groups=...).query(..., exclude_same_group /
one_per_group)) on one GPU against the ungrouped probed query and the exact grouped search of the same run:

    python tools/ivf_group_bench.py [N] [Q] [D] [k] [n_lists]      # default 1,000,000  8,192  528  15  1,024

The bank is tools/neighbors_group_bench.py's archive of objects (long-tailed object sizes, 47,837 objects at the default
N; every alert its object's centre plus a small jitter; rows shuffled); a query is one more alert of a random bank object
and carries that object's id.  tools/ivf_bench.py's timing: HIP events after a warm-up call, seven blocks, the MEDIAN block
reported.  Prints one JSON line:
  fit_ms         IvfIndex(bank, n_lists, groups=...) end to end, once; layout_groups_ms: the groups in list order alone
  exact          per mode (ungrouped, exclude, one, both): ms of ivf.index.query with the mode's switches
  query          per mode and per nprobe in 1 8 32:
                   ms          ivf.query end to end (with the probes)
                   select_ms, merge_ms   the two kernels of a separate, untimed call, from torch.profiler's kernel records
                   recall      of SOURCES: the fraction of the groups in the exact answer of the same mode (ivf.index.query,
                               same switches) that the probed answer's row holds too
                   peak_gib    peak device memory of one call above what was allocated before it
                   over_ungrouped   ms / the ungrouped ms at the same nprobe; over_exact: ms / the mode's exact ms
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd                                         # noqa: E402
from ivf_bench import kernel_times, once                  # noqa: E402
from neighbors_bench import BLOCKS, peak_gib, timed       # noqa: E402
from neighbors_group_bench import archive                 # noqa: E402

NPROBES = (1, 8, 32)


def source_recall(got, want, groups):
    """The fraction of the groups of want's valid rows that the same row of got holds."""
    g_got = torch.where(got >= 0, groups[got.clamp(min=0)], torch.full_like(got, torch.iinfo(torch.int64).min))
    g_want = groups[want.clamp(min=0)]
    hit = ((g_got[:, :, None] == g_want[:, None, :]) & (want[:, None, :] >= 0)).any(dim=1).sum()
    return float(hit) / max(int((want >= 0).sum()), 1)


def main():
    args = [int(a) for a in sys.argv[1:6]]
    n, nq, d, k, nl = args + [1_000_000, 8192, 528, 15, 1024][len(args):]
    if not torch.cuda.is_available():
        sys.exit("ivf_group_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    bank, bg, _rank, q, qg, sizes = archive(n, nq, d, dev)
    ivf, fit_ms = once(lambda: btsbot_amd.IvfIndex(bank, nl, n_iter=10, seed=0, groups=bg))
    modes = {
        "ungrouped": {},
        "exclude": dict(query_groups=qg, exclude_same_group=True),
        "one": dict(one_per_group=True),
        "both": dict(query_groups=qg, exclude_same_group=True, one_per_group=True),
    }
    r3 = lambda x: round(x, 3)   # noqa: E731
    L = btsbot_amd._lib.lib()
    lg = torch.empty_like(ivf._list_groups)
    out = dict(n_bank=n, n_query=nq, dim=d, k=k, n_lists=nl, objects=int(len(sizes)), largest_object=int(sizes.max()),
               device=torch.cuda.get_device_name(0), blocks=BLOCKS, fit_ms=r3(fit_ms),
               layout_groups_ms=r3(timed(lambda: L.btsbot_ivf_layout_groups(
                   btsbot_amd._lib.ptr(ivf.groups), n, nl, btsbot_amd._lib.ptr(ivf._row_of), ivf._list_rows,
                   btsbot_amd._lib.ptr(lg), btsbot_amd._lib.stream(dev)))),
               largest_list=int(ivf.list_sizes.max()), exact={}, query={})
    want = {}
    for name, kw in modes.items():
        out["exact"][name] = r3(timed(lambda: ivf.index.query(q, k, **kw)))
        want[name] = ivf.index.query(q, k, **kw)[0]
    for nprobe in NPROBES:
        if nprobe > min(nl, 32):
            continue
        row = {}
        for name, kw in modes.items():
            fn = lambda: ivf.query(q, k, nprobe, **kw)   # noqa: E731
            ms = timed(fn)
            kt = kernel_times(fn, ("ivf_select_kernel", "ivf_merge_kernel"))
            row[name] = dict(ms=r3(ms),
                             select_ms=None if "ivf_select_kernel" not in kt else r3(kt["ivf_select_kernel"]),
                             merge_ms=None if "ivf_merge_kernel" not in kt else r3(kt["ivf_merge_kernel"]),
                             recall=round(source_recall(fn()[0], want[name], bg), 4), peak_gib=r3(peak_gib(fn)),
                             over_ungrouped=r3(ms / row["ungrouped"]["ms"]) if name != "ungrouped" else 1.0,
                             over_exact=r3(ms / out["exact"][name]))
        out["query"][str(nprobe)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
