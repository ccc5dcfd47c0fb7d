#!/usr/bin/env python
"""Time the stamp decode on one GPU against the host decode, in the same run:

    python tools/stamp_decode_bench.py [B ...] [--kernel-only]      # B alerts (3 stamps each), default 1024 8192

For each B and for two kinds of synthetic 63x63 float32 stamps -- `noise` (Gaussian pixels: almost all literals, the
worst case for a Huffman decoder) and `smooth` (a tilted plane plus a source, rounded to 1/8: mostly matches) -- gzip
level 9, 512 distinct stamps of each kind drawn at random so that the lanes of a wave never hold the same stream:
  kernel_ms             btsbot_decode_stamps alone (blob, offsets and workspace already on the device)
  decode_call_ms        alert_utils.decode_stamps_device: join, one upload, the launch
  triplets_device_ms    make_triplets(decode="device", fallback=None)
  triplets_host_ms      make_triplets as shipped: decode_stamp in a Python loop on one host thread, then prep_triplets
  host_pool16_ms        decode_stamp over the same stamps on a pool of 16 threads (zlib releases the GIL)
Device figures: HIP events after >= 0.5 s of the same work, seven blocks, the MEDIAN block (tools/alert_features_bench.py's
timed()).  The two host figures are wall-clock medians of three runs over min(B, 1024) alerts, scaled to B alerts
(`host_alerts` says how many were run).  One JSON line per (B, kind)."""
import ctypes as C
import gzip
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from alert_features_bench import timed   # noqa: E402
from btsbot_amd import _lib, alert_utils   # noqa: E402

DISTINCT = 512
KEYS = ("cutoutScience", "cutoutTemplate", "cutoutDifference")


def fits_gz(img):
    cards = [f"{'SIMPLE':<8}= {'T':>20}", f"{'BITPIX':<8}= {-32:>20}", f"{'NAXIS':<8}= {2:>20}",
             f"{'NAXIS1':<8}= {img.shape[1]:>20}", f"{'NAXIS2':<8}= {img.shape[0]:>20}", "END"]
    header = "".join(c.ljust(80) for c in cards).encode("ascii")
    header += b" " * (-len(header) % 2880)
    data = img.astype(">f4").tobytes()
    return gzip.compress(header + data + b"\0" * (-len(data) % 2880), compresslevel=9, mtime=0)


def pool_of(kind, rng):
    y, x = np.mgrid[0:63, 0:63].astype(np.float32)
    out = []
    for _ in range(DISTINCT):
        if kind == "noise":
            img = rng.standard_normal((63, 63)).astype(np.float32) * 30 + 100
        else:
            a, b, c = rng.uniform(-1, 1, 3)
            cx, cy, s = rng.uniform(20, 43), rng.uniform(20, 43), rng.uniform(1.5, 4)
            img = 100 + a * x + b * y + 500 * c * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
            img = (np.round(img * 8) / 8).astype(np.float32)
        out.append(fits_gz(img))
    return out


def wall(fn, repeats=3):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernel_only = "--kernel-only" in sys.argv
    sizes = [int(a) for a in args] or [1024, 8192]
    if not torch.cuda.is_available():
        sys.exit("stamp_decode_bench: needs a GPU (the host decode alone is not what this tool is for)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    pools = {k: pool_of(k, rng) for k in ("noise", "smooth")}
    L = _lib.lib()
    for b in sizes:
        for kind, pool in pools.items():
            n = 3 * b
            stamps = [pool[i] for i in rng.integers(0, DISTINCT, n)]
            alerts = [{k: {"stampData": s} for k, s in zip(KEYS, stamps[i:i + 3])} for i in range(0, n, 3)]
            raw, shapes, status = alert_utils.decode_stamps_device(stamps, dev)
            torch.cuda.synchronize(dev)
            assert not status.any().item() and (shapes == 63).all().item()
            check = rng.integers(0, n, 8)
            for i in check:
                assert np.array_equal(raw[i].cpu().numpy(), alert_utils.decode_stamp(stamps[i]))

            blob = torch.frombuffer(bytearray(b"".join(stamps)), dtype=torch.uint8).to(dev)
            offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in stamps])]), dtype=torch.int64, device=dev)
            ws_bytes = L.btsbot_decode_stamps_workspace(n)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            ptr = [C.c_void_p(t.data_ptr()) for t in (blob, offsets, raw, shapes, status, ws)]

            def kernel():
                _lib.check(L.btsbot_decode_stamps(ptr[0], ptr[1], n, ptr[2], ptr[3], ptr[4], ptr[5], ws_bytes, st),
                           "btsbot_decode_stamps")

            steps = max(1, min(20, 16384 // b))
            k_ms, k_all = timed(kernel, steps, dev)
            row = {"alerts": b, "stamps": n, "kind": kind, "compressed_bytes_mean": round(blob.numel() / n, 1),
                   "kernel_ms": round(k_ms, 4), "kernel_stamps_per_s": round(n / k_ms * 1e3),
                   "blocks_kernel_ms": [round(x, 4) for x in k_all], "workspace_mib": round(ws_bytes / 2 ** 20, 1)}
            if not kernel_only:
                c_ms, _ = timed(lambda: alert_utils.decode_stamps_device(stamps, dev), steps, dev)
                t_ms, _ = timed(lambda: alert_utils.make_triplets(alerts, dev, decode="device", fallback=None), steps, dev)
                hb = min(b, 1024)

                def host_path():
                    alert_utils.make_triplets(alerts[:hb], dev)
                    torch.cuda.synchronize(dev)

                with ThreadPoolExecutor(16) as pool16:
                    h16 = wall(lambda: list(pool16.map(alert_utils.decode_stamp, stamps[:3 * hb], chunksize=64)))
                h1 = wall(host_path)
                row.update({"decode_call_ms": round(c_ms, 4), "triplets_device_ms": round(t_ms, 4), "host_alerts": hb,
                            "triplets_host_ms": round(h1 * b / hb, 2), "host_pool16_ms": round(h16 * b / hb, 2),
                            "device_alerts_per_s": round(b / t_ms * 1e3), "host_alerts_per_s": round(hb / h1 * 1e3),
                            "host_pool16_alerts_per_s": round(hb / h16 * 1e3)})
            row.update({"steps_per_block": steps, "lib": os.path.basename(_lib.LIB_PATH),
                        "device": torch.cuda.get_device_name(dev)})
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
