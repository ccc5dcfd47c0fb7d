#!/usr/bin/env python
"""Time retention for the streaming states (btsbot_trigger_rehash / btsbot_feature_rehash, ObjectState.expire) on one GPU:

    python tools/retention_bench.py [N]          # N alerts of history, default 1,000,000

The state is the one trigger_bench.py and feature_state_bench.py build -- their history of N alerts (a million: 47,837
objects) replayed into a table of 2^20 slots -- and the cut is the median last_jd of its objects, so about half of them
go.  Timed with HIP events after >= 0.5 s of the same work, seven blocks, the MEDIAN block reported (as bench.py does).
Every timed call starts from the same full state: expire() only reads the table it leaves, so putting that table back
(host work, not timed) undoes it.  Prints one JSON line with, for each of the two states:
  rehash_kernel_ms    the one launch of the rehash symbol into a destination that was reset before (not timed)
  rehash_none_expire_ms / rehash_all_expire_ms / rehash_empty_source_ms
                      the same launch with the cut at -inf (every record claimed and copied), at +inf (no claim, no copy)
                      and over an empty table of the same size (nothing to count): where the kernel's time goes
  reset_kernel_ms     the launch of the reset symbol on the destination
  expire_ms           state.expire(cut) end to end: the allocation of the second table, its reset, the rehash, the swap
  kernel_share        rehash_kernel_ms / expire_ms
  export_reload_ms    the way to the same state before there was expire(): export() -> keep last_jd >= cut ->
                      from_export() at the same capacity (host clock: the route ends in its second host read)
  expire_over_export_reload = expire_ms / export_reload_ms
  same_state          the two routes were compared once, export() against export(): true
"""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from btsbot_amd import FeatureState, TriggerState, _lib, val   # noqa: E402
from feature_state_bench import KEYS as FEATURE_KEYS   # noqa: E402
from feature_state_bench import with_packet_fields   # noqa: E402
from trigger_bench import history, host_timed, timed   # noqa: E402

CAPACITY, STEPS, RELOAD_STEPS = 1 << 20, 200, 5
TRIGGER_KEYS = ("object_id", "jd", "magpsf", "raw_preds")


def same(a, b):
    return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


def measure(state, empty, reload, dev):
    """-> the figures of one state that holds the history; empty: a state of the same kind that holds nothing;
    reload(records) is the class's from_export at CAPACITY."""
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    held = state.export()
    cut = float(held["last_jd"].median())
    going = int((held["last_jd"] < cut).sum())
    full = state._installed()

    def restore():
        state._install(*full)

    arrays, table = state._allocate(CAPACITY)                       # a destination of the bench's own (arrays: kept alive)
    reset, rehash = getattr(L, state._RESET), getattr(L, state._REHASH)

    def reset_dst():
        _lib.check(reset(C.byref(table), st), state._RESET)

    def rehash_dst(src=full[2], keep_from=cut):
        _lib.check(rehash(C.byref(src), C.byref(table), C.c_double(keep_from), st), state._REHASH)

    rk_ms, rk_all = timed(rehash_dst, STEPS, dev, before=reset_dst)
    none_ms, _ = timed(lambda: rehash_dst(keep_from=float("-inf")), STEPS, dev, before=reset_dst)
    all_ms, _ = timed(lambda: rehash_dst(keep_from=float("inf")), STEPS, dev, before=reset_dst)
    empty_ms, _ = timed(lambda: rehash_dst(src=empty._table), STEPS, dev, before=reset_dst)
    zk_ms, zk_all = timed(reset_dst, STEPS, dev)
    ex_ms, ex_all = timed(lambda: state.expire(cut), STEPS, dev, before=restore)
    restore()
    state.expire(cut)
    after, counters, expired = state.export(), state.counters(), state.n_expired()
    restore()

    def old_route():
        records = state.export()
        keep = records["last_jd"] >= cut
        return reload({k: v[keep] for k, v in records.items()})

    other = old_route().export()
    agree = all(same(after[k], other[k]) for k in after)
    er_ms, er_all = host_timed(old_route, RELOAD_STEPS)
    r4 = lambda xs: [round(x, 4) for x in xs]   # noqa: E731
    return {"objects": int(held["object_id"].numel()), "expired": going, "n_expired": expired, "counters_after": counters,
            "bytes_per_slot": int(sum(t.numel() * t.element_size() for t in full[1][:-1]) // CAPACITY),
            "rehash_kernel_ms": round(rk_ms, 4), "rehash_none_expire_ms": round(none_ms, 4),
            "rehash_all_expire_ms": round(all_ms, 4), "rehash_empty_source_ms": round(empty_ms, 4),
            "reset_kernel_ms": round(zk_ms, 4), "expire_ms": round(ex_ms, 4),
            "kernel_share": round(rk_ms / ex_ms, 4), "export_reload_ms": round(er_ms, 4),
            "expire_over_export_reload": round(ex_ms / er_ms, 5), "same_state": agree,
            "blocks_rehash_kernel_ms": r4(rk_all), "blocks_reset_kernel_ms": r4(zk_all), "blocks_expire_ms": r4(ex_all),
            "blocks_export_reload_ms": r4(er_all)}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    if not torch.cuda.is_available():
        sys.exit("retention_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    hist, sizes, _ = history(n)
    trig = TriggerState(val.REFERENCE_POLICIES, CAPACITY, dev)
    trig.update(*(torch.from_numpy(hist[k]).to(dev) for k in TRIGGER_KEYS))
    feat = FeatureState(CAPACITY, dev)
    packets = with_packet_fields(hist, 2)
    feat.update(*(torch.from_numpy(packets[k]).to(dev) for k in FEATURE_KEYS))
    out = {"alerts": n, "objects": int(len(sizes)), "capacity": CAPACITY,
           "steps_per_block": {"rehash": STEPS, "reset": STEPS, "expire": STEPS, "export_reload": RELOAD_STEPS},
           "trigger": measure(trig, TriggerState(val.REFERENCE_POLICIES, CAPACITY, dev),
                              lambda r: TriggerState.from_export(r, val.REFERENCE_POLICIES, CAPACITY, dev), dev),
           "feature": measure(feat, FeatureState(CAPACITY, dev), lambda r: FeatureState.from_export(r, CAPACITY, dev), dev),
           "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
