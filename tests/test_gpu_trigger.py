"""btsbot_amd.TriggerState (btsbot_trigger_update / _reset / _load) on the device against the streaming restatement of
tests/test_trigger_host.py and, where the stream is time-ordered, against the offline restatement of
tests/test_policy_host.py and val.policy_eval.  Every output is a count or a copy of an input: every comparison is exact,
NaN positions included."""
import numpy as np
import pytest
import torch

from test_gpu_policy import T0, _cat, _object, _one
from test_policy_host import REFERENCE_POLICIES, restate_objects
from test_trigger_host import (CHUNKS, EXPORTED, RESERVED_ID, SAME_AS_OFFLINE, StreamRestatement, same_arrays,
                               sorted_golden)

pytestmark = pytest.mark.gpu

KEYS = ("object_id", "jd", "magpsf", "raw_preds")
OFFLINE = ("object_id", "jd", "magpsf", "label", "raw_preds")
K1 = {"k1": (0.5, 19.0, 1, None), "k1_gate": (0.5, 19.0, 1, 18.5)}
SWEEP16 = {f"t{i}": (0.05 + 0.055 * i, 19.0, 1 + i % 3, None if i % 2 else 18.5) for i in range(16)}
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 1031)
SCENARIOS = ("never", "first", "last", "random")


def _state(cuda, policies=REFERENCE_POLICIES, capacity=512):
    from btsbot_amd import TriggerState
    return TriggerState(policies, capacity, cuda)


def _args(cuda, rows, s=0, e=None):
    return [torch.from_numpy(np.ascontiguousarray(rows[k][s:e])).to(cuda) for k in KEYS]


def _feed(state, cuda, rows, chunk=None):
    """update() chunk by chunk -> (fired uint8 [n, n_pol], dropped bool [n]) over all rows, read once at the end."""
    n = len(rows["jd"])
    outs = [state.update(*_args(cuda, rows, s, s + (chunk or n))) for s in range(0, n, chunk or max(n, 1))]
    for o in outs:
        assert o["fired"].dtype in (torch.bool, torch.uint8) and o["fired"].device.type == "cuda"
    return (torch.cat([o["fired"] for o in outs]).cpu().numpy().astype(np.uint8),
            torch.cat([o["dropped"] for o in outs]).cpu().numpy().astype(bool))


def _export(state):
    out = state.export()
    assert tuple(out) == EXPORTED and all(v.device.type == "cuda" for v in out.values())
    assert out["object_id"].dtype == torch.int64 and out["n_alerts"].dtype == torch.int64
    assert out["pred"].dtype == out["count"].dtype == torch.int32 and out["trigger_jd"].dtype == torch.float64
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want, keys):
    diff = same_arrays(got, want, keys)
    assert diff is None, diff


def _offline(rows, policies=REFERENCE_POLICIES):
    return restate_objects(*(rows[k] for k in OFFLINE), policies)


def _fired_rows_are_the_triggers(rows, fired, exported):
    """Column sums = objects that fired; a fired row carries its object's trigger; no (object, policy) pair twice."""
    assert list(fired.sum(0)) == list(exported["pred"].sum(0))
    at = {int(o): k for k, o in enumerate(exported["object_id"])}
    seen = set()
    for i, q in np.argwhere(fired):
        o = at[int(rows["object_id"][i])]
        assert (int(o), int(q)) not in seen
        seen.add((int(o), int(q)))
        assert rows["jd"][i] == exported["trigger_jd"][o, q]
        m = rows["magpsf"][i]
        assert m == exported["trigger_mag"][o, q] or (np.isnan(m) and np.isnan(exported["trigger_mag"][o, q]))
    return seen


@pytest.fixture(scope="module")
def golden_stream():
    stream, shuffled = sorted_golden()
    return stream, shuffled, _offline(shuffled)


@pytest.fixture(scope="module")
def run_lengths():
    """Objects of every size in SIZES in each of the four scenarios, shuffled into one batch; and the same alerts split
    at each object's median jd into an earlier and a later shuffled batch."""
    rng = np.random.default_rng(17)
    plan = [(n, sc) for n in SIZES for sc in SCENARIOS]
    objs = [_object(1000 + 7 * k, n, rng, sc, label=k % 2) for k, (n, sc) in enumerate(plan)]
    whole = _cat(objs, rng)
    early = np.zeros(len(whole["jd"]), dtype=bool)
    for o in objs:
        early |= (whole["object_id"] == o["object_id"][0]) & (whole["jd"] < np.median(o["jd"]))
    halves = [{k: v[m] for k, v in whole.items()} for m in (early, ~early)]
    return plan, whole, halves


# ---- 1. the fixture, cut into batches any way ---------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", CHUNKS)
def test_fixture_chunk_invariance(cuda, golden_stream, chunk):
    from btsbot_amd import val
    stream, _, want = golden_stream
    state = _state(cuda)
    fired, dropped = _feed(state, cuda, stream, chunk)
    got = _export(state)
    _same(got, want, SAME_AS_OFFLINE + ("pred",))
    dev = val.policy_eval(*[torch.from_numpy(np.ascontiguousarray(stream[k])).to(cuda) for k in OFFLINE])
    exported = state.export()
    for k in SAME_AS_OFFLINE + ("pred",):
        assert dev[k].dtype == exported[k].dtype and dev[k].shape == exported[k].shape, k
    _same(got, {k: v.cpu().numpy() for k, v in dev.items()}, SAME_AS_OFFLINE + ("pred",))
    assert not dropped.any()
    assert state.counters() == dict(objects=len(want["object_id"]), taken=len(stream["jd"]), dropped=0, late=0)
    pairs = _fired_rows_are_the_triggers(stream, fired, got)
    # new_triggers over the same stream: the same set, with the triggers' values
    other, n, found = _state(cuda), len(stream["jd"]), set()
    for s in range(0, n, chunk):
        new = {k: v.cpu().numpy() for k, v in other.new_triggers(*_args(cuda, stream, s, s + chunk)).items()}
        assert set(new) == {"object_id", "policy", "trigger_jd", "trigger_mag", "alert"}
        for oid, q, tjd, tmag, a in zip(*(new[k] for k in ("object_id", "policy", "trigger_jd", "trigger_mag", "alert"))):
            assert stream["object_id"][s + a] == oid and fired[s + a, q] == 1
            assert (tjd, tmag) == (stream["jd"][s + a], stream["magpsf"][s + a])
            found.add((int(np.searchsorted(got["object_id"], oid)), int(q)))
        assert len(new["alert"]) == fired[s:s + chunk].sum()
    assert found == pairs
    _same(_export(other), got, EXPORTED)


# ---- 2. run lengths and carries ---------------------------------------------------------------------------------------
def test_run_lengths_one_batch(cuda, run_lengths):
    plan, whole, _ = run_lengths
    state = _state(cuda)
    fired, dropped = _feed(state, cuda, whole)
    got = _export(state)
    _same(got, _offline(whole), SAME_AS_OFFLINE + ("pred",))
    assert list(got["n_alerts"]) == [n for n, _ in plan] and not dropped.any()
    _fired_rows_are_the_triggers(whole, fired, got)


def test_run_lengths_carried_through_the_slot(cuda, run_lengths):
    plan, whole, halves = run_lengths
    state = _state(cuda)
    fired = [_feed(state, cuda, h)[0] for h in halves]
    got = _export(state)
    _same(got, _offline(whole), SAME_AS_OFFLINE + ("pred",))
    assert state.counters()["late"] == 0
    both = {k: np.concatenate([h[k] for h in halves]) for k in KEYS}
    _fired_rows_are_the_triggers(both, np.concatenate(fired), got)
    for k, (n, sc) in enumerate(plan):
        in_half = [f[h["object_id"] == got["object_id"][k]].sum(0) for f, h in zip(fired, halves)]
        if sc == "never":
            assert not in_half[0].any() and not in_half[1].any()
        elif sc == "last":               # the count and the gate are completed by the latest alert
            assert not in_half[0].any() and list(in_half[1]) == ([1] * 4 if n >= 2 else [0, 0, 1, 1])
        elif sc == "first" and n >= 4:   # the two earliest alerts lie before the median
            assert list(in_half[0]) == [1] * 4 and not in_half[1].any()


# ---- 3. ties ------------------------------------------------------------------------------------------------------------
def test_ties(cuda):
    for mags, scores, trig in (([18.1, 18.2, 18.3], [0.1, 0.9, 0.9], [18.2, 18.2]),
                               ([18.1, 18.2, 18.3], [0.9, 0.1, 0.9], [18.1, 18.1])):
        case = _one([T0 + 1, T0 + 1, T0 + 3], mags, scores)
        state = _state(cuda, K1)
        fired, _ = _feed(state, cuda, case)
        got = _export(state)
        _same(got, _offline(case, K1), SAME_AS_OFFLINE)
        assert list(got["trigger_mag"][0]) == trig and fired.sum() == 2
    # equal jd in two batches: arrival decides
    for first, second, trig in (((18.2, 0.9), (18.1, 0.9), 18.2), ((18.2, 0.1), (18.1, 0.9), 18.1)):
        state = _state(cuda, K1)
        f1, _ = _feed(state, cuda, _one([T0 + 1], [first[0]], [first[1]]))
        f2, _ = _feed(state, cuda, _one([T0 + 1], [second[0]], [second[1]]))
        got = _export(state)
        _same(got, _offline(_one([T0 + 1, T0 + 1], [first[0], second[0]], [first[1], second[1]]), K1), SAME_AS_OFFLINE)
        assert list(got["trigger_mag"][0]) == [trig, trig] and state.counters()["late"] == 0
        assert f1.sum() + f2.sum() == 2 and f1.sum() == (2 if trig == 18.2 else 0)
    # 130 alerts at 10 epochs: one batch; and the time-sorted stream cut inside an epoch and inside a 64-alert step
    rng = np.random.default_rng(5)
    pols = dict(REFERENCE_POLICIES, k7=(0.5, 19.0, 7, 18.35))
    case = _one(T0 + rng.integers(0, 10, 130).astype(np.float64), np.round(rng.uniform(18.3, 19.3, 130), 1),
                np.clip(rng.normal(0.45, 0.2, 130), 0, 1))
    assert len(np.unique(case["jd"])) == 10
    want = _offline(case, pols)
    state = _state(cuda, pols)
    _feed(state, cuda, case)
    _same(_export(state), want, SAME_AS_OFFLINE + ("pred",))
    order = np.argsort(case["jd"], kind="stable")
    srt = {k: v[order] for k, v in case.items()}
    assert srt["jd"][69] == srt["jd"][70]
    for chunk in (70, 33):
        state = _state(cuda, pols)
        _feed(state, cuda, srt, chunk)
        _same(_export(state), want, SAME_AS_OFFLINE + ("pred",))
        assert state.counters()["late"] == 0


# ---- 4. NaN magnitudes --------------------------------------------------------------------------------------------------
def test_nan_magnitudes(cuda):
    nan = np.nan
    mid = _one([T0, T0 + 1, T0 + 2, T0 + 3], [18.4, nan, 18.8, 18.7], [0.9, 0.9, 0.1, 0.9])
    allnan = _one([T0, T0 + 1, T0 + 2], [nan, nan, nan], [0.9, 0.9, 0.9], oid=8)
    first = _one([T0 + 1, T0, T0 + 2], [18.2, nan, 18.3], [0.9, 0.9, 0.9], oid=9)
    rng = np.random.default_rng(3)
    big = _cat([_object(1, 70, rng, "random"), _object(2, 300, rng, "last")], rng)
    big["magpsf"][::7] = nan
    case = _cat([mid, allnan, first, big])
    want = _offline(case)
    order = np.argsort(case["jd"], kind="stable")
    srt = {k: v[order] for k, v in case.items()}
    for rows, chunk in ((case, None), (srt, 1), (srt, 50)):
        state = _state(cuda)
        fired, _ = _feed(state, cuda, rows, chunk)
        got = _export(state)
        _same(got, want, SAME_AS_OFFLINE + ("pred",))
        _fired_rows_are_the_triggers(rows, fired, got)
        k = {int(o): i for i, o in enumerate(got["object_id"])}
        assert got["min_magpsf"][k[7]] == 18.4 and list(got["trigger_jd"][k[7]]) == [T0 + 3, T0 + 3, T0, T0]
        assert np.isnan(got["min_magpsf"][k[8]]) and not got["pred"][k[8]].any() and (got["count"][k[8]] == 0).all()
        assert list(got["trigger_jd"][k[9]]) == [T0 + 2, T0 + 2, T0 + 1, T0 + 1]
    # no magnitude at all, policies without a cut that NaN could pass: a gated policy never fires
    state = _state(cuda, {"gated": (0.5, 19.0, 1, 30.0)})
    _feed(state, cuda, allnan)
    assert not _export(state)["pred"].any()


# ---- 5. a full table ----------------------------------------------------------------------------------------------------
def test_full_table_drops_new_objects_only(cuda):
    rng = np.random.default_rng(23)
    ids = rng.choice(np.arange(-5000, 5000, dtype=np.int64) * 7919, 296, replace=False)
    old, new = ids[:256], ids[256:]

    def batch(which, t0):
        oid = np.repeat(which, rng.integers(1, 4, len(which)))
        n = len(oid)
        rows = dict(object_id=oid, jd=t0 + rng.uniform(0, 5, n), magpsf=np.round(rng.uniform(18.0, 19.4, n), 2),
                    raw_preds=np.clip(rng.normal(0.6, 0.3, n), 0, 1).astype(np.float32))
        order = rng.permutation(n)
        return {k: v[order] for k, v in rows.items()}

    b1, b2 = batch(old, T0), batch(np.concatenate([new, old[100:150]]), T0 + 10)
    state, host = _state(cuda, capacity=256), StreamRestatement(capacity=256)
    f1, d1 = _feed(state, cuda, b1)
    assert not d1.any() and state.counters() == dict(objects=256, taken=len(b1["jd"]), dropped=0, late=0)
    f2, d2 = _feed(state, cuda, b2)
    is_new = np.isin(b2["object_id"], new)
    assert np.array_equal(d2, is_new) and 0 < is_new.sum() < len(is_new) and not f2[is_new].any()
    hf1, hd1 = host.update(*(b1[k] for k in KEYS))
    hf2, hd2 = host.update(*(b2[k] for k in KEYS))
    assert np.array_equal(f1, hf1) and np.array_equal(f2, hf2) and np.array_equal(d2, hd2) and not hd1.any()
    assert state.counters() == host.counters() == dict(objects=256, taken=len(b1["jd"]) + int((~is_new).sum()),
                                                       dropped=int(is_new.sum()), late=0)
    got = _export(state)
    _same(got, host.export(), EXPORTED)
    # ... which is the restatement run on the alerts that were not dropped
    kept = {k: np.concatenate([b1[k], b2[k][~is_new]]) for k in KEYS}
    plain = StreamRestatement()
    plain.update(*(b1[k] for k in KEYS))
    plain.update(*(b2[k][~is_new] for k in KEYS))
    _same(got, plain.export(), EXPORTED)
    assert len(got["object_id"]) == 256 and got["n_alerts"].sum() == len(kept["jd"])


# ---- 6. awkward ids -----------------------------------------------------------------------------------------------------
def test_awkward_ids(cuda):
    cap = 64
    i64 = np.iinfo(np.int64)
    ids = np.array([0, cap, 2 * cap, 3 * cap, 17 * cap, -cap, 1 << 40, -1, -2, -123456789012345, i64.max, i64.min + 1,
                    5, 5 + (1 << 32), 5 + (1 << 33), 5 + (1 << 62), 5 - (1 << 63) + (1 << 32), i64.max - 1], dtype=np.int64)
    assert len(np.unique(ids)) == len(ids) and RESERVED_ID not in ids
    rng = np.random.default_rng(2)

    def batch(t0):
        oid = np.concatenate([np.repeat(ids, 2), np.full(3, RESERVED_ID, dtype=np.int64)])
        n = len(oid)
        rows = dict(object_id=oid, jd=t0 + rng.uniform(0, 5, n), magpsf=np.round(rng.uniform(18.0, 19.4, n), 2),
                    raw_preds=np.clip(rng.normal(0.7, 0.3, n), 0, 1).astype(np.float32))
        order = rng.permutation(n)
        return {k: v[order] for k, v in rows.items()}

    state, host = _state(cuda, capacity=cap), StreamRestatement(capacity=cap)
    for t0 in (T0, T0 + 10):
        b = batch(t0)
        fired, dropped = _feed(state, cuda, b)
        hf, hd = host.update(*(b[k] for k in KEYS))
        assert np.array_equal(dropped, b["object_id"] == RESERVED_ID) and np.array_equal(dropped, hd)
        assert np.array_equal(fired, hf) and not fired[dropped].any()
        assert state.counters() == host.counters() and state.counters()["objects"] == len(ids)   # found again, not re-made
    got = _export(state)
    _same(got, host.export(), EXPORTED)
    assert np.array_equal(got["object_id"], np.sort(ids)) and (got["n_alerts"] == 4).all()


# ---- 7. arrival order ---------------------------------------------------------------------------------------------------
def test_arrival_order_is_kept(cuda, golden_stream):
    _, shuffled, want = golden_stream
    state, host = _state(cuda), StreamRestatement()
    fired, _ = _feed(state, cuda, shuffled, 64)
    hf = np.concatenate([host.update(*(shuffled[k][s:s + 64] for k in KEYS))[0] for s in range(0, len(shuffled["jd"]), 64)])
    got = _export(state)
    _same(got, host.export(), EXPORTED)
    assert np.array_equal(fired, hf)
    assert state.counters() == host.counters() and host.late > 1000
    assert same_arrays(got, want, ("trigger_jd",)) is not None          # not the offline result
    # the whole shuffled fixture as ONE batch is sorted inside the batch: the offline result
    one = _state(cuda)
    _feed(one, cuda, shuffled)
    _same(_export(one), want, SAME_AS_OFFLINE + ("pred",))
    assert one.counters()["late"] == 0


# ---- 8. export / load ---------------------------------------------------------------------------------------------------
def test_export_and_load(cuda, golden_stream):
    from btsbot_amd import TriggerState
    stream, _, want = golden_stream
    half = len(stream["jd"]) // 2
    parts = [{k: v[:half] for k, v in stream.items()}, {k: v[half:] for k, v in stream.items()}]
    whole = _state(cuda)
    _feed(whole, cuda, stream, 257)
    first = _state(cuda)
    f1, _ = _feed(first, cuda, parts[0], 257)
    records = first.export()
    moved = TriggerState.from_export(records, REFERENCE_POLICIES, capacity=1024, device=cuda)
    assert moved.capacity == 1024 and moved.counters()["objects"] == len(records["object_id"])
    _same(_export(moved), {k: v.cpu().numpy() for k, v in records.items()}, EXPORTED)
    f2, _ = _feed(moved, cuda, parts[1], 257)
    got = _export(moved)
    _same(got, _export(whole), EXPORTED)
    _same(got, want, SAME_AS_OFFLINE + ("pred",))
    _fired_rows_are_the_triggers(stream, np.concatenate([f1, f2]), got)
    # numpy records load too; an id twice, the reserved id and too small a table raise
    as_numpy = {k: v.cpu().numpy() for k, v in records.items()}
    _same(_export(TriggerState.from_export(as_numpy, REFERENCE_POLICIES, capacity=256, device=cuda)), as_numpy, EXPORTED)
    twice = {k: np.concatenate([v, v[3:4]]) for k, v in as_numpy.items()}
    with pytest.raises(ValueError, match="came before"):
        TriggerState.from_export(twice, REFERENCE_POLICIES, capacity=1024, device=cuda)
    reserved = {k: v.copy() for k, v in as_numpy.items()}
    reserved["object_id"][0] = RESERVED_ID
    with pytest.raises(ValueError, match="no slot"):
        TriggerState.from_export(reserved, REFERENCE_POLICIES, capacity=1024, device=cuda)
    with pytest.raises(ValueError, match="no slot"):
        TriggerState.from_export(as_numpy, REFERENCE_POLICIES, capacity=64, device=cuda)
    with pytest.raises(ValueError, match="policies"):
        TriggerState.from_export(as_numpy, K1, capacity=1024, device=cuda)


# ---- 9. policy counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pol", (1, 4, 5, 16))
def test_policy_counts(cuda, run_lengths, n_pol):
    _, whole, halves = run_lengths
    pols = dict(list(SWEEP16.items())[:n_pol])
    want = _offline(whole, pols)
    assert n_pol == 1 or 0 < want["pred"].sum() < want["pred"].size
    for batches in ([whole], halves):
        state = _state(cuda, pols)
        fired = np.concatenate([_feed(state, cuda, b)[0] for b in batches])
        got = _export(state)
        assert got["pred"].shape == (len(want["object_id"]), n_pol) and fired.shape[1] == n_pol
        _same(got, want, SAME_AS_OFFLINE + ("pred",))
        _fired_rows_are_the_triggers({k: np.concatenate([b[k] for b in batches]) for k in KEYS}, fired, got)


# ---- 10. the empty batch, streams, reset, argument checks ---------------------------------------------------------------
def test_empty_batch_streams_and_reset(cuda, golden_stream):
    stream, _, want = golden_stream
    state = _state(cuda)
    e = torch.zeros(0, device=cuda)
    out = state.update(e.long(), e.double(), e.double(), e.float())
    assert tuple(out["fired"].shape) == (0, 4) and tuple(out["dropped"].shape) == (0,)
    assert state.counters() == dict(objects=0, taken=0, dropped=0, late=0) and _export(state)["object_id"].size == 0
    assert all(v.numel() == 0 for v in state.new_triggers(e.long(), e.double(), e.double(), e.float()).values())
    args = _args(cuda, stream)
    torch.cuda.synchronize(cuda)
    side = torch.cuda.Stream(cuda)
    with torch.cuda.stream(side):
        state.update(*args)
        state.update(e.long(), e.double(), e.double(), e.float())          # a no-op in the middle of a stream
    torch.cuda.current_stream(cuda).wait_stream(side)
    _same(_export(state), want, SAME_AS_OFFLINE + ("pred",))
    state.reset()
    assert state.counters() == dict(objects=0, taken=0, dropped=0, late=0) and _export(state)["object_id"].size == 0
    _feed(state, cuda, stream, 257)
    _same(_export(state), want, SAME_AS_OFFLINE + ("pred",))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        state.update(*(a.cpu() for a in args))
    with pytest.raises(ValueError):
        state.update(args[0], args[1][:3], args[2], args[3])               # lengths
    with pytest.raises(ValueError):
        state.update(args[1], args[1], args[2], args[3])                   # float ids
    _same(_export(state), want, SAME_AS_OFFLINE + ("pred",))               # a refused call changes nothing
