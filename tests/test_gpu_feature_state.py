"""btsbot_amd.FeatureState (btsbot_feature_update / _reset / _load) on the device against the streaming restatement of
tests/test_feature_state_host.py and, where the stream is time-ordered, against the reference's recorded columns, the
offline restatement of tests/test_alert_features_host.py and alert_features on the device.  Every output is a selection or
one float64 subtraction rounded once: every comparison is exact, NaN positions included."""
import numpy as np
import pytest
import torch

from test_alert_features_host import restate
from test_feature_state_host import (CAUSAL, EXPORTED, NAMES, FeatureStreamRestatement, final_columns, golden_rows)
from test_gpu_alert_features import _objects, _one_object
from test_trigger_host import CHUNKS, RESERVED_ID, same_arrays

pytestmark = pytest.mark.gpu

T0 = 2459300.5
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 1031)
COUNTERS = ("objects", "taken", "dropped", "late")


def _state(cuda, capacity=512):
    from btsbot_amd import FeatureState
    return FeatureState(capacity, cuda)


def _args(cuda, rows, s=0, e=None):
    return [torch.from_numpy(np.ascontiguousarray(rows[k][s:e])).to(cuda) for k in NAMES]


def _feed(state, cuda, rows, chunk=None):
    """update() chunk by chunk -> (features float32 [n, 8], dropped bool [n]) over all rows, read once at the end."""
    n = len(rows["jd"])
    outs = [state.update(*_args(cuda, rows, s, s + (chunk or n))) for s in range(0, n, chunk or max(n, 1))]
    for o in outs:
        assert o["features"].dtype == torch.float32 and o["features"].device.type == "cuda" and o["features"].shape[1] == 8
        assert o["dropped"].dtype == torch.bool and o["dropped"].device.type == "cuda"
    return (torch.cat([o["features"] for o in outs]).cpu().numpy(), torch.cat([o["dropped"] for o in outs]).cpu().numpy())


def _host_feed(host, rows, chunk=None):
    n = len(rows["jd"])
    outs = [host.update(*(rows[k][s:s + (chunk or n)] for k in NAMES)) for s in range(0, n, chunk or max(n, 1))]
    return np.concatenate([o[0] for o in outs]).astype(np.float32), np.concatenate([o[1] for o in outs])


def _export(state):
    out = state.export()
    assert tuple(out) == EXPORTED and all(v.device.type == "cuda" for v in out.values())
    assert out["object_id"].dtype == torch.int64 and out["n_alerts"].dtype == torch.int64
    assert all(out[k].dtype == torch.float64 for k in EXPORTED[2:])
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want, keys=None):
    diff = same_arrays(got, want, keys) if keys else same_arrays({"rows": got}, {"rows": want}, ("rows",))
    assert diff is None, diff


def _against_restatement(cuda, batches, capacity=512, chunk=None):
    """Feeds the batches to a state and to the restatement: rows, dropped flags, export and counters must agree.
    -> (state, host, features over all batches, dropped over all batches)."""
    state, host = _state(cuda, capacity), FeatureStreamRestatement(capacity)
    feats, drops = [], []
    for b in batches:
        f, d = _feed(state, cuda, b, chunk)
        hf, hd = _host_feed(host, b, chunk)
        _same(f, hf)
        assert np.array_equal(d, hd)
        feats.append(f)
        drops.append(d)
    _same(_export(state), host.export(), EXPORTED)
    assert state.counters() == host.counters() and tuple(state.counters()) == COUNTERS
    return state, host, np.concatenate(feats), np.concatenate(drops)


def _offline_device(cuda, rows):
    from btsbot_amd import alert_utils
    return alert_utils.alert_features(*_args(cuda, rows)).cpu().numpy()


def _cat(cases):
    return {k: np.concatenate([c[k] for c in cases]) for k in NAMES}


def _batch(ids, t0, rng, reserved=0):
    """1-3 alerts (awkward ids: exactly 2) per id after t0, shuffled, plus `reserved` alerts of the reserved id."""
    oid = np.concatenate([ids, np.full(reserved, RESERVED_ID, dtype=np.int64)])
    n = len(oid)
    jd = t0 + rng.uniform(0, 5, n)
    rows = dict(object_id=oid, jd=jd, magpsf=np.round(rng.uniform(18.0, 19.4, n), 2),
                jdstarthist=t0 - 20 + rng.choice([-3.25, 0.0, 30.0], n), ndethist=rng.integers(1, 50, n).astype(np.int32))
    rows["ncovhist"] = (rows["ndethist"] + rng.integers(0, 2000, n)).astype(np.int32)
    order = rng.permutation(n)
    return {k: rows[k][order] for k in NAMES}


@pytest.fixture(scope="module")
def golden_stream(cuda):
    """(the fixture sorted by jd, as recorded, alert_features on the device over the sorted fixture)."""
    stream, shuffled = golden_rows()
    return stream, shuffled, _offline_device(cuda, stream)


@pytest.fixture(scope="module")
def run_lengths(cuda):
    """An object of every size in SIZES shuffled into one batch; the same alerts split at each object's median jd into an
    earlier and a later shuffled batch (with where each half's rows lie in the whole); alert_features over the whole."""
    whole = _objects(SIZES, seed=17)
    early = np.zeros(len(whole["jd"]), dtype=bool)
    for oid in np.unique(whole["object_id"]):
        mine = whole["object_id"] == oid
        early |= mine & (whole["jd"] < np.median(whole["jd"][mine]))
    halves = [{k: whole[k][m] for k in NAMES} for m in (early, ~early)]
    where = np.concatenate([np.flatnonzero(early), np.flatnonzero(~early)])
    return whole, halves, where, _offline_device(cuda, whole)


# ---- 1. the fixture, cut into batches any way ---------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", CHUNKS)
def test_fixture_chunk_invariance(cuda, golden_stream, chunk):
    stream, _, offline = golden_stream
    state, host, feats, dropped = _against_restatement(cuda, [stream], chunk=chunk)
    _same(feats[:, CAUSAL], stream["reference"].astype(np.float32)[:, CAUSAL])
    _same(feats[:, CAUSAL], offline[:, CAUSAL])
    _same(feats[:, 0:2], feats[:, 2:4])
    _same(final_columns(_export(state), stream["object_id"]).astype(np.float32), offline[:, 0:2])
    assert not dropped.any() and state.counters() == dict(objects=36, taken=376, dropped=0, late=0)


# ---- 2. run lengths and carries ---------------------------------------------------------------------------------------
def test_run_lengths_one_batch(cuda, run_lengths):
    whole, _, _, offline = run_lengths
    state, _, feats, dropped = _against_restatement(cuda, [whole])
    _same(feats[:, CAUSAL], offline[:, CAUSAL])
    got = _export(state)
    assert sorted(got["n_alerts"]) == sorted(SIZES) and not dropped.any() and state.counters()["late"] == 0
    _same(final_columns(got, whole["object_id"]).astype(np.float32), offline[:, 0:2])


def test_run_lengths_carried_through_the_slot(cuda, run_lengths):
    whole, halves, where, offline = run_lengths
    state, _, feats, _ = _against_restatement(cuda, halves)
    _same(feats[:, CAUSAL], offline[where][:, CAUSAL])
    got = _export(state)
    assert sorted(got["n_alerts"]) == sorted(SIZES) and state.counters()["late"] == 0
    _same(final_columns(got, whole["object_id"]).astype(np.float32), offline[:, 0:2])


# ---- 3. ties ------------------------------------------------------------------------------------------------------------
def test_ties(cuda):
    t = T0
    # equal jd inside a batch: input position decides who is "so far"
    #            alert:  0      1      2      3      4      5
    case = _one_object([t + 2, t + 2, t + 0, t + 5, t + 2, t + 9], [18.0, 17.5, 18.0, 17.5, 19.0, 20.25])
    _, _, got, _ = _against_restatement(cuda, [case])
    _same(got[:, CAUSAL], restate(*(case[k] for k in NAMES)).astype(np.float32)[:, CAUSAL])
    assert list(got[:, 2]) == [18.0, 17.5, 18.0, 17.5, 17.5, 17.5] and list(got[:, 3]) == [18.0, 18.0, 18.0, 19.0, 19.0, 20.25]
    assert list(got[:, 5]) == [2.0, 0.0, 0.0, 3.0, 0.0, 7.0]             # 3 ties 1's minimum: the earlier epoch stays
    # equal jd across two batches: arrival decides
    for mags, so_far, since in (((18.2, 18.1), [18.2, 18.1], [0.0, 0.0]), ((18.1, 18.2), [18.1, 18.1], [0.0, 0.0])):
        both = _one_object([t + 1, t + 1], mags)
        parts = [{k: v[:1] for k, v in both.items()}, {k: v[1:] for k, v in both.items()}]
        state, _, got, _ = _against_restatement(cuda, parts)
        _same(got[:, CAUSAL], restate(*(both[k] for k in NAMES)).astype(np.float32)[:, CAUSAL])
        assert list(got[:, 2]) == [np.float32(m) for m in so_far] and list(got[:, 5]) == since
        assert state.counters()["late"] == 0
    # the same magpsf at two epochs: days_since_peak counts from the earlier one, in one batch and across two
    twice = _one_object([t + 3, t, t + 5], [17.5, 17.5, 18.0])
    for parts in ([twice], [{k: v[1:2] for k, v in twice.items()}, {k: v[[0, 2]] for k, v in twice.items()}]):
        state, _, got, _ = _against_restatement(cuda, parts)
        by_jd = got[np.argsort(np.concatenate([p["jd"] for p in parts]))]
        assert list(by_jd[:, 5]) == [0.0, 3.0, 5.0] and list(by_jd[:, 6]) == [1.0, 1.0, 1.0]
        assert _export(state)["peak_jd"][0] == t
    # 130 alerts at 10 epochs: one batch; and the time-sorted stream cut inside an epoch and inside a 64-alert step
    rng = np.random.default_rng(5)
    case = _one_object(t + rng.integers(0, 10, 130).astype(np.float64), 18 + rng.integers(0, 6, 130) * 0.5)
    assert len(np.unique(case["jd"])) == 10
    want = restate(*(case[k] for k in NAMES)).astype(np.float32)
    _, _, got, _ = _against_restatement(cuda, [case])
    _same(got[:, CAUSAL], want[:, CAUSAL])
    order = np.argsort(case["jd"], kind="stable")
    srt = {k: v[order] for k, v in case.items()}
    assert srt["jd"][69] == srt["jd"][70]
    for chunk in (70, 33):
        state, _, got, _ = _against_restatement(cuda, [srt], chunk=chunk)
        _same(got[:, CAUSAL], want[order][:, CAUSAL])
        assert state.counters()["late"] == 0


# ---- 4. NaNs ------------------------------------------------------------------------------------------------------------
def test_nans(cuda):
    nan = np.nan
    t = T0

    def named(case, oid):
        return dict(case, object_id=np.full(len(case["jd"]), oid, dtype=np.int64))

    mid = named(_one_object([t, t + 1, t + 2, t + 3], [19.0, nan, 18.0, 18.5]), 7)
    first = named(_one_object([t + 1, t, t + 2], [18.0, nan, 19.0]), 9)               # the NaN is the earliest alert
    allnan = named(_one_object([t, t + 1], [nan, nan]), 8)
    jsh = named(_one_object([t, t + 1, t + 2], [19.0, 18.0, 18.5], jsh=[t - 1, nan, t - 1]), 10)
    big = _objects([70, 300], seed=3)
    big["magpsf"][::7] = nan
    big["jdstarthist"][::11] = nan
    case = _cat([mid, first, allnan, jsh, big])
    want = restate(*(case[k] for k in NAMES)).astype(np.float32)
    order = np.argsort(case["jd"], kind="stable")
    srt = {k: v[order] for k, v in case.items()}
    for rows, chunk, back in ((case, None, np.arange(len(order))), (srt, 1, order), (srt, 50, order)):
        state, _, got, _ = _against_restatement(cuda, [rows], chunk=chunk)
        _same(got[:, CAUSAL], want[back][:, CAUSAL])
        oid = rows["object_id"]
        by_jd = lambda k: got[oid == k][np.argsort(rows["jd"][oid == k])]     # noqa: E731
        assert list(by_jd(7)[:, 2]) == [19.0, 19.0, 18.0, 18.0] and list(by_jd(7)[:, 5]) == [0.0, 1.0, 0.0, 1.0]
        assert np.isnan(by_jd(9)[0, [0, 1, 2, 3, 5, 6]]).all() and by_jd(9)[0, 4] == 1.0 and not np.isnan(by_jd(9)[1:]).any()
        assert np.isnan(by_jd(8)[:, [0, 1, 2, 3, 5, 6]]).all() and list(by_jd(8)[:, 4]) == [1.0, 2.0]
        assert list(by_jd(8)[:, 7]) == [6.0, 7.0]
        assert np.isnan(by_jd(10)[1, [4, 6]]).all() and by_jd(10)[1, 5] == 0.0 and not np.isnan(by_jd(10)[[0, 2]]).any()
        exported = _export(state)
        k8 = int(np.searchsorted(exported["object_id"], 8))
        assert np.isnan([exported[f][k8] for f in ("peakmag", "peak_jd", "maxmag")]).all() and exported["n_alerts"][k8] == 2


# ---- 5. a full table ----------------------------------------------------------------------------------------------------
def test_full_table_drops_new_objects_only(cuda):
    rng = np.random.default_rng(23)
    ids = rng.choice(np.arange(-5000, 5000, dtype=np.int64) * 7919, 296, replace=False)
    old, new = ids[:256], ids[256:]
    b1 = _batch(np.repeat(old, rng.integers(1, 4, len(old))), T0, rng)
    again = np.concatenate([new, old[100:150]])
    b2 = _batch(np.repeat(again, rng.integers(1, 4, len(again))), T0 + 10, rng)
    state, host, feats, dropped = _against_restatement(cuda, [b1, b2], capacity=256)
    d1, d2 = dropped[:len(b1["jd"])], dropped[len(b1["jd"]):]
    is_new = np.isin(b2["object_id"], new)
    assert not d1.any() and np.array_equal(d2, is_new) and 0 < is_new.sum() < len(is_new)
    f2 = feats[len(b1["jd"]):]
    assert np.isnan(f2[is_new]).all() and not np.isnan(f2[~is_new]).any()
    assert state.counters() == dict(objects=256, taken=len(b1["jd"]) + int((~is_new).sum()), dropped=int(is_new.sum()), late=0)
    # ... which is the restatement run on the alerts that were kept
    plain = FeatureStreamRestatement()
    p1, _ = _host_feed(plain, b1)
    p2, _ = _host_feed(plain, {k: v[~is_new] for k, v in b2.items()})
    _same(feats[:len(b1["jd"])], p1)
    _same(f2[~is_new], p2)
    got = _export(state)
    _same(got, plain.export(), EXPORTED)
    assert len(got["object_id"]) == 256 and got["n_alerts"].sum() == len(b1["jd"]) + (~is_new).sum()


# ---- 6. awkward ids -----------------------------------------------------------------------------------------------------
def test_awkward_ids(cuda):
    cap = 64
    i64 = np.iinfo(np.int64)
    ids = np.array([0, cap, 2 * cap, 3 * cap, 17 * cap, -cap, 1 << 40, -1, -2, -123456789012345, i64.max, i64.min + 1,
                    5, 5 + (1 << 32), 5 + (1 << 33), 5 + (1 << 62), 5 - (1 << 63) + (1 << 32), i64.max - 1], dtype=np.int64)
    assert len(np.unique(ids)) == len(ids) and RESERVED_ID not in ids
    rng = np.random.default_rng(2)
    batches = [_batch(np.repeat(ids, 2), t0, rng, reserved=3) for t0 in (T0, T0 + 10)]
    state, _, feats, dropped = _against_restatement(cuda, batches, capacity=cap)
    assert np.array_equal(dropped, np.concatenate([b["object_id"] for b in batches]) == RESERVED_ID)
    assert np.isnan(feats[dropped]).all() and not np.isnan(feats[~dropped]).any()
    assert state.counters() == dict(objects=len(ids), taken=4 * len(ids), dropped=6, late=0)      # found again, not re-made
    got = _export(state)
    assert np.array_equal(got["object_id"], np.sort(ids)) and (got["n_alerts"] == 4).all()


# ---- 7. arrival order ---------------------------------------------------------------------------------------------------
def test_arrival_order_is_kept(cuda, golden_stream):
    _, shuffled, _ = golden_stream
    want = shuffled["reference"].astype(np.float32)
    state, host, feats, _ = _against_restatement(cuda, [shuffled], chunk=64)
    assert state.counters()["late"] == host.late > 0
    assert same_arrays({"rows": feats[:, CAUSAL]}, {"rows": want[:, CAUSAL]}, ("rows",)) is not None    # not the offline result
    # the whole shuffled fixture as ONE batch is sorted inside the batch: the offline result
    one, _, feats, _ = _against_restatement(cuda, [shuffled])
    _same(feats[:, CAUSAL], want[:, CAUSAL])
    assert one.counters() == dict(objects=36, taken=376, dropped=0, late=0)


# ---- 8. export / load ---------------------------------------------------------------------------------------------------
def test_export_and_load(cuda, golden_stream):
    from btsbot_amd import FeatureState
    stream, _, offline = golden_stream
    half = len(stream["jd"]) // 2
    parts = [{k: v[:half] for k, v in stream.items()}, {k: v[half:] for k, v in stream.items()}]
    whole = _state(cuda)
    _feed(whole, cuda, stream, 257)
    first = _state(cuda)
    f1, _ = _feed(first, cuda, parts[0], 257)
    records = first.export()
    moved = FeatureState.from_export(records, capacity=1024, device=cuda)
    assert moved.capacity == 1024 and moved.counters() == dict(objects=len(records["object_id"]), taken=0, dropped=0, late=0)
    _same(_export(moved), {k: v.cpu().numpy() for k, v in records.items()}, EXPORTED)
    f2, _ = _feed(moved, cuda, parts[1], 257)
    _same(_export(moved), _export(whole), EXPORTED)
    _same(np.concatenate([f1, f2])[:, CAUSAL], offline[:, CAUSAL])
    # numpy records load too; an id twice, the reserved id and too small a table raise
    as_numpy = {k: v.cpu().numpy() for k, v in records.items()}
    _same(_export(FeatureState.from_export(as_numpy, capacity=256, device=cuda)), as_numpy, EXPORTED)
    twice = {k: np.concatenate([v, v[3:4]]) for k, v in as_numpy.items()}
    with pytest.raises(ValueError, match="came before"):
        FeatureState.from_export(twice, capacity=1024, device=cuda)
    reserved = {k: v.copy() for k, v in as_numpy.items()}
    reserved["object_id"][0] = RESERVED_ID
    with pytest.raises(ValueError, match="no slot"):
        FeatureState.from_export(reserved, capacity=1024, device=cuda)
    with pytest.raises(ValueError, match="no slot"):
        FeatureState.from_export(as_numpy, capacity=16, device=cuda)
    with pytest.raises(ValueError, match="lack"):
        FeatureState.from_export({k: v for k, v in as_numpy.items() if k != "peak_jd"}, capacity=256, device=cuda)
    with pytest.raises(ValueError, match="n_alerts"):
        FeatureState.from_export(dict(as_numpy, n_alerts=as_numpy["n_alerts"][:3]), capacity=256, device=cuda)


# ---- 9. the empty batch, streams, reset, argument checks ----------------------------------------------------------------
def test_empty_batch_streams_and_reset(cuda, golden_stream):
    stream, _, offline = golden_stream
    host = FeatureStreamRestatement()
    _host_feed(host, stream)
    want = host.export()
    state = _state(cuda)
    e = torch.zeros(0, device=cuda)
    empty = (e.long(), e.double(), e.double(), e.double(), e.int(), e.int())
    out = state.update(*empty)
    assert tuple(out["features"].shape) == (0, 8) and tuple(out["dropped"].shape) == (0,)
    assert state.counters() == dict(objects=0, taken=0, dropped=0, late=0) and _export(state)["object_id"].size == 0
    args = _args(cuda, stream)
    torch.cuda.synchronize(cuda)
    side = torch.cuda.Stream(cuda)
    with torch.cuda.stream(side):
        feats = state.update(*args)["features"]
        state.update(*empty)                                                # a no-op in the middle of a stream
    torch.cuda.current_stream(cuda).wait_stream(side)
    _same(feats.cpu().numpy()[:, CAUSAL], offline[:, CAUSAL])
    _same(_export(state), want, EXPORTED)
    state.reset()
    assert state.counters() == dict(objects=0, taken=0, dropped=0, late=0) and _export(state)["object_id"].size == 0
    _feed(state, cuda, stream, 257)
    _same(_export(state), want, EXPORTED)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        state.update(*(a.cpu() for a in args))
    with pytest.raises(ValueError):
        state.update(args[0], args[1][:3], *args[2:])                       # lengths
    with pytest.raises(ValueError):
        state.update(*args[:5], args[5][:3])
    with pytest.raises(ValueError):
        state.update(args[1], *args[1:])                                    # float ids
    with pytest.raises(ValueError):
        state.update(args[0].cpu().numpy(), *args[1:])                      # not a tensor
    _same(_export(state), want, EXPORTED)                                   # a refused call changes nothing
    assert state.counters() == dict(objects=36, taken=376, dropped=0, late=0)


# ---- 10. packets ------------------------------------------------------------------------------------------------------
def test_make_metadata_with_a_state(cuda):
    """Packets of three objects in two calls, the earlier epochs first: the six causal custom columns equal those of one
    stateless call over all packets; without a state the output is what it was (the host assembly from the offline
    restatement)."""
    from btsbot_amd import alert_utils
    rng = np.random.default_rng(12)
    names = ["ZTF23abhvlji", "ZTF23abdsfms", "ATLAS23xyz"]
    obj = rng.integers(0, 3, 24)
    obj[:3] = np.arange(3)
    jd = np.sort(2459200.5 + rng.uniform(0, 30, 24))
    packets = [{"objectId": names[obj[k]],
                "candidate": {"jd": float(jd[k]), "magpsf": float(np.round(rng.uniform(17, 20), 1)),
                              "jdstarthist": 2459199.0 + float(rng.uniform(0, 4)), "ndethist": int(rng.integers(1, 20)),
                              "ncovhist": int(rng.integers(20, 500)), "fwhm": float(rng.uniform(1, 4))},
                "classifications": {"sgscore1": float(rng.uniform(0, 1))}} for k in range(24)]
    packets[5]["candidate"]["magpsf"] = None
    causal = ["peakmag_so_far", "maxmag_so_far", "age", "days_since_peak", "days_to_peak", "nnotdet"]
    cols = ["sgscore1", "age", "peakmag", "days_to_peak", "fwhm", "nnotdet", "maxmag_so_far", "days_since_peak", "maxmag",
            "peakmag_so_far"]
    whole = alert_utils.make_metadata(packets, cols, device=cuda).cpu().numpy()
    # without a state: unchanged
    rows = [p["candidate"] | p["classifications"] for p in packets]
    num = lambda c: np.array([np.nan if r[c] is None else r[c] for r in rows], dtype=np.float64)      # noqa: E731
    feats = restate(obj, *(num(c) for c in NAMES[1:]))
    host = np.stack([feats[:, alert_utils.CUSTOM_COLS.index(c)] if c in alert_utils.CUSTOM_COLS else num(c) for c in cols],
                    axis=1).astype(np.float32)
    _same(whole, host)
    # with one: two calls continue the light curves
    state = _state(cuda)
    got = torch.cat([alert_utils.make_metadata(packets[:10], cols, device=cuda, state=state),
                     alert_utils.make_metadata(packets[10:], cols, device=cuda, state=state)]).cpu().numpy()
    keep = [cols.index(c) for c in causal + ["sgscore1", "fwhm"]]
    _same(got[:, keep], whole[:, keep])
    _same(got[:, cols.index("peakmag")], got[:, cols.index("peakmag_so_far")])
    _same(got[:, cols.index("maxmag")], got[:, cols.index("maxmag_so_far")])
    assert (got[:, cols.index("peakmag")] != whole[:, cols.index("peakmag")]).any()
    assert state.counters() == dict(objects=3, taken=24, dropped=0, late=0)
    exported = _export(state)
    assert sorted(exported["object_id"]) == sorted(alert_utils.object_keys(names).tolist())
    # two stateless calls do NOT: the second starts every light curve again
    apart = torch.cat([alert_utils.make_metadata(packets[:10], cols, device=cuda),
                       alert_utils.make_metadata(packets[10:], cols, device=cuda)]).cpu().numpy()
    assert same_arrays({"rows": apart[:, keep]}, {"rows": whole[:, keep]}, ("rows",)) is not None
    # a full table: the dropped rows carry NaN in the custom columns, the packet fields stay
    tiny = _state(cuda, capacity=2)
    full = alert_utils.make_metadata(packets, cols, device=cuda, state=tiny).cpu().numpy()
    custom = [k for k, c in enumerate(cols) if c in alert_utils.CUSTOM_COLS]
    lost = np.isnan(full[:, cols.index("nnotdet")])
    assert tiny.counters()["objects"] == 2 and tiny.counters()["dropped"] == lost.sum() > 0
    assert len(set(obj[lost])) == 1 and np.isnan(full[lost][:, custom]).all()
    _same(full[:, [cols.index("sgscore1"), cols.index("fwhm")]], whole[:, [cols.index("sgscore1"), cols.index("fwhm")]])
    _same(full[~lost][:, keep], whole[~lost][:, keep])
