"""Retention on the device (ObjectState.expire / resize / n_expired; btsbot_trigger_rehash, btsbot_feature_rehash) for
btsbot_amd.TriggerState and btsbot_amd.FeatureState against the host model of tests/test_retention_host.py: the
restatements with an ``expire`` that deletes the objects whose last_jd < before_jd.  A rehash copies records and counts
objects, so every comparison is exact, NaN positions included."""
import numpy as np
import pytest
import torch

from test_feature_state_host import EXPORTED as FEATURE_EXPORTED
from test_feature_state_host import NAMES, SHARED_CAPACITY, SHARED_EXPORT, TRIGGER_NAMES, golden_rows, shared_batches
from test_policy_host import REFERENCE_POLICIES
from test_retention_host import SHARED_EXPIRE_AFTER, RetainingFeatures, RetainingTriggers, shared_cut
from test_trigger_host import EXPORTED as TRIGGER_EXPORTED
from test_trigger_host import same_arrays

pytestmark = pytest.mark.gpu

T0 = 2459300.5
SWEEP16 = {f"t{i}": (0.05 + 0.055 * i, 19.0, 1 + i % 3, None if i % 2 else 18.5) for i in range(16)}


class Kind:
    """One of the two states with its host model: how to make both, which columns update() takes, what it returns."""

    def __init__(self, name, names, exported, out, policies=None):
        self.name, self.names, self.exported, self.out, self.policies = name, names, exported, out, policies

    def __repr__(self):
        return self.name

    def state(self, cuda, capacity):
        from btsbot_amd import FeatureState, TriggerState
        return FeatureState(capacity, cuda) if self.policies is None else TriggerState(self.policies, capacity, cuda)

    def model(self, capacity=None):
        return RetainingFeatures(capacity) if self.policies is None else RetainingTriggers(self.policies, capacity)

    def from_export(self, cuda, records, capacity):
        from btsbot_amd import FeatureState, TriggerState
        if self.policies is None:
            return FeatureState.from_export(records, capacity=capacity, device=cuda)
        return TriggerState.from_export(records, self.policies, capacity=capacity, device=cuda)

    def update(self, state, cuda, rows):
        """-> (the per-alert output, dropped) of one update() as numpy."""
        out = state.update(*(torch.from_numpy(np.ascontiguousarray(rows[k])).to(cuda) for k in self.names))
        return out[self.out].cpu().numpy().astype(np.uint8 if self.out == "fired" else np.float32), out["dropped"].cpu().numpy()

    def model_update(self, model, rows):
        out, dropped = model.update(*(rows[k] for k in self.names))
        return out.astype(np.uint8 if self.out == "fired" else np.float32), dropped


TRIGGERS = Kind("triggers", TRIGGER_NAMES, TRIGGER_EXPORTED, "fired", REFERENCE_POLICIES)
FEATURES = Kind("features", NAMES, FEATURE_EXPORTED, "features")
TRIGGERS16 = Kind("triggers16", TRIGGER_NAMES, TRIGGER_EXPORTED, "fired", SWEEP16)
BOTH = (TRIGGERS, FEATURES)


def _export(state):
    return {k: v.cpu().numpy() for k, v in state.export().items()}


def _same(got, want, keys):
    diff = same_arrays(got, want, keys)
    assert diff is None, diff


def _rows(ids, jd, rng, mag=None, score=None):
    """Alerts with the columns of both states' update(); magnitudes and scores drawn unless given."""
    n = len(ids)
    ndet = rng.integers(1, 50, n).astype(np.int32)
    return dict(object_id=np.asarray(ids, dtype=np.int64), jd=np.asarray(jd, dtype=np.float64),
                magpsf=np.round(rng.uniform(17.5, 20.5, n), 2) if mag is None else np.full(n, mag, dtype=np.float64),
                jdstarthist=np.full(n, T0 - 10.0), ndethist=ndet, ncovhist=(ndet + rng.integers(0, 2000, n)).astype(np.int32),
                raw_preds=(rng.uniform(0, 1, n) if score is None else np.full(n, score)).astype(np.float32))


def _step(kind, state, model, cuda, rows):
    """One batch into the state and the model; the per-alert outputs must agree.  -> dropped."""
    out, dropped = kind.update(state, cuda, rows)
    want, want_dropped = kind.model_update(model, rows)
    _same({"out": out}, {"out": want}, ("out",))
    assert np.array_equal(dropped, want_dropped)
    return dropped


def _agree(kind, state, model):
    got = _export(state)
    _same(got, model.export(), kind.exported)
    assert state.counters() == model.counters() and state.n_expired() == model.expired
    return got


def _filtered(records, keep):
    return {k: v[keep] for k, v in records.items()}


# ---- 1. a stream with an expire in the middle ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def retention_stream():
    """The recorded fixture (36 objects, 376 alerts) as a time-ordered stream, with scores for the trigger state (seeded:
    the fixture records none).  In the fixture no object that has gone quiet by the middle of the stream is seen again
    (no cut gives an object that returns), so three synthetic alerts for each of the two objects that end first are
    appended after the fixture's last alert: they come back as new objects."""
    stream, _ = golden_rows()
    rows = {k: stream[k] for k in NAMES}
    ids = np.unique(rows["object_id"])
    ends = np.array([rows["jd"][rows["object_id"] == o].max() for o in ids])
    back = ids[np.argsort(ends)[:2]]
    rng = np.random.default_rng(7)
    extra = _rows(np.repeat(back, 3), rows["jd"].max() + 1.0 + np.arange(6.0), rng)
    rows = {k: np.concatenate([rows[k], extra[k].astype(rows[k].dtype)]) for k in NAMES}
    rows["raw_preds"] = rng.uniform(0, 1, len(rows["jd"])).astype(np.float32)
    assert len(rows["jd"]) == 382 and (np.diff(rows["jd"]) >= 0).all()
    return rows, back


def _cut_of(stream, upto):
    """The median last_jd of the objects held after stream[:upto], from the host model."""
    host = RetainingFeatures()
    host.update(*(stream[k][:upto] for k in NAMES))
    return float(np.median([o["last_jd"] for o in host.objects.values()]))


@pytest.mark.parametrize("capacity", (64, 1024))
@pytest.mark.parametrize("chunk", (7, 64))
@pytest.mark.parametrize("kind", BOTH, ids=repr)
def test_stream_with_an_expire_in_the_middle(cuda, retention_stream, kind, chunk, capacity):
    stream, back = retention_stream
    n = len(stream["jd"])
    starts = list(range(0, n, chunk))
    middle = starts[len(starts) // 2]
    cut = _cut_of(stream, middle + chunk)
    state, model = kind.state(cuda, capacity), kind.model(capacity)
    for s in starts:
        dropped = _step(kind, state, model, cuda, {k: v[s:s + chunk] for k, v in stream.items()})
        assert not dropped.any()
        if s == middle:
            held = len(model.objects)
            assert state.expire(cut) is None
            gone = model.expire(cut)
            assert 4 * len(gone) >= held and 4 * (held - len(gone)) >= held                # a quarter goes, a quarter stays
            assert set(back) <= set(gone) and set(back) <= set(stream["object_id"][s + chunk:])   # ... and two come back
            _agree(kind, state, model)
    got = _agree(kind, state, model)
    assert state.n_expired() == len(gone) and state.counters()["taken"] == n
    at = {int(o): k for k, o in enumerate(got["object_id"])}
    assert [int(got["n_alerts"][at[int(o)]]) for o in back] == [3, 3]                     # made afresh


# ---- 2. (and 8.) a probe chain that wraps round the end of the table --------------------------------------------------
def mix64(x):
    """csrc/object_table.h's hash (splitmix64's finaliser), restated."""
    m = (1 << 64) - 1
    x &= m
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & m
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & m
    return x ^ (x >> 31)


def chain_ids(capacity=16, home=14, n=6):
    ids = [i for i in range(1, 4000) if mix64(i) & (capacity - 1) == home][:n]
    assert len(ids) == n
    return ids


@pytest.mark.parametrize("kind", (TRIGGERS, FEATURES, TRIGGERS16), ids=repr)
def test_probe_chain_with_wrap_around(cuda, kind):
    """Six objects whose home slot is 14 of 16 sit in slots 14, 15, 0, 1, 2, 3; the first and the third go.  A delete in
    place that leaves holes at 14 and 0 loses the four behind them: they would be made afresh.  With 16 policies (some
    fired before the expire, some not) every count and trigger pair has to come through.  Every score is 0.6 and every
    magnitude at most 18.5: a policy with thr < 0.6 fires on an object as soon as it has k alerts, the others never."""
    ids = chain_ids()
    rng = np.random.default_rng(11)
    state, model = kind.state(cuda, 16), kind.model(16)
    for k, oid in enumerate(ids):                                    # one after the other: the chain is in this order
        _step(kind, state, model, cuda, _rows([oid], [T0 + k], rng, 18.0 + 0.1 * k, 0.6))
    assert state._key.cpu().tolist()[14:] + state._key.cpu().tolist()[:4] == ids           # the chain does wrap
    _step(kind, state, model, cuda, _rows([ids[1]], [T0 + 10], rng, 18.2, 0.6))                  # the second is seen again
    before = model.export()
    if kind.policies is not None:
        assert 0 < before["pred"].sum() < before["pred"].size and before["count"].max() >= 2
    cut = T0 + 2.5
    state.expire(cut)
    assert model.expire(cut) == sorted([ids[0], ids[2]])
    got = _agree(kind, state, model)
    keep = ~np.isin(before["object_id"], [ids[0], ids[2]])
    _same(got, _filtered(before, keep), kind.exported)
    dropped = _step(kind, state, model, cuda, _rows(ids, T0 + 20 + np.arange(6.0), rng, 18.4, 0.6))
    assert not dropped.any()
    got = _agree(kind, state, model)
    by_id = dict(zip(got["object_id"].tolist(), got["n_alerts"].tolist()))
    assert [by_id[i] for i in ids] == [1, 3, 1, 2, 2, 2]              # survivors go on, the two removed are new objects
    assert state.counters()["objects"] == 6 and state.n_expired() == 2


# ---- 3. a full table opens up -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BOTH, ids=repr)
def test_a_full_table_opens_up(cuda, kind):
    rng = np.random.default_rng(13)
    state, model = kind.state(cuda, 8), kind.model(8)
    ids = np.arange(8, dtype=np.int64) * 7919 - 20000
    _step(kind, state, model, cuda, _rows(ids, T0 + np.arange(8.0), rng))
    assert _step(kind, state, model, cuda, _rows([99], [T0 + 8], rng)).all()               # the ninth is dropped
    assert state.counters() == dict(objects=8, taken=8, dropped=1, late=0)
    state.expire(T0 + 2.5)
    assert len(model.expire(T0 + 2.5)) == 3
    _agree(kind, state, model)
    flags = [bool(_step(kind, state, model, cuda, _rows([oid], [T0 + 9 + k], rng))[0])     # one by one: which three are
             for k, oid in enumerate((100, 101, 102, 103))]                                # held is then not a race
    assert flags == [False, False, False, True]
    _agree(kind, state, model)
    assert state.counters() == dict(objects=8, taken=11, dropped=2, late=0) and state.n_expired() == 3


# ---- 4. edges -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shared():
    return shared_batches(), shared_cut()


@pytest.mark.parametrize("kind", BOTH, ids=repr)
def test_edges(cuda, shared, kind):
    state = kind.state(cuda, SHARED_CAPACITY)
    state.expire(T0)
    assert _export(state)["object_id"].size == 0 and state.n_expired() == 0               # empty stays empty
    assert state.counters() == dict(objects=0, taken=0, dropped=0, late=0)
    model = kind.model(SHARED_CAPACITY)
    for b in shared[0]:
        _step(kind, state, model, cuda, b)
    before, counters = _export(state), state.counters()
    assert counters["objects"] == SHARED_CAPACITY and counters["dropped"] > 0 and counters["late"] > 0
    for nothing in (float("-inf"), float("nan")):
        state.expire(nothing)
        _same(_export(state), before, kind.exported)
        assert state.counters() == counters and state.n_expired() == 0
    state.expire(float("inf"))
    assert _export(state)["object_id"].size == 0 and state.n_expired() == SHARED_CAPACITY
    assert state.counters() == dict(counters, objects=0)
    # a loaded record whose last_jd is NaN survives every cut
    records = {k: v.copy() for k, v in before.items()}
    records["last_jd"][2] = np.nan
    loaded = kind.from_export(cuda, records, 16)
    for cut in (float("-inf"), T0, 1e9, float("inf")):
        loaded.expire(cut)
        assert records["object_id"][2] in _export(loaded)["object_id"]
    _same(_export(loaded), _filtered(records, np.arange(SHARED_CAPACITY) == 2), kind.exported)
    assert loaded.n_expired() == SHARED_CAPACITY - 1 and loaded.counters()["objects"] == 1


# ---- 5. return_expired --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BOTH, ids=repr)
def test_return_expired_and_the_rest_are_the_old_export(cuda, shared, kind):
    batches, cut = shared
    state = kind.state(cuda, SHARED_CAPACITY)
    for b in batches[:SHARED_EXPIRE_AFTER + 1]:
        kind.update(state, cuda, b)
    before, live = _export(state), state.export()
    gone = state.expire(cut, return_expired=True)
    assert tuple(gone) == kind.exported and all(v.device.type == "cuda" for v in gone.values())
    assert all(gone[k].dtype == live[k].dtype and gone[k].shape[1:] == live[k].shape[1:] for k in kind.exported)
    gone, after = {k: v.cpu().numpy() for k, v in gone.items()}, _export(state)
    is_gone = before["last_jd"] < cut
    assert 0 < is_gone.sum() < len(is_gone)
    _same(gone, _filtered(before, is_gone), kind.exported)
    _same(after, _filtered(before, ~is_gone), kind.exported)
    assert state.n_expired() == is_gone.sum()
    none = state.expire(float("-inf"), return_expired=True)
    assert tuple(none) == kind.exported and all(v.shape[0] == 0 for v in none.values())


# ---- 6. resize ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BOTH, ids=repr)
def test_resize(cuda, shared, kind):
    batches, _ = shared
    # growing: the objects a full table was dropping find slots
    state, model = kind.state(cuda, SHARED_CAPACITY), kind.model(SHARED_CAPACITY)
    for b in batches[:4]:
        _step(kind, state, model, cuda, b)
    before, counters = _export(state), state.counters()
    assert counters["dropped"] > 2
    state.resize(64)
    model.capacity = 64
    assert state.capacity == 64 and state.counters() == counters and state.n_expired() == 0
    _same(_export(state), before, kind.exported)
    dropped = _step(kind, state, model, cuda, batches[4])
    assert not dropped.any() and state.counters()["objects"] == SHARED_CAPACITY + 1
    _agree(kind, state, model)
    # shrinking: nine objects do not fit eight slots, and the state is as it was
    before, counters = _export(state), state.counters()
    with pytest.raises(ValueError, match="1 objects found no slot"):
        state.resize(8)
    assert state.capacity == 64 and state.counters() == counters and state.n_expired() == 0
    _same(_export(state), before, kind.exported)
    rng = np.random.default_rng(19)
    _step(kind, state, model, cuda, _rows([3001, 1000], [T0 + 500, T0 + 501], rng))
    before = _agree(kind, state, model)
    assert len(before["object_id"]) == 10
    # ... but eight of them do
    cut = float(np.sort(before["last_jd"])[2])
    state.resize(8, cut)
    assert len(model.expire(cut)) == 2
    model.capacity = 8
    assert state.capacity == 8 and state.n_expired() == 2
    _same(_agree(kind, state, model), _filtered(before, before["last_jd"] >= cut), kind.exported)
    assert _step(kind, state, model, cuda, _rows([4000], [T0 + 502], rng)).all()           # full again
    _agree(kind, state, model)


# ---- 7. more slots than threads -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BOTH, ids=repr)
def test_more_slots_than_threads(cuda, kind):
    """2^21 slots: the sweep's grid is capped at 2^20 threads, so every thread takes two slots."""
    rng = np.random.default_rng(23)
    n = 5000
    ids = rng.choice(np.arange(-(1 << 40), 1 << 40, 1 << 20, dtype=np.int64), n, replace=False) + rng.integers(0, 1 << 20, n)
    state = kind.state(cuda, 1 << 21)
    _, dropped = kind.update(state, cuda, _rows(ids, T0 + rng.permutation(n).astype(np.float64), rng))
    assert not dropped.any()
    before = _export(state)
    assert len(before["object_id"]) == n
    state.expire(T0 + n / 2)
    keep = before["last_jd"] >= T0 + n / 2
    assert keep.sum() == n // 2
    _same(_export(state), _filtered(before, keep), kind.exported)
    assert state.counters() == dict(objects=n // 2, taken=n, dropped=0, late=0) and state.n_expired() == n - n // 2


# ---- 9. the two states agree --------------------------------------------------------------------------------------------
def test_trigger_and_feature_state_agree_across_an_expire(cuda, shared):
    batches, cut = shared
    trig, feat = TRIGGERS.state(cuda, SHARED_CAPACITY), FEATURES.state(cuda, SHARED_CAPACITY)
    host = RetainingFeatures(capacity=SHARED_CAPACITY)
    for k, b in enumerate(batches):
        cols = {name: torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for name, v in b.items()}
        td = trig.update(*(cols[name] for name in TRIGGER_NAMES))["dropped"]
        fd = feat.update(*(cols[name] for name in NAMES))["dropped"]
        _, hd = host.update(*(b[name] for name in NAMES))
        if k == SHARED_EXPIRE_AFTER:
            trig.expire(cut)
            feat.expire(cut)
            assert len(host.expire(cut)) == 5
        assert torch.equal(td, fd) and np.array_equal(fd.cpu().numpy(), hd)
        assert trig.counters() == feat.counters() == host.counters()
        assert trig.n_expired() == feat.n_expired() == host.expired
        _same(_export(trig), _export(feat), SHARED_EXPORT)
        _same(_export(feat), host.export(), SHARED_EXPORT)
    assert host.expired > 0 and host.counters()["dropped"] > 0 and host.counters()["late"] > 0


# ---- 10. expire reads nothing on the host -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BOTH, ids=repr)
def test_expire_does_not_synchronise(cuda, shared, kind):
    batches, cut = shared
    state, model = kind.state(cuda, SHARED_CAPACITY), kind.model(SHARED_CAPACITY)
    for b in batches[:SHARED_EXPIRE_AFTER + 1]:
        _step(kind, state, model, cuda, b)
    torch.cuda.synchronize(cuda)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            state.counters()
            control = False
        except RuntimeError:
            control = True                                             # a host read is an error in this mode
        if control:
            state.expire(cut)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not control:
        pytest.skip("this build of torch does not report a host read in sync debug mode: nothing to tell expire() by")
    assert len(model.expire(cut)) > 0
    _agree(kind, state, model)
