"""Streaming light-curve features (btsbot_amd.FeatureState, btsbot_feature_update), host side: a plain numpy restatement
of the streaming rule -- a dict per object, one loop over alerts -- tied to the reference's recorded prep_alerts output
(tests/golden/alert_features.npz): a time-ordered stream cut into batches any way gives columns 2-7 of the recording,
exactly, and the records at the end hold its columns 0-1.  Then the C entry points' and the class's argument checks and
the objectId -> int64 keys, none of which needs a device.  tests/test_gpu_feature_state.py imports the restatement as
its oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_alert_features_host import GOLDEN, restate
from test_trigger_host import CHUNKS, RESERVED_ID, StreamRestatement, same_arrays

NAMES = ("object_id", "jd", "magpsf", "jdstarthist", "ncovhist", "ndethist")
EXPORTED = ("object_id", "n_alerts", "first_jd", "last_jd", "peakmag", "peak_jd", "maxmag")
CAUSAL = slice(2, 8)                       # the columns a stream can know: *_so_far, age, days_*, nnotdet
EXAMPLE_IDS = ("ZTF23abhvlji", "ZTF23abdsfms")     # the two objects of the reference's example candidates table


class FeatureStreamRestatement:
    """The rule of FeatureState.update, one alert at a time.  capacity: objects the state can hold (None: any number);
    which slot an object takes is the table's business, that a new object needs a free one is the rule."""

    def __init__(self, capacity=None):
        self.capacity = capacity
        self.objects = {}
        self.taken = self.dropped = self.late = 0

    def update(self, object_id, jd, magpsf, jdstarthist, ncovhist, ndethist):
        """-> (features float64 [n, 8] before the one rounding to float32, dropped bool [n])."""
        object_id = np.asarray(object_id, dtype=np.int64)
        jd, magpsf, jsh = (np.asarray(x, dtype=np.float64) for x in (jd, magpsf, jdstarthist))
        n = len(jd)
        out, dropped = np.full((n, 8), np.nan, dtype=np.float64), np.zeros(n, dtype=bool)
        # which object comes first does not matter; inside an object: (jd, input position)
        for i in np.lexsort((np.arange(n), jd, object_id)):
            oid = int(object_id[i])
            if oid == RESERVED_ID or (oid not in self.objects and self.capacity is not None
                                      and len(self.objects) >= self.capacity):
                dropped[i] = True
                self.dropped += 1
                continue
            o = self.objects.setdefault(oid, dict(n_alerts=0, first_jd=np.inf, last_jd=-np.inf, peakmag=np.nan,
                                                  peak_jd=np.nan, maxmag=np.nan))
            self.taken += 1
            o["n_alerts"] += 1
            if jd[i] < o["last_jd"]:
                self.late += 1
            o["first_jd"], o["last_jd"] = min(o["first_jd"], jd[i]), max(o["last_jd"], jd[i])
            m = magpsf[i]
            if not np.isnan(m):
                if np.isnan(o["peakmag"]) or m < o["peakmag"] or (m == o["peakmag"] and jd[i] < o["peak_jd"]):
                    o["peakmag"], o["peak_jd"] = m, jd[i]
                if np.isnan(o["maxmag"]) or m > o["maxmag"]:
                    o["maxmag"] = m
            first = np.nan if np.isnan(jsh[i]) else min(jsh[i], o["first_jd"])
            out[i] = (o["peakmag"], o["maxmag"], o["peakmag"], o["maxmag"], jd[i] - first, jd[i] - o["peak_jd"],
                      o["peak_jd"] - first, float(int(ncovhist[i]) - int(ndethist[i])))
        return out, dropped

    def export(self):
        ids = sorted(self.objects)
        rec = [self.objects[k] for k in ids]
        out = dict(object_id=np.array(ids, dtype=np.int64), n_alerts=np.array([r["n_alerts"] for r in rec], dtype=np.int64))
        for k in EXPORTED[2:]:
            out[k] = np.array([r[k] for r in rec], dtype=np.float64)
        return out

    def counters(self):
        return dict(objects=len(self.objects), taken=self.taken, dropped=self.dropped, late=self.late)


def golden_rows():
    """(the fixture's alert rows stably sorted by jd with the reference's rows in the same order, the rows as recorded)."""
    g = dict(np.load(GOLDEN))
    rows = {k: g[k] for k in NAMES}
    rows["reference"] = g["reference"]
    order = np.argsort(rows["jd"], kind="stable")
    return {k: v[order] for k, v in rows.items()}, rows


def stream_in_chunks(state, rows, chunk):
    """Feeds rows chunk by chunk; -> (features, dropped) over all rows."""
    outs = [state.update(*(rows[k][s:s + chunk] for k in NAMES)) for s in range(0, len(rows["jd"]), chunk)]
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


def final_columns(exported, object_id):
    """Columns 0-1 of alert_features over a whole stream, from the records at its end: [n, 2]."""
    at = np.searchsorted(exported["object_id"], object_id)
    return np.stack([exported["peakmag"][at], exported["maxmag"][at]], axis=1)


def _same(got, want):
    diff = same_arrays({"x": got}, {"x": want}, ("x",))
    assert diff is None, diff


@pytest.fixture(scope="module")
def fixture_rows():
    return golden_rows()


@pytest.mark.parametrize("chunk", CHUNKS)
def test_any_chunking_of_a_time_ordered_stream_equals_the_reference(fixture_rows, chunk):
    stream, _ = fixture_rows
    state = FeatureStreamRestatement()
    feats, dropped = stream_in_chunks(state, stream, chunk)
    want = stream["reference"]
    assert feats.dtype == np.float64 and want.dtype == np.float64
    _same(feats[:, CAUSAL], want[:, CAUSAL])
    _same(feats.astype(np.float32)[:, CAUSAL], want.astype(np.float32)[:, CAUSAL])
    _same(feats[:, 0:2], feats[:, 2:4])
    _same(final_columns(state.export(), stream["object_id"]), want[:, 0:2])
    assert not dropped.any() and state.counters() == dict(objects=36, taken=376, dropped=0, late=0)
    assert (feats[:, 0] != want[:, 0]).any() and (feats[:, 1] != want[:, 1]).any()     # columns 0-1 do look at the future


def test_one_shuffled_batch_is_sorted_inside_and_chunks_of_it_are_not(fixture_rows):
    """Inside a batch an object's alerts are taken by (jd, input position), so the whole fixture in its shuffled order as
    ONE batch gives the recorded columns; the same order in chunks of 64 is taken as it arrives: late alerts, another
    result (and the same records wherever the order does not matter)."""
    _, shuffled = fixture_rows
    one = FeatureStreamRestatement()
    feats, _ = one.update(*(shuffled[k] for k in NAMES))
    _same(feats[:, CAUSAL], shuffled["reference"][:, CAUSAL])
    assert one.late == 0
    arrival = FeatureStreamRestatement()
    late_feats, _ = stream_in_chunks(arrival, shuffled, 64)
    assert arrival.late > 0 and arrival.counters()["taken"] == 376
    assert same_arrays({"x": late_feats[:, CAUSAL]}, {"x": shuffled["reference"][:, CAUSAL]}, ("x",)) is not None
    _same(late_feats[:, 7], shuffled["reference"][:, 7])
    got, want = arrival.export(), one.export()
    assert same_arrays(got, want, ("object_id", "n_alerts", "first_jd", "last_jd", "peakmag", "maxmag")) is None


def test_restatement_ties_and_nans_against_the_offline_restatement():
    """Equal jd, equal magnitudes, NaN magpsf and NaN jdstarthist: the time-ordered stream in chunks against
    tests/test_alert_features_host.restate on the whole."""
    rng = np.random.default_rng(4)
    n = 240
    rows = dict(object_id=rng.integers(0, 6, n).astype(np.int64), jd=2459010.5 + rng.integers(0, 25, n).astype(np.float64),
                magpsf=18 + rng.integers(0, 6, n) * 0.5, jdstarthist=2459000.5 + rng.integers(0, 20, n).astype(np.float64),
                ncovhist=rng.integers(50, 900, n).astype(np.int32), ndethist=rng.integers(1, 50, n).astype(np.int32))
    rows["magpsf"][::7] = np.nan
    rows["magpsf"][rows["object_id"] == 5] = np.nan
    rows["jdstarthist"][::11] = np.nan
    order = np.argsort(rows["jd"], kind="stable")
    rows = {k: v[order] for k, v in rows.items()}
    want = restate(*(rows[k] for k in NAMES))
    for chunk in (1, 33, n):
        state = FeatureStreamRestatement()
        feats, _ = stream_in_chunks(state, rows, chunk)
        _same(feats[:, CAUSAL], want[:, CAUSAL])
        _same(final_columns(state.export(), rows["object_id"]), want[:, 0:2])
        assert state.late == 0


def test_full_state_and_reserved_id_drop_alerts():
    t = 2459300.5
    state = FeatureStreamRestatement(capacity=2)
    ids = np.array([5, 6, 7, 5, RESERVED_ID], dtype=np.int64)
    z = np.zeros(5, dtype=np.int32)
    feats, dropped = state.update(ids, t + np.arange(5.0), np.full(5, 18.0), np.full(5, t - 1), z + 9, z + 2)
    assert list(dropped) == [False, False, True, False, True]
    assert state.counters() == dict(objects=2, taken=3, dropped=2, late=0)
    assert np.isnan(feats[dropped]).all() and list(feats[~dropped, 4]) == [1.0, 2.0, 4.0]
    assert list(feats[~dropped, 5]) == [0.0, 0.0, 3.0] and list(feats[~dropped, 7]) == [7.0] * 3


# ---- what TriggerState and FeatureState share: the table, the drop rule, the late rule, the counters -----------------
SHARED_CAPACITY = 8
SHARED_EXPORT = ("object_id", "n_alerts", "last_jd")
TRIGGER_NAMES = ("object_id", "jd", "magpsf", "raw_preds")


def shared_batches():
    """Five batches (the columns of both states' update) that reach every branch the two states share, for a table of
    SHARED_CAPACITY slots and 12 distinct objects:
      0  objects of 1, 63, 64, 65 and 129 alerts (the carry crosses no, one and two 64-alert steps), shuffled, some NaN magpsf
      1  the empty batch
      2  three more objects (the table is full from here on) and two alerts of the reserved id (dropped)
      3  earlier epochs of two held objects, one run of 65: every one late against the slot's last_jd; and four new
         objects, which find no slot (dropped)
      4  70 alerts of a held object shuffled inside, their epochs on both sides of its last_jd: late and timely alerts in one
         step; a new object again (dropped again)"""
    from test_gpu_alert_features import _objects
    rng = np.random.default_rng(41)

    def with_scores(rows):
        rows = {k: rows[k] for k in NAMES}
        rows["raw_preds"] = rng.uniform(0, 1, len(rows["jd"])).astype(np.float32)
        return rows

    def alerts(ids, jd):
        n = len(ids)
        ndet = rng.integers(1, 50, n).astype(np.int32)
        order = rng.permutation(n)
        rows = dict(object_id=np.asarray(ids, dtype=np.int64), jd=np.asarray(jd, dtype=np.float64),
                    magpsf=np.round(rng.uniform(17.5, 20.5, n), 2), jdstarthist=np.full(n, 2458990.5), ndethist=ndet,
                    ncovhist=(ndet + rng.integers(0, 2000, n)).astype(np.int32))
        return with_scores({k: v[order] for k, v in rows.items()})

    first = _objects([1, 63, 64, 65, 129], seed=31)                     # ids 1000, 1007, 1014, 1021, 1028
    first["magpsf"][::9] = np.nan
    held63, held129 = 1007, 1028
    lo = {o: first["jd"][first["object_id"] == o].min() for o in (held63, held129)}
    hi129 = first["jd"][first["object_id"] == held129].max()
    empty = {k: v[:0] for k, v in with_scores(first).items()}
    more = alerts([2000, 2001, 2002, 2000, 2001, 2002, RESERVED_ID, RESERVED_ID], 2459400.5 + rng.uniform(0, 9, 8))
    new = [3000, 3001, 3002, 3003]
    earlier = alerts([held63] * 65 + [held129] * 3 + new * 2,
                     np.concatenate([lo[held63] - rng.uniform(1, 50, 65), lo[held129] - rng.uniform(1, 50, 3),
                                     2459400.5 + rng.uniform(0, 9, 8)]))
    around = alerts([held129] * 70 + [3000], np.concatenate([hi129 + rng.uniform(-30, 30, 70), [2459420.5]]))
    around["magpsf"][::8] = np.nan
    return [with_scores(first), empty, more, earlier, around]


def test_both_restatements_agree_on_what_the_states_share():
    """The batches of tests/test_gpu_object_states.py through both restatements: counters, dropped flags and the exported
    object_id, n_alerts and last_jd agree after every batch, and the batches do reach the branches they are meant to."""
    trig, feat = StreamRestatement(capacity=SHARED_CAPACITY), FeatureStreamRestatement(capacity=SHARED_CAPACITY)
    seen, lates = [], []
    for b in shared_batches():
        _, td = trig.update(*(b[k] for k in TRIGGER_NAMES))
        _, fd = feat.update(*(b[k] for k in NAMES))
        assert np.array_equal(td, fd) and trig.counters() == feat.counters()
        diff = same_arrays(trig.export(), feat.export(), SHARED_EXPORT)
        assert diff is None, diff
        seen.append((len(b["jd"]), int(td.sum()), np.array_equal(td, b["object_id"] == RESERVED_ID)))
        lates.append(trig.late)
    assert seen[0] == (322, 0, True) and seen[1] == (0, 0, True) and seen[2] == (8, 2, True)
    assert seen[3][:2] == (76, 8) and seen[4][:2] == (71, 1)
    assert lates[:3] == [0, 0, 0] and lates[3] == 68 and 0 < lates[4] - lates[3] < 70
    got = trig.counters()
    assert got["objects"] == SHARED_CAPACITY and got["dropped"] == 11 and got["taken"] == 322 + 6 + 68 + 70
    every = np.concatenate([b["object_id"] for b in shared_batches()])
    assert len(np.unique(every)) == 12 + 1 and sorted(trig.export()["n_alerts"]) == [1, 2, 2, 2, 64, 65, 128, 202]
    assert sum(int(np.isnan(b["magpsf"]).sum()) for b in shared_batches()) > 0


# ---- the C entry points, argument checks only (they return before any HIP call) ------------------------------------
TABLE_FIELDS = ("key", "n_alerts", "first_jd", "last_jd", "peak_mag", "peak_jd", "max_mag", "counters")


def _table(capacity=8, null=None):
    from btsbot_amd import _lib
    return _lib.FeatureTable(*(0 if f == null else 0x1000 for f in TABLE_FIELDS), capacity)   # never dereferenced


def _invalid(status):
    from btsbot_amd import _lib
    return status == _lib.ERR_INVALID_ARG and len(_lib.lib().btsbot_last_error()) > 0


def test_the_three_symbols_exist():
    from btsbot_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("btsbot_feature_reset", "btsbot_feature_update", "btsbot_feature_load"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    assert _lib.lib().btsbot_abi_version() == 1


def test_c_entry_points_reject_bad_arguments_before_any_device_call():
    from btsbot_amd import _lib
    L = _lib.lib()
    p = C.c_void_p(0x1000)                                     # a non-NULL pointer that is never dereferenced
    null = C.c_void_p(0)

    def update(t, n=4, runs=4, ptrs=None):
        ptrs = ptrs or [p] * 10            # perm, offsets | ids, jd, magpsf, jdstarthist, ncovhist, ndethist, out8, dropped
        return L.btsbot_feature_update(C.byref(t) if t is not None else None, ptrs[0], ptrs[1], n, runs, *ptrs[2:], null)

    def load(t, m=4, ptrs=None):
        return L.btsbot_feature_load(C.byref(t) if t is not None else None, m, *(ptrs or [p] * 7), null)

    calls = (lambda t: L.btsbot_feature_reset(C.byref(t) if t is not None else None, null), update, load)
    for call in calls:
        assert _invalid(call(None))                                                    # NULL table
        for field in TABLE_FIELDS:
            assert _invalid(call(_table(null=field))), field                           # NULL table array
        for cap in (0, -8, 3, 1000, 12):
            assert _invalid(call(_table(capacity=cap))), cap                           # not a power of two
            assert b"power of two" in L.btsbot_last_error()
    ok = _table()
    for k in range(10):                                                                # each NULL per-alert pointer
        ptrs = [p] * 10
        ptrs[k] = null
        assert _invalid(update(ok, ptrs=ptrs)), k
        assert b"feature_update" in L.btsbot_last_error()
    assert _invalid(update(ok, n=-1)) and _invalid(update(ok, runs=-1)) and _invalid(update(ok, n=4, runs=0))
    for k in range(7):
        ptrs = [p] * 7
        ptrs[k] = null
        assert _invalid(load(ok, ptrs=ptrs)), k
        assert b"feature_load" in L.btsbot_last_error()
    assert _invalid(load(ok, m=-1))
    assert update(ok, n=0, runs=0) == _lib.OK and load(ok, m=0) == _lib.OK             # nothing to launch


# ---- the class, argument checks only --------------------------------------------------------------------------------
def test_feature_state_checks_arguments_without_a_device():
    import btsbot_amd
    from btsbot_amd import features
    assert btsbot_amd.FeatureState is features.FeatureState and features.RESERVED_ID == RESERVED_ID
    for cap in (1000, 0, -4, 3, 1 << 31, 256.0):
        with pytest.raises(ValueError, match="power of two"):
            btsbot_amd.FeatureState(capacity=cap)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.FeatureState(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.FeatureState(256, torch.device("cpu"))
    with pytest.raises(ValueError, match="power of two"):
        btsbot_amd.FeatureState.from_export({}, capacity=100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.FeatureState.from_export({}, capacity=64, device="cpu")


def test_make_metadata_checks_columns_before_it_touches_a_state():
    """With a state the unknown-column errors still come before any device work: the state is never asked."""
    from btsbot_amd import alert_utils
    packets = [{"objectId": EXAMPLE_IDS[k % 2], "candidate": {"jd": 2459000.5 + k, "magpsf": 19.0, "jdstarthist": 2458999.0,
                                                              "ncovhist": 10 + k, "ndethist": 3}} for k in range(4)]

    class Untouched:
        def update(self, *a):
            raise AssertionError("state.update was called")

    with pytest.raises(KeyError, match="no_such_column"):
        alert_utils.make_metadata(packets, ["age", "no_such_column"], device="cuda:1000", state=Untouched())


# ---- objectId -> int64 ----------------------------------------------------------------------------------------------
def test_object_keys():
    from btsbot_amd.alert_utils import object_keys, object_names
    rng = np.random.default_rng(1)
    names = ["ZTF%02d%s" % (rng.integers(0, 100), "".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz"), 7)))
             for _ in range(200)] + ["ZTF00aaaaaaa", "ZTF99zzzzzzz", "ZTF18aaaaaab"] + list(EXAMPLE_IDS)
    keys = object_keys(names)
    assert keys.dtype == np.int64 and keys.shape == (len(names),) and (keys >= 0).all()
    assert object_names(keys) == names                                                  # exact and reversible
    assert len(set(keys.tolist())) == len(set(names))
    assert keys[-5] == 0 and keys[-4] == 100 * 26 ** 7 - 1 and keys[-3] == 18 * 26 ** 7 + 1
    a, b = object_keys(EXAMPLE_IDS)
    assert a > 0 and b > 0 and a != b
    other = ["ZTF22aaaaaa", "ZTF22aaaaaaaa", "ZTF22aaaaaaA", "ztf22aaaaaaa", "ZTF2xaaaaaaa", "ZTF220000003", "", "ATLAS19abc",
             "2023ixf", "ZTF２２aaaaaaa", "étoile"]
    hashed = object_keys(other)
    assert (hashed < 0).all() and len(set(hashed.tolist())) == len(other) and RESERVED_ID not in hashed
    assert (hashed >= -(2 ** 63 - 1)).all()
    assert np.array_equal(hashed, object_keys(list(reversed(other)))[::-1])             # stable across calls
    import hashlib
    h = int.from_bytes(hashlib.blake2b(b"ATLAS19abc", digest_size=8).digest(), "big")
    assert int(object_keys(["ATLAS19abc"])[0]) == -(1 + h % (2 ** 63 - 1))
    with pytest.raises(ValueError):
        object_names(hashed[:1])
    assert object_keys([]).shape == (0,)
