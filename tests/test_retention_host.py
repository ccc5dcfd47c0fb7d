"""Retention for the streaming states (ObjectState.expire / resize, btsbot_trigger_rehash, btsbot_feature_rehash), host
side: the host model of retention -- the restatements of tests/test_trigger_host.py and tests/test_feature_state_host.py
with an ``expire`` that deletes the objects whose last_jd < before_jd and counts them -- and the argument checks of the
two C entry points and of the two methods, none of which needs a device.  tests/test_gpu_retention.py imports the
model as its oracle."""
import ctypes as C

import numpy as np
import pytest

from test_feature_state_host import (NAMES, SHARED_CAPACITY, SHARED_EXPORT, TABLE_FIELDS, TRIGGER_NAMES,
                                     FeatureStreamRestatement, shared_batches)
from test_trigger_host import RESERVED_ID, StreamRestatement, same_arrays

TRIGGER_FIELDS = ("key", "n_alerts", "min_magpsf", "last_jd", "count", "trigger", "counters")
SHARED_EXPIRE_AFTER = 2          # shared_batches(): expire once the table is full


class _Retention:
    """expire(before_jd): forget the objects with last_jd < before_jd (in exactly this form: a NaN on either side keeps the
    object); -> their ids.  An object that comes back is made afresh by update(), which is the restatement's as it is."""
    expired = 0

    def expire(self, before_jd):
        gone = sorted(k for k, o in self.objects.items() if o["last_jd"] < before_jd)
        for k in gone:
            del self.objects[k]
        self.expired += len(gone)
        return gone


class RetainingTriggers(_Retention, StreamRestatement):
    pass


class RetainingFeatures(_Retention, FeatureStreamRestatement):
    pass


def shared_cut():
    """A cut for shared_batches() after batch SHARED_EXPIRE_AFTER: the sixth of the eight last_jd held then, so five
    objects go.  Batch 3 then makes five objects (its four new ones, and the held object of 63 alerts, which is among the
    five and comes back with earlier epochs): as many as there are free slots, so which of them find one is no race
    between the runs of a launch."""
    host = RetainingFeatures(capacity=SHARED_CAPACITY)
    for b in shared_batches()[:SHARED_EXPIRE_AFTER + 1]:
        host.update(*(b[k] for k in NAMES))
    return float(np.sort([o["last_jd"] for o in host.objects.values()])[5])


def test_the_model_expires_by_the_comparison_as_written():
    t = 2459300.5
    for state, cols in ((RetainingTriggers(capacity=4), lambda n: (np.full(n, 18.0), np.full(n, 0.9, dtype=np.float32))),
                        (RetainingFeatures(capacity=4), lambda n: (np.full(n, 18.0), np.full(n, t - 1),
                                                                    np.full(n, 9, dtype=np.int32), np.full(n, 2, dtype=np.int32)))):
        state.update(np.array([5, 6, 7, 5], dtype=np.int64), t + np.arange(4.0), *cols(4))
        state.objects[7]["last_jd"] = np.nan
        assert state.expire(-np.inf) == [] and state.expire(np.nan) == [] and state.expire(t + 1.0) == []
        assert state.expire(t + 3.0) == [6] and state.expired == 1                     # 5 was seen again at t + 3: not below
        assert state.counters() == dict(objects=2, taken=4, dropped=0, late=0)
        _, dropped = state.update(np.array([6, 8, 9], dtype=np.int64), t + 5 + np.arange(3.0), *cols(3))
        assert list(dropped) == [False, False, True] and state.objects[6]["n_alerts"] == 1      # 6 is a new object
        assert state.expire(np.inf) == [5, 6, 8] and state.expired == 4 and list(state.objects) == [7]   # NaN stays


def test_both_models_agree_on_what_the_states_share_after_an_expire():
    cut = shared_cut()
    trig, feat = RetainingTriggers(capacity=SHARED_CAPACITY), RetainingFeatures(capacity=SHARED_CAPACITY)
    new_dropped_after = 0
    for k, b in enumerate(shared_batches()):
        before = set(trig.objects)
        _, td = trig.update(*(b[k_] for k_ in TRIGGER_NAMES))
        _, fd = feat.update(*(b[k_] for k_ in NAMES))
        assert np.array_equal(td, fd)
        if k == SHARED_EXPIRE_AFTER:
            assert trig.counters()["objects"] == SHARED_CAPACITY
            gone = trig.expire(cut)
            assert gone == feat.expire(cut) and len(gone) == 5
        if k == SHARED_EXPIRE_AFTER + 1:
            made = set(trig.objects) - before
            returned = made & set(gone)
            assert len(made) == 5 and len(returned) == 1 and trig.counters()["objects"] == SHARED_CAPACITY
            assert trig.objects[min(returned)]["n_alerts"] == 65                       # a new object: its 63 are forgotten
        if k > SHARED_EXPIRE_AFTER:
            new_dropped_after += int((td & (b["object_id"] != RESERVED_ID)).sum())
        assert trig.counters() == feat.counters() and trig.expired == feat.expired
        diff = same_arrays(trig.export(), feat.export(), SHARED_EXPORT)
        assert diff is None, diff
    # without the expire every new object of batches 3 and 4 is dropped (9 alerts); now each finds a freed slot
    assert trig.expired == 5 and new_dropped_after == 0 and trig.counters()["dropped"] == 2 and trig.counters()["late"] > 0


# ---- the C entry points, argument checks only (they return before any HIP call) ------------------------------------
def _trigger_table(at=0x1000, capacity=8, n_policies=4, null=None):
    from btsbot_amd import _lib
    return _lib.TriggerTable(*(0 if f == null else at for f in TRIGGER_FIELDS), capacity, n_policies)   # never dereferenced


def _feature_table(at=0x1000, capacity=8, null=None):
    from btsbot_amd import _lib
    return _lib.FeatureTable(*(0 if f == null else at for f in TABLE_FIELDS), capacity)                 # never dereferenced


def test_the_two_symbols_exist_with_the_declared_argument_types():
    from btsbot_amd import _lib
    raw, L = C.CDLL(_lib.LIB_PATH), _lib.lib()
    for name, table in (("btsbot_trigger_rehash", _lib.TriggerTable), ("btsbot_feature_rehash", _lib.FeatureTable)):
        assert hasattr(raw, name) and name in _lib.SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == [C.POINTER(table), C.POINTER(table), C.c_double, C.c_void_p]
    assert L.btsbot_abi_version() == 1


@pytest.mark.parametrize("symbol, make, fields", (("btsbot_trigger_rehash", _trigger_table, TRIGGER_FIELDS),
                                                  ("btsbot_feature_rehash", _feature_table, TABLE_FIELDS)))
def test_rehash_rejects_bad_arguments_before_any_device_call(symbol, make, fields):
    from btsbot_amd import _lib
    L = _lib.lib()
    fn, null, who = getattr(L, symbol), C.c_void_p(0), symbol[len("btsbot_"):].encode()

    def invalid(src, dst, says=b""):
        status = fn(C.byref(src) if src is not None else None, C.byref(dst) if dst is not None else None, 2459000.5, null)
        msg = L.btsbot_last_error()
        return status == _lib.ERR_INVALID_ARG and who in msg and says in msg

    good_src, good_dst = make(0x1000), make(0x2000, capacity=64)
    for bad_is_src in (True, False):
        pair = (lambda bad: (bad, good_dst)) if bad_is_src else (lambda bad: (good_src, bad))
        assert invalid(*pair(None), says=b"NULL")                                       # NULL table
        for field in fields:
            assert invalid(*pair(make(0x3000, null=field)), says=b"NULL"), field        # NULL table array
        for cap in (0, -8, 3, 1000, 12):
            assert invalid(*pair(make(0x3000, capacity=cap)), says=b"power of two"), cap
    assert invalid(good_src, good_src, says=b"key") and invalid(good_src, make(0x1000, capacity=64), says=b"key")
    if make is _trigger_table:
        for npol in (0, 17, -1):
            assert invalid(good_src, make(0x2000, n_policies=npol), says=b"n_policies"), npol
        assert invalid(good_src, make(0x2000, n_policies=5), says=b"n_policies differs")
        assert invalid(make(0x1000, n_policies=16), good_dst, says=b"n_policies differs")


# ---- the methods, argument checks only ----------------------------------------------------------------------------------
def test_expire_and_resize_check_their_arguments_without_a_device():
    """The checks come before anything touches the table, so a state that was never given one (there is no device to
    make it on) is enough to see them."""
    import btsbot_amd
    for cls in (btsbot_amd.TriggerState, btsbot_amd.FeatureState):
        state = cls.__new__(cls)
        for cap in (1000, 0, -4, 3, 1 << 31, 256.0, None):
            with pytest.raises(ValueError, match="power of two"):
                state.resize(cap)
        for jd in (2459000, "2459000.5", None, np.float32(2459000.5), [2459000.5]):
            with pytest.raises(ValueError, match="before_jd must be a float"):
                state.expire(jd)
            with pytest.raises(ValueError, match="before_jd must be a float"):
                state.expire(jd, return_expired=True)
        for jd in (2459000, "2459000.5"):
            with pytest.raises(ValueError, match="before_jd must be a float or None"):
                state.resize(64, jd)
        assert not hasattr(state, "_table")
