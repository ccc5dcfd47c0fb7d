"""Streaming policy triggers (btsbot_amd.TriggerState, btsbot_trigger_update), host side: a plain numpy restatement of the
streaming rules -- a dict per object, one loop over alerts -- tied to the offline restatement of tests/test_policy_host.py
(which that file ties to the reference's recorded output): the final state of a time-ordered stream cut into batches any
way equals restate_objects on the whole, exactly.  Then the C entry points' and the class's argument checks, none of
which needs a device.  tests/test_gpu_trigger.py imports the restatement as its oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_policy_host import GOLDEN, REFERENCE_POLICIES, golden_inputs, restate_objects

RESERVED_ID = np.iinfo(np.int64).min
CHUNKS = (1, 7, 64, 257, 1541)
SAME_AS_OFFLINE = ("object_id", "n_alerts", "min_magpsf", "trigger_jd", "trigger_mag")
EXPORTED = ("object_id", "n_alerts", "min_magpsf", "last_jd", "count", "pred", "trigger_jd", "trigger_mag")


class StreamRestatement:
    """The rules of TriggerState.update, one alert at a time.  capacity: objects the state can hold (None: any number);
    which slot an object takes is the table's business, that a new object needs a free one is the rule."""

    def __init__(self, policies=REFERENCE_POLICIES, capacity=None):
        self.policies = [(float(thr), float(cut), int(k), np.nan if gate is None else float(gate))
                         for thr, cut, k, gate in policies.values()]
        self.capacity = capacity
        self.objects = {}
        self.taken = self.dropped = self.late = 0

    def update(self, object_id, jd, magpsf, raw_preds):
        """-> (fired uint8 [n, n_pol], dropped bool [n])."""
        object_id = np.asarray(object_id, dtype=np.int64)
        jd, magpsf = np.asarray(jd, dtype=np.float64), np.asarray(magpsf, dtype=np.float64)
        score = np.asarray(raw_preds, dtype=np.float32).astype(np.float64)
        n, npol = len(jd), len(self.policies)
        fired, dropped = np.zeros((n, npol), dtype=np.uint8), np.zeros(n, dtype=bool)
        # which object comes first does not matter (objects are independent, and new ones of one batch either all find
        # a slot or the test does not depend on which do); inside an object: (jd, input position)
        for i in np.lexsort((np.arange(n), jd, object_id)):
            oid = int(object_id[i])
            if oid == RESERVED_ID or (oid not in self.objects and self.capacity is not None
                                      and len(self.objects) >= self.capacity):
                dropped[i] = True
                self.dropped += 1
                continue
            o = self.objects.setdefault(oid, dict(n_alerts=0, min_magpsf=np.nan, last_jd=-np.inf, count=[0] * npol,
                                                  trigger_jd=[-1.0] * npol, trigger_mag=[-1.0] * npol))
            self.taken += 1
            o["n_alerts"] += 1
            if jd[i] < o["last_jd"]:
                self.late += 1
            o["last_jd"] = max(o["last_jd"], jd[i])
            if not np.isnan(magpsf[i]) and not o["min_magpsf"] <= magpsf[i]:
                o["min_magpsf"] = magpsf[i]
            for q, (thr, cut, k, gate) in enumerate(self.policies):
                o["count"][q] += int(score[i] > thr and magpsf[i] < cut)
                if o["trigger_jd"][q] < 0 and o["count"][q] >= k and (np.isnan(gate) or o["min_magpsf"] <= gate):
                    o["trigger_jd"][q], o["trigger_mag"][q] = jd[i], magpsf[i]
                    fired[i, q] = 1
        return fired, dropped

    def export(self):
        ids = sorted(self.objects)
        npol = len(self.policies)
        rec = [self.objects[k] for k in ids]
        out = dict(object_id=np.array(ids, dtype=np.int64), n_alerts=np.array([r["n_alerts"] for r in rec], dtype=np.int64),
                   min_magpsf=np.array([r["min_magpsf"] for r in rec], dtype=np.float64),
                   last_jd=np.array([r["last_jd"] for r in rec], dtype=np.float64),
                   count=np.array([r["count"] for r in rec], dtype=np.int32).reshape(len(ids), npol),
                   trigger_jd=np.array([r["trigger_jd"] for r in rec], dtype=np.float64).reshape(len(ids), npol),
                   trigger_mag=np.array([r["trigger_mag"] for r in rec], dtype=np.float64).reshape(len(ids), npol))
        out["pred"] = (out["trigger_jd"] >= 0).astype(np.int32)
        return out

    def counters(self):
        return dict(objects=len(self.objects), taken=self.taken, dropped=self.dropped, late=self.late)


def same_arrays(got, want, keys):
    """Exact equality of the named arrays, shapes, dtypes' values and NaN positions included; the first difference."""
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape:
            return f"{k}: shape {g.shape} != {w.shape}"
        if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            at = tuple(np.argwhere(~((g == w) | ((g != g) & (w != w))))[0])
            return f"{k}: first difference at {at}: got {g[at]}, want {w[at]}"
    return None


def sorted_golden():
    """The fixture's alert rows stably sorted by jd: a time-ordered stream."""
    rows, _, _ = golden_inputs(dict(np.load(GOLDEN)))
    order = np.argsort(rows["jd"], kind="stable")
    return {k: v[order] for k, v in rows.items()}, rows


def stream_in_chunks(state, rows, chunk):
    """Feeds rows (a dict of the four per-alert arrays and more) chunk by chunk; -> (fired, dropped) over all rows."""
    fired, dropped = [], []
    for s in range(0, len(rows["jd"]), chunk):
        f, d = state.update(*(rows[k][s:s + chunk] for k in ("object_id", "jd", "magpsf", "raw_preds")))
        fired.append(f)
        dropped.append(d)
    return np.concatenate(fired), np.concatenate(dropped)


@pytest.fixture(scope="module")
def offline():
    stream, shuffled = sorted_golden()
    want = restate_objects(*(shuffled[k] for k in ("object_id", "jd", "magpsf", "label", "raw_preds")), REFERENCE_POLICIES)
    return stream, shuffled, want


@pytest.mark.parametrize("chunk", CHUNKS)
def test_any_chunking_of_a_time_ordered_stream_equals_the_offline_result(offline, chunk):
    stream, _, want = offline
    state = StreamRestatement()
    fired, dropped = stream_in_chunks(state, stream, chunk)
    got = state.export()
    assert same_arrays(got, want, SAME_AS_OFFLINE + ("pred",)) is None, same_arrays(got, want, SAME_AS_OFFLINE + ("pred",))
    assert state.counters() == dict(objects=len(want["object_id"]), taken=len(stream["jd"]), dropped=0, late=0)
    assert not dropped.any() and list(fired.sum(0)) == list(want["pred"].sum(0)) == [80, 73, 81, 69]
    # every fired row is its object's trigger
    at = {int(o): k for k, o in enumerate(want["object_id"])}
    for i, q in np.argwhere(fired):
        o = at[int(stream["object_id"][i])]
        assert (stream["jd"][i], stream["magpsf"][i]) == (want["trigger_jd"][o, q], want["trigger_mag"][o, q])


def test_one_shuffled_batch_is_sorted_inside_and_chunks_of_it_are_not(offline):
    """Inside a batch an object's alerts are taken by (jd, input position), so the whole fixture in its shuffled order as
    ONE batch equals the offline result; the same order in chunks of 64 is taken as it arrives: late alerts, another
    result."""
    _, shuffled, want = offline
    one = StreamRestatement()
    one.update(*(shuffled[k] for k in ("object_id", "jd", "magpsf", "raw_preds")))
    assert same_arrays(one.export(), want, SAME_AS_OFFLINE) is None and one.late == 0
    arrival = StreamRestatement()
    stream_in_chunks(arrival, shuffled, 64)
    got = arrival.export()
    assert arrival.late == 1101
    assert same_arrays(got, want, ("object_id", "n_alerts", "min_magpsf")) is None     # order-free
    assert same_arrays(got, want, ("trigger_jd",)) is not None


def test_full_state_and_reserved_id_drop_alerts():
    t = 2459300.5
    state = StreamRestatement(capacity=2)
    ids = np.array([5, 6, 7, 5, RESERVED_ID], dtype=np.int64)
    fired, dropped = state.update(ids, t + np.arange(5.0), np.full(5, 18.0), np.full(5, 0.9, dtype=np.float32))
    assert list(dropped) == [False, False, True, False, True]
    assert state.counters() == dict(objects=2, taken=3, dropped=2, late=0)
    assert list(fired[:, 2]) == [1, 1, 0, 0, 0] and list(fired[:, 0]) == [0, 0, 0, 1, 0]


# ---- the C entry points, argument checks only (they return before any HIP call) ------------------------------------
def _table(capacity=8, n_policies=4, null=None):
    from btsbot_amd import _lib
    fields = ["key", "n_alerts", "min_magpsf", "last_jd", "count", "trigger", "counters"]
    return _lib.TriggerTable(*(0 if f == null else 0x1000 for f in fields), capacity, n_policies)   # never dereferenced


def _invalid(status):
    from btsbot_amd import _lib
    return status == _lib.ERR_INVALID_ARG and len(_lib.lib().btsbot_last_error()) > 0


def test_the_three_symbols_exist():
    from btsbot_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("btsbot_trigger_update", "btsbot_trigger_reset", "btsbot_trigger_load"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    assert _lib.lib().btsbot_abi_version() == 1


def test_c_entry_points_reject_bad_arguments_before_any_device_call():
    from btsbot_amd import _lib
    L = _lib.lib()
    p = C.c_void_p(0x1000)                                     # a non-NULL pointer that is never dereferenced
    null = C.c_void_p(0)
    table4 = (C.c_double * 64)(*([0.5, 19.0, 1.0, float("nan")] * 16))

    def update(t, tab=table4, n=4, runs=4, ptrs=None):
        ptrs = ptrs or [p] * 8                                 # perm, offsets | ids, jd, magpsf, raw, fired, dropped
        return L.btsbot_trigger_update(C.byref(t) if t is not None else None, tab, ptrs[0], ptrs[1], n, runs, *ptrs[2:], null)

    def load(t, m=4, ptrs=None):
        return L.btsbot_trigger_load(C.byref(t) if t is not None else None, m, *(ptrs or [p] * 6), null)

    calls = (lambda t: L.btsbot_trigger_reset(C.byref(t) if t is not None else None, null), update, load)
    for call in calls:
        assert _invalid(call(None))                                                    # NULL table
        for field in ("key", "n_alerts", "min_magpsf", "last_jd", "count", "trigger", "counters"):
            assert _invalid(call(_table(null=field))), field                        # NULL table array
        for cap in (0, -8, 3, 1000, 12):
            assert _invalid(call(_table(capacity=cap))), cap                        # not a power of two
            assert b"power of two" in L.btsbot_last_error()
        for npol in (0, 17, -1):
            assert _invalid(call(_table(n_policies=npol))), npol
            assert b"n_policies" in L.btsbot_last_error()
    ok = _table()
    for k in range(8):                                                                 # each NULL per-alert pointer
        ptrs = [p] * 8
        ptrs[k] = null
        assert _invalid(update(ok, ptrs=ptrs)), k
    assert _invalid(update(ok, tab=C.cast(null, C.POINTER(C.c_double))))
    assert _invalid(update(ok, n=-1)) and _invalid(update(ok, runs=-1)) and _invalid(update(ok, n=4, runs=0))
    for bad_k in (0.0, 1.5, -2.0, float("nan")):
        tab = (C.c_double * 16)(*([0.5, 19.0, 1.0, float("nan")] * 3 + [0.5, 19.0, bad_k, 18.5]))
        assert _invalid(update(ok, tab=tab)) and b"k must be" in L.btsbot_last_error()
    for k in range(6):
        ptrs = [p] * 6
        ptrs[k] = null
        assert _invalid(load(ok, ptrs=ptrs)), k
    assert _invalid(load(ok, m=-1))
    assert update(ok, n=0, runs=0) == _lib.OK and load(ok, m=0) == _lib.OK             # nothing to launch


# ---- the class, argument checks only --------------------------------------------------------------------------------
def test_trigger_state_checks_arguments_without_a_device():
    import btsbot_amd
    from btsbot_amd import triggers
    assert btsbot_amd.TriggerState is triggers.TriggerState and triggers.RESERVED_ID == RESERVED_ID
    with pytest.raises(ValueError, match="1..16"):
        btsbot_amd.TriggerState({f"t{i}": (0.5, 19.0, 1, None) for i in range(17)})
    with pytest.raises(ValueError, match="empty"):
        btsbot_amd.TriggerState({})
    with pytest.raises(ValueError, match="power of two"):
        btsbot_amd.TriggerState(capacity=1000)
    for pol in ({"k0": (0.5, 19.0, 0, None)}, {"k1.5": (0.5, 19.0, 1.5, None)}, {"short": (0.5, 19.0, 1)}):
        with pytest.raises(ValueError):
            btsbot_amd.TriggerState(pol)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.TriggerState(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.TriggerState(REFERENCE_POLICIES, 256, torch.device("cpu"))


def test_grouping_by_object_then_jd_keeps_its_old_result():
    """_group_by_object without the second key returns what it did (input order inside an object); with it, (jd, input
    position) order."""
    from btsbot_amd.alert_utils import _group_by_object
    ids = torch.tensor([7, 3, 7, 3, 7, 9])
    jd = torch.tensor([5.0, 2.0, 1.0, 2.0, 1.0, 0.0], dtype=torch.float64)
    perm, off = _group_by_object(ids)
    assert perm.tolist() == [1, 3, 0, 2, 4, 5] and off.tolist() == [0, 2, 5, 6, 6, 6, 6]
    perm, off = _group_by_object(ids, then_by=jd)
    assert perm.tolist() == [1, 3, 2, 4, 0, 5] and off.tolist() == [0, 2, 5, 6, 6, 6, 6]
    assert perm.dtype == torch.int32 and off.dtype == torch.int32
