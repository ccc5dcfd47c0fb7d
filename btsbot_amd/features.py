"""Streaming light-curve features: the custom metadata columns of an alert, from its object's history kept on the device.

``alert_utils.alert_features`` derives ``age``, ``days_since_peak``, ``days_to_peak``, ``peakmag_so_far``,
``maxmag_so_far`` and ``nnotdet`` per object from the alerts that are in the same call.  A live stream hands over tonight's
alerts only; ``FeatureState`` keeps, per object and in a hash table on the device, the few numbers that summarise its light
curve so far (``btsbot_feature_update``, csrc/feature_state.hip), and one launch per batch advances them and writes the
batch's ``CUSTOM_COLS`` rows:

    feats = FeatureState(capacity=1 << 20)
    for object_id, jd, magpsf, jdstarthist, ncovhist, ndethist in nights:
        out = feats.update(object_id, jd, magpsf, jdstarthist, ncovhist, ndethist)   # "features" f32 [n, 8], "dropped"

The cost of a batch follows the batch, not the history.  Cut a time-ordered stream into batches anywhere: columns 2-7 of
the rows equal ``alert_features`` over the whole stream bit for bit (every output is a selection or one float64
subtraction rounded once).  Columns 0-1 (``peakmag``, ``maxmag``) look at an object's future, which a stream does not
have: they repeat the so-far columns 2-3, and the whole-curve values are ``export()``'s ``peakmag`` / ``maxmag`` at the
end of the stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping

import torch

from . import _lib
from .alert_utils import _FEATURE_INPUTS, _group_by_object

RESERVED_ID = -(1 << 63)          # BTSBOT_TRIGGER_FREE: the free-slot marker, the one id a state cannot hold
_COUNTERS = ("objects", "taken", "dropped", "late")
_RECORD = ("object_id", "n_alerts", "first_jd", "last_jd", "peakmag", "peak_jd", "maxmag")


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


class FeatureState:
    """Per-object light-curve state on one GPU.

    capacity: slots of the table, a power of two (an object takes one slot for good: there is no eviction).  Per object
    id (any int64 but ``RESERVED_ID``) the state holds n_alerts, first_jd and last_jd (the smallest and largest jd seen),
    peakmag (the smallest magpsf seen, NaN skipped) with peak_jd (the jd it was first reached at) and maxmag.

    Calls on one state must be ordered by the caller's streams: concurrent ``update`` calls are undefined."""

    def __init__(self, capacity: int = 1 << 20, device="cuda"):
        if not isinstance(capacity, int) or capacity < 1 or capacity & (capacity - 1) or capacity > 1 << 30:
            raise ValueError(f"capacity must be a power of two (at most 2^30), got {capacity!r}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"btsbot_amd.FeatureState runs on the GPU; there is no CPU fallback (device is {dev})")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.capacity, self.device = capacity, dev
        self._key = torch.empty(capacity, dtype=torch.int64, device=dev)
        self._n = torch.empty(capacity, dtype=torch.int32, device=dev)
        self._first, self._last, self._peak, self._peak_jd, self._max = (
            torch.empty(capacity, dtype=torch.float64, device=dev) for _ in range(5))
        self._counters = torch.empty((_lib.TRIGGER_COUNTER_ROWS, 8), dtype=torch.int64, device=dev)
        self._table = _lib.FeatureTable(*(t.data_ptr() for t in (self._key, self._n, self._first, self._last, self._peak,
                                                                 self._peak_jd, self._max, self._counters)), capacity)
        self.reset()

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self) -> None:
        """Forget every object and zero the counters (one launch, no host synchronisation)."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().btsbot_feature_reset(C.byref(self._table), self._stream()), "btsbot_feature_reset")

    def update(self, object_id: torch.Tensor, jd: torch.Tensor, magpsf: torch.Tensor, jdstarthist: torch.Tensor,
               ncovhist: torch.Tensor, ndethist: torch.Tensor) -> Dict[str, torch.Tensor]:
        """One batch of [n] device tensors into the state; jd, magpsf, jdstarthist are taken as float64, ncovhist,
        ndethist as int32, as in ``alert_features``.

        Batches are taken in call order; inside a batch an object's alerts are taken in (jd, input position) order, so the
        batches of a time-sorted stream are taken exactly in ``alert_features``' order.  Alert i of object o: n_alerts +=
        1; i is *late* (counted, and taken all the same, in arrival order) when jd < last_jd; first_jd = min(first_jd, jd),
        last_jd = max(last_jd, jd); a magpsf that is not NaN replaces (peakmag, peak_jd) when it is lower, or equal with a
        lower jd, and maxmag when it is higher.  Then the row, in the order of ``CUSTOM_COLS``, from the record as it
        stands: peakmag, maxmag (so far: columns 0-1 repeat columns 2-3), peakmag_so_far, maxmag_so_far, age = jd - first,
        days_since_peak = jd - peak_jd, days_to_peak = peak_jd - first with first = min(jdstarthist, first_jd) (NaN when
        jdstarthist is), nnotdet = ncovhist - ndethist.  Compared and subtracted in float64, rounded to float32 once.  jd
        must be finite (not checked).

        Returns ``features`` float32 [n, 8] in input order and ``dropped`` bool [n]: alerts of an object that found no
        free slot (table full; objects already in the table keep being updated) and alerts with ``RESERVED_ID`` change
        nothing, are counted and get an all-NaN row.

        No host synchronisation: two stable sorts, the offsets and one launch are queued on the current stream, and
        nothing on this path reads a device value on the host."""
        cols = (object_id, jd, magpsf, jdstarthist, ncovhist, ndethist)
        names = ("object_id",) + _FEATURE_INPUTS
        for name, t in zip(names, cols):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
        if object_id.device.type != "cuda":
            raise RuntimeError("btsbot_amd.FeatureState.update runs on the GPU; there is no CPU "
                               f"fallback (object_id is on {object_id.device})")
        n = object_id.shape[0] if object_id.dim() == 1 else -1
        for name, t in zip(names, cols):
            if t.dim() != 1 or t.shape[0] != n:
                raise ValueError(f"{name} must be [{max(n, 0)}], got {tuple(t.shape)}")
        if object_id.dtype.is_floating_point or object_id.dtype == torch.bool:
            raise ValueError(f"object_id must be an integer tensor, got {object_id.dtype}")
        dev = self.device
        if object_id.device != dev:
            raise ValueError(f"object_id is on {object_id.device}, the state on {dev}")
        ids = object_id.to(torch.int64).contiguous()
        jd, magpsf, jdstarthist = (t.to(device=dev, dtype=torch.float64).contiguous() for t in cols[1:4])
        ncovhist, ndethist = (t.to(device=dev, dtype=torch.int32).contiguous() for t in cols[4:])
        out = torch.empty((n, 8), dtype=torch.float32, device=dev)                       # the kernel writes every element
        dropped = torch.empty(n, dtype=torch.uint8, device=dev)
        if n:
            perm, offsets = _group_by_object(ids, then_by=jd)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().btsbot_feature_update(
                    C.byref(self._table), _ptr(perm), _ptr(offsets), n, n, _ptr(ids), _ptr(jd), _ptr(magpsf),
                    _ptr(jdstarthist), _ptr(ncovhist), _ptr(ndethist), _ptr(out), _ptr(dropped), self._stream()),
                    "btsbot_feature_update")
        return {"features": out, "dropped": dropped.view(torch.bool)}

    def export(self) -> Dict[str, torch.Tensor]:
        """The objects held, in ascending id order: ``object_id``, ``n_alerts`` (int64), ``first_jd``, ``last_jd``,
        ``peakmag``, ``peak_jd``, ``maxmag`` (float64).  At the end of a stream ``peakmag`` / ``maxmag`` are columns 0-1 of
        ``alert_features`` over the whole of it.  One host read."""
        slots = (self._key != RESERVED_ID).nonzero()[:, 0]                               # the one host read
        slots = slots[torch.argsort(self._key[slots])]
        return {"object_id": self._key[slots], "n_alerts": self._n[slots].to(torch.int64), "first_jd": self._first[slots],
                "last_jd": self._last[slots], "peakmag": self._peak[slots], "peak_jd": self._peak_jd[slots],
                "maxmag": self._max[slots]}

    @classmethod
    def from_export(cls, records: Mapping, capacity: int = 1 << 20, device="cuda") -> "FeatureState":
        """A state holding ``records`` (what ``export()`` returned, tensors or arrays): a service restart, or a move to a
        larger table.  Raises ValueError when an id comes twice, is ``RESERVED_ID``, or the records do not fit the
        capacity."""
        state = cls(capacity, device)
        dev = state.device
        missing = [k for k in _RECORD if k not in records]
        if missing:
            raise ValueError(f"records lack {missing}")
        ids = torch.as_tensor(records["object_id"]).to(device=dev, dtype=torch.int64).contiguous()
        m = ids.shape[0] if ids.dim() == 1 else -1
        n_alerts = torch.as_tensor(records["n_alerts"]).to(device=dev, dtype=torch.int32).contiguous()
        fields = [torch.as_tensor(records[k]).to(device=dev, dtype=torch.float64).contiguous() for k in _RECORD[2:]]
        for name, t in zip(_RECORD, [ids, n_alerts] + fields):
            if m < 0 or tuple(t.shape) != (m,):
                raise ValueError(f"records[{name!r}] must be [{max(m, 0)}], got {list(t.shape)}")
        if m:
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().btsbot_feature_load(
                    C.byref(state._table), m, _ptr(ids), _ptr(n_alerts), *(_ptr(f) for f in fields), state._stream()),
                    "btsbot_feature_load")
            present, no_slot = state._counters.sum(0)[4:6].tolist()                      # the one host read
            if present or no_slot:
                raise ValueError(f"from_export: {present} records carry an id that came before, {no_slot} found no slot "
                                 f"in a table of {capacity} (or carry the reserved id)")
        return state

    def counters(self) -> Dict[str, int]:
        """``objects`` held, alerts ``taken``, alerts ``dropped``, ``late`` alerts since the state was made or reset (a
        loaded record counts as an object, its alerts were taken elsewhere).  One host read."""
        return dict(zip(_COUNTERS, self._counters.sum(0)[:4].tolist()))
