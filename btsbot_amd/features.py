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

from typing import Dict, Mapping

import torch

from . import _lib
from ._lib import ptr as _ptr
from ._object_state import RESERVED_ID, ObjectState   # noqa: F401  (RESERVED_ID: part of this module's names)
from .alert_utils import _FEATURE_INPUTS

_RECORD = ("object_id", "n_alerts", "first_jd", "last_jd", "peakmag", "peak_jd", "maxmag")


class FeatureState(ObjectState):
    """Per-object light-curve state on one GPU.

    capacity: slots of the table, a power of two (an object keeps its slot until ``expire`` forgets it; ``resize`` moves
    the records to a table of another size; an object that comes back after it was expired is a new object: its
    ``*_so_far`` and peak columns start again, ``age`` still follows the packet's jdstarthist).  Per object
    id (any int64 but ``RESERVED_ID``) the state holds n_alerts, first_jd and last_jd (the smallest and largest jd seen),
    peakmag (the smallest magpsf seen, NaN skipped) with peak_jd (the jd it was first reached at) and maxmag.

    Calls on one state must be ordered by the caller's streams: concurrent ``update`` calls are undefined."""
    _RESET, _REHASH = "btsbot_feature_reset", "btsbot_feature_rehash"
    _ARRAYS = ("_key", "_n", "_first", "_last", "_peak", "_peak_jd", "_max", "_counters")

    def __init__(self, capacity: int = 1 << 20, device="cuda"):
        super().__init__(capacity, device)

    def _allocate(self, capacity: int):
        arrays = self._empty(capacity, [((), torch.float64)] * 5)
        return arrays, _lib.FeatureTable(*(t.data_ptr() for t in arrays), capacity)

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
        n = self._check_batch(("object_id",) + _FEATURE_INPUTS, cols)
        dev = self.device
        ids = object_id.to(torch.int64).contiguous()
        jd, magpsf, jdstarthist = (t.to(device=dev, dtype=torch.float64).contiguous() for t in cols[1:4])
        ncovhist, ndethist = (t.to(device=dev, dtype=torch.int32).contiguous() for t in cols[4:])
        out = torch.empty((n, 8), dtype=torch.float32, device=dev)                       # the kernel writes every element
        dropped = torch.empty(n, dtype=torch.uint8, device=dev)
        if n:
            perm, offsets = self._runs(ids, jd)
            self._call("btsbot_feature_update", _ptr(perm), _ptr(offsets), n, n, _ptr(ids), _ptr(jd), _ptr(magpsf),
                       _ptr(jdstarthist), _ptr(ncovhist), _ptr(ndethist), _ptr(out), _ptr(dropped))
        return {"features": out, "dropped": dropped.view(torch.bool)}

    def export(self) -> Dict[str, torch.Tensor]:
        """The objects held, in ascending id order: ``object_id``, ``n_alerts`` (int64), ``first_jd``, ``last_jd``,
        ``peakmag``, ``peak_jd``, ``maxmag`` (float64).  At the end of a stream ``peakmag`` / ``maxmag`` are columns 0-1 of
        ``alert_features`` over the whole of it.  One host read."""
        return self._records(self._installed()[1], self._held_slots())

    def _records(self, arrays, slots):
        out = {"object_id": arrays[0][slots], "n_alerts": arrays[1][slots].to(torch.int64)}
        out.update((name, t[slots]) for name, t in zip(_RECORD[2:], arrays[2:7]))
        return out

    @classmethod
    def from_export(cls, records: Mapping, capacity: int = 1 << 20, device="cuda") -> "FeatureState":
        """A state holding ``records`` (what ``export()`` returned, tensors or arrays): a service restart, or a move to a
        larger table.  Raises ValueError when an id comes twice, is ``RESERVED_ID``, or the records do not fit the
        capacity."""
        state = cls(capacity, device)
        dev = state.device
        state._require(records, _RECORD)
        ids = torch.as_tensor(records["object_id"]).to(device=dev, dtype=torch.int64).contiguous()
        m = ids.shape[0] if ids.dim() == 1 else -1
        n_alerts = torch.as_tensor(records["n_alerts"]).to(device=dev, dtype=torch.int32).contiguous()
        fields = [torch.as_tensor(records[k]).to(device=dev, dtype=torch.float64).contiguous() for k in _RECORD[2:]]
        state._load("btsbot_feature_load", m, [(name, t, (m,)) for name, t in zip(_RECORD, [ids, n_alerts] + fields)],
                    lambda shape: f"[{max(m, 0)}]")
        return state
