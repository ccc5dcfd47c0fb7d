"""Streaming policy triggers: which objects does a scanning policy fire on NOW.

``val.policy_eval`` answers "does (thr, cut, k, gate) fire on this object, and at which alert first" for a finished
split.  A live stream ends at a tensor of scores batch after batch; ``TriggerState`` keeps, per object and in a hash table
on the device, the few numbers that summarise its history for a fixed set of policies (``btsbot_trigger_update``,
csrc/trigger_state.hip), and one launch per scored batch advances them and marks the alerts a policy fires at:

    state = TriggerState(REFERENCE_POLICIES, capacity=1 << 20)
    for object_id, jd, magpsf, triplets, metadata in nights:
        scores = stream.score(triplets, metadata)
        new = state.new_triggers(object_id, jd, magpsf, scores)      # object_id, policy, trigger_jd, trigger_mag, alert

The cost of a batch follows the batch, not the history.  Cut a time-ordered stream into batches anywhere: ``export()``
then equals ``val.policy_eval`` over the whole stream bit for bit (every output is a count or a copy of an input).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping

import torch

from . import _lib
from ._lib import ptr as _ptr
from ._object_state import RESERVED_ID, ObjectState   # noqa: F401  (RESERVED_ID: part of this module's names)
from .val import POLICIES_PER_LAUNCH, REFERENCE_POLICIES, _policy_table

_RECORD = ("object_id", "n_alerts", "min_magpsf", "last_jd", "count", "trigger_jd", "trigger_mag")


class TriggerState(ObjectState):
    """Per-object policy state on one GPU.

    policies: name -> (thr, cut, k, gate or None) as for ``val.policy_eval``, 1..16 of them, fixed for the life of the
    state; capacity: slots of the table, a power of two (an object keeps its slot until ``expire`` forgets it; ``resize``
    moves the records to a table of another size; an object that comes back after it was expired is a new object, on
    which the policies may fire again).  Per object id (any int64 but ``RESERVED_ID``) the state holds n_alerts,
    min_magpsf (NaN skipped), last_jd (the largest jd seen) and per policy the count of valid alerts and (trigger_jd,
    trigger_mag), (-1, -1) until the policy has fired.

    Calls on one state must be ordered by the caller's streams: concurrent ``update`` calls are undefined."""
    _RESET, _REHASH = "btsbot_trigger_reset", "btsbot_trigger_rehash"
    _ARRAYS = ("_key", "_n", "_min", "_last", "_count", "_trig", "_counters")

    def __init__(self, policies: Mapping = REFERENCE_POLICIES, capacity: int = 1 << 20, device="cuda"):
        table = _policy_table(policies)
        if table.shape[0] > POLICIES_PER_LAUNCH:
            raise ValueError(f"a TriggerState holds 1..{POLICIES_PER_LAUNCH} policies, got {table.shape[0]}")
        for name, row in zip(policies, table.tolist()):
            if not row[2] >= 1 or row[2] != int(row[2]):
                raise ValueError(f"policy {name!r}: k must be an integer >= 1, got {row[2]!r}")
        self.policies = dict(policies)
        self._policy_rows = table.contiguous()                               # host, float64 [n_pol, 4]
        self.n_policies = table.shape[0]
        super().__init__(capacity, device)

    def _allocate(self, capacity: int):
        npol, f64 = self.n_policies, torch.float64
        arrays = self._empty(capacity, (((), f64), ((), f64), ((npol,), torch.int32), ((npol, 2), f64)))
        return arrays, _lib.TriggerTable(*(t.data_ptr() for t in arrays), capacity, npol)

    def update(self, object_id: torch.Tensor, jd: torch.Tensor, magpsf: torch.Tensor,
               raw_preds: torch.Tensor) -> Dict[str, torch.Tensor]:
        """One batch of [n] device tensors into the state; jd and magpsf are taken as float64, raw_preds as float32 and
        compared as that value widened to float64, as in ``val.policy_eval``.

        Batches are taken in call order; inside a batch an object's alerts are taken in (jd, input position) order, so the
        batches of a time-sorted stream are taken exactly in ``policy_eval``'s order.  Alert i of object o: n_alerts += 1;
        i is *late* (counted, and taken all the same, in arrival order) when jd < last_jd; last_jd = max(last_jd, jd);
        min_magpsf takes magpsf unless it is NaN; per policy count += (raw > thr and magpsf < cut) (a NaN magpsf is never
        valid); a policy that has not fired yet fires at i when count >= k and (without a gate, or) min_magpsf <= gate.
        jd must be >= 0 and finite (not checked).

        Returns ``fired`` bool [n, n_pol] (the policy fires at this alert: at most once per object and policy over the
        life of the state) and ``dropped`` bool [n]: alerts of an object that found no free slot (table full; objects
        already in the table keep being updated) and alerts with ``RESERVED_ID`` change nothing and are counted.

        No host synchronisation: two stable sorts, the offsets and one launch are queued on the current stream, and
        nothing on this path reads a device value on the host (no ``.item()``, ``.cpu()``, ``nonzero``)."""
        n = self._check_batch(("object_id", "jd", "magpsf", "raw_preds"), (object_id, jd, magpsf, raw_preds))
        dev = self.device
        ids = object_id.to(torch.int64).contiguous()
        jd, magpsf = (t.to(device=dev, dtype=torch.float64).contiguous() for t in (jd, magpsf))
        raw = raw_preds.to(device=dev, dtype=torch.float32).contiguous()
        fired = torch.empty((n, self.n_policies), dtype=torch.uint8, device=dev)        # the kernel writes every element
        dropped = torch.empty(n, dtype=torch.uint8, device=dev)
        if n:
            perm, offsets = self._runs(ids, jd)
            self._call("btsbot_trigger_update", C.cast(C.c_void_p(self._policy_rows.data_ptr()), C.POINTER(C.c_double)),
                       _ptr(perm), _ptr(offsets), n, n, _ptr(ids), _ptr(jd), _ptr(magpsf), _ptr(raw), _ptr(fired),
                       _ptr(dropped))
        return {"fired": fired.view(torch.bool), "dropped": dropped.view(torch.bool)}

    def new_triggers(self, object_id: torch.Tensor, jd: torch.Tensor, magpsf: torch.Tensor,
                     raw_preds: torch.Tensor) -> Dict[str, torch.Tensor]:
        """``update``, then the batch's triggers as tensors of equal length, ordered by (alert, policy): ``object_id``,
        ``policy`` (index into the state's policies), ``trigger_jd``, ``trigger_mag`` and ``alert`` (the row of the batch).
        One host read (the number of triggers)."""
        fired = self.update(object_id, jd, magpsf, raw_preds)["fired"]
        where = fired.nonzero()                                                          # the one host read
        row, pol = where[:, 0], where[:, 1]
        return {"object_id": object_id[row].to(torch.int64), "policy": pol,
                "trigger_jd": jd.to(device=self.device, dtype=torch.float64)[row],
                "trigger_mag": magpsf.to(device=self.device, dtype=torch.float64)[row], "alert": row}

    def export(self) -> Dict[str, torch.Tensor]:
        """The objects held, in ascending id order: ``object_id``, ``n_alerts`` (int64), ``min_magpsf``, ``last_jd``,
        ``count`` int32 [n_obj, n_pol], ``pred`` int32 (``trigger_jd >= 0``), ``trigger_jd``, ``trigger_mag`` float64
        [n_obj, n_pol]; where the names are ``val.policy_eval``'s, so are shapes and dtypes.  One host read."""
        return self._records(self._installed()[1], self._held_slots())

    def _records(self, arrays, slots):
        key, n, lo, last, count, trig, _ = arrays
        trig = trig[slots]
        return {"object_id": key[slots], "n_alerts": n[slots].to(torch.int64), "min_magpsf": lo[slots],
                "last_jd": last[slots], "count": count[slots], "pred": (trig[:, :, 0] >= 0).to(torch.int32),
                "trigger_jd": trig[:, :, 0].contiguous(), "trigger_mag": trig[:, :, 1].contiguous()}

    @classmethod
    def from_export(cls, records: Mapping, policies: Mapping = REFERENCE_POLICIES, capacity: int = 1 << 20,
                    device="cuda") -> "TriggerState":
        """A state holding ``records`` (what ``export()`` returned, tensors or arrays; ``pred`` is not needed): a service
        restart, or a move to a larger table.  ``policies`` must be the exporting state's.  Raises ValueError when an id
        comes twice, is ``RESERVED_ID``, or the records do not fit the capacity."""
        state = cls(policies, capacity, device)
        dev, npol = state.device, state.n_policies
        state._require(records, _RECORD)
        ids = torch.as_tensor(records["object_id"]).to(device=dev, dtype=torch.int64).contiguous()
        m = ids.shape[0] if ids.dim() == 1 else -1
        n_alerts = torch.as_tensor(records["n_alerts"]).to(device=dev, dtype=torch.int32).contiguous()
        lo, last = (torch.as_tensor(records[k]).to(device=dev, dtype=torch.float64).contiguous()
                    for k in ("min_magpsf", "last_jd"))
        count = torch.as_tensor(records["count"]).to(device=dev, dtype=torch.int32).contiguous()
        trig = torch.stack([torch.as_tensor(records[k]).to(device=dev, dtype=torch.float64)
                            for k in ("trigger_jd", "trigger_mag")], dim=-1).contiguous()
        fields = (("object_id", ids, (m,)), ("n_alerts", n_alerts, (m,)), ("min_magpsf", lo, (m,)),
                  ("last_jd", last, (m,)), ("count", count, (m, npol)), ("trigger_jd / trigger_mag", trig, (m, npol, 2)))
        state._load("btsbot_trigger_load", m, fields, lambda shape: f"{list(shape)} for {npol} policies")
        return state
