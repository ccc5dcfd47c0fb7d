"""What the per-object streaming states (``TriggerState``, ``FeatureState``) share: a hash table of object ids on the
device (csrc/object_table.h) with a record per object, advanced by one launch per batch.  The base owns the table's
common arrays, the checks of a batch's columns, the grouping, the slots an export reads and the end of a load; a state
adds its record arrays, its ctypes table struct (``self._table``) and its kernel calls."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Mapping, Sequence, Tuple

import torch

from . import _lib
from .alert_utils import _group_by_object

RESERVED_ID = -(1 << 63)          # BTSBOT_TRIGGER_FREE: the free-slot marker, the one id a state cannot hold
_COUNTERS = ("objects", "taken", "dropped", "late")


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


class ObjectState:
    _RESET = ""                   # the state's reset symbol

    def __init__(self, capacity: int, device):
        """Checks capacity and device and allocates key, n_alerts and the counters; the state builds ``self._table`` over
        them and its own arrays, then calls ``reset()``."""
        if not isinstance(capacity, int) or capacity < 1 or capacity & (capacity - 1) or capacity > 1 << 30:
            raise ValueError(f"capacity must be a power of two (at most 2^30), got {capacity!r}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"btsbot_amd.{type(self).__name__} runs on the GPU; there is no CPU fallback "
                               f"(device is {dev})")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.capacity, self.device = capacity, dev
        self._key = torch.empty(capacity, dtype=torch.int64, device=dev)
        self._n = torch.empty(capacity, dtype=torch.int32, device=dev)
        self._counters = torch.empty((_lib.TRIGGER_COUNTER_ROWS, 8), dtype=torch.int64, device=dev)

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, symbol: str, *args) -> None:
        """symbol(table, *args, stream) on the state's device."""
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.lib(), symbol)(C.byref(self._table), *args, self._stream()), symbol)

    def reset(self) -> None:
        """Forget every object and zero the counters (one launch, no host synchronisation)."""
        self._call(self._RESET)

    def _check_batch(self, names: Sequence[str], cols: Sequence) -> int:
        """The columns of a batch, object_id first: tensors, on the state's GPU, all [n]; -> n."""
        for name, t in zip(names, cols):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
        object_id = cols[0]
        if object_id.device.type != "cuda":
            raise RuntimeError(f"btsbot_amd.{type(self).__name__}.update runs on the GPU; there is no CPU "
                               f"fallback (object_id is on {object_id.device})")
        n = object_id.shape[0] if object_id.dim() == 1 else -1
        for name, t in zip(names, cols):
            if t.dim() != 1 or t.shape[0] != n:
                raise ValueError(f"{name} must be [{max(n, 0)}], got {tuple(t.shape)}")
        if object_id.dtype.is_floating_point or object_id.dtype == torch.bool:
            raise ValueError(f"object_id must be an integer tensor, got {object_id.dtype}")
        if object_id.device != self.device:
            raise ValueError(f"object_id is on {object_id.device}, the state on {self.device}")
        return n

    @staticmethod
    def _runs(ids: torch.Tensor, jd: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(perm, offsets): the batch grouped by object, (jd, input position) order inside one; no host read."""
        return _group_by_object(ids, then_by=jd)

    def _held_slots(self) -> torch.Tensor:
        """The slots that hold an object, in ascending id order.  One host read."""
        slots = (self._key != RESERVED_ID).nonzero()[:, 0]                               # the one host read
        return slots[torch.argsort(self._key[slots])]

    @staticmethod
    def _require(records: Mapping, keys: Sequence[str]) -> None:
        missing = [k for k in keys if k not in records]
        if missing:
            raise ValueError(f"records lack {missing}")

    def _load(self, symbol: str, m: int, fields: Sequence[Tuple[str, torch.Tensor, tuple]],
              expected: Callable[[tuple], str]) -> None:
        """The end of ``from_export``: ``fields`` are (name, tensor, the shape it must have) in the order of the load
        symbol's arguments, m the number of records (-1: object_id is not [m]).  One host read."""
        for name, t, shape in fields:
            if m < 0 or tuple(t.shape) != shape:
                raise ValueError(f"records[{name!r}] must be {expected(shape)}, got {list(t.shape)}")
        if m:
            self._call(symbol, m, *(_ptr(t) for _, t, _ in fields))
            present, no_slot = self._counters.sum(0)[4:6].tolist()                       # the one host read
            if present or no_slot:
                raise ValueError(f"from_export: {present} records carry an id that came before, {no_slot} found no slot "
                                 f"in a table of {self.capacity} (or carry the reserved id)")

    def counters(self) -> Dict[str, int]:
        """``objects`` held, alerts ``taken``, alerts ``dropped``, ``late`` alerts since the state was made or reset (a
        loaded record counts as an object, its alerts were taken elsewhere).  One host read."""
        return dict(zip(_COUNTERS, self._counters.sum(0)[:4].tolist()))
