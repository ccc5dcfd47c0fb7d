"""What the per-object streaming states (``TriggerState``, ``FeatureState``) share: a hash table of object ids on the
device (csrc/object_table.h) with a record per object, advanced by one launch per batch.  The base owns the checks of a
batch's columns, the grouping, the slots an export reads, the end of a load and retention (``expire``, ``resize``: the
survivors are re-inserted into a second table on the device, nothing is deleted in place); a state adds the list of its
table's arrays (``_ARRAYS``), a hook that allocates them with the ctypes table struct over them (``_allocate``), what an
export gathers from them (``_records``) and its kernel calls."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Mapping, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream
from .alert_utils import _group_by_object

RESERVED_ID = -(1 << 63)          # BTSBOT_TRIGGER_FREE: the free-slot marker, the one id a state cannot hold
_COUNTERS = ("objects", "taken", "dropped", "late")


def _check_capacity(capacity) -> None:
    if not isinstance(capacity, int) or capacity < 1 or capacity & (capacity - 1) or capacity > 1 << 30:
        raise ValueError(f"capacity must be a power of two (at most 2^30), got {capacity!r}")


def _check_jd(before_jd, optional: bool = False) -> None:
    if not isinstance(before_jd, float) and not (optional and before_jd is None):
        raise ValueError(f"before_jd must be a float{' or None' if optional else ''}, got {type(before_jd).__name__}")


class ObjectState:
    _RESET = ""                   # the state's reset symbol
    _REHASH = ""                  # the state's rehash symbol
    _ARRAYS: Tuple[str, ...] = ()  # the attributes that hold the table's arrays, in the order of the ctypes struct:
    #                                "_key", "_n", the state's own (one of them "_last"), "_counters"

    def __init__(self, capacity: int, device):
        """Checks capacity and device, then allocates the table (the state's ``_allocate``, which may use what the state
        set before it called this) and resets it."""
        _check_capacity(capacity)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"btsbot_amd.{type(self).__name__} runs on the GPU; there is no CPU fallback "
                               f"(device is {dev})")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self._install(capacity, *self._allocate(capacity))
        self.reset()

    def _allocate(self, capacity: int):
        """The state's hook: (its arrays, uninitialised, at ``capacity`` slots in the order of ``_ARRAYS``; the ctypes
        table struct over them)."""
        raise NotImplementedError

    def _empty(self, capacity: int, record: Sequence[Tuple[tuple, torch.dtype]]) -> list:
        """key, n_alerts, the state's ``record`` arrays ((shape after [capacity], dtype) each) and the counters."""
        spec = [((), torch.int64), ((), torch.int32), *record]
        return [torch.empty((capacity,) + tuple(shape), dtype=dtype, device=self.device) for shape, dtype in spec] + [
            torch.empty((_lib.TRIGGER_COUNTER_ROWS, 8), dtype=torch.int64, device=self.device)]

    def _install(self, capacity: int, arrays: Sequence[torch.Tensor], table) -> None:
        self.capacity, self._table = capacity, table
        for name, t in zip(self._ARRAYS, arrays):
            setattr(self, name, t)

    def _installed(self):
        return self.capacity, [getattr(self, name) for name in self._ARRAYS], self._table

    def _call(self, symbol: str, *args) -> None:
        """symbol(table, *args, stream) on the state's device."""
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.lib(), symbol)(C.byref(self._table), *args, _stream(self.device)), symbol)

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

    @staticmethod
    def _slots(held: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
        """The slots of the mask ``held``, in ascending id order.  One host read."""
        slots = held.nonzero()[:, 0]                                                     # the one host read
        return slots[torch.argsort(key[slots])]

    def _held_slots(self) -> torch.Tensor:
        """The slots that hold an object, in ascending id order.  One host read."""
        return self._slots(self._key != RESERVED_ID, self._key)

    def _records(self, arrays: Sequence[torch.Tensor], slots: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The state's hook: what ``export()`` returns, gathered from ``arrays`` (in the order of ``_ARRAYS``) at ``slots``."""
        raise NotImplementedError

    # ---- retention
    def _rebuild(self, capacity: int, keep_from: float):
        """The objects with last_jd >= keep_from (or NaN) into a second table of ``capacity`` slots, which becomes the
        state's: allocate, reset, one rehash launch, swap.  -> what was installed before, untouched (the rehash only reads
        it).  No host synchronisation."""
        old = self._installed()
        arrays, table = self._allocate(capacity)
        L, stream = _lib.lib(), _stream(self.device)
        with torch.cuda.device(self.device):
            _lib.check(getattr(L, self._RESET)(C.byref(table), stream), self._RESET)
            _lib.check(getattr(L, self._REHASH)(C.byref(old[2]), C.byref(table), C.c_double(keep_from), stream),
                       self._REHASH)
        for t in old[1]:          # (the old arrays may have been allocated on another stream than the one that reads them now)
            t.record_stream(torch.cuda.current_stream(self.device))
        self._install(capacity, arrays, table)
        return old

    def expire(self, before_jd: float, return_expired: bool = False):
        """Forget every object whose last_jd < before_jd (a Python float): its slot is free again, and the probe chains
        are as short as if it had never been there.  The comparison is exactly that one: a record with a NaN last_jd
        stays, ``-inf`` and NaN expire nothing, ``+inf`` every record whose last_jd is a number.  An object that comes
        back later is a NEW object: it is counted again, a trigger state's policies may fire on it again, a feature
        state's ``*_so_far`` and peak columns start again (``age`` still follows the packet's jdstarthist).

        The survivors are re-inserted into a second set of the state's arrays on the device (nothing is deleted in place,
        ``update`` is untouched), so for the length of the call the state takes twice its memory; torch's caching
        allocator hands the released set to the next call.  ``counters()`` goes on across the call (``objects`` drops by
        the number expired, which ``n_expired()`` accumulates).

        No host synchronisation: an allocation, the reset and one launch are queued on the current stream, and nothing
        on this path reads a device value on the host.  With ``return_expired`` the removed records are gathered from the
        old arrays before they are released and returned in the form of ``export()`` (same keys, dtypes, ascending ids),
        at the price of one host read."""
        _check_jd(before_jd)
        _, old, _ = self._rebuild(self.capacity, before_jd)
        if not return_expired:
            return None
        key, last = old[0], old[self._ARRAYS.index("_last")]
        return self._records(old, self._slots((key != RESERVED_ID) & (last < before_jd), key))

    def resize(self, capacity: int, before_jd: Optional[float] = None) -> None:
        """The same records in a table of ``capacity`` slots (a power of two, larger or smaller), without the objects
        ``expire(before_jd)`` would forget when ``before_jd`` is given.  Everyone who holds the state keeps holding it.
        Raises ValueError, and leaves the state exactly as it was, when the records do not fit.  Peak memory: both tables.
        One host read (the number of records that found no slot)."""
        _check_capacity(capacity)
        _check_jd(before_jd, optional=True)
        old = self._rebuild(capacity, float("-inf") if before_jd is None else before_jd)
        no_slot = int(self._counters[:, 7].sum())                                        # the one host read
        if no_slot:
            self._install(*old)
            raise ValueError(f"resize: {no_slot} objects found no slot in a table of {capacity}; the state keeps its "
                             f"table of {self.capacity}")

    def n_expired(self) -> int:
        """Objects expired since the state was made or reset.  One host read."""
        return int(self._counters[:, 6].sum())

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
