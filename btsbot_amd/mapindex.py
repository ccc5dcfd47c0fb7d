"""Neighbours on the map: exact radius and k-nearest search for 2-D fp32 points on a uniform grid, on the device.

``EmbeddingIndex`` walks 128 x 128 tiles of split-f16 products, made for embedding rows of hundreds of columns; on a 2-D
map -- ``embedding_layout``'s result, ``EmbeddingMap.embedding_`` -- its work is quadratic in the rows while an answer
has a dozen entries.  ``MapIndex`` sorts the points into the cells of a uniform grid once and looks only at the cells an
answer can lie in (csrc/grid.hip): linear in the rows plus the output.

    mi = MapIndex(points, groups=None, cells=None)               # points float32 [N, 2]; len(mi), mi.points, mi.groups
    indptr, indices, dist = mi.radius(queries, r)                # a CSR: int64 [Q + 1], int64 [T], float32 [T]
    counts = mi.count_within(queries, r)                         # int64 [Q] == indptr.diff(), without a host read
    idx, dist = mi.query(queries, k)                             # int64 [Q, k], float32 [Q, k]

The answers are ``EmbeddingIndex``'s at D = 2 and the Euclidean metric, bit for bit where that index is exact about the
same thing.  A bank row is *eligible* if it is finite (both coordinates finite and ``fl(fl(x*x) + fl(y*y)) <= FLT_MAX``),
is not row ``self_offset + q`` and, under ``exclude_same_group``, is not of q's group.  The distance of a pair is
``sqrtf(fl(fl(t0*t0) + fl(t1*t1)))`` with ``t = q - b`` -- what ``EmbeddingIndex`` returns at D = 2.  ``radius`` holds
the eligible rows with distance ``<= r`` in fp32 (``r = +inf``: all of them; ``r = 0``: the duplicates), ``query`` the k
smallest by (distance, index), filled with ``-1 / +inf``; a non-finite query row has an empty list, a count of 0 and
``-1 / NaN``.  A row's answer does not depend, bit for bit, on the other rows of the call, on ``cells``, on the order
of the bank rows (beyond the indices themselves) or on the run: the grid only chooses which pairs are looked at, and it
provably looks at every member.  There is no CPU fallback, no cosine metric, no ``one_per_group`` and no ``add``:
rebuilding is one sort.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream
from .neighbors import _check_group_args, _check_radius_args, _csr_order, _groups

POINTS_PER_CELL = 2      # the default resolution aims at this many points per cell on uniform data
DEFAULT_MAX_CELLS = 2048  # ... with at most this many cells per axis (cell_start: 16 MiB)


def default_cells(n: int) -> int:
    """Cells per axis for ``n`` points: from ``n`` alone, so that nothing is read from the device."""
    return max(1, min(DEFAULT_MAX_CELLS, math.isqrt(max(n, 1) // POINTS_PER_CELL)))


def _points(t, name: str, device=None) -> torch.Tensor:
    """A [rows, 2] float tensor on the GPU as contiguous fp32; the shape is checked before the device."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dim() != 2 or not t.is_floating_point():
        raise ValueError(f"{name} must be a floating-point [rows, 2] tensor, got {t.dtype} {tuple(t.shape)}")
    if t.shape[1] != 2:
        raise ValueError(f"{name}: the grid holds 2-D points, got D = {t.shape[1]}")
    if t.shape[0] >= 1 << 31:
        raise ValueError(f"{name}: at most 2^31 - 1 rows, got {t.shape[0]}")
    if t.device.type != "cuda":
        raise RuntimeError(f"btsbot_amd.mapindex runs on the GPU; there is no CPU fallback ({name} is on {t.device})")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, the index on {device}")
    return t.detach().to(torch.float32).contiguous()


def _check_cells(cells) -> None:
    if cells is not None and (isinstance(cells, bool) or not isinstance(cells, int)
                              or not 1 <= cells <= _lib.GRID_MAX_CELLS):
        raise ValueError(f"cells must be None or an int in 1..{_lib.GRID_MAX_CELLS}, got {cells!r}")


def _check_k(k) -> None:
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= _lib.GRID_MAX_K:
        raise ValueError(f"k must be an int in 1..{_lib.GRID_MAX_K}, got {k!r}")


def check_grid_method(dim, metric: str, one_per_group: bool = False, group_mode: str = "exclude") -> None:
    """ValueError for what ``method="grid"`` cannot answer (the graph functions call it before anything else)."""
    if metric != "euclidean":
        raise ValueError(f'method="grid" knows the euclidean metric only, got {metric!r}')
    if one_per_group or group_mode != "exclude":
        raise ValueError('method="grid" knows group_mode="exclude" only (no one_per_group / "distinct"), got '
                         f"{group_mode!r}")
    if dim is not None and dim != 2:
        raise ValueError(f'method="grid" holds 2-D points, got D = {dim}')


class MapIndex:
    """2-D points on one GPU, sorted into the cells of a uniform grid over the bounding box of the finite ones.

    groups: one int64 group per point (an alert's object), or None; ``exclude_same_group`` needs them.
    cells: cells per axis (None: ``default_cells(N)``); no answer depends on it.

    Built by three launches, a stable sort and a ``searchsorted``, without a host read.  Calls on one index must be
    ordered by the caller's streams."""

    def __init__(self, points: torch.Tensor, *, groups: Optional[torch.Tensor] = None, cells: Optional[int] = None):
        _check_cells(cells)
        pts = _points(points, "points")
        self.device = dev = pts.device
        n = int(pts.shape[0])
        self._n = n
        self._points = pts
        self._groups = None if groups is None else _groups(groups, "groups", n, dev)
        self.cells = G = default_cells(n) if cells is None else cells
        self._lanes = 0   # lanes per query row of the radius kernels (0: the library's choice); tools/map_index_bench.py
        L = _lib.lib()
        inf = float("inf")
        with torch.cuda.device(dev):
            finite = torch.empty(n, dtype=torch.uint8, device=dev)
            _lib.check(L.btsbot_grid_finite(_ptr(pts), n, _ptr(finite), _stream(self.device)), "btsbot_grid_finite")
            if n:
                fin = finite.view(torch.bool)[:, None]
                bbox = torch.cat([torch.where(fin, pts, pts.new_full((), inf)).amin(dim=0),
                                  torch.where(fin, pts, pts.new_full((), -inf)).amax(dim=0)]).contiguous()
            else:
                bbox = torch.tensor([inf, inf, -inf, -inf], dtype=torch.float32, device=dev)
            self._geom = torch.empty(4, dtype=torch.float32, device=dev)
            cell = torch.empty(n, dtype=torch.int32, device=dev)
            _lib.check(L.btsbot_grid_cells(_ptr(pts), n, C.c_void_p(bbox.data_ptr()), G, C.c_void_p(self._geom.data_ptr()),
                                           _ptr(cell), _stream(self.device)), "btsbot_grid_cells")
            cell, order = torch.sort(cell, stable=True)
            self._cell_start = torch.searchsorted(cell, torch.arange(G * G + 1, dtype=torch.int32, device=dev)
                                                  ).to(torch.int32).contiguous()
            self._sorted_points = pts[order].contiguous()
            self._sorted_rows = order.to(torch.int32).contiguous()
            self._sorted_groups = None if self._groups is None else self._groups[order].contiguous()

    def __len__(self) -> int:
        return self._n

    @property
    def points(self) -> torch.Tensor:
        """The fp32 points held, [len, 2], in the order they were given."""
        return self._points

    @property
    def groups(self) -> Optional[torch.Tensor]:
        """The points' groups, int64 [len], or None."""
        return self._groups

    def _grid_args(self, self_offset: int, query_groups, flags: int):
        return (C.c_void_p(self._geom.data_ptr()), self.cells, C.c_void_p(self._cell_start.data_ptr()),
                _ptr(self._sorted_points), _ptr(self._sorted_rows), _ptr(self._sorted_groups) if flags else None, self._n,
                self_offset, _ptr(query_groups) if flags else None, flags)

    def _query_args(self, queries, query_groups, exclude_same_group, self_offset):
        flags = _check_group_args(1, self._groups is not None, query_groups, exclude_same_group, False)
        q = _points(queries, "queries", self.device)
        if isinstance(self_offset, bool) or not isinstance(self_offset, int):
            raise ValueError(f"self_offset must be an int, got {self_offset!r}")
        if query_groups is not None:
            query_groups = _groups(query_groups, "query_groups", int(q.shape[0]), self.device)
        return q, query_groups, flags

    def _radii(self, r, nq: int) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """(fp32 [Q] radii, a device flag "some radius is negative or NaN" or None for a float)"""
        if isinstance(r, torch.Tensor):
            if r.device != self.device:
                raise ValueError(f"r is on {r.device}, the index on {self.device}")
            rad = r.detach().to(torch.float32).contiguous()
            return rad, (~(rad >= 0)).any().to(torch.int64)
        return torch.full((nq,), float(r), dtype=torch.float32, device=self.device), None   # rounded to fp32 once

    def _count(self, q, rad, grid, visited: bool):
        nq = int(q.shape[0])
        counts = torch.zeros(nq, dtype=torch.int64, device=self.device)
        vis = torch.zeros(nq, dtype=torch.int64, device=self.device) if visited else None
        _lib.check(_lib.lib().btsbot_grid_radius_count(_ptr(q), nq, _ptr(rad), *grid, self._lanes, _ptr(counts), _ptr(vis),
                                                       _stream(self.device)), "btsbot_grid_radius_count")
        return counts, vis

    def radius(self, queries: torch.Tensor, r, *, query_groups: Optional[torch.Tensor] = None,
               exclude_same_group: bool = False, self_offset: int = -1, sort: str = "index",
               max_total: Optional[int] = None,
               stats: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Every eligible point within ``r`` of each query row, as a CSR: ``indptr`` int64 [Q + 1], ``indices`` int64
        [T], ``dist`` float32 [T].  r: a float (rounded to fp32 once) or a float tensor [Q] of per-row radii; negative or
        NaN is a ``ValueError``.  sort: ``"index"`` orders a row's list by bank index, ``"distance"`` by (dist, index).
        max_total: ValueError (naming the total) instead of lists longer than this in all, raised before they are
        written.  stats: a dict that receives ``visited`` (the pairs whose distance was computed, once per pass),
        ``total`` and ``error_flag`` (the fill kernel's bounds check; 0, or the call raises).  self_offset >= 0: query
        row i is row i + self_offset of the index and is not in its own list.  The count and the fill kernel walk the
        same cells; the host reads the total between them, to allocate, and the error flag at the end."""
        _check_radius_args(r, int(queries.shape[0]) if isinstance(queries, torch.Tensor) and queries.dim() == 2 else None,
                           sort, 0, max_total)
        q, query_groups, flags = self._query_args(queries, query_groups, exclude_same_group, self_offset)
        nq, dev = int(q.shape[0]), self.device
        L = _lib.lib()
        with torch.cuda.device(dev):
            rad, bad = self._radii(r, nq)
            grid = self._grid_args(self_offset, query_groups, flags)
            counts, vis = self._count(q, rad, grid, stats is not None)
            indptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            indptr[1:] = torch.cumsum(counts, 0)
            zero = indptr.new_zeros(())
            total, bad, visited = torch.stack([indptr[-1], zero if bad is None else bad,
                                               zero if vis is None else vis.sum()]).tolist()   # the one sizing read
            if bad:
                raise ValueError("r must be >= 0 in every row (and not NaN)")
            if max_total is not None and total > max_total:
                raise ValueError(f"the lists hold T = {total} entries, more than max_total = {max_total}")
            cand = torch.empty(total, dtype=torch.int32, device=dev)
            dist = torch.empty(total, dtype=torch.float32, device=dev)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(L.btsbot_grid_radius_fill(_ptr(q), nq, _ptr(rad), *grid, self._lanes, _ptr(indptr), total,
                                                 _ptr(cand), _ptr(dist), C.c_void_p(err.data_ptr()), _stream(self.device)),
                       "btsbot_grid_radius_fill")
            rows = torch.repeat_interleave(torch.arange(nq, device=dev), counts, output_size=total)
            order = _csr_order(rows, cand.to(torch.int64), dist, max(self._n, 1), sort)
            indices, dist = cand[order].to(torch.int64), dist[order]
            flag = int(err.item())
            if stats is not None:
                stats.update(visited=int(visited), total=int(total), error_flag=flag)
            if flag:
                raise RuntimeError("btsbot_grid_radius_fill: a member fell past the end of its row's region (the count "
                                   "and the fill pass disagree); the lists are not returned")
            return indptr, indices, dist

    def count_within(self, queries: torch.Tensor, r, *, query_groups: Optional[torch.Tensor] = None,
                     exclude_same_group: bool = False, self_offset: int = -1) -> torch.Tensor:
        """int64 [Q]: how many eligible points lie within ``r`` of each query row -- the ``indptr.diff()`` of ``radius``
        with the same arguments, from the count pass alone: no lists, no host read.  (A negative or NaN entry of a
        radius TENSOR on the device cannot raise here; such a row counts 0.)"""
        _check_radius_args(r, int(queries.shape[0]) if isinstance(queries, torch.Tensor) and queries.dim() == 2 else None,
                           "index", 0, None)
        q, query_groups, flags = self._query_args(queries, query_groups, exclude_same_group, self_offset)
        with torch.cuda.device(self.device):
            rad, _bad = self._radii(r, int(q.shape[0]))
            return self._count(q, rad, self._grid_args(self_offset, query_groups, flags), False)[0]

    def query(self, queries: torch.Tensor, k: int, *, query_groups: Optional[torch.Tensor] = None,
              exclude_same_group: bool = False, self_offset: int = -1) -> Tuple[torch.Tensor, torch.Tensor]:
        """``idx`` int64 [Q, k] and ``dist`` float32 [Q, k]: each query row's ``k`` nearest eligible points, ordered by
        (dist, index); ``-1 / +inf`` where fewer are eligible, ``-1 / NaN`` for a non-finite query row.  One launch, no
        host read."""
        _check_k(k)
        q, query_groups, flags = self._query_args(queries, query_groups, exclude_same_group, self_offset)
        nq = int(q.shape[0])
        idx = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        dist = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().btsbot_grid_knn(_ptr(q), nq, k, *self._grid_args(self_offset, query_groups, flags),
                                                  _ptr(idx), _ptr(dist), _stream(self.device)), "btsbot_grid_knn")
        return idx, dist
