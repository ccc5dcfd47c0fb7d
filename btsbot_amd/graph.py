"""The neighbour graph of an archive, kept current while the archive grows and forgets (csrc/knn_graph.hip, DESIGN.md
sections 4x and 4y).

Every analysis of embedding rows starts from the graph of all rows among all rows -- the local outlier factor, the layout's
fuzzy graph, HDBSCAN's core distances -- and that graph is the whole cost of each.  ``EmbeddingIndex.add`` packs only the
new rows; a ``KnnGraph`` beside the index follows it at the cost of the new rows, not of the history:

    index = EmbeddingIndex(bank, groups=obj)
    g = KnnGraph(index, 20)                      # knn_graph(bank, 20, include_self=False, ...), kept
    g.idx, g.dist                                # int64 / float32 [len(g), k], views of storage that grows by doubling
    index.add(rows, groups=obj_new)
    g.update()                                   # brings the graph to len(index): Q x (N + Q) and N x Q pairs, not (N + Q)^2
    kept = index.remove(old)                     # rows leave the index (a stable compaction)
    g.update()                                   # follows: one pass over the lists, one query for the damaged rows
    g.rebuild()                                  # from scratch: one index.query(bank, k, self_offset=0, ...)
    lof = local_outlier_factor(None, 20, knn=(g.idx, g.dist))
    fg = fuzzy_graph(*g.self_first())            # (idx, dist) [N, k + 1], the row itself in column 0

Adding ``Q`` rows to ``N`` changes the graph in two ways only.  The new rows need lists: ``index.query(new, k,
self_offset=n0, ...)``.  An old row's list changes only by new rows entering it: a temporary index of the new rows answers
``radius(old rows, r, sort="distance")`` with ``r`` each old row's current k-th distance (``+inf`` where the list is not
full), and ``btsbot_knn_graph_merge`` merges these offers into the lists in place, one wave per row.

What an updated graph promises:
  (A) every list is valid in ``knn_graph``'s sense, and its ``dist`` is the direct-form fp32 distance of that very pair,
      the bits ``query`` / ``radius`` / ``rank_of`` return for it;
  (B) an old row's list is exactly the first ``k`` -- by fp32 (dist, index), and in the ``"distinct"`` modes emitting an
      entry only if its group differs from every entry before it -- of (its list before) united with (every eligible new
      row); a new row's list is ``index.query``'s;
  (C) hence the updated graph equals the rebuilt one on every row that has no second candidate within the tile search's
      selection band at its k-th place, and on integer-coordinate rows everywhere.  Where two candidates lie inside that
      band (``tau``) the two graphs may hold different, equally admissible rows: ``query`` selects exactly
      only up to ``tau``, so no bit-for-bit promise against a rebuild is made there.
A row's answer does not depend on ``splits`` or on the run.  However the adds are cut, (B) holds, and an OLD row's list is
the same bit for bit (``add(A); update(); add(B); update()`` against ``add(A + B); update()``); the lists of the rows of A
agree where (C) says so.

``update`` reads the host where ``radius`` does (twice, to size the candidates and the lists) and once more for ``stats``;
the rest is queued on the current stream.  There is no CPU fallback.

After ``index.remove``.  The graph keeps a copy of the ids it covers (``index.ids``, 8 bytes per row) and sees from
``index.generation`` that rows have left.  A removal changes the graph in two ways only.  A surviving row whose list held
none of the removed rows keeps its list, renumbered; a surviving row whose list lost an entry needs the next-nearest rows.
``btsbot_knn_graph_compact`` writes every survivor's list -- the entries whose row survived, renumbered, in order -- into a
second pair of arrays (the graph takes twice its memory for the call) and marks the DAMAGED rows: those that lost an entry
and whose list was full (in the ``"distinct"`` modes: any that lost an entry, since a further row of the lost entry's group
may surface; in the plain modes a list with a free slot held every eligible row, so what is left is complete).  The rows
added since go through the add path above, with radius 0 for a damaged row, and the damaged rows then get one
``index.query(bank[rows], k, self_rows=rows, ...)``.  ``group_mode="distinct"`` alone cannot mask a row and keep its
group: a damaged row there rebuilds the graph (``stats["rebuilt"]``).  The cost is (damaged rows) x N pairs and one
streaming pass, not N x N.

What an update after removals promises:
  (R1) the compacted list C_a of a surviving old row is its present entries whose row survived, renumbered, in order, with
       the same ``dist`` bits and a -1 / +inf tail;
  (R2) an undamaged row's list is rule (B) applied to C_a and the eligible new rows; with no new rows it is C_a, bit for
       bit;
  (R3) a damaged row's list is ``index.query``'s for that row with itself excluded and the graph's group switches;
  (R4) hence the updated graph equals the rebuilt one wherever (C) already says so: on every separated row, and on
       integer-coordinate rows everywhere.
(A) holds throughout, and a row's answer does not depend on ``splits``, on how removals and adds are cut between updates,
or on the run.  Beyond today's host reads, an update after a removal reads the survivor count and the damaged rows.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from . import _lib
from .mapindex import MapIndex
from ._lib import ptr as _ptr, stream as _stream
from .neighbors import GROUP_MODES, EmbeddingIndex, _check_group_args, _check_k, _metric

__all__ = ["KnnGraph"]


class KnnGraph:
    """``knn_graph(index.bank, k, include_self=False, ...)`` kept beside an ``EmbeddingIndex`` (see the module text).

    rows_or_index: rows float [N, D] (an ``EmbeddingIndex`` is built on them, with ``groups``) or an ``EmbeddingIndex``,
    which brings its own metric and groups: ``groups=`` next to an index is a ``ValueError``.  A ``MapIndex`` is a
    ``ValueError``: it has no ``add``, and rebuilding its graph is one sort.  ``k``, ``group_mode`` and ``splits`` are
    ``knn_graph``'s (``k <= 32`` in the ``"distinct"`` modes, ``k <= 64`` otherwise); ``group_mode`` means nothing without
    groups.  ``update()`` follows ``index.add`` and ``index.remove`` alike; the graph keeps the ids of the rows it covers
    (8 bytes per row) to see which have left.  Calls on one graph and its index must be ordered by the caller's
    streams."""

    def __init__(self, rows_or_index: Union[torch.Tensor, EmbeddingIndex], k: int, metric: str = "euclidean", *,
                 groups: Optional[torch.Tensor] = None, group_mode: str = "exclude", splits: int = 0):
        if isinstance(rows_or_index, MapIndex):
            raise ValueError("a KnnGraph follows an EmbeddingIndex; a MapIndex has no add (rebuilding its graph is one "
                             'sort: knn_graph(points, k, method="grid"))')
        _check_k(k, splits)
        _metric(metric)
        if group_mode not in GROUP_MODES:
            raise ValueError(f"group_mode must be one of {GROUP_MODES}, got {group_mode!r}")
        if isinstance(rows_or_index, EmbeddingIndex):
            index = rows_or_index
            if groups is not None:
                raise ValueError("groups= next to an index: the graph uses the index's own groups (build the index with "
                                 "groups=...)" + ("" if index.groups is None else "; this one already has them"))
            if metric != index.metric:
                raise ValueError(f"metric = {metric!r}, the index holds {index.metric!r}")
        else:
            if groups is not None:
                _check_group_args(k, True, groups, "exclude" in group_mode, "distinct" in group_mode)
            index = EmbeddingIndex(rows_or_index, metric, groups=groups)
        self._exclude = index.groups is not None and "exclude" in group_mode
        self._distinct = index.groups is not None and "distinct" in group_mode
        if index.groups is not None:
            _check_group_args(k, True, index.groups, self._exclude, self._distinct)
        self.index = index
        self.k = k
        self.metric = index.metric
        self.group_mode = group_mode
        self.splits = splits
        self.device = index.device
        self._n = 0
        self._ids = index.ids[:0]
        self._generation = index.generation
        self._idx = torch.empty((0, k), dtype=torch.int64, device=self.device)
        self._dist = torch.empty((0, k), dtype=torch.float32, device=self.device)
        self.rebuild()

    def __len__(self) -> int:
        """The rows the graph covers."""
        return self._n

    @property
    def idx(self) -> torch.Tensor:
        """int64 [len, k] (a view of the graph's storage)."""
        return self._idx[:self._n]

    @property
    def dist(self) -> torch.Tensor:
        """float32 [len, k] (a view of the graph's storage)."""
        return self._dist[:self._n]

    def _group_kw(self, lo: int, hi: int) -> dict:
        """The group arguments of ``query`` for the index's rows lo..hi as query rows."""
        if self.index.groups is None:
            return {}
        return dict(query_groups=self.index.groups[lo:hi], exclude_same_group=self._exclude, one_per_group=self._distinct)

    def _reserve(self, n: int) -> None:
        """Room for n rows; what is held moves once per doubling, as in the index."""
        cap = int(self._idx.shape[0])
        if n <= cap:
            return
        cap = max(n, 2 * cap)
        idx = torch.empty((cap, self.k), dtype=torch.int64, device=self.device)
        dist = torch.empty((cap, self.k), dtype=torch.float32, device=self.device)
        idx[:self._n].copy_(self._idx[:self._n])
        dist[:self._n].copy_(self._dist[:self._n])
        self._idx, self._dist = idx, dist

    def rebuild(self) -> "KnnGraph":
        """The graph of the rows the index holds now, from scratch: one ``index.query(bank, k, self_offset=0, ...)``."""
        n = len(self.index)
        with torch.cuda.device(self.device):
            idx, dist = self.index.query(self.index.bank, self.k, splits=self.splits, self_offset=0, **self._group_kw(0, n))
            if n > int(self._idx.shape[0]):
                self._idx, self._dist = idx, dist          # (the search's own output becomes the storage)
            else:
                self._idx[:n].copy_(idx)
                self._dist[:n].copy_(dist)
        self._n = n
        self._follow()
        return self

    def _follow(self) -> None:
        """Remembers which rows of the index the graph now covers: their ids and the index's generation."""
        self._ids = self.index.ids[:self._n].clone()
        self._generation = self.index.generation

    def _radii(self, n0: int, damaged: Optional[torch.Tensor] = None) -> torch.Tensor:
        """float32 [n0]: what a new row must not exceed to enter an old row's list -- the last distance of a full list
        (not below 0: ``1 - cos`` may round there), ``+inf`` for a list with a free slot, 0 for the -1 / NaN list of a
        non-finite row (whose radius list is empty anyway) and for a row ``damaged`` (uint8 [n0]) marks: its list is
        replaced by a query, and ``+inf`` would offer it every new row."""
        last_i, last_d = self._idx[:n0, self.k - 1], self._dist[:n0, self.k - 1]
        r = torch.where(last_i >= 0, last_d.clamp(min=0), torch.full_like(last_d, float("inf")))
        r = torch.where(torch.isnan(self._dist[:n0, 0]), torch.zeros_like(r), r)
        return r if damaged is None else torch.where(damaged != 0, torch.zeros_like(r), r)

    def _offers(self, n0: int, n1: int, stats: Optional[dict] = None,
                damaged: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The CSR of (new row, distance) per old row, by (dist, index), the new rows numbered as the index numbers
        them."""
        index = self.index
        tmp = EmbeddingIndex(index.bank[n0:n1], self.metric, groups=None if index.groups is None else index.groups[n0:n1])
        kw = {}
        if self._exclude:
            kw = dict(query_groups=index.groups[:n0], exclude_same_group=True)
        indptr, off_idx, off_dist = tmp.radius(index.bank[:n0], self._radii(n0, damaged), sort="distance",
                                               splits=self.splits, stats=stats, **kw)
        return indptr, off_idx + n0, off_dist

    def _merge(self, n0: int, indptr: torch.Tensor, off_idx: torch.Tensor, off_dist: torch.Tensor,
               changed_count: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None) -> None:
        """btsbot_knn_graph_merge on the graph's first n0 rows.  rows: None, every row is visited and one without offers
        leaves at once; or int64, the rows to visit.  changed_count: int32 [1], the changed rows are added to it."""
        groups = self.index.groups if self._distinct else None
        _lib.check(_lib.lib().btsbot_knn_graph_merge(
            _ptr(self._idx), _ptr(self._dist), self.k, self.k, n0, _ptr(indptr), _ptr(off_idx), _ptr(off_dist),
            int(off_idx.shape[0]), _ptr(groups), 0 if groups is None else int(groups.shape[0]),
            _lib.KNN_GRAPH_DISTINCT if self._distinct else 0, _ptr(rows), 0 if rows is None else int(rows.shape[0]),
            None, _ptr(changed_count), _stream(self.device)),
            "btsbot_knn_graph_merge")

    def update(self, stats: Optional[dict] = None) -> "KnnGraph":
        """Brings the graph to the rows the index holds now, after ``index.add`` and ``index.remove`` (the module text
        has the steps and what the result promises); a no-op when nothing changed.  stats: a dict that receives
        ``new_rows``, ``offers`` (new rows within an old row's k-th distance, in all), ``touched`` (old rows with at least
        one offer), ``changed`` (old rows whose list differs after the merge) and ``candidates`` (the pairs the reverse
        search verified in the direct form); and, only when the call followed a removal, ``removed`` (old rows gone),
        ``damaged`` (rows searched again) and ``rebuilt`` (True: ``group_mode="distinct"`` had a damaged row and the
        graph was built from scratch).  Reads the host where ``radius`` does, twice, and once more for ``stats``; after a
        removal also for the survivor count and for the damaged rows.  Returns the graph."""
        if self.index.generation != self._generation:
            return self._update_after_removal(stats)
        n0, n1 = self._n, len(self.index)
        if stats is not None:
            stats.update(new_rows=n1 - n0, offers=0, touched=0, changed=0, candidates=0)
        if n1 == n0:
            return self
        with torch.cuda.device(self.device):
            self._reserve(n1)
            self._grow(n0, n1, stats)
        self._n = n1
        self._follow()
        return self

    def _grow(self, n0: int, n1: int, stats: Optional[dict], damaged: Optional[torch.Tensor] = None) -> None:
        """The add half: the lists of the index's rows n0..n1, and their offers merged into the lists of rows 0..n0
        (``damaged``: ``_radii``'s).  The storage holds n1 rows."""
        index = self.index
        idx, dist = index.query(index.bank[n0:n1], self.k, splits=self.splits, self_offset=n0, **self._group_kw(n0, n1))
        self._idx[n0:n1].copy_(idx)
        self._dist[n0:n1].copy_(dist)
        if n0:
            st = {}
            indptr, off_idx, off_dist = self._offers(n0, n1, st, damaged)
            changed = torch.zeros(1, dtype=torch.int32, device=self.device) if stats is not None else None
            self._merge(n0, indptr, off_idx, off_dist, changed)
            if stats is not None:
                touched, n_changed = torch.stack([(indptr.diff() > 0).sum(), changed[0].to(torch.int64)]).tolist()
                stats.update(offers=int(off_idx.shape[0]), touched=int(touched), changed=int(n_changed),
                             candidates=int(st["candidates"]))

    def _update_after_removal(self, stats: Optional[dict]) -> "KnnGraph":
        """``update`` when ``index.generation`` has moved since the graph last followed the index."""
        index, k, dev = self.index, self.k, self.device
        n0, n1 = self._n, len(index)
        with torch.cuda.device(dev):
            # where each row the graph covers stands now: survivors keep their order, so they are rows 0..s-1 of the
            # index, and rows s..n1-1 were added since (and are still there)
            if n1:
                now = index.ids
                pos = torch.searchsorted(now, self._ids).clamp(max=n1 - 1)
                new_of_old = torch.where(now[pos] == self._ids, pos, torch.full_like(pos, -1))
            else:
                new_of_old = torch.full((n0,), -1, dtype=torch.int64, device=dev)
            s = int((new_of_old >= 0).sum()) if n0 else 0                   # the host read for the survivor count
            if stats is not None:
                stats.update(new_rows=n1 - s, offers=0, touched=0, changed=0, candidates=0, removed=n0 - s, damaged=0,
                             rebuilt=False)
            rows = new_of_old[:0]
            damaged = None
            if s < n0:
                idx = torch.empty((max(n1, 1), k), dtype=torch.int64, device=dev)
                dist = torch.empty((max(n1, 1), k), dtype=torch.float32, device=dev)
                damaged = torch.zeros(s, dtype=torch.uint8, device=dev)
                _lib.check(_lib.lib().btsbot_knn_graph_compact(
                    _ptr(self._idx), _ptr(self._dist), k, k, n0, _ptr(new_of_old), _ptr(idx), _ptr(dist), k, s,
                    _lib.KNN_GRAPH_DISTINCT if self._distinct else 0, _ptr(damaged), None, _stream(dev)),
                    "btsbot_knn_graph_compact")
                self._idx, self._dist, self._n = idx, dist, s
                rows = damaged.nonzero().view(-1)                             # the host read for the damaged rows
            else:
                self._reserve(n1)
            n_damaged = int(rows.shape[0])
            if stats is not None:
                stats.update(damaged=n_damaged)
            if n_damaged and self._distinct and not self._exclude:
                # "distinct" alone cannot mask the row itself while keeping its group
                if stats is not None:
                    stats.update(rebuilt=True)
                return self.rebuild()
            if n1 > s:
                self._grow(s, n1, stats, damaged if n_damaged else None)
            if n_damaged:
                kw = {}
                if index.groups is not None:
                    kw = dict(query_groups=index.groups[rows], exclude_same_group=self._exclude,
                              one_per_group=self._distinct)
                idx, dist = index.query(index.bank[rows], k, splits=self.splits, self_rows=rows, **kw)
                self._idx[rows] = idx
                self._dist[rows] = dist
        self._n = n1
        self._follow()
        return self

    def self_first(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(idx, dist)`` [N, k + 1] with the row itself in column 0 at distance 0 (-1 / NaN for a non-finite row): the
        layout of ``knn_graph(bank, k + 1, include_self=True, ...)``, which ``fuzzy_graph`` and ``embedding_layout(knn=)``
        take.  New tensors; nothing is read from the host."""
        n, rows = self._n, self.index.bank[:self._n]
        idx = torch.empty((n, self.k + 1), dtype=torch.int64, device=self.device)
        dist = torch.empty((n, self.k + 1), dtype=torch.float32, device=self.device)
        finite = torch.isfinite(rows).all(dim=1)
        idx[:, 0] = torch.where(finite, torch.arange(n, device=self.device), torch.full_like(idx[:, 0], -1))
        dist[:, 0] = torch.where(finite, torch.zeros_like(dist[:, 0]), torch.full_like(dist[:, 0], float("nan")))
        idx[:, 1:], dist[:, 1:] = self.idx, self.dist
        return idx, dist
