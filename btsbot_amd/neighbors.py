"""Similar alerts: exact k-nearest neighbours over embedding rows, on the device.

``model.embed(...)`` and ``ScoreStream(embed=...)`` hand out a learned vector per alert; this module answers "which rows
of an archive lie nearest to these" without ever forming the [Q, N] distance matrix (csrc/knn*.hip):

    idx, dist = embedding_neighbors(queries, bank, k)            # int64 [Q, k], float32 [Q, k]
    index = EmbeddingIndex(bank)                                 # packs the bank once
    index.add(more_rows)                                         # packs only the new rows
    kept = index.remove(mask_or_rows)                            # stable compaction; side = side[kept] stays aligned
    idx, dist = index.query(queries, k)
    idx, dist = knn_graph(emb, k)                                # every row among the others (self first, distance 0)

``dist`` is the Euclidean distance (not squared) or, with ``metric="cosine"``, ``1 - cos`` (``cos = 0`` for a zero row),
recomputed for the returned rows in the direct form from the fp32 rows.  Rows are ordered by (dist, bank index).  Where
fewer than ``k`` bank rows are eligible the tail is ``idx = -1, dist = +inf``; a bank row that holds a non-finite value is
never returned; a query row that does gets ``idx = -1, dist = NaN`` throughout.  A row's answer does not depend, bit for
bit, on the other rows of the call, on ``splits`` or on the run.  Nothing here synchronises with the host; the work is
queued on the current stream.  There is no CPU fallback.

Rows that belong together.  A row is one alert, and the alerts of one object are near-copies of each other, so the search
can be told which rows belong together: a *group* is an int64 per row, any value (``alert_utils.object_keys``).

    index = EmbeddingIndex(bank, groups=obj)                     # one group per bank row; add(rows, groups=...)
    idx, dist = index.query(q, k, query_groups=obj_q, exclude_same_group=True)   # never a row of the query's own group
    idx, dist = index.query(q, k, one_per_group=True)            # the k nearest GROUPS, each by its nearest row
    idx, dist = knn_graph(emb, k, groups=obj, group_mode="exclude")              # self first, then rows of OTHER groups
    score = neighbor_vote(idx, dist, labels)                     # the positive fraction among a row's neighbours

``exclude_same_group`` removes every bank row whose group equals the query row's; ``one_per_group`` keeps of each group
only its nearest row (by the ranking of the candidates: selection score, then index) and answers with the ``k`` nearest
groups, ordered by (dist, index) of these rows; it holds ``k <= 32``.  Both may be combined.  A non-finite bank row is
never a group's representative.  Both happen inside the selection kernel: the answer is exact however many alerts an
object has, and keeps every property above (``splits``, batch cuts, runs, incremental ``add``).

Everything within r.  The second question of an archive: not the k nearest, all rows within ``r``.

    indptr, indices, dist = index.radius(queries, r)             # a CSR: int64 [Q + 1], int64 [T], float32 [T]
    counts = index.count_within(queries, r)                      # int64 [Q] == indptr.diff(); 0 is novelty
    indptr, indices, dist = radius_neighbors(queries, bank, r)   # packs the bank for this one call
    indptr, indices, dist = radius_graph(emb, r, include_self=True)

Bank row b is in query row q's list if and only if b is eligible (finite, not the position ``self_offset`` masks, not of
q's group under ``exclude_same_group``) and the direct-form fp32 distance -- the device function ``query`` applies to the
rows it returns -- is ``<= r``, compared in fp32.  Hence ``dist`` is bit-identical to ``query``'s for the same pair; the
rows of ``query(q, k)`` with ``dist <= r`` are the head of the list sorted by (dist, index); identical rows are at exactly
0 and ``r = 0`` returns the duplicates; a non-finite query row has an empty list; and a row's list does not depend, bit
for bit, on the other rows of the call, on ``splits``, on the run or on how the index was built.  ``r`` is a float
(rounded to fp32 once) or a float tensor [Q] of per-row radii; negative or NaN is a ``ValueError``, ``+inf`` returns every
finite eligible row; for the cosine metric it is in ``1 - cos``.  Two tile passes count and write the candidates -- pairs
whose GEMM-form value is within ``r^2`` plus a margin that covers the error of both forms --, a third kernel computes
their direct-form distances, torch compacts and orders; nothing of size Q x N is written, the host is read twice (to
size the candidates, then the lists).  The margin grows with ``|q|^2 + |b|^2``: centre the rows (``rows - rows.mean(0)``),
or data far from the origin relative to its spread verifies most pairs -- exactly, and slowly.

Where a row stands.  The third question: not which rows are near, but how near a GIVEN row is.

    rank, dist = index.rank_of(queries, targets)                 # int64 [Q, t], float32 [Q, t] for targets int64 [Q, t]
    rank, dist = neighbor_ranks(queries, bank, targets)          # packs the bank for this one call

``rank[q, c]`` is the number of eligible bank rows b with (direct-form distance, b) before (``dist[q, c]``,
``targets[q, c]``): 0-based, without a cap, the position of the target in ``radius(q, dist[:, c], sort="distance")``
with the same switches, bit for bit.  The tile walk counts the pairs that are surely before -- below the target's
distance by more than the margin of both forms -- and hands the pairs inside the margin to the direct form; two host
reads (the number of these band pairs, the fill's error flag).  ``quality.trustworthiness`` is built on it.

On a 2-D map.  ``radius_graph`` and ``knn_graph`` take ``method="grid"`` for 2-D rows and the
euclidean metric: ``mapindex.MapIndex`` answers from a uniform grid in time linear in the rows plus the output, with the
same membership, ordering and distances (the radius lists are bit-identical).  The default, ``"tiles"``, is the path
described above.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream

METRICS = tuple(_lib.KNN_METRIC)


def _rows(t, name: str, device=None) -> torch.Tensor:
    """A [rows, D] float tensor on the GPU as contiguous fp32."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"btsbot_amd.neighbors runs on the GPU; there is no CPU fallback ({name} is on {t.device})")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, the bank on {device}")
    if t.dim() != 2 or not t.is_floating_point():
        raise ValueError(f"{name} must be a floating-point [rows, D] tensor, got {t.dtype} {tuple(t.shape)}")
    if not 1 <= t.shape[1] <= _lib.KNN_MAX_DIM:
        raise ValueError(f"{name}: D must be in 1..{_lib.KNN_MAX_DIM}, got {t.shape[1]}")
    if t.shape[0] >= 1 << 31:
        raise ValueError(f"{name}: at most 2^31 - 1 rows, got {t.shape[0]}")
    return t.detach().to(torch.float32).contiguous()


def _n_rows_or_none(x) -> Optional[int]:
    return int(x.shape[0]) if isinstance(x, torch.Tensor) and x.dim() == 2 else None


def _same_dim(queries, bank) -> Tuple[torch.Tensor, torch.Tensor]:
    q = _rows(queries, "queries")
    b = _rows(bank, "bank", q.device)
    if q.shape[1] != b.shape[1]:
        raise ValueError(f"queries have D = {q.shape[1]}, the bank D = {b.shape[1]}")
    return q, b


def _check_splits(splits) -> None:
    if not isinstance(splits, int) or isinstance(splits, bool) or not 0 <= splits <= _lib.KNN_MAX_SPLITS:
        raise ValueError(f"splits must be an int in 0..{_lib.KNN_MAX_SPLITS} (0: the library's choice), got {splits!r}")


def _check_cap(name: str, v) -> None:
    if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0):
        raise ValueError(f"{name} must be None or an int >= 0, got {v!r}")


def _check_k(k, splits) -> None:
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= _lib.KNN_MAX_K:
        raise ValueError(f"k must be an int in 1..{_lib.KNN_MAX_K}, got {k!r}")
    _check_splits(splits)


def _scan_counts(counts: torch.Tensor) -> torch.Tensor:
    """int64 [counts.numel() + 1]: where each (query, split)'s region starts, and the total at the end."""
    offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    offsets[1:] = torch.cumsum(counts.view(-1), 0, dtype=torch.int64)
    return offsets


def _metric(metric) -> int:
    if metric not in _lib.KNN_METRIC:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    return _lib.KNN_METRIC[metric]


def _groups(g, name: str, rows: int, device) -> torch.Tensor:
    """One int64 group per row, [rows] on ``device``, contiguous.  ValueError otherwise: nothing is converted, a group
    is an identity and a silent cast could merge two."""
    if not isinstance(g, torch.Tensor) or g.dtype != torch.int64:
        raise ValueError(f"{name} must be an int64 torch.Tensor, got "
                         f"{g.dtype if isinstance(g, torch.Tensor) else type(g).__name__}")
    if g.device != device:
        raise ValueError(f"{name} is on {g.device}, its rows on {device}")
    if g.dim() != 1 or g.shape[0] != rows:
        raise ValueError(f"{name} must hold one group per row, [{rows}], got {tuple(g.shape)}")
    return g.detach().contiguous()


def _check_group_args(k: int, has_groups: bool, query_groups, exclude_same_group, one_per_group) -> int:
    """The flags of btsbot_knn_query_grouped; ValueError for a combination that cannot be answered."""
    if not isinstance(exclude_same_group, bool) or not isinstance(one_per_group, bool):
        raise ValueError("exclude_same_group and one_per_group must be bools")
    if (exclude_same_group or one_per_group) and not has_groups:
        raise ValueError("exclude_same_group / one_per_group need an index built with groups=...")
    if exclude_same_group and query_groups is None:
        raise ValueError("exclude_same_group needs query_groups (one int64 group per query row)")
    if one_per_group and k > _lib.KNN_MAX_K_ONE_PER_GROUP:
        raise ValueError(f"one_per_group holds k <= {_lib.KNN_MAX_K_ONE_PER_GROUP}, got k = {k}")
    return (_lib.KNN_EXCLUDE_SAME if exclude_same_group else 0) | (_lib.KNN_ONE_PER_GROUP if one_per_group else 0)


class EmbeddingIndex:
    """A bank of embedding rows on one GPU with its packed operand image (norms, per-row scales, f16 head and remainder
    planes), built once and extended by ``add``.  A row's image depends on the row alone, so an index built by several
    ``add`` calls answers bit for bit like one built at once.

    Rows leave by ``remove`` (a stable compaction: the survivors keep their order and move as bytes -- the fp32 rows, the
    packed records, the groups, the ids).  After any mix of ``add`` and ``remove`` the index answers ``query``, ``radius``,
    ``count_within`` and ``rank_of`` bit for bit like ``EmbeddingIndex(index.bank.clone(), metric, groups=index.groups)``
    built at once.  ``ids`` int64 [len], ascending, is every row's permanent number -- the rows ever added before it,
    never reused --, ``locate(ids)`` the current row of an id, and ``generation`` the number of ``remove`` calls that
    removed at least one row: what a ``KnnGraph`` or a fit compares to see that rows have left.

    groups: one int64 group per bank row (an alert's object), or None.  An index with groups takes them with every
    ``add`` and can answer ``query(..., exclude_same_group=True)`` and ``query(..., one_per_group=True)``.

    Calls on one index must be ordered by the caller's streams."""

    def __init__(self, bank: torch.Tensor, metric: str = "euclidean", *, groups: Optional[torch.Tensor] = None):
        self._metric_id = _metric(metric)
        self.metric = metric
        rows = _rows(bank, "bank")
        self.device = rows.device
        self.dim = int(rows.shape[1])
        self._n = 0
        self._cap = 0
        self._bank = rows.new_empty((0, self.dim))
        self._packed = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._groups = None if groups is None else torch.empty(0, dtype=torch.int64, device=self.device)
        self._ids = torch.empty(0, dtype=torch.int64, device=self.device)
        self._next_id = 0
        self.generation = 0
        self.add(rows, groups=groups)

    def __len__(self) -> int:
        return self._n

    @property
    def bank(self) -> torch.Tensor:
        """The fp32 rows held, [len, D] (a view of the index's storage)."""
        return self._bank[:self._n]

    @property
    def groups(self) -> Optional[torch.Tensor]:
        """The rows' groups, int64 [len] (a view of the index's storage), or None for an index without groups."""
        return None if self._groups is None else self._groups[:self._n]

    @property
    def ids(self) -> torch.Tensor:
        """The rows' permanent numbers, int64 [len], ascending (a view of the index's storage): a row's id is the
        number of rows ever added before it, and is never reused."""
        return self._ids[:self._n]

    def _record_bytes(self) -> int:
        return int(_lib.lib().btsbot_knn_bank_bytes(1, self.dim))

    def add(self, rows: torch.Tensor, *, groups: Optional[torch.Tensor] = None) -> "EmbeddingIndex":
        """Appends ``rows`` [n, D]; only they are packed (what is held already moves as bytes when the storage grows).
        groups: int64 [n], required if and only if the index was built with groups."""
        rows = _rows(rows, "rows", self.device)
        if rows.shape[1] != self.dim:
            raise ValueError(f"rows: D = {rows.shape[1]}, the index holds D = {self.dim}")
        n = int(rows.shape[0])
        if self._n + n >= 1 << 31:
            raise ValueError(f"an index holds at most 2^31 - 1 rows ({self._n} + {n})")
        if (groups is None) != (self._groups is None):
            raise ValueError("add(rows, groups=...) takes groups if and only if the index was built with groups")
        if groups is not None:
            groups = _groups(groups, "groups", n, self.device)
        if n == 0:
            return self
        L = _lib.lib()
        rec = self._record_bytes()
        with torch.cuda.device(self.device):
            if self._n + n > self._cap:
                cap = max(self._n + n, 2 * self._cap) if self._cap else n
                bank = torch.empty((cap, self.dim), dtype=torch.float32, device=self.device)
                packed = torch.empty(cap * rec, dtype=torch.uint8, device=self.device)
                bank[:self._n].copy_(self._bank[:self._n])
                packed[:self._n * rec].copy_(self._packed[:self._n * rec])
                if self._groups is not None:
                    grp = torch.empty(cap, dtype=torch.int64, device=self.device)
                    grp[:self._n].copy_(self._groups[:self._n])
                    self._groups = grp
                ids = torch.empty(cap, dtype=torch.int64, device=self.device)
                ids[:self._n].copy_(self._ids[:self._n])
                self._ids = ids
                self._bank, self._packed, self._cap = bank, packed, cap
            new = self._bank[self._n:self._n + n]
            new.copy_(rows)
            if groups is not None:
                self._groups[self._n:self._n + n].copy_(groups)
            torch.arange(self._next_id, self._next_id + n, out=self._ids[self._n:self._n + n])
            _lib.check(L.btsbot_knn_pack_bank(_ptr(new), self._n, n, self.dim, self._metric_id, _ptr(self._packed),
                                              self._cap, _stream(self.device)), "btsbot_knn_pack_bank")
        self._n += n
        self._next_id += n
        return self

    def remove(self, which: torch.Tensor) -> torch.Tensor:
        """Removes rows and returns ``kept`` int64 [len after], ascending: the OLD row number of every surviving row, so
        that ``side = side[kept]`` keeps any per-row array of the caller aligned.  which: bool [len] (True: remove) or
        int64 [m] row numbers (any order, repeats allowed).  A stable compaction out of place into fresh storage, which
        is then swapped in: the survivors keep their order, their ids and their bytes (rows, packed records, groups).
        Removing nothing returns ``arange(len)`` and leaves ``generation`` as it is.  One host read: the survivor count
        and the range check of int64 rows.  A wrong dtype, device or mask length and a row out of range are a
        ``ValueError``, and the index stays as it was."""
        n, dev = self._n, self.device
        if not isinstance(which, torch.Tensor) or which.dtype not in (torch.bool, torch.int64):
            raise ValueError("which must be a bool [len] mask (True: remove) or int64 row numbers, got "
                             f"{which.dtype if isinstance(which, torch.Tensor) else type(which).__name__}")
        if which.device != dev:
            raise ValueError(f"which is on {which.device}, the index on {dev}")
        if which.dim() != 1 or (which.dtype == torch.bool and which.shape[0] != n):
            raise ValueError(f"which must be a bool mask [{n}] or int64 [m], got {which.dtype} {tuple(which.shape)}")
        if dev.type != "cuda":
            raise RuntimeError(f"btsbot_amd.neighbors runs on the GPU; there is no CPU fallback (which is on {dev})")
        with torch.cuda.device(dev):
            if which.dtype == torch.bool:
                keep = ~which
                bad = torch.zeros((), dtype=torch.int64, device=dev)
            else:
                bad = ((which < 0) | (which >= n)).any().to(torch.int64)
                keep = torch.ones(n + 1, dtype=torch.bool, device=dev)        # (slot n takes the rows out of range)
                keep[torch.where((which < 0) | (which >= n), torch.full_like(which, n), which)] = False
                keep = keep[:n]
            at = torch.cumsum(keep, 0, dtype=torch.int64)
            s, bad = torch.stack([at[-1] if n else bad.new_zeros(()), bad]).tolist()      # the one host read
            if bad:
                raise ValueError(f"which names a row outside 0..{n - 1}")
            rows = torch.arange(n, device=dev)
            if s == n:
                return rows
            # the survivors' old numbers without a second read: row a goes to slot at[a] - 1, a removed one to slot s
            kept = torch.empty(s + 1, dtype=torch.int64, device=dev)
            kept.scatter_(0, torch.where(keep, at - 1, torch.full_like(at, s)), rows)
            kept = kept[:s].contiguous()
            rec = self._record_bytes()
            bank = self._bank[:n].index_select(0, kept)
            packed = self._packed[:n * rec].view(n, rec).index_select(0, kept).view(-1)
            ids = self._ids[:n].index_select(0, kept)
            if self._groups is not None:
                self._groups = self._groups[:n].index_select(0, kept)
            self._bank, self._packed, self._ids, self._cap, self._n = bank, packed, ids, s, s
        self.generation += 1
        return kept

    def locate(self, ids: torch.Tensor) -> torch.Tensor:
        """int64, the shape of ``ids``: the current row of each permanent id, -1 where it is gone (or was never given).
        ``torch.searchsorted`` on ``index.ids``; nothing is read from the host."""
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64:
            raise ValueError("ids must be an int64 torch.Tensor, got "
                             f"{ids.dtype if isinstance(ids, torch.Tensor) else type(ids).__name__}")
        if ids.device != self.device:
            raise ValueError(f"ids is on {ids.device}, the index on {self.device}")
        if self.device.type != "cuda":
            raise RuntimeError(f"btsbot_amd.neighbors runs on the GPU; there is no CPU fallback (ids is on {ids.device})")
        if self._n == 0:
            return torch.full_like(ids, -1)
        own = self.ids
        pos = torch.searchsorted(own, ids.contiguous()).clamp(max=self._n - 1)
        return torch.where(own[pos] == ids, pos, torch.full_like(pos, -1))

    def _prelude(self, queries, k, splits, query_groups, exclude_same_group, one_per_group, self_offset, targets=None):
        """The common arguments of ``query``, ``radius`` and ``rank_of``, checked in their order: ``(flags, q, nq,
        query_groups, splits)``, with ``splits == 0`` resolved to the library's choice."""
        flags = _check_group_args(k, self._groups is not None, query_groups, exclude_same_group, one_per_group)
        q = _rows(queries, "queries", self.device)
        if q.shape[1] != self.dim:
            raise ValueError(f"queries: D = {q.shape[1]}, the index holds D = {self.dim}")
        if not isinstance(self_offset, int):
            raise ValueError(f"self_offset must be an int, got {self_offset!r}")
        if targets is not None and targets.device != self.device:
            raise ValueError(f"targets is on {targets.device}, the index on {self.device}")
        nq = int(q.shape[0])
        if query_groups is not None:
            query_groups = _groups(query_groups, "query_groups", nq, self.device)
        if splits == 0:
            splits = max(1, int(_lib.lib().btsbot_knn_splits(max(nq, 1), self._n, self.dim, 1)))
        return flags, q, nq, query_groups, splits

    def query(self, queries: torch.Tensor, k: int, *, query_groups: Optional[torch.Tensor] = None,
              exclude_same_group: bool = False, one_per_group: bool = False, splits: int = 0,
              self_offset: int = -1, self_rows: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``idx`` int64 [Q, k] and ``dist`` float32 [Q, k] of each query row's ``k`` nearest rows of the index.
        splits: bank slices searched by separate workgroups (0: the library's choice; the answer does not depend on it).
        self_offset >= 0: query row i is row i + self_offset of the index and is not its own candidate.
        self_rows: int64 [Q], query row i is row ``self_rows[i]`` of the index -- scattered rows, where ``self_offset``
        masks a run -- and is not its own candidate: on an index without groups the search runs with the row numbers as
        the groups of both sides (all 64 bits decide, so exactly the row itself is excluded); on an index with groups it
        needs ``exclude_same_group=True``, under which the row's own group covers the row.  Not beside ``self_offset``.
        query_groups: int64 [Q], the query rows' groups.  exclude_same_group: no row of the query row's own group.
        one_per_group: at most one row per group, its nearest; the ``k`` nearest groups (``k <= 32``)."""
        _check_k(k, splits)
        _check_self_rows(self_rows, _n_rows_or_none(queries), self_offset, self._groups is not None, exclude_same_group,
                         self.device)
        flags, q, nq, query_groups, splits = self._prelude(queries, k, splits, query_groups, exclude_same_group,
                                                           one_per_group, self_offset)
        bank_groups = self._groups
        if self_rows is not None and self._groups is None:
            flags, query_groups = _lib.KNN_EXCLUDE_SAME, self_rows.detach().contiguous()
            bank_groups = torch.arange(self._n, device=self.device)
        idx = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        dist = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        if nq == 0:
            return idx, dist
        L = _lib.lib()
        need = int(L.btsbot_knn_workspace_grouped(nq, self._n, self.dim, k, splits, flags))
        if need < 0:
            _lib.check(need, "btsbot_knn_workspace_grouped")
        with torch.cuda.device(self.device):
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            args = (_ptr(q), nq, _ptr(self._bank), _ptr(self._packed), self._n, self.dim, k, self._metric_id,
                    self_offset, splits, _ptr(idx), _ptr(dist), _ptr(ws), need, _stream(self.device))
            if flags == 0:
                _lib.check(L.btsbot_knn_query(*args), "btsbot_knn_query")
            else:
                _lib.check(L.btsbot_knn_query_grouped(*args, _ptr(query_groups), _ptr(bank_groups), flags),
                           "btsbot_knn_query_grouped")
        return idx, dist

    def radius(self, queries: torch.Tensor, r, *, query_groups: Optional[torch.Tensor] = None,
               exclude_same_group: bool = False, self_offset: int = -1, sort: str = "index", splits: int = 0,
               max_total: Optional[int] = None,
               stats: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Every row of the index within ``r`` of each query row, as a CSR: ``indptr`` int64 [Q + 1], ``indices`` int64
        [T], ``dist`` float32 [T] (see the module text).  r: a float, or a float tensor [Q] of per-row radii.
        sort: ``"index"`` orders a row's list by bank index, ``"distance"`` by (dist, index).  max_total: ValueError
        (naming the total) instead of lists longer than this in all.  stats: a dict that receives ``candidates`` (the
        pairs whose distance was computed in the direct form), ``total`` and ``error_flag`` (the fill kernel's bounds
        check; 0, or the call raises).  The other arguments are ``query``'s.  Two host reads: the number of
        candidates, then the total, each to allocate."""
        _check_radius_args(r, _n_rows_or_none(queries), sort, splits, max_total)
        flags, q, nq, query_groups, splits = self._prelude(queries, 1, splits, query_groups, exclude_same_group, False,
                                                           self_offset)
        n, dev, L = self._n, self.device, _lib.lib()
        with torch.cuda.device(dev):
            if isinstance(r, torch.Tensor):
                if r.device != dev:
                    raise ValueError(f"r is on {r.device}, the index on {dev}")
                rad = r.detach().to(torch.float32).contiguous()
                bad = (~(rad >= 0)).any().to(torch.int64)
            else:
                rad = torch.full((nq,), float(r), dtype=torch.float32, device=dev)   # rounded to fp32 once
                bad = torch.zeros((), dtype=torch.int64, device=dev)
            counts = torch.zeros((nq, splits), dtype=torch.int32, device=dev)
            need = int(L.btsbot_knn_radius_workspace(nq, self.dim))
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            head = (_ptr(q), nq)
            tail = (_ptr(self._packed), n, self.dim, self._metric_id, _ptr(rad), self_offset, splits,
                    _ptr(query_groups) if flags else None, _ptr(self._groups) if flags else None, flags)
            if nq and n:
                _lib.check(L.btsbot_knn_radius_count(*head, *tail, _ptr(counts), _ptr(ws), need, _stream(self.device)),
                           "btsbot_knn_radius_count")
            offsets = _scan_counts(counts)
            n_cand, bad = torch.stack([offsets[-1], bad]).tolist()          # the host read that sizes the candidates
            if bad:
                raise ValueError("r must be >= 0 in every row (and not NaN)")
            cand = torch.zeros(n_cand, dtype=torch.int32, device=dev)
            cdist = torch.empty(n_cand, dtype=torch.float32, device=dev)
            keep = torch.zeros(n_cand, dtype=torch.uint8, device=dev)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            if n_cand:
                _lib.check(L.btsbot_knn_radius_fill(*head, _ptr(self._bank), *tail, _ptr(counts), _ptr(offsets), n_cand,
                                                    _ptr(cand), _ptr(cdist), _ptr(keep), _ptr(err), _ptr(ws), need,
                                                    _stream(self.device)), "btsbot_knn_radius_fill")
            row_off = offsets[::splits]                                       # [Q + 1]: a row's candidates are contiguous
            kept = torch.cat([offsets.new_zeros(1), torch.cumsum(keep, 0, dtype=torch.int64)])
            indptr = kept[row_off]
            total, flag = torch.stack([indptr[-1], err[0].to(torch.int64)]).tolist()   # the read that sizes the lists
            if stats is not None:
                stats.update(candidates=int(n_cand), total=int(total), error_flag=int(flag))
            if flag:
                raise RuntimeError("btsbot_knn_radius_fill: a candidate fell past the end of its region (the count and "
                                   "the fill pass disagree); the lists are not returned")
            if max_total is not None and total > max_total:
                raise ValueError(f"the lists hold T = {total} entries, more than max_total = {max_total}")
            rows = torch.repeat_interleave(torch.arange(nq, device=dev), row_off.diff(), output_size=n_cand)
            order = _csr_order(rows, cand.to(torch.int64), cdist, max(n, 1), sort, keep=keep, total=total)
            return indptr, cand[order].to(torch.int64), cdist[order]

    def rank_of(self, queries: torch.Tensor, targets: torch.Tensor, *, query_groups: Optional[torch.Tensor] = None,
                exclude_same_group: bool = False, one_per_group: bool = False, self_offset: int = -1, splits: int = 0,
                max_band: Optional[int] = None, stats: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Where given rows of the index stand in each query row's neighbour ordering: ``rank``
        int64 [Q, t] and ``dist`` float32 [Q, t] for ``targets`` int64 [Q, t], bank row numbers, 1 <= t <= 64.
        ``dist[q, c]`` is the direct-form distance to row ``targets[q, c]``, the bits ``query`` and ``radius`` return
        for that pair; ``rank[q, c]`` is the number of eligible rows b with (distance, b) before (``dist[q, c]``,
        ``targets[q, c]``): 0-based, the position of the target in ``radius(q, dist[:, c], sort="distance")`` with the
        same switches, bit for bit.  ``rank = -1`` where the target is < 0 or >= len(index), is not eligible for the
        row (non-finite, the masked self, the row's own group under ``exclude_same_group``) or the query row is
        non-finite; ``dist`` is NaN where the target is out of range or either row is non-finite.  There is no cap on
        the rank.  max_band: ValueError (naming the total) instead of more than this many band pairs, the pairs whose
        order against a target only the direct form can decide.  stats: receives ``band`` and ``error_flag``.  The
        other arguments are ``radius``'s; ``one_per_group`` is not a rank mode.  Two host reads: the number of band
        pairs, to allocate them, and the fill's error flag."""
        _check_rank_args(targets, _n_rows_or_none(queries), splits, max_band, one_per_group)
        flags, q, nq, query_groups, splits = self._prelude(queries, 1, splits, query_groups, exclude_same_group, False,
                                                           self_offset, targets=targets)
        n, dev, t, L = self._n, self.device, int(targets.shape[1]), _lib.lib()
        tg = targets.detach().contiguous()
        with torch.cuda.device(dev):
            dist = torch.full((nq, t), float("nan"), dtype=torch.float32, device=dev)
            rank = torch.full((nq, t), -1, dtype=torch.int32, device=dev)
            if stats is not None:
                stats.update(band=0, error_flag=0)
            if nq == 0:
                return rank.to(torch.int64), dist
            counts = torch.zeros((nq, splits), dtype=torch.int32, device=dev)
            need = int(L.btsbot_knn_rank_workspace(nq, self.dim, t))
            if need < 0:
                _lib.check(need, "btsbot_knn_rank_workspace")
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            head = (_ptr(q), nq, _ptr(self._bank), _ptr(self._packed), n, self.dim, self._metric_id, _ptr(tg), t,
                    self_offset, splits, _ptr(query_groups) if flags else None, _ptr(self._groups) if flags else None,
                    flags)
            _lib.check(L.btsbot_knn_rank_count(*head, _ptr(dist), _ptr(rank), _ptr(counts), _ptr(ws), need,
                                               _stream(self.device)), "btsbot_knn_rank_count")
            offsets = _scan_counts(counts)
            n_band = int(offsets[-1])                                       # the host read that sizes the band pairs
            if max_band is not None and n_band > max_band:
                raise ValueError(f"the band holds {n_band} pairs, more than max_band = {max_band}")
            flag = 0
            if n_band:
                cand = torch.full((n_band,), -1, dtype=torch.int32, device=dev)
                cmask = torch.zeros(n_band, dtype=torch.int64, device=dev)
                err = torch.zeros(1, dtype=torch.int32, device=dev)
                _lib.check(L.btsbot_knn_rank_fill(*head, _ptr(dist), _ptr(rank), _ptr(counts), _ptr(offsets), n_band,
                                                  _ptr(cand), _ptr(cmask), _ptr(err), _ptr(ws), need, _stream(self.device)),
                           "btsbot_knn_rank_fill")
                flag = int(err[0])                                          # the second read: the fill's bounds check
            if stats is not None:
                stats.update(band=n_band, error_flag=flag)
            if flag:
                raise RuntimeError("btsbot_knn_rank_fill: a band pair fell past the end of its region (the count and "
                                   "the fill pass disagree); the ranks are not returned")
            return rank.to(torch.int64), dist

    def count_within(self, queries: torch.Tensor, r, **kw) -> torch.Tensor:
        """int64 [Q]: how many rows of the index lie within ``r`` of each query row -- exact, the ``indptr.diff()`` of
        ``radius`` with the same arguments (it goes through the lists; 0 is novelty, thousands a crowded region)."""
        return self.radius(queries, r, **kw)[0].diff()


def _check_self_rows(self_rows, n_query, self_offset, has_groups: bool, exclude_same_group, device) -> None:
    """ValueError for a ``self_rows`` that ``query`` cannot honour, before anything touches the device."""
    if self_rows is None:
        return
    if not isinstance(self_rows, torch.Tensor) or self_rows.dtype != torch.int64:
        raise ValueError("self_rows must be an int64 torch.Tensor [Q] of bank row numbers, got "
                         f"{self_rows.dtype if isinstance(self_rows, torch.Tensor) else type(self_rows).__name__}")
    if self_rows.dim() != 1 or (n_query is not None and self_rows.shape[0] != n_query):
        raise ValueError(f"self_rows must hold one bank row per query row, [{n_query}], got {tuple(self_rows.shape)}")
    if isinstance(self_offset, int) and self_offset >= 0:
        raise ValueError("self_rows and self_offset >= 0 both say which bank row a query row is: give one")
    if has_groups and exclude_same_group is not True:
        raise ValueError("self_rows on an index with groups needs exclude_same_group=True (the row's own group then "
                         "covers the row; the group switches have no way to mask one row and keep its group)")
    if self_rows.device != device:
        raise ValueError(f"self_rows is on {self_rows.device}, the index on {device}")


def _stale_fit(index, n_fit: int, generation: int) -> Optional[str]:
    """None, or why a fit of ``n_fit`` rows made at ``generation`` no longer describes ``index`` (the head of the
    RuntimeError of ``NoveltyModel.score`` and ``ClusterModel.predict``)."""
    if len(index) != n_fit:
        return f"the index holds {len(index)} rows, the fit {n_fit}: a fit does not follow index.add"
    now = getattr(index, "generation", 0)
    if now != generation:
        return (f"rows were removed from the index since the fit (generation {generation} -> {now}): a fit does not "
                "follow index.remove")
    return None


SORTS = ("index", "distance")


def _check_radius_args(r, n_query, sort, splits, max_total) -> None:
    """ValueError for what ``radius`` cannot answer, before anything touches the device."""
    if isinstance(r, torch.Tensor):
        if not r.is_floating_point() or r.dim() != 1 or (n_query is not None and r.shape[0] != n_query):
            raise ValueError(f"r as a tensor holds one float radius per query row, [{n_query}], got {r.dtype} "
                             f"{tuple(r.shape)}")
        if r.device.type == "cpu" and not bool((r >= 0).all()):
            raise ValueError("r must be >= 0 in every row (and not NaN)")
    elif isinstance(r, bool) or not isinstance(r, (int, float)) or not r >= 0:
        raise ValueError(f"r must be a float >= 0 (and not NaN) or a tensor of them, got {r!r}")
    if sort not in SORTS:
        raise ValueError(f"sort must be one of {SORTS}, got {sort!r}")
    _check_splits(splits)
    _check_cap("max_total", max_total)


def _check_rank_args(targets, n_query, splits, max_band, one_per_group=False) -> None:
    """ValueError for what ``rank_of`` cannot answer, before anything touches the device."""
    if one_per_group:
        raise ValueError("one_per_group is not a rank mode (a rank counts rows, not groups)")
    if not isinstance(targets, torch.Tensor) or targets.dtype != torch.int64:
        raise ValueError(f"targets must be an int64 torch.Tensor [Q, t] of bank row numbers, got "
                         f"{targets.dtype if isinstance(targets, torch.Tensor) else type(targets).__name__}")
    if targets.dim() != 2 or not 1 <= targets.shape[1] <= _lib.KNN_MAX_K or \
            (n_query is not None and targets.shape[0] != n_query):
        raise ValueError(f"targets must be [Q = {n_query}, t] with 1 <= t <= {_lib.KNN_MAX_K}, got {tuple(targets.shape)}")
    _check_splits(splits)
    _check_cap("max_band", max_band)


def neighbor_ranks(queries: torch.Tensor, bank: torch.Tensor, targets: torch.Tensor, metric: str = "euclidean", *,
                   bank_groups: Optional[torch.Tensor] = None, query_groups: Optional[torch.Tensor] = None,
                   exclude_same_group: bool = False, self_offset: int = -1, splits: int = 0,
                   max_band: Optional[int] = None, stats: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``rank`` int64 [Q, t] and ``dist`` float32 [Q, t] of the rows ``targets`` [Q, t] of ``bank`` [N, D] in the
    neighbour ordering of each row of ``queries`` [Q, D], as ``EmbeddingIndex.rank_of`` returns them.  Packs the bank for
    this one call."""
    _metric(metric)
    _check_rank_args(targets, _n_rows_or_none(queries), splits, max_band)
    _check_group_args(1, bank_groups is not None, query_groups, exclude_same_group, False)
    q, b = _same_dim(queries, bank)
    return EmbeddingIndex(b, metric, groups=bank_groups).rank_of(
        q, targets, query_groups=query_groups, exclude_same_group=exclude_same_group, self_offset=self_offset,
        splits=splits, max_band=max_band, stats=stats)


def _float_order(dist: torch.Tensor) -> torch.Tensor:
    """int64 in [0, 2^32) that orders like the fp32 values (negative ones included: 1 - cos may round below 0)"""
    b = dist.view(torch.int32).to(torch.int64)
    ub = b & 0xFFFFFFFF
    return torch.where(b < 0, 0xFFFFFFFF - ub, ub + 0x80000000)


def _csr_order(rows, idx, dist, n_bank: int, sort: str, keep=None, total=None) -> torch.Tensor:
    """The permutation that drops the entries ``keep`` rejects (``total`` stay) and orders the rest by row, then by
    ``sort``: one sort by (row, index) does both, a second, stable one by (row, dist) gives the distance order."""
    key = rows * n_bank + idx
    if keep is not None:
        key = torch.where(keep != 0, key, torch.full_like(key, torch.iinfo(torch.int64).max))
    order = torch.sort(key).indices
    if total is not None:
        order = order[:total]
    if sort == "distance":
        order = order[torch.sort((rows[order] << 32) | _float_order(dist[order]), stable=True).indices]
    return order


def radius_neighbors(queries: torch.Tensor, bank: torch.Tensor, r, metric: str = "euclidean", *,
                     bank_groups: Optional[torch.Tensor] = None, query_groups: Optional[torch.Tensor] = None,
                     exclude_same_group: bool = False, sort: str = "index", splits: int = 0,
                     max_total: Optional[int] = None,
                     stats: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Every row of ``bank`` [N, D] within ``r`` of each row of ``queries`` [Q, D], as the CSR ``EmbeddingIndex.radius``
    returns.  Packs the bank for this one call."""
    _metric(metric)
    _check_radius_args(r, _n_rows_or_none(queries), sort, splits, max_total)
    _check_group_args(1, bank_groups is not None, query_groups, exclude_same_group, False)
    q, b = _same_dim(queries, bank)
    return EmbeddingIndex(b, metric, groups=bank_groups).radius(
        q, r, query_groups=query_groups, exclude_same_group=exclude_same_group, sort=sort, splits=splits,
        max_total=max_total, stats=stats)


def radius_graph(emb: torch.Tensor, r, include_self: bool = True, metric: str = "euclidean", *,
                 groups: Optional[torch.Tensor] = None, group_mode: str = "exclude", sort: str = "index",
                 splits: int = 0, max_total: Optional[int] = None, stats: Optional[dict] = None,
                 method: str = "tiles") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Every row of ``emb`` [N, D] among the others within ``r``: the CSR of ``EmbeddingIndex.radius`` with N rows.
    include_self=True: a finite row is in its own list at distance 0 (DBSCAN counts it); False: it is not, by
    position -- its duplicates are.  groups / group_mode="exclude": the others are rows of OTHER groups only (the row
    itself stays under include_self=True).  A non-finite row has an empty list.
    method: ``"tiles"`` (``EmbeddingIndex``) or, for a 2-D ``emb`` and the euclidean metric, ``"grid"`` (``MapIndex``:
    the same lists bit for bit, in time linear in N plus the edges; ``splits`` has no part in it, ``stats`` receives
    ``visited`` in place of ``candidates``)."""
    _metric(metric)
    _check_method(method)
    if group_mode != "exclude":
        raise ValueError(f'radius lists know group_mode="exclude" only, got {group_mode!r}')
    _check_radius_args(r, _n_rows_or_none(emb), sort, splits, max_total)
    if method == "grid":
        from .mapindex import check_grid_method
        check_grid_method(int(emb.shape[1]) if isinstance(emb, torch.Tensor) and emb.dim() == 2 else None, metric)
    rows = _rows(emb, "emb")
    n = int(rows.shape[0])
    kw = dict(sort=sort, splits=splits, max_total=max_total, stats=stats)
    if groups is not None:
        groups = _groups(groups, "groups", n, rows.device)
        kw.update(query_groups=groups, exclude_same_group=True)
    if method == "grid":
        from .mapindex import MapIndex
        del kw["splits"]
        index = MapIndex(rows, groups=groups)
    else:
        index = EmbeddingIndex(rows, metric, groups=groups)
    if include_self and groups is None and metric == "euclidean":
        return index.radius(rows, r, **kw)         # the row itself is a bank row at exactly 0
    indptr, indices, dist = index.radius(rows, r, self_offset=0, **kw)
    if not include_self:
        return indptr, indices, dist
    # the row itself, by position, at distance 0
    finite = torch.isfinite(rows).all(dim=1) & torch.isfinite((rows * rows).sum(dim=1))
    own = finite.nonzero().view(-1)
    at = torch.repeat_interleave(torch.arange(n, device=rows.device), indptr.diff(), output_size=int(indices.shape[0]))
    at, indices, dist = torch.cat([at, own]), torch.cat([indices, own]), torch.cat([dist, dist.new_zeros(own.shape[0])])
    order = _csr_order(at, indices, dist, max(n, 1), sort)
    indptr = indptr + torch.cat([indptr.new_zeros(1), torch.cumsum(finite, 0, dtype=torch.int64)])
    return indptr, indices[order], dist[order]


def embedding_neighbors(queries: torch.Tensor, bank: torch.Tensor, k: int, metric: str = "euclidean", *,
                        bank_groups: Optional[torch.Tensor] = None, query_groups: Optional[torch.Tensor] = None,
                        exclude_same_group: bool = False, one_per_group: bool = False,
                        splits: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The ``k`` nearest rows of ``bank`` [N, D] for every row of ``queries`` [Q, D]: ``idx`` int64 [Q, k], ``dist``
    float32 [Q, k] (see the module text).  Packs the bank for this one call; keep an ``EmbeddingIndex`` to query a bank
    more than once.  bank_groups / query_groups / exclude_same_group / one_per_group: as ``EmbeddingIndex(groups=...)``
    and its ``query``."""
    _check_k(k, splits)
    _metric(metric)
    _check_group_args(k, bank_groups is not None, query_groups, exclude_same_group, one_per_group)
    q, b = _same_dim(queries, bank)
    return EmbeddingIndex(b, metric, groups=bank_groups).query(
        q, k, query_groups=query_groups, exclude_same_group=exclude_same_group, one_per_group=one_per_group, splits=splits)


GROUP_MODES = ("exclude", "distinct", "exclude+distinct")
METHODS = ("tiles", "grid")


def _check_method(method) -> None:
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")


def knn_graph(emb: torch.Tensor, k: int, include_self: bool = True, metric: str = "euclidean", *,
              groups: Optional[torch.Tensor] = None, group_mode: str = "exclude",
              splits: int = 0, method: str = "tiles") -> Tuple[torch.Tensor, torch.Tensor]:
    """Every row of ``emb`` [N, D] among the others: ``idx`` int64 [N, k], ``dist`` float32 [N, k].

    include_self=True: the row itself first at distance 0, then its ``k - 1`` nearest others -- the layout pynndescent
    and umap-learn's ``precomputed_knn`` use.  include_self=False: ``k`` others.  A row is excluded by position, not by
    value: its duplicates are legitimate neighbours at distance 0.

    groups: int64 [N], the rows' groups (objects); a row's own group is its query group.  group_mode: ``"exclude"`` the
    others are rows of OTHER groups only; ``"distinct"`` the others hold at most one row per group (the row's own group
    may be among them, by another of its rows); ``"exclude+distinct"`` both.  The row itself stays in column 0 under
    include_self=True in every mode.
    method: ``"tiles"`` (``EmbeddingIndex``) or, for a 2-D ``emb``, the euclidean metric and group_mode ``"exclude"``,
    ``"grid"`` (``MapIndex``: the k smallest by (dist, index) of the direct-form distance, in time linear in N)."""
    _check_k(k, splits)
    _metric(metric)
    _check_method(method)
    if group_mode not in GROUP_MODES:
        raise ValueError(f"group_mode must be one of {GROUP_MODES}, got {group_mode!r}")
    if method == "grid":
        from .mapindex import check_grid_method
        check_grid_method(int(emb.shape[1]) if isinstance(emb, torch.Tensor) and emb.dim() == 2 else None, metric,
                          group_mode=group_mode)
    rows = _rows(emb, "emb")
    if groups is None:
        kw = {}
    else:
        groups = _groups(groups, "groups", int(rows.shape[0]), rows.device)
        kw = dict(query_groups=groups, exclude_same_group="exclude" in group_mode, one_per_group="distinct" in group_mode)
        _check_group_args(k - 1 if include_self else k, True, groups, kw["exclude_same_group"], kw["one_per_group"])
    if method == "grid":
        from .mapindex import MapIndex
        index = MapIndex(rows, groups=groups)
        kw.pop("one_per_group", None)
        if not include_self:
            return index.query(rows, k, self_offset=0, **kw)
        return _self_first_graph(index, k, None, **kw)
    index = EmbeddingIndex(rows, metric, groups=groups)
    if not include_self:
        return index.query(rows, k, splits=splits, self_offset=0, **kw)
    return _self_first_graph(index, k, splits, **kw)


def _self_first_graph(index, k: int, splits: Optional[int] = 0, **kw) -> Tuple[torch.Tensor, torch.Tensor]:
    """``knn_graph(index.bank, k, include_self=True)`` from an index already packed (kw: the group arguments of
    ``query``).  splits=None: a ``MapIndex``, which has none."""
    if splits is None:
        rows = index.points
    else:
        rows = index.bank
        kw["splits"] = splits
    n = int(rows.shape[0])
    idx = torch.empty((n, k), dtype=torch.int64, device=rows.device)
    dist = torch.empty((n, k), dtype=torch.float32, device=rows.device)
    finite = torch.isfinite(rows).all(dim=1)
    idx[:, 0] = torch.where(finite, torch.arange(n, device=rows.device), torch.full_like(idx[:, 0], -1))
    dist[:, 0] = torch.where(finite, torch.zeros_like(dist[:, 0]), torch.full_like(dist[:, 0], float("nan")))
    if k > 1:
        idx[:, 1:], dist[:, 1:] = index.query(rows, k - 1, self_offset=0, **kw)
    return idx, dist


def neighbor_vote(idx: torch.Tensor, dist: torch.Tensor, labels: torch.Tensor, weights: str = "uniform") -> torch.Tensor:
    """The kNN score of every row, float32 [Q]: the positive fraction (``labels`` [N], non-zero = positive, indexed by
    ``idx``) among the row's valid neighbours (``idx >= 0``), or with ``weights="distance"`` the ``1 / dist``-weighted
    fraction, where a neighbour at distance 0 takes the whole vote (several: they share it).  NaN where a row has no valid
    neighbour.  With ``knn_graph(emb, k, include_self=False, groups=obj, group_mode="exclude")`` this is the
    leave-one-object-out kNN score of an embedding.  Torch operations on the tensors' device; nothing is synchronised."""
    if weights not in ("uniform", "distance"):
        raise ValueError(f'weights must be "uniform" or "distance", got {weights!r}')
    if idx.dim() != 2 or idx.shape != dist.shape or idx.dtype != torch.int64 or not dist.is_floating_point():
        raise ValueError(f"idx must be int64 [Q, k] and dist floating point of the same shape, got {idx.dtype} "
                         f"{tuple(idx.shape)} and {dist.dtype} {tuple(dist.shape)}")
    if labels.dim() != 1:
        raise ValueError(f"labels must be [N], got {tuple(labels.shape)}")
    valid = idx >= 0
    if labels.shape[0] == 0:
        pos = torch.zeros_like(valid)
    else:
        pos = (labels[idx.clamp(min=0)] != 0) & valid
    if weights == "uniform":
        w = valid.to(torch.float32)
    else:
        # 1 / dist up to a factor per row, the row's smallest distance: no weight overflows for a tiny distance
        d = torch.where(valid, dist.to(torch.float32), torch.full_like(dist, float("inf"), dtype=torch.float32))
        dmin = d.min(dim=1, keepdim=True).values if d.shape[1] else d.new_zeros((d.shape[0], 1))
        zero = valid & (d == 0)
        w = torch.where(dmin == 0, zero.to(torch.float32), torch.where(valid, dmin / d, torch.zeros_like(d)))
    den = w.sum(dim=1)
    num = (w * pos.to(torch.float32)).sum(dim=1)
    return torch.where(den > 0, num / den.clamp(min=torch.finfo(torch.float32).tiny), torch.full_like(den, float("nan")))
