"""The partitioned form of the embedding index: k-means on the device and a probed nearest-row search.

``EmbeddingIndex.query`` is exact and linear in the archive.  An ``IvfIndex`` cuts the rows into lists around k-means
centroids and searches, for every query row, only the lists of its ``nprobe`` nearest centroids (csrc/ivf.hip, DESIGN.md
section 4ab):

    fit = kmeans(emb, n_clusters, n_iter=10, init="random", seed=0)    # fit.centroids, .labels, .counts, .inertia, .n_iter
    ivf = IvfIndex(bank, n_lists=None, centroids=None, n_iter=10, seed=0, groups=None)
    idx, dist = ivf.query(queries, k, nprobe=8)                        # int64 [Q, k] ORIGINAL row numbers, float32 [Q, k]
    lists = ivf.probes(queries, nprobe)                                # int64 [Q, nprobe]
    idx, dist = ivf.knn_graph(k, include_self=True, nprobe=8)          # knn_graph's layout
    ivf.add(rows); kept = ivf.remove(which); ivf.refit(n_iter=10)
    ivf = IvfIndex(bank, n_lists, groups=obj)                          # int64 [N]: ivf.groups; ivf.add(rows, groups=obj_new)
    idx, dist = ivf.query(q, k, nprobe, query_groups=obj_q, exclude_same_group=True)    # no row of the query's own object
    idx, dist = ivf.query(q, k, nprobe, one_per_group=True)                             # the k nearest OBJECTS
    idx, dist = ivf.knn_graph(k, nprobe=8, group_mode="exclude")       # or "distinct", "exclude+distinct"

What an answer is.  With ``allowed(q)`` = the finite bank rows whose label is in ``probes(q)``, minus ``self_rows[q]``, the
answer of ``query`` is exactly the k-nearest answer over ``allowed(q)``: the selection scores, the merge and the returned
direct-form fp32 distances are those of ``EmbeddingIndex.query`` (``dist[q, j]`` has the bits ``ivf.index.query`` and
``radius`` return for that pair), ordered by (dist, original row number).  Fewer than ``k`` allowed rows give a tail of
``-1 / +inf``, a non-finite query row ``-1 / NaN``.  With ``nprobe == n_lists`` it is the exact search.  Which lists are
looked at is the only approximation; it is measured as recall and never hidden in the distances.  A row's answer does not
depend, bit for bit, on the other rows of the call, on the run, or on how the index was grown (``add`` in pieces against
built at once on the same centroids).

By source.  An index built with ``groups`` (one int64 per row, an alert's object) answers the two switches of
``EmbeddingIndex.query`` with the same contract over the probed lists.  Under ``exclude_same_group`` ``allowed(q)`` is
further restricted to the rows of another group than ``query_groups[q]``, and the answer is exactly
``EmbeddingIndex.query``'s grouped answer over ``allowed(q)``.  Under ``one_per_group`` (``k <= 32``) it is the k nearest
groups present in ``allowed(q)``, each by its best row by (score, row) -- a group whose rows lie in several probed lists
meets in the merge and is returned once.  ``self_rows`` stays a compare of positions and combines with every mode.
Distances are ``direct_distance()``'s, the bits of ``ivf.index.query`` for the same pair; the answer is ordered by (dist,
original row); the tail is ``-1 / +inf`` where fewer rows -- or groups -- are eligible and ``-1 / NaN`` for a non-finite
query row.  With ``nprobe == n_lists`` the answer is ``ivf.index.query(...)`` with the same switches, bit for bit, and a
row's answer still does not depend on the other rows of the call, on the run, or on whether the index was grown by ``add``.
Nothing is over-fetched and filtered: both switches act inside the selection kernel and its merge.

k-means.  ``init="random"`` takes ``n_clusters`` distinct finite rows by a permutation drawn from
``torch.Generator().manual_seed(seed)`` on the host (FAISS's rule); a float32 ``[n_clusters, D]`` tensor is taken as the
initial centroids.  An iteration assigns every row to its nearest centroid with ``EmbeddingIndex(centroids).query(rows, 1)``
-- a label is whatever that search returns, ties to the lower centroid -- and recomputes the centroids with
``btsbot_kmeans_update``: deterministic, no atomic on a sum, a centroid's bits depend on its cluster's rows alone.  A
cluster that ends an iteration empty keeps its centroid.  A non-finite row has label -1, enters no sum and no list.  After
the last iteration the rows are assigned once more: ``labels``, ``counts`` and ``inertia`` belong to the returned centroids.

The price of the lists is a second packed image in list order: every list starts on a 128-row tile boundary and is padded
with the record of a non-finite row, ``record_bytes`` per row (2.1 GB at 10^6 x 528) plus up to 128 padding records per
list, and with groups 8 bytes per position for the groups in list order.  Only the euclidean metric is built.  There is no
CPU fallback.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream
from .neighbors import GROUP_MODES, EmbeddingIndex, _check_group_args, _check_k, _groups, _n_rows_or_none, _rows

GRAPH_CHUNK = 65536   # rows per query call of IvfIndex.knn_graph


class KMeansFit(NamedTuple):
    centroids: torch.Tensor   # float32 [n_clusters, D]
    labels: torch.Tensor      # int64 [N], -1 for a non-finite row
    counts: torch.Tensor      # int64 [n_clusters]
    inertia: float            # the float64 sum of the squared returned distances
    n_iter: int


def _check_metric(metric) -> None:
    if metric != "euclidean":
        raise ValueError(f'IvfIndex and kmeans are built for metric="euclidean" only; {metric!r} is not built')


def _check_count(name: str, v, lo: int, hi: int) -> None:
    if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an int in {lo}..{hi}, got {v!r}")


def _check_n_iter(n_iter) -> None:
    if not isinstance(n_iter, int) or isinstance(n_iter, bool) or n_iter < 0:
        raise ValueError(f"n_iter must be an int >= 0, got {n_iter!r}")


def _check_seed(seed) -> None:
    if not isinstance(seed, int) or isinstance(seed, bool):
        raise ValueError(f"seed must be an int, got {seed!r}")


def _check_centroids(c, name: str, dim: Optional[int], device=None, n_clusters: Optional[int] = None) -> None:
    """ValueError for centroids that cannot be used, before anything touches the device."""
    if not isinstance(c, torch.Tensor) or c.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 torch.Tensor [n_clusters, D], got "
                         f"{c.dtype if isinstance(c, torch.Tensor) else type(c).__name__}")
    if c.dim() != 2 or not 1 <= c.shape[0] <= _lib.IVF_MAX_LISTS:
        raise ValueError(f"{name} must be [n_clusters, D] with 1 <= n_clusters <= {_lib.IVF_MAX_LISTS}, got {tuple(c.shape)}")
    if n_clusters is not None and c.shape[0] != n_clusters:
        raise ValueError(f"{name} holds {c.shape[0]} rows, n_clusters = {n_clusters}")
    if device is not None and c.device != device:
        raise ValueError(f"{name} is on {c.device}, the rows on {device}")
    if dim is not None and c.shape[1] != dim:
        raise ValueError(f"{name}: D = {c.shape[1]}, the rows have D = {dim}")


def default_n_lists(n_rows: int) -> int:
    """``round(sqrt(N))``, clipped to 1 .. 65,536."""
    return max(1, min(_lib.IVF_MAX_LISTS, int(round(float(n_rows) ** 0.5))))


def _assign(centroids: torch.Tensor, rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(labels int64 [N], dist float32 [N]): every row's nearest centroid by the existing exact search; -1 / NaN for a
    non-finite row."""
    idx, dist = EmbeddingIndex(centroids).query(rows, 1)
    return idx[:, 0].contiguous(), dist[:, 0].contiguous()


def kmeans_update(rows: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor,
                  order: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One centroid update in place (``btsbot_kmeans_update``): ``centroids[c]`` becomes the mean of the rows with
    ``labels == c``; an empty cluster's row is left untouched.  Returns the clusters' sizes, int64 [n_clusters].
    rows: float32 [N, D] contiguous; labels: int64 [N] in -1 .. n_clusters - 1; centroids: float32 [n_clusters, D]
    contiguous; order: the stable argsort of ``labels``, if the caller has it."""
    _check_centroids(centroids, "centroids", None)
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous float32 [N, D] tensor")
    if rows.device.type != "cuda":
        raise RuntimeError(f"btsbot_amd.ivf runs on the GPU; there is no CPU fallback (rows is on {rows.device})")
    n, dim = int(rows.shape[0]), int(rows.shape[1])
    if not 1 <= dim <= _lib.KNN_MAX_DIM:
        raise ValueError(f"rows: D must be in 1..{_lib.KNN_MAX_DIM}, got {dim}")
    _check_centroids(centroids, "centroids", dim, rows.device)
    if not centroids.is_contiguous():
        raise ValueError("centroids must be contiguous (they are updated in place)")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.shape != (n,) or \
            labels.device != rows.device:
        raise ValueError(f"labels must be an int64 [{n}] tensor on {rows.device}")
    nc = int(centroids.shape[0])
    L = _lib.lib()
    with torch.cuda.device(rows.device):
        labels = labels.contiguous()
        if order is None:
            order = torch.sort(labels, stable=True).indices
        counts = torch.empty(nc, dtype=torch.int64, device=rows.device)
        need = int(L.btsbot_kmeans_workspace(n, dim, nc))
        if need < 0:
            _lib.check(need, "btsbot_kmeans_workspace")
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=rows.device)
        _lib.check(L.btsbot_kmeans_update(_ptr(rows), n, dim, _ptr(labels), _ptr(order.contiguous()), nc, _ptr(centroids),
                                          _ptr(counts), _ptr(ws), need, _stream(rows.device)), "btsbot_kmeans_update")
    return counts


def _lloyd(rows: torch.Tensor, centroids: torch.Tensor, n_iter: int) -> None:
    for _ in range(n_iter):
        labels, _ = _assign(centroids, rows)
        kmeans_update(rows, labels, centroids)


def _random_init(rows: torch.Tensor, n_clusters: int, seed: int) -> torch.Tensor:
    """``n_clusters`` distinct finite rows by a host permutation of the finite rows (one host read: their number)."""
    finite = torch.isfinite(rows).all(dim=1) & torch.isfinite((rows * rows).sum(dim=1))
    at = finite.nonzero().view(-1)
    n_finite = int(at.shape[0])
    if n_clusters > n_finite:
        raise ValueError(f'n_clusters = {n_clusters} exceeds the {n_finite} finite rows (init="random" takes distinct rows)')
    perm = torch.randperm(n_finite, generator=torch.Generator().manual_seed(seed))[:n_clusters]
    return rows[at[perm.to(rows.device)]].clone()


def kmeans(emb: torch.Tensor, n_clusters: int, n_iter: int = 10, init="random", seed: int = 0,
           metric: str = "euclidean") -> KMeansFit:
    """Lloyd's k-means of the rows of ``emb`` [N, D] on the device (see the module text).  init: ``"random"`` or a
    float32 ``[n_clusters, D]`` tensor of initial centroids.  One host read for ``inertia`` (and one for the random
    init)."""
    _check_metric(metric)
    _check_count("n_clusters", n_clusters, 1, _lib.IVF_MAX_LISTS)
    _check_n_iter(n_iter)
    _check_seed(seed)
    if isinstance(init, str):
        if init != "random":
            raise ValueError(f'init must be "random" or a float32 [n_clusters, D] tensor, got {init!r} (k-means++ is not built)')
    else:
        _check_centroids(init, "init", None, n_clusters=n_clusters)
    rows = _rows(emb, "emb")
    if not isinstance(init, str):
        _check_centroids(init, "init", int(rows.shape[1]), rows.device)
    with torch.cuda.device(rows.device):
        centroids = _random_init(rows, n_clusters, seed) if isinstance(init, str) else init.detach().clone().contiguous()
        _lloyd(rows, centroids, n_iter)
        labels, dist = _assign(centroids, rows)
        counts = torch.bincount(labels[labels >= 0], minlength=n_clusters)
        d = torch.where(labels >= 0, dist.to(torch.float64), torch.zeros((), dtype=torch.float64, device=rows.device))
        inertia = float((d * d).sum())
    return KMeansFit(centroids, labels, counts, inertia, n_iter)


class IvfIndex:
    """An ``EmbeddingIndex`` (``.index``: the fp32 rows, ids and packed records; rows keep their numbers) with its rows
    cut into ``n_lists`` lists around centroids, and the list-ordered operand image the probed search walks.

    n_lists: None is ``round(sqrt(N))``, clipped to 1 .. 65,536.  centroids: a finite float32 ``[n_lists, D]`` tensor
    skips the fit (checking that it is finite is the one host read of the construction).  n_iter, seed: the fit's, from
    ``init="random"``.  groups: one int64 group per bank row (an alert's object), or None; they are kept by ``.index``
    (``ivf.groups`` is ``ivf.index.groups``, and ``ivf.index.query(..., exclude_same_group=True)`` works as ever) and, in
    list order, next to the list image.  An index with groups takes them with every ``add``.  Calls on one index must be
    ordered by the caller's streams."""

    def __init__(self, bank: torch.Tensor, n_lists: Optional[int] = None, *, centroids: Optional[torch.Tensor] = None,
                 n_iter: int = 10, seed: int = 0, metric: str = "euclidean", groups: Optional[torch.Tensor] = None):
        _check_metric(metric)
        if n_lists is not None:
            _check_count("n_lists", n_lists, 1, _lib.IVF_MAX_LISTS)
        _check_n_iter(n_iter)
        _check_seed(seed)
        if centroids is not None:
            _check_centroids(centroids, "centroids", None, n_clusters=n_lists)
        if groups is not None and _n_rows_or_none(bank) is not None:
            groups = _groups(groups, "groups", int(bank.shape[0]), bank.device)
        rows = _rows(bank, "bank")
        if centroids is not None:
            _check_centroids(centroids, "centroids", int(rows.shape[1]), rows.device)
        self.metric = metric
        self.index = EmbeddingIndex(rows, groups=groups)
        self.device, self.dim = self.index.device, self.index.dim
        with torch.cuda.device(self.device):
            if centroids is not None:
                c = centroids.detach().clone().contiguous()
                if not bool(torch.isfinite(c).all()):
                    raise ValueError("centroids must be finite")
            else:
                if n_lists is None:
                    n_lists = default_n_lists(len(self.index))
                c = _random_init(self.index.bank, n_lists, seed)
                _lloyd(self.index.bank, c, n_iter)
            self._set_centroids(c)
            self.labels = _assign(c, self.index.bank)[0]
            self._layout()

    def __len__(self) -> int:
        return len(self.index)

    @property
    def groups(self) -> Optional[torch.Tensor]:
        """The rows' groups, int64 [len] (``index.groups``), or None for an index without groups."""
        return self.index.groups

    @property
    def n_lists(self) -> int:
        return int(self.centroids.shape[0])

    def _set_centroids(self, c: torch.Tensor) -> None:
        self.centroids = c
        self._cindex = EmbeddingIndex(c)

    def _layout(self) -> None:
        """The list image, the row maps and the list sizes from ``self.labels`` (``btsbot_ivf_layout``) and, on an index
        with groups, the groups in list order (``btsbot_ivf_layout_groups``)."""
        L, dev, n, nl = _lib.lib(), self.device, len(self.index), self.n_lists
        rec = self.index._record_bytes()
        rows = int(L.btsbot_ivf_list_rows(n, nl))
        if rows < 0:
            _lib.check(rows, "btsbot_ivf_list_rows")
        with torch.cuda.device(dev):
            order = torch.sort(self.labels, stable=True).indices
            self._list_packed = torch.empty(rows * rec, dtype=torch.uint8, device=dev)
            self._row_of = torch.empty(rows, dtype=torch.int32, device=dev)
            self._pos_of = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            self.list_sizes = torch.empty(nl, dtype=torch.int64, device=dev)
            self._list_tile = torch.empty(nl + 1, dtype=torch.int32, device=dev)
            need = 2 * ((4 * (nl + 1) + 255) // 256 * 256)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            _lib.check(L.btsbot_ivf_layout(_ptr(self.index._packed), n, self.dim, _ptr(self.labels), _ptr(order), nl,
                                           _ptr(self._list_packed), rows, _ptr(self._row_of), _ptr(self._pos_of),
                                           _ptr(self.list_sizes), _ptr(self._list_tile), _ptr(ws), need, _stream(dev)),
                       "btsbot_ivf_layout")
            self._list_groups = None
            if self.index.groups is not None:
                self._list_groups = torch.empty(rows, dtype=torch.int64, device=dev)
                _lib.check(L.btsbot_ivf_layout_groups(_ptr(self.index.groups), n, nl, _ptr(self._row_of), rows,
                                                      _ptr(self._list_groups), _stream(dev)), "btsbot_ivf_layout_groups")
        self._list_rows = rows

    def lists(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """The lists as a CSR: ``indptr`` int64 [n_lists + 1] and ``rows`` int64 [finite rows], list l's original row
        numbers, ascending, at ``rows[indptr[l]:indptr[l + 1]]`` (read from the list image's row map)."""
        indptr = torch.zeros(self.n_lists + 1, dtype=torch.int64, device=self.device)
        indptr[1:] = torch.cumsum(self.list_sizes, 0)
        return indptr, self._row_of[self._row_of >= 0].to(torch.int64)

    # ---- growth
    def add(self, rows: torch.Tensor, *, groups: Optional[torch.Tensor] = None) -> "IvfIndex":
        """``index.add(rows, groups=groups)``; the new rows' labels come from the FIXED centroids, then the lists are laid
        out again.  groups: int64 [n], required if and only if the index was built with groups."""
        if (groups is None) != (self.index.groups is None):
            raise ValueError("add(rows, groups=...) takes groups if and only if the index was built with groups")
        rows = _rows(rows, "rows", self.device)
        if rows.shape[1] != self.dim:
            raise ValueError(f"rows: D = {rows.shape[1]}, the index holds D = {self.dim}")
        self.index.add(rows, groups=groups)
        if rows.shape[0]:
            with torch.cuda.device(self.device):
                self.labels = torch.cat([self.labels, _assign(self.centroids, rows)[0]])
                self._layout()
        return self

    def remove(self, which: torch.Tensor) -> torch.Tensor:
        """``index.remove(which)``: returns ``kept``; ``labels`` becomes ``labels[kept]`` (the groups follow inside
        ``index``) and the lists are laid out again."""
        n = len(self.index)
        kept = self.index.remove(which)
        if int(kept.shape[0]) != n:
            with torch.cuda.device(self.device):
                self.labels = self.labels[kept].contiguous()
                self._layout()
        return kept

    def refit(self, n_iter: int = 10, seed: int = 0) -> "IvfIndex":
        """k-means again from the current centroids over the current rows (``seed`` has no part in it: nothing is drawn),
        then every row is assigned and the lists are laid out again."""
        _check_n_iter(n_iter)
        _check_seed(seed)
        with torch.cuda.device(self.device):
            c = self.centroids.clone()
            _lloyd(self.index.bank, c, n_iter)
            self._set_centroids(c)
            self.labels = _assign(c, self.index.bank)[0]
            self._layout()
        return self

    # ---- search
    def _check_nprobe(self, nprobe) -> None:
        hi = min(self.n_lists, _lib.IVF_MAX_NPROBE)
        if not isinstance(nprobe, int) or isinstance(nprobe, bool) or not 1 <= nprobe <= hi:
            raise ValueError(f"nprobe must be an int in 1..{hi} (min(n_lists, {_lib.IVF_MAX_NPROBE}): the merge's cap), "
                             f"got {nprobe!r}")

    def _queries(self, queries) -> torch.Tensor:
        q = _rows(queries, "queries", self.device)
        if q.shape[1] != self.dim:
            raise ValueError(f"queries: D = {q.shape[1]}, the index holds D = {self.dim}")
        return q

    def probes(self, queries: torch.Tensor, nprobe: int) -> torch.Tensor:
        """int64 [Q, nprobe]: the lists of each query row's ``nprobe`` nearest centroids, nearest first
        (``EmbeddingIndex(centroids).query(queries, nprobe)[0]``; -1 throughout for a non-finite query row).  An empty
        list may be probed and contributes nothing."""
        self._check_nprobe(nprobe)
        return self._cindex.query(self._queries(queries), nprobe)[0]

    def query(self, queries: torch.Tensor, k: int, nprobe: int = 8, self_rows: Optional[torch.Tensor] = None, *,
              query_groups: Optional[torch.Tensor] = None, exclude_same_group: bool = False,
              one_per_group: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """``idx`` int64 [Q, k] (ORIGINAL row numbers) and ``dist`` float32 [Q, k]: each query row's ``k`` nearest rows
        among the lists of its ``nprobe`` nearest centroids (see the module text).  self_rows: int64 [Q], query row i is
        bank row ``self_rows[i]`` and is excluded by position, so its duplicates stay legitimate neighbours; it combines
        with both switches.  query_groups: int64 [Q], the query rows' groups.  exclude_same_group: no row of the query
        row's own group.  one_per_group: at most one row per group, its nearest; the ``k`` nearest groups (``k <= 32``).
        Both need an index built with ``groups``."""
        _check_k(k, 0)
        self._check_nprobe(nprobe)
        flags = 0
        if query_groups is not None or exclude_same_group is not False or one_per_group is not False:
            flags = _check_group_args(k, self.index.groups is not None, query_groups, exclude_same_group, one_per_group)
            nq = _n_rows_or_none(queries)
            if query_groups is not None and nq is not None:
                query_groups = _groups(query_groups, "query_groups", nq, self.device)
        if self_rows is not None:
            nq = _n_rows_or_none(queries)
            if not isinstance(self_rows, torch.Tensor) or self_rows.dtype != torch.int64:
                raise ValueError("self_rows must be an int64 torch.Tensor [Q] of bank row numbers, got "
                                 f"{self_rows.dtype if isinstance(self_rows, torch.Tensor) else type(self_rows).__name__}")
            if self_rows.dim() != 1 or (nq is not None and self_rows.shape[0] != nq):
                raise ValueError(f"self_rows must hold one bank row per query row, [{nq}], got {tuple(self_rows.shape)}")
            if self_rows.device != self.device:
                raise ValueError(f"self_rows is on {self_rows.device}, the index on {self.device}")
        q = self._queries(queries)
        nq, dev, n = int(q.shape[0]), self.device, len(self.index)
        idx = torch.empty((nq, k), dtype=torch.int64, device=dev)
        dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
        if nq == 0:
            return idx, dist
        L = _lib.lib()
        need = int(L.btsbot_ivf_workspace_grouped(nq, self.dim, k, nprobe, self.n_lists, flags))
        if need < 0:
            _lib.check(need, "btsbot_ivf_workspace_grouped")
        with torch.cuda.device(dev):
            probes = self._cindex.query(q, nprobe)[0]
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            sr = None if self_rows is None else self_rows.detach().contiguous()
            args = (_ptr(q), nq, _ptr(self.index._bank), n, self.dim, k, _ptr(probes), nprobe, _ptr(sr),
                    _ptr(self._list_packed), self._list_rows, _ptr(self._row_of), _ptr(self._pos_of), _ptr(self._list_tile),
                    self.n_lists, _ptr(idx), _ptr(dist), _ptr(ws), need, _stream(dev))
            if flags == 0:
                _lib.check(L.btsbot_ivf_query(*args), "btsbot_ivf_query")
            else:
                _lib.check(L.btsbot_ivf_query_grouped(*args, _ptr(query_groups), _ptr(self._list_groups), flags),
                           "btsbot_ivf_query_grouped")
        return idx, dist

    def knn_graph(self, k: int, include_self: bool = True, nprobe: int = 8,
                  group_mode: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Every row of the index among the others, in ``neighbors.knn_graph``'s layout: ``idx`` int64 [N, k], ``dist``
        float32 [N, k].  include_self=True: the row itself first at distance 0 (-1 / NaN for a non-finite row), then its
        ``k - 1`` nearest others among its probed lists; False: ``k`` others.  A row is excluded by position: its
        duplicates are legitimate neighbours.  group_mode (an index with groups; a row's own group is its query group):
        ``"exclude"`` the others are rows of OTHER groups only, ``"distinct"`` at most one row per group,
        ``"exclude+distinct"`` both, as ``neighbors.knn_graph``; None: no groups are read.  The rows are asked in chunks."""
        _check_k(k, 0)
        self._check_nprobe(nprobe)
        kw = {}
        if group_mode is not None:
            if group_mode not in GROUP_MODES:
                raise ValueError(f"group_mode must be None or one of {GROUP_MODES}, got {group_mode!r}")
            groups = self.index.groups
            if groups is None:
                raise ValueError("group_mode needs an index built with groups=...")
            kw = dict(exclude_same_group="exclude" in group_mode, one_per_group="distinct" in group_mode)
            _check_group_args(k - 1 if include_self else k, True, groups, kw["exclude_same_group"], kw["one_per_group"])
        rows, dev = self.index.bank, self.device
        n = int(rows.shape[0])
        idx = torch.empty((n, k), dtype=torch.int64, device=dev)
        dist = torch.empty((n, k), dtype=torch.float32, device=dev)
        first = 0
        if include_self:
            finite = torch.isfinite(rows).all(dim=1)
            idx[:, 0] = torch.where(finite, torch.arange(n, device=dev), torch.full_like(idx[:, 0], -1))
            dist[:, 0] = torch.where(finite, torch.zeros_like(dist[:, 0]), torch.full_like(dist[:, 0], float("nan")))
            first = 1
        if k > first:
            for a in range(0, n, GRAPH_CHUNK):
                b = min(n, a + GRAPH_CHUNK)
                if kw:
                    kw["query_groups"] = groups[a:b]
                i, d = self.query(rows[a:b], k - first, nprobe, self_rows=torch.arange(a, b, device=dev), **kw)
                idx[a:b, first:], dist[a:b, first:] = i, d
        return idx, dist
