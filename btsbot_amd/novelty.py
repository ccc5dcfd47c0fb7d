"""Which alerts look like nothing in the archive: the local outlier factor on the exact neighbour lists, on the device.

``count_within(queries, r)`` answers novelty with a radius nobody knows in advance, and one that means something else in
a dense cluster than in a sparse region.  The local outlier factor (LOF, Breunig et al. 2000; scikit-learn's
``LocalOutlierFactor``) compares a row's density with its neighbours' densities and takes ``n_neighbors`` alone
(csrc/lof.hip):

    lof = local_outlier_factor(emb, n_neighbors=20)              # float64 [N]; about 1 inside a cluster, >> 1 isolated
    m = NoveltyModel(bank_or_index, n_neighbors=20)              # rows, an EmbeddingIndex or a MapIndex
    m.kdist, m.lrd, m.lof                                        # float64 [N]: the fit of the bank among itself
    s = m.score(queries)                                         # float64 [Q]: scikit-learn's novelty=True
    t = m.threshold(contamination=0.01)                          # float; ``s > t`` flags
    d = kth_neighbor_distance(idx, dist)                         # float32 [Q]: the last present distance

With ``kdist(i)`` the distance of row i's last neighbour, ``reach(i, j) = max(dist(i, j), kdist(j))``, ``lrd(i) = 1 /
(mean_j reach(i, j) + 1e-10)`` and ``lof(i) = mean_j lrd(j) / lrd(i)`` over the row's present neighbours: float64 on the
fp32 direct-form distances ``knn_graph`` / ``query`` return, summed in an order fixed by the row's own columns, so a row's
score does not depend, bit for bit, on the other rows of the call, on ``splits`` or on the run.  A row with fewer than
``n_neighbors`` eligible neighbours is scored on those it has (scikit-learn clips ``n_neighbors`` instead); a non-finite
row, and a row with no eligible neighbour, scores NaN.  A row among ``n_neighbors + 1`` duplicates has ``lrd = 1e10`` and
``lof = 1`` exactly, as in scikit-learn.  Ties go by (dist, index).

Rows that belong together.  An archive where one object holds many epochs defeats a plain LOF: a lone far object with five
alerts has four near-identical siblings, is as dense as they are and scores about 1.  With ``groups=obj`` (an int64 per
row, ``alert_utils.object_keys``) the fit leaves a row's own object out of its neighbours (``group_mode="exclude"``;
``"distinct"`` / ``"exclude+distinct"`` as ``knn_graph``), and ``score(..., query_groups=obj_q, exclude_same_group=True)``
does the same for new alerts of objects the archive knows.

Fit and score read nothing from the host and are queued on the current stream; only ``threshold`` reads.  There is no CPU
fallback.  A fit does NOT follow ``index.add`` or ``index.remove`` by itself: ``refit()`` recomputes it for the rows the
index holds now, and ``score`` refuses an index that has grown since, or that rows were removed from (it compares
``index.generation``: after ``remove`` and ``add`` the lengths can coincide).

Following the archive.  ``NoveltyModel(index, 20, keep_graph=True)`` keeps the neighbour graph of the fit
(``model.graph``, a ``graph.KnnGraph``, DESIGN.md sections 4x and 4y), and ``model.update()`` after ``index.add`` and
``index.remove`` brings graph and fit to the rows the index holds now at the cost of the new rows and of the rows whose list
lost an entry: ``graph.update()`` and ``btsbot_lof_fit`` over all rows.
``update`` reads the host where ``radius`` does.  A graph kept elsewhere serves the same way:
``local_outlier_factor(None, k, knn=(g.idx, g.dist))`` and ``fuzzy_graph(*g.self_first())`` take it as it is.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from . import _lib
from .graph import KnnGraph
from .mapindex import MapIndex
from ._lib import ptr as _ptr, stream as _stream
from .neighbors import GROUP_MODES, EmbeddingIndex, _stale_fit, knn_graph

__all__ = ["NoveltyModel", "local_outlier_factor", "kth_neighbor_distance"]


def _check_n_neighbors(k) -> None:
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= _lib.LOF_MAX_K:
        raise ValueError(f"n_neighbors must be an int in 1..{_lib.LOF_MAX_K}, got {k!r}")


def _check_group_mode(group_mode) -> None:
    if group_mode not in GROUP_MODES:
        raise ValueError(f"group_mode must be one of {GROUP_MODES}, got {group_mode!r}")


def _graph(idx, dist, name: str = "knn") -> Tuple[torch.Tensor, torch.Tensor]:
    """(idx int64 [rows, k], dist float32 [rows, k]) on one GPU, contiguous; ValueError otherwise."""
    if not isinstance(idx, torch.Tensor) or not isinstance(dist, torch.Tensor):
        raise ValueError(f"{name} must be (idx, dist), two torch.Tensors")
    if idx.dim() != 2 or idx.shape != dist.shape or idx.dtype != torch.int64 or dist.dtype != torch.float32:
        raise ValueError(f"{name}: idx must be int64 [rows, k] and dist float32 of the same shape, got {idx.dtype} "
                         f"{tuple(idx.shape)} and {dist.dtype} {tuple(dist.shape)}")
    if idx.device.type != "cuda":
        raise RuntimeError(f"btsbot_amd.novelty runs on the GPU; there is no CPU fallback ({name} is on {idx.device})")
    if dist.device != idx.device:
        raise ValueError(f"{name}: idx is on {idx.device}, dist on {dist.device}")
    if not 1 <= idx.shape[1] <= _lib.LOF_MAX_K:
        raise ValueError(f"{name}: k must be in 1..{_lib.LOF_MAX_K}, got {idx.shape[1]}")
    return idx.detach().contiguous(), dist.detach().contiguous()


def _fit(idx: torch.Tensor, dist: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """btsbot_lof_fit on a checked graph: (kdist, lrd, lof), float64 [n] each."""
    n, k = int(idx.shape[0]), int(idx.shape[1])
    dev = idx.device
    with torch.cuda.device(dev):
        kdist, lrd, lof = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        _lib.check(_lib.lib().btsbot_lof_fit(_ptr(idx), _ptr(dist), n, k, _ptr(kdist), _ptr(lrd), _ptr(lof), _stream(dev)),
                   "btsbot_lof_fit")
    return kdist, lrd, lof


def _score(idx: torch.Tensor, dist: torch.Tensor, kdist: torch.Tensor, lrd: torch.Tensor,
           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """btsbot_lof_score on a checked graph of new rows: (lrd, lof), float64 [q] each."""
    q, k = int(idx.shape[0]), int(idx.shape[1])
    dev = idx.device
    with torch.cuda.device(dev):
        out_lrd, out_lof = (torch.empty(q, dtype=torch.float64, device=dev) for _ in range(2))
        _lib.check(_lib.lib().btsbot_lof_score(_ptr(idx), _ptr(dist), q, k, _ptr(kdist), _ptr(lrd), int(kdist.shape[0]),
                                               _ptr(out_lrd), _ptr(out_lof), _stream(dev)), "btsbot_lof_score")
    return out_lrd, out_lof


def local_outlier_factor(emb: Optional[torch.Tensor], n_neighbors: int = 20, metric: str = "euclidean", *,
                         groups: Optional[torch.Tensor] = None, group_mode: str = "exclude", method: str = "tiles",
                         knn: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, splits: int = 0) -> torch.Tensor:
    """The local outlier factor of every row of ``emb`` [N, D] among the others, float64 [N]: about 1 inside a cluster,
    far above 1 for an isolated row, NaN for a non-finite row or one without an eligible neighbour.

    The graph is ``knn_graph(emb, n_neighbors, include_self=False, metric, groups=, group_mode=, method=, splits=)`` and
    every argument check is that function's (``method="grid"`` for a 2-D map; the ``"distinct"`` modes hold
    ``n_neighbors <= 32``).  knn=(idx, dist): such a graph computed before, of at least ``n_neighbors`` columns (the first
    ``n_neighbors`` are read; ``emb`` may be None).  Nothing is read from the host."""
    _check_n_neighbors(n_neighbors)
    _check_group_mode(group_mode)
    if knn is None:
        idx, dist = knn_graph(emb, n_neighbors, False, metric, groups=groups, group_mode=group_mode, splits=splits,
                              method=method)
    else:
        if not isinstance(knn, (tuple, list)) or len(knn) != 2:
            raise ValueError("knn must be (idx, dist) as knn_graph(..., include_self=False) returns them")
        idx, dist = _graph(*knn)
        if idx.shape[1] < n_neighbors:
            raise ValueError(f"knn holds {idx.shape[1]} columns, fewer than n_neighbors = {n_neighbors}")
        if isinstance(emb, torch.Tensor) and emb.dim() == 2 and emb.shape[0] != idx.shape[0]:
            raise ValueError(f"knn holds {idx.shape[0]} rows, emb {emb.shape[0]}")
        if idx.shape[1] > n_neighbors:
            idx, dist = idx[:, :n_neighbors].contiguous(), dist[:, :n_neighbors].contiguous()
    return _fit(idx, dist)[2]


class NoveltyModel:
    """The LOF fit of a bank among itself, kept to score new rows against it (scikit-learn's ``novelty=True``).

    bank_or_index: rows float [N, D] (an ``EmbeddingIndex`` is built on them, with ``groups``), an ``EmbeddingIndex`` or a
    ``MapIndex``.  An index brings its own metric and groups: ``groups=`` next to an index is a ``ValueError``.
    group_mode: how the FIT treats the groups, as ``knn_graph`` (``"exclude"``: a row's neighbours are rows of other
    groups only).  ``kdist``, ``lrd`` and ``lof`` are float64 [N].

    The fit does not follow ``index.add`` or ``index.remove``; ``refit()`` recomputes it.  keep_graph=True (an ``EmbeddingIndex`` or rows;
    a ``MapIndex`` is a ``ValueError``): the model keeps ``graph``, the ``KnnGraph`` of ``n_neighbors`` columns the fit
    is computed on (``n_neighbors <= 32`` in the ``"distinct"`` modes); ``refit()`` rebuilds it, and ``update()`` follows
    ``index.add`` and ``index.remove`` at the cost of the new and the damaged rows.  The default keeps nothing.  Calls on one model must be ordered by the
    caller's streams."""

    def __init__(self, bank_or_index: Union[torch.Tensor, EmbeddingIndex, MapIndex], n_neighbors: int = 20,
                 metric: str = "euclidean", *, groups: Optional[torch.Tensor] = None, group_mode: str = "exclude",
                 keep_graph: bool = False):
        _check_n_neighbors(n_neighbors)
        _check_group_mode(group_mode)
        if not isinstance(keep_graph, bool):
            raise ValueError(f"keep_graph must be a bool, got {keep_graph!r}")
        if keep_graph and isinstance(bank_or_index, MapIndex):
            raise ValueError("keep_graph=True needs an EmbeddingIndex: a MapIndex has no add to follow")
        if isinstance(bank_or_index, (EmbeddingIndex, MapIndex)):
            index = bank_or_index
            if groups is not None:
                raise ValueError("groups= next to an index: the model uses the index's own groups (build the index with "
                                 "groups=...)" + ("" if index.groups is None else "; this one already has them"))
            index_metric = getattr(index, "metric", "euclidean")
            if metric != index_metric:
                raise ValueError(f"metric = {metric!r}, the index holds {index_metric!r}")
        else:
            index = EmbeddingIndex(bank_or_index, metric, groups=groups)
        if isinstance(index, MapIndex) and index.groups is not None and group_mode != "exclude":
            raise ValueError(f'a MapIndex knows group_mode="exclude" only, got {group_mode!r}')
        self.index = index
        self.n_neighbors = n_neighbors
        self.metric = getattr(index, "metric", "euclidean")
        self.group_mode = group_mode
        self.device = index.device
        self.graph = None
        if keep_graph:
            self.graph = KnnGraph(index, n_neighbors, self.metric, group_mode=group_mode)
            self._set_fit(_fit(self.graph.idx, self.graph.dist))
        else:
            self.refit()

    def __len__(self) -> int:
        """The rows the fit covers."""
        return int(self.kdist.shape[0])

    def _rows(self) -> torch.Tensor:
        return self.index.points if isinstance(self.index, MapIndex) else self.index.bank

    def refit(self) -> "NoveltyModel":
        """Fits the rows the index holds now (after ``index.add``): one neighbour search and three launches.  A kept
        graph is rebuilt."""
        if self.graph is not None:
            self.graph.rebuild()
            self._set_fit(_fit(self.graph.idx, self.graph.dist))
            return self
        kw = {}
        if self.index.groups is not None:
            kw = dict(query_groups=self.index.groups, exclude_same_group="exclude" in self.group_mode)
            if not isinstance(self.index, MapIndex):
                kw["one_per_group"] = "distinct" in self.group_mode
        idx, dist = self.index.query(self._rows(), self.n_neighbors, self_offset=0, **kw)
        self._set_fit(_fit(idx, dist))
        return self

    def _set_fit(self, fit) -> None:
        self.kdist, self.lrd, self.lof = fit
        self._generation = getattr(self.index, "generation", 0)

    def update(self, stats: Optional[dict] = None) -> "NoveltyModel":
        """Follows ``index.add`` and ``index.remove`` at the cost of the new and the damaged rows (``keep_graph=True`` only): ``graph.update(stats)``, then
        ``btsbot_lof_fit`` over all rows -- the fit is three launches whatever the archive holds, so it is not made
        incremental.  ``kdist``, ``lrd`` and ``lof`` are those of the updated graph, whose promise is ``KnnGraph``'s.
        Reads the host where ``radius`` does."""
        if getattr(self, "graph", None) is None:
            raise RuntimeError("update() needs the model's neighbour graph: build the model with keep_graph=True (or "
                               "call refit(), which searches every pair again)")
        self.graph.update(stats)
        self._set_fit(_fit(self.graph.idx, self.graph.dist))
        return self

    def score(self, queries: torch.Tensor, *, query_groups: Optional[torch.Tensor] = None,
              exclude_same_group: bool = False, one_per_group: bool = False, return_lrd: bool = False, splits: int = 0):
        """The local outlier factor of NEW rows ``queries`` [Q, D] against the fitted bank, float64 [Q] (with
        ``return_lrd`` the pair ``(lof, lrd)``): ``index.query(queries, n_neighbors, ...)`` and one launch.  A query
        identical to a bank row finds it at distance 0.  query_groups / exclude_same_group / one_per_group: as
        ``EmbeddingIndex.query`` -- leave out the rows of the query's own object.  NaN for a non-finite row and for a row
        without an eligible neighbour.  Nothing is read from the host."""
        stale = _stale_fit(self.index, len(self), self._generation)
        if stale is not None:
            raise RuntimeError(stale + " -- call refit()" + (" or update()" if self.graph is not None else
                                                             " (a model built with keep_graph=True has update())"))
        kw = dict(query_groups=query_groups, exclude_same_group=exclude_same_group)
        if isinstance(self.index, MapIndex):
            if one_per_group:
                raise ValueError("a MapIndex has no one_per_group")
            if splits:
                raise ValueError("a MapIndex has no splits")
        else:
            kw.update(one_per_group=one_per_group, splits=splits)
        idx, dist = self.index.query(queries, self.n_neighbors, **kw)
        lrd, lof = _score(idx, dist, self.kdist, self.lrd)
        return (lof, lrd) if return_lrd else lof

    def threshold(self, contamination: float = 0.01) -> float:
        """The ``(1 - contamination)`` quantile (linear interpolation) of the finite ``lof`` of the bank: ``score > t``
        flags about that share of rows that look like the bank's own.  scikit-learn's ``offset_`` with the sign turned.
        NaN when no row has a finite ``lof``.  The one host read of the model."""
        if isinstance(contamination, bool) or not isinstance(contamination, (int, float)) or not 0 < contamination <= 0.5:
            raise ValueError(f"contamination must be a float in (0, 0.5], got {contamination!r}")
        if len(self) == 0:
            return float("nan")
        finite = torch.isfinite(self.lof)
        vals = torch.sort(torch.where(finite, self.lof, torch.full_like(self.lof, float("inf")))).values
        cnt = finite.sum()
        pos = (1.0 - float(contamination)) * (cnt - 1).clamp(min=0).to(torch.float64)
        lo = pos.floor().to(torch.int64)
        hi = torch.minimum(lo + 1, (cnt - 1).clamp(min=0))
        v_lo, v_hi = vals.gather(0, torch.stack([lo, hi]))     # (a 0-dim tensor as an index would be read by the host)
        t = v_lo + (v_hi - v_lo) * (pos - lo.to(torch.float64))
        return float(torch.where(cnt > 0, t, torch.full_like(t, float("nan"))))


def kth_neighbor_distance(idx: torch.Tensor, dist: torch.Tensor) -> torch.Tensor:
    """float32 [Q]: the distance of each row's last present neighbour (``idx >= 0``) in lists as ``query`` / ``knn_graph``
    return them -- the k-th neighbour's distance where the row has k, the plainest novelty score there is.  NaN where a
    row has none.  Torch operations on the tensors' device; nothing is synchronised."""
    if idx.dim() != 2 or idx.shape != dist.shape or idx.dtype != torch.int64 or not dist.is_floating_point():
        raise ValueError(f"idx must be int64 [Q, k] and dist floating point of the same shape, got {idx.dtype} "
                         f"{tuple(idx.shape)} and {dist.dtype} {tuple(dist.shape)}")
    q, k = idx.shape
    d = dist.to(torch.float32)
    if k == 0:
        return d.new_full((q,), float("nan"))
    last = ((idx >= 0) * torch.arange(1, k + 1, device=idx.device)).amax(dim=1) - 1
    got = d.gather(1, last.clamp(min=0)[:, None])[:, 0]
    return torch.where(last >= 0, got, torch.full_like(got, float("nan")))
