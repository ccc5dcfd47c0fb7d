"""Clusters of any density: HDBSCAN on the exact searches, the spanning tree on the device.

``dbscan(emb, eps)`` needs a radius nobody knows in advance, and one radius cannot serve an archive whose clumps differ
in density by orders of magnitude.  HDBSCAN (Campello et al. 2013; scikit-learn's ``HDBSCAN``) takes ``min_cluster_size``
alone (csrc/mr_offer.hip, csrc/mst.hip, csrc/hdbscan_tree.hip):

    labels, prob = hdbscan(emb, min_cluster_size=5)              # int64 [N] (-1: noise), float64 [N]
    mst = mutual_reachability_mst(emb_or_index, min_samples)     # .edges int64 [n - 1, 2], .weights f32, .core f32 [N]
    tree = ClusterTree(mst)                                      # one tree, any parameters afterwards
    labels, prob = tree.labels(min_cluster_size, method="eom")
    labels = tree.cut(eps, min_cluster_size=1)                   # DBSCAN* at any eps from the same tree
    glosh = tree.outlier_scores(min_cluster_size)                # float64 [N]: GLOSH, 0 in a cluster's core, -> 1 far out
    m = ClusterModel(bank_or_index, min_cluster_size=5)          # the fit, kept to answer NEW rows
    labels, prob = m.predict(queries)                            # int64 [Q], float64 [Q]; return_details=True: a dict too

``core(i)`` is the distance from row i to its ``(min_samples - 1)``-th nearest other finite row (scikit-learn's rule: its
neighbour call counts the row itself) -- ``knn_graph(emb, min_samples - 1, include_self=False)``'s last column, 0 for
``min_samples = 1`` --, ``w(a, b) = max(d(a, b), core(a), core(b))`` in fp32 on the direct-form distances ``query``,
``radius`` and ``rank_of`` return, and the tree is a minimum spanning tree of the complete graph on the finite rows under
``w``.  It is built by Boruvka rounds: every row asks the grouped k-nearest search for its ``search_k`` nearest rows of
OTHER components (the row's component is its group), an offer kernel picks the lightest and decides whether the list
proves it the lightest of all, the rows it does not are asked again by ``radius`` at the weight found, and every
component's lightest offer is hooked by a lock-free union.  Nothing of size N x N is formed.  Which of several equally
light edges the tree holds may differ between runs; its sorted weights, and everything derived, may not.

The hierarchy (``btsbot_hdbscan_tree``, host C++ in the same library) is TIE-INVARIANT: all edges of one weight are
applied at once and every set of components they join becomes one node with two or more children.  Mutual-reachability
weights tie by construction (``w = core(a)`` for many edges of ``a``), and scikit-learn's binary dendrogram depends on
the order tied edges arrive in: its labels can change when the rows are merely permuted.  Here labels and probabilities
are a function of the rows alone -- not of their order, ``search_k``, ``splits``, the method or the run.  Two more stated
departures: ``lambda = 1 / w`` at ``w = 0`` is the tree's largest finite lambda (scikit-learn: infinite stabilities), and
clusters are numbered by their smallest row (``dbscan``'s rule).

With ``groups=obj`` a row's density is counted in OTHER objects' alerts (``group_mode="exclude"``, as ``dbscan(groups=)``
and the LOF); edges still join all finite rows.  A non-finite row has no core distance and no edge: label -1,
probability 0.  ``method="grid"`` takes the searches of a 2-D map from ``MapIndex``.  There is no CPU fallback.

New rows (csrc/mr_offer.hip, csrc/hdbscan_predict.hip).
``ClusterModel.predict`` answers a row ``q`` that was not
fitted from ONE neighbour search.  ``core(q)`` is the distance to its ``(min_samples - 1)``-th nearest eligible bank row
-- the value it would have as a row of the bank; the bank's own core distances do not move --, ``w(q, b) = max(dist(q, b),
core(q), core(b))`` in fp32, and the *nearest mutual-reachability neighbour* is the eligible bank row with the smallest
``(w, b)`` among ALL of them: the offer kernel takes it from the list of ``max(search_k, min_samples - 1, 1)`` rows where
the list proves it (the list is not full, or ``w`` is STRICTLY below what a row outside the list can have), the other rows
are asked again by ``radius`` at the weight found.  ``lambda_q = 1 / w`` in float64; from the cluster the neighbour fell
out of the row climbs, if the neighbour left it later than ``lambda_q``, to the cluster alive at ``lambda_q`` (a cluster
born AT ``lambda_q`` is left: everything that joins at one weight joins the parent); the label is that cluster's, the
strength ``min(lambda_q, m) / m`` as for a fitted row, the GLOSH score ``1 - min(lambda_q, death) / death`` with ``death``
the largest lambda below the cluster.  Fewer than ``min_samples - 1`` eligible rows: label -1, strength 0, score 1; a
non-finite row: -1, 0, NaN.  Every step is one correctly rounded operation on the search's fp32 distances, so a row's
answer does not depend, bit for bit, on the other rows of the call, on ``search_k``, ``splits``, the method or the run.
Departures from the ``hdbscan`` library's ``approximate_predict``: the exact nearest neighbour instead of the best of
``2 * min_samples``, this library's core-distance rule, the multiway tree, and ``lam_zero`` at ``w = 0``.
"""
from __future__ import annotations

import copy
import ctypes as C
import math
import time
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream
from .mapindex import MapIndex, check_grid_method
from .neighbors import EmbeddingIndex, _check_method, _check_splits, _groups, _metric, _rows, _stale_fit

__all__ = ["hdbscan", "mutual_reachability_mst", "MutualReachabilityMST", "ClusterTree", "ClusterModel"]

SELECTION_METHODS = tuple(_lib.HDBSCAN_METHOD)
U = 2.0 ** -24


def _check_int(name: str, v, lo: int, hi: Optional[int] = None) -> None:
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{name} must be an int {'>= ' + str(lo) if hi is None else f'in {lo}..{hi}'}, got {v!r}")


def _check_selection(min_cluster_size, method, allow_single_cluster) -> None:
    _check_int("min_cluster_size", min_cluster_size, 2)
    if method not in SELECTION_METHODS:
        raise ValueError(f"cluster_selection_method must be one of {SELECTION_METHODS}, got {method!r}")
    if not isinstance(allow_single_cluster, bool):
        raise ValueError(f"allow_single_cluster must be a bool, got {allow_single_cluster!r}")


def _check_mst_args(min_samples, search_k, splits, stats) -> None:
    _check_int("min_samples", min_samples, 1, _lib.KNN_MAX_K + 1)   # the core graph holds min_samples - 1 columns
    _check_int("search_k", search_k, 1, _lib.MST_MAX_K)
    _check_splits(splits)
    if stats is not None and not isinstance(stats, dict):
        raise ValueError(f"stats must be None or a dict, got {type(stats).__name__}")


class MutualReachabilityMST:
    """``edges`` int64 [n_finite - 1, 2] (lo, hi), ``weights`` float32 [n_finite - 1] in the order the rounds found
    them, ``core`` float32 [N] (NaN for a non-finite row), ``n`` = N."""

    def __init__(self, edges: torch.Tensor, weights: torch.Tensor, core: torch.Tensor):
        self.edges, self.weights, self.core = edges, weights, core
        self.n = int(core.shape[0])
        self.device = core.device

    def __len__(self) -> int:
        return int(self.weights.shape[0])


def _comp_view(index, comp: torch.Tensor):
    """A shallow copy of ``index`` whose groups are ``comp``: the searches exclude a row's own component.  The index
    itself, its rows and its own groups are not touched."""
    view = copy.copy(index)
    view._groups = comp
    if isinstance(index, MapIndex):
        view._sorted_groups = comp[index._sorted_rows.to(torch.int64)].contiguous()
    return view


def _sq_norms(rows: torch.Tensor) -> torch.Tensor:
    """float64 [rows]: |row|^2, 0 for a non-finite row"""
    sq = (rows.to(torch.float64) ** 2).sum(dim=1)
    return torch.where(torch.isfinite(sq), sq, torch.zeros_like(sq))


def _slack(index, rows: torch.Tensor, bank_sq_max: Optional[torch.Tensor] = None):
    """(slack [rows] or None, squared?, rel) of ``btsbot_mst_offer_knn`` and ``btsbot_cluster_offer_knn``: how far below
    the last listed distance a row the list of ``rows[i]`` does not hold may lie.  The grid ranks by the returned distance
    itself: nothing.  The tile search ranks its candidates by the expansion form and guarantees the j-th returned squared
    distance within tau = 8 (D + 2, or D + 6 below D = 4) u (|q|^2 + max |b|^2) of the j-th best, with the row's own
    |q|^2 (cosine: 8 (D + 2) u on 1 - cos; tests/knn_ref.py clause 3); the direct form the lists carry is within (D + 4) u
    relative of the truth at both ends.  bank_sq_max: max |b|^2 of the bank; None: ``rows`` ARE the bank."""
    if isinstance(index, MapIndex):
        return None, 0, 0.0
    d = index.dim
    rel = 4 * (d + 4) * U
    if index.metric == "cosine":
        return torch.full((int(rows.shape[0]),), 8 * (d + 2) * U, dtype=torch.float32, device=index.device), 0, rel
    sq = _sq_norms(rows)
    if bank_sq_max is None:
        bank_sq_max = sq.max() if sq.numel() else 0.0
    tau = 8 * (d + 2 if d >= 4 else d + 6) * U * (sq + bank_sq_max)
    return (tau * (1 + 2.0 ** -20)).to(torch.float32), 1, rel


def _radius_tier(index, rows: torch.Tensor, todo: torch.Tensor, best_w: torch.Tensor, query_groups, exclude_same_group,
                 skw: dict):
    """The second tier of an offer: ``radius`` around the unresolved rows ``todo`` at the weight their lists found, which
    contains the answer.  (indptr, indices, rdist, total) -- the caller's ``offer_csr`` takes the minimum over them.
    query_groups: of all ``rows``, or None.  skw: the search's own keywords (``splits``)."""
    st = {}
    asked, radius = rows[todo], best_w[todo]
    gkw = {} if query_groups is None else dict(query_groups=query_groups[todo])
    indptr, indices, rdist = index.radius(asked, radius, exclude_same_group=exclude_same_group, stats=st, **gkw, **skw)
    return indptr, indices, rdist, st["total"]


def _index_of(emb_or_index, groups, method: str, metric: str, what: str = "tree"):
    """The index ``mutual_reachability_mst`` and ``ClusterModel`` search: the one given (it brings its own metric and
    groups), or one built on the rows -- a ``MapIndex`` with ``method="grid"``."""
    if isinstance(emb_or_index, (EmbeddingIndex, MapIndex)):
        index = emb_or_index
        if groups is not None:
            raise ValueError("groups= next to an index: the " + what + " uses the index's own groups (build the index with "
                             "groups=...)" + ("" if index.groups is None else "; this one already has them"))
        index_metric = getattr(index, "metric", "euclidean")
        if metric != index_metric:
            raise ValueError(f"metric = {metric!r}, the index holds {index_metric!r}")
    else:
        _metric(metric)
        if method == "grid":
            check_grid_method(int(emb_or_index.shape[1]) if isinstance(emb_or_index, torch.Tensor)
                              and emb_or_index.dim() == 2 else None, metric)
        if groups is not None and (not isinstance(groups, torch.Tensor) or groups.dtype != torch.int64):
            raise ValueError("groups must be an int64 torch.Tensor, got "
                             f"{groups.dtype if isinstance(groups, torch.Tensor) else type(groups).__name__}")
        rows = _rows(emb_or_index, "emb")
        if groups is not None:
            groups = _groups(groups, "groups", int(rows.shape[0]), rows.device)
        index = MapIndex(rows, groups=groups) if method == "grid" else EmbeddingIndex(rows, metric, groups=groups)
    return index


def mutual_reachability_mst(emb_or_index: Union[torch.Tensor, EmbeddingIndex, MapIndex], min_samples: int = 5,
                            groups: Optional[torch.Tensor] = None, method: str = "tiles", search_k: int = 8,
                            stats: Optional[dict] = None, *, metric: str = "euclidean",
                            splits: int = 0) -> MutualReachabilityMST:
    """A minimum spanning tree of the mutual-reachability graph of the finite rows (see the module text).

    emb_or_index: rows float [N, D] (an index is built on them: ``EmbeddingIndex``, or ``MapIndex`` with
    ``method="grid"``, 2-D and euclidean only), an ``EmbeddingIndex`` or a ``MapIndex``.  An index brings its own metric
    and groups: ``groups=`` next to an index is a ``ValueError``.  groups: int64 [N]; core distances are then counted in
    rows of OTHER groups.  search_k: the list length of a round's search, 1..64 (no answer depends on it; 1 sends every
    row that is not inside a full list's reach through the radius tier).  splits: ``EmbeddingIndex.query``'s.
    stats: a dict that receives ``rounds``, ``n_finite`` and per round the lists ``components`` (at its start),
    ``unresolved`` (rows sent to the radius tier) and ``radius_total`` (entries of their lists); a dict that comes with
    ``{"time": True}`` also receives ``ms_search``, ``ms_offer``, ``ms_radius`` and ``ms_merge`` per round (the device
    is synchronised around every step then: tools/hdbscan_bench.py).
    Fewer finite rows than ``max(min_samples, 2)`` is a ``ValueError``; more than ``ceil(log2 n_finite) + 1`` rounds a
    ``RuntimeError``.  Host reads per round: the unresolved rows, the radius search's own, the number of components."""
    _check_mst_args(min_samples, search_k, splits, stats)
    _check_method(method)
    index = _index_of(emb_or_index, groups, method, metric)
    grid = isinstance(index, MapIndex)
    if grid and splits:
        raise ValueError("a MapIndex has no splits")
    rows = index.points if grid else index.bank
    n, dev, L = len(index), index.device, _lib.lib()
    skw = {} if grid else {"splits": splits}
    with torch.cuda.device(dev):
        comp = torch.arange(n, dtype=torch.int64, device=dev)
        # the finite rows are those a search answers; core distances from the graph among the others
        gkw = {} if index.groups is None else dict(query_groups=index.groups, exclude_same_group=True)
        probe = index.query(rows, max(min_samples - 1, 1), self_offset=0, **gkw, **skw)[1]
        finite = ~torch.isnan(probe[:, 0]) if n else torch.zeros(0, dtype=torch.bool, device=dev)
        if min_samples > 1:
            core = probe[:, -1].contiguous()
        else:
            core = torch.where(finite, torch.zeros_like(probe[:, 0]), torch.full_like(probe[:, 0], float("nan")))
            if index.groups is not None:   # (with groups the probe left the own object out; finiteness is the row's own)
                finite = ~torch.isnan(index.query(rows, 1, self_offset=0, **skw)[1][:, 0])
                core = torch.where(finite, torch.zeros_like(core), torch.full_like(core, float("nan")))
        n_finite = int(finite.sum()) if n else 0
        if n_finite < max(min_samples, 2):
            raise ValueError(f"{n_finite} finite rows, fewer than max(min_samples, 2) = {max(min_samples, 2)}")
        slack, squared, rel = _slack(index, rows)
        parent = torch.arange(n, dtype=torch.int32, device=dev)
        comp_w = torch.empty(n, dtype=torch.int32, device=dev)
        comp_edge = torch.empty(n, dtype=torch.int64, device=dev)
        edges = torch.zeros((n, 2), dtype=torch.int64, device=dev)
        weights = torch.zeros(n, dtype=torch.float32, device=dev)
        cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        best_w = torch.empty(n, dtype=torch.float32, device=dev)
        best_j = torch.empty(n, dtype=torch.int32, device=dev)
        unres = torch.empty(n, dtype=torch.uint8, device=dev)
        max_rounds = math.ceil(math.log2(n_finite)) + 1
        log = dict(rounds=0, n_finite=n_finite, components=[], unresolved=[], radius_total=[])
        timed = bool(stats and stats.get("time"))
        if timed:
            log.update(ms_search=[], ms_offer=[], ms_radius=[], ms_merge=[])

        def lap(key, since):
            """appends the milliseconds of a step to the log (a timed call only)"""
            if not timed:
                return 0.0
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            if key is not None:
                log[key].append((now - since) * 1e3)
            return now
        components = n_finite
        while components > 1:
            if log["rounds"] == max_rounds:
                raise RuntimeError(f"the spanning tree is not complete after {max_rounds} rounds ({components} components "
                                   f"of {n_finite} finite rows are left): every round at least halves them")
            view = _comp_view(index, comp)
            t0 = lap(None, 0.0)
            idx, dist = view.query(rows, search_k, query_groups=comp, exclude_same_group=True, **skw)
            t0 = lap("ms_search", t0)
            _lib.check(L.btsbot_mst_offer_knn(_ptr(idx), _ptr(dist), n, search_k, _ptr(core), _ptr(slack), squared, rel,
                                              _ptr(best_w), _ptr(best_j), _ptr(unres), _stream(dev)),
                       "btsbot_mst_offer_knn")
            todo = unres.nonzero().view(-1)                       # a host read: the rows of the radius tier
            t0 = lap("ms_offer", t0)
            total = 0
            if todo.numel():
                indptr, indices, rdist, total = _radius_tier(view, rows, todo, best_w, comp, True, skw)
                _lib.check(L.btsbot_mst_offer_csr(_ptr(indptr), _ptr(indices), _ptr(rdist), _ptr(todo), int(todo.numel()),
                                                  n, _ptr(core), _ptr(best_w), _ptr(best_j), _stream(dev)),
                           "btsbot_mst_offer_csr")
            t0 = lap("ms_radius", t0)
            _lib.check(L.btsbot_mst_merge(_ptr(best_w), _ptr(best_j), n, _ptr(comp), _ptr(parent), _ptr(comp_w),
                                          _ptr(comp_edge), _ptr(edges), _ptr(weights), n, _ptr(cursor), _stream(dev)),
                       "btsbot_mst_merge")
            log["rounds"] += 1
            log["components"].append(components)
            log["unresolved"].append(int(todo.numel()))
            log["radius_total"].append(int(total))
            left = n_finite - int(cursor.item())                  # the round's one read of its own: the components left
            lap("ms_merge", t0)
            if left >= components:
                raise RuntimeError(f"round {log['rounds']} joined nothing: {components} components are left")
            components = left
        if stats is not None:
            stats.update(log)
        m = n_finite - 1
        return MutualReachabilityMST(edges[:m].contiguous(), weights[:m].contiguous(), core)


def _host_edges(edges, weights, min_cluster_size, method, allow_single_cluster) -> Tuple[np.ndarray, np.ndarray]:
    """What the host passes take: the selection checked, ``edges`` int64 [m, 2] and ``weights`` float32 [m], contiguous."""
    _check_selection(min_cluster_size, method, allow_single_cluster)
    edges = np.ascontiguousarray(edges, dtype=np.int64).reshape(-1, 2)
    weights = np.ascontiguousarray(weights, dtype=np.float32)
    if edges.shape[0] != weights.shape[0]:
        raise ValueError(f"{edges.shape[0]} edges, {weights.shape[0]} weights")
    return edges, weights


def _tree_host(edges: np.ndarray, weights: np.ndarray, n: int, min_cluster_size: int, method: str = "eom",
               allow_single_cluster: bool = False):
    """``btsbot_hdbscan_tree`` on host arrays: (labels int64 [n], prob float64 [n], (parent, child, lambda, size))."""
    edges, weights = _host_edges(edges, weights, min_cluster_size, method, allow_single_cluster)
    labels, prob = np.empty(n, np.int64), np.empty(n, np.float64)
    cap = 2 * n
    cp, cc, cs = (np.empty(cap, np.int64) for _ in range(3))
    cl = np.empty(cap, np.float64)
    count = C.c_int64(0)

    def p(a):
        return C.c_void_p(a.ctypes.data)

    _lib.check(_lib.lib().btsbot_hdbscan_tree(p(edges), p(weights), edges.shape[0], n, min_cluster_size,
                                              _lib.HDBSCAN_METHOD[method], int(allow_single_cluster), p(labels), p(prob),
                                              p(cp), p(cc), p(cl), p(cs), cap, C.byref(count)), "btsbot_hdbscan_tree")
    m = count.value
    return labels, prob, (cp[:m].copy(), cc[:m].copy(), cl[:m].copy(), cs[:m].copy())


def _model_host(edges: np.ndarray, weights: np.ndarray, n: int, min_cluster_size: int, method: str = "eom",
                allow_single_cluster: bool = False) -> dict:
    """``btsbot_hdbscan_model`` on host arrays: the tables of a fitted tree as numpy arrays -- ``row_cluster`` int32 [n],
    ``row_lambda`` and ``outlier`` float64 [n]; ``parent`` int32, ``birth`` float64, ``label`` int32, ``max_lambda`` and
    ``death`` float64 [nc] -- and ``lam_zero``, a float."""
    edges, weights = _host_edges(edges, weights, min_cluster_size, method, allow_single_cluster)
    cap = max(n - 1, 1)
    t = dict(row_cluster=np.empty(n, np.int32), row_lambda=np.empty(n, np.float64), outlier=np.empty(n, np.float64),
             parent=np.empty(cap, np.int32), birth=np.empty(cap, np.float64), label=np.empty(cap, np.int32),
             max_lambda=np.empty(cap, np.float64), death=np.empty(cap, np.float64))
    nc, lam_zero = C.c_int64(0), C.c_double(0.0)
    _lib.check(_lib.lib().btsbot_hdbscan_model(C.c_void_p(edges.ctypes.data), C.c_void_p(weights.ctypes.data),
                                               edges.shape[0], n, min_cluster_size, _lib.HDBSCAN_METHOD[method],
                                               int(allow_single_cluster), *(C.c_void_p(a.ctypes.data) for a in t.values()),
                                               cap, C.byref(nc), C.byref(lam_zero)), "btsbot_hdbscan_model")
    for name in ("parent", "birth", "label", "max_lambda", "death"):
        t[name] = t[name][:nc.value].copy()
    t["lam_zero"] = lam_zero.value
    return t


class ClusterTree:
    """The hierarchy of one spanning tree, asked with any parameters afterwards: ``labels`` runs the host pass of the
    library (O(n log n), no GPU call), ``cut`` the component kernels on the tree's device."""

    def __init__(self, mst: MutualReachabilityMST):
        if not all(isinstance(getattr(mst, a, None), torch.Tensor) for a in ("edges", "weights", "core")):
            raise ValueError("ClusterTree takes what mutual_reachability_mst returns (edges, weights, core)")
        self.mst = mst
        self.n = int(mst.core.shape[0])
        self.device = mst.core.device
        self._edges = mst.edges.detach().cpu().numpy()
        self._weights = mst.weights.detach().cpu().numpy()
        self.condensed = None

    def labels(self, min_cluster_size: int = 5, method: str = "eom",
               allow_single_cluster: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """``labels`` int64 [N] (-1: noise) and ``prob`` float64 [N] on the tree's device; ``self.condensed`` then holds
        the condensed tree (parent, child, lambda, size) as numpy arrays."""
        lab, prob, self.condensed = _tree_host(self._edges, self._weights, self.n, min_cluster_size, method,
                                               allow_single_cluster)
        return torch.from_numpy(lab).to(self.device), torch.from_numpy(prob).to(self.device)

    def outlier_scores(self, min_cluster_size: int = 5) -> torch.Tensor:
        """GLOSH (Campello et al. 2015) of the fitted rows, float64 [N] on the tree's device: ``1 - lambda_row / death``
        with ``death`` the largest lambda at which any row leaves the subtree of the cluster the row fell out of -- 0 for
        the rows that stay to the end, towards 1 for a row that leaves long before; 0 where that ``death`` is 0, NaN for a
        non-finite row.  The score does not depend on which clusters are selected.  The host pass, no GPU call."""
        t = _model_host(self._edges, self._weights, self.n, min_cluster_size)
        return torch.from_numpy(t["outlier"]).to(self.device)

    def cut(self, eps: float, min_cluster_size: int = 1) -> torch.Tensor:
        """DBSCAN* at ``eps``: int64 [N], the components of the tree's edges with ``w <= eps`` among the rows with
        ``core <= eps``, numbered 0, 1, ... by their smallest row; components smaller than ``min_cluster_size`` and every
        other row are -1.  On ``dbscan(emb, eps, min_samples)``'s core rows these are its labels."""
        if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not eps >= 0:
            raise ValueError(f"eps must be a float >= 0, got {eps!r}")
        _check_int("min_cluster_size", min_cluster_size, 1)
        from .clusters import graph_components
        dev, n = self.device, self.n
        if dev.type != "cuda":
            raise RuntimeError(f"ClusterTree.cut runs on the GPU; there is no CPU fallback (the tree is on {dev})")
        with torch.cuda.device(dev):
            eps32 = torch.tensor(float(eps), dtype=torch.float32, device=dev)   # rounded to fp32 once
            keep = self.mst.weights <= eps32
            src, dst = self.mst.edges[keep, 0], self.mst.edges[keep, 1]
            order = torch.sort(src).indices
            indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            indptr[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
            mask = self.mst.core <= eps32
            root = graph_components(indptr, dst[order].contiguous(), mask)
            size = torch.bincount(root[mask], minlength=n)
            is_root = mask & (root == torch.arange(n, device=dev)) & (size >= min_cluster_size)
            number = torch.cumsum(is_root, 0, dtype=torch.int64) - 1
            ok = mask & is_root[root.clamp(min=0)]
            return torch.where(ok, number[root.clamp(min=0)], torch.full_like(root, -1))


def hdbscan(emb: torch.Tensor, min_cluster_size: int = 5, min_samples: Optional[int] = None, metric: str = "euclidean", *,
            cluster_selection_method: str = "eom", allow_single_cluster: bool = False,
            groups: Optional[torch.Tensor] = None, method: str = "tiles", search_k: int = 8, splits: int = 0,
            return_tree: bool = False):
    """``labels`` int64 [N] (-1: noise) and ``prob`` float64 [N], the membership strength, of the rows of ``emb`` [N, D]
    (see the module text).  min_samples: None = ``min_cluster_size``.  cluster_selection_method: ``"eom"`` or
    ``"leaf"``.  groups: int64 [N], an alert's object: densities are counted in other objects' alerts.  method:
    ``"tiles"`` or, for a 2-D map, ``"grid"``.  return_tree: also the ``ClusterTree``."""
    _check_selection(min_cluster_size, cluster_selection_method, allow_single_cluster)
    if min_samples is None:
        min_samples = min_cluster_size
    _check_mst_args(min_samples, search_k, splits, None)
    _metric(metric)
    _check_method(method)
    if isinstance(emb, (EmbeddingIndex, MapIndex)):
        raise ValueError("hdbscan takes rows; build the tree of an index with mutual_reachability_mst")
    mst = mutual_reachability_mst(emb, min_samples, groups, method, search_k, metric=metric, splits=splits)
    tree = ClusterTree(mst)
    labels, prob = tree.labels(min_cluster_size, cluster_selection_method, allow_single_cluster)
    return (labels, prob, tree) if return_tree else (labels, prob)


class ClusterModel:
    """The HDBSCAN fit of a bank, kept to assign new rows to its clusters (see the module text).

    bank_or_index: rows float [N, D] (an index is built on them, with ``groups``: an ``EmbeddingIndex``, or a ``MapIndex``
    with ``method="grid"``), an ``EmbeddingIndex`` or a ``MapIndex``.  An index brings its own metric and groups:
    ``groups=`` next to an index is a ``ValueError``.  The other arguments are ``hdbscan``'s; ``search_k`` and ``splits``
    are those of the fit's rounds.  ``labels`` int64, ``prob`` and ``outlier_scores`` float64 [N] are the fit -- ``labels``
    and ``prob`` are ``hdbscan``'s, ``outlier_scores`` is ``tree.outlier_scores(min_cluster_size)`` --, ``tree``, ``mst``
    and ``index`` what it was made of.  The tables ``predict`` walks live on the index's device.

    The fit does not follow ``index.add`` or ``index.remove``; ``refit()`` recomputes it, and ``predict`` refuses an index
    that has grown since or that rows were removed from (``index.generation``).  Calls on one model must be ordered by the caller's streams.  There is no CPU fallback."""

    def __init__(self, bank_or_index: Union[torch.Tensor, EmbeddingIndex, MapIndex], min_cluster_size: int = 5,
                 min_samples: Optional[int] = None, metric: str = "euclidean", *, cluster_selection_method: str = "eom",
                 allow_single_cluster: bool = False, groups: Optional[torch.Tensor] = None, method: str = "tiles",
                 search_k: int = 8, splits: int = 0):
        _check_selection(min_cluster_size, cluster_selection_method, allow_single_cluster)
        if min_samples is None:
            min_samples = min_cluster_size
        _check_mst_args(min_samples, search_k, splits, None)
        _check_method(method)
        self.index = _index_of(bank_or_index, groups, method, metric, "model")
        if isinstance(self.index, MapIndex) and splits:
            raise ValueError("a MapIndex has no splits")
        self.min_cluster_size, self.min_samples = min_cluster_size, min_samples
        self.cluster_selection_method, self.allow_single_cluster = cluster_selection_method, allow_single_cluster
        self.metric = getattr(self.index, "metric", "euclidean")
        self.search_k, self.splits = search_k, splits
        self.device = self.index.device
        self.refit()

    def __len__(self) -> int:
        """The rows the fit covers."""
        return int(self.labels.shape[0])

    def refit(self) -> "ClusterModel":
        """Fits the rows the index holds now (after ``index.add``): the spanning tree's rounds, the host pass, and the
        copy of its tables to the device."""
        dev = self.device
        self.mst = mutual_reachability_mst(self.index, self.min_samples, search_k=self.search_k, metric=self.metric,
                                           splits=self.splits)
        self.tree = ClusterTree(self.mst)
        self.labels, self.prob = self.tree.labels(self.min_cluster_size, self.cluster_selection_method,
                                                  self.allow_single_cluster)
        t = _model_host(self.tree._edges, self.tree._weights, self.tree.n, self.min_cluster_size,
                        self.cluster_selection_method, self.allow_single_cluster)
        self.lam_zero = t.pop("lam_zero")
        self.tables = {k: torch.from_numpy(v).to(dev) for k, v in t.items()}
        self.outlier_scores = self.tables["outlier"]
        self._bank_sq_max = None
        if isinstance(self.index, EmbeddingIndex) and self.metric == "euclidean":
            self._bank_sq_max = _sq_norms(self.index.bank).max()
        self._generation = getattr(self.index, "generation", 0)
        return self

    def _offer(self, idx: torch.Tensor, dist: torch.Tensor, q: torch.Tensor):
        """btsbot_cluster_offer_knn on the lists of the rows ``q``: (core_q, best_w, best_j, unresolved)"""
        nq, k, dev = int(idx.shape[0]), int(idx.shape[1]), self.device
        slack, squared, rel = _slack(self.index, q, self._bank_sq_max)
        core_q = torch.empty(nq, dtype=torch.float32, device=dev)
        best_w = torch.empty(nq, dtype=torch.float32, device=dev)
        best_j = torch.empty(nq, dtype=torch.int32, device=dev)
        unres = torch.empty(nq, dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().btsbot_cluster_offer_knn(_ptr(idx), _ptr(dist), nq, k, len(self), self.min_samples,
                                                       _ptr(self.mst.core), _ptr(slack), squared, rel, _ptr(core_q),
                                                       _ptr(best_w), _ptr(best_j), _ptr(unres), _stream(dev)),
                   "btsbot_cluster_offer_knn")
        return core_q, best_w, best_j, unres

    def _assign(self, best_w: torch.Tensor, best_j: torch.Tensor):
        """btsbot_cluster_assign: (labels, prob, outlier, lambda, cluster, neighbor) of the rows' neighbours"""
        nq, dev, t = int(best_w.shape[0]), self.device, self.tables
        labels, cluster, neighbor = (torch.empty(nq, dtype=torch.int64, device=dev) for _ in range(3))
        prob, outlier, lam = (torch.empty(nq, dtype=torch.float64, device=dev) for _ in range(3))
        _lib.check(_lib.lib().btsbot_cluster_assign(_ptr(best_w), _ptr(best_j), nq, len(self), _ptr(t["row_cluster"]),
                                                    _ptr(t["row_lambda"]), int(t["parent"].shape[0]), _ptr(t["parent"]),
                                                    _ptr(t["birth"]), _ptr(t["label"]), _ptr(t["max_lambda"]),
                                                    _ptr(t["death"]), self.lam_zero, _ptr(labels), _ptr(prob),
                                                    _ptr(outlier), _ptr(lam), _ptr(cluster), _ptr(neighbor), _stream(dev)),
                   "btsbot_cluster_assign")
        return labels, prob, outlier, lam, cluster, neighbor

    def predict(self, queries: torch.Tensor, query_groups: Optional[torch.Tensor] = None, exclude_same_group: bool = False,
                search_k: Optional[int] = None, stats: Optional[dict] = None, *, return_details: bool = False,
                splits: Optional[int] = None):
        """``labels`` int64 [Q] (-1: noise) and ``prob`` float64 [Q] of NEW rows ``queries`` [Q, D] against the fitted
        clusters; with ``return_details`` also a dict of ``neighbor`` int64 (the nearest mutual-reachability neighbour,
        -1 without one), ``lambda`` float64, ``outlier`` float64 (GLOSH) and ``cluster`` int64 (the condensed tree's
        cluster less N, -1 without one), [Q] each.  query_groups / exclude_same_group: as ``EmbeddingIndex.query`` --
        leave out the rows of the query's own object, from the row's density and from its neighbours.  search_k: the
        list length, 1..64; None = ``min(64, max(8, 2 * min_samples))``; the list holds ``max(search_k, min_samples - 1,
        1)`` rows and no answer depends on it.  splits: ``EmbeddingIndex.query``'s (None: the model's).  stats: a dict
        that receives ``unresolved`` (rows sent to the radius tier) and ``radius_total`` (entries of their lists).  One
        host read, the unresolved rows, and the radius search's own when there are any."""
        stale = _stale_fit(self.index, len(self), self._generation)
        if stale is not None:
            raise RuntimeError(stale + " -- call refit()")
        ms = self.min_samples
        if search_k is None:
            search_k = min(_lib.MST_MAX_K, max(8, 2 * ms))
        if splits is None:
            splits = self.splits
        _check_mst_args(ms, search_k, splits, stats)
        if not isinstance(return_details, bool):
            raise ValueError(f"return_details must be a bool, got {return_details!r}")
        index, dev, L = self.index, self.device, _lib.lib()
        grid = isinstance(index, MapIndex)
        if grid and splits:
            raise ValueError("a MapIndex has no splits")
        k = max(search_k, ms - 1, 1)
        skw = {} if grid else {"splits": splits}
        idx, dist = index.query(queries, k, query_groups=query_groups, exclude_same_group=exclude_same_group, **skw)
        nq, n = int(idx.shape[0]), len(self)
        with torch.cuda.device(dev):
            q = queries.detach().to(torch.float32).contiguous()
            core_q, best_w, best_j, unres = self._offer(idx, dist, q)
            todo = unres.nonzero().view(-1)                       # the host read: the rows of the radius tier
            total = 0
            if todo.numel():
                indptr, indices, rdist, total = _radius_tier(index, q, todo, best_w, query_groups, exclude_same_group, skw)
                _lib.check(L.btsbot_cluster_offer_csr(_ptr(indptr), _ptr(indices), _ptr(rdist), _ptr(todo),
                                                      int(todo.numel()), nq, n, _ptr(self.mst.core), _ptr(core_q),
                                                      _ptr(best_w), _ptr(best_j), _stream(dev)), "btsbot_cluster_offer_csr")
            labels, prob, outlier, lam, cluster, neighbor = self._assign(best_w, best_j)
        if stats is not None:
            stats.update(unresolved=int(todo.numel()), radius_total=int(total))
        if return_details:
            return labels, prob, {"neighbor": neighbor, "lambda": lam, "outlier": outlier, "cluster": cluster}
        return labels, prob
