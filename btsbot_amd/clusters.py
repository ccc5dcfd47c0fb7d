"""The clumps of an embedding or of its map: connected components and DBSCAN, on the device.

    root = graph_components(indptr, indices, mask=None)          # int64 [N]: the smallest row of the row's component
    labels, core = dbscan(emb, eps, min_samples=5)               # int64 [N] (-1: noise), bool [N]

``dbscan`` follows ``sklearn.cluster.DBSCAN`` and reproduces its ``labels_`` exactly (tests/radius_ref.py):

* the graph is ``radius_graph(emb, eps, include_self=True)``: a row counts itself;
* ``core = count >= min_samples``;
* the clusters are the connected components of the core-core edges, numbered 0, 1, ... in the order of their smallest
  core row;
* a non-core row with core rows within ``eps`` takes the smallest label among them; every other non-core row is -1.

With ``groups=obj`` (one int64 per row, an alert's object) a row's density is the number of DISTINCT groups among the
rows within ``eps`` -- otherwise one object with fifty epochs is a cluster of its own --; everything else is unchanged.
A non-finite row has no neighbours, not even itself: label -1, not core.  The components and the labelling are HIP
kernels (csrc/components.hip); counting and numbering are torch operations on the same device.
``method="grid"`` takes the graph of a 2-D map from ``mapindex.MapIndex`` (section 4q): the same graph, the same labels.
There is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .mapindex import check_grid_method
from ._lib import ptr as _ptr, stream as _stream
from .neighbors import _check_method, _groups, _metric, _rows, radius_graph


def _csr(indptr, indices, n: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, int]:
    for name, t in (("indptr", indptr), ("indices", indices)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1:
            raise ValueError(f"{name} must be a 1-D int64 torch.Tensor, got "
                             f"{(t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if indptr.shape[0] < 1 or (n is not None and indptr.shape[0] != n + 1):
        raise ValueError(f"indptr must hold N + 1 entries{'' if n is None else f' = {n + 1}'}, got {indptr.shape[0]}")
    if indptr.device.type != "cuda":
        raise RuntimeError(f"btsbot_amd.clusters runs on the GPU; there is no CPU fallback (indptr is on {indptr.device})")
    if indices.device != indptr.device:
        raise ValueError(f"indices is on {indices.device}, indptr on {indptr.device}")
    return indptr.contiguous(), indices.contiguous(), int(indptr.shape[0]) - 1


def graph_components(indptr: torch.Tensor, indices: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``root`` int64 [N]: the smallest row index of the row's connected component in the CSR graph (``indptr`` int64
    [N + 1], ``indices`` int64 with values in [0, N)), restricted to the rows and edges whose both ends pass ``mask``
    (bool [N]; None: every row); -1 where the mask is False.  An edge in either direction joins.  The result is a
    function of the graph alone.  Three launches on the current stream, no host read."""
    indptr, indices, n = _csr(indptr, indices)
    dev = indptr.device
    if n >= 1 << 31:
        raise ValueError(f"at most 2^31 - 1 rows, got {n}")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.shape != (n,) or mask.device != dev:
            raise ValueError(f"mask must be a bool tensor [{n}] on {dev}")
        mask = mask.contiguous().view(torch.uint8)
    root = torch.empty(n, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        parent = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().btsbot_graph_components(_ptr(indptr), _ptr(indices), _ptr(mask), n, _ptr(parent),
                                                      _ptr(root), _stream(dev)), "btsbot_graph_components")
    return root


def dbscan(emb: torch.Tensor, eps: float, min_samples: int = 5, metric: str = "euclidean", *,
           groups: Optional[torch.Tensor] = None,
           graph: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
           method: str = "tiles") -> Tuple[torch.Tensor, torch.Tensor]:
    """``labels`` int64 [N] (-1: noise) and ``core`` bool [N] of the rows of ``emb`` [N, D]: sklearn's DBSCAN (see the
    module text).  groups: int64 [N]; a row's density is then the number of distinct groups within ``eps``.
    graph: ``(indptr, indices)`` of ``radius_graph(emb, eps, include_self=True)``, to reuse one.
    method: ``radius_graph``'s, ``"tiles"`` or, for a 2-D map, ``"grid"``: the same graph, hence the same labels."""
    _metric(metric)
    _check_method(method)
    if method == "grid":
        check_grid_method(int(emb.shape[1]) if isinstance(emb, torch.Tensor) and emb.dim() == 2 else None, metric)
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not eps >= 0:
        raise ValueError(f"eps must be a float >= 0, got {eps!r}")
    if isinstance(min_samples, bool) or not isinstance(min_samples, int) or min_samples < 1:
        raise ValueError(f"min_samples must be an int >= 1, got {min_samples!r}")
    rows = _rows(emb, "emb")
    n, dev = int(rows.shape[0]), rows.device
    if groups is not None:
        groups = _groups(groups, "groups", n, dev)
    if graph is None:
        indptr, indices, _dist = radius_graph(rows, float(eps), include_self=True, metric=metric, method=method)
    else:
        indptr, indices, _n = _csr(graph[0], graph[1], n)
        if indptr.device != dev:
            raise ValueError(f"graph is on {indptr.device}, emb on {dev}")
    with torch.cuda.device(dev):
        if groups is None:
            count = indptr.diff()
        else:   # distinct (row, group) pairs: the groups as dense ids, one key per pair
            gid = torch.unique(groups, return_inverse=True)[1]
            at = torch.repeat_interleave(torch.arange(n, device=dev), indptr.diff(), output_size=int(indices.shape[0]))
            pairs = torch.unique(at * max(n, 1) + gid[indices])
            count = torch.bincount(pairs // max(n, 1), minlength=n)
        core = count >= min_samples
        root = graph_components(indptr, indices, core)
        is_root = core & (root == torch.arange(n, device=dev))
        cluster = torch.cumsum(is_root, 0, dtype=torch.int64) - 1        # read at the roots only
        labels = torch.empty(n, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().btsbot_dbscan_labels(_ptr(indptr), _ptr(indices), _ptr(core.view(torch.uint8)), _ptr(root),
                                                   _ptr(cluster), n, _ptr(labels), _stream(dev)), "btsbot_dbscan_labels")
    return labels, core
