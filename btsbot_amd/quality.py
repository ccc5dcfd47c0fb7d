"""How faithful is a 2-D map of embedding rows: trustworthiness, continuity and neighbour recall, on the device.

    t = trustworthiness(emb, y, n_neighbors=5)          # are a row's MAP neighbours near it in embedding space?
    c = continuity(emb, y, n_neighbors=5)               # are a row's EMBEDDING neighbours near it on the map?
    q = map_quality(emb, y, n_neighbors=15)             # both, the neighbour recall, n, k and the number of rows judged
    t = trustworthiness(emb, y, 15, rows=sample)        # a million-row map judged from a sample of its rows

Trustworthiness is sklearn's (``sklearn.manifold.trustworthiness``): with the k nearest map neighbours of each row i
(the row itself excluded) and r(i, j) the 0-based rank of row j among the others in embedding space,

    T = 1 - 2 / (m k (2 n - 3 k - 1)) * sum_i sum_j max(0, r(i, j) + 1 - k)

over the m judged rows.  Continuity swaps the roles of the two spaces.  Nothing of size n x n is formed: the neighbours
come from ``MapIndex.query`` / ``EmbeddingIndex.query`` and the ranks from ``EmbeddingIndex.rank_of`` (DESIGN.md section
4r), which has no cap on the rank -- a bad map is exactly the one whose map neighbours stand at ranks near n / 2.  Ranks
and neighbours are ordered by (direct-form fp32 distance, row index), so ties are broken by the row number in both
spaces.  The penalties are summed as int64 on the device; the formula is evaluated once in Python float64.

``rows``: int64 row numbers to judge (m = their number; the default is every row); their neighbours and ranks are still
among all n rows.  ``groups``: int64 [n], the rows' objects; neighbours and ranks are then among rows of OTHER groups on
both sides, as ``embedding_layout(groups=...)`` builds its map.  Rows that hold a non-finite value in ``emb`` or on the
map are left out of n, of m and of every neighbour list.  ``ValueError`` unless ``n_neighbors < n / 2``.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .neighbors import METRICS, EmbeddingIndex, _check_method, _groups, _rows

__all__ = ["trustworthiness", "continuity", "map_quality"]


def _check_k(k, n=None) -> None:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.KNN_MAX_K:
        raise ValueError(f"n_neighbors must be an int in 1..{_lib.KNN_MAX_K}, got {k!r}")
    if n is not None and not k < n / 2:
        raise ValueError(f"n_neighbors = {k} must be less than n / 2 = {n / 2} (n = {n} finite rows)")


def _inputs(emb, y, k, metric, rows, groups):
    """(emb [n, D], y [n, 2], rows int64 [m], groups or None) over the finite rows, renumbered 0..n-1; the checks that
    need no device come first."""
    _check_k(k)
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    if isinstance(emb, torch.Tensor) and emb.dim() == 2:
        _check_k(k, int(emb.shape[0]))
    if rows is not None and (not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.dim() != 1):
        raise ValueError("rows must be None or an int64 tensor [m] of row numbers")
    if rows is not None and groups is None and k + 1 > _lib.KNN_MAX_K:
        raise ValueError(f"with rows= the row itself takes one neighbour slot: n_neighbors <= {_lib.KNN_MAX_K - 1}")
    e = _rows(emb, "emb")
    p = _rows(y, "y", e.device)
    if p.shape[1] != 2 or p.shape[0] != e.shape[0]:
        raise ValueError(f"y must be [{e.shape[0]}, 2], the map positions of emb's rows, got {tuple(p.shape)}")
    n_all = int(e.shape[0])
    if groups is not None:
        groups = _groups(groups, "groups", n_all, e.device)
    if rows is not None:
        if rows.device != e.device:
            raise ValueError(f"rows is on {rows.device}, emb on {e.device}")
        if rows.numel() and not bool(((rows >= 0) & (rows < n_all)).all()):
            raise ValueError(f"rows must lie in 0..{n_all - 1}")
    ok = torch.isfinite(e).all(dim=1) & torch.isfinite((e * e).sum(dim=1)) & torch.isfinite(p).all(dim=1) & \
        torch.isfinite((p * p).sum(dim=1))
    keep = ok.nonzero().view(-1)
    sampled = rows is not None
    if int(keep.shape[0]) != n_all:
        new = torch.cumsum(ok, 0, dtype=torch.int64) - 1
        e, p = e[keep].contiguous(), p[keep].contiguous()
        groups = None if groups is None else groups[keep].contiguous()
        if sampled:
            rows = new[rows[ok[rows]]]
    n = int(e.shape[0])
    _check_k(k, n)
    return e, p, (rows.contiguous() if sampled else None), groups


def _kw(index_groups, rows):
    if index_groups is None:
        return {}
    return dict(query_groups=index_groups if rows is None else index_groups[rows], exclude_same_group=True)


def _neighbors(index, pts, rows, k, groups):
    """int64 [m, k]: the k nearest OTHER rows (of other groups, with groups) of the judged rows in ``index``, by
    (dist, index); -1 where fewer exist."""
    q = pts if rows is None else pts[rows]
    kw = _kw(groups, rows)
    if groups is not None:
        return index.query(q, k, **kw)[0]
    if rows is None:
        return index.query(q, k, self_offset=0)[0]
    # a sample: the row itself is masked by value of its number, not by position -- ask for one more and drop it (if
    # k + 1 duplicates of lower number crowd it out, the first k are the answer as they stand)
    idx = index.query(q, k + 1)[0]
    own = idx == rows[:, None]
    pos = torch.where(own.any(dim=1), own.to(torch.int64).argmax(dim=1), torch.full_like(rows, k))
    cols = torch.arange(k, device=idx.device)[None, :]
    return torch.gather(idx, 1, cols + (cols >= pos[:, None]).to(torch.int64))


def _before(d1, i1, d2, i2):
    return (d1 < d2) | ((d1 == d2) & (i1 < i2))


def _ranks(index, pts, rows, targets, groups):
    """int64 [m, t]: ``rank_of`` of ``targets`` among the OTHER rows (of other groups) for the judged rows; -1 stays"""
    q = pts if rows is None else pts[rows]
    kw = _kw(groups, rows)
    if groups is not None:
        return index.rank_of(q, targets, **kw)[0]
    if rows is None:
        return index.rank_of(q, targets, self_offset=0)[0]
    # a sample: the row itself is a bank row like any other; it joins the targets, which gives its own distance (0, or
    # what 1 - cos of a row with itself rounds to), and leaves every rank it is before
    t = int(targets.shape[1])
    both = torch.cat([targets, rows[:, None]], dim=1)
    rank = torch.empty_like(both)
    dist = torch.empty(both.shape, dtype=torch.float32, device=both.device)
    for c0 in range(0, t + 1, _lib.KNN_MAX_K):
        rank[:, c0:c0 + _lib.KNN_MAX_K], dist[:, c0:c0 + _lib.KNN_MAX_K] = \
            index.rank_of(q, both[:, c0:c0 + _lib.KNN_MAX_K].contiguous())
    own = _before(dist[:, t:], rows[:, None], dist[:, :t], targets) & (targets != rows[:, None])
    return torch.where(rank[:, :t] >= 0, rank[:, :t] - own.to(torch.int64), rank[:, :t])


def _penalty(rank, k):
    """int64 [m]: sum over the columns of max(0, rank + 1 - k); a column without a rank (-1) adds nothing"""
    return (rank + 1 - k).clamp(min=0).sum(dim=1)


def _score(pen_sum: int, m: int, n: int, k: int) -> float:
    if m == 0:
        return float("nan")
    return 1.0 - 2.0 / (float(m) * k * (2.0 * n - 3.0 * k - 1.0)) * float(pen_sum)


def _map_index(p, groups, method):
    if method == "grid":
        from .mapindex import MapIndex
        return MapIndex(p, groups=groups)
    return EmbeddingIndex(p, groups=groups)


def trustworthiness(emb: torch.Tensor, y: torch.Tensor, n_neighbors: int = 5, *, metric: str = "euclidean",
                    rows: Optional[torch.Tensor] = None, groups: Optional[torch.Tensor] = None, method: str = "grid",
                    return_rows: bool = False):
    """sklearn's trustworthiness of the map ``y`` [N, 2] of ``emb`` [N, D] as a Python float (see the module text).
    method: where the map neighbours come from, ``"grid"`` (``MapIndex``) or ``"tiles"`` (``EmbeddingIndex`` at D = 2);
    the value is the same.  return_rows=True: (T, the judged rows' penalties, int64 [m])."""
    _check_method(method)
    e, p, rows, groups = _inputs(emb, y, n_neighbors, metric, rows, groups)
    k, n = n_neighbors, int(e.shape[0])
    nb = _neighbors(_map_index(p, groups, method), p, rows, k, groups)
    pen = _penalty(_ranks(EmbeddingIndex(e, metric, groups=groups), e, rows, nb, groups), k)
    t = _score(int(pen.sum()), int(pen.shape[0]), n, k)
    return (t, pen) if return_rows else t


def continuity(emb: torch.Tensor, y: torch.Tensor, n_neighbors: int = 5, *, metric: str = "euclidean",
               rows: Optional[torch.Tensor] = None, groups: Optional[torch.Tensor] = None, return_rows: bool = False):
    """Continuity: trustworthiness with the two spaces swapped -- the embedding-space neighbours' ranks on the map,
    from an ``EmbeddingIndex`` over ``y``."""
    e, p, rows, groups = _inputs(emb, y, n_neighbors, metric, rows, groups)
    k, n = n_neighbors, int(e.shape[0])
    nb = _neighbors(EmbeddingIndex(e, metric, groups=groups), e, rows, k, groups)
    pen = _penalty(_ranks(EmbeddingIndex(p, groups=groups), p, rows, nb, groups), k)
    c = _score(int(pen.sum()), int(pen.shape[0]), n, k)
    return (c, pen) if return_rows else c


def map_quality(emb: torch.Tensor, y: torch.Tensor, n_neighbors: int = 15, *, metric: str = "euclidean",
                rows: Optional[torch.Tensor] = None, groups: Optional[torch.Tensor] = None, method: str = "grid") -> dict:
    """``{"trustworthiness", "continuity", "neighbor_recall", "n", "k", "rows"}``: both figures from one set of
    neighbour lists, and the mean share of a row's k embedding neighbours that are among its k map neighbours."""
    _check_method(method)
    e, p, rows, groups = _inputs(emb, y, n_neighbors, metric, rows, groups)
    k, n = n_neighbors, int(e.shape[0])
    hi = EmbeddingIndex(e, metric, groups=groups)
    nb_map = _neighbors(_map_index(p, groups, method), p, rows, k, groups)
    nb_emb = _neighbors(hi, e, rows, k, groups)
    pen_t = _penalty(_ranks(hi, e, rows, nb_map, groups), k)
    pen_c = _penalty(_ranks(EmbeddingIndex(p, groups=groups), p, rows, nb_emb, groups), k)
    m = int(pen_t.shape[0])
    shared = torch.zeros((), dtype=torch.int64, device=e.device)
    for r0 in range(0, m, 1 << 16):
        a, b = nb_emb[r0:r0 + (1 << 16)], nb_map[r0:r0 + (1 << 16)]
        shared += ((a[:, :, None] == b[:, None, :]) & (a[:, :, None] >= 0)).any(dim=2).sum()
    sums = torch.stack([pen_t.sum(), pen_c.sum(), shared]).tolist()
    return {"trustworthiness": _score(sums[0], m, n, k), "continuity": _score(sums[1], m, n, k),
            "neighbor_recall": sums[2] / (m * k) if m else float("nan"), "n": n, "k": k, "rows": m}
