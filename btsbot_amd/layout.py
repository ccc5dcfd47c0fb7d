"""Map of the embeddings: a deterministic UMAP layout of embedding rows, on the device.

The reference ends a run by embedding the test split and laying the rows out with UMAP (train.py:449-469, the columns
``umap_emb_1, umap_emb_2`` of its CSV).  This module is that last step, from the exact neighbour graph of
``knn_graph`` to ``[N, 2]`` coordinates (csrc/layout.hip):

    y = embedding_layout(emb)                                   # float32 [N, 2]
    idx, dist = knn_graph(emb, 15, include_self=True)
    g = fuzzy_graph(idx, dist)                                  # symmetric CSR graph, sigma, rho
    a, b = find_ab_params(1.0, 0.1)
    y = optimize_layout(g, y0, 200, a, b, seed=0)               # or epochs first_epoch..last_epoch of the schedule

The epochs are a Jacobi form of umap-learn's ``optimize_layout_euclidean``: every epoch reads the previous positions
and writes new ones, a vertex is moved by its own lanes only and negative samples come from a counter hash, so the same
input gives the same map bit for bit, whatever the grid or the run -- which also means the result is not umap-learn's
(whose sequential, racy updates cannot be reproduced).  Nothing synchronises with the host except the one read of the
D x D covariance ``init="pca"`` needs; the work is queued on the current stream.  There is no CPU fallback.

New rows are placed on a map that stays fixed (umap-learn's ``transform``):

    m = EmbeddingMap(bank)                                      # index + embedding_layout; or .from_positions(bank, y)
    y_new = m.transform(queries)                                # float32 [Q, 2]; m.extend(rows) also adds them
    idx, dist = index.query(queries, 15)
    w, sigma = query_memberships(idx, dist)
    y_new = layout_transform(idx, dist, bank_y, 100, a=a, b=b)  # every epoch of the schedule in one launch
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream

_U64 = (1 << 64) - 1


def _int(v, name: str, lo: int, hi: Optional[int] = None) -> int:
    if not isinstance(v, int) or isinstance(v, bool) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{name} must be an int in {lo}..{'' if hi is None else hi}, got {v!r}")
    return v


def _on_gpu(t: torch.Tensor, name: str, device=None) -> None:
    if t.device.type != "cuda":
        raise RuntimeError(f"btsbot_amd.layout runs on the GPU; there is no CPU fallback ({name} is on {t.device})")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")


def find_ab_params(spread: float = 1.0, min_dist: float = 0.1) -> Tuple[float, float]:
    """umap-learn's ``find_ab_params``: the (a, b) for which 1 / (1 + a x^(2b)) is the least-squares fit, on 300 points
    of [0, 3 spread], of the curve that is 1 up to ``min_dist`` and exp(-(x - min_dist) / spread) beyond.  A
    Levenberg-Marquardt iteration from (1, 1) in numpy (what scipy's ``curve_fit`` runs there)."""
    spread, min_dist = float(spread), float(min_dist)
    if not (spread > 0 and 0 <= min_dist < 3 * spread):
        raise ValueError(f"need spread > 0 and 0 <= min_dist < 3 spread, got spread={spread!r} min_dist={min_dist!r}")
    x = np.linspace(0.0, 3.0 * spread, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    x, y = x[1:], y[1:]                       # x = 0 fits exactly whatever (a, b) and has no finite log
    lx = 2.0 * np.log(x)

    def resid(p):
        return 1.0 / (1.0 + p[0] * np.exp(p[1] * lx)) - y

    p = np.array([1.0, 1.0])
    r = resid(p)
    lam = 1e-3
    for _ in range(200):
        t = np.exp(p[1] * lx)
        f2 = (1.0 + p[0] * t) ** -2
        J = np.stack([-t * f2, -p[0] * t * lx * f2], axis=1)
        A, g = J.T @ J, J.T @ r
        step = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
        q = p + step
        rq = resid(q) if q[0] > 0 else None
        if rq is not None and rq @ rq <= r @ r:
            done = np.abs(step).max() < 1e-12
            p, r, lam = q, rq, lam * 0.3
            if done:
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return float(p[0]), float(p[1])


class FuzzyGraph:
    """umap's fuzzy simplicial set of a kNN graph as a symmetric CSR matrix on the device.

    ``indptr`` int64 [N + 1]; ``indices`` int32 [E] (columns ascending inside a row) and ``weights`` float32 [E], where
    ``weights[i -> j] == weights[j -> i]`` bit for bit; ``sigma``, ``rho`` float32 [N]; ``w_max`` float32 [1].
    ``indices`` and ``weights`` are views of buffers sized for the worst case; reading them (or ``n_edges``) is what
    fetches E from the device -- ``optimize_layout`` does not."""

    def __init__(self, indptr, indices, weights, w_max, sigma, rho):
        self.indptr, self._indices, self._weights, self.w_max, self.sigma, self.rho = indptr, indices, weights, w_max, sigma, rho
        self._e = None

    @property
    def n(self) -> int:
        return int(self.indptr.shape[0]) - 1

    @property
    def n_edges(self) -> int:
        if self._e is None:
            self._e = int(self.indptr[-1])
        return self._e

    @property
    def indices(self) -> torch.Tensor:
        return self._indices[:self.n_edges]

    @property
    def weights(self) -> torch.Tensor:
        return self._weights[:self.n_edges]


def _check_knn(idx, dist) -> Tuple[int, int]:
    for t, name in ((idx, "idx"), (dist, "dist")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if idx.dtype != torch.int64 or dist.dtype != torch.float32:
        raise ValueError(f"idx must be int64 and dist float32 (knn_graph's outputs), got {idx.dtype} and {dist.dtype}")
    if idx.dim() != 2 or idx.shape != dist.shape:
        raise ValueError(f"idx and dist must both be [N, k], got {tuple(idx.shape)} and {tuple(dist.shape)}")
    n, k = int(idx.shape[0]), int(idx.shape[1])
    if not 2 <= k <= _lib.LAYOUT_MAX_K:
        raise ValueError(f"k (columns, the row itself included) must be in 2..{_lib.LAYOUT_MAX_K}, got {k}")
    if 2 * n * k >= 1 << 31:
        raise ValueError(f"2 N k must stay below 2^31, got N = {n}, k = {k}")
    _on_gpu(idx, "idx")
    _on_gpu(dist, "dist", idx.device)
    return n, k


def fuzzy_graph(idx: torch.Tensor, dist: torch.Tensor) -> FuzzyGraph:
    """The fuzzy graph of ``knn_graph(emb, k, include_self=True)``'s ``idx`` int64 [N, k] and ``dist`` float32 [N, k]
    (2 <= k <= 64, column 0 the row itself): umap-learn's ``smooth_knn_dist`` (local_connectivity 1, the bisection in
    float64) and the probabilistic union ``w = (a + b) - a b``.  Entries with ``idx = -1`` are dropped."""
    n, k = _check_knn(idx, dist)
    dev = idx.device
    idx, dist = idx.contiguous(), dist.contiguous()
    L = _lib.lib()
    with torch.cuda.device(dev):
        present = idx >= 0
        mean_all = (torch.where(present, dist, torch.zeros_like(dist)).double().sum()
                    / present.sum().clamp(min=1).double()).reshape(1)
        sigma = torch.empty(n, dtype=torch.float32, device=dev)
        rho = torch.empty(n, dtype=torch.float32, device=dev)
        memb = torch.empty((n, k), dtype=torch.float32, device=dev)
        cap = max(2 * n * (k - 1), 1)
        indptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        indices = torch.empty(cap, dtype=torch.int32, device=dev)
        weights = torch.empty(cap, dtype=torch.float32, device=dev)
        w_max = torch.empty(1, dtype=torch.float32, device=dev)
        _lib.check(L.btsbot_layout_smooth_knn(_ptr(idx), _ptr(dist), n, k, _ptr(mean_all), _ptr(sigma), _ptr(rho),
                                              _ptr(memb), _stream(dev)), "btsbot_layout_smooth_knn")
        need = int(L.btsbot_layout_symmetrize_workspace(n, k))
        if need < 0:
            _lib.check(need, "btsbot_layout_symmetrize_workspace")
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        _lib.check(L.btsbot_layout_symmetrize(_ptr(idx), _ptr(memb), n, k, _ptr(indptr), _ptr(indices), _ptr(weights),
                                              _ptr(w_max), _ptr(ws), need, _stream(dev)), "btsbot_layout_symmetrize")
    return FuzzyGraph(indptr, indices, weights, w_max, sigma, rho)


def _check_epoch_args(n_epochs, seed, negative_sample_rate, learning_rate, first_epoch, last_epoch) -> int:
    _int(n_epochs, "n_epochs", 1, (1 << 31) - 1)
    _int(negative_sample_rate, "negative_sample_rate", 0, _lib.LAYOUT_MAX_NEGATIVES)
    if not isinstance(seed, int) or isinstance(seed, bool):
        raise ValueError(f"seed must be an int, got {seed!r}")
    if not float(learning_rate) > 0:
        raise ValueError(f"learning_rate must be positive, got {learning_rate!r}")
    last = n_epochs if last_epoch is None else last_epoch
    _int(first_epoch, "first_epoch", 1, n_epochs)
    _int(last, "last_epoch", 1, n_epochs)
    if first_epoch > last:
        raise ValueError(f"first_epoch ({first_epoch}) is past last_epoch ({last})")
    return last


def optimize_layout(g: FuzzyGraph, y0: torch.Tensor, n_epochs: int, a: float, b: float, *, seed: int = 0,
                    negative_sample_rate: int = 5, learning_rate: float = 1.0, first_epoch: int = 1,
                    last_epoch: Optional[int] = None, blocks: int = 0) -> torch.Tensor:
    """Epochs ``first_epoch..last_epoch`` (default: all) of an ``n_epochs`` schedule from the positions ``y0`` float32
    [N, 2] (not modified); returns the new positions.  Stepping the schedule in several calls gives, bit for bit, what
    one call gives; so does any ``blocks`` (the grid size; 0: the library's choice)."""
    if not isinstance(g, FuzzyGraph):
        raise TypeError(f"g must be a FuzzyGraph (fuzzy_graph's result), got {type(g).__name__}")
    last = _check_epoch_args(n_epochs, seed, negative_sample_rate, learning_rate, first_epoch, last_epoch)
    _int(blocks, "blocks", 0, (1 << 31) - 1)
    if not (float(a) > 0 and float(b) > 0):
        raise ValueError(f"a and b must be positive, got a={a!r} b={b!r}")
    if not isinstance(y0, torch.Tensor):
        raise TypeError(f"y0 must be a torch.Tensor, got {type(y0).__name__}")
    if y0.dtype != torch.float32 or y0.dim() != 2 or tuple(y0.shape) != (g.n, 2):
        raise ValueError(f"y0 must be float32 [{g.n}, 2], got {y0.dtype} {tuple(y0.shape)}")
    _on_gpu(y0, "y0")
    _on_gpu(g.indptr, "the graph", y0.device)
    dev = y0.device
    with torch.cuda.device(dev):
        ya = y0.detach().clone(memory_format=torch.contiguous_format)
        yb = torch.empty_like(ya)
        _lib.check(_lib.lib().btsbot_layout_epochs(_ptr(g.indptr), _ptr(g._indices), _ptr(g._weights), _ptr(g.w_max), g.n,
                                                   _ptr(ya), _ptr(yb), n_epochs, first_epoch, last, float(a), float(b),
                                                   seed & _U64, negative_sample_rate, float(learning_rate), blocks,
                                                   _stream(dev)), "btsbot_layout_epochs")
    return yb if (last - first_epoch + 1) % 2 else ya


def _hash_init(y: torch.Tensor, seed: int, mode: int) -> torch.Tensor:
    _lib.check(_lib.lib().btsbot_layout_init(_ptr(y), int(y.shape[0]), seed & _U64, mode, _stream(y.device)),
               "btsbot_layout_init")
    return y


def pca_directions(cov: np.ndarray) -> np.ndarray:
    """The two leading eigenvectors of a covariance [D, D] as float64 [D, 2], each signed so that its largest-magnitude
    loading is positive (a second column of zeros when D = 1)."""
    cov = np.asarray(cov, dtype=np.float64)
    _w, vec = np.linalg.eigh((cov + cov.T) / 2)
    comps = vec[:, ::-1][:, :2]
    if comps.shape[1] < 2:
        comps = np.concatenate([comps, np.zeros((comps.shape[0], 2 - comps.shape[1]))], axis=1)
    comps = comps.copy()
    for c in range(2):
        j = int(np.argmax(np.abs(comps[:, c])))
        if comps[j, c] < 0:
            comps[:, c] = -comps[:, c]
    return comps


def _initial_positions(rows: torch.Tensor, finite: torch.Tensor, init, seed: int) -> torch.Tensor:
    n, dev = int(rows.shape[0]), rows.device
    if isinstance(init, torch.Tensor):
        if init.dtype != torch.float32 or tuple(init.shape) != (n, 2):
            raise ValueError(f"init must be float32 [{n}, 2], got {init.dtype} {tuple(init.shape)}")
        _on_gpu(init, "init", dev)
        return init.detach().clone(memory_format=torch.contiguous_format)
    nan = torch.full((), float("nan"), device=dev)
    if init == "random":
        y = _hash_init(torch.empty((n, 2), dtype=torch.float32, device=dev), seed, 0)
        return torch.where(finite[:, None], y, nan)
    keep = finite[:, None]
    cnt = finite.sum().clamp(min=1).to(torch.float32)
    x = torch.where(keep, rows, torch.zeros_like(rows))
    xc = torch.where(keep, x - x.sum(dim=0) / cnt, torch.zeros_like(rows))
    cov = (xc.t() @ xc) / cnt
    comps = pca_directions(cov.cpu().numpy())                     # the one host read
    proj = xc @ torch.from_numpy(comps).to(device=dev, dtype=torch.float32)
    top = proj.abs().max().clamp(min=torch.finfo(torch.float32).tiny) if n else proj.new_ones(())
    y = _hash_init((proj * (10.0 / top)).contiguous(), seed, 1)
    return torch.where(keep, y, nan)


def embedding_layout(emb: torch.Tensor, n_neighbors: int = 15, min_dist: float = 0.1, spread: float = 1.0,
                     n_epochs: Optional[int] = None, init="pca", seed: int = 0, metric: str = "euclidean",
                     negative_sample_rate: int = 5, learning_rate: float = 1.0,
                     knn: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, *,
                     groups: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The 2-D UMAP map of the rows of ``emb`` [N, D]: ``knn_graph`` (``n_neighbors`` columns, the row itself included,
    as umap-learn counts them) -> ``fuzzy_graph`` -> initial positions -> ``optimize_layout``; float32 [N, 2].

    n_epochs=None: 500 for N <= 10,000 and 200 otherwise, as umap-learn.  init: "pca" (the two leading principal
    directions scaled to max |y| = 10 plus a jitter of 1e-4), "random" (uniform in [-10, 10)) or a float32 [N, 2]
    tensor.  knn=(idx, dist): a neighbour graph already made (``knn_graph(emb, n_neighbors, include_self=True)``).  A
    row that holds a non-finite value has no edges and a NaN position.  groups: int64 [N], the rows' objects: the graph
    is ``knn_graph(emb, n_neighbors, groups=groups, group_mode="exclude")`` -- the row itself, then rows of OTHER
    objects --, so the map is no picture of object identity (not together with ``knn``)."""
    from .neighbors import METRICS, _rows, knn_graph
    _int(n_neighbors, "n_neighbors", 2, _lib.LAYOUT_MAX_K)
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    if not (isinstance(init, torch.Tensor) or init in ("pca", "random")):
        raise ValueError(f"init must be 'pca', 'random' or a float32 [N, 2] tensor, got {init!r}")
    if n_epochs is not None:
        _int(n_epochs, "n_epochs", 1, (1 << 31) - 1)
    a, b = find_ab_params(spread, min_dist)
    if knn is not None and not (isinstance(knn, (tuple, list)) and len(knn) == 2):
        raise ValueError("knn must be the pair (idx, dist) of knn_graph(emb, n_neighbors, include_self=True)")
    if knn is not None and groups is not None:
        raise ValueError("groups shape the neighbour graph: give them to knn_graph(..., groups=...), not beside knn=")
    rows = _rows(emb, "emb")
    n = int(rows.shape[0])
    epochs = n_epochs if n_epochs is not None else (500 if n <= 10000 else 200)
    _check_epoch_args(epochs, seed, negative_sample_rate, learning_rate, 1, None)
    with torch.cuda.device(rows.device):
        if knn is None:
            knn = knn_graph(rows, n_neighbors, include_self=True, metric=metric, groups=groups, group_mode="exclude")
        elif isinstance(knn[0], torch.Tensor) and knn[0].shape[0] != n:
            raise ValueError(f"knn has {knn[0].shape[0]} rows, emb {n}")
        g = fuzzy_graph(*knn)
        y0 = _initial_positions(rows, torch.isfinite(rows).all(dim=1), init, seed)
        if n == 0:
            return y0
        return optimize_layout(g, y0, epochs, a, b, seed=seed, negative_sample_rate=negative_sample_rate,
                               learning_rate=learning_rate)


# ---- new rows on an existing map
def query_memberships(idx: torch.Tensor, dist: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The memberships of ``EmbeddingIndex.query(queries, k)``'s ``idx`` int64 [Q, k] and ``dist`` float32 [Q, k] (2 <= k
    <= 64; rows that are NOT in the bank, so there is no self column): umap-learn's ``smooth_knn_dist`` as its
    ``transform`` calls it (``rho = 0``), ``w = exp(-d / sigma)``; 0 where ``idx = -1``.  Returns ``(w [Q, k], sigma
    [Q])``, float32.  A row's result depends on that row alone."""
    n, k = _check_knn(idx, dist)
    dev = idx.device
    idx, dist = idx.contiguous(), dist.contiguous()
    with torch.cuda.device(dev):
        sigma = torch.empty(n, dtype=torch.float32, device=dev)
        w = torch.empty((n, k), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().btsbot_layout_smooth_knn_query(_ptr(idx), _ptr(dist), n, k, _ptr(sigma), _ptr(w), _stream(dev)),
                   "btsbot_layout_smooth_knn_query")
    return w, sigma


def _positions(t, name: str, rows: Optional[int], dev) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 2 or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"{name} must be float32 [{'N' if rows is None else rows}, 2], got {t.dtype} {tuple(t.shape)}")
    _on_gpu(t, name, dev)
    return t.detach().contiguous()


def layout_transform(idx: torch.Tensor, dist: torch.Tensor, bank_y: torch.Tensor, n_epochs: int = 100, *, a: float,
                     b: float, seed: int = 0, negative_sample_rate: int = 5, learning_rate: float = 1.0,
                     y0: Optional[torch.Tensor] = None, first_epoch: int = 1, last_epoch: Optional[int] = None,
                     blocks: int = 0) -> torch.Tensor:
    """Positions float32 [Q, 2] of Q new rows on the map ``bank_y`` float32 [N, 2], which stays fixed: umap-learn's
    ``transform``.  ``idx``, ``dist``: the rows' neighbours in the bank (``EmbeddingIndex.query``).  A row starts at the
    mean of its neighbours' positions weighted by ``query_memberships`` and runs epochs ``first_epoch..last_epoch``
    (default: all) of an ``n_epochs`` schedule at a quarter of ``learning_rate``, the whole schedule in one launch.  With
    ``y0`` float32 [Q, 2] (not modified) the rows start there instead, so the schedule can be stepped: ``first_epoch > 1``
    needs it.  ``last_epoch=0`` (with ``first_epoch=1`` and no ``y0``) returns the start alone.  A row's position depends
    on that row alone -- not on the other rows of the call, on ``blocks`` (the grid; 0: the library's choice) or on the
    run; a row without neighbours (a non-finite query) gets NaN."""
    n, k = _check_knn(idx, dist)
    start_only = last_epoch == 0 and first_epoch == 1 and y0 is None and not isinstance(last_epoch, bool)
    last = 0 if start_only else _check_epoch_args(n_epochs, seed, negative_sample_rate, learning_rate, first_epoch, last_epoch)
    if start_only:
        _check_epoch_args(n_epochs, seed, negative_sample_rate, learning_rate, 1, None)
    _int(blocks, "blocks", 0, (1 << 31) - 1)
    if not (float(a) > 0 and float(b) > 0):
        raise ValueError(f"a and b must be positive, got a={a!r} b={b!r}")
    dev = idx.device
    bank_y = _positions(bank_y, "bank_y", None, dev)
    if y0 is not None:
        y0 = _positions(y0, "y0", n, dev)
    elif first_epoch > 1:
        raise ValueError(f"first_epoch = {first_epoch} needs y0, the positions after epoch {first_epoch - 1}")
    n_bank = int(bank_y.shape[0])
    if n and not n_bank:
        raise ValueError("bank_y is empty: there is no map to place the rows on")
    w, _sigma = query_memberships(idx, dist)
    idx = idx.contiguous()
    with torch.cuda.device(dev):
        y = torch.empty((n, 2), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().btsbot_layout_transform(_ptr(idx), _ptr(w), _ptr(bank_y), n_bank, n, k, _ptr(y0) if y0 is not None
                                                      else C.c_void_p(0), _ptr(y), n_epochs, first_epoch, last, float(a),
                                                      float(b), seed & _U64, negative_sample_rate, float(learning_rate),
                                                      blocks, _stream(dev)), "btsbot_layout_transform")
    return y


class EmbeddingMap:
    """A bank of embedding rows (an ``EmbeddingIndex``) with its 2-D map, and the placement of new rows on it.

        m = EmbeddingMap(bank)                          # embedding_layout of the bank
        m = EmbeddingMap.from_positions(bank, y)        # a map made earlier
        y_new = m.transform(queries)                    # the map does not move
        m.extend(rows)                                  # transform, then the rows join the bank at those positions
        kept = m.remove(which)                          # rows leave the bank and the map; the survivors do not move
        mi = m.map_index()                              # a MapIndex over embedding_: neighbours ON the map

    ``n_neighbors`` counts the row itself in the fit (as ``embedding_layout``) and is the number of bank rows a new row is
    attached to in ``transform`` (as umap-learn).  ``transform`` runs 100 epochs whatever the number of rows
    (``n_epochs=None``), so that a row's position does not depend on the size of the call.  Calls on one map must be
    ordered by the caller's streams."""

    def __init__(self, bank: torch.Tensor, n_neighbors: int = 15, min_dist: float = 0.1, spread: float = 1.0,
                 n_epochs: Optional[int] = None, init="pca", seed: int = 0, metric: str = "euclidean"):
        from .neighbors import EmbeddingIndex, _self_first_graph
        _int(n_neighbors, "n_neighbors", 2, _lib.LAYOUT_MAX_K)
        self.a, self.b = find_ab_params(spread, min_dist)
        self.n_neighbors = n_neighbors
        self.index = EmbeddingIndex(bank, metric)
        self.embedding_ = embedding_layout(self.index.bank, n_neighbors, min_dist, spread, n_epochs, init, seed, metric,
                                           knn=_self_first_graph(self.index, n_neighbors))

    @classmethod
    def from_positions(cls, bank_or_index, y: torch.Tensor, n_neighbors: int = 15, min_dist: float = 0.1,
                       spread: float = 1.0) -> "EmbeddingMap":
        """The map ``y`` float32 [N, 2] of ``bank_or_index`` (rows [N, D], packed here, or an ``EmbeddingIndex``, used
        as it is), laid out earlier -- ``embedding_layout``'s result or a run's ``_umap.csv``."""
        from .neighbors import EmbeddingIndex
        _int(n_neighbors, "n_neighbors", 2, _lib.LAYOUT_MAX_K)
        m = cls.__new__(cls)
        m.a, m.b = find_ab_params(spread, min_dist)
        m.n_neighbors = n_neighbors
        m.index = bank_or_index if isinstance(bank_or_index, EmbeddingIndex) else EmbeddingIndex(bank_or_index)
        m.embedding_ = _positions(y, "y", len(m.index), m.index.device).clone()
        return m

    def __len__(self) -> int:
        return len(self.index)

    def transform(self, queries: torch.Tensor, n_epochs: Optional[int] = None, seed: int = 0) -> torch.Tensor:
        """Positions float32 [Q, 2] of ``queries`` [Q, D] on the map (``layout_transform`` of their ``n_neighbors``
        nearest bank rows); a row that holds a non-finite value gets NaN."""
        epochs = 100 if n_epochs is None else _int(n_epochs, "n_epochs", 1, (1 << 31) - 1)
        idx, dist = self.index.query(queries, self.n_neighbors)
        return layout_transform(idx, dist, self.embedding_, epochs, a=self.a, b=self.b, seed=seed)

    def extend(self, rows: torch.Tensor, n_epochs: Optional[int] = None, seed: int = 0) -> torch.Tensor:
        """``transform(rows)``, after which the rows join the bank at those positions (and are neighbours and samples
        of later calls); returns the new positions."""
        y = self.transform(rows, n_epochs, seed)
        self.index.add(rows)
        self.embedding_ = torch.cat([self.embedding_, y])
        self._map_index = None
        return y

    def remove(self, which: torch.Tensor) -> torch.Tensor:
        """Removes rows from the bank and from the map (``EmbeddingIndex.remove``; ``which``: a bool [len] mask or int64
        row numbers) and returns ``kept`` int64, the old row number of every survivor.  ``embedding_`` becomes
        ``embedding_[kept]``: the survivors' positions do not move, and ``transform`` then attaches new rows to
        survivors only.  The cached ``MapIndex`` is dropped."""
        kept = self.index.remove(which)
        self.embedding_ = self.embedding_[kept]
        self._map_index = None
        return kept

    def quality(self, n_neighbors: Optional[int] = None, rows: Optional[torch.Tensor] = None) -> dict:
        """``quality.map_quality`` of ``embedding_`` against the bank it maps: trustworthiness, continuity and
        neighbour recall at ``n_neighbors`` (default: the map's own), judged from ``rows`` (default: every row)."""
        from .quality import map_quality
        k = self.n_neighbors if n_neighbors is None else n_neighbors
        return map_quality(self.index.bank, self.embedding_, k, metric=self.index.metric, rows=rows)

    def map_index(self):
        """A ``MapIndex`` over ``embedding_`` -- radius, count and k-nearest questions about the MAP positions --,
        built at the first call and kept until ``extend`` moves on (or ``embedding_`` is replaced)."""
        from .mapindex import MapIndex
        cached = getattr(self, "_map_index", None)
        if cached is None or cached[0] is not self.embedding_:
            cached = (self.embedding_, MapIndex(self.embedding_))
            self._map_index = cached
        return cached[1]
