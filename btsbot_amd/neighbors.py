"""Similar alerts: exact k-nearest neighbours over embedding rows, on the device.

``model.embed(...)`` and ``ScoreStream(embed=...)`` hand out a learned vector per alert; this module answers "which rows
of an archive lie nearest to these" without ever forming the [Q, N] distance matrix (csrc/knn.hip):

    idx, dist = embedding_neighbors(queries, bank, k)            # int64 [Q, k], float32 [Q, k]
    index = EmbeddingIndex(bank)                                 # packs the bank once
    index.add(more_rows)                                         # packs only the new rows
    idx, dist = index.query(queries, k)
    idx, dist = knn_graph(emb, k)                                # every row among the others (self first, distance 0)

``dist`` is the Euclidean distance (not squared) or, with ``metric="cosine"``, ``1 - cos`` (``cos = 0`` for a zero row),
recomputed for the returned rows in the direct form from the fp32 rows.  Rows are ordered by (dist, bank index).  Where
fewer than ``k`` bank rows are eligible the tail is ``idx = -1, dist = +inf``; a bank row that holds a non-finite value is
never returned; a query row that does gets ``idx = -1, dist = NaN`` throughout.  A row's answer does not depend, bit for
bit, on the other rows of the call, on ``splits`` or on the run.  Nothing here synchronises with the host; the work is
queued on the current stream.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib

METRICS = tuple(_lib.KNN_METRIC)


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


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


def _check_k(k, splits) -> None:
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= _lib.KNN_MAX_K:
        raise ValueError(f"k must be an int in 1..{_lib.KNN_MAX_K}, got {k!r}")
    if not isinstance(splits, int) or isinstance(splits, bool) or not 0 <= splits <= _lib.KNN_MAX_SPLITS:
        raise ValueError(f"splits must be an int in 0..{_lib.KNN_MAX_SPLITS} (0: the library's choice), got {splits!r}")


def _metric(metric) -> int:
    if metric not in _lib.KNN_METRIC:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    return _lib.KNN_METRIC[metric]


class EmbeddingIndex:
    """A bank of embedding rows on one GPU with its packed operand image (norms, per-row scales, f16 head and remainder
    planes), built once and extended by ``add``.  A row's image depends on the row alone, so an index built by several
    ``add`` calls answers bit for bit like one built at once.

    Calls on one index must be ordered by the caller's streams."""

    def __init__(self, bank: torch.Tensor, metric: str = "euclidean"):
        self._metric_id = _metric(metric)
        self.metric = metric
        rows = _rows(bank, "bank")
        self.device = rows.device
        self.dim = int(rows.shape[1])
        self._n = 0
        self._cap = 0
        self._bank = rows.new_empty((0, self.dim))
        self._packed = torch.empty(0, dtype=torch.uint8, device=self.device)
        self.add(rows)

    def __len__(self) -> int:
        return self._n

    @property
    def bank(self) -> torch.Tensor:
        """The fp32 rows held, [len, D] (a view of the index's storage)."""
        return self._bank[:self._n]

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _record_bytes(self) -> int:
        return int(_lib.lib().btsbot_knn_bank_bytes(1, self.dim))

    def add(self, rows: torch.Tensor) -> "EmbeddingIndex":
        """Appends ``rows`` [n, D]; only they are packed (what is held already moves as bytes when the storage grows)."""
        rows = _rows(rows, "rows", self.device)
        if rows.shape[1] != self.dim:
            raise ValueError(f"rows: D = {rows.shape[1]}, the index holds D = {self.dim}")
        n = int(rows.shape[0])
        if self._n + n >= 1 << 31:
            raise ValueError(f"an index holds at most 2^31 - 1 rows ({self._n} + {n})")
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
                self._bank, self._packed, self._cap = bank, packed, cap
            new = self._bank[self._n:self._n + n]
            new.copy_(rows)
            _lib.check(L.btsbot_knn_pack_bank(_ptr(new), self._n, n, self.dim, self._metric_id, _ptr(self._packed),
                                              self._cap, self._stream()), "btsbot_knn_pack_bank")
        self._n += n
        return self

    def query(self, queries: torch.Tensor, k: int, *, splits: int = 0,
              self_offset: int = -1) -> Tuple[torch.Tensor, torch.Tensor]:
        """``idx`` int64 [Q, k] and ``dist`` float32 [Q, k] of each query row's ``k`` nearest rows of the index.
        splits: bank slices searched by separate workgroups (0: the library's choice; the answer does not depend on it).
        self_offset >= 0: query row i is row i + self_offset of the index and is not its own candidate."""
        _check_k(k, splits)
        q = _rows(queries, "queries", self.device)
        if q.shape[1] != self.dim:
            raise ValueError(f"queries: D = {q.shape[1]}, the index holds D = {self.dim}")
        if not isinstance(self_offset, int):
            raise ValueError(f"self_offset must be an int, got {self_offset!r}")
        nq = int(q.shape[0])
        idx = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        dist = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        if nq == 0:
            return idx, dist
        L = _lib.lib()
        need = int(L.btsbot_knn_workspace(nq, self._n, self.dim, k, splits))
        if need < 0:
            _lib.check(need, "btsbot_knn_workspace")
        with torch.cuda.device(self.device):
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            _lib.check(L.btsbot_knn_query(_ptr(q), nq, _ptr(self._bank), _ptr(self._packed), self._n, self.dim, k,
                                          self._metric_id, self_offset, splits, _ptr(idx), _ptr(dist), _ptr(ws), need,
                                          self._stream()), "btsbot_knn_query")
        return idx, dist


def embedding_neighbors(queries: torch.Tensor, bank: torch.Tensor, k: int, metric: str = "euclidean", *,
                        splits: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The ``k`` nearest rows of ``bank`` [N, D] for every row of ``queries`` [Q, D]: ``idx`` int64 [Q, k], ``dist``
    float32 [Q, k] (see the module text).  Packs the bank for this one call; keep an ``EmbeddingIndex`` to query a bank
    more than once."""
    _check_k(k, splits)
    _metric(metric)
    q = _rows(queries, "queries")
    b = _rows(bank, "bank", q.device)
    if q.shape[1] != b.shape[1]:
        raise ValueError(f"queries have D = {q.shape[1]}, the bank D = {b.shape[1]}")
    return EmbeddingIndex(b, metric).query(q, k, splits=splits)


def knn_graph(emb: torch.Tensor, k: int, include_self: bool = True, metric: str = "euclidean", *,
              splits: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Every row of ``emb`` [N, D] among the others: ``idx`` int64 [N, k], ``dist`` float32 [N, k].

    include_self=True: the row itself first at distance 0, then its ``k - 1`` nearest others -- the layout pynndescent
    and umap-learn's ``precomputed_knn`` use.  include_self=False: ``k`` others.  A row is excluded by position, not by
    value: its duplicates are legitimate neighbours at distance 0."""
    _check_k(k, splits)
    _metric(metric)
    rows = _rows(emb, "emb")
    index = EmbeddingIndex(rows, metric)
    if not include_self:
        return index.query(rows, k, splits=splits, self_offset=0)
    return _self_first_graph(index, k, splits)


def _self_first_graph(index: EmbeddingIndex, k: int, splits: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``knn_graph(index.bank, k, include_self=True)`` from an index already packed."""
    rows = index.bank
    n = int(rows.shape[0])
    idx = torch.empty((n, k), dtype=torch.int64, device=rows.device)
    dist = torch.empty((n, k), dtype=torch.float32, device=rows.device)
    finite = torch.isfinite(rows).all(dim=1)
    idx[:, 0] = torch.where(finite, torch.arange(n, device=rows.device), torch.full_like(idx[:, 0], -1))
    dist[:, 0] = torch.where(finite, torch.zeros_like(dist[:, 0]), torch.full_like(dist[:, 0], float("nan")))
    if k > 1:
        idx[:, 1:], dist[:, 1:] = index.query(rows, k - 1, splits=splits, self_offset=0)
    return idx, dist
