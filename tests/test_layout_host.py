"""CPU: the host side of btsbot_amd.layout -- argument errors (nothing here needs a GPU: every check comes before the
first device call), find_ab_params, the C declarations, and the restatement's own graph and trustworthiness
(tests/layout_ref.py)."""
import os
import re

import numpy as np
import pytest
import torch

import btsbot_amd
import layout_ref as R
from btsbot_amd import _lib
from btsbot_amd.layout import FuzzyGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _knn(n=6, k=3):
    return torch.zeros((n, k), dtype=torch.int64), torch.zeros((n, k), dtype=torch.float32)


def _graph(n=6):
    return FuzzyGraph(torch.zeros(n + 1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(1),
                      torch.zeros(1), torch.zeros(n), torch.zeros(n))


# ---- argument errors
def test_fuzzy_graph_argument_errors():
    idx, dist = _knn()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.fuzzy_graph(idx, dist)
    with pytest.raises(TypeError):
        btsbot_amd.fuzzy_graph(idx.numpy(), dist)
    with pytest.raises(ValueError, match="int64"):
        btsbot_amd.fuzzy_graph(idx.int(), dist)
    with pytest.raises(ValueError, match="float32"):
        btsbot_amd.fuzzy_graph(idx, dist.double())
    with pytest.raises(ValueError, match=r"\[N, k\]"):
        btsbot_amd.fuzzy_graph(idx, dist[:, :2])
    with pytest.raises(ValueError, match=r"\[N, k\]"):
        btsbot_amd.fuzzy_graph(idx[0], dist[0])
    for k in (1, 65):
        with pytest.raises(ValueError, match="2..64"):
            btsbot_amd.fuzzy_graph(*_knn(4, k))
    with pytest.raises(ValueError, match="2\\^31"):
        btsbot_amd.fuzzy_graph(torch.empty((1 << 25, 64), dtype=torch.int64, device="meta"),
                               torch.empty((1 << 25, 64), dtype=torch.float32, device="meta"))


def test_optimize_layout_argument_errors():
    g, y0 = _graph(), torch.zeros((6, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.optimize_layout(g, y0, 10, 1.5, 0.9)
    with pytest.raises(TypeError, match="FuzzyGraph"):
        btsbot_amd.optimize_layout((g.indptr, g.indices), y0, 10, 1.5, 0.9)
    with pytest.raises(TypeError):
        btsbot_amd.optimize_layout(g, y0.numpy(), 10, 1.5, 0.9)
    for bad in (torch.zeros((5, 2)), torch.zeros((6, 3)), torch.zeros(12), torch.zeros((6, 2), dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"float32 \[6, 2\]"):
            btsbot_amd.optimize_layout(g, bad, 10, 1.5, 0.9)
    for rate in (-1, 65, 2.0, True):
        with pytest.raises(ValueError, match="negative_sample_rate"):
            btsbot_amd.optimize_layout(g, y0, 10, 1.5, 0.9, negative_sample_rate=rate)
    with pytest.raises(ValueError, match="past last_epoch"):
        btsbot_amd.optimize_layout(g, y0, 10, 1.5, 0.9, first_epoch=5, last_epoch=4)
    for kw in (dict(first_epoch=0), dict(first_epoch=11), dict(last_epoch=11), dict(last_epoch=0), dict(first_epoch=1.0)):
        with pytest.raises(ValueError, match="epoch"):
            btsbot_amd.optimize_layout(g, y0, 10, 1.5, 0.9, **kw)
    for n_epochs in (0, -3, 2.5):
        with pytest.raises(ValueError, match="n_epochs"):
            btsbot_amd.optimize_layout(g, y0, n_epochs, 1.5, 0.9)
    with pytest.raises(ValueError, match="seed"):
        btsbot_amd.optimize_layout(g, y0, 10, 1.5, 0.9, seed=1.5)
    with pytest.raises(ValueError, match="learning_rate"):
        btsbot_amd.optimize_layout(g, y0, 10, 1.5, 0.9, learning_rate=0.0)
    with pytest.raises(ValueError, match="a and b"):
        btsbot_amd.optimize_layout(g, y0, 10, -1.0, 0.9)
    with pytest.raises(ValueError, match="blocks"):
        btsbot_amd.optimize_layout(g, y0, 10, 1.5, 0.9, blocks=-1)


def test_embedding_layout_argument_errors():
    emb = torch.zeros((6, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.embedding_layout(emb)
    with pytest.raises(TypeError):
        btsbot_amd.embedding_layout(emb.numpy())
    for k in (1, 65, 15.0):
        with pytest.raises(ValueError, match="n_neighbors"):
            btsbot_amd.embedding_layout(emb, n_neighbors=k)
    with pytest.raises(ValueError, match="metric"):
        btsbot_amd.embedding_layout(emb, metric="manhattan")
    with pytest.raises(ValueError, match="init"):
        btsbot_amd.embedding_layout(emb, init="spectral")
    with pytest.raises(ValueError, match="n_epochs"):
        btsbot_amd.embedding_layout(emb, n_epochs=0)
    with pytest.raises(ValueError, match="min_dist"):
        btsbot_amd.embedding_layout(emb, min_dist=5.0)
    with pytest.raises(ValueError, match="knn"):
        btsbot_amd.embedding_layout(emb, knn=_knn()[0])


# ---- find_ab_params
def test_find_ab_params_defaults():
    a, b = btsbot_amd.find_ab_params(1, 0.1)
    assert abs(a - 1.5769) <= 1e-3 and abs(b - 0.8951) <= 1e-3
    assert btsbot_amd.find_ab_params() == (a, b)


@pytest.mark.parametrize("spread,min_dist", [(1.0, 0.5), (2.0, 0.01), (0.5, 0.25)])
def test_find_ab_params_against_curve_fit(spread, min_dist):
    scipy_optimize = pytest.importorskip("scipy.optimize")
    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    want, _ = scipy_optimize.curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    got = btsbot_amd.find_ab_params(spread, min_dist)
    assert np.allclose(got, want, rtol=1e-4, atol=1e-4), (got, want)


# ---- the C ABI
def test_the_new_symbols_are_declared():
    header = open(os.path.join(ROOT, "include", "btsbot_hip.h")).read()
    for name in ("btsbot_layout_smooth_knn", "btsbot_layout_symmetrize", "btsbot_layout_epochs",
                 "btsbot_layout_symmetrize_workspace", "btsbot_layout_init"):
        assert name in _lib.SYMBOLS
        assert re.search(r"\b(int|int64_t) " + name + r"\(", header), name
    assert "layout.hip" in open(os.path.join(ROOT, "btsbot_amd", "csrc", "Makefile")).read()
    assert _lib.ABI_VERSION == 1


# ---- the restatement
def test_restatement_trustworthiness_equals_sklearn():
    manifold = pytest.importorskip("sklearn.manifold")
    rng = np.random.default_rng(3)
    X = rng.standard_normal((200, 12))
    for Y in (X[:, :2], rng.standard_normal((200, 2)), X[:, 3:5] + 0.1 * rng.standard_normal((200, 2))):
        for k in (5, 15):
            assert abs(R.trustworthiness(X, Y, k) - manifold.trustworthiness(X, Y, n_neighbors=k)) <= 1e-12


@pytest.mark.parametrize("n,k", [(3, 2), (65, 15), (40, 64), (300, 33)])
def test_restatement_graph_is_symmetric_with_ascending_rows(n, k):
    emb = np.random.default_rng(n).standard_normal((n, 7)).astype(np.float32)
    emb[n // 2] = emb[0]                                            # a duplicate: distance 0 beyond column 0
    idx, dist = R.knn_exact(emb, k)
    g = R.fuzzy_graph(idx, dist)
    R.check_symmetric(g.indptr, g.indices, g.weights)
    assert g.indptr[0] == 0 and g.indptr[-1] == len(g.indices) == len(g.weights)
    assert (g.weights >= 0).all() and (g.weights <= 1).all() and g.weights.max() == 1
    # every directed neighbour is an edge, and nothing else is
    want = {(i, int(j)) for i in range(n) for j in idx[i, 1:] if j >= 0}
    want |= {(j, i) for i, j in want}
    rows = np.repeat(np.arange(n), np.diff(g.indptr))
    assert set(zip(rows.tolist(), g.indices.tolist())) == want
    # smooth_knn_dist's defining property where the bisection converged and the floor is idle
    rho, sigma, memb = R.smooth_knn(idx, dist)
    full = (idx >= 0).all(axis=1) & (sigma > 2e-3 * dist.mean(axis=1))
    if k <= n and full.any():
        assert np.abs(memb[full].astype(np.float64).sum(axis=1) - np.log2(k)).max() <= 1e-4
    if k >= 3:
        assert dist[0, 1] == 0 and rho[0] == dist[0, 2] > 0             # the duplicate is skipped: smallest POSITIVE distance


def test_restatement_hash_and_inits():
    assert int(R.mix64(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF       # splitmix64's first output from 0
    y = R.random_init(1000, 5)
    assert y.dtype == np.float32 and y.shape == (1000, 2) and (y >= -10).all() and (y < 10).all()
    assert abs(y.mean()) < 0.5 and not np.array_equal(y, R.random_init(1000, 6))
    j = R.jitter(np.zeros((1000, 2), dtype=np.float32), 5)
    assert np.abs(j).max() <= 1e-4 and np.abs(j).max() > 5e-5
    emb, _ = R.cluster_set(100, 8, 0)
    emb[7, 3] = np.nan
    p = R.pca_init(emb, 0)
    assert np.isnan(p[7]).all() and abs(np.nanmax(np.abs(p)) - 10) < 1e-3


def test_epoch_bound_constant_is_within_the_limit():
    assert R.EPOCH_C <= R.EPOCH_C_LIMIT == 256
    assert R.EPOCH_C == 2.0 ** round(np.log2(R.EPOCH_C))
    if R.EPOCH_MEASURED is not None:
        assert 8 * R.EPOCH_MEASURED <= R.EPOCH_C < 16 * R.EPOCH_MEASURED
