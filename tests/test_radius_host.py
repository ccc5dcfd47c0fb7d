"""Host tests of the radius search and DBSCAN (no GPU): the restatements of tests/radius_ref.py against scikit-learn, the
emulated candidate pass against the must-in set, the argument checks and the C ABI's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import btsbot_amd
from btsbot_amd import _lib
import radius_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- DBSCAN: the rule of btsbot_amd.clusters is sklearn's
@pytest.mark.parametrize("name, X, eps, min_samples", R.dbscan_sets(), ids=lambda v: v if isinstance(v, str) else None)
def test_dbscan_ref_equals_sklearn(name, X, eps, min_samples):
    cluster = pytest.importorskip("sklearn.cluster")
    assert R.pairs_in_band(X, eps) == 0
    want = cluster.DBSCAN(eps=float(np.float32(eps)), min_samples=min_samples, algorithm="brute").fit(X.astype(np.float64))
    labels, core = R.dbscan_ref(X, eps, min_samples)
    assert labels.max() >= 1 and (labels == -1).any() and (~core & (labels >= 0)).any(), "a set that tests nothing"
    assert np.array_equal(labels, want.labels_)
    assert np.array_equal(np.flatnonzero(core), want.core_sample_indices_)


def test_dbscan_ref_gives_a_border_row_between_two_clusters_the_lower_label():
    cluster = pytest.importorskip("sklearn.cluster")
    X, eps, min_samples, border = R.border_set()
    labels, core = R.dbscan_ref(X, eps, min_samples)
    assert not core[border] and core[:border].all() and core[border + 1:].all()
    assert labels.tolist() == [0] * 5 + [0] + [1] * 5
    want = cluster.DBSCAN(eps=float(np.float32(eps)), min_samples=min_samples, algorithm="brute").fit(X.astype(np.float64))
    assert np.array_equal(labels, want.labels_)


def test_dbscan_ref_counts_distinct_groups():
    rng = np.random.default_rng(3)
    centres = rng.uniform(0, 100, size=(40, 2))
    X = (np.repeat(centres, 5, axis=0) + rng.normal(0, 0.01, size=(200, 2))).astype(np.float32)
    obj = np.repeat(np.arange(40), 5)
    labels, core = R.dbscan_ref(X, 0.2, 5)
    assert core.all() and labels.max() >= 30
    labels, core = R.dbscan_ref(X, 0.2, 5, groups=obj)
    assert not core.any() and (labels == -1).all()


# ---- the radius restatement
@pytest.mark.parametrize("metric", ("euclidean", "cosine"))
def test_radius_restatement_equals_sklearn(metric):
    nb = pytest.importorskip("sklearn.neighbors")
    q, b = R.make_rows("normal", 40, 7, 1), R.make_rows("normal", 300, 7, 2)
    d = R.d64_matrix(q, b, metric)
    el = R.eligible(q, b)
    r = R.pick_radius(d, el, 7, metric)
    assert R.band_share(d, el, r, 7, metric) == 0
    indptr, indices, dist = R.radius_lists(q, b, r, metric)
    assert 0 < indptr[-1] < el.sum()
    want = nb.NearestNeighbors(radius=r, algorithm="brute", metric=metric).fit(b.astype(np.float64)) \
        .radius_neighbors(q.astype(np.float64), return_distance=False)
    for i in range(40):
        assert sorted(want[i].tolist()) == indices[indptr[i]:indptr[i + 1]].tolist()
    R.check_radius(q, b, r, indptr, indices, dist, metric)
    order = R.radius_lists(q, b, r, metric, sort="distance")
    R.check_radius(q, b, r, *order, metric, sort="distance")


def test_check_radius_notices_what_it_should():
    q, b = R.make_rows("normal", 20, 5, 1), R.make_rows("normal", 100, 5, 2)
    d = R.d64_matrix(q, b, "euclidean")
    r = R.pick_radius(d, R.eligible(q, b), 5, "euclidean")
    indptr, indices, dist = R.radius_lists(q, b, r)
    row = int(np.argmax(np.diff(indptr) >= 2))
    a = indptr[row]
    with pytest.raises(AssertionError, match="must-in"):
        R.check_radius(q, b, r, indptr - (indptr > a), np.delete(indices, a), np.delete(dist, a))
    bad = indices.copy()
    bad[a], bad[a + 1] = indices[a + 1], indices[a]
    with pytest.raises(AssertionError, match="ordered by index"):
        R.check_radius(q, b, r, indptr, bad, dist)
    far = int(np.argmax(d[row]))
    at = a + int(np.searchsorted(indices[a:indptr[row + 1]], far))
    with pytest.raises(AssertionError, match="must-out"):
        R.check_radius(q, b, r, indptr + (indptr > a), np.insert(indices, at, far),
                       np.insert(dist, at, np.float32(d[row, far])))
    off = dist.copy()
    off[a] *= np.float32(1 + 1e-4)
    with pytest.raises(AssertionError, match="distance"):
        R.check_radius(q, b, r, indptr, indices, off)


# ---- the candidate pass loses no member
WORST = {}


@pytest.mark.parametrize("metric", ("euclidean", "cosine"))
@pytest.mark.parametrize("dim", (1, 33, 528, 1024))
def test_emulated_candidate_pass_keeps_every_must_in_pair(dim, metric):
    worst = 0.0
    for kind in R.KINDS:
        q, b = R.make_rows(kind, 48, dim, 1000), R.make_rows(kind, 300, dim, 2000)
        d = R.d64_matrix(q, b, metric)
        el = R.eligible(q, b)
        for frac in (0.05, 0.6):
            r = R.pick_radius(d, el, dim, metric, fractions=(frac,))
            adm, g, margin = R.emulate_candidates(q, b, r, metric)
            must_in, _ = R.split_by_band(R.d64_matrix(q, b, metric, r), r, dim, metric)
            # (stricter than needed: also every pair the float64 distance puts within r at all)
            inside = el & (must_in | (d <= r))
            assert adm[inside].all(), f"{kind} D={dim} {metric}: {(inside & ~adm).sum()} members are no candidates"
            exact = d ** 2 if metric == "euclidean" else d
            worst = max(worst, float((np.abs(g.astype(np.float64) - exact) / margin)[el].max()))
    WORST[(dim, metric)] = worst
    print(f"D={dim} {metric}: worst |GEMM form - float64| / margin = {worst:.4f}")
    assert worst < 1.0


def test_emulated_candidate_pass_admits_nothing_for_bad_rows():
    q, b = R.make_rows("normal", 8, 5, 1), R.make_rows("normal", 50, 5, 2)
    q[3, 0], b[7, 1] = np.nan, np.inf
    adm, _, _ = R.emulate_candidates(q, b, np.inf)
    assert not adm[3].any() and not adm[:, 7].any() and adm[np.arange(8) != 3][:, np.arange(50) != 7].all()


# ---- arguments
def test_radius_arguments_are_checked_before_the_device_is_touched():
    q, b = torch.zeros(4, 3), torch.zeros(9, 3)
    for bad in (-1.0, float("nan"), "1", None, True):
        with pytest.raises(ValueError, match="r must be"):
            btsbot_amd.radius_neighbors(q, b, bad)
    for bad in (torch.ones(3), torch.ones(4, 1), torch.ones(4, dtype=torch.int64)):
        with pytest.raises(ValueError, match="one float radius per query row"):
            btsbot_amd.radius_neighbors(q, b, bad)
    with pytest.raises(ValueError, match="r must be >= 0 in every row"):
        btsbot_amd.radius_neighbors(q, b, torch.tensor([1.0, 2.0, float("nan"), 1.0]))
    with pytest.raises(ValueError, match="r must be >= 0 in every row"):
        btsbot_amd.radius_graph(q, torch.tensor([1.0, -2.0, 0.0, 1.0]))
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="max_total"):
            btsbot_amd.radius_neighbors(q, b, 1.0, max_total=bad)
    with pytest.raises(ValueError, match="sort"):
        btsbot_amd.radius_neighbors(q, b, 1.0, sort="score")
    with pytest.raises(ValueError, match="splits"):
        btsbot_amd.radius_neighbors(q, b, 1.0, splits=33)
    with pytest.raises(ValueError, match="metric"):
        btsbot_amd.radius_neighbors(q, b, 1.0, metric="manhattan")
    with pytest.raises(ValueError, match="group_mode"):
        btsbot_amd.radius_graph(q, 1.0, group_mode="distinct")
    with pytest.raises(ValueError, match="need an index built with groups"):
        btsbot_amd.radius_neighbors(q, b, 1.0, exclude_same_group=True, query_groups=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # valid arguments: only the device is missing
        btsbot_amd.radius_neighbors(q, b, float("inf"), max_total=0)
    with pytest.raises(ValueError, match="eps"):
        btsbot_amd.dbscan(q, -0.5)
    with pytest.raises(ValueError, match="min_samples"):
        btsbot_amd.dbscan(q, 0.5, min_samples=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.dbscan(q, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.graph_components(torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        btsbot_amd.graph_components(torch.zeros(5, dtype=torch.int32), torch.zeros(0, dtype=torch.int64))


def test_the_new_symbols_are_declared_exported_and_refuse_bad_arguments():
    header = open(os.path.join(ROOT, "include", "btsbot_hip.h")).read()
    raw, L = C.CDLL(_lib.LIB_PATH), _lib.lib()
    for name in ("btsbot_knn_radius_workspace", "btsbot_knn_radius_count", "btsbot_knn_radius_fill",
                 "btsbot_graph_components", "btsbot_dbscan_labels"):
        assert name in _lib.SYMBOLS and hasattr(raw, name)
        assert re.search(r"^(int|int64_t) " + name + r"\(", header, re.M), name
    assert "components.hip" in open(os.path.join(ROOT, "btsbot_amd", "csrc", "Makefile")).read()
    for name in ("radius_neighbors", "radius_graph", "graph_components", "dbscan", "clusters"):
        assert name in btsbot_amd.__all__ and hasattr(btsbot_amd, name)
    assert L.btsbot_knn_radius_workspace(0, 5) == 0 and L.btsbot_knn_radius_workspace(3, 5) == 512
    assert L.btsbot_knn_radius_workspace(3, 1025) == _lib.ERR_INVALID_ARG
    p = C.c_void_p(256)          # never dereferenced: every call below is refused first
    bad = _lib.ERR_INVALID_ARG

    def count(nq=4, nb=9, dim=3, metric=0, splits=1, flags=0, ws=768, radius=p, qg=None, bg=None):
        return L.btsbot_knn_radius_count(p, nq, p, nb, dim, metric, radius, -1, splits, qg, bg, flags, p, p, ws, None)

    assert count(splits=0) == bad and b"splits" in L.btsbot_last_error()
    assert count(splits=33) == bad
    assert count(flags=2) == bad and b"flags" in L.btsbot_last_error()
    assert count(flags=1) == bad and b"query_group" in L.btsbot_last_error()
    assert count(metric=2) == bad and count(dim=0) == bad and count(radius=None) == bad
    assert count(ws=767) == bad and b"workspace" in L.btsbot_last_error()
    assert count(nq=0) == _lib.OK
    fill = (p, 4, p, p, 9, 3, 0, p, -1, 1, None, None, 0, p, p)
    assert L.btsbot_knn_radius_fill(*fill, -1, p, p, p, p, p, 768, None) == bad
    assert L.btsbot_knn_radius_fill(*fill, 0, p, p, p, p, p, 768, None) == _lib.OK       # nothing to do
    assert L.btsbot_knn_radius_fill(*fill, 5, None, p, p, p, p, 512, None) == bad
    assert L.btsbot_graph_components(p, p, None, -1, p, p, None) == bad
    assert L.btsbot_graph_components(None, p, None, 3, p, p, None) == bad
    assert L.btsbot_graph_components(p, p, None, 0, p, p, None) == _lib.OK
    assert L.btsbot_dbscan_labels(p, p, p, p, None, 3, p, None) == bad
    assert L.btsbot_dbscan_labels(p, p, p, p, p, 1 << 31, p, None) == bad
