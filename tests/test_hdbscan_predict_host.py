"""Cluster prediction without a GPU: the tables of a fitted tree (``btsbot_hdbscan_model`` through ctypes) against the
float64 restatement of tests/hdbscan_predict_ref.py, exactly; GLOSH; and the restatement's prediction against the sets it
is used on by tests/test_gpu_cluster_predict.py."""
import ctypes as C
import functools
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hdbscan_ref as R                                                   # noqa: E402
import hdbscan_predict_ref as P                                           # noqa: E402
import btsbot_amd                                                         # noqa: E402
from btsbot_amd import _lib                                               # noqa: E402
from btsbot_amd.hdbscan import _model_host, _tree_host                    # noqa: E402

SETS = dict(R.equality_sets())
TABLES = ("row_cluster", "row_lambda", "outlier", "parent", "birth", "label", "max_lambda", "death")


@functools.lru_cache(maxsize=None)
def _dist(name):
    return R.dist_matrix(SETS[name])


@functools.lru_cache(maxsize=None)
def _mst(name, min_samples):
    core, W = R.mutual_reachability(_dist(name), min_samples)
    return (core,) + R.mst(W)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a.astype(np.int64)


def _same_tables(got, ref, lam_zero):
    for name in TABLES:
        assert got[name].shape == ref[name].shape, name
        assert np.array_equal(_bits(got[name]), _bits(np.asarray(ref[name], got[name].dtype))), name
    assert got["row_cluster"].dtype == got["parent"].dtype == got["label"].dtype == np.int32
    assert got["lam_zero"] == lam_zero


# ---- 1. the tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("method", ("eom", "leaf"))
def test_library_tables_equal_the_restatement_and_rebuild_the_labels(name, method):
    n = len(SETS[name])
    for mcs, ms in R.PAIRS:
        _core, edges, weights = _mst(name, ms)
        w32 = weights.astype(np.float32)
        for single in (False, True):
            got = _model_host(edges, w32, n, mcs, method, single)
            ref_tree = R.tree(edges, weights, n, mcs, method, single)
            ref = P.tables(ref_tree["condensed"], n, method, single)
            _same_tables(got, ref, P.lam_zero_of(weights))
            # labels and probabilities rebuilt from the library's own tables are btsbot_hdbscan_tree's
            lab, prob, _cond = _tree_host(edges, w32, n, mcs, method, single)
            again = P.labels_from(got)
            assert np.array_equal(again[0], lab) and np.array_equal(_bits(again[1]), _bits(prob))
            assert np.array_equal(lab, ref_tree["labels"])
            # a parent stands before its children, the root alone has none
            assert got["parent"][0] == -1 and (got["parent"][1:] >= 0).all()
            assert (got["parent"] < np.arange(len(got["parent"]))).all()


def test_tables_of_rows_without_an_edge_and_of_no_edges():
    n = len(SETS["32-D seed 0"])
    _core, edges, weights = _mst("32-D seed 0", 5)
    got = _model_host(edges, weights.astype(np.float32), n + 3, 10)
    assert (got["row_cluster"][n:] == -1).all() and (got["row_lambda"][n:] == 0).all() and np.isnan(got["outlier"][n:]).all()
    ref = P.tables(R.tree(edges, weights, n, 10)["condensed"], n)
    assert np.array_equal(got["row_cluster"][:n], ref["row_cluster"])
    got = _model_host(np.zeros((0, 2), np.int64), np.zeros(0, np.float32), 4, 2)
    assert len(got["parent"]) == 0 and (got["row_cluster"] == -1).all() and np.isnan(got["outlier"]).all()
    assert got["lam_zero"] == 1.0
    got = _model_host(np.zeros((0, 2), np.int64), np.zeros(0, np.float32), 0, 2)
    assert len(got["row_cluster"]) == 0 and len(got["parent"]) == 0


# ---- 2. GLOSH -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETS))
def test_glosh_lies_in_the_unit_interval_and_is_zero_where_a_subtree_ends(name):
    n = len(SETS[name])
    for mcs, ms in R.PAIRS:
        _core, edges, weights = _mst(name, ms)
        t = _model_host(edges, weights.astype(np.float32), n, mcs)
        s, c = t["outlier"], t["row_cluster"]
        assert (c >= 0).all() and ((s >= 0) & (s <= 1)).all()
        nc = len(t["parent"])
        inside = [[] for _ in range(nc)]              # the clusters of every cluster's subtree
        for k in range(nc):
            a = k
            while a >= 0:
                inside[a].append(k)
                a = t["parent"][a]
        for k in range(nc):
            rows = np.flatnonzero(np.isin(c, inside[k]))
            assert t["death"][k] == t["row_lambda"][rows].max()
            top = rows[t["row_lambda"][rows] == t["death"][k]]
            assert len(top) >= 1 and (s[top] == 0).all()      # the row(s) that carry the subtree's largest lambda


def test_glosh_ranks_planted_far_rows_above_every_blob_row():
    """Four rows planted with spread 60: with (10, 5) the planted rows score 0.9881 to 0.9915 and no blob row above
    0.2626, a gap of 0.72 (seed 0; the set's own twelve far rows, spread 12, reach 0.9608 and are not blob rows)."""
    x, origin, _centres, _spreads = P.blobs_32d_parts(0)
    planted = np.random.default_rng(77).normal(0, 60.0, size=(4, 32)).astype(np.float32)
    X = np.concatenate([x, planted])
    ref = R.hdbscan_ref(R.dist_matrix(X), 10, 5)
    t = _model_host(ref["edges"], ref["weights"].astype(np.float32), len(X), 10)
    s = t["outlier"]
    blob = np.flatnonzero(origin >= 0)
    print(f"planted {np.sort(s[len(x):])}, blob rows at most {s[blob].max():.4f}, the set's far rows at most "
          f"{s[np.flatnonzero(origin < 0)].max():.4f}")
    assert s[len(x):].min() > s[blob].max()
    assert s[len(x):].min() > 0.95 and s[blob].max() < 0.9


# ---- 3. the restatement's prediction on the sets of the device tests ----------------------------------------------------
@pytest.mark.parametrize("seed", R.SEEDS_32D)
def test_restatement_puts_fresh_draws_into_their_blobs_and_far_rows_into_noise(seed):
    x, origin, _c, _s = P.blobs_32d_parts(seed)
    queries, q_origin = P.fresh_draws(seed)
    Dq = P.cross_dist(queries, x)
    for mcs, ms in R.PAIRS:
        ref = R.hdbscan_ref(R.dist_matrix(x), mcs, ms)
        t = P.tables(ref["condensed"], len(x), "eom", False)
        out = P.predict(Dq, ref["core"], t, P.lam_zero_of(ref["weights"]), ms)
        want = np.full(len(queries), -1)
        for b in range(5):
            lab = ref["labels"][origin == b]
            want[q_origin == b] = np.bincount(lab[lab >= 0]).argmax()
            assert (lab == want[q_origin == b][0]).mean() >= 0.9       # the blob is a cluster of the fit
        miss = int((out["label"] != want).sum())
        print(f"seed {seed} ({mcs}, {ms}): {miss} of {len(queries)} queries land elsewhere")
        assert miss <= 0.02 * len(queries)
        assert (out["label"][q_origin < 0] == -1).all() and (out["prob"][q_origin < 0] == 0).all()
        inside = out["label"] >= 0
        assert ((out["prob"][inside] > 0) & (out["prob"][inside] <= 1)).all()
        assert ((out["outlier"] >= 0) & (out["outlier"] <= 1)).all()
        assert out["outlier"][q_origin < 0].min() > out["outlier"][q_origin >= 0].max()


def test_restatement_returns_a_fitted_row_to_its_own_cluster():
    """A query that IS a bank row (not masked) finds itself at distance 0: w = its own core distance, and it ends in the
    cluster it fell out of or -- where it fell out below its core density -- in an ancestor of it."""
    name = "2-D seed 0"
    X = SETS[name]
    D = _dist(name)
    ref = R.hdbscan_ref(D, 10, 5)
    t = P.tables(ref["condensed"], len(X))
    out = P.predict(D, ref["core"], t, P.lam_zero_of(ref["weights"]), 5)
    same = out["cluster"] == t["row_cluster"]
    print(f"{int(same.sum())} of {len(X)} rows end in the cluster they fell out of")
    assert same.mean() > 0.9
    for i in np.flatnonzero(~same):
        a = t["row_cluster"][out["neighbor"][i]]
        while a >= 0 and a != out["cluster"][i]:
            a = t["parent"][a]
        assert a == out["cluster"][i]
    agree = out["label"] == ref["labels"]
    assert agree.mean() > 0.9


def test_the_radius_tier_of_the_device_test_is_not_empty():
    """tests/test_gpu_cluster_predict.py sends bank rows with a 1e-3 jitter through ``search_k=1``: the list then ends at
    the query's own core distance, nothing is strictly below its floor, and every full list is unresolved."""
    x = SETS["32-D seed 0"]
    queries = P.jittered_rows(x)
    Dq = P.cross_dist(queries, x)
    core = R.mutual_reachability(_dist("32-D seed 0"), 5)[0]
    ok = P.resolved(Dq, core, 5, 4)
    assert (~ok).sum() > 0
    ok = P.resolved(Dq, core, 5, 64)
    print(f"search_k = 64: {int((~ok).sum())} of {len(ok)} rows unresolved without slack")


# ---- 4. arguments ---------------------------------------------------------------------------------------------------------
def _raw_model(edges, weights, n, mcs=2, method=0, cap=None, nulls=()):
    L = _lib.lib()
    cap = max(n - 1, 1) if cap is None else cap
    size = min(max(n, 1), 8)                  # (a refused n is refused before anything of its size is touched)
    arrs = dict(row_cluster=np.empty(size, np.int32), row_lambda=np.empty(size), outlier=np.empty(size),
                parent=np.empty(max(cap, 1), np.int32), birth=np.empty(max(cap, 1)), label=np.empty(max(cap, 1), np.int32),
                max_lambda=np.empty(max(cap, 1)), death=np.empty(max(cap, 1)))
    nc, lz = C.c_int64(0), C.c_double(0)
    ptr = {k: (None if k in nulls else C.c_void_p(v.ctypes.data)) for k, v in arrs.items()}
    e = None if "edges" in nulls else C.c_void_p(edges.ctypes.data)
    w = None if "weights" in nulls else C.c_void_p(weights.ctypes.data)
    return L.btsbot_hdbscan_model(e, w, len(weights), n, mcs, method, 0, *ptr.values(), cap,
                                  None if "n_clusters" in nulls else C.byref(nc),
                                  None if "lam_zero" in nulls else C.byref(lz))


def test_bad_arguments_are_refused():
    edges = np.array([[0, 1], [1, 2], [2, 3]], np.int64)
    one = np.ones(3, np.float32)
    assert _raw_model(edges, one, 4) == _lib.OK
    for null in ("edges", "weights", "row_cluster", "row_lambda", "outlier", "n_clusters", "lam_zero"):
        assert _raw_model(edges, one, 4, nulls=(null,)) == _lib.ERR_INVALID_ARG, null
    two = np.array([1.0, 3.0, 1.0], np.float32)                       # mcs 2: the root and two children, three clusters
    assert _raw_model(edges, two, 4, cap=3) == _lib.OK
    assert _raw_model(edges, two, 4, cap=2) == _lib.ERR_INVALID_ARG
    assert _raw_model(edges, two, 4, nulls=("parent",)) == _lib.ERR_INVALID_ARG
    assert _raw_model(edges, two, 4, cap=-1) == _lib.ERR_INVALID_ARG
    assert _raw_model(edges, one, -1) == _lib.ERR_INVALID_ARG
    assert _raw_model(edges, one, 1 << 30) == _lib.ERR_INVALID_ARG
    assert _raw_model(edges, one, 3) == _lib.ERR_INVALID_ARG          # n_edges >= n
    assert _raw_model(edges, one, 4, mcs=1) == _lib.ERR_INVALID_ARG
    assert _raw_model(edges, one, 4, method=2) == _lib.ERR_INVALID_ARG
    for bad_e, bad_w, n in ((np.array([[0, 1], [1, 0]], np.int64), one[:2], 3),          # a cycle
                            (np.array([[0, 1], [2, 3]], np.int64), one[:2], 4),          # two trees
                            (np.array([[0, 1], [1, 3]], np.int64), one[:2], 3),          # out of range
                            (np.array([[0, 0], [1, 2]], np.int64), one[:2], 3),          # a self-loop
                            (edges[:2], np.array([1.0, -1.0], np.float32), 3),
                            (edges[:2], np.array([1.0, np.nan], np.float32), 3)):
        with pytest.raises(_lib.BtsbotHipError):
            _model_host(bad_e, bad_w, n, 2)
    with pytest.raises(ValueError):
        _model_host(edges, one, 4, 1)
    with pytest.raises(ValueError):
        _model_host(edges, one[:2], 4, 2)
    # the device entry points check their sizes before anything is launched
    L = _lib.lib()
    p = C.c_void_p(16)
    assert L.btsbot_cluster_offer_knn(p, p, -1, 4, 4, 2, p, None, 0, 0.0, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_cluster_offer_knn(p, p, 4, 0, 4, 1, p, None, 0, 0.0, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_cluster_offer_knn(p, p, 4, 65, 4, 1, p, None, 0, 0.0, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_cluster_offer_knn(p, p, 4, 4, 4, 6, p, None, 0, 0.0, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_cluster_offer_knn(p, p, 4, 4, 4, 2, p, None, 0, 1.0, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_cluster_offer_knn(None, p, 4, 4, 4, 2, p, None, 0, 0.0, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_cluster_offer_knn(p, p, 0, 4, 4, 2, p, None, 0, 0.0, p, p, p, p, None) == _lib.OK
    assert L.btsbot_cluster_offer_csr(p, p, p, p, 1 << 31, 4, 4, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_cluster_offer_csr(None, p, p, p, 2, 4, 4, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_cluster_offer_csr(p, p, p, p, 0, 4, 4, p, p, p, p, None) == _lib.OK
    assert L.btsbot_cluster_assign(p, p, 4, 4, p, p, 1, p, p, p, p, p, 0.0, p, p, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_cluster_assign(p, p, 4, 4, p, p, -1, p, p, p, p, p, 1.0, p, p, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_cluster_assign(None, p, 4, 4, p, p, 1, p, p, p, p, p, 1.0, p, p, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_cluster_assign(p, p, 0, 4, p, p, 1, p, p, p, p, p, 1.0, p, p, p, p, p, p, None) == _lib.OK


def test_python_argument_errors_come_before_the_device():
    import torch
    x = torch.zeros((8, 4))
    for kw in (dict(min_cluster_size=1), dict(min_cluster_size=True), dict(min_samples=0), dict(min_samples=66),
               dict(metric="manhattan"), dict(cluster_selection_method="best"), dict(allow_single_cluster=1),
               dict(method="cells"), dict(search_k=0), dict(search_k=65), dict(splits=-1), dict(method="grid"),
               dict(groups=torch.zeros(8))):
        with pytest.raises(ValueError):
            btsbot_amd.ClusterModel(x, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.ClusterModel(x)


def test_names_and_defaults():
    assert "ClusterModel" in btsbot_amd.__all__ and hasattr(btsbot_amd, "ClusterModel")
    for sym in ("btsbot_hdbscan_model", "btsbot_cluster_offer_knn", "btsbot_cluster_offer_csr", "btsbot_cluster_assign"):
        assert sym in _lib.SYMBOLS and hasattr(_lib.lib(), sym)
    sig = inspect.signature(btsbot_amd.ClusterModel.__init__).parameters
    assert [sig[k].default for k in ("min_cluster_size", "min_samples", "metric", "cluster_selection_method",
                                     "allow_single_cluster", "groups", "method", "search_k", "splits")] == \
        [5, None, "euclidean", "eom", False, None, "tiles", 8, 0]
    sig = inspect.signature(btsbot_amd.ClusterModel.predict).parameters
    assert list(sig)[1:6] == ["queries", "query_groups", "exclude_same_group", "search_k", "stats"]
    assert sig["search_k"].default is None and sig["return_details"].default is False
    assert inspect.signature(btsbot_amd.ClusterTree.outlier_scores).parameters["min_cluster_size"].default == 5
    from btsbot_amd.train import cluster_config
    assert cluster_config({"algorithm": "hdbscan", "outlier_scores": True}) == dict(
        algorithm="hdbscan", min_cluster_size=5, min_samples=None, on="map", method="tiles", outlier_scores=True)
    assert "outlier_scores" not in cluster_config({"algorithm": "hdbscan", "outlier_scores": False})
    for bad in ({"eps": 0.5, "outlier_scores": True}, {"algorithm": "hdbscan", "outlier_scores": 1}):
        with pytest.raises(ValueError, match=r"config\['embedding_clusters'\]"):
            cluster_config(bad)
