"""HDBSCAN without a GPU: the float64 restatement (tests/hdbscan_ref.py) against scikit-learn, its invariance and
robustness on the sets the device tests use, and the library's host pass ``btsbot_hdbscan_tree`` through ctypes against
the restatement, exactly."""
import functools
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hdbscan_ref as R                                                   # noqa: E402
import btsbot_amd                                                         # noqa: E402
from btsbot_amd import _lib                                               # noqa: E402
from btsbot_amd.hdbscan import _tree_host                                 # noqa: E402


@functools.lru_cache(maxsize=None)
def _set(name):
    kind, _, seed = name.partition(":")
    if kind == "32d":
        return R.blobs_32d(int(seed)), None
    if kind == "2d":
        return R.blobs_2d(int(seed)), None
    if kind == "lattice":
        return R.lattice(), None
    if kind == "clumps":
        return R.clumps_2d(), None
    if kind == "70d":
        return R.blobs_70d(), None
    if kind == "bad":
        return R.blobs_32d_with_bad_rows(), None
    return R.object_set()


@functools.lru_cache(maxsize=None)
def _dist(name):
    return R.dist_matrix(_set(name)[0])


@functools.lru_cache(maxsize=None)
def _mst(name, min_samples, tie="first"):
    core, W = R.mutual_reachability(_dist(name), min_samples)
    return R.mst(W, tie)


SETS_32D = [f"32d:{s}" for s in R.SEEDS_32D]
SETS_2D = [f"2d:{s}" for s in R.SEEDS_2D]
SMALL = SETS_32D + SETS_2D + ["lattice", "objects"]


def _perms(n, count=3):
    return [np.random.default_rng(900 + i).permutation(n) for i in range(count)]


# ---- 1. the restatement is scikit-learn's HDBSCAN ---------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS_32D)
@pytest.mark.parametrize("mcs,ms", R.PAIRS)
def test_restatement_is_sklearn_on_32d(name, mcs, ms):
    from sklearn.cluster import HDBSCAN
    X = _set(name)[0].astype(np.float64)
    sk = HDBSCAN(min_cluster_size=mcs, min_samples=ms, algorithm="brute").fit(X)
    for perm in _perms(len(X)):       # scikit-learn agrees with itself on this set, so it can be the yardstick
        again = HDBSCAN(min_cluster_size=mcs, min_samples=ms, algorithm="brute").fit(X[perm])
        assert R.same_partition(sk.labels_[perm], again.labels_)
        assert np.abs(sk.probabilities_[perm] - again.probabilities_).max() <= 1e-6
    ref = R.hdbscan_ref(_dist(name), mcs, ms)
    worst = float(np.abs(ref["prob"] - sk.probabilities_).max())
    print(f"{name} ({mcs}, {ms}): {ref['labels'].max() + 1} clusters, max |prob - sklearn| = {worst:.2e}")
    assert sk.labels_.max() >= 1
    assert R.same_partition(ref["labels"], sk.labels_)
    assert worst <= 1e-6


@pytest.mark.parametrize("name", SETS_2D)
def test_restatement_against_sklearn_on_2d_is_reported(name):
    """On 2-D blobs scikit-learn's labels depend on the row order (tied weights, a binary dendrogram): only counted."""
    from sklearn.cluster import HDBSCAN
    X = _set(name)[0].astype(np.float64)
    for mcs, ms in R.PAIRS:
        sk = HDBSCAN(min_cluster_size=mcs, min_samples=ms, algorithm="brute").fit(X)
        ref = R.hdbscan_ref(_dist(name), mcs, ms)
        print(f"{name} ({mcs}, {ms}): same partition {R.same_partition(ref['labels'], sk.labels_)}, "
              f"{int((np.abs(ref['prob'] - sk.probabilities_) > 1e-6).sum())} probabilities differ by more than 1e-6")


# ---- 2. invariance under row permutation ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_restatement_does_not_depend_on_the_row_order(name):
    D = _dist(name)
    for mcs, ms in R.PAIRS:
        ref = R.hdbscan_ref(D, mcs, ms)
        for perm in _perms(len(D)):
            got = R.hdbscan_ref(D[np.ix_(perm, perm)], mcs, ms)
            assert R.same_partition(ref["labels"][perm], got["labels"]), (name, mcs, ms)
            assert np.array_equal(ref["prob"][perm], got["prob"]), (name, mcs, ms)


# ---- 3. the sets of the device's equality tests are robust ------------------------------------------------------------
def _scaled(D, dim, seed):
    s = np.random.default_rng(seed).uniform(-1, 1, size=D.shape)
    s = np.triu(s, 1)
    return D * (1 + (s + s.T) * R.band(dim))


# (the lattice is left out on purpose: its fp32 distances are exact on the device, and any scaling breaks its ties)
@pytest.mark.parametrize("name,pairs", [(n, R.PAIRS) for n in SETS_32D + SETS_2D] +
                         [("clumps", ((10, 5),)), ("70d", ((10, 5),)), ("bad", ((10, 5),))])
def test_equality_sets_keep_their_labels_under_fp32_noise(name, pairs):
    X, _ = _set(name)
    D = _dist(name)
    for mcs, ms in pairs:
        ref = R.hdbscan_ref(D, mcs, ms)
        assert ref["labels"].max() >= 1
        for draw in range(5):
            got = R.hdbscan_ref(_scaled(D, X.shape[1], 50 + draw), mcs, ms)
            assert np.array_equal(ref["labels"], got["labels"]), (name, mcs, ms, draw)


def test_object_set_keeps_its_labels_under_fp32_noise():
    X, obj = _set("objects")
    D = _dist("objects")
    for groups in (None, obj):
        ref = R.hdbscan_ref(D, 5, 5, groups=groups)
        for draw in range(5):
            got = R.hdbscan_ref(_scaled(D, X.shape[1], 70 + draw), 5, 5, groups=groups)
            assert np.array_equal(ref["labels"], got["labels"]), draw


# ---- 4. btsbot_hdbscan_tree equals the restatement --------------------------------------------------------------------
def _same_tree(got, ref):
    lab, prob, cond = got
    assert np.array_equal(lab, ref["labels"])
    assert np.array_equal(prob.view(np.int64), ref["prob"].view(np.int64))
    for a, b in zip(cond, ref["condensed"]):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("method", ("eom", "leaf"))
def test_library_tree_equals_the_restatement(name, method):
    n = len(_dist(name))
    edges, weights = _mst(name, 5)
    seen = set()
    for mcs in (2, 5, 15):
        for single in (False, True):
            ref = R.tree(edges, weights, n, mcs, method, single)
            _same_tree(_tree_host(edges, weights.astype(np.float32), n, mcs, method, single), ref)
            seen.add(int(ref["labels"].max()) + 1)
    print(f"{name} {method}: cluster counts met {sorted(seen)}")


@pytest.mark.parametrize("method", ("eom", "leaf"))
def test_library_tree_does_not_depend_on_edge_order_or_on_which_mst(method):
    n = len(_dist("lattice"))
    edges, weights = _mst("lattice", 5)
    other_e, other_w = _mst("lattice", 5, "last")
    assert np.array_equal(np.sort(weights), np.sort(other_w))
    assert {tuple(sorted(e)) for e in edges.tolist()} != {tuple(sorted(e)) for e in other_e.tolist()}
    for mcs in (2, 5, 15):
        ref = R.tree(edges, weights, n, mcs, method)
        for seed in range(3):
            order = np.random.default_rng(seed).permutation(len(edges))
            flip = np.random.default_rng(seed).integers(0, 2, len(edges)).astype(bool)
            shuffled = np.where(flip[:, None], edges[:, ::-1], edges)[order]
            _same_tree(_tree_host(shuffled, weights[order].astype(np.float32), n, mcs, method), ref)
        _same_tree(_tree_host(other_e, other_w.astype(np.float32), n, mcs, method), ref)
        _same_tree((lambda o: (o["labels"], o["prob"], o["condensed"]))(R.tree(other_e, other_w, n, mcs, method)), ref)


# ---- 5, 6. degenerate weights -----------------------------------------------------------------------------------------
def test_a_single_weight_is_one_multiway_node():
    n = 9
    edges = np.array([[i, i + 1] for i in range(n - 1)], np.int64)
    w = np.ones(n - 1, np.float32)
    lab, prob, cond = _tree_host(edges, w, n, 3)
    assert (lab == -1).all() and (prob == 0).all()
    assert np.array_equal(cond[0], np.full(n, n)) and np.array_equal(cond[1], np.arange(n)) and (cond[2] == 1.0).all()
    lab, prob, _ = _tree_host(edges, w, n, 3, "eom", True)
    assert (lab == 0).all() and (prob == 1).all()
    lab, prob, _ = _tree_host(edges, w, n, 3, "leaf", True)
    assert (lab == 0).all() and (prob == 1).all()
    for method in ("eom", "leaf"):
        for single in (False, True):
            _same_tree(_tree_host(edges, w, n, 3, method, single), R.tree(edges, w, n, 3, method, single))


def test_zero_weights_take_the_largest_finite_lambda():
    """min_samples + 2 duplicates: their block of the tree has w = 0, and lambda there is 1 / the smallest positive weight"""
    ms = 4
    X = np.concatenate([np.zeros((ms + 2, 3)), R.blobs_32d(0)[:40, :3] + 5.0, [[30.0, 0.0, 0.0]]]).astype(np.float32)
    D = R.dist_matrix(X)
    ref = R.hdbscan_ref(D, 5, ms)
    assert (ref["weights"] == 0).sum() == ms + 1
    lam = ref["condensed"][2]
    assert np.isfinite(lam).all() and lam.max() == 1.0 / ref["weights"][ref["weights"] > 0].min()
    dup = ref["labels"][:ms + 2]
    assert dup[0] >= 0 and (dup == dup[0]).all() and (ref["prob"][:ms + 2] == 1.0).all()
    _same_tree(_tree_host(ref["edges"], ref["weights"].astype(np.float32), len(X), 5), ref)
    # all weights zero: lambda = 1
    edges = np.array([[0, 1], [1, 2], [2, 3]], np.int64)
    lab, prob, cond = _tree_host(edges, np.zeros(3, np.float32), 4, 2, "eom", True)
    assert (lab == 0).all() and (prob == 1).all() and (cond[2] == 1.0).all()


def test_rows_without_an_edge_are_noise():
    edges, weights = _mst("32d:0", 5)
    n = len(_dist("32d:0"))
    lab, prob, _ = _tree_host(edges, weights.astype(np.float32), n + 3, 10)
    ref = R.tree(edges, weights, n, 10)
    assert np.array_equal(lab[:n], ref["labels"]) and (lab[n:] == -1).all() and (prob[n:] == 0).all()


# ---- 7. interface -----------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device():
    import torch
    x = torch.zeros((8, 4))
    for kw in (dict(min_cluster_size=1), dict(min_cluster_size=2.0), dict(min_cluster_size=True), dict(min_samples=0),
               dict(min_samples=66), dict(metric="manhattan"), dict(cluster_selection_method="best"),
               dict(allow_single_cluster=1), dict(method="cells"), dict(search_k=0), dict(search_k=65), dict(splits=-1),
               dict(method="grid"), dict(groups=torch.zeros(8))):
        with pytest.raises(ValueError):
            btsbot_amd.hdbscan(x, **kw)
    with pytest.raises(ValueError):
        btsbot_amd.hdbscan(torch.zeros((8, 2)), method="grid", metric="cosine")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.hdbscan(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.mutual_reachability_mst(x, 5)
    with pytest.raises(ValueError):
        btsbot_amd.mutual_reachability_mst(x, 5, stats=[])
    with pytest.raises(ValueError):
        btsbot_amd.ClusterTree(object())
    edges = np.array([[0, 1], [1, 2]], np.int64)
    one = np.ones(2, np.float32)
    with pytest.raises(ValueError):
        _tree_host(edges, one, 3, 1)
    with pytest.raises(ValueError):
        _tree_host(edges, one, 3, 2, "best")
    for bad_e, bad_w, n in ((np.array([[0, 1], [1, 0]], np.int64), one, 3),          # a cycle
                            (np.array([[0, 1], [2, 3]], np.int64), one, 4),          # two trees
                            (np.array([[0, 1], [1, 3]], np.int64), one, 3),          # out of range
                            (np.array([[0, 0], [1, 2]], np.int64), one, 3),          # a self-loop
                            (edges, np.array([1.0, -1.0], np.float32), 3),
                            (edges, np.array([1.0, np.nan], np.float32), 3)):
        with pytest.raises(_lib.BtsbotHipError):
            _tree_host(bad_e, bad_w, n, 2)


def test_names_and_defaults():
    for name in ("hdbscan", "mutual_reachability_mst", "MutualReachabilityMST", "ClusterTree"):
        assert name in btsbot_amd.__all__ and hasattr(btsbot_amd, name)
    for sym in ("btsbot_mst_offer_knn", "btsbot_mst_offer_csr", "btsbot_mst_merge", "btsbot_hdbscan_tree"):
        assert sym in _lib.SYMBOLS and hasattr(_lib.lib(), sym)
    sig = inspect.signature(btsbot_amd.hdbscan).parameters
    assert [sig[k].default for k in ("min_cluster_size", "min_samples", "metric", "cluster_selection_method",
                                     "allow_single_cluster", "groups", "method", "search_k", "splits", "return_tree")] == \
        [5, None, "euclidean", "eom", False, None, "tiles", 8, 0, False]
    sig = inspect.signature(btsbot_amd.mutual_reachability_mst).parameters
    assert list(sig)[:6] == ["emb_or_index", "min_samples", "groups", "method", "search_k", "stats"]
    # the default algorithm of config['embedding_clusters'] is still DBSCAN, with eps required
    from btsbot_amd.train import cluster_config
    assert cluster_config({"eps": 0.5}) == dict(algorithm="dbscan", eps=0.5, min_samples=5, on="map", method="tiles")
    with pytest.raises(ValueError, match=r"config\['embedding_clusters'\]"):
        cluster_config({"min_samples": 3})
    with pytest.raises(ValueError, match=r"config\['embedding_clusters'\]"):
        cluster_config({"algorithm": "hdbscan", "eps": 0.5})
    assert cluster_config({"algorithm": "hdbscan"}) == dict(algorithm="hdbscan", min_cluster_size=5, min_samples=None,
                                                            on="map", method="tiles")
