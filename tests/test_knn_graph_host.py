"""KnnGraph without a GPU: the merge rule of tests/knn_graph_ref.py against the brute force on integer rows -- in every
group mode, with unfilled lists and with the offers cut at the old k-th distance, which proves the rule, the distinct-mode
argument and the radius cut of DESIGN.md section 4x --, the separated-row mask, and the argument errors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import knn_graph_ref as KG                                                # noqa: E402
import knn_group_ref as G                                                 # noqa: E402
import knn_ref as R                                                       # noqa: E402
import btsbot_amd                                                         # noqa: E402
from btsbot_amd import KnnGraph, MapIndex, NoveltyModel                   # noqa: E402

MODES = {"plain": (False, False), **G.MODES}


def _offers(x, n0, a, groups, exclude, r=None):
    """Row a's offers among the rows from n0 on, by brute force: (idx, dist fp32), ordered by (dist, index); r: only those
    with fp32 dist <= r."""
    d2 = R.dist64_matrix(x[a:a + 1], x[n0:], "euclidean")[0]
    dist = np.sqrt(d2).astype(np.float32)
    idx = np.arange(n0, len(x), dtype=np.int64)
    keep = np.ones(len(idx), bool)
    if exclude:
        keep &= groups[n0:] != groups[a]
    if r is not None:
        keep &= dist <= r
    idx, dist = idx[keep], dist[keep]
    o = np.lexsort((idx, dist))
    return idx[o], dist[o]


@pytest.mark.parametrize("cut", (False, True), ids=("all-offers", "cut-at-kth"))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n0,q,d,k,pattern", [(200, 100, 5, 15, "runs"), (200, 24, 5, 32, "mod40"), (7, 60, 33, 15, "mod3"),
                                              (50, 130, 5, 15, "one"), (129, 127, 5, 32, "distinct")])
def test_merged_brute_force_lists_are_the_brute_force_over_all_rows(n0, q, d, k, pattern, mode, cut):
    exclude, one = MODES[mode]
    x = R.make_rows("integer", n0 + q, d, 11)
    groups = G.make_groups(pattern, n0 + q, 3) if mode != "plain" else None
    kw = dict(exclude=exclude, one=one)
    old_i, old_d = KG.brute_lists(x[:n0], x[:n0], k, 0, None if groups is None else groups[:n0],
                                  None if groups is None else groups[:n0], **kw)
    want_i, want_d = KG.brute_lists(x[:n0], x, k, 0, None if groups is None else groups[:n0], groups, **kw)
    touched = 0
    for a in range(n0):
        r = None
        if cut:      # what KnnGraph._radii asks radius for: the last distance of a full list, +inf otherwise
            r = old_d[a, k - 1] if old_i[a, k - 1] >= 0 else np.float32(np.inf)
        oi, od = _offers(x, n0, a, groups, exclude, r)
        touched += len(oi) > 0
        got_i, got_d = KG.merge_lists(old_i[a], old_d[a], oi, od, k, groups, one)
        assert (got_i == want_i[a]).all(), f"row {a}: {got_i.tolist()} != {want_i[a].tolist()}"
        assert np.array_equal(got_d.view(np.int32), want_d[a].view(np.int32)), f"row {a}: distances"
    assert touched > 0 or (exclude and pattern == "one")     # (one group, excluded: nothing is eligible)


def test_merge_lists_ties_tail_and_nan_rows():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    # an offer that ties an old entry's distance goes behind it; the tail shrinks
    i, d = KG.merge_lists([3, 5, -1, -1], [1.0, 2.0, inf, inf], [10, 11], [1.0, 2.0], 4)
    assert i.tolist() == [3, 10, 5, 11] and d.tolist() == [1.0, 1.0, 2.0, 2.0]
    i, d = KG.merge_lists([3, 5, 7], [1.0, 2.0, 3.0], [10], [3.0], 3)
    assert i.tolist() == [3, 5, 7]
    # the distinct rule: an offer of group 0 before the old entry of group 0 replaces it, a later one is dropped
    groups = np.array([0, 1, 2, 0, 1, 2, 3], np.int64)
    i, d = KG.merge_lists([0, 1, -1], [1.0, 2.0, inf], [3, 4, 5, 6], [0.5, 2.5, 3.0, 3.5], 3, groups, True)
    assert i.tolist() == [3, 1, 5] and d.tolist() == [0.5, 2.0, 3.0]
    i, d = KG.merge_lists([-1, -1], [nan, nan], [4], [0.0], 2)
    assert i.tolist() == [-1, -1] and np.isnan(d).all()


def test_separated_rows_sees_a_tie_at_the_kth_place():
    x = np.zeros((6, 4), np.float32)
    x[:, 0] = [0, 1, 2, 4, 7, 7]         # row 0's distances: 1, 2, 4, 7, 7
    sep = KG.separated_rows(x, 4)
    assert not sep[0]                    # the 4th and the 5th candidate tie
    assert KG.separated_rows(x, 3)[0] and KG.separated_rows(x, 5).all()
    x[5, 0] = np.nan
    assert KG.separated_rows(x, 4).all()


def test_shares_of_the_gpu_tests_cases_stay_under_the_cap():
    """The non-separated share of every set tests/test_gpu_knn_graph.py holds to the rebuild (its cap: 5 %)."""
    for n, d, k, pattern, mode in ((468, 32, 15, None, "plain"), (256, 5, 64, None, "plain"), (70, 33, 15, None, "plain"),
                                   (430, 32, 20, None, "plain"), (468, 32, 15, "runs", "exclude"),
                                   (468, 32, 15, "mod40_hi32", "distinct"), (468, 32, 32, "runs_hi32", "exclude+distinct")):
        groups = None if pattern is None else G.make_groups(pattern, n, 7)
        sep = KG.separated_rows(R.make_rows("normal", n, d, 7), k, "euclidean", groups, *MODES[mode])
        assert 1.0 - sep.mean() <= 0.05, (n, d, k, pattern, 1.0 - sep.mean())
    # the set NoveltyModel(keep_graph=True) is held to a fresh fit on: no row inside the band
    assert KG.separated_rows(R.make_rows("normal", 430, 5, 7), 15).all()


# ---- argument errors that need no GPU --------------------------------------------------------------------------------
def test_a_mapindex_is_refused():
    m = object.__new__(MapIndex)
    with pytest.raises(ValueError, match="MapIndex"):
        KnnGraph(m, 5)
    with pytest.raises(ValueError, match="MapIndex"):
        NoveltyModel(m, 5, keep_graph=True)


def test_groups_beside_an_index_are_refused():
    index = object.__new__(btsbot_amd.EmbeddingIndex)
    index.metric, index._groups, index._n = "euclidean", None, 0
    with pytest.raises(ValueError, match="groups= next to an index"):
        KnnGraph(index, 5, groups=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="metric"):
        KnnGraph(index, 5, "cosine")


@pytest.mark.parametrize("k", (0, 65, 2.0, True))
def test_bad_k(k):
    with pytest.raises(ValueError, match="k must be"):
        KnnGraph(torch.zeros(4, 3), k)


def test_bad_mode_splits_metric_and_the_distinct_cap():
    rows, groups = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="group_mode"):
        KnnGraph(rows, 5, group_mode="collapse")
    with pytest.raises(ValueError, match="splits"):
        KnnGraph(rows, 5, splits=33)
    with pytest.raises(ValueError, match="metric"):
        KnnGraph(rows, 5, "manhattan")
    with pytest.raises(ValueError, match="one_per_group holds k <= 32"):
        KnnGraph(rows, 33, groups=groups, group_mode="distinct")
    with pytest.raises(ValueError, match="one_per_group holds k <= 32"):
        KnnGraph(rows, 33, groups=groups, group_mode="exclude+distinct")
    with pytest.raises(ValueError, match="keep_graph"):
        NoveltyModel(rows, 5, keep_graph=1)


def test_update_without_keep_graph_names_the_switch():
    model = object.__new__(NoveltyModel)
    model.graph = None
    with pytest.raises(RuntimeError, match="keep_graph=True"):
        model.update()


def test_cpu_tensors_have_no_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KnnGraph(torch.zeros(4, 3), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KnnGraph(torch.zeros(4, 3), 2, groups=torch.zeros(4, dtype=torch.int64), group_mode="distinct")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NoveltyModel(torch.zeros(4, 3), 2, keep_graph=True)
