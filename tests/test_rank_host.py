"""Host tests of the neighbour ranks and the map quality (no GPU): the checker of tests/rank_ref.py against the emulated
passes and their seeded faults, the float64 trustworthiness against scikit-learn, the argument checks and the C ABI's
refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import btsbot_amd
from btsbot_amd import _lib
import knn_ref as K
import rank_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _integer_set(dim, seed=0):
    q, b = K.make_rows("integer", 40, dim, 5 + seed), K.make_rows("integer", 300, dim, 6 + seed)
    targets = RR.random_targets(40, 300, 6, 7 + seed)
    targets[:, 5] = targets[:, 0]                            # a repeated target
    targets[:, 4] = np.arange(40)                            # the row itself (masked under self_offset = 0)
    return q, b, targets


# ---- the checker and the emulation
@pytest.mark.parametrize("dim", (5, 33, 528))
def test_checker_accepts_the_clean_emulation_on_integer_rows(dim):
    q, b, targets = _integer_set(dim)
    obj_q, obj_b = (np.arange(40) % 7).astype(np.int64), (np.arange(300) % 7).astype(np.int64)
    for splits, kw in ((1, {}), (3, {"self_offset": 0}), (2, {"qgroups": obj_q, "bgroups": obj_b})):
        stats = {}
        rank, dist = RR.emulate_ranks(q, b, targets, splits=splits, stats=stats, **kw)
        RR.check_ranks(q, b, targets, rank, dist, exact=True, **kw)
        assert stats["band"] > 0 and (rank >= 0).any()
    # the same ranks whatever the number of splits
    ref = RR.emulate_ranks(q, b, targets, splits=1)[0]
    assert all(np.array_equal(RR.emulate_ranks(q, b, targets, splits=s)[0], ref) for s in (2, 3, 0))


@pytest.mark.parametrize("fault", RR.FAULTS)
def test_checker_rejects_each_seeded_fault_on_the_tie_rich_set(fault):
    q, b, targets = _integer_set(33)
    kw = {"self_offset": 0}
    b[:40] = q                                               # the query rows ARE bank rows 0..39
    rank, dist = RR.emulate_ranks(q, b, targets, splits=3, **kw)
    RR.check_ranks(q, b, targets, rank, dist, exact=True, **kw)
    rank, dist = RR.emulate_ranks(q, b, targets, splits=3, fault=fault, **kw)
    with pytest.raises(AssertionError, match="rank"):
        RR.check_ranks(q, b, targets, rank, dist, exact=True, **kw)


@pytest.mark.parametrize("metric", ("euclidean", "cosine"))
@pytest.mark.parametrize("kind", K.KINDS)
def test_emulation_lies_in_the_interval_on_float_rows(kind, metric):
    for n_q, n, dim in ((30, 127, 5), (20, 200, 33), (8, 150, 528)):
        q, b = K.make_rows(kind, n_q, dim, 1000), K.make_rows(kind, n, dim, 2000)
        targets = RR.random_targets(n_q, n, 5, 3)
        targets[0, 0], targets[0, 1] = -1, n
        rank, dist = RR.emulate_ranks(q, b, targets, metric, splits=2)
        share, worst = RR.check_ranks(q, b, targets, rank, dist, metric)
        print(f"{kind} {metric} {n_q}x{n}x{dim}: open intervals {share:.4f}, worst distance error {worst:.3f} of the band")


def test_checker_covers_status_and_distance():
    q, b = K.make_rows("normal", 6, 5, 1), K.make_rows("normal", 50, 5, 2)
    q[2, 1], b[7, 0] = np.nan, np.inf
    targets = RR.random_targets(6, 50, 3, 1)
    targets[0] = [-1, 50, 7]
    rank, dist = RR.emulate_ranks(q, b, targets)
    assert (rank[0] == -1).all() and np.isnan(dist[0]).all() and (rank[2] == -1).all() and np.isnan(dist[2]).all()
    RR.check_ranks(q, b, targets, rank, dist)
    bad = rank.copy()
    bad[0, 0] = 0
    with pytest.raises(AssertionError, match="validity"):
        RR.check_ranks(q, b, targets, bad, dist)
    off = dist.copy()
    off[1, 1] *= np.float32(1 + 1e-4)
    with pytest.raises(AssertionError, match="distance"):
        RR.check_ranks(q, b, targets, rank, off)
    off = dist.copy()
    off[0, 0] = 1.0
    with pytest.raises(AssertionError, match="distance"):
        RR.check_ranks(q, b, targets, rank, off)


def test_selection_scores_are_exact_on_integer_rows():
    """what lets test_gpu_rank hold rank_of(query's rows) to arange(k) there: the emulated two-pass query returns the
    float64 (d^2, index) order, ties included"""
    for dim in (5, 33, 528):
        q, b = K.make_rows("integer", 30, dim, 5), K.make_rows("integer", 300, dim, 6)
        idx, dist = K.emulate(q, b, 15, splits=3)
        K.check_exact(q, b, idx, dist, 15)


# ---- the float64 restatement of trustworthiness is sklearn's
@pytest.mark.parametrize("metric", ("euclidean", "cosine"))
def test_trustworthiness_restatement_equals_sklearn(metric):
    manifold = pytest.importorskip("sklearn.manifold")
    import layout_ref
    import radius_ref as R
    emb = R.clusters_32d(21, 300)
    rng = np.random.default_rng(2)
    for y in (layout_ref.pca_init(emb, 1), rng.standard_normal((300, 2)).astype(np.float32)):
        y = np.asarray(y, np.float32)
        for k in (5, 15):
            want = manifold.trustworthiness(emb.astype(np.float64), y.astype(np.float64), n_neighbors=k, metric=metric)
            got = RR.trustworthiness64(emb, y, k, metric)
            assert abs(got - want) <= 1e-12, (k, got, want)
            lo, hi, open_sets = RR.trustworthiness64(emb, y, k, metric, interval=True)
            assert lo <= got <= hi and hi - lo < 1e-3
        # continuity is trustworthiness with the spaces swapped (the map is euclidean)
        if metric == "euclidean":
            want = manifold.trustworthiness(y.astype(np.float64), emb.astype(np.float64), n_neighbors=5)
            assert abs(RR.trustworthiness64(emb, y, 5, swap=True) - want) <= 1e-12


def test_trustworthiness_restatement_breaks_ties_by_index_and_takes_rows_and_groups():
    emb, y = RR.lattice_3d(5)
    t = RR.trustworthiness64(emb, y, 5)
    assert 0.5 < t < 1.0
    rows = np.array([3, 77, 120, 9])
    tr = RR.trustworthiness64(emb, y, 5, rows=rows)
    lo, hi, _ = RR.trustworthiness64(emb, y, 5, rows=rows, interval=True)
    assert lo < tr < hi                                       # tied distances are open to the interval, not to tr
    groups = (np.arange(125) // 5).astype(np.int64)           # the five rows of one (x, y) column share a group
    tg = RR.trustworthiness64(emb, y, 5, groups=groups)
    assert tg != t
    nb, _ = RR.neighbors64(y, 5, groups=groups)
    assert (groups[nb] != groups[:, None]).all()


# ---- arguments
def test_rank_arguments_are_checked_before_the_device_is_touched():
    q, b = torch.zeros(4, 3), torch.zeros(9, 3)
    tg = torch.zeros((4, 2), dtype=torch.int64)
    for bad in (torch.zeros((4, 2), dtype=torch.int32), torch.zeros(4, dtype=torch.int64), [[0, 1]] * 4,
                torch.zeros((3, 2), dtype=torch.int64), torch.zeros((4, 0), dtype=torch.int64),
                torch.zeros((4, 65), dtype=torch.int64)):
        with pytest.raises(ValueError, match="targets must be"):
            btsbot_amd.neighbor_ranks(q, b, bad)
    with pytest.raises(ValueError, match="splits"):
        btsbot_amd.neighbor_ranks(q, b, tg, splits=33)
    with pytest.raises(ValueError, match="metric"):
        btsbot_amd.neighbor_ranks(q, b, tg, metric="manhattan")
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="max_band"):
            btsbot_amd.neighbor_ranks(q, b, tg, max_band=bad)
    with pytest.raises(ValueError, match="need an index built with groups"):
        btsbot_amd.neighbor_ranks(q, b, tg, exclude_same_group=True, query_groups=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # valid arguments: only the device is missing
        btsbot_amd.neighbor_ranks(q, b, tg)
    assert "one_per_group" in btsbot_amd.EmbeddingIndex.rank_of.__doc__
    with pytest.raises(ValueError, match="one_per_group is not a rank mode"):
        btsbot_amd.EmbeddingIndex.rank_of(object.__new__(btsbot_amd.EmbeddingIndex), q, tg, one_per_group=True)


def test_quality_arguments_are_checked_before_the_device_is_touched():
    emb, y = torch.zeros(20, 3), torch.zeros(20, 2)
    for fn in (btsbot_amd.trustworthiness, btsbot_amd.continuity, btsbot_amd.map_quality):
        with pytest.raises(ValueError, match="less than n / 2"):
            fn(emb, y, 10)
        for bad in (0, 65, 2.0, True):
            with pytest.raises(ValueError, match="n_neighbors"):
                fn(emb, y, bad)
        with pytest.raises(ValueError, match="metric"):
            fn(emb, y, 5, metric="manhattan")
        with pytest.raises(ValueError, match="rows"):
            fn(emb, y, 5, rows=torch.zeros(3, dtype=torch.int32))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(emb, y, 5)
    with pytest.raises(ValueError, match="method"):
        btsbot_amd.trustworthiness(emb, y, 5, method="tree")


def test_a_run_writes_the_quality_json_and_keeps_the_key_from_embedding_layout(tmp_path, monkeypatch):
    import inspect
    import json
    from btsbot_amd import quality, train
    seen = {}

    def stub(emb, y, k, **kw):
        seen.update(k=k, **kw)
        return {"trustworthiness": 0.9, "continuity": 0.8, "neighbor_recall": 0.5, "n": 4, "k": k, "rows": 4}

    monkeypatch.setattr(quality, "map_quality", stub)
    path = train.write_map_quality(str(tmp_path / "mm_ConvNeXt_testing"), None, None, True, {"n_neighbors": 10, "seed": 1})
    assert os.path.basename(path) == "mm_ConvNeXt_testing_umap_quality.json" and json.load(open(path))["k"] == 10
    assert seen == {"k": 10, "metric": "euclidean", "groups": None}
    assert json.load(open(train.write_map_quality(str(tmp_path / "b"), None, None, 7)))["k"] == 7
    with pytest.raises(ValueError, match="quality"):
        train.write_map_quality(str(tmp_path / "c"), None, None, "yes")
    src = inspect.getsource(train.write_embeddings)
    assert src.index('kw.pop("quality"') < src.index("embedding_layout(emb_dev, **kw)") < src.index("write_map_quality(")


def test_the_rank_symbols_are_declared_exported_and_refuse_bad_arguments():
    header = open(os.path.join(ROOT, "include", "btsbot_hip.h")).read()
    raw, L = C.CDLL(_lib.LIB_PATH), _lib.lib()
    for name in ("btsbot_knn_rank_workspace", "btsbot_knn_rank_count", "btsbot_knn_rank_fill"):
        assert name in _lib.SYMBOLS and hasattr(raw, name)
        assert re.search(r"^(int|int64_t) " + name + r"\(", header, re.M), name
    for name in ("neighbor_ranks", "trustworthiness", "continuity", "map_quality", "quality"):
        assert name in btsbot_amd.__all__ and hasattr(btsbot_amd, name)
    assert hasattr(btsbot_amd.EmbeddingIndex, "rank_of") and hasattr(btsbot_amd.EmbeddingMap, "quality")
    bad = _lib.ERR_INVALID_ARG
    assert L.btsbot_knn_rank_workspace(0, 5, 3) == 0
    assert L.btsbot_knn_rank_workspace(3, 5, 2) == 512 + 256 + 12    # query image, thresholds, the rows' widest limits
    assert L.btsbot_knn_rank_workspace(3, 1025, 2) == bad and L.btsbot_knn_rank_workspace(3, 5, 65) == bad
    assert L.btsbot_knn_rank_workspace(3, 5, 0) == bad
    p = C.c_void_p(256)          # never dereferenced: every call below is refused first
    ws = 780

    def count(nq=4, nb=9, dim=3, metric=0, t=2, splits=1, flags=0, ws=ws, targets=p, qg=None, bg=None, dist=p):
        return L.btsbot_knn_rank_count(p, nq, p, p, nb, dim, metric, targets, t, -1, splits, qg, bg, flags, dist, p, p, p,
                                       ws, None)

    need = L.btsbot_knn_rank_workspace(4, 3, 2)
    assert count(splits=0) == bad and b"splits" in L.btsbot_last_error()
    assert count(splits=33) == bad
    assert count(flags=2) == bad and b"rank modes" in L.btsbot_last_error()
    assert count(flags=1) == bad and b"query_group" in L.btsbot_last_error()
    assert count(metric=2) == bad and count(dim=0) == bad and count(t=0) == bad and count(t=65) == bad
    assert count(targets=None) == bad and b"NULL" in L.btsbot_last_error()
    assert count(ws=need - 1) == bad and b"workspace" in L.btsbot_last_error()
    assert count(ws=need, dist=None) == bad and b"NULL" in L.btsbot_last_error()
    assert count(nq=0) == _lib.OK
    fill = (p, 4, p, p, 9, 3, 0, p, 2, -1, 1, None, None, 0, p, p, p, p)
    assert L.btsbot_knn_rank_fill(*fill, -1, p, p, p, p, need, None) == bad and b"n_band" in L.btsbot_last_error()
    assert L.btsbot_knn_rank_fill(*fill, 0, p, p, p, p, need, None) == _lib.OK          # nothing to do
    assert L.btsbot_knn_rank_fill(*fill, 5, None, p, p, p, need, None) == bad
    assert L.btsbot_knn_rank_fill(*fill, 5, p, p, p, p, need - 1, None) == bad
