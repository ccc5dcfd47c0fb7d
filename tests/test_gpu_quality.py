"""GPU tests of the map quality (run with -m gpu on an MI355X): trustworthiness / continuity / map_quality against the
float64 restatement of tests/rank_ref.py -- inside the interval its band leaves on float rows and within that width of
scikit-learn, to the last bit on an integer lattice --, with rows=, groups= and both methods."""
import json

import numpy as np
import pytest
import torch

import btsbot_amd
import layout_ref
import radius_ref as R
import rank_ref as RR

pytestmark = pytest.mark.gpu

K = 15
_SETS = {}


def _cluster_maps():
    """the ten-cluster set with its PCA map and a shuffled map (a bad one), and the float64 figures, computed once"""
    if not _SETS:
        emb = R.clusters_32d(13)
        good = np.asarray(layout_ref.pca_init(emb, 1), np.float32)
        bad = good[np.random.default_rng(4).permutation(len(good))].copy()
        for name, y in (("pca", good), ("shuffled", bad)):
            ref = {}
            for swap in (False, True):
                lo, hi, open_sets = RR.trustworthiness64(emb, y, K, swap=swap, interval=True)
                ref[swap] = (lo, hi, open_sets, RR.trustworthiness64(emb, y, K, swap=swap))
            _SETS[name] = (emb, y, ref)
    return _SETS


def _gpu(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


@pytest.mark.parametrize("name", ("pca", "shuffled"))
def test_inside_the_float64_interval_and_near_sklearn(cuda, name):
    manifold = pytest.importorskip("sklearn.manifold")
    emb, y, ref = _cluster_maps()[name]
    te, ty = _gpu(cuda, emb, y)
    for swap, fn in ((False, btsbot_amd.trustworthiness), (True, btsbot_amd.continuity)):
        lo, hi, open_sets, mid = ref[swap]
        assert open_sets == 0, "a condition on the inputs: a neighbour set the fp32 band leaves open"
        got = fn(te, ty, K)
        a, b = (y, emb) if swap else (emb, y)
        want = manifold.trustworthiness(a.astype(np.float64), b.astype(np.float64), n_neighbors=K)
        print(f"{name} {'continuity' if swap else 'trustworthiness'}: device {got:.12f} in [{lo:.12f}, {hi:.12f}], "
              f"float64 {mid:.12f}, sklearn {want:.12f}")
        assert isinstance(got, float) and lo <= got <= hi
        assert abs(got - want) <= (hi - lo) + 1e-12
    q = btsbot_amd.map_quality(te, ty, K)
    assert (q["n"], q["k"], q["rows"]) == (512, K, 512)
    assert q["trustworthiness"] == btsbot_amd.trustworthiness(te, ty, K)
    assert q["continuity"] == btsbot_amd.continuity(te, ty, K)
    nb_e, nb_y = RR.neighbors64(emb, K)[0], RR.neighbors64(y, K)[0]
    recall = np.mean([len(set(a) & set(b)) / K for a, b in zip(nb_e.tolist(), nb_y.tolist())])
    assert abs(q["neighbor_recall"] - recall) <= 1e-12
    assert (q["trustworthiness"] > 0.9) == (name == "pca")


def test_lattice_rows_methods_sampling_and_groups_equal_the_restatement(cuda):
    emb, y = RR.lattice_3d(7)
    te, ty = _gpu(cuda, emb, y)
    assert btsbot_amd.trustworthiness(te, ty, K) == RR.trustworthiness64(emb, y, K)
    assert btsbot_amd.trustworthiness(te, ty, K, method="tiles") == RR.trustworthiness64(emb, y, K)
    assert btsbot_amd.continuity(te, ty, K) == RR.trustworthiness64(emb, y, K, swap=True)
    # a sample of the rows, repeated rows included
    rows = np.array([3, 77, 120, 9, 342, 0, 77], np.int64)
    (tr,) = _gpu(cuda, rows)
    for method in ("grid", "tiles"):
        t, pen = btsbot_amd.trustworthiness(te, ty, K, rows=tr, method=method, return_rows=True)
        assert t == RR.trustworthiness64(emb, y, K, rows=rows)
        assert pen.dtype == torch.int64 and pen.shape == (7,) and pen[1] == pen[6]
    assert btsbot_amd.continuity(te, ty, K, rows=tr) == RR.trustworthiness64(emb, y, K, rows=rows, swap=True)
    q = btsbot_amd.map_quality(te, ty, K, rows=tr)
    assert q["rows"] == 7 and q["n"] == 343 and q["trustworthiness"] == RR.trustworthiness64(emb, y, K, rows=rows)
    # groups: the seven rows above one (x, y) position are one object -- neighbours and ranks among other objects
    groups = (np.arange(343) // 7).astype(np.int64)
    (tg,) = _gpu(cuda, groups)
    for method in ("grid", "tiles"):
        assert btsbot_amd.trustworthiness(te, ty, K, groups=tg, method=method) == \
            RR.trustworthiness64(emb, y, K, groups=groups)
    assert btsbot_amd.continuity(te, ty, K, groups=tg) == RR.trustworthiness64(emb, y, K, groups=groups, swap=True)
    assert btsbot_amd.trustworthiness(te, ty, K, groups=tg, rows=tr) == \
        RR.trustworthiness64(emb, y, K, groups=groups, rows=rows)
    # rows that are not finite leave n, m and every list
    emb2, y2 = np.vstack([emb, emb[:2]]), np.vstack([y, y[:2]])
    emb2[343, 0], y2[344, 1] = np.nan, np.nan
    te2, ty2 = _gpu(cuda, emb2, y2)
    assert btsbot_amd.trustworthiness(te2, ty2, K) == RR.trustworthiness64(emb, y, K)
    with pytest.raises(ValueError, match="less than n / 2"):
        btsbot_amd.trustworthiness(te[:100], ty[:100], 50)
    with pytest.raises(ValueError, match="less than n / 2"):      # ... of the FINITE rows
        btsbot_amd.continuity(te2[300:], ty2[300:], 22)


def test_embedding_map_quality_and_the_json_of_a_run(cuda, tmp_path):
    from btsbot_amd import train
    emb, y, _ = _cluster_maps()["pca"]
    te, ty = _gpu(cuda, emb, y)
    m = btsbot_amd.EmbeddingMap.from_positions(te, ty, n_neighbors=K)
    assert m.quality() == btsbot_amd.map_quality(te, ty, K)
    assert m.quality(5, rows=torch.arange(0, 512, 8, device=cuda))["rows"] == 64
    path = train.write_map_quality(str(tmp_path / "mm_run"), te, ty, True, {"n_neighbors": K, "seed": 3})
    assert path.endswith("mm_run_umap_quality.json") and json.load(open(path)) == btsbot_amd.map_quality(te, ty, K)
    assert json.load(open(train.write_map_quality(str(tmp_path / "b"), te, ty, 5)))["k"] == 5
