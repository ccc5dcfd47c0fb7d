"""CPU-side checks of the local outlier factor (no GPU call is made): the float64 restatement the GPU tests hold the
kernels to IS scikit-learn's LOF, stays within the fp32 bound on the device's distances, and shows what groups are for;
the argument errors, the exported symbols and the opt-in key of run_training."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import lof_ref as R          # noqa: E402
import radius_ref as RR      # noqa: E402

import btsbot_amd            # noqa: E402
from btsbot_amd import _lib  # noqa: E402

SEEDS = (21, 22, 23)
KS = (5, 20)
SETS = [(name, seed) for name in ("clusters_32d", "blobs_2d") for seed in SEEDS]


def _sklearn_lof():
    from sklearn.neighbors import LocalOutlierFactor
    return LocalOutlierFactor


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


@pytest.fixture(scope="module")
def sets():
    """name, seed -> (X fp32, new rows fp32, float64 distance matrices bank x bank and new x bank)"""
    out = {}
    for name, seed in SETS:
        x = getattr(RR, name)(seed)
        q = R.perturbed_draws(x, seed)
        out[name, seed] = (x, q, R.distances64(x, x), R.distances64(q, x))
    return out


# ---- 1. the restatement is scikit-learn's LOF ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,seed", SETS)
def test_the_restatement_is_sklearns_lof_in_float64(sets, name, seed, k):
    """Float64 distances, the kernel's sum order: what is left against scikit-learn is the order of float64 sums of at
    most 64 terms, k 2^-52 relative -- 1e-12 holds it with room."""
    x, q, dxx, dqx = sets[name, seed]
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    idx, dist = R.knn64(dxx, k, self_offset=0)
    kdist, lrd, lof = R.lof_fit64(idx, dist)
    LocalOutlierFactor = _sklearn_lof()
    want = -LocalOutlierFactor(n_neighbors=k, algorithm="brute").fit(x64).negative_outlier_factor_
    print(f"{name} seed {seed} k {k}: fit, largest relative difference {_rel(lof, want):.3e}")
    assert _rel(lof, want) <= 1e-12
    qi, qd = R.knn64(dqx, k)
    _, s = R.lof_score64(qi, qd, kdist, lrd)
    want_s = -LocalOutlierFactor(n_neighbors=k, algorithm="brute", novelty=True).fit(x64).score_samples(q64)
    print(f"{name} seed {seed} k {k}: score of {len(q)} new rows, largest relative difference {_rel(s, want_s):.3e}")
    assert s.shape == (130,) and _rel(s, want_s) <= 1e-12


# ---- 2. on the device's fp32 distances --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,seed", SETS)
def test_fp32_direct_form_distances_stay_within_the_bound(sets, name, seed, k):
    """The same comparison on fp32 direct-form distances (emulated): 4 (D + 2) 2^-24 -- a ratio of means of ratios of
    distances, each carrying at most (D + 2) / 2 fp32 roundings, twice over.  The neighbour SETS equal scikit-learn's
    first: a swapped neighbour would be a different question, not a rounding."""
    x, q, _, _ = sets[name, seed]
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    bound = R.fp32_bound(x.shape[1])
    LocalOutlierFactor = _sklearn_lof()
    est = LocalOutlierFactor(n_neighbors=k, algorithm="brute", novelty=True).fit(x64)
    idx, dist = R.knn(R.distances32(x, x), k, self_offset=0)
    assert all(set(a) == set(b) for a, b in zip(idx.tolist(), est.kneighbors(return_distance=False).tolist()))
    kdist, lrd, lof = R.lof_fit(idx, dist)
    want = -est.negative_outlier_factor_
    print(f"{name} seed {seed} k {k}: fit on fp32 distances, largest relative difference {_rel(lof, want):.3e} "
          f"(bound {bound:.3e})")
    assert _rel(lof, want) <= bound
    qi, qd = R.knn(R.distances32(q, x), k)
    assert all(set(a) == set(b) for a, b in zip(qi.tolist(), est.kneighbors(q64, return_distance=False).tolist()))
    _, s = R.lof_score(qi, qd, kdist, lrd)
    want_s = -est.score_samples(q64)
    print(f"{name} seed {seed} k {k}: score on fp32 distances, largest relative difference {_rel(s, want_s):.3e}")
    assert _rel(s, want_s) <= bound


def test_a_block_of_duplicates_has_lrd_1e10_and_lof_1_as_in_sklearn():
    k = 5
    x = RR.clusters_32d(24, n=64)
    x[:k + 1] = x[0]
    idx, dist = R.knn(R.distances32(x, x), k, self_offset=0)
    _, lrd, lof = R.lof_fit(idx, dist)
    assert (lrd[:k + 1] == 1e10).all() and (lof[:k + 1] == 1.0).all()
    with pytest.warns(UserWarning, match="Duplicate values"):
        want = -_sklearn_lof()(n_neighbors=k, algorithm="brute").fit(x.astype(np.float64)).negative_outlier_factor_
    assert (want[:k + 1] == 1.0).all()


def test_fewer_than_k_neighbours_and_absent_entries():
    """m < k: the present entries alone count; an index out of range is no entry; m = 0 is NaN throughout."""
    idx = np.array([[1, 2, -1], [0, 2, 7], [-1, -1, -1], [0, 1, 2]], np.int64)      # (7 is out of range for n = 4)
    dist = np.array([[1.0, 2.0, np.inf], [1.0, 3.0, 0.5], [np.nan] * 3, [4.0, 5.0, 6.0]], np.float32)
    kdist, lrd, lof = R.lof_fit(idx, dist)
    assert kdist.tolist()[:2] == [2.0, 3.0] and np.isnan(kdist[2]) and kdist[3] == 6.0
    assert np.isnan(lrd[2]) and np.isnan(lof[2])
    # row 0: reach = max(1, kdist(1) = 3), max(2, kdist(2) = NaN -> 2)
    assert lrd[0] == 1.0 / ((3.0 + 2.0) / 2.0 + 1e-10)
    assert np.isnan(lof[[0, 1, 3]]).all()                   # a NaN neighbour lrd (row 2's) propagates
    # new rows against that bank: the out-of-range entry and the tail do not count
    own, s = R.lof_score(np.array([[0, 3, 9], [1, -1, -1]], np.int64),
                         np.array([[1.0, 7.0, 0.1], [0.25, np.inf, np.inf]], np.float32), kdist, lrd)
    assert own[0] == 1.0 / ((2.0 + 7.0) / 2.0 + 1e-10) and own[1] == 1.0 / (3.0 / 1.0 + 1e-10)
    assert s[0] == (lrd[0] / own[0] + lrd[3] / own[0]) / 2.0 and s[1] == (lrd[1] / own[1]) / 1.0


# ---- 3. the masking case ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (31, 32, 33))
def test_many_epochs_mask_a_far_object_until_its_own_alerts_are_left_out(seed):
    x, obj, planted = R.masking_set(seed)
    d = R.distances32(x, x)
    fin = np.ones(len(x), bool)
    plain = R.lof_fit(*R.knn(d, 4, self_offset=0, finite_b=fin))[2]
    grouped = R.lof_fit(*R.knn(d, 4, self_offset=0, qgroups=obj, bgroups=obj))[2]
    print(f"seed {seed}: planted alerts ungrouped <= {plain[planted].max():.3f}, own object excluded >= "
          f"{grouped[planted].min():.2f}; all others <= {plain[~planted].max():.3f} and <= {grouped[~planted].max():.3f}")
    assert planted.sum() == 15
    assert (plain[planted] < 1.5).all()                       # four siblings at 1e-3: as dense as its neighbours
    assert (grouped[planted] > 3).all() and (grouped[~planted] < 2).all()


# ---- 4. argument errors -------------------------------------------------------------------------------------------------
def _fake_index(groups):
    index = btsbot_amd.EmbeddingIndex.__new__(btsbot_amd.EmbeddingIndex)      # no device: the checks come first
    index.metric, index._n, index._groups, index.device = "euclidean", 3, groups, torch.device("cpu")
    return index


def test_argument_errors_are_value_errors():
    x = torch.zeros(10, 8)
    for k in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError, match="n_neighbors"):
            btsbot_amd.local_outlier_factor(x, k)
        with pytest.raises(ValueError, match="n_neighbors"):
            btsbot_amd.NoveltyModel(x, k)
    with pytest.raises(ValueError, match="group_mode"):
        btsbot_amd.local_outlier_factor(x, 5, groups=torch.zeros(10, dtype=torch.int64), group_mode="leave-out")
    with pytest.raises(ValueError, match="group_mode"):
        btsbot_amd.NoveltyModel(x, 5, group_mode="leave-out")
    with pytest.raises(ValueError, match="index's own groups"):
        btsbot_amd.NoveltyModel(_fake_index(torch.zeros(3, dtype=torch.int64)), 2, groups=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="metric"):
        btsbot_amd.NoveltyModel(_fake_index(None), 2, metric="cosine")
    with pytest.raises(ValueError, match="metric"):
        btsbot_amd.local_outlier_factor(x, 5, metric="manhattan")
    with pytest.raises(ValueError, match="knn"):
        btsbot_amd.local_outlier_factor(None, 5, knn=(torch.zeros(4, 5, dtype=torch.int32), torch.zeros(4, 5)))
    with pytest.raises(ValueError, match="knn"):
        btsbot_amd.local_outlier_factor(None, 5, knn=torch.zeros(4, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.local_outlier_factor(x, 5)
    model = btsbot_amd.NoveltyModel.__new__(btsbot_amd.NoveltyModel)
    model.lof = model.kdist = torch.ones(4, dtype=torch.float64)
    for c in (0, 0.0, 0.51, -0.1, 1, True, "1%", float("nan")):
        with pytest.raises(ValueError, match="contamination"):
            model.threshold(c)


def test_kth_neighbor_distance_is_the_last_present_distance():
    idx = torch.tensor([[3, 1, 2], [0, 2, -1], [-1, -1, -1]])
    dist = torch.tensor([[0.5, 1.0, 1.5], [2.0, 2.5, float("inf")], [float("nan")] * 3])
    got = btsbot_amd.kth_neighbor_distance(idx, dist)
    assert got.dtype == torch.float32 and got[:2].tolist() == [1.5, 2.5] and torch.isnan(got[2])
    with pytest.raises(ValueError):
        btsbot_amd.kth_neighbor_distance(idx.to(torch.int32), dist)


# ---- 5. exports ---------------------------------------------------------------------------------------------------------
def test_the_lof_symbols_and_names_are_exported():
    raw, L = C.CDLL(_lib.LIB_PATH), _lib.lib()
    for s in ("btsbot_lof_fit", "btsbot_lof_score"):
        assert s in _lib.SYMBOLS and hasattr(raw, s), s
    assert len(L.btsbot_lof_fit.argtypes) == 8 and len(L.btsbot_lof_score.argtypes) == 10
    for name in ("novelty", "NoveltyModel", "local_outlier_factor", "kth_neighbor_distance"):
        assert name in btsbot_amd.__all__ and hasattr(btsbot_amd, name)


def test_the_c_entry_points_refuse_bad_arguments_before_any_device_call():
    L = _lib.lib()
    p = C.c_void_p(256)      # never dereferenced: every call below is refused, or has nothing to do
    bad = _lib.ERR_INVALID_ARG
    for k in (0, 65, -1):
        assert L.btsbot_lof_fit(p, p, 4, k, p, p, p, None) == bad
        assert b"btsbot_lof_fit" in L.btsbot_last_error()
        assert L.btsbot_lof_score(p, p, 4, k, p, p, 9, p, p, None) == bad
        assert b"btsbot_lof_score" in L.btsbot_last_error()
    assert L.btsbot_lof_fit(p, p, -1, 5, p, p, p, None) == bad and L.btsbot_lof_score(p, p, 4, 5, p, p, -1, p, p, None) == bad
    assert L.btsbot_lof_fit(p, p, 4, 5, None, p, p, None) == bad and b"NULL" in L.btsbot_last_error()
    assert L.btsbot_lof_fit(None, p, 4, 5, p, p, p, None) == bad
    assert L.btsbot_lof_score(p, p, 4, 5, p, p, 9, p, None, None) == bad and b"NULL" in L.btsbot_last_error()
    assert L.btsbot_lof_score(p, p, 4, 5, None, p, 9, p, p, None) == bad
    assert L.btsbot_lof_fit(p, p, 4, 5, C.c_void_p(260), p, p, None) == bad and b"misaligned" in L.btsbot_last_error()
    assert L.btsbot_lof_score(p, C.c_void_p(258), 4, 5, p, p, 9, p, p, None) == bad
    assert L.btsbot_lof_fit(None, None, 0, 5, None, None, None, None) == _lib.OK           # nothing to do: no launch
    assert L.btsbot_lof_score(None, None, 0, 5, None, None, 9, None, None, None) == _lib.OK


# ---- 6. run_training: the new key is opt-in ----------------------------------------------------------------------------
def test_run_training_writes_the_lof_file_only_on_request():
    import inspect
    from btsbot_amd import train
    src = inspect.getsource(train.write_embeddings)
    src = src[src.index('"""', src.index('"""') + 3):]               # the code behind the docstring
    gate = src.index('config.get("embedding_novelty")')
    assert src.index('np.save(stem + ".npy", out)') < gate          # the .npy and .csv are written as before, first
    assert src.index('to_csv(stem + ".csv"') < gate
    assert src.index("_lof.npy") > gate and src.index("local_outlier_factor") > gate
    assert src[gate:].startswith('config.get("embedding_novelty")\n    if nov:')
    assert "embedding_novelty" not in inspect.getsource(train.run_training)    # report.json has no part in it
