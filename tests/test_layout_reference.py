"""CPU: can the epoch bound of tests/test_gpu_layout.py (tests/layout_ref.py) see a subtly wrong epoch kernel?

The float64 restatement of one epoch takes one seeded fault at a time -- the mistakes a rewrite of layout_epoch_kernel is
likely to make -- and must then miss the bound |dy| <= c 2^-24 (|y| + alpha sum |term|) at the LARGEST c the bound may
ever take (EPOCH_C_LIMIT = 256), on a case of the GPU file.  The restatement without a fault, evaluated in fp32 instead
(positions, differences and sums rounded to fp32 after every epoch: another arithmetic than the device's, as far from
float64), is printed beside the bound and must stay inside it.
"""
import numpy as np
import pytest

import layout_ref as R

A, B = 1.5769434, 0.8950609


def _knn_case(n, k, seed):
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((n, 5)).astype(np.float32)
    g = R.fuzzy_graph(*R.knn_exact(emb, k))
    y = (4.0 * rng.standard_normal((n, 2))).astype(np.float32)
    return g, y


def _fire_case():
    """Weights 0.7 (fp32: just below) beside w_max = 1: 10 r = 6.9999999 in float64 but 7 in fp32, so epoch 10 fires in
    fp32 only (and epoch 11 in float64 only)."""
    n = 12
    pairs = {(i, i + 1): np.float32(0.7) for i in range(0, n - 1, 2)}
    pairs[(1, 2)] = np.float32(1.0)
    rng = np.random.default_rng(2)
    return R.graph_from_pairs(n, pairs), (3.0 * rng.standard_normal((n, 2))).astype(np.float32)


def _worst(g, y, n, n_epochs, rate, fault, seed=3):
    ref, scale = R.epoch(g, y, n, n_epochs, A, B, seed, rate)
    bad, _ = R.epoch(g, y, n, n_epochs, A, B, seed, rate, fault=fault)
    return R.epoch_ratio(bad, ref, scale)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_bound_catches_the_fault(fault):
    if fault == "fire_fp32":
        g, y = _fire_case()
        cases = [(g, y, 10, 200, 5), (g, y, 11, 200, 1)]
    elif fault == "no_self_check":
        # N = 2: half of all samples hit the vertex itself
        g = R.graph_from_pairs(2, {(0, 1): np.float32(1.0)})
        cases = [(g, np.array([[0.5, -0.25], [-1.0, 2.0]], dtype=np.float32), 1, 10, 5)]
    elif fault == "no_clip":
        # neighbours closer than the clip radius: both kinds of term exceed 4 before the clip
        g, y = _knn_case(65, 5, 1)
        cases = [(g, (y * np.float32(0.01)).astype(np.float32), 1, 10, 5)]
    else:
        g, y = _knn_case(65, 5, 1)
        cases = [(g, y, 1, 10, 5), (g, y, 100, 200, 1)]
    for g, y, n, n_epochs, rate in cases:
        ratio = _worst(g, y, n, n_epochs, rate, fault)
        print(f"{fault}: epoch {n}/{n_epochs}, rate {rate}: {ratio:.3g} x 2^-24 (bound at most {R.EPOCH_C_LIMIT:g})")
        assert ratio > 10 * R.EPOCH_C_LIMIT, (fault, n, n_epochs, rate, ratio)
        with pytest.raises(AssertionError, match="epoch error"):
            bad, _ = R.epoch(g, y, n, n_epochs, A, B, 3, rate, fault=fault)
            ref, scale = R.epoch(g, y, n, n_epochs, A, B, 3, rate)
            R.check_epoch(bad, ref, scale, c=R.EPOCH_C_LIMIT)


def test_faults_that_need_a_rate_are_silent_without_one():
    """negative_sample_rate = 0: no sample to drop and no self sample, so those two restatements ARE the reference --
    the harness does not report a difference where there is none."""
    g, y = _knn_case(65, 5, 1)
    for fault in ("drop_sample", "no_self_check"):
        assert _worst(g, y, 1, 10, 0, fault) == 0.0


def test_rounding_to_fp32_stays_inside_the_bound():
    for g, y in (_knn_case(65, 5, 1), _knn_case(300, 15, 2), (R.hub_graph(300, 4), _knn_case(300, 5, 4)[1])):
        for n, n_epochs in ((1, 10), (5, 10), (100, 200), (200, 200)):
            ref, scale = R.epoch(g, y, n, n_epochs, A, B, 3, 5)
            ratio = R.check_epoch(ref.astype(np.float32), ref, scale)
            assert ratio <= 1.0
            print(f"N = {g.n}, epoch {n}/{n_epochs}: rounding the result to fp32 is {ratio:.2f} x 2^-24")


def test_nan_rows_stay_nan_and_are_never_a_sample():
    g, y = _knn_case(65, 5, 1)
    # vertex 7 loses its edges and its position
    keep = (np.repeat(np.arange(65), np.diff(g.indptr)) != 7) & (g.indices != 7)
    rows = np.repeat(np.arange(65), np.diff(g.indptr))[keep]
    h = R.Graph(np.searchsorted(rows, np.arange(66)).astype(np.int64), g.indices[keep], g.weights[keep], None, None)
    y[7] = np.nan
    new, scale = R.epoch(h, y, 1, 10, A, B, 3, 5)
    assert np.isnan(new[7]).all() and np.isfinite(np.delete(new, 7, axis=0)).all()
    with pytest.raises(AssertionError, match="NaN"):
        R.check_epoch(np.nan_to_num(new), new, scale)


def test_schedule_fires_each_edge_as_often_as_its_weight_says():
    g, _ = _knn_case(65, 5, 1)
    r = (g.weights / g.weights.max()).astype(np.float64)
    fired = np.zeros(len(r))
    for n in range(1, 201):
        fired += np.floor(n * r) > np.floor((n - 1) * r)
    assert np.array_equal(fired, np.floor(200 * r))
    assert (fired[g.weights < g.weights.max() / 200] == 0).all()
