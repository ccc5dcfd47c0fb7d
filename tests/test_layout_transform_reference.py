"""CPU: the float64 restatement of the transform (tests/layout_transform_ref.py) -- can the epoch bound of
tests/test_gpu_layout_transform.py see a subtly wrong transform kernel, is a row's answer a function of the row alone,
and does the recipe place fresh draws of a cluster among that cluster's bank points?

Each seeded fault -- the mistakes a rewrite of layout_transform_kernel is likely to make -- is applied for one epoch to
the cluster case and must then miss the bound |dy| <= c 2^-24 (|y| + alpha sum |term|) at the LARGEST c the bound may
ever take (TRANSFORM_C_LIMIT = 256) by more than a factor 100.
"""
import numpy as np
import pytest

import layout_ref as R
import layout_transform_ref as T

A, B = 1.5769434, 0.8950609
MISS = 100.0                                  # every fault misses the bound at c = 256 by more than this factor


@pytest.fixture(scope="module")
def fitted():
    """seed -> (bank map Y, bank labels, idx, dist, query labels): N = 512, Q = 130 fresh draws, k = 15, 200-epoch fit."""
    out = {}
    for seed in (0, 1, 2):
        bank, bank_labels, queries, labels = T.split_cluster_set(seed)
        g = R.fuzzy_graph(*R.knn_exact(bank, 15))
        Y = R.layout(g, R.pca_init(bank, seed), 200, A, B, seed=seed)
        out[seed] = (Y, bank_labels) + T.knn_query(queries, bank, 15) + (labels,)
    return out


def _fault_case(fitted, fault):
    Y, _, idx, dist, _ = fitted[0]
    w, _ = T.query_memberships(idx, dist)
    if fault == "fire_fp32":
        # weights 0.7 (fp32: just below) beside the row's maximum 1: 10 r = 6.9999999 in float64 but 7 in fp32, so epoch
        # 10 fires in fp32 only and epoch 11 in float64 only
        w = w.copy()
        w[::3, 0], w[::3, 1] = np.float32(1.0), np.float32(0.7)
        epochs = [(10, 100, 5), (11, 100, 1)]
    elif fault == "global_wmax":
        # the rows' own maxima (0.28 .. 0.36 here) differ: r changes, and with it which slots fire
        epochs = [(1, 10, 5), (50, 100, 1)]
    else:
        epochs = [(1, 10, 5), (50, 100, 1), (100, 100, 5)]
    return idx, w, Y, T.init_positions(idx, w, Y), epochs


@pytest.mark.parametrize("fault", T.FAULTS)
def test_the_bound_catches_the_fault(fitted, fault):
    idx, w, Y, y, epochs = _fault_case(fitted, fault)
    for n, n_epochs, rate in epochs:
        ref, scale = T.transform_epoch(idx, w, Y, y, n, n_epochs, A, B, 3, rate)
        bad, _ = T.transform_epoch(idx, w, Y, y, n, n_epochs, A, B, 3, rate, fault=fault)
        ratio = R.epoch_ratio(bad, ref, scale)
        print(f"{fault}: epoch {n}/{n_epochs}, rate {rate}: {ratio:.3g} x 2^-24, {ratio / T.TRANSFORM_C_LIMIT:.3g} x the "
              f"bound at c = {T.TRANSFORM_C_LIMIT:g}")
        assert ratio > MISS * T.TRANSFORM_C_LIMIT, (fault, n, n_epochs, rate, ratio)
        with pytest.raises(AssertionError, match="epoch error"):
            R.check_epoch(bad, ref, scale, c=T.TRANSFORM_C_LIMIT)


def test_the_bound_constants_are_consistent():
    assert T.TRANSFORM_C <= T.TRANSFORM_C_LIMIT and np.log2(T.TRANSFORM_C) == int(np.log2(T.TRANSFORM_C))
    if T.TRANSFORM_MEASURED is not None:
        assert 8 * T.TRANSFORM_MEASURED <= T.TRANSFORM_C < 16 * T.TRANSFORM_MEASURED


def test_drop_sample_is_silent_without_a_rate(fitted):
    idx, w, Y, y, _ = _fault_case(fitted, "drop_sample")
    ref, scale = T.transform_epoch(idx, w, Y, y, 1, 10, A, B, 3, 0)
    assert R.epoch_ratio(T.transform_epoch(idx, w, Y, y, 1, 10, A, B, 3, 0, fault="drop_sample")[0], ref, scale) == 0.0


def test_rounding_to_fp32_stays_inside_the_bound(fitted):
    idx, w, Y, y, _ = _fault_case(fitted, "no_clip")
    for n, n_epochs in ((1, 10), (5, 10), (50, 100), (100, 100)):
        ref, scale = T.transform_epoch(idx, w, Y, y, n, n_epochs, A, B, 3, 5)
        assert R.check_epoch(ref.astype(np.float32), ref, scale, c=T.TRANSFORM_C) <= 1.0


def test_a_row_of_the_restatement_depends_on_the_row_alone(fitted):
    Y, _, idx, dist, _ = fitted[1]
    idx, dist = np.concatenate([idx, idx[:3]]), np.concatenate([dist, dist[:3]])      # three duplicate rows
    whole = T.transform(idx, dist, Y, 12, A, B, seed=5)
    assert np.isfinite(whole).all()
    assert np.array_equal(whole[-3:], whole[:3])
    parts = [T.transform(idx[s], dist[s], Y, 12, A, B, seed=5) for s in (slice(0, 1), slice(1, 65), slice(65, None))]
    assert np.array_equal(np.concatenate(parts), whole)
    perm = np.random.default_rng(0).permutation(len(idx))
    assert np.array_equal(T.transform(idx[perm], dist[perm], Y, 12, A, B, seed=5), whole[perm])
    # stepping the schedule, y0 threaded through
    step = T.transform(idx, dist, Y, 12, A, B, seed=5, last_epoch=5)
    assert np.array_equal(T.transform(idx, dist, Y, 12, A, B, seed=5, y0=step, first_epoch=6), whole)
    assert not np.array_equal(T.transform(idx, dist, Y, 12, A, B, seed=6), whole)


def test_memberships_of_the_restatement(fitted):
    _, _, idx, dist, _ = fitted[2]
    w, sigma = T.query_memberships(idx, dist)
    # the bisection's target: sum_j exp(-d_j / sigma) = log2 k, rho = 0
    psum = np.exp(-dist.astype(np.float64) / sigma.astype(np.float64)[:, None]).sum(axis=1)
    assert np.abs(psum - np.log2(15)).max() < 2e-5
    assert np.array_equal(w, np.exp(-dist.astype(np.float64) / sigma.astype(np.float64)[:, None]).astype(np.float32))
    # no self column: column 0 is a neighbour like any other; d = 0 is weight 1, idx = -1 weight 0, no slot at all NaN
    idx2, dist2 = idx[:4].copy(), dist[:4].copy()
    dist2[0, 0] = 0.0
    idx2[1, 10:], dist2[1, 10:] = -1, np.inf
    idx2[2], dist2[2] = -1, np.nan
    w2, sigma2 = T.query_memberships(idx2, dist2)
    assert w2[0, 0] == 1.0 and (w2[1, 10:] == 0).all() and (w2[1, :10] > 0).all() and (w2[2] == 0).all()
    assert np.array_equal(w2[3], w[3]) and sigma2[3] == sigma[3]
    Y = fitted[2][0]
    y0 = T.init_positions(idx2, w2, Y)
    assert np.isnan(y0[2]).all() and np.isfinite(np.delete(y0, 2, axis=0)).all()
    lo, hi = Y[idx2[3]].min(axis=0), Y[idx2[3]].max(axis=0)
    assert (y0[3] >= lo).all() and (y0[3] <= hi).all()                                # a convex combination
    out = T.transform(idx2, dist2, Y, 10, A, B)
    assert np.isnan(out[2]).all() and np.isfinite(np.delete(out, 2, axis=0)).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_quality_of_the_restatement(fitted, seed):
    Y, bank_labels, idx, dist, labels = fitted[seed]
    w, _ = T.query_memberships(idx, dist)
    y0 = T.init_positions(idx, w, Y)
    y = T.transform(idx, dist, Y, 100, A, B, seed=seed)
    purity, start = T.query_purity(y, labels, Y, bank_labels), T.query_purity(y0, labels, Y, bank_labels)
    print(f"seed {seed}: purity {purity:.4f} (the weighted-mean start alone {start:.4f}), largest move from the start "
          f"{np.abs(y - y0).max():.3f}")
    assert np.isfinite(y).all()
    assert purity >= 1.0 - 2.0 / len(idx)
