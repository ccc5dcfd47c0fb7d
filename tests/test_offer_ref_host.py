"""The offer restatement of tests/offer_ref.py without a GPU: its prediction form against tests/hdbscan_predict_ref.py --
``resolved`` and the neighbour ``predict`` chooses -- on a small integer-valued case, and the hand-made lists against what
they claim to hold."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hdbscan_predict_ref as P                                           # noqa: E402
import offer_ref as O                                                     # noqa: E402

Q, N = 14, 24


def _case(seed):
    """integer distances and core distances with many ties; bank rows 3 and 17 and query 5 are not finite"""
    rng = np.random.default_rng(seed)
    Dq = rng.integers(1, 12, size=(Q, N)).astype(np.float64)
    core = rng.integers(0, 8, size=N).astype(np.float64)
    Dq[:, [3, 17]], core[[3, 17]] = np.nan, np.nan
    Dq[5] = np.nan
    eligible = rng.random((Q, N)) < 0.8
    eligible[7] = False                                  # a row that sees nothing
    eligible[9, 4:] = False                              # a row that sees fewer than any list holds
    return Dq, core, eligible


def _lists(Dq, core, eligible, k):
    """what a search returns: the k nearest eligible rows by (distance, index), a -1 / +inf tail, -1 / NaN throughout
    for a non-finite query row"""
    idx, dist = np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, np.float32)
    for i in range(Q):
        if np.isnan(Dq[i]).all():
            dist[i] = np.nan
            continue
        at = np.flatnonzero(P._seen(Dq, core, eligible, i))
        order = at[np.lexsort((at, Dq[i, at]))][:k]
        idx[i, :len(order)], dist[i, :len(order)] = order, Dq[i, order]
    return idx, dist


TRIVIAL = dict(row_cluster=np.zeros(N, np.int64), row_lambda=np.zeros(N), parent=np.array([-1]), birth=np.zeros(1),
               label=np.zeros(1, np.int64), max_lambda=np.zeros(1), death=np.zeros(1))


@pytest.mark.parametrize("seed", (0, 1))
@pytest.mark.parametrize("min_samples", (1, 2, 4))
def test_predict_form_agrees_with_the_prediction_restatement(seed, min_samples):
    Dq, core, eligible = _case(seed)
    want = P.predict(Dq, core, TRIVIAL, 1.0, min_samples, eligible)
    asked = 0
    for k in (3, 4, 8, 24):
        idx, dist = _lists(Dq, core, eligible, k)
        for slack, squared, rel in ((None, False, 0.0), (np.full(Q, 1.0, np.float32), False, 0.0),
                                    (np.full(Q, 3.0, np.float32), True, 2.0 ** -10)):
            got = O.offer_knn(idx, dist, N, core, slack, squared, rel, min_samples)
            ok = P.resolved(Dq, core, min_samples, k, slack, squared, rel, eligible)
            has = got["best_j"] >= 0
            assert np.array_equal(got["unresolved"][has] == 0, ok[has]), (k, rel)
            assert not got["unresolved"][~has].any()
            assert np.array_equal(got["core_q"].astype(np.float64), want["core"], equal_nan=True)
            done = got["unresolved"] == 0
            assert np.array_equal(got["best_j"][done], want["neighbor"][done]), (k, rel)
            assert np.array_equal(got["best_w"][done].astype(np.float64), want["w"][done], equal_nan=True)
            # the radius tier: every eligible row within the weight found, in any order
            todo = np.flatnonzero(~done)
            asked += len(todo)
            inside = [np.flatnonzero(P._seen(Dq, core, eligible, i) & (Dq[i] <= got["best_w"][i]))[::-1] for i in todo]
            indptr = np.concatenate([[0], np.cumsum([len(x) for x in inside])]).astype(np.int64)
            indices = np.concatenate(inside + [np.zeros(0, np.int64)])
            rdist = np.concatenate([Dq[i, x] for i, x in zip(todo, inside)] + [np.zeros(0)]).astype(np.float32)
            w, j = O.offer_csr(indptr, indices, rdist, todo, Q, N, core, got["core_q"], got["best_w"], got["best_j"])
            assert np.array_equal(j, want["neighbor"]) and np.array_equal(w.astype(np.float64), want["w"], equal_nan=True)
    assert asked > 0


@pytest.mark.parametrize("k", (1, 16, 17, 64))
@pytest.mark.parametrize("min_samples", (None, 1, 2))
def test_lists_hold_what_they_claim(k, min_samples):
    n = 70 if min_samples is None else 50
    both = set()
    for slack in (None, "plain", "squared"):
        for rel in (0.0, 2.0 ** -10):
            case = O.lists(k, n, 70, slack, rel, min_samples)
            # (the weights the boundary rows aim at enter comparisons only: a max picks them, nothing is computed of them)
            vals = [case["dist"], np.delete(case["core"], range(O.BOUNDARY_BANK, O.BOUNDARY_BANK + len(O.BOUNDARY)))]
            for v in vals + ([] if case["slack"] is None else [case["slack"]]):
                v = v[np.isfinite(v)].astype(np.float64)
                assert ((v * 64) % 1 == 0).all() and (np.abs(v) < 64).all()
            if case["squared"]:
                full = (case["idx"][:, -1] >= 0) & (case["idx"][:, -1] < n) & (case["dist"][:, -1] > 0)
                d, s = case["dist"][full, -1].astype(np.float64), case["slack"][full].astype(np.float64)
                assert np.array_equal(np.sqrt(d * d - s) * 5, d * 4)    # d_last = 5 a, s = 9 a^2, floor 4 a
            ref = O.offer_knn(case["idx"], case["dist"], n, case["core"], case["slack"], case["squared"], rel, min_samples)
            flags = O.boundary_flags(case)
            assert (k == 1) == (not flags) and {r: int(ref["unresolved"][r]) for r in flags} == flags
            assert ref["best_j"][O.EMPTY] == -1 and ref["best_j"][O.BAD_INDEX_FIRST] != n + 5
            tie = O.TIE_CORE if min_samples is None else O.TIE_DIST
            assert ref["best_j"][tie] == case["idx"][tie].min() == case["idx"][tie, -1]
            assert ref["best_w"][O.CLAMP] == 0 and not np.signbit(ref["best_w"][O.CLAMP])
            both |= set(ref["unresolved"].tolist())
    assert both == {0, 1}
