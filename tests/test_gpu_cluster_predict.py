"""GPU tests of ClusterModel.predict and the GLOSH scores (run with -m gpu on an MI355X): given the device's own fp32
distances, label, neighbour, cluster, lambda, strength and outlier score equal the float64 restatement of
tests/hdbscan_predict_ref.py bit for bit -- every step of the rule is one correctly rounded operation --, whatever the
batch, ``search_k``, ``splits`` or the method."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import btsbot_amd
import hdbscan_ref as R
import hdbscan_predict_ref as P

pytestmark = pytest.mark.gpu

INF = float("inf")


@functools.lru_cache(maxsize=None)
def _bank(name):
    kind, _, seed = name.partition(":")
    if kind == "32d":
        return R.blobs_32d(int(seed))[:300]
    if kind == "2d":
        return R.blobs_2d(int(seed))[:360]
    if kind == "bad":
        return R.blobs_32d_with_bad_rows()
    return R.lattice()


@functools.lru_cache(maxsize=None)
def _queries(name):
    """130 to 300 rows per set: more than one workgroup of the offer kernel at any list length, the last one partial"""
    kind, _, seed = name.partition(":")
    X = _bank(name)
    rng = np.random.default_rng(40 + len(X))
    if kind in ("32d", "bad"):
        fresh, _origin = P.fresh_draws(int(seed) if kind == "32d" else 1)                      # 160
        return np.concatenate([fresh, P.jittered_rows(R.blobs_32d(int(seed) if kind == "32d" else 1), count=37)])
    lo, hi = X.min(0) - 3, X.max(0) + 3
    spread = rng.uniform(lo, hi, size=(150, 2))
    if kind == "2d":
        return np.concatenate([spread.astype(np.float32), P.jittered_rows(X, count=61)])
    # the lattice: also points of the lattice itself and the centres of its cells, where distances and weights tie
    on = np.stack(np.meshgrid(np.arange(-1.0, 13.0, 2.0), np.arange(-1.0, 13.0, 2.0)), -1).reshape(-1, 2)
    return np.concatenate([spread, on, on[:20] + 0.5, on[:11] * 0.5 + np.array([20.0, 3.0])]).astype(np.float32)


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    if got.dtype == np.float64:
        want = np.asarray(want, np.float64)
        nan = np.isnan(want)                       # (a NaN is a NaN, whatever its payload)
        assert np.array_equal(np.isnan(got), nan), what
        assert np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64)), what
    else:
        assert np.array_equal(got, want), what


def _dq(index, tq, n):
    """float64 [Q, N]: the device's own direct-form distances of every eligible pair (NaN elsewhere)"""
    indptr, indices, dist = index.radius(tq, INF, sort="index")
    indptr, indices, dist = _np(indptr), _np(indices), _np(dist)
    Dq = np.full((len(indptr) - 1, n), np.nan)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    Dq[rows, indices] = dist
    return Dq


def _restated(m, tq, eligible=None):
    n = len(m)
    t = P.tables(m.tree.condensed, n, m.cluster_selection_method, m.allow_single_cluster)
    core = _np(m.mst.core).astype(np.float64)
    Dq = _dq(m.index, tq, n)
    return P.predict(Dq, core, t, P.lam_zero_of(_np(m.mst.weights)), m.min_samples, eligible), Dq, core, t


def _check(m, tq, ref, Dq, core, eligible=None, **kw):
    labels, prob, d = m.predict(tq, return_details=True, **kw)
    assert labels.dtype == torch.int64 and prob.dtype == torch.float64 and labels.shape == prob.shape == (len(tq),)
    assert d["neighbor"].dtype == d["cluster"].dtype == torch.int64 and d["lambda"].dtype == d["outlier"].dtype == torch.float64
    _same(_np(labels), ref["label"], "label")
    _same(_np(d["neighbor"]), ref["neighbor"], "neighbor")
    _same(_np(d["cluster"]), ref["cluster"], "cluster")
    _same(_np(d["lambda"]), ref["lam"], "lambda")
    _same(_np(prob), ref["prob"], "prob")
    _same(_np(d["outlier"]), ref["outlier"], "outlier")
    # the neighbour is the smallest (w, index) over ALL eligible rows of the bank
    nb = _np(d["neighbor"])
    for i in np.flatnonzero(nb >= 0):
        ok = ~np.isnan(Dq[i]) & ~np.isnan(core)
        if eligible is not None:
            ok &= eligible[i]
        w = np.maximum(np.maximum(Dq[i], ref["core"][i]), core)
        at = np.flatnonzero(ok)
        assert (w[at] > w[nb[i]]).sum() + (w[at] == w[nb[i]]).sum() == len(at)
        assert nb[i] == at[w[at] == w[nb[i]]][0]
    return labels, prob, d


def _bits(out):
    labels, prob, d = out
    return [labels, prob.view(torch.int64), d["neighbor"], d["cluster"], d["lambda"].view(torch.int64),
            d["outlier"].view(torch.int64)]


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _climbs(t, ref):
    out = np.full(len(ref["cluster"]), -1)
    for i in np.flatnonzero(ref["neighbor"] >= 0):
        a, k = t["row_cluster"][ref["neighbor"][i]], 0
        while a != ref["cluster"][i]:
            a, k = t["parent"][a], k + 1
        out[i] = k
    return out


# ---- 1, 4. equality with the restatement; the neighbour is the nearest of all -------------------------------------------
@pytest.mark.parametrize("name,method", [("32d:0", "tiles"), ("32d:1", "tiles"), ("2d:0", "tiles"), ("2d:0", "grid"),
                                         ("lattice", "tiles"), ("lattice", "grid")])
def test_predictions_equal_the_restatement_bit_for_bit(cuda, name, method):
    X, Q = _bank(name), _queries(name)
    assert 130 <= len(Q) <= 300
    tx, tq = torch.from_numpy(X).to(cuda), torch.from_numpy(Q).to(cuda)
    seen = set()
    for mcs, ms in R.PAIRS:
        for sel in ("eom", "leaf"):
            m = btsbot_amd.ClusterModel(tx, mcs, ms, cluster_selection_method=sel, method=method)
            ref, Dq, core, t = _restated(m, tq)
            stats = {}
            labels, _prob, d = _check(m, tq, ref, Dq, core, stats=stats)
            climbs = _climbs(t, ref)
            seen |= set(_np(labels).tolist())
            print(f"{name} {method} ({mcs}, {ms}) {sel}: {len(t['parent'])} clusters, labels {sorted(set(_np(labels).tolist()))}, "
                  f"{int((_np(labels) < 0).sum())} of {len(Q)} noise, climbs up to {climbs.max()}, {stats}")
            assert stats["unresolved"] <= len(Q) and (stats["radius_total"] > 0) == (stats["unresolved"] > 0)
    assert -1 in seen and len(seen) >= 3


# ---- 2. the radius tier ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,method", [("32d:0", "tiles"), ("2d:0", "grid")])
def test_the_radius_tier_runs_and_changes_nothing(cuda, name, method):
    X = _bank(name)
    Q = P.jittered_rows(X)
    tx, tq = torch.from_numpy(X).to(cuda), torch.from_numpy(Q).to(cuda)
    m = btsbot_amd.ClusterModel(tx, 10, 5, method=method)
    ref, Dq, core, _t = _restated(m, tq)
    want = int((~P.resolved(Dq, core, 5, 4)).sum())     # (without slack: a lower bound for the tile search)
    stats, wide = {}, {}
    one = _check(m, tq, ref, Dq, core, search_k=1, stats=stats)
    many = _check(m, tq, ref, Dq, core, search_k=64, stats=wide)
    print(f"{name} {method}: search_k = 1 sends {stats}, the restatement's predicate {want}; search_k = 64 {wide}")
    assert stats["unresolved"] > 0 and stats["radius_total"] >= stats["unresolved"] and stats["unresolved"] >= want > 0
    if method == "grid":
        assert stats["unresolved"] == want
    assert wide["unresolved"] < stats["unresolved"]
    assert _equal(one, many)


# ---- 3. independence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("32d:0", "2d:0"))
def test_a_rows_answer_does_not_depend_on_the_batch_search_k_splits_or_method(cuda, name):
    X, Q = _bank(name), _queries(name)
    tx, tq = torch.from_numpy(X).to(cuda), torch.from_numpy(Q).to(cuda)
    m = btsbot_amd.ClusterModel(tx, 10, 5)
    base = m.predict(tq, return_details=True)
    perm = torch.from_numpy(np.random.default_rng(8).permutation(len(Q))).to(cuda)
    got = m.predict(tq[perm], return_details=True)
    assert all(torch.equal(x[perm], y) for x, y in zip(_bits(base), _bits(got)))
    halves = [m.predict(part, return_details=True) for part in (tq[:67], tq[67:])]
    assert all(torch.equal(x, torch.cat([a, b])) for x, a, b in zip(_bits(base), _bits(halves[0]), _bits(halves[1])))
    twice = m.predict(torch.cat([tq, tq]), return_details=True)
    assert all(torch.equal(torch.cat([x, x]), y) for x, y in zip(_bits(base), _bits(twice)))
    for kw in (dict(search_k=1), dict(search_k=3), dict(search_k=64), dict(splits=3), dict(splits=1)):
        assert _equal(base, m.predict(tq, return_details=True, **kw)), kw
    assert _equal(base, m.predict(tq, return_details=True))                        # the run
    again = btsbot_amd.ClusterModel(tx, 10, 5, search_k=3, splits=3)                 # the fit's own switches
    assert _equal(base, again.predict(tq, return_details=True))
    if name == "2d:0":
        grid = btsbot_amd.ClusterModel(tx, 10, 5, method="grid")
        assert isinstance(grid.index, btsbot_amd.MapIndex)
        assert torch.equal(grid.labels, m.labels) and torch.equal(grid.prob.view(torch.int64), m.prob.view(torch.int64))
        for kw in ({}, dict(search_k=1), dict(search_k=64)):
            assert _equal(base, grid.predict(tq, return_details=True, **kw)), kw


# ---- 5. edges -------------------------------------------------------------------------------------------------------------
def test_a_list_that_is_not_full_duplicates_and_non_finite_rows(cuda):
    # N < k_s: every list holds all rows and nothing goes to the radius tier
    X = _bank("32d:0")[:7]
    tx = torch.from_numpy(X).to(cuda)
    Q = np.concatenate([X[:3] + 0.25, _queries("32d:0")[:140]]).astype(np.float32)
    tq = torch.from_numpy(Q).to(cuda)
    m = btsbot_amd.ClusterModel(tx, 2, 3, allow_single_cluster=True)
    ref, Dq, core, _t = _restated(m, tq)
    stats = {}
    _check(m, tq, ref, Dq, core, stats=stats, search_k=8)
    assert stats == dict(unresolved=0, radius_total=0)
    # min_samples = 1 and an exact duplicate of a bank row: w = 0, lambda = lam_zero
    X = _bank("32d:2")
    tx = torch.from_numpy(X).to(cuda)
    Q = np.concatenate([X[[7, 150]], _queries("32d:2")[:150]])
    Q[5] = np.nan
    Q[9, 3] = np.inf
    tq = torch.from_numpy(Q).to(cuda)
    m = btsbot_amd.ClusterModel(tx, 5, 1)
    ref, Dq, core, _t = _restated(m, tq)
    labels, prob, d = _check(m, tq, ref, Dq, core)
    assert (m.mst.core == 0).all() and d["neighbor"][:2].tolist() == [7, 150]
    assert (d["lambda"][:2] == m.lam_zero).all() and m.lam_zero == 1.0 / float(m.mst.weights.min())
    # a non-finite query row
    for i in (5, 9):
        assert labels[i] == -1 and prob[i] == 0 and torch.isnan(d["outlier"][i]) and torch.isnan(d["lambda"][i])
        assert d["neighbor"][i] == -1 and d["cluster"][i] == -1


def test_non_finite_bank_rows_are_never_a_neighbour(cuda):
    X, Q = _bank("bad"), _queries("bad")
    Q = np.concatenate([Q, np.nan_to_num(X[list(R.BAD_ROWS)], nan=0.0, posinf=0.0, neginf=0.0)])   # next to the bad rows
    tx, tq = torch.from_numpy(X).to(cuda), torch.from_numpy(Q).to(cuda)
    m = btsbot_amd.ClusterModel(tx, 10, 5)
    bad = list(R.BAD_ROWS)
    assert (m.labels[bad] == -1).all() and (m.prob[bad] == 0).all() and torch.isnan(m.outlier_scores[bad]).all()
    assert (m.tables["row_cluster"][bad] == -1).all()
    ref, Dq, core, _t = _restated(m, tq)
    for kw in (dict(search_k=1), {}):
        _labels, _prob, d = _check(m, tq, ref, Dq, core, **kw)
        assert not np.isin(_np(d["neighbor"]), bad).any() and (d["neighbor"] >= 0).all()


def test_three_levels_single_cluster_and_the_root(cuda):
    X, Q = _bank("lattice"), _queries("lattice")
    tx, tq = torch.from_numpy(X).to(cuda), torch.from_numpy(Q).to(cuda)
    m = btsbot_amd.ClusterModel(tx, 5, 5)
    ref, Dq, core, t = _restated(m, tq)
    labels, prob, d = _check(m, tq, ref, Dq, core)
    depth = np.zeros(len(t["parent"]), np.int64)
    for c in range(1, len(depth)):
        depth[c] = depth[t["parent"][c]] + 1
    # from the details alone: the cluster the neighbour fell out of lies two levels below the cluster the row ends in
    tab = {k: _np(v) for k, v in m.tables.items()}
    start = tab["row_cluster"][_np(d["neighbor"])]
    climbed = depth[start] - depth[_np(d["cluster"])]
    print(f"lattice: depths {depth.tolist()}, climbs {np.bincount(climbed).tolist()}")
    assert depth.max() >= 2 and climbed.max() >= 2 and (climbed >= 0).all()
    # a row that ends at the root is noise ...
    root = d["cluster"] == 0
    assert int(root.sum()) > 0 and (labels[root] == -1).all() and (prob[root] == 0).all()
    # ... unless the root may be a cluster; then every row with a neighbour has a label
    single = btsbot_amd.ClusterModel(tx, 5, 5, allow_single_cluster=True, cluster_selection_method="leaf")
    ref1, Dq1, core1, _t = _restated(single, tq)
    _check(single, tq, ref1, Dq1, core1)
    one = np.ones((9, 2), np.float32) * np.arange(9, dtype=np.float32)[:, None]          # one weight: the root alone
    only = btsbot_amd.ClusterModel(torch.from_numpy(one).to(cuda), 3, 2, allow_single_cluster=True)
    assert (only.labels == 0).all() and len(only.tables["parent"]) == 1
    tq1 = torch.tensor([[0.5, 0.5], [40.0, 40.0], [4.0, 4.0]], device=cuda)
    ref2, Dq2, core2, _t = _restated(only, tq1)
    labels, prob, d = _check(only, tq1, ref2, Dq2, core2)
    assert labels.tolist() == [0, 0, 0] and prob[0] == 1 and prob[2] == 1 and 0 < prob[1] < 1 and d["outlier"][1] > 0.9


# ---- 6. groups ------------------------------------------------------------------------------------------------------------
def test_groups_leave_the_own_object_out(cuda):
    X, obj = R.object_set()
    rng = np.random.default_rng(12)
    rows = rng.choice(len(X), size=150, replace=False)
    Q = (X[rows] + rng.normal(0, 0.05, size=(150, X.shape[1]))).astype(np.float32)       # new alerts of known objects
    q_obj = obj[rows].copy()
    q_obj[:10] = obj.max() + 1 + np.arange(10)                                            # ... and of new ones
    tx, tq = torch.from_numpy(X).to(cuda), torch.from_numpy(Q).to(cuda)
    g, qg = torch.from_numpy(obj).to(cuda), torch.from_numpy(q_obj).to(cuda)
    m = btsbot_amd.ClusterModel(tx, 5, 5, groups=g)
    want_l, want_p = btsbot_amd.hdbscan(tx, 5, 5, groups=g)
    assert torch.equal(m.labels, want_l) and torch.equal(m.prob.view(torch.int64), want_p.view(torch.int64))
    eligible = q_obj[:, None] != obj[None, :]
    ref, Dq, core, _t = _restated(m, tq, eligible)
    for kw in ({}, dict(search_k=1)):
        _l, _p, d = _check(m, tq, ref, Dq, core, eligible, query_groups=qg, exclude_same_group=True, **kw)
        assert (g[d["neighbor"]] != qg).all()
    plain, Dq, core, _t = _restated(m, tq)
    _l, _p, d = _check(m, tq, plain, Dq, core)
    print(f"objects: without the switch {int((g[d['neighbor']] == qg).sum())} of 150 neighbours are of the own object")
    index = btsbot_amd.EmbeddingIndex(tx, groups=g)
    again = btsbot_amd.ClusterModel(index, 5, 5)
    assert again.index is index and _equal(m.predict(tq, qg, True, return_details=True),
                                           again.predict(tq, qg, True, return_details=True))
    with pytest.raises(ValueError, match="groups= next to an index"):
        btsbot_amd.ClusterModel(index, 5, 5, groups=g)


def test_too_few_eligible_rows_under_exclude_same_group(cuda):
    """All rows but three belong to one object: a new alert of that object sees three rows, fewer than min_samples - 1."""
    X = _bank("32d:0")[:80]
    obj = np.ones(80, np.int64)
    obj[:3] = 0
    Q = _queries("32d:0")[:140]
    q_obj = np.ones(140, np.int64)
    q_obj[::3] = 0
    q_obj[1::7] = 5
    tx, tq = torch.from_numpy(X).to(cuda), torch.from_numpy(Q).to(cuda)
    g, qg = torch.from_numpy(obj).to(cuda), torch.from_numpy(q_obj).to(cuda)
    m = btsbot_amd.ClusterModel(tx, 5, 5, groups=g)
    eligible = q_obj[:, None] != obj[None, :]
    ref, Dq, core, _t = _restated(m, tq, eligible)
    labels, prob, d = _check(m, tq, ref, Dq, core, eligible, query_groups=qg, exclude_same_group=True)
    few = torch.from_numpy(q_obj == 1).to(cuda)
    assert (labels[few] == -1).all() and (prob[few] == 0).all() and (d["outlier"][few] == 1).all()
    assert (d["neighbor"][few] == -1).all() and (d["neighbor"][~few] >= 0).all()


# ---- 7, 8. the fit --------------------------------------------------------------------------------------------------------
def test_the_fit_is_hdbscans_and_does_not_follow_add(cuda):
    X = _bank("32d:1")
    tx = torch.from_numpy(X).to(cuda)
    for kw in (dict(min_cluster_size=10, min_samples=5), dict(min_cluster_size=5, min_samples=10,
                                                              cluster_selection_method="leaf")):
        m = btsbot_amd.ClusterModel(tx, **kw)
        labels, prob, tree = btsbot_amd.hdbscan(tx, return_tree=True, **kw)
        assert torch.equal(m.labels, labels) and torch.equal(m.prob.view(torch.int64), prob.view(torch.int64))
        glosh = tree.outlier_scores(kw["min_cluster_size"])
        assert glosh.dtype == torch.float64 and glosh.device == tx.device and glosh.shape == (len(X),)
        assert torch.equal(m.outlier_scores.view(torch.int64), glosh.view(torch.int64))
        t = P.tables(m.tree.condensed, len(X), m.cluster_selection_method, False)
        _same(_np(glosh), t["outlier"])
        for name in ("row_cluster", "parent", "label"):
            assert m.tables[name].dtype == torch.int32 and m.tables[name].device == tx.device
            _same(_np(m.tables[name]).astype(np.int64), t[name], name)
        for name in ("row_lambda", "birth", "max_lambda", "death"):
            _same(_np(m.tables[name]), t[name], name)
        assert float(glosh.min()) == 0 and 0.5 < float(glosh.max()) <= 1
    # the fit does not follow index.add
    index = btsbot_amd.EmbeddingIndex(tx[:250])
    m = btsbot_amd.ClusterModel(index, 10, 5)
    tq = torch.from_numpy(_queries("32d:1")).to(cuda)
    before = m.predict(tq, return_details=True)
    index.add(tx[250:])
    with pytest.raises(RuntimeError, match="refit"):
        m.predict(tq)
    assert m.refit() is m and len(m) == 300
    after = m.predict(tq, return_details=True)
    whole = btsbot_amd.ClusterModel(tx, 10, 5)
    assert _equal(after, whole.predict(tq, return_details=True)) and not _equal(before, after)


# ---- 9. run_training --------------------------------------------------------------------------------------------------------
def test_run_training_writes_outlier_scores_only_when_asked(cuda, tmp_path):
    import pandas as pd
    from btsbot_amd.synthetic import synthetic_batch
    from btsbot_amd.train import run_training
    from helpers import CONFIGS, METADATA_COLS
    _, meta, _ = synthetic_batch(448, seed=21)
    lab = (meta[:, 5] > meta[:, 5].median()).long().numpy()
    d = tmp_path / "data"
    d.mkdir()
    for split, sl in (("train", slice(0, 256)), ("val", slice(256, 384)), ("test", slice(384, 448))):
        df = pd.DataFrame(meta[sl].numpy(), columns=METADATA_COLS)
        df["label"] = lab[sl]
        df.to_csv(d / f"{split}_cand_v11_N100.csv", index=False)
    base = dict(CONFIGS["um_nn"][1], model_name="um_nn", train_data_version="v11", epochs=1, batch_size=64,
                learning_rate="3e-3", warmup_epochs=1, beta_1=0.9, beta_2=0.999, patience=3, random_seed=2,
                generate_embeddings=True)
    runs = (("g1", {"algorithm": "hdbscan", "min_cluster_size": 4, "on": "embedding", "outlier_scores": True}),
            ("g0", {"algorithm": "hdbscan", "min_cluster_size": 4, "on": "embedding"}))
    for run, clu in runs:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            run_training(dict(base, embedding_clusters=clu), data_base_dir=str(tmp_path) + "/", run_name=run, device=cuda,
                         precision="f32", models_root=str(tmp_path / "models"), embeddings_root=str(tmp_path / "embeddings"))
        stem = str(tmp_path / "embeddings" / f"um_nn_{run}")
        emb = torch.from_numpy(np.load(stem + ".npy")).to(cuda)
        want_l, _p, tree = btsbot_amd.hdbscan(emb, 4, return_tree=True)
        assert np.array_equal(np.load(stem + "_clusters.npy"), want_l.cpu().numpy())
        if run == "g1":
            got = np.load(stem + "_cluster_outlier.npy")
            assert got.dtype == np.float64 and got.shape == (64,)
            _same(got, _np(tree.outlier_scores(4)))
        else:
            assert not os.path.exists(stem + "_cluster_outlier.npy") and os.path.exists(stem + "_cluster_prob.npy")


# ---- 10. arguments --------------------------------------------------------------------------------------------------------
def test_argument_checks(cuda):
    X = _bank("2d:0")
    tx = torch.from_numpy(X).to(cuda)
    tq = tx[:5].clone()
    m = btsbot_amd.ClusterModel(tx, 10, 5)
    for kw in (dict(search_k=0), dict(search_k=65), dict(search_k=2.0), dict(search_k=True), dict(splits=-1),
               dict(splits=33), dict(stats=[]), dict(return_details=1), dict(exclude_same_group=True),
               dict(query_groups=torch.zeros(5, dtype=torch.int64, device=cuda), exclude_same_group=True)):
        with pytest.raises(ValueError):
            m.predict(tq, **kw)
    with pytest.raises(ValueError):
        m.predict(torch.zeros((5, 3), device=cuda))
    with pytest.raises(ValueError):
        m.predict(torch.zeros(5, device=cuda))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict(tq.cpu())
    grid = btsbot_amd.ClusterModel(btsbot_amd.MapIndex(tx), 10, 5)
    with pytest.raises(ValueError, match="splits"):
        grid.predict(tq, splits=2)
    with pytest.raises(ValueError, match="splits"):
        btsbot_amd.ClusterModel(btsbot_amd.MapIndex(tx), 10, 5, splits=2)
    with pytest.raises(ValueError, match="metric"):
        btsbot_amd.ClusterModel(btsbot_amd.EmbeddingIndex(tx, "cosine"), 10, 5)
    with pytest.raises(ValueError, match="finite rows"):
        btsbot_amd.ClusterModel(tx[:4], 5, 5)
    with pytest.raises(ValueError):
        m.tree.outlier_scores(1)
    # nothing to answer: empty tensors of the right kinds
    labels, prob, d = m.predict(tx[:0], return_details=True)
    assert labels.shape == prob.shape == d["neighbor"].shape == (0,) and labels.dtype == torch.int64
    # the cosine metric goes the same way
    X32 = _bank("32d:0")
    t32, q32 = torch.from_numpy(X32).to(cuda), torch.from_numpy(_queries("32d:0")).to(cuda)
    cos = btsbot_amd.ClusterModel(t32, 10, 5, "cosine")
    ref, Dq, core, _t = _restated(cos, q32)
    _check(cos, q32, ref, Dq, core)
    _check(cos, q32, ref, Dq, core, search_k=1)
