"""GPU tests of the local outlier factor (run with -m gpu on an MI355X): btsbot_lof_fit / btsbot_lof_score equal the float64
restatement of tests/lof_ref.py bit for bit on the device's own neighbour lists; rows with fewer than k neighbours, absent
entries, duplicates and non-finite rows; scikit-learn end to end within the fp32 bound; a row's score does not depend on
the other rows of the call, on ``splits`` or on how the index was built; what groups are for; the C entry points' errors;
nothing reads the host."""
import ctypes as C
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import btsbot_amd
import lof_ref as R
import radius_ref as RR
from btsbot_amd import _lib, novelty

pytestmark = pytest.mark.gpu

N, D, Q = 509, 32, 130          # 509: no multiple of the 4, 8 or 16 rows a workgroup holds
METRICS = ("euclidean", "cosine")


@functools.lru_cache(maxsize=None)
def _rows():
    """(bank fp32 [N, D], new rows fp32 [Q, D]): computed once, never written"""
    x = RR.clusters_32d(41, n=N)
    q = R.perturbed_draws(x, 41, q=Q)
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


@functools.lru_cache(maxsize=None)
def _sklearn(name, seed, k):
    """(the set, its new rows, scikit-learn's novelty estimator fitted to the float64 rows)"""
    from sklearn.neighbors import LocalOutlierFactor
    x = getattr(RR, name)(seed)
    q = R.perturbed_draws(x, seed)
    est = LocalOutlierFactor(n_neighbors=k, algorithm="brute", novelty=True).fit(x.astype(np.float64))
    return x, q, est


def _gpu(dev, *arrays):
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays]


def _np(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def _same_bits(got, want, what=""):
    """float64 arrays equal bit for bit; a NaN equals a NaN (its payload is not part of the contract)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64)), what


# ---- 1. bit equality with the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", (1, 5, 20, 64))
def test_fit_and_score_equal_the_restatement_bit_for_bit(cuda, k, metric):
    x, q = _rows()
    tx, tq = _gpu(cuda, x, q)
    index = btsbot_amd.EmbeddingIndex(tx, metric)
    idx, dist = index.query(tx, k, self_offset=0)
    kdist, lrd, lof = novelty._fit(idx, dist)
    want = R.lof_fit(*_np(idx, dist))
    for g, w, name in zip(_np(kdist, lrd, lof), want, ("kdist", "lrd", "lof")):
        assert np.isfinite(w).all(), name
        _same_bits(g, w, (name, k, metric))
    qi, qd = index.query(tq, k)
    for g, w, name in zip(_np(*novelty._score(qi, qd, kdist, lrd)), R.lof_score(*_np(qi, qd), want[0], want[1]),
                          ("lrd", "lof")):
        assert np.isfinite(w).all(), name
        _same_bits(g, w, ("score " + name, k, metric))
    # the public calls are these two
    model = btsbot_amd.NoveltyModel(index, k, metric)
    for g, w in zip(_np(model.kdist, model.lrd, model.lof), want):
        _same_bits(g, w)
    s, s_lrd = model.score(tq, return_lrd=True)
    _same_bits(_np(s)[0], R.lof_score(*_np(qi, qd), want[0], want[1])[1])
    _same_bits(_np(s_lrd)[0], R.lof_score(*_np(qi, qd), want[0], want[1])[0])
    _same_bits(_np(btsbot_amd.local_outlier_factor(tx, k, metric))[0], want[2])
    _same_bits(_np(btsbot_amd.local_outlier_factor(None, k, knn=(idx, dist)))[0], want[2])


def test_a_wider_graph_is_read_to_n_neighbors_and_lof_may_be_left_out(cuda):
    x, _ = _rows()
    tx, = _gpu(cuda, x)
    idx, dist = btsbot_amd.knn_graph(tx, 20, include_self=False)
    want = R.lof_fit(*_np(idx[:, :7], dist[:, :7]))
    _same_bits(_np(btsbot_amd.local_outlier_factor(tx, 7, knn=(idx, dist)))[0], want[2])
    with pytest.raises(ValueError, match="fewer than n_neighbors"):
        btsbot_amd.local_outlier_factor(tx, 21, knn=(idx, dist))
    kdist, lrd = (torch.empty(N, dtype=torch.float64, device=cuda) for _ in range(2))
    i7, d7 = idx[:, :7].contiguous(), dist[:, :7].contiguous()
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    assert _lib.lib().btsbot_lof_fit(C.c_void_p(i7.data_ptr()), C.c_void_p(d7.data_ptr()), N, 7, C.c_void_p(kdist.data_ptr()),
                                     C.c_void_p(lrd.data_ptr()), None, stream) == _lib.OK
    _same_bits(_np(kdist)[0], want[0])
    _same_bits(_np(lrd)[0], want[1])


# ---- 2. fewer than k neighbours ---------------------------------------------------------------------------------------
def test_fewer_than_k_rows_are_scored_on_those_there_are(cuda):
    x, q = _rows()
    tx, tq = _gpu(cuda, x[:7], q[:9])
    model = btsbot_amd.NoveltyModel(tx, 20)
    idx, dist = _np(*btsbot_amd.knn_graph(tx, 20, include_self=False))
    assert ((idx >= 0).sum(axis=1) == 6).all()
    want = R.lof_fit(idx, dist)
    for g, w in zip(_np(model.kdist, model.lrd, model.lof), want):
        assert np.isfinite(w).all()
        _same_bits(g, w)
    qi, qd = _np(*model.index.query(tq, 20))
    assert ((qi >= 0).sum(axis=1) == 7).all()
    _same_bits(_np(model.score(tq))[0], R.lof_score(qi, qd, want[0], want[1])[1])


@pytest.mark.parametrize("k", (3, 20, 40))
def test_a_hand_made_graph_with_mixed_tails(cuda, k):
    """Tails of every length, rows without any entry, an index out of range, and a present entry BEHIND an absent one
    (no graph of the library's has that; the definition covers it)."""
    rng = np.random.default_rng(5 + k)
    n = 37
    idx = rng.integers(0, n, size=(n, k)).astype(np.int64)
    dist = np.sort(rng.uniform(0.1, 2.0, size=(n, k)).astype(np.float32), axis=1)
    m = rng.integers(0, k + 1, size=n)
    m[[3, 11]] = 0
    m[5] = k
    tail = np.arange(k)[None, :] >= m[:, None]
    idx[tail] = -1
    dist[tail] = np.inf
    idx[5, 0] = n + 3                                         # out of range: no entry
    idx[7, :] = -1
    idx[7, k - 1], dist[7, k - 1] = 2, 1.25                   # behind a gap
    want = R.lof_fit(idx, dist)
    assert np.isnan(want[0][[3, 11]]).all() and want[0][7] == 1.25
    ti, td = _gpu(cuda, idx, dist)
    got = _np(*novelty._fit(ti, td))
    for g, w, name in zip(got, want, ("kdist", "lrd", "lof")):
        _same_bits(g, w, name)
    has = ((idx >= 0) & (idx < n)).any(axis=1)
    assert np.array_equal(np.isfinite(got[1]), has) and not has[[3, 11]].any() and has[[5, 7]].all()
    # the same lists as NEW rows against that fit (their indices beyond the bank count as absent there too)
    qi, qd = idx[:20].copy(), dist[:20].copy()
    for g, w in zip(_np(*novelty._score(*_gpu(cuda, qi, qd), *_gpu(cuda, want[0], want[1]))),
                    R.lof_score(qi, qd, want[0], want[1])):
        _same_bits(g, w)


def test_one_group_for_all_and_non_finite_rows_score_nan(cuda):
    x, q = _rows()
    tx, tq = _gpu(cuda, x[:64], q[:8])
    one = torch.zeros(64, dtype=torch.int64, device=cuda)
    assert torch.isnan(btsbot_amd.local_outlier_factor(tx, 5, groups=one)).all()
    model = btsbot_amd.NoveltyModel(tx, 5, groups=one)
    assert torch.isnan(model.lof).all() and torch.isnan(model.kdist).all() and torch.isnan(model.lrd).all()
    assert torch.isnan(model.score(tq)).all()                 # (the bank's rows are present, their kdist and lrd NaN)
    assert np.isnan(model.threshold(0.1))
    bad = np.array(x[:64])
    bad[9, 3], bad[40, 0] = np.nan, np.inf
    tb, = _gpu(cuda, bad)
    idx, dist = _np(*btsbot_amd.knn_graph(tb, 5, include_self=False))
    assert not np.isin(idx, (9, 40)).any() and (idx[[9, 40]] == -1).all()
    lof = _np(btsbot_amd.local_outlier_factor(tb, 5))[0]
    assert np.isnan(lof[[9, 40]]).all() and np.isfinite(np.delete(lof, (9, 40))).all()
    _same_bits(lof, R.lof_fit(idx, dist)[2])
    qbad = np.array(q[:8])
    qbad[2, 1] = np.nan
    s = _np(btsbot_amd.NoveltyModel(tb, 5).score(_gpu(cuda, qbad)[0]))[0]
    assert np.isnan(s[2]) and np.isfinite(np.delete(s, 2)).all()


# ---- 3. duplicates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (5, 20))
def test_a_block_of_duplicates_has_lrd_1e10_and_lof_exactly_1(cuda, k):
    x = np.array(_rows()[0][:128])
    x[:k + 1] = x[0]
    tx, = _gpu(cuda, x)
    model = btsbot_amd.NoveltyModel(tx, k)
    assert (model.kdist[:k + 1] == 0).all() and (model.lrd[:k + 1] == 1e10).all() and (model.lof[:k + 1] == 1.0).all()
    assert (model.lrd[k + 1:] < 1e3).all()
    from sklearn.neighbors import LocalOutlierFactor
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # ("duplicate values are leading to incorrect results")
        want = -LocalOutlierFactor(n_neighbors=k, algorithm="brute").fit(x.astype(np.float64)).negative_outlier_factor_
    assert (want[:k + 1] == 1.0).all()
    s = model.score(tx[:2])                                    # a new row ON the block: k of its rows at distance 0
    assert (s == 1.0).all()


# ---- 4. scikit-learn end to end --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (5, 20))
@pytest.mark.parametrize("name,seed", [(n, s) for n in ("clusters_32d", "blobs_2d") for s in (21, 22, 23)])
def test_fit_and_score_against_sklearn_end_to_end(cuda, name, seed, k):
    x, q, est = _sklearn(name, seed, k)
    bound = R.fp32_bound(x.shape[1])
    tx, tq = _gpu(cuda, x, q)
    model = btsbot_amd.NoveltyModel(tx, k)
    idx = _np(model.index.query(tx, k, self_offset=0)[0])[0]
    assert all(set(a) == set(b) for a, b in zip(idx.tolist(), est.kneighbors(return_distance=False).tolist()))
    want = -est.negative_outlier_factor_
    got = _np(model.lof)[0]
    err = np.max(np.abs(got - want) / want)
    print(f"{name} seed {seed} k {k}: fit vs scikit-learn {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    qi = _np(model.index.query(tq, k)[0])[0]
    assert all(set(a) == set(b) for a, b in zip(qi.tolist(),
                                                est.kneighbors(q.astype(np.float64), return_distance=False).tolist()))
    want_s = -est.score_samples(q.astype(np.float64))
    err = np.max(np.abs(_np(model.score(tq))[0] - want_s) / want_s)
    print(f"{name} seed {seed} k {k}: score vs scikit-learn {err:.3e}")
    assert err <= bound
    t = model.threshold(0.05)
    assert abs(t - np.quantile(want, 0.95)) <= 2 * bound * t


# ---- 5. independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_a_rows_score_does_not_depend_on_the_call(cuda, metric):
    x, q = _rows()
    tx, tq = _gpu(cuda, x, q)
    model = btsbot_amd.NoveltyModel(tx, 20, metric)
    whole = model.score(tq)
    assert torch.isfinite(whole).all()
    single = torch.cat([model.score(tq[i:i + 1]) for i in range(Q)])
    assert torch.equal(whole, single)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(Q)).to(cuda)
    assert torch.equal(model.score(tq[perm]), whole[perm])
    rep = torch.cat([torch.arange(Q, device=cuda), torch.arange(0, Q, 3, device=cuda), torch.arange(Q - 1, -1, -1, device=cuda)])
    assert torch.equal(model.score(tq[rep]), whole[rep])
    for splits in (1, 3, 7):
        assert torch.equal(model.score(tq, splits=splits), whole)
    grown = btsbot_amd.EmbeddingIndex(tx[:200], metric)
    grown.add(tx[200:201]).add(tx[201:])
    again = btsbot_amd.NoveltyModel(grown, 20, metric)
    for a, b in ((again.kdist, model.kdist), (again.lrd, model.lrd), (again.lof, model.lof), (again.score(tq), whole)):
        assert torch.equal(a, b)


def test_a_fit_does_not_follow_add_until_refit(cuda):
    x, q = _rows()
    tx, tq = _gpu(cuda, x, q)
    index = btsbot_amd.EmbeddingIndex(tx[:300])
    model = btsbot_amd.NoveltyModel(index, 10)
    assert len(model) == 300
    index.add(tx[300:])
    assert len(model) == 300
    with pytest.raises(RuntimeError, match="refit"):
        model.score(tq)
    assert model.refit() is model and len(model) == N
    assert torch.equal(model.lof, btsbot_amd.local_outlier_factor(tx, 10))
    assert torch.equal(model.score(tq), btsbot_amd.NoveltyModel(tx, 10).score(tq))


# ---- 6. groups, and the 2-D map ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (31, 32, 33))
def test_excluding_the_own_object_unmasks_the_far_objects(cuda, seed):
    x, obj, planted = R.masking_set(seed)
    tx, tobj = _gpu(cuda, x, obj)
    tp = torch.from_numpy(planted).to(cuda)
    plain = btsbot_amd.local_outlier_factor(tx, 4)
    grouped = btsbot_amd.local_outlier_factor(tx, 4, groups=tobj)
    print(f"seed {seed}: planted alerts ungrouped <= {float(plain[tp].max()):.3f}, own object excluded >= "
          f"{float(grouped[tp].min()):.2f}; all others <= {float(grouped[~tp].max()):.3f}")
    assert bool((plain[tp] < 1.5).all())
    assert bool((grouped[tp] > 3).all()) and bool((grouped[~tp] < 2).all())
    # tonight's alerts of the same objects, scored against the archive without their own object
    model = btsbot_amd.NoveltyModel(tx, 4, groups=tobj)
    assert torch.equal(model.lof, grouped)
    new = tx + 1e-3 * torch.randn(tx.shape, generator=torch.Generator(device=cuda).manual_seed(seed), device=cuda)
    masked = model.score(new)
    shown = model.score(new, query_groups=tobj, exclude_same_group=True)
    assert bool((masked[tp] < 1.5).all()) and bool((shown[tp] > 3).all()) and bool((shown[~tp] < 2).all())
    distinct = model.score(new, one_per_group=True)                       # the nearest OBJECTS, the own one among them
    assert bool(torch.isfinite(distinct).all())


@pytest.mark.parametrize("seed", (21, 22))
def test_the_grid_gives_the_tiles_bits_on_a_map(cuda, seed):
    pts = RR.blobs_2d(seed)
    tp, = _gpu(cuda, pts)
    groups = torch.arange(len(pts), device=cuda) // 3
    for kw in ({}, {"groups": groups}):
        tiles = btsbot_amd.local_outlier_factor(tp, 10, **kw)
        grid = btsbot_amd.local_outlier_factor(tp, 10, method="grid", **kw)
        assert torch.isfinite(tiles).all() and torch.equal(tiles, grid)
    by_map = btsbot_amd.NoveltyModel(btsbot_amd.MapIndex(tp, groups=groups), 10)
    by_rows = btsbot_amd.NoveltyModel(tp, 10, groups=groups)
    assert torch.equal(by_map.lof, by_rows.lof)
    new = tp[:50] + 0.01
    assert torch.equal(by_map.score(new), by_rows.score(new))
    assert torch.equal(by_map.score(new, query_groups=groups[:50], exclude_same_group=True),
                       by_rows.score(new, query_groups=groups[:50], exclude_same_group=True))
    with pytest.raises(ValueError, match="exclude"):
        btsbot_amd.NoveltyModel(btsbot_amd.MapIndex(tp, groups=groups), 10, group_mode="distinct")


def test_kth_neighbor_distance_and_threshold(cuda):
    x, q = _rows()
    tx, tq = _gpu(cuda, x, q)
    model = btsbot_amd.NoveltyModel(tx, 20)
    idx, dist = model.index.query(tq, 20)
    assert torch.equal(btsbot_amd.kth_neighbor_distance(idx, dist), dist[:, 19])
    few = btsbot_amd.EmbeddingIndex(tx[:7]).query(tq, 20)
    assert torch.equal(btsbot_amd.kth_neighbor_distance(*few), few[1][:, 6])
    lof = _np(model.lof)[0]
    for c in (0.01, 0.1, 0.5):
        assert abs(model.threshold(c) - np.quantile(lof, 1 - c)) <= 1e-12 * np.quantile(lof, 1 - c)


# ---- 7. the C entry points ---------------------------------------------------------------------------------------------
def test_c_abi_errors(cuda):
    L = _lib.lib()
    idx = torch.zeros((4, 5), dtype=torch.int64, device=cuda)
    dist = torch.ones((4, 5), dtype=torch.float32, device=cuda)
    a, b, c = (torch.full((4,), 7.0, dtype=torch.float64, device=cuda) for _ in range(3))
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    bad = _lib.ERR_INVALID_ARG
    for k in (0, 65):
        assert L.btsbot_lof_fit(p(idx), p(dist), 4, k, p(a), p(b), p(c), None) == bad
        assert L.btsbot_lof_score(p(idx), p(dist), 4, k, p(a), p(b), 4, p(b), p(c), None) == bad
    assert L.btsbot_lof_fit(p(idx), p(dist), 4, 5, None, p(b), p(c), None) == bad
    assert L.btsbot_lof_fit(p(idx), p(dist), 4, 5, p(a), None, p(c), None) == bad
    assert L.btsbot_lof_score(p(idx), p(dist), 4, 5, p(a), p(b), 4, p(b), None, None) == bad
    assert L.btsbot_lof_fit(p(idx), p(dist), 0, 5, p(a), p(b), p(c), None) == _lib.OK
    assert L.btsbot_lof_score(p(idx), p(dist), 0, 5, p(a), p(b), 4, p(b), p(c), None) == _lib.OK
    torch.cuda.synchronize(cuda)
    assert all(bool((t == 7.0).all()) for t in (a, b, c))     # nothing was launched


# ---- 8. no host read --------------------------------------------------------------------------------------------------
def test_fit_and_score_do_not_synchronise_with_the_host(cuda):
    x, q = _rows()
    tx, tq = _gpu(cuda, x, q)
    obj = torch.arange(N, device=cuda) // 4
    want = (btsbot_amd.local_outlier_factor(tx, 20), btsbot_amd.local_outlier_factor(tx, 20, groups=obj),
            btsbot_amd.NoveltyModel(tx, 20).score(tq))
    torch.cuda.synchronize(cuda)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                # a host read is an error in this mode
    try:
        got = (btsbot_amd.local_outlier_factor(tx, 20), btsbot_amd.local_outlier_factor(tx, 20, groups=obj),
               btsbot_amd.NoveltyModel(tx, 20).score(tq))
        btsbot_amd.NoveltyModel(tx, 20, groups=obj).score(tq, query_groups=obj[:Q], exclude_same_group=True, return_lrd=True)
        btsbot_amd.kth_neighbor_distance(*btsbot_amd.EmbeddingIndex(tx).query(tq, 5))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


# ---- run_training --------------------------------------------------------------------------------------------------------
def test_run_training_writes_the_lof_file_on_request(cuda, tmp_path):
    import pandas as pd
    from btsbot_amd.alert_utils import object_keys
    from btsbot_amd.synthetic import synthetic_batch
    from btsbot_amd.train import run_training
    from helpers import CONFIGS, METADATA_COLS
    _, meta, _ = synthetic_batch(448, seed=21)
    lab = (meta[:, 5] > meta[:, 5].median()).long().numpy()
    d = tmp_path / "data"
    d.mkdir()
    names = [f"obj{i // 4}" for i in range(64)]
    for split, sl in (("train", slice(0, 256)), ("val", slice(256, 384)), ("test", slice(384, 448))):
        df = pd.DataFrame(meta[sl].numpy(), columns=METADATA_COLS)
        df["label"] = lab[sl]
        if split == "test":
            df["objectId"] = names
        df.to_csv(d / f"{split}_cand_v11_N100.csv", index=False)
    cfg = dict(CONFIGS["um_nn"][1], model_name="um_nn", train_data_version="v11", epochs=2, batch_size=64,
               learning_rate="3e-3", warmup_epochs=1, beta_1=0.9, beta_2=0.999, patience=3, random_seed=2,
               generate_embeddings=True, embedding_novelty={"k": 5, "group_by": "objectId"})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hist, _ = run_training(cfg, data_base_dir=str(tmp_path) + "/", run_name="n0", device=cuda, precision="f32",
                               models_root=str(tmp_path / "models"), embeddings_root=str(tmp_path / "embeddings"))
    stem = str(tmp_path / "embeddings" / "um_nn_n0")
    assert hist["embeddings_file"] == stem + ".npy" and not os.path.exists(stem + "_knn.npz")
    emb, lof = np.load(stem + ".npy"), np.load(stem + "_lof.npy")
    assert lof.dtype == np.float64 and lof.shape == (64,)
    groups = torch.from_numpy(object_keys(names)).to(cuda)
    _same_bits(lof, _np(btsbot_amd.local_outlier_factor(torch.from_numpy(emb).to(cuda), 5, groups=groups))[0])
