"""GPU tests of the embedding layout (run with -m gpu on an MI355X): fuzzy_graph / optimize_layout / embedding_layout
against the float64 restatement of tests/layout_ref.py -- the graph exactly (sigma and the weights up to exp's last bits),
every epoch one at a time under the bound |dy| <= EPOCH_C 2^-24 (|y| + alpha sum |term|) -- against themselves bit for
bit (runs, stepping, grid size), and as a map: trustworthiness and label purity of ten Gaussian clusters."""
import os
import warnings

import numpy as np
import pytest
import torch

import btsbot_amd
import layout_ref as R
from btsbot_amd.layout import FuzzyGraph

pytestmark = pytest.mark.gpu

A, B = btsbot_amd.find_ab_params(1.0, 0.1)
KINDS = ("normal", "clusters", "tripled", "integer", "outlier", "short")


def _rows(kind, n, k, seed):
    rng = np.random.default_rng(seed)
    d = 5
    if kind == "normal":
        x = rng.standard_normal((n, d))
    elif kind == "clusters":                                   # clusters of sigma 0.01 at offset 10
        x = 10.0 + 3.0 * rng.standard_normal((4, d))[np.arange(n) % 4] + 0.01 * rng.standard_normal((n, d))
    elif kind == "tripled":                                    # every row three times: distance 0 beyond column 0
        x = rng.standard_normal(((n + 2) // 3, d))[np.arange(n) // 3]
    elif kind == "integer":                                    # ties
        x = rng.integers(-8, 9, size=(n, 2)).astype(np.float64)
    elif kind == "outlier":
        x = rng.standard_normal((n, d))
        x[n // 2] = 1e4
    else:                                                      # fewer rows than columns: tails of idx = -1
        x = rng.standard_normal((k - 1, d))
    return x.astype(np.float32)


def _dev_graph(g):
    return tuple(t.cpu().numpy() for t in (g.indptr, g.indices, g.weights, g.sigma, g.rho))


@pytest.mark.parametrize("n,k", [(3, 2), (65, 15), (257, 64), (1000, 33)])
def test_graph_equals_the_restatement(cuda, n, k):
    for kind in KINDS:
        emb = torch.from_numpy(_rows(kind, n, k, n + k)).to(cuda)
        idx, dist = btsbot_amd.knn_graph(emb, k, include_self=True)
        g = btsbot_amd.fuzzy_graph(idx, dist)
        ref = R.fuzzy_graph(idx.cpu().numpy(), dist.cpu().numpy())
        ds, dw = R.check_graph(_dev_graph(g), ref)
        print(f"N={n} k={k} {kind}: E={g.n_edges}, sigma off {ds:.2e} relative, weights off {dw:.2e}")
        if kind == "short":
            assert (idx[:, -1] == -1).all()
        assert float(g.w_max) == (ref.weights.max() if len(ref.weights) else 0.0)


def test_graph_of_a_non_finite_row_and_of_nothing(cuda):
    x = _rows("normal", 65, 15, 1)
    x[7, 2] = np.nan
    idx, dist = btsbot_amd.knn_graph(torch.from_numpy(x).to(cuda), 15)
    g = btsbot_amd.fuzzy_graph(idx, dist)
    R.check_graph(_dev_graph(g), R.fuzzy_graph(idx.cpu().numpy(), dist.cpu().numpy()))
    indptr = g.indptr.cpu().numpy()
    assert indptr[8] == indptr[7] and not (g.indices == 7).any()
    g = btsbot_amd.fuzzy_graph(idx[:0], dist[:0])
    assert g.n == 0 and g.n_edges == 0 and g.indices.shape == (0,)


# ---- one epoch at a time
def _epoch_case(name):
    """(restatement graph, positions float32 [N, 2]) with coincident points on edges and under samples, and a NaN row."""
    rng = np.random.default_rng(len(name))
    if name == "pair":
        return R.graph_from_pairs(2, {(0, 1): np.float32(1.0)}), np.array([[0.5, -0.25], [-1.0, 2.0]], dtype=np.float32)
    if name.startswith("hub"):
        # vertex 0 has n - 2 slots once vertex 5 is dropped: 128 (the longest row a group of lanes walks alone), 129 (the
        # shortest the whole workgroup walks) and 298 (two trips of the workgroup)
        n = int(name[3:])
        g = R.hub_graph(n, 4)
    else:
        n, k = {"knn65": (65, 5), "knn1025": (1025, 15)}[name]
        g = R.fuzzy_graph(*R.knn_exact(rng.standard_normal((n, 5)).astype(np.float32), k))
    y = (4.0 * rng.standard_normal((n, 2))).astype(np.float32)
    y[3::7] = y[3]                                             # coincident points under negative samples ...
    rows = np.repeat(np.arange(n), np.diff(g.indptr))
    for e in range(0, len(rows), max(len(rows) // 9, 1)):      # ... and on edges
        if rows[e] != 5 and g.indices[e] != 5:
            y[g.indices[e]] = y[rows[e]]
    g = R.drop_vertex(g, 5)
    y[5] = np.nan
    return g, y


def _upload(g, dev):
    w = torch.from_numpy(g.weights).to(dev)
    return FuzzyGraph(torch.from_numpy(g.indptr).to(dev), torch.from_numpy(g.indices).to(dev), w,
                      w.max().reshape(1) if len(g.weights) else torch.zeros(1, device=dev), None, None)


@pytest.mark.parametrize("n_epochs", [10, 200])
@pytest.mark.parametrize("name", ["pair", "knn65", "hub130", "hub131", "hub300", "knn1025"])
def test_each_epoch_against_the_restatement(cuda, name, n_epochs):
    g, y = _epoch_case(name)
    dg, dy = _upload(g, cuda), torch.from_numpy(y).to(cuda)
    worst, stats = 0.0, {}
    for rate in (0, 1, 5):
        for n in (1, 2, n_epochs // 2, n_epochs):
            got = btsbot_amd.optimize_layout(dg, dy, n_epochs, A, B, seed=3, negative_sample_rate=rate, first_epoch=n,
                                             last_epoch=n).cpu().numpy()
            ref, scale = R.epoch(g, y, n, n_epochs, A, B, 3, rate, stats=stats)
            ratio = R.epoch_ratio(got, ref, scale)
            print(f"{name} epoch {n}/{n_epochs} rate {rate}: {ratio:.2f} x 2^-24")
            worst = max(worst, ratio)
    # five consecutive epochs, the device stepping from its own output
    cur = dy
    for n in range(1, 6):
        nxt = btsbot_amd.optimize_layout(dg, cur, n_epochs, A, B, seed=3, first_epoch=n, last_epoch=n)
        ref, scale = R.epoch(g, cur.cpu().numpy(), n, n_epochs, A, B, 3, 5, stats=stats)
        worst = max(worst, R.epoch_ratio(nxt.cpu().numpy(), ref, scale))
        cur = nxt
    print(f"{name} / {n_epochs}: worst {worst:.2f} x 2^-24 (bound {R.EPOCH_C:g}); events {stats}")
    if name == "pair":
        assert stats["self_sample"] > 0
    else:
        assert stats["coincident_edge"] > 0 and stats["coincident_sample"] > 0 and stats["nan_sample"] > 0
    if name.startswith("hub"):
        assert int(np.diff(g.indptr).max()) == int(name[3:]) - 2 > 64   # a row longer than a wave
    assert worst <= R.EPOCH_C, f"epoch error is {worst:.1f} x 2^-24 of (|y| + alpha sum |term|), bound {R.EPOCH_C}"


# ---- determinism
def _bits(t):
    return t.contiguous().view(torch.int32)


def test_layout_is_reproducible_bit_for_bit(cuda):
    emb = torch.from_numpy(R.cluster_set(1025, 16, 2)[0]).to(cuda)
    y1 = btsbot_amd.embedding_layout(emb, n_epochs=30, seed=4)
    y2 = btsbot_amd.embedding_layout(emb, n_epochs=30, seed=4)
    assert torch.isfinite(y1).all() and torch.equal(_bits(y1), _bits(y2))
    assert not torch.equal(_bits(y1), _bits(btsbot_amd.embedding_layout(emb, n_epochs=30, seed=5)))
    knn = btsbot_amd.knn_graph(emb, 15)
    assert torch.equal(_bits(y1), _bits(btsbot_amd.embedding_layout(emb, n_epochs=30, seed=4, knn=knn)))
    g = btsbot_amd.fuzzy_graph(*knn)
    y0 = btsbot_amd.embedding_layout(emb, n_epochs=1, seed=4, init="random", learning_rate=1e-30)   # ~ the initial positions
    whole = btsbot_amd.optimize_layout(g, y0, 20, A, B, seed=4)
    step = y0
    for n in range(1, 21):
        step = btsbot_amd.optimize_layout(g, step, 20, A, B, seed=4, first_epoch=n, last_epoch=n)
    assert torch.equal(_bits(whole), _bits(step))
    two = btsbot_amd.optimize_layout(g, btsbot_amd.optimize_layout(g, y0, 20, A, B, seed=4, last_epoch=7), 20, A, B, seed=4,
                                     first_epoch=8)
    assert torch.equal(_bits(whole), _bits(two))
    for blocks in (1, 3, 1000):
        assert torch.equal(_bits(whole), _bits(btsbot_amd.optimize_layout(g, y0, 20, A, B, seed=4, blocks=blocks))), blocks


def test_layout_does_not_synchronise_with_the_host(cuda):
    emb = torch.from_numpy(R.cluster_set(300, 8, 5)[0]).to(cuda)
    knn = btsbot_amd.knn_graph(emb, 15)
    btsbot_amd.embedding_layout(emb, n_epochs=5, init="random")           # warm: code objects, the allocator's blocks
    torch.cuda.synchronize(cuda)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            btsbot_amd.embedding_layout(emb, n_epochs=5, init="pca")      # the one host read: the covariance
            control = False
        except RuntimeError:
            control = True                                                 # a host read is an error in this mode
        if control:
            y = btsbot_amd.embedding_layout(emb, n_epochs=5, init="random")
            y = btsbot_amd.embedding_layout(emb, n_epochs=5, init=y, knn=knn)
            g = btsbot_amd.fuzzy_graph(*knn)
            y = btsbot_amd.optimize_layout(g, y, 5, A, B, first_epoch=2, last_epoch=4)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not control:
        pytest.skip("this build of torch does not report a host read in sync debug mode: nothing to tell the calls by")
    assert torch.isfinite(y).all() and g.n_edges > 0


def test_random_init_equals_the_restatement(cuda):
    emb = torch.from_numpy(R.cluster_set(300, 8, 2)[0]).to(cuda)
    g = btsbot_amd.fuzzy_graph(*btsbot_amd.knn_graph(emb, 5))
    # one epoch at a vanishing learning rate moves nothing: the result IS the initial position
    y0 = btsbot_amd.embedding_layout(emb, n_neighbors=5, n_epochs=1, seed=9, init="random", learning_rate=1e-30)
    assert np.array_equal(y0.cpu().numpy(), R.random_init(300, 9))
    given = torch.from_numpy(R.random_init(300, 1)).to(cuda)
    y = btsbot_amd.embedding_layout(emb, n_neighbors=5, n_epochs=3, seed=9, init=given)
    assert torch.equal(_bits(y), _bits(btsbot_amd.optimize_layout(g, given, 3, A, B, seed=9)))
    p0 = btsbot_amd.embedding_layout(emb, n_neighbors=5, n_epochs=1, seed=9, learning_rate=1e-30).cpu().numpy()
    want = R.pca_init(emb.cpu().numpy(), 9)
    assert np.abs(p0 - want).max() <= 1e-3 and abs(np.abs(p0).max() - 10) <= 1e-3


# ---- quality
@pytest.fixture(scope="module")
def quality_set():
    X, labels = R.cluster_set(512, 32, 1)
    return X, labels, R.trustworthiness(X, R.pca_init(X, 0), 15)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_quality_of_the_map(cuda, quality_set, seed):
    X, labels, t_pca = quality_set
    emb = torch.from_numpy(X).to(cuda)
    knn = btsbot_amd.knn_graph(emb, 15)
    y = btsbot_amd.embedding_layout(emb, n_neighbors=15, n_epochs=200, init="pca", seed=seed, knn=knn).cpu().numpy()
    # the restatement from the device's own graph and initial positions
    g = R.fuzzy_graph(knn[0].cpu().numpy(), knn[1].cpu().numpy())
    y0 = btsbot_amd.embedding_layout(emb, n_epochs=1, init="pca", seed=seed, knn=knn, learning_rate=1e-30).cpu().numpy()
    t_ref = R.trustworthiness(X, R.layout(g, y0, 200, A, B, seed=seed), 15)
    t_dev, purity = R.trustworthiness(X, y, 15), R.label_purity(y, labels, 5)
    print(f"seed {seed}: trustworthiness {t_dev:.4f} (restatement {t_ref:.4f}, PCA {t_pca:.4f}), purity {purity:.4f}")
    assert np.isfinite(y).all()
    assert t_dev >= t_ref - 0.01 and t_dev >= 0.955
    assert purity >= 0.99


def test_quality_from_random_positions(cuda, quality_set):
    X, _labels, t_pca = quality_set
    y = btsbot_amd.embedding_layout(torch.from_numpy(X).to(cuda), n_epochs=200, init="random", seed=0).cpu().numpy()
    t = R.trustworthiness(X, y, 15)
    print(f"init='random': trustworthiness {t:.4f} (PCA {t_pca:.4f})")
    assert np.isfinite(y).all() and t > t_pca


def test_non_finite_rows_have_nan_positions(cuda):
    X, _ = R.cluster_set(300, 8, 3)
    X[[4, 250], [1, 7]] = [np.nan, np.inf]
    for init in ("pca", "random"):
        y = btsbot_amd.embedding_layout(torch.from_numpy(X).to(cuda), n_epochs=20, init=init).cpu().numpy()
        assert np.isnan(y[[4, 250]]).all() and np.isfinite(np.delete(y, [4, 250], axis=0)).all()
    assert btsbot_amd.embedding_layout(torch.zeros((0, 8), device=cuda)).shape == (0, 2)


# ---- write_embeddings
def test_run_training_writes_the_map_on_request(cuda, tmp_path):
    import pandas as pd
    from btsbot_amd import architectures
    from btsbot_amd.synthetic import synthetic_batch
    from btsbot_amd.train import run_training, write_embeddings
    from helpers import CONFIGS, METADATA_COLS
    _, meta, _ = synthetic_batch(448, seed=21)
    lab = (meta[:, 5] > meta[:, 5].median()).long().numpy()
    d = tmp_path / "data"
    d.mkdir()
    for split, sl in (("train", slice(0, 256)), ("val", slice(256, 384)), ("test", slice(384, 448))):
        df = pd.DataFrame(meta[sl].numpy(), columns=METADATA_COLS)
        df["label"] = lab[sl]
        if split == "test":
            df["candid"] = np.arange(sl.start, sl.stop) + 1_000_000
        df.to_csv(d / f"{split}_cand_v11_N100.csv", index=False)
    cfg = dict(CONFIGS["um_nn"][1], model_name="um_nn", train_data_version="v11", epochs=2, batch_size=64,
               learning_rate="3e-3", warmup_epochs=1, beta_1=0.9, beta_2=0.999, patience=3, random_seed=2,
               generate_embeddings=True, embedding_layout={"n_neighbors": 5, "n_epochs": 50})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hist, model_dir = run_training(cfg, data_base_dir=str(tmp_path) + "/", run_name="u0", device=cuda, precision="f32",
                                       models_root=str(tmp_path / "models"), embeddings_root=str(tmp_path / "embeddings"))
    stem = str(tmp_path / "embeddings" / "um_nn_u0")
    assert hist["embeddings_file"] == stem + ".npy"
    assert sorted(os.listdir(tmp_path / "embeddings")) == ["um_nn_u0.csv", "um_nn_u0.npy", "um_nn_u0_umap.csv"]
    table = pd.read_csv(stem + "_umap.csv")
    assert list(table.columns) == ["umap_emb_1", "umap_emb_2", "candid"]
    assert list(table["candid"]) == list(np.arange(384, 448) + 1_000_000)
    y = table[["umap_emb_1", "umap_emb_2"]].to_numpy()
    assert y.shape == (64, 2) and np.isfinite(y).all()
    emb = torch.from_numpy(np.load(stem + ".npy")).to(cuda)
    want = btsbot_amd.embedding_layout(emb, n_neighbors=5, n_epochs=50, seed=2).cpu().numpy()   # seed: the run's random_seed
    assert np.allclose(y, want, rtol=1e-6, atol=0)             # (the CSV's decimal digits)
    # without the key: today's files, byte for byte
    plain = {k: v for k, v in cfg.items() if k != "embedding_layout"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = getattr(architectures, "um_nn")(plain, precision="f32")
        write_embeddings(model, plain, str(tmp_path) + "/", model_dir, str(tmp_path / "plain" / "um_nn_u0"), batch_size=64,
                         device=cuda)
    assert sorted(os.listdir(tmp_path / "plain")) == ["um_nn_u0.csv", "um_nn_u0.npy"]
    for ext in (".npy", ".csv"):
        assert open(stem + ext, "rb").read() == open(str(tmp_path / "plain" / "um_nn_u0") + ext, "rb").read()
