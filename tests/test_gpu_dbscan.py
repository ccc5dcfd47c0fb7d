"""GPU tests of graph_components and dbscan (run with -m gpu on an MI355X): labels and core masks equal the numpy rule of
tests/radius_ref.py -- which equals scikit-learn's DBSCAN, tests/test_radius_host.py -- exactly, on sets that have no
pair within the band of eps; the components equal scipy's on a random masked graph."""
import warnings

import numpy as np
import pytest
import torch

import btsbot_amd
import radius_ref as R

pytestmark = pytest.mark.gpu


def _dbscan(cuda, X, eps, min_samples, **kw):
    labels, core = btsbot_amd.dbscan(torch.from_numpy(X).to(cuda), eps, min_samples, **kw)
    assert labels.dtype == torch.int64 and core.dtype == torch.bool and labels.shape == core.shape == (len(X),)
    return labels.cpu().numpy(), core.cpu().numpy()


@pytest.mark.parametrize("name, X, eps, min_samples", R.dbscan_sets(), ids=lambda v: v if isinstance(v, str) else None)
def test_labels_and_core_equal_the_rule_exactly(cuda, name, X, eps, min_samples):
    assert R.pairs_in_band(X, eps) == 0                       # on the CPU, first: equality is then the contract
    want_l, want_c = R.dbscan_ref(X, eps, min_samples)
    labels, core = _dbscan(cuda, X, eps, min_samples)
    assert np.array_equal(core, want_c)
    assert np.array_equal(labels, want_l)


def test_a_chain_across_tile_edges_is_one_cluster(cuda):
    X = np.zeros((600, 2), np.float32)
    X[:, 0] = np.arange(600) * 0.5
    X = X[np.random.default_rng(1).permutation(600)]
    assert R.pairs_in_band(X, 0.75) == 0
    labels, core = _dbscan(cuda, X, 0.75, 3)
    want_l, want_c = R.dbscan_ref(X, 0.75, 3)
    assert np.array_equal(labels, want_l) and np.array_equal(core, want_c)
    assert (labels == 0).all() and core.sum() == 598         # the two ends see one neighbour and themselves


def test_all_noise_min_samples_one_and_the_border_row(cuda):
    X = R.blobs_2d(11)
    labels, core = _dbscan(cuda, X, 1e-4, 2)
    assert (labels == -1).all() and not core.any()
    labels, core = _dbscan(cuda, X, 1e-4, 1)                  # every row is a cluster of its own, numbered by row
    assert core.all() and np.array_equal(labels, np.arange(360))
    bad = X.copy()
    bad[[7, 200], [0, 1]] = [np.nan, np.inf]                  # no neighbours, not even themselves
    labels, core = _dbscan(cuda, bad, 1e-4, 1)
    assert not core[[7, 200]].any() and (labels[[7, 200]] == -1).all() and labels.max() == 357
    X, eps, min_samples, border = R.border_set()
    labels, core = _dbscan(cuda, X, eps, min_samples)
    assert labels.tolist() == [0] * 5 + [0] + [1] * 5 and not core[border] and core.sum() == 10


def test_groups_count_objects_not_alerts(cuda):
    rng = np.random.default_rng(3)
    centres = rng.uniform(0, 1000, size=(512, 2))
    X = (np.repeat(centres, 5, axis=0) + rng.normal(0, 0.01, size=(2560, 2))).astype(np.float32)
    obj = np.repeat(np.arange(512) * 7 - 100, 5).astype(np.int64)
    perm = rng.permutation(2560)
    X, obj = X[perm], obj[perm]
    # ... and one place where single alerts of six different objects meet
    X = np.r_[X, (np.float32(2000) + rng.normal(0, 0.01, size=(6, 2))).astype(np.float32)]
    obj = np.r_[obj, 10000 + np.arange(6)]
    eps = 0.2
    assert R.pairs_in_band(X, eps) == 0
    # (five alerts reach a count of 5, the row itself included: min_samples = 5 makes every object a cluster without
    #  groups; min_samples = 6, as the clump of six shows, cannot)
    labels, core = _dbscan(cuda, X, eps, 5)
    want_l, want_c = R.dbscan_ref(X, eps, 5)
    assert np.array_equal(labels, want_l) and np.array_equal(core, want_c)
    assert core.all() and labels.max() >= 500
    tg = torch.from_numpy(obj).to(cuda)
    for min_samples in (5, 6):
        labels, core = _dbscan(cuda, X, eps, min_samples, groups=tg)
        want_l, want_c = R.dbscan_ref(X, eps, min_samples, groups=obj)
        assert np.array_equal(labels, want_l) and np.array_equal(core, want_c)
        assert core[-6:].all() and core.sum() == 6 and (labels[-6:] == 0).all() and (labels[:-6] == -1).all()


def _numpy_components(n, rows, cols, mask):
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for u, v in zip(rows.tolist(), cols.tolist()):
        if mask[u] and mask[v]:
            a, b = find(u), find(v)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(i) if mask[i] else -1 for i in range(n)], np.int64)


@pytest.mark.parametrize("n, degree", [(1, 0), (1000, 1), (5000, 2), (70000, 1)])
def test_graph_components_on_a_random_masked_graph(cuda, n, degree):
    rng = np.random.default_rng(n)
    rows = np.repeat(np.arange(n), degree)
    cols = rng.integers(0, n, size=len(rows))
    rows, cols = np.r_[rows, cols[: len(cols) // 2]], np.r_[cols, rows[: len(cols) // 2]]   # some edges in both lists
    order = np.argsort(rows, kind="stable")
    rows, cols = rows[order], cols[order]
    indptr = np.r_[0, np.cumsum(np.bincount(rows, minlength=n))].astype(np.int64)
    mask = rng.random(n) < 0.8
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import connected_components
        keep = mask[rows] & mask[cols]
        g = csr_matrix((np.ones(keep.sum()), (rows[keep], cols[keep])), shape=(n, n))
        _, comp = connected_components(g, directed=False)
        first = np.full(comp.max() + 1, n)
        np.minimum.at(first, comp, np.arange(n))
        want = np.where(mask, first[comp], -1)
    except ImportError:
        want = _numpy_components(n, rows, cols, mask)
    ip, ii, m = (torch.from_numpy(a).to(cuda) for a in (indptr, cols.astype(np.int64), mask))
    root = btsbot_amd.graph_components(ip, ii, m)
    assert root.dtype == torch.int64 and np.array_equal(root.cpu().numpy(), want)
    assert torch.equal(btsbot_amd.graph_components(ip, ii, m), root)
    full = btsbot_amd.graph_components(ip, ii).cpu().numpy()
    assert np.array_equal(full, _numpy_components(n, rows, cols, np.ones(n, bool)))


def test_a_radius_graph_can_be_reused(cuda):
    name, X, eps, min_samples = R.dbscan_sets()[0]
    t = torch.from_numpy(X).to(cuda)
    indptr, indices, _dist = btsbot_amd.radius_graph(t, eps, include_self=True)
    for ms in (min_samples, 8):
        l1, c1 = btsbot_amd.dbscan(t, eps, ms, graph=(indptr, indices))
        l2, c2 = btsbot_amd.dbscan(t, eps, ms)
        assert torch.equal(l1, l2) and torch.equal(c1, c2)
    with pytest.raises(ValueError, match="indptr"):
        btsbot_amd.dbscan(t, eps, graph=(indptr[:-1], indices))


def test_run_training_writes_the_clusters_only_when_asked(cuda, tmp_path, capsys):
    import os
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
                generate_embeddings=True, embedding_layout={"n_epochs": 30, "n_neighbors": 8})
    for run, on in (("c0", "map"), ("c1", "embedding")):
        cfg = dict(base, embedding_clusters={"eps": 0.5, "min_samples": 3, "on": on})
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            run_training(cfg, data_base_dir=str(tmp_path) + "/", run_name=run, device=cuda, precision="f32",
                         models_root=str(tmp_path / "models"), embeddings_root=str(tmp_path / "embeddings"))
        stem = str(tmp_path / "embeddings" / f"um_nn_{run}")
        table = pd.read_csv(stem + "_umap.csv")
        if on == "map":
            assert list(table.columns) == ["umap_emb_1", "umap_emb_2", "cluster"] and len(table) == 64
            assert table["cluster"].dtype == np.int64 and (table["cluster"] >= -1).all()
            assert not os.path.exists(stem + "_clusters.npy")
        else:
            assert list(table.columns) == ["umap_emb_1", "umap_emb_2"]
            emb = torch.from_numpy(np.load(stem + ".npy")).to(cuda)
            labels = np.load(stem + "_clusters.npy")
            assert labels.dtype == np.int64 and np.array_equal(labels, btsbot_amd.dbscan(emb, 0.5, 3)[0].cpu().numpy())
    # a config that cannot be answered ends the embedding step as any of its errors does: reported, the run goes on
    capsys.readouterr()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hist, _ = run_training(dict(base, embedding_clusters={"eps": 0.5, "on": "rows"}), data_base_dir=str(tmp_path) + "/",
                               run_name="c2", device=cuda, precision="f32", models_root=str(tmp_path / "models"),
                               embeddings_root=str(tmp_path / "embeddings"))
    said = capsys.readouterr().out
    assert "Error generating embeddings" in said and "config['embedding_clusters']" in said
    assert "embeddings_file" not in hist and not os.path.exists(str(tmp_path / "embeddings" / "um_nn_c2_umap.csv"))
