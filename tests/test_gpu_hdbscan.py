"""GPU tests of mutual_reachability_mst, ClusterTree and hdbscan (run with -m gpu on an MI355X): the tree is a minimum
spanning tree of the mutual-reachability graph with the direct-form bits, and labels equal the float64 restatement of
tests/hdbscan_ref.py -- which equals scikit-learn's HDBSCAN where that agrees with itself, tests/test_hdbscan_host.py --
exactly, on sets that keep their labels under fp32-sized noise (checked on the host, same file)."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import btsbot_amd
import hdbscan_ref as R
import radius_ref

pytestmark = pytest.mark.gpu

SETS_32D = [f"32d:{s}" for s in R.SEEDS_32D]
SETS_2D = [f"2d:{s}" for s in R.SEEDS_2D]
FLAT = SETS_2D + ["lattice"]                     # the sets the grid can hold


@functools.lru_cache(maxsize=None)
def _set(name):
    kind, _, seed = name.partition(":")
    if kind == "32d":
        return R.blobs_32d(int(seed)), None
    if kind == "2d":
        return R.blobs_2d(int(seed)), None
    if kind == "lattice":
        return R.lattice(), None
    if kind == "clumps":
        return R.clumps_2d(), None
    if kind == "70d":
        return R.blobs_70d(), None
    return R.object_set()


@functools.lru_cache(maxsize=None)
def _dist(name):
    return R.dist_matrix(_set(name)[0])


@functools.lru_cache(maxsize=None)
def _ref(name, mcs, ms, grouped=False):
    return R.hdbscan_ref(_dist(name), mcs, ms, groups=_set(name)[1] if grouped else None)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _spans(edges, rows, n):
    """a host union-find: the edges join exactly ``rows`` into one tree"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in edges.tolist():
        ra, rb = find(a), find(b)
        if ra == rb:
            return False
        parent[ra] = rb
    return len({find(r) for r in rows.tolist()}) == 1 and set(np.unique(edges).tolist()) == set(rows.tolist())


def _close(got, want, rel):
    return bool((np.abs(got - want) <= rel * np.abs(want)).all())


# ---- 1. the tree is a minimum spanning tree ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,method", [(n, "tiles") for n in SETS_32D + FLAT + ["objects"]] + [(n, "grid") for n in FLAT])
def test_the_tree_is_a_minimum_spanning_tree(cuda, name, method):
    X = _set(name)[0]
    n, dim = X.shape
    t = torch.from_numpy(X).to(cuda)
    stats = {}
    mst = btsbot_amd.mutual_reachability_mst(t, 5, method=method, stats=stats)
    print(f"{name} {method}: {stats}")
    assert mst.edges.dtype == torch.int64 and mst.edges.shape == (n - 1, 2) and mst.weights.dtype == torch.float32
    assert mst.core.shape == (n,) and stats["rounds"] == len(stats["components"]) <= int(np.ceil(np.log2(n))) + 1
    assert _spans(mst.edges.cpu().numpy(), np.arange(n), n)
    core = btsbot_amd.knn_graph(t, 4, include_self=False, method=method)[1][:, -1]
    assert torch.equal(_bits(mst.core), _bits(core.contiguous()))
    a, b = mst.edges[:, 0], mst.edges[:, 1]
    dist = btsbot_amd.EmbeddingIndex(t).rank_of(t[a], b[:, None].contiguous())[1][:, 0]
    want = torch.maximum(dist, torch.maximum(mst.core[a], mst.core[b]))
    assert torch.equal(_bits(mst.weights), _bits(want))
    ref = _ref(name, 5, 5)
    got_w, ref_w = np.sort(mst.weights.cpu().numpy().astype(np.float64)), np.sort(ref["weights"])
    assert _close(got_w, ref_w, R.band(dim))
    if name == "lattice":
        assert np.array_equal(got_w, ref_w)


# ---- 2. labels and probabilities ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,method", [(n, "tiles") for n in SETS_32D + FLAT] + [(n, "grid") for n in FLAT])
def test_labels_equal_the_restatement(cuda, name, method):
    X = _set(name)[0]
    t = torch.from_numpy(X).to(cuda)
    for mcs, ms in R.PAIRS:
        labels, prob = btsbot_amd.hdbscan(t, mcs, ms, method=method)
        assert labels.dtype == torch.int64 and prob.dtype == torch.float64 and labels.shape == prob.shape == (len(X),)
        ref = _ref(name, mcs, ms)
        got_p = prob.cpu().numpy()
        worst = float((np.abs(got_p - ref["prob"]) / np.where(ref["prob"] > 0, ref["prob"], 1)).max())
        print(f"{name} {method} ({mcs}, {ms}): {int(labels.max()) + 1} clusters, {int((labels < 0).sum())} noise rows, "
              f"worst relative probability error {worst:.2e}")
        assert np.array_equal(labels.cpu().numpy(), ref["labels"])
        assert _close(got_p, ref["prob"], 4 * R.band(X.shape[1]))


# ---- 3. invariance -----------------------------------------------------------------------------------------------------
def _answer(t, method, **kw):
    mst = btsbot_amd.mutual_reachability_mst(t, 5, method=method, **kw)
    labels, prob = btsbot_amd.ClusterTree(mst).labels(10)
    return torch.sort(mst.weights).values, labels, prob


@pytest.mark.parametrize("name,method", [("32d:0", "tiles"), ("2d:0", "tiles"), ("2d:0", "grid")])
def test_no_answer_depends_on_search_k_splits_method_or_row_order(cuda, name, method):
    X = _set(name)[0]
    t = torch.from_numpy(X).to(cuda)
    base = _answer(t, method)
    others = [dict(search_k=k) for k in (1, 3, 64)]
    if method == "tiles":
        others += [dict(splits=s) for s in (1, 2, 5)]
    for kw in others:
        stats = {}
        got = _answer(t, method, stats=stats, **kw)
        print(f"{name} {method} {kw}: unresolved per round {stats['unresolved']}")
        if kw.get("search_k") == 1:
            assert sum(stats["unresolved"]) > 0               # the radius tier ran
        for a, b in zip(base, got):
            assert torch.equal(_bits(a), _bits(b)), kw
    if method == "grid":
        for a, b in zip(base, _answer(t, "tiles")):
            assert torch.equal(_bits(a), _bits(b))
    perm = np.random.default_rng(5).permutation(len(X))
    w, labels, prob = _answer(torch.from_numpy(X[perm]).to(cuda), method)
    assert torch.equal(_bits(w), _bits(base[0]))
    assert R.same_partition(base[1].cpu().numpy()[perm], labels.cpu().numpy())
    assert np.array_equal(base[2].cpu().numpy()[perm], prob.cpu().numpy())


# ---- 4. larger N --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,method", [("clumps", "grid"), ("70d", "tiles")])
def test_larger_sets_cross_tiles_workgroups_and_rounds(cuda, name, method):
    X = _set(name)[0]
    stats = {}
    t = torch.from_numpy(X).to(cuda)
    tree = btsbot_amd.ClusterTree(btsbot_amd.mutual_reachability_mst(t, 5, method=method, stats=stats))
    labels, prob = tree.labels(10)
    ref = _ref(name, 10, 5)
    print(f"{name}: N = {len(X)}, {stats}, {int(labels.max()) + 1} clusters")
    assert stats["rounds"] >= 3 and len(tree.mst) == len(X) - 1
    assert np.array_equal(labels.cpu().numpy(), ref["labels"])
    assert _close(prob.cpu().numpy(), ref["prob"], 4 * R.band(X.shape[1]))


# ---- 5. a cut of the tree is DBSCAN on its core rows --------------------------------------------------------------------
@pytest.mark.parametrize("name, X, eps, min_samples", radius_ref.dbscan_sets(),
                         ids=lambda v: v if isinstance(v, str) else None)
def test_a_cut_of_the_tree_is_dbscan_on_its_core_rows(cuda, name, X, eps, min_samples):
    assert radius_ref.pairs_in_band(X, eps) == 0
    t = torch.from_numpy(X).to(cuda)
    labels, core = btsbot_amd.dbscan(t, eps, min_samples)
    tree = btsbot_amd.ClusterTree(btsbot_amd.mutual_reachability_mst(t, min_samples))
    cut = tree.cut(eps)
    assert cut.dtype == torch.int64 and torch.equal(cut >= 0, core)
    assert torch.equal(cut[core], labels[core])
    big = tree.cut(eps, min_cluster_size=20)
    sizes = torch.bincount(cut[core])
    assert torch.equal(big >= 0, core & (sizes[cut.clamp(min=0)] >= 20))
    assert R.same_partition(big.cpu().numpy(), torch.where(big >= 0, cut, big).cpu().numpy())
    assert int(big.max()) + 1 == int((sizes >= 20).sum())


# ---- 6. groups ----------------------------------------------------------------------------------------------------------
def test_groups_dissolve_the_objects_into_the_real_clusters(cuda):
    X, obj = _set("objects")
    t, g = torch.from_numpy(X).to(cuda), torch.from_numpy(obj).to(cuda)
    plain, _ = btsbot_amd.hdbscan(t, 5, 5)
    plain = plain.cpu().numpy()
    # five near-identical alerts: every object is a cluster of its own
    assert plain.min() >= 0 and len(set(plain.tolist())) == len(set(obj.tolist()))
    assert R.same_partition(plain, obj)
    labels, prob = btsbot_amd.hdbscan(t, 5, 5, groups=g)
    ref = _ref("objects", 5, 5, True)
    print(f"objects: {int(labels.max()) + 1} clusters with groups, {len(set(obj.tolist()))} objects")
    assert 2 <= int(labels.max()) + 1 <= 12
    assert np.array_equal(labels.cpu().numpy(), ref["labels"])
    assert _close(prob.cpu().numpy(), ref["prob"], 4 * R.band(X.shape[1]))
    index = btsbot_amd.EmbeddingIndex(t, groups=g)
    mst = btsbot_amd.mutual_reachability_mst(index, 5)
    assert torch.equal(index.groups, g)                        # the index's own groups are not touched
    again, _ = btsbot_amd.ClusterTree(mst).labels(5)
    assert torch.equal(again, labels)
    with pytest.raises(ValueError, match="groups= next to an index"):
        btsbot_amd.mutual_reachability_mst(index, 5, groups=g)


# ---- 7. edge cases ------------------------------------------------------------------------------------------------------
def test_non_finite_rows_too_few_rows_and_single_linkage(cuda):
    X, bad = R.blobs_32d_with_bad_rows(), list(R.BAD_ROWS)
    t = torch.from_numpy(X).to(cuda)
    labels, prob, tree = btsbot_amd.hdbscan(t, 10, 5, return_tree=True)
    assert (labels[bad] == -1).all() and (prob[bad] == 0).all() and torch.isnan(tree.mst.core[bad]).all()
    assert len(tree.mst) == len(X) - 4 and not np.isin(tree.mst.edges.cpu().numpy(), bad).any()
    ref = R.hdbscan_ref(R.dist_matrix(X), 10, 5)
    assert np.array_equal(labels.cpu().numpy(), ref["labels"])
    few = torch.from_numpy(X[[3, 100, 0, 1, 2]]).to(cuda)
    with pytest.raises(ValueError, match="finite rows"):
        btsbot_amd.hdbscan(few, 5, 4)
    labels, _ = btsbot_amd.hdbscan(few, 2, 3, allow_single_cluster=True)
    assert labels.tolist() == [-1, -1, 0, 0, 0]
    with pytest.raises(ValueError, match="finite rows"):
        btsbot_amd.mutual_reachability_mst(few[:3], 1)
    # min_samples = 1: plain single linkage
    from scipy.sparse.csgraph import minimum_spanning_tree
    X = _set("32d:2")[0]
    mst = btsbot_amd.mutual_reachability_mst(torch.from_numpy(X).to(cuda), 1)
    assert (mst.core == 0).all()
    want = minimum_spanning_tree(_dist("32d:2")).sum()
    got = float(mst.weights.to(torch.float64).sum())
    assert abs(got - want) <= R.band(32) * want


# ---- 8. run_training ----------------------------------------------------------------------------------------------------
def test_run_training_writes_hdbscan_clusters_only_when_asked(cuda, tmp_path):
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
    runs = (("h0", {"algorithm": "hdbscan", "min_cluster_size": 4, "min_samples": 3, "on": "map", "method": "grid"}),
            ("h1", {"algorithm": "hdbscan", "min_cluster_size": 4, "on": "embedding"}),
            ("h2", {"eps": 0.5, "min_samples": 3, "on": "embedding"}))
    for run, clu in runs:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            run_training(dict(base, embedding_clusters=clu), data_base_dir=str(tmp_path) + "/", run_name=run, device=cuda,
                         precision="f32", models_root=str(tmp_path / "models"), embeddings_root=str(tmp_path / "embeddings"))
        stem = str(tmp_path / "embeddings" / f"um_nn_{run}")
        table = pd.read_csv(stem + "_umap.csv")
        emb = torch.from_numpy(np.load(stem + ".npy")).to(cuda)
        if run == "h0":
            y = torch.from_numpy(table[["umap_emb_1", "umap_emb_2"]].to_numpy().astype(np.float32)).to(cuda)
            prob = np.load(stem + "_cluster_prob.npy")
            assert list(table.columns) == ["umap_emb_1", "umap_emb_2", "cluster"] and table["cluster"].dtype == np.int64
            assert prob.dtype == np.float64 and prob.shape == (64,) and ((prob >= 0) & (prob <= 1)).all()
            assert ((table["cluster"].to_numpy() < 0) == (prob == 0)).all()
            assert not os.path.exists(stem + "_clusters.npy") and y.shape == (64, 2)
        elif run == "h1":
            want_l, want_p = btsbot_amd.hdbscan(emb, 4)
            assert list(table.columns) == ["umap_emb_1", "umap_emb_2"]
            assert np.array_equal(np.load(stem + "_clusters.npy"), want_l.cpu().numpy())
            assert np.array_equal(np.load(stem + "_cluster_prob.npy"), want_p.cpu().numpy())
        else:   # the default algorithm: the files of the DBSCAN run, and no probabilities
            assert list(table.columns) == ["umap_emb_1", "umap_emb_2"]
            assert np.array_equal(np.load(stem + "_clusters.npy"), btsbot_amd.dbscan(emb, 0.5, 3)[0].cpu().numpy())
            assert not os.path.exists(stem + "_cluster_prob.npy")
