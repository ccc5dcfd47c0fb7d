"""GPU tests of the grouped embedding neighbours (run with -m gpu on an MI355X): EmbeddingIndex(groups=...) / query's
exclude_same_group and one_per_group / knn_graph(groups=...) / embedding_layout(groups=...) / btsbot_knn_query_grouped
against the float64 brute force on the host under the contract of tests/knn_group_ref.py, against the ungrouped search
where the two must agree bit for bit, and against themselves (splits, batch cuts, runs, incremental index)."""
import ctypes as C

import numpy as np
import pytest
import torch

import btsbot_amd
from btsbot_amd import _lib
import knn_group_ref as G
import knn_ref as R

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "cosine")


def _gpu(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _np(idx, dist):
    return idx.cpu().numpy(), dist.cpu().numpy()


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _switches(mode):
    exclude, one = G.MODES[mode]
    return dict(exclude_same_group=exclude, one_per_group=one)


def _check_kw(qg, bg, mode):
    exclude, one = G.MODES[mode]
    return dict(query_groups=qg, bank_groups=bg, exclude=exclude, one=one)


# ---- the contract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_contract_in_the_three_modes_on_the_covering_cases(cuda, case, metric):
    k, splits = case[3], case[4]
    for kind in R.KINDS:
        q, b, qg, bg = G.case_inputs(case, kind)
        tq, tb, tqg, tbg = _gpu(cuda, q, b, qg, bg)
        index = btsbot_amd.EmbeddingIndex(tb, metric, groups=tbg)
        for mode in G.MODES:
            idx, dist = _np(*index.query(tq, k, query_groups=tqg, splits=splits, **_switches(mode)))
            worst = G.check_group_neighbors(q, b, idx, dist, k, metric, **_check_kw(qg, bg, mode))
            print(f"{G.case_id(case)} {metric} {kind} {mode}: worst distance error {worst[0]:.3f} of its bound, worst "
                  f"rank excess {worst[1]:.3f} tau")


@pytest.mark.parametrize("d", [5, 33, 528])
def test_exact_answers_on_integer_rows(cuda, d):
    """Clause 4 on rows with period-24 duplicates spread over different groups: the (score, index) ranking decides the
    representative and the order, inside a tile, across tiles and across splits, in both passes."""
    b = R.make_rows("integer", 1000, d, 6)
    q = R.make_rows("integer", 130, d, 5)
    bg = G.make_groups("runs_hi32", 1000, 3)
    qg = bg[np.random.default_rng(1).integers(0, 1000, size=130)]
    tq, tb, tqg, tbg = _gpu(cuda, q, b, qg, bg)
    index = btsbot_amd.EmbeddingIndex(tb, groups=tbg)
    for mode in G.MODES:
        for splits in (1, 2, 7, 0):
            idx, dist = _np(*index.query(tq, 32, query_groups=tqg, splits=splits, **_switches(mode)))
            G.check_group_exact(q, b, idx, dist, 32, **_check_kw(qg, bg, mode))
    idx, dist = _np(*index.query(tb[:130], 15, query_groups=tbg[:130], splits=2, self_offset=0, one_per_group=True))
    G.check_group_exact(b[:130], b, idx, dist, 15, self_offset=0, **_check_kw(bg[:130], bg, "distinct"))


# ---- reductions to the ungrouped answers, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_reductions_to_the_ungrouped_query(cuda, metric):
    q, b = R.make_rows("clustered", 130, 33, 3), R.make_rows("clustered", 4099, 33, 4)
    b[1000:1100] = b[:100]
    tq, tb = _gpu(cuda, q, b)
    n = len(b)
    wide = torch.arange(n, device=cuda) * (1 << 32) - (1 << 40)          # all distinct, equal in their low 32 bits
    plain = btsbot_amd.EmbeddingIndex(tb, metric)
    index = btsbot_amd.EmbeddingIndex(tb, metric, groups=wide)
    for k, splits in ((15, 0), (32, 7), (1, 1)):
        ref = plain.query(tq, k, splits=splits)
        assert _same(index.query(tq, k, one_per_group=True, splits=splits), ref), (k, splits)
        away = torch.arange(130, device=cuda) * (1 << 32) + 5              # query groups disjoint from the bank's
        assert _same(index.query(tq, k, query_groups=away, exclude_same_group=True, splits=splits), ref), (k, splits)
        assert _same(index.query(tq, k, query_groups=away, exclude_same_group=True, one_per_group=True, splits=splits), ref)
        assert _same(index.query(tq, k, query_groups=away, splits=splits), ref)      # groups, no switch
    rows = torch.arange(n, device=cuda)
    index = btsbot_amd.EmbeddingIndex(tb, metric, groups=rows)
    ref = plain.query(tb[:130], 15, self_offset=0)
    assert _same(index.query(tb[:130], 15, query_groups=rows[:130], exclude_same_group=True), ref)
    assert _same(btsbot_amd.embedding_neighbors(tb[:130], tb, 15, metric, bank_groups=rows, query_groups=rows[:130],
                                                exclude_same_group=True), ref)


def test_the_grouped_entry_point_without_flags_is_the_ungrouped_one(cuda):
    q, b = R.make_rows("normal", 65, 33, 1), R.make_rows("normal", 1000, 33, 2)
    tq, tb = _gpu(cuda, q, b)
    index = btsbot_amd.EmbeddingIndex(tb)
    ref = index.query(tq, 15, splits=7)
    L = _lib.lib()
    need = int(L.btsbot_knn_workspace(65, 1000, 33, 15, 7))
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    idx = torch.empty((65, 15), dtype=torch.int64, device=cuda)
    dist = torch.empty((65, 15), dtype=torch.float32, device=cuda)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    rc = L.btsbot_knn_query_grouped(p(tq), 65, p(index._bank), p(index._packed), 1000, 33, 15, 0, -1, 7, p(idx), p(dist),
                                    p(ws), need, stream, None, None, 0)
    assert rc == _lib.OK and _same((idx, dist), ref)
    # k = 64 stays open to the exclusion; only one_per_group holds k <= 32
    g = torch.arange(1000, device=cuda) % 40
    gi = btsbot_amd.EmbeddingIndex(tb, groups=g)
    i64, d64 = _np(*gi.query(tq, 64, query_groups=g[:65], exclude_same_group=True, splits=2))
    G.check_group_neighbors(q, b, i64, d64, 64, **_check_kw(g[:65].cpu().numpy(), g.cpu().numpy(), "exclude"))
    with pytest.raises(ValueError, match="k <= 32"):
        gi.query(tq, 33, one_per_group=True)
    rc = L.btsbot_knn_query_grouped(p(tq), 65, p(index._bank), p(index._packed), 1000, 33, 33, 0, -1, 7, p(idx), p(dist),
                                    p(ws), 1 << 40, stream, None, p(g), 2)
    assert rc == _lib.ERR_INVALID_ARG


# ---- determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(G.MODES))
def test_answers_do_not_depend_on_splits_batching_the_run_or_how_the_index_grew(cuda, mode):
    q, b = R.make_rows("clustered", 130, 33, 3), R.make_rows("clustered", 4099, 33, 4)
    b[1000:1100] = b[:100]                                   # exact duplicates in other tiles, and in other groups
    bg = G.make_groups("runs_hi32", 4099, 1)
    qg = bg[np.arange(130) * 31]
    tq, tb, tqg, tbg = _gpu(cuda, q, b, qg, bg)
    sw = _switches(mode)
    index = btsbot_amd.EmbeddingIndex(tb, groups=tbg)
    ref = index.query(tq, 15, query_groups=tqg, splits=1, **sw)
    G.check_group_neighbors(q, b, *_np(*ref), 15, **_check_kw(qg, bg, mode))
    for splits in (2, 7, 0, 1):
        assert _same(index.query(tq, 15, query_groups=tqg, splits=splits, **sw), ref), splits
    i1, d1 = index.query(tq[:63], 15, query_groups=tqg[:63], splits=2, **sw)
    i2, d2 = index.query(tq[63:], 15, query_groups=tqg[63:], splits=7, **sw)
    assert _same((torch.cat([i1, i2]), torch.cat([d1, d2])), ref)
    parts = btsbot_amd.EmbeddingIndex(tb[:127], groups=tbg[:127])
    assert parts.add(tb[127:130], groups=tbg[127:130]) is parts
    parts.add(tb[130:], groups=tbg[130:])
    assert len(parts) == 4099 and torch.equal(parts.groups, index.groups) and torch.equal(parts.groups, tbg)
    assert _same(parts.query(tq, 15, query_groups=tqg, splits=7, **sw), ref)
    with pytest.raises(ValueError, match="if and only if"):
        parts.add(tb[:3])
    with pytest.raises(ValueError, match="if and only if"):
        btsbot_amd.EmbeddingIndex(tb).add(tb[:3], groups=tbg[:3])
    with pytest.raises(ValueError, match="one group per row"):
        parts.add(tb[:3], groups=tbg[:4])
    with pytest.raises(ValueError, match="int64"):
        parts.query(tq, 15, query_groups=tqg.int(), **sw)
    with pytest.raises(ValueError, match="is on"):
        parts.query(tq, 15, query_groups=tqg.cpu(), **sw)
    assert len(parts) == 4099 and btsbot_amd.EmbeddingIndex(tb).groups is None


# ---- edges -----------------------------------------------------------------------------------------------------------
def test_edges(cuda):
    q, b = R.make_rows("normal", 65, 32, 1), R.make_rows("normal", 300, 32, 2)
    bg = np.arange(300, dtype=np.int64) // 3 - 50              # objects of three rows
    qg = bg[np.arange(65) * 4]
    b[[3, 4, 5], [0, 5, 31]] = [np.nan, np.inf, -np.inf]       # a group whose rows are all non-finite
    q[[7, 64], [0, 31]] = [np.nan, np.inf]
    tq, tb, tqg, tbg = _gpu(cuda, q, b, qg, bg)
    # a group whose BEST row is non-finite: row 30 would be query 12's nearest of its group
    b[30] = q[12]
    b[30, 7] = np.inf
    tb = _gpu(cuda, b)[0]
    for metric in METRICS:
        index = btsbot_amd.EmbeddingIndex(tb, metric, groups=tbg)
        for mode in G.MODES:
            for splits in (1, 3):
                idx, dist = _np(*index.query(tq, 15, query_groups=tqg, splits=splits, **_switches(mode)))
                G.check_group_neighbors(q, b, idx, dist, 15, metric, **_check_kw(qg, bg, mode))
                assert (idx[[7, 64]] == -1).all() and np.isnan(dist[[7, 64]]).all()
                assert not np.isin(idx, [3, 4, 5, 30]).any()
    # fewer eligible groups than k
    few = tbg % 5
    index = btsbot_amd.EmbeddingIndex(tb, groups=few)
    idx, dist = _np(*index.query(tq, 15, query_groups=few[:65], one_per_group=True))
    G.check_group_neighbors(q, b, idx, dist, 15, **_check_kw(few[:65].cpu().numpy(), few.cpu().numpy(), "distinct"))
    assert (idx[0, :5] >= 0).all() and (idx[0, 5:] == -1).all() and np.isposinf(dist[0, 5:]).all()
    idx, dist = _np(*index.query(tq, 15, query_groups=few[:65], one_per_group=True, exclude_same_group=True, splits=3))
    assert (idx[0, :4] >= 0).all() and (idx[0, 4:] == -1).all()
    # a bank that is entirely the query's group
    one = torch.full((300,), -9, dtype=torch.int64, device=cuda)
    index = btsbot_amd.EmbeddingIndex(tb, groups=one)
    idx, dist = _np(*index.query(tq[:5], 4, query_groups=one[:5], exclude_same_group=True))
    assert (idx == -1).all() and np.isposinf(dist).all()
    idx, dist = _np(*index.query(tq[:5], 4, one_per_group=True))
    assert (idx[:, 0] >= 0).all() and (idx[:, 1:] == -1).all()
    # Q = 0 and N = 0
    idx, dist = index.query(tq[:0], 3, query_groups=one[:0], exclude_same_group=True, one_per_group=True)
    assert idx.shape == (0, 3) and dist.shape == (0, 3) and idx.dtype == torch.int64 and dist.dtype == torch.float32
    empty = btsbot_amd.EmbeddingIndex(tb[:0], groups=one[:0])
    idx, dist = _np(*empty.query(tq[:5], 3, query_groups=one[:5], exclude_same_group=True, one_per_group=True))
    assert (idx == -1).all() and np.isposinf(dist).all() and len(empty.groups) == 0
    # the errors come before any launch
    with pytest.raises(ValueError, match="needs query_groups"):
        index.query(tq, 3, exclude_same_group=True)
    with pytest.raises(ValueError, match="built with groups"):
        btsbot_amd.EmbeddingIndex(tb).query(tq, 3, one_per_group=True)
    with pytest.raises(ValueError, match="int64"):
        btsbot_amd.EmbeddingIndex(tb, groups=one.int())
    with pytest.raises(ValueError, match="one group per row"):
        btsbot_amd.EmbeddingIndex(tb, groups=one[:299])
    with pytest.raises(ValueError, match="is on"):
        btsbot_amd.EmbeddingIndex(tb, groups=one.cpu())


# ---- the graph and the map -------------------------------------------------------------------------------------------
def test_knn_graph_with_groups_and_the_map_of_it(cuda):
    emb = R.make_rows("normal", 300, 33, 9)
    obj = G.make_groups("runs", 300, 2)
    t, tobj = _gpu(cuda, emb, obj)
    rows = np.arange(300)
    for mode in G.MODES:
        exclude, one = G.MODES[mode]
        idx, dist = _np(*btsbot_amd.knn_graph(t, 15, groups=tobj, group_mode=mode))
        assert (idx[:, 0] == rows).all() and (dist[:, 0] == 0).all(), mode
        G.check_group_neighbors(emb, emb, idx[:, 1:], dist[:, 1:], 14, self_offset=0, **_check_kw(obj, obj, mode))
        if exclude:
            assert (obj[idx[:, 1:]] != obj[:, None]).all()
        others, od = _np(*btsbot_amd.knn_graph(t, 14, include_self=False, groups=tobj, group_mode=mode))
        assert (others == idx[:, 1:]).all() and (od.view(np.int32) == dist[:, 1:].view(np.int32)).all()
    assert _same(btsbot_amd.knn_graph(t, 15, groups=None, group_mode="distinct"), btsbot_amd.knn_graph(t, 15))
    graph = btsbot_amd.knn_graph(t, 15, groups=tobj)           # the default mode is "exclude"
    assert _same(graph, btsbot_amd.knn_graph(t, 15, groups=tobj, group_mode="exclude"))
    y = btsbot_amd.embedding_layout(t, 15, n_epochs=30, seed=3, groups=tobj)
    y_ref = btsbot_amd.embedding_layout(t, 15, n_epochs=30, seed=3, knn=graph)
    assert torch.equal(y.view(torch.int32), y_ref.view(torch.int32)) and bool(torch.isfinite(y).all())
    assert not torch.equal(y, btsbot_amd.embedding_layout(t, 15, n_epochs=30, seed=3))
    with pytest.raises(ValueError, match="not beside knn"):
        btsbot_amd.embedding_layout(t, 15, knn=graph, groups=tobj)


# ---- the domain: alerts of one object are near-copies of each other ------------------------------------------------------
def test_neighbours_of_an_alert_are_its_own_object_until_it_is_excluded(cuda):
    """2560 alerts: 512 objects of 5 alerts (sigma 1e-3) on the 32-D ten-cluster set.  The float64 brute force gives:
    ungrouped, the 5 nearest rows of an alert are its own object (the alert and its four other epochs) in 100 % of the
    slots; with the own object excluded 0 %, and every neighbour carries the alert's label (purity 1.000).  Both figures
    are asserted on the brute force first, then on the device."""
    rows, obj, lab = G.object_set()
    x = rows.astype(np.float64)
    d2 = ((x * x).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * x @ x.T)
    nn = np.argsort(d2, axis=1, kind="stable")[:, :5]
    assert (obj[nn] == obj[:, None]).mean() >= 0.99
    d2x = np.where(obj[None, :] == obj[:, None], np.inf, d2)
    nnx = np.argsort(d2x, axis=1, kind="stable")[:, :5]
    assert (obj[nnx] != obj[:, None]).all() and (lab[nnx] == lab[:, None]).mean() == 1.0
    t, tobj, tlab = _gpu(cuda, rows, obj, lab)
    idx, _ = btsbot_amd.embedding_neighbors(t, t, 5)
    assert (tobj[idx] == tobj[:, None]).float().mean().item() >= 0.99
    idx, dist = btsbot_amd.knn_graph(t, 5, include_self=False, groups=tobj, group_mode="exclude")
    assert not bool((tobj[idx] == tobj[:, None]).any())
    assert (tlab[idx] == tlab[:, None]).float().mean().item() == 1.0
    G.check_group_neighbors(rows, rows, *_np(idx, dist), 5, self_offset=0, **_check_kw(obj, obj, "exclude"))
    # the leave-one-object-out kNN score: one label against the rest
    vote = btsbot_amd.neighbor_vote(idx, dist, (tlab == 3).long(), "distance")
    assert torch.equal(vote, (tlab == 3).float())
    # the nearest SOURCES: five distinct objects, none of them the alert's own
    idx, _ = btsbot_amd.knn_graph(t, 5, include_self=False, groups=tobj, group_mode="exclude+distinct")
    near = tobj[idx].cpu().numpy()
    assert all(len(set(r.tolist())) == 5 for r in near) and (near != obj[:, None]).all()


def test_run_training_writes_the_grouped_graph_on_request(cuda, tmp_path):
    """The dict form of config['embedding_neighbors'] and 'group_by' of config['embedding_layout'] (the plain int is the
    existing test's)."""
    import warnings
    import pandas as pd
    from btsbot_amd import architectures
    from btsbot_amd.alert_utils import object_keys
    from btsbot_amd.to_HF import cpu_state_dict
    from btsbot_amd.train import write_embeddings
    from helpers import CONFIGS, METADATA_COLS
    from btsbot_amd.synthetic import synthetic_batch
    _, meta, _ = synthetic_batch(64, seed=21)
    d = tmp_path / "data"
    d.mkdir()
    names = [f"ZTF21aaaaa{'abcdefghijklmnop'[i // 4]}{'ab'[i % 2]}" for i in range(64)]
    df = pd.DataFrame(meta.numpy(), columns=METADATA_COLS)
    df["label"] = 0
    df["candid"] = np.arange(64) + 1_000_000
    df["objectId"] = names
    df.to_csv(d / "test_cand_v11_N100.csv", index=False)
    cfg = dict(CONFIGS["um_nn"][1], model_name="um_nn", train_data_version="v11", random_seed=2,
               embedding_neighbors={"k": 5, "group_by": "objectId", "mode": "exclude"},
               embedding_layout={"n_neighbors": 5, "n_epochs": 20, "group_by": "objectId"})
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = architectures.um_nn(cfg, precision="f32")
    mdir = tmp_path / "model"
    mdir.mkdir()
    torch.save(cpu_state_dict(model), mdir / "best_model.pth")
    stem = str(tmp_path / "emb" / "run")
    write_embeddings(model, cfg, str(tmp_path) + "/", str(mdir), stem, device=cuda)
    emb = torch.from_numpy(np.load(stem + ".npy")).to(cuda)
    z = np.load(stem + "_knn.npz")
    assert sorted(z.files) == ["candid", "distances", "groups", "indices"]
    ids = object_keys(names)
    assert np.array_equal(z["groups"], ids) and z["groups"].dtype == np.int64
    idx, dist = _np(*btsbot_amd.knn_graph(emb, 5, groups=torch.from_numpy(ids).to(cuda), group_mode="exclude"))
    assert np.array_equal(z["indices"], idx) and np.array_equal(z["distances"].view(np.int32), dist.view(np.int32))
    assert (ids[idx[:, 1:]] != ids[:, None]).all()
    y = btsbot_amd.embedding_layout(emb, 5, n_epochs=20, seed=2, groups=torch.from_numpy(ids).to(cuda)).cpu().numpy()
    got = pd.read_csv(stem + "_umap.csv")
    assert np.allclose(got[["umap_emb_1", "umap_emb_2"]].to_numpy(), y, rtol=1e-6)
    cfg["embedding_neighbors"]["group_by"] = "object"
    with pytest.raises(KeyError, match="'object'"):
        write_embeddings(model, cfg, str(tmp_path) + "/", str(mdir), stem, device=cuda)
