"""GPU tests of the embedding neighbours (run with -m gpu on an MI355X): embedding_neighbors / EmbeddingIndex / knn_graph /
btsbot_knn_query against the float64 brute force on the host, under the contract of tests/knn_ref.py (validity, returned
distance, rank within tau, exact answers on integer rows), and against themselves bit for bit (splits, batch cuts, runs,
incremental index)."""
import os
import warnings

import numpy as np
import pytest
import torch

import btsbot_amd
import knn_ref as R

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "cosine")


def _gpu(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _np(idx, dist):
    return idx.cpu().numpy(), dist.cpu().numpy()


def _report(tag, worst):
    print(f"{tag}: worst distance error {worst[0]:.3f} of its bound, worst rank excess {worst[1]:.3f} tau")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "Q{}-N{}-D{}-k{}-s{}".format(*c))
def test_contract_on_the_covering_cases(cuda, case, metric):
    k, splits = case[3], case[4]
    for kind in R.KINDS:
        q, b = R.case_inputs(case, kind)
        tq, tb = _gpu(cuda, q, b)
        idx, dist = _np(*btsbot_amd.embedding_neighbors(tq, tb, k, metric, splits=splits))
        _report(f"{case} {metric} {kind}", R.check_neighbors(q, b, idx, dist, k, metric))


@pytest.mark.parametrize("metric", METRICS)
def test_contract_on_the_larger_case(cuda, metric):
    """More than one workgroup per XCD and the library's own choice of splits."""
    n_q, n, d, k, splits = R.LARGE
    q, b = R.case_inputs(R.LARGE, "normal")
    tq, tb = _gpu(cuda, q, b)
    idx, dist = _np(*btsbot_amd.embedding_neighbors(tq, tb, k, metric, splits=splits))
    _report(f"{R.LARGE} {metric}", R.check_neighbors(q, b, idx, dist, k, metric))


def test_contract_on_rows_near_1e6(cuda):
    q, b = R.make_rows("normal", 65, 33, 1) * np.float32(3e5), R.make_rows("normal", 1000, 33, 2) * np.float32(3e5)
    tq, tb = _gpu(cuda, q, b)
    for metric in METRICS:
        idx, dist = _np(*btsbot_amd.embedding_neighbors(tq, tb, 15, metric, splits=2))
        _report(f"1e6 {metric}", R.check_neighbors(q, b, idx, dist, 15, metric))


@pytest.mark.parametrize("d", [5, 33, 528])
def test_exact_answers_on_integer_rows(cuda, d):
    """Clause 4: ties go to the lower bank index inside a tile, across tiles and across splits, in both passes."""
    q, b = R.make_rows("integer", 130, d, 5), R.make_rows("integer", 1000, d, 6)
    tq, tb = _gpu(cuda, q, b)
    for splits in (1, 2, 7, 0):
        idx, dist = _np(*btsbot_amd.embedding_neighbors(tq, tb, 64, splits=splits))
        R.check_exact(q, b, idx, dist, 64)
    idx, dist = _np(*btsbot_amd.EmbeddingIndex(tb).query(tb[:130], 15, splits=2, self_offset=0))
    R.check_exact(b[:130], b, idx, dist, 15, self_offset=0)


@pytest.mark.parametrize("metric", METRICS)
def test_answers_do_not_depend_on_splits_batching_or_the_run(cuda, metric):
    q, b = R.make_rows("clustered", 130, 33, 3), R.make_rows("clustered", 4099, 33, 4)
    b[1000:1100] = b[:100]                                   # exact duplicates in other tiles
    tq, tb = _gpu(cuda, q, b)
    index = btsbot_amd.EmbeddingIndex(tb, metric)
    ref_i, ref_d = index.query(tq, 15, splits=1)
    R.check_neighbors(q, b, *_np(ref_i, ref_d), 15, metric)
    for splits in (2, 7, 0, 1):
        i, d = index.query(tq, 15, splits=splits)
        assert torch.equal(i, ref_i) and torch.equal(d.view(torch.int32), ref_d.view(torch.int32)), splits
    i1, d1 = index.query(tq[:63], 15, splits=2)
    i2, d2 = index.query(tq[63:], 15, splits=7)
    assert torch.equal(torch.cat([i1, i2]), ref_i)
    assert torch.equal(torch.cat([d1, d2]).view(torch.int32), ref_d.view(torch.int32))
    i, d = btsbot_amd.embedding_neighbors(tq, tb, 15, metric)
    assert torch.equal(i, ref_i) and torch.equal(d.view(torch.int32), ref_d.view(torch.int32))


@pytest.mark.parametrize("metric", METRICS)
def test_index_built_by_three_adds_equals_one_built_at_once(cuda, metric):
    q, b = R.make_rows("scaled", 65, 31, 7), R.make_rows("scaled", 1000, 31, 8)
    tq, tb = _gpu(cuda, q, b)
    whole = btsbot_amd.EmbeddingIndex(tb, metric)
    parts = btsbot_amd.EmbeddingIndex(tb[:127], metric)
    assert parts.add(tb[127:130]) is parts
    parts.add(tb[130:])
    assert len(parts) == len(whole) == 1000 and torch.equal(parts.bank, whole.bank)
    rec = len(whole._packed) // 1000
    assert torch.equal(parts._packed[:1000 * rec], whole._packed)
    for splits in (1, 7):
        (i1, d1), (i2, d2) = whole.query(tq, 15, splits=splits), parts.query(tq, 15, splits=splits)
        assert torch.equal(i1, i2) and torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    R.check_neighbors(q, b, *_np(i2, d2), 15, metric)


@pytest.mark.parametrize("metric", METRICS)
def test_knn_graph_with_and_without_self(cuda, metric):
    emb = R.make_rows("normal", 300, 33, 9)
    emb[200:220] = emb[:20]                                  # duplicates: legitimate neighbours at distance 0
    (t,) = _gpu(cuda, emb)
    idx, dist = _np(*btsbot_amd.knn_graph(t, 15, include_self=False, metric=metric))
    R.check_neighbors(emb, emb, idx, dist, 15, metric, self_offset=0)
    assert (idx[:20, 0] == np.arange(200, 220)).all() and (idx[200:220, 0] == np.arange(20)).all()
    if metric == "euclidean":
        assert (dist[:20, 0] == 0).all() and (dist[200:220, 0] == 0).all()
    ids, ds = _np(*btsbot_amd.knn_graph(t, 15, metric=metric))
    assert (ids[:, 0] == np.arange(300)).all() and (ds[:, 0] == 0).all()
    assert (ids[:, 1:] == idx[:, :14]).all() and (ds[:, 1:].view(np.int32) == dist[:, :14].view(np.int32)).all()
    ids, ds = _np(*btsbot_amd.knn_graph(t, 1))
    assert (ids[:, 0] == np.arange(300)).all() and (ds == 0).all()


def test_non_finite_rows_and_zero_rows(cuda):
    q, b = R.make_rows("normal", 65, 32, 1), R.make_rows("normal", 300, 32, 2)
    b[[3, 128, 299], [0, 5, 31]] = [np.nan, np.inf, -np.inf]
    b[50] = 0
    q[[7, 64], [0, 31]] = [np.nan, np.inf]
    q[9] = 0
    tq, tb = _gpu(cuda, q, b)
    for metric in METRICS:
        for splits in (1, 7):
            idx, dist = _np(*btsbot_amd.embedding_neighbors(tq, tb, 15, metric, splits=splits))
            R.check_neighbors(q, b, idx, dist, 15, metric)
            assert (idx[[7, 64]] == -1).all() and np.isnan(dist[[7, 64]]).all()
            assert not np.isin(idx, [3, 128, 299]).any()
    idx, dist = _np(*btsbot_amd.embedding_neighbors(tq, tb, 15, "cosine"))
    assert (dist[9] == 1).all() and (idx[9] == np.arange(15) + (np.arange(15) >= 3)).all()   # cos = 0: index order
    # nothing eligible at all
    bad = torch.full((5, 32), float("nan"), device=cuda)
    idx, dist = _np(*btsbot_amd.embedding_neighbors(tq[:3], bad, 4))
    assert (idx == -1).all() and np.isposinf(dist).all()


def test_no_queries_and_an_empty_bank(cuda):
    (tb,) = _gpu(cuda, R.make_rows("normal", 10, 8, 1))
    idx, dist = btsbot_amd.embedding_neighbors(tb[:0], tb, 3)
    assert idx.shape == (0, 3) and dist.shape == (0, 3) and idx.dtype == torch.int64 and dist.dtype == torch.float32
    idx, dist = _np(*btsbot_amd.embedding_neighbors(tb, tb[:0], 3))
    assert (idx == -1).all() and np.isposinf(dist).all()
    idx, dist = _np(*btsbot_amd.embedding_neighbors(tb.double(), tb.half(), 3))        # other float dtypes are converted
    R.check_neighbors(tb.cpu().numpy(), tb.half().float().cpu().numpy(), idx, dist, 3)


def test_run_training_writes_the_knn_graph_on_request(cuda, tmp_path):
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
        if split == "test":
            df["candid"] = np.arange(sl.start, sl.stop) + 1_000_000
        df.to_csv(d / f"{split}_cand_v11_N100.csv", index=False)
    cfg = dict(CONFIGS["um_nn"][1], model_name="um_nn", train_data_version="v11", epochs=2, batch_size=64,
               learning_rate="3e-3", warmup_epochs=1, beta_1=0.9, beta_2=0.999, patience=3, random_seed=2,
               generate_embeddings=True, embedding_neighbors=5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hist, _ = run_training(cfg, data_base_dir=str(tmp_path) + "/", run_name="k0", device=cuda, precision="f32",
                               models_root=str(tmp_path / "models"), embeddings_root=str(tmp_path / "embeddings"))
    stem = tmp_path / "embeddings" / "um_nn_k0"
    assert hist["embeddings_file"] == str(stem) + ".npy"
    emb = np.load(str(stem) + ".npy")
    z = np.load(str(stem) + "_knn.npz")
    assert sorted(z.files) == ["candid", "distances", "indices"]
    idx, dist = _np(*btsbot_amd.knn_graph(torch.from_numpy(emb).to(cuda), 5, include_self=True))
    assert z["indices"].dtype == np.int64 and z["distances"].dtype == np.float32
    assert np.array_equal(z["indices"], idx) and np.array_equal(z["distances"].view(np.int32), dist.view(np.int32))
    assert list(z["candid"]) == list(np.arange(384, 448) + 1_000_000)
    assert (idx[:, 0] == np.arange(64)).all()
    R.check_neighbors(emb, emb, idx[:, 1:], dist[:, 1:], 4, self_offset=0)
    assert not os.path.exists(str(stem) + "_knn.npy")
