"""CPU-side checks of the embedding neighbours (btsbot_amd.neighbors, btsbot_knn_*): the contract checker itself -- a
numpy emulation of the two-pass scheme stays inside its bounds on every input set the GPU test uses, and seeded faults
do not --, the exported symbols, the argument limits (no GPU call is made) and the opt-in key of run_training."""
import ctypes as C

import numpy as np
import pytest
import torch

import btsbot_amd
from btsbot_amd import _lib
import knn_ref as R

METRICS = ("euclidean", "cosine")


# ---- 1. a correct implementation stays inside the bounds -----------------------------------------------------------
@pytest.mark.parametrize("form", ["split", "fp32"])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "Q{}-N{}-D{}-k{}-s{}".format(*c))
def test_emulation_meets_the_contract(case, metric, form):
    k, splits = case[3], case[4]
    for kind in R.KINDS:
        q, b = R.case_inputs(case, kind)
        idx, dist = R.emulate(q, b, k, metric, splits, form=form)
        R.check_neighbors(q, b, idx, dist, k, metric)


@pytest.mark.parametrize("metric", METRICS)
def test_emulation_meets_the_contract_large_case(metric):
    q, b = R.case_inputs(R.LARGE, "normal")
    idx, dist = R.emulate(q, b, R.LARGE[3], metric, R.LARGE[4])
    R.check_neighbors(q, b, idx, dist, R.LARGE[3], metric)


@pytest.mark.parametrize("d", [5, 33, 528])
@pytest.mark.parametrize("splits", [1, 2, 7])
def test_emulation_is_exact_on_integer_rows(d, splits):
    q, b = R.make_rows("integer", 130, d, 5), R.make_rows("integer", 1000, d, 6)
    idx, dist = R.emulate(q, b, 64, "euclidean", splits)
    R.check_exact(q, b, idx, dist, 64)
    idx, dist = R.emulate(b[:130], b, 15, "euclidean", splits, self_offset=0)
    R.check_exact(b[:130], b, idx, dist, 15, self_offset=0)


def test_emulation_handles_non_finite_rows_and_scale():
    q, b = R.make_rows("normal", 20, 33, 1), R.make_rows("normal", 300, 33, 2)
    q, b = q * np.float32(1e6), b * np.float32(1e6)
    b[[3, 128, 299], [0, 5, 32]] = [np.nan, np.inf, -np.inf]
    q[7, 0] = np.nan
    for metric in METRICS:
        idx, dist = R.emulate(q, b, 15, metric, 2)
        R.check_neighbors(q, b, idx, dist, 15, metric)
        assert (idx[7] == -1).all() and np.isnan(dist[7]).all()


# ---- 2. seeded faults are rejected -----------------------------------------------------------------------------------
def _good():
    q, b = R.make_rows("normal", 40, 33, 11), R.make_rows("normal", 700, 33, 12)
    return q, b, 15


def test_checker_rejects_a_dropped_bank_tile():
    q, b, k = _good()
    idx, dist = R.emulate(q, b, k, splits=2, drop_tile=2)
    with pytest.raises(AssertionError, match="rank"):
        R.check_neighbors(q, b, idx, dist, k)


def test_checker_rejects_a_dropped_split():
    q, b, k = _good()
    idx, dist = R.emulate(q, b, k, splits=2, drop_split=1)
    with pytest.raises(AssertionError, match="rank"):
        R.check_neighbors(q, b, idx, dist, k)


def test_checker_rejects_tied_rows_in_the_wrong_order():
    q, b = R.make_rows("integer", 30, 5, 5), R.make_rows("integer", 400, 5, 6)
    idx, dist = R.emulate(q, b, 15, splits=2)
    R.check_exact(q, b, idx, dist, 15)
    R.check_neighbors(q, b, idx, dist, 15)
    tied = np.argwhere(dist[:, 1:] == dist[:, :-1])
    assert len(tied)
    i, j = tied[0]
    bad = idx.copy()
    bad[i, [j, j + 1]] = bad[i, [j + 1, j]]
    with pytest.raises(AssertionError, match="sorted"):
        R.check_neighbors(q, b, bad, dist, 15)
    with pytest.raises(AssertionError, match="exact"):
        R.check_exact(q, b, bad, dist, 15)


def test_checker_rejects_indices_off_by_one():
    q, b, k = _good()
    idx, dist = R.emulate(q, b, k)
    with pytest.raises(AssertionError):
        R.check_neighbors(q, b, np.minimum(idx + 1, len(b) - 1), dist, k)
    with pytest.raises(AssertionError):
        R.check_neighbors(q, b, idx - 1, dist, k)


def test_checker_rejects_unrooted_distances():
    q, b, k = _good()
    idx, dist = R.emulate(q, b, k)
    with pytest.raises(AssertionError, match="distance"):
        R.check_neighbors(q, b, idx, (dist * dist).astype(np.float32), k)


def test_checker_rejects_self_not_excluded():
    q, b, k = _good()
    idx, dist = R.emulate(b[:40], b, k)                       # no exclusion: every row finds itself first
    with pytest.raises(AssertionError, match="ineligible"):
        R.check_neighbors(b[:40], b, idx, dist, k, self_offset=0)
    idx, dist = R.emulate(b[:40], b, k, self_offset=0)
    R.check_neighbors(b[:40], b, idx, dist, k, self_offset=0)


def test_checker_rejects_norms_of_a_stale_bank():
    q, b, k = _good()
    stale = R.make_rows("normal", 700, 33, 13) * np.float32(1.5)
    idx, dist = R.emulate(q, b, k, stale_bank=stale)
    with pytest.raises(AssertionError, match="rank"):
        R.check_neighbors(q, b, idx, dist, k)


def test_checker_rejects_a_short_or_padded_answer():
    q, b, k = _good()
    idx, dist = R.emulate(q, b[:7], k)
    R.check_neighbors(q, b[:7], idx, dist, k)                 # k > N: the tail is -1 / +inf
    assert (idx[:, 7:] == -1).all() and np.isposinf(dist[:, 7:]).all()
    bad = idx.copy()
    bad[:, 7] = 0
    with pytest.raises(AssertionError, match="tail"):
        R.check_neighbors(q, b[:7], bad, dist, k)


# ---- 3. / 4. the library: symbols and limits, no GPU call ---------------------------------------------------------------
KNN_SYMBOLS = ("btsbot_knn_bank_bytes", "btsbot_knn_pack_bank", "btsbot_knn_splits", "btsbot_knn_workspace",
               "btsbot_knn_query")


def test_library_exports_the_knn_symbols():
    L = C.CDLL(_lib.LIB_PATH)
    for s in KNN_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(L, s), s
    assert _lib.lib().btsbot_abi_version() == 1
    for name in ("neighbors", "EmbeddingIndex", "embedding_neighbors", "knn_graph"):
        assert name in btsbot_amd.__all__ and hasattr(btsbot_amd, name)


def test_sizes_follow_the_record_layout():
    L = _lib.lib()
    assert L.btsbot_knn_bank_bytes(1, 1) == 16 + 4 * 32
    assert L.btsbot_knn_bank_bytes(1000, 528) == 1000 * (16 + 4 * 544)
    assert L.btsbot_knn_bank_bytes(0, 5) == 0
    assert L.btsbot_knn_splits(8192, 1_000_000, 528, 15) == 8
    assert L.btsbot_knn_splits(1, 100, 5, 1) == 1             # one bank tile: nothing to split
    assert L.btsbot_knn_splits(1, 1_000_000, 528, 15) == 32
    assert L.btsbot_knn_workspace(0, 100, 5, 3, 0) == 0
    w1, w7 = L.btsbot_knn_workspace(10, 5000, 5, 3, 1), L.btsbot_knn_workspace(10, 5000, 5, 3, 7)
    assert w7 - w1 == 10 * 6 * 3 * 8


BAD_SHAPES = [  # (n_query, n_bank, dim, k)
    (4, 10, 0, 1), (4, 10, 1025, 1), (4, 10, -3, 1), (4, 10, 8, 0), (4, 10, 8, 65), (4, 1 << 31, 8, 1),
    (4, -1, 8, 1), (-1, 10, 8, 1),
]


@pytest.mark.parametrize("shape", BAD_SHAPES)
def test_limits_come_back_as_invalid_arg(shape):
    L = _lib.lib()
    nq, nb, dim, k = shape
    junk = C.c_void_p(256)     # never dereferenced: the shape is refused before any HIP call
    assert L.btsbot_knn_splits(nq, nb, dim, k) == _lib.ERR_INVALID_ARG
    assert b"btsbot_knn_splits" in L.btsbot_last_error()
    assert L.btsbot_knn_workspace(nq, nb, dim, k, 0) == _lib.ERR_INVALID_ARG
    assert L.btsbot_knn_query(junk, nq, junk, junk, nb, dim, k, 0, -1, 0, junk, junk, junk, 1 << 40,
                              None) == _lib.ERR_INVALID_ARG
    assert b"btsbot_knn_query" in L.btsbot_last_error()
    if nq >= 0 and k == 1:
        assert L.btsbot_knn_bank_bytes(nb, dim) == _lib.ERR_INVALID_ARG
        assert L.btsbot_knn_pack_bank(junk, 0, 1, dim, 0, junk, nb, None) == _lib.ERR_INVALID_ARG
        assert b"btsbot_knn_pack_bank" in L.btsbot_last_error()


def test_other_argument_errors_of_the_c_entry_points():
    L = _lib.lib()
    junk = C.c_void_p(256)
    bad = _lib.ERR_INVALID_ARG
    assert L.btsbot_knn_query(junk, 4, junk, junk, 10, 8, 3, 2, -1, 0, junk, junk, junk, 1 << 40, None) == bad   # metric
    assert b"metric" in L.btsbot_last_error()
    for splits in (-1, 33):
        assert L.btsbot_knn_query(junk, 4, junk, junk, 10, 8, 3, 0, -1, splits, junk, junk, junk, 1 << 40, None) == bad
        assert b"splits" in L.btsbot_last_error()
        assert L.btsbot_knn_workspace(4, 10, 8, 3, splits) == bad
    need = L.btsbot_knn_workspace(4, 10, 8, 3, 1)
    assert L.btsbot_knn_query(junk, 4, junk, junk, 10, 8, 3, 0, -1, 1, junk, junk, junk, need - 1, None) == bad
    assert b"workspace" in L.btsbot_last_error()
    assert L.btsbot_knn_query(None, 4, junk, junk, 10, 8, 3, 0, -1, 1, junk, junk, junk, need, None) == bad
    assert b"NULL" in L.btsbot_last_error()
    assert L.btsbot_knn_query(junk, 4, junk, C.c_void_p(260), 10, 8, 3, 0, -1, 1, junk, junk, junk, need, None) == bad
    assert L.btsbot_knn_pack_bank(junk, 0, 1, 8, 7, junk, 10, None) == bad
    assert L.btsbot_knn_pack_bank(junk, 8, 3, 8, 0, junk, 10, None) == bad      # rows 8..10 of a bank of 10
    assert b"do not fit" in L.btsbot_last_error()
    assert L.btsbot_knn_pack_bank(None, 0, 1, 8, 0, junk, 10, None) == bad
    # nothing to do: no launch, no error
    assert L.btsbot_knn_query(None, 0, None, None, 10, 8, 3, 0, -1, 0, None, None, None, 0, None) == _lib.OK
    assert L.btsbot_knn_pack_bank(None, 0, 0, 8, 0, None, 10, None) == _lib.OK


def test_python_wrappers_refuse_cpu_tensors_and_bad_arguments():
    q, b = torch.zeros(3, 8), torch.zeros(10, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.embedding_neighbors(q, b, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.EmbeddingIndex(b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.knn_graph(b, 2)
    for k in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError, match="k must be"):
            btsbot_amd.embedding_neighbors(q, b, k)
        with pytest.raises(ValueError, match="k must be"):
            btsbot_amd.knn_graph(b, k)
    with pytest.raises(ValueError, match="metric"):
        btsbot_amd.embedding_neighbors(q, b, 2, metric="manhattan")
    with pytest.raises(ValueError, match="metric"):
        btsbot_amd.EmbeddingIndex(b, metric="l2")
    with pytest.raises(ValueError, match="splits"):
        btsbot_amd.embedding_neighbors(q, b, 2, splits=33)
    with pytest.raises(TypeError):
        btsbot_amd.embedding_neighbors(q.numpy(), b, 2)


# ---- 5. run_training: the new key is opt-in ------------------------------------------------------------------------
def test_run_training_writes_the_knn_file_only_on_request():
    import inspect
    from btsbot_amd import train
    src = inspect.getsource(train.write_embeddings)
    src = src[src.index('"""', src.index('"""') + 3):]               # the code behind the docstring
    gate = src.index('config.get("embedding_neighbors")')
    assert src.index('np.save(stem + ".npy", out)') < gate          # the .npy and .csv are written as before, first
    assert src.index('to_csv(stem + ".csv"') < gate
    assert src.index("_knn.npz") > gate and src.index("knn_graph") > gate
    body = src[gate:]
    assert body.startswith('config.get("embedding_neighbors")\n    if k:')
