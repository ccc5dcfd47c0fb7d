"""CPU-side checks of the grouped embedding neighbours (btsbot_knn_query_grouped, EmbeddingIndex(groups=...)): a numpy
emulation of the grouped two-pass scheme stays inside the contract of tests/knn_group_ref.py on every case the GPU test
uses, seeded faults do not, ``neighbor_vote`` equals a plain loop, and the new entry point refuses bad arguments before any
GPU call."""
import ctypes as C

import numpy as np
import pytest
import torch

import btsbot_amd
from btsbot_amd import _lib
import knn_group_ref as G
import knn_ref as R

METRICS = ("euclidean", "cosine")


def _kw(qg, bg, mode):
    exclude, one = G.MODES[mode]
    return dict(query_groups=qg, bank_groups=bg, exclude=exclude, one=one)


# ---- 1. a correct implementation stays inside the bounds -----------------------------------------------------------
@pytest.mark.parametrize("mode", list(G.MODES))
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_emulation_meets_the_contract(case, mode):
    k, splits = case[3], case[4]
    metric = METRICS[G.CASES.index(case) % 2]                 # both metrics over the list; the GPU test runs the product
    for kind in R.KINDS:
        q, b, qg, bg = G.case_inputs(case, kind)
        kw = _kw(qg, bg, mode)
        idx, dist = G.emulate(q, b, k, metric, splits, **kw)
        G.check_group_neighbors(q, b, idx, dist, k, metric, **kw)


def test_without_flags_the_emulation_and_the_checker_are_knn_refs():
    q, b, qg, bg = G.case_inputs(G.CASES[2], "normal")
    idx, dist = G.emulate(q, b, 15, "euclidean", 7, query_groups=qg, bank_groups=bg)
    ref_i, ref_d = R.emulate(q, b, 15, "euclidean", 7)
    assert np.array_equal(idx, ref_i) and np.array_equal(dist.view(np.int32), ref_d.view(np.int32))
    assert G.check_group_neighbors(q, b, idx, dist, 15) == R.check_neighbors(q, b, idx, dist, 15)


def _integer_case(n_q=130, n=1000, d=5):
    """Integer rows with period-24 duplicates spread over different groups (runs of 1-9 rows against period 24)."""
    b = R.make_rows("integer", n, d, 6)
    bg = G.make_groups("runs_hi32", n, 3)
    return b[:n_q].copy(), b, bg[:n_q].copy(), bg


@pytest.mark.parametrize("mode", list(G.MODES))
@pytest.mark.parametrize("splits", [1, 2, 7, 0])
def test_emulation_is_exact_on_integer_rows(splits, mode):
    q, b, qg, bg = _integer_case()
    kw = _kw(qg, bg, mode)
    idx, dist = G.emulate(q, b, 32, "euclidean", splits, self_offset=0, **kw)
    G.check_group_exact(q, b, idx, dist, 32, self_offset=0, **kw)
    G.check_group_neighbors(q, b, idx, dist, 32, self_offset=0, **kw)


def test_emulation_handles_non_finite_rows_and_small_banks():
    q, b = R.make_rows("normal", 20, 33, 1), R.make_rows("normal", 300, 33, 2)
    bg = np.arange(300, dtype=np.int64) // 3                   # objects of three rows
    qg = bg[np.arange(20) * 7]
    b[[3, 4, 5], 0] = np.nan                                   # a group whose rows are all non-finite
    b[30, 5] = np.inf                                          # groups that lose a row
    q[7, 0] = np.nan
    for mode in G.MODES:
        kw = _kw(qg, bg, mode)
        idx, dist = G.emulate(q, b, 15, "euclidean", 2, **kw)
        G.check_group_neighbors(q, b, idx, dist, 15, **kw)
        assert (idx[7] == -1).all() and np.isnan(dist[7]).all() and not np.isin(idx, [3, 4, 5, 30]).any()
    kw = _kw(np.full(20, 7, np.int64), np.full(300, 7, np.int64), "exclude")     # the bank is the query's group
    idx, dist = G.emulate(q, b, 4, **kw)
    G.check_group_neighbors(q, b, idx, dist, 4, **kw)
    assert (idx[:7] == -1).all() and np.isposinf(dist[:7]).all()
    kw = _kw(qg, bg % 5, "distinct")                                              # five groups, k = 15
    idx, dist = G.emulate(q, b, 15, **kw)
    G.check_group_neighbors(q, b, idx, dist, 15, **kw)
    assert (idx[0, :5] >= 0).all() and (idx[0, 5:] == -1).all()


# ---- 2. seeded faults are rejected -----------------------------------------------------------------------------------
def _rejected(fault, mode, cases=G.CASES):
    """The listed cases on which the checkers reject the emulation with ``fault`` seeded."""
    hit = []
    for case in cases:
        q, b, qg, bg = G.case_inputs(case, "normal")
        kw = _kw(qg, bg, mode)
        idx, dist = G.emulate(q, b, case[3], "euclidean", case[4], **kw, **fault)
        try:
            G.check_group_neighbors(q, b, idx, dist, case[3], **kw)
        except AssertionError as e:
            hit.append((G.case_id(case), str(e)))
    return hit


def test_checker_rejects_groups_compared_on_their_low_32_bits():
    for mode in G.MODES:
        hit = _rejected(dict(low32=True), mode)
        wide = {G.case_id(c) for c in G.CASES if c[5] in ("runs_hi32", "mod40_hi32", "negative")}
        assert hit and {c for c, _ in hit} <= wide, (mode, hit)   # (ids below 2^32 are compared in full either way)
    q, b, qg, bg = _integer_case()
    for mode in G.MODES:
        kw = _kw(qg, bg, mode)
        idx, dist = G.emulate(q, b, 15, splits=2, low32=True, **kw)
        with pytest.raises(AssertionError, match="exact"):
            G.check_group_exact(q, b, idx, dist, 15, **kw)


def test_checker_rejects_a_merge_that_does_not_collapse_groups_across_splits():
    for mode in ("distinct", "exclude+distinct"):
        hit = _rejected(dict(no_merge_collapse=True), mode)
        assert any("a group returned twice" in msg for _, msg in hit), hit
        assert not _rejected(dict(no_merge_collapse=True), mode, [c for c in G.CASES if c[4] == 1])   # one split: no fault
    q, b, qg, bg = _integer_case()
    kw = _kw(qg, bg % 3, "distinct")                           # every group has its best rows in several splits
    idx, dist = G.emulate(q, b, 15, splits=7, no_merge_collapse=True, **kw)
    with pytest.raises(AssertionError, match="exact"):
        G.check_group_exact(q, b, idx, dist, 15, **kw)


def test_checker_rejects_the_first_offered_row_as_representative():
    for mode in ("distinct", "exclude+distinct"):
        hit = _rejected(dict(first_offered=True), mode)
        assert any("rank" in msg for _, msg in hit), hit
    q, b, qg, bg = _integer_case()
    kw = _kw(qg, bg, "distinct")
    idx, dist = G.emulate(q, b, 15, splits=2, first_offered=True, **kw)
    with pytest.raises(AssertionError, match="exact"):
        G.check_group_exact(q, b, idx, dist, 15, **kw)


def test_checker_rejects_an_exclusion_skipped_for_one_bank_tile():
    for mode in ("exclude", "exclude+distinct"):
        hit = _rejected(dict(skip_exclude_tile=1), mode)
        assert any("ineligible" in msg for _, msg in hit), hit
        assert not _rejected(dict(skip_exclude_tile=1), mode, [c for c in G.CASES if c[1] <= G.TILE])   # no such tile


# ---- 3. neighbor_vote ------------------------------------------------------------------------------------------------
def _vote_loop(idx, dist, labels, weights):
    out = np.full(len(idx), np.nan, np.float32)
    for i in range(len(idx)):
        js = [j for j in range(idx.shape[1]) if idx[i, j] >= 0]
        if not js:
            continue
        zero = [j for j in js if dist[i, j] == 0]
        if weights == "uniform":
            w = {j: 1.0 for j in js}
        elif zero:
            w = {j: 1.0 for j in zero}
        else:
            w = {j: 1.0 / float(dist[i, j]) for j in js}
        out[i] = sum(w[j] for j in w if labels[idx[i, j]] != 0) / sum(w.values())
    return out


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_neighbor_vote_equals_a_plain_loop(weights):
    rng = np.random.default_rng(4)
    n, q, k = 50, 40, 7
    labels = rng.integers(0, 2, size=n)
    idx = rng.integers(0, n, size=(q, k))
    dist = np.sort(rng.random((q, k)).astype(np.float32) + 0.01, axis=1)
    for i in range(q):                                          # tails of -1 / +inf of every length
        cut = k - i % (k + 1)
        idx[i, cut:] = -1
        dist[i, cut:] = np.inf
    assert (idx[7] == -1).all()                                 # the all-invalid row
    dist[3, 0] = 0.0                                            # one zero distance takes the whole vote
    dist[8, :2] = 0.0                                           # two share it
    labels[idx[8, 0]], labels[idx[8, 1]] = 1, 0
    idx[8, 1] = idx[8, 1] if idx[8, 1] != idx[8, 0] else (idx[8, 0] + 1) % n
    dist[10, 0] = 1e-42                                         # 1 / dist overflows fp32
    got = btsbot_amd.neighbor_vote(torch.from_numpy(idx), torch.from_numpy(dist), torch.from_numpy(labels), weights)
    want = _vote_loop(idx, dist, labels, weights)
    assert got.dtype == torch.float32 and got.shape == (q,)
    assert np.isnan(got[7].item()) and np.isnan(want[7])
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-5, atol=1e-6, equal_nan=True)
    if weights == "distance":
        assert got[3].item() == float(labels[idx[3, 0]] != 0)
    with pytest.raises(ValueError, match="weights"):
        btsbot_amd.neighbor_vote(torch.from_numpy(idx), torch.from_numpy(dist), torch.from_numpy(labels), "rank")


# ---- 4. the library and the wrappers: symbols and limits, no GPU call ------------------------------------------------
def _grouped(L, *, nq=4, nb=10, dim=8, k=3, metric=0, splits=1, ws=1 << 40, qg=256, bg=256, flags=3, q=256):
    p = lambda v: C.c_void_p(v) if v else None   # (never dereferenced: refused before any HIP call)
    return L.btsbot_knn_query_grouped(p(q), nq, p(256), p(256), nb, dim, k, metric, -1, splits, p(256), p(256), p(256), ws,
                                      None, p(qg), p(bg), flags)


def test_the_grouped_entry_point_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert "btsbot_knn_query_grouped" in _lib.SYMBOLS and hasattr(C.CDLL(_lib.LIB_PATH), "btsbot_knn_query_grouped")
    assert (_lib.KNN_EXCLUDE_SAME, _lib.KNN_ONE_PER_GROUP, _lib.KNN_MAX_K_ONE_PER_GROUP) == (1, 2, 32) == (1, 2, G.MAX_K_ONE)
    bad = _lib.ERR_INVALID_ARG
    for flags in (4, -1, 7):
        assert _grouped(L, flags=flags) == bad and b"flags" in L.btsbot_last_error()
    assert _grouped(L, k=33, flags=2) == bad and b"k <= 32" in L.btsbot_last_error()
    assert _grouped(L, k=33, flags=3) == bad
    assert _grouped(L, k=65, flags=1) == bad
    assert _grouped(L, qg=0, flags=1) == bad and b"query_group" in L.btsbot_last_error()
    assert _grouped(L, bg=0, flags=2) == bad
    assert _grouped(L, bg=0, flags=1) == bad
    assert _grouped(L, metric=2) == bad and b"metric" in L.btsbot_last_error()
    assert _grouped(L, splits=33) == bad
    assert _grouped(L, ws=8) == bad and b"workspace" in L.btsbot_last_error()
    assert _grouped(L, q=0) == bad and b"NULL" in L.btsbot_last_error()
    assert b"btsbot_knn_query_grouped" in L.btsbot_last_error()
    assert _grouped(L, nq=0, q=0) == _lib.OK                    # nothing to do: no launch, no error
    # the workspace: btsbot_knn_workspace's, plus 8 bytes per list entry of the padded query tiles under ONE_PER_GROUP
    base = L.btsbot_knn_workspace(130, 5000, 5, 3, 7)
    assert L.btsbot_knn_workspace_grouped(130, 5000, 5, 3, 7, 0) == L.btsbot_knn_workspace_grouped(130, 5000, 5, 3, 7, 1) == base
    for flags in (2, 3):
        assert L.btsbot_knn_workspace_grouped(130, 5000, 5, 3, 7, flags) == base + 256 * 7 * 3 * 8
    assert L.btsbot_knn_workspace_grouped(130, 5000, 5, 3, 0, 2) - L.btsbot_knn_workspace(130, 5000, 5, 3, 0) == \
        256 * L.btsbot_knn_splits(130, 5000, 5, 3) * 3 * 8
    assert L.btsbot_knn_workspace_grouped(130, 5000, 5, 65, 7, 2) == bad
    assert _grouped(L, ws=L.btsbot_knn_workspace_grouped(4, 10, 8, 3, 1, 3) - 1) == bad and b"workspace" in L.btsbot_last_error()


def test_python_wrappers_refuse_bad_group_arguments_before_any_launch(monkeypatch):
    assert "neighbor_vote" in btsbot_amd.__all__
    from btsbot_amd import neighbors as N
    dev = torch.device("cpu")
    g = torch.arange(10)
    assert N._groups(g, "groups", 10, dev) is not None
    for wrong, what in ((g.int(), "int64"), (g.float(), "int64"), (g[:9], "one group per row"), (g[None], "one group per"),
                        (g.numpy(), "int64")):
        with pytest.raises(ValueError, match=what):
            N._groups(wrong, "groups", 10, dev)
    with pytest.raises(ValueError, match="is on"):
        N._groups(g, "groups", 10, torch.device("cuda:0"))
    with pytest.raises(ValueError, match="needs query_groups"):
        N._check_group_args(5, True, None, True, False)
    for switches in ((True, False), (False, True)):
        with pytest.raises(ValueError, match="built with groups"):
            N._check_group_args(5, False, g, *switches)
    with pytest.raises(ValueError, match="k <= 32"):
        N._check_group_args(33, True, g, False, True)
    assert N._check_group_args(33, True, g, True, False) == 1
    assert N._check_group_args(32, True, None, False, True) == 2
    assert N._check_group_args(64, True, g, False, False) == 0
    # the public calls run these checks in front of everything that touches the GPU
    q, b = torch.zeros(3, 8), torch.zeros(10, 8)
    with pytest.raises(ValueError, match="needs query_groups"):
        btsbot_amd.embedding_neighbors(q, b, 2, bank_groups=g, exclude_same_group=True)
    with pytest.raises(ValueError, match="built with groups"):
        btsbot_amd.embedding_neighbors(q, b, 2, one_per_group=True)
    with pytest.raises(ValueError, match="k <= 32"):
        btsbot_amd.embedding_neighbors(q, b, 33, bank_groups=g, one_per_group=True)
    with pytest.raises(ValueError, match="group_mode"):
        btsbot_amd.knn_graph(b, 2, groups=g, group_mode="collapse")
