"""IvfIndex by source without a GPU: the checkers of ivf_group_ref.py pass the float64 restatement's own answers and see
seeded faults, and the argument checks that need no device -- Python's and the new C entry points' -- refuse what they
should."""
import ctypes

import numpy as np
import pytest
import torch

import btsbot_amd
import ivf_group_ref as G
import ivf_ref as V
import knn_ref as R
from btsbot_amd import _lib
from btsbot_amd.neighbors import EmbeddingIndex
from knn_group_ref import MODES

N, NQ, D, LISTS, NPROBE, K = 400, 20, 8, 6, 3, 5


def _case(kind="normal", seed=0, k=K):
    """Rows in six lists, three probed; group = row % 40, so every group has rows in several lists; a query row takes the
    group of its nearest allowed row."""
    b = R.make_rows(kind, N, D, 10 + seed)
    q = R.make_rows(kind, NQ, D, 20 + seed)
    c = b[np.arange(LISTS) * 7].copy()
    bg = (np.arange(N, dtype=np.int64) % 40) * 3 - 50
    plain, _ = V.query64(q, b, c, k, NPROBE)
    qg = bg[plain[:, 0]]
    return q, b, c, qg, bg


def _sorted_in(q_row, b, rows):
    """(idx, dist fp32) of ``rows`` in (float64 distance, row) order."""
    rows = np.asarray(sorted(rows), np.int64)
    d2 = R.direct64(q_row, b[rows], "euclidean")
    o = np.argsort(d2, kind="stable")
    return rows[o], np.sqrt(d2[o]).astype(np.float32)


@pytest.mark.parametrize("mode", list(MODES))
def test_the_restatement_passes_its_own_contract(mode):
    q, b, c, qg, bg = _case()
    ex, one = MODES[mode]
    idx, dist, al, _pr, _lab = G.query64(q, b, c, K, NPROBE, qg, bg, ex, one)
    G.check_group_allowed(q, b, idx, dist, K, al, qg, bg, ex, one)
    if ex:
        assert not (bg[idx] == qg[:, None]).any()
    if one:
        assert all(len(set(bg[r].tolist())) == K for r in idx)
    # with self_rows: the row itself leaves by position, its group stays unless excluded
    sr = np.arange(NQ, dtype=np.int64) * 3
    idx, dist, al, _pr, _lab = G.query64(b[sr], b, c, K, NPROBE, bg[sr], bg, ex, one, self_rows=sr)
    G.check_group_allowed(b[sr], b, idx, dist, K, al, bg[sr], bg, ex, one)
    assert not (idx == sr[:, None]).any()


def test_a_row_of_the_querys_own_group_is_seen():
    q, b, c, qg, bg = _case()
    idx, dist, al, _pr, _lab = G.query64(q, b, c, K, NPROBE, qg, bg, True, False)
    i = 3
    own = np.flatnonzero(al[i] & (bg == qg[i]))
    assert len(own), "the query's group has no allowed row: the case is wrong"
    # the nearest row of its own group, put where it would stand by distance: only the groups can tell
    bad_i, bad_d = idx.copy(), dist.copy()
    bad_i[i], bad_d[i] = (x[:K] for x in _sorted_in(q[i], b, list(idx[i, :-1]) + [own[np.argmin(R.direct64(q[i], b[own], "euclidean"))]]))
    assert (bg[bad_i[i]] == qg[i]).sum() == 1
    with pytest.raises(AssertionError, match="ineligible row"):
        G.check_group_allowed(q, b, bad_i, bad_d, K, al, qg, bg, True, False)
    V.check_allowed(q[i:i + 1], b, bad_i[i:i + 1], bad_d[i:i + 1], K, al[i:i + 1])    # the ungrouped contract is blind to it


def test_a_group_returned_twice_from_two_probed_lists_is_seen():
    q, b, c, qg, bg = _case()
    idx, dist, al, _pr, labels = G.query64(q, b, c, K, NPROBE, qg, bg, False, True)
    for i in range(NQ):
        for r in idx[i]:
            twin = np.flatnonzero(al[i] & (bg == bg[r]) & (labels != labels[r]))
            if len(twin):
                break
        else:
            continue
        break
    else:
        raise AssertionError("no returned group has rows in two probed lists: the case is wrong")
    bad_i, bad_d = idx.copy(), dist.copy()
    bad_i[i], bad_d[i] = _sorted_in(q[i], b, list(idx[i, :-1]) + [twin[0]] if idx[i, -1] != r else list(idx[i, 1:]) + [twin[0]])
    assert labels[twin[0]] != labels[r] and (bg[bad_i[i]] == bg[r]).sum() == 2
    with pytest.raises(AssertionError, match="a group returned twice"):
        G.check_group_allowed(q, b, bad_i, bad_d, K, al, qg, bg, False, True)


def test_a_row_behind_its_groups_nearest_in_another_probed_list_is_seen():
    """Three groups whose nearest rows stand within 1.2 tau of each other: returning group 10 by its row in list 1, 1.1 tau
    behind its nearest in list 0, leaves every r_j within tau of t_j -- only the group's own minimum tells."""
    tau = 8 * (D + 2) * R.U * 1.0
    q = np.zeros((1, D), np.float32)
    b = np.zeros((4, D), np.float32)
    b[:, 0] = np.sqrt(1 + np.array([0.0, 0.6, 1.1, 1.2]) * tau)
    bg = np.array([10, 20, 10, 30], np.int64)
    labels, probes = np.array([0, 0, 1, 1]), np.array([[0, 1]])
    al = V.allowed_mask(b, labels, probes)
    qg = np.array([99], np.int64)
    idx, dist = G.group_answer64(q, b, 3, al, qg, bg, False, True)
    assert idx.tolist() == [[0, 1, 3]]
    G.check_group_allowed(q, b, idx, dist, 3, al, qg, bg, False, True)
    bad_i, bad_d = _sorted_in(q[0], b, [1, 2, 3])
    assert bad_i.tolist() == [1, 2, 3] and labels[2] != labels[0]
    with pytest.raises(AssertionError, match="behind its own group's nearest"):
        G.check_group_allowed(q, b, bad_i[None], bad_d[None], 3, al, qg, bg, False, True)


@pytest.mark.parametrize("mode", list(MODES))
def test_a_swapped_tie_is_seen(mode):
    q, b, c, qg, bg = _case(kind="integer", k=6)
    ex, one = MODES[mode]
    idx, dist, al, _pr, _lab = G.query64(q, b, c, 6, NPROBE, qg, bg, ex, one)
    G.check_group_exact_allowed(q, b, idx, dist, 6, al, qg, bg, ex, one)
    G.check_group_allowed(q, b, idx, dist, 6, al, qg, bg, ex, one)
    rows = [(i, j) for i in range(NQ) for j in range(5) if dist[i, j] == dist[i, j + 1] and idx[i, j + 1] >= 0]
    assert rows, "the integer rows are drawn from few distinct rows: ties are everywhere"
    i, j = rows[0]
    bad = idx.copy()
    bad[i, j], bad[i, j + 1] = idx[i, j + 1], idx[i, j]
    with pytest.raises(AssertionError, match="exact: indices"):
        G.check_group_exact_allowed(q, b, bad, dist, 6, al, qg, bg, ex, one)
    with pytest.raises(AssertionError, match="not sorted"):
        G.check_group_allowed(q, b, bad, dist, 6, al, qg, bg, ex, one)


def test_a_wrong_tail_is_seen():
    """One group in the whole bank: one_per_group has one row to give, exclusion of that group none."""
    q, b, c, _qg, _bg = _case()
    bg = np.full(N, 7, np.int64)
    qg = np.full(NQ, 7, np.int64)
    q[2, 1] = np.inf
    idx, dist, al, _pr, _lab = G.query64(q, b, c, K, NPROBE, qg, bg, False, True)
    assert (idx[:, 1:] == -1).all() and (idx[[0, 1, 3], 0] >= 0).all() and np.isnan(dist[2]).all()
    G.check_group_allowed(q, b, idx, dist, K, al, qg, bg, False, True)
    plain = V.query64(q, b, c, K, NPROBE)
    with pytest.raises(AssertionError, match="tail"):
        G.check_group_allowed(q, b, *plain, K, al, qg, bg, False, True)       # the ungrouped answer: K rows of group 7
    none_i, none_d, al, _pr, _lab = G.query64(q, b, c, K, NPROBE, qg, bg, True, True)
    assert (none_i == -1).all() and np.isposinf(none_d[[0, 1, 3]]).all()
    G.check_group_allowed(q, b, none_i, none_d, K, al, qg, bg, True, True)
    bad = none_d.copy()
    bad[5, -1] = 1.0
    with pytest.raises(AssertionError, match="tail"):
        G.check_group_allowed(q, b, none_i, bad, K, al, qg, bg, True, True)


def _bare_index(groups):
    """An IvfIndex that holds only what the argument checks read (four lists, D = 3, on the CPU)."""
    ivf = btsbot_amd.IvfIndex.__new__(btsbot_amd.IvfIndex)
    ivf.centroids, ivf.device, ivf.dim = torch.zeros((4, 3)), torch.device("cpu"), 3
    ivf.index = EmbeddingIndex.__new__(EmbeddingIndex)
    ivf.index._groups, ivf.index._n = groups, 5
    return ivf


def test_group_arguments_refused_before_the_device():
    rows = torch.zeros((10, 4))
    with pytest.raises(ValueError, match="groups must be an int64"):
        btsbot_amd.IvfIndex(rows, 2, groups=torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError, match="one group per row"):
        btsbot_amd.IvfIndex(rows, 2, groups=torch.zeros(9, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.IvfIndex(rows, 2, groups=torch.zeros(10, dtype=torch.int64))

    q, qg = torch.zeros((2, 3)), torch.zeros(2, dtype=torch.int64)
    plain = _bare_index(None)
    assert plain.groups is None
    for kw in (dict(exclude_same_group=True, query_groups=qg), dict(one_per_group=True)):
        with pytest.raises(ValueError, match="built with groups"):
            plain.query(q, 3, 2, **kw)
    for mode in MODES:
        with pytest.raises(ValueError, match="built with groups"):
            plain.knn_graph(3, nprobe=2, group_mode=mode)
    with pytest.raises(ValueError, match="takes groups if and only if"):
        plain.add(q, groups=qg)

    ivf = _bare_index(torch.zeros(5, dtype=torch.int64))
    assert ivf.groups.shape == (5,)
    with pytest.raises(ValueError, match="takes groups if and only if"):
        ivf.add(q)
    with pytest.raises(ValueError, match="needs query_groups"):
        ivf.query(q, 3, 2, exclude_same_group=True)
    with pytest.raises(ValueError, match="k <= 32"):
        ivf.query(q, 33, 2, one_per_group=True)
    with pytest.raises(ValueError, match="k <= 32"):
        ivf.knn_graph(34, nprobe=2, group_mode="distinct")
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # (k = 34 is fine without one_per_group)
        ivf.query(q, 34, 2, exclude_same_group=True, query_groups=qg)
    with pytest.raises(ValueError, match="must be bools"):
        ivf.query(q, 3, 2, one_per_group=1)
    with pytest.raises(ValueError, match="query_groups must be an int64"):
        ivf.query(q, 3, 2, exclude_same_group=True, query_groups=qg.to(torch.int32))
    with pytest.raises(ValueError, match="one group per row"):
        ivf.query(q, 3, 2, exclude_same_group=True, query_groups=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="group_mode must be"):
        ivf.knn_graph(3, nprobe=2, group_mode="same")
    # k, nprobe and self_rows keep their place in front
    with pytest.raises(ValueError, match="nprobe must be an int in 1..4"):
        ivf.query(q, 3, 5, one_per_group=True)
    with pytest.raises(ValueError, match="self_rows must be an int64"):
        ivf.query(q, 3, 2, one_per_group=True, self_rows=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ivf.query(q, 3, 2, one_per_group=True, self_rows=torch.zeros(2, dtype=torch.int64))


def test_grouped_c_entry_points_check_their_arguments_on_the_host():
    L, vp = _lib.lib(), ctypes.c_void_p

    def refused(rc, word):
        assert rc == _lib.ERR_INVALID_ARG and word in L.btsbot_last_error().decode(), (rc, word, L.btsbot_last_error())

    plain = L.btsbot_ivf_workspace(100, 528, 15, 8, 1024)
    assert L.btsbot_ivf_workspace_grouped(100, 528, 15, 8, 1024, 0) == plain
    assert L.btsbot_ivf_workspace_grouped(100, 528, 15, 8, 1024, _lib.KNN_EXCLUDE_SAME) == plain
    lg = 100 * 8 * 15 * 8                                       # int64 [k][n_query * nprobe], and no n_lists term
    for flags in (_lib.KNN_ONE_PER_GROUP, _lib.KNN_ONE_PER_GROUP | _lib.KNN_EXCLUDE_SAME):
        assert plain + lg <= L.btsbot_ivf_workspace_grouped(100, 528, 15, 8, 1024, flags) < plain + lg + 256
        assert (L.btsbot_ivf_workspace_grouped(100, 528, 15, 8, 65536, flags) - L.btsbot_ivf_workspace(100, 528, 15, 8, 65536)
                == L.btsbot_ivf_workspace_grouped(100, 528, 15, 8, 1024, flags) - plain)
    refused(L.btsbot_ivf_workspace_grouped(100, 528, 15, 8, 1024, 4), "flags")
    refused(L.btsbot_ivf_workspace_grouped(100, 528, 33, 8, 1024, _lib.KNN_ONE_PER_GROUP), "k=33")
    assert L.btsbot_ivf_workspace_grouped(100, 528, 33, 8, 1024, _lib.KNN_EXCLUDE_SAME) > 0
    refused(L.btsbot_ivf_workspace_grouped(100, 528, 15, 33, 1024, 1), "nprobe")

    rows = L.btsbot_ivf_list_rows(1000, 16)

    def ask(k, flags, qg, lgp, ws=1 << 30):
        return L.btsbot_ivf_query_grouped(vp(16), 10, vp(16), 1000, 33, k, vp(16), 4, vp(0), vp(16), rows, vp(16), vp(16), vp(16),
                                          16, vp(16), vp(16), vp(16), ws, vp(0), qg, lgp, flags)

    refused(ask(5, 8, vp(16), vp(16)), "flags")
    refused(ask(33, _lib.KNN_ONE_PER_GROUP, vp(16), vp(16)), "k=33")
    refused(ask(5, _lib.KNN_EXCLUDE_SAME, vp(0), vp(16)), "query_group")
    refused(ask(5, _lib.KNN_EXCLUDE_SAME, vp(16), vp(0)), "list_group")
    refused(ask(5, _lib.KNN_ONE_PER_GROUP, vp(0), vp(0)), "list_group")
    refused(ask(5, _lib.KNN_ONE_PER_GROUP, vp(0), vp(16), ws=L.btsbot_ivf_workspace(10, 33, 5, 4, 16)), "workspace")
    refused(L.btsbot_ivf_layout_groups(vp(0), 1000, 16, vp(16), rows, vp(16), vp(0)), "bank_group")
    refused(L.btsbot_ivf_layout_groups(vp(16), 1000, 16, vp(16), rows, vp(0), vp(0)), "list_group")
    refused(L.btsbot_ivf_layout_groups(vp(16), 1000, 16, vp(16), rows + 128, vp(16), vp(0)), "n_list_rows")
