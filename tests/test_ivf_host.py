"""IvfIndex and k-means without a GPU: the checkers of ivf_ref.py see seeded faults (and pass the float64 restatement's
own answers), and the argument checks that need no device refuse what they should."""
import ctypes

import numpy as np
import pytest
import torch

import btsbot_amd
import ivf_ref as V
import knn_ref as R
from btsbot_amd import _lib


def _case(seed=0, n=400, n_q=20, d=8, n_lists=6, nprobe=2, k=5, kind="normal"):
    b = R.make_rows(kind, n, d, 10 + seed)
    q = R.make_rows(kind, n_q, d, 20 + seed)
    c = b[np.arange(n_lists) * 7].copy()
    labels = V.assign64(b, c)
    probes = V.probes64(q, c, nprobe)
    idx, dist = V.query64(q, b, c, k, nprobe)
    return q, b, c, labels, probes, idx, dist


def test_the_restatement_passes_its_own_contract():
    q, b, c, labels, probes, idx, dist = _case()
    al = V.allowed_mask(b, labels, probes)
    V.check_allowed(q, b, idx, dist, 5, al)
    sr = np.arange(20, dtype=np.int64)
    idx2, dist2 = V.query64(b[:20], b, c, 5, 2, self_rows=sr)
    V.check_allowed(b[:20], b, idx2, dist2, 5, V.allowed_mask(b, labels, V.probes64(b[:20], c, 2), sr))
    assert not (idx2 == sr[:, None]).any()


def test_a_returned_row_outside_the_probed_lists_is_seen():
    q, b, c, labels, probes, idx, dist = _case()
    al = V.allowed_mask(b, labels, probes)
    outside = np.nonzero(~al[3] & V.usable_rows(b))[0]
    # the nearest row that is NOT allowed, put where it would stand by distance: only the mask can tell
    d2 = R.direct64(q[3], b[outside], "euclidean")
    bad_i, bad_d = idx.copy(), dist.copy()
    bad_i[3, -1], bad_d[3, -1] = outside[np.argmin(d2)], max(np.sqrt(d2.min()), dist[3, -2] * (1 + 1e-6))
    with pytest.raises(AssertionError, match="outside the allowed set"):
        V.check_allowed(q, b, bad_i, bad_d, 5, al)


def test_fewer_allowed_rows_than_k_and_non_finite_rows():
    q, b, c, labels, probes, idx, dist = _case(n=60, n_lists=6, nprobe=1, k=15)
    b[4] = np.nan
    q[2, 1] = np.inf
    labels = V.assign64(b, c)
    assert labels[4] == -1
    idx, dist = V.query64(q, b, c, 15, 1)
    assert (idx[2] == -1).all() and np.isnan(dist[2]).all() and (idx[:, -1] == -1).any() and not (idx == 4).any()
    al = V.allowed_mask(b, labels, V.probes64(q, c, 1))
    V.check_allowed(q, b, idx, dist, 15, al)
    short = np.nonzero((idx[:, -1] == -1) & (idx[:, 0] >= 0))[0][0]
    bad = dist.copy()
    bad[short, -1] = 1.0
    with pytest.raises(AssertionError, match="tail"):
        V.check_allowed(q, b, idx, bad, 15, al)


def test_a_swapped_tie_is_seen():
    q, b, c, labels, probes, idx, dist = _case(kind="integer", n=300, d=5, k=6)
    al = V.allowed_mask(b, labels, probes)
    V.check_exact_allowed(q, b, idx, dist, 6, al)
    rows = [(i, j) for i in range(len(q)) for j in range(5) if dist[i, j] == dist[i, j + 1] and idx[i, j + 1] >= 0]
    assert rows, "the integer rows are drawn from 24 distinct rows: ties are everywhere"
    i, j = rows[0]
    bad = idx.copy()
    bad[i, j], bad[i, j + 1] = idx[i, j + 1], idx[i, j]
    with pytest.raises(AssertionError, match="exact: indices"):
        V.check_exact_allowed(q, b, bad, dist, 6, al)
    with pytest.raises(AssertionError, match="not sorted"):
        V.check_allowed(q, b, bad, dist, 6, al)


def test_a_centroid_off_by_twice_the_bound_is_seen():
    rng = np.random.default_rng(3)
    rows = (rng.standard_normal((1000, 33)) + 0.5).astype(np.float32)
    labels = rng.integers(-1, 7, 1000)
    labels[labels == 3] = 2                       # cluster 3 is empty
    prev = np.full((7, 33), 77.0)
    mean = V.means64(rows, labels, 7, prev)
    bound = V.mean_bound(rows, labels, 7)
    assert (bound[3] == 0).all() and (bound[[0, 1, 2, 4, 5, 6]] > 0).all()
    # an fp32 summation in the kernel's shape stays inside the bound
    got = prev.astype(np.float32)
    for c in range(7):
        x = rows[labels == c]
        if len(x):
            parts = [np.add.reduce(x[a:a + V.CHUNK], axis=0, dtype=np.float32) for a in range(0, len(x), V.CHUNK)]
            s = parts[0]
            for p in parts[1:]:
                s = s + p
            got[c] = s / np.float32(len(x))
    V.check_centroids(got, rows, labels, 7, prev)
    off = mean.copy()
    off[5, 11] += 2 * bound[5, 11]
    with pytest.raises(AssertionError, match="centroid 5"):
        V.check_centroids(off, rows, labels, 7, prev)
    touched = mean.copy()
    touched[3, 0] = 0.0
    with pytest.raises(AssertionError, match="empty cluster"):
        V.check_centroids(touched, rows, labels, 7, prev)


def test_a_missing_list_row_is_seen():
    labels = np.array([2, 0, -1, 2, 1, 0, 2], np.int64)
    indptr, rows = np.array([0, 2, 3, 6]), np.array([1, 5, 4, 0, 3, 6])
    V.check_lists(labels, 3, indptr, rows)
    with pytest.raises(AssertionError, match="list 2"):
        V.check_lists(labels, 3, np.array([0, 2, 3, 5]), np.array([1, 5, 4, 0, 6]))
    with pytest.raises(AssertionError, match="list 0"):
        V.check_lists(labels, 3, indptr, np.array([5, 1, 4, 0, 3, 6]))


def test_lloyd_in_float64_finds_integer_blobs():
    bank, _ = V.blobs(500, 0, seed=1, spread=0.05)
    init = bank[:10].astype(np.float64)
    cs, ls, final = V.lloyd(bank, init, 3)
    assert (final == np.arange(500) % 10).all() and (ls == final).all()
    assert np.abs(cs[-1] - np.round(cs[-1])).max() < 0.05 and (cs[2] == cs[3]).all()


def test_arguments_refused_before_the_device():
    rows = torch.zeros((10, 4))
    with pytest.raises(ValueError, match="not built"):
        btsbot_amd.kmeans(rows, 2, metric="cosine")
    with pytest.raises(ValueError, match="not built"):
        btsbot_amd.IvfIndex(rows, 2, metric="cosine")
    for bad in (0, 65537, 2.0, True):
        with pytest.raises(ValueError, match="n_clusters"):
            btsbot_amd.kmeans(rows, bad)
        with pytest.raises(ValueError, match="n_lists"):
            btsbot_amd.IvfIndex(rows, bad)
    with pytest.raises(ValueError, match="n_iter"):
        btsbot_amd.kmeans(rows, 2, n_iter=-1)
    with pytest.raises(ValueError, match="k-means\\+\\+ is not built"):
        btsbot_amd.kmeans(rows, 2, init="k-means++")
    with pytest.raises(ValueError, match="float32"):
        btsbot_amd.kmeans(rows, 2, init=torch.zeros((2, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="n_clusters = 2"):
        btsbot_amd.kmeans(rows, 2, init=torch.zeros((3, 4)))
    with pytest.raises(ValueError, match="float32"):
        btsbot_amd.IvfIndex(rows, centroids=torch.zeros((3, 4), dtype=torch.float16))
    with pytest.raises(ValueError, match="n_clusters = 2"):
        btsbot_amd.IvfIndex(rows, 2, centroids=torch.zeros((3, 4)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        btsbot_amd.kmeans(rows, 2)
    assert [btsbot_amd.ivf.default_n_lists(n) for n in (0, 1, 2, 1000, 10 ** 6, 10 ** 10)] == [1, 1, 1, 32, 1000, 65536]

    # query's k, nprobe and self_rows are checked before its rows: an index that holds only what those checks read
    ivf = btsbot_amd.IvfIndex.__new__(btsbot_amd.IvfIndex)
    ivf.centroids, ivf.device, ivf.dim = torch.zeros((4, 3)), torch.device("cpu"), 3
    q = torch.zeros((2, 3))
    for k in (0, 65, 1.0):
        with pytest.raises(ValueError, match="k must be"):
            ivf.query(q, k)
    for nprobe in (0, 5, 33, True):
        with pytest.raises(ValueError, match="nprobe must be an int in 1..4"):
            ivf.query(q, 3, nprobe)
        with pytest.raises(ValueError, match="nprobe"):
            ivf.probes(q, nprobe)
        with pytest.raises(ValueError, match="nprobe"):
            ivf.knn_graph(3, nprobe=nprobe)
    with pytest.raises(ValueError, match="self_rows must be an int64"):
        ivf.query(q, 3, 2, self_rows=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="one bank row per query row"):
        ivf.query(q, 3, 2, self_rows=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ivf.query(q, 3, 2)


def test_c_entry_points_check_their_arguments_on_the_host():
    L, vp = _lib.lib(), ctypes.c_void_p

    def refused(rc, word):
        assert rc == _lib.ERR_INVALID_ARG and word in L.btsbot_last_error().decode(), (rc, word, L.btsbot_last_error())

    assert L.btsbot_ivf_list_rows(1000, 16) == (1000 // 128 + 16) * 128
    assert L.btsbot_ivf_list_rows(0, 1) == 128
    refused(L.btsbot_ivf_list_rows(10, 0), "n_lists")
    refused(L.btsbot_ivf_list_rows(10, 65537), "n_lists")
    need = L.btsbot_ivf_workspace(100, 528, 15, 8, 1024)
    image = (100 * (16 + 4 * 544) + 255) // 256 * 256
    assert need >= image + 100 * 8 * 15 * 8 and need < image + 100 * 8 * 15 * 8 + 100 * 8 * 4 + 3 * 4 * 1025 + 6 * 256
    refused(L.btsbot_ivf_workspace(100, 528, 65, 8, 1024), "k")
    refused(L.btsbot_ivf_workspace(100, 528, 15, 33, 1024), "nprobe")
    refused(L.btsbot_ivf_workspace(100, 528, 15, 8, 4), "nprobe")
    refused(L.btsbot_ivf_workspace(1 << 30, 528, 15, 8, 16), "2^31")
    refused(L.btsbot_kmeans_workspace(100, 0, 4), "dim")
    assert L.btsbot_kmeans_workspace(1000, 33, 7) >= (1000 // 64 + 7) * 33 * 4
    rows = L.btsbot_ivf_list_rows(1000, 16)
    q = lambda nprobe, lr, ws: L.btsbot_ivf_query(vp(0), 10, vp(0), 1000, 33, 5, vp(0), nprobe, vp(0), vp(0), lr, vp(0),   # noqa: E731
                                                  vp(0), vp(0), 16, vp(0), vp(0), vp(0), ws, vp(0))
    refused(q(17, rows, 0), "nprobe")
    refused(q(4, rows + 128, 0), "n_list_rows")
    refused(q(4, rows, 0), "NULL")
    refused(L.btsbot_kmeans_update(vp(0), 10, 4, vp(0), vp(0), 2, vp(0), vp(0), vp(0), 0, vp(0)), "NULL")
    refused(L.btsbot_kmeans_update(vp(16), 10, 4, vp(16), vp(16), 2, vp(16), vp(16), vp(16), 8, vp(0)), "workspace")
    refused(L.btsbot_ivf_layout(vp(16), 10, 4, vp(16), vp(16), 2, vp(16), 128, vp(16), vp(16), vp(16), vp(16), vp(16), 0, vp(0)),
            "n_list_rows")
    refused(L.btsbot_ivf_layout(vp(16), 10, 4, vp(16), vp(16), 2, vp(16), 256, vp(16), vp(16), vp(16), vp(16), vp(16), 0, vp(0)),
            "workspace")
