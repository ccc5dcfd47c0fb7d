"""What the grouped IvfIndex tests share (numpy, no GPU): the contract of ``IvfIndex.query`` under ``exclude_same_group``
and ``one_per_group`` (btsbot_amd/ivf.py) as checkers, and its float64 restatement.

With allowed(q) of ivf_ref (the finite bank rows of the probed lists, minus self_rows[q]) and, under exclusion, only its
rows of another group than query_groups[q]:
  ``check_group_allowed``        clauses 1-3 of knn_group_ref.check_group_neighbors with "eligible" read as that set
  ``check_group_exact_allowed``  clause 4 on integer rows in [-8, 8], by knn_group_ref.exact_answer's rule
u, the distance bound and tau are knn_ref's, in ivf_ref.check_allowed's form (the maximum norm over the WHOLE bank: the
selection scores are those of the exact search, whatever list a row lies in).  No new tolerance.
"""
import numpy as np

import ivf_ref as V
from knn_group_ref import _group_minima
from knn_ref import U, dist64_matrix, direct64


def eligible(allowed, query_groups, bank_groups, exclude):
    """bool [Q, N]: ``allowed`` and, under exclusion, of another group than the query row."""
    el = np.array(allowed, bool, copy=True)
    if exclude:
        el &= np.asarray(bank_groups, np.int64)[None, :] != np.asarray(query_groups, np.int64)[:, None]
    return el


def check_group_allowed(q, b, idx, dist, k, allowed, query_groups, bank_groups, exclude, one):
    """Clauses 1-3; raises AssertionError naming the clause.  Returns the worst (distance error / bound, rank excess /
    tau)."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    idx, dist = np.asarray(idx), np.asarray(dist)
    bg = np.asarray(bank_groups, np.int64)
    n_q, d = q.shape
    n = b.shape[0]
    assert idx.shape == (n_q, k) and dist.shape == (n_q, k), "shape"
    assert idx.dtype == np.int64 and dist.dtype == np.float32, "dtype"
    assert np.asarray(allowed).shape == (n_q, n), "mask shape"
    el = eligible(allowed, query_groups, bg, exclude)
    dm = dist64_matrix(q, b, "euclidean") if n else np.zeros((n_q, 0))
    qfin = V.usable_rows(q)
    bfin = V.usable_rows(b)
    bb_max = float((b[bfin].astype(np.float64) ** 2).sum(1).max()) if bfin.any() else 0.0
    worst_d = worst_r = 0.0
    for i in range(n_q):
        if not qfin[i]:
            assert (idx[i] == -1).all() and np.isnan(dist[i]).all(), f"validity: non-finite query row {i}"
            continue
        cols = np.flatnonzero(el[i])
        if one:
            groups_i, gmin = _group_minima(dm[i, cols], bg[cols])
            m = min(k, len(groups_i))
        else:
            m = min(k, len(cols))
        assert (idx[i, m:] == -1).all() and np.isposinf(dist[i, m:]).all(), f"validity: tail of row {i}"
        got = idx[i, :m]
        assert ((got >= 0) & (got < n)).all(), f"validity: index out of range in row {i}"
        assert len(set(got.tolist())) == m, f"validity: repeated index in row {i}"
        assert el[i, got].all(), f"validity: ineligible row returned for query {i}"
        if one:
            assert len(set(bg[got].tolist())) == m, f"validity: a group returned twice for query {i}"
        dd = dist[i, :m].astype(np.float64)
        assert np.isfinite(dd).all(), f"validity: non-finite distance in row {i}"
        order_ok = (dd[1:] > dd[:-1]) | ((dd[1:] == dd[:-1]) & (got[1:] > got[:-1]))
        assert order_ok.all(), f"validity: row {i} not sorted by (dist, index)"
        if m == 0:
            continue
        r = direct64(q[i], b[got], "euclidean")
        d64 = np.sqrt(r)
        bound = (d + 4) * U * d64
        tau = 8 * (d + 2 if d >= 4 else d + 6) * U * (float((q[i].astype(np.float64) ** 2).sum()) + bb_max)
        err = np.abs(dd - d64)
        assert (err <= bound).all(), (f"distance: row {i} off by {err.max():.3e} "
                                      f"({(err / np.where(bound > 0, bound, 1)).max():.2f} of the bound)")
        t = np.sort(gmin if one else dm[i, cols])[:m]
        excess = r - t
        assert (excess <= tau).all(), f"rank: row {i} exceeds t_j by {excess.max():.3e} = {excess.max() / tau:.2f} tau"
        if one:
            over = r - gmin[np.searchsorted(groups_i, bg[got])]
            assert (over <= tau).all(), (f"rank: row {i} returns a row {over.max():.3e} = {over.max() / tau:.2f} tau "
                                         f"behind its own group's nearest")
        nz = bound > 0
        if nz.any():
            worst_d = max(worst_d, float((err[nz] / bound[nz]).max()))
        if tau > 0:
            worst_r = max(worst_r, float(excess.max() / tau))
    return worst_d, worst_r


def group_answer64(q, b, k, allowed, query_groups, bank_groups, exclude, one):
    """The grouped answer over the mask restated in float64 (knn_group_ref.exact_answer's rule: under ``one`` a group is
    represented by its lowest row at the group's minimum distance): (idx int64 [Q, k], dist fp32 [Q, k])."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    bg = np.asarray(bank_groups, np.int64)
    el = eligible(allowed, query_groups, bg, exclude)
    d2 = dist64_matrix(q, b, "euclidean") if b.shape[0] else np.zeros((q.shape[0], 0))
    idx = np.full((q.shape[0], k), -1, np.int64)
    dist = np.full((q.shape[0], k), np.inf, np.float32)
    ok = V.usable_rows(q)
    for i in range(q.shape[0]):
        if not ok[i]:
            dist[i] = np.nan
            continue
        cols = np.flatnonzero(el[i])
        if one and len(cols):
            g = bg[cols]
            o = np.lexsort((cols, d2[i, cols], g))          # by group, then distance, then row
            cols = np.sort(cols[o][np.r_[True, g[o][1:] != g[o][:-1]]])
        order = cols[np.argsort(d2[i, cols], kind="stable")][:k]
        idx[i, :len(order)] = order
        dist[i, :len(order)] = np.sqrt(d2[i, order]).astype(np.float32)
    return idx, dist


def check_group_exact_allowed(q, b, idx, dist, k, allowed, query_groups, bank_groups, exclude, one):
    """Clause 4 under the mask (integer rows in [-8, 8]), ties included."""
    d2 = dist64_matrix(np.asarray(q, np.float32), np.asarray(b, np.float32), "euclidean")
    assert (d2 == np.round(d2)).all()
    assert V.usable_rows(q).all()
    want_i, want_d = group_answer64(q, b, k, allowed, query_groups, bank_groups, exclude, one)
    idx, dist = np.asarray(idx), np.asarray(dist)
    for i in range(len(want_i)):
        assert (idx[i] == want_i[i]).all(), f"exact: indices of row {i}: {idx[i].tolist()} != {want_i[i].tolist()}"
        assert (dist[i] == want_d[i]).all(), f"exact: distances of row {i}"


def query64(q, b, centroids, k, nprobe, query_groups, bank_groups, exclude, one, self_rows=None, labels=None):
    """The whole grouped query restated in float64: ivf_ref's labels, probes and mask, then ``group_answer64``.
    Returns (idx, dist, allowed, probes, labels)."""
    b = np.asarray(b, np.float32)
    if labels is None:
        labels = V.assign64(b, centroids)
    pr = V.probes64(q, centroids, nprobe)
    al = V.allowed_mask(b, labels, pr, self_rows)
    idx, dist = group_answer64(q, b, k, al, query_groups, bank_groups, exclude, one)
    return idx, dist, al, pr, labels
