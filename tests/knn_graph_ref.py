"""What the KnnGraph tests share (no GPU): the merge rule of btsbot_knn_graph_merge written plainly, the float64 mask of
the rows on which an updated graph must equal a rebuilt one, and the contract of a list that went through ``u`` merges
(btsbot_amd/graph.py).  Builds on knn_ref and knn_group_ref, which stay as they are.

The rule (B): an old row's list becomes the first k, by fp32 (dist, index), of its present entries and its offers; in the
distinct modes an entry is emitted only if its group differs from every entry emitted before it; the tail is -1 / +inf.

Separated rows (C): a row whose k-th and (k+1)-th smallest eligible float64 squared distances (in the distinct modes: of
the per-group minima, and no group among the first k + 1 holds a second row within the band of its nearest) lie more than
2 tau apart, tau as in knn_ref; a row with at most k eligible candidates is separated.

The contract after u merges: knn_ref's clauses 1 and 2 as they stand; clause 3 with
    euclidean  r_j <= (t_j + tau) ((1 + e) / (1 - e))^(2 u),   e = (D + 4) 2^-24
    cosine     r_j <= t_j + tau + 2 u delta,                   delta = 4 (D + 2) 2^-24
(each merge orders by the fp32 direct form, whose rounding enters the bound once on either side of a comparison).
"""
import numpy as np

import knn_group_ref as G
import knn_ref as R

U = R.U


def merge_lists(old_idx, old_dist, offer_idx, offer_dist, k, groups=None, distinct=False):
    """One row: (idx int64 [k], dist float32 [k]) from its list (old_idx [k], old_dist [k]) and its offers."""
    old_idx, old_dist = np.asarray(old_idx, np.int64), np.asarray(old_dist, np.float32)
    if np.isnan(old_dist[0]):                       # a non-finite row keeps its -1 / NaN list
        return old_idx.copy(), old_dist.copy()
    present = old_idx >= 0
    ci = np.concatenate([old_idx[present], np.asarray(offer_idx, np.int64)])
    cd = np.concatenate([old_dist[present], np.asarray(offer_dist, np.float32)])
    out_i, out_d = np.full(k, -1, np.int64), np.full(k, np.inf, np.float32)
    seen, m = set(), 0
    for t in np.lexsort((ci, cd)):
        if m == k:
            break
        if distinct:
            g = int(groups[ci[t]])
            if g in seen:
                continue
            seen.add(g)
        out_i[m], out_d[m] = ci[t], cd[t]
        m += 1
    return out_i, out_d


def merge_graph(idx, dist, indptr, offer_idx, offer_dist, k, groups=None, distinct=False):
    """``merge_lists`` over the rows of a graph and a CSR of offers."""
    out_i, out_d = np.array(idx, np.int64), np.array(dist, np.float32)
    for a in range(len(out_i)):
        lo, hi = int(indptr[a]), int(indptr[a + 1])
        out_i[a], out_d[a] = merge_lists(idx[a], dist[a], offer_idx[lo:hi], offer_dist[lo:hi], k, groups, distinct)
    return out_i, out_d


def brute_lists(q, b, k, self_offset=-1, query_groups=None, bank_groups=None, exclude=False, one=False):
    """knn_group_ref.exact_answer: the lists of integer rows."""
    return G.exact_answer(q, b, k, self_offset=self_offset, query_groups=query_groups, bank_groups=bank_groups,
                          exclude=exclude, one=one)


def _tau(rows, i, bb_max, metric):
    d = rows.shape[1]
    if metric == "euclidean":
        return 8 * (d + 2 if d >= 4 else d + 6) * U * (float((rows[i].astype(np.float64) ** 2).sum()) + bb_max)
    return 8 * (d + 2) * U


def separated_rows(rows, k, metric="euclidean", groups=None, exclude=False, one=False):
    """bool [N]: the rows of ``knn_graph(rows, k, include_self=False, ...)`` with no second candidate inside the
    selection band at the k-th place (non-finite rows count as separated: their list is fixed)."""
    rows = np.asarray(rows, np.float32)
    n = len(rows)
    g = None if groups is None else np.asarray(groups, np.int64)
    el = G.eligible_mask(rows, n, 0, g, g, exclude and g is not None)
    dm = R.dist64_matrix(rows, rows, metric)
    fin = R.finite_rows(rows)
    bb_max = float((rows[fin].astype(np.float64) ** 2).sum(1).max()) if fin.any() else 0.0
    out = np.ones(n, bool)
    for i in range(n):
        if not fin[i]:
            continue
        tau = _tau(rows, i, bb_max, metric)
        cols = np.flatnonzero(el[i])
        d = dm[i, cols]
        if one and g is not None:
            o = np.lexsort((d, g[cols]))
            gs, ds = g[cols][o], d[o]
            first = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]])
            gmin = ds[first]
            second = np.full(len(first), np.inf)
            has2 = np.r_[first[1:], len(ds)] - first > 1
            second[has2] = ds[first[has2] + 1]
            order = np.argsort(gmin, kind="stable")
            d = gmin[order]
            head = order[:k + 1]
            if (second[head] - gmin[head] <= 2 * tau).any():
                out[i] = False
                continue
        else:
            d = np.sort(d)
        if len(d) > k and d[k] - d[k - 1] <= 2 * tau:
            out[i] = False
    return out


def check_graph(rows, idx, dist, k, metric="euclidean", updates=0, groups=None, exclude=False, one=False):
    """The contract of a graph (every row of ``rows`` among the others) whose lists went through at most ``updates``
    merges: knn_ref / knn_group_ref clauses 1 and 2 as stated there, clause 3 with the bound of the module text.  Raises
    AssertionError naming the clause; returns the worst rank excess over the un-merged tau."""
    rows = np.asarray(rows, np.float32)
    idx, dist = np.asarray(idx), np.asarray(dist)
    n, d = rows.shape
    g = None if groups is None else np.asarray(groups, np.int64)
    exclude, one = exclude and g is not None, one and g is not None
    assert idx.shape == (n, k) and dist.shape == (n, k), "shape"
    assert idx.dtype == np.int64 and dist.dtype == np.float32, "dtype"
    el = G.eligible_mask(rows, n, 0, g, g, exclude)
    dm = R.dist64_matrix(rows, rows, metric)
    fin = R.finite_rows(rows)
    bb_max = float((rows[fin].astype(np.float64) ** 2).sum(1).max()) if fin.any() else 0.0
    e = (d + 4) * U
    worst = 0.0
    for i in range(n):
        if not fin[i]:
            assert (idx[i] == -1).all() and np.isnan(dist[i]).all(), f"validity: non-finite row {i}"
            continue
        cols = np.flatnonzero(el[i])
        if one:
            groups_i, gmin = G._group_minima(dm[i, cols], g[cols])
            m = min(k, len(groups_i))
        else:
            m = min(k, len(cols))
        assert (idx[i, m:] == -1).all() and np.isposinf(dist[i, m:]).all(), f"validity: tail of row {i}"
        got = idx[i, :m]
        assert ((got >= 0) & (got < n)).all(), f"validity: index out of range in row {i}"
        assert len(set(got.tolist())) == m, f"validity: repeated index in row {i}"
        assert el[i, got].all(), f"validity: ineligible row returned for row {i}"
        if one:
            assert len(set(g[got].tolist())) == m, f"validity: a group returned twice for row {i}"
        dd = dist[i, :m].astype(np.float64)
        assert np.isfinite(dd).all(), f"validity: non-finite distance in row {i}"
        assert ((dd[1:] > dd[:-1]) | ((dd[1:] == dd[:-1]) & (got[1:] > got[:-1]))).all(), \
            f"validity: row {i} not sorted by (dist, index)"
        if m == 0:
            continue
        r = R.direct64(rows[i], rows[got], metric)
        tau = _tau(rows, i, bb_max, metric)
        if metric == "euclidean":
            d64, bound = np.sqrt(r), (d + 4) * U * np.sqrt(r)
        else:
            d64, bound = r, np.full(m, 4 * (d + 2) * U)
        err = np.abs(dd - d64)
        assert (err <= bound).all(), f"distance: row {i} off by {err.max():.3e}"
        t = np.sort(gmin if one else dm[i, cols])[:m]

        def limit(base):
            if metric == "euclidean":
                return (base + tau) * ((1 + e) / (1 - e)) ** (2 * updates)
            return base + tau + 2 * updates * 4 * (d + 2) * U
        assert (r <= limit(t)).all(), (f"rank: row {i} exceeds t_j by {(r - t).max():.3e} = {(r - t).max() / tau:.2f} tau "
                                       f"after {updates} merges")
        if one:
            own = gmin[np.searchsorted(groups_i, g[got])]
            assert (r <= limit(own)).all(), f"rank: row {i} returns a row behind its own group's nearest"
        if tau > 0:
            worst = max(worst, float((r - t).max() / tau))
    return worst
