"""What the IvfIndex / k-means tests share (numpy, no GPU): the contract of btsbot_amd/ivf.py as
checkers, and float64 restatements of Lloyd's iteration and of the whole probed query.

The query.  With allowed(q) = the finite bank rows whose label is in probes(q), minus self_rows[q]:
  (A) clauses 1-3 of knn_ref hold with "eligible" read as allowed(q), for the same u, distance bound and tau
      (``check_allowed``); fewer than k allowed rows: tail -1 / +inf; a non-finite query row: -1 / NaN
  (B) clause 4: on integer rows in [-8, 8] idx is the stable float64 argsort of the squared distances over allowed(q), ties
      by original row number, and dist is exact (``check_exact_allowed``)
tau keeps knn_ref's form, 8 (D + 2) u (|q|^2 + max_b |b|^2) with the maximum over the WHOLE bank: the selection scores are
those of the exact search, whatever list a row lies in.

The centroid update (K1).  btsbot_kmeans_update sums a cluster's n rows, in ascending row order, in this shape: chunks of
C = 64 rows counted from the cluster's first row; a chunk's rows are added one after the other (at most C - 1 additions
touch a term); the cluster's m = ceil(n / C) chunk sums are added one after the other (at most m - 1 more); the sum is
divided by float(n) (one rounding for the quotient, one for n > 2^24).  Every term passes through at most
a = min(n, C) - 1 + m - 1 additions, so by the standard bound for any summation order of depth a
    |fl(sum) - sum| <= gamma_a * sum |x_i|,    gamma_a = a u / (1 - a u),   u = 2^-24
and with the two roundings of the division
    |centroid - mean| <= gamma_{a + 2} * (sum |x_i|) / n
per element (``mean_bound``).  The float64 mean it is compared with carries n 2^-53 of the same magnitude, which is added.
"""
import numpy as np

from knn_ref import U, dist64_matrix, direct64, finite_rows

CHUNK = 64   # csrc/ivf.hip: KM_CHUNK


def usable_rows(x):
    """bool [n]: finite rows whose squared norm is finite in fp32 (the rows the packer keeps)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return finite_rows(x) & np.isfinite((x * x).sum(1, dtype=np.float32))


def allowed_mask(b, labels, probes, self_rows=None):
    """bool [Q, N]: bank row n is allowed for query q."""
    b, labels, probes = np.asarray(b, np.float32), np.asarray(labels), np.asarray(probes)
    n_q, n = probes.shape[0], b.shape[0]
    ok = usable_rows(b) & (labels >= 0)
    al = np.zeros((n_q, n), bool)
    for i in range(n_q):
        al[i] = ok & np.isin(labels, probes[i][probes[i] >= 0])
    if self_rows is not None:
        s = np.asarray(self_rows)
        rows = np.arange(n_q)
        inside = (s >= 0) & (s < n)
        al[rows[inside], s[inside]] = False
    return al


def check_allowed(q, b, idx, dist, k, allowed):
    """Clauses 1-3 under the [Q, N] mask ``allowed``; raises AssertionError naming the clause.  Returns the worst
    (distance error / bound, rank excess / tau)."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    idx, dist, el = np.asarray(idx), np.asarray(dist), np.asarray(allowed, bool)
    n_q, d = q.shape
    n = b.shape[0]
    assert idx.shape == (n_q, k) and dist.shape == (n_q, k), "shape"
    assert idx.dtype == np.int64 and dist.dtype == np.float32, "dtype"
    assert el.shape == (n_q, n), "mask shape"
    dm = dist64_matrix(q, b, "euclidean") if n else np.zeros((n_q, 0))
    qfin = usable_rows(q)
    bfin = usable_rows(b)
    bb_max = float((b[bfin].astype(np.float64) ** 2).sum(1).max()) if bfin.any() else 0.0
    worst_d = worst_r = 0.0
    for i in range(n_q):
        if not qfin[i]:
            assert (idx[i] == -1).all() and np.isnan(dist[i]).all(), f"validity: non-finite query row {i}"
            continue
        m = min(k, int(el[i].sum()))
        assert (idx[i, m:] == -1).all() and np.isposinf(dist[i, m:]).all(), f"validity: tail of row {i}"
        got = idx[i, :m]
        assert ((got >= 0) & (got < n)).all(), f"validity: index out of range in row {i}"
        assert len(set(got.tolist())) == m, f"validity: repeated index in row {i}"
        assert el[i, got].all(), f"validity: a row outside the allowed set returned for query {i}"
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
        t = np.sort(dm[i][el[i]])[:m]
        excess = r - t
        assert (excess <= tau).all(), f"rank: row {i} exceeds t_j by {excess.max():.3e} = {excess.max() / tau:.2f} tau"
        nz = bound > 0
        if nz.any():
            worst_d = max(worst_d, float((err[nz] / bound[nz]).max()))
        if tau > 0:
            worst_r = max(worst_r, float(excess.max() / tau))
    return worst_d, worst_r


def check_exact_allowed(q, b, idx, dist, k, allowed):
    """Clause 4 under the mask (integer rows in [-8, 8])."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    idx, dist, el = np.asarray(idx), np.asarray(dist), np.asarray(allowed, bool)
    d2 = dist64_matrix(q, b, "euclidean")
    assert (d2 == np.round(d2)).all()
    for i in range(q.shape[0]):
        row = np.where(el[i], d2[i], np.inf)
        order = np.argsort(row, kind="stable")
        m = min(k, int(el[i].sum()))
        want_i = np.full(k, -1, np.int64)
        want_d = np.full(k, np.inf, np.float32)
        want_i[:m] = order[:m]
        want_d[:m] = np.sqrt(row[order[:m]]).astype(np.float32)
        assert (idx[i] == want_i).all(), f"exact: indices of row {i}: {idx[i].tolist()} != {want_i.tolist()}"
        assert (dist[i] == want_d).all(), f"exact: distances of row {i}"


# ---------------------------------------------------------------------------------------------------------------------
# k-means in float64
def assign64(rows, centroids):
    """int64 [N]: every row's nearest centroid by the float64 direct-form distance, ties to the lower centroid; -1 for
    a row that is not usable."""
    rows, c = np.asarray(rows, np.float32), np.asarray(centroids, np.float64)
    ok = usable_rows(rows)
    x = np.where(ok[:, None], rows, np.float32(0)).astype(np.float64)
    d2 = ((x[:, None, :] - c[None, :, :]) ** 2).sum(2) if x.shape[1] * x.shape[0] * c.shape[0] <= 1 << 24 else \
        np.stack([((x - c[j]) ** 2).sum(1) for j in range(c.shape[0])], axis=1)
    return np.where(ok, np.argmin(d2, axis=1), -1).astype(np.int64)


def means64(rows, labels, n_clusters, prev):
    """float64 [n_clusters, D]: every cluster's mean; an empty cluster keeps ``prev``'s row."""
    rows, labels = np.asarray(rows, np.float32).astype(np.float64), np.asarray(labels)
    out = np.array(prev, np.float64, copy=True)
    for c in range(n_clusters):
        m = labels == c
        if m.any():
            out[c] = rows[m].sum(0) / int(m.sum())
    return out


def lloyd(rows, init, n_iter):
    """The float64 restatement of ``kmeans``: n_iter times (assign, update), then one more assignment.  Returns
    (centroids float64 after every iteration [n_iter + 1, n_clusters, D] with the initial ones first, the labels each
    update used [n_iter, N], the final labels [N])."""
    c = np.asarray(init, np.float64)
    cs, ls = [c], []
    for _ in range(n_iter):
        lab = assign64(rows, c)
        c = means64(rows, lab, c.shape[0], c)
        ls.append(lab)
        cs.append(c)
    return np.stack(cs), np.stack(ls) if ls else np.zeros((0, len(rows)), np.int64), assign64(rows, c)


def mean_bound(rows, labels, n_clusters, chunk=CHUNK):
    """float64 [n_clusters, D]: the per-element bound of the module text (0 for an empty cluster)."""
    rows, labels = np.asarray(rows, np.float32).astype(np.float64), np.asarray(labels)
    out = np.zeros((n_clusters, rows.shape[1]))
    for c in range(n_clusters):
        m = labels == c
        n = int(m.sum())
        if n == 0:
            continue
        a = min(n, chunk) - 1 + (n + chunk - 1) // chunk - 1 + 2
        gamma = a * U / (1 - a * U)
        out[c] = (gamma + n * 2.0 ** -53) * np.abs(rows[m]).sum(0) / n
    return out


def check_centroids(got, rows, labels, n_clusters, prev):
    """(K1): every centroid within ``mean_bound`` of the float64 mean, an empty cluster's row equal to ``prev``'s."""
    got = np.asarray(got, np.float64)
    labels = np.asarray(labels)
    want = means64(rows, labels, n_clusters, prev)
    bound = mean_bound(rows, labels, n_clusters)
    for c in range(n_clusters):
        if not (labels == c).any():
            assert (got[c] == np.asarray(prev, np.float64)[c]).all(), f"centroid {c}: an empty cluster's row was touched"
            continue
        err = np.abs(got[c] - want[c])
        assert (err <= bound[c]).all(), (f"centroid {c}: off by {err.max():.3e}, "
                                         f"{(err / np.where(bound[c] > 0, bound[c], 1)).max():.2f} of the bound")


def check_lists(labels, n_lists, indptr, rows):
    """The lists as a CSR hold, for every list, exactly the rows of that label in ascending row number."""
    labels, indptr, rows = np.asarray(labels), np.asarray(indptr), np.asarray(rows)
    assert indptr.shape == (n_lists + 1,) and indptr[0] == 0 and indptr[-1] == len(rows), "lists: indptr"
    for l in range(n_lists):
        want = np.nonzero(labels == l)[0]
        got = rows[indptr[l]:indptr[l + 1]]
        assert got.shape == want.shape and (got == want).all(), f"lists: list {l} holds {got.tolist()[:8]}.. not its rows"


# ---------------------------------------------------------------------------------------------------------------------
# the query in float64
def probes64(q, centroids, nprobe):
    """int64 [Q, nprobe]: the nprobe nearest centroids by the float64 direct-form distance, ties to the lower centroid;
    -1 throughout for a query row that is not usable."""
    q, c = np.asarray(q, np.float32), np.asarray(centroids, np.float32)
    ok = usable_rows(q)
    out = np.full((q.shape[0], nprobe), -1, np.int64)
    for i in np.nonzero(ok)[0]:
        out[i] = np.argsort(direct64(q[i], c, "euclidean"), kind="stable")[:nprobe]
    return out


def query64(q, b, centroids, k, nprobe, self_rows=None, labels=None):
    """The whole query restated in float64: labels (unless given) and probes from float64 distances to the centroids, then
    the k nearest allowed rows by the float64 direct-form distance, ties by row number.  (idx int64 [Q, k], dist fp32)."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    if labels is None:
        labels = assign64(b, centroids)
    pr = probes64(q, centroids, nprobe)
    al = allowed_mask(b, labels, pr, self_rows)
    idx = np.full((q.shape[0], k), -1, np.int64)
    dist = np.full((q.shape[0], k), np.inf, np.float32)
    ok = usable_rows(q)
    for i in range(q.shape[0]):
        if not ok[i]:
            dist[i] = np.nan
            continue
        rows = np.nonzero(al[i])[0]
        d2 = direct64(q[i], b[rows], "euclidean")
        o = np.argsort(d2, kind="stable")[:k]
        idx[i, :len(o)] = rows[o]
        dist[i, :len(o)] = np.sqrt(d2[o]).astype(np.float32)
    return idx, dist


def brute64(q, b, k):
    """int64 [Q, k]: the exact k nearest usable bank rows in float64 (direct form), ties by row number."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    rows = np.nonzero(usable_rows(b))[0]
    out = np.full((q.shape[0], k), -1, np.int64)
    for i in range(q.shape[0]):
        o = np.argsort(direct64(q[i], b[rows], "euclidean"), kind="stable")[:k]
        out[i, :len(o)] = rows[o]
    return out


def recall(idx, truth):
    """The fraction of ``truth``'s valid entries found in the same row of ``idx``."""
    idx, truth = np.asarray(idx), np.asarray(truth)
    hit = total = 0
    for a, t in zip(idx, truth):
        t = t[t >= 0]
        hit += len(np.intersect1d(a[a >= 0], t))
        total += len(t)
    return hit / max(total, 1)


def blobs(n, n_queries, seed, dim=32, n_blobs=10, spread=1.0):
    """The 32-D ten-cluster set: integer centres in [-6, 6], N(0, spread) around them; (bank fp32 [n, dim], queries)."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(-6, 7, size=(n_blobs, dim)).astype(np.float64)
    bank = centres[np.arange(n) % n_blobs] + spread * rng.standard_normal((n, dim))
    queries = centres[rng.integers(0, n_blobs, n_queries)] + spread * rng.standard_normal((n_queries, dim))
    return bank.astype(np.float32), queries.astype(np.float32)


def laid_out(kind_rows, lists, n_lists, step, base=0.0, sigma=1.0):
    """``kind_rows`` [n, d] with row i's first coordinate moved next to centroid ``lists[i]`` of ``axis_centroids``: the
    centroids stand ``step`` apart along the first axis, centred on ``base``, and the coordinate keeps its own deviation
    from ``base`` (of standard deviation ``sigma``) scaled to step / 16, so it strays less than step / 2 and the row's
    nearest centroid is ``lists[i]`` by a margin of about step^2 / 3.  The other coordinates are the kind's, and the
    norms -- hence the contract's tau -- stay near the kind's own."""
    out = np.array(kind_rows, np.float32, copy=True)
    dev = (out[:, 0].astype(np.float64) - base) / sigma
    out[:, 0] = (base + step * (np.asarray(lists) - (n_lists - 1) / 2) + np.clip(dev, -6, 6) * step / 16).astype(np.float32)
    return out


def axis_centroids(n_lists, d, step, base=0.0):
    c = np.full((n_lists, d), base, np.float64)
    c[:, 0] = base + step * (np.arange(n_lists) - (n_lists - 1) / 2)
    return c.astype(np.float32)
