"""What the radius-search and DBSCAN tests share (no GPU): the contract of ``EmbeddingIndex.radius`` as a checker, the
choice of a radius a test may use, a numpy emulation of the candidate pass, the DBSCAN rule in numpy and the seeded sets.

The contract (include/btsbot_hip.h), with u = 2^-24, d64 the float64 distance from the fp32 inputs
(Euclidean: not squared; cosine: 1 - cos) and band = (D + 4) u relative (cosine: 4 (D + 2) u absolute), the bound of
the direct-form fp32 distance that decides membership:
  1 validity   indptr starts at 0 and does not decrease; a row's indices are eligible (finite bank row, not the excluded
               self, not of the query's group under exclude), distinct, and ordered as asked: by index, or by (dist,
               index); a non-finite query row has an empty list
  2 distance   |dist - d64| <= band
  3 must-in    every eligible pair with d64 (1 + band) <= r (cosine d64 + band <= r) is present
  4 must-out   every pair with d64 (1 - band) > r (cosine d64 - band > r) is absent
Pairs between 3 and 4 -- the free band -- may go either way.  A test's radius must leave at most 1 % of the pairs
within r there (``band_share``; ``pick_radius`` finds such an r from the float64 matrix alone).
"""
import numpy as np

from knn_ref import KINDS, TILE, U, _pack, direct64, dist64_matrix, eligible_mask, finite_rows, make_rows  # noqa: F401

# (Q, N, D, splits)
CASES = [(1, 1, 1, 1), (63, 7, 5, 2), (65, 127, 31, 1), (130, 128, 32, 7), (63, 129, 33, 2), (65, 1000, 528, 7),
         (130, 4099, 1024, 0)]


def band_of(d, metric):
    return (d + 4) * U if metric == "euclidean" else 4 * (d + 2) * U


def eligible(q, b, self_offset=-1, qgroups=None, bgroups=None):
    """bool [Q, N]: finite bank rows of finite query rows, without the masked self and the query's own group"""
    el = eligible_mask(b, q.shape[0], self_offset) & finite_rows(q)[:, None]
    if qgroups is not None:
        el &= np.asarray(qgroups)[:, None] != np.asarray(bgroups)[None, :]
    return el


def d64_matrix(q, b, metric, r=None):
    """float64 [Q, N] distances (Euclidean: the root of the expansion form, whose float64 error is far below the band;
    with ``r`` the pairs within 1e-3 of the boundary are redone in the direct form)."""
    dm = dist64_matrix(q, b, metric)
    if metric != "euclidean":
        return dm
    d = np.sqrt(dm)
    if r is not None:
        rr = np.broadcast_to(np.asarray(r, np.float64), (q.shape[0],))
        fin = finite_rows(b)
        for i in range(q.shape[0]):
            near = fin & (np.abs(d[i] - rr[i]) <= 1e-3 * rr[i] + 1e-300)
            if near.any() and finite_rows(q[i:i + 1])[0]:
                d[i, near] = np.sqrt(direct64(q[i], b[near], metric))
    return d


def split_by_band(d, r, dim, metric):
    """(must_in, must_out) bool [Q, N] for radii r (scalar or [Q])"""
    band = band_of(dim, metric)
    rr = np.broadcast_to(np.asarray(r, np.float64), (d.shape[0],))[:, None]
    if metric == "euclidean":
        return d * (1 + band) <= rr, d * (1 - band) > rr
    return d + band <= rr, d - band > rr


def band_share(d, el, r, dim, metric):
    """the pairs of the free band as a fraction of the eligible pairs within r (0 if there are none)"""
    must_in, must_out = split_by_band(d, r, dim, metric)
    free = el & ~must_in & ~must_out
    within = el & (d <= np.broadcast_to(np.asarray(r, np.float64), (d.shape[0],))[:, None])
    return free.sum() / max(1, within.sum())


def pick_radius(d, el, dim, metric, fractions=(0.05, 0.3, 0.6)):
    """An fp32 radius (as a Python float) from the float64 matrix alone: the middle of the widest gap between
    neighbouring distances near a quantile, the first of ``fractions`` that leaves at most 1 % of the pairs within r in
    the free band; if none does (distances all inside one band width: cosine of rows far from the origin), a radius
    beyond every pair."""
    vals = np.unique(d[el])
    if len(vals) == 0:
        return 1.0
    for f in fractions:
        at = int(f * (len(vals) - 1))
        lo, hi = max(0, at - 32), min(len(vals) - 1, at + 32)
        if hi == lo:
            continue
        g = int(np.argmax(np.diff(vals[lo:hi + 1]))) + lo
        r = float(np.float32(0.5 * (vals[g] + vals[g + 1])))
        if band_share(d, el, r, dim, metric) <= 0.01:
            return r
    return float(np.float32(2.0 * vals[-1] + 8 * band_of(dim, metric) + 1e-30))


def check_radius(q, b, r, indptr, indices, dist, metric="euclidean", sort="index", self_offset=-1, qgroups=None,
                 bgroups=None):
    """Clauses 1-4; AssertionError naming the clause.  Returns (worst distance error / band, pairs in the free band,
    pairs of the free band that were returned)."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    indptr, indices, dist = np.asarray(indptr), np.asarray(indices), np.asarray(dist)
    n_q, dim = q.shape
    n = b.shape[0]
    assert indptr.dtype == np.int64 and indices.dtype == np.int64 and dist.dtype == np.float32, "dtype"
    assert indptr.shape == (n_q + 1,) and indptr[0] == 0 and (np.diff(indptr) >= 0).all(), "validity: indptr"
    assert indices.shape == dist.shape == (indptr[-1],), "validity: lengths"
    el = eligible(q, b, self_offset, qgroups, bgroups)
    d = d64_matrix(q, b, metric, r) if n else np.zeros((n_q, 0))
    must_in, must_out = split_by_band(d, r, dim, metric)
    band = band_of(dim, metric)
    worst = 0.0
    n_free = int((el & ~must_in & ~must_out).sum())
    free_taken = 0
    for i in range(n_q):
        got, dd = indices[indptr[i]:indptr[i + 1]], dist[indptr[i]:indptr[i + 1]].astype(np.float64)
        assert ((got >= 0) & (got < n)).all(), f"validity: index out of range in row {i}"
        assert len(set(got.tolist())) == len(got), f"validity: repeated index in row {i}"
        assert el[i, got].all(), f"validity: ineligible row returned for query {i}"
        if sort == "index":
            assert (np.diff(got) > 0).all(), f"validity: row {i} not ordered by index"
        else:
            ok = (dd[1:] > dd[:-1]) | ((dd[1:] == dd[:-1]) & (got[1:] > got[:-1]))
            assert ok.all(), f"validity: row {i} not ordered by (dist, index)"
        taken = np.zeros(n, bool)
        taken[got] = True
        miss = el[i] & must_in[i] & ~taken
        assert not miss.any(), f"must-in: row {i} lacks {np.flatnonzero(miss)[:5].tolist()}"
        extra = taken & must_out[i]
        assert not extra.any(), f"must-out: row {i} holds {np.flatnonzero(extra)[:5].tolist()}"
        free_taken += int((taken & ~must_in[i] & ~must_out[i]).sum())
        if len(got):
            r64 = direct64(q[i], b[got], metric)
            d64 = np.sqrt(r64) if metric == "euclidean" else r64
            bound = band * d64 if metric == "euclidean" else np.full(len(got), band)
            err = np.abs(dd - d64)
            assert (err <= bound).all(), f"distance: row {i} off by {err.max():.3e}"
            nz = bound > 0
            if nz.any():
                worst = max(worst, float((err[nz] / bound[nz]).max()))
    return worst, n_free, free_taken


def radius_lists(q, b, r, metric="euclidean", sort="index", **kw):
    """The float64 restatement itself: (indptr, indices, dist) of the pairs with d64 <= r"""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    el = eligible(q, b, kw.get("self_offset", -1), kw.get("qgroups"), kw.get("bgroups"))
    d = d64_matrix(q, b, metric, r)
    rr = np.broadcast_to(np.asarray(r, np.float64), (q.shape[0],))
    indptr, idx, dist = [0], [], []
    for i in range(q.shape[0]):
        got = np.flatnonzero(el[i] & (d[i] <= rr[i]))
        if sort == "distance":
            got = got[np.lexsort((got, d[i, got]))]
        idx.append(got)
        dist.append(d[i, got])
        indptr.append(indptr[-1] + len(got))
    cat = (lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t))
    return np.asarray(indptr, np.int64), cat(idx, np.int64), cat(dist, np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the candidate pass in numpy: split f16 operands, fp32 arithmetic, the margin of DESIGN.md 4p
def emulate_candidates(q, b, r, metric="euclidean"):
    """(admitted bool [Q, N], g fp32 [Q, N] the GEMM-form value, margin fp32 [Q, N] = limit - r^2 (cosine: - r)) as
    knn_radius_kernel forms them, up to the summation order inside a product."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    dim = q.shape[1]
    f = np.float32
    cosine = metric == "cosine"
    qh, ql, qq, qs, qok, _ = _pack(q, False)
    bh, bl, bias, bscale, bok, _ = _pack(b, cosine)
    qscale = (2 * qs).astype(f)
    acc = (ql.astype(f) @ bh.astype(f).T + qh.astype(f) @ bl.astype(f).T) + qh.astype(f) @ bh.astype(f).T
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = (bias[None, :] - (acc * qscale[:, None]) * bscale[None, :]).astype(f)
        rr = np.broadcast_to(np.asarray(r, f), (q.shape[0],))
        qq = np.where(qok, qq, f(0)).astype(f)
        if cosine:
            qinv = np.where(qok & (qq > 0), f(0.5) / np.sqrt(np.where(qq > 0, qq, f(1)), dtype=f), f(0)).astype(f)
            ctau = f(16 * (dim + 8) * U)
            g = (s * qinv[:, None] + f(1)).astype(f)
            lim = np.broadcast_to((rr + ctau).astype(f)[:, None], g.shape)
            margin = np.full(g.shape, ctau, f)
        else:
            rel, ctau = f(1 + 4 * (dim + 4) * U), f(8 * (dim + 8) * U)
            g = (s + qq[:, None]).astype(f)
            r2 = ((rr * rr).astype(f) * rel).astype(f)
            lim = (ctau * (qq[:, None] + bias[None, :]).astype(f) + r2[:, None]).astype(f)
            margin = (lim - (rr.astype(np.float64) ** 2)[:, None]).astype(f)
        lim = np.where((qok & (rr >= 0))[:, None], lim, f(-np.inf))
        adm = (g <= lim) & (s < np.inf)
    return adm, g, margin


# ---------------------------------------------------------------------------------------------------------------------
# DBSCAN: sklearn's rule, independent of the visiting order
def dbscan_ref(X, eps, min_samples, groups=None, metric="euclidean"):
    """(labels int64 [N], core bool [N]): a row counts itself; core = count >= min_samples (with groups: the number of
    distinct groups within eps); clusters = components of the core-core edges, numbered by their smallest core row; a
    non-core row takes the smallest label among its core neighbours, else -1.  Non-finite rows have no neighbours."""
    X = np.asarray(X, np.float32)
    n = X.shape[0]
    eps = float(np.float32(eps))
    fin = finite_rows(X)
    within = np.zeros((n, n), bool)
    for i in np.flatnonzero(fin):
        d = direct64(X[i], X[fin], metric)
        within[i, np.flatnonzero(fin)] = (np.sqrt(d) if metric == "euclidean" else d) <= eps
    if groups is None:
        count = within.sum(1)
    else:
        g = np.asarray(groups)
        count = np.array([len(set(g[within[i]].tolist())) for i in range(n)])
    core = count >= min_samples
    labels = np.full(n, -1, np.int64)
    nxt = 0
    for i in range(n):
        if not core[i] or labels[i] >= 0:
            continue
        labels[i] = nxt
        stack = [i]
        while stack:
            u = stack.pop()
            for v in np.flatnonzero((within[u] | within[:, u]) & core & (labels < 0)):
                labels[v] = nxt
                stack.append(int(v))
        nxt += 1
    for i in np.flatnonzero(~core):
        nb = labels[within[i] & core]
        if len(nb):
            labels[i] = nb.min()
    return labels, core


def pairs_in_band(X, eps, metric="euclidean", times=1.0):
    """how many pairs of rows lie within ``times`` band widths of eps (the sets of the DBSCAN tests must have none)"""
    X = np.asarray(X, np.float32)
    eps = float(np.float32(eps))
    d = d64_matrix(X, X, metric, eps)
    band = band_of(X.shape[1], metric) * times
    near = np.abs(d - eps) <= (band * d if metric == "euclidean" else band)
    return int(np.triu(near & finite_rows(X)[:, None] & finite_rows(X)[None, :], 1).sum())


def blobs_2d(seed, n=360):
    """three blobs and a uniform background in the plane"""
    rng = np.random.default_rng(seed)
    per = n // 4
    centres = np.array([[0.0, 0.0], [4.0, 1.0], [1.5, 4.5]])
    pts = [c + rng.normal(0, 0.45, size=(per, 2)) for c in centres]
    pts.append(rng.uniform(-2.5, 7.0, size=(n - 3 * per, 2)))
    x = np.concatenate(pts)
    return x[rng.permutation(n)].astype(np.float32)


def clusters_32d(seed, n=512):
    """ten clusters in 32 dimensions"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 3.0, size=(10, 32))
    x = centres[np.arange(n) % 10] + rng.normal(0, 0.95, size=(n, 32))
    return x[rng.permutation(n)].astype(np.float32)


def border_set():
    """(X, eps, min_samples, border row): two clusters on a line and one non-core row within eps of a core row of
    each; the cluster that comes first in the rows is label 0, and the border row takes it"""
    xs = [2.0 + 0.1 * j for j in range(5)] + [1.2] + [0.1 * j for j in range(5)]
    return np.array([[x, 0.0] for x in xs], np.float32), 0.85, 4, 5


# (set, eps, min_samples) of the host and the device DBSCAN tests
def dbscan_sets():
    return [("blobs a", blobs_2d(11), 0.3, 5), ("blobs b", blobs_2d(12), 0.45, 8),
            ("32-D a", clusters_32d(13), 7.0, 5), ("32-D b", clusters_32d(14), 6.5, 10)]
