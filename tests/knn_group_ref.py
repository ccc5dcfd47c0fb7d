"""What the grouped embedding-neighbour tests share (no GPU): group patterns, the covering cases, ``check_group_neighbors``
and ``check_group_exact`` -- the contract of btsbot_knn_query_grouped (include/btsbot_hip.h) -- and a
numpy emulation of the grouped two-pass scheme.  Everything builds on knn_ref, which stays as it is.

A group is an int64 per row.  The contract, with knn_ref's u, tau and distance bound:
  1 validity   knn_ref's clause 1, a row being eligible if it is finite, not the excluded self and, under
               exclude_same_group, of another group than the query row; under one_per_group the returned rows' groups are
               pairwise distinct; m = min(k, number of eligible rows -- under one_per_group: of eligible groups)
  2 distance   unchanged
  3 rank       t_j = j-th smallest eligible float64 squared distance -- under one_per_group: j-th smallest per-group
               minimum --, r_j <= t_j + tau; under one_per_group every returned row is also within tau of its own group's
               minimum
  4 exact      integer rows in [-8, 8]: the stable float64 argsort over the eligible rows -- under one_per_group after
               keeping, per group, the lowest index at the group's minimum distance --, ties included
"""
import numpy as np

import knn_ref as R

U, TILE = R.U, R.TILE
MAX_K_ONE = 32   # k's cap under one_per_group (csrc/knn_tile.h, MAX_K_ONE)
MODES = {"exclude": (True, False), "distinct": (False, True), "exclude+distinct": (True, True)}   # (exclude, one)
PATTERNS = ("runs", "mod3", "mod40", "one", "distinct", "runs_hi32", "mod40_hi32", "negative")

# (Q, N, D, k, splits, pattern): a covering subset of Q {1, 65, 130} x N {7, 129, 1000, 4099} x D {5, 33, 528} x
# k {1, 15, 32} x splits {1, 2, 7, 0} x the patterns
CASES = [
    (1, 7, 5, 1, 1, "runs"),
    (65, 129, 33, 15, 2, "mod3"),
    (130, 1000, 528, 15, 7, "runs"),
    (65, 4099, 5, 32, 0, "mod40"),
    (130, 4099, 33, 32, 7, "runs_hi32"),
    (65, 1000, 33, 15, 2, "one"),
    (130, 129, 5, 32, 1, "distinct"),
    (1, 4099, 528, 15, 7, "negative"),
    (65, 1000, 5, 1, 0, "mod40_hi32"),
]


def case_id(c):
    return "Q{}-N{}-D{}-k{}-s{}-{}".format(*c)


def make_groups(pattern, n, seed=0):
    """int64 [n].  runs: 1-9 consecutive rows per group (they straddle bank tiles and split edges); modG: arange % G
    (every group in every tile, more same-group candidates than a bucket round holds); one: a single group; distinct:
    every row its own; *_hi32: ids g + (j << 32), so that different groups agree in their low 32 bits; negative: negative
    ids, again with pairs equal in their low 32 bits."""
    rng = np.random.default_rng(5000 + seed)
    rows = np.arange(n, dtype=np.int64)
    if pattern.startswith("runs") or pattern == "negative":
        lens = rng.integers(1, 10, size=n + 1)
        run = np.repeat(np.arange(n + 1, dtype=np.int64), lens)[:n]
        if pattern == "runs":
            return run * 7 - 3
        if pattern == "runs_hi32":
            return (run % 5) + ((run // 5) << 32)
        return (run % 3) - ((run // 3 + 1) << 32)
    if pattern == "mod3":
        return rows % 3
    if pattern == "mod40":
        return rows % 40 - 20
    if pattern == "mod40_hi32":
        return (rows % 40 % 4) + ((rows % 40 // 4) << 32)
    if pattern == "one":
        return np.full(n, 7, np.int64)
    if pattern == "distinct":
        return rows * 3 - n
    raise ValueError(pattern)


def case_inputs(case, kind, seed=0):
    """(q, b, query_groups, bank_groups): knn_ref's rows; every query row takes the group of some bank row, so that an
    exclusion always removes something."""
    q_n, n, _d, _k, _s, pattern = case
    q, b = R.case_inputs(case[:5], kind, seed)
    bg = make_groups(pattern, n, seed)
    qg = bg[np.random.default_rng(6000 + seed).integers(0, n, size=q_n)]
    return q, b, qg, bg


def eligible_mask(b, n_query, self_offset=-1, query_groups=None, bank_groups=None, exclude=False):
    """bool [Q, N]"""
    el = R.eligible_mask(b, n_query, self_offset)
    if exclude:
        el &= np.asarray(bank_groups)[None, :] != np.asarray(query_groups)[:, None]
    return el


def _group_minima(d, g):
    """(the groups present, the smallest of d per group) for 1-D d and g of one length"""
    if len(d) == 0:
        return np.zeros(0, np.int64), np.zeros(0)
    o = np.lexsort((d, g))
    gs = g[o]
    first = np.r_[True, gs[1:] != gs[:-1]]
    return gs[first], d[o][first]


def check_group_neighbors(q, b, idx, dist, k, metric="euclidean", self_offset=-1, query_groups=None, bank_groups=None,
                          exclude=False, one=False):
    """Clauses 1-3; raises AssertionError naming the clause.  Returns the worst (distance error / bound, rank excess /
    tau)."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    idx, dist = np.asarray(idx), np.asarray(dist)
    n_q, d = q.shape
    n = b.shape[0]
    bg = None if bank_groups is None else np.asarray(bank_groups, np.int64)
    assert idx.shape == (n_q, k) and dist.shape == (n_q, k), "shape"
    assert idx.dtype == np.int64 and dist.dtype == np.float32, "dtype"
    el = eligible_mask(b, n_q, self_offset, query_groups, bg, exclude)
    dm = R.dist64_matrix(q, b, metric) if n else np.zeros((n_q, 0))
    qfin = R.finite_rows(q)
    bfin = R.finite_rows(b)
    bb_max = float(((b[bfin].astype(np.float64)) ** 2).sum(1).max()) if bfin.any() else 0.0
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
        r = R.direct64(q[i], b[got], metric)
        if metric == "euclidean":
            d64 = np.sqrt(r)
            bound = (d + 4) * U * d64
            tau = 8 * (d + 2 if d >= 4 else d + 6) * U * (float((q[i].astype(np.float64) ** 2).sum()) + bb_max)
        else:
            d64 = r
            bound = np.full(m, 4 * (d + 2) * U)
            tau = 8 * (d + 2) * U
        err = np.abs(dd - d64)
        assert (err <= bound).all(), (f"distance: row {i} off by {err.max():.3e} "
                                      f"({(err / np.where(bound > 0, bound, 1)).max():.2f} of the bound)")
        t = np.sort(gmin if one else dm[i, cols])[:m]
        excess = r - t
        assert (excess <= tau).all(), f"rank: row {i} exceeds t_j by {excess.max():.3e} = {excess.max() / tau:.2f} tau"
        if one:
            own = gmin[np.searchsorted(groups_i, bg[got])]
            over = r - own
            assert (over <= tau).all(), (f"rank: row {i} returns a row {over.max():.3e} = {over.max() / tau:.2f} tau "
                                         f"behind its own group's nearest")
        nz = bound > 0
        if nz.any():
            worst_d = max(worst_d, float((err[nz] / bound[nz]).max()))
        if tau > 0:
            worst_r = max(worst_r, float(excess.max() / tau))
    return worst_d, worst_r


def exact_answer(q, b, k, self_offset=-1, query_groups=None, bank_groups=None, exclude=False, one=False):
    """Clause 4's (idx, dist) on integer rows."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    el = eligible_mask(b, q.shape[0], self_offset, query_groups, bank_groups, exclude)
    d2 = R.dist64_matrix(q, b, "euclidean")
    assert (d2 == np.round(d2)).all()
    want_i = np.full((q.shape[0], k), -1, np.int64)
    want_d = np.full((q.shape[0], k), np.inf, np.float32)
    for i in range(q.shape[0]):
        cols = np.flatnonzero(el[i])
        if one and len(cols):
            g = np.asarray(bank_groups, np.int64)[cols]
            o = np.lexsort((cols, d2[i, cols], g))          # by group, then distance, then index
            cols = np.sort(cols[o][np.r_[True, g[o][1:] != g[o][:-1]]])
        order = cols[np.argsort(d2[i, cols], kind="stable")][:k]
        want_i[i, :len(order)] = order
        want_d[i, :len(order)] = np.sqrt(d2[i, order]).astype(np.float32)
    return want_i, want_d


def check_group_exact(q, b, idx, dist, k, **kw):
    want_i, want_d = exact_answer(q, b, k, **kw)
    idx, dist = np.asarray(idx), np.asarray(dist)
    for i in range(len(want_i)):
        assert (idx[i] == want_i[i]).all(), f"exact: indices of row {i}: {idx[i].tolist()} != {want_i[i].tolist()}"
        assert (dist[i] == want_d[i]).all(), f"exact: distances of row {i}"


# ---------------------------------------------------------------------------------------------------------------------
# the grouped two-pass scheme in numpy (knn_ref.emulate's arithmetic, "split" form)
def _best_per_group(c, s, g):
    """Of the candidates c (scores s, groups g) the best of every group by (score, index), in (score, index) order."""
    o = np.lexsort((c, s))
    _, first = np.unique(g[o], return_index=True)
    return o[np.sort(first)]


def emulate(q, b, k, metric="euclidean", splits=1, self_offset=-1, query_groups=None, bank_groups=None, exclude=False,
            one=False, low32=False, no_merge_collapse=False, first_offered=False, skip_exclude_tile=None):
    """(idx int64 [Q, k], dist fp32 [Q, k]) as the grouped kernels compute them, up to the summation order inside a
    product.  Seeded faults for the tests of the checkers: low32 compares groups on their low 32 bits; no_merge_collapse
    lets the merge keep two rows of one group that come from different splits; first_offered makes a group's
    representative the first row of the group a list was offered (the lowest index), not the best; skip_exclude_tile
    leaves the exclusion out for one bank tile."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    n_q, n = q.shape[0], b.shape[0]
    cosine = metric == "cosine"
    f = np.float32
    qh, ql, _, qs, qok, qz = R._pack(q, False)
    qscale = (2 * qs).astype(f)
    bh, bl, bias, bscale, _bok, bz = R._pack(b, cosine)
    acc = (ql.astype(f) @ bh.astype(f).T + qh.astype(f) @ bl.astype(f).T) + qh.astype(f) @ bh.astype(f).T
    with np.errstate(invalid="ignore", over="ignore"):
        score = (bias[None, :] - (acc * qscale[:, None]) * bscale[None, :]).astype(f)
    keep = score < np.inf
    if self_offset >= 0:
        rows = np.arange(n_q)
        cols = rows + self_offset
        ok = cols < n
        keep[rows[ok], cols[ok]] = False
    bg = None if bank_groups is None else np.asarray(bank_groups, np.int64)
    qg = None if query_groups is None else np.asarray(query_groups, np.int64)
    if low32:
        bg = bg & 0xffffffff
        qg = None if qg is None else qg & 0xffffffff
    if exclude:
        same = bg[None, :] == qg[:, None]
        if skip_exclude_tile is not None:
            same[:, skip_exclude_tile * TILE:(skip_exclude_tile + 1) * TILE] = False
        keep &= ~same
    tiles = (n + TILE - 1) // TILE
    if splits == 0:
        splits = max(1, min(32, tiles, -(-512 // max(1, -(-n_q // TILE)))))
    tps = -(-tiles // splits) if tiles else 0
    idx = np.full((n_q, k), -1, np.int64)
    dist = np.full((n_q, k), np.inf, f)
    cols_all = np.arange(n)
    for i in range(n_q):
        if not qok[i]:
            dist[i] = np.nan
            continue
        pool = []
        for s in range(splits):
            lo_, hi_ = min(s * tps * TILE, n), min((s + 1) * tps * TILE, n)
            c = cols_all[lo_:hi_][keep[i, lo_:hi_]]
            if one and len(c):
                if first_offered:
                    _, first = np.unique(bg[c], return_index=True)
                    c = c[np.sort(first)]
                else:
                    c = c[_best_per_group(c, score[i, c], bg[c])]
            pool.append(c[np.lexsort((c, score[i, c]))[:k]])
        c = np.concatenate(pool) if pool else np.zeros(0, np.int64)
        if one and len(c) and not no_merge_collapse:
            c = c[_best_per_group(c, score[i, c], bg[c])]
        c = c[np.lexsort((c, score[i, c]))[:k]]
        if cosine:
            dot = (bz[c] * qz[i]).sum(1, dtype=f)
            qq, bb = (qz[i] * qz[i]).sum(dtype=f), (bz[c] * bz[c]).sum(1, dtype=f)
            ok = (qq > 0) & (bb > 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                dd = (f(1) - np.where(ok, dot / np.sqrt(qq, dtype=f) / np.sqrt(bb, dtype=f), f(0))).astype(f)
        else:
            diff = bz[c] - qz[i]
            dd = np.sqrt((diff * diff).sum(1, dtype=f), dtype=f)
        o = np.lexsort((c, dd))
        idx[i, :len(c)] = c[o]
        dist[i, :len(c)] = dd[o]
    return idx, dist


# ---------------------------------------------------------------------------------------------------------------------
# the domain check: objects of near-copies
def object_set(n_objects=512, per_object=5, sigma=1e-3, seed=1):
    """(rows fp32 [5 n, 32], object int64 [5 n], label int64 [5 n]): every point of layout_ref's 32-D ten-cluster set
    repeated as an object of ``per_object`` alerts, jittered by N(0, sigma^2)."""
    import layout_ref
    pts, lab = layout_ref.cluster_set(n_objects, 32, seed)
    rng = np.random.default_rng(7000 + seed)
    rows = np.repeat(pts.astype(np.float64), per_object, axis=0)
    rows = (rows + sigma * rng.standard_normal(rows.shape)).astype(np.float32)
    obj = np.repeat(np.arange(len(pts), dtype=np.int64), per_object)
    return rows, obj, np.repeat(np.asarray(lab, np.int64), per_object)
