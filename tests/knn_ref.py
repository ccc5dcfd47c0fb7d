"""What the embedding-neighbour tests share (no GPU): seeded inputs, the float64 brute force, ``check_neighbors`` -- the
contract of btsbot_knn_query (include/btsbot_hip.h) -- and a numpy emulation of the two-pass scheme.

The contract, with u = 2^-24 and d64 the float64 distance from the fp32 inputs, for every returned (i, j):
  1 validity   indices distinct, in range, eligible (finite row, not the excluded self), sorted by (dist, index); fewer
               than k eligible rows: tail idx = -1, dist = +inf; a non-finite query row: idx = -1, dist = NaN throughout
  2 distance   euclidean |dist - d64| <= (D + 4) u d64  (direct form: gamma_{D+2} on the square, halved by the root, plus
               the root's rounding, a factor 2 to spare; identical rows give exactly 0); cosine |dist - d64| <= 4 (D + 2) u
  3 rank       t_j = j-th smallest eligible float64 squared distance, r_j = that of the j-th returned row:
               r_j <= t_j + tau, tau = 8 (D + 2) u (|q|^2 + max_b |b|^2) (twice the worst-case error of the fp32 expansion
               form, which also covers the split product's dropped remainder x remainder term, 2^-22 relative per
               product <= D u for D >= 4; D < 4: 8 (D + 6) u); cosine: on 1 - cos with tau = 8 (D + 2) u
  4 exact      integer coordinates in [-8, 8]: idx = the stable float64 argsort of the squared distances, ties included,
               dist = sqrt of the exact integer rounded to fp32 (``check_exact``)
The t_j come from the float64 expansion |q|^2 + |b|^2 - 2 q.b (one matrix product): its error is 2^-29 of tau, and it is
exact on integer rows.  The distances of the RETURNED rows (clause 2, r_j) are float64 sums of (q_i - b_i)^2.
"""
import numpy as np

U = 2.0 ** -24
TILE = 128   # the kernel's bank tile (csrc/knn_tile.h)

# (Q, N, D, k, splits): a covering subset of Q {1, 63, 65, 130} x N {1, 7, 127, 128, 129, 1000, 4099} x
# D {1, 5, 31, 32, 33, 528, 1024} x k {1, 15, 64} (k > N included) x splits {1, 2, 7, 0}
CASES = [
    (1, 1, 1, 1, 1),
    (63, 7, 5, 15, 2),
    (65, 127, 31, 1, 1),
    (130, 128, 32, 15, 7),
    (63, 129, 33, 64, 2),
    (65, 1000, 528, 15, 7),
    (130, 4099, 1024, 64, 0),
    (1, 4099, 5, 15, 7),
    (130, 1000, 32, 64, 2),
]
KINDS = ("normal", "scaled", "clustered")
LARGE = (300, 20000, 528, 15, 0)


def make_rows(kind, n, d, seed):
    """fp32 [n, d]: N(0,1) rows, rows scaled by 1e4, clustered rows (offset 10, sigma 0.01), or integer rows in [-8, 8]
    drawn from 24 distinct rows (heavy duplication: with period 24 the duplicates straddle every tile and split edge)."""
    rng = np.random.default_rng(seed)
    if kind == "integer":
        base = rng.integers(-8, 9, size=(24, d)).astype(np.float32)
        return base[np.arange(n) % 24].copy()
    x = rng.standard_normal((n, d))
    if kind == "scaled":
        x *= 1e4
    elif kind == "clustered":
        x = 10.0 + 0.01 * x
    elif kind != "normal":
        raise ValueError(kind)
    return x.astype(np.float32)


def case_inputs(case, kind, seed=0):
    q_n, n, d, _k, _s = case
    return make_rows(kind, q_n, d, 1000 + seed), make_rows(kind, n, d, 2000 + seed)


def finite_rows(x):
    return np.isfinite(x).all(axis=1)


def dist64_matrix(q, b, metric):
    """float64 [Q, N]: squared Euclidean distances (expansion form) or 1 - cos; non-finite rows give garbage the callers
    mask."""
    q64 = np.nan_to_num(q.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    b64 = np.nan_to_num(b.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    dot = q64 @ b64.T
    qq, bb = (q64 * q64).sum(1), (b64 * b64).sum(1)
    if metric == "euclidean":
        return np.maximum(qq[:, None] + bb[None, :] - 2.0 * dot, 0.0)
    den = np.sqrt(qq)[:, None] * np.sqrt(bb)[None, :]
    return 1.0 - np.where(den > 0, dot / np.where(den > 0, den, 1.0), 0.0)


def direct64(qrow, brows, metric):
    """float64 distances of one query row to some bank rows, direct form (euclidean: SQUARED)."""
    q64, b64 = qrow.astype(np.float64), brows.astype(np.float64)
    if metric == "euclidean":
        return ((b64 - q64) ** 2).sum(1)
    den = np.sqrt((q64 * q64).sum()) * np.sqrt((b64 * b64).sum(1))
    return 1.0 - np.where(den > 0, (b64 @ q64) / np.where(den > 0, den, 1.0), 0.0)


def eligible_mask(b, n_query, self_offset):
    """bool [Q, N]"""
    el = np.broadcast_to(finite_rows(b)[None, :], (n_query, b.shape[0])).copy()
    if self_offset >= 0:
        rows = np.arange(n_query)
        cols = rows + self_offset
        ok = cols < b.shape[0]
        el[rows[ok], cols[ok]] = False
    return el


def check_neighbors(q, b, idx, dist, k, metric="euclidean", self_offset=-1):
    """Clauses 1-3; raises AssertionError naming the clause.  Returns the worst (distance error / bound, rank excess /
    tau) for the record."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    idx, dist = np.asarray(idx), np.asarray(dist)
    n_q, d = q.shape
    n = b.shape[0]
    assert idx.shape == (n_q, k) and dist.shape == (n_q, k), "shape"
    assert idx.dtype == np.int64 and dist.dtype == np.float32, "dtype"
    el = eligible_mask(b, n_q, self_offset)
    dm = dist64_matrix(q, b, metric) if n else np.zeros((n_q, 0))
    qfin = finite_rows(q)
    bb_max = float(((b[finite_rows(b)].astype(np.float64)) ** 2).sum(1).max()) if finite_rows(b).any() else 0.0
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
        assert el[i, got].all(), f"validity: ineligible row returned for query {i}"
        dd = dist[i, :m].astype(np.float64)
        assert np.isfinite(dd).all(), f"validity: non-finite distance in row {i}"
        order_ok = (dd[1:] > dd[:-1]) | ((dd[1:] == dd[:-1]) & (got[1:] > got[:-1]))
        assert order_ok.all(), f"validity: row {i} not sorted by (dist, index)"
        if m == 0:
            continue
        r = direct64(q[i], b[got], metric)
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
        t = np.sort(dm[i][el[i]])[:m]
        excess = r - t
        assert (excess <= tau).all(), f"rank: row {i} exceeds t_j by {excess.max():.3e} = {excess.max() / tau:.2f} tau"
        nz = bound > 0
        if nz.any():
            worst_d = max(worst_d, float((err[nz] / bound[nz]).max()))
        if tau > 0:
            worst_r = max(worst_r, float(excess.max() / tau))
    return worst_d, worst_r


def check_exact(q, b, idx, dist, k, self_offset=-1):
    """Clause 4 (euclidean, integer rows in [-8, 8])."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    idx, dist = np.asarray(idx), np.asarray(dist)
    el = eligible_mask(b, q.shape[0], self_offset)
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
# the two-pass scheme in numpy: fp32 arithmetic throughout, f16 head + remainder operands ("split") or the fp32 product
def _pack(x, cosine):
    x = np.asarray(x, np.float32)
    fin = finite_rows(x)
    xz = np.where(fin[:, None], x, np.float32(0))
    with np.errstate(over="ignore"):
        ss = (xz * xz).sum(1, dtype=np.float32)
    ok = fin & np.isfinite(ss)
    amax = np.abs(xz).max(1) if x.shape[1] else np.zeros(len(x), np.float32)
    _, ex = np.frexp(amax)
    e = np.where(ok & (amax > 0), np.clip(15 - ex, -120, 120), 0).astype(np.int32)
    scaled = np.where(ok[:, None], np.ldexp(xz, e[:, None]), np.float32(0)).astype(np.float32)
    hi = scaled.astype(np.float16)
    lo = (scaled - hi.astype(np.float32)).astype(np.float16)
    down = np.ldexp(np.float32(1), -e).astype(np.float32)
    if cosine:
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(ss > 0, down / np.sqrt(ss, dtype=np.float32), np.float32(0)).astype(np.float32)
        bias = np.zeros(len(x), np.float32)
    else:
        scale, bias = down, ss
    bias = np.where(ok, bias, np.float32(np.inf)).astype(np.float32)
    scale = np.where(ok, scale, np.float32(0)).astype(np.float32)
    return hi, lo, bias, scale, ok, np.where(ok, xz.T, np.float32(0)).T


def emulate(q, b, k, metric="euclidean", splits=1, self_offset=-1, form="split", drop_tile=None, drop_split=None,
            stale_bank=None):
    """(idx int64 [Q, k], dist fp32 [Q, k]) as the kernels compute them, up to the summation order inside a product.
    Seeded faults for the tests of ``check_neighbors``: drop_tile / drop_split leave a bank tile / a split's candidates
    out; stale_bank takes the biases (norms) from another bank."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    n_q, d = q.shape
    n = b.shape[0]
    cosine = metric == "cosine"
    qh, ql, _, qs, qok, qz = _pack(q, False)
    qscale = (2 * qs).astype(np.float32)
    bh, bl, bias, bscale, bok, bz = _pack(b, cosine)
    if stale_bank is not None:
        bias = _pack(stale_bank, cosine)[2]
    f = np.float32
    if form == "split":
        acc = (ql.astype(f) @ bh.astype(f).T + qh.astype(f) @ bl.astype(f).T) + qh.astype(f) @ bh.astype(f).T
        with np.errstate(invalid="ignore", over="ignore"):
            score = bias[None, :] - (acc * qscale[:, None]) * bscale[None, :]
    else:   # the fp32 product
        dot = qz @ bz.T
        with np.errstate(invalid="ignore", over="ignore"):
            if cosine:
                nrm = np.sqrt((bz * bz).sum(1, dtype=f), dtype=f)
                score = np.where(bok, -2 * dot / np.where(nrm > 0, nrm, f(1)) * (nrm > 0), f(np.inf))
            else:
                score = bias[None, :] - 2 * dot
    score = score.astype(f)
    keep = np.isfinite(score) | np.isneginf(score)
    keep &= score < np.inf
    if self_offset >= 0:
        rows = np.arange(n_q)
        cols = rows + self_offset
        ok = cols < n
        keep[rows[ok], cols[ok]] = False
    tiles = (n + TILE - 1) // TILE
    if splits == 0:
        splits = max(1, min(32, tiles, -(-512 // max(1, -(-n_q // TILE)))))
    tps = -(-tiles // splits) if tiles else 0
    if drop_tile is not None:
        keep[:, drop_tile * TILE:(drop_tile + 1) * TILE] = False
    idx = np.full((n_q, k), -1, np.int64)
    dist = np.full((n_q, k), np.inf, f)
    cols_all = np.arange(n)
    for i in range(n_q):
        if not qok[i]:
            dist[i] = np.nan
            continue
        pool = []
        for s in range(splits):
            if s == drop_split:
                continue
            lo_, hi_ = min(s * tps * TILE, n), min((s + 1) * tps * TILE, n)
            c = cols_all[lo_:hi_][keep[i, lo_:hi_]]
            o = np.lexsort((c, score[i, c]))[:k]
            pool.append(c[o])
        c = np.concatenate(pool) if pool else np.zeros(0, np.int64)
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
