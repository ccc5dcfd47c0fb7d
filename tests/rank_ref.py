"""What the neighbour-rank and map-quality tests share (no GPU): the contract of ``EmbeddingIndex.rank_of`` as a float64
checker over the fp32 inputs, a numpy emulation of its passes with seeded faults, and trustworthiness / continuity in
float64.

The contract (include/btsbot_hip.h).  dist[q, c] is the direct-form fp32 distance of query row q
and bank row targets[q, c]; rank[q, c] the number of eligible bank rows b with (direct-form distance, b) before
(dist[q, c], targets[q, c]).  With d64 the float64 distance and band = radius_ref.band_of (the bound of the direct form:
(D + 4) u relative, cosine 4 (D + 2) u absolute) a pair b is
  surely before   d64_b (1 + band) < d64_t (1 - band)      (cosine: d64_b + band < d64_t - band)
  surely after    d64_b (1 - band) > d64_t (1 + band)
and free otherwise: lo = the surely-before pairs, hi = lo + the free ones, and a device rank must lie in [lo, hi].
rank = -1 where the target is out of range or not eligible for q or q is non-finite; dist = NaN where the target is out
of range or either row is non-finite.  On integer rows (``make_rows("integer")``: d^2 is an exact integer below 2^24, its
fp32 root is monotone) the order is known exactly: ``exact=True`` holds the rank to the float64 (d^2, index) order.
"""
import numpy as np

import radius_ref as R
from knn_ref import TILE, U, _pack, dist64_matrix, finite_rows

FAULTS = ("no_index_tiebreak", "lo_without_margin", "self_not_masked", "target_counts_itself", "split_twice",
          "mask_every_column")


def random_targets(n_q, n, t, seed):
    """int64 [n_q, t], uniform over the bank rows"""
    return np.random.default_rng(seed).integers(0, max(n, 1), size=(n_q, t)).astype(np.int64)


def _eligible(q, b, self_offset, qgroups, bgroups, self_rows=None):
    el = R.eligible(q, b, self_offset, qgroups, bgroups)
    if self_rows is not None:
        el[np.arange(q.shape[0]), np.asarray(self_rows)] = False
    return el


def rank_intervals(q, b, targets, metric="euclidean", self_offset=-1, qgroups=None, bgroups=None, exact=False,
                   self_rows=None):
    """(lo, hi int64 [Q, t], valid bool [Q, t], d64 float64 [Q, t]): the interval a rank must lie in where ``valid``
    (elsewhere it must be -1).  exact: lo = hi = the float64 (d^2, index) order (euclidean, integer rows).
    self_rows: int [Q], the bank row that IS query row q (masked like self_offset's, for sampled rows)."""
    q, b, targets = np.asarray(q, np.float32), np.asarray(b, np.float32), np.asarray(targets)
    n_q, dim = q.shape
    n = b.shape[0]
    el = _eligible(q, b, self_offset, qgroups, bgroups, self_rows)
    inr = (targets >= 0) & (targets < n)
    tc = np.where(inr, targets, 0)
    rows = np.arange(n_q)[:, None]
    valid = inr & (el[rows, tc] if n else False)
    if exact:
        assert metric == "euclidean"
        d = dist64_matrix(q, b, metric)
        assert (d == np.round(d)).all() and d.max(initial=0) < 2 ** 24
    else:
        d = R.d64_matrix(q, b, metric) if n else np.zeros((n_q, 0))
    band = R.band_of(dim, metric)
    lo = np.zeros(targets.shape, np.int64)
    hi = np.zeros(targets.shape, np.int64)
    dt_all = np.where(inr, d[rows, tc] if n else 0.0, np.nan)
    cols = np.arange(n)
    for c in range(targets.shape[1]):
        dt = dt_all[:, c][:, None]
        other = el & (cols[None, :] != tc[:, c][:, None])
        if exact:
            bef = (d < dt) | ((d == dt) & (cols[None, :] < tc[:, c][:, None]))
            lo[:, c] = hi[:, c] = (bef & other).sum(1)
        elif metric == "euclidean":
            sure = d * (1 + band) < dt * (1 - band)
            after = d * (1 - band) > dt * (1 + band)
            lo[:, c] = (sure & other).sum(1)
            hi[:, c] = (~after & other).sum(1)
        else:
            sure = d + band < dt - band
            after = d - band > dt + band
            lo[:, c] = (sure & other).sum(1)
            hi[:, c] = (~after & other).sum(1)
    if exact:
        dt_all = np.sqrt(dt_all)
    return lo, hi, valid, dt_all


def check_ranks(q, b, targets, rank, dist, metric="euclidean", self_offset=-1, qgroups=None, bgroups=None, exact=False):
    """AssertionError naming the clause; returns (share of valid (q, c) with lo != hi, worst distance error / band)."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    targets, rank, dist = np.asarray(targets), np.asarray(rank), np.asarray(dist)
    assert rank.dtype == np.int64 and dist.dtype == np.float32, "dtype"
    assert rank.shape == targets.shape == dist.shape, "shape"
    n = b.shape[0]
    lo, hi, valid, d64 = rank_intervals(q, b, targets, metric, self_offset, qgroups, bgroups, exact)
    assert (rank[~valid] == -1).all(), "validity: a rank where the target is out of range / not eligible / q non-finite"
    inr = (targets >= 0) & (targets < n)
    both_fin = inr & finite_rows(q)[:, None] & (finite_rows(b)[np.where(inr, targets, 0)] if n else False)
    assert np.isnan(dist[~both_fin]).all(), "distance: not NaN for an out-of-range target or a non-finite row"
    assert np.isfinite(dist[both_fin]).all(), "distance: NaN or inf for a finite pair"
    band = R.band_of(q.shape[1], metric)
    err = np.abs(dist[both_fin].astype(np.float64) - d64[both_fin])
    bound = band * d64[both_fin] if metric == "euclidean" else np.full(err.shape, band)
    assert (err <= bound).all(), f"distance: off by {err.max():.3e}"
    if exact:
        assert (dist[both_fin] == d64[both_fin].astype(np.float32)).all(), "distance: not the root of the exact integer"
    bad = valid & ((rank < lo) | (rank > hi))
    assert not bad.any(), (f"rank: {int(bad.sum())} outside [lo, hi], first at {np.argwhere(bad)[0].tolist()}: "
                           f"{rank[bad][0]} not in [{lo[bad][0]}, {hi[bad][0]}]")
    nz = bound > 0
    worst = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    return float((valid & (lo != hi)).sum() / max(1, valid.sum())), worst


# ---------------------------------------------------------------------------------------------------------------------
# the passes in numpy: split f16 operands, fp32 arithmetic, both limits, band verification in the direct form
def direct32(q, b, metric):
    """fp32 [Q, N]: the direct-form distance as the device forms it, up to the summation order inside a row"""
    f = np.float32
    qz = np.where(finite_rows(q)[:, None], q, f(0)).astype(f)
    bz = np.where(finite_rows(b)[:, None], b, f(0)).astype(f)
    out = np.empty((q.shape[0], b.shape[0]), f)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(q.shape[0]):
            if metric == "euclidean":
                diff = bz - qz[i]
                out[i] = np.sqrt((diff * diff).sum(1, dtype=f), dtype=f)
            else:
                dot = (bz * qz[i]).sum(1, dtype=f)
                qq, bb = (qz[i] * qz[i]).sum(dtype=f), (bz * bz).sum(1, dtype=f)
                ok = (qq > 0) & (bb > 0)
                out[i] = f(1) - np.where(ok, dot / np.sqrt(qq, dtype=f) / np.sqrt(np.where(ok, bb, f(1)), dtype=f), f(0))
    return out


def emulate_ranks(q, b, targets, metric="euclidean", splits=1, self_offset=-1, qgroups=None, bgroups=None, fault=None,
                  stats=None):
    """(rank int64 [Q, t], dist fp32 [Q, t]) as the thresholds kernel, the tile pass and the band verification compute
    them.  fault: one of FAULTS, a seeded mistake ``check_ranks`` must reject."""
    assert fault is None or fault in FAULTS
    q, b, targets = np.asarray(q, np.float32), np.asarray(b, np.float32), np.asarray(targets)
    f = np.float32
    n_q, dim = q.shape
    n, t = b.shape[0], targets.shape[1]
    cosine = metric == "cosine"
    qh, ql, qq, qs, qok, _ = _pack(q, False)
    bh, bl, bias, bscale, bok, _ = _pack(b, cosine)
    qscale = (2 * qs).astype(f)
    acc = (ql.astype(f) @ bh.astype(f).T + qh.astype(f) @ bl.astype(f).T) + qh.astype(f) @ bh.astype(f).T
    d32 = direct32(q, b, metric)
    el = R.eligible(q, b, -1 if fault == "self_not_masked" else self_offset, qgroups, bgroups)
    el_target = R.eligible(q, b, self_offset, qgroups, bgroups)
    rel, relm = f(1 + 4 * (dim + 4) * U), f(1 - 4 * (dim + 4) * U)
    ctau = f((16 if cosine else 8) * (dim + 8) * U)
    qq = np.where(qok, qq, f(0)).astype(f)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = (bias[None, :] - (acc * qscale[:, None]) * bscale[None, :]).astype(f)
        if cosine:
            qinv = np.where(qok & (qq > 0), f(0.5) / np.sqrt(np.where(qq > 0, qq, f(1)), dtype=f), f(0)).astype(f)
            g = (s * qinv[:, None] + f(1)).astype(f)
            x = np.zeros_like(g)
        else:
            g = (s + qq[:, None]).astype(f)
            x = (qq[:, None] + bias[None, :]).astype(f)
    tiles = (n + TILE - 1) // TILE
    if splits == 0:
        splits = max(1, min(32, tiles, -(-512 // max(1, -(-n_q // TILE)))))
    tps = -(-tiles // splits) if tiles else 0
    rank = np.full((n_q, t), -1, np.int64)
    dist = np.full((n_q, t), np.nan, f)
    cols = np.arange(n)
    n_band = 0
    for i in range(n_q):
        lo_c, hi_c, ok_c = np.full(t, -np.inf, f), np.full(t, -np.inf, f), np.zeros(t, bool)
        for c in range(t):
            tg = targets[i, c]
            if not (0 <= tg < n) or not qok[i] or not bok[tg]:
                continue
            dist[i, c] = d = d32[i, tg]
            if not el_target[i, tg]:
                continue
            ok_c[c] = True
            rank[i, c] = 0
            with np.errstate(over="ignore"):
                if cosine:
                    hi_c[c], lo_c[c] = d + ctau, d - ctau
                else:
                    hi_c[c], lo_c[c] = (d * d) * rel, ((d * d) if fault == "lo_without_margin" else (d * d) * relm)
        with np.errstate(invalid="ignore", over="ignore"):
            m = (ctau * x[i]).astype(f)
            widest = hi_c.max() + m
            passing = el[i] & (s[i] < np.inf) & (g[i] <= widest)
            mlo = np.zeros_like(m) if fault == "lo_without_margin" else m
            sure = passing[None, :] & ok_c[:, None] & (g[i][None, :] < lo_c[:, None] - mlo[None, :])     # [t, N]
            band = passing[None, :] & ok_c[:, None] & ~sure & (g[i][None, :] <= hi_c[:, None] + m[None, :])
        for sp in range(splits):
            a, e = min(sp * tps * TILE, n), min((sp + 1) * tps * TILE, n)
            add = sure[:, a:e].sum(1)
            rank[i] += np.where(ok_c, add * (2 if fault == "split_twice" and sp == splits - 1 else 1), 0)
        entries = np.flatnonzero(band.any(0))
        n_band += len(entries)
        for bi in entries:
            d = d32[i, bi]
            for c in np.flatnonzero(ok_c if fault == "mask_every_column" else band[:, bi]):
                dc, tg = dist[i, c], targets[i, c]
                if fault == "no_index_tiebreak":
                    bef = d < dc
                elif fault == "target_counts_itself":
                    bef = d < dc or (d == dc and bi <= tg)
                else:
                    bef = d < dc or (d == dc and bi < tg)
                rank[i, c] += int(bef)
    if stats is not None:
        stats["band"] = n_band
    return rank, dist


# ---------------------------------------------------------------------------------------------------------------------
# trustworthiness and continuity in float64, ties by (dist, index)
def _d64(x, metric):
    x = np.asarray(x, np.float32)
    d = dist64_matrix(x, x, metric)
    return np.sqrt(d) if metric == "euclidean" else d


def neighbors64(x, k, metric="euclidean", rows=None, groups=None):
    """int64 [m, k]: the k nearest OTHER rows (of other groups) of the judged rows by the float64 (dist, index) order,
    and the number of judged rows whose k-th and (k + 1)-th distances are within the fp32 band of each other (where the
    device may hold another set)."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    d = _d64(x, metric)[rows]
    mask = np.arange(n)[None, :] == rows[:, None]
    if groups is not None:
        mask |= np.asarray(groups)[None, :] == np.asarray(groups)[rows][:, None]
    d = np.where(mask, np.inf, d)
    order = np.lexsort((np.broadcast_to(np.arange(n), d.shape), d), axis=1)
    ds = np.take_along_axis(d, order, 1)
    band = R.band_of(x.shape[1], metric)
    gap = ds[:, k] - ds[:, k - 1]
    close = gap <= (2 * band * ds[:, k] if metric == "euclidean" else 2 * band)
    return order[:, :k].astype(np.int64), int(close.sum())


def _penalty_sum(rank, k):
    return int(np.maximum(0, rank + 1 - k).sum())


def _formula(pen, m, n, k):
    return 1.0 - 2.0 / (m * k * (2.0 * n - 3.0 * k - 1.0)) * pen


def trustworthiness64(emb, y, k, metric="euclidean", rows=None, groups=None, swap=False, interval=False):
    """sklearn's trustworthiness from float64 distances with (dist, index) ties (swap=True: continuity).
    interval=True: (T from the hi ranks, T from the lo ranks, rows whose neighbour set the band leaves open): where the
    device value must lie, its ranks being exact in the fp32 direct form."""
    emb, y = np.asarray(emb, np.float32), np.asarray(y, np.float32)
    hi_space, lo_space = (y, emb) if swap else (emb, y)         # ranks are taken in hi_space, neighbours in lo_space
    m_hi, m_lo = ("euclidean", metric) if swap else (metric, "euclidean")
    n = emb.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    nb, open_sets = neighbors64(lo_space, k, m_lo, rows, groups)
    qg = None if groups is None else np.asarray(groups)[rows]
    if interval:
        lo, hi, valid, _ = rank_intervals(hi_space[rows], hi_space, nb, m_hi, -1, qg, groups, self_rows=rows)
        assert valid.all()
        return (_formula(_penalty_sum(hi, k), len(rows), n, k), _formula(_penalty_sum(lo, k), len(rows), n, k), open_sets)
    d = _d64(hi_space, m_hi)[rows]
    cols = np.arange(n)
    other = cols[None, :] != rows[:, None]
    if groups is not None:
        other &= np.asarray(groups)[None, :] != qg[:, None]
    rank = np.zeros(nb.shape, np.int64)
    for c in range(k):
        dt = d[np.arange(len(rows)), nb[:, c]][:, None]
        bef = (d < dt) | ((d == dt) & (cols[None, :] < nb[:, c][:, None]))
        rank[:, c] = (bef & other).sum(1)
    return _formula(_penalty_sum(rank, k), len(rows), n, k)


def lattice_3d(side=7):
    """(emb int-valued fp32 [side^3, 3], y = its first two coordinates): every distance is the root of an exact integer
    in both spaces, so the device's ranks and neighbour sets are the float64 (dist, index) ones"""
    g = np.arange(side, dtype=np.float32)
    emb = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return emb, emb[:, :2].copy()
