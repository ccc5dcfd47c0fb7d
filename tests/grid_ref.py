"""What the MapIndex tests share (no GPU): the three rules of csrc/grid.hip in numpy float32, one
rounded operation at a time, the brute-force answers they define, and the seeded sets.

  distance    sqrt(fl(fl(t0 t0) + fl(t1 t1))), t = q - b: what direct_distance of csrc/knn_tile.h gives at D = 2
  finite row  both coordinates finite and fl(fl(x x) + fl(y y)) <= FLT_MAX
  cells       c(x) = clamp(floor(fl(fl(x - x0) * inv_h)), 0, G - 1), a monotone function of x; a query with radius r walks
              c(lo) .. c(hi), lo = down(fl(x - R)), hi = up(fl(x + R)), R = up(fl(max(r, 2^-60) * (1 + 16 u)))
"""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
INF = F(np.inf)


def distance(q, b):
    """fp32 [Q, N] for q [Q, 2] and b [N, 2]"""
    q, b = np.asarray(q, F), np.asarray(b, F)
    with np.errstate(over="ignore", invalid="ignore"):
        t0 = (q[:, None, 0] - b[None, :, 0]).astype(F)
        t1 = (q[:, None, 1] - b[None, :, 1]).astype(F)
        s0 = (t0 * t0).astype(F)
        s1 = (t1 * t1).astype(F)
        ss = (s0 + s1).astype(F)
        return np.sqrt(ss, dtype=F)


def finite_rows(x):
    x = np.asarray(x, F)
    with np.errstate(over="ignore", invalid="ignore"):
        sx = (x[:, 0] * x[:, 0]).astype(F)
        sy = (x[:, 1] * x[:, 1]).astype(F)
        ss = (sx + sy).astype(F)
        return (np.abs(x[:, 0]) <= FLT_MAX) & (np.abs(x[:, 1]) <= FLT_MAX) & (ss <= FLT_MAX)


def geometry(points, G):
    """(x0 [2], inv_h [2]) fp32 as grid_geometry_kernel forms them from the bounding box of the finite rows"""
    pts = np.asarray(points, F)
    fin = finite_rows(pts)
    x0, inv = np.zeros(2, F), np.zeros(2, F)
    for a in range(2):
        lo = pts[fin, a].min() if fin.any() else INF
        hi = pts[fin, a].max() if fin.any() else -INF
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            ext = F(hi - lo)
            v = F(F(G) / ext)
        ok = ext > 0 and v <= FLT_MAX and abs(lo) <= FLT_MAX
        x0[a] = lo if abs(lo) <= FLT_MAX else F(0)
        inv[a] = v if ok else F(0)
    return x0, inv


def cell_of(x, x0, inv_h, G):
    """int cells of the fp32 numbers x (+-inf allowed)"""
    x = np.asarray(x, F)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (x - F(x0)).astype(F)
        v = np.floor((t * F(inv_h)).astype(F))
    v = np.where(np.isnan(v), F(0), v)
    return np.clip(v, 0, G - 1).astype(np.int64)


def inflate(r):
    r = np.asarray(r, F)
    with np.errstate(over="ignore"):
        R = (np.maximum(r, F(2.0 ** -60)) * F(1 + 2.0 ** -20)).astype(F)
    return np.nextafter(R, INF)


def safe_cells(x, r, x0, inv_h, G):
    """(c0, c1): the cells a query coordinate x with radius r walks on one axis"""
    x = np.asarray(x, F)
    R = inflate(r)
    with np.errstate(over="ignore", invalid="ignore"):
        lo = np.nextafter((x - R).astype(F), -INF)
        hi = np.nextafter((x + R).astype(F), INF)
    return cell_of(lo, x0, inv_h, G), cell_of(hi, x0, inv_h, G)


def eligible(q, b, self_offset=-1, qgroups=None, bgroups=None):
    """bool [Q, N]"""
    q, b = np.asarray(q, F), np.asarray(b, F)
    el = finite_rows(q)[:, None] & finite_rows(b)[None, :]
    if self_offset >= 0:
        rows = np.arange(q.shape[0])
        cols = rows + self_offset
        ok = cols < b.shape[0]
        el[rows[ok], cols[ok]] = False
    if qgroups is not None:
        el &= np.asarray(qgroups, np.int64)[:, None] != np.asarray(bgroups, np.int64)[None, :]
    return el


def radius_lists(q, b, r, sort="index", **kw):
    """(indptr int64, indices int64, dist fp32): the eligible pairs with distance() <= r in fp32"""
    q, b = np.asarray(q, F), np.asarray(b, F)
    el = eligible(q, b, **kw)
    d = distance(q, b)
    rr = np.broadcast_to(np.asarray(r, F), (q.shape[0],))
    indptr, idx, dist = [0], [], []
    for i in range(q.shape[0]):
        got = np.flatnonzero(el[i] & (d[i] <= rr[i]))
        if sort == "distance":
            got = got[np.lexsort((got, d[i, got]))]
        idx.append(got)
        dist.append(d[i, got])
        indptr.append(indptr[-1] + len(got))
    return (np.asarray(indptr, np.int64), np.concatenate(idx).astype(np.int64) if idx else np.zeros(0, np.int64),
            np.concatenate(dist).astype(F) if dist else np.zeros(0, F))


def knn(q, b, k, **kw):
    """(idx int64 [Q, k], dist fp32 [Q, k]): the k smallest eligible rows by (distance(), index); -1 / +inf where fewer
    are eligible, -1 / NaN for a non-finite query row"""
    q, b = np.asarray(q, F), np.asarray(b, F)
    el = eligible(q, b, **kw)
    d = distance(q, b)
    idx = np.full((q.shape[0], k), -1, np.int64)
    dist = np.full((q.shape[0], k), np.inf, F)
    qfin = finite_rows(q)
    for i in range(q.shape[0]):
        if not qfin[i]:
            dist[i] = np.nan
            continue
        got = np.flatnonzero(el[i])
        got = got[np.lexsort((got, d[i, got]))][:k]
        idx[i, :len(got)] = got
        dist[i, :len(got)] = d[i, got]
    return idx, dist


# ---------------------------------------------------------------------------------------------------------------------
# the sets
def edge_set(G=64, seed=5):
    """about 2,000 rows in [0, 8]^2 (the corners are rows, so the box is exactly that and a cell is 8 / G wide): exact
    duplicates, rows exactly on cell edges and one fp32 ulp to either side, a NaN row, an inf row, a row with
    |x| = 1e20 (finite coordinates, an overflowing norm) and one far outlier as the LAST row (drop it for the plain
    box)."""
    rng = np.random.default_rng(seed)
    pts = [np.array([[0, 0], [8, 8]], F), rng.uniform(0, 8, size=(1500, 2)).astype(F)]
    h = 8.0 / G
    edges = (np.arange(1, G, max(1, G // 16)) * h).astype(F)
    other = rng.uniform(0, 8, size=len(edges)).astype(F)
    for e in (edges, np.nextafter(edges, -INF), np.nextafter(edges, INF)):
        pts.append(np.stack([e, other], 1))
        pts.append(np.stack([other, e], 1))
        pts.append(np.stack([e, e[::-1]], 1))
    x = np.concatenate(pts).astype(F)
    x = np.concatenate([x, x[100:350]])                       # exact duplicates, far apart in the rows
    x = x[rng.permutation(len(x))]
    x[17] = [np.nan, 1.0]
    x[400] = [2.0, np.inf]
    x[901] = [1e20, 3.0]
    return np.concatenate([x, np.array([[900.0, -700.0]], F)]).astype(F)


def offset_set(seed=6, n=500):
    """rows near (4096, 4096), where an ulp of a coordinate is 4.9e-4: r = 0.01 is twenty ulps"""
    rng = np.random.default_rng(seed)
    return (4096.0 + rng.uniform(0, 0.25, size=(n, 2))).astype(F)


def zero_extent_set(n=50):
    """every row the same point"""
    return np.full((n, 2), 3.25, F)


def queries_for(b, n=130, seed=7):
    """n query rows: bank rows, rows near bank rows, rows outside the box, a NaN row and an overflowing one"""
    rng = np.random.default_rng(seed)
    b = np.asarray(b, F)
    fin = b[finite_rows(b)]
    lo, hi = fin.min(0), fin.max(0)
    span = np.maximum(hi - lo, F(1e-3))
    take = fin[rng.integers(0, len(fin), size=n)]
    q = take.copy()
    q[n // 3:2 * n // 3] += (rng.normal(0, 0.01, size=(2 * n // 3 - n // 3, 2)) * span).astype(F)
    out = np.arange(2 * n // 3, n)
    q[out] = (lo - span * 0.5 + rng.uniform(0, 2, size=(len(out), 2)) * span * np.array([1.0, 0.1])).astype(F)
    q[out[::2], 1] = (hi[1] + span[1] * rng.uniform(0.01, 0.5, size=len(out[::2]))).astype(F)
    q[5] = [np.nan, 0.0]
    q[6] = [3e19, 3e19]
    return q.astype(F)


def high_bit_groups(n, seed=8, distinct=9):
    """int64 ids that differ only in the high 32 bits"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, distinct, size=n).astype(np.int64) << 32) + 12345
