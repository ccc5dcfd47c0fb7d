"""float64 numpy restatement of btsbot_amd.layout (csrc/layout.hip), the checks the GPU tests
apply, and a numpy trustworthiness.

The restatement follows the algorithm step for step: the same bisection (float64, sigma rounded to fp32 once), the same
fp32 union ``w = (a + b) - a b``, the same fp32 ``r = w / w_max`` with the float64 firing rule, the same counter hash.
What it does differently is the arithmetic of an epoch's terms and their sum: float64 here, fp32 (with the hardware's
exp2 / log2) on the device.  ``epoch(..., fault=...)`` makes one seeded mistake at a time (tests/test_layout_reference.py).
"""
import numpy as np

U64 = np.uint64
F32, F64 = np.float32, np.float64

# |y_dev - y_ref| <= EPOCH_C * 2^-24 * (|y_ref| + alpha * sum |term|) per coordinate.  EPOCH_MEASURED is the worst ratio
# measured on an MI355X over every case of tests/test_gpu_layout.py against this restatement (the hub row of 129 slots,
# epoch 1 of 10; 5.82 on the kNN graph of 1,025 vertices, 0.93 on the pair); EPOCH_C is 8 x that, rounded up to a power
# of two (the kernel's exp2 / log2 are approximate and cases differ), and may not exceed 256: past that a dropped term
# of alpha * 1e-2 begins to hide.
EPOCH_MEASURED = 5.99
EPOCH_C = 64.0
EPOCH_C_LIMIT = 256.0
FAULTS = ("drop_sample", "no_self_check", "no_clip", "alpha_neighbour", "exponent_b", "fire_fp32", "no_factor_2")


def mix64(x):
    """splitmix64's step and finaliser on uint64 arrays (wrapping)."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=U64) + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def hash_base(seed, epoch):
    return mix64(np.array([seed & ((1 << 64) - 1)], dtype=U64) ^ mix64(np.array([epoch], dtype=U64)))[0]


def counter_hash(seed, epoch, slot, sample):
    with np.errstate(over="ignore"):
        return mix64(hash_base(seed, epoch) + U64(64) * np.asarray(slot, dtype=U64) + np.asarray(sample, dtype=U64))


def _unit(h):
    return (h >> U64(40)).astype(F64) / 16777216.0


def random_init(n, seed):
    """Uniform in [-10, 10): float32 [n, 2]."""
    h = counter_hash(seed, 0, np.repeat(np.arange(n), 2), np.tile(np.arange(2), n))
    return (20.0 * _unit(h) - 10.0).astype(F32).reshape(n, 2)


def jitter(y, seed):
    n = y.shape[0]
    h = counter_hash(seed, 0, np.repeat(np.arange(n), 2), np.tile(np.arange(2), n))
    return (y.astype(F64).reshape(-1) + (2.0 * _unit(h) - 1.0) * 1e-4).astype(F32).reshape(n, 2)


def pca_init(emb, seed):
    """init="pca" in float64 (the device forms covariance and projection in fp32: equal up to that)."""
    from btsbot_amd.layout import pca_directions
    emb = np.asarray(emb, dtype=F64)
    fin = np.isfinite(emb).all(axis=1)
    xc = np.where(fin[:, None], emb - emb[fin].mean(axis=0), 0.0) if fin.any() else np.zeros_like(emb)
    proj = xc @ pca_directions(xc.T @ xc / max(int(fin.sum()), 1))
    y = jitter((proj * (10.0 / max(np.abs(proj).max(), np.finfo(F32).tiny))).astype(F32), seed)
    y[~fin] = np.nan
    return y


# ---- steps 1 and 2
def smooth_knn(idx, dist):
    """rho, sigma float32 [n] and the memberships float32 [n, k] of idx int64 [n, k], dist float32 [n, k]."""
    idx, dist = np.asarray(idx), np.asarray(dist, dtype=F32)
    n, k = idx.shape
    d = dist.astype(F64)
    present = idx >= 0
    nb = present.copy()
    nb[:, 0] = False
    pos = nb & (dist > 0)
    rho = np.where(pos.any(axis=1), np.where(pos, d, np.inf).min(axis=1), 0.0)
    with np.errstate(invalid="ignore"):
        x = np.where(nb, d - rho[:, None], 0.0)
    target = np.log2(float(k))
    lo, hi, mid = np.zeros(n), np.full(n, np.inf), np.ones(n)
    done = np.zeros(n, dtype=bool)
    for _ in range(64):
        with np.errstate(over="ignore", invalid="ignore"):
            psum = np.where(nb, np.where(x > 0, np.exp(-(x / mid[:, None])), 1.0), 0.0).sum(axis=1)
        done |= np.abs(psum - target) < 1e-5
        if done.all():
            break
        gt = psum > target
        hi = np.where(~done & gt, mid, hi)
        lo = np.where(~done & ~gt, mid, lo)
        with np.errstate(invalid="ignore"):
            new = np.where(gt | np.isfinite(hi), (lo + hi) / 2.0, mid * 2.0)
        mid = np.where(done, mid, new)
    cnt = present.sum(axis=1)
    mean_row = np.where(present, d, 0.0).sum(axis=1) / np.maximum(cnt, 1)
    mean_all = np.where(present, d, 0.0).sum() / max(int(present.sum()), 1)
    mid = np.maximum(mid, 1e-3 * np.where(rho > 0, mean_row, mean_all))
    sigma = mid.astype(F32)
    edge = nb & (idx < n) & (idx != np.arange(n)[:, None])
    with np.errstate(over="ignore", invalid="ignore"):
        memb = np.where(edge, np.where(x > 0, np.exp(-(x / sigma.astype(F64)[:, None])), 1.0), 0.0).astype(F32)
    return rho.astype(F32), sigma, memb


class Graph:
    def __init__(self, indptr, indices, weights, sigma, rho):
        self.indptr, self.indices, self.weights, self.sigma, self.rho = indptr, indices, weights, sigma, rho
        self.n = len(indptr) - 1


def fuzzy_graph(idx, dist):
    idx = np.asarray(idx)
    n, k = idx.shape
    rho, sigma, memb = smooth_knn(idx, dist)
    rows = np.repeat(np.arange(n, dtype=np.int64), k).reshape(n, k)
    edge = (idx >= 0) & (idx < n) & (idx != rows)
    edge[:, 0] = False
    i, j, a = rows[edge], idx[edge], memb[edge]
    kf, kr = i * n + j, j * n + i
    keys = np.unique(np.concatenate([kf, kr]))
    fwd, rev = np.zeros(len(keys), dtype=F32), np.zeros(len(keys), dtype=F32)
    fwd[np.searchsorted(keys, kf)] = a
    rev[np.searchsorted(keys, kr)] = a
    w = (fwd + rev) - fwd * rev                                       # fp32, in exactly this form
    assert w.dtype == F32
    indptr = np.searchsorted(keys // max(n, 1), np.arange(n + 1)).astype(np.int64)
    return Graph(indptr, (keys % max(n, 1)).astype(np.int32), w, sigma, rho)


def graph_from_pairs(n, pairs):
    """The symmetric CSR graph of {(i, j): weight} (each undirected pair named once)."""
    both = sorted([(i, j, w) for (i, j), w in pairs.items()] + [(j, i, w) for (i, j), w in pairs.items()])
    rows = np.array([p[0] for p in both], dtype=np.int64)
    return Graph(np.searchsorted(rows, np.arange(n + 1)).astype(np.int64), np.array([p[1] for p in both], dtype=np.int32),
                 np.array([p[2] for p in both], dtype=F32), None, None)


def hub_graph(n, seed):
    """Vertex 0 joined to every other vertex (a row longer than a wave: several trips of its lanes) plus a ring of weight
    1; the hub's weights are uniform in [0.05, 1)."""
    rng = np.random.default_rng(seed)
    pairs = {(0, j): F32(rng.uniform(0.05, 1.0)) for j in range(1, n)}
    for i in range(1, n - 1):
        pairs[(i, i + 1)] = F32(1.0)
    return graph_from_pairs(n, pairs)


# ---- step 4
def alpha_of(epoch, n_epochs, learning_rate=1.0):
    return float(F32(float(learning_rate) * (1.0 - (epoch - 1) / float(n_epochs))))


def drop_vertex(g, v):
    """g without the edges of vertex v (what a non-finite embedding row looks like)."""
    rows = np.repeat(np.arange(g.n), np.diff(g.indptr))
    keep = (rows != v) & (g.indices != v)
    return Graph(np.searchsorted(rows[keep], np.arange(g.n + 1)).astype(np.int64), g.indices[keep], g.weights[keep], None, None)


def epoch(g, y, n, n_epochs, a, b, seed=0, negative_sample_rate=5, learning_rate=1.0, fault=None, stats=None):
    """Epoch ``n`` of the schedule from the positions ``y`` (float32 [N, 2]) in float64.  Returns (y_new float64 [N, 2],
    scale float64 [N, 2]) with scale = |y_new| + alpha_n * sum |term|, the quantity the epoch bound is stated in.
    stats (a dict): counts of the special events met are added to it."""
    assert fault is None or fault in FAULTS
    N = g.n
    y = np.asarray(y, dtype=F32).astype(F64)
    a, b = float(F32(a)), float(F32(b))
    w = g.weights
    with np.errstate(invalid="ignore", divide="ignore"):
        r32 = w / (w.max() if len(w) else F32(0))
        if fault == "fire_fp32":
            fire = np.floor(F32(n) * r32) > np.floor(F32(n - 1) * r32)
        else:
            fire = np.floor(n * r32.astype(F64)) > np.floor((n - 1) * r32.astype(F64))
    slot = np.nonzero(fire)[0]
    v = np.repeat(np.arange(N), np.diff(g.indptr))[slot]
    u = g.indices[slot].astype(np.int64)
    total, mag = np.zeros((N, 2)), np.zeros((N, 2))

    def clip(t):
        return t if fault == "no_clip" else np.clip(t, -4.0, 4.0)

    def add(rows, t):
        np.add.at(total, rows, t)
        np.add.at(mag, rows, np.abs(t))

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        diff = y[v] - y[u]
        d2 = (diff * diff).sum(axis=1)
        coeff = -2.0 * a * b * d2 ** (b if fault == "exponent_b" else b - 1.0) / (1.0 + a * d2 ** b)
        t = (1.0 if fault == "no_factor_2" else 2.0) * clip(coeff[:, None] * diff)
        add(v, np.where((d2 > 0)[:, None], t, 0.0))
        if stats is not None:
            for key, val in (("fired", len(slot)), ("coincident_edge", int((d2 == 0).sum())),
                             ("trips", int(np.diff(g.indptr).max(initial=0) + 7) // 8)):
                stats[key] = stats.get(key, 0) + val if key != "trips" else max(stats.get(key, 0), val)
        for s in range(negative_sample_rate - (1 if fault == "drop_sample" and negative_sample_rate else 0)):
            h = counter_hash(seed, n, slot, s)
            tgt = (((h >> U64(32)) * U64(N)) >> U64(32)).astype(np.int64)
            ok = np.isfinite(y[tgt]).all(axis=1)
            if fault != "no_self_check":
                ok &= tgt != v
            diff = y[v] - y[tgt]
            d2 = (diff * diff).sum(axis=1)
            coeff = 2.0 * b / ((0.001 + d2) * (1.0 + a * d2 ** b))
            t = np.where((d2 > 0)[:, None], clip(coeff[:, None] * diff), 4.0)
            add(v[ok], t[ok])
            if stats is not None:
                for key, val in (("self_sample", int((tgt == v).sum())), ("nan_sample", int((~np.isfinite(y[tgt]).all(axis=1)).sum())),
                                 ("coincident_sample", int(((d2 == 0) & (tgt != v)).sum()))):
                    stats[key] = stats.get(key, 0) + val
    al = alpha_of(n + 1 if fault == "alpha_neighbour" else n, n_epochs, learning_rate)
    y_new = y + al * total
    return y_new, np.abs(y_new) + al * mag


def epoch_ratio(y_dev, y_ref, scale):
    """The worst |y_dev - y_ref| / (2^-24 scale) over the finite coordinates; NaN rows must be NaN on both sides."""
    y_dev = np.asarray(y_dev, dtype=F64)
    nan = np.isnan(y_ref)
    assert np.array_equal(np.isnan(y_dev), nan), "NaN positions differ"
    if nan.all():
        return 0.0
    err = np.abs(y_dev - y_ref)[~nan]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0, 0.0, err / (2.0 ** -24 * scale[~nan]))
    return float(ratio.max())


def check_epoch(y_dev, y_ref, scale, c=None):
    ratio = epoch_ratio(y_dev, y_ref, scale)
    c = EPOCH_C if c is None else c
    assert ratio <= c, f"epoch error is {ratio:.1f} x 2^-24 of (|y| + alpha sum |term|), bound {c}"
    return ratio


def layout(g, y0, n_epochs, a, b, seed=0, negative_sample_rate=5, learning_rate=1.0):
    """All epochs; positions go through fp32 between epochs as on the device."""
    y = np.asarray(y0, dtype=F32)
    for n in range(1, n_epochs + 1):
        y = epoch(g, y, n, n_epochs, a, b, seed, negative_sample_rate, learning_rate)[0].astype(F32)
    return y


# ---- graph checks
def check_graph(dev, ref):
    """dev: (indptr, indices, weights, sigma, rho) as numpy arrays from the device; ref: fuzzy_graph's Graph."""
    indptr, indices, weights, sigma, rho = dev
    assert np.array_equal(indptr, ref.indptr), "indptr"
    assert np.array_equal(indices, ref.indices), "indices"
    assert np.array_equal(rho, ref.rho), "rho"
    rel = np.abs(sigma.astype(F64) - ref.sigma) / ref.sigma
    assert rel.max(initial=0.0) <= 2.0 ** -22, f"sigma off by {rel.max():.3e} relative"
    dw = np.abs(weights.astype(F64) - ref.weights)
    assert dw.max(initial=0.0) <= 3 * 2.0 ** -23, f"weights off by {dw.max():.3e}"
    check_symmetric(indptr, indices, weights)
    return float(rel.max(initial=0.0)), float(dw.max(initial=0.0))


def check_symmetric(indptr, indices, weights):
    """Columns strictly ascending inside a row, no self loops, weights[i -> j] == weights[j -> i] bit for bit."""
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    keys = rows * n + indices
    assert (np.diff(keys) > 0).all(), "columns not ascending"
    assert (rows != indices).all(), "self loop"
    back = np.searchsorted(keys, indices.astype(np.int64) * n + rows)
    assert (back < len(keys)).all() and np.array_equal(keys[back], indices.astype(np.int64) * n + rows), "an edge lacks its reverse"
    assert np.array_equal(weights.view(np.int32), weights[back].view(np.int32)), "weights not bitwise symmetric"


# ---- quality
def _ranks_and_neighbours(X, Y, k):
    X, Y = np.asarray(X, dtype=F64), np.asarray(Y, dtype=F64)

    def sqd(Z):
        s = (Z * Z).sum(axis=1)
        D = np.maximum(s[:, None] + s[None, :] - 2.0 * Z @ Z.T, 0.0)
        np.fill_diagonal(D, np.inf)
        return D

    return np.argsort(sqd(X), axis=1, kind="stable"), np.argsort(sqd(Y), axis=1, kind="stable")[:, :k]


def trustworthiness(X, Y, k):
    """Venna & Kaski's trustworthiness of the map Y of X at k neighbours (sklearn.manifold.trustworthiness)."""
    n = len(X)
    ind_x, ind_y = _ranks_and_neighbours(X, Y, k)
    inv = np.zeros((n, n), dtype=np.int64)
    inv[np.arange(n)[:, None], ind_x] = np.arange(1, n + 1)
    ranks = inv[np.arange(n)[:, None], ind_y] - k
    return 1.0 - ranks[ranks > 0].sum() * 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))


def label_purity(Y, labels, k):
    """Mean share of a point's k nearest map neighbours that carry its label."""
    Y = np.asarray(Y, dtype=F64)
    s = (Y * Y).sum(axis=1)
    D = s[:, None] + s[None, :] - 2.0 * Y @ Y.T
    np.fill_diagonal(D, np.inf)
    nn = np.argsort(D, axis=1, kind="stable")[:, :k]
    return float((labels[nn] == labels[:, None]).mean())


def cluster_set(n, d, seed, clusters=10):
    """The quality set: ``clusters`` Gaussian clusters (centres 4 N(0, 1), unit noise) in d dimensions."""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((clusters, d))
    labels = np.arange(n) % clusters
    return (centres[labels] + rng.standard_normal((n, d))).astype(F32), labels


def knn_exact(emb, k):
    """knn_graph(emb, k, include_self=True) by float64 brute force (finite rows): idx int64, dist float32; the row itself
    first, ties by index, a tail of idx = -1, dist = +inf where k > N."""
    emb = np.asarray(emb, dtype=F64)
    n = len(emb)
    D = np.sqrt(((emb[:, None, :] - emb[None, :, :]) ** 2).sum(axis=2))
    np.fill_diagonal(D, -1.0)
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    idx = np.full((n, k), -1, dtype=np.int64)
    dist = np.full((n, k), np.inf)
    idx[:, :order.shape[1]] = order
    dist[:, :order.shape[1]] = np.take_along_axis(D, order, axis=1)
    dist[:, 0] = 0.0
    return idx, dist.astype(F32)
