"""float64 numpy restatement of the transform of btsbot_amd.layout (query_memberships / layout_transform, csrc/layout.hip,
DESIGN.md section 4o): new rows placed on a map that stays fixed.  Not a test file.

It follows the device step for step -- the bisection in float64 with sigma rounded to fp32 once, the weighted-mean start
summed in float64 in slot order, fp32 ``r = w / w_rowmax`` with the float64 firing rule, the same hash -- and differs in
the arithmetic of an epoch's terms and their sum: float64 here, fp32 (with the hardware's exp2 / log2) on the device.
``transform_epoch(..., fault=...)`` makes one seeded mistake at a time (tests/test_layout_transform_reference.py).

The sample hash, which with the text of DESIGN.md section 4o is its definition:

    rowkey  = fold over the row's slots j = 0 .. k-1, from key = 0, of
              key <- mix64(key + ((uint32(idx_j) << 32) | bits(w_j)))          (idx = -1 counts as 0xffffffff)
    h       = mix64(hash_base(seed, n) + rowkey + 64 j + s)                    (epoch n, slot j, sample s; wrapping)
    t       = ((h >> 32) * N_bank) >> 32

``w_j`` is the fp32 membership the epochs are given, a function of the row's ``idx`` and ``dist`` alone.
"""
import numpy as np

from layout_ref import F32, F64, U64, alpha_of, cluster_set, epoch_ratio, hash_base, mix64  # noqa: F401 (re-exported)

# |y_dev - y_ref| <= TRANSFORM_C * 2^-24 * (|y_ref| + alpha * sum |term|) per coordinate, one epoch at a time.
# TRANSFORM_MEASURED is the worst ratio measured on an MI355X over every case of tests/test_gpu_layout_transform.py
# against this restatement (bank 512, Q = 130, k = 15; 4.46 at bank 300, k = 64; 1.65 / 1.29 / 0.86 on the three small
# cases); TRANSFORM_C is 8 x that, rounded up to a power of two, and may not exceed the limit the fault test is stated at.
TRANSFORM_MEASURED = 4.51
TRANSFORM_C = 64.0
TRANSFORM_C_LIMIT = 256.0
FAULTS = ("drop_sample", "no_clip", "alpha_neighbour", "exponent_b", "fire_fp32", "factor_2_kept", "global_wmax",
          "alpha_not_quartered")


# ---- step 1
def query_memberships(idx, dist):
    """(w float32 [Q, k], sigma float32 [Q]) of idx int64 [Q, k], dist float32 [Q, k]: no self column, rho = 0, the floor
    of sigma from the row's own mean distance."""
    idx, dist = np.asarray(idx), np.asarray(dist, dtype=F32)
    q, k = idx.shape
    nb = idx >= 0
    x = np.where(nb, dist.astype(F64), 0.0)
    target = np.log2(float(k))
    lo, hi, mid = np.zeros(q), np.full(q, np.inf), np.ones(q)
    done = np.zeros(q, dtype=bool)
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
    cnt = nb.sum(axis=1)
    mid = np.maximum(mid, np.where(cnt > 0, 1e-3 * (x.sum(axis=1) / np.maximum(cnt, 1)), 0.0))
    sigma = mid.astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.where(nb, np.where(x > 0, np.exp(-(x / sigma.astype(F64)[:, None])), 1.0), 0.0).astype(F32)
    return w, sigma


# ---- step 2
def init_positions(idx, w, Y):
    """sum_j w_j Y[idx_j] / sum_j w_j in float64, slot after slot, rounded once: float32 [Q, 2]; NaN without a slot."""
    idx, w, Y = np.asarray(idx), np.asarray(w, dtype=F32).astype(F64), np.asarray(Y, dtype=F32).astype(F64)
    q, k = idx.shape
    sw, s = np.zeros(q), np.zeros((q, 2))
    for j in range(k):
        pres = (idx[:, j] >= 0) & (idx[:, j] < len(Y))
        u = np.where(pres, idx[:, j], 0)
        sw = sw + np.where(pres, w[:, j], 0.0)
        with np.errstate(invalid="ignore"):
            s = s + np.where(pres[:, None], w[:, j, None] * Y[u], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (s / sw[:, None]).astype(F32)


# ---- step 3
def rowkey(idx, w):
    idx, w = np.asarray(idx, dtype=np.int64), np.ascontiguousarray(w, dtype=F32)
    key = np.zeros(idx.shape[0], dtype=U64)
    bits = w.view(np.uint32).astype(U64)
    hi = (idx & np.int64(0xFFFFFFFF)).astype(U64) << U64(32)
    with np.errstate(over="ignore"):
        for j in range(idx.shape[1]):
            key = mix64(key + (hi[:, j] | bits[:, j]))
    return key


def transform_epoch(idx, w, Y, y, n, n_epochs, a, b, seed=0, negative_sample_rate=5, learning_rate=1.0, fault=None,
                    stats=None):
    """Epoch ``n`` of the schedule for the queries at ``y`` (float32 [Q, 2]) against the fixed positions ``Y`` (float32
    [N, 2]), in float64.  Returns (y_new float64 [Q, 2], scale float64 [Q, 2]) with scale = |y_new| + alpha_n * sum
    |term|.  stats (a dict): counts of the special events met are added to it."""
    assert fault is None or fault in FAULTS
    idx, w = np.asarray(idx, dtype=np.int64), np.asarray(w, dtype=F32)
    Y = np.asarray(Y, dtype=F32).astype(F64)
    y = np.asarray(y, dtype=F32).astype(F64)
    Q, k = idx.shape
    N = len(Y)
    a, b = float(F32(a)), float(F32(b))
    pres = (idx >= 0) & (idx < N)
    wmax = np.full(Q, w.max(initial=F32(0)), dtype=F32) if fault == "global_wmax" else w.max(axis=1, initial=F32(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        r32 = np.where(pres, w / wmax[:, None], F32(0)).astype(F32)
        if fault == "fire_fp32":
            fire = np.floor(F32(n) * r32) > np.floor(F32(n - 1) * r32)
        else:
            fire = np.floor(n * r32.astype(F64)) > np.floor((n - 1) * r32.astype(F64))
    v, j = np.nonzero(fire)
    u = idx[v, j]
    total, mag = np.zeros((Q, 2)), np.zeros((Q, 2))

    def clip(t):
        return t if fault == "no_clip" else np.clip(t, -4.0, 4.0)

    def add(rows, t):
        np.add.at(total, rows, t)
        np.add.at(mag, rows, np.abs(t))

    def count(key, val):
        if stats is not None:
            stats[key] = stats.get(key, 0) + int(val)

    key = rowkey(idx, w)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        diff = y[v] - Y[u]
        d2 = (diff * diff).sum(axis=1)
        coeff = -2.0 * a * b * d2 ** (b if fault == "exponent_b" else b - 1.0) / (1.0 + a * d2 ** b)
        t = (2.0 if fault == "factor_2_kept" else 1.0) * clip(coeff[:, None] * diff)      # one end moves: no factor 2
        add(v, np.where((d2 > 0)[:, None], t, 0.0))
        count("fired", len(v))
        count("coincident_neighbour", (d2 == 0).sum())
        count("clipped", (np.abs(coeff[:, None] * diff) > 4.0).any(axis=1).sum())
        base = hash_base(seed, n) + key[v] + U64(64) * j.astype(U64)
        for s in range(negative_sample_rate - (1 if fault == "drop_sample" and negative_sample_rate else 0)):
            h = mix64(base + U64(s))
            tgt = (((h >> U64(32)) * U64(N)) >> U64(32)).astype(np.int64)
            ok = np.isfinite(Y[tgt]).all(axis=1)
            diff = y[v] - Y[tgt]
            d2 = (diff * diff).sum(axis=1)
            coeff = 2.0 * b / ((0.001 + d2) * (1.0 + a * d2 ** b))
            t = np.where((d2 > 0)[:, None], clip(coeff[:, None] * diff), 4.0)
            add(v[ok], t[ok])
            count("nan_sample", (~ok).sum())
            count("coincident_sample", ((d2 == 0) & ok).sum())
            count("clipped", ((np.abs(coeff[:, None] * diff) > 4.0).any(axis=1) & ok).sum())
    al = alpha_of(n + 1 if fault == "alpha_neighbour" else n, n_epochs,
                  float(learning_rate) / (1.0 if fault == "alpha_not_quartered" else 4.0))
    y_new = y + al * total
    return y_new, np.abs(y_new) + al * mag


def transform(idx, dist, Y, n_epochs, a, b, seed=0, negative_sample_rate=5, learning_rate=1.0, y0=None, first_epoch=1,
              last_epoch=None):
    """layout_transform: memberships, the start (unless y0), then the epochs; positions go through fp32 between epochs
    as on the device.  float32 [Q, 2]."""
    w, _ = query_memberships(idx, dist)
    y = init_positions(idx, w, Y) if y0 is None else np.asarray(y0, dtype=F32)
    for n in range(first_epoch, (n_epochs if last_epoch is None else last_epoch) + 1):
        y = transform_epoch(idx, w, Y, y, n, n_epochs, a, b, seed, negative_sample_rate, learning_rate)[0].astype(F32)
    return y


# ---- the cluster case and its score
def knn_query(queries, bank, k):
    """EmbeddingIndex.query by float64 brute force: idx int64 [Q, k], dist float32 [Q, k]; ordered by (dist, index);
    non-finite bank rows are never returned, a non-finite query gets idx = -1, dist = NaN; tails of -1 / +inf."""
    queries, bank = np.asarray(queries, dtype=F64), np.asarray(bank, dtype=F64)
    ok = np.isfinite(bank).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        D = np.sqrt(((queries[:, None, :] - bank[None, :, :]) ** 2).sum(axis=2)).astype(F32)
    D[:, ~ok] = np.inf
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    idx = np.full((len(queries), k), -1, dtype=np.int64)
    dist = np.full((len(queries), k), np.inf, dtype=F32)
    idx[:, :order.shape[1]] = order
    dist[:, :order.shape[1]] = np.take_along_axis(D, order, axis=1)
    idx[~np.isfinite(dist)] = -1
    bad = ~np.isfinite(queries).all(axis=1)
    idx[bad], dist[bad] = -1, np.nan
    return idx, dist


def query_purity(y, labels, Y, bank_labels, k=5):
    """Mean share of a query's k nearest BANK map points that carry its label."""
    y, Y = np.asarray(y, dtype=F64), np.asarray(Y, dtype=F64)
    D = ((y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    nn = np.argsort(D, axis=1, kind="stable")[:, :k]
    return float((bank_labels[nn] == labels[:, None]).mean())


def split_cluster_set(seed, n_bank=512, n_query=130, d=32):
    """cluster_set(n_bank + n_query, d, seed): the first n_bank rows are the bank, the rest the fresh draws."""
    X, labels = cluster_set(n_bank + n_query, d, seed)
    return X[:n_bank], labels[:n_bank], X[n_bank:], labels[n_bank:]
