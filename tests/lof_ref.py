"""float64 numpy restatement of btsbot_amd.novelty (csrc/lof.hip), a brute-force kNN with optional
groups, and the sets the novelty tests share (no GPU).

The definition, on idx int64 [rows, k] and dist fp32 [rows, k] (converted to float64 once).  An entry (row, c) is PRESENT
when 0 <= idx[row, c] < n (n: the rows kdist / lrd are held for); a -1 tail is no entry, an index out of range neither.
m(row) = the number of present entries.
  kdist(i)    = dist of row i's last present column                                  NaN when m = 0
  reach(i, c) = fmax(dist[i, c], kdist(idx[i, c]))      (a NaN kdist leaves dist)
  lrd(i)      = 1 / (sum_c reach(i, c) / m + 1e-10)                                  NaN when m = 0
  lof(i)      = (sum_c lrd(idx[i, c]) / lrd(i)) / m     (each quotient first)        NaN when m = 0

The order of a row's sum, the kernel's (``tree_sum``): W slots, W = 16, 32 or 64 the smallest that holds k; slot c holds
column c's term where the entry is present and +0.0 otherwise (absent entries, c >= k); for o = W/2, W/4, ..., 1 every
slot takes v[c] + v[c ^ o] at once (the butterfly of a group of W lanes); the sum is slot 0.  numpy's float64 ``+`` and
``/`` are the IEEE operations the kernel uses, and there is no product in front of a sum that could fuse, so the
restatement is bit for bit what the device must give.
"""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
EPS = 1e-10          # scikit-learn's constant in lrd


def lanes_for(k):
    return 16 if k <= 16 else 32 if k <= 32 else 64


def tree_sum(terms, present):
    """float64 [rows]: the sums of terms [rows, k] over the present entries in the kernel's order."""
    rows, k = terms.shape
    w = lanes_for(k)
    v = np.zeros((rows, w), F64)
    v[:, :k] = np.where(present, terms, 0.0)
    lanes = np.arange(w)
    o = w // 2
    with np.errstate(invalid="ignore", over="ignore"):
        while o >= 1:
            v = v + v[:, lanes ^ o]
            o //= 2
    return v[:, 0]


def _entries(idx, dist, n):
    idx = np.asarray(idx, np.int64)
    d = np.asarray(dist, F32).astype(F64)
    present = (idx >= 0) & (idx < n)
    return idx, d, present, present.sum(axis=1)


def kdist_of(idx, dist, n=None):
    idx = np.asarray(idx, np.int64)
    idx, d, present, m = _entries(idx, dist, idx.shape[0] if n is None else n)
    k = idx.shape[1]
    last = np.where(present, np.arange(k)[None, :], -1).max(axis=1) if k else np.full(idx.shape[0], -1)
    out = np.full(idx.shape[0], np.nan)
    has = last >= 0
    out[has] = d[np.flatnonzero(has), last[has]]
    return out


def _lrd(idx, d, present, m, bank_kdist):
    j = np.where(present, idx, 0)
    kd = bank_kdist[j] if len(bank_kdist) else np.zeros(idx.shape)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = tree_sum(np.fmax(d, kd), present)
        return np.where(m > 0, 1.0 / (s / np.maximum(m, 1).astype(F64) + EPS), np.nan)


def _lof(idx, present, m, bank_lrd, own):
    j = np.where(present, idx, 0)
    lj = bank_lrd[j] if len(bank_lrd) else np.zeros(idx.shape)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = tree_sum(lj / own[:, None], present)
        return np.where(m > 0, s / np.maximum(m, 1).astype(F64), np.nan)


def lof_fit(idx, dist):
    """(kdist, lrd, lof), float64 [n] each, of the graph of a bank among itself."""
    idx, d, present, m = _entries(idx, dist, np.asarray(idx).shape[0])
    kdist = kdist_of(idx, dist)
    lrd = _lrd(idx, d, present, m, kdist)
    return kdist, lrd, _lof(idx, present, m, lrd, lrd)


def lof_score(idx, dist, kdist, lrd):
    """(lrd, lof), float64 [q] each, of new rows against a bank fitted to (kdist, lrd)."""
    kdist, lrd = np.asarray(kdist, F64), np.asarray(lrd, F64)
    idx, d, present, m = _entries(idx, dist, len(kdist))
    own = _lrd(idx, d, present, m, kdist)
    return own, _lof(idx, present, m, lrd, own)


# ---------------------------------------------------------------------------------------------------------------------
# brute-force neighbours
def distances64(q, b):
    """float64 [Q, N] Euclidean distances in the direct form"""
    q, b = np.asarray(q, F64), np.asarray(b, F64)
    return np.sqrt(((q[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))


def distances32(q, b):
    """the device's direct form emulated in fp32: fp32 differences, squares and sums, one fp32 root (the order of the
    sum is numpy's, not the wave's: (D + 2) / 2 roundings relative either way)"""
    q, b = np.asarray(q, F32), np.asarray(b, F32)
    t = q[:, None, :] - b[None, :, :]
    return np.sqrt((t * t).sum(axis=2, dtype=F32), dtype=F32)


def knn(d, k, self_offset=-1, qgroups=None, bgroups=None, finite_q=None, finite_b=None):
    """(idx int64 [Q, k], dist fp32 [Q, k]) from a distance matrix d [Q, N]: the k smallest by (dist, index) among the
    eligible columns (not q + self_offset, not of the row's group, finite), the tail -1 / +inf; a non-finite query row
    -1 / NaN."""
    nq, n = d.shape
    el = np.ones((nq, n), bool)
    if self_offset >= 0:
        r = np.arange(nq)
        ok = r + self_offset < n
        el[r[ok], r[ok] + self_offset] = False
    if qgroups is not None:
        el &= np.asarray(qgroups)[:, None] != np.asarray(bgroups)[None, :]
    if finite_b is not None:
        el &= np.asarray(finite_b)[None, :]
    idx = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, F32)
    for i in range(nq):
        if finite_q is not None and not finite_q[i]:
            dist[i] = np.nan
            continue
        cols = np.flatnonzero(el[i])
        order = cols[np.lexsort((cols, d[i, cols]))][:k]
        idx[i, :len(order)] = order
        dist[i, :len(order)] = d[i, order]
    return idx, dist


def knn64(d, k, **kw):
    """as ``knn`` but the distances stay float64 (what the scikit-learn comparison in float64 needs)"""
    idx, _ = knn(d, k, **kw)
    dist = np.where(idx >= 0, np.take_along_axis(d, np.maximum(idx, 0), axis=1), np.inf)
    return idx, dist


def lof_fit64(idx, dist64):
    """``lof_fit`` on float64 distances (no rounding to fp32): the restatement as scikit-learn sees the data"""
    idx = np.asarray(idx, np.int64)
    n = idx.shape[0]
    present = (idx >= 0) & (idx < n)
    m = present.sum(axis=1)
    d = np.asarray(dist64, F64)
    last = np.where(present, np.arange(idx.shape[1])[None, :], -1).max(axis=1)
    kdist = np.where(last >= 0, d[np.arange(n), np.maximum(last, 0)], np.nan)
    lrd = _lrd(idx, d, present, m, kdist)
    return kdist, lrd, _lof(idx, present, m, lrd, lrd)


def lof_score64(idx, dist64, kdist, lrd):
    idx = np.asarray(idx, np.int64)
    present = (idx >= 0) & (idx < len(kdist))
    m = present.sum(axis=1)
    own = _lrd(idx, np.asarray(dist64, F64), present, m, kdist)
    return own, _lof(idx, present, m, lrd, own)


# ---------------------------------------------------------------------------------------------------------------------
# the sets
def perturbed_draws(x, seed, q=130, scale=0.3):
    """q new rows: rows of x drawn with replacement plus N(0, scale)"""
    rng = np.random.default_rng(1000 + seed)
    rows = rng.integers(0, x.shape[0], size=q)
    return (x[rows] + rng.normal(0, scale, size=(q, x.shape[1]))).astype(F32)


def masking_set(seed, objects=128, epochs=5, planted=3):
    """(X fp32 [objects * epochs, 32], obj int64, planted bool): an archive of multi-epoch objects.  Object centres are
    centres[i % 10] + N(0, 0.95) in 32-D (ten clusters, centres N(0, 3)); the first ``planted`` objects are re-drawn as
    4 * N(0, 3): far from every cluster; an alert is its object's centre + N(0, 1e-3); the rows are permuted."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 3.0, size=(10, 32))
    oc = centres[np.arange(objects) % 10] + rng.normal(0, 0.95, size=(objects, 32))
    oc[:planted] = 4.0 * rng.normal(0, 3.0, size=(planted, 32))
    obj = np.repeat(np.arange(objects), epochs)
    x = oc[obj] + rng.normal(0, 1e-3, size=(objects * epochs, 32))
    perm = rng.permutation(objects * epochs)
    obj = obj[perm].astype(np.int64)
    return x[perm].astype(F32), obj, obj < planted


# relative bound of the fp32 direct form on a LOF: a ratio of means of ratios of distances, each carrying at most
# (D + 2) / 2 fp32 roundings, twice over
def fp32_bound(dim):
    return 4 * (dim + 2) * U
