"""What the cluster-prediction tests share (no GPU): DESIGN.md section 4w restated in numpy float64 on top of
tests/hdbscan_ref.py.

    t = tables(condensed, n, method="eom", allow_single_cluster=False)     the per-row and per-cluster tables, GLOSH
    lam_zero = lam_zero_of(weights)                                        1 / the smallest positive tree weight (or 1)
    out = predict(Dq, core, t, lam_zero, min_samples, eligible=None)       per query row
    ok = resolved(Dq, core, min_samples, k_s, slack=None, squared=False, rel=0.0, eligible=None)

``condensed`` = (parent, child, lam, size) in the canonical order of ``btsbot_hdbscan_tree``; cluster ``c`` of the tables
is condensed id ``n + c``.  ``Dq`` float64 [Q, N] holds fp32 distances (NaN towards a non-finite bank row, a NaN row for a
non-finite query), ``core`` the bank's core distances (NaN for a non-finite row), ``eligible`` bool [Q, N] the rows a
query may see (None: all).  Weights are fp32 values and ``max`` is exact, so ``w`` is computed in float64 without error;
``1 / w``, ``min``, the division and the subtraction are single float64 operations, as on the device.
"""
import numpy as np

import hdbscan_ref as R  # noqa: F401  (the sets and the tree the tables are made of)


def lam_zero_of(weights):
    w = np.asarray(weights, np.float64)
    pos = w[w > 0]
    return 1.0 / pos.min() if len(pos) else 1.0


def tables(condensed, n, method="eom", allow_single_cluster=False):
    parent_, child_, lam_, size_ = condensed
    nc = int(max(parent_.max(), child_.max())) - n + 1 if len(parent_) else 0
    birth, par = np.zeros(nc), np.full(nc, -1, np.int64)
    row_sum, child_sum, max_lam = np.zeros(nc), np.zeros(nc), np.zeros(nc)
    kids = [[] for _ in range(nc)]
    fell, lam_row = np.full(n, -1, np.int64), np.zeros(n)
    for p, ch, lam, s in zip(parent_.tolist(), child_.tolist(), lam_.tolist(), size_.tolist()):
        if ch >= n:
            birth[ch - n], par[ch - n] = lam, p - n
    for p, ch, lam, s in zip(parent_.tolist(), child_.tolist(), lam_.tolist(), size_.tolist()):
        c = p - n
        max_lam[c] = max(max_lam[c], lam)
        if ch < n:
            row_sum[c] = row_sum[c] + (lam - birth[c])
            fell[ch], lam_row[ch] = c, lam
        else:
            child_sum[c] = child_sum[c] + s * (lam - birth[c])
            kids[c].append(ch - n)
    stab = row_sum + child_sum
    flag, best = np.zeros(nc, bool), np.zeros(nc)
    for c in range(nc - 1, -1, -1):
        if method == "leaf":
            flag[c] = not kids[c]
        elif not kids[c]:
            flag[c], best[c] = True, stab[c]
        else:
            s = 0.0
            for k in kids[c]:
                s = s + best[k]
            flag[c], best[c] = (False, s) if s > stab[c] else (True, stab[c])
    if nc and not allow_single_cluster:
        flag[0] = False
    sel = np.full(nc, -1, np.int64)
    for c in range(nc):
        up = sel[par[c]] if par[c] >= 0 else -1
        sel[c] = up if up >= 0 else (c if flag[c] else -1)
    number = {c: i for i, c in enumerate(sorted(set(sel[sel >= 0].tolist())))}
    label = np.array([number[s] if s >= 0 else -1 for s in sel.tolist()], np.int64).reshape(nc)
    max_lambda = np.array([max_lam[s] if s >= 0 else 0.0 for s in sel.tolist()], np.float64).reshape(nc)
    death = max_lam.copy()
    for c in range(nc - 1, 0, -1):
        death[par[c]] = max(death[par[c]], death[c])
    outlier = np.full(n, np.nan)
    for r in range(n):
        if fell[r] >= 0:
            d = death[fell[r]]
            outlier[r] = 0.0 if d == 0 else 1.0 - lam_row[r] / d
    return dict(row_cluster=fell, row_lambda=lam_row, outlier=outlier, parent=par, birth=birth, label=label,
                max_lambda=max_lambda, death=death)


def labels_from(t):
    """(labels, prob) of the fitted rows rebuilt from the tables"""
    n = len(t["row_cluster"])
    labels, prob = np.full(n, -1, np.int64), np.zeros(n)
    for r in range(n):
        c = t["row_cluster"][r]
        if c < 0 or t["label"][c] < 0:
            continue
        m = t["max_lambda"][c]
        labels[r] = t["label"][c]
        prob[r] = 1.0 if m == 0 else min(t["row_lambda"][r], m) / m
    return labels, prob


def _seen(Dq, core, eligible, i):
    ok = ~np.isnan(Dq[i]) & ~np.isnan(core)
    return ok if eligible is None else ok & eligible[i]


def query_core(d_sorted, min_samples):
    k = min_samples - 1
    return 0.0 if k == 0 else (d_sorted[k - 1] if len(d_sorted) >= k else np.inf)


def predict(Dq, core, t, lam_zero, min_samples, eligible=None):
    Q = Dq.shape[0]
    out = dict(label=np.full(Q, -1, np.int64), prob=np.zeros(Q), outlier=np.ones(Q), neighbor=np.full(Q, -1, np.int64),
               lam=np.zeros(Q), cluster=np.full(Q, -1, np.int64), w=np.full(Q, np.inf), core=np.full(Q, np.inf))
    for i in range(Q):
        if np.isnan(Dq[i]).all():                       # a non-finite query row
            out["outlier"][i] = out["lam"][i] = out["w"][i] = out["core"][i] = np.nan
            continue
        ok = _seen(Dq, core, eligible, i)
        at = np.flatnonzero(ok)
        cq = query_core(np.sort(Dq[i, at]), min_samples)
        out["core"][i] = cq
        if not len(at) or np.isinf(cq):
            continue
        w = np.maximum(np.maximum(Dq[i, at], cq), np.maximum(core[at], 0.0))
        b = int(at[np.flatnonzero(w == w.min())[0]])    # the smallest (w, index)
        wq = float(w.min())
        lam = lam_zero if wq == 0 else 1.0 / wq
        c = int(t["row_cluster"][b])
        if t["row_lambda"][b] > lam:
            while t["parent"][c] >= 0 and t["birth"][c] >= lam:
                c = int(t["parent"][c])
        lab, m, d = int(t["label"][c]), t["max_lambda"][c], t["death"][c]
        out["label"][i] = lab
        out["prob"][i] = 0.0 if lab < 0 else (1.0 if m == 0 else min(lam, m) / m)
        out["outlier"][i] = 0.0 if d == 0 else 1.0 - min(lam, d) / d
        out["neighbor"][i], out["lam"][i], out["cluster"][i], out["w"][i] = b, lam, c, wq
    return out


def resolved(Dq, core, min_samples, k_s, slack=None, squared=False, rel=0.0, eligible=None):
    """bool [Q]: the list of the ``k_s`` nearest eligible rows proves its lightest entry the smallest (w, index) of all --
    the list is not full, or w_best < floor STRICTLY.  slack: float [Q] or None, as ``btsbot_cluster_offer_knn`` takes
    it.  (A row without a neighbour counts as resolved: there is nothing to ask again.)"""
    Q = Dq.shape[0]
    out = np.ones(Q, bool)
    for i in range(Q):
        at = np.flatnonzero(_seen(Dq, core, eligible, i))
        if len(at) < k_s:
            continue
        order = at[np.lexsort((at, Dq[i, at]))][:k_s]
        d = Dq[i, order]
        cq = query_core(d, min_samples)
        w_best = np.maximum(np.maximum(d, cq), np.maximum(core[order], 0.0)).min()
        floor = float(d[-1])
        if slack is not None:
            s = float(slack[i])
            floor = np.sqrt(max(floor * floor - s, 0.0)) if squared else floor - s
        floor *= 1.0 - rel
        out[i] = w_best < floor
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the sets
def blobs_32d_parts(seed, dim=32, sizes=(40, 50, 60, 70, 80), far=12):
    """(X, origin int64 [N], centres, spreads) of ``hdbscan_ref.blobs_32d(seed)``: the same draws replayed, so that a row's
    blob (-1: one of the far rows) and the blobs' centres are known"""
    rng = np.random.default_rng(100 + seed)
    centres = rng.normal(0, 4.0, size=(len(sizes), dim))
    spreads = [0.5 + 0.25 * i for i in range(len(sizes))]
    parts = [c + rng.normal(0, s, size=(m, dim)) for c, s, m in zip(centres, spreads, sizes)]
    parts.append(rng.normal(0, 12.0, size=(far, dim)))
    origin = np.concatenate([np.full(m, i) for i, m in enumerate(sizes)] + [np.full(far, -1)])
    perm = rng.permutation(len(origin))
    x = np.concatenate(parts)[perm].astype(R.F32)
    assert np.array_equal(x, R.blobs_32d(seed, dim, sizes, far), equal_nan=True)
    return x, origin[perm], centres, spreads


def fresh_draws(seed, per_blob=30, far=10):
    """(queries fp32 [5 * per_blob + far, 32], origin): new rows from the blobs of ``blobs_32d(seed)``, then rows far from
    all of them (origin -1)"""
    _, _, centres, spreads = blobs_32d_parts(seed)
    rng = np.random.default_rng(1000 + seed)
    parts = [c + rng.normal(0, s, size=(per_blob, centres.shape[1])) for c, s in zip(centres, spreads)]
    parts.append(rng.normal(0, 60.0, size=(far, centres.shape[1])))
    origin = np.concatenate([np.full(per_blob, i) for i in range(len(centres))] + [np.full(far, -1)])
    return np.concatenate(parts).astype(R.F32), origin


def jittered_rows(x, seed=9, count=200, scale=1e-3):
    """``count`` rows of ``x`` (without repetition) plus a jitter of ``scale``"""
    rng = np.random.default_rng(seed)
    rows = rng.choice(len(x), size=count, replace=False)
    return (x[rows] + rng.normal(0, scale, size=(count, x.shape[1]))).astype(R.F32)


def cross_dist(Q, X, metric="euclidean"):
    """float64 [Q, N]: ``hdbscan_ref.dist_matrix``'s distances (float64 direct form, rounded to fp32 once) from the rows of
    ``Q`` to the rows of ``X``; NaN where either row is not finite"""
    from knn_ref import direct64, finite_rows
    Q, X = np.asarray(Q, R.F32), np.asarray(X, R.F32)
    out = np.full((len(Q), len(X)), np.nan)
    fx = np.flatnonzero(finite_rows(X))
    for i in np.flatnonzero(finite_rows(Q)):
        d = direct64(Q[i], X[fx], metric)
        out[i, fx] = (np.sqrt(d) if metric == "euclidean" else d).astype(R.F32)
    return out
