"""What the HDBSCAN tests share (no GPU): DESIGN.md section 4v restated in numpy float64 from a distance matrix, and the
seeded sets.

    D = dist_matrix(X)                      float64 [N, N]: the float64 direct-form distance of the fp32 rows, rounded to
                                            fp32 once (NaN for a non-finite row)
    core, W = mutual_reachability(D, min_samples, groups=None)
    edges, weights = mst(W)                 dense Prim over the finite rows; tie="last" builds another valid tree
    out = tree(edges, weights, n, min_cluster_size, method="eom", allow_single_cluster=False)
    out = hdbscan_ref(D, min_cluster_size, min_samples, ...)        all of the above

The hierarchy is the tie-invariant one: all tree edges of one weight are applied at once and every set of old components
they join becomes ONE node with two or more children.  ``out`` holds ``labels`` int64 [N], ``prob`` float64 [N] and
``condensed`` = (parent, child, lam, size) in the canonical order of ``btsbot_hdbscan_tree``:

* clusters are numbered n, n + 1, ... by (smallest row, size descending): the root is n, a parent comes before its children,
  siblings stand in the order of their smallest rows;
* a row's entry is (the cluster it fell out of, the row, the lambda it fell out at, 1), a cluster's (its parent, the
  cluster, the lambda of the split, its size); the entries are sorted by (parent, child), rows (< n) before clusters.

The float64 sums are sequential in that order: a cluster's rows ascending, then -- a second sum -- its child clusters
ascending; stability = row sum + child sum.
"""
import numpy as np

from knn_ref import U, direct64, finite_rows

F32 = np.float32
PAIRS = ((10, 5), (15, 15), (5, 10))     # (min_cluster_size, min_samples)


# ---------------------------------------------------------------------------------------------------------------------
# distances, core distances, the spanning tree
def dist_matrix(X, metric="euclidean"):
    X = np.asarray(X, F32)
    n = X.shape[0]
    fin = finite_rows(X)
    with np.errstate(over="ignore", invalid="ignore"):
        fin &= np.isfinite((X.astype(np.float64) ** 2).sum(1).astype(F32))
    D = np.full((n, n), np.nan)
    at = np.flatnonzero(fin)
    for i in at:
        d = direct64(X[i], X[at], metric)
        D[i, at] = (np.sqrt(d) if metric == "euclidean" else d).astype(F32)
    return D


def mutual_reachability(D, min_samples, groups=None):
    """(core float64 [N] -- NaN for a non-finite row --, W float64 [N, N] = max(D, core_a, core_b), NaN off the finite
    rows).  core(i): the distance to the (min_samples - 1)-th nearest OTHER finite row (of another group, with groups),
    0 for min_samples = 1, +inf where there are fewer."""
    n = D.shape[0]
    fin = ~np.isnan(np.diag(D))
    core = np.full(n, np.nan)
    for i in np.flatnonzero(fin):
        ok = fin.copy()
        ok[i] = False
        if groups is not None:
            ok &= np.asarray(groups) != groups[i]
        d = np.sort(D[i, ok])
        k = min_samples - 1
        core[i] = 0.0 if k == 0 else (d[k - 1] if len(d) >= k else np.inf)
    W = np.maximum(D, np.maximum(core[:, None], core[None, :]))
    W[~fin, :] = np.nan
    W[:, ~fin] = np.nan
    return core, W


def mst(W, tie="first"):
    """(edges int64 [m, 2], weights float64 [m]) of a minimum spanning tree of the finite rows of W (dense Prim from
    the first finite row).  tie: which of several equally light candidates joins -- ``"first"`` or ``"last"`` by row --,
    so that the two calls give different trees wherever weights tie."""
    fin = np.flatnonzero(~np.isnan(np.diag(W)))
    m = len(fin)
    if m < 2:
        return np.zeros((0, 2), np.int64), np.zeros(0)
    Wf = W[np.ix_(fin, fin)]
    inside = np.zeros(m, bool)
    inside[0] = True
    best = Wf[0].copy()
    frm = np.zeros(m, np.int64)
    edges, weights = [], []
    for _ in range(m - 1):
        cand = np.where(inside, np.inf, best)
        lo = cand.min()
        if np.isinf(lo):                                   # only +inf weights are left
            j = int(np.flatnonzero(~inside)[0])
        else:
            hits = np.flatnonzero(cand == lo)
            j = int(hits[0] if tie == "first" else hits[-1])
        inside[j] = True
        edges.append((fin[frm[j]], fin[j]))
        weights.append(cand[j])
        upd = (Wf[j] <= best) if tie == "last" else (Wf[j] < best)
        upd &= ~inside
        best[upd] = Wf[j][upd]
        frm[upd] = j
    return np.array(edges, np.int64), np.array(weights, np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the hierarchy, the condensed tree, the selection
def _hierarchy(edges, weights, n):
    """nodes: rows 0..n-1 are leaves; internal node v >= n has w[v], children[v], size[v], minrow[v].  Returns the root."""
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    node_of = list(range(n))
    w, children = {}, {}
    size = {i: 1 for i in range(n)}
    minrow = {i: i for i in range(n)}
    nxt = n
    order = np.argsort(weights, kind="stable")
    at = 0
    while at < len(order):
        end = at
        while end < len(order) and weights[order[end]] == weights[order[at]]:
            end += 1
        olds = {}
        pairs = []
        for e in order[at:end]:
            ra, rb = find(edges[e, 0]), find(edges[e, 1])
            olds[ra], olds[rb] = node_of[ra], node_of[rb]
            pairs.append((ra, rb))
        for ra, rb in pairs:
            ra, rb = find(ra), find(rb)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        fresh = {}
        for r_old, node in olds.items():
            r = find(r_old)
            if r not in fresh:
                fresh[r] = nxt
                w[nxt], children[nxt], size[nxt], minrow[nxt] = float(weights[order[at]]), [], 0, n
                nxt += 1
            v = fresh[r]
            children[v].append(node)
            size[v] += size[node]
            minrow[v] = min(minrow[v], minrow[node])
        for r, v in fresh.items():
            assert len(children[v]) >= 2
            node_of[r] = v
        at = end
    return nxt - 1, w, children, size, minrow


def _rows_under(v, n, children):
    out, stack = [], [v]
    while stack:
        x = stack.pop()
        if x < n:
            out.append(x)
        else:
            stack.extend(children[x])
    return out


def tree(edges, weights, n, min_cluster_size, method="eom", allow_single_cluster=False):
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    weights = np.asarray(weights, np.float64)
    labels = np.full(n, -1, np.int64)
    prob = np.zeros(n)
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64))
    if len(edges) == 0:
        return dict(labels=labels, prob=prob, condensed=empty)
    root, w, children, size, minrow = _hierarchy(edges, weights, n)
    assert size[root] == len(edges) + 1, "the edges are not a spanning tree of the rows they name"
    pos = weights[weights > 0]
    lam_zero = 1.0 / pos.min() if len(pos) else 1.0

    def lam_of(v):
        return lam_zero if w[v] == 0 else 1.0 / w[v]

    # clusters in discovery order: [minrow, size, birth, parent]; entries (parent, child row or ("c", cluster), lam, size)
    clusters = [[minrow[root], size[root], 0.0, -1]]
    entries = []
    stack = [(root, 0)]
    while stack:
        v, c = stack.pop()
        lam = lam_of(v)
        real = [x for x in children[v] if size[x] >= min_cluster_size]
        for x in children[v]:
            if size[x] >= min_cluster_size:
                continue
            for r in _rows_under(x, n, children):
                entries.append((c, r, lam, 1))
        if len(real) == 1:
            stack.append((real[0], c))
        elif len(real) >= 2:
            for x in real:
                clusters.append([minrow[x], size[x], lam, c])
                entries.append((c, ("c", len(clusters) - 1), lam, size[x]))
                stack.append((x, len(clusters) - 1))
    # canonical numbering
    rank = sorted(range(len(clusters)), key=lambda k: (clusters[k][0], -clusters[k][1]))
    new_id = {k: n + i for i, k in enumerate(rank)}
    cond = sorted((new_id[p], ch if not isinstance(ch, tuple) else new_id[ch[1]], lam, s) for p, ch, lam, s in entries)
    nc = len(clusters)
    birth = np.zeros(nc)
    par = np.full(nc, -1, np.int64)
    for k, (_mr, _s, b, p) in enumerate(clusters):
        birth[new_id[k] - n] = b
        par[new_id[k] - n] = -1 if p < 0 else new_id[p] - n
    row_sum, child_sum, max_lam = np.zeros(nc), np.zeros(nc), np.zeros(nc)
    kids = [[] for _ in range(nc)]
    fell = np.full(n, -1, np.int64)
    lam_row = np.zeros(n)
    for p, ch, lam, s in cond:
        c = p - n
        max_lam[c] = max(max_lam[c], lam)
        if ch < n:
            row_sum[c] = row_sum[c] + (lam - birth[c])
            fell[ch], lam_row[ch] = c, lam
        else:
            child_sum[c] = child_sum[c] + s * (lam - birth[c])
            kids[c].append(ch - n)
    stab = row_sum + child_sum
    flag = np.zeros(nc, bool)
    if method == "leaf":
        for c in range(nc):
            flag[c] = not kids[c]
    else:
        best = np.zeros(nc)
        for c in range(nc - 1, -1, -1):
            if not kids[c]:
                flag[c], best[c] = True, stab[c]
                continue
            s = 0.0
            for k in kids[c]:
                s = s + best[k]
            if s > stab[c]:
                flag[c], best[c] = False, s
            else:
                flag[c], best[c] = True, stab[c]
    if not allow_single_cluster:
        flag[0] = False
    sel = np.full(nc, -1, np.int64)           # the nearest selected ancestor-or-self
    for c in range(nc):
        up = sel[par[c]] if par[c] >= 0 else -1
        sel[c] = up if up >= 0 else (c if flag[c] else -1)
    chosen = sorted(set(sel[sel >= 0].tolist()))
    number = {c: i for i, c in enumerate(chosen)}
    for r in range(n):
        if fell[r] >= 0 and sel[fell[r]] >= 0:
            s = sel[fell[r]]
            labels[r] = number[s]
            prob[r] = 1.0 if max_lam[s] == 0 else min(lam_row[r], max_lam[s]) / max_lam[s]
    parent_, child_, lam_, size_ = (np.array(x) for x in zip(*cond))
    return dict(labels=labels, prob=prob,
                condensed=(parent_.astype(np.int64), child_.astype(np.int64), lam_.astype(np.float64),
                           size_.astype(np.int64)), stability=stab)


def hdbscan_ref(D, min_cluster_size, min_samples=None, method="eom", allow_single_cluster=False, groups=None, tie="first"):
    ms = min_cluster_size if min_samples is None else min_samples
    core, W = mutual_reachability(D, ms, groups)
    edges, weights = mst(W, tie)
    out = tree(edges, weights, D.shape[0], min_cluster_size, method, allow_single_cluster)
    out.update(core=core, edges=edges, weights=weights)
    return out


def same_partition(a, b):
    """labels equal up to renumbering (noise stays noise)"""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs))


# ---------------------------------------------------------------------------------------------------------------------
# the sets
def blobs_32d(seed, dim=32, sizes=(40, 50, 60, 70, 80), far=12):
    """five blobs of 40 to 80 rows with different spreads plus 12 far rows (N = 312), permuted"""
    rng = np.random.default_rng(100 + seed)
    centres = rng.normal(0, 4.0, size=(len(sizes), dim))
    parts = [c + rng.normal(0, 0.5 + 0.25 * i, size=(s, dim)) for i, (c, s) in enumerate(zip(centres, sizes))]
    parts.append(rng.normal(0, 12.0, size=(far, dim)))
    x = np.concatenate(parts)
    return x[rng.permutation(len(x))].astype(F32)


def blobs_2d(seed, sizes=(60, 80, 100, 120), far=12):
    """four blobs of different densities and 12 background rows in the plane (N = 372), permuted"""
    rng = np.random.default_rng(200 + seed)
    centres = np.array([[0.0, 0.0], [6.0, 1.0], [1.5, 7.0], [8.0, 8.0]])
    parts = [c + rng.normal(0, 0.3 + 0.2 * i, size=(s, 2)) for i, (c, s) in enumerate(zip(centres, sizes))]
    parts.append(rng.uniform(-4.0, 12.0, size=(far, 2)))
    x = np.concatenate(parts)
    return x[rng.permutation(len(x))].astype(F32)


def lattice():
    """a 12 x 12 unit lattice and two 5 x 5 lattices of spacing 1/2 (N = 194), permuted: every distance is the correctly
    rounded root of an exact rational, and ties are everywhere"""
    g = np.stack(np.meshgrid(np.arange(12.0), np.arange(12.0)), -1).reshape(-1, 2)
    h = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0)), -1).reshape(-1, 2) * 0.5
    x = np.concatenate([g, h + np.array([20.0, 3.0]), h + np.array([4.0, 19.0])])
    return x[np.random.default_rng(7).permutation(len(x))].astype(F32)


def clumps_2d(n=3000, seed=5):
    """uneven clumps in the plane: densities two orders of magnitude apart, and a thin background"""
    rng = np.random.default_rng(300 + seed)
    k = 12
    centres = rng.uniform(0, 60, size=(k, 2))
    share = rng.dirichlet(np.ones(k) * 2.0)
    counts = np.maximum((share * (n - n // 20)).astype(int), 20)
    counts[-1] += (n - n // 20) - counts.sum()
    parts = [c + rng.normal(0, 0.15 * 2.0 ** (i % 5), size=(m, 2)) for i, (c, m) in enumerate(zip(centres, counts))]
    parts.append(rng.uniform(-5, 65, size=(n - sum(len(p) for p in parts), 2)))
    x = np.concatenate(parts)
    return x[rng.permutation(len(x))].astype(F32)


def blobs_70d(n=1300, seed=6):
    rng = np.random.default_rng(400 + seed)
    k = 8
    centres = rng.normal(0, 3.0, size=(k, 70))
    which = rng.integers(0, k, size=n - 40)
    x = np.concatenate([centres[which] + rng.normal(0, 0.4 + 0.1 * which[:, None], size=(n - 40, 70)),
                        rng.normal(0, 9.0, size=(40, 70))])
    return x[rng.permutation(n)].astype(F32)


def object_set(seed=31):
    """(X fp32 [objects * 5, 32], obj int64): 5 near-identical alerts per object, as tests/lof_ref.masking_set"""
    from lof_ref import masking_set
    x, obj, _planted = masking_set(seed, objects=96, epochs=5, planted=3)
    return x, obj


BAD_ROWS = (3, 100, 311)


def blobs_32d_with_bad_rows(seed=1):
    """the 32-D set with a NaN, a +inf and a -inf planted in the rows BAD_ROWS"""
    x = blobs_32d(seed).copy()
    x[3, 0], x[100, 7], x[311, 31] = np.nan, np.inf, -np.inf
    return x


def equality_sets():
    """(name, X) of the sets on which the device must give the restatement's labels exactly"""
    out = [(f"32-D seed {s}", blobs_32d(s)) for s in SEEDS_32D]
    out += [(f"2-D seed {s}", blobs_2d(s)) for s in SEEDS_2D]
    out.append(("lattice", lattice()))
    return out


SEEDS_32D = (0, 1, 2)
SEEDS_2D = (0, 1, 2)


def band(dim):
    return (dim + 4) * U
