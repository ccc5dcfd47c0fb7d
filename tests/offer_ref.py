"""What the offer tests share (no GPU): the four offer entry points of csrc/mr_offer.hip restated in numpy, and the
hand-made lists they are asked about.

    out = offer_knn(idx, dist, n, core, slack=None, squared=False, rel=0.0, min_samples=None)
    best_w, best_j = offer_csr(indptr, indices, dist, rows, n_rows, n, core, row_core, best_w, best_j)
    case = lists(k, n, rows=70, slack=None | "plain" | "squared", rel=0.0, min_samples=None, seed=0)

``min_samples=None`` is the spanning tree's form (``btsbot_mst_offer_knn``: the rows ARE the bank, a row's core distance
is ``core[row]``, the list proves its lightest entry when ``w <= max(floor, core(row))``); an int is prediction's
(``btsbot_cluster_offer_knn``: the core distance is column ``min_samples - 2`` of the row's own list, ``w < floor``
strictly, and ``core_q`` is an output).  ``out`` holds ``best_w`` float32, ``best_j`` int32, ``unresolved`` uint8 and, for
prediction, ``core_q`` float32.

Every distance, core distance and slack of ``lists`` is a multiple of 2^-6 below 64 (the boundary rows' one-step
neighbours apart, which enter comparisons only), ``rel`` is 0 or 2^-10, and the squared slacks are Pythagorean:
``d_last = 5 a``, ``s = 9 a^2``, floor ``4 a``.  Every product, difference and square root of the floor is then exact in
float64, with or without a fused multiply-add, and the restatement below needs no care about the order of roundings.
"""
import numpy as np

F32 = np.float32
INF32 = F32(np.inf)
NO_KEY = (1 << 64) - 1


def _bits(w):
    return int(np.asarray(w, F32).view(np.uint32))


def key_of(d, core_row, core_j, j):
    """(w, j) as one integer: ``w = max(d, core_row, core_j)`` (a NaN is ignored), clamped at +0"""
    w = np.fmax(F32(d), np.fmax(F32(core_row), F32(core_j)))
    w = w if w > 0 else F32(0.0)
    return (_bits(w) << 32) | (int(j) & 0xffffffff)


def _unkey(key):
    return np.array(key >> 32, np.uint32).view(F32)[()], np.int32(key & 0xffffffff)


def floor_of(d_last, slack, squared, rel):
    """the float64 lower bound of the distance of a row the full list does not hold"""
    f = float(d_last)
    if slack is not None:
        s = float(slack)
        f = float(np.sqrt(max(f * f - s, 0.0))) if squared else f - s
    return f * (1.0 - float(F32(rel)))


def offer_knn(idx, dist, n, core, slack=None, squared=False, rel=0.0, min_samples=None):
    idx, dist, core = np.asarray(idx, np.int64), np.asarray(dist, F32), np.asarray(core, F32)
    rows, k = idx.shape
    predict = min_samples is not None
    out = dict(best_w=np.empty(rows, F32), best_j=np.empty(rows, np.int32), unresolved=np.zeros(rows, np.uint8))
    if predict:
        out["core_q"] = np.empty(rows, F32)
    for r in range(rows):
        present = (idx[r] >= 0) & (idx[r] < n)
        if predict:
            col = min_samples - 2
            core_row = F32(0.0) if col < 0 else (dist[r, col] if present[col] else INF32)
        else:
            core_row = core[r]
        key = NO_KEY
        for c in np.flatnonzero(present & ~np.isnan(dist[r])):
            key = min(key, key_of(dist[r, c], core_row, core[idx[r, c]], idx[r, c]))
        w, j = (INF32, np.int32(-1)) if key == NO_KEY else _unkey(key)
        if predict:
            if np.isnan(dist[r, 0]):                      # a non-finite query row
                out["core_q"][r] = out["best_w"][r] = F32(np.nan)
                out["best_j"][r] = -1
                continue
            out["core_q"][r] = core_row
            if not core_row < INF32:                      # fewer than min_samples - 1 eligible rows (or a NaN there)
                w, j = INF32, np.int32(-1)
        out["best_w"][r], out["best_j"][r] = w, j
        if j < 0 or not present[k - 1]:                   # nothing to prove, or the list holds every eligible row
            continue
        floor = floor_of(dist[r, k - 1], None if slack is None else slack[r], squared, rel)
        if predict:
            out["unresolved"][r] = 0 if float(w) < floor else 1
        else:
            out["unresolved"][r] = 0 if float(w) <= np.fmax(floor, float(core_row)) else 1
    return out


def offer_csr(indptr, indices, dist, rows, n_rows, n, core, row_core, best_w, best_j):
    """the minimum over the CSR lists of the rows ``rows``, kept where it is below the (w, j) the row holds already"""
    best_w, best_j = np.array(best_w, F32), np.array(best_j, np.int32)
    for u, r in enumerate(np.asarray(rows).tolist()):
        if r < 0 or r >= n_rows:
            continue
        key = NO_KEY
        for e in range(int(indptr[u]), int(indptr[u + 1])):
            j, d = int(indices[e]), F32(dist[e])
            if 0 <= j < n and not np.isnan(d):
                key = min(key, key_of(d, row_core[r], core[j], j))
        old = NO_KEY if best_j[r] < 0 else (_bits(best_w[r]) << 32) | int(best_j[r])
        if key < old:
            best_w[r], best_j[r] = _unkey(key)
    return best_w, best_j


# ---------------------------------------------------------------------------------------------------------------------
# the lists
STEP = 2.0 ** -6
# rows of a set of lists that are made by hand (the others are drawn)
EMPTY, TAIL, BAD_INDEX_FIRST, BAD_INDEX_LAST, NAN_DIST, NAN_FIRST, TIE_DIST, TIE_CORE, CLAMP, NAN_CORE = range(10)
BOUNDARY = ("at", "below", "above", "core_at", "core_above", "far_above")   # rows 12.., towards bank rows 20..
BOUNDARY_ROW, BOUNDARY_BANK = 12, 20
ZERO, NEG_ZERO, NO_CORE, HEAVY = 26, 27, 28, 29                             # bank rows of core distance 0, -0, NaN and 63


def _grid(rng, lo, hi, size=None):
    """multiples of 2^-6 in [lo, hi)"""
    return (rng.integers(round(lo / STEP), round(hi / STEP), size=size) * STEP).astype(F32)


def lists(k, n, rows=70, slack=None, rel=0.0, min_samples=None, seed=0):
    """dict(idx int64 [rows, k], dist float32 [rows, k], core float32 [n], slack float32 [rows] or None, squared, rel,
    min_samples, n, boundary = {row: what}).  ``n`` is the bank: ``rows`` itself for the spanning tree's form."""
    rng = np.random.default_rng(1000 * k + seed)
    predict = min_samples is not None
    assert n >= 30 and rows >= 30 and (predict or n == rows)
    core = _grid(rng, 0.0, 12.0, n)
    core[[ZERO, NEG_ZERO, NO_CORE, HEAVY]] = 0.0, -0.0, np.nan, 63.0
    idx = np.stack([rng.permutation(n)[np.arange(k) % n] for _ in range(rows)]).astype(np.int64)
    a = rng.integers(1, 11, size=rows) * 0.25                       # 5 a <= 12.5, 9 a^2 <= 56.25
    a[[TIE_DIST, TIE_CORE]] = 2.5
    d_last = _grid(rng, 4.0, 40.0, rows)
    d_last[TIE_DIST], d_last[TIE_CORE] = 20.0, 12.5
    if slack == "squared":
        d_last = (5 * a).astype(F32)
    dist = np.stack([np.sort(_grid(rng, 0.0, float(d) + STEP, k)) for d in d_last])
    dist[:, -1] = d_last
    s = {None: None, "plain": _grid(rng, 0.0, 2.0, rows), "squared": (9 * a * a).astype(F32)}[slack]

    idx[EMPTY] = -1
    idx[TAIL, (k + 1) // 2:] = -1
    idx[BAD_INDEX_FIRST, 0], dist[BAD_INDEX_FIRST, 0] = n + 5, 0.0   # (would win if it were taken)
    idx[BAD_INDEX_LAST, -1] = 1 << 40                                # (the list is not full)
    dist[NAN_DIST, k // 2] = np.nan
    dist[NAN_FIRST, 0] = np.nan                                      # prediction: a non-finite query row
    # ties in w at different indices, the smallest index in the last column: by equal distances above every core
    # distance, and by the row's own core distance above every distance (prediction: at min_samples = k + 1)
    heavier = (HEAVY, *range(BOUNDARY_BANK, BOUNDARY_BANK + len(BOUNDARY)))
    for r in (TIE_DIST, TIE_CORE):
        idx[r] = np.sort(np.where(np.isin(idx[r], heavier), 0, idx[r]))[::-1]
    dist[TIE_DIST] = d_last[TIE_DIST]
    # 1 - cos rounded below 0, towards rows of core distance 0 and -0: w is clamped at +0
    idx[CLAMP, 0], dist[CLAMP, 0] = ZERO, -STEP
    if k > 1:
        idx[CLAMP, 1], dist[CLAMP, 1] = NEG_ZERO, -0.0
    idx[NAN_CORE, 0] = NO_CORE
    if not predict:
        core[TIE_CORE], core[CLAMP], core[EMPTY] = 50.0, 0.0, np.nan

    # boundary rows: full lists whose lightest entry has w at, one step below and one step above the floor, and (the
    # tree's form) at and one step above a core distance of the row's own that lies above the floor.  The entry is column
    # 0, at distance 0 towards a bank row whose core distance is the weight wanted; every other entry is HEAVY.
    boundary = {}
    for i, what in enumerate(BOUNDARY):
        r, j = BOUNDARY_ROW + i, BOUNDARY_BANK + i
        exact = floor_of(d_last[r], None if s is None else s[r], slack == "squared", rel)
        floor = F32(exact)
        assert float(floor) == exact and floor > 0.5
        own = F32(np.ceil(floor) + 2.0) if what.startswith("core") and not predict else F32(0.0)
        base = max(floor, own)
        core[j] = {"at": base, "core_at": base, "below": np.nextafter(base, -INF32), "above": np.nextafter(base, INF32),
                   "core_above": np.nextafter(base, INF32), "far_above": F32(62.0)}[what]
        idx[r], dist[r] = HEAVY, d_last[r]
        idx[r, 0] = j
        if k > 1:
            dist[r, 0] = 0.0
        if not predict:
            core[r] = own
        boundary[r] = what
    return dict(idx=idx, dist=dist.astype(F32), core=core, slack=s, squared=slack == "squared", rel=rel,
                min_samples=min_samples, n=n, boundary=boundary)


def boundary_flags(case):
    """{row: unresolved} of the boundary rows where the form decides it: the tree resolves a row AT the larger of the floor
    and its own core distance, prediction only one strictly below the floor.  (k = 1: the entry is the last column itself
    and never lies below the floor; min_samples > 2: the row's core distance is a listed distance above 0.)"""
    k, ms = case["idx"].shape[1], case["min_samples"]
    if k == 1 or (ms is not None and ms > 2):
        return {}
    open_at = ("above", "core_above", "far_above") if ms is None else ("at", "above", "core_at", "core_above", "far_above")
    return {r: int(what in open_at) for r, what in case["boundary"].items()}


def csr_lists(n_rows, n, seed=0):
    """dict(indptr, indices, dist, rows): lists of 23 of the rows -- one of 150 entries, one empty, two whose row number
    is out of range, entries out of range and NaN distances among the others"""
    rng = np.random.default_rng(77 + seed)
    rows = rng.permutation(n_rows)[:23].astype(np.int64)
    lens = rng.integers(1, 40, size=len(rows))
    lens[2], lens[5] = 150, 0
    rows[7], rows[11] = n_rows + 3, -1
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = rng.integers(0, n, size=int(indptr[-1])).astype(np.int64)
    dist = _grid(rng, 0.0, 40.0, int(indptr[-1]))
    bad = rng.permutation(len(indices))[:30]
    indices[bad[:10]], indices[bad[10:20]] = n + 1, -1
    dist[bad[20:]] = np.nan
    return dict(indptr=indptr, indices=indices, dist=dist, rows=rows)
