"""What the tests of removal share (no GPU): the compaction rule of btsbot_knn_graph_compact written plainly, the removal
patterns, and the cases -- each a script of build / remove / add steps over one array of rows -- that
tests/test_gpu_index_remove.py runs and tests/test_knn_graph_remove_host.py holds to the cap (btsbot_amd/graph.py,
DESIGN.md section 4y).  Builds on knn_ref, knn_group_ref and knn_graph_ref, which stay as they are.

The rule: a surviving old row's list becomes its present entries whose row survived, renumbered through ``new_of_old``, in
order, with the same ``dist`` bits, then a -1 / +inf tail.  An entry outside [0, n_old) is dropped like a removed one.  A
row whose ``dist[0]`` is NaN is copied as it stands and is not damaged.  A row is DAMAGED iff at least one present entry
was dropped and either the list was full (``idx[k - 1] >= 0``) or ``distinct`` is set.
"""
import numpy as np

import knn_group_ref as G
import knn_ref as R

CAP = 0.05    # the non-separated share a comparison with the rebuild may leave out (the KnnGraph tests' cap)


def compact_lists(idx, dist, new_of_old, k, distinct=False):
    """(idx int64 [s, k], dist float32 [s, k], damaged bool [s]) for the ``s`` survivors of ``new_of_old`` [n_old]."""
    idx, dist = np.asarray(idx, np.int64), np.asarray(dist, np.float32)
    new_of_old = np.asarray(new_of_old, np.int64)
    n_old = len(new_of_old)
    s = int((new_of_old >= 0).sum())
    out_i, out_d = np.full((s, k), -1, np.int64), np.full((s, k), np.inf, np.float32)
    damaged = np.zeros(s, bool)
    for a in range(n_old):
        j = int(new_of_old[a])
        if j < 0:
            continue
        if np.isnan(dist[a, 0]):
            out_i[j], out_d[j] = idx[a, :k], dist[a, :k]
            continue
        m, dropped = 0, 0
        for c in range(k):
            e = int(idx[a, c])
            if e < 0:
                continue
            if e >= n_old or new_of_old[e] < 0:
                dropped += 1
                continue
            out_i[j, m], out_d[j, m] = new_of_old[e], dist[a, c]
            m += 1
        damaged[j] = dropped > 0 and (idx[a, k - 1] >= 0 or distinct)
    return out_i, out_d, damaged


def dropped_entries(idx, dist, new_of_old, k):
    """The present entries ``compact_lists`` drops, over the surviving rows that are not NaN rows."""
    idx, new_of_old = np.asarray(idx, np.int64)[:, :k], np.asarray(new_of_old, np.int64)
    n_old = len(new_of_old)
    rows = (new_of_old >= 0) & ~np.isnan(np.asarray(dist, np.float32)[:, 0])
    gone = (idx >= n_old) | (new_of_old[np.clip(idx, 0, n_old - 1)] < 0)
    return int(((idx >= 0) & gone)[rows].sum())


def new_of_old_from(keep):
    """int64 [n]: the survivors numbered 0.. in order, -1 for the rows ``keep`` (bool [n]) drops."""
    keep = np.asarray(keep, bool)
    return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)


PATTERNS = ("mod7", "oldest60", "oldest1", "tile", "groups4", "allbut9")


def keep_mask(n, pattern, groups=None):
    """bool [n], True for the rows that stay."""
    i = np.arange(n)
    if pattern == "mod7":
        return i % 7 != 3
    if pattern == "oldest60":
        return i >= 60
    if pattern == "oldest1":
        return i >= 1
    if pattern == "tile":
        return (i < 100) | (i > 227)
    if pattern == "groups4":
        rank = np.searchsorted(np.unique(groups), groups)
        return rank % 4 != 1
    if pattern == "allbut9":
        return i % ((n + 8) // 9) == 0
    raise ValueError(pattern)


B, RM, AD = "build", "remove", "add"
_D32 = ((B, 300), (RM, "mod7"), (AD, 37), (RM, "oldest60"), (AD, 93), (RM, "tile"))
_INT = ((B, 200), (RM, "mod7"), (AD, 100), (RM, "oldest60"))
# name: (kind, total, D, k, metric, group pattern, group mode, script, planted non-finite rows)
CASES = {
    "normal-D32-k15": ("normal", 430, 32, 15, "euclidean", None, "exclude", _D32, ()),
    "normal-D5-k64": ("normal", 256, 5, 64, "euclidean", None, "exclude",
                      ((B, 129), (RM, "mod7"), (AD, 127), (RM, "oldest60")), ()),
    "cosine-D32-k15": ("normal", 430, 32, 15, "cosine", None, "exclude",
                       ((B, 300), (RM, "mod7"), (AD, 130), (RM, "oldest60")), ()),
    "unfilled-D33-k15": ("normal", 70, 33, 15, "euclidean", None, "exclude", ((B, 70), (RM, "allbut9")), ()),
    "groups-exclude": ("normal", 430, 32, 15, "euclidean", "runs", "exclude",
                       ((B, 300), (RM, "groups4"), (AD, 130), (RM, "mod7")), ()),
    "groups-distinct": ("normal", 430, 32, 15, "euclidean", "mod40_hi32", "distinct",
                        ((B, 300), (RM, "mod7"), (AD, 130), (RM, "oldest60")), ()),
    "groups-exclude+distinct": ("normal", 430, 32, 32, "euclidean", "runs_hi32", "exclude+distinct",
                                ((B, 300), (RM, "groups4"), (AD, 130), (RM, "mod7")), ()),
    "normal-D528-k15": ("normal", 430, 528, 15, "euclidean", None, "exclude", ((B, 300), (RM, "mod7"), (AD, 130)), ()),
    "integer-k15": ("integer", 300, 5, 15, "euclidean", None, "exclude", _INT, ()),
    "integer-k64": ("integer", 300, 5, 64, "euclidean", None, "exclude", _INT, ()),
    "integer-groups-exclude": ("integer", 300, 5, 15, "euclidean", "runs", "exclude", _INT, ()),
    "nonfinite": ("normal", 430, 32, 15, "euclidean", None, "exclude", _D32, (5, 128, 299, 300)),
}
# held to rules R1-R3 only: at D = 528 a quarter of the rows is not separated
NOT_REBUILD = ("normal-D528-k15",)


def inputs(name):
    """(rows float32 [total, D], groups int64 [total] or None) of a case."""
    kind, total, d, k, metric, pattern, mode, script, bad = CASES[name]
    x = R.make_rows(kind, total, d, 7).copy()
    for j, b in enumerate(bad):
        x[b, b % d] = (np.nan, np.inf, -np.inf)[j % 3]
    groups = None if pattern is None else G.make_groups(pattern, total, 7)
    return x, groups


def modes(name):
    """(exclude, one) of a case."""
    pattern, mode = CASES[name][5], CASES[name][6]
    return pattern is not None and "exclude" in mode, pattern is not None and "distinct" in mode


def states(name):
    """The script of a case, step by step: a list of (step, argument, before, after, keep) with ``before`` / ``after``
    the rows of ``inputs(name)`` the archive holds (int64, ascending) and ``keep`` the bool mask over ``before`` of a
    remove step (None otherwise)."""
    script = CASES[name][7]
    _, groups = inputs(name)
    cur, nxt, out = np.zeros(0, np.int64), 0, []
    for step, arg in script:
        keep = None
        if step == RM:
            keep = keep_mask(len(cur), arg, None if groups is None else groups[cur])
            after = cur[keep]
        else:
            after = np.concatenate([cur, np.arange(nxt, nxt + arg, dtype=np.int64)])
            nxt += arg
        out.append((step, arg, cur, after, keep))
        cur = after
    return out
