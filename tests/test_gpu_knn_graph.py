"""GPU tests of KnnGraph (run with -m gpu on an MI355X; btsbot_amd/graph.py, csrc/knn_graph.hip):
rule (B) bit for bit after every update, the updated graph against the rebuilt one on the separated rows, the contract
with the rank bound of u merges, NoveltyModel(keep_graph=True), and the merge kernel alone on hand-made offers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import btsbot_amd
import knn_graph_ref as KG
import knn_group_ref as G
import knn_ref as R
from btsbot_amd import EmbeddingIndex, KnnGraph, NoveltyModel, _lib, knn_graph, novelty

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAP = 0.05    # the non-separated share a comparison with the rebuild may leave out

# name: (kind, rows at build, adds, D, k, metric, group pattern, group mode, splits, non-finite rows)
CASES = {
    "normal-300-D32-k15": ("normal", 300, (1, 37, 130), 32, 15, "euclidean", None, "exclude", 0, ()),
    "normal-129-D5-k64": ("normal", 129, (127,), 5, 64, "euclidean", None, "exclude", 0, ()),
    "normal-7-D33-k15": ("normal", 7, (3, 60), 33, 15, "euclidean", None, "exclude", 0, ()),        # unfilled lists
    "normal-300-D528-k15": ("normal", 300, (130,), 528, 15, "euclidean", None, "exclude", 0, ()),
    "clustered-300-D32-k15": ("clustered", 300, (1, 37, 130), 32, 15, "euclidean", None, "exclude", 0, ()),   # rule (B) only
    "integer-200-k15": ("integer", 200, (24, 100), 5, 15, "euclidean", None, "exclude", 0, ()),
    "integer-200-k64": ("integer", 200, (24, 100), 5, 64, "euclidean", None, "exclude", 0, ()),
    "cosine-300-D32-k15": ("normal", 300, (1, 37, 130), 32, 15, "cosine", None, "exclude", 0, ()),
    "nonfinite-300-D32-k15": ("normal", 300, (1, 37, 130), 32, 15, "euclidean", None, "exclude", 0, (5, 128, 299, 300, 420)),
    "empty-add": ("normal", 300, (0, 37, 0), 32, 15, "euclidean", None, "exclude", 0, ()),
    "splits1": ("normal", 300, (1, 37, 130), 32, 15, "euclidean", None, "exclude", 1, ()),
    "splits7": ("normal", 300, (1, 37, 130), 32, 15, "euclidean", None, "exclude", 7, ()),
    "groups-exclude": ("normal", 300, (1, 37, 130), 32, 15, "euclidean", "runs", "exclude", 0, ()),
    "groups-distinct": ("normal", 300, (1, 37, 130), 32, 15, "euclidean", "mod40_hi32", "distinct", 0, ()),
    "groups-exclude+distinct": ("normal", 300, (1, 37, 130), 32, 32, "euclidean", "runs_hi32", "exclude+distinct", 0, ()),
    "groups-distinct-unfilled": ("normal", 7, (3, 60), 33, 15, "euclidean", "mod3", "distinct", 0, ()),
    "integer-groups-exclude": ("integer", 200, (24, 100), 5, 15, "euclidean", "runs", "exclude", 0, ()),
    "integer-groups-distinct": ("integer", 200, (24, 100), 5, 15, "euclidean", "mod40", "distinct", 0, ()),
    "integer-groups-exclude+distinct": ("integer", 200, (24, 100), 5, 32, "euclidean", "runs_hi32", "exclude+distinct", 0, ()),
}
# held to the rebuild: the integer sets on every row, these on every separated row (D = 528: 28 % of the rows are not,
# the clustered kind: every row -- both are held to rule (B) only)
REBUILD = ("normal-300-D32-k15", "normal-129-D5-k64", "normal-7-D33-k15", "integer-200-k15", "integer-200-k64", "splits7",
           "groups-exclude", "groups-distinct", "groups-exclude+distinct", "integer-groups-exclude",
           "integer-groups-distinct", "integer-groups-exclude+distinct")


def _np(*tensors):
    return tuple(t.detach().cpu().numpy().copy() for t in tensors)


def _differ(got_i, got_d, want_i, want_d):
    """bool [rows]: where two graphs differ in an index or in a distance bit (a NaN equals a NaN)"""
    nan = np.isnan(want_d) & np.isnan(got_d)
    bits = (got_d.view(np.int32) != want_d.view(np.int32)) & ~nan
    return (got_i != want_i).any(axis=1) | bits.any(axis=1)


def _group_kw(tg, lo, hi, mode):
    if tg is None:
        return {}
    return dict(query_groups=tg[lo:hi], exclude_same_group="exclude" in mode, one_per_group="distinct" in mode)


def _inputs(name):
    kind, n0, adds, d, k, metric, pattern, mode, splits, bad = CASES[name]
    total = n0 + sum(adds)
    x = R.make_rows(kind, total, d, 7).copy()
    for j, b in enumerate(bad):
        x[b, b % d] = (np.nan, np.inf, -np.inf)[j % 3]
    groups = None if pattern is None else G.make_groups(pattern, total, 7)
    return x, groups


@functools.lru_cache(maxsize=None)
def _run(name):
    """Builds the graph, runs the adds, and checks rule (B) bit for bit at every update.  Returns what the other checks
    read: the rows, the groups, the final graph and the stats of every update (numpy; never written)."""
    kind, n0, adds, d, k, metric, pattern, mode, splits, bad = CASES[name]
    x, groups = _inputs(name)
    tx = torch.from_numpy(x).to(DEV)
    tg = None if groups is None else torch.from_numpy(groups).to(DEV)
    exclude, one = tg is not None and "exclude" in mode, tg is not None and "distinct" in mode
    index = EmbeddingIndex(tx[:n0], metric, groups=None if tg is None else tg[:n0])
    g = KnnGraph(index, k, metric, group_mode=mode, splits=splits)
    built = knn_graph(tx[:n0], k, False, metric, groups=None if tg is None else tg[:n0], group_mode=mode)
    assert not _differ(*_np(g.idx, g.dist), *_np(*built)).any(), "the graph at build is not knn_graph's"
    assert g.index is index and g.k == k and len(g) == n0
    all_stats = []
    for q in adds:
        n1 = n0 + q
        before_i, before_d = _np(g.idx, g.dist)
        index.add(tx[n0:n1], groups=None if tg is None else tg[n0:n1])
        stats = {}
        assert g.update(stats) is g and len(g) == n1
        got_i, got_d = _np(g.idx, g.dist)
        if q == 0:
            assert stats == dict(new_rows=0, offers=0, touched=0, changed=0, candidates=0)
            assert not _differ(got_i, got_d, before_i, before_d).any()
            continue
        # new rows: index.query's lists
        want = index.query(tx[n0:n1], k, self_offset=n0, **_group_kw(tg, n0, n1, mode))
        assert not _differ(got_i[n0:], got_d[n0:], *_np(*want)).any(), "a new row's list is not index.query's"
        # old rows: merge_lists on the list before and EVERY eligible new row, distances from radius(+inf)
        tmp = EmbeddingIndex(tx[n0:n1], metric, groups=None if tg is None else tg[n0:n1])
        kw = dict(query_groups=tg[:n0], exclude_same_group=True) if exclude else {}
        indptr, oi, od = _np(*tmp.radius(tx[:n0], float("inf"), sort="distance", **kw))
        want_i, want_d = KG.merge_graph(before_i, before_d, indptr, oi + n0, od, k, groups, one)
        wrong = _differ(got_i[:n0], got_d[:n0], want_i, want_d)
        assert not wrong.any(), f"rule (B): old rows {np.flatnonzero(wrong)[:8].tolist()} after adding {q} to {n0}"
        changed = int(_differ(want_i, want_d, before_i, before_d).sum())
        assert stats["changed"] == changed and stats["new_rows"] == q
        assert changed <= stats["touched"] <= n0 and stats["touched"] <= stats["offers"] <= len(oi)
        assert stats["offers"] <= stats["candidates"]
        all_stats.append(stats)
        n0 = n1
    out_i, out_d = _np(g.idx, g.dist)
    for a in (x, out_i, out_d):
        a.setflags(write=False)
    return dict(x=x, groups=groups, idx=out_i, dist=out_d, stats=all_stats, exclude=exclude, one=one)


# ---- 1. rule (B), bit for bit, every case -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_every_update_obeys_the_merge_rule_bit_for_bit(cuda, name):
    res = _run(name)
    if sum(CASES[name][2]):
        assert res["stats"] and res["stats"][-1]["offers"] > 0


def test_splits_and_the_cut_of_the_adds_do_not_change_an_old_rows_list(cuda):
    a, b, c = _run("normal-300-D32-k15"), _run("splits1"), _run("splits7")
    assert not _differ(b["idx"], b["dist"], a["idx"], a["dist"]).any()
    assert not _differ(c["idx"], c["dist"], a["idx"], a["dist"]).any()
    # add(A); update(); add(B); update() against add(A + B); update(): the rows held at build agree bit for bit
    for name in ("normal-300-D32-k15", "integer-200-k15", "groups-distinct"):
        kind, n0, adds, d, k, metric, pattern, mode, splits, bad = CASES[name]
        res = _run(name)
        tx = torch.from_numpy(res["x"].copy()).to(DEV)
        tg = None if res["groups"] is None else torch.from_numpy(res["groups"].copy()).to(DEV)
        index = EmbeddingIndex(tx[:n0], metric, groups=None if tg is None else tg[:n0])
        g = KnnGraph(index, k, metric, group_mode=mode)
        index.add(tx[n0:], groups=None if tg is None else tg[n0:])
        once_i, once_d = _np(g.update().idx, g.dist)
        differ = _differ(once_i, once_d, res["idx"], res["dist"])
        assert not differ[:n0].any(), name
        if kind == "integer":
            assert not differ.any(), name


# ---- 2. against the rebuild -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", REBUILD)
def test_the_updated_graph_equals_the_rebuilt_one_on_separated_rows(cuda, name):
    kind, n0, adds, d, k, metric, pattern, mode, splits, bad = CASES[name]
    res = _run(name)
    tx = torch.from_numpy(res["x"].copy()).to(DEV)
    tg = None if res["groups"] is None else torch.from_numpy(res["groups"].copy()).to(DEV)
    rebuilt = _np(*knn_graph(tx, k, False, metric, groups=tg, group_mode=mode))
    differ = _differ(res["idx"], res["dist"], *rebuilt)
    if kind == "integer":
        assert not differ.any(), f"rows {np.flatnonzero(differ)[:8].tolist()}"
        return
    sep = KG.separated_rows(res["x"], k, metric, res["groups"], res["exclude"], res["one"])
    share = 1.0 - sep.mean()
    print(f"{name}: non-separated share {share:.4f}, rows that differ from the rebuild {int(differ.sum())}")
    assert share <= CAP
    assert not (differ & sep).any(), f"separated rows {np.flatnonzero(differ & sep)[:8].tolist()} differ from the rebuild"


# ---- 3. the contract after the updates --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("normal-300-D32-k15", "normal-7-D33-k15", "normal-300-D528-k15", "cosine-300-D32-k15",
                                  "nonfinite-300-D32-k15", "groups-exclude", "groups-distinct", "groups-exclude+distinct"))
def test_the_contract_holds_after_the_updates(cuda, name):
    kind, n0, adds, d, k, metric, pattern, mode, splits, bad = CASES[name]
    res = _run(name)
    worst = KG.check_graph(res["x"], res["idx"], res["dist"], k, metric, updates=len(adds), groups=res["groups"],
                           exclude=res["exclude"], one=res["one"])
    print(f"{name}: worst rank excess {worst:.3f} tau after {len(adds)} updates")


def test_self_first_is_knn_graphs_layout(cuda):
    for name in ("nonfinite-300-D32-k15", "groups-exclude"):
        kind, n0, adds, d, k, metric, pattern, mode, splits, bad = CASES[name]
        x, groups = _inputs(name)
        tx = torch.from_numpy(x).to(DEV)
        tg = None if groups is None else torch.from_numpy(groups).to(DEV)
        g = KnnGraph(tx, k, metric, groups=tg, group_mode=mode)
        want = knn_graph(tx, k + 1, True, metric, groups=tg, group_mode=mode)
        assert not _differ(*_np(*g.self_first()), *_np(*want)).any()
        assert g.rebuild() is g and not _differ(*_np(g.idx, g.dist), *_np(want[0][:, 1:], want[1][:, 1:])).any()
        fg = btsbot_amd.fuzzy_graph(*g.self_first())
        assert fg is not None


def test_storage_grows_by_doubling_and_the_views_follow(cuda):
    x = torch.from_numpy(R.make_rows("normal", 400, 5, 3)).to(DEV)
    index = EmbeddingIndex(x[:100])
    g = KnnGraph(index, 5)
    caps = []
    for lo in range(100, 400, 20):
        index.add(x[lo:lo + 20])
        g.update()
        caps.append(int(g._idx.shape[0]))
        assert g.idx.shape == (lo + 20, 5) and g.idx.data_ptr() == g._idx.data_ptr()
    assert len(set(caps)) <= 3 and caps[-1] >= 400          # 100 -> 200 -> 400: two moves for fifteen updates
    with pytest.raises(ValueError, match="metric"):
        KnnGraph(index, 5, "cosine")
    with pytest.raises(ValueError, match="groups= next to an index"):
        KnnGraph(index, 5, groups=torch.zeros(400, dtype=torch.int64, device=DEV))


# ---- 4. NoveltyModel(keep_graph=True) ---------------------------------------------------------------------------------
def _same_f64(got, want):
    got, want = got.cpu().numpy(), want.cpu().numpy()
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


@pytest.mark.parametrize("kind,n0,adds,d,k", [("integer", 200, (24, 100), 5, 15), ("normal", 300, (1, 37, 92), 5, 15),
                                              ("normal", 300, (130,), 32, 20)])
def test_novelty_model_follows_the_graph(cuda, kind, n0, adds, d, k):
    total = n0 + sum(adds)
    x = R.make_rows(kind, total, d, 7)
    tx = torch.from_numpy(x).to(DEV)
    index = EmbeddingIndex(tx[:n0])
    model = NoveltyModel(index, k, keep_graph=True)
    assert isinstance(model.graph, KnnGraph) and model.graph.k == k and model.graph.index is index
    fresh = NoveltyModel(EmbeddingIndex(tx[:n0]), k)
    assert fresh.graph is None
    assert all(_same_f64(getattr(model, f), getattr(fresh, f)) for f in ("kdist", "lrd", "lof"))
    lo = n0
    for q in adds:
        index.add(tx[lo:lo + q])
        lo += q
        with pytest.raises(RuntimeError, match=r"call refit\(\) or update\(\)"):
            model.score(tx[:4])
        assert model.update() is model and len(model) == lo == len(model.graph)
        want = novelty._fit(model.graph.idx, model.graph.dist)
        assert all(_same_f64(getattr(model, f), w) for f, w in zip(("kdist", "lrd", "lof"), want))
        s = model.score(tx[:9] + 0.25)
        assert s.shape == (9,) and bool(torch.isfinite(s).all())
    exact = kind == "integer" or (d == 5 and KG.separated_rows(x, k).all())
    if d == 5:
        assert exact, "the D = 5 set must have no non-separated row"
    if exact:
        fresh = NoveltyModel(EmbeddingIndex(tx), k)
        assert all(_same_f64(getattr(model, f), getattr(fresh, f)) for f in ("kdist", "lrd", "lof"))
        assert _same_f64(model.score(tx[:9] + 0.25), fresh.score(tx[:9] + 0.25))
    model.refit()
    assert not _differ(*_np(model.graph.idx, model.graph.dist), *_np(*knn_graph(tx, k, False))).any()


def test_a_model_without_keep_graph_behaves_as_before(cuda):
    x = torch.from_numpy(R.make_rows("normal", 160, 5, 7)).to(DEV)
    index = EmbeddingIndex(x[:130])
    model = NoveltyModel(index, 10)
    assert model.graph is None
    index.add(x[130:])
    with pytest.raises(RuntimeError, match="call refit"):
        model.score(x[:4])
    with pytest.raises(RuntimeError, match="keep_graph=True"):
        model.update()
    assert len(model.refit()) == 160 and model.score(x[:4]).shape == (4,)
    with pytest.raises(ValueError, match="MapIndex"):
        NoveltyModel(btsbot_amd.MapIndex(x[:, :2].contiguous()), 5, keep_graph=True)
    grouped = NoveltyModel(x, 10, groups=torch.arange(160, device=DEV) // 4, group_mode="exclude+distinct", keep_graph=True)
    assert grouped.graph.group_mode == "exclude+distinct" and grouped.graph.index.groups is not None


# ---- 5. the merge kernel alone ----------------------------------------------------------------------------------------
def _sorted_lists(rng, n_old, k, groups=None, distinct=False, fill=None):
    """Hand-made lists ordered by (dist, index): full or a random number of present entries (``fill``: that many),
    distinct groups on demand."""
    idx = np.full((n_old, k), -1, np.int64)
    dist = np.full((n_old, k), np.inf, np.float32)
    for a in range(n_old):
        cand = rng.permutation(n_old)
        if distinct:
            cand = cand[np.sort(np.unique(groups[cand], return_index=True)[1])]
        want = fill if fill is not None else (k if rng.random() < 0.5 else int(rng.integers(0, k + 1)))
        c = cand[:min(len(cand), want)]
        d = rng.integers(0, 40, size=len(c)).astype(np.float32) / 4           # many ties
        o = np.lexsort((c, d))
        idx[a, :len(c)], dist[a, :len(c)] = c[o], d[o]
    return idx, dist


def _csr(rng, n_old, counts, n_new):
    """Offers per old row: ``counts[a]`` distinct new rows n_old .. n_old + n_new, distances on the lists' grid (ties)."""
    indptr = np.zeros(n_old + 1, np.int64)
    indptr[1:] = np.cumsum(counts)
    oi, od = [], []
    for a in range(n_old):
        c = n_old + rng.permutation(n_new)[:counts[a]].astype(np.int64)
        d = rng.integers(0, 40, size=len(c)).astype(np.float32) / 4
        o = np.lexsort((c, d))
        oi.append(c[o])
        od.append(d[o])
    return indptr, np.concatenate(oi) if oi else np.zeros(0, np.int64), np.concatenate(od) if od else np.zeros(0, np.float32)


def _merge_c(idx, dist, indptr, oi, od, k, groups=None, distinct=False, rows=None, stride=None):
    """btsbot_knn_graph_merge on copies: (idx, dist, changed_rows, changed_count)."""
    n_old = len(idx)
    stride = stride or k
    ti = torch.full((n_old, stride), -7, dtype=torch.int64, device=DEV)
    td = torch.full((n_old, stride), -7.0, dtype=torch.float32, device=DEV)
    ti[:, :k], td[:, :k] = torch.from_numpy(idx).to(DEV), torch.from_numpy(dist).to(DEV)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (indptr, oi, od)]
    tg = None if groups is None else torch.from_numpy(groups).to(DEV)
    tr = None if rows is None else torch.from_numpy(np.asarray(rows, np.int64)).to(DEV)
    flags = torch.zeros(max(n_old, 1), dtype=torch.uint8, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda a: C.c_void_p(a.data_ptr() if a is not None and a.numel() else 0)    # noqa: E731
    rc = _lib.lib().btsbot_knn_graph_merge(p(ti), p(td), stride, k, n_old, p(t[0]), p(t[1]), p(t[2]), len(oi), p(tg),
                                           0 if tg is None else len(groups), 1 if distinct else 0, p(tr),
                                           0 if tr is None else len(rows), p(flags), p(count),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "btsbot_knn_graph_merge")
    torch.cuda.synchronize()
    assert bool((ti[:, k:] == -7).all()) and bool((td[:, k:] == -7.0).all()), "the merge wrote past column k"
    return ti[:, :k].cpu().numpy(), td[:, :k].cpu().numpy(), flags[:n_old].cpu().numpy(), int(count[0])


def _check_merge(idx, dist, indptr, oi, od, k, groups=None, distinct=False, **kw):
    want_i, want_d = KG.merge_graph(idx, dist, indptr, oi, od, k, groups, distinct)
    got_i, got_d, flags, count = _merge_c(idx, dist, indptr, oi, od, k, groups, distinct, **kw)
    wrong = _differ(got_i, got_d, want_i, want_d)
    assert not wrong.any(), f"rows {np.flatnonzero(wrong)[:8].tolist()}"
    changed = _differ(want_i, want_d, idx, dist)
    assert np.array_equal(flags.astype(bool), changed) and count == int(changed.sum())
    return int(changed.sum())


@pytest.mark.parametrize("distinct", (False, True), ids=("plain", "distinct"))
@pytest.mark.parametrize("k", (1, 15, 32))
def test_merge_kernel_on_hand_made_offers(cuda, k, distinct):
    rng = np.random.default_rng(100 + k)
    n_old, n_new = 133, 200
    groups = rng.integers(-3, 9, size=n_old + n_new).astype(np.int64) + (rng.integers(0, 3, size=n_old + n_new) << 32)
    idx, dist = _sorted_lists(rng, n_old, k, groups, distinct)
    # no offers at all
    none = _csr(rng, n_old, np.zeros(n_old, np.int64), n_new)
    assert _check_merge(idx, dist, *none, k, groups, distinct) == 0
    # one row holds every offer: more than 64, repeated groups, ties with the old entries' distances
    counts = np.zeros(n_old, np.int64)
    counts[77] = 170
    assert _check_merge(idx, dist, *_csr(rng, n_old, counts, n_new), k, groups, distinct) <= 1
    # a few offers for some rows, many for others; the rows= form gives the same lists
    counts = np.where(rng.random(n_old) < 0.5, 0, rng.integers(1, 100, size=n_old))
    csr = _csr(rng, n_old, counts, n_new)
    changed = _check_merge(idx, dist, *csr, k, groups, distinct)
    assert changed > 0
    assert _check_merge(idx, dist, *csr, k, groups, distinct, rows=np.flatnonzero(counts), stride=k + 3) == changed


def test_merge_kernel_ties_unfilled_and_nan_rows(cuda):
    inf, nan, k = np.float32(np.inf), np.float32(np.nan), 4
    idx = np.array([[3, 5, -1, -1], [3, 5, 7, 9], [-1, -1, -1, -1], [-1, -1, -1, -1], [0, 1, 2, 3]], np.int64)
    dist = np.array([[1, 2, inf, inf], [1, 2, 3, 3], [inf] * 4, [nan] * 4, [1, 1, 1, 1]], np.float32)
    indptr = np.array([0, 2, 4, 6, 7, 9], np.int64)
    oi = np.array([10, 11, 10, 12, 11, 12, 10, 10, 11], np.int64)
    od = np.array([1, 2, 3, 3, 0.5, 0.5, 0, 1, 1], np.float32)
    got_i, got_d, flags, count = _merge_c(idx, dist, indptr, oi, od, k)
    assert got_i.tolist() == [[3, 10, 5, 11], [3, 5, 7, 9], [11, 12, -1, -1], [-1, -1, -1, -1], [0, 1, 2, 3]]
    assert got_d[0].tolist() == [1, 1, 2, 2] and np.isnan(got_d[3]).all() and got_d[2].tolist() == [0.5, 0.5, inf, inf]
    assert flags.tolist() == [1, 0, 1, 0, 0] and count == 2
    _check_merge(idx, dist, indptr, oi, od, k)
    # 64 columns: the widest list, every lane a column
    rng = np.random.default_rng(5)
    wide_i, wide_d = _sorted_lists(rng, 70, 64)
    assert _check_merge(wide_i, wide_d, *_csr(rng, 70, rng.integers(0, 130, size=70), 140), 64) > 0


def test_merge_entry_refuses_bad_arguments(cuda):
    L = _lib.lib()
    t = torch.zeros(64, dtype=torch.int64, device=DEV)
    f = torch.zeros(64, dtype=torch.float32, device=DEV)
    p = lambda a: C.c_void_p(a.data_ptr())    # noqa: E731

    def call(k=4, stride=4, flags=0, groups=t, n_old=4, n_offers=4, idx=t):
        return L.btsbot_knn_graph_merge(p(idx) if idx is not None else None, p(f), stride, k, n_old, p(t), p(t), p(f), n_offers,
                                        p(groups) if groups is not None else None, 64, flags, None, 0, None, None, None)
    for kw in (dict(k=0), dict(k=65, stride=65), dict(k=33, stride=33, flags=1), dict(stride=3), dict(flags=2),
               dict(flags=1, groups=None), dict(n_old=-1), dict(n_offers=1 << 31), dict(idx=None)):
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
        assert b"btsbot_knn_graph_merge" in L.btsbot_last_error()
    assert call(n_offers=0) == _lib.OK and call(n_old=0) == _lib.OK
