"""GPU tests of MapIndex and of method="grid" (run with -m gpu on an MI355X): radius lists, counts and k-nearest rows equal,
bit for bit, the fp32 rule of tests/grid_ref.py and the tile path (EmbeddingIndex at D = 2); no answer depends on the grid
resolution, on the lanes per query row, on the other rows of the call or on the order of the bank; the graphs and DBSCAN
through the grid equal those through the tiles."""
import functools

import numpy as np
import pytest
import torch

import btsbot_amd
import grid_ref as GR
import radius_ref as R

pytestmark = pytest.mark.gpu

SETS = ("blobs", "edges", "offset")
SORTS = ("index", "distance")


@functools.lru_cache(maxsize=None)
def _set(name):
    """(bank, bank groups, queries, query groups, the radii of the set): computed once, never written"""
    b = {"blobs": lambda: R.blobs_2d(11), "edges": GR.edge_set, "offset": GR.offset_set}[name]()
    if name == "blobs":
        b = b.copy()
        b[300:330] = b[:30]                                   # exact duplicates
    q = GR.queries_for(b)
    bg, qg = GR.high_bit_groups(len(b), 8), GR.high_bit_groups(len(q), 9)
    qc, bc = _for_the_checker(q), _for_the_checker(b)
    d = R.d64_matrix(qc, bc, "euclidean")
    picked = R.pick_radius(d, R.eligible(qc, bc), 2, "euclidean")
    small = {"blobs": 0.05, "edges": 0.125, "offset": 0.01}[name]
    per_row = np.where(np.arange(len(q)) % 4 == 0, 0.0, np.where(np.arange(len(q)) % 4 == 1, np.inf, picked)).astype(np.float32)
    for a in (b, q, bg, qg, per_row):
        a.setflags(write=False)
    return b, bg, q, qg, (0.0, small, picked, float("inf"), per_row)


def _for_the_checker(x):
    """radius_ref knows non-finite COORDINATES only; a row whose squared norm overflows (non-finite by the device's rule,
    at every D) is shown to it as NaN"""
    x = np.array(x, np.float32)
    x[~GR.finite_rows(x)] = np.nan
    return x


def _gpu(dev, *arrays):
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays]


def _np(out):
    return tuple(t.cpu().numpy() for t in out)


def _same_csr(got, want, what):
    (ip, ii, dd), (wp, wi, wd) = got, want
    assert ip.dtype == ii.dtype == np.int64 and dd.dtype == np.float32, what
    assert np.array_equal(ip, wp), what
    assert np.array_equal(ii, wi), what
    assert np.array_equal(dd.view(np.int32), wd.view(np.int32)), what


def _check64(qc, bc, r, got, sort, ref_kw):
    """radius_ref.check_radius, the float64 contract, for the rows whose radius is > 0.  Its float64 distances come from
    the expansion form, whose absolute error (1e-7 on these sets, 1e-4 on the offset one) cannot tell the exact 0 of a
    duplicate from a tiny distance, so it has no say at r = 0: such a row is shown to it with radius -1 and an empty
    list (the fp32 rule and the tile path check those rows)."""
    ip, ii, dd = got
    rr = np.broadcast_to(np.asarray(r, np.float64), (len(qc),)).copy()
    if not (rr > 0).any():
        return
    keep = np.repeat(rr > 0, np.diff(ip))
    ip = np.r_[0, np.cumsum(np.where(rr > 0, np.diff(ip), 0))].astype(np.int64)
    rr[rr == 0] = -1.0
    with np.errstate(invalid="ignore"):
        R.check_radius(qc, bc, rr, ip, ii[keep], dd[keep], "euclidean", sort=sort, **ref_kw)


def _rows(out):
    ip, ii, dd = _np(out) if isinstance(out[0], torch.Tensor) else out
    return [(ii[a:b].tobytes(), dd[a:b].tobytes()) for a, b in zip(ip[:-1], ip[1:])]


def _variants(bg, qg):
    """(keyword arguments of the device call, those of the references)"""
    for self_offset in (-1, 0):
        for excl in (False, True):
            dev_kw = dict(self_offset=self_offset)
            ref_kw = dict(self_offset=self_offset)
            if excl:
                dev_kw.update(query_groups=qg, exclude_same_group=True)
                ref_kw.update(qgroups=qg.cpu().numpy(), bgroups=bg.cpu().numpy())
            yield dev_kw, ref_kw


@pytest.mark.parametrize("name", SETS)
def test_radius_equals_the_fp32_rule_and_the_tile_path_bit_for_bit(cuda, name):
    b, bg, q, qg, radii = _set(name)
    tb, tbg, tq, tqg = _gpu(cuda, b, bg, q, qg)
    mi = btsbot_amd.MapIndex(tb, groups=tbg)
    tiles = btsbot_amd.EmbeddingIndex(tb, groups=tbg)
    assert len(mi) == len(b) and torch.equal(mi.points, tb) and torch.equal(mi.groups, tbg)
    qc, bc = _for_the_checker(q), _for_the_checker(b)
    pairs = 0
    for r in radii:
        tr = r if isinstance(r, float) else _gpu(cuda, r)[0]
        for sort in SORTS:
            for dev_kw, ref_kw in _variants(tbg, tqg):
                what = (name, "per row" if not isinstance(r, float) else r, sort, sorted(dev_kw.items(), key=str)[:1])
                stats = {}
                got = _np(mi.radius(tq, tr, sort=sort, stats=stats, **dev_kw))
                assert stats["error_flag"] == 0 and stats["total"] == len(got[1]) <= stats["visited"]
                _same_csr(got, GR.radius_lists(q, b, r, sort=sort, **ref_kw), what)          # the rule: no band
                _same_csr(got, _np(tiles.radius(tq, tr, sort=sort, **dev_kw)), what)         # the tile path
                _check64(qc, bc, r, got, sort, ref_kw)
                pairs += len(got[1])
                ip = got[0]
                assert ip[6] == ip[5] == ip[7]                # the two non-finite query rows have empty lists
    assert pairs > 10000


@pytest.mark.parametrize("name", SETS)
def test_counts_are_the_list_lengths_without_a_host_read(cuda, name):
    b, bg, q, qg, radii = _set(name)
    tb, tbg, tq, tqg = _gpu(cuda, b, bg, q, qg)
    mi = btsbot_amd.MapIndex(tb, groups=tbg)
    trs = [r if isinstance(r, float) else _gpu(cuda, r)[0] for r in radii]
    variants = list(_variants(tbg, tqg))
    want = [[mi.radius(tq, tr, **dev_kw)[0].diff() for dev_kw, _ in variants] for tr in trs]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                # a host read is an error in this mode
    try:
        got = [[mi.count_within(tq, tr, **dev_kw) for dev_kw, _ in variants] for tr in trs]
        knn = mi.query(tq, 5)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for g_row, w_row in zip(got, want):
        for g, w in zip(g_row, w_row):
            assert g.dtype == torch.int64 and torch.equal(g, w)
    assert knn[0].shape == (len(q), 5)
    assert int(got[3][0].max()) == int(GR.finite_rows(b).sum())           # r = +inf: every finite row


@pytest.mark.parametrize("name", SETS)
def test_query_equals_the_brute_force_by_distance_then_index(cuda, name):
    b, bg, q, qg, _radii = _set(name)
    tb, tbg, tq, tqg = _gpu(cuda, b, bg, q, qg)
    mi = btsbot_amd.MapIndex(tb, groups=tbg)
    for k in (1, 5, 15, 64):
        for dev_kw, ref_kw in _variants(tbg, tqg):
            idx, dist = _np(mi.query(tq, k, **dev_kw))
            want_i, want_d = GR.knn(q, b, k, **ref_kw)
            assert idx.dtype == np.int64 and dist.dtype == np.float32
            assert np.array_equal(idx, want_i), (name, k, dev_kw.keys())
            assert np.array_equal(dist.view(np.int32), want_d.view(np.int32)), (name, k)
            assert (idx[[5, 6]] == -1).all() and np.isnan(dist[[5, 6]]).all()


def test_query_fills_where_fewer_than_k_rows_are_eligible(cuda):
    b, bg, _q, _qg, _radii = _set("edges")
    keep = np.r_[np.arange(30), [17, 400, 901], np.arange(7)]             # 40 rows: duplicates and the three bad rows
    b, bg = b[keep], (np.arange(40, dtype=np.int64) % 3 << 32) + 7
    q = np.concatenate([b[:20], GR.queries_for(b, 20, seed=3)])
    qg = (np.arange(40, dtype=np.int64) % 3 << 32) + 7
    tb, tbg, tq, tqg = _gpu(cuda, b, bg, q, qg)
    for cells in (None, 1, 64):
        mi = btsbot_amd.MapIndex(tb, groups=tbg, cells=cells)
        for k in (1, 5, 36, 37, 38, 64):
            for dev_kw, ref_kw in _variants(tbg, tqg):
                idx, dist = _np(mi.query(tq, k, **dev_kw))
                want_i, want_d = GR.knn(q, b, k, **ref_kw)
                assert np.array_equal(idx, want_i), (cells, k)
                assert np.array_equal(dist.view(np.int32), want_d.view(np.int32)), (cells, k)
    assert (want_i[0] == -1).sum() > 30 and np.isposinf(want_d[0][want_i[0] == -1]).all()


@pytest.mark.parametrize("name", SETS)
def test_answers_do_not_depend_on_the_cells_the_lanes_the_call_or_the_bank_order(cuda, name):
    b, bg, q, qg, radii = _set(name)
    tb, tbg, tq, tqg = _gpu(cuda, b, bg, q, qg)
    r = radii[2]
    kw = dict(query_groups=tqg, exclude_same_group=True)
    base = btsbot_amd.MapIndex(tb, groups=tbg)
    ref = {sort: _rows(base.radius(tq, r, sort=sort, **kw)) for sort in SORTS}
    ref_all = _rows(base.radius(tq, float("inf")))
    ref_k = _np(base.query(tq, 15, **kw))
    for cells in (1, 7, 2048):
        mi = btsbot_amd.MapIndex(tb, groups=tbg, cells=cells)
        assert mi.cells == cells
        for sort in SORTS:
            assert _rows(mi.radius(tq, r, sort=sort, **kw)) == ref[sort], (cells, sort)
        assert _rows(mi.radius(tq, float("inf"))) == ref_all, cells
        got_k = _np(mi.query(tq, 15, **kw))
        assert np.array_equal(got_k[0], ref_k[0]) and np.array_equal(got_k[1].view(np.int32), ref_k[1].view(np.int32)), cells
        assert torch.equal(mi.count_within(tq, r, **kw), base.count_within(tq, r, **kw))
    for lanes in (1, 4, 8, 16, 32, 64):
        base._lanes = lanes
        assert _rows(base.radius(tq, r, sort="distance", **kw)) == ref["distance"], lanes
        assert _rows(base.radius(tq, float("inf"))) == ref_all, lanes
    base._lanes = 0
    # the other rows of the call: permuted, split into two calls, duplicated
    nq = len(q)
    perm = torch.randperm(nq, generator=torch.Generator().manual_seed(5)).to(cuda)
    pkw = dict(query_groups=tqg[perm], exclude_same_group=True)
    assert _rows(base.radius(tq[perm], r, sort="distance", **pkw)) == [ref["distance"][i] for i in perm.tolist()]
    pk = _np(base.query(tq[perm], 15, **pkw))
    assert np.array_equal(pk[0], ref_k[0][perm.cpu().numpy()])
    assert np.array_equal(pk[1].view(np.int32), ref_k[1][perm.cpu().numpy()].view(np.int32))
    halves = []
    for part in (slice(0, 63), slice(63, nq)):
        halves += _rows(base.radius(tq[part], r, sort="distance", query_groups=tqg[part], exclude_same_group=True))
    assert halves == ref["distance"]
    twice = _rows(base.radius(torch.cat([tq, tq]), r, sort="distance", query_groups=torch.cat([tqg, tqg]),
                              exclude_same_group=True))
    assert twice == ref["distance"] + ref["distance"]
    assert _rows(base.radius(tq, r, sort="distance", **kw)) == ref["distance"]          # ... and the run
    # the order of the bank: the same pairs once the indices are mapped back
    bperm = torch.randperm(len(b), generator=torch.Generator().manual_seed(6)).to(cuda)
    shuffled = btsbot_amd.MapIndex(tb[bperm], groups=tbg[bperm])
    ip, ii, dd = _np(shuffled.radius(tq, r, **kw))
    rp, ri, rd = _np(base.radius(tq, r, **kw))
    assert np.array_equal(ip, rp)
    back = bperm.cpu().numpy()[ii]
    for i in range(nq):
        o = np.argsort(back[ip[i]:ip[i + 1]], kind="stable")
        assert np.array_equal(back[ip[i]:ip[i + 1]][o], ri[rp[i]:rp[i + 1]])
        assert np.array_equal(dd[ip[i]:ip[i + 1]][o].view(np.int32), rd[rp[i]:rp[i + 1]].view(np.int32))
    sk = _np(shuffled.query(tq, 15, **kw))
    assert np.array_equal(sk[1].view(np.int32), ref_k[1].view(np.int32))                # ties may swap rows, not distances
    wider = _np(base.query(tq, 16, **kw))       # a row whose 16 nearest distances are distinct has one answer for k = 15
    untied = np.array([len(set(row.tolist())) == len(row) for row in wider[1]]) & (wider[0] >= 0).all(1)
    assert untied.sum() > (0 if name == "edges" else 20)      # (a condition on the inputs: the edge set is full of ties)
    assert np.array_equal(back_map(bperm, sk[0])[untied], ref_k[0][untied])


def back_map(bperm, idx):
    p = bperm.cpu().numpy()
    return np.where(idx >= 0, p[np.clip(idx, 0, None)], -1)


def test_radius_graph_through_the_grid_equals_the_tiles(cuda):
    b, bg, _q, _qg, radii = _set("blobs")
    tb, tbg = _gpu(cuda, b, bg)
    obj = (torch.arange(len(b), device=cuda) % 37).to(torch.int64) - 5
    for r in (radii[2], 0.0, torch.from_numpy(np.where(np.arange(len(b)) % 2 == 0, 0.3, 0.1).astype(np.float32)).to(cuda)):
        for include_self in (True, False):
            for groups in (None, obj, tbg):
                for sort in SORTS:
                    kw = dict(include_self=include_self, groups=groups, sort=sort)
                    stats = {}
                    got = _np(btsbot_amd.radius_graph(tb, r, method="grid", stats=stats, **kw))
                    _same_csr(got, _np(btsbot_amd.radius_graph(tb, r, method="tiles", **kw)), (include_self, sort))
                    assert stats["error_flag"] == 0 and stats["visited"] >= stats["total"]
    ip, ii, _dd = _np(btsbot_amd.radius_graph(tb, 0.0, include_self=False, method="grid"))
    assert np.array_equal(ii, np.r_[np.arange(300, 330), np.arange(30)]) and (np.diff(ip) <= 1).all()
    total = int(btsbot_amd.radius_graph(tb, radii[2], method="grid")[0][-1])
    assert btsbot_amd.radius_graph(tb, radii[2], method="grid", max_total=total)[1].shape[0] == total
    with pytest.raises(ValueError, match=f"T = {total}"):
        btsbot_amd.radius_graph(tb, radii[2], method="grid", max_total=total - 1)
    with pytest.raises(ValueError, match="r must be >= 0 in every row"):
        btsbot_amd.radius_graph(tb, torch.full((len(b),), float("nan"), device=cuda), method="grid")
    # nothing to do
    ip, ii, dd = btsbot_amd.radius_graph(tb[:0], 1.0, method="grid")
    assert ip.tolist() == [0] and ii.shape == dd.shape == (0,) and (ii.dtype, dd.dtype) == (torch.int64, torch.float32)
    empty = btsbot_amd.MapIndex(tb[:0])
    assert empty.radius(tb[:3], float("inf"))[0].tolist() == [0] * 4 and empty.count_within(tb[:3], 1.0).tolist() == [0] * 3
    assert empty.query(tb[:3], 2)[0].tolist() == [[-1, -1]] * 3 and btsbot_amd.MapIndex(tb).query(tb[:0], 3)[0].shape == (0, 3)


def test_knn_graph_through_the_grid(cuda):
    b, bg, _q, _qg, _radii = _set("edges")
    tb, tbg = _gpu(cuda, b, bg)
    idx, dist = _np(btsbot_amd.knn_graph(tb, 5, method="grid"))
    fin = np.isfinite(b).all(1)
    assert np.array_equal(idx[fin, 0], np.flatnonzero(fin)) and (dist[fin, 0] == 0).all() and (idx[~fin, 0] == -1).all()
    want_i, want_d = GR.knn(b, b, 4, self_offset=0)
    assert np.array_equal(idx[:, 1:], want_i) and np.array_equal(dist[:, 1:].view(np.int32), want_d.view(np.int32))
    idx, dist = _np(btsbot_amd.knn_graph(tb, 5, include_self=False, groups=tbg, method="grid"))
    want_i, want_d = GR.knn(b, b, 5, self_offset=0, qgroups=bg, bgroups=bg)
    assert np.array_equal(idx, want_i) and np.array_equal(dist.view(np.int32), want_d.view(np.int32))
    # on a set without ties the tile path picks the same rows
    blobs = torch.from_numpy(R.blobs_2d(12)).to(cuda)
    g, t = btsbot_amd.knn_graph(blobs, 15, method="grid"), btsbot_amd.knn_graph(blobs, 15, method="tiles")
    assert torch.equal(g[0], t[0]) and torch.equal(g[1].view(torch.int32), t[1].view(torch.int32))


def _dbscan(cuda, X, eps, min_samples, **kw):
    labels, core = btsbot_amd.dbscan(torch.from_numpy(X).to(cuda), eps, min_samples, method="grid", **kw)
    assert labels.dtype == torch.int64 and core.dtype == torch.bool and labels.shape == core.shape == (len(X),)
    return labels.cpu().numpy(), core.cpu().numpy()


@pytest.mark.parametrize("name, X, eps, min_samples", R.dbscan_sets()[:2], ids=lambda v: v if isinstance(v, str) else None)
def test_dbscan_through_the_grid_equals_the_rule_exactly(cuda, name, X, eps, min_samples):
    assert X.shape[1] == 2 and R.pairs_in_band(X, eps) == 0   # on the CPU, first: equality is then the contract
    want_l, want_c = R.dbscan_ref(X, eps, min_samples)
    labels, core = _dbscan(cuda, X, eps, min_samples)
    assert np.array_equal(core, want_c) and np.array_equal(labels, want_l)
    tl, tc = btsbot_amd.dbscan(torch.from_numpy(X).to(cuda), eps, min_samples)
    assert np.array_equal(tl.cpu().numpy(), labels) and np.array_equal(tc.cpu().numpy(), core)


def test_dbscan_through_the_grid_on_the_chain_and_the_grouped_set(cuda):
    X = np.zeros((600, 2), np.float32)
    X[:, 0] = np.arange(600) * 0.5
    X = X[np.random.default_rng(1).permutation(600)]
    assert R.pairs_in_band(X, 0.75) == 0
    labels, core = _dbscan(cuda, X, 0.75, 3)
    want_l, want_c = R.dbscan_ref(X, 0.75, 3)
    assert np.array_equal(labels, want_l) and np.array_equal(core, want_c)
    assert (labels == 0).all() and core.sum() == 598
    rng = np.random.default_rng(3)
    centres = rng.uniform(0, 1000, size=(512, 2))
    X = (np.repeat(centres, 5, axis=0) + rng.normal(0, 0.01, size=(2560, 2))).astype(np.float32)
    obj = np.repeat(np.arange(512) * 7 - 100, 5).astype(np.int64)
    perm = rng.permutation(2560)
    X, obj = X[perm], obj[perm]
    X = np.r_[X, (np.float32(2000) + rng.normal(0, 0.01, size=(6, 2))).astype(np.float32)]
    obj = np.r_[obj, 10000 + np.arange(6)]
    assert R.pairs_in_band(X, 0.2) == 0
    tg = torch.from_numpy(obj).to(cuda)
    for min_samples, groups in ((5, None), (5, obj), (6, obj)):
        labels, core = _dbscan(cuda, X, 0.2, min_samples, **({} if groups is None else {"groups": tg}))
        want_l, want_c = R.dbscan_ref(X, 0.2, min_samples, groups=groups)
        assert np.array_equal(labels, want_l) and np.array_equal(core, want_c)


def test_more_than_one_block_of_rows_against_the_tiles(cuda):
    """20,000 rows in 64 clumps: several workgroups per kernel, cells from empty to crowded"""
    rng = np.random.default_rng(9)
    X = (rng.normal(0, 25, size=(64, 2))[np.arange(20000) % 64] + rng.normal(0, 0.6, size=(20000, 2))).astype(np.float32)
    t = torch.from_numpy(X).to(cuda)
    mi = btsbot_amd.MapIndex(t)
    assert mi.cells == 100
    _, d10 = mi.query(t[::40], 11)
    eps = float(d10[:, 10].median())
    stats = {}
    got = btsbot_amd.radius_graph(t, eps, method="grid", stats=stats)
    want = btsbot_amd.radius_graph(t, eps, method="tiles")
    for g, w in zip(got, want):
        assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w)
    assert stats["error_flag"] == 0 and 20000 < stats["total"] <= stats["visited"] < 20000 * 20000 // 50
    idx, dist = _np(mi.query(t[::67], 15, self_offset=-1))
    want_i, want_d = GR.knn(X[::67], X, 15)
    assert np.array_equal(idx, want_i) and np.array_equal(dist.view(np.int32), want_d.view(np.int32))
    assert torch.equal(mi.count_within(t, eps), got[0].diff())


def test_embedding_map_keeps_one_map_index_until_it_is_extended(cuda):
    gen = torch.Generator(device=cuda).manual_seed(6)
    rows = torch.randn((96, 16), generator=gen, device=cuda)
    y = torch.randn((96, 2), generator=gen, device=cuda)
    m = btsbot_amd.EmbeddingMap.from_positions(rows, y, n_neighbors=10)
    mi = m.map_index()
    assert isinstance(mi, btsbot_amd.MapIndex) and m.map_index() is mi and len(mi) == 96 and torch.equal(mi.points, m.embedding_)
    m.extend(torch.randn((8, 16), generator=gen, device=cuda), n_epochs=5)
    again = m.map_index()
    assert again is not mi and len(again) == 104 and torch.equal(again.points, m.embedding_)
    idx, dist = again.query(m.embedding_, 1)
    assert torch.equal(idx[:, 0], torch.arange(104, device=cuda)) and bool((dist == 0).all())


def test_run_training_clusters_the_map_through_the_grid_when_asked(cuda, tmp_path, capsys):
    import warnings
    import pandas as pd
    from btsbot_amd.synthetic import synthetic_batch
    from btsbot_amd.train import run_training
    from helpers import CONFIGS, METADATA_COLS
    _, meta, _ = synthetic_batch(448, seed=21)
    lab = (meta[:, 5] > meta[:, 5].median()).long().numpy()
    d = tmp_path / "data"
    d.mkdir()
    for split, sl in (("train", slice(0, 256)), ("val", slice(256, 384)), ("test", slice(384, 448))):
        df = pd.DataFrame(meta[sl].numpy(), columns=METADATA_COLS)
        df["label"] = lab[sl]
        df.to_csv(d / f"{split}_cand_v11_N100.csv", index=False)
    base = dict(CONFIGS["um_nn"][1], model_name="um_nn", train_data_version="v11", epochs=1, batch_size=64,
                learning_rate="3e-3", warmup_epochs=1, beta_1=0.9, beta_2=0.999, patience=3, random_seed=2,
                generate_embeddings=True, embedding_layout={"n_epochs": 30, "n_neighbors": 8})
    tables = {}
    for run, method in (("g", "grid"), ("t", "tiles")):
        cfg = dict(base, embedding_clusters={"eps": 0.5, "min_samples": 3, "on": "map", "method": method})
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            run_training(cfg, data_base_dir=str(tmp_path) + "/", run_name=run, device=cuda, precision="f32",
                         models_root=str(tmp_path / "models"), embeddings_root=str(tmp_path / "embeddings"))
        tables[method] = pd.read_csv(str(tmp_path / "embeddings" / f"um_nn_{run}_umap.csv"))
    g, t = tables["grid"], tables["tiles"]
    assert list(g.columns) == ["umap_emb_1", "umap_emb_2", "cluster"] and len(g) == 64
    assert g["cluster"].dtype == np.int64 and (g["cluster"] >= -1).all()
    if np.array_equal(g[["umap_emb_1", "umap_emb_2"]].to_numpy(), t[["umap_emb_1", "umap_emb_2"]].to_numpy()):
        assert np.array_equal(g["cluster"].to_numpy(), t["cluster"].to_numpy())       # the same map: the same labels
    # an unknown method ends the embedding step as any of its errors does: reported, the run goes on
    capsys.readouterr()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run_training(dict(base, embedding_clusters={"eps": 0.5, "method": "cells"}), data_base_dir=str(tmp_path) + "/",
                     run_name="x", device=cuda, precision="f32", models_root=str(tmp_path / "models"),
                     embeddings_root=str(tmp_path / "embeddings"))
    said = capsys.readouterr().out
    assert "Error generating embeddings" in said and "config['embedding_clusters']" in said
