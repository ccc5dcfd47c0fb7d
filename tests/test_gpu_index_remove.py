"""GPU tests of removal (run with -m gpu on an MI355X; btsbot_amd/neighbors.py, btsbot_amd/graph.py, csrc/knn_graph.hip,
DESIGN.md section 4y): EmbeddingIndex.remove / ids / locate against an index built at once, query(self_rows=), rules R1-R3
bit for bit after every update, the updated graph against the rebuilt one (R4), independence of splits and of how removals
and adds are cut, btsbot_knn_graph_compact alone on hand-made lists, and what hangs on the graph and the index."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import knn_graph_ref as KG
import knn_graph_remove_ref as RR
import knn_ref as R
from btsbot_amd import ClusterModel, EmbeddingIndex, EmbeddingMap, KnnGraph, NoveltyModel, _lib, knn_graph, novelty

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INTEGER = tuple(n for n in RR.CASES if RR.CASES[n][0] == "integer")


def _np(*tensors):
    return tuple(t.detach().cpu().numpy().copy() for t in tensors)


def _differ(got_i, got_d, want_i, want_d):
    """bool [rows]: where two graphs differ in an index or in a distance bit (a NaN equals a NaN)"""
    nan = np.isnan(want_d) & np.isnan(got_d)
    bits = (got_d.view(np.int32) != want_d.view(np.int32)) & ~nan
    return (got_i != want_i).any(axis=1) | bits.any(axis=1)


def _same(a, b):
    """two tensors, or tuples of them, equal bit for bit (NaN included)"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        a, b = a.contiguous().view(torch.int32 if a.dtype == torch.float32 else torch.int64), \
            b.contiguous().view(torch.int32 if b.dtype == torch.float32 else torch.int64)
    return bool(torch.equal(a, b))


@functools.lru_cache(maxsize=None)
def _device_inputs(name):
    x, groups = RR.inputs(name)
    return x, groups, torch.from_numpy(x).to(DEV), None if groups is None else torch.from_numpy(groups).to(DEV)


def _apply(index, step, arg, before, after, keep, tx, tg, as_rows=False):
    """One step of a script on the index; a remove step returns ``kept``."""
    if step == RR.RM:
        which = torch.from_numpy(~keep).to(DEV)
        if as_rows:      # the int64 form: any order, repeats allowed
            gone = np.flatnonzero(~keep)
            which = torch.from_numpy(np.concatenate([gone[::-1], gone[:3]]).astype(np.int64)).to(DEV)
        return index.remove(which)
    new = torch.from_numpy(after[len(before):]).to(DEV)
    index.add(tx[new], groups=None if tg is None else tg[new])
    return None


def _group_kw(tg_now, rows, exclude, one):
    if tg_now is None:
        return {}
    return dict(query_groups=tg_now[rows], exclude_same_group=exclude, one_per_group=one)


# ---- 1. the index ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RR.CASES))
def test_the_index_answers_like_one_built_at_once_after_every_step(cuda, name):
    kind, total, d, k, metric, pattern, mode, script, bad = RR.CASES[name]
    x, groups, tx, tg = _device_inputs(name)
    exclude, one = RR.modes(name)
    index, generation = None, 0
    for t, (step, arg, before, after, keep) in enumerate(RR.states(name)):
        if step == RR.B:
            index = EmbeddingIndex(tx[:arg], metric, groups=None if tg is None else tg[:arg])
        else:
            kept = _apply(index, step, arg, before, after, keep, tx, tg, as_rows=(t // 2) % 2 == 1)
            if step == RR.RM:
                generation += 1
                assert kept.dtype == torch.int64 and np.array_equal(kept.cpu().numpy(), np.flatnonzero(keep))
        n = len(after)
        assert len(index) == n and index.generation == generation
        assert index.ids.dtype == torch.int64 and np.array_equal(index.ids.cpu().numpy(), after)
        ask = torch.from_numpy(np.array([-1, 0, 59, 60, 150, total - 1, total, 1 << 40], np.int64)).to(DEV)
        where = {int(r): j for j, r in enumerate(after)}
        assert index.locate(ask).tolist() == [where.get(int(a), -1) for a in ask.tolist()]
        assert index.locate(ask.view(2, 4)).shape == (2, 4)
        # removing nothing is a no-op
        for nothing in (torch.zeros(n, dtype=torch.bool, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV)):
            assert index.remove(nothing).tolist() == list(range(n)) and index.generation == generation and len(index) == n
        now = torch.from_numpy(after).to(DEV)
        tg_now = None if tg is None else tg[now]
        assert _same(index.bank, tx[now]) and (tg is None or _same(index.groups, tg_now))
        fresh = EmbeddingIndex(index.bank.clone(), metric, groups=None if tg is None else index.groups.clone())
        q = tx[torch.arange(0, total, 5, device=DEV)] + 0.0      # rows in the archive, rows removed and rows not yet added
        qg = None if tg is None else tg[torch.arange(0, total, 5, device=DEV)]
        all_rows = torch.arange(n, device=DEV)
        forms = [dict(), dict(splits=3)]
        if tg is not None:
            forms += [dict(query_groups=qg, exclude_same_group=True), dict(one_per_group=True),
                      dict(query_groups=qg, exclude_same_group=True, one_per_group=True)]
        kq = min(k, 32)
        for kw in forms:
            assert _same(index.query(q, kq, **kw), fresh.query(q, kq, **kw)), (t, kw)
        own = _group_kw(tg_now, all_rows, exclude, one)
        got = index.query(index.bank, k, self_offset=0, **own)
        assert _same(got, fresh.query(fresh.bank, k, self_offset=0, **own)), t
        kth = got[1][:, k - 1]
        kth = kth[torch.isfinite(kth)]
        r_med = float(kth.median()) if kth.numel() else 1.0
        rkw = dict(query_groups=qg, exclude_same_group=True) if tg is not None else {}
        for r in (r_med, float("inf")):
            assert _same(index.radius(q, r, sort="distance", **rkw), fresh.radius(q, r, sort="distance", **rkw)), (t, r)
        assert _same(index.count_within(q, r_med), fresh.count_within(q, r_med))
        targets = torch.from_numpy(np.random.default_rng(t).integers(-1, n + 1, size=(q.shape[0], 5))).to(DEV)
        assert _same(index.rank_of(q, targets, **rkw), fresh.rank_of(q, targets, **rkw)), t


def test_remove_refuses_bad_arguments_and_survives_an_empty_archive(cuda):
    x = torch.from_numpy(R.make_rows("normal", 40, 5, 3)).to(DEV)
    index = EmbeddingIndex(x[:30])
    for which in (torch.tensor([3, 30], device=DEV), torch.tensor([-1], device=DEV), torch.zeros(29, dtype=torch.bool, device=DEV),
                  torch.zeros(30, dtype=torch.int32, device=DEV), torch.zeros(30, dtype=torch.bool)):
        with pytest.raises(ValueError):
            index.remove(which)
        assert len(index) == 30 and index.generation == 0 and index.ids.tolist() == list(range(30))
    assert _same(index.query(x, 3), EmbeddingIndex(x[:30]).query(x, 3))
    # every row goes: remove itself does not fail, and add starts again with the next ids
    assert index.remove(torch.ones(30, dtype=torch.bool, device=DEV)).shape == (0,)
    assert len(index) == 0 and index.generation == 1 and index.ids.shape == (0,)
    assert index.locate(torch.tensor([0, 29], device=DEV)).tolist() == [-1, -1]
    index.add(x[30:])
    assert index.ids.tolist() == list(range(30, 40)) and _same(index.query(x, 3), EmbeddingIndex(x[30:]).query(x, 3))


# ---- 2. self_rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", INTEGER + ("normal-D32-k15", "normal-D5-k64"))
def test_self_rows_masks_a_scattered_row_as_self_offset_masks_a_run(cuda, name):
    kind, total, d, k, metric, pattern, mode, script, bad = RR.CASES[name]
    x, groups, tx, tg = _device_inputs(name)
    exclude, one = RR.modes(name)
    # (the index has been through a removal: three more rows stood in front and left)
    index = EmbeddingIndex(torch.cat([tx[:3] + 1.0, tx]), metric, groups=None if tg is None else torch.cat([tg[:3], tg]))
    assert index.remove(torch.arange(3, device=DEV)).tolist() == list(range(3, total + 3)) and len(index) == total
    rows = torch.from_numpy(np.random.default_rng(3).permutation(total)[:97].astype(np.int64)).to(DEV)
    kw_all = _group_kw(tg, torch.arange(total, device=DEV), exclude, one)
    want = _np(*(t[rows] for t in index.query(tx, k, self_offset=0, **kw_all)))
    got = _np(*index.query(tx[rows], k, self_rows=rows, **_group_kw(tg, rows, exclude, one)))
    differ = _differ(*got, *want)
    if kind != "integer":
        sep = KG.separated_rows(x, k, metric, groups, exclude, one)[rows.cpu().numpy()]
        assert 1.0 - sep.mean() <= RR.CAP
        differ &= sep
    assert not differ.any(), f"rows {rows[torch.from_numpy(differ).to(DEV)].tolist()[:8]}"
    assert (got[0] != rows.cpu().numpy()[:, None]).all(), "a row is its own neighbour"
    again = _np(*index.query(tx[rows], k, self_rows=rows, splits=7, **_group_kw(tg, rows, exclude, one)))
    assert not _differ(*again, *got).any()


def test_self_rows_refuses_what_it_cannot_honour(cuda):
    x = torch.from_numpy(R.make_rows("normal", 40, 5, 3)).to(DEV)
    rows = torch.arange(8, device=DEV)
    plain, grouped = EmbeddingIndex(torch.cat([x, x[:1]])), EmbeddingIndex(x, groups=torch.arange(40, device=DEV) // 4)
    plain.remove(torch.tensor([40], device=DEV))
    with pytest.raises(ValueError, match="self_offset"):
        plain.query(x[:8], 3, self_rows=rows, self_offset=0)
    with pytest.raises(ValueError, match=r"\[8\]"):
        plain.query(x[:8], 3, self_rows=rows[:7])
    with pytest.raises(ValueError, match="int64"):
        plain.query(x[:8], 3, self_rows=rows.to(torch.int32))
    with pytest.raises(ValueError, match="is on cpu"):
        plain.query(x[:8], 3, self_rows=rows.cpu())
    with pytest.raises(ValueError, match="exclude_same_group=True"):
        grouped.query(x[:8], 3, self_rows=rows)
    with pytest.raises(ValueError, match="exclude_same_group=True"):
        grouped.query(x[:8], 3, self_rows=rows, one_per_group=True)
    ok = grouped.query(x[:8], 3, self_rows=rows, query_groups=grouped.groups[:8], exclude_same_group=True)
    assert _same(ok, grouped.query(x[:8], 3, query_groups=grouped.groups[:8], exclude_same_group=True))


# ---- 3. rules R1-R3 at every update ------------------------------------------------------------------------------------
def _check_update(name, g, index, gcur, after, before_i, before_d, stats, tx, tg):
    """One ``update`` from the rows ``gcur`` (what the graph covered) to ``after`` (what the index holds) against the
    reference.  Returns (damaged bool [s], s, rebuilt)."""
    kind, total, d, k, metric, pattern, mode, script, bad = RR.CASES[name]
    _, groups, _, _ = _device_inputs(name)
    exclude, one = RR.modes(name)
    where = {int(r): j for j, r in enumerate(after)}
    new_of_old = np.array([where.get(int(r), -1) for r in gcur], np.int64)
    s, n1 = int((new_of_old >= 0).sum()), len(after)
    assert (np.diff(new_of_old[new_of_old >= 0]) > 0).all() and (new_of_old[new_of_old >= 0] == np.arange(s)).all()
    got_i, got_d = _np(g.idx, g.dist)
    assert len(g) == n1 and got_i.shape == (n1, k)
    removed = len(gcur) - s
    now = torch.from_numpy(after).to(DEV)
    tg_now = None if tg is None else tg[now]
    g_now = None if groups is None else groups[after]
    if removed == 0:
        assert set(stats) == {"new_rows", "offers", "touched", "changed", "candidates"}, "an update without a removal"
        c_i, c_d, damaged = before_i, before_d, np.zeros(s, bool)
    else:
        c_i, c_d, damaged = RR.compact_lists(before_i, before_d, new_of_old, k, one)
        assert stats["removed"] == removed and stats["damaged"] == int(damaged.sum()) and stats["new_rows"] == n1 - s
        rebuilt = mode == "distinct" and bool(damaged.any())
        assert stats["rebuilt"] is rebuilt
        if rebuilt:
            want = index.query(index.bank, k, self_offset=0, **_group_kw(tg_now, torch.arange(n1, device=DEV), exclude, one))
            assert not _differ(got_i, got_d, *_np(*want)).any(), "the rebuilt graph is not index.query's"
            return damaged, s, True
    # new rows: index.query's lists
    if n1 > s:
        new = torch.arange(s, n1, device=DEV)
        want = index.query(index.bank[s:], k, self_offset=s, **_group_kw(tg_now, new, exclude, one))
        assert not _differ(got_i[s:], got_d[s:], *_np(*want)).any(), "a new row's list is not index.query's"
    # undamaged old rows (R1, R2): the compacted list merged with EVERY eligible new row, distances from radius(+inf)
    want_i, want_d = c_i, c_d
    if n1 > s and s:
        tmp = EmbeddingIndex(index.bank[s:].clone(), metric, groups=None if tg is None else tg_now[s:].clone())
        kw = dict(query_groups=tg_now[:s], exclude_same_group=True) if exclude else {}
        indptr, oi, od = _np(*tmp.radius(index.bank[:s], float("inf"), sort="distance", **kw))
        want_i, want_d = KG.merge_graph(c_i, c_d, indptr, oi + s, od, k, g_now, one)
    wrong = _differ(got_i[:s], got_d[:s], want_i, want_d) & ~damaged
    assert not wrong.any(), f"R1 / R2: undamaged rows {np.flatnonzero(wrong)[:8].tolist()}"
    # damaged rows (R3): index.query's for that row, itself excluded
    if damaged.any():
        rows = torch.from_numpy(np.flatnonzero(damaged)).to(DEV)
        want = index.query(index.bank[rows], k, self_rows=rows, **_group_kw(tg_now, rows, exclude, one))
        wrong = _differ(got_i[:s][damaged], got_d[:s][damaged], *_np(*want))
        assert not wrong.any(), f"R3: damaged rows {np.flatnonzero(damaged)[wrong][:8].tolist()}"
    return damaged, s, False


@functools.lru_cache(maxsize=None)
def _run(name, splits=0, update_after=None, stop=None):
    """Plays a case's script (``stop``: its first steps only) with ``update()`` after every step (or after the steps
    ``update_after`` names) and checks rules R1-R3 at every update.  Returns the final state (numpy; never written)."""
    kind, total, d, k, metric, pattern, mode, script, bad = RR.CASES[name]
    x, groups, tx, tg = _device_inputs(name)
    index = g = None
    gcur, merges, rebuilt_any, damaged_seen, old_undamaged = None, 0, False, 0, None
    steps = RR.states(name)[:stop]
    for t, (step, arg, before, after, keep) in enumerate(steps):
        if step == RR.B:
            index = EmbeddingIndex(tx[:arg], metric, groups=None if tg is None else tg[:arg])
            g = KnnGraph(index, k, metric, group_mode=mode, splits=splits)
            gcur = after
            continue
        _apply(index, step, arg, before, after, keep, tx, tg)
        if update_after is not None and t not in update_after:
            continue
        before_i, before_d = _np(g.idx, g.dist)
        stats = {}
        assert g.update(stats) is g
        damaged, s, rebuilt = _check_update(name, g, index, gcur, after, before_i, before_d, stats, tx, tg)
        # which rows of the final archive were never searched again since the build (their lists went through R1 / R2 only)
        alive = np.isin(gcur, after)
        carried = np.ones(len(gcur), bool) if old_undamaged is None else old_undamaged
        old_undamaged = np.concatenate([carried[alive] & ~damaged & (not rebuilt), np.zeros(len(after) - s, bool)])
        merges = 0 if rebuilt else merges + (len(after) > s and s > 0)
        rebuilt_any |= rebuilt
        damaged_seen += int(damaged.sum())
        gcur = after
    out_i, out_d = _np(g.idx, g.dist)
    for a in (out_i, out_d):
        a.setflags(write=False)
    return dict(rows=gcur, idx=out_i, dist=out_d, merges=merges, rebuilt=rebuilt_any, damaged=damaged_seen,
                old_undamaged=old_undamaged)


@pytest.mark.parametrize("name", list(RR.CASES))
def test_every_update_obeys_rules_r1_to_r3_bit_for_bit(cuda, name):
    res = _run(name)
    assert res["damaged"] > 0, "the script damaged no row"
    assert res["rebuilt"] == (name == "groups-distinct")
    assert np.array_equal(res["rows"], RR.states(name)[-1][3])


def test_a_list_with_a_free_slot_that_loses_an_entry_is_complete_as_it_is(cuda):
    """Twelve rows at k = 15: every list holds every other row, so after a removal nothing is damaged, nothing is
    searched again, and the compacted lists are the rebuilt ones bit for bit."""
    x = torch.from_numpy(R.make_rows("normal", 12, 33, 7)).to(DEV)
    index = EmbeddingIndex(x)
    g = KnnGraph(index, 15)
    kept = index.remove(torch.tensor([2, 7, 8], device=DEV))
    stats = {}
    g.update(stats)
    assert stats == dict(new_rows=0, offers=0, touched=0, changed=0, candidates=0, removed=3, damaged=0, rebuilt=False)
    assert not _differ(*_np(g.idx, g.dist), *_np(*knn_graph(x[kept], 15, False))).any()
    assert int((g.idx >= 0).sum(dim=1).max()) == 8


# ---- 4. against the rebuild (R4) and the contract -----------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in RR.CASES if n not in RR.NOT_REBUILD])
def test_the_updated_graph_equals_the_rebuilt_one_on_separated_rows(cuda, name):
    kind, total, d, k, metric, pattern, mode, script, bad = RR.CASES[name]
    x, groups, tx, tg = _device_inputs(name)
    exclude, one = RR.modes(name)
    res = _run(name)
    now = torch.from_numpy(res["rows"]).to(DEV)
    x_now, g_now = x[res["rows"]], None if groups is None else groups[res["rows"]]
    rebuilt = _np(*knn_graph(tx[now], k, False, metric, groups=None if tg is None else tg[now], group_mode=mode))
    differ = _differ(res["idx"], res["dist"], *rebuilt)
    if kind == "integer":
        assert not differ.any(), f"rows {np.flatnonzero(differ)[:8].tolist()}"
    else:
        sep = KG.separated_rows(x_now, k, metric, g_now, exclude, one)
        share = 1.0 - sep.mean()
        print(f"{name}: non-separated share {share:.4f}, rows that differ from the rebuild {int(differ.sum())}")
        assert share <= RR.CAP
        assert not (differ & sep).any(), f"separated rows {np.flatnonzero(differ & sep)[:8].tolist()} differ from the rebuild"
    worst = KG.check_graph(x_now, res["idx"], res["dist"], k, metric, updates=res["merges"], groups=g_now, exclude=exclude,
                           one=one)
    print(f"{name}: worst rank excess {worst:.3f} tau after {res['merges']} merges")


# ---- 5. independence ---------------------------------------------------------------------------------------------------
def test_splits_do_not_change_a_list(cuda):
    a = _run("normal-D32-k15")
    for splits in (1, 7):
        b = _run("normal-D32-k15", splits=splits)
        assert not _differ(b["idx"], b["dist"], a["idx"], a["dist"]).any(), splits


@pytest.mark.parametrize("name", ("normal-D32-k15", "integer-k15", "groups-exclude"))
def test_how_removals_and_adds_are_cut_between_updates_does_not_matter(cuda, name):
    kind, total, d, k, metric, pattern, mode, script, bad = RR.CASES[name]
    x, groups, tx, tg = _device_inputs(name)
    exclude, one = RR.modes(name)
    # remove; add; update against remove; update; add; update: steps 1 and 2 of the script
    every, joined = _run(name, stop=3), _run(name, update_after=(2,), stop=3)
    assert np.array_equal(every["old_undamaged"], joined["old_undamaged"])
    differ = _differ(joined["idx"], joined["dist"], every["idx"], every["dist"])
    held = every["old_undamaged"] & joined["old_undamaged"]
    if kind != "integer":
        sep = KG.separated_rows(x[every["rows"]], k, metric, None if groups is None else groups[every["rows"]], exclude, one)
        assert pattern is not None or held.sum() > 0      # (a seventh removed at k = 15: about a tenth of the lists lose nothing)
        assert not (differ & (held | sep)).any(), np.flatnonzero(differ & (held | sep))[:8].tolist()
    else:
        assert not differ.any(), np.flatnonzero(differ)[:8].tolist()
    # remove(A); update(); remove(B); update() against remove(A + B); update()
    n0 = script[0][1]
    keep_a = RR.keep_mask(n0, "mod7")
    keep_b = RR.keep_mask(int(keep_a.sum()), "oldest60")
    both = keep_a.copy()
    both[np.flatnonzero(keep_a)[~keep_b]] = False
    graphs = []
    for masks in ((keep_a, keep_b), (both,)):
        index = EmbeddingIndex(tx[:n0], metric, groups=None if tg is None else tg[:n0])
        g = KnnGraph(index, k, metric, group_mode=mode)
        undamaged = np.ones(n0, bool)
        for m in masks:
            before = _np(g.idx, g.dist)
            index.remove(torch.from_numpy(~m).to(DEV))
            stats = {}
            g.update(stats)
            dam = RR.compact_lists(*before, RR.new_of_old_from(m), k, one)[2]
            assert stats["damaged"] == int(dam.sum()) and stats["removed"] == int((~m).sum())
            undamaged = undamaged[m] & ~dam
        graphs.append((_np(g.idx, g.dist), undamaged))
    (two, und_two), (once, und_once) = graphs
    differ = _differ(*two, *once)
    if kind == "integer":
        assert not differ.any()
    else:
        rows = np.flatnonzero(both)
        sep = KG.separated_rows(x[rows], k, metric, None if groups is None else groups[rows], exclude, one)
        assert not und_once[~und_two].any(), "a row undamaged by the union was damaged by a part"
        assert und_once.sum() > 0 and not (differ & (und_once | sep)).any()


# ---- 6. the kernel alone -----------------------------------------------------------------------------------------------
def _hand_lists(rng, n_old, k, fill_share=0.5):
    """Sorted lists as btsbot_knn_query writes them: full, or a random number of present entries; ties in dist."""
    idx = np.full((n_old, k), -1, np.int64)
    dist = np.full((n_old, k), np.inf, np.float32)
    for a in range(n_old):
        want = k if rng.random() < fill_share else int(rng.integers(0, k + 1))
        c = rng.permutation(n_old)[:min(n_old, want)]
        dd = rng.integers(0, 40, size=len(c)).astype(np.float32) / 4
        o = np.lexsort((c, dd))
        idx[a, :len(c)], dist[a, :len(c)] = c[o], dd[o]
    return idx, dist


def _compact_c(idx, dist, new_of_old, k, distinct=False, stride=None, with_counts=True):
    """btsbot_knn_graph_compact: (idx, dist, damaged, counts), and a check that nothing else was written."""
    n_old, stride = len(idx), stride or k
    s = int((new_of_old >= 0).sum())
    ti = torch.full((n_old, stride), -7, dtype=torch.int64, device=DEV)
    td = torch.full((n_old, stride), -7.0, dtype=torch.float32, device=DEV)
    ti[:, :k], td[:, :k] = torch.from_numpy(idx).to(DEV), torch.from_numpy(dist).to(DEV)
    tn = torch.from_numpy(np.asarray(new_of_old, np.int64)).to(DEV)
    oi = torch.full((s + 1, stride), -9, dtype=torch.int64, device=DEV)
    od = torch.full((s + 1, stride), -9.0, dtype=torch.float32, device=DEV)
    dam = torch.full((s + 1,), 5, dtype=torch.uint8, device=DEV)
    counts = torch.tensor([100, 1000], dtype=torch.int32, device=DEV)
    p = lambda a: C.c_void_p(a.data_ptr() if a is not None and a.numel() else 0)    # noqa: E731
    rc = _lib.lib().btsbot_knn_graph_compact(p(ti), p(td), stride, k, n_old, p(tn), p(oi), p(od), stride, s,
                                             1 if distinct else 0, p(dam), p(counts) if with_counts else None,
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "btsbot_knn_graph_compact")
    torch.cuda.synchronize()
    assert bool((oi[:, k:] == -9).all()) and bool((od[:, k:] == -9.0).all()), "the compaction wrote past column k"
    assert bool((oi[s] == -9).all()) and bool((od[s] == -9.0).all()) and int(dam[s]) == 5, "it wrote past row n_new"
    assert bool((ti[:, :k] == torch.from_numpy(idx).to(DEV)).all()), "it wrote to its input"
    c = counts.tolist()
    return oi[:s, :k].cpu().numpy(), od[:s, :k].cpu().numpy(), dam[:s].cpu().numpy(), (c[0] - 100, c[1] - 1000)


def _check_compact(idx, dist, new_of_old, k, distinct=False, **kw):
    want_i, want_d, want_dam = RR.compact_lists(idx, dist, new_of_old, k, distinct)
    got_i, got_d, dam, counts = _compact_c(idx, dist, new_of_old, k, distinct, **kw)
    wrong = _differ(got_i, got_d, want_i, want_d)
    assert not wrong.any(), f"rows {np.flatnonzero(wrong)[:8].tolist()}"
    assert np.array_equal(dam.astype(bool), want_dam) and set(np.unique(dam)) <= {0, 1}
    if kw.get("with_counts", True):
        assert counts == (int(want_dam.sum()), RR.dropped_entries(idx, dist, new_of_old, k)), counts
    else:
        assert counts == (0, 0)
    return int(want_dam.sum())


@pytest.mark.parametrize("k,distinct", [(k, False) for k in (1, 15, 16, 17, 32, 33, 64)] + [(k, True) for k in (1, 16, 17, 32)])
def test_compact_kernel_on_hand_made_lists(cuda, k, distinct):
    rng = np.random.default_rng(200 + k)
    damaged_seen = 0
    for n_old in (1, 5, 257):
        idx, dist = _hand_lists(rng, n_old, k)
        if n_old == 257:
            idx[7], dist[7] = -1, np.nan                          # a NaN row that survives, and one that is removed
            idx[8], dist[8] = -1, np.nan
            idx[9, 0] = n_old + 3                                 # an entry out of range: dropped, never a subscript
            idx[10, min(1, k - 1)] = 1 << 40
        for share in (0.0, 0.3, 1.0):
            keep = rng.random(n_old) >= share
            if n_old == 257:
                keep[7], keep[8] = True, False
            new_of_old = RR.new_of_old_from(keep)
            for stride in (k, k + 3):
                damaged_seen += _check_compact(idx, dist, new_of_old, k, distinct, stride=stride)
        _check_compact(idx, dist, RR.new_of_old_from(rng.random(n_old) >= 0.3), k, distinct, with_counts=False)
    assert damaged_seen > 0


def test_compact_entry_refuses_bad_arguments(cuda):
    L = _lib.lib()
    t = torch.zeros(256, dtype=torch.int64, device=DEV)
    f = torch.zeros(256, dtype=torch.float32, device=DEV)
    o = torch.zeros(256, dtype=torch.int64, device=DEV)
    of = torch.zeros(256, dtype=torch.float32, device=DEV)
    nw = torch.arange(8, dtype=torch.int64, device=DEV)
    dam = torch.zeros(64, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    at = lambda a, off=0: C.c_void_p(a.data_ptr() + off)    # noqa: E731

    def call(k=4, stride=4, out_stride=4, flags=0, n_old=8, n_new=8, idx=at(t), dist=at(f), new=at(nw), out_idx=at(o),
             out_dist=at(of), damaged=at(dam), counts=at(cnt)):
        return L.btsbot_knn_graph_compact(idx, dist, stride, k, n_old, new, out_idx, out_dist, out_stride, n_new, flags,
                                          damaged, counts, None)
    assert call() == _lib.OK and call(counts=None) == _lib.OK
    for kw in (dict(k=0), dict(k=65, stride=65, out_stride=65), dict(k=33, stride=33, out_stride=33, flags=1), dict(stride=3),
               dict(out_stride=3), dict(flags=2), dict(n_old=-1), dict(n_new=-1), dict(n_old=1 << 31), dict(n_new=9),
               dict(idx=None), dict(new=None), dict(out_dist=None), dict(damaged=None),
               dict(idx=at(t, 4)), dict(dist=at(f, 2)), dict(out_idx=at(o, 4)), dict(counts=at(cnt, 2)),
               dict(out_idx=at(t)), dict(out_idx=at(t, 8 * 31)), dict(out_dist=at(f, 4 * 31)), dict(out_idx=at(nw, 0)),
               dict(idx=at(o, 8 * 16))):
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
        assert b"btsbot_knn_graph_compact" in L.btsbot_last_error()
    assert call(n_old=0, n_new=0) == _lib.OK and call(n_new=0, out_idx=None, out_dist=None, damaged=None) == _lib.OK
    torch.cuda.synchronize()


# ---- 7. what hangs on the graph and the index ---------------------------------------------------------------------------
def _same_f64(got, want, rows=None):
    got, want = got.cpu().numpy(), want.cpu().numpy()
    if rows is not None:
        got, want = got[rows], want[rows]
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


@pytest.mark.parametrize("name", ("integer-k15", "normal-D32-k15"))
def test_novelty_model_follows_removals(cuda, name):
    kind, total, d, k, metric, pattern, mode, script, bad = RR.CASES[name]
    x, groups, tx, tg = _device_inputs(name)
    new = torch.from_numpy(R.make_rows(kind, 50, d, 99)).to(DEV)
    index = model = None
    for step, arg, before, after, keep in RR.states(name):
        if step == RR.B:
            index = EmbeddingIndex(tx[:arg], metric)
            model = NoveltyModel(index, k, keep_graph=True)
            continue
        _apply(index, step, arg, before, after, keep, tx, tg)
        with pytest.raises(RuntimeError, match=r"call refit\(\) or update\(\)"):
            model.score(new)
        assert model.update() is model and len(model) == len(index) == len(model.graph) == len(after)
        want = novelty._fit(model.graph.idx, model.graph.dist)
        assert all(_same_f64(getattr(model, f), w) for f, w in zip(("kdist", "lrd", "lof"), want))
        fresh = NoveltyModel(EmbeddingIndex(index.bank.clone(), metric), k, keep_graph=True)
        # a row's fit is a function of its own list and its neighbours' lists (lof: and of theirs)
        same = ~_differ(*_np(model.graph.idx, model.graph.dist), *_np(fresh.graph.idx, fresh.graph.dist))
        if kind == "integer":
            assert same.all()
        nb = _np(fresh.graph.idx)[0]
        ok1 = same & np.where(nb >= 0, same[np.clip(nb, 0, None)], True).all(axis=1)
        ok2 = ok1 & np.where(nb >= 0, ok1[np.clip(nb, 0, None)], True).all(axis=1)
        assert same.mean() >= 1.0 - RR.CAP      # (R4: the graphs differ on non-separated rows only)
        assert _same_f64(model.kdist, fresh.kdist, same) and _same_f64(model.lrd, fresh.lrd, ok1)
        assert _same_f64(model.lof, fresh.lof, ok2)
        got, want = model.score(new, return_lrd=True), fresh.score(new, return_lrd=True)
        qi = _np(index.query(new, k)[0])[0]
        okq = np.where(qi >= 0, ok1[np.clip(qi, 0, None)], True).all(axis=1)
        assert _same_f64(got[0], want[0], okq) and _same_f64(got[1], want[1], okq) and (kind != "integer" or okq.all())


def test_fits_refuse_an_index_that_lost_rows_and_grew_back(cuda):
    x = torch.from_numpy(R.make_rows("normal", 170, 5, 7)).to(DEV)
    index = EmbeddingIndex(x[:150])
    model, clusters = NoveltyModel(index, 10), ClusterModel(index, 5)
    index.remove(torch.arange(20, device=DEV))
    index.add(x[150:])
    assert len(index) == len(model) == len(clusters) == 150
    with pytest.raises(RuntimeError, match=r"index.remove -- call refit\(\)"):
        model.score(x[:4])
    with pytest.raises(RuntimeError, match=r"index.remove -- call refit\(\)"):
        clusters.predict(x[:4])
    assert model.refit().score(x[:4]).shape == (4,) and clusters.refit().predict(x[:4])[0].shape == (4,)


def test_embedding_map_remove_keeps_the_survivors_where_they_are(cuda):
    x = torch.from_numpy(R.make_rows("normal", 200, 8, 7)).to(DEV)
    y = torch.from_numpy(R.make_rows("normal", 200, 2, 8)).to(DEV)
    m = EmbeddingMap.from_positions(x, y, n_neighbors=5)
    first = m.map_index()
    mask = torch.from_numpy(~RR.keep_mask(200, "mod7")).to(DEV)
    kept = m.remove(mask)
    assert torch.equal(kept, (~mask).nonzero().view(-1)) and len(m) == int((~mask).sum()) == m.embedding_.shape[0]
    assert _same(m.embedding_, y[kept]) and _same(m.index.bank, x[kept])
    assert m.map_index() is not first and len(m.map_index()) == len(m)
    # a removed row asked again is attached to survivors only: the same placement as on a map that never held it
    asked = x[mask]
    assert _same(m.transform(asked), EmbeddingMap.from_positions(x[kept], y[kept], n_neighbors=5).transform(asked))
    idx = m.index.query(asked, 5)[0]
    assert bool((idx < len(m)).all()) and not bool((x[kept][idx] == asked[:, None, :]).all(dim=2).any())
