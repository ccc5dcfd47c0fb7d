"""IvfIndex by source on the GPU: ``exclude_same_group`` and ``one_per_group`` in the probed search against the contract of
ivf_group_ref.py.  The lists are controlled as in test_gpu_ivf.py -- centroids that differ along
the first axis only, rows moved next to the centroid of the list they are meant for --, the group patterns are
knn_group_ref's, and a query row's group is that of its nearest allowed bank row, so an exclusion always removes the row the
ungrouped search would return first.

Every contract case asserts its premises on the float64 restatement before the device is asked, for at least half of its
finite query rows:
  (i)    the ungrouped answer holds a row of the query's group                                  (modes that exclude)
  (ii)   the ungrouped answer holds two rows of one group                                       (modes that collapse)
  (iii)  some group OF THE ANSWER has eligible rows in two different probed lists, and its nearest row is not in the list of
         the query's nearest centroid: the merge is where that group's best is found            (modes that collapse)
  (few)  fewer eligible groups than k                                                           (case e)
  (none) the exclusion leaves nothing                                                           (case e, one group)
Which premises a case carries is in CASES: `runs` and `negative` give every run of 1-9 consecutive rows a group of its own,
which lies in one list but for the runs on a list edge, so (iii) belongs to the patterns that put every group into every
list (a, c), and (ii) to those and to d, whose k = 32 of 4,099 rows in runs holds two rows of a run.  In a only one group
has rows in two lists (list 1 holds one row), and it is the query's own where a query's nearest row is that row: there
(iii) is a premise of "distinct" alone ("iii-").  Two thirds of c's queries are meant for lists of fewer than 40 rows,
which lack some of the 40 groups whatever the kind of rows."""
import functools

import numpy as np
import pytest
import torch

import btsbot_amd
import ivf_group_ref as G
import ivf_ref as V
import knn_group_ref as KG
import knn_ref as R
from btsbot_amd import neighbors
from knn_group_ref import MODES
from test_gpu_ivf import BASE, CASES as PLAIN, SIGMA, STEP, _bits, _np, _same, _sizes_40, _spread

pytestmark = pytest.mark.gpu

CROWDED = [129, 0, 700, 1, 128, 42, 0, 0]
SMALL_40 = [l for l, s in enumerate(_sizes_40()) if s < 40]
# name: (Q, N, D, k, list sizes, nprobe, group pattern, the list each query row is meant for, NaN rows, premises)
CASES = {
    "a": (65, 129, 33, 15, [0, 1, 128, 0], 4, "mod3", [(0, 3, 1, 0, 3, 2)[i % 6] for i in range(65)], False, "i ii iii-"),
    "b": (130, 1000, 528, 15, CROWDED, 4, "runs", [2] * 130, False, "i"),
    "b-nan": (130, 1000, 528, 15, CROWDED, 4, "runs", [2] * 130, True, "i"),
    "c": (300, 4099, 33, 32, _sizes_40(), 32, "mod40_hi32",
          [i % 40 if i % 3 == 0 else SMALL_40[i % len(SMALL_40)] for i in range(300)], False, "i ii iii"),
    "d": (300, 4099, 33, 32, _sizes_40(), 32, "negative", None, False, "i ii"),
    "e-one": (130, 1000, 33, 32, PLAIN["k-above-allowed"][4], 4, "one", PLAIN["k-above-allowed"][6], True, "i none"),
    "e-distinct": (130, 1000, 33, 32, PLAIN["k-above-allowed"][4], 4, "distinct", PLAIN["k-above-allowed"][6], True, "i few"),
    "f": (1, 1, 1, 1, [1], 1, "runs", [0], False, "i"),
}


@functools.lru_cache(maxsize=None)
def _reference(name, kind):
    """The case's inputs and everything the float64 restatement says about them (shared by the modes; left unchanged)."""
    n_q, n, d, k, sizes, nprobe, pattern, q_lists, nan, _prem = CASES[name]
    assert sum(sizes) == n
    step, base = STEP[kind], BASE[kind]
    b_lists = _spread(sizes)
    q_lists = np.arange(n_q) % len(sizes) if q_lists is None else np.asarray(q_lists)
    b = V.laid_out(R.make_rows(kind, n, d, 2000), b_lists, len(sizes), step, base, SIGMA[kind])
    q = V.laid_out(R.make_rows(kind, n_q, d, 1000), q_lists, len(sizes), step, base, SIGMA[kind])
    c = V.axis_centroids(len(sizes), d, step, base)
    sizes = np.asarray(sizes).copy()
    labels = b_lists.astype(np.int64)
    if nan:
        for r in (0, 130, n - 1):
            sizes[b_lists[r]] -= 1
            labels[r] = -1
            b[r, r % d] = np.nan
        q[0, 0] = np.inf
        q[n_q - 1, d - 1] = np.nan
    bg = KG.make_groups(pattern, n)
    probes = V.probes64(q, c, nprobe)
    al = V.allowed_mask(b, labels, probes)
    plain, _ = V.query64(q, b, c, k, nprobe, labels=labels)
    qg = np.where(plain[:, 0] >= 0, bg[np.maximum(plain[:, 0], 0)], bg[0])
    return dict(q=q, b=b, c=c, sizes=sizes, k=k, nprobe=nprobe, labels=labels, probes=probes, al=al, plain=plain, qg=qg,
                bg=bg, dm=R.dist64_matrix(q, b, "euclidean"))


def _premises(ref, exclude):
    """{premise: bool per finite query row} from the restatement alone."""
    q, bg, qg, plain, labels, k = ref["q"], ref["bg"], ref["qg"], ref["plain"], ref["labels"], ref["k"]
    el = G.eligible(ref["al"], qg, bg, exclude)
    answer, _ = G.group_answer64(q, ref["b"], k, ref["al"], qg, bg, exclude, True)
    out = {p: [] for p in ("i", "ii", "iii", "few", "none")}
    for i in np.flatnonzero(V.usable_rows(q)):
        got = plain[i][plain[i] >= 0]
        out["i"].append(bool((bg[got] == qg[i]).any()))
        out["ii"].append(len(set(bg[got].tolist())) < len(got))
        cols = np.flatnonzero(el[i])
        o = np.lexsort((ref["dm"][i, cols], bg[cols]))                     # by group, then distance
        g, lab = bg[cols][o], labels[cols][o]
        first = np.flatnonzero(np.r_[True, g[1:] != g[:-1]]) if len(g) else np.zeros(0, np.int64)
        spans = np.add.reduceat(np.r_[False, (g[1:] == g[:-1]) & (lab[1:] != lab[:-1])], first) > 0 if len(g) else first
        met = spans & (lab[first] != ref["probes"][i, 0]) & np.isin(g[first], bg[answer[i][answer[i] >= 0]]) if len(g) else first
        out["iii"].append(bool(met.any()))
        out["few"].append(len(first) < k)
        out["none"].append(len(cols) == 0)
    return {p: np.asarray(v) for p, v in out.items()}


def _check_premises(name, kind, mode):
    ref = _reference(name, kind)
    ex, one = MODES[mode]
    hold = _premises(ref, ex)
    for p in CASES[name][9].split():
        if p == "iii-" and mode != "distinct":
            continue
        p = p.rstrip("-")
        if (p == "i" and not ex) or (p in ("ii", "iii", "few") and not one) or (p == "none" and not ex):
            continue
        assert 2 * int(hold[p].sum()) >= len(hold[p]), (f"case {name} {kind} {mode}: premise ({p}) holds for {int(hold[p].sum())} "
                                                         f"of {len(hold[p])} finite query rows: the case is wrong")


def _build(cuda, b, c, groups=None):
    return btsbot_amd.IvfIndex(torch.from_numpy(b).to(cuda), centroids=torch.from_numpy(c).to(cuda),
                               groups=None if groups is None else torch.from_numpy(groups).to(cuda))


def _kw(cuda, mode, qg):
    ex, one = MODES[mode]
    return dict(query_groups=torch.from_numpy(np.ascontiguousarray(qg)).to(cuda), exclude_same_group=ex, one_per_group=one)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_contract_on_the_covering_cases(cuda, name, mode, kind):
    _check_premises(name, kind, mode)
    ref = _reference(name, kind)
    q, b, k, nprobe, qg, bg = (ref[x] for x in ("q", "b", "k", "nprobe", "qg", "bg"))
    ex, one = MODES[mode]
    ivf = _build(cuda, b, ref["c"], bg)
    assert ivf.list_sizes.tolist() == ref["sizes"].tolist(), "the case's lists are not the ones it was laid out for"
    assert torch.equal(ivf.groups, torch.from_numpy(bg).to(cuda))
    tq = torch.from_numpy(q).to(cuda)
    labels, probes = _np(ivf.labels, ivf.probes(tq, nprobe))
    got = ivf.query(tq, k, nprobe, **_kw(cuda, mode, qg))
    idx, dist = _np(*got)
    worst = G.check_group_allowed(q, b, idx, dist, k, V.allowed_mask(b, labels, probes), qg, bg, ex, one)
    print(f"{name} {mode} {kind}: distance error {worst[0]:.2f} of the bound, rank excess {worst[1]:.3f} tau")
    if nprobe == len(ref["sizes"]):
        KG.check_group_neighbors(q, b, idx, dist, k, query_groups=qg, bank_groups=bg, exclude=ex, one=one)
        assert _same(got, ivf.index.query(tq, k, **_kw(cuda, mode, qg))), "every list probed is not the exact grouped search"


@pytest.mark.parametrize("d", [5, 33, 528])
def test_exact_answers_on_integer_rows(cuda, d):
    b, q = R.make_rows("integer", 1000, d, 5), R.make_rows("integer", 65, d, 6)
    c = b[[0, 5, 11, 17, 23]].copy()
    bg = KG.make_groups("mod40", 1000)
    ivf = _build(cuda, b, c, bg)
    tq, tb = torch.from_numpy(q).to(cuda), torch.from_numpy(b).to(cuda)
    labels = _np(ivf.labels)[0]
    assert (labels == V.assign64(b, c)).all() and int(ivf.list_sizes.max()) > 129
    sr = torch.arange(65, device=cuda) * 3
    for mode, (ex, one) in MODES.items():
        for nprobe in (1, 2):
            probes = _np(ivf.probes(tq, nprobe))[0]
            assert (probes == V.probes64(q, c, nprobe)).all()
            al = V.allowed_mask(b, labels, probes)
            qg = bg[V.query64(q, b, c, 1, nprobe, labels=labels)[0][:, 0]]
            idx, dist = _np(*ivf.query(tq, 15, nprobe, **_kw(cuda, mode, qg)))
            G.check_group_exact_allowed(q, b, idx, dist, 15, al, qg, bg, ex, one)
        # a query row that IS a bank row leaves by position; its group stays unless the mode excludes it
        qg = bg[::3][:65]
        idx, dist = _np(*ivf.query(tb[sr], 15, 2, self_rows=sr, **_kw(cuda, mode, qg)))
        al = V.allowed_mask(b, labels, _np(ivf.probes(tb[sr], 2))[0], sr.cpu().numpy())
        G.check_group_exact_allowed(b[::3][:65], b, idx, dist, 15, al, qg, bg, ex, one)
        # every list probed: the exact grouped search, bit for bit
        qg = bg[V.brute64(q, b, 1)[:, 0]]
        full = ivf.query(tq, 15, 5, **_kw(cuda, mode, qg))
        KG.check_group_exact(q, b, *_np(*full), 15, query_groups=qg, bank_groups=bg, exclude=ex, one=one)
        assert _same(full, ivf.index.query(tq, 15, **_kw(cuda, mode, qg)))


@pytest.mark.parametrize("mode", list(MODES))
def test_a_row_answers_alone_as_in_any_call(cuda, mode):
    sizes = CROWDED
    b = V.laid_out(R.make_rows("normal", 1000, 33, 2000), _spread(sizes), 8, STEP["normal"])
    q = V.laid_out(R.make_rows("normal", 130, 33, 77), np.arange(130) % 8, 8, STEP["normal"])
    c = V.axis_centroids(8, 33, STEP["normal"])
    bg = KG.make_groups("runs", 1000)
    k, nprobe = 15, 3
    qg = bg[V.query64(q, b, c, 1, nprobe)[0][:, 0]]
    ivf = _build(cuda, b, c, bg)
    tq = torch.from_numpy(q).to(cuda)
    kw = _kw(cuda, mode, qg)
    idx, dist = ivf.query(tq, k, nprobe, **kw)
    assert _same((idx, dist), ivf.query(tq, k, nprobe, **kw)), "a second run differs"
    assert _same((idx[7:8], dist[7:8]), ivf.query(tq[7:8], k, nprobe, **_kw(cuda, mode, qg[7:8]))), "row 7 alone differs"
    perm = np.random.default_rng(1).integers(0, 130, 400)                          # permuted and duplicated
    tp = torch.from_numpy(perm).to(cuda)
    assert _same((idx[tp], dist[tp]), ivf.query(tq[tp], k, nprobe, **_kw(cuda, mode, qg[perm]))), "a permuted call differs"
    # grown by three adds on the same centroids
    tb, tc, tg = torch.from_numpy(b).to(cuda), torch.from_numpy(c).to(cuda), torch.from_numpy(bg).to(cuda)
    grown = btsbot_amd.IvfIndex(tb[:100], centroids=tc, groups=tg[:100])
    for lo, hi in ((100, 300), (300, 700), (700, 1000)):
        grown.add(tb[lo:hi], groups=tg[lo:hi])
    assert torch.equal(grown.labels, ivf.labels) and torch.equal(grown.groups, ivf.groups)
    assert _same((idx, dist), grown.query(tq, k, nprobe, **kw)), "an index grown by three adds differs"
    # remove, then the survivors against a fresh index on them with groups[kept]
    gone = torch.from_numpy(np.random.default_rng(2).choice(1000, 333, replace=False)).to(cuda)
    kept = grown.remove(gone)
    fresh = btsbot_amd.IvfIndex(tb[kept], centroids=tc, groups=tg[kept])
    assert torch.equal(grown.groups, tg[kept]) and torch.equal(grown.labels, fresh.labels)
    after = grown.query(tq, k, nprobe, **kw)
    assert _same(after, fresh.query(tq, k, nprobe, **kw)), "after remove the index differs from a fresh one"
    ex, one = MODES[mode]
    labels, probes = _np(grown.labels, grown.probes(tq, nprobe))
    G.check_group_allowed(q, b[kept.cpu().numpy()], *_np(*after), k, V.allowed_mask(b[kept.cpu().numpy()], labels, probes), qg,
                          bg[kept.cpu().numpy()], ex, one)


def test_the_ungrouped_path_is_untouched_by_the_groups(cuda):
    ref = _reference("b", "normal")
    with_groups, without = _build(cuda, ref["b"], ref["c"], ref["bg"]), _build(cuda, ref["b"], ref["c"])
    assert without.groups is None
    tq = torch.from_numpy(ref["q"]).to(cuda)
    for nprobe in (1, 4):
        assert _same(with_groups.query(tq, 15, nprobe), without.query(tq, 15, nprobe))
    sr = torch.arange(130, device=cuda) * 7
    tb = with_groups.index.bank
    assert _same(with_groups.query(tb[sr], 15, 4, self_rows=sr), without.query(tb[sr], 15, 4, self_rows=sr))
    assert _same(with_groups.knn_graph(5, nprobe=4), without.knn_graph(5, nprobe=4))
    with pytest.raises(ValueError, match="built with groups"):
        without.knn_graph(5, nprobe=4, group_mode="exclude")


def test_knn_graph_by_group_mode(cuda):
    rng = np.random.default_rng(9)
    lists = np.arange(300) % 6
    emb = V.laid_out(rng.standard_normal((300, 16)).astype(np.float32), lists, 6, 4.0)
    emb[200] = emb[5]                 # a duplicate, of another group
    emb[17, 3] = np.nan
    obj = KG.make_groups("mod40", 300)
    te, tobj = torch.from_numpy(emb).to(cuda), torch.from_numpy(obj).to(cuda)
    ivf = _build(cuda, emb, V.axis_centroids(6, 16, 4.0), obj)
    rows = torch.arange(300, device=cuda)[:, None]
    self_col = neighbors.knn_graph(te, 1)[0][:, 0]              # the row itself, -1 for the NaN row
    for mode, (ex, one) in MODES.items():
        for include_self in (True, False):
            want = neighbors.knn_graph(te, 6, include_self, groups=tobj, group_mode=mode)
            got = ivf.knn_graph(6, include_self, nprobe=6, group_mode=mode)
            assert _same(got, want), f"{mode}, include_self={include_self}: with every list probed the graph is not knn_graph's"
            assert bool(torch.isnan(got[1][17]).all()) and bool((got[0][17] == -1).all())
        idx, dist = ivf.knn_graph(6, nprobe=2, group_mode=mode)
        others, od = idx[:, 1:].contiguous(), dist[:, 1:].contiguous()
        assert torch.equal(idx[:, 0], self_col)
        assert not bool((others == rows).any()), "a row is its own neighbour"
        if not ex:
            assert int(idx[5, 1]) == 200 and float(dist[5, 1]) == 0.0 and int(idx[200, 1]) == 5
        sr = np.arange(300, dtype=np.int64)
        al = V.allowed_mask(emb, ivf.labels.cpu().numpy(), ivf.probes(te, 2).cpu().numpy(), sr)
        G.check_group_allowed(emb, emb, *_np(others, od), 5, al, obj, obj, ex, one)


def test_neighbours_of_an_alert_are_its_own_object_until_it_is_excluded(cuda):
    """2560 alerts: 512 objects of 5 alerts (sigma 1e-3) on the 32-D ten-cluster set, 16 lists fitted by IvfIndex itself,
    nprobe 4.  Ungrouped, an alert's nearest rows are its own object in every slot that an allowed epoch of it can fill;
    with group_mode="exclude" never.  The label purity of the excluded graph -- alerts all of whose neighbours carry the
    alert's label, by neighbor_vote -- is held to the float64 brute force over the same allowed sets minus two alerts."""
    rows, obj, lab = KG.object_set()
    t, tobj, tlab = (torch.from_numpy(a).to(cuda) for a in (rows, obj, lab))
    ivf = btsbot_amd.IvfIndex(t, 16, groups=tobj)
    n = len(rows)
    al = V.allowed_mask(rows, ivf.labels.cpu().numpy(), ivf.probes(t, 4).cpu().numpy(), np.arange(n))
    idx, _ = ivf.knn_graph(4, include_self=False, nprobe=4)
    own = torch.from_numpy((al & (obj[None, :] == obj[:, None])).sum(1)).to(cuda)           # allowed other epochs: <= 4
    slot = torch.arange(4, device=cuda)[None, :] < own[:, None]
    assert float((own == 4).float().mean()) >= 0.9, "the fit cuts most objects apart: the case is wrong"
    assert bool((tobj[idx.clamp(min=0)] == tobj[:, None])[slot].all()) and bool((idx >= 0)[slot].all())
    idx, dist = ivf.knn_graph(5, include_self=False, nprobe=4, group_mode="exclude")
    assert bool((idx >= 0).all()) and not bool((tobj[idx] == tobj[:, None]).any())
    G.check_group_allowed(rows, rows, *_np(idx, dist), 5, al, obj, obj, True, False)
    votes = torch.stack([btsbot_amd.neighbor_vote(idx, dist, (tlab == c).long()) for c in range(10)], dim=1)
    pure = int((votes[torch.arange(n, device=cuda), tlab] == 1.0).sum())
    x = rows.astype(np.float64)
    d2 = (x * x).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * x @ x.T
    nn = np.argsort(np.where(al & (obj[None, :] != obj[:, None]), d2, np.inf), axis=1, kind="stable")[:, :5]
    pure64 = int((lab[nn] == lab[:, None]).all(axis=1).sum())
    print(f"label purity of the excluded graph at nprobe 4 of 16: device {pure / n:.4f}, float64 over the same allowed sets "
          f"{pure64 / n:.4f}")
    assert pure >= pure64 - 2
    # the nearest SOURCES: five distinct objects, none of them the alert's own
    idx, _ = ivf.knn_graph(5, include_self=False, nprobe=4, group_mode="exclude+distinct")
    near = tobj[idx].cpu().numpy()
    assert all(len(set(r.tolist())) == 5 for r in near) and (near != obj[:, None]).all()
