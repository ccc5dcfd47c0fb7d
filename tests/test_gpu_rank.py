"""GPU tests of the neighbour ranks (run with -m gpu on an MI355X): EmbeddingIndex.rank_of / neighbor_ranks against the
radius search (the radius invariant, bit for bit), against the float64 order on integer rows, against the interval
contract of tests/rank_ref.py on float rows, against ``query``, and against themselves (splits, batch cuts,
permutations of rows and columns, runs, incremental index)."""
import numpy as np
import pytest
import torch

import btsbot_amd
import radius_ref as R
import rank_ref as RR

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "cosine")
T_VALUES = (1, 15, 64)


def _gpu(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _np(out):
    return tuple(t.cpu().numpy() for t in out)


def _rank(index, q, targets, **kw):
    """rank_of with stats=; the fill kernel's error flag must be clear"""
    stats = {}
    rank, dist = index.rank_of(q, targets, stats=stats, **kw)
    assert stats["error_flag"] == 0 and stats["band"] >= 0
    assert rank.dtype == torch.int64 and dist.dtype == torch.float32 and rank.shape == dist.shape == targets.shape
    return rank, dist, stats


def _bits(rank, dist):
    return rank.cpu().numpy().tobytes(), dist.cpu().numpy().view(np.int32).tobytes()


def _check_radius_invariant(index, tq, targets, rank, dist, columns, **kw):
    """rank[q, c] is the position of targets[q, c] in radius(q, r = dist[:, c], sort="distance"); returns the number of
    (q, c) compared.  A column's rows without a rank, or with a distance below 0 (1 - cos may round there, and a
    negative radius is refused), are asked with r = 0 and not compared."""
    rank_h, dist_h, tg_h = rank.cpu().numpy(), dist.cpu().numpy(), targets.cpu().numpy()
    seen = 0
    for c in columns:
        use = (rank_h[:, c] >= 0) & (dist_h[:, c] >= 0)
        r = torch.from_numpy(np.where(use, dist_h[:, c], 0).astype(np.float32)).to(tq.device)
        stats = {}
        ip, ii, dd = _np(index.radius(tq, r, sort="distance", stats=stats, **kw))
        assert stats["error_flag"] == 0
        for i in np.flatnonzero(use):
            row, drow = ii[ip[i]:ip[i + 1]], dd[ip[i]:ip[i + 1]]
            at = np.flatnonzero(row == tg_h[i, c])
            assert len(at) == 1, f"row {i} column {c}: the target is not in its own radius list"
            assert at[0] == rank_h[i, c], f"row {i} column {c}: rank {rank_h[i, c]}, position {at[0]} of {len(row)}"
            assert drow[at[0]].view(np.int32) == dist_h[i, c].view(np.int32), f"row {i} column {c}: distance bits"
        seen += int(use.sum())
    return seen


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "Q{}-N{}-D{}-s{}".format(*c))
def test_radius_invariant_on_the_covering_cases(cuda, case, metric):
    n_q, n, dim, splits = case
    seen = 0
    for kind in R.KINDS:
        q, b = R.make_rows(kind, n_q, dim, 1000), R.make_rows(kind, n, dim, 2000)
        m = min(n_q, n)
        b[:m:3] = q[:m:3]                                       # every third query row IS its bank row (self_offset = 0)
        obj_q, obj_b = (np.arange(n_q) % 5).astype(np.int64), (np.arange(n) % 5).astype(np.int64)
        tq, tb, gq, gb = _gpu(cuda, q, b, obj_q, obj_b)
        index = btsbot_amd.EmbeddingIndex(tb, metric, groups=gb)
        for t in T_VALUES:
            (targets,) = _gpu(cuda, RR.random_targets(n_q, n, t, 7 + t))
            columns = sorted({0, t // 2, t - 1})
            for kw in ({}, {"self_offset": 0}, {"query_groups": gq, "exclude_same_group": True}):
                rank, dist, stats = _rank(index, tq, targets, splits=splits, **kw)
                seen += _check_radius_invariant(index, tq, targets, rank, dist, columns, **kw)
    print(f"{case} {metric}: {seen} (q, c) compared with their radius lists")
    assert seen > 0


@pytest.mark.parametrize("dim", [5, 33, 528])
def test_exact_ranks_on_integer_rows(cuda, dim):
    """d^2 is an exact integer: the ranks are the float64 (d^2, index) order, ties (abundant) by the index rule"""
    q, b = R.make_rows("integer", 130, dim, 5), R.make_rows("integer", 1000, dim, 6)
    b[:130:2] = q[::2]
    targets = RR.random_targets(130, 1000, 15, 3)
    targets[:, 14] = targets[:, 0]                              # a repeated target
    targets[:, 13] = np.arange(130)                             # the row itself
    obj_q, obj_b = (np.arange(130) % 7).astype(np.int64), (np.arange(1000) % 7).astype(np.int64)
    tq, tb, tt, gq, gb = _gpu(cuda, q, b, targets, obj_q, obj_b)
    index = btsbot_amd.EmbeddingIndex(tb, groups=gb)
    for splits, kw, ref in ((1, {}, {}), (7, {"self_offset": 0}, {"self_offset": 0}), (0, {}, {}),
                            (2, {"query_groups": gq, "exclude_same_group": True}, {"qgroups": obj_q, "bgroups": obj_b})):
        rank, dist, stats = _rank(index, tq, tt, splits=splits, **kw)
        RR.check_ranks(q, b, targets, *_np((rank, dist)), exact=True, **ref)
        assert stats["band"] > 0
        assert torch.equal(rank[:, 14], rank[:, 0]) and torch.equal(dist[:, 14], dist[:, 0])
    assert (index.rank_of(tq, tt, self_offset=0)[0][:, 13] == -1).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", [c for c in R.CASES if c[2] <= 33], ids=lambda c: "Q{}-N{}-D{}-s{}".format(*c))
def test_interval_contract_on_float_rows(cuda, case, metric):
    n_q, n, dim, splits = case
    for kind in R.KINDS:
        q, b = R.make_rows(kind, n_q, dim, 1000), R.make_rows(kind, n, dim, 2000)
        targets = RR.random_targets(n_q, n, 15, 11)
        tq, tb, tt = _gpu(cuda, q, b, targets)
        rank, dist, stats = _rank(btsbot_amd.EmbeddingIndex(tb, metric), tq, tt, splits=splits)
        share, worst = RR.check_ranks(q, b, targets, *_np((rank, dist)), metric)
        print(f"{case} {metric} {kind}: {share:.4f} of the (q, c) have lo != hi, {stats['band']} band pairs, worst "
              f"distance error {worst:.3f} of the band")
        if (metric, kind) == ("cosine", "clustered"):
            # rows at offset 10 with sigma 0.01: every 1 - cos is about sigma^2 / offset^2 = 1e-6, inside the direct
            # form's ABSOLUTE band 4 (D + 2) u >= 7e-7 -- float64 can order none of these pairs, the interval holds
            # whatever is returned, and this kind rests on the radius invariant above (as the D = 528 cases do)
            continue
        assert share <= 0.05, "a condition on the inputs: too many thresholds the float64 order leaves open"


@pytest.mark.parametrize("metric", METRICS)
def test_ranks_of_the_rows_query_returns(cuda, metric):
    q, b = R.make_rows("normal", 130, 33, 11), R.make_rows("normal", 1000, 33, 12)
    tq, tb = _gpu(cuda, q, b)
    index = btsbot_amd.EmbeddingIndex(tb, metric)
    for k in T_VALUES:
        idx, d = index.query(tq, k)
        rank, dist, _ = _rank(index, tq, idx)
        assert torch.equal(dist.view(torch.int32), d.view(torch.int32))
        assert bool((rank >= torch.arange(k, device=cuda)).all())
        assert bool((rank[:, 1:] > rank[:, :-1]).all())
    if metric == "euclidean":
        # integer rows: the selection's scores are exact (tests/test_rank_host.py), so query returns the first k of the
        # (distance, index) order and their ranks are 0 .. k-1
        tq, tb = _gpu(cuda, R.make_rows("integer", 130, 33, 5), R.make_rows("integer", 1000, 33, 6))
        index = btsbot_amd.EmbeddingIndex(tb)
        for k in T_VALUES:
            idx, d = index.query(tq, k, self_offset=0)
            rank, dist, _ = _rank(index, tq, idx, self_offset=0)
            assert torch.equal(rank, torch.arange(k, device=cuda).expand(130, k))
            assert torch.equal(dist.view(torch.int32), d.view(torch.int32))


@pytest.mark.parametrize("metric", METRICS)
def test_ranks_do_not_depend_on_splits_batching_order_columns_the_run_or_how_the_index_was_built(cuda, metric):
    q, b = R.make_rows("clustered", 130, 33, 3), R.make_rows("clustered", 4099, 33, 4)
    b[1000:1100] = b[:100]                                   # exact duplicates in other tiles
    targets = RR.random_targets(130, 4099, 15, 5)
    targets[:, 1] = np.arange(130) % 100 + 1000              # duplicates as targets
    tq, tb, tt = _gpu(cuda, q, b, targets)
    index = btsbot_amd.EmbeddingIndex(tb, metric)
    rank, dist, stats = _rank(index, tq, tt, splits=1)
    RR.check_ranks(q, b, targets, *_np((rank, dist)), metric)
    ref = _bits(rank, dist)
    for splits in (2, 7, 0, 1):                              # ... and a second run of splits = 1
        assert _bits(*_rank(index, tq, tt, splits=splits)[:2]) == ref, splits
    for cut in (64, 65, 128):
        parts = [_rank(index, tq[a:e], tt[a:e], splits=2)[:2] for a, e in ((0, cut), (cut, 130))]
        assert _bits(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])) == ref, cut
    perm = torch.randperm(130, generator=torch.Generator().manual_seed(5)).to(cuda)
    got = _rank(index, tq[perm], tt[perm].contiguous(), splits=7)
    assert _bits(got[0], got[1]) == _bits(rank[perm], dist[perm])
    cperm = torch.randperm(15, generator=torch.Generator().manual_seed(6)).to(cuda)
    got = _rank(index, tq, tt[:, cperm].contiguous(), splits=3)
    assert _bits(got[0], got[1]) == _bits(rank[:, cperm], dist[:, cperm])
    for c in (0, 1, 14):                                     # a column alone
        got = _rank(index, tq, tt[:, c:c + 1].contiguous())
        assert _bits(got[0], got[1]) == _bits(rank[:, c:c + 1], dist[:, c:c + 1])
    parts = btsbot_amd.EmbeddingIndex(tb[:127], metric)
    parts.add(tb[127:130]).add(tb[130:])
    assert _bits(*_rank(parts, tq, tt, splits=2)[:2]) == ref
    assert _bits(*btsbot_amd.neighbor_ranks(tq, tb, tt, metric)) == ref


@pytest.mark.parametrize("metric", METRICS)
def test_edges(cuda, metric):
    # N = 1 and t = 1
    (one,) = _gpu(cuda, R.make_rows("normal", 1, 5, 1))
    rank, dist, _ = _rank(btsbot_amd.EmbeddingIndex(one, metric), one, torch.zeros((1, 1), dtype=torch.int64, device=cuda))
    assert rank.tolist() == [[0]] and abs(dist.item()) < 1e-6
    # targets out of range, non-finite target and query rows
    q, b = R.make_rows("normal", 5, 33, 1), R.make_rows("normal", 300, 33, 2)
    b[[3, 128], [0, 5]] = [np.nan, np.inf]
    q[2, 7] = np.nan
    targets = RR.random_targets(5, 300, 4, 2)
    targets[:, 0] = [-1, 300, 7, 3, 128]
    targets[1, 1] = 2 ** 40
    targets[:, 2:] = [[10, 299], [0, 127], [129, 5], [299, 299], [64, 0]]
    tq, tb, tt = _gpu(cuda, q, b, targets)
    for splits in (1, 3):
        rank, dist, _ = _rank(btsbot_amd.EmbeddingIndex(tb, metric), tq, tt, splits=splits)
        rank_h, dist_h = _np((rank, dist))
        RR.check_ranks(q, b, targets, rank_h, dist_h, metric)
        assert rank_h[:, 0].tolist() == [-1] * 5 and np.isnan(dist_h[:, 0]).all() and (rank_h[2] == -1).all()
        assert rank_h[1, 1] == -1 and np.isnan(dist_h[1, 1]) and (rank_h[[0, 1, 3, 4], 2:] >= 0).all()
    # no queries, an empty bank
    index = btsbot_amd.EmbeddingIndex(tb, metric)
    rank, dist = index.rank_of(tq[:0], tt[:0])
    assert rank.shape == dist.shape == (0, 4) and rank.dtype == torch.int64
    rank, dist = btsbot_amd.neighbor_ranks(tq, tb[:0], tt, metric)
    assert (rank == -1).all() and torch.isnan(dist).all()


def test_identical_rows_rank_by_index_and_max_band(cuda):
    """every pair is in the band: the ranks are the index order (less the masked self)"""
    b = np.tile(R.make_rows("normal", 1, 31, 1), (300, 1))
    (tb,) = _gpu(cuda, b)
    targets = torch.arange(300, device=cuda).view(300, 1).repeat(1, 3)
    targets[:, 1] = (targets[:, 1] * 7) % 300
    targets[:, 2] = 299 - targets[:, 2]
    for metric in METRICS:
        index = btsbot_amd.EmbeddingIndex(tb, metric)
        rank, dist, stats = _rank(index, tb, targets, splits=2)
        assert torch.equal(rank, targets) and bool((dist == dist[0, 0]).all()) and stats["band"] == 300 * 300
        rank, _, stats = _rank(index, tb, targets, self_offset=0)
        rows = torch.arange(300, device=cuda)[:, None]
        want = torch.where(targets == rows, torch.full_like(targets, -1), targets - (rows < targets).to(torch.int64))
        assert torch.equal(rank, want) and stats["band"] == 300 * 299
        assert index.rank_of(tb, targets, max_band=300 * 300)[0].shape == (300, 3)
        with pytest.raises(ValueError, match=f"holds {300 * 300} pairs"):
            index.rank_of(tb, targets, max_band=300 * 300 - 1)
