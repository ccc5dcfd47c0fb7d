"""GPU tests of the radius search (run with -m gpu on an MI355X): EmbeddingIndex.radius / count_within / radius_neighbors /
radius_graph against the float64 brute force on the host under the contract of tests/radius_ref.py (validity, returned
distance, must-in, must-out, a free band that holds at most 1 % of the pairs within r), exact lists on integer rows,
bit-equality with ``query`` and with themselves (splits, batch cuts, permutation, runs, incremental index)."""
import numpy as np
import pytest
import torch

import btsbot_amd
import radius_ref as R

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "cosine")


def _gpu(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _np(out):
    return tuple(t.cpu().numpy() for t in out)


def _rows(out):
    """a CSR as one (indices bytes, distance bytes) pair per row: what bit-equality compares"""
    ip, ii, dd = _np(out)
    return [(ii[a:b].tobytes(), dd[a:b].tobytes()) for a, b in zip(ip[:-1], ip[1:])]


def _radius_for(q, b, dim, metric, **kw):
    d = R.d64_matrix(q, b, metric)
    el = R.eligible(q, b, **kw)
    r = R.pick_radius(d, el, dim, metric)
    assert R.band_share(d, el, r, dim, metric) <= 0.01, "a condition on the inputs: the free band holds too many pairs"
    return r


def _call(fn, *args, **kw):
    """the call with stats=; the fill kernel's error flag must be clear"""
    stats = {}
    out = fn(*args, stats=stats, **kw)
    assert stats["error_flag"] == 0 and stats["total"] == out[1].shape[0] <= stats["candidates"]
    return out, stats


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "Q{}-N{}-D{}-s{}".format(*c))
def test_contract_on_the_covering_cases(cuda, case, metric):
    n_q, n, dim, splits = case
    for kind in R.KINDS:
        q, b = R.make_rows(kind, n_q, dim, 1000), R.make_rows(kind, n, dim, 2000)
        r = _radius_for(q, b, dim, metric)
        tq, tb = _gpu(cuda, q, b)
        out, stats = _call(btsbot_amd.radius_neighbors, tq, tb, r, metric, splits=splits)
        worst, n_free, free_taken = R.check_radius(q, b, r, *_np(out), metric)
        print(f"{case} {metric} {kind}: r = {r:.6g}, {stats['total']} pairs of {stats['candidates']} candidates "
              f"({n_q * n} in all), worst distance error {worst:.3f} of the band, free band {free_taken}/{n_free}")


@pytest.mark.parametrize("dim", [5, 33, 528])
def test_exact_lists_on_integer_rows(cuda, dim):
    """d^2 is an integer and r = fp32(sqrt(m)) for an m that occurs: the lists are {d^2 <= m}, boundary pairs included"""
    q, b = R.make_rows("integer", 130, dim, 5), R.make_rows("integer", 1000, dim, 6)
    d2 = R.dist64_matrix(q, b, "euclidean")
    assert (d2 == np.round(d2)).all()
    vals = np.unique(d2[d2 > 0])
    m = float(vals[len(vals) // 3])
    assert (d2 == m).sum() > 0
    r = float(np.float32(np.sqrt(m)))
    tq, tb = _gpu(cuda, q, b)
    for splits, sort in ((1, "index"), (7, "index"), (2, "distance"), (0, "distance")):
        (ip, ii, dd), _ = _call(btsbot_amd.radius_neighbors, tq, tb, r, splits=splits, sort=sort)
        ip, ii, dd = _np((ip, ii, dd))
        for i in range(130):
            want = np.flatnonzero(d2[i] <= m)
            if sort == "distance":
                want = want[np.lexsort((want, d2[i, want]))]
            assert np.array_equal(ii[ip[i]:ip[i + 1]], want), f"row {i} splits {splits}"
            assert np.array_equal(dd[ip[i]:ip[i + 1]], np.sqrt(d2[i, want]).astype(np.float32))


@pytest.mark.parametrize("metric", METRICS)
def test_query_rows_within_r_are_the_head_of_the_radius_list(cuda, metric):
    q, b = R.make_rows("normal", 130, 33, 11), R.make_rows("normal", 1000, 33, 12)
    d = R.d64_matrix(q, b, metric)
    r = R.pick_radius(d, R.eligible(q, b), 33, metric, fractions=(0.02,))
    tq, tb = _gpu(cuda, q, b)
    index = btsbot_amd.EmbeddingIndex(tb, metric)
    (ip, ii, dd), _ = _call(index.radius, tq, r, sort="distance")
    ip, ii, dd = _np((ip, ii, dd))
    r32 = np.float32(r)
    seen = 0
    for k in (1, 15, 64):
        idx, dist = _np(index.query(tq, k))
        for i in range(130):
            sel = dist[i] <= r32
            m = int(sel.sum())
            seen += m
            assert m <= ip[i + 1] - ip[i]
            assert np.array_equal(idx[i][sel], ii[ip[i]:ip[i] + m]), (k, i)
            assert np.array_equal(dist[i][sel].view(np.int32), dd[ip[i]:ip[i] + m].view(np.int32)), (k, i)
            if m < k:
                assert ip[i + 1] - ip[i] == m, (k, i)
    assert seen > 1000


@pytest.mark.parametrize("metric", METRICS)
def test_lists_do_not_depend_on_splits_batching_order_the_run_or_how_the_index_was_built(cuda, metric):
    q, b = R.make_rows("clustered", 130, 33, 3), R.make_rows("clustered", 4099, 33, 4)
    b[1000:1100] = b[:100]                                   # exact duplicates in other tiles
    r = _radius_for(q, b, 33, metric)
    tq, tb = _gpu(cuda, q, b)
    index = btsbot_amd.EmbeddingIndex(tb, metric)
    for sort in ("index", "distance"):
        ref, _ = _call(index.radius, tq, r, splits=1, sort=sort)
        R.check_radius(q, b, r, *_np(ref), metric, sort=sort)
        ref = _rows(ref)
        for splits in (2, 7, 0, 1):                          # ... and a second run of splits = 1
            assert _rows(_call(index.radius, tq, r, splits=splits, sort=sort)[0]) == ref, splits
        singles = [_rows(index.radius(tq[i:i + 1], r, splits=2, sort=sort))[0] for i in (0, 1, 63, 64, 129)]
        assert singles == [ref[i] for i in (0, 1, 63, 64, 129)]
        perm = torch.randperm(130, generator=torch.Generator().manual_seed(5)).to(cuda)
        got = _rows(index.radius(tq[perm], r, splits=7, sort=sort))
        assert got == [ref[i] for i in perm.tolist()]
        parts = btsbot_amd.EmbeddingIndex(tb[:127], metric)
        parts.add(tb[127:130]).add(tb[130:])
        assert _rows(parts.radius(tq, r, splits=2, sort=sort)) == ref
        assert _rows(btsbot_amd.radius_neighbors(tq, tb, r, metric, sort=sort)) == ref


def test_r_zero_returns_the_duplicates(cuda):
    b = R.make_rows("scaled", 1200, 31, 8)
    b[1000:1100] = b[:100]
    (tb,) = _gpu(cuda, b)
    (ip, ii, dd), _ = _call(btsbot_amd.radius_neighbors, tb[:130], tb, 0.0, splits=7)
    ip, ii, dd = _np((ip, ii, dd))
    assert (dd == 0).all()
    for i in range(130):
        assert ii[ip[i]:ip[i + 1]].tolist() == ([i, 1000 + i] if i < 100 else [i])
    ip, ii, dd = _np(btsbot_amd.radius_graph(tb, 0.0, include_self=False))
    assert np.array_equal(ii, np.r_[np.arange(1000, 1100), np.arange(100)]) and (np.diff(ip) <= 1).all()


@pytest.mark.parametrize("metric", METRICS)
def test_r_infinite_returns_every_finite_row_and_bad_rows_have_no_part(cuda, metric):
    q, b = R.make_rows("normal", 5, 33, 1), R.make_rows("normal", 300, 33, 2)
    b[[3, 128, 299], [0, 5, 31]] = [np.nan, np.inf, -np.inf]
    q[2, 7] = np.nan
    tq, tb = _gpu(cuda, q, b)
    good = np.setdiff1d(np.arange(300), [3, 128, 299])
    for splits in (1, 3):
        out, _ = _call(btsbot_amd.radius_neighbors, tq, tb, float("inf"), metric, splits=splits)
        ip, ii, dd = _np(out)
        assert np.diff(ip).tolist() == [297, 297, 0, 297, 297]
        for i in (0, 1, 3, 4):
            assert np.array_equal(ii[ip[i]:ip[i + 1]], good)
        R.check_radius(q, b, np.inf, ip, ii, dd, metric)
    r = _radius_for(q, b, 33, metric)
    out, _ = _call(btsbot_amd.radius_neighbors, tq, tb, r, metric, sort="distance")
    R.check_radius(q, b, r, *_np(out), metric, sort="distance")
    assert out[0][3] == out[0][2]                                  # the non-finite query row's list is empty


@pytest.mark.parametrize("metric", METRICS)
def test_per_row_radii_equal_the_scalar_form_row_by_row(cuda, metric):
    q, b = R.make_rows("normal", 65, 31, 1), R.make_rows("normal", 1000, 31, 2)
    d = R.d64_matrix(q, b, metric)
    el = R.eligible(q, b)
    radii = [R.pick_radius(d, el, 31, metric, fractions=(f,)) for f in (0.01, 0.05, 0.2)]
    per_row = np.array([radii[i % 3] for i in range(65)], np.float32)
    tq, tb = _gpu(cuda, q, b)
    index = btsbot_amd.EmbeddingIndex(tb, metric)
    got, _ = _call(index.radius, tq, torch.from_numpy(per_row).to(cuda), splits=2)
    R.check_radius(q, b, per_row.astype(np.float64), *_np(got), metric)
    got = _rows(got)
    for j, r in enumerate(radii):
        want = _rows(index.radius(tq, r, splits=7))
        assert all(got[i] == want[i] for i in range(j, 65, 3))
    with pytest.raises(ValueError, match="r must be >= 0 in every row"):
        index.radius(tq, torch.from_numpy(np.where(np.arange(65) == 9, np.nan, per_row).astype(np.float32)).to(cuda))
    with pytest.raises(ValueError, match="r must be >= 0 in every row"):
        index.radius(tq, torch.from_numpy(np.where(np.arange(65) == 64, -1, per_row).astype(np.float32)).to(cuda))


def test_no_queries_and_an_empty_bank(cuda):
    (tb,) = _gpu(cuda, R.make_rows("normal", 10, 8, 1))
    ip, ii, dd = btsbot_amd.radius_neighbors(tb[:0], tb, 1.0)
    assert ip.tolist() == [0] and ii.shape == dd.shape == (0,)
    assert (ip.dtype, ii.dtype, dd.dtype) == (torch.int64, torch.int64, torch.float32)
    ip, ii, dd = btsbot_amd.radius_neighbors(tb, tb[:0], float("inf"))
    assert ip.tolist() == [0] * 11 and ii.shape == dd.shape == (0,)
    ip, ii, dd = btsbot_amd.radius_graph(tb[:0], 1.0)
    assert ip.tolist() == [0] and ii.shape == (0,)
    index = btsbot_amd.EmbeddingIndex(tb)
    assert index.count_within(tb[:0], 1.0).shape == (0,)


@pytest.mark.parametrize("metric", METRICS)
def test_groups_and_self_offset_against_the_restatement(cuda, metric):
    emb = R.make_rows("normal", 300, 33, 9)
    emb[200:220] = emb[:20]
    obj = (np.arange(300) % 37).astype(np.int64) - 5
    r = _radius_for(emb, emb, 33, metric, self_offset=0)
    t, g = _gpu(cuda, emb, obj)
    index = btsbot_amd.EmbeddingIndex(t, metric, groups=g)
    out, _ = _call(index.radius, t, r, self_offset=0, splits=2)
    R.check_radius(emb, emb, r, *_np(out), metric, self_offset=0)
    plain = _rows(out)
    assert _rows(btsbot_amd.radius_graph(t, r, include_self=False, metric=metric)) == plain
    out, _ = _call(index.radius, t, r, query_groups=g, exclude_same_group=True, splits=3, sort="distance")
    R.check_radius(emb, emb, r, *_np(out), metric, sort="distance", qgroups=obj, bgroups=obj)
    assert _rows(btsbot_amd.radius_graph(t, r, include_self=False, metric=metric, groups=g, sort="distance")) == _rows(out)
    # include_self=True: the row itself, at 0, in front of the same lists
    for kw in ({}, {"groups": g}):
        ip0, ii0, dd0 = _np(btsbot_amd.radius_graph(t, r, include_self=False, metric=metric, **kw))
        ip, ii, dd = _np(btsbot_amd.radius_graph(t, r, include_self=True, metric=metric, **kw))
        assert np.array_equal(np.diff(ip), np.diff(ip0) + 1)
        for i in range(300):
            row, row0 = ii[ip[i]:ip[i + 1]], ii0[ip0[i]:ip0[i + 1]]
            assert np.array_equal(row, np.sort(np.r_[row0, i])) and dd[ip[i]:ip[i + 1]][row == i] == 0


def test_count_within_and_max_total(cuda):
    q, b = R.make_rows("normal", 65, 5, 1), R.make_rows("normal", 1000, 5, 2)
    r = _radius_for(q, b, 5, "euclidean")
    tq, tb = _gpu(cuda, q, b)
    index = btsbot_amd.EmbeddingIndex(tb)
    (ip, ii, _dd), stats = _call(index.radius, tq, r)
    counts = index.count_within(tq, r, splits=3)
    assert counts.dtype == torch.int64 and torch.equal(counts, ip.diff())
    d = R.d64_matrix(q, b, "euclidean", r)
    assert R.band_share(d, R.eligible(q, b), r, 5, "euclidean") == 0  # no pair in the band: the counts are the float64 ones
    assert np.array_equal(counts.cpu().numpy(), (d <= r).sum(1))
    total = int(ip[-1])
    assert index.radius(tq, r, max_total=total)[1].shape[0] == total
    with pytest.raises(ValueError, match=f"T = {total}"):
        index.radius(tq, r, max_total=total - 1)
    with pytest.raises(ValueError, match="max_total"):
        index.count_within(tq, r, max_total=0)
