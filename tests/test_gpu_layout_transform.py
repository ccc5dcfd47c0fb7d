"""GPU tests of the transform of the embedding layout (run with -m gpu on an MI355X): query_memberships / layout_transform /
EmbeddingMap against the float64 restatement of tests/layout_transform_ref.py -- sigma and the weights up to exp's last
bits, the weighted-mean start to one ulp, every epoch one at a time under the bound |dy| <= TRANSFORM_C 2^-24 (|y| + alpha
sum |term|) -- against themselves bit for bit (runs, grid size, stepping, how the rows are batched), and as a map: fresh
draws of ten Gaussian clusters land among their cluster's bank points."""
import numpy as np
import pytest
import torch

import btsbot_amd
import layout_ref as R
import layout_transform_ref as T

pytestmark = pytest.mark.gpu

A, B = btsbot_amd.find_ab_params(1.0, 0.1)
SHAPES = [(512, 130, 15), (300, 67, 64), (65, 9, 2), (2, 5, 2), (7, 3, 15)]


def _rows(n_bank, q, k, seed):
    """(bank [N, 5], queries [Q, 5], map [N, 2]) float32.  Queries: normal rows, row 1 equal to a bank row (d = 0), from
    five rows on a far outlier (row 3) and a NaN row (row 4); banks of 60 rows or more: the second half of bank and
    queries are small integers (ties), and bank row 7 is non-finite with a NaN map position."""
    rng = np.random.default_rng(seed)
    bank, queries = rng.standard_normal((n_bank, 5)), rng.standard_normal((q, 5))
    if n_bank >= 60:
        bank[n_bank // 2:] = rng.integers(-3, 4, size=(n_bank - n_bank // 2, 5))
        queries[q // 2:] = rng.integers(-3, 4, size=(q - q // 2, 5))
    queries[1] = bank[min(1, n_bank - 1)]
    if q >= 5:
        queries[3] = 1e4
        queries[4, 2] = np.nan
    Y = 4.0 * rng.standard_normal((n_bank, 2))
    if n_bank >= 60:
        bank[7, 1] = np.nan
        Y[7] = np.nan
    return bank.astype(np.float32), queries.astype(np.float32), Y.astype(np.float32)


class Case:
    def __init__(self, cuda, shape):
        n_bank, q, k = shape
        self.shape = shape
        self.bank, self.queries, self.Y = _rows(n_bank, q, k, n_bank + q + k)
        self.index = btsbot_amd.EmbeddingIndex(torch.from_numpy(self.bank).to(cuda))
        self.d_idx, self.d_dist = self.index.query(torch.from_numpy(self.queries).to(cuda), k)
        self.d_Y = torch.from_numpy(self.Y).to(cuda)
        self.idx, self.dist = self.d_idx.cpu().numpy(), self.d_dist.cpu().numpy()
        self.d_w, self.d_sigma = btsbot_amd.query_memberships(self.d_idx, self.d_dist)
        self.w = self.d_w.cpu().numpy()
        self._paths = {}

    def run(self, n_epochs=10, **kw):
        return btsbot_amd.layout_transform(self.d_idx, self.d_dist, self.d_Y, n_epochs, a=A, b=B, **kw)

    def path(self, n_epochs, rate):
        """The restatement's fp32 positions before every epoch of the schedule (from the device's own weights), once."""
        if (n_epochs, rate) not in self._paths:
            ys = [T.init_positions(self.idx, self.w, self.Y)]
            for n in range(1, n_epochs):
                ys.append(T.transform_epoch(self.idx, self.w, self.Y, ys[-1], n, n_epochs, A, B, 3, rate)[0].astype(np.float32))
            self._paths[(n_epochs, rate)] = ys
        return self._paths[(n_epochs, rate)]


@pytest.fixture(scope="module")
def cases(cuda):
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Case(cuda, shape)
        return made[shape]
    return get


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- memberships and start
@pytest.mark.parametrize("shape", SHAPES)
def test_memberships_and_start_equal_the_restatement(cases, shape):
    c = cases(shape)
    n_bank, q, k = shape
    assert c.idx.shape == (q, k)
    if n_bank < k:
        assert (c.idx[:, n_bank:] == -1).all() and (c.idx[0, :n_bank] >= 0).all()      # tails of idx = -1
    if n_bank >= 60:
        assert not (c.idx == 7).any()                                                 # the non-finite bank row
    assert c.dist[1, 0] == 0.0                                                         # the query equal to a bank row
    if q >= 5:
        assert (c.idx[4] == -1).all() and np.isnan(c.dist[4]).all()
    w_ref, sigma_ref = T.query_memberships(c.idx, c.dist)
    sigma = c.d_sigma.cpu().numpy()
    rel = np.abs(sigma.astype(np.float64) - sigma_ref) / sigma_ref
    dw = np.abs(c.w.astype(np.float64) - w_ref)
    print(f"{shape}: sigma off {rel.max():.2e} relative, weights off {dw.max():.2e}")
    assert rel.max() <= 2.0 ** -22, f"sigma off by {rel.max():.3e} relative"
    assert dw.max() <= 3 * 2.0 ** -23, f"weights off by {dw.max():.3e}"
    assert c.w[1, 0] == 1.0 and (c.w[c.idx < 0] == 0).all()
    # the start: the device and the restatement round the same float64 value
    start = c.run(last_epoch=0).cpu().numpy()
    ref = T.init_positions(c.idx, c.w, c.Y)
    assert np.array_equal(np.isnan(start), np.isnan(ref))
    assert np.isnan(ref).all(axis=1).sum() == (1 if q >= 5 else 0)
    ok = ~np.isnan(ref)
    ulps = np.abs(start[ok].astype(np.float64) - ref[ok]) / np.spacing(np.abs(ref[ok]))
    print(f"{shape}: the start is off by at most {ulps.max():.0f} ulp")
    assert ulps.max() <= 1.0


# ---- one epoch at a time
@pytest.mark.parametrize("shape", SHAPES)
def test_each_epoch_against_the_restatement(cases, cuda, shape):
    c = cases(shape)
    worst, stats = 0.0, {}
    for n_epochs in (10, 100):
        for rate in (0, 1, 5):
            ys = c.path(n_epochs, rate)
            for n in (1, 2, n_epochs // 2, n_epochs):
                y = ys[n - 1].copy()
                y[0] = c.Y[c.idx[0, 0]]                      # a query ON a neighbour (and, in a bank of two, on samples)
                got = c.run(n_epochs, seed=3, negative_sample_rate=rate, y0=torch.from_numpy(y).to(cuda), first_epoch=n,
                            last_epoch=n).cpu().numpy()
                ref, scale = T.transform_epoch(c.idx, c.w, c.Y, y, n, n_epochs, A, B, 3, rate, stats=stats)
                ratio = R.epoch_ratio(got, ref, scale)
                print(f"{shape} epoch {n}/{n_epochs} rate {rate}: {ratio:.2f} x 2^-24")
                worst = max(worst, ratio)
    print(f"{shape}: worst {worst:.2f} x 2^-24 (bound {T.TRANSFORM_C:g}); events {stats}")
    assert stats["fired"] > 0 and stats["coincident_neighbour"] > 0
    if shape[0] >= 60:
        assert stats["nan_sample"] > 0
    if shape[0] >= 300:
        assert stats["clipped"] > 0
    if shape[0] == 2:
        assert stats["coincident_sample"] > 0
    assert worst <= T.TRANSFORM_C, f"epoch error is {worst:.1f} x 2^-24 of (|y| + alpha sum |term|), bound {T.TRANSFORM_C}"


# ---- bit for bit
def test_transform_is_reproducible_bit_for_bit(cases, cuda):
    c = cases(SHAPES[0])
    whole = c.run(seed=4)
    nan = torch.isnan(whole).any(dim=1)
    assert nan.sum() == 1 and nan[4]
    assert torch.equal(_bits(whole), _bits(c.run(seed=4)))
    assert not torch.equal(_bits(whole), _bits(c.run(seed=5)))
    for blocks in (1, 3):
        assert torch.equal(_bits(whole), _bits(c.run(seed=4, blocks=blocks))), blocks
    step = None
    for n in range(1, 11):
        step = c.run(seed=4, y0=step, first_epoch=n, last_epoch=n)
    assert torch.equal(_bits(whole), _bits(step))
    two = c.run(seed=4, y0=c.run(seed=4, last_epoch=7), first_epoch=8)
    assert torch.equal(_bits(whole), _bits(two))
    start = c.run(last_epoch=0)
    assert torch.equal(_bits(whole), _bits(c.run(seed=4, y0=start)))


def test_a_row_depends_on_the_row_alone(cases, cuda):
    c = cases(SHAPES[0])
    whole = c.run(seed=4)

    def part(rows):
        return btsbot_amd.layout_transform(c.d_idx[rows], c.d_dist[rows], c.d_Y, 10, a=A, b=B, seed=4)

    parts = torch.cat([part(slice(0, 1)), part(slice(1, 65)), part(slice(65, 130))])
    assert torch.equal(_bits(whole), _bits(parts))
    perm = torch.from_numpy(np.random.default_rng(1).permutation(130)).to(cuda)
    assert torch.equal(_bits(whole[perm]), _bits(part(perm)))
    twice = torch.cat([torch.arange(130, device=cuda), torch.tensor([0, 1, 2, 77, 129], device=cuda)])
    dup = part(twice)
    assert torch.equal(_bits(dup[130:]), _bits(whole[twice[130:]])) and torch.equal(_bits(dup[:130]), _bits(whole))


def test_extend_equals_a_map_of_the_concatenation(cases, cuda):
    c = cases(SHAPES[0])
    bank, queries = torch.from_numpy(c.bank).to(cuda), torch.from_numpy(c.queries).to(cuda)
    finite = torch.isfinite(queries).all(dim=1)
    rows, later = queries[finite][:40], queries[40:]
    m = btsbot_amd.EmbeddingMap.from_positions(bank, c.d_Y, n_neighbors=15)
    assert len(m) == 512 and torch.equal(_bits(m.embedding_), _bits(c.d_Y))
    placed = m.extend(rows, seed=2)
    assert len(m) == 552 and m.embedding_.shape == (552, 2) and torch.equal(_bits(m.embedding_[512:]), _bits(placed))
    assert torch.isfinite(placed).all()
    one = btsbot_amd.EmbeddingMap.from_positions(torch.cat([bank, rows]), torch.cat([c.d_Y, placed]), n_neighbors=15)
    got, want = m.transform(later, n_epochs=20, seed=3), one.transform(later, n_epochs=20, seed=3)
    assert torch.equal(_bits(got), _bits(want))
    # the index may be handed over as it is; the default is 100 epochs whatever Q
    same = btsbot_amd.EmbeddingMap.from_positions(one.index, one.embedding_)
    assert same.index is one.index
    assert torch.equal(_bits(same.transform(later[:3])), _bits(one.transform(later, n_epochs=100)[:3]))
    # the new rows are neighbours now (row 1 is a copy of a bank row, which comes first in a tie)
    idx, dist = m.index.query(rows[2:7], 1)
    assert idx.flatten().tolist() == [514, 515, 516, 517, 518] and (dist == 0).all()


def test_transform_does_not_synchronise_with_the_host(cases, cuda):
    c = cases(SHAPES[0])
    m = btsbot_amd.EmbeddingMap.from_positions(c.index, c.d_Y)
    queries = torch.from_numpy(c.queries).to(cuda)
    m.transform(queries, n_epochs=3)                                       # warm: code objects, the allocator's blocks
    torch.cuda.synchronize(cuda)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                # a host read is an error in this mode
    try:
        y = m.transform(queries, n_epochs=3)
        w, _sigma = btsbot_amd.query_memberships(c.d_idx, c.d_dist)
        y2 = c.run(3, y0=y, first_epoch=2, last_epoch=3)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert y.shape == y2.shape == (130, 2) and w.shape == (130, 15)


# ---- edge cases
def test_edge_cases(cases, cuda):
    c = cases(SHAPES[0])
    empty = btsbot_amd.layout_transform(c.d_idx[:0], c.d_dist[:0], c.d_Y, a=A, b=B)
    assert empty.shape == (0, 2) and empty.dtype == torch.float32
    w, sigma = btsbot_amd.query_memberships(c.d_idx[:0], c.d_dist[:0])
    assert w.shape == (0, 15) and sigma.shape == (0,)
    m = btsbot_amd.EmbeddingMap.from_positions(c.index, c.d_Y)
    assert m.transform(torch.zeros((0, 5), device=cuda)).shape == (0, 2)
    for shape in SHAPES:
        cs = cases(shape)
        y = cs.run(100).cpu().numpy()                                      # the default rate, the whole schedule
        nan = np.isnan(cs.queries).any(axis=1)
        assert np.isnan(y[nan]).all() and np.isfinite(y[~nan]).all(), shape
        assert nan.sum() == (1 if shape[1] >= 5 else 0)


def test_errors(cases, cuda):
    c = cases(SHAPES[0])
    idx, dist, Y = c.d_idx, c.d_dist, c.d_Y
    f = btsbot_amd.layout_transform
    with pytest.raises(ValueError, match="k "):
        f(idx[:, :1], dist[:, :1], Y, a=A, b=B)
    with pytest.raises(ValueError, match="k "):
        btsbot_amd.query_memberships(idx.repeat(1, 5), dist.repeat(1, 5))             # k = 75
    with pytest.raises(ValueError, match="int64"):
        f(idx.int(), dist, Y, a=A, b=B)
    with pytest.raises(ValueError, match="float32"):
        btsbot_amd.query_memberships(idx, dist.double())
    with pytest.raises(ValueError, match=r"\[N, k\]"):
        f(idx, dist[:, :14], Y, a=A, b=B)
    with pytest.raises(TypeError):
        f(idx.cpu().numpy(), dist, Y, a=A, b=B)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(idx.cpu(), dist.cpu(), Y, a=A, b=B)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(idx, dist, Y.cpu(), a=A, b=B)
    with pytest.raises(ValueError, match="bank_y"):
        f(idx, dist, Y.double(), a=A, b=B)
    with pytest.raises(ValueError, match="bank_y"):
        f(idx, dist, Y.reshape(-1), a=A, b=B)
    with pytest.raises(ValueError, match="empty"):
        f(idx, dist, Y[:0], a=A, b=B)
    with pytest.raises(ValueError, match="y0"):
        f(idx, dist, Y, a=A, b=B, y0=Y[:129])
    with pytest.raises(ValueError, match="needs y0"):
        f(idx, dist, Y, a=A, b=B, first_epoch=2)
    with pytest.raises(ValueError, match="first_epoch"):
        f(idx, dist, Y, 10, a=A, b=B, y0=Y[:130], first_epoch=11)
    with pytest.raises(ValueError, match="last_epoch"):
        f(idx, dist, Y, 10, a=A, b=B, y0=Y[:130], first_epoch=1, last_epoch=0)        # the start alone takes no y0
    with pytest.raises(ValueError, match="negative_sample_rate"):
        f(idx, dist, Y, a=A, b=B, negative_sample_rate=65)
    with pytest.raises(ValueError, match="positive"):
        f(idx, dist, Y, a=0.0, b=B)
    with pytest.raises(ValueError, match="n_neighbors"):
        btsbot_amd.EmbeddingMap.from_positions(c.index, Y, n_neighbors=1)
    with pytest.raises(ValueError, match="y must be"):
        btsbot_amd.EmbeddingMap.from_positions(c.index, Y[:100])
    # the C ABI says the same
    from btsbot_amd import _lib
    L = _lib.lib()
    args = (idx.data_ptr(), c.d_w.data_ptr(), Y.data_ptr(), 512, 130, 15, None, torch.empty_like(Y).data_ptr())
    assert L.btsbot_layout_transform(*args, 10, 2, 5, A, B, 0, 5, 1.0, 0, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_layout_transform(*args[:3], 0, *args[4:], 10, 1, 5, A, B, 0, 5, 1.0, 0, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_layout_smooth_knn_query(idx.data_ptr(), dist.data_ptr(), 130, 65, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.btsbot_layout_transform(None, None, None, 512, 0, 15, None, None, 10, 1, 10, A, B, 0, 5, 1.0, 0, None) == 0


# ---- as a map
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fresh_draws_land_in_their_cluster(cuda, seed):
    bank, bank_labels, queries, labels = T.split_cluster_set(seed)
    m = btsbot_amd.EmbeddingMap(torch.from_numpy(bank).to(cuda), n_neighbors=15, n_epochs=200, seed=seed)
    y = m.transform(torch.from_numpy(queries).to(cuda), seed=seed).cpu().numpy()
    Y = m.embedding_.cpu().numpy()
    assert Y.shape == (512, 2) and np.isfinite(Y).all() and np.isfinite(y).all()
    # the restatement of the same recipe on the device's own map and neighbours
    idx, dist = (t.cpu().numpy() for t in m.index.query(torch.from_numpy(queries).to(cuda), 15))
    y_ref = T.transform(idx, dist, Y, 100, A, B, seed=seed)
    purity, purity_ref = T.query_purity(y, labels, Y, bank_labels), T.query_purity(y_ref, labels, Y, bank_labels)
    print(f"seed {seed}: purity {purity:.4f} (restatement {purity_ref:.4f}); furthest from the restatement "
          f"{np.abs(y - y_ref).max():.2e}")
    assert purity >= purity_ref - 2.0 / len(queries)
    for lab in range(10):
        box = Y[bank_labels == lab]
        lo, hi = box.min(axis=0), box.max(axis=0)
        mine = y[labels == lab]
        assert (mine >= lo - (hi - lo)).all() and (mine <= hi + (hi - lo)).all(), (seed, lab)
