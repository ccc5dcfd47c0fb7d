"""CPU checks of the grid search's rules (tests/grid_ref.py states them in numpy float32; csrc/grid.hip, DESIGN.md section
4q): the distance rule against float64, the safe range -- every member's cell lies in the cells its query walks, at
every resolution --, the argument checks of MapIndex and of method="grid", and the C ABI's refusals.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import btsbot_amd
import grid_ref as GR
import radius_ref as R
from btsbot_amd import _lib
from btsbot_amd import mapindex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = (1, 7, 64, 2048)


def _sets():
    """(name, bank, radii)"""
    edges = GR.edge_set()
    return [("edges", edges[:-1], (0.0, 1e-3, 0.125, 0.3, np.inf)),
            ("outlier", edges, (0.0, 0.125, 40.0, np.inf)),
            ("offset", GR.offset_set(), (0.0, 0.01, np.inf)),
            ("zero extent", GR.zero_extent_set(), (0.0, 0.5, np.inf)),
            ("blobs", R.blobs_2d(11), (0.0, 0.3, np.inf))]


@pytest.mark.parametrize("name, b, radii", _sets(), ids=lambda v: v if isinstance(v, str) else None)
def test_the_fp32_distance_rule_is_within_the_band_of_float64(name, b, radii):
    q = GR.queries_for(b)
    fq, fb = GR.finite_rows(q), GR.finite_rows(b)
    assert fq.sum() >= 120 and (~fq).sum() == 2
    d32 = GR.distance(q[fq], b[fb]).astype(np.float64)
    d64 = np.sqrt(((q[fq].astype(np.float64)[:, None, :] - b[fb].astype(np.float64)[None, :, :]) ** 2).sum(-1))
    band = R.band_of(2, "euclidean")
    assert (np.abs(d32 - d64) <= band * d64).all()
    assert (d32[d64 == 0] == 0).all() and (d64 == 0).sum() > 0          # a bank row as a query: exactly 0


def test_the_finite_rule_is_the_packed_banks():
    x = np.array([[1, 2], [np.nan, 0], [0, np.inf], [-np.inf, 0], [1e20, 0], [1.3e19, 1.3e19], [1.4e19, 1.4e19],
                  [-1e19, 1e19]], np.float32)
    assert GR.finite_rows(x).tolist() == [True, False, False, False, False, True, False, True]
    # R.finite_rows looks at the coordinates only; where the norm is finite too the two agree
    b = GR.edge_set()
    assert (GR.finite_rows(b) <= R.finite_rows(b)).all() and (GR.finite_rows(b) != R.finite_rows(b)).sum() == 1


def test_the_cell_function_is_monotone_and_total():
    rng = np.random.default_rng(0)
    xs = np.sort(np.concatenate([rng.normal(0, 50, 4000), rng.uniform(-1e30, 1e30, 200), [-np.inf, np.inf, 0.0, -0.0],
                                 np.arange(-8, 9) * 0.125]).astype(np.float32))
    for x0, inv in ((0.0, 8.0), (-3.7, 0.33), (4096.0, 8192.0), (1e30, 1e-30), (0.0, 0.0), (-3e38, 0.0), (2.5, 3e38)):
        for G in CELLS:
            c = GR.cell_of(xs, x0, inv, G)
            assert (np.diff(c) >= 0).all() and c.min() >= 0 and c.max() <= G - 1, (x0, inv, G)


@pytest.mark.parametrize("name, b, radii", _sets(), ids=lambda v: v if isinstance(v, str) else None)
@pytest.mark.parametrize("G", CELLS)
def test_every_members_cell_lies_in_the_range_its_query_walks(name, b, radii, G):
    q = GR.queries_for(b)
    fq, fb = GR.finite_rows(q), GR.finite_rows(b)
    q, pts = q[fq], b[fb]
    x0, inv = GR.geometry(b, G)
    if name in ("edges", "offset", "blobs"):
        assert (inv > 0).all()
    if name == "zero extent":
        assert (inv == 0).all()
    d = GR.distance(q, pts)
    cells = [GR.cell_of(pts[:, a], x0[a], inv[a], G) for a in range(2)]
    if name == "edges" and G in (64, 2048):   # the rows placed on the edges and an ulp to either side land on both sides
        on = np.isin(pts[:, 0], (np.arange(1, 64) * 0.125).astype(np.float32))
        assert on.sum() > 20 and (cells[0][on] == (pts[on, 0] * (G / 8)).astype(np.int64)).all()
    members = 0
    for r in radii + (np.where(np.arange(len(q)) % 3 == 0, 0.0, np.where(np.arange(len(q)) % 3 == 1, 0.2, np.inf)),):
        rr = np.broadcast_to(np.asarray(r, np.float32), (len(q),))
        member = d <= rr[:, None]
        members += int(member.sum())
        for a in range(2):
            c0, c1 = GR.safe_cells(q[:, a], rr, x0[a], inv[a], G)
            assert (c0 <= c1).all() and c0.min() >= 0 and c1.max() <= G - 1
            inside = (c0[:, None] <= cells[a][None, :]) & (cells[a][None, :] <= c1[:, None])
            assert (inside | ~member).all(), (name, G, r if np.isscalar(r) else "per row", a)
        if np.isscalar(r) and np.isinf(r):
            assert member.all()
    assert members > len(q)


def test_the_safe_range_survives_underflow_and_overflow():
    """a distance that underflows to 0 (so the pair is a member at r = 0) and one that overflows (a member at +inf only)"""
    b = np.array([[0.0, 0.0], [1e-30, 0.0], [3e-23, 0.0], [1.5e19, 0.0], [-1e19, 1e19]], np.float32)
    q = np.array([[0.0, 0.0], [1e19, -1e19]], np.float32)
    d = GR.distance(q, b)
    assert d[0, 1] == 0 and d[0, 2] > 0 and d[1, 4] == np.inf
    for G in CELLS:
        x0, inv = GR.geometry(b, G)
        for r in (0.0, 1e-30, np.inf):
            for a in range(2):
                c0, c1 = GR.safe_cells(q[:, a], np.float32(r), x0[a], inv[a], G)
                cb = GR.cell_of(b[:, a], x0[a], inv[a], G)
                member = d <= np.float32(r)
                assert (((c0[:, None] <= cb[None, :]) & (cb[None, :] <= c1[:, None])) | ~member).all(), (G, r, a)


def test_default_cells_come_from_n_alone():
    assert [mapindex.default_cells(n) for n in (0, 1, 2, 360, 100_000, 1_000_000, 10 ** 9)] == [1, 1, 1, 13, 223, 707, 2048]


# ---- arguments
def test_arguments_are_checked_before_the_device_is_touched():
    p2, p3 = torch.zeros(6, 2), torch.zeros(6, 3)
    with pytest.raises(ValueError, match="D = 3"):
        btsbot_amd.MapIndex(p3)
    with pytest.raises(ValueError, match=r"\[rows, 2\]"):
        btsbot_amd.MapIndex(torch.zeros(6, 2, dtype=torch.int64))
    for bad in (0, 4097, 2.0, True):
        with pytest.raises(ValueError, match="cells"):
            btsbot_amd.MapIndex(p2, cells=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # valid arguments: only the device is missing
        btsbot_amd.MapIndex(p2, cells=7)
    for fn, args in ((btsbot_amd.radius_graph, (1.0,)), (btsbot_amd.knn_graph, (3,)), (btsbot_amd.dbscan, (0.5,))):
        with pytest.raises(ValueError, match="D = 3"):
            fn(p3, *args, method="grid")
        with pytest.raises(ValueError, match="euclidean"):
            fn(p2, *args, metric="cosine", method="grid")
        with pytest.raises(ValueError, match="method"):
            fn(p2, *args, method="cells")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(p2, *args, method="grid")
    for mode in ("distinct", "exclude+distinct"):
        with pytest.raises(ValueError, match="group_mode"):
            btsbot_amd.knn_graph(p2, 3, groups=torch.zeros(6, dtype=torch.int64), group_mode=mode, method="grid")
    with pytest.raises(ValueError, match="group_mode"):
        btsbot_amd.radius_graph(p2, 1.0, group_mode="distinct", method="grid")
    for bad in (0, 65, 1.0, True):
        with pytest.raises(ValueError, match="k must be"):
            btsbot_amd.knn_graph(p2, bad, method="grid")
        with pytest.raises(ValueError, match="k must be"):
            mapindex._check_k(bad)
    # r, sort and max_total: _check_radius_args as it stands
    for bad in (-1.0, float("nan"), "1", None, True):
        with pytest.raises(ValueError, match="r must be"):
            btsbot_amd.radius_graph(p2, bad, method="grid")
    with pytest.raises(ValueError, match="one float radius per query row"):
        btsbot_amd.radius_graph(p2, torch.ones(5), method="grid")
    with pytest.raises(ValueError, match="r must be >= 0 in every row"):
        btsbot_amd.radius_graph(p2, torch.tensor([1.0, 2.0, float("nan"), 1.0, 1.0, 1.0]), method="grid")
    with pytest.raises(ValueError, match="sort"):
        btsbot_amd.radius_graph(p2, 1.0, sort="score", method="grid")
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="max_total"):
            btsbot_amd.radius_graph(p2, 1.0, max_total=bad, method="grid")
    # the defaults are today's paths
    import inspect
    for fn in (btsbot_amd.radius_graph, btsbot_amd.knn_graph, btsbot_amd.dbscan):
        assert inspect.signature(fn).parameters["method"].default == "tiles"


def test_the_grid_symbols_are_declared_exported_and_refuse_bad_arguments():
    header = open(os.path.join(ROOT, "include", "btsbot_hip.h")).read()
    raw, L = C.CDLL(_lib.LIB_PATH), _lib.lib()
    for name in ("btsbot_grid_finite", "btsbot_grid_cells", "btsbot_grid_radius_count", "btsbot_grid_radius_fill",
                 "btsbot_grid_knn"):
        assert name in _lib.SYMBOLS and hasattr(raw, name)
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert "grid.hip" in open(os.path.join(ROOT, "btsbot_amd", "csrc", "Makefile")).read()
    assert "btsbot_grid_knn" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("MapIndex", "mapindex"):
        assert name in btsbot_amd.__all__ and hasattr(btsbot_amd, name)
    p = C.c_void_p(256)          # never dereferenced: every call below is refused first, or has nothing to do
    bad = _lib.ERR_INVALID_ARG
    assert L.btsbot_grid_finite(p, -1, p, None) == bad and L.btsbot_grid_finite(p, 0, p, None) == _lib.OK
    assert L.btsbot_grid_finite(None, 3, p, None) == bad
    assert L.btsbot_grid_cells(p, 3, p, 0, p, p, None) == bad and b"cells" in L.btsbot_last_error()
    assert L.btsbot_grid_cells(p, 3, p, 4097, p, p, None) == bad
    assert L.btsbot_grid_cells(p, 3, None, 8, p, p, None) == bad

    def count(nq=4, cells=8, nb=9, flags=0, lanes=0, qg=None, bg=None, geom=p, counts=p):
        return L.btsbot_grid_radius_count(p, nq, p, geom, cells, p, p, p, bg, nb, -1, qg, flags, lanes, counts, None, None)

    assert count(cells=0) == bad and count(cells=4097) == bad and count(nb=1 << 31) == bad and count(nq=-1) == bad
    assert count(flags=2) == bad and b"flags" in L.btsbot_last_error()
    assert count(flags=1) == bad and b"query_group" in L.btsbot_last_error()
    assert count(lanes=3) == bad and b"lanes" in L.btsbot_last_error()
    assert count(geom=None) == bad and count(counts=None) == bad
    assert count(nq=0) == _lib.OK
    fill = (p, 4, p, p, 8, p, p, p, None, 9, -1, None, 0, 0, p)
    assert L.btsbot_grid_radius_fill(*fill, -1, p, p, p, None) == bad
    assert L.btsbot_grid_radius_fill(*fill, 0, p, p, p, None) == _lib.OK          # nothing to do
    assert L.btsbot_grid_radius_fill(*fill, 5, None, p, p, None) == bad
    knn = (p, 8, p, p, p, None, 9, -1, None, 0)
    assert L.btsbot_grid_knn(p, 4, 0, *knn, p, p, None) == bad and b"k=" in L.btsbot_last_error()
    assert L.btsbot_grid_knn(p, 4, 65, *knn, p, p, None) == bad
    assert L.btsbot_grid_knn(p, 4, 5, *knn, None, p, None) == bad
    assert L.btsbot_grid_knn(p, 0, 5, *knn, p, p, None) == _lib.OK
