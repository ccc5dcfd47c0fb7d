"""GPU tests of the four offer entry points of csrc/mr_offer.hip alone (run with -m gpu on an MI355X): on the hand-made
lists of tests/offer_ref.py, ``best_w``, ``best_j``, ``unresolved`` and ``core_q`` equal the numpy restatement bit for bit --
for the spanning tree's form and for prediction's, at list lengths on both sides of every lane width, with 70 rows (more
than one workgroup at every width, the last one partial)."""
import ctypes as C

import numpy as np
import pytest
import torch

from btsbot_amd import _lib
import offer_ref as O

pytestmark = pytest.mark.gpu

ROWS, BANK = 70, 50
KS = (1, 16, 17, 32, 33, 64)
SLACKS = (None, "plain", "squared")
RELS = (0.0, 2.0 ** -10)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _stream(cuda):
    return C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    for name, ref in want.items():
        g = got[name].cpu().numpy()
        assert g.dtype == ref.dtype and g.shape == ref.shape, (what, name)
        bad = np.flatnonzero(_bits(g) != _bits(ref))
        assert not len(bad), (what, name, bad[:8].tolist(), g[bad[:8]].tolist(), ref[bad[:8]].tolist())


def _offer_knn(case, cuda):
    """the device's answer to the lists of ``case``: a dict of tensors, as ``offer_ref.offer_knn``'s"""
    idx, dist, core, slack = (_dev(case[name], cuda) for name in ("idx", "dist", "core", "slack"))
    rows, k = idx.shape
    out = dict(best_w=torch.full((rows,), -7.0, dtype=torch.float32, device=cuda),
               best_j=torch.full((rows,), -7, dtype=torch.int32, device=cuda),
               unresolved=torch.full((rows,), 7, dtype=torch.uint8, device=cuda))
    L, ms = _lib.lib(), case["min_samples"]
    if ms is None:
        _lib.check(L.btsbot_mst_offer_knn(_p(idx), _p(dist), rows, k, _p(core), _p(slack), int(case["squared"]), case["rel"],
                                          _p(out["best_w"]), _p(out["best_j"]), _p(out["unresolved"]), _stream(cuda)),
                   "btsbot_mst_offer_knn")
    else:
        out["core_q"] = torch.full((rows,), -7.0, dtype=torch.float32, device=cuda)
        _lib.check(L.btsbot_cluster_offer_knn(_p(idx), _p(dist), rows, k, case["n"], ms, _p(core), _p(slack),
                                              int(case["squared"]), case["rel"], _p(out["core_q"]), _p(out["best_w"]),
                                              _p(out["best_j"]), _p(out["unresolved"]), _stream(cuda)),
                   "btsbot_cluster_offer_knn")
    return out


def _check_knn(case, cuda, what):
    ref = O.offer_knn(case["idx"], case["dist"], case["n"], case["core"], case["slack"], case["squared"], case["rel"],
                      case["min_samples"])
    got = _offer_knn(case, cuda)
    _same(got, ref, what)
    flags = O.boundary_flags(case)                     # the restatement itself shows the rule of its form
    assert {r: int(ref["unresolved"][r]) for r in flags} == flags, what
    return ref


@pytest.mark.parametrize("k", KS)
def test_mst_offer_knn_equals_the_restatement(cuda, k):
    seen = set()
    for slack in SLACKS:
        for rel in RELS:
            ref = _check_knn(O.lists(k, ROWS, ROWS, slack, rel), cuda, (k, slack, rel))
            seen |= set(ref["unresolved"].tolist())
            assert ref["best_j"][O.EMPTY] == -1 and ref["unresolved"][O.EMPTY] == 0
    assert seen == {0, 1}


@pytest.mark.parametrize("k", KS)
def test_cluster_offer_knn_equals_the_restatement(cuda, k):
    seen = set()
    for ms in (1, 2, k + 1):
        for slack in SLACKS:
            for rel in RELS:
                ref = _check_knn(O.lists(k, BANK, ROWS, slack, rel, min_samples=ms), cuda, (k, ms, slack, rel))
                seen |= set(ref["unresolved"].tolist())
                assert np.isnan(ref["best_w"][O.NAN_FIRST]) and np.isnan(ref["core_q"][O.NAN_FIRST])
                if ms > 1:                              # the core column is absent: +inf, and no neighbour
                    assert np.isinf(ref["core_q"][O.EMPTY]) and ref["best_j"][O.EMPTY] == -1
                if ms == k + 1 and k > 1:
                    assert np.isinf(ref["core_q"][O.TAIL]) and np.isinf(ref["best_w"][O.TAIL])
    assert seen == {0, 1}


@pytest.mark.parametrize("form", ("mst", "cluster"))
def test_offer_csr_equals_the_restatement(cuda, form):
    predict = form == "cluster"
    n = BANK if predict else ROWS
    case = O.lists(16, n, ROWS, "plain", 0.0, min_samples=2 if predict else None)
    first = O.offer_knn(case["idx"], case["dist"], n, case["core"], case["slack"], False, 0.0, case["min_samples"])
    csr = O.csr_lists(ROWS, n)
    row_core = first["core_q"] if predict else case["core"]
    best_w, best_j = first["best_w"].copy(), first["best_j"].copy()
    # what a row holds already wins, loses, or is nothing at all
    asked = [r for r in csr["rows"].tolist() if 0 <= r < ROWS]
    best_w[asked[0]], best_j[asked[0]] = 0.0, 0
    best_w[asked[1]], best_j[asked[1]] = np.inf, -1
    best_w[asked[3]], best_j[asked[3]] = 63.0, 5
    want_w, want_j = O.offer_csr(csr["indptr"], csr["indices"], csr["dist"], csr["rows"], ROWS, n, case["core"], row_core,
                                 best_w, best_j)
    changed = want_j != best_j
    assert changed[asked[1]] and changed[asked[3]] and not changed[asked[0]]
    assert 0 < changed[asked].sum() < len(asked) and not changed[np.setdiff1d(np.arange(ROWS), asked)].any()
    t = {name: _dev(a, cuda) for name, a in csr.items()}
    core, core_q, w, j = (_dev(a, cuda) for a in (case["core"], row_core, best_w, best_j))
    L, m = _lib.lib(), len(csr["rows"])
    if predict:
        _lib.check(L.btsbot_cluster_offer_csr(_p(t["indptr"]), _p(t["indices"]), _p(t["dist"]), _p(t["rows"]), m, ROWS, n,
                                              _p(core), _p(core_q), _p(w), _p(j), _stream(cuda)), "btsbot_cluster_offer_csr")
    else:
        _lib.check(L.btsbot_mst_offer_csr(_p(t["indptr"]), _p(t["indices"]), _p(t["dist"]), _p(t["rows"]), m, n, _p(core),
                                          _p(w), _p(j), _stream(cuda)), "btsbot_mst_offer_csr")
    _same(dict(best_w=w, best_j=j), dict(best_w=want_w, best_j=want_j), form)
