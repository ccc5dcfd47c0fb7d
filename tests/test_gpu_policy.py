"""btsbot_policy_eval and val.policy_performance on the device: the per-object policy metrics of the reference's
diagnostic_fig (val.py:381-614) against its recorded output and against the numpy restatement of
tests/test_policy_host.py (which that file ties to the recording).  Every output is a selection, an integer count or one
float64 subtraction, so every comparison is exact, NaN positions included."""
import ctypes as C
import json
import warnings

import numpy as np
import pytest
import torch

from helpers import CONFIGS, seeded_state
from test_policy_host import (GOLDEN, REFERENCE_POLICIES, golden_inputs, restate_objects, restate_policies,
                              same_performance)

pytestmark = pytest.mark.gpu

NAMES = ("object_id", "jd", "magpsf", "label", "raw_preds")
PER_OBJECT = ("object_id", "n_alerts", "label", "min_magpsf", "first_alert", "pred", "trigger_jd", "trigger_mag")
T0 = 2459300.5
UP32 = np.nextafter(np.float32(0.5), np.float32(1))          # one float32 ulp above 0.5


def _dev(cuda, case, keys=NAMES):
    return [torch.from_numpy(np.ascontiguousarray(case[k])).to(cuda) for k in keys]


def _eval(cuda, case, policies=REFERENCE_POLICIES):
    from btsbot_amd import val
    out = val.policy_eval(*_dev(cuda, case), policies=policies)
    assert set(out) == set(PER_OBJECT) and all(v.device.type == "cuda" for v in out.values())
    assert out["pred"].dtype == torch.int32 and out["trigger_jd"].dtype == torch.float64
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(cuda, case, policies=REFERENCE_POLICIES):
    """policy_eval against the restatement, every per-object output."""
    got, want = _eval(cuda, case, policies), restate_objects(*(case[k] for k in NAMES), policies)
    for k in PER_OBJECT:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        bad = np.argwhere(~((got[k] == want[k]) | (np.isnan(got[k].astype(np.float64)) & np.isnan(want[k].astype(np.float64)))))
        assert bad.size == 0, (f"{k}: {len(bad)} entries differ, first at {bad[0]} (object {want['object_id'][bad[0][0]]} of "
                               f"{want['n_alerts'][bad[0][0]]} alerts): got {got[k][tuple(bad[0])]}, want {want[k][tuple(bad[0])]}")
    return got


def _object(oid, n, rng, scenario, label=1):
    """n alerts in shuffled input order, 0.02-4 day gaps.  never: no alert is valid.  first: the two earliest alerts are
    valid and bright, so every reference policy fires as early as it can.  last: the count and the gate are completed
    by the latest alert only.  random: clustered scores, magnitudes on both sides of the cut and the gate."""
    t = T0 + rng.uniform(0, 50) + np.cumsum(rng.uniform(0.02, 4.0, n))
    mag = np.round(rng.uniform(18.6, 18.95, n), 3)                 # valid by magnitude, fainter than the gate
    score = rng.uniform(0.05, 0.45, n).astype(np.float32)
    if scenario == "first":
        score[:2], mag[:2] = 0.95, (18.2, 18.3)[:min(n, 2)]
    elif scenario == "last":
        score[-2:], mag[-1] = (0.7, 0.9)[-min(n, 2):], 18.45
    elif scenario == "random":
        score = np.clip(rng.normal(0.6, 0.3, n), 0, 1).astype(np.float32)
        mag = np.round(rng.uniform(18.0, 19.6, n), 2)
    order = rng.permutation(n)
    return dict(object_id=np.full(n, oid, dtype=np.int64), jd=t[order], magpsf=mag[order],
                label=np.full(n, label, dtype=np.int64), raw_preds=score[order])


def _cat(cases, rng=None):
    case = {k: np.concatenate([c[k] for c in cases]) for k in NAMES}
    if rng is not None:
        order = rng.permutation(len(case["jd"]))
        case = {k: v[order] for k, v in case.items()}
    return case


def _one(jd, mag, score, label=1, oid=7):
    n = len(jd)
    return dict(object_id=np.full(n, oid, dtype=np.int64), jd=np.asarray(jd, dtype=np.float64),
                magpsf=np.asarray(mag, dtype=np.float64), label=np.full(n, label, dtype=np.int64),
                raw_preds=np.asarray(score, dtype=np.float32))


def test_golden_fixture(cuda):
    """policy_performance equals the dictionary the reference's diagnostic_fig recorded for the fixture, exactly."""
    from btsbot_amd import val
    rows, extra, want = golden_inputs(dict(np.load(GOLDEN)))
    got = val.policy_performance(*_dev(cuda, rows), **dict(zip(extra, _dev(cuda, extra, list(extra)))))
    assert same_performance(got, want) is None, same_performance(got, want)
    assert all(isinstance(got[n][k], float) for n in got for k in ("policy_precision", "policy_recall", "med_save_dt"))
    _check(cuda, rows)


def _boundary_batch():
    from btsbot_amd.val import POLICY_TILE as T
    rng = np.random.default_rng(11)
    plan = [(1, "random"), (2, "first"), (3, "last"), (63, "never"), (64, "first"), (65, "never"), (T - 1, "first"),
            (T, "last"), (T + 1, "never"), (2 * T + 7, "first"), (T + 9, "last"), (40, "last"), (17, "random"),
            (90, "random"), (2, "never"), (2, "last")]
    return plan, _cat([_object(100 + 3 * k, n, rng, sc, label=k % 2) for k, (n, sc) in enumerate(plan)], rng)


def test_size_boundaries(cuda):
    """Objects of 1, 2, 3, 63, 64, 65, T - 1, T, T + 1 and 2 T + 7 alerts in one shuffled batch: each of the three kernel
    forms (one wave; one workgroup over an LDS tile; an object streamed through the tile) and each hand-over between
    them, with an object that never fires, one that fires at the first possible alert and one that fires at its last
    alert in every form."""
    plan, case = _boundary_batch()
    got = _check(cuda, case)
    assert list(got["n_alerts"]) == [n for n, _ in plan]
    for k, (n, sc) in enumerate(plan):
        jd = case["jd"][case["object_id"] == 100 + 3 * k]
        if sc == "never":
            assert not got["pred"][k].any() and (got["trigger_jd"][k] == -1).all() and (got["trigger_mag"][k] == -1).all()
        elif sc == "first" and n >= 2:
            assert got["pred"][k].all() and list(got["trigger_jd"][k]) == [np.sort(jd)[1]] * 2 + [jd.min()] * 2
        elif sc == "last" and n >= 2:
            assert got["pred"][k].all() and (got["trigger_jd"][k] == jd.max()).all() and (got["trigger_mag"][k] == 18.45).all()


def test_size_boundaries_sixteen_policies(cuda):
    """The same batch under 16 distinct policies (thr, cut, k = 1..3, with and without a gate), against the restatement:
    more than four policies select the wide kernel, which the sweep test otherwise compares only with the kernel's own
    single-policy calls.  Objects of 65, T - 1, T, T + 1, 2 T + 7 and T + 9 alerts lie in adjacent slots of a workgroup:
    each hands the LDS tile and the wave minima over to the next."""
    _, case = _boundary_batch()
    pols = {f"p{i}": (0.08 + 0.055 * i, (19.0, 18.9, 18.7)[i % 3], 1 + (i // 2) % 3, None if i % 2 else 18.3 + 0.04 * i)
            for i in range(16)}
    assert len({p[0] for p in pols.values()}) == 16 and {p[2] for p in pols.values()} == {1, 2, 3}
    got = _check(cuda, case, pols)
    assert got["pred"].any(axis=0).all() and not got["pred"].all(axis=0).any()     # every policy fires somewhere, none everywhere


def test_hand_over_across_waves_and_tiles(cuda):
    """Objects of T + 1 and 2 T + 7 alerts in input order: the only alert that completes the count sits in the second
    tile, and the first magpsf <= gate comes after it in time (from the first tile)."""
    from btsbot_amd.val import POLICY_TILE as T
    rng = np.random.default_rng(4)
    for n in (T + 1, 2 * T + 7):
        rank = rng.permutation(n)                                     # time rank of every alert
        a_first, a_count, a_gate = 5, T + rng.integers(0, n - T), 3   # a valid alert; the second one; the bright one
        for a, r in ((a_first, 10), (a_count, n // 2), (a_gate, n - 40)):
            other = np.flatnonzero(rank == r)[0]
            rank[other], rank[a] = rank[a], r
        case = _one(T0 + 0.25 * rank, np.round(rng.uniform(18.6, 18.95, n), 3), rng.uniform(0.05, 0.45, n))
        case["raw_preds"][[a_first, a_count]] = 0.9
        case["magpsf"][a_gate] = 18.4
        got = _check(cuda, case)
        jd = case["jd"]
        # bts_p1: the second valid alert; bts_p2 and prod_p2: the bright alert; prod_p1: the first valid alert
        assert list(got["trigger_jd"][0]) == [jd[a_count], jd[a_gate], jd[a_first], jd[a_gate]]
        assert list(got["trigger_mag"][0]) == [case["magpsf"][a_count], 18.4, case["magpsf"][a_first], 18.4]


def test_ties(cuda):
    """Equal jd inside an object are ordered by input position: of two alerts at the same jd, the policy (k = 1) fires at
    the valid one; when that is the later in input, the earlier one is not yet 'so far'.  Then many ties in the LDS forms."""
    k1 = {"k1": (0.5, 19.0, 1, None), "k1_gate": (0.5, 19.0, 1, 18.5)}
    later = _check(cuda, _one([T0 + 1, T0 + 1, T0 + 3], [18.1, 18.2, 18.3], [0.1, 0.9, 0.9]), k1)
    assert list(later["trigger_mag"][0]) == [18.2, 18.2] and list(later["trigger_jd"][0]) == [T0 + 1, T0 + 1]
    earlier = _check(cuda, _one([T0 + 1, T0 + 1, T0 + 3], [18.1, 18.2, 18.3], [0.9, 0.1, 0.9]), k1)
    assert list(earlier["trigger_mag"][0]) == [18.1, 18.1]
    # the gate is met by the later-in-input alert of the tie only: the policy fires there, not at the valid earlier one
    gate = _check(cuda, _one([T0 + 1, T0 + 1, T0 + 3], [18.9, 18.4, 18.3], [0.9, 0.1, 0.9]), k1)
    assert list(gate["trigger_mag"][0]) == [18.9, 18.4]
    rng = np.random.default_rng(5)
    for n in (200, 1500):
        jd = T0 + rng.integers(0, n // 4, n).astype(np.float64)          # about four alerts per epoch
        _check(cuda, _one(jd, np.round(rng.uniform(18.3, 19.3, n), 1), np.clip(rng.normal(0.45, 0.2, n), 0, 1)),
               dict(REFERENCE_POLICIES, k7=(0.5, 19.0, 7, 18.35)))


def test_strict_comparisons(cuda):
    """raw == thr is not valid, one float32 ulp above is; magpsf == cut is not valid; magpsf == gate fires."""
    at = _check(cuda, _one([T0, T0 + 1, T0 + 2], [18.0, 18.0, 18.0], [0.5, 0.5, np.nextafter(np.float32(0.85), np.float32(0))]))
    assert not at["pred"].any()
    above = _check(cuda, _one([T0, T0 + 1, T0 + 2], [18.0, 18.0, 18.0], [UP32, UP32, np.float32(0.85)]))
    assert above["pred"].all()                       # float32(0.85) widened to float64 lies above 0.85
    assert list(above["trigger_jd"][0]) == [T0 + 1, T0 + 1, T0 + 2, T0 + 2]
    cut = _check(cuda, _one([T0, T0 + 1, T0 + 2], [19.0, 19.0, np.nextafter(19.0, 0)], [0.9, 0.9, 0.9]))
    assert list(cut["pred"][0]) == [0, 0, 1, 0] and cut["trigger_jd"][0, 2] == T0 + 2
    gate = _check(cuda, _one([T0, T0 + 1, T0 + 2, T0 + 3], [18.8, 18.8, np.nextafter(18.5, 19), 18.5], [0.9] * 4))
    assert list(gate["trigger_jd"][0]) == [T0 + 1, T0 + 3, T0, T0 + 3]


def test_nan_magnitudes(cuda):
    """A NaN magpsf is never valid and the minimum skips it; an object without any magnitude never fires and has a NaN
    min_magpsf."""
    nan = np.nan
    mid = _check(cuda, _one([T0, T0 + 1, T0 + 2, T0 + 3], [18.4, nan, 18.8, 18.7], [0.9, 0.9, 0.1, 0.9]))
    assert list(mid["trigger_jd"][0]) == [T0 + 3, T0 + 3, T0, T0] and mid["min_magpsf"][0] == 18.4
    allnan = _check(cuda, _one([T0, T0 + 1, T0 + 2], [nan, nan, nan], [0.9, 0.9, 0.9]))
    assert not allnan["pred"].any() and np.isnan(allnan["min_magpsf"][0]) and (allnan["trigger_jd"] == -1).all()
    first = _check(cuda, _one([T0 + 1, T0, T0 + 2], [18.2, nan, 18.3], [0.9, 0.9, 0.9]))     # the earliest alert has none
    assert list(first["trigger_jd"][0]) == [T0 + 2, T0 + 2, T0 + 1, T0 + 1]
    rng = np.random.default_rng(3)
    big = _cat([_object(1, 70, rng, "random"), _object(2, 1100, rng, "random"), _object(3, 1100, rng, "last")], rng)
    big["magpsf"][::7] = nan
    _check(cuda, big)


def test_sweep_equals_single_policy_calls(cuda):
    """33 policies (three launches of 16, 16 and 1) equal 33 calls with one policy each."""
    from btsbot_amd import val
    rng = np.random.default_rng(9)
    case = _cat([_object(k, n, rng, "random", label=k % 2) for k, n in enumerate([2, 5, 9, 30, 64, 65, 130, 300, 1100] * 2)], rng)
    sweep = {f"t{t:.3f}": (float(t), 19.0, 1 + i % 3, None if i % 2 else 18.5) for i, t in enumerate(np.linspace(0.02, 0.98, 33))}
    got = _check(cuda, case, sweep)
    assert 0 < got["pred"].sum() < got["pred"].size and (got["pred"][:, 0] != got["pred"][:, 32]).any()
    n = len(case["jd"])
    extra = dict(save_time=np.full(n, T0 - 3.0), trigger_time=np.full(n, T0 - 5.0))
    args, kw = _dev(cuda, case), dict(zip(extra, _dev(cuda, extra, list(extra))))
    perf = val.policy_performance(*args, policies=sweep, **kw)
    assert list(perf) == list(sweep)
    for i, (name, pol) in enumerate(sweep.items()):
        one = _eval(cuda, case, {name: pol})
        for k in ("pred", "trigger_jd", "trigger_mag"):
            assert np.array_equal(one[k][:, 0], got[k][:, i], equal_nan=True), (name, k)
        alone = val.policy_performance(*args, policies={name: pol}, **kw)
        assert same_performance(alone, {name: perf[name]}) is None, same_performance(alone, {name: perf[name]})
    _, want = restate_policies(*(case[k] for k in NAMES), sweep, **extra)
    assert same_performance(perf, want) is None, same_performance(perf, want)


def test_other_counts_and_cuts(cuda):
    """k = 3 and cut = 18, neither used by the reference."""
    rng = np.random.default_rng(21)
    case = _cat([_object(k, n, rng, "random") for k, n in enumerate([3, 4, 8, 33, 64, 70, 400, 1030])], rng)
    case["magpsf"] = np.round(rng.uniform(17.5, 19.6, len(case["jd"])), 2)
    pols = {"k3": (0.5, 19.0, 3, None), "k3_gate": (0.5, 19.0, 3, 17.7), "cut18": (0.5, 18.0, 1, None),
            "k3_cut18": (0.3, 18.0, 3, 18.5), "k5": (0.7, 19.5, 5, 17.6)}
    got = _check(cuda, case, pols)
    assert got["pred"].any(axis=0).all() and not got["pred"].all(axis=0).any()
    assert (got["trigger_jd"][:, 1] > got["trigger_jd"][:, 0]).any()          # the gate delays some triggers


def test_empty_batch_and_error_paths(cuda):
    from btsbot_amd import _lib, val
    e = torch.zeros(0, device=cuda)
    out = val.policy_eval(e.long(), e.double(), e.double(), e.long(), e.float())
    assert tuple(out["pred"].shape) == (0, 4) and tuple(out["trigger_jd"].shape) == (0, 4) and out["object_id"].numel() == 0
    perf = val.policy_performance(e.long(), e.double(), e.double(), e.long(), e.float())
    assert list(perf) == list(REFERENCE_POLICIES) and all(p["policy_precision"] == -999.0 for p in perf.values())
    f64 = torch.zeros(4, dtype=torch.float64, device=cuda)
    i64 = torch.zeros(4, dtype=torch.int64, device=cuda)
    f32 = torch.zeros(4, device=cuda)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        val.policy_eval(i64.cpu(), f64.cpu(), f64.cpu(), i64.cpu(), f32.cpu())
    with pytest.raises(ValueError):
        val.policy_eval(i64, f64[:3], f64, i64, f32)                               # lengths
    with pytest.raises(ValueError):
        val.policy_eval(f32, f64, f64, i64, f32)                                   # float ids
    with pytest.raises(ValueError):
        val.policy_performance(i64, f64, f64, i64, f32, junk=torch.zeros(3, dtype=torch.bool, device=cuda))
    with pytest.raises(_lib.BtsbotHipError, match="k must be"):
        val.policy_eval(i64, f64, f64, i64, f32, policies={"k0": (0.5, 19.0, 0, None)})
    with pytest.raises(_lib.BtsbotHipError, match="k must be"):
        val.policy_eval(i64, f64, f64, i64, f32, policies={"k1.5": (0.5, 19.0, 1.5, None)})
    # the C entry itself
    L = _lib.lib()
    i32 = torch.zeros(5, dtype=torch.int32, device=cuda)
    pred = torch.zeros(4, 17, dtype=torch.int32, device=cuda)
    trig = torch.zeros(4, 17, 2, dtype=torch.float64, device=cuda)
    info = torch.zeros(4, 3, dtype=torch.float64, device=cuda)
    table = (C.c_double * (4 * 17))(*([0.5, 19.0, 1.0, float("nan")] * 17))
    p = [C.c_void_p(t.data_ptr()) for t in (i32, i32, f64, f64, f32, i32)]
    o = [C.c_void_p(t.data_ptr()) for t in (pred, trig, info)]

    def call(n_alerts=4, n_objects=1, n_pol=4, ptrs=p, outs=o, tab=table):
        return L.btsbot_policy_eval(ptrs[0], ptrs[1], n_alerts, n_objects, *ptrs[2:], tab, n_pol, *outs, C.c_void_p(0))

    for n_pol in (17, 0):
        with pytest.raises(_lib.BtsbotHipError, match="n_policies"):
            _lib.check(call(n_pol=n_pol), "btsbot_policy_eval")
    table[2] = 0.0
    with pytest.raises(_lib.BtsbotHipError, match="k must be"):
        _lib.check(call(), "btsbot_policy_eval")
    table[2] = 1.0
    for null in (0, 3, 4):                                                         # perm, magpsf, raw_pred
        args = list(p)
        args[null] = C.c_void_p(0)
        assert call(ptrs=args) == _lib.ERR_INVALID_ARG and b"policy_eval" in L.btsbot_last_error()
    assert call(outs=[o[0], C.c_void_p(0), o[2]]) == _lib.ERR_INVALID_ARG
    assert call(tab=C.cast(C.c_void_p(0), C.POINTER(C.c_double))) == _lib.ERR_INVALID_ARG
    assert call(n_alerts=-1) == _lib.ERR_INVALID_ARG and call(n_objects=-1) == _lib.ERR_INVALID_ARG
    assert call(n_alerts=0, n_objects=0) == _lib.OK                                # nothing to launch
    torch.cuda.synchronize()
    assert not pred.any() and not trig.any() and not info.any()


def test_fit_writes_policy_performance(cuda, tmp_path):
    """train.fit with the validation split's candidate table: report.json's val_summary carries policy_performance, equal
    to policy_performance on the returned best_raw_preds; without a table the summary has exactly the alert-level keys."""
    import btsbot_amd
    from btsbot_amd import data, val
    from btsbot_amd.synthetic import synthetic_batch
    from btsbot_amd.train import Trainer, fit
    kind, cfg = CONFIGS["um_nn"]
    _, meta, _ = synthetic_batch(512, seed=21)
    lab = (meta[:, 5] > meta[:, 5].median()).long()
    rng = np.random.default_rng(6)
    obj = rng.integers(0, 24, 128)
    cand = {"objectId": np.array([f"ZTF21{k:07d}" for k in obj]), "jd": T0 + rng.uniform(0, 40, 128),
            "magpsf": np.round(rng.uniform(17.0, 19.4, 128), 2), "save_time": (T0 + 5.0 + obj % 7).astype(np.float64)}
    summaries = {}
    for name, table in (("with", cand), ("without", None)):
        torch.manual_seed(11)                       # the dropout masks of a one-process run come from torch's device RNG:
        torch.cuda.manual_seed_all(11)              # both runs draw the same ones, as run_training's random_seed arranges
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = btsbot_amd.um_nn(cfg, precision="f32")
        m.load_state_dict(seeded_state(kind, cfg, seed=3))
        m = m.to(cuda).train()
        ds = data.DeviceDataset(None, meta[:384], lab[:384], 64, device=cuda,
                                generator=torch.Generator(device=cuda).manual_seed(2))
        tr = Trainer(m, lr=3e-3, betas=(0.9, 0.999), pos_weight=ds.pos_weight, epochs=2, warmup_epochs=1)
        kw = {} if table is None else {"val_cand": table}
        hist = fit(tr, ds, None, meta[384:], lab[384:], str(tmp_path / name), epochs=2, patience=2, config=cfg, **kw)
        with open(tmp_path / name / "report.json") as f:
            summaries[name] = json.load(f)["val_summary"]
        assert same_performance(summaries[name].get("policy_performance", {}), hist["val_summary"].get("policy_performance", {})) is None
        if table is not None:
            ids = torch.from_numpy(obj).to(cuda)
            want = val.policy_performance(ids, torch.from_numpy(cand["jd"]).to(cuda), torch.from_numpy(cand["magpsf"]).to(cuda),
                                          torch.from_numpy(hist["best_val_labels"]).to(cuda).long(),
                                          torch.from_numpy(hist["best_raw_preds"]).to(cuda),
                                          save_time=torch.from_numpy(cand["save_time"]).to(cuda))
            _, host = restate_policies(obj, cand["jd"], cand["magpsf"], hist["best_val_labels"].astype(np.int64),
                                       hist["best_raw_preds"], save_time=cand["save_time"])
            got = hist["val_summary"]["policy_performance"]
            assert same_performance(got, want) is None, same_performance(got, want)
            assert same_performance(got, host) is None, same_performance(got, host)
    assert set(summaries["with"]) == set(summaries["without"]) | {"policy_performance"}
    assert set(summaries["without"]) == {"roc_auc", "bal_acc", "bts_acc", "notbts_acc", "alert_precision", "alert_recall",
                                         "TP", "TN", "FP", "FN"}
    assert summaries["without"] == {k: v for k, v in summaries["with"].items() if k != "policy_performance"}
