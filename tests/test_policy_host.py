"""The per-object policy metrics of the reference's diagnostic_fig (val.py:381-614), host side: a plain numpy restatement
of the rules btsbot_policy_eval and val.policy_performance implement, tied to the reference's recorded output
(tests/golden/policy_performance.npz, made by tests/golden/make_policy_golden.py from the reference's own function), and
the rules a fixture can miss, on hand-made objects.  tests/test_gpu_policy.py imports the restatement as its oracle."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_performance.npz")
REFERENCE_POLICIES = {"bts_p1": (0.5, 19.0, 2, None), "bts_p2": (0.5, 19.0, 2, 18.5),
                      "prod_p1": (0.85, 19.0, 1, None), "prod_p2": (0.85, 19.0, 1, 18.5)}
BINS = np.arange(17.0, 18.75, 0.25)
JAN1_2021 = 2459215.5


def restate_objects(object_id, jd, magpsf, label, raw_preds, policies):
    """Per object (ascending id): ids, n_alerts, label of the first alert in input order, min magpsf (NaN skipped), and
    per policy pred, trigger_jd, trigger_mag.  Alerts of an object are walked in (jd, input position) order; a policy
    fires at an alert when the valid alerts so far number at least k and (no gate or) the minimum so far is <= gate."""
    object_id, jd, magpsf, label = (np.asarray(x) for x in (object_id, jd, magpsf, label))
    score = np.asarray(raw_preds, dtype=np.float32).astype(np.float64)
    jd, magpsf = jd.astype(np.float64), magpsf.astype(np.float64)
    ids = np.unique(object_id)
    pols = list(policies.values())
    out = dict(object_id=ids, n_alerts=np.zeros(len(ids), dtype=np.int64), label=np.zeros(len(ids), dtype=np.int64),
               min_magpsf=np.full(len(ids), np.nan), first_alert=np.zeros(len(ids), dtype=np.int64),
               pred=np.zeros((len(ids), len(pols)), dtype=np.int32),
               trigger_jd=np.full((len(ids), len(pols)), -1.0), trigger_mag=np.full((len(ids), len(pols)), -1.0))
    for o, oid in enumerate(ids):
        rows = np.flatnonzero(object_id == oid)                        # input order
        out["n_alerts"][o], out["label"][o], out["first_alert"][o] = len(rows), label[rows[0]], rows[0]
        m = magpsf[rows]
        if not np.isnan(m).all():
            out["min_magpsf"][o] = np.nanmin(m)
        walk = rows[np.lexsort((rows, jd[rows]))]                      # by jd, equal jd by input position
        so_far = np.fmin.accumulate(magpsf[walk])                      # NaN skipped; NaN until a magnitude is seen
        for p, (thr, cut, k, gate) in enumerate(pols):
            count = np.cumsum((score[walk] > thr) & (magpsf[walk] < cut))
            fires = count >= k
            if gate is not None and not np.isnan(gate):
                fires &= so_far <= gate
            if fires.any():
                at = walk[np.argmax(fires)]
                assert fires[-1]                                       # monotone: fires at the last alert too
                out["pred"][o, p], out["trigger_jd"][o, p], out["trigger_mag"][o, p] = 1, jd[at], magpsf[at]
    return out


def restate_policies(object_id, jd, magpsf, label, raw_preds, policies=REFERENCE_POLICIES, junk=None, save_time=None,
                     trigger_time=None):
    """(per-object arrays of restate_objects, the reference's policy_performance dictionary).  junk / save_time /
    trigger_time are per alert row; an object takes its first alert's."""
    obj = restate_objects(object_id, jd, magpsf, label, raw_preds, policies)
    first = obj["first_alert"]
    n_obj = len(first)
    is_junk = np.zeros(n_obj, dtype=bool) if junk is None else np.asarray(junk, dtype=bool)[first]
    save = np.full(n_obj, np.nan) if save_time is None else np.asarray(save_time, dtype=np.float64)[first]
    trig = np.full(n_obj, np.nan) if trigger_time is None else np.asarray(trigger_time, dtype=np.float64)[first]
    with np.errstate(invalid="ignore"):
        thinned = (obj["label"] == 1) & (obj["min_magpsf"] > 18.5)
    taken = ~is_junk & (obj["n_alerts"] >= 2) & ~thinned
    obj["taken"] = taken
    perf = {}
    for p, name in enumerate(policies):
        pred, tjd = obj["pred"][:, p] == 1, obj["trigger_jd"][:, p]
        pos, neg = taken & (obj["label"] == 1), taken & (obj["label"] != 1)
        tp, fp, fn, tn = pos & pred, neg & pred, pos & ~pred, neg & ~pred
        if tp.sum() == 0 or tn.sum() == 0:
            perf[name] = dict(policy_precision=-999.0, policy_recall=-999.0, binned_precision=[-999.0],
                              binned_recall=[-999.0], peakmag_bins=list(BINS), med_save_dt=-999.0, med_trigger_dt=-999.0)
            continue
        btp, bfp, bfn = (np.histogram(obj["min_magpsf"][m], bins=BINS)[0] for m in (tp, fp, fn))
        with np.errstate(invalid="ignore", divide="ignore"):
            ok_s = tp & (save >= JAN1_2021) & (tjd > 0)
            ok_t = tp & (trig >= JAN1_2021) & (trig < 1e10) & (tjd > 0)
            perf[name] = dict(policy_precision=tp.sum() / (tp.sum() + fp.sum()), policy_recall=tp.sum() / (tp.sum() + fn.sum()),
                              binned_precision=list(btp / (btp + bfp)), binned_recall=list(btp / (btp + bfn)),
                              peakmag_bins=list(BINS),
                              med_save_dt=float(np.median((tjd - save)[ok_s])) if ok_s.any() else np.nan,
                              med_trigger_dt=float(np.median((tjd - trig)[ok_t])) if ok_t.any() else np.nan)
        obj.setdefault("cells", {})[name] = dict(tp=tp, fp=fp, fn=fn, tn=tn, n_save=int(ok_s.sum()), n_trigger=int(ok_t.sum()))
    return obj, perf


def same_performance(got, want):
    """Exact equality of two policy_performance dictionaries, NaN positions included; returns the first difference."""
    if list(got) != list(want):
        return f"policies {list(got)} != {list(want)}"
    for name in want:
        if set(got[name]) != set(want[name]):
            return f"{name}: keys {sorted(got[name])} != {sorted(want[name])}"
        for key, w in want[name].items():
            g = np.atleast_1d(np.asarray(got[name][key], dtype=np.float64))
            w = np.atleast_1d(np.asarray(w, dtype=np.float64))
            if g.shape != w.shape or not np.array_equal(g, w, equal_nan=True):
                return f"{name}.{key}: got {g.tolist()}, want {w.tolist()}"
    return None


def golden_inputs(g):
    """The fixture's per-alert arrays, the per-object junk / save / trigger columns spread over the alert rows as a csv
    join would, and the reference's recorded dictionary."""
    oid = g["object_id"]
    rows = dict(object_id=oid, jd=g["jd"], magpsf=g["magpsf"], label=g["label"], raw_preds=g["raw_preds"])
    extra = dict(junk=g["obj_junk"][oid], save_time=g["obj_save_time"][oid], trigger_time=g["obj_trigger_time"][oid])
    want = {str(name): dict(policy_precision=float(g["ref_precision"][p]), policy_recall=float(g["ref_recall"][p]),
                            binned_precision=list(g["ref_binned_precision"][p]), binned_recall=list(g["ref_binned_recall"][p]),
                            peakmag_bins=list(g["ref_peakmag_bins"]), med_save_dt=float(g["ref_med_save_dt"][p]),
                            med_trigger_dt=float(g["ref_med_trigger_dt"][p]))
            for p, name in enumerate(g["policy_names"])}
    return rows, extra, want


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_restatement_reproduces_the_reference(golden):
    """The restatement gives the reference's recorded policy_performance for its four policies exactly: precision, recall,
    every binned entry, both medians.  The fixture is not thin: every confusion cell and every bin is populated and at
    least 20 objects enter each median."""
    from btsbot_amd import val
    assert val.REFERENCE_POLICIES == REFERENCE_POLICIES and list(golden["policy_names"]) == list(REFERENCE_POLICIES)
    assert np.array_equal(np.asarray(val.PEAKMAG_BINS), BINS) and np.array_equal(golden["ref_peakmag_bins"], BINS)
    assert val.JAN1_2021_JD == JAN1_2021
    rows, extra, want = golden_inputs(golden)
    oid, jd = rows["object_id"], rows["jd"]
    sizes = np.bincount(oid)
    assert 1000 <= len(jd) <= 2500 and 120 <= len(sizes) <= 200 and sizes.min() == 1 and sizes.max() > 64
    assert all(len(np.unique(jd[oid == k])) == sizes[k] for k in range(len(sizes)))            # distinct jd per object
    assert golden["raw_preds"].dtype == np.float32 and (golden["raw_preds"] == 0.5).sum() >= 3
    assert (golden["raw_preds"] == np.float32(0.85)).sum() >= 3 and golden["obj_junk"].sum() >= 2
    assert not np.array_equal(oid, np.sort(oid))                                               # shuffled
    obj, got = restate_policies(**rows, **extra)
    assert same_performance(got, want) is None, same_performance(got, want)
    for name in REFERENCE_POLICIES:
        c = obj["cells"][name]
        assert min(c[k].sum() for k in ("tp", "fp", "fn", "tn")) > 0 and c["n_save"] >= 20 and c["n_trigger"] >= 20
        assert np.isfinite(want[name]["binned_precision"]).all() and np.isfinite(want[name]["binned_recall"]).all()
    # the gate matters, the policies differ, triggers are not all at the first alert, some objects are filtered
    assert (obj["pred"][:, 0] != obj["pred"][:, 1]).any() and (obj["pred"][:, 0] != obj["pred"][:, 2]).any()
    assert (obj["trigger_jd"][:, 1] > obj["trigger_jd"][:, 0])[obj["pred"][:, 1] == 1].any()
    assert (~obj["taken"]).sum() > 10 and ((obj["label"] == 1) & (obj["min_magpsf"] > 18.5)).any()


def _one(jd, mag, score, label=1, oid=7):
    n = len(jd)
    return dict(object_id=np.full(n, oid, dtype=np.int64), jd=np.asarray(jd, dtype=np.float64),
                magpsf=np.asarray(mag, dtype=np.float64), label=np.full(n, label, dtype=np.int64),
                raw_preds=np.asarray(score, dtype=np.float32))


def _cat(*cases):
    return {k: np.concatenate([c[k] for c in cases]) for k in cases[0]}


def test_minus_999_without_a_true_positive_or_a_true_negative():
    t = 2459300.5
    saved = _one([t, t + 1], [18.0, 18.2], [0.9, 0.9], label=1, oid=1)
    passed = _one([t, t + 1], [18.0, 18.2], [0.1, 0.1], label=0, oid=2)
    missed = _one([t, t + 1], [18.0, 18.2], [0.1, 0.1], label=1, oid=3)
    _, both = restate_policies(**_cat(saved, passed))
    assert both["prod_p1"]["policy_precision"] == 1.0 and both["prod_p1"]["policy_recall"] == 1.0
    assert len(both["prod_p1"]["binned_precision"]) == 6 and np.isnan(both["prod_p1"]["med_save_dt"])
    for case in (_cat(saved, missed), _cat(missed, passed)):              # no TN; no TP
        _, perf = restate_policies(**case)
        for name in REFERENCE_POLICIES:
            assert perf[name]["policy_precision"] == perf[name]["policy_recall"] == -999.0
            assert perf[name]["binned_precision"] == perf[name]["binned_recall"] == [-999.0]
            assert perf[name]["med_save_dt"] == perf[name]["med_trigger_dt"] == -999.0
            assert perf[name]["peakmag_bins"] == list(BINS)


def test_even_count_median_averages_the_two_middle_values():
    """Four true positives saved 1, 2, 4 and 8 days after the scanners: the median is 3, not torch.nanmedian's 2; the
    device-side column median agrees, with NaN rows and an empty column."""
    from btsbot_amd.val import _median_columns
    t = 2459300.5
    objs = [_one([t, t + d], [18.0, 18.2], [0.1, 0.9], oid=k) for k, d in enumerate((1.0, 2.0, 4.0, 8.0))]
    objs.append(_one([t, t + 1], [18.0, 18.2], [0.1, 0.1], label=0, oid=9))
    case = _cat(*objs)
    n = len(case["jd"])
    _, perf = restate_policies(**case, save_time=np.full(n, t), trigger_time=np.full(n, t - 0.5))
    assert perf["prod_p1"]["med_save_dt"] == 3.0 and perf["prod_p1"]["med_trigger_dt"] == 3.5
    nan = float("nan")
    x = torch.tensor([[1.0, nan, 5.0], [nan, nan, 1.0], [8.0, nan, 2.0], [2.0, nan, nan], [4.0, nan, nan]], dtype=torch.float64)
    med = _median_columns(x)
    assert med[0] == 3.0 and torch.isnan(med[1]) and med[2] == 2.0
    assert torch.nanmedian(x[:, 0]) == 2.0                                 # what the plain call would have given
    a, b = 0.1, 0.7                                                        # (a + b) / 2 is what np.median rounds to
    assert _median_columns(torch.tensor([[a], [b]], dtype=torch.float64))[0].item() == np.median([a, b])


def test_histogram_edges():
    """np.histogram's bins: 18.5 itself counts in the last bin, 18.5000001 and anything below 17.0 are dropped, an edge
    belongs to the bin on its right."""
    t = 2459300.5
    peaks = (18.5, 18.5000001, 16.9, 17.0, 17.25, 18.4999)
    objs = [_one([t, t + 1], [pk, pk + 0.3], [0.9, 0.9], label=0, oid=k) for k, pk in enumerate(peaks)]   # six FP
    objs.append(_one([t, t + 1], [18.1, 18.2], [0.9, 0.9], label=1, oid=20))                               # a TP
    objs.append(_one([t, t + 1], [18.1, 18.2], [0.1, 0.1], label=0, oid=21))                               # a TN
    obj, perf = restate_policies(**_cat(*objs))
    assert perf["prod_p1"]["policy_precision"] == 1 / 7
    fp = np.histogram(obj["min_magpsf"][obj["cells"]["prod_p1"]["fp"]], bins=BINS)[0]
    assert list(fp) == [1, 1, 0, 0, 0, 2]
    bp = perf["prod_p1"]["binned_precision"]
    assert bp[0] == 0.0 and bp[1] == 0.0 and np.isnan(bp[2]) and np.isnan(bp[3]) and bp[4] == 1.0 and bp[5] == 0.0


def test_label_is_the_first_alert_in_input_order():
    """Not the earliest alert's, not the majority's: the first row of the object as the table lists it."""
    t = 2459300.5
    case = _one([t + 5, t, t + 1], [18.0, 18.1, 18.2], [0.9, 0.9, 0.9])
    case["label"] = np.array([0, 1, 1])
    other = _one([t, t + 1], [18.0, 18.2], [0.9, 0.9], label=1, oid=3)
    obj, _ = restate_policies(**_cat(other, case))
    assert list(obj["object_id"]) == [3, 7] and list(obj["label"]) == [1, 0] and list(obj["first_alert"]) == [0, 2]


def test_policy_wrappers_check_arguments_without_a_device():
    import btsbot_amd
    from btsbot_amd import val
    assert btsbot_amd.policy_eval is val.policy_eval and btsbot_amd.policy_performance is val.policy_performance
    assert btsbot_amd.REFERENCE_POLICIES is val.REFERENCE_POLICIES and val.POLICY_TILE > 64
    z = torch.zeros(4, dtype=torch.float64)
    i = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        val.policy_eval(i, z, z, i, z.float())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        val.policy_performance(i, z, z, i, z.float())
