"""The data of the reference's diagnostic figure (val.py:173-682), host side: ``restate_diagnostic``, a plain numpy
restatement of the bin rule of btsbot_alert_histograms and of the ROC steps of diagnostics.roc_points, tied to what the
reference's own ``diagnostic_fig`` drew for the fixture (tests/golden/diagnostic_fig.npz, made by
tests/golden/make_diagnostic_golden.py: the inputs and return values of its hist2d / hist / bar / plot calls, sklearn's
roc_curve and the returned scalars).  tests/test_gpu_diagnostic.py imports the restatement as its oracle.  The figure
itself (``draw_diagnostic_fig``) is drawn from the fixture's data where matplotlib is installed."""
import os

import numpy as np
import pytest

from test_policy_host import JAN1_2021, REFERENCE_POLICIES, restate_policies

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diagnostic_fig.npz")
MAG_EDGES, SCORE_EDGES = np.linspace(16, 21, 29), np.linspace(0, 1, 29)
CLASS_EDGES = np.arange(15, 21.5, 0.5)
CLASSES = ("TP", "FP", "TN", "FN")


def bin_of(x, edges, right_closed=False):
    """The bin of every x over ``edges``, -1 for none: bin i holds edges[i] <= x < edges[i+1], the last bin also
    x == edges[-1]; NaN and everything outside are in no bin.  right_closed: the WRONG rule edges[i] < x <= edges[i+1]
    (first bin also x == edges[0]), kept to show that the fixture tells the two apart."""
    x, edges = np.asarray(x, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    nb = len(edges) - 1
    out = np.full(x.shape, -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(nb):
            if right_closed:
                inside = (x > edges[i]) & (x <= edges[i + 1]) | ((x == edges[0]) if i == 0 else False)
            else:
                inside = (x >= edges[i]) & (x < edges[i + 1]) | ((x == edges[nb]) if i == nb - 1 else False)
            out[inside] = i
    return out


def restate_histograms(magpsf, raw_preds, label, mag_edges=MAG_EDGES, score_edges=SCORE_EDGES, class_edges=CLASS_EDGES,
                       right_closed=False, pred_ge=False, marginals_from_joint=False):
    """joint [n_mag, n_score], mag, score, cls [4, n_class] (TP, FP, TN, FN), total [4] as int64 numpy.  The three
    switches are faults on purpose (see test_the_fixture_sees_faults)."""
    mag = np.asarray(magpsf, dtype=np.float64)
    score = np.asarray(raw_preds, dtype=np.float32).astype(np.float64)
    pos = np.asarray(label) != 0
    nm, ns, nc = len(mag_edges) - 1, len(score_edges) - 1, len(class_edges) - 1
    mb, sb, cb = (bin_of(v, e, right_closed) for v, e in ((mag, mag_edges), (score, score_edges), (mag, class_edges)))
    with np.errstate(invalid="ignore"):
        pred = score >= 0.5 if pred_ge else score > 0.5
    which = np.where(pos, np.where(pred, 0, 3), np.where(pred, 1, 2))
    both = (mb >= 0) & (sb >= 0)
    joint = np.bincount(mb[both] * ns + sb[both], minlength=nm * ns).reshape(nm, ns)
    if marginals_from_joint:
        m_cnt, s_cnt = joint.sum(1), joint.sum(0)
    else:
        m_cnt, s_cnt = np.bincount(mb[mb >= 0], minlength=nm), np.bincount(sb[sb >= 0], minlength=ns)
    cls = np.bincount(which[cb >= 0] * nc + cb[cb >= 0], minlength=4 * nc).reshape(4, nc)
    return dict(joint=joint.astype(np.int64), mag=m_cnt.astype(np.int64), score=s_cnt.astype(np.int64),
                cls=cls.astype(np.int64), total=np.bincount(which, minlength=4).astype(np.int64))


def restate_roc(raw_preds, label):
    """sklearn's roc_curve(label, raw_preds) with its defaults, step by step, and the trapezoid area."""
    score = np.asarray(raw_preds, dtype=np.float32).astype(np.float64)
    y = (np.asarray(label) == 1).astype(np.int64)
    order = np.argsort(-score, kind="stable")                       # a stable descending sort
    score, y = score[order], y[order]
    last = np.r_[score[1:] != score[:-1], True] if len(score) else np.zeros(0, dtype=bool)
    tps = np.cumsum(y)[last]                                        # one point per distinct score
    fps = np.arange(1, len(y) + 1)[last] - tps
    thr = score[last]
    if len(tps) > 2:                                                # interior points where neither count bends: dropped
        keep = np.r_[True, (np.diff(fps, 2) != 0) | (np.diff(tps, 2) != 0), True]
        tps, fps, thr = tps[keep], fps[keep], thr[keep]
    tps, fps, thr = np.r_[0, tps].astype(np.float64), np.r_[0, fps].astype(np.float64), np.r_[np.inf, thr]
    nan = np.full(len(tps), np.nan)
    fpr = fps / fps[-1] if fps[-1] > 0 else nan
    tpr = tps / tps[-1] if tps[-1] > 0 else nan.copy()
    auc = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2)) if len(fpr) >= 2 else float("nan")
    return dict(fpr=fpr, tpr=tpr, thresholds=thr, auc=auc)


def restate_save_dt(object_id, jd, magpsf, label, raw_preds, policies=REFERENCE_POLICIES, junk=None, save_time=None,
                    trigger_time=None):
    """(per policy: None, or the sorted save_dt values of the true-positive objects and their 50-bin histogram over
    [min, max] with its edges; the policy_performance dictionary)."""
    obj, perf = restate_policies(object_id, jd, magpsf, label, raw_preds, policies, junk, save_time, trigger_time)
    save = np.full(len(obj["first_alert"]), np.nan) if save_time is None else \
        np.asarray(save_time, dtype=np.float64)[obj["first_alert"]]
    out = {}
    for p, name in enumerate(policies):
        out[name] = None
        if name in obj.get("cells", {}):
            tjd = obj["trigger_jd"][:, p]
            with np.errstate(invalid="ignore"):
                ok = obj["cells"][name]["tp"] & (save >= JAN1_2021) & (tjd > 0)
            vals = np.sort((tjd - save)[ok])
            if len(vals):
                counts, edges = np.histogram(vals, bins=50, range=(vals.min(), vals.max()))
                out[name] = dict(values=vals, counts=counts, edges=edges)
    return out, perf


def restate_diagnostic(object_id, jd, magpsf, label, raw_preds, junk=None, save_time=None, trigger_time=None,
                       policies=REFERENCE_POLICIES, **faults):
    """Everything diagnostics.diagnostic_data counts, in numpy."""
    save, perf = restate_save_dt(object_id, jd, magpsf, label, raw_preds, policies, junk, save_time, trigger_time)
    return dict(hist=restate_histograms(magpsf, raw_preds, label, **faults), roc=restate_roc(raw_preds, label),
                policy_save_dt=save, policy_performance=perf)


def golden_inputs(g):
    oid = g["object_id"]
    rows = dict(object_id=oid, jd=g["jd"], magpsf=g["magpsf"], label=g["label"], raw_preds=g["raw_preds"])
    extra = dict(junk=g["obj_junk"][oid], save_time=g["obj_save_time"][oid], trigger_time=g["obj_trigger_time"][oid])
    return rows, extra


def differences(hist, g):
    """Names of the recorded count arrays that ``hist`` does not equal."""
    want = dict(joint=g["ref_joint"], mag=g["ref_mag_counts"], score=g["ref_score_counts"], cls=g["ref_class_counts"])
    return [k for k, w in want.items() if not np.array_equal(hist[k], w.astype(np.int64))]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_restatement_reproduces_the_reference(golden):
    """Counts, ROC points, save_dt histograms and their edges equal what the reference's figure drew, exactly; auc within
    1e-12 (a few hundred terms of magnitude <= 1: the summation order can move it by about 1e-13)."""
    g = golden
    assert os.path.getsize(GOLDEN) < 100_000
    assert np.array_equal(g["ref_mag_edges"], MAG_EDGES) and np.array_equal(g["ref_score_edges"], SCORE_EDGES)
    assert np.array_equal(g["ref_class_edges"], CLASS_EDGES)
    rows, extra = golden_inputs(g)
    got = restate_diagnostic(**rows, **extra)
    assert differences(got["hist"], g) == []
    # the fixture is not thin
    assert (g["ref_class_counts"] > 0).sum(1).min() >= 6 and len(g["sk_fpr"]) >= 200
    mag, score = rows["magpsf"], rows["raw_preds"].astype(np.float64)
    for values, edges in ((mag, MAG_EDGES), (score, SCORE_EDGES), (mag, CLASS_EDGES)):
        assert np.isin(values, edges).sum() >= 3
    for v in (15.0, 16.0, 18.5, 21.0):
        assert (mag == v).any(), v
    for edge in (15.0, 21.0):                                      # and a few ulps either side of the outer edges
        assert ((mag < edge) & (mag > edge - 1e-13)).any() and ((mag > edge) & (mag < edge + 1e-13)).any(), edge
    assert all((rows["raw_preds"] == np.float32(v)).any() for v in (0.0, 1.0, 0.5))
    near = [k for k in range(1, 28) if any((rows["raw_preds"] == np.nextafter(np.float32(SCORE_EDGES[k]), np.float32(d))).any()
                                           for d in (0, 1))]
    assert len(near) >= 2
    tot = got["hist"]["total"]
    for k, c in enumerate(CLASSES):
        assert tot[k] == int(g["ref_totals"][k]), c
    # ROC: sklearn's arrays, and the line the figure drew
    roc = got["roc"]
    for k in ("fpr", "tpr", "thresholds"):
        assert np.array_equal(roc[k], g["sk_" + k]), k
    assert np.array_equal(g["ref_roc_x"], g["sk_fpr"]) and np.array_equal(g["ref_roc_y"], g["sk_tpr"])
    assert abs(roc["auc"] - float(g["ref_scalars"][0])) <= 1e-12
    # the three drawn save_dt histograms
    names = list(REFERENCE_POLICIES)
    assert [str(s) for s in g["policy_names"]] == names
    for q in range(3):
        dt = got["policy_save_dt"][names[q]]
        assert np.array_equal(dt["counts"], g["ref_save_dt_counts"][q].astype(np.int64)), names[q]
        assert np.array_equal(dt["edges"], g["ref_save_dt_edges"][q]), names[q]
        assert dt["counts"].sum() == len(dt["values"]) >= 20


def test_the_fixture_sees_faults(golden):
    """A right-closed bin rule, pred = raw >= 0.5 and marginals summed from the joint histogram each differ from the
    recording."""
    rows, _ = golden_inputs(golden)
    args = (rows["magpsf"], rows["raw_preds"], rows["label"])
    assert differences(restate_histograms(*args), golden) == []
    closed = differences(restate_histograms(*args, right_closed=True), golden)
    assert {"joint", "mag", "score", "cls"} <= set(closed), closed
    ge = restate_histograms(*args, pred_ge=True)
    assert differences(ge, golden) == ["cls"] and not np.array_equal(ge["total"], golden["ref_totals"].astype(np.int64))
    # (every score of the fixture is inside [0, 1] -- roc_curve takes no NaN --, so it is the score marginal that shows it:
    #  the alerts brighter than 16 or fainter than 21 are in it and in no cell of the joint histogram)
    summed = differences(restate_histograms(*args, marginals_from_joint=True), golden)
    assert summed == ["score"], summed


def test_bin_rule_by_hand():
    e = np.array([0.0, 1.0, 2.5, 4.0])
    x = np.array([0.0, -0.0, 1.0, np.nextafter(1.0, 0), 2.5, 4.0, np.nextafter(4.0, 9), np.nan, np.inf, -np.inf, -1e-300])
    assert list(bin_of(x, e)) == [0, 0, 1, 0, 2, 2, -1, -1, -1, -1, -1]
    assert list(bin_of(x, e, right_closed=True)) == [0, 0, 0, 0, 1, 2, -1, -1, -1, -1, -1]
    h = restate_histograms([16.0, 21.0, 15.0, np.nan, 30.0], [0.5, np.nan, 1.0, 0.7, 0.2], [1, 1, 0, 0, 0])
    assert h["total"].tolist() == [0, 2, 1, 2]                     # 0.5 and NaN predict 0; every alert is in a total
    assert h["joint"].sum() == 1 and h["joint"][0, 14] == 1        # (16.0, 0.5) alone has both coordinates inside
    assert h["mag"].sum() == 2 and h["score"].sum() == 4 and h["cls"].sum() == 3
    assert h["cls"][3, 2] == 1 and h["cls"][3, 11] == 1 and h["cls"][1, 0] == 1


def test_roc_by_hand():
    sklearn_metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(3)
    for n, decimals in ((1, 2), (2, 2), (3, 1), (50, 1), (400, 2), (400, 7)):
        y = rng.integers(0, 2, n)
        y[0], y[-1] = (1, 0) if n > 1 else (1, 1)
        s = np.round(rng.random(n), decimals).astype(np.float32)
        want = sklearn_metrics.roc_curve(y, s.astype(np.float64)) if n > 1 else None
        got = restate_roc(s, y)
        if want is not None:
            for k, w in zip(("fpr", "tpr", "thresholds"), want):
                assert np.array_equal(got[k], w), (n, decimals, k)
            assert abs(got["auc"] - sklearn_metrics.auc(want[0], want[1])) <= 1e-12
    only_pos = restate_roc([0.2, 0.9], [1, 1])
    assert np.isnan(only_pos["fpr"]).all() and list(only_pos["tpr"]) == [0.0, 0.5, 1.0] and np.isnan(only_pos["auc"])


def test_wrappers_check_arguments_without_a_device():
    import torch
    import btsbot_amd
    from btsbot_amd import diagnostics
    for name in ("alert_histograms", "roc_points", "diagnostic_data", "diagnostic_fig", "draw_diagnostic_fig"):
        assert getattr(btsbot_amd, name) is getattr(diagnostics, name)
    z, i = torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="runs on the GPU; there is no CPU fallback"):
        diagnostics.alert_histograms(z, z.float(), i)
    for kw in (dict(mag_bins=65), dict(score_bins=0), dict(class_bins=[1.0, 3.0, 2.0]), dict(class_bins=[1.0, np.nan]),
               dict(mag_bins=np.linspace(0, 1, 67)), dict(class_bins=[1.0])):
        with pytest.raises(ValueError):
            diagnostics.alert_histograms(z, z.float(), i, **kw)


def test_draw_diagnostic_fig_from_the_fixture(golden, tmp_path, monkeypatch):
    """The figure drawn from the fixture's data alone: a 4 x 3 grid, the ROC line through the recorded points, the density
    panel's array equal to the recorded one, a PDF on disk, and no torch.cuda call on the way."""
    pytest.importorskip("matplotlib")
    import torch
    from btsbot_amd import diagnostics
    g = golden
    rows, extra = golden_inputs(g)
    r = restate_diagnostic(**rows, **extra)
    names = list(REFERENCE_POLICIES)
    tp, fp, tn, fn = (int(v) for v in r["hist"]["total"])
    data = {
        "roc": {"fpr": g["sk_fpr"].tolist(), "tpr": g["sk_tpr"].tolist(), "thresholds": g["sk_thresholds"].tolist(),
                "auc": float(g["ref_scalars"][0])},
        "score_mag_hist": {"counts": g["ref_joint"].astype(int).tolist(), "mag_edges": g["ref_mag_edges"].tolist(),
                           "score_edges": g["ref_score_edges"].tolist(), "mag_counts": g["ref_mag_counts"].astype(int).tolist(),
                           "score_counts": g["ref_score_counts"].astype(int).tolist()},
        "class_mag_hist": dict({"bins": g["ref_class_edges"].tolist()},
                               **{c: g["ref_class_counts"][k].astype(int).tolist() for k, c in enumerate(CLASSES)}),
        "confusion": {"TP": tp, "FP": fp, "TN": tn, "FN": fn,
                      "normalized": [[tn / (tn + fp), fp / (tn + fp)], [fn / (fn + tp), tp / (fn + tp)]]},
        "summary": dict(zip(("roc_auc", "bal_acc", "bts_acc", "notbts_acc", "alert_precision", "alert_recall"),
                            (float(v) for v in g["ref_scalars"]))),
        "history": {"loss": [0.7, 0.5, 0.4], "val_loss": [0.8, 0.6, 0.5], "accuracy": [0.6, 0.8, 0.85],
                    "val_accuracy": [0.55, 0.75, 0.8]},
        "policy_performance": r["policy_performance"],
        "policy_save_dt": {k: None if v is None else {kk: vv.tolist() for kk, vv in v.items()}
                           for k, v in r["policy_save_dt"].items()},
    }

    def no_cuda(*a, **k):
        raise AssertionError("draw_diagnostic_fig touched torch.cuda")
    for fn_name in ("current_stream", "synchronize", "current_device", "_lazy_init", "is_available", "device_count"):
        monkeypatch.setattr(torch.cuda, fn_name, no_cuda)
    fig = diagnostics.draw_diagnostic_fig(data, "fixture")
    path = tmp_path / "fixture.pdf"
    fig.savefig(str(path), bbox_inches="tight")
    monkeypatch.undo()
    assert path.stat().st_size > 10_000
    main = [ax for ax in fig.axes if ax.get_subplotspec() is not None and ax.get_subplotspec().get_gridspec().get_geometry() == (4, 3)]
    assert sorted(ax.get_subplotspec().num1 for ax in main) == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11]   # cell 3 holds the 2 x 2
    inner = [ax for ax in fig.axes if ax.get_subplotspec() is not None and ax.get_subplotspec().get_gridspec().get_geometry() == (2, 2)]
    assert len(inner) == 3 and len(fig.axes) == 15                                                    # + the colour bar
    roc_ax = next(ax for ax in main if ax.get_subplotspec().num1 == 2)
    line = next(ln for ln in roc_ax.lines if str(ln.get_label()).startswith("ROC"))
    assert np.array_equal(line.get_xdata(), g["sk_fpr"]) and np.array_equal(line.get_ydata(), g["sk_tpr"])
    mesh = next(ax for ax in inner if ax.collections).collections[0]
    drawn = np.ma.filled(mesh.get_array(), 0).reshape(28, 28).T                                       # [mag bin, score bin]
    assert np.array_equal(drawn, g["ref_joint"])
    bars = next(ax for ax in main if ax.get_subplotspec().num1 == 5)
    heights = np.array([p.get_height() for p in bars.patches if p.get_width() == 0.5]).reshape(4, 12)
    assert np.array_equal(heights, g["ref_class_counts"])
    for q in range(3):                                                                                # the save_dt stairs
        st_ax = next(ax for ax in main if ax.get_subplotspec().num1 == 9 + q)
        stairs = [p for p in st_ax.patches if hasattr(p, "get_data")]
        assert len(stairs) == 1 and np.array_equal(stairs[0].get_data().values, g["ref_save_dt_counts"][q])
    import matplotlib.pyplot as plt
    plt.close(fig)
