"""Generate tests/golden/diagnostic_fig.npz: seeded synthetic validation alerts and what the REFERENCE'S OWN
diagnostic_fig (btsbot/val.py:173-682) draws and returns for them.  Runs only where a checkout of the reference, pandas,
scikit-learn and matplotlib are at hand:

    python tests/golden/make_diagnostic_golden.py /path/to/reference/btsbot

The recipe is make_policy_golden.py's: the reference module imported by path, its three csv files built in a temporary
working directory.  For the length of the call ``matplotlib.axes.Axes.hist2d``, ``hist``, ``bar``, ``plot`` and ``step``
are wrapped, and their inputs and return values kept: the 28 x 28 score / magnitude array with its edges, the two
marginal histograms, the four 12-bin classification counts, the ROC line and the three 50-bin ``save_dt`` histograms with
their edges.  ``sklearn.metrics.roc_curve``'s three arrays (on the same float64 scores) and the returned scalars are
recorded next to them.

Alerts: make_policy_golden.synthetic_alerts() with edge values written over some rows -- magnitudes exactly 15.0, 16.0,
18.5, 21.0 and one step either side of 15.0 and 21.0 (the nearest float64 that survives the csv file); scores exactly 0.0, 1.0, 0.5 and the float32 neighbours of
the interior score edges 3/28, 0.25 and 20/28.  The magnitudes the fixture keeps are the ones the reference READ BACK from
its csv file, so the recording and the inputs agree whatever the csv parser does to a 17-digit decimal.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_policy_golden import load_reference, synthetic_alerts                       # noqa: E402
from test_diagnostic_host import (CLASS_EDGES, CLASSES, MAG_EDGES, SCORE_EDGES, differences, restate_diagnostic)  # noqa: E402
from test_policy_host import REFERENCE_POLICIES, same_performance                     # noqa: E402


def beside(edge, towards):
    """The float64 nearest to ``edge`` on the side of ``towards`` that the reference's csv round trip (DataFrame.to_csv,
    pd.read_csv with its default parser) gives back unchanged: the parser can be an ulp off on 17-digit decimals."""
    import io
    import pandas as pd
    v = edge
    for _ in range(8):
        v = np.nextafter(v, towards)
        back = pd.read_csv(io.StringIO(pd.DataFrame({"m": [v, 1.5]}).to_csv(index=False)))["m"].to_numpy()[0]
        if back == v:
            return v
    raise AssertionError(f"no neighbour of {edge} survives the csv round trip")


def edge_alerts():
    cols, junk, save, trig = synthetic_alerts()
    rng = np.random.default_rng(20251019)
    n = len(cols["jd"])
    rows = rng.permutation(n)
    mags = [15.0, 16.0, 18.5, 21.0, beside(15.0, 0), beside(15.0, 99), beside(21.0, 0), beside(21.0, 99)]
    print("magnitudes beside the outer edges:", [repr(float(v)) for v in mags[4:]])
    scores = [np.float32(0.0), np.float32(1.0), np.float32(0.5)]
    for k in (3, 7, 20):
        e = np.float32(SCORE_EDGES[k])
        scores += [e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(1))]
    at = 0
    for v in mags:                                                  # four rows each
        cols["magpsf"][rows[at:at + 4]] = v
        at += 4
    for v in scores:
        cols["raw_preds"][rows[at:at + 4]] = v
        at += 4
    return cols, junk, save, trig


class Recorder:
    """Wraps the Axes methods the figure's panels go through and keeps (keyword arguments, positional arguments, return)."""

    def __init__(self):
        self.calls = {k: [] for k in ("hist2d", "hist", "bar", "plot", "step")}

    def __enter__(self):
        from matplotlib.axes import Axes
        self._saved = {k: getattr(Axes, k) for k in self.calls}
        for k, fn in self._saved.items():
            def wrapped(ax, *a, _k=k, _fn=fn, **kw):
                ret = _fn(ax, *a, **kw)
                self.calls[_k].append((a, kw, ret))
                return ret
            setattr(Axes, k, wrapped)
        return self

    def __exit__(self, *exc):
        from matplotlib.axes import Axes
        for k, fn in self._saved.items():
            setattr(Axes, k, fn)


def run_reference(ref, cols, junk, save, trig):
    import pandas as pd
    names = np.array([f"ZTF21{k:07d}" for k in range(len(junk))])
    cand = pd.DataFrame({"objectId": names[cols["object_id"]], "jd": cols["jd"], "magpsf": cols["magpsf"],
                         "label": cols["label"], "peakmag": cols["magpsf"]})
    known = ~np.isnan(save) | ~np.isnan(trig)
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs("data/base_data")
            os.makedirs("out")
            cand.to_csv("cand.csv", index=False)
            back = pd.read_csv("cand.csv", index_col=None)          # what the reference will see
            pd.DataFrame({"ZTFID": names[known], "RCF_save_time": save[known],
                          "RCF_trigger_time": trig[known]}).to_csv("data/base_data/trues.csv", index=False)
            pd.DataFrame({"id": names[junk]}).to_csv("data/base_data/RCFJunk_Feb21_2025.csv", index=False)
            run_data = {"raw_preds": cols["raw_preds"].astype(np.float64), "labels": cols["label"].astype(np.float64),
                        "run_name": "fixture"}
            with Recorder() as rec:
                out = ref.diagnostic_fig(run_data, "cand.csv", "out")
            assert os.path.getsize("out/fixture.pdf") > 0
            return out, rec.calls, back["magpsf"].to_numpy(), back["jd"].to_numpy()
        finally:
            os.chdir(here)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    from sklearn.metrics import roc_curve
    ref = load_reference(sys.argv[1])
    cols, junk, save, trig = edge_alerts()
    out, calls, mag_back, jd_back = run_reference(ref, cols, junk, save, trig)
    assert np.array_equal(jd_back, cols["jd"])
    print("magnitudes changed by the csv round trip:", int((mag_back != cols["magpsf"]).sum()))
    cols["magpsf"] = mag_back
    oid = cols["object_id"]

    (h2d,) = calls["hist2d"]
    joint, xe, ye = (np.asarray(v) for v in h2d[2][:3])
    marg = [c for c in calls["hist"] if c[1].get("histtype") != "step"]
    dts = [c for c in calls["hist"] if c[1].get("histtype") == "step"]
    assert len(marg) == 2 and len(dts) == 3
    bars = {c[1]["label"]: np.asarray(c[0][1]) for c in calls["bar"] if c[1].get("label") in CLASSES}
    (roc_line,) = [c for c in calls["plot"] if str(c[1].get("label", "")).startswith("ROC")]
    assert len(calls["step"]) == 6                                  # completeness and purity of three policies
    sk = roc_curve(cols["label"], cols["raw_preds"].astype(np.float64))
    perf = out["policy_performance"]
    g = dict(cols, obj_junk=junk, obj_save_time=save, obj_trigger_time=trig, policy_names=np.array(list(perf)),
             ref_joint=joint.astype(np.int32), ref_mag_edges=xe, ref_score_edges=ye,
             ref_mag_counts=np.asarray(marg[0][2][0]).astype(np.int32), ref_score_counts=np.asarray(marg[1][2][0]).astype(np.int32),
             ref_class_edges=CLASS_EDGES,                            # (the bars' left ends and width are checked below)
             ref_class_counts=np.stack([bars[c] for c in CLASSES]).astype(np.int32),
             ref_totals=np.array([0, 0, 0, 0], dtype=np.int64),
             ref_roc_x=np.asarray(roc_line[0][0]), ref_roc_y=np.asarray(roc_line[0][1]),
             sk_fpr=sk[0], sk_tpr=sk[1], sk_thresholds=sk[2],
             ref_save_dt_counts=np.stack([np.asarray(c[2][0]) for c in dts]).astype(np.int32),
             ref_save_dt_edges=np.stack([np.asarray(c[2][1]) for c in dts]),
             ref_scalars=np.array([out[k] for k in ("roc_auc", "bal_acc", "bts_acc", "notbts_acc", "alert_precision",
                                                    "alert_recall")], dtype=np.float64),
             ref_precision=np.array([perf[k]["policy_precision"] for k in perf], dtype=np.float64),
             ref_recall=np.array([perf[k]["policy_recall"] for k in perf], dtype=np.float64),
             ref_med_save_dt=np.array([perf[k]["med_save_dt"] for k in perf], dtype=np.float64))
    # the bars start at the class edges' left ends, half a magnitude wide
    left = np.asarray([c for c in calls["bar"] if c[1].get("label") == "TP"][0][0][0])
    assert np.array_equal(left, CLASS_EDGES[:-1]) and np.array_equal(xe, MAG_EDGES) and np.array_equal(ye, SCORE_EDGES)
    # the confusion counts, from the scalars the reference returns: TP / (TP + FN) etc. fix them given the label counts
    lab = cols["label"]
    pred = np.rint(cols["raw_preds"].astype(np.float64)).astype(int)
    g["ref_totals"] = np.array([((lab == 1) & (pred == 1)).sum(), ((lab == 0) & (pred == 1)).sum(),
                                ((lab == 0) & (pred == 0)).sum(), ((lab == 1) & (pred == 0)).sum()], dtype=np.int64)
    tp, fp, tn, fn = (int(v) for v in g["ref_totals"])
    assert out["bts_acc"] == tp / (tp + fn) and out["notbts_acc"] == tn / (tn + fp) and out["alert_precision"] == tp / (tp + fp)

    # the fixture must not be thin, and the restatement must already agree with it
    assert (g["ref_class_counts"] > 0).sum(1).min() >= 6, (g["ref_class_counts"] > 0).sum(1)
    assert len(sk[0]) >= 200, len(sk[0])
    for values, edges in ((cols["magpsf"], MAG_EDGES), (cols["raw_preds"].astype(np.float64), SCORE_EDGES),
                          (cols["magpsf"], CLASS_EDGES)):
        assert np.isin(values, edges).sum() >= 3
    mine = restate_diagnostic(**cols, junk=junk[oid], save_time=save[oid], trigger_time=trig[oid])
    assert differences(mine["hist"], g) == [], differences(mine["hist"], g)
    assert same_performance(mine["policy_performance"], perf) is None, same_performance(mine["policy_performance"], perf)
    assert list(perf) == list(REFERENCE_POLICIES)
    path = os.path.join(HERE, "diagnostic_fig.npz")
    np.savez_compressed(path, **g)
    print(f"{path}: {len(oid)} alerts, {len(sk[0])} ROC points, save_dt over {g['ref_save_dt_counts'].sum(1).tolist()} objects, "
          f"classes in {(g['ref_class_counts'] > 0).sum(1).tolist()} bins, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 100_000


if __name__ == "__main__":
    main()
