"""Generate tests/golden/policy_performance.npz: seeded synthetic validation alerts and the ``policy_performance``
dictionary the REFERENCE'S OWN diagnostic_fig (btsbot/val.py:173-682) returns for them.  Runs only where a checkout of the
reference, pandas, scikit-learn and matplotlib are at hand:

    python tests/golden/make_policy_golden.py /path/to/reference/btsbot

The reference module is imported by path.  Its ``utils`` and ``architectures`` imports serve run_val only, so empty
stand-in modules take their place.  diagnostic_fig reads ``data/base_data/trues.csv`` (scanners' save and trigger
times), ``data/base_data/RCFJunk_Feb21_2025.csv`` (junk objects) and the candidate csv, and writes its figure: all of
that happens in a temporary working directory.

Alerts: about 150 objects and 1,500 alerts in shuffled order; jd distinct inside an object (the reference sorts with an
unstable sort, so ties would not be defined); sizes 1, 1, 2, 2, 3, ... plus a few of 40-80; labels about half and half;
peak magnitudes over 16.8-19.6; scores clustered by label but overlapping, several exactly 0.5 and several exactly the
float32 next to 0.85 (and the float32 below it).  The scores are float32 values and go to the reference widened to
float64, so that its comparisons are the float64 ones of the contract whatever the numpy version's promotion rules.
A few junk objects; save and trigger times known for about half the objects, some before 2021, some triggers 1e12.
Every jd and time has five decimals and every magnitude three: the reference reads them back from csv files, and short
decimals survive its parser exactly.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_policy_host import REFERENCE_POLICIES, restate_policies, same_performance   # noqa: E402


def load_reference(ref_dir):
    utils = types.ModuleType("utils")
    utils.FlexibleDataset = object
    sys.modules.setdefault("utils", utils)
    sys.modules.setdefault("architectures", types.ModuleType("architectures"))
    spec = importlib.util.spec_from_file_location("reference_val", os.path.join(ref_dir, "val.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synthetic_alerts(seed=20250221, n_objects=150):
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([np.repeat(np.arange(1, 13), 2), rng.integers(3, 14, n_objects - 24 - 6), [41, 48, 57, 66, 73, 80]])
    low32 = np.nextafter(np.float32(0.85), np.float32(0))
    oid, jd, mag, lab, raw = [], [], [], [], []
    junk, save, trig = np.zeros(len(sizes), dtype=bool), np.full(len(sizes), np.nan), np.full(len(sizes), np.nan)
    for k, n in enumerate(sizes):
        label = int(rng.random() < 0.55)
        t = np.round(2459250.5 + float(rng.uniform(0, 700)) + np.cumsum(rng.uniform(0.02, 4.0, n)), 5)
        assert len(np.unique(t)) == n
        peak = float(rng.uniform(16.8, 18.9 if label else 19.6))
        at = int(rng.integers(0, n))                                   # the light curve's brightest alert
        m = peak + np.abs(np.arange(n) - at) * float(rng.uniform(0.02, 0.5)) + rng.uniform(0, 0.2, n)
        m[at] = peak
        m = np.round(m, 3)
        good = rng.random() < (0.85 if label else 0.2)                 # what the model thinks of the object
        s = np.clip(rng.normal(0.82 if good else 0.25, 0.2, n), 0.001, 0.999).astype(np.float32)
        pick = rng.random(n)
        s[pick < 0.04] = np.float32(0.5)
        s[(pick >= 0.04) & (pick < 0.08)] = np.float32(0.85)
        s[(pick >= 0.08) & (pick < 0.10)] = low32
        order = rng.permutation(n)                                     # input order is not time order
        oid.append(np.full(n, k)); jd.append(t[order]); mag.append(m[order]); lab.append(np.full(n, label)); raw.append(s[order])
        junk[k] = rng.random() < 0.04
        if rng.random() < (0.85 if label else 0.15):
            early = rng.random() < 0.12
            save[k] = round((2458800.5 if early else t[0]) + float(rng.uniform(-3, 12)), 5)
            u = rng.random()
            trig[k] = np.nan if u < 0.1 else 1e12 if u < 0.2 else round(save[k] - float(rng.uniform(0, 2)), 5)
    cols = dict(object_id=np.concatenate(oid).astype(np.int64), jd=np.concatenate(jd), magpsf=np.concatenate(mag),
                label=np.concatenate(lab).astype(np.int64), raw_preds=np.concatenate(raw).astype(np.float32))
    order = rng.permutation(len(cols["jd"]))
    return {k: v[order] for k, v in cols.items()}, junk, save, trig


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
            pd.DataFrame({"ZTFID": names[known], "RCF_save_time": save[known],
                          "RCF_trigger_time": trig[known]}).to_csv("data/base_data/trues.csv", index=False)
            pd.DataFrame({"id": names[junk]}).to_csv("data/base_data/RCFJunk_Feb21_2025.csv", index=False)
            run_data = {"raw_preds": cols["raw_preds"].astype(np.float64), "labels": cols["label"].astype(np.float64),
                        "run_name": "fixture"}
            return ref.diagnostic_fig(run_data, "cand.csv", "out")["policy_performance"]
        finally:
            os.chdir(here)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    cols, junk, save, trig = synthetic_alerts()
    oid = cols["object_id"]
    perf = run_reference(ref, cols, junk, save, trig)
    assert list(perf) == list(REFERENCE_POLICIES)
    obj, mine = restate_policies(**cols, junk=junk[oid], save_time=save[oid], trigger_time=trig[oid])
    assert same_performance(mine, perf) is None, same_performance(mine, perf)
    for name in perf:                                                  # the fixture must not be thin
        c = obj["cells"][name]
        cells = {k: int(c[k].sum()) for k in ("tp", "fp", "fn", "tn")}
        assert min(cells.values()) > 0, (name, cells)
        assert np.isfinite(perf[name]["binned_precision"]).all() and np.isfinite(perf[name]["binned_recall"]).all(), name
        assert c["n_save"] >= 20 and c["n_trigger"] >= 20, (name, c["n_save"], c["n_trigger"])
        print(name, cells, "medians over", c["n_save"], c["n_trigger"], {k: perf[name][k] for k in
              ("policy_precision", "policy_recall", "med_save_dt", "med_trigger_dt")})
    out = dict(cols, obj_junk=junk, obj_save_time=save, obj_trigger_time=trig, policy_names=np.array(list(perf)),
               ref_precision=np.array([perf[k]["policy_precision"] for k in perf], dtype=np.float64),
               ref_recall=np.array([perf[k]["policy_recall"] for k in perf], dtype=np.float64),
               ref_binned_precision=np.array([perf[k]["binned_precision"] for k in perf], dtype=np.float64),
               ref_binned_recall=np.array([perf[k]["binned_recall"] for k in perf], dtype=np.float64),
               ref_peakmag_bins=np.array(perf["bts_p1"]["peakmag_bins"], dtype=np.float64),
               ref_med_save_dt=np.array([perf[k]["med_save_dt"] for k in perf], dtype=np.float64),
               ref_med_trigger_dt=np.array([perf[k]["med_trigger_dt"] for k in perf], dtype=np.float64))
    path = os.path.join(HERE, "policy_performance.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(oid)} alerts, {len(junk)} objects, largest {np.bincount(oid).max()}, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
