"""Generate tests/golden/alert_features.npz: seeded synthetic alert packets and the eight custom metadata columns the
REFERENCE'S OWN prep_alerts (btsbot/alert_utils.py:333-441) computes for them.  Runs only where a checkout of the
reference, pandas and tqdm are at hand:

    python tests/golden/make_alert_features_golden.py /path/to/reference/btsbot

The reference module is imported by path.  Its astropy import is only used by make_triplet, so an empty stand-in
module takes its place; without Kowalski credentials its non-detection query returns NaN without touching the network.

Packets: a few hundred alerts of a few dozen objects in shuffled order; jd distinct inside an object (the reference
sorts with an unstable sort, so ties would not be defined), near 2459000 with spacings down to 1e-4 day; jdstarthist
before, at and after the first detection; magpsf on a 0.01 mag grid, so minima repeat at several epochs.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
COLS = ["peakmag", "maxmag", "peakmag_so_far", "maxmag_so_far", "age", "days_since_peak", "days_to_peak", "nnotdet"]


def load_reference(ref_dir):
    for name in ("astropy", "astropy.io", "astropy.io.fits"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["astropy"].io = sys.modules["astropy.io"]
    sys.modules["astropy.io"].fits = sys.modules["astropy.io.fits"]
    for var in ("KOWALSKI_USER", "KOWALSKI_PASS"):
        os.environ.pop(var, None)
    spec = importlib.util.spec_from_file_location("reference_alert_utils", os.path.join(ref_dir, "alert_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synthetic_packets(seed=20240607, n_objects=36):
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([[1, 1, 2, 3], rng.integers(2, 12, n_objects - 8), [20, 33, 47, 71]])
    alerts = []
    for k, n in enumerate(sizes):
        t0 = 2459000.5 + float(rng.uniform(0, 400))
        # nightly-to-weekly gaps, with runs of same-night alerts 1e-4 .. 1e-3 day apart
        gaps = np.where(rng.random(n) < 0.35, rng.uniform(1e-4, 1e-3, n), rng.uniform(0.02, 6.0, n))
        jd = t0 + np.cumsum(gaps)
        assert len(np.unique(jd)) == n
        mag = np.round(19.0 + 1.5 * np.cos(np.linspace(0, 3, n) + rng.uniform(0, 3)) + rng.normal(0, 0.15, n), 2)
        side = k % 3     # jdstarthist before / exactly at / after the first detection of the batch
        for i in range(n):
            start = jd.min() + (-float(rng.uniform(0.5, 30)), 0.0, float(rng.uniform(0.001, 2.0)))[side]
            ndet = int(rng.integers(1, 60))
            alerts.append({"objectId": f"ZTF21{k:07d}", "candid": int(rng.integers(1 << 40)),
                           "candidate": {"jd": float(jd[i]), "magpsf": float(mag[i]), "jdstarthist": float(start),
                                         "ndethist": ndet, "ncovhist": ndet + int(rng.integers(0, 900))},
                           "classifications": {}})
    order = rng.permutation(len(alerts))
    return [alerts[i] for i in order]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    alerts = synthetic_packets()
    df = ref.prep_alerts(alerts, 0, np.zeros(len(alerts)))
    names = sorted({a["objectId"] for a in alerts})
    cand = [a["candidate"] for a in alerts]
    out = dict(
        object_id=np.array([names.index(a["objectId"]) for a in alerts], dtype=np.int64),
        jd=np.array([c["jd"] for c in cand], dtype=np.float64),
        magpsf=np.array([c["magpsf"] for c in cand], dtype=np.float64),
        jdstarthist=np.array([c["jdstarthist"] for c in cand], dtype=np.float64),
        ncovhist=np.array([c["ncovhist"] for c in cand], dtype=np.int32),
        ndethist=np.array([c["ndethist"] for c in cand], dtype=np.int32),
        columns=np.array(COLS),
        reference=df[COLS].to_numpy().astype(np.float64),
    )
    assert np.isfinite(out["reference"]).all()
    path = os.path.join(HERE, "alert_features.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(alerts)} alerts, {len(names)} objects, largest {np.bincount(out['object_id']).max()}")


if __name__ == "__main__":
    main()
