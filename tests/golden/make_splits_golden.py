"""Generate tests/golden/splits.npz: seeded synthetic base tables of five sets and what the REFERENCE'S OWN
query_data/train_val_test_split.py makes of them -- the labels of cut_set_and_assign_splits per set, the merged order per
split, and the rows create_subset keeps for three settings.  Runs only where a checkout of the reference and pandas are
at hand:

    python tests/golden/make_splits_golden.py /path/to/reference/btsbot

The reference file is imported by path and run in a temporary directory laid out as it expects: ``data/base_data/`` with
the base tables, and a working directory beside ``data/`` (it reads and writes ``../data/...``).  The global numpy
generator is seeded with 2 before each merge_sets_across_split, whose own seed argument the reference ignores.

Tables: sets trues, dims (with its type table), vars, rejects, junk; 41 to 60 objects each, rows in shuffled
order; object sizes (after the row cut) include 1, 1, 2, 3, 63, 64, 65 and one of 1,100; jd distinct inside an object on
a 1e-5 day grid; magpsf on a 0.1 mag grid, so minima repeat at several rows, some NaN but never a whole object; peakmag
(one value per object) on both sides of and exactly at 18.4, 18.5, 18.6; some rows fail the row cut only_pd_gr_ps; a
unique candid per row.  Every input column is recorded as pandas reads it back from the csv, the way the reference saw
it.  The npz holds arrays of numbers and names only.
"""
import contextlib
import importlib.util
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SETS = ("trues", "dims", "vars", "rejects", "junk")
SPLITS = ("train", "val", "test")
VERSION = "vT"
# (N_max_p, N_max_n, sne_only, keep_near_threshold, rise_only)
SETTINGS = ((5, 3, False, True, False), (4, 0, False, True, False), (5, 3, True, False, True))
SIZES = {"trues": [1, 1, 2, 3, 63, 64, 65], "dims": [64, 1, 7, 7], "vars": [1100, 1, 2, 65, 4], "rejects": [63, 5, 5, 2],
         "junk": [3, 1, 6, 12]}
# objects per set: with seed 2 every set takes the same draws, and the first "test" among them is draw 40
N_OBJECTS = {"trues": 44, "dims": 60, "vars": 50, "rejects": 41, "junk": 42}
PEAKMAGS = (18.0, 18.3, 18.4, 18.45, 18.5, 18.55, 18.6, 18.7, 19.2)
TYPES = ("SN Ia", "AGN", None, "CV?", "SN II", "star", "bogus", "SN Ib")
INPUTS = ("candid", "objectId", "jd", "magpsf", "peakmag", "isdiffpos", "fid", "sgscore1", "sgscore2")
LABELS = ("N", "is_rise", "near_threshold", "is_SN")


def _name(set_index, k):
    letters = "".join(chr(ord("a") + (k // 26 ** p) % 26) for p in range(6, -1, -1))
    return f"ZTF2{set_index}{letters}"


def synthetic_set(pd, set_index, rng, candid0):
    sizes = list(SIZES[SETS[set_index]])
    sizes += [int(x) for x in rng.integers(1, 17, N_OBJECTS[SETS[set_index]] - len(sizes))]
    rows = []
    for k, n in enumerate(sizes):
        extra = int(rng.binomial(n, 0.08)) + (k % 5 == 0)              # rows that fail the row cut
        ticks = rng.choice(40_000_000, n + extra, replace=False)
        jd = np.round(2459000.5 + ticks * 1e-5, 5)
        assert len(np.unique(jd)) == n + extra
        mag = np.round(19.0 + 1.2 * np.cos(np.linspace(0, 5, n + extra) + rng.uniform(0, 3)) + rng.normal(0, 0.2, n + extra), 1)
        mag = np.maximum(mag, 17.9)                                     # a floor: the minimum repeats
        mag[rng.random(n + extra) < 0.12] = np.nan
        fails = np.zeros(n + extra, dtype=bool)
        fails[rng.choice(n + extra, extra, replace=False)] = True
        if np.isnan(mag[~fails]).all():
            mag[np.flatnonzero(~fails)[0]] = 19.3
        peakmag = PEAKMAGS[(k + set_index) % len(PEAKMAGS)]
        for i in range(n + extra):
            how = int(rng.integers(3)) if fails[i] else -1              # 0: negative difference, 1: i band, 2: no PS1 match
            rows.append({"passes": not fails[i], "size": n, "objectId": _name(set_index, 37 * k + 5), "jd": jd[i], "magpsf": mag[i], "peakmag": peakmag,
                         "isdiffpos": "f" if how == 0 else "t", "fid": 3 if how == 1 else int(rng.integers(1, 3)),
                         "sgscore1": -999.0 if how == 2 else float(np.round(rng.uniform(0, 1), 3)),
                         "sgscore2": -999.0 if how == 2 or rng.random() < 0.3 else float(np.round(rng.uniform(0, 1), 3))})
    # shuffled table order, drawn again until the val and the test draws of seed 2 each fall on an object of more than
    # five alerts (objects that appear late are mostly small, and a split of small objects has nothing to cut)
    while True:
        order = rng.permutation(len(rows))
        first = {}
        for i in order:
            if rows[i]["passes"]:
                first.setdefault(rows[i]["objectId"], (len(first), rows[i]["size"]))
        draws = np.random.RandomState(2).choice(3, size=len(first), p=[0.81, 0.09, 0.10])
        if all(any(draws[r] == c and n > 5 for r, n in first.values()) for c in (1, 2)):
            break
    cand = pd.DataFrame([rows[i] for i in order]).drop(columns=["passes", "size"])
    cand.insert(0, "candid", candid0 + rng.permutation(len(cand)))
    return cand, sizes


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import pandas as pd
    spec = importlib.util.spec_from_file_location("reference_splits",
                                                  os.path.join(sys.argv[1], "query_data", "train_val_test_split.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(20240611)
    out = {"sets": np.array(SETS), "splits": np.array(SPLITS), "settings": np.array(SETTINGS, dtype=np.int64)}
    home = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        base, data, work = os.path.join(tmp, "data", "base_data"), os.path.join(tmp, "data"), os.path.join(tmp, "work")
        os.makedirs(base)
        os.makedirs(work)
        candid0 = 1000
        for s, name in enumerate(SETS):
            cand, sizes = synthetic_set(pd, s, rng, candid0)
            candid0 += len(cand)
            cand.to_csv(os.path.join(base, f"{name}_candidates.csv"), index=False)
            trips = np.broadcast_to(cand["candid"].to_numpy(np.float64)[:, None, None, None], (len(cand), 2, 2, 3))
            np.save(os.path.join(base, f"{name}_triplets.npy"), np.ascontiguousarray(trips))
            if name == "dims":
                ids = pd.unique(cand["objectId"])
                table = pd.DataFrame({"ZTFID": ids, "type": [TYPES[i % len(TYPES)] for i in range(len(ids))]})
                table.to_csv(os.path.join(base, "dims.csv"), index=False)
                table = pd.read_csv(os.path.join(base, "dims.csv"))
                out["dims_table_ZTFID"] = table["ZTFID"].to_numpy().astype(str)
                out["dims_table_type"] = table["type"].fillna("").to_numpy().astype(str)      # "" = unclassified
        os.chdir(work)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                for name in SETS:
                    ref.cut_set_and_assign_splits(name, ref.only_pd_gr_ps, version_name=VERSION)
                for split in SPLITS:
                    np.random.seed(2)
                    ref.merge_sets_across_split(list(SETS), split, VERSION)
                for p, n, sne, knt, rise in SETTINGS:
                    for split in SPLITS:
                        ref.create_subset(split, VERSION, N_max_p=p, N_max_n=n, sne_only=sne, keep_near_threshold=knt,
                                          rise_only=rise)
        finally:
            os.chdir(home)

        for name in SETS:
            cand = pd.read_csv(os.path.join(base, f"{name}_candidates.csv"), index_col=False)   # as the reference read it
            for c in INPUTS:
                col = cand[c].to_numpy()
                out[f"{name}_{c}"] = col.astype(str) if col.dtype == object else col
            row_of = {c: i for i, c in enumerate(cand["candid"].tolist())}
            n = len(cand)
            rec = {"split": np.full(n, -1, dtype=np.int8), "N": np.zeros(n, dtype=np.int32),
                   **{c: np.zeros(n, dtype=bool) for c in LABELS[1:]}}
            for code, split in enumerate(SPLITS):
                part = pd.read_csv(os.path.join(base, f"{name}_{split}_cand_{VERSION}.csv"), index_col=False)
                assert (part["split"] == split).all() and (part["source_set"] == name).all()
                trips = np.load(os.path.join(base, f"{name}_{split}_triplets_{VERSION}.npy"))
                assert np.array_equal(trips[:, 0, 0, 0], part["candid"].to_numpy(np.float64))
                rows = np.array([row_of[c] for c in part["candid"].tolist()], dtype=np.int64)
                assert np.all(np.diff(rows) > 0)                          # table order survives
                rec["split"][rows] = code
                for c in LABELS:
                    rec[c][rows] = part[c].to_numpy()
            for c, v in rec.items():
                out[f"{name}_ref_{c}"] = v                                # split -1: the row did not survive
        for split in SPLITS:
            merged = pd.read_csv(os.path.join(data, f"{split}_cand_{VERSION}.csv"), index_col=False)
            out[f"merged_{split}"] = merged["candid"].to_numpy(np.int64)
            for i, (p, n, sne, knt, rise) in enumerate(SETTINGS):
                suffix = ref.create_cuts_str(p, n if n else p, sne, knt, rise)
                kept = pd.read_csv(os.path.join(data, f"{split}_cand_{VERSION}{suffix}.csv"), index_col=False)
                trips = np.load(os.path.join(data, f"{split}_triplets_{VERSION}{suffix}.npy"))
                assert np.array_equal(trips[:, 0, 0, 0], kept["candid"].to_numpy(np.float64))
                out[f"kept_{split}_{i}"] = kept["candid"].to_numpy(np.int64)
        out["file_names"] = np.array(sorted(f for f in os.listdir(data) if f.endswith(".csv")))
    path = os.path.join(HERE, "splits.npz")
    np.savez_compressed(path, **out)
    total = sum(len(out[f"{s}_candid"]) for s in SETS)
    print(f"{path}: {total} rows in {len(SETS)} sets; kept per setting and split: "
          + ", ".join(str(len(out[f'kept_{sp}_{i}'])) for i in range(len(SETTINGS)) for sp in SPLITS))


if __name__ == "__main__":
    main()
