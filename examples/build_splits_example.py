#!/usr/bin/env python3
"""From labelled base tables to the files ``load_split`` reads: the reference's query_data/train_val_test_split.py on the
device.

Synthetic base tables of four sets (``trues``, ``dims`` with its type table, ``vars``, ``rejects``) are written to
``{dir}/data/base_data``; ``cut_set_and_assign_splits`` labels each set (``split``, ``N``, ``is_rise``, ``near_threshold``,
``is_SN``: one HIP launch per table instead of a pandas pass per object), ``merge_sets_across_split`` merges and shuffles
each split, ``create_subset`` cuts it to ``_N100``; at the end ``btsbot.data.load_split`` loads ``train`` / ``val`` /
``test`` the way ``train_example.py`` and ``run_val`` do.

    python examples/build_splits_example.py [--dir /tmp/btsbot_splits] [--objects 80] [--version v1]
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import btsbot_amd as btsbot  # noqa: E402
from btsbot_amd import splits  # noqa: E402

SETS = ("trues", "dims", "vars", "rejects")
COLS = ["sgscore1", "distpsnr1", "fwhm", "peakmag"]


def base_table(set_index, n_objects, rng, candid0):
    """One set: long-tailed object sizes (a few objects beyond N = 100), rows in shuffled order."""
    sizes = np.minimum((rng.pareto(1.2, n_objects) * 6 + 1).astype(np.int64), 400)
    obj = np.repeat(np.arange(n_objects), sizes)
    n = len(obj)
    letters = ["".join(chr(97 + (k // 26 ** p) % 26) for p in range(6, -1, -1)) for k in range(n_objects)]
    peak = np.round(rng.uniform(17.5, 19.5, n_objects), 1)
    cand = pd.DataFrame({
        "candid": candid0 + rng.permutation(n), "objectId": [f"ZTF2{set_index}{letters[k]}" for k in obj],
        "jd": np.round(2459000.5 + rng.uniform(0, 300, n), 5), "magpsf": np.round(peak[obj] + rng.exponential(0.8, n), 1),
        "peakmag": peak[obj], "label": int(SETS[set_index] in ("trues", "dims")),
        "isdiffpos": rng.choice(["t", "f"], n, p=[0.93, 0.07]), "fid": rng.choice([1, 2, 3], n, p=[0.45, 0.45, 0.1]),
        "sgscore1": np.round(rng.uniform(0, 1, n), 3), "sgscore2": np.round(rng.uniform(0, 1, n), 3),
        "distpsnr1": np.round(rng.uniform(0, 10, n), 2), "fwhm": np.round(rng.uniform(1, 5, n), 2)})
    cand = cand.iloc[rng.permutation(n)].reset_index(drop=True)
    triplets = rng.standard_normal((n, 63, 63, 3)).astype(np.float32)
    triplets[:, 0, 0, 0] = cand["candid"].to_numpy()                     # a row's triplet can be told from its pixels
    return cand, triplets


def main():
    p = argparse.ArgumentParser(description="Build train / val / test split files on the device (MI355X)")
    p.add_argument("--dir", default=None, help="where data/ goes (default: a temporary directory)")
    p.add_argument("--objects", type=int, default=80, help="objects per set")
    p.add_argument("--version", default="v1")
    args = p.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        root = args.dir or tmp
        data_dir = os.path.join(root, "data")
        base = os.path.join(data_dir, "base_data")
        os.makedirs(base, exist_ok=True)
        rng = np.random.default_rng(0)
        candid0 = 1
        for s, name in enumerate(SETS):
            cand, triplets = base_table(s, args.objects, rng, candid0)
            candid0 += len(cand)
            cand.to_csv(os.path.join(base, f"{name}_candidates.csv"), index=False)
            np.save(os.path.join(base, f"{name}_triplets.npy"), triplets)
            if name == "dims":
                ids = pd.unique(cand["objectId"])
                types = rng.choice(["SN Ia", "SN II", "AGN", "CV", "star"], len(ids))
                pd.DataFrame({"ZTFID": ids, "type": types}).to_csv(os.path.join(base, "dims.csv"), index=False)

        for name in SETS:
            written = splits.cut_set_and_assign_splits(name, splits.only_pd_gr_ps, args.version, base,
                                                       non_sn_types=os.path.join(base, "dims.csv"))
            print(f"{name}: rows per split {written}")
        for split in splits.SPLIT_NAMES:
            merged = splits.merge_sets_across_split(SETS, split, args.version, base, data_dir)
            kept = splits.create_subset(split, args.version, data_dir, N_max_p=100)
            print(f"{split}: {merged} rows merged, {kept} in {split}_cand_{args.version}{splits.cuts_suffix(100)}.csv")

        config = {"model_name": "mm_ConvNeXt", "train_data_version": args.version, "N_max": 100, "metadata_cols": COLS}
        objects = {}
        for split in splits.SPLIT_NAMES:
            triplets, metadata, labels, cand = btsbot.data.load_split(root + os.sep, config, split)
            assert (triplets[:, 0, 0, 0].numpy() == cand["candid"].to_numpy().astype(np.float32)).all()
            objects[split] = set(cand["objectId"])
            print(f"load_split({split!r}): triplets {tuple(triplets.shape)}, metadata {tuple(metadata.shape)}, "
                  f"{int(labels.sum())} of {len(labels)} labelled 1, {len(objects[split])} objects, "
                  f"largest N {int(cand['N'].max())}, {int(cand['is_rise'].sum())} rise alerts")
        assert not (objects["train"] & objects["val"]) and not (objects["train"] & objects["test"])
        print("no object is in two splits")


if __name__ == "__main__":
    main()
