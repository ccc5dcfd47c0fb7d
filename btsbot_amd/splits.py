"""Labelled alert tables -> the files ``data.load_split`` reads (the reference's query_data/train_val_test_split.py).

    for s in ("trues", "dims", "vars", "rejects"):
        cut_set_and_assign_splits(s, only_pd_gr_ps, "v12", base_dir, non_sn_types=dims_table)
    for split in SPLIT_NAMES:
        merge_sets_across_split(["trues", "dims", "vars", "rejects"], split, "v12", base_dir, data_dir)
        create_subset(split, "v12", data_dir, N_max_p=100)           # -> {split}_cand_v12_N100.csv, ..._triplets_...npy

``cut_set_and_assign_splits`` and ``create_subset`` there loop over the objects of a table and scan the whole table once
per object.  Here what those loops need per alert -- its position in its object, the object's size, first row and
minimum magnitude, how many alerts of the object are later -- comes from one kernel over the whole table
(``btsbot_split_labels``) behind the stable device sort of the object ids that ``alert_features`` uses, and the labels
are gathers:

    lab = label_set(object_id, jd, magpsf, peakmag)      # device tensors -> split, N, is_rise, near_threshold, ...
    keep = subset_mask("train", source_set, lab["N"], split_labels(object_id, jd, magpsf)["later"], N_max_p=100)

The random draws are the reference's own (numpy's legacy generator, ``RandomState(seed)``): ``split`` of the k-th object
in order of first appearance is draw k of one ``choice``; ``N`` of the p-th alert (table order) of an object of n alerts
is ``RandomState(seed).permutation(n)[p] + 1``, so all objects of one size share one permutation.

Two departures from the reference, both where it is not defined: an object whose ``magpsf`` are all NaN has ``is_rise``
false on every alert (there: whatever the last row's ``jd`` gives, under a deprecation warning), and
``merge_sets_across_split`` shuffles with ``RandomState(seed)`` (there the ``seed`` argument is ignored, so the order
depends on the caller's global generator).  Alerts of one object with equal ``jd`` are ordered by input position, as
everywhere in this package.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

from .alert_utils import _check_table, _group_by_object, _launch_grouped, object_keys

SPLIT_NAMES = ("train", "val", "test")                                     # the codes of label_set()["split"]
SOURCE_SETS = ("trues", "dims", "vars", "rejects", "junk", "extIas")       # the codes of subset_mask's source_set
NON_SN_TYPES = ("AGN", "AGN?", "bogus", "bogus?", "duplicate", "nova", "rock", "star", "varstar", "QSO", "CV", "CV?",
                "CLAGN", "Blazar")


def split_labels(object_id: torch.Tensor, jd: torch.Tensor, magpsf: torch.Tensor) -> dict:
    """The outputs of ``btsbot_split_labels`` for a table of n alerts, one row per alert in input order, on the inputs'
    device.  With O(i) the alerts of i's object (object_id: any integers, equal = same object; jd, magpsf as float64):

    pos int32: the alerts of O(i) above row i;  size int32: |O(i)|;  first_row int32: the object's first row;
    later int32: the alerts j of O(i) with (jd[j], j) > (jd[i], i) -- a NaN jd is later than every finite one, NaN jd
    among themselves go by row --, per object a permutation of 0 .. size - 1;  is_rise bool: jd[i] <= the jd of the
    lowest row at the object's minimum non-NaN magpsf (false on an object without one);  peakmag float64: that minimum,
    NaN if none.  No host synchronisation."""
    n = _check_table("splits.split_labels", object_id, jd=jd, magpsf=magpsf)
    dev = object_id.device
    jd, magpsf = (t.to(device=dev, dtype=torch.float64).contiguous() for t in (jd, magpsf))
    i32 = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]
    rise = torch.empty(n, dtype=torch.uint8, device=dev)
    peak = torch.empty(n, dtype=torch.float64, device=dev)
    if n:
        _launch_grouped("btsbot_split_labels", _group_by_object(object_id), n, jd, magpsf, *i32, rise, peak)
    return {"pos": i32[0], "size": i32[1], "first_row": i32[2], "later": i32[3], "is_rise": rise.bool(), "peakmag": peak}


def label_set(object_id: torch.Tensor, jd: torch.Tensor, magpsf: torch.Tensor, peakmag: Optional[torch.Tensor] = None,
              seed: int = 2, fractions: Sequence[float] = (0.81, 0.09, 0.10)) -> dict:
    """The labels ``cut_set_and_assign_splits`` of the reference gives one set's table (train_val_test_split.py:107-140),
    as device tensors [n] in input order:

    split int8 (index into SPLIT_NAMES): draw ``object_rank`` of ``RandomState(seed).choice(3, n_objects, p=fractions)``;
    N int32: ``RandomState(seed).permutation(size)[pos] + 1``;  is_rise bool, peakmag float64 (the object's minimum
    non-NaN magpsf): see ``split_labels``;  near_threshold bool: 18.4 < peakmag < 18.6 on the ``peakmag`` argument (the
    table's column, as the reference reads it) when given, else on the computed one;  object_rank int32: the ordinal of
    the object in order of first appearance.

    One host read: the number of objects and the distinct object sizes, which size the two draws; the permutations of
    the distinct sizes go back as one table and N, split are gathers.  Raises on CPU tensors: there is no CPU path."""
    n = _check_table("splits.label_set", object_id, jd=jd, magpsf=magpsf, peakmag=peakmag)
    fractions = [float(f) for f in fractions]
    if len(fractions) != len(SPLIT_NAMES) or min(fractions) < 0 or abs(sum(fractions) - 1.0) > 1e-8:
        raise ValueError(f"fractions must be {len(SPLIT_NAMES)} non-negative numbers summing to 1, got {fractions}")
    dev = object_id.device
    k = split_labels(object_id, jd, magpsf)
    pk = k["peakmag"] if peakmag is None else peakmag.to(device=dev, dtype=torch.float64)
    out = {"is_rise": k["is_rise"], "near_threshold": (pk > 18.4) & (pk < 18.6), "peakmag": k["peakmag"]}
    if n == 0:
        empty = torch.empty(0, dtype=torch.int32, device=dev)
        return {"split": empty.to(torch.int8), "N": empty, **out, "object_rank": empty.clone()}
    size, first = k["size"].long(), k["first_row"].long()
    heads = first == torch.arange(n, device=dev)
    rank = (torch.cumsum(heads, 0) - 1)[first]
    # the distinct sizes, compacted in ascending order without a sync: d distinct sizes sum to at most n, so d < dmax
    dmax = math.isqrt(2 * n) + 1
    present = torch.zeros(n + 1, dtype=torch.bool, device=dev)
    present[size] = True
    slot = torch.cumsum(present, 0)
    distinct = torch.zeros(dmax + 1, dtype=torch.int64, device=dev)
    distinct.scatter_(0, torch.where(present, slot - 1, dmax), torch.arange(n + 1, device=dev))   # slot dmax: scrap
    host = torch.cat([heads.sum().view(1), slot[-1:], distinct[:dmax]]).cpu().numpy()               # the host read
    n_objects, sizes = int(host[0]), host[2:2 + int(host[1])]
    draws = np.random.RandomState(seed).choice(len(SPLIT_NAMES), size=n_objects, p=fractions).astype(np.int8)
    table = np.concatenate([np.random.RandomState(seed).permutation(int(s)) + 1 for s in sizes]).astype(np.int32)
    starts = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)[:-1]])).to(dev)
    which = torch.searchsorted(torch.from_numpy(np.ascontiguousarray(sizes)).to(dev), size)
    out["N"] = torch.from_numpy(table).to(dev)[starts[which] + k["pos"]]
    out["split"] = torch.from_numpy(draws).to(dev)[rank]
    out["object_rank"] = rank.to(torch.int32)
    return {key: out[key] for key in ("split", "N", "is_rise", "near_threshold", "peakmag", "object_rank")}


def _resolve_n_max(N_max_p: int, N_max_n: int):
    N_max_p, N_max_n = int(N_max_p), int(N_max_n)
    if N_max_p < 0 or N_max_n < 0:
        raise ValueError(f"N_max_p and N_max_n must not be negative, got {N_max_p}, {N_max_n}")
    return N_max_p, (N_max_p if N_max_p and not N_max_n else N_max_n)


def subset_mask(split_name: str, source_set: torch.Tensor, N: torch.Tensor, later: torch.Tensor, N_max_p: int,
                N_max_n: int = 0, is_SN: Optional[torch.Tensor] = None, near_threshold: Optional[torch.Tensor] = None,
                is_rise: Optional[torch.Tensor] = None, sne_only: bool = False, keep_near_threshold: bool = True,
                rise_only: bool = False) -> torch.Tensor:
    """The rows ``create_subset`` of the reference keeps of a merged split table (train_val_test_split.py:208-252), bool
    [n], elementwise on the device.

    source_set: the code (index into SOURCE_SETS) of the alert's OBJECT -- the reference reads it off the object's
    first row; ``create_subset`` here passes ``source_set[first_row]``.  N: the label of ``label_set``, as stored in the
    table.  later: ``split_labels(...)["later"]`` computed over THIS table, the merged split file, not over the base set
    the labels were drawn on: rows of the object may have been cut since (dims), and "the N_max_n latest alerts" counts
    the rows that are left.  With N_max_p > 0 (N_max_n = 0 means N_max_p): in "train", trues keep N <= N_max_p, dims and
    rejects N <= N_max_n; in the other splits these three keep everything; vars and junk keep later < N_max_n in every
    split; any other set is dropped.  N_max_p = 0 keeps everything.  Then the cuts sne_only (is_SN), not
    keep_near_threshold (~near_threshold) and rise_only (is_rise), each needing its column."""
    if split_name not in SPLIT_NAMES:
        raise ValueError(f"split_name must be one of {SPLIT_NAMES}, got {split_name!r}")
    N_max_p, N_max_n = _resolve_n_max(N_max_p, N_max_n)
    if source_set.device.type != "cuda":
        raise RuntimeError("btsbot_amd.splits.subset_mask runs on the GPU; there is no CPU fallback (source_set is on "
                           f"{source_set.device})")
    n = source_set.shape[0]
    cols = {"source_set": source_set, "N": N, "later": later, "is_SN": is_SN, "near_threshold": near_threshold,
            "is_rise": is_rise}
    for name, t in cols.items():
        if t is not None and (t.dim() != 1 or t.shape[0] != n):
            raise ValueError(f"{name} must be [{n}], got {tuple(t.shape)}")
    for name, wanted in (("is_SN", sne_only), ("near_threshold", not keep_near_threshold), ("is_rise", rise_only)):
        if wanted and cols[name] is None:
            raise ValueError(f"this cut needs the column {name}")
    dev = source_set.device
    N, later = N.to(dev), later.to(dev)
    keep = torch.ones(n, dtype=torch.bool, device=dev)
    if N_max_p:
        trues, dims, var, rejects, junk = (source_set == SOURCE_SETS.index(s)
                                           for s in ("trues", "dims", "vars", "rejects", "junk"))
        if split_name == "train":
            keep = (trues & (N <= N_max_p)) | ((dims | rejects) & (N <= N_max_n))
        else:
            keep = trues | dims | rejects
        keep = keep | ((var | junk) & (later < N_max_n))
    if sne_only:
        keep = keep & is_SN.to(dev).bool()
    if not keep_near_threshold:
        keep = keep & ~near_threshold.to(dev).bool()
    if rise_only:
        keep = keep & is_rise.to(dev).bool()
    return keep


def cuts_suffix(N_max_p: int, N_max_n: int = 0, sne_only: bool = False, keep_near_threshold: bool = True,
                rise_only: bool = False) -> str:
    """The suffix ``create_subset`` puts after the version in its file names (create_cuts_str of the reference, after
    its N_max_n = 0 -> N_max_p): "_N100", "_Np100n50", then "_sne", "_nnt", "_rt"."""
    N_max_p, N_max_n = _resolve_n_max(N_max_p, N_max_n)
    s = ""
    if N_max_p:
        s += f"_N{N_max_p}" if N_max_p == N_max_n else f"_Np{N_max_p}n{N_max_n}"
    return s + ("_sne" if sne_only else "") + ("" if keep_near_threshold else "_nnt") + ("_rt" if rise_only else "")


# ---- the file drivers ------------------------------------------------------------------------------------------------
def _is_diffpos(cand):
    col = cand["isdiffpos"]
    if col.dtype != bool:
        cand["isdiffpos"] = col = (col == "t") | (col == True)     # noqa: E712  (the reference rewrites the column too)
    return col.to_numpy(dtype=bool)


def only_pd_gr(cand) -> np.ndarray:
    """Row cut: positive differences in g or r (isdiffpos is 't', fid 1 or 2).  Rewrites ``isdiffpos`` as booleans."""
    fid = cand["fid"].to_numpy()
    return _is_diffpos(cand) & ((fid == 1) | (fid == 2))


def only_pd_gr_ps(cand) -> np.ndarray:
    """``only_pd_gr`` and a PS1 match: sgscore1 >= 0 or sgscore2 >= 0."""
    return only_pd_gr(cand) & ((cand["sgscore1"].to_numpy() >= 0) | (cand["sgscore2"].to_numpy() >= 0))


def _device_columns(cand, device, *names):
    ids = torch.from_numpy(object_keys(cand["objectId"].tolist())).to(device)
    return (ids,) + tuple(torch.from_numpy(cand[c].to_numpy(dtype=np.float64)).to(device) for c in names)


def _write(trips, cand, rows, trip_path, cand_path):
    np.save(trip_path, trips[rows])
    cand.iloc[rows].to_csv(cand_path, index=False)


def cut_set_and_assign_splits(set_name: str, cuts, version_name: str, base_dir: str, seed: int = 2, non_sn_types=None,
                              fractions: Sequence[float] = (0.81, 0.09, 0.10), device="cuda") -> dict:
    """``{base_dir}/{set_name}_triplets.npy`` + ``{set_name}_candidates.csv`` (columns objectId, jd, magpsf, peakmag and
    whatever else travels along) -> per split ``{set_name}_{split}_triplets_{version_name}.npy`` and
    ``{set_name}_{split}_cand_{version_name}.csv`` with the columns source_set, N, split, is_SN, near_threshold, is_rise
    added (``label_set`` on ``device``).  Returns the number of rows written per split.

    cuts: None, a bool row mask, or a callable ``cand -> mask`` (``only_pd_gr``, ``only_pd_gr_ps``), applied first.
    is_SN is true for the sets trues and extIas.  For dims it is true for the objects that ``non_sn_types`` (required
    then: a table, or the path of a csv, with the columns ZTFID and type) does not list under one of NON_SN_TYPES, and
    the rows with peakmag <= 18.5 are dropped after the draws, so the dropped objects still took theirs."""
    import pandas as pd
    if set_name not in SOURCE_SETS:
        raise ValueError(f"set_name must be one of {SOURCE_SETS}, got {set_name!r}")
    if set_name == "dims" and non_sn_types is None:
        raise ValueError("the set dims needs non_sn_types: a table (or csv path) with the columns ZTFID and type")
    trips = np.load(os.path.join(base_dir, f"{set_name}_triplets.npy"), mmap_mode="r")
    cand = pd.read_csv(os.path.join(base_dir, f"{set_name}_candidates.csv"), index_col=False)
    if len(trips) != len(cand):
        raise ValueError(f"{set_name}: {len(trips)} triplets for {len(cand)} candidates")
    rows = np.arange(len(cand))
    if cuts is not None:
        mask = np.asarray(cuts(cand) if callable(cuts) else cuts, dtype=bool)
        if mask.shape != (len(cand),):
            raise ValueError(f"cuts must give one bool per row, got shape {mask.shape}")
        rows = rows[mask]
        cand = cand.iloc[rows].reset_index(drop=True)
    lab = label_set(*_device_columns(cand, device, "jd", "magpsf", "peakmag"), seed=seed, fractions=fractions)
    lab = {k: lab[k].cpu().numpy() for k in ("split", "N", "is_rise", "near_threshold")}
    cand["source_set"] = set_name
    cand["N"] = lab["N"]
    cand["split"] = np.array(SPLIT_NAMES, dtype=object)[lab["split"]]
    cand["is_SN"] = set_name in ("trues", "extIas")
    cand["near_threshold"] = lab["near_threshold"]
    cand["is_rise"] = lab["is_rise"]
    keep = np.ones(len(cand), dtype=bool)
    if set_name == "dims":
        table = pd.read_csv(non_sn_types) if isinstance(non_sn_types, (str, os.PathLike)) else non_sn_types
        sn_ids = table.loc[~table["type"].isin(NON_SN_TYPES), "ZTFID"].to_numpy()
        cand["is_SN"] = cand["objectId"].isin(sn_ids)
        keep = (cand["peakmag"] > 18.5).to_numpy()
    written = {}
    for code, split in enumerate(SPLIT_NAMES):
        sel = np.flatnonzero(keep & (lab["split"] == code))
        np.save(os.path.join(base_dir, f"{set_name}_{split}_triplets_{version_name}.npy"), trips[rows[sel]])
        cand.iloc[sel].to_csv(os.path.join(base_dir, f"{set_name}_{split}_cand_{version_name}.csv"), index=False)
        written[split] = len(sel)
    return written


def merge_sets_across_split(set_names: Sequence[str], split_name: str, version_name: str, base_dir: str, data_dir: str,
                            seed: int = 2) -> int:
    """The ``{set}_{split_name}_*_{version_name}`` files of ``set_names`` in ``base_dir``, concatenated in that order
    and shuffled by ``RandomState(seed).permutation``, -> ``{data_dir}/{split_name}_triplets_{version_name}.npy`` and
    ``{split_name}_cand_{version_name}.csv``.  Returns the number of rows.  Deterministic in ``seed`` -- the one place
    where the reference is not: it ignores its own seed argument and draws from the global generator (seeded with
    ``seed`` just before the call, it gives this order)."""
    import pandas as pd
    frames = [pd.read_csv(os.path.join(base_dir, f"{s}_{split_name}_cand_{version_name}.csv"), index_col=False)
              for s in set_names]
    cand = pd.concat([f for f in frames if len(f)] or frames[:1]).reset_index(drop=True)   # (a set may have no row here)
    trips = np.concatenate([np.load(os.path.join(base_dir, f"{s}_{split_name}_triplets_{version_name}.npy"),
                                    mmap_mode="r") for s in set_names], axis=0)
    order = np.random.RandomState(seed).permutation(len(cand))
    _write(trips, cand, order, os.path.join(data_dir, f"{split_name}_triplets_{version_name}.npy"),
           os.path.join(data_dir, f"{split_name}_cand_{version_name}.csv"))
    return len(order)


def create_subset(split_name: str, version_name: str, data_dir: str, N_max_p: int, N_max_n: int = 0,
                  sne_only: bool = False, keep_near_threshold: bool = True, rise_only: bool = False,
                  device="cuda") -> int:
    """The merged ``{split_name}_*_{version_name}`` files of ``data_dir`` -> the same with ``cuts_suffix(...)`` after
    the version, holding the rows of ``subset_mask`` in file order.  ``later`` and each object's source set (that of its
    first row) are taken over the merged table, on ``device``.  Returns the number of rows kept; missing parent files
    raise FileNotFoundError."""
    import pandas as pd
    suffix = cuts_suffix(N_max_p, N_max_n, sne_only, keep_near_threshold, rise_only)
    stem = os.path.join(data_dir, f"{split_name}_")
    trips = np.load(f"{stem}triplets_{version_name}.npy", mmap_mode="r")
    cand = pd.read_csv(f"{stem}cand_{version_name}.csv", index_col=False)
    unknown = set(cand["source_set"]) - set(SOURCE_SETS)
    if unknown:
        raise ValueError(f"unknown source_set {sorted(unknown)}")
    k = split_labels(*_device_columns(cand, device, "jd", "magpsf"))
    codes = torch.from_numpy(cand["source_set"].map(SOURCE_SETS.index).to_numpy(dtype=np.int64)).to(device)

    def col(name):
        return torch.from_numpy(cand[name].to_numpy(dtype=bool)).to(device)

    keep = subset_mask(split_name, codes[k["first_row"].long()], torch.from_numpy(cand["N"].to_numpy(np.int64)).to(device),
                       k["later"], N_max_p, N_max_n, is_SN=col("is_SN") if sne_only else None,
                       near_threshold=None if keep_near_threshold else col("near_threshold"),
                       is_rise=col("is_rise") if rise_only else None, sne_only=sne_only,
                       keep_near_threshold=keep_near_threshold, rise_only=rise_only)
    rows = np.flatnonzero(keep.cpu().numpy())
    _write(trips, cand, rows, f"{stem}triplets_{version_name}{suffix}.npy", f"{stem}cand_{version_name}{suffix}.csv")
    return len(rows)


def subsample_data(split: str, version: str, data_dir: str, perc_to_keep: float = 10, random_seed: int = 2,
                   suffix: str = "_N100") -> int:
    """Keep ``int(n_objects * perc_to_keep / 100)`` objects of ``{split}_*_{version}{suffix}``, drawn without
    replacement by ``RandomState(random_seed)`` from the objects in order of first appearance, with all their rows in
    file order -> ``{split}_*_{version}s{perc_to_keep}{suffix}``.  Returns the number of rows kept."""
    import pandas as pd
    stem = os.path.join(data_dir, f"{split}_")
    trips = np.load(f"{stem}triplets_{version}{suffix}.npy", mmap_mode="r")
    cand = pd.read_csv(f"{stem}cand_{version}{suffix}.csv", index_col=False)
    objs = pd.unique(cand["objectId"])
    kept = np.random.RandomState(random_seed).choice(objs, size=int(len(objs) * perc_to_keep / 100), replace=False)
    rows = np.flatnonzero(cand["objectId"].isin(kept).to_numpy())
    _write(trips, cand, rows, f"{stem}triplets_{version}s{perc_to_keep}{suffix}.npy",
           f"{stem}cand_{version}s{perc_to_keep}{suffix}.csv")
    return len(rows)
