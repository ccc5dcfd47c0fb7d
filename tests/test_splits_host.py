"""Building the training splits (reference query_data/train_val_test_split.py), host side: a plain numpy restatement of
what btsbot_split_labels, label_set and subset_mask compute, tied with exact equality to what the reference's own
functions recorded (tests/golden/splits.npz, made by tests/golden/make_splits_golden.py), and the checks of splits.py that
need no device.  tests/test_gpu_splits.py imports the restatement as the kernel's oracle."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "splits.npz")
SPLITS = ("train", "val", "test")
SOURCE_SETS = ("trues", "dims", "vars", "rejects", "junk", "extIas")
NON_SN = ("AGN", "AGN?", "bogus", "bogus?", "duplicate", "nova", "rock", "star", "varstar", "QSO", "CV", "CV?", "CLAGN",
          "Blazar")


def restate_kernel(object_id, jd, magpsf):
    """The six outputs of btsbot_split_labels, object by object.  later ranks the object's alerts by (jd is NaN, jd,
    row); the peak is the lowest row at the minimum non-NaN magpsf, and is_rise is jd <= its jd (all false without
    one)."""
    object_id, jd, magpsf = np.asarray(object_id), np.asarray(jd, dtype=np.float64), np.asarray(magpsf, dtype=np.float64)
    n = len(jd)
    out = dict(pos=np.zeros(n, np.int32), size=np.zeros(n, np.int32), first_row=np.zeros(n, np.int32),
               later=np.zeros(n, np.int32), is_rise=np.zeros(n, bool), peakmag=np.full(n, np.nan))
    for o in np.unique(object_id):
        rows = np.flatnonzero(object_id == o)
        t, m = jd[rows], magpsf[rows]
        out["pos"][rows] = np.arange(len(rows))
        out["size"][rows] = len(rows)
        out["first_row"][rows] = rows[0]
        order = np.lexsort((rows, np.where(np.isnan(t), 0.0, t), np.isnan(t)))      # earliest first
        out["later"][rows[order]] = len(rows) - 1 - np.arange(len(rows))
        if not np.isnan(m).all():
            peak = np.nanmin(m)
            out["peakmag"][rows] = peak
            with np.errstate(invalid="ignore"):
                out["is_rise"][rows] = t <= t[np.flatnonzero(m == peak)[0]]
    return out


def restate_labels(object_id, jd, magpsf, peakmag=None, seed=2, fractions=(0.81, 0.09, 0.10)):
    """label_set: the k-th object in order of first appearance takes draw k of one choice; the alert at position p of an
    object of n alerts takes RandomState(seed).permutation(n)[p] + 1."""
    k = restate_kernel(object_id, jd, magpsf)
    n = len(k["pos"])
    heads = k["first_row"] == np.arange(n)
    rank = (np.cumsum(heads) - 1)[k["first_row"]] if n else np.zeros(0, np.int64)
    draws = np.random.RandomState(seed).choice(3, size=int(heads.sum()), p=list(fractions))
    perms = {s: np.random.RandomState(seed).permutation(int(s)) + 1 for s in np.unique(k["size"])}
    pk = k["peakmag"] if peakmag is None else np.asarray(peakmag, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        near = (pk > 18.4) & (pk < 18.6)
    return dict(split=draws[rank].astype(np.int8), N=np.array([perms[s][p] for s, p in zip(k["size"], k["pos"])], np.int32),
                is_rise=k["is_rise"], near_threshold=near, peakmag=k["peakmag"], object_rank=rank.astype(np.int32))


def restate_subset(split_name, source_set, N, later, N_max_p, N_max_n=0, is_SN=None, near_threshold=None, is_rise=None,
                   sne_only=False, keep_near_threshold=True, rise_only=False):
    """subset_mask, one alert at a time; source_set holds the name of the set of the alert's object."""
    N_max_n = N_max_n or N_max_p
    keep = np.ones(len(N), dtype=bool)
    for i in range(len(N)):
        if N_max_p:
            s = source_set[i]
            if s in ("vars", "junk"):
                keep[i] = later[i] < N_max_n
            elif s not in ("trues", "dims", "rejects"):
                keep[i] = False
            elif split_name == "train":
                keep[i] = N[i] <= (N_max_p if s == "trues" else N_max_n)
        if (sne_only and not is_SN[i]) or (not keep_near_threshold and near_threshold[i]) or (rise_only and not is_rise[i]):
            keep[i] = False
    return keep


def restate_suffix(N_max_p, N_max_n, sne_only, keep_near_threshold, rise_only):
    N_max_n = N_max_n or N_max_p
    s = "" if not N_max_p else f"_N{N_max_p}" if N_max_p == N_max_n else f"_Np{N_max_p}n{N_max_n}"
    return s + "_sne" * bool(sne_only) + "_nnt" * (not keep_near_threshold) + "_rt" * bool(rise_only)


def load_golden():
    return dict(np.load(GOLDEN))


def cut_rows(g, name):
    """The rows of a base table that pass only_pd_gr_ps."""
    col = {c: g[f"{name}_{c}"] for c in ("isdiffpos", "fid", "sgscore1", "sgscore2")}
    return np.flatnonzero((col["isdiffpos"] == "t") & ((col["fid"] == 1) | (col["fid"] == 2))
                          & ((col["sgscore1"] >= 0) | (col["sgscore2"] >= 0)))


def set_table(g, name):
    """(rows passing the cut, integer object ids, jd, magpsf, peakmag) of one base set after its row cut."""
    rows = cut_rows(g, name)
    ids = np.unique(g[f"{name}_objectId"], return_inverse=True)[1].astype(np.int64)
    return (rows, ids[rows]) + tuple(g[f"{name}_{c}"][rows] for c in ("jd", "magpsf", "peakmag"))


def merged_table(g, split):
    """The merged file of one split as the recording orders it: columns of the surviving rows of all sets, concatenated
    in the order of g["sets"] and shuffled by RandomState(2).permutation."""
    cols = {c: [] for c in ("candid", "objectId", "jd", "magpsf", "source_set", "N", "is_SN", "near_threshold", "is_rise")}
    for name in g["sets"]:
        rows = np.flatnonzero(g[f"{name}_ref_split"] == SPLITS.index(split))
        for c in ("candid", "objectId", "jd", "magpsf"):
            cols[c].append(g[f"{name}_{c}"][rows])
        for c in ("N", "is_SN", "near_threshold", "is_rise"):
            cols[c].append(g[f"{name}_ref_{c}"][rows])
        cols["source_set"].append(np.full(len(rows), name))
    cols = {c: np.concatenate(v) for c, v in cols.items()}
    order = np.random.RandomState(2).permutation(len(cols["candid"]))
    cols = {c: v[order] for c, v in cols.items()}
    cols["object_id"] = np.unique(cols["objectId"], return_inverse=True)[1].astype(np.int64)
    return cols


def settings(g):
    return [dict(N_max_p=int(p), N_max_n=int(n), sne_only=bool(s), keep_near_threshold=bool(k), rise_only=bool(r))
            for p, n, s, k, r in g["settings"]]


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def test_fixture_is_not_trivial(golden):
    g = golden
    assert tuple(g["sets"]) == ("trues", "dims", "vars", "rejects", "junk") and tuple(g["splits"]) == SPLITS
    sizes = np.concatenate([np.bincount(set_table(g, s)[1]) for s in g["sets"]])
    assert {1, 2, 3, 63, 64, 65, 1100} <= set(sizes.tolist()) and (sizes == 1).sum() >= 2
    for name in g["sets"]:
        rows, ids, jd, mag, _ = set_table(g, name)
        assert 0 < len(rows) < len(g[f"{name}_candid"])                                  # the row cut drops some rows
        assert all(len(np.unique(jd[ids == k])) == (ids == k).sum() for k in np.unique(ids))   # distinct jd per object
        assert np.isnan(mag).any() and not any(np.isnan(mag[ids == k]).all() for k in np.unique(ids))
        assert set(g[f"{name}_ref_split"].tolist()) == {-1, 0, 1, 2}
    # the minimum repeats, and its lowest row is not its earliest epoch: the tie rule of is_rise decides
    _, ids, jd, mag, _ = set_table(g, "vars")
    big = np.flatnonzero(ids == np.argmax(np.bincount(ids)))
    at_min = big[mag[big] == np.nanmin(mag[big])]
    assert len(big) == 1100 and len(at_min) > 1 and jd[at_min[0]] > jd[at_min].min()
    pk = np.concatenate([g[f"{s}_peakmag"] for s in g["sets"]])
    assert {18.4, 18.5, 18.6} <= set(pk.tolist()) and (pk < 18.4).any() and (pk > 18.6).any()
    assert ((pk > 18.4) & (pk < 18.5)).any() and ((pk > 18.5) & (pk < 18.6)).any()
    candid = np.concatenate([g[f"{s}_candid"] for s in g["sets"]])
    assert len(np.unique(candid)) == len(candid)
    names = [set(g[f"{s}_objectId"].tolist()) for s in g["sets"]]
    assert sum(map(len, names)) == len(set().union(*names))                              # no object in two sets


@pytest.mark.parametrize("name", ["trues", "dims", "vars", "rejects", "junk"])
def test_label_restatement_reproduces_the_reference(golden, name):
    """split, N, is_rise, near_threshold, is_SN and the surviving rows of every base set, as the reference's
    cut_set_and_assign_splits recorded them."""
    g = golden
    rows, ids, jd, mag, peakmag = set_table(g, name)
    lab = restate_labels(ids, jd, mag, peakmag)
    is_sn = np.full(len(rows), name == "trues")
    survive = np.ones(len(rows), dtype=bool)
    if name == "dims":
        sn_ids = g["dims_table_ZTFID"][~np.isin(g["dims_table_type"], NON_SN)]
        is_sn = np.isin(g["dims_objectId"][rows], sn_ids)
        assert is_sn.any() and not is_sn.all()
        survive = peakmag > 18.5
        assert not survive.all()
    ref_split = g[f"{name}_ref_split"]
    assert np.array_equal(np.flatnonzero(ref_split >= 0), rows[survive])
    kept = rows[survive]
    assert np.array_equal(lab["split"][survive], ref_split[kept])
    assert np.array_equal(lab["N"][survive], g[f"{name}_ref_N"][kept])
    assert np.array_equal(lab["is_rise"][survive], g[f"{name}_ref_is_rise"][kept])
    assert np.array_equal(lab["near_threshold"][survive], g[f"{name}_ref_near_threshold"][kept])
    assert np.array_equal(is_sn[survive], g[f"{name}_ref_is_SN"][kept])
    assert lab["is_rise"].any() and not lab["is_rise"].all() and lab["near_threshold"].any()


@pytest.mark.parametrize("split", SPLITS)
def test_subset_restatement_reproduces_the_reference(golden, split):
    """The merged order of every split (the reference's shuffle with the global generator seeded 2) and the candids
    create_subset kept, in file order, for the three recorded settings."""
    g = golden
    m = merged_table(g, split)
    assert np.array_equal(m["candid"], g[f"merged_{split}"])
    k = restate_kernel(m["object_id"], m["jd"], m["magpsf"])
    for i, kw in enumerate(settings(g)):
        keep = restate_subset(split, m["source_set"][k["first_row"]], m["N"], k["later"], is_SN=m["is_SN"],
                              near_threshold=m["near_threshold"], is_rise=m["is_rise"], **kw)
        assert np.array_equal(m["candid"][keep], g[f"kept_{split}_{i}"]), (split, kw)
    assert 0 < len(g[f"kept_{split}_0"]) < len(m["candid"]) and len(g[f"kept_{split}_1"]) != len(g[f"kept_{split}_0"])


def test_cuts_suffix_matches_the_recorded_file_names(golden):
    from btsbot_amd import splits
    want = {f"{s}_cand_vT.csv" for s in SPLITS}
    for kw in settings(golden):
        suffix = splits.cuts_suffix(**kw)
        assert suffix == restate_suffix(**kw)
        want |= {f"{s}_cand_vT{suffix}.csv" for s in SPLITS}
    assert sorted(want) == golden["file_names"].tolist()
    assert splits.cuts_suffix(100) == "_N100" and splits.cuts_suffix(100, 100) == "_N100"
    assert splits.cuts_suffix(100, 50) == "_Np100n50" and splits.cuts_suffix(0, 0, True, False, True) == "_sne_nnt_rt"
    with pytest.raises(ValueError):
        splits.cuts_suffix(-1)


def test_row_cuts_match_the_recording(golden):
    """only_pd_gr_ps of splits.py on the recorded tables: the rows the reference's cut let through."""
    import pandas as pd
    from btsbot_amd import splits
    for name in ("trues", "vars", "rejects", "junk"):
        cand = pd.DataFrame({c: golden[f"{name}_{c}"] for c in ("isdiffpos", "fid", "sgscore1", "sgscore2")})
        mask = splits.only_pd_gr_ps(cand)
        assert np.array_equal(np.flatnonzero(mask), np.flatnonzero(golden[f"{name}_ref_split"] >= 0))
        assert cand["isdiffpos"].dtype == bool                            # rewritten as booleans, as the reference does
        assert np.array_equal(splits.only_pd_gr_ps(cand), mask) and (splits.only_pd_gr(cand) >= mask).all()


def test_splits_have_no_cpu_fallback():
    import btsbot_amd
    from btsbot_amd import _lib, splits
    assert btsbot_amd.label_set is splits.label_set and btsbot_amd.subset_mask is splits.subset_mask
    assert btsbot_amd.SPLIT_NAMES == SPLITS and btsbot_amd.SOURCE_SETS == SOURCE_SETS and splits.NON_SN_TYPES == NON_SN
    assert "btsbot_split_labels" in _lib.SYMBOLS
    z = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        splits.label_set(torch.arange(4), z, z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        splits.split_labels(torch.arange(4), z, z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        splits.subset_mask("train", torch.zeros(4, dtype=torch.int64), torch.ones(4), torch.zeros(4), 5)
    with pytest.raises(ValueError):
        splits.subset_mask("train", torch.zeros(4, dtype=torch.int64), torch.ones(4), torch.zeros(4), -1)
    with pytest.raises(ValueError):
        splits.subset_mask("holdout", torch.zeros(4, dtype=torch.int64), torch.ones(4), torch.zeros(4), 5)
