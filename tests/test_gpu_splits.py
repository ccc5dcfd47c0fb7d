"""btsbot_split_labels, label_set, subset_mask and the file drivers of splits.py on the device, against the numpy
restatement of tests/test_splits_host.py (which that file ties to the reference's recorded output) and against the
recording itself.  Every output is a selection or a count, so every comparison is exact, NaN positions included."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_splits_host import (SOURCE_SETS, SPLITS, load_golden, merged_table, restate_kernel, restate_labels,
                              restate_subset, set_table, settings)

pytestmark = pytest.mark.gpu

KERNEL_OUT = ("pos", "size", "first_row", "later", "is_rise", "peakmag")
LABEL_OUT = ("split", "N", "is_rise", "near_threshold", "peakmag", "object_rank")
DTYPES = dict(pos=torch.int32, size=torch.int32, first_row=torch.int32, later=torch.int32, is_rise=torch.bool,
              peakmag=torch.float64, split=torch.int8, N=torch.int32, near_threshold=torch.bool, object_rank=torch.int32)


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def _dev(cuda, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays)


def _same(got, want, keys, what=""):
    for k in keys:
        g = got[k]
        assert g.dtype == DTYPES[k] and g.device.type == "cuda" and tuple(g.shape) == want[k].shape, (what, k)
        g = g.cpu().numpy()
        bad = np.flatnonzero(~((g == want[k]) | ((g != g) & (want[k] != want[k]))))
        assert bad.size == 0, f"{what}{k}: {bad.size} rows differ, first row {bad[0]}: got {g[bad[0]]}, want {want[k][bad[0]]}"


def _check_kernel(cuda, ids, jd, mag):
    from btsbot_amd import splits
    got = splits.split_labels(*_dev(cuda, ids, jd, mag))
    _same(got, restate_kernel(ids, jd, mag), KERNEL_OUT)
    return {k: v.cpu().numpy() for k, v in got.items()}


def _table(sizes, seed, nan_mag=0.1):
    """One shuffled table with an object of every given size: jd on a grid that repeats inside large objects, magpsf on
    a 0.1 grid with a floor (the minimum repeats), some NaN."""
    rng = np.random.default_rng(seed)
    ids = np.concatenate([np.full(n, 1000 + 7 * k) for k, n in enumerate(sizes)]).astype(np.int64)
    n = len(ids)
    jd = 2459000.5 + rng.integers(0, 4000, n) * 0.25
    mag = np.maximum(np.round(19 + rng.normal(0, 0.8, n), 1), 18.2)
    mag[rng.random(n) < nan_mag] = np.nan
    order = rng.permutation(n)
    return ids[order], jd[order], mag[order]


# ---- the recording -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["trues", "dims", "vars", "rejects", "junk"])
def test_golden_label_set(cuda, golden, name):
    """label_set over every recorded base set after its row cut: the restatement's six outputs, and split, N, is_rise,
    near_threshold as the reference wrote them for the rows that survive."""
    from btsbot_amd import splits
    rows, ids, jd, mag, peakmag = set_table(golden, name)
    got = splits.label_set(*_dev(cuda, ids, jd, mag, peakmag))
    assert tuple(got) == LABEL_OUT
    _same(got, restate_labels(ids, jd, mag, peakmag), LABEL_OUT, name + " ")
    ref_split = golden[f"{name}_ref_split"][rows]
    live = ref_split >= 0                                                  # (dims: the bright rows were dropped later)
    assert live.any() and np.array_equal(got["split"].cpu().numpy()[live], ref_split[live])
    for k in ("N", "is_rise", "near_threshold"):
        assert np.array_equal(got[k].cpu().numpy()[live], golden[f"{name}_ref_{k}"][rows][live]), k


@pytest.mark.parametrize("split", SPLITS)
def test_golden_subset_mask(cuda, golden, split):
    """subset_mask over the merged table of every split, later and the object's set taken over that table on the device:
    the candids the reference's create_subset kept, in file order, for the three recorded settings."""
    from btsbot_amd import splits
    assert splits.SOURCE_SETS == SOURCE_SETS
    m = merged_table(golden, split)
    k = splits.split_labels(*_dev(cuda, m["object_id"], m["jd"], m["magpsf"]))
    codes, n_label, is_sn, near, rise = _dev(cuda, np.array([SOURCE_SETS.index(s) for s in m["source_set"]]), m["N"],
                                             m["is_SN"], m["near_threshold"], m["is_rise"])
    for i, kw in enumerate(settings(golden)):
        keep = splits.subset_mask(split, codes[k["first_row"].long()], n_label, k["later"], is_SN=is_sn,
                                  near_threshold=near, is_rise=rise, **kw)
        assert keep.dtype == torch.bool and keep.device.type == "cuda"
        assert np.array_equal(m["candid"][keep.cpu().numpy()], golden[f"kept_{split}_{i}"]), kw
    # N_max_p = 0: no cut by N; an unknown set (extIas) is dropped once there is one
    assert bool(splits.subset_mask(split, codes, n_label, k["later"], 0).all())
    assert not bool(splits.subset_mask(split, torch.full_like(codes, SOURCE_SETS.index("extIas")), n_label, k["later"], 5).any())


# ---- the kernel's forms and boundaries ---------------------------------------------------------------------------------
BOUNDARY_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1280, 2500]


@pytest.fixture(scope="module")
def boundary_table():
    return _table(BOUNDARY_SIZES, seed=21)


def test_size_boundaries(cuda, boundary_table):
    """One object at every size where the kernel changes form (one wave up to 64, the LDS tile up to 1024, streamed in
    batches of 256 above) or a batch ends, interleaved in one shuffled table: the raw outputs equal the restatement, and
    per object later + 1 and N are permutations of 1 .. size."""
    from btsbot_amd import splits
    from btsbot_amd.alert_utils import FEATURE_TILE
    assert FEATURE_TILE == 1024
    ids, jd, mag = boundary_table
    got = _check_kernel(cuda, ids, jd, mag)
    lab = splits.label_set(*_dev(cuda, ids, jd, mag))
    _same(lab, restate_labels(ids, jd, mag), LABEL_OUT)
    n_label, split = lab["N"].cpu().numpy(), lab["split"].cpu().numpy()
    assert sorted(np.bincount(ids)[np.unique(ids)].tolist()) == BOUNDARY_SIZES
    for o in np.unique(ids):
        rows = np.flatnonzero(ids == o)
        want = np.arange(1, len(rows) + 1)
        assert np.array_equal(np.sort(n_label[rows]), want) and np.array_equal(np.sort(got["later"][rows] + 1), want)
        assert np.array_equal(got["pos"][rows], want - 1) and (split[rows] == split[rows[0]]).all()
    big = ids == ids[np.argmax(got["size"])]
    assert big.sum() == 2500 and len(np.unique(jd[big])) < 2500                   # jd repeats: later fell back on position


def test_one_object_and_empty_table(cuda):
    from btsbot_amd import splits
    ids, jd, mag = _table([300], seed=4)
    got = _check_kernel(cuda, ids, jd, mag)
    assert (got["size"] == 300).all() and (got["first_row"] == 0).all()
    lab = splits.label_set(*_dev(cuda, ids, jd, mag))
    _same(lab, restate_labels(ids, jd, mag), LABEL_OUT)
    assert (lab["object_rank"] == 0).all() and len(set(lab["split"].tolist())) == 1
    e = torch.zeros(0, device=cuda)
    k = splits.split_labels(e.long(), e.double(), e.double())
    lab = splits.label_set(e.long(), e.double(), e.double())
    for out, keys in ((k, KERNEL_OUT), (lab, LABEL_OUT)):
        assert tuple(out) == keys
        for key in keys:
            assert tuple(out[key].shape) == (0,) and out[key].dtype == DTYPES[key] and out[key].device.type == "cuda"
    assert tuple(splits.subset_mask("val", e.long(), e.int(), e.int(), 5).shape) == (0,)


def test_ties_and_nan(cuda):
    """The tie rules, on one small object and again inside objects of the LDS forms."""
    t, nan = 2459010.5, np.nan
    one = lambda jd, mag: (np.full(len(jd), 5, dtype=np.int64), np.array(jd, dtype=np.float64), np.array(mag, dtype=np.float64))
    # the minimum 17.5 at rows 1 and 3; row 1 is the lowest row but the LATER epoch: jd_peak = t + 4, not t + 1
    got = _check_kernel(cuda, *one([t + 2, t + 4, t + 0, t + 1, t + 5], [18.0, 17.5, 18.0, 17.5, 19.0]))
    assert got["is_rise"].tolist() == [True, True, True, True, False] and (got["peakmag"] == 17.5).all()
    # equal jd: later follows input position (rows 0, 1, 3 share t + 2: row 3 is the latest of them)
    got = _check_kernel(cuda, *one([t + 2, t + 2, t + 0, t + 2, t + 9], [18.0, 17.5, 18.0, 17.5, 19.0]))
    assert got["later"].tolist() == [3, 2, 4, 1, 0] and got["is_rise"].tolist() == [True, True, True, True, False]
    # NaN magpsf rows are skipped by the minimum, wherever they lie
    got = _check_kernel(cuda, *one([t + 3, t + 1, t + 2, t + 0], [nan, 18.5, 18.0, nan]))
    assert got["is_rise"].tolist() == [False, True, True, True] and (got["peakmag"] == 18.0).all()
    # only NaN magnitudes: is_rise false everywhere, peakmag NaN (the documented departure from the reference)
    got = _check_kernel(cuda, *one([t, t + 1, t + 2], [nan, nan, nan]))
    assert not got["is_rise"].any() and np.isnan(got["peakmag"]).all() and got["later"].tolist() == [2, 1, 0]
    # a NaN jd: later than every finite one, never a rise alert; two of them: by row; at the peak: no rise alert at all
    got = _check_kernel(cuda, *one([t + 1, nan, t, nan, t + 2], [18.0, 19.0, 17.0, 19.0, 18.5]))
    assert got["later"].tolist() == [3, 1, 4, 0, 2] and got["is_rise"].tolist() == [False, False, True, False, False]
    got = _check_kernel(cuda, *one([t + 1, nan, t], [18.0, 17.0, 17.5]))
    assert not got["is_rise"].any() and got["later"].tolist() == [1, 0, 2]
    # the same inside the LDS forms: few epochs, few magnitudes, NaN in both columns, an all-NaN object of each form
    rng = np.random.default_rng(5)
    ids, jd, mag = _table([70, 200, 1500, 90, 1100], seed=6, nan_mag=0.3)
    jd = 2459000.5 + rng.integers(0, 12, len(jd)).astype(np.float64)
    jd[rng.random(len(jd)) < 0.05] = nan
    mag[(ids == 1000 + 7 * 3) | (ids == 1000 + 7 * 4)] = nan
    got = _check_kernel(cuda, ids, jd, mag)
    assert not got["is_rise"][ids >= 1000 + 7 * 3].any() and got["is_rise"][ids < 1000 + 7 * 3].any()
    for o in np.unique(ids):
        rows = np.flatnonzero(ids == o)
        assert np.array_equal(np.sort(got["later"][rows]), np.arange(len(rows)))


def test_draws_follow_size_position_and_first_appearance(cuda):
    """Objects of equal size get equal N by position; split is constant inside an object, follows the order of first
    appearance, and does not change when the rows inside objects are reordered; another seed gives other draws."""
    from btsbot_amd import splits
    rng = np.random.default_rng(9)
    sizes = [7, 7, 7, 70, 70, 1, 1, 30] + [int(x) for x in rng.integers(1, 12, 60)]
    ids, jd, mag = _table(sizes, seed=10)
    lab = {k: v.cpu().numpy() for k, v in splits.label_set(*_dev(cuda, ids, jd, mag)).items()}
    by_size = {}
    for o in np.unique(ids):
        rows = np.flatnonzero(ids == o)
        assert (lab["split"][rows] == lab["split"][rows[0]]).all() and (lab["object_rank"][rows] == lab["object_rank"][rows[0]]).all()
        assert np.array_equal(by_size.setdefault(len(rows), lab["N"][rows]), lab["N"][rows])
    first = np.unique(ids, return_index=True)[1]
    assert np.array_equal(lab["object_rank"][np.sort(first)], np.arange(len(sizes)))
    draws = np.random.RandomState(2).choice(3, size=len(sizes), p=[0.81, 0.09, 0.10])
    assert np.array_equal(lab["split"], draws[lab["object_rank"]]) and set(draws.tolist()) == {0, 1, 2}
    # the rows of every object shuffled among the object's own places: first appearances stay where they were
    jd2, mag2 = jd.copy(), mag.copy()
    for o in np.unique(ids):
        rows = np.flatnonzero(ids == o)
        shuffled = rng.permutation(rows)
        jd2[rows], mag2[rows] = jd[shuffled], mag[shuffled]
    again = {k: v.cpu().numpy() for k, v in splits.label_set(*_dev(cuda, ids, jd2, mag2)).items()}
    assert np.array_equal(again["split"], lab["split"]) and np.array_equal(again["N"], lab["N"])
    assert not np.array_equal(again["is_rise"], lab["is_rise"])
    other = splits.label_set(*_dev(cuda, ids, jd, mag), seed=3, fractions=(0.5, 0.25, 0.25))
    _same(other, restate_labels(ids, jd, mag, seed=3, fractions=(0.5, 0.25, 0.25)), LABEL_OUT)
    assert not np.array_equal(other["N"].cpu().numpy(), lab["N"])
    # near_threshold reads the peakmag column when there is one, the computed minimum otherwise
    col = np.where(np.arange(len(ids)) % 2 == 0, 18.5, 18.6)
    assert np.array_equal(splits.label_set(*_dev(cuda, ids, jd, mag, col))["near_threshold"].cpu().numpy(), col == 18.5)
    assert np.array_equal(lab["near_threshold"], (lab["peakmag"] > 18.4) & (lab["peakmag"] < 18.6))


def test_misuse_raises(cuda):
    from btsbot_amd import _lib, splits
    ids = torch.arange(6, device=cuda) // 2
    f64 = torch.zeros(6, dtype=torch.float64, device=cuda)
    for fn in (splits.label_set, splits.split_labels):
        with pytest.raises(ValueError):
            fn(ids, f64[:5], f64)                                          # lengths
        with pytest.raises(ValueError):
            fn(ids.view(3, 2), f64, f64)                                   # shape
        with pytest.raises(ValueError):
            fn(ids.double(), f64, f64)                                     # float ids
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(ids.cpu(), f64.cpu(), f64.cpu())
    with pytest.raises(ValueError):
        splits.label_set(ids, f64, f64, peakmag=f64[:2])
    for fractions in ((0.8, 0.1, 0.2), (0.5, 0.5), (1.2, -0.1, -0.1)):
        with pytest.raises(ValueError, match="fractions"):
            splits.label_set(ids, f64, f64, fractions=fractions)
    i32 = torch.zeros(6, dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError):
        splits.subset_mask("train", ids, i32, i32, -1)
    with pytest.raises(ValueError):
        splits.subset_mask("train", ids, i32, i32, 5, -2)
    with pytest.raises(ValueError):
        splits.subset_mask("train", ids, i32[:4], i32, 5)
    with pytest.raises(ValueError):
        splits.subset_mask("train", ids, i32, i32, 5, rise_only=True)      # the cut's column is missing
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        splits.subset_mask("train", ids.cpu(), i32.cpu(), i32.cpu(), 5)
    # the C entry: NULL pointers and negative counts are refused, nothing is launched for an empty table
    L = _lib.lib()
    u8 = torch.zeros(6, dtype=torch.uint8, device=cuda)
    off = torch.zeros(7, dtype=torch.int32, device=cuda)
    p = [C.c_void_p(t.data_ptr()) for t in (i32, off, f64, f64, i32, i32, i32, i32, u8, f64)]
    call = lambda a, n, m: L.btsbot_split_labels(a[0], a[1], n, m, *a[2:], C.c_void_p(0))
    for null in (0, 3, 9):                                                  # perm, magpsf, peakmag
        args = list(p)
        args[null] = C.c_void_p(0)
        assert call(args, 6, 1) == _lib.ERR_INVALID_ARG and b"split_labels" in L.btsbot_last_error()
    assert call(p, -1, 1) == _lib.ERR_INVALID_ARG and call(p, 6, -1) == _lib.ERR_INVALID_ARG
    assert call(p, 6, 0) == _lib.ERR_INVALID_ARG and call(p, 0, 0) == _lib.OK
    torch.cuda.synchronize()
    assert not u8.any()


# ---- files -------------------------------------------------------------------------------------------------------------
def test_files_end_to_end(cuda, tmp_path):
    """Base tables of two sets -> cut_set_and_assign_splits -> merge_sets_across_split -> create_subset(N_max_p=100):
    data.load_split reads all three splits; every triplet still lies beside its table row (candid is in the pixels); no
    object is in two splits; the written labels are label_set's and the kept rows subset_mask's."""
    import pandas as pd
    from btsbot_amd import data, splits
    rng = np.random.default_rng(12)
    base = tmp_path / "data" / "base_data"
    os.makedirs(base)
    tables, candid0 = {}, 1
    for s, name in enumerate(("trues", "vars")):
        sizes = [130, 3] + [int(x) for x in rng.integers(1, 7, 44)]
        ids, jd, mag = _table(sizes, seed=30 + s)
        names = [f"ZTF2{s}" + "".join(chr(97 + (k // 26 ** p) % 26) for p in range(6, -1, -1)) for k in ids]
        cand = pd.DataFrame({"candid": candid0 + rng.permutation(len(ids)), "objectId": names, "jd": jd, "magpsf": mag, "peakmag": 18.0 + (ids % 9) * 0.1, "label": 1 - s,
                             "sgscore1": np.round(rng.uniform(0, 1, len(ids)), 3), "fid": rng.integers(1, 3, len(ids))})
        candid0 += len(cand)
        cand.to_csv(base / f"{name}_candidates.csv", index=False)
        np.save(base / f"{name}_triplets.npy", np.broadcast_to(cand["candid"].to_numpy(np.float64)[:, None, None, None],
                                                                (len(cand), 2, 2, 3)).copy())
        tables[name] = cand
    cut = (tables["vars"]["fid"] == 1).to_numpy()
    n_trues = splits.cut_set_and_assign_splits("trues", None, "v9", str(base), device=cuda)
    n_vars = splits.cut_set_and_assign_splits("vars", cut, "v9", str(base), device=cuda)
    assert sum(n_trues.values()) == len(tables["trues"]) and sum(n_vars.values()) == int(cut.sum())
    data_dir = tmp_path / "data"
    seen, cols = {}, ["sgscore1", "fid", "peakmag"]
    for split in SPLITS:
        n_merged = splits.merge_sets_across_split(["trues", "vars"], split, "v9", str(base), str(data_dir))
        assert n_merged == n_trues[split] + n_vars[split] > 0
        n_kept = splits.create_subset(split, "v9", str(data_dir), N_max_p=100, device=cuda)
        config = {"model_name": "um_nn", "train_data_version": "v9", "metadata_cols": cols}
        _, meta, labels, cand = data.load_split(str(tmp_path) + "/", config, split)
        assert len(cand) == n_kept and tuple(meta.shape) == (n_kept, 3) and labels.shape[0] == n_kept
        trips = np.load(data_dir / f"{split}_triplets_v9_N100.npy")
        assert trips.shape == (n_kept, 2, 2, 3) and (trips == cand["candid"].to_numpy(np.float64)[:, None, None, None]).all()
        assert (cand["split"] == split).all() and set(cand["source_set"]) <= {"trues", "vars"}
        assert split != "train" or set(cand["source_set"]) == {"trues", "vars"}
        assert np.array_equal(cand["is_SN"].to_numpy(), (cand["source_set"] == "trues").to_numpy())
        assert np.array_equal(labels.numpy(), cand["is_SN"].to_numpy().astype(np.int64))
        for obj in set(cand["objectId"]):
            assert seen.setdefault(obj, split) == split
        # the rows kept: the merged file under the restated rule
        merged = pd.read_csv(data_dir / f"{split}_cand_v9.csv")
        k = restate_kernel(np.unique(merged["objectId"], return_inverse=True)[1], merged["jd"].to_numpy(), merged["magpsf"].to_numpy())
        keep = restate_subset(split, merged["source_set"].to_numpy()[k["first_row"]], merged["N"].to_numpy(), k["later"], 100)
        assert np.array_equal(merged["candid"].to_numpy()[keep], cand["candid"].to_numpy())
        if split == "train":
            assert 0 < n_kept < n_merged                                   # the 130-alert objects lose alerts
    assert set(seen.values()) == set(SPLITS)
    # the labels written: label_set's, on the tables as they were cut
    for name, table in (("trues", tables["trues"]), ("vars", tables["vars"][cut].reset_index(drop=True))):
        ids = np.unique(table["objectId"], return_inverse=True)[1]
        lab = restate_labels(ids, table["jd"].to_numpy(), table["magpsf"].to_numpy(), table["peakmag"].to_numpy())
        parts = [pd.read_csv(base / f"{name}_{sp}_cand_v9.csv") for sp in SPLITS]
        parts = pd.concat([f for f in parts if len(f)]).set_index("candid").loc[table["candid"]]
        assert parts["split"].tolist() == [SPLITS[c] for c in lab["split"]]
        for c in ("N", "is_rise", "near_threshold"):
            assert np.array_equal(parts[c].to_numpy(), lab[c]), (name, c)
    # subsample_data keeps whole objects, int(n_objects * perc / 100) of them
    n_sub = splits.subsample_data("train", "v9", str(data_dir), perc_to_keep=50)
    full = pd.read_csv(data_dir / "train_cand_v9_N100.csv")
    sub = pd.read_csv(data_dir / "train_cand_v9s50_N100.csv")
    assert len(sub) == n_sub and sub["objectId"].nunique() == int(full["objectId"].nunique() * 0.5)
    assert np.array_equal(full[full["objectId"].isin(set(sub["objectId"]))]["candid"].to_numpy(), sub["candid"].to_numpy())
    assert (np.load(data_dir / "train_triplets_v9s50_N100.npy")[:, 0, 0, 0] == sub["candid"].to_numpy()).all()
