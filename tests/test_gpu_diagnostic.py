"""btsbot_alert_histograms, diagnostics.roc_points and diagnostics.diagnostic_data on the device: against what the
reference's diagnostic_fig drew for the fixture (tests/golden/diagnostic_fig.npz) and against the numpy restatement of
tests/test_diagnostic_host.py (which that file ties to the recording).  Every output is an integer count, a selection or
one float64 division, so every comparison is exact; the area under the ROC curve alone is held within 1e-12 (a sum of at
most a few thousand terms of magnitude <= 1, whose order can move it by about 1e-13)."""
import ctypes as C
import json
import math
import warnings

import numpy as np
import pytest
import torch

from helpers import CONFIGS, seeded_state
from test_diagnostic_host import (CLASS_EDGES, CLASSES, GOLDEN, differences, golden_inputs, restate_diagnostic,
                                  restate_histograms, restate_roc)
from test_policy_host import REFERENCE_POLICIES, same_performance

pytestmark = pytest.mark.gpu

KEYS = ("joint", "mag", "score", "cls", "total")
T0 = 2459300.5


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _check(cuda, mag, raw, lab, **bins):
    """alert_histograms against the restatement on the same edges, every count."""
    from btsbot_amd import diagnostics
    mag, raw, lab = np.asarray(mag, dtype=np.float64), np.asarray(raw, dtype=np.float32), np.asarray(lab, dtype=np.int64)
    got = diagnostics.alert_histograms(*_dev(cuda, mag, raw, lab), **bins)
    assert all(got[k].dtype == torch.int64 and got[k].device.type == "cuda" for k in KEYS + ("counts",))
    want = restate_histograms(mag, raw, lab, got["mag_edges"], got["score_edges"], got["class_edges"])
    for k in KEYS:
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape, (k, g.shape, want[k].shape)
        bad = np.argwhere(g != want[k])
        assert bad.size == 0, f"{k}: {len(bad)} counters differ, first at {bad[0]}: got {g[tuple(bad[0])]}, want {want[k][tuple(bad[0])]}"
    assert int(got["total"].sum()) == len(mag)
    return {k: got[k].cpu().numpy() for k in KEYS}


def _seeded(n, seed):
    """Magnitudes over 14.5-21.5 in hundredths (so that many sit on an edge), scores half of them float32 multiples of
    1/56 (every other one the float32 next to a score edge, not the edge itself), labels half and half."""
    rng = np.random.default_rng(seed)
    mag = np.round(rng.uniform(14.5, 21.5, n), 2)
    raw = rng.random(n).astype(np.float32)
    grid = rng.random(n) < 0.5
    raw[grid] = (np.round(raw[grid] * 56) / 56).astype(np.float32)
    return mag, raw, rng.integers(0, 2, n)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_golden_histograms(cuda, golden):
    """alert_histograms on the fixture equals the arrays the reference's figure drew, exactly."""
    rows, _ = golden_inputs(golden)
    got = _check(cuda, rows["magpsf"], rows["raw_preds"], rows["label"])
    assert differences(got, golden) == []
    assert np.array_equal(got["total"], golden["ref_totals"])


def test_golden_diagnostic_data(cuda, golden):
    """diagnostic_data on the fixture: the recorded counts and ROC points exactly, auc within 1e-12, the save_dt histograms
    of the three drawn policies with their edges, policy_performance equal to the direct call."""
    from btsbot_amd import diagnostics, val
    g = golden
    rows, extra = golden_inputs(g)
    args = _dev(cuda, *(rows[k] for k in ("object_id", "jd", "magpsf", "label", "raw_preds")))
    kw = dict(zip(extra, _dev(cuda, *extra.values())))
    hist = {"loss": [0.6, 0.5], "val_accuracy": np.array([0.7, 0.8])}
    data = diagnostics.diagnostic_data(*args, **kw, history=hist)
    json.loads(json.dumps(data))                                              # serialisable as it stands
    assert set(data) == {"roc", "score_mag_hist", "class_mag_hist", "confusion", "summary", "history", "policy_performance",
                         "policy_save_dt"}
    sm, ch = data["score_mag_hist"], data["class_mag_hist"]
    mine = dict(joint=np.array(sm["counts"]), mag=np.array(sm["mag_counts"]), score=np.array(sm["score_counts"]),
                cls=np.array([ch[c] for c in CLASSES]))
    assert differences(mine, g) == []
    assert np.array_equal(sm["mag_edges"], g["ref_mag_edges"]) and np.array_equal(sm["score_edges"], g["ref_score_edges"])
    assert np.array_equal(ch["bins"], CLASS_EDGES)
    for k in ("fpr", "tpr", "thresholds"):
        assert np.array_equal(np.array(data["roc"][k]), g["sk_" + k]), k
    assert abs(data["roc"]["auc"] - float(g["ref_scalars"][0])) <= 1e-12
    tp, fp, tn, fn = (int(v) for v in g["ref_totals"])
    assert [data["confusion"][c] for c in CLASSES] == [tp, fp, tn, fn]
    assert data["confusion"]["normalized"] == [[tn / (tn + fp), fp / (tn + fp)], [fn / (fn + tp), tp / (fn + tp)]]
    assert data["summary"] == val.alert_summary(args[4], args[3])
    for k, v in zip(("bal_acc", "bts_acc", "notbts_acc", "alert_precision", "alert_recall"), g["ref_scalars"][1:]):
        assert data["summary"][k] == float(v), k
    assert data["history"] == {"loss": [0.6, 0.5], "val_accuracy": [0.7, 0.8]}
    direct = val.policy_performance(*args, **kw)
    assert same_performance(data["policy_performance"], direct) is None
    want = restate_diagnostic(**rows, **extra)["policy_save_dt"]
    names = list(REFERENCE_POLICIES)
    assert list(data["policy_save_dt"]) == names
    for q, name in enumerate(names):
        dt = data["policy_save_dt"][name]
        assert np.array_equal(np.sort(dt["values"]), want[name]["values"]), name
        assert np.array_equal(dt["counts"], want[name]["counts"]) and np.array_equal(dt["edges"], want[name]["edges"]), name
        if q < 3:                                                              # the three the reference draws
            assert np.array_equal(dt["counts"], g["ref_save_dt_counts"][q]) and np.array_equal(dt["edges"], g["ref_save_dt_edges"][q])
        assert float(np.median(dt["values"])) == data["policy_performance"][name]["med_save_dt"]
    # without save times there is nothing to draw; an empty split gives empty panels
    bare = diagnostics.diagnostic_data(*args)
    assert all(v is None for v in bare["policy_save_dt"].values()) and bare["history"] == {}
    assert same_performance(bare["policy_performance"], val.policy_performance(*args)) is None
    e = torch.zeros(0, device=cuda)
    empty = diagnostics.diagnostic_data(e.long(), e.double(), e.double(), e.long(), e.float())
    assert np.sum(empty["score_mag_hist"]["counts"]) == 0 and empty["roc"]["thresholds"] == [math.inf]
    assert all(v is None for v in empty["policy_save_dt"].values())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1023, 1025, 300_007, 1_000_003])
def test_alert_counts(cuda, n):
    """One lane, one wave less one, one wave, one wave and one, four waves and one, a workgroup (1024 threads) less one and
    one more.  The grid is capped at 256 workgroups of 1024 threads, 262,144 alerts a sweep: at 300,007 alerts the first 37
    workgroups make a second trip of the grid-stride loop and the others do not; 1,000,003 was added so that every
    workgroup makes three trips and some a fourth."""
    got = _check(cuda, *_seeded(n, 100 + n))
    if n >= 257:
        assert (got["mag"] > 0).all() and (got["score"] > 0).all() and got["total"].min() > 0


def test_a_counter_passes_65535(cuda):
    """70,000 alerts in one bin of every histogram."""
    n = 70_000
    got = _check(cuda, np.full(n, 18.25), np.full(n, 0.75, dtype=np.float32), np.ones(n, dtype=np.int64))
    assert got["joint"].max() == n and got["mag"].max() == n and got["score"].max() == n and got["cls"][0].max() == n
    assert got["total"].tolist() == [n, 0, 0, 0]


def test_bin_shapes(cuda):
    """One bin per table; 64 bins per table with a 64 x 64 joint histogram; a caller's non-uniform class bins."""
    mag, raw, lab = _seeded(5_003, 7)
    one = _check(cuda, mag, raw, lab, mag_bins=1, score_bins=1, class_bins=[16.0, 21.0])
    assert one["joint"].shape == (1, 1) and one["cls"].shape == (4, 1) and one["score"][0] == len(raw)
    big = _check(cuda, mag, raw, lab, mag_bins=64, mag_range=(15, 21), score_bins=64, class_bins=np.linspace(14.75, 21.25, 65))
    assert big["joint"].shape == (64, 64) and (big["joint"] > 0).sum() > 2000
    odd = _check(cuda, mag, raw, lab, mag_bins=[15.0, 15.01, 17.5, 19.995, 21.3], score_bins=[0.1, 0.5, 0.50001, 0.9],
                 class_bins=[14.9, 16.0, 16.01, 18.5, 20.0, 21.49])
    assert odd["cls"].shape == (4, 5) and (odd["cls"].sum(0) > 0).all()


def test_special_values(cuda):
    """NaN, +inf, -inf and -0.0 magnitudes, NaN scores: in no bin (a NaN score predicts 0), still in the totals; -0.0 is 0.0."""
    nan, inf = np.nan, np.inf
    mag = [nan, inf, -inf, -0.0, 0.0, 18.0, 18.0, 18.0, 16.0, 21.0]
    raw = [0.9, 0.9, 0.1, 0.6, 0.6, nan, 0.5, 1.0, 0.0, -0.0]
    lab = [1, 0, 0, 1, 1, 1, 1, 0, 0, 1]
    got = _check(cuda, mag, raw, lab, mag_bins=[-1.0, 0.0, 17.0, 21.0], class_bins=[0.0, 18.0, 21.0])
    assert got["total"].tolist() == [3, 2, 2, 3]
    assert got["mag"].tolist() == [0, 3, 4] and got["score"].sum() == 9 and got["joint"].sum() == 6
    assert got["cls"].tolist() == [[2, 0], [0, 1], [1, 0], [0, 3]]
    rng = np.random.default_rng(12)
    mag, raw, lab = _seeded(4_001, 13)
    mag[rng.random(4_001) < 0.1] = nan
    mag[rng.random(4_001) < 0.02] = inf
    raw[rng.random(4_001) < 0.1] = nan
    _check(cuda, mag, raw, lab)


def test_out_is_added_into(cuda):
    """Two calls on the halves of a split, the second into the first one's buffer, equal one call on the whole."""
    from btsbot_amd import diagnostics
    mag, raw, lab = _seeded(2_001, 5)
    whole = diagnostics.alert_histograms(*_dev(cuda, mag, raw.astype(np.float32), lab))
    first = diagnostics.alert_histograms(*_dev(cuda, mag[:900], raw[:900], lab[:900]))
    before = first["counts"].clone()
    second = diagnostics.alert_histograms(*_dev(cuda, mag[900:], raw[900:], lab[900:]), out=first["counts"])
    assert second["counts"].data_ptr() == first["counts"].data_ptr() and not torch.equal(before, second["counts"])
    assert torch.equal(second["counts"], whole["counts"]) and int(whole["total"].sum()) == 2_001
    with pytest.raises(ValueError):
        diagnostics.alert_histograms(*_dev(cuda, mag, raw, lab), mag_bins=5, out=first["counts"])


def test_argument_errors(cuda):
    """ValueError / BTSBOT_ERR_INVALID_ARG before any launch: 65 bins, a joint histogram of more than 4096 cells (which
    needs a table of more than 64 bins: 17 x 241 = 4097), unsorted edges, mismatched lengths, CPU tensors."""
    from btsbot_amd import _lib, diagnostics
    mag, raw, lab = _dev(cuda, *_seeded(16, 1))
    for kw in (dict(mag_bins=65), dict(score_bins=65), dict(class_bins=np.linspace(15, 21, 67)),
               dict(mag_bins=17, score_bins=np.linspace(0, 1, 242)), dict(class_bins=[15.0, 17.0, 16.0]),
               dict(mag_bins=[16.0, 16.0, 17.0]), dict(score_bins=[0.0, np.inf])):
        with pytest.raises(ValueError):
            diagnostics.alert_histograms(mag, raw, lab, **kw)
    with pytest.raises(ValueError):
        diagnostics.alert_histograms(mag, raw[:5], lab)
    with pytest.raises(ValueError):
        diagnostics.roc_points(raw[:5], lab)
    with pytest.raises(RuntimeError, match="runs on the GPU; there is no CPU fallback"):
        diagnostics.alert_histograms(mag.cpu(), raw.cpu(), lab.cpu())
    # the C entry itself
    L = _lib.lib()
    out = torch.zeros(4484, dtype=torch.int64, device=cuda)
    lab32 = lab.to(torch.int32)
    ptr = [C.c_void_p(t.data_ptr()) for t in (mag, raw, lab32)]
    dp = C.POINTER(C.c_double)

    def call(me, se, ce, n=16, ptrs=ptr, o=out, nm=None):
        arr = [np.ascontiguousarray(e, dtype=np.float64) for e in (me, se, ce)]
        return L.btsbot_alert_histograms(*ptrs, n, arr[0].ctypes.data_as(dp), len(arr[0]) - 1 if nm is None else nm,
                                         arr[1].ctypes.data_as(dp), len(arr[1]) - 1, arr[2].ctypes.data_as(dp),
                                         len(arr[2]) - 1, C.c_void_p(o.data_ptr()), C.c_void_p(0))
    ok = (np.linspace(16, 21, 29), np.linspace(0, 1, 29), CLASS_EDGES)
    for bad in ((np.linspace(16, 21, 67), ok[1], ok[2]), (ok[0], np.linspace(0, 1, 67), ok[2]), (ok[0], ok[1], np.linspace(15, 21, 67)),
                (np.linspace(16, 21, 18), np.linspace(0, 1, 242), ok[2]), ([16.0, 18.0, 17.0], ok[1], ok[2]),
                (ok[0], [0.0, 0.5, 0.5], ok[2]), (ok[0], ok[1], [15.0, np.nan])):
        assert call(*bad) == _lib.ERR_INVALID_ARG and b"alert_histograms" in L.btsbot_last_error()
    assert call(*ok, nm=0) == _lib.ERR_INVALID_ARG and call(*ok, n=-1) == _lib.ERR_INVALID_ARG
    for null in range(3):
        args = list(ptr)
        args[null] = C.c_void_p(0)
        assert call(*ok, ptrs=args) == _lib.ERR_INVALID_ARG
    assert call(*ok, n=0) == _lib.OK                                           # nothing to launch
    torch.cuda.synchronize()
    assert not out.any()
    assert call(*ok) == _lib.OK
    torch.cuda.synchronize()
    assert int(out[28 * 28 + 28 + 28 + 48:28 * 28 + 28 + 28 + 52].sum()) == 16 and not out[28 * 28 + 28 + 28 + 52:].any()


def _roc_case(cuda, raw, lab):
    from btsbot_amd import diagnostics
    raw, lab = np.asarray(raw, dtype=np.float32), np.asarray(lab, dtype=np.int64)
    got = diagnostics.roc_points(*_dev(cuda, raw, lab))
    want = restate_roc(raw, lab)
    for k in ("fpr", "tpr", "thresholds"):
        assert got[k].dtype == np.float64 and np.array_equal(got[k], want[k], equal_nan=True), k
    assert got["auc"] == want["auc"] or (math.isnan(got["auc"]) and math.isnan(want["auc"]))
    return got


def test_roc_points(cuda, golden):
    """The fixture's recorded roc_curve; then heavy ties, all scores equal, one class only and a single alert against the
    restatement -- and against sklearn's roc_curve itself where it is installed."""
    g = golden
    got = _roc_case(cuda, g["raw_preds"], g["label"])
    for k in ("fpr", "tpr", "thresholds"):
        assert np.array_equal(got[k], g["sk_" + k]), k
    assert abs(got["auc"] - float(g["ref_scalars"][0])) <= 1e-12
    rng = np.random.default_rng(8)
    ties = (np.round(rng.random(5_000), 2), rng.integers(0, 2, 5_000))
    cases = {"ties": ties, "equal": (np.full(300, 0.4), rng.integers(0, 2, 300)), "all_pos": (rng.random(200), np.ones(200)),
             "all_neg": (rng.random(200), np.zeros(200)), "one": ([0.3], [1]), "three": ([0.1, 0.9, 0.5], [0, 1, 1])}
    out = {name: _roc_case(cuda, *case) for name, case in cases.items()}
    assert len(out["ties"]["fpr"]) <= 102 and len(out["equal"]["fpr"]) == 2 and out["equal"]["auc"] == 0.5
    assert np.isnan(out["all_pos"]["fpr"]).all() and np.isnan(out["all_neg"]["tpr"]).all() and math.isnan(out["all_pos"]["auc"])
    assert out["one"]["thresholds"].tolist() == [math.inf, np.float32(0.3)]
    try:
        from sklearn.metrics import roc_curve
    except ImportError:
        return
    for name, (raw, lab) in cases.items():
        if name == "one":
            continue                                                          # (roc_curve's own checks want two alerts)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                   # "no negative samples": the NaN column
            want = roc_curve(np.asarray(lab, dtype=np.int64), np.asarray(raw, dtype=np.float32).astype(np.float64))
        for k, w in zip(("fpr", "tpr", "thresholds"), want):
            assert np.array_equal(out[name][k], w, equal_nan=True), (name, k)


def _same(a, b):
    """Equality of two JSON-like values, NaN equal to NaN."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a):
        return math.isnan(b)
    return a == b and type(a) == type(b)


def test_fit_writes_the_diagnostic(cuda, tmp_path):
    """train.fit(diagnostic=True) on the smallest synthetic split (the run of test_gpu_policy.py, on 128 training alerts):
    diagnostic.json loads and equals diagnostic_data on the same arrays, the PDF is there where matplotlib is, and
    report.json is byte for byte what the same run writes with the flag off.

    Why 128 training alerts and not that test's 384: the epoch's training loss is one float atomic add per wave
    (eval_metrics_kernel), so with the six waves of 384 alerts its last bit depends on the order in which they arrive.  On
    384 alerts two runs in one process wrote train_loss[0] = 0.7543132305145264 and 0.7543133497238159 (one float32 ulp
    apart, everything else equal) although fit reads the flag only after report.json is closed: report.json of two
    separate runs is not comparable byte for byte there, flag or no flag.  With 128 alerts two waves add, and a + b is
    b + a."""
    import btsbot_amd
    from btsbot_amd import data, diagnostics
    from btsbot_amd.synthetic import synthetic_batch
    from btsbot_amd.train import Trainer, fit
    kind, cfg = CONFIGS["um_nn"]
    _, meta, _ = synthetic_batch(512, seed=21)
    lab = (meta[:, 5] > meta[:, 5].median()).long()
    rng = np.random.default_rng(6)
    obj = rng.integers(0, 24, 128)
    cand = {"objectId": np.array([f"ZTF21{k:07d}" for k in obj]), "jd": T0 + rng.uniform(0, 40, 128),
            "magpsf": np.round(rng.uniform(17.0, 19.4, 128), 2), "save_time": (T0 + 5.0 + obj % 7).astype(np.float64)}
    reports, hists = {}, {}
    for name, flag in (("on", True), ("off", False)):
        torch.manual_seed(11)
        torch.cuda.manual_seed_all(11)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = btsbot_amd.um_nn(cfg, precision="f32")
        m.load_state_dict(seeded_state(kind, cfg, seed=3))
        m = m.to(cuda).train()
        ds = data.DeviceDataset(None, meta[:128], lab[:128], 64, device=cuda,
                                generator=torch.Generator(device=cuda).manual_seed(2))
        tr = Trainer(m, lr=3e-3, betas=(0.9, 0.999), pos_weight=ds.pos_weight, epochs=2, warmup_epochs=1)
        hists[name] = fit(tr, ds, None, meta[384:], lab[384:], str(tmp_path / name), epochs=2, patience=2, config=cfg,
                          val_cand=cand, diagnostic=flag, run_name="tiny")
        reports[name] = (tmp_path / name / "report.json").read_bytes()
    assert reports["on"] == reports["off"]
    assert not (tmp_path / "off" / "diagnostic.json").exists() and not (tmp_path / "off" / "tiny.pdf").exists()
    assert set(hists["on"]) == set(hists["off"]) and hists["on"]["val_summary"] == hists["off"]["val_summary"]
    with open(tmp_path / "on" / "diagnostic.json") as f:
        got = json.load(f)
    h = hists["on"]
    ids, jd, mag, save = _dev(cuda, obj, cand["jd"], cand["magpsf"], cand["save_time"])
    curves = {"loss": h["train_loss"], "val_loss": h["val_loss"], "accuracy": h["train_accuracy"], "val_accuracy": h["val_accuracy"]}
    want = diagnostics.diagnostic_data(ids, jd, mag, torch.from_numpy(h["best_val_labels"]).to(cuda).long(),
                                       torch.from_numpy(h["best_raw_preds"]).to(cuda), save_time=save, history=curves)
    assert _same(got, json.loads(json.dumps(want)))
    assert got["history"]["val_loss"] == h["val_loss"] and sum(got["confusion"][c] for c in CLASSES) == 128
    assert same_performance(got["policy_performance"], h["val_summary"]["policy_performance"]) is None
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    assert (tmp_path / "on" / "tiny.pdf").stat().st_size > 10_000
