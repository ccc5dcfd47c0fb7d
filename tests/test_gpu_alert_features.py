"""btsbot_alert_features on the device: the custom metadata columns of prep_alerts (reference alert_utils.py:333-441)
against the numpy restatement of tests/test_alert_features_host.py (which that file ties to the reference's recorded
output).  Every output is a selection or one float64 subtraction rounded once, so every comparison is exact, NaN
positions included."""
import ctypes as C
import gzip

import numpy as np
import pytest
import torch

from helpers import MM_PICO, build_model, seeded_state
from test_alert_features_host import GOLDEN, restate

pytestmark = pytest.mark.gpu

NAMES = ("object_id", "jd", "magpsf", "jdstarthist", "ncovhist", "ndethist")


def _run(cuda, case):
    from btsbot_amd import alert_utils
    out = alert_utils.alert_features(*(torch.from_numpy(np.ascontiguousarray(case[k])).to(cuda) for k in NAMES))
    assert out.dtype == torch.float32 and out.device.type == "cuda" and tuple(out.shape) == (len(case["jd"]), 8)
    return out.cpu().numpy()


def _check(cuda, case):
    got, want = _run(cuda, case), restate(*(case[k] for k in NAMES)).astype(np.float32)
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).all(axis=1))
    assert bad.size == 0, (f"{bad.size} rows differ, first: alert {bad[0]} of object {case['object_id'][bad[0]]}: "
                           f"got {got[bad[0]]}, want {want[bad[0]]}")
    return got


def _objects(sizes, seed, shuffle=True):
    """One batch with an object of every given size: jd near 2459000 with gaps from 1e-4 day to days, magpsf on a 0.01
    grid (minima repeat), jdstarthist on either side of the first detection."""
    rng = np.random.default_rng(seed)
    oid, jd, mag, jsh = [], [], [], []
    for k, n in enumerate(sizes):
        gaps = np.where(rng.random(n) < 0.4, rng.uniform(1e-4, 1e-3, n), rng.uniform(0.02, 5.0, n))
        t = 2459000.5 + rng.uniform(0, 300) + np.cumsum(gaps)
        oid.append(np.full(n, 1000 + 7 * k))
        jd.append(rng.permutation(t))
        mag.append(np.round(19 + 1.5 * np.cos(np.linspace(0, 9, n) + rng.uniform(0, 3)) + rng.normal(0, 0.2, n), 2))
        jsh.append(t.min() + rng.choice([-3.25, 0.0, 0.75], n))
    case = dict(object_id=np.concatenate(oid).astype(np.int64), jd=np.concatenate(jd), magpsf=np.concatenate(mag),
                jdstarthist=np.concatenate(jsh))
    n = len(case["jd"])
    case["ndethist"] = rng.integers(1, 50, n).astype(np.int32)
    case["ncovhist"] = (case["ndethist"] + rng.integers(0, 2000, n)).astype(np.int32)
    if shuffle:
        order = rng.permutation(n)
        case = {k: v[order] for k, v in case.items()}
    return case


def _one_object(jd, mag, jsh=None):
    n = len(jd)
    return dict(object_id=np.full(n, 5, dtype=np.int64), jd=np.asarray(jd, dtype=np.float64),
                magpsf=np.asarray(mag, dtype=np.float64),
                jdstarthist=np.full(n, np.min(jd) - 1.0) if jsh is None else np.asarray(jsh, dtype=np.float64),
                ncovhist=np.arange(10, 10 + n, dtype=np.int32), ndethist=np.full(n, 4, dtype=np.int32))


def test_golden_fixture(cuda):
    """The reference's recorded columns for the fixture's shuffled packets, through alert_features."""
    g = dict(np.load(GOLDEN))
    got, want = _run(cuda, g), g["reference"].astype(np.float32)
    assert np.array_equal(got, want)


def test_size_boundaries(cuda):
    """Objects of 1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1 and 2 TILE + 7 alerts in one shuffled batch: each of the
    three kernel forms (one wave; one workgroup over an LDS tile; an object streamed through the tile) and each hand-over
    between them, at the smallest sizes where they can go wrong."""
    from btsbot_amd.alert_utils import FEATURE_TILE as T
    _check(cuda, _objects([1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 7], seed=11))


def test_ties(cuda):
    """Equal jd inside an object: input order decides who is 'so far'.  The same minimum at two epochs: the earlier one
    gives jdpk.  A later alert fainter than the peak: days_since_peak > 0 and maxmag_so_far moves."""
    t = 2459010.5
    #            alert:  0      1      2      3      4      5
    case = _one_object([t + 2, t + 2, t + 0, t + 5, t + 2, t + 9],
                       [18.0, 17.5, 18.0, 17.5, 19.0, 20.25])
    got = _check(cuda, case)
    # time order: 2, then 0 < 1 < 4 (equal jd, input order), then 3, 5
    assert list(got[:, 2]) == [18.0, 17.5, 18.0, 17.5, 17.5, 17.5]       # alert 0 does not see alert 1 yet
    assert list(got[:, 3]) == [18.0, 18.0, 18.0, 19.0, 19.0, 20.25]      # maxmag_so_far moves with 4 and 5
    assert list(got[:, 5]) == [2.0, 0.0, 0.0, 3.0, 0.0, 7.0]             # 3 ties 1's minimum: the earlier epoch stays
    assert got[0, 5] == 2.0 and got[5, 5] > 0 and list(got[:, 0]) == [17.5] * 6 and list(got[:, 1]) == [20.25] * 6
    # the same, as the first 64 / first FEATURE_TILE alerts of larger objects (the LDS forms), ties across the batch
    rng = np.random.default_rng(5)
    for n in (200, 1500):
        jd = t + rng.integers(0, n // 4, n).astype(np.float64)            # about four alerts per epoch
        mag = 18 + rng.integers(0, 6, n) * 0.5                            # six magnitudes: minima repeat
        _check(cuda, _one_object(jd, mag))


def test_float64_time_differences(cuda):
    """Two alerts of one object 1e-5 day apart at jd ~ 2459000.5: a float32 jd would give 0 (its spacing there is 0.25 day);
    the result is the float64 difference rounded to float32."""
    a, b = 2459000.5, 2459000.5 + 1e-5
    got = _check(cuda, _one_object([b, a], [18.0, 17.0], jsh=[a - 2e-5, a - 2e-5]))
    assert np.float32(a) == np.float32(b)
    assert got[0, 5] == np.float32(b - a) and got[0, 5] > 0 and got[1, 5] == 0
    assert got[0, 4] == np.float32(b - (a - 2e-5)) and got[0, 6] == np.float32(a - (a - 2e-5))


def test_non_finite_inputs(cuda):
    """NaN magpsf are skipped (mid-object: nothing else changes; first alert: its own so-far columns and the peak's
    epoch are NaN; a whole object: columns 0-3, 5, 6 are NaN).  A NaN jdstarthist is not swallowed by the minimum: age
    and days_to_peak are NaN for that alert only."""
    t = 2459100.5
    nan = np.nan
    mid = _one_object([t, t + 1, t + 2, t + 3], [19.0, nan, 18.0, 18.5])
    got = _check(cuda, mid)
    assert list(got[:, 2]) == [19.0, 19.0, 18.0, 18.0] and list(got[:, 5]) == [0.0, 1.0, 0.0, 1.0]
    first = _one_object([t + 1, t, t + 2], [18.0, nan, 19.0])           # alert 1 is the earliest
    got = _check(cuda, first)
    assert np.isnan(got[1, [2, 3, 5, 6]]).all() and got[1, 0] == 18.0 and got[1, 4] == 1.0
    assert not np.isnan(got[[0, 2]]).any()
    allnan = _one_object([t, t + 1], [nan, nan])
    got = _check(cuda, allnan)
    assert np.isnan(got[:, [0, 1, 2, 3, 5, 6]]).all() and list(got[:, 4]) == [1.0, 2.0] and list(got[:, 7]) == [6.0, 7.0]
    jsh = _one_object([t, t + 1, t + 2], [19.0, 18.0, 18.5], jsh=[t - 1, nan, t - 1])
    got = _check(cuda, jsh)
    assert np.isnan(got[1, [4, 6]]).all() and got[1, 5] == 0.0 and not np.isnan(got[[0, 2]]).any()
    # the same inside objects of the LDS forms
    big = _objects([70, 1100], seed=3)
    big["magpsf"][::7] = nan
    big["jdstarthist"][::11] = nan
    _check(cuda, big)


def test_object_ids(cuda):
    """Negative ids, ids beyond 2^40, and two objects whose alerts interleave in the input."""
    case = _objects([5, 9, 4, 66], seed=2, shuffle=False)
    ids = np.array([-(1 << 45) - 3, (1 << 41) + 1, -1, (1 << 62)], dtype=np.int64)
    case["object_id"] = ids[(case["object_id"] - 1000) // 7]
    n = len(case["jd"])
    order = np.arange(n)
    order[:14] = [0, 5, 1, 6, 2, 7, 3, 8, 4, 9, 10, 11, 12, 13]           # objects 0 and 1 interleaved
    case = {k: v[order] for k, v in case.items()}
    assert list(case["object_id"][:4]) == [ids[0], ids[1], ids[0], ids[1]]
    _check(cuda, case)


def test_empty_batch_and_error_paths(cuda):
    from btsbot_amd import _lib, alert_utils
    e = torch.zeros(0, device=cuda)
    out = alert_utils.alert_features(e.long(), e.double(), e.double(), e.double(), e.int(), e.int())
    assert tuple(out.shape) == (0, 8) and out.dtype == torch.float32 and out.device.type == "cuda"
    assert tuple(alert_utils.make_metadata([], ["age", "sgscore1"], device=cuda).shape) == (0, 2)
    L = _lib.lib()
    i32 = torch.zeros(5, dtype=torch.int32, device=cuda)
    f64 = torch.zeros(4, dtype=torch.float64, device=cuda)
    o = torch.zeros(4, 8, device=cuda)
    p = [C.c_void_p(t.data_ptr()) for t in (i32, i32, f64, f64, f64, i32, i32, o)]
    for null in (0, 4, 7):                                                  # perm, magpsf, out8
        args = list(p)
        args[null] = C.c_void_p(0)
        assert L.btsbot_alert_features(args[0], args[1], 4, 1, *args[2:], C.c_void_p(0)) == _lib.ERR_INVALID_ARG
        assert b"alert_features" in L.btsbot_last_error()
    assert L.btsbot_alert_features(p[0], p[1], -1, 1, *p[2:], C.c_void_p(0)) == _lib.ERR_INVALID_ARG
    assert L.btsbot_alert_features(p[0], p[1], 4, -1, *p[2:], C.c_void_p(0)) == _lib.ERR_INVALID_ARG
    assert L.btsbot_alert_features(p[0], p[1], 0, 0, *p[2:], C.c_void_p(0)) == _lib.OK      # nothing to launch
    torch.cuda.synchronize()
    assert not o.any()
    with pytest.raises(ValueError):
        alert_utils.alert_features(torch.zeros(3, device=cuda), f64[:3], f64[:3], f64[:3], i32[:3], i32[:3])   # float ids
    with pytest.raises(ValueError):
        alert_utils.alert_features(i32[:3].long(), f64, f64[:3], f64[:3], i32[:3], i32[:3])                    # lengths


# ---- packets -> scores ---------------------------------------------------------------------------------
def _fits_gz(arr):
    """The stamp format alert packets carry (as tests/test_data_path.py writes it): gzip of a single-HDU FITS image, 80-character
    cards in 2880-byte blocks, big-endian float32 samples, NAXIS1 = fastest axis."""
    cards = [f"{'SIMPLE':<8}= {'T':>20}", f"{'BITPIX':<8}= {-32:>20d}", f"{'NAXIS':<8}= {2:>20d}",
             f"{'NAXIS1':<8}= {arr.shape[1]:>20d}", f"{'NAXIS2':<8}= {arr.shape[0]:>20d}", "END"]
    hdr = "".join(c.ljust(80) for c in cards)
    hdr = hdr.ljust((len(hdr) + 2879) // 2880 * 2880)
    data = arr.astype(">f4").tobytes()
    data += b"\0" * ((-len(data)) % 2880)
    return gzip.compress(hdr.encode("ascii") + data)


def test_packets_to_scores_end_to_end(cuda):
    """16 packets of 5 objects -> make_triplets + make_metadata -> a seeded mm_ConvNeXt in f32: the logits equal, bit for bit,
    those from the same triplets with the metadata matrix assembled on the host from the restatement, columns in the (shuffled)
    order of metadata_cols."""
    from btsbot_amd import alert_utils
    rng = np.random.default_rng(8)
    cols = list(MM_PICO["metadata_cols"])
    assert set(alert_utils.CUSTOM_COLS) - {"peakmag", "maxmag"} < set(cols) and "new_drb" in cols
    cols = [cols[i] for i in rng.permutation(len(cols))]
    plain = [c for c in cols if c not in alert_utils.CUSTOM_COLS and c != "new_drb"]
    obj = rng.integers(0, 5, 16)
    obj[:5] = np.arange(5)
    alerts = []
    for k in range(16):
        cand = {c: float(rng.uniform(-1, 1)) for c in plain}
        cand.update(jd=2459200.5 + float(rng.uniform(0, 30)), magpsf=float(np.round(rng.uniform(17, 20), 1)),
                    jdstarthist=2459199.0 + float(rng.uniform(0, 4)), ndethist=int(rng.integers(1, 20)),
                    ncovhist=int(rng.integers(20, 500)))
        cls = {"sgscore1": cand.pop("sgscore1")}                            # one field arrives under 'classifications'
        if k == 3:
            cand["fwhm"] = None                                             # a None field is NaN ...
        stamps = [rng.standard_normal((63, 63)).astype(np.float32) for _ in range(3)]
        alerts.append({"objectId": f"ZTF22{obj[k]:07d}", "candidate": cand, "classifications": cls,
                       **{f"cutout{n}": {"stampData": _fits_gz(s)} for n, s in zip(("Science", "Template", "Difference"), stamps)}})
    drb = rng.uniform(0, 1, 16)

    triplets, drop = alert_utils.make_triplets(alerts, device=cuda)
    meta = alert_utils.make_metadata(alerts, cols, new_drb=drb, device=cuda)
    assert not drop.any() and meta.dtype == torch.float32 and tuple(meta.shape) == (16, len(cols))

    rows = [a["candidate"] | a["classifications"] for a in alerts]
    feats = restate(obj, *(np.array([r[c] for r in rows]) for c in NAMES[1:]))
    host = np.empty((16, len(cols)), dtype=np.float64)
    for j, c in enumerate(cols):
        if c in alert_utils.CUSTOM_COLS:
            host[:, j] = feats[:, alert_utils.CUSTOM_COLS.index(c)]
        elif c == "new_drb":
            host[:, j] = drb
        else:
            host[:, j] = [np.nan if r[c] is None else r[c] for r in rows]
    host = host.astype(np.float32)
    got = meta.cpu().numpy()
    assert np.isnan(host[3, cols.index("fwhm")]) and np.isnan(host).sum() == 1
    assert np.array_equal(got, host, equal_nan=True)

    keep = np.arange(16) != 3                                               # ... and that alert is not scored
    model = build_model("mm_ConvNeXt", MM_PICO, seeded_state("mm_ConvNeXt", MM_PICO, seed=4), cuda, "f32")
    sel = torch.from_numpy(keep).to(cuda)
    with torch.no_grad():
        a = model(image_input=triplets[sel], metadata_input=meta[sel]).cpu().numpy()
        b = model(image_input=triplets[sel], metadata_input=torch.from_numpy(host[keep]).to(cuda)).cpu().numpy()
    assert np.isfinite(a).all() and a.std() > 0 and np.array_equal(a, b)
