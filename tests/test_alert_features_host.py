"""The custom metadata columns of prep_alerts (reference alert_utils.py:333-441), host side: a plain numpy restatement
of what btsbot_alert_features computes, tied to the reference's recorded output (tests/golden/alert_features.npz, made
by tests/golden/make_alert_features_golden.py from the reference's own function), and the argument checks of the Python
wrappers that need no device.  tests/test_gpu_alert_features.py imports the restatement as the kernel's oracle."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alert_features.npz")


def restate(object_id, jd, magpsf, jdstarthist, ncovhist, ndethist):
    """float64 [N, 8] in the order of alert_utils.CUSTOM_COLS.  Per alert i, over boolean masks: O = same object,
    P = the alerts of O with (jd, position) <= (jd[i], i).  NaN magpsf are skipped; an empty selection gives NaN."""
    object_id, jd, magpsf, jdstarthist = map(np.asarray, (object_id, jd, magpsf, jdstarthist))
    n = len(jd)
    pos = np.arange(n)
    out = np.full((n, 8), np.nan, dtype=np.float64)
    for i in range(n):
        O = object_id == object_id[i]
        P = O & ((jd < jd[i]) | ((jd == jd[i]) & (pos <= i)))
        seen = ~np.isnan(magpsf)
        first = np.nan if np.isnan(jdstarthist[i]) else min(jdstarthist[i], jd[O].min())
        jdpk = np.nan
        if (O & seen).any():
            out[i, 0], out[i, 1] = magpsf[O & seen].min(), magpsf[O & seen].max()
        if (P & seen).any():
            out[i, 2], out[i, 3] = magpsf[P & seen].min(), magpsf[P & seen].max()
            at_peak = np.flatnonzero(P & (magpsf == out[i, 2]))
            jdpk = jd[at_peak[np.lexsort((at_peak, jd[at_peak]))[0]]]     # earliest by (jd, position)
        out[i, 4] = jd[i] - first
        out[i, 5] = jd[i] - jdpk
        out[i, 6] = jdpk - first
        out[i, 7] = float(int(ncovhist[i]) - int(ndethist[i]))
    return out


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_restatement_reproduces_the_reference(golden):
    """The numpy restatement equals what the reference's prep_alerts recorded for the fixture's shuffled packets, bit
    for bit: in float64 and after the cast to float32 that feeds the model."""
    from btsbot_amd import alert_utils
    assert tuple(golden["columns"]) == alert_utils.CUSTOM_COLS
    n = len(golden["jd"])
    sizes = np.bincount(golden["object_id"])
    assert 200 <= n <= 1000 and 24 <= len(sizes) <= 60 and sizes.max() > 64 and sizes.min() == 1
    jd, oid = golden["jd"], golden["object_id"]
    assert all(len(np.unique(jd[oid == k])) == (oid == k).sum() for k in range(len(sizes)))     # distinct jd per object
    assert np.diff(np.sort(jd[oid == np.argmax(sizes)])).min() < 1e-3
    first_det = np.array([jd[oid == k].min() for k in oid])
    assert (golden["jdstarthist"] < first_det).any() and (golden["jdstarthist"] > first_det).any()
    got = restate(oid, jd, golden["magpsf"], golden["jdstarthist"], golden["ncovhist"], golden["ndethist"])
    assert got.dtype == np.float64 and golden["reference"].dtype == np.float64
    assert np.array_equal(got, golden["reference"])
    assert np.array_equal(got.astype(np.float32), golden["reference"].astype(np.float32))
    # the fixture is not trivial: so-far columns differ from the whole-object ones, peaks lie in the past
    assert (got[:, 2] != got[:, 0]).any() and (got[:, 3] != got[:, 1]).any() and (got[:, 5] > 0).any()


def _packets(n=6):
    return [{"objectId": f"ZTF{k % 2}", "candidate": {"jd": 2459000.5 + k, "magpsf": 19.0 - 0.1 * k, "jdstarthist": 2458999.0,
                                                     "ncovhist": 10 + k, "ndethist": 3, "sgscore1": 0.5, "drb": None},
             "classifications": {"braai": 0.9}} for k in range(n)]


def test_make_metadata_rejects_unknown_columns_before_device_work():
    """A column that is neither a packet field, nor a custom column, nor a supplied new_drb is a KeyError naming it --
    raised before anything touches a device (this test runs without one, and asks for one that cannot exist)."""
    from btsbot_amd import alert_utils
    nowhere = "cuda:1000"
    with pytest.raises(KeyError, match="no_such_column"):
        alert_utils.make_metadata(_packets(), ["sgscore1", "age", "no_such_column"], device=nowhere)
    with pytest.raises(KeyError, match="new_drb"):
        alert_utils.make_metadata(_packets(), ["sgscore1", "new_drb", "age"], device=nowhere)
    short = _packets()
    for a in short:
        del a["candidate"]["jdstarthist"]       # a custom column's own input is missing
    with pytest.raises(KeyError, match="jdstarthist"):
        alert_utils.make_metadata(short, ["age"], device=nowhere)
    with pytest.raises(ValueError, match="new_drb"):
        alert_utils.make_metadata(_packets(), ["new_drb"], new_drb=np.zeros(5), device=nowhere)


def test_alert_features_has_no_cpu_fallback():
    import btsbot_amd
    from btsbot_amd import alert_utils
    assert btsbot_amd.alert_features is alert_utils.alert_features
    assert btsbot_amd.make_metadata is alert_utils.make_metadata and btsbot_amd.CUSTOM_COLS is alert_utils.CUSTOM_COLS
    assert alert_utils.FEATURE_TILE > 64
    z = torch.zeros(4, dtype=torch.float64)
    i = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        alert_utils.alert_features(torch.arange(4), z, z, z, i, i)
