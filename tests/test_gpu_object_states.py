"""btsbot_amd.TriggerState and btsbot_amd.FeatureState on the same batches: what they share (csrc/object_table.h: the table,
the drop rule, the late rule, the counters) must come out the same from both, whatever each does with its own record.
tests/test_feature_state_host.py checks on the host that the batches reach every shared branch."""
import numpy as np
import pytest
import torch

from test_feature_state_host import (NAMES, SHARED_CAPACITY, SHARED_EXPORT, TRIGGER_NAMES, FeatureStreamRestatement,
                                     shared_batches)
from test_trigger_host import same_arrays

pytestmark = pytest.mark.gpu


def test_trigger_and_feature_state_agree_on_what_they_share(cuda):
    from btsbot_amd import FeatureState, TriggerState
    trig, feat = TriggerState(capacity=SHARED_CAPACITY, device=cuda), FeatureState(SHARED_CAPACITY, cuda)
    host = FeatureStreamRestatement(capacity=SHARED_CAPACITY)
    for b in shared_batches():
        cols = {k: torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for k, v in b.items()}
        td = trig.update(*(cols[k] for k in TRIGGER_NAMES))["dropped"]
        fd = feat.update(*(cols[k] for k in NAMES))["dropped"]
        assert torch.equal(td, fd)
        assert trig.counters() == feat.counters()
        te, fe = ({k: v.cpu().numpy() for k, v in s.export().items()} for s in (trig, feat))
        diff = same_arrays(te, fe, SHARED_EXPORT)
        assert diff is None, diff
        # ... and it is what the rule says, so the agreement is not two states doing nothing
        _, hd = host.update(*(b[k] for k in NAMES))
        assert np.array_equal(fd.cpu().numpy(), hd) and feat.counters() == host.counters()
    assert feat.counters()["objects"] == SHARED_CAPACITY and feat.counters()["dropped"] > 0 and feat.counters()["late"] > 0
