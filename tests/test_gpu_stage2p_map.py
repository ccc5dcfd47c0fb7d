"""stage2p's fp32 map and last downsample (btsbot_amd/csrc/stage2p.hip): the map's rows are a padded pitch apart and
only the live ones exist, the downsample's LayerNorm normalises the four pixels its convolution reads, half a wave each,
and the convolution streams its filter through a ring of one whole tile.  None of this changes the arithmetic.

Nine alerts with 4, 5 and 7 alerts per workgroup (btsbot_set_option "stage2p_alerts") are workgroups of 4 / 4 / 1,
5 / 4 and 7 / 2 alerts: every form gets a full workgroup, a ragged one (its last alert is alert 8 each time) and a last
pixel row that is not row 0 of a 16-column tile.  f16x2 runs 5 alerts per workgroup where 7 are asked for (by design:
the doubled planes of 7 do not fit the LDS).

Inputs: synthetic_batch(9, seed=11) with alert 1 shifted by a constant and a 16 x 16 pixel patch of alert 2 zeroed in
all three cutouts; weights seeded_state(seed=3).  On the CPU the oracle's taps for these inputs are finite with
max|ref| = 6.93 (stage 2) and 4.93 (stage 3).

Tolerance: the error is owned by the 16-bit operand rounding, which this change does not touch.  Each figure is held to
what the library before this change measured on exactly these inputs, x 1.25 (PARENT below, NEW beside it: measured
on an MI355X; the figures are max|d| / max(1, max|ref|) against the fp32 oracle).  The new figures equal the previous
ones to every printed digit: the taps and logits are the same bits (the benchmark's logits.npy of both libraries are
numpy.array_equal as well).
"""
import pytest
import torch

from helpers import CONFIGS, seeded_state, build_model, run_model
from btsbot_amd import _lib
from btsbot_amd.synthetic import synthetic_batch
from oracle import convnext_oracle as O   # checker only

pytestmark = pytest.mark.gpu

N = 9
SLICES = ("stage2 whole map", "stage2 pixels 0 1 3 4", "stage2 pixels 2 5 6 7 8", "stage2 alert 8 (ragged workgroup)",
          "stage3 whole", "stage3 alert 8 (ragged workgroup)")
# (precision, alerts per workgroup asked for) -> the SLICES figures; the library before this change
PARENT = {
    ("bf16", 4): (8.524783e-03, 8.524783e-03, 8.044469e-03, 5.947166e-03, 7.061242e-03, 5.703994e-03),
    ("bf16", 5): (8.524783e-03, 8.524783e-03, 8.044469e-03, 5.947166e-03, 7.061242e-03, 5.703994e-03),
    ("bf16", 7): (8.524783e-03, 8.524783e-03, 8.044469e-03, 5.947166e-03, 7.061242e-03, 5.703994e-03),
    ("f16", 4): (1.009658e-03, 1.005587e-03, 1.009658e-03, 8.437653e-04, 1.061117e-03, 8.330794e-04),
    ("f16", 5): (1.009658e-03, 1.005587e-03, 1.009658e-03, 8.437653e-04, 1.061117e-03, 8.330794e-04),
    ("f16", 7): (1.009658e-03, 1.005587e-03, 1.009658e-03, 8.437653e-04, 1.061117e-03, 8.330794e-04),
    ("f16x2", 4): (4.370816e-06, 3.854578e-06, 4.370816e-06, 3.871785e-06, 3.626841e-06, 2.937741e-06),
    ("f16x2", 5): (4.370816e-06, 3.854578e-06, 4.370816e-06, 3.871785e-06, 3.626841e-06, 2.937741e-06),
    ("f16x2", 7): (4.370816e-06, 3.854578e-06, 4.370816e-06, 3.871785e-06, 3.626841e-06, 2.937741e-06),
}
# this kernel, for the record
NEW = {
    ("bf16", 4): (8.524783e-03, 8.524783e-03, 8.044469e-03, 5.947166e-03, 7.061242e-03, 5.703994e-03),
    ("bf16", 5): (8.524783e-03, 8.524783e-03, 8.044469e-03, 5.947166e-03, 7.061242e-03, 5.703994e-03),
    ("bf16", 7): (8.524783e-03, 8.524783e-03, 8.044469e-03, 5.947166e-03, 7.061242e-03, 5.703994e-03),
    ("f16", 4): (1.009658e-03, 1.005587e-03, 1.009658e-03, 8.437653e-04, 1.061117e-03, 8.330794e-04),
    ("f16", 5): (1.009658e-03, 1.005587e-03, 1.009658e-03, 8.437653e-04, 1.061117e-03, 8.330794e-04),
    ("f16", 7): (1.009658e-03, 1.005587e-03, 1.009658e-03, 8.437653e-04, 1.061117e-03, 8.330794e-04),
    ("f16x2", 4): (4.370816e-06, 3.854578e-06, 4.370816e-06, 3.871785e-06, 3.626841e-06, 2.937741e-06),
    ("f16x2", 5): (4.370816e-06, 3.854578e-06, 4.370816e-06, 3.871785e-06, 3.626841e-06, 2.937741e-06),
    ("f16x2", 7): (4.370816e-06, 3.854578e-06, 4.370816e-06, 3.871785e-06, 3.626841e-06, 2.937741e-06),
}


def stress_inputs():
    img, meta, labels = synthetic_batch(N, seed=11)
    img = img.clone()
    img[1] += 0.5                        # pixel values are ~ 1/63 after the L2 normalisation
    img[2, :, 20:36, 20:36] = 0.0
    return img, meta, labels


def make_case():
    kind, cfg = CONFIGS["mm_pico"]
    sd = seeded_state(kind, cfg, seed=3)
    img, meta, labels = stress_inputs()
    taps = {}
    with torch.no_grad():
        O.mm_convnext_forward(sd, cfg, img, meta, taps=taps)
    ref2 = taps["stage2"].permute(0, 2, 3, 1).reshape(N, 9, 256).contiguous()   # NCHW -> [alert][pixel][channel]
    ref3 = taps["stage3"].permute(0, 2, 3, 1).reshape(N, 1, 512).contiguous()
    for ref in (ref2, ref3):
        assert torch.isfinite(ref).all() and 1.0 <= ref.abs().max().item() <= 100.0
    return kind, cfg, sd, img, meta, labels, ref2, ref3


@pytest.fixture(scope="module")
def case():
    return make_case()


def set_alerts(m, g):
    _lib.check(_lib.lib().btsbot_set_option(m._handle.ptr, b"stage2p_alerts", g), "btsbot_set_option")


def forward(case, cuda, m, g, n=N):
    """logits and the stage-2 / stage-3 taps of the first n alerts with g alerts per workgroup"""
    kind, _, _, img, meta = case[:5]
    run_model(kind, m, img[:1].to(cuda), meta[:1].to(cuda))   # (the handle exists from the first forward on)
    set_alerts(m, g)
    logits = run_model(kind, m, img[:n].to(cuda), meta[:n].to(cuda)).cpu()
    return logits, m.read_tap("stage2").cpu().reshape(n, 9, 256), m.read_tap("stage3").cpu().reshape(n, 1, 512)


def stage2_errors(case, cuda, prec, g):
    kind, cfg, sd = case[:3]
    ref2, ref3 = case[6:]
    m = build_model(kind, cfg, sd, cuda, prec)
    assert m.schedule_flag("stage2p")   # the fused stage-2 launch, not the launch-by-launch path
    m.set_debug_taps(True)
    _, got2, got3 = forward(case, cuda, m, g)
    assert torch.isfinite(got2).all() and torch.isfinite(got3).all()
    d2 = (got2 - ref2).abs() / max(1.0, ref2.abs().max().item())
    d3 = (got3 - ref3).abs() / max(1.0, ref3.abs().max().item())
    figs = (d2.max(), d2[:, [0, 1, 3, 4]].max(), d2[:, [2, 5, 6, 7, 8]].max(), d2[8].max(), d3.max(), d3[8].max())
    return dict(zip(SLICES, (f.item() for f in figs)))


@pytest.mark.parametrize("g", [4, 5, 7])
@pytest.mark.parametrize("prec", ["bf16", "f16", "f16x2"])
def test_stage2_and_stage3_taps_against_oracle(cuda, case, prec, g):
    errs = stage2_errors(case, cuda, prec, g)
    print(f'    ("{prec}", {g}): (' + ", ".join(f"{errs[k]:.6e}" for k in SLICES) + "),")
    for what, bound in zip(SLICES, PARENT[(prec, g)]):
        assert errs[what] <= 1.25 * bound, f"{prec}, {g} alerts per workgroup, {what}: {errs[what]} > 1.25 x {bound}"


@pytest.mark.parametrize("g", [4, 5, 7])
def test_alert_is_independent_of_its_neighbours(cuda, case, g):
    """alert 0 alone and in front of eight others: column 0 of workgroup 0 both times"""
    kind, cfg, sd = case[:3]
    m = build_model(kind, cfg, sd, cuda, "bf16")
    m.set_debug_taps(True)
    nine = forward(case, cuda, m, g)
    one = forward(case, cuda, m, g, n=1)
    for a, b in zip(one, nine):
        assert torch.equal(a[0], b[0])


def test_logits_do_not_depend_on_alerts_per_workgroup(cuda, case):
    kind, cfg, sd = case[:3]
    m = build_model(kind, cfg, sd, cuda, "bf16")
    m.set_debug_taps(True)
    got = [forward(case, cuda, m, g)[0] for g in (4, 5, 7)]
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


@pytest.mark.parametrize("g", [4, 5, 7])
def test_fp8_is_finite_and_repeatable(cuda, case, g):
    """(its distance from the oracle is test_gpu_parity.py's)"""
    kind, cfg, sd = case[:3]
    m = build_model(kind, cfg, sd, cuda, "fp8")
    assert m.schedule_flag("stage2p")
    m.set_debug_taps(True)
    first, second = forward(case, cuda, m, g)[0], forward(case, cuda, m, g)[0]
    assert torch.isfinite(first).all() and torch.equal(first, second)


def test_keeping_form_runs_on_the_ragged_shape(cuda, case):
    """The training forward's instantiation on the nine alerts (5 / 4): one optimiser step gives a finite loss and finite
    gradients (after one AdamW step the first moment is 0.1 x the gradient).  The numbers are test_full_backward_16bit's."""
    from btsbot_amd.train import Trainer
    kind, cfg, sd, img, meta, labels = case[:6]
    m = build_model(kind, cfg, sd, cuda, "bf16").train()
    assert m.schedule_flag("s2_keep")
    tr = Trainer(m, lr=1e-4)
    loss = tr.step(img.to(cuda), meta.to(cuda), labels.to(cuda))
    assert torch.isfinite(loss).item()
    assert torch.isfinite(tr.exp_avg).all()
    for k, p in m.named_parameters():
        assert torch.isfinite(p).all(), k
