"""stage0b's block LayerNorm (btsbot_amd/csrc/stage0b.hip): the depthwise outputs cross from lane = channel to
lane = pixel through one fp32 LDS image and are normalised in registers.  Three alerts = three workgroups cover every
pixel slot of the kernel, in each 16-bit mode, against the fp32 oracle's stage-0 activations.

Inputs: synthetic_batch(3, seed=11) with alert 1 shifted by a constant (large mean against a small variance in front
of the stem) and a 16 x 16 pixel patch of alert 2 zeroed in all three cutouts (4 x 4 stem pixels whose channels are
the stem bias alone).  On the CPU the oracle's stage-0 taps for these inputs are finite with max|ref| = 5.51.

Tolerance: the error is owned by the 16-bit operand rounding, which this change does not touch (fp32 statistics, the
normalised value rounded once); a re-ordered fp32 sum moves last bits.  So each mode is held to what the previous
kernel (cross-wave single-pass LayerNorm through a 16-bit image) measured on exactly these inputs, x 1.25:

  max|d| / max(1, max|ref|)      previous kernel      this kernel
  bf16                           4.459596e-03         4.459596e-03
  f16                            6.725999e-04         6.725999e-04
  f16x2                          1.180683e-05         1.181764e-05
(bf16 / f16: the worst element is the same one, to every printed digit.)
"""
import pytest
import torch

from helpers import CONFIGS, seeded_state, build_model, run_model
from btsbot_amd.synthetic import synthetic_batch
from oracle import convnext_oracle as O   # checker only

pytestmark = pytest.mark.gpu

# measured on an MI355X with the kernel before this change (see the table above)
PARENT = {"bf16": 4.459596e-03, "f16": 6.725999e-04, "f16x2": 1.180683e-05}
NEW = {"bf16": 4.459596e-03, "f16": 6.725999e-04, "f16x2": 1.181764e-05}   # this kernel, for the record
TOL = {k: 1.25 * v for k, v in PARENT.items()}


def stress_inputs():
    img, meta, _ = synthetic_batch(3, seed=11)
    img = img.clone()
    img[1] += 0.5                        # pixel values are ~ 1/63 after the L2 normalisation
    img[2, :, 20:36, 20:36] = 0.0
    return img, meta


@pytest.fixture(scope="module")
def case():
    kind, cfg = CONFIGS["mm_pico"]
    sd = seeded_state(kind, cfg, seed=3)
    img, meta = stress_inputs()
    taps = {}
    with torch.no_grad():
        O.mm_convnext_forward(sd, cfg, img, meta, taps=taps)
    ref = taps["stage0"].permute(0, 2, 3, 1).reshape(3, 225, 64).contiguous()   # NCHW -> [alert][pixel][channel]
    assert torch.isfinite(ref).all() and 1.0 <= ref.abs().max().item() <= 100.0
    return kind, cfg, sd, img, meta, ref


def stage0_error(case, cuda, prec):
    """(whole map, pixel 224, row 14, column 14) of max|d| / max(1, max|ref|)"""
    kind, cfg, sd, img, meta, ref = case
    m = build_model(kind, cfg, sd, cuda, prec)
    m.set_debug_taps(True)
    run_model(kind, m, img.to(cuda), meta.to(cuda))
    got = m.read_tap("stage0").cpu().reshape(3, 225, 64)
    assert torch.isfinite(got).all()
    d = (got - ref).abs().reshape(3, 15, 15, 64) / max(1.0, ref.abs().max().item())
    return d.max().item(), d[:, 14, 14].max().item(), d[:, 14].max().item(), d[:, :, 14].max().item()


@pytest.mark.parametrize("prec", ["bf16", "f16", "f16x2"])
def test_stage0_activations_all_pixels(cuda, case, prec):
    whole, last, row14, col14 = stage0_error(case, cuda, prec)
    print(f"stage0 {prec}: max|d|/scale {whole:.4e}  pixel 224 {last:.4e}  row 14 {row14:.4e}  column 14 {col14:.4e}")
    assert whole <= TOL[prec], f"{prec}: {whole} > {TOL[prec]}"
    # the lone pixel of the eighth column block, and the last row / column (the padded depthwise tiles' edge)
    assert last <= TOL[prec] and row14 <= TOL[prec] and col14 <= TOL[prec]


def test_alert_is_independent_of_its_batch(cuda, case):
    kind, cfg, sd, img, meta, _ = case
    m = build_model(kind, cfg, sd, cuda, "bf16")
    three = run_model(kind, m, img.to(cuda), meta.to(cuda)).cpu()
    one = run_model(kind, m, img[:1].to(cuda), meta[:1].to(cuda)).cpu()
    assert torch.equal(one[0], three[0])
