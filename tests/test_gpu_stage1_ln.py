"""stage1b's block LayerNorm (btsbot_amd/csrc/stage1b.hip): the depthwise outputs cross from lane = channel to
lane = pixel through one fp32 LDS image and are normalised in registers.  Three alerts are two workgroups: the first
holds two alerts (all 98 rows of the image, rows 93..97 among them), the second one alert (the ragged form), in each
16-bit mode, against the fp32 oracle's stage-1 activations.

Inputs: synthetic_batch(3, seed=11) with alert 1 shifted by a constant and a 16 x 16 pixel patch of alert 2 zeroed in
all three cutouts.  On the CPU the oracle's stage-1 taps for these inputs are finite with max|ref| = 5.742
(5.489 / 5.742 / 5.256 per alert).

Tolerance: the error is owned by the 16-bit operand rounding, which this change does not touch (fp32 statistics, the
normalised value rounded once); a re-ordered, two-pass fp32 sum moves last bits and may flip single 16-bit roundings.
So each mode is held to what the previous kernel (transposing lane reduction, single-pass variance, LayerNorm written
through a 16-bit image) measured on exactly these inputs, x 1.25:

  max|d| / max(1, max|ref|)      previous kernel      this kernel
  bf16                           5.396218e-03         5.396218e-03
  f16                            6.653125e-04         6.637179e-04
  f16x2                          1.438654e-05         1.442806e-05
(bf16: the same figure to every printed digit.)
"""
import pytest
import torch

from helpers import CONFIGS, seeded_state, build_model, run_model
from btsbot_amd.synthetic import synthetic_batch
from oracle import convnext_oracle as O   # checker only

pytestmark = pytest.mark.gpu

# measured on an MI355X with the kernel before this change (see the table above)
PARENT = {"bf16": 5.396218e-03, "f16": 6.653125e-04, "f16x2": 1.438654e-05}
NEW = {"bf16": 5.396218e-03, "f16": 6.637179e-04, "f16x2": 1.442806e-05}   # this kernel, for the record
TOL = {k: 1.25 * v for k, v in PARENT.items()}


def stress_inputs():
    img, meta, labels = synthetic_batch(3, seed=11)
    img = img.clone()
    img[1] += 0.5                        # pixel values are ~ 1/63 after the L2 normalisation
    img[2, :, 20:36, 20:36] = 0.0
    return img, meta, labels


@pytest.fixture(scope="module")
def case():
    kind, cfg = CONFIGS["mm_pico"]
    sd = seeded_state(kind, cfg, seed=3)
    img, meta, labels = stress_inputs()
    taps = {}
    with torch.no_grad():
        O.mm_convnext_forward(sd, cfg, img, meta, taps=taps)
    ref = taps["stage1"].permute(0, 2, 3, 1).reshape(3, 49, 128).contiguous()   # NCHW -> [alert][pixel][channel]
    assert torch.isfinite(ref).all() and 1.0 <= ref.abs().max().item() <= 100.0
    return kind, cfg, sd, img, meta, labels, ref


def stage1_error(case, cuda, prec):
    """max|d| / max(1, max|ref|) over the whole map and over the slices the image layout makes special"""
    kind, cfg, sd, img, meta, _, ref = case
    m = build_model(kind, cfg, sd, cuda, prec)
    m.set_debug_taps(True)
    run_model(kind, m, img.to(cuda), meta.to(cuda))
    got = m.read_tap("stage1").cpu().reshape(3, 49, 128)
    assert torch.isfinite(got).all()
    d = (got - ref).abs() / max(1.0, ref.abs().max().item())
    g = d.reshape(3, 7, 7, 128)
    return {"whole map": d.max().item(),
            "alert 1, last five pixels (image rows 93..97)": d[1, 44:].max().item(),
            "alert 0, pixel 48": d[0, 48].max().item(),
            "row 6": g[:, 6].max().item(),
            "column 6": g[:, :, 6].max().item(),
            "alert 2 (ragged workgroup)": d[2].max().item()}


@pytest.mark.parametrize("prec", ["bf16", "f16", "f16x2"])
def test_stage1_activations_all_pixels(cuda, case, prec):
    errs = stage1_error(case, cuda, prec)
    print(f"stage1 {prec}: " + "  ".join(f"{k} {v:.6e}" for k, v in errs.items()))
    for what, e in errs.items():
        assert e <= TOL[prec], f"{prec}, {what}: {e} > {TOL[prec]}"


def test_alert_is_independent_of_its_partner(cuda, case):
    """alert 0 alone (nal = 1) and beside alert 1 (nal = 2): workgroup 0 both times, so the same chunk rotation"""
    kind, cfg, sd, img, meta, _, _ = case
    m = build_model(kind, cfg, sd, cuda, "bf16")
    m.set_debug_taps(True)
    three = run_model(kind, m, img.to(cuda), meta.to(cuda)).cpu()
    tap3 = m.read_tap("stage1").cpu().reshape(3, 49, 128)
    one = run_model(kind, m, img[:1].to(cuda), meta[:1].to(cuda)).cpu()
    tap1 = m.read_tap("stage1").cpu().reshape(1, 49, 128)
    assert torch.equal(tap1[0], tap3[0])
    assert torch.equal(one[0], three[0])


def test_keeping_form_rows_match_inference(cuda, case, monkeypatch):
    """The training forward's instantiation (keep_xn stored from the registers that hold the LayerNorm output) at the
    ragged shape: one forward and backward on the three alerts must run and give a finite loss and finite gradients.
    Nothing is compared with the inference kernel here: the numbers are
    test_full_backward_16bit[...stage1_keeping_kernel...]'s."""
    monkeypatch.setenv("BTSBOT_AMD_S1_TRAIN", "1")
    kind, cfg, sd, img, meta, labels, _ = case
    m = build_model(kind, cfg, sd, cuda, "bf16").train()
    assert m.schedule_flag("s1_keep")
    logits = m(image_input=img.to(cuda), metadata_input=meta.to(cuda))
    loss = torch.nn.BCEWithLogitsLoss()(logits, labels.to(cuda).float().unsqueeze(1))
    loss.backward()
    assert torch.isfinite(loss).item()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
