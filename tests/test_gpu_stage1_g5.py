"""stage1b's form under the overlap hint (btsbot_amd/csrc/stage1b.hip, G = 5; btsbot_set_option "forwards_in_flight",
Schedule::s1_g5): five alerts' 245 pixels on the 256 pixel slots of an eight-wave workgroup.  Twelve alerts are workgroups
of 5, 5 and 2 (the ragged form), in each plain 16-bit mode, against the fp32 oracle's stage-1 activations and, bit for
bit, against the two-alert form a plain call runs; the smallest batches (1, 5, 6 alerts: one alert, a full workgroup,
full + 1), 519 alerts (104 workgroups, every alert's bits those of its first copy) and an fp8 handle (its stage 1 runs
the bf16 instantiation) against the oracle's scores.

Inputs: synthetic_batch(12, seed=11) with alert 4 (the last of workgroup 0: image rows 196..244) shifted by a constant and
a 16 x 16 pixel patch of alert 11 (the ragged workgroup) zeroed in all three cutouts.  On the CPU the oracle's stage-1
taps for these inputs are finite with max|ref| = 5.790 (alert 4; 5.26 .. 5.59 for the others).

Tolerance: the form changes which wave holds which pixel and channel group, and with it the previous kernel's chunk
rotation went (a workgroup walked the fc2 chunks in an order derived from its index; now every workgroup of both forms
adds them in the same order, which is what makes the two forms bit-equal); every product, its operands' roundings and
the fp32 statistics are the previous kernel's.  So each mode is held, over the whole map and over every slice below, to
what the previous kernel (two alerts per four-wave workgroup, rotation) measured over the whole map on exactly these
inputs, x 1.25 -- both libraries run in one job on an MI355X:

  max|d| / max(1, max|ref|)      previous kernel      this kernel
  bf16                           4.802566e-03         4.802566e-03
  f16                            8.009638e-04         8.129153e-04

and slice by slice (previous kernel / this kernel):
  bf16  position 0 in a workgroup                            4.802566e-03 / 4.802566e-03
  bf16  position 1 in a workgroup                            4.449545e-03 / 4.449545e-03
  bf16  position 2 in a workgroup                            4.462829e-03 / 4.462845e-03
  bf16  position 3 in a workgroup                            4.161042e-03 / 4.161084e-03
  bf16  position 4 in a workgroup                            4.494618e-03 / 4.494659e-03
  bf16  pixel 48                                             3.561205e-03 / 3.561205e-03
  bf16  row 6                                                4.075519e-03 / 4.075519e-03
  bf16  column 6                                             4.494618e-03 / 4.494659e-03
  bf16  image rows 240..244 (alerts 4, 9: last five pixels)  3.896000e-03 / 3.895995e-03
  bf16  alerts 10, 11 (ragged workgroup)                     4.325171e-03 / 4.325254e-03
  f16   position 0 in a workgroup                            7.021815e-04 / 7.021815e-04
  f16   position 1 in a workgroup                            6.900036e-04 / 7.329764e-04
  f16   position 2 in a workgroup                            8.009638e-04 / 8.129153e-04
  f16   position 3 in a workgroup                            6.424757e-04 / 6.410346e-04
  f16   position 4 in a workgroup                            7.084404e-04 / 7.084712e-04
  f16   pixel 48                                             6.523993e-04 / 6.623846e-04
  f16   row 6                                                6.921345e-04 / 6.930816e-04
  f16   column 6                                             6.523993e-04 / 6.623846e-04
  f16   image rows 240..244 (alerts 4, 9: last five pixels)  6.921345e-04 / 6.930816e-04
  f16   alerts 10, 11 (ragged workgroup)                     6.900036e-04 / 7.329764e-04
"""
import pytest
import torch

from helpers import CONFIGS, seeded_state, build_model, run_model
from test_gpu_parity import TOL_SCORE
from btsbot_amd import _lib
from btsbot_amd.synthetic import synthetic_batch
from oracle import convnext_oracle as O   # checker only

pytestmark = pytest.mark.gpu

NAL, G = 12, 5
# measured on an MI355X with the kernel before this change (see the table above)
PARENT = {"bf16": 4.802566e-03, "f16": 8.009638e-04}
NEW = {"bf16": 4.802566e-03, "f16": 8.129153e-04}   # this kernel, for the record
TOL = {k: 1.25 * v for k, v in PARENT.items()}


def stress_inputs():
    img, meta, labels = synthetic_batch(NAL, seed=11)
    img = img.clone()
    img[4] += 0.5                        # pixel values are ~ 1/63 after the L2 normalisation
    img[11, :, 20:36, 20:36] = 0.0
    return img, meta, labels


@pytest.fixture(scope="module")
def case():
    kind, cfg = CONFIGS["mm_pico"]
    sd = seeded_state(kind, cfg, seed=3)
    img, meta, _ = stress_inputs()
    taps = {}
    with torch.no_grad():
        logits = O.mm_convnext_forward(sd, cfg, img, meta, taps=taps)
    ref = taps["stage1"].permute(0, 2, 3, 1).reshape(NAL, 49, 128).contiguous()   # NCHW -> [alert][pixel][channel]
    assert torch.isfinite(ref).all() and 1.0 <= ref.abs().max().item() <= 100.0
    assert torch.isfinite(logits).all()
    return kind, cfg, sd, img, meta, ref, logits


@pytest.fixture(scope="module")
def models(cuda, case):
    """one handle per mode, shared by the tests of this file (the handle exists from the first forward on)"""
    kind, cfg, sd, img, meta = case[:5]
    made = {}

    def get(prec):
        if prec not in made:
            made[prec] = build_model(kind, cfg, sd, cuda, prec)
            run_model(kind, made[prec], img[:1].to(cuda), meta[:1].to(cuda))
        return made[prec]
    return get


def forward(case, m, cuda, idx, in_flight, taps=False):
    """logits (and the stage-1 tap) of alerts `idx` with the overlap hint set or not"""
    kind, cfg, sd, img, meta = case[:5]
    _lib.check(_lib.lib().btsbot_set_option(m._handle.ptr, b"forwards_in_flight", int(in_flight)), "btsbot_set_option")
    m.set_debug_taps(taps)
    try:
        out = run_model(kind, m, img[idx].to(cuda), meta[idx].to(cuda)).cpu()
        tap = m.read_tap("stage1").cpu().reshape(-1, 49, 128) if taps else None
    finally:
        m.set_debug_taps(False)
        _lib.lib().btsbot_set_option(m._handle.ptr, b"forwards_in_flight", 0)
    return out, tap


def stage1_error(case, m, cuda):
    """max|d| / max(1, max|ref|) over the whole map and over the slices the five-alert image makes special"""
    ref = case[5]
    _, got = forward(case, m, cuda, slice(None), True, taps=True)
    assert got.shape == ref.shape and torch.isfinite(got).all()
    d = (got - ref).abs() / max(1.0, ref.abs().max().item())
    g = d.reshape(NAL, 7, 7, 128)
    errs = {"whole map": d.max().item()}
    for pos in range(G):
        errs[f"position {pos} in a workgroup"] = d[pos::G].max().item()
    errs["pixel 48"] = d[:, 48].max().item()
    errs["row 6"] = g[:, 6].max().item()
    errs["column 6"] = g[:, :, 6].max().item()
    errs["image rows 240..244 (alerts 4, 9: last five pixels)"] = d[4::G, 44:].max().item()
    errs["alerts 10, 11 (ragged workgroup)"] = d[10:].max().item()
    return errs


def test_the_hint_selects_the_form(cuda, case, models):
    for prec, want in (("bf16", True), ("f16", True), ("fp8", True), ("f16x2", False)):
        m = models(prec)
        assert not m.schedule_flag("s1_g5"), prec
        assert _lib.lib().btsbot_set_option(m._handle.ptr, b"forwards_in_flight", 1) == _lib.OK
        try:
            assert m.schedule_flag("s1_g5") == want, prec
        finally:
            _lib.lib().btsbot_set_option(m._handle.ptr, b"forwards_in_flight", 0)
        assert not m.schedule_flag("s1_g5"), prec


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_stage1_activations_all_positions(cuda, case, models, prec):
    errs = stage1_error(case, models(prec), cuda)
    print(f"stage1 {prec}: " + "  ".join(f"{k} {v:.6e}" for k, v in errs.items()))
    for what, e in errs.items():
        assert e <= TOL[prec], f"{prec}, {what}: {e} > {TOL[prec]}"


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_five_alert_form_gives_the_two_alert_forms_bits(cuda, case, models, prec):
    """the hinted forward (workgroups of 5, 5, 2) against the plain one (six workgroups of 2): stage-1 map and logits"""
    m = models(prec)
    plain, tap2 = forward(case, m, cuda, slice(None), False, taps=True)
    hinted, tap5 = forward(case, m, cuda, slice(None), True, taps=True)
    assert torch.isfinite(tap5).all() and tap5.shape == (NAL, 49, 128)
    assert torch.equal(tap5, tap2)
    assert torch.equal(hinted, plain)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("nb", [1, 5, 6])
def test_smallest_batches_match_the_oracle(cuda, case, models, prec, nb):
    """nal = 1, one full workgroup, full + 1"""
    logits = case[6]
    out, _ = forward(case, models(prec), cuda, slice(0, nb), True)
    assert out.shape == logits[:nb].shape and torch.isfinite(out).all()
    ds = (torch.sigmoid(out) - torch.sigmoid(logits[:nb])).abs().max().item()
    print(f"{prec}, {nb} alerts: max|dscore| {ds:.3e}")
    assert ds <= TOL_SCORE[prec], f"{prec}, {nb} alerts: max|dscore| {ds}"


def test_alert_is_independent_of_its_partners(cuda, case, models):
    """alert 0 alone (nal = 1) and as the first of twelve; alerts 5..9 as a call of their own (workgroup 0) and as
    workgroup 1 of the twelve: the same bits, no sum depends on the workgroup index"""
    m = models("bf16")
    twelve, tap12 = forward(case, m, cuda, slice(None), True, taps=True)
    one, tap1 = forward(case, m, cuda, slice(0, 1), True, taps=True)
    five, tap5 = forward(case, m, cuda, slice(5, 10), True, taps=True)
    assert torch.equal(tap1[0], tap12[0]) and torch.equal(one[0], twelve[0])
    assert torch.equal(tap5, tap12[5:10]) and torch.equal(five, twelve[5:10])


def test_bits_do_not_depend_on_the_place_in_a_batch(cuda, case, models):
    """519 alerts = 104 workgroups, the twelve inputs over and over: every alert gives the bits of its first copy, whatever
    its workgroup and its position in it, hinted or not; every alert is within the score bound of the oracle"""
    logits = case[6]
    idx = torch.arange(519) % NAL
    m = models("bf16")
    out, _ = forward(case, m, cuda, idx, True)
    plain, _ = forward(case, m, cuda, idx, False)
    assert out.shape == (519, 1) and torch.isfinite(out).all()
    assert torch.equal(out, out[:NAL][idx]) and torch.equal(out, plain)
    ds = (torch.sigmoid(out) - torch.sigmoid(logits[idx])).abs().max().item()
    print(f"bf16, 519 alerts: max|dscore| {ds:.3e}")
    assert ds <= TOL_SCORE["bf16"], f"519 alerts: max|dscore| {ds}"


def test_fp8_handle_runs_this_form(cuda, case, models):
    """stage 1 of an fp8 handle is the bf16 instantiation: full workgroup + 1"""
    logits = case[6]
    out, _ = forward(case, models("fp8"), cuda, slice(0, 6), True)
    assert torch.isfinite(out).all()
    ds = (torch.sigmoid(out) - torch.sigmoid(logits[:6])).abs().max().item()
    print(f"fp8, 6 alerts: max|dscore| {ds:.3e}")
    assert ds <= TOL_SCORE["fp8"], f"fp8: max|dscore| {ds}"
