"""Host-side checks of btsbot_amd.attribution (no GPU): the argument checks of saliency(), and two properties of the
float64 oracle the GPU tests lean on -- the integrated-gradients completeness gap closes with the step count, and the
image gradient's rows / columns 60..62 are exactly zero (the 4x4 / stride-4 stem never reads them)."""
import pytest
import torch

import attribution_ref as R
from btsbot_amd import attribution
from btsbot_amd.synthetic import synthetic_batch
from helpers import CONFIGS, seeded_state


class _NoModel:
    """saliency() must refuse bad arguments before it touches the model."""

    def __getattr__(self, name):
        raise AssertionError(f"saliency touched model.{name} before it had checked its arguments")


def test_saliency_refuses_bad_arguments_before_touching_the_model():
    img, meta, _ = synthetic_batch(2, seed=1)
    m = _NoModel()
    with pytest.raises(ValueError, match="unknown method"):
        attribution.saliency(m, image_input=img, metadata_input=meta, method="lime")
    with pytest.raises(ValueError, match="unknown target"):
        attribution.saliency(m, image_input=img, metadata_input=meta, target="loss")
    with pytest.raises(ValueError, match="steps >= 1"):
        attribution.saliency(m, image_input=img, metadata_input=meta, method="integrated_gradients", steps=0)
    with pytest.raises(ValueError, match="n_samples >= 1"):
        attribution.saliency(m, image_input=img, metadata_input=meta, method="smoothgrad", n_samples=0)
    with pytest.raises(ValueError, match="image baseline must have shape"):
        attribution.saliency(m, image_input=img, metadata_input=meta, method="integrated_gradients",
                             baseline=(torch.zeros(3, 60, 60), None))
    with pytest.raises(ValueError, match="metadata baseline must have shape"):
        attribution.saliency(m, image_input=img, metadata_input=meta, method="integrated_gradients",
                             baseline=(None, torch.zeros(meta.shape[1] + 1)))
    with pytest.raises(ValueError, match="no image input"):
        attribution.saliency(m, metadata_input=meta, method="integrated_gradients", baseline=(torch.zeros(3, 63, 63), None))
    with pytest.raises(ValueError, match="belongs to integrated_gradients"):
        attribution.saliency(m, image_input=img, metadata_input=meta, method="gradient", baseline=(None, None))
    with pytest.raises(ValueError, match="return_delta"):
        attribution.saliency(m, image_input=img, metadata_input=meta, method="smoothgrad", return_delta=True)
    with pytest.raises(ValueError, match="no input tensor"):
        attribution.saliency(m)


def test_saliency_is_exported_with_its_methods():
    import btsbot_amd
    assert btsbot_amd.saliency is attribution.saliency and "saliency" in btsbot_amd.__all__
    assert attribution.METHODS == ("gradient", "gradient_x_input", "smoothgrad", "integrated_gradients")


def test_oracle_completeness_gap_shrinks_with_steps_and_border_is_zero():
    kind, cfg = CONFIGS["mm_pico"]
    sd = seeded_state(kind, cfg, seed=3)
    img, meta, _ = synthetic_batch(2, seed=4)
    grad, value = R.oracle_fns(kind, cfg, sd, "logit")
    gi, gm = grad(img, meta)
    assert gi.shape == (2, 3, 63, 63) and gm.shape == meta.shape
    assert gi.abs().max().item() > 0 and gm.abs().max().item() > 0
    assert (gi[:, :, 60:, :] == 0).all() and (gi[:, :, :, 60:] == 0).all()
    base_m = sd["metadata_branch.0.running_mean"]
    gaps = []
    for steps in (8, 64):
        _ai, _am, delta = R.integrated_gradients_ref(grad, value, img, meta, torch.zeros(3, 63, 63), base_m, steps)
        gaps.append(delta.abs().max().item())
    travel = (value(img, meta) - value(torch.zeros_like(img), base_m.expand_as(meta))).abs().max().item()
    print(f"completeness gap: {gaps[0]:.3e} at 8 steps, {gaps[1]:.3e} at 64 (f(x) - f(baseline) up to {travel:.3e})")
    assert gaps[1] < gaps[0]
    # (64 midpoints on a path along which the gradient changes by O(1) of itself: the quadrature error stays a small
    #  fraction of the integral; 1/20 is loose on purpose, the property under test is the line above)
    assert gaps[1] <= 0.05 * travel
