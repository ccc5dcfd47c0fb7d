"""Which pixels and which metadata columns moved this score: attribution maps on the input gradients of the HIP
backward (``model.input_gradients``: ``btsbot_forward_keep_eval`` + ``btsbot_backward_inputs``).

Everything here is torch ops on the device around that one call; nothing is read back to the host.  The methods:

``"gradient"``              d f / d x
``"gradient_x_input"``      x * d f / d x
``"smoothgrad"``            the mean gradient over ``n_samples`` noisy copies, x + sigma * N(0, 1), sigma = ``noise_level``
                            times the range (max - min) of each cutout -- per alert and channel -- and of each metadata
                            column over the batch (Smilkov et al. 2017)
``"integrated_gradients"``  (x - x0) times the mean gradient at ``steps`` midpoints of the straight path from the baseline
                            x0 to x (Sundararajan et al. 2017); completeness: sum(attr) = f(x) - f(x0) up to the
                            quadrature error, which ``return_delta=True`` reports per alert

f is the logit (``target="logit"``) or the score (``target="score"``).  ConvNeXt wirings and um_nn; eval mode only.
"""
from __future__ import annotations

import inspect
from typing import Optional, Tuple

import torch

METHODS = ("gradient", "gradient_x_input", "smoothgrad", "integrated_gradients")
TARGETS = ("logit", "score")


def _draw_noise(k: int, image: Optional[torch.Tensor], meta: Optional[torch.Tensor], generator=None):
    """Unit normal noise of SmoothGrad's draw ``k``, shaped like the inputs (``None`` for a missing one).  The one place
    noise comes from: a test plants its own draws by replacing this function."""
    def one(t):
        return None if t is None else torch.randn(t.shape, dtype=t.dtype, device=t.device, generator=generator)
    return one(image), one(meta)


def _call_kwargs(model, image, meta):
    """The inputs under the names this model's ``forward`` takes."""
    names = inspect.signature(model.forward).parameters
    if "input_data" in names:
        return {"input_data": image if image is not None else meta}
    return {"image_input": image, "metadata_input": meta}


def _grads(model, image, meta, target, batch_size):
    return model.input_gradients(target=target, batch_size=batch_size, **_call_kwargs(model, image, meta))


def _value(model, image, meta, target):
    """f of every alert, [B], as the deployed forward computes it."""
    with torch.no_grad():
        logits = model(**_call_kwargs(model, image, meta)).reshape(-1)
    return torch.sigmoid(logits) if target == "score" else logits


def _check_baseline(name, base, ref):
    if base is None or ref is None:
        if base is not None:
            raise ValueError(f"saliency: a {name} baseline was given, but there is no {name} input")
        return None
    base = torch.as_tensor(base, dtype=ref.dtype, device=ref.device)
    if tuple(base.shape) not in (tuple(ref.shape), tuple(ref.shape[1:])):
        raise ValueError(f"saliency: the {name} baseline must have shape {tuple(ref.shape)} or {tuple(ref.shape[1:])}, "
                         f"got {tuple(base.shape)}")
    return base.expand_as(ref)


def saliency(model, image_input: Optional[torch.Tensor] = None, metadata_input: Optional[torch.Tensor] = None,
             method: str = "gradient", target: str = "logit", *, n_samples: int = 16, noise_level: float = 0.1,
             steps: int = 32, baseline: Optional[Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = None,
             return_delta: bool = False, batch_size: int = 1024, generator=None):
    """``(image_attr [B,3,63,63], meta_attr [B,n_meta])`` for every alert of the batch (``None`` for an input the wiring
    lacks; pass only the inputs it has).  ``method`` is one of ``METHODS``, ``target`` one of ``TARGETS`` (module
    docstring).  ``baseline=(image_baseline, meta_baseline)`` (integrated gradients; each ``None`` or of the input's shape,
    with or without the batch dimension) defaults to zero triplets and the metadata BatchNorm's ``running_mean`` -- the
    input the branch maps to its bias.  ``return_delta=True`` (integrated gradients) appends the completeness gap
    ``sum(attr) - (f(x) - f(baseline))`` per alert, ``[B]``, computed on the device."""
    if method not in METHODS:
        raise ValueError(f"saliency: unknown method {method!r} (have {list(METHODS)})")
    if target not in TARGETS:
        raise ValueError(f"saliency: unknown target {target!r} (have {list(TARGETS)})")
    if image_input is None and metadata_input is None:
        raise ValueError("saliency: no input tensor")
    if method == "smoothgrad" and (int(n_samples) < 1 or not float(noise_level) >= 0.0):
        raise ValueError("saliency: smoothgrad needs n_samples >= 1 and noise_level >= 0")
    if method == "integrated_gradients" and int(steps) < 1:
        raise ValueError("saliency: integrated_gradients needs steps >= 1")
    if return_delta and method != "integrated_gradients":
        raise ValueError("saliency: return_delta is the completeness gap of integrated_gradients")
    if baseline is not None and method != "integrated_gradients":
        raise ValueError("saliency: a baseline belongs to integrated_gradients")
    img = image_input.detach().to(torch.float32) if image_input is not None else None
    meta = metadata_input.detach().to(torch.float32) if metadata_input is not None else None
    base_i, base_m = (None, None) if baseline is None else baseline
    base_i, base_m = _check_baseline("image", base_i, img), _check_baseline("metadata", base_m, meta)

    if method in ("gradient", "gradient_x_input"):
        gi, gm = _grads(model, img, meta, target, batch_size)
        if method == "gradient_x_input":
            gi = gi * img if gi is not None else None
            gm = gm * meta if gm is not None else None
        return gi, gm

    if method == "smoothgrad":
        si = noise_level * (img.amax(dim=(2, 3), keepdim=True) - img.amin(dim=(2, 3), keepdim=True)) if img is not None else None
        sm = noise_level * (meta.amax(dim=0, keepdim=True) - meta.amin(dim=0, keepdim=True)) if meta is not None else None
        acc_i = torch.zeros_like(img) if img is not None else None
        acc_m = torch.zeros_like(meta) if meta is not None else None
        for k in range(int(n_samples)):
            ni, nm = _draw_noise(k, img, meta, generator)
            gi, gm = _grads(model, img + si * ni if img is not None else None, meta + sm * nm if meta is not None else None,
                            target, batch_size)
            if acc_i is not None:
                acc_i += gi
            if acc_m is not None:
                acc_m += gm
        return (acc_i / n_samples if acc_i is not None else None, acc_m / n_samples if acc_m is not None else None)

    # integrated gradients, midpoint rule
    if img is not None and base_i is None:
        base_i = torch.zeros_like(img)
    if meta is not None and base_m is None:
        base_m = model.metadata_running_mean().to(device=meta.device, dtype=meta.dtype).expand_as(meta)
    acc_i = torch.zeros_like(img) if img is not None else None
    acc_m = torch.zeros_like(meta) if meta is not None else None
    for k in range(int(steps)):
        a = (k + 0.5) / int(steps)
        gi, gm = _grads(model, base_i + a * (img - base_i) if img is not None else None,
                        base_m + a * (meta - base_m) if meta is not None else None, target, batch_size)
        if acc_i is not None:
            acc_i += gi
        if acc_m is not None:
            acc_m += gm
    attr_i = (img - base_i) * acc_i / int(steps) if img is not None else None
    attr_m = (meta - base_m) * acc_m / int(steps) if meta is not None else None
    if not return_delta:
        return attr_i, attr_m
    total = sum(t.flatten(1).sum(dim=1) for t in (attr_i, attr_m) if t is not None)
    fx = _value(model, img, meta, target)
    f0 = _value(model, base_i.contiguous() if base_i is not None else None,
                base_m.contiguous() if base_m is not None else None, target)
    return attr_i, attr_m, total - (fx - f0)
