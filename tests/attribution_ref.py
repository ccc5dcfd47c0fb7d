"""float64 restatement of btsbot_amd.attribution's methods, driven by autograd through the CPU oracle
(oracle/convnext_oracle.py).  Checker only: plain loops, one gradient call per sample or step."""
import torch

from oracle import convnext_oracle as O


def oracle_fns(kind, cfg, sd, target="logit", dtype=torch.float64):
    """(grad, value): grad(img, meta) -> (d_img, d_meta) of every alert's own f, value(img, meta) -> f [B]; f the eval-mode
    logit or score of the oracle in `dtype`.  Eval-mode rows are independent, so the gradient of sum_b f_b is per alert."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}

    def f(img, meta):
        out = O.forward(kind, sd, cfg, img, meta, training=False).reshape(-1)
        return torch.sigmoid(out) if target == "score" else out

    def prep(t):
        return None if t is None else t.detach().to("cpu", dtype)

    def value(img, meta):
        with torch.no_grad():
            return f(prep(img), prep(meta))

    def grad(img, meta):
        xs = [None if t is None else prep(t).requires_grad_(True) for t in (img, meta)]
        f(*xs).sum().backward()
        return tuple(None if x is None else x.grad for x in xs)

    return grad, value


def smoothgrad_ref(grad, img, meta, noises, noise_level):
    """noises: list of (noise_img, noise_meta) unit-normal draws; sigma = noise_level * range, per cutout (alert, channel)
    and per metadata column over the batch."""
    img = None if img is None else img.double()
    meta = None if meta is None else meta.double()
    si = None if img is None else noise_level * (img.amax(dim=(2, 3), keepdim=True) - img.amin(dim=(2, 3), keepdim=True))
    sm = None if meta is None else noise_level * (meta.amax(dim=0, keepdim=True) - meta.amin(dim=0, keepdim=True))
    acc = [None, None]
    for ni, nm in noises:
        g = grad(None if img is None else img + si * ni.double(), None if meta is None else meta + sm * nm.double())
        acc = [gi if a is None else (a if gi is None else a + gi) for a, gi in zip(acc, g)]
    return tuple(None if a is None else a / len(noises) for a in acc)


def integrated_gradients_ref(grad, value, img, meta, base_img, base_meta, steps):
    """Midpoint rule on the straight path; returns (attr_img, attr_meta, delta [B]) with
    delta = sum(attr) - (f(x) - f(baseline))."""
    xs = [None if t is None else t.double() for t in (img, meta)]
    bs = [None if x is None else b.double().expand_as(x) for x, b in zip(xs, (base_img, base_meta))]
    acc = [None if x is None else torch.zeros_like(x) for x in xs]
    for k in range(steps):
        a = (k + 0.5) / steps
        g = grad(*[None if x is None else b + a * (x - b) for x, b in zip(xs, bs)])
        acc = [None if c is None else c + gi for c, gi in zip(acc, g)]
    attr = [None if x is None else (x - b) * c / steps for x, b, c in zip(xs, bs, acc)]
    total = sum(t.flatten(1).sum(dim=1) for t in attr if t is not None)
    delta = total - (value(*xs) - value(*bs))
    return attr[0], attr[1], delta
