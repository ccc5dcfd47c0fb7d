"""Input gradients of the ConvNeXt wirings on the GPU: the stem's input-gradient kernel and the BatchNorm input-gradient
kernel alone against float64, the autograd path in eval and train mode against autograd through the CPU oracle, the
16-bit modes, independence of the alerts of an eval call, repeatability, model.input_gradients / saliency against the
float64 restatement (tests/attribution_ref.py), and the C ABI of btsbot_backward_inputs.

Error measure of a gradient: per alert, max |got - ref| over the alert's entries relative to the alert's largest |ref|.
fp32 bound 5e-4: the project's fp32 gradient bound (tests/test_gpu_train.py)."""
import ctypes as C
import functools

import pytest
import torch

import attribution_ref as R
from btsbot_amd import _lib, attribution, ops
from btsbot_amd.synthetic import synthetic_batch
from helpers import CONFIGS, MV_CONFIGS, build_model, run_model, seeded_state, seeded_state_mv
from oracle import convnext_oracle as O   # checker only

pytestmark = pytest.mark.gpu

F32_BOUND = 5e-4
U = 2.0 ** -24


def _per_alert_err(got, ref):
    got, ref = got.detach().cpu().double().flatten(1), ref.detach().cpu().double().flatten(1)
    scale = ref.abs().amax(dim=1).clamp_min(1e-30)
    return ((got - ref).abs().amax(dim=1) / scale).max().item()


def _call(kind, m, img, meta):
    if kind in ("mm_ConvNeXt", "frozen_fusion", "mm_MaxViT"):
        return m(image_input=img, metadata_input=meta)
    return m(input_data=img if kind in ("ConvNeXt", "MaxViT") else meta)


def _inputs(kind, B, seed, dev=None, grad=False):
    img, meta, labels = synthetic_batch(B, seed=seed)
    img = None if kind == "um_nn" else img
    meta = None if kind == "ConvNeXt" else meta
    if dev is not None:
        img, meta = (None if t is None else t.to(dev).requires_grad_(grad) for t in (img, meta))
    return img, meta, labels


@functools.lru_cache(maxsize=None)
def _oracle_eval_grads(name, B, seed=4):
    """fp32 oracle, eval form: (logits, d_img, d_meta) of sum_b logit_b.  Computed once per case, never modified."""
    kind, cfg = CONFIGS[name]
    sd = seeded_state(kind, cfg, seed=3)
    img, meta, _ = _inputs(kind, B, seed)
    xs = [None if t is None else t.clone().requires_grad_(True) for t in (img, meta)]
    logits = O.forward(kind, sd, cfg, xs[0], xs[1], training=False)
    logits.sum().backward()
    return (logits.detach(),) + tuple(None if x is None else x.grad for x in xs)


# ---------------------------------------------------------------------------------------------------------------------
# 1. stem_dgrad alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C0", [64, 80])
@pytest.mark.parametrize("B", [1, 3])
def test_stem_dgrad_alone(cuda, B, C0):
    g = torch.Generator().manual_seed(100 * B + C0)
    dxn = torch.randn(B, 15, 15, C0, generator=g)
    w = torch.randn(C0, 3, 4, 4, generator=g)
    out = torch.full((B, 3, 63, 63), float("nan"), device=cuda)
    ops.cnt_stem_dgrad(dxn.to(cuda), w.to(cuda), out)
    got = out.cpu()
    assert not torch.isnan(got).any(), "an element was never written"
    # rows and columns 60..62: the stem never reads them -- exactly zero
    assert (got[:, :, 60:, :] == 0).all() and (got[:, :, :, 60:] == 0).all()
    ref = torch.einsum("bijo,ocuv->bciujv", dxn.double(), w.double()).reshape(B, 3, 60, 60)
    mag = torch.einsum("bijo,ocuv->bciujv", dxn.double().abs(), w.double().abs()).reshape(B, 3, 60, 60)
    err = (got[:, :, :60, :60].double() - ref).abs()
    bound = (C0 + 1) * U * mag          # a chain of C0 fused multiply-adds in fp32 + the final rounding
    print(f"stem_dgrad B={B} C0={C0}: worst error / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the BatchNorm kernels alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 257])
def test_bn_input_gradient_kernel_alone(cuda, M):
    n = 25
    g = torch.Generator().manual_seed(M)
    x, dy = torch.randn(M, n, generator=g) * 2 + 0.5, torch.randn(M, n, generator=g)
    w, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    rm, rv = torch.randn(n, generator=g), torch.rand(n, generator=g) + 0.1
    d = lambda t: t.to(cuda)
    e = lambda *s: torch.full(s, float("nan"), device=cuda)

    # eval form: forward on the running statistics, then dx = dy * w * rstd
    xhat, out, rstd = ops.ht_bn_eval_fwd(d(x), d(w), d(b), d(rm), d(rv), e(M, n), e(M, n), e(n))
    r64 = 1.0 / torch.sqrt(rv.double() + 1e-5)
    xh64 = (x.double() - rm.double()) * r64
    assert ((rstd.cpu().double() - r64).abs() <= 4 * U * r64).all()
    assert ((xhat.cpu().double() - xh64).abs() <= 8 * U * (x.double().abs() + rm.double().abs()) * r64).all()
    o64 = xh64 * w.double() + b.double()
    assert ((out.cpu().double() - o64).abs() <= 12 * U * ((x.double().abs() + rm.double().abs()) * r64 * w.double().abs()
                                                           + b.double().abs())).all()
    dx = ops.ht_bn_bwd_in(d(dy), d(w), xhat, rstd, e(M, n), eval=True)
    ref = dy.double() * w.double() * rstd.cpu().double()      # (on the kernel's own fp32 rstd: this kernel alone)
    assert not torch.isnan(dx).any()
    assert ((dx.cpu().double() - ref).abs() <= 4 * U * ref.abs()).all()

    # batch-statistics form, behind bn_fwd and bn_bwd (whose two column sums it reads)
    xhat, out, rstd = ops.ht_bn_fwd(d(x), d(w), d(b), e(M, n), e(M, n), e(n))
    dw, db = ops.ht_bn_bwd(d(dy), d(w), xhat, rstd, e(n), e(n))
    dx = ops.ht_bn_bwd_in(d(dy), d(w), xhat, rstd, e(M, n), sum_dy=db, sum_dyx=dw)
    assert not torch.isnan(dx).any()
    xh, rs, dy64, w64 = xhat.cpu().double(), rstd.cpu().double(), dy.double(), w.double()
    s, q = dy64.sum(0), (dy64 * xh).sum(0)
    gain = (w64 * rs).abs() / M
    ref = (w64 * rs / M) * (M * dy64 - s - xh * q)
    # the kernel's sums carry a chain of at most M + 8 fp32 additions each; the combination a handful of roundings
    bound = gain * ((M + 8) * U * (dy64.abs().sum(0) + xh.abs() * (dy64 * xh).abs().sum(0))
                    + 8 * U * (M * dy64.abs() + s.abs() + (xh * q).abs()))
    err = (dx.cpu().double() - ref).abs()
    print(f"bn_bwd_in M={M}: worst error / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= bound).all()
    if M == 1:
        assert (dx == 0).all()      # one row: xhat = 0 and dy - sum(dy) = 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. eval mode, f32: logits.sum().backward() leaves the oracle's gradients on the inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mm_pico", "convnext", "mm_nano_ls", "frozen_fusion", "um_nn"])
def test_eval_mode_input_gradients_f32(cuda, name):
    kind, cfg = CONFIGS[name]
    B = 6
    sd = seeded_state(kind, cfg, seed=3)
    m = build_model(kind, cfg, sd, cuda, "f32")
    img, meta, _ = _inputs(kind, B, 4, cuda, grad=True)
    logits = _call(kind, m, img, meta)
    logits.sum().backward()
    ref_logits, ref_di, ref_dm = _oracle_eval_grads(name, B)
    assert (logits.detach().cpu() - ref_logits).abs().max().item() <= 1e-4 * max(1.0, ref_logits.abs().max().item())
    worst = 0.0
    for what, x, ref in (("image", img, ref_di), ("metadata", meta, ref_dm)):
        if x is None:
            continue
        assert x.grad is not None, f"{what}.grad is None"
        assert x.grad.shape == x.shape
        err = _per_alert_err(x.grad, ref)
        worst = max(worst, err)
        assert err <= F32_BOUND, f"{what}: per-alert relative error {err:.3e}"
    if img is not None:
        assert (img.grad[:, :, 60:, :] == 0).all() and (img.grad[:, :, :, 60:] == 0).all()
    print(f"{name}: worst per-alert relative input-gradient error {worst:.2e}")
    assert all(p.grad is None for p in m.parameters()), "an eval-mode backward left a parameter gradient"
    # under no_grad the call is the plain scoring call, whatever the inputs require
    with torch.no_grad():
        again = _call(kind, m, img, meta)
    plain = run_model(kind, m, None if img is None else img.detach(), None if meta is None else meta.detach())
    assert not again.requires_grad and torch.equal(again, plain)


# ---------------------------------------------------------------------------------------------------------------------
# 4. train mode, f32: batch statistics + planted dropout, parameters and inputs together
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mm_pico", "frozen_fusion"])
def test_train_mode_input_and_parameter_gradients_f32(cuda, name):
    kind, cfg = CONFIGS[name]
    B = 6
    sd = seeded_state(kind, cfg, seed=3)
    mcfg = cfg["meta_model_config"] if kind == "frozen_fusion" else cfg
    g = torch.Generator().manual_seed(9)
    masks = {"meta": (torch.rand(B, mcfg["meta_fc1_neurons"], generator=g) >= mcfg["meta_dropout"]).float(),
             "comb": (torch.rand(B, cfg["comb_fc2_neurons"], generator=g) >= cfg["comb_dropout"]).float()}
    m = build_model(kind, cfg, sd, cuda, "f32").train()
    m._forced_masks = {k: v.to(torch.uint8) for k, v in masks.items()}
    trainable = [k for k, _p in m.named_parameters()]
    img, meta, labels = _inputs(kind, B, 4, cuda, grad=True)
    lossf = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([2.0], device=cuda))
    lossf(m(image_input=img, metadata_input=meta), labels.to(cuda).float().unsqueeze(1)).backward()

    osd = {k: v.clone() for k, v in sd.items()}
    for k in trainable:
        osd[k].requires_grad_(True)
    cimg, cmeta, _ = _inputs(kind, B, 4)
    cimg, cmeta = cimg.requires_grad_(True), cmeta.requires_grad_(True)
    O.bce_with_logits(O.forward(kind, osd, cfg, cimg, cmeta, training=True, masks=masks),
                      labels.float().unsqueeze(1), 2.0).backward()
    e_img, e_meta = _per_alert_err(img.grad, cimg.grad), _per_alert_err(meta.grad, cmeta.grad)
    print(f"{name} (train): per-alert relative error image {e_img:.2e}, metadata {e_meta:.2e}")
    assert e_img <= F32_BOUND and e_meta <= F32_BOUND
    got = dict(m.named_parameters())
    worst = 0.0
    for k in trainable:
        assert got[k].grad is not None, k
        a, b = got[k].grad.cpu().double(), osd[k].grad.double()
        err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-7)
        worst = max(worst, err)
        assert err <= F32_BOUND, f"grad {k}: rel err {err:.3e}"
    print(f"{name} (train): worst relative parameter-gradient error {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# 5. 16-bit modes, default schedule, eval form
# ---------------------------------------------------------------------------------------------------------------------
# prec: (measured on the MI355X -- mm_pico, B = 24, batch seed 4, the larger of image and metadata --, bound = twice that).
# Both bounds lie below the project's 16-bit parameter-gradient bounds (test_full_backward_16bit: bf16 4.5e-2, f16 8e-3).
BOUND_16 = {"bf16": (1.373e-2, 2.75e-2), "f16": (1.989e-3, 3.98e-3)}


def _eval_grads_16(cuda, prec, B=24, seed=4):
    kind, cfg = CONFIGS["mm_pico"]
    m = build_model(kind, cfg, seeded_state(kind, cfg, seed=3), cuda, prec)
    img, meta, _ = _inputs(kind, B, seed, cuda, grad=True)
    _call(kind, m, img, meta).sum().backward()
    return img.grad, meta.grad


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_eval_mode_input_gradients_16bit(cuda, prec):
    di, dm = _eval_grads_16(cuda, prec)
    _l, ref_di, ref_dm = _oracle_eval_grads("mm_pico", 24)
    e_img, e_meta = _per_alert_err(di, ref_di), _per_alert_err(dm, ref_dm)
    print(f"{prec}: per-alert relative error against the fp32 oracle: image {e_img:.3e}, metadata {e_meta:.3e}")
    measured, bound = BOUND_16[prec]
    assert bound is not None, "the 16-bit bound has not been measured"
    assert max(e_img, e_meta) <= bound, (prec, e_img, e_meta, measured, bound)


def test_eval_mode_input_gradients_f16x2_meets_the_f32_bound(cuda):
    di, dm = _eval_grads_16(cuda, "f16x2")
    _l, ref_di, ref_dm = _oracle_eval_grads("mm_pico", 24)
    e_img, e_meta = _per_alert_err(di, ref_di), _per_alert_err(dm, ref_dm)
    print(f"f16x2: per-alert relative error image {e_img:.3e}, metadata {e_meta:.3e}")
    assert e_img <= F32_BOUND and e_meta <= F32_BOUND


# ---------------------------------------------------------------------------------------------------------------------
# 6. independence of the alerts of an eval call, and repeatability
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_alerts_are_independent_and_calls_repeat(cuda, prec):
    kind, cfg = CONFIGS["mm_pico"]
    m = build_model(kind, cfg, seeded_state(kind, cfg, seed=3), cuda, prec)
    img, meta, _ = _inputs(kind, 7, 4, cuda)
    di, dm = m.input_gradients(image_input=img, metadata_input=meta)
    di2, dm2 = m.input_gradients(image_input=img, metadata_input=meta)
    assert torch.equal(di, di2) and torch.equal(dm, dm2), "the same call twice gave different bits"
    bound = F32_BOUND if prec == "f32" else BOUND_16[prec][1]
    assert bound is not None
    for a in (0, 6):
        oi, om = m.input_gradients(image_input=img[a:a + 1], metadata_input=meta[a:a + 1])
        e_img, e_meta = _per_alert_err(di[a:a + 1], oi), _per_alert_err(dm[a:a + 1], om)
        print(f"{prec} alert {a}: alone vs in a call of 7: image {e_img:.2e} (bits equal: {torch.equal(di[a:a + 1], oi)}), "
              f"metadata {e_meta:.2e} (bits equal: {torch.equal(dm[a:a + 1], om)})")
        assert e_img <= bound and e_meta <= bound


# ---------------------------------------------------------------------------------------------------------------------
# 7. model.input_gradients and saliency
# ---------------------------------------------------------------------------------------------------------------------
def test_input_gradients_targets_and_chunks(cuda):
    kind, cfg = CONFIGS["mm_pico"]
    m = build_model(kind, cfg, seeded_state(kind, cfg, seed=3), cuda, "f32")
    img, meta, _ = _inputs(kind, 10, 4, cuda)
    before = [p.grad for p in m.parameters()]
    li, lm = m.input_gradients(image_input=img, metadata_input=meta)
    si, sm = m.input_gradients(image_input=img, metadata_input=meta, target="score")
    s = torch.sigmoid(run_model(kind, m, img, meta)).double().cpu()
    f = (s * (1 - s))
    assert _per_alert_err(si, li.cpu().double() * f.view(-1, 1, 1, 1)) <= F32_BOUND
    assert _per_alert_err(sm, lm.cpu().double() * f.view(-1, 1)) <= F32_BOUND
    ci, cm = m.input_gradients(image_input=img, metadata_input=meta, batch_size=4)   # chunks of 4, 4, 2
    assert _per_alert_err(ci, li) <= F32_BOUND and _per_alert_err(cm, lm) <= F32_BOUND
    assert all(p.grad is b for p, b in zip(m.parameters(), before)) and all(b is None for b in before)
    _l, ref_di, ref_dm = _oracle_eval_grads("mm_pico", 10)
    assert _per_alert_err(li, ref_di) <= F32_BOUND and _per_alert_err(lm, ref_dm) <= F32_BOUND
    with pytest.raises(RuntimeError, match="eval mode only"):
        m.train().input_gradients(image_input=img, metadata_input=meta)
    m.eval()
    with pytest.raises(ValueError, match="target"):
        m.input_gradients(image_input=img, metadata_input=meta, target="loss")


def test_maxvit_input_gradients_are_refused(cuda):
    kind, cfg = MV_CONFIGS["maxvit"]
    m = build_model(kind, cfg, seeded_state_mv(kind, cfg, seed=3), cuda, "f32")
    img, _meta, _ = synthetic_batch(2, seed=4)
    with pytest.raises(NotImplementedError, match="MaxViT"):
        m.input_gradients(input_data=img.to(cuda))
    with pytest.raises(NotImplementedError, match="MaxViT"):
        attribution.saliency(m, image_input=img.to(cuda))


def test_saliency_methods_against_the_float64_restatement(cuda, monkeypatch):
    kind, cfg = CONFIGS["mm_pico"]
    sd = seeded_state(kind, cfg, seed=3)
    m = build_model(kind, cfg, sd, cuda, "f32")
    B = 3
    cimg, cmeta, _ = _inputs(kind, B, 4)
    img, meta = cimg.to(cuda), cmeta.to(cuda)
    grad, value = R.oracle_fns(kind, cfg, sd, "logit")

    gi, gm = attribution.saliency(m, image_input=img, metadata_input=meta, method="gradient")
    ri, rm_ = grad(cimg, cmeta)
    assert _per_alert_err(gi, ri) <= F32_BOUND and _per_alert_err(gm, rm_) <= F32_BOUND
    xi, xm = attribution.saliency(m, image_input=img, metadata_input=meta, method="gradient_x_input")
    assert _per_alert_err(xi, ri * cimg.double()) <= F32_BOUND and _per_alert_err(xm, rm_ * cmeta.double()) <= F32_BOUND

    # SmoothGrad with planted noise, n = 3
    g = torch.Generator().manual_seed(11)
    noises = [(torch.randn(cimg.shape, generator=g), torch.randn(cmeta.shape, generator=g)) for _ in range(3)]
    monkeypatch.setattr(attribution, "_draw_noise", lambda k, i, mt, gen=None: (noises[k][0].to(i.device), noises[k][1].to(mt.device)))
    si, sm = attribution.saliency(m, image_input=img, metadata_input=meta, method="smoothgrad", n_samples=3, noise_level=0.1)
    ri, rm_ = R.smoothgrad_ref(grad, cimg, cmeta, noises, 0.1)
    e = max(_per_alert_err(si, ri), _per_alert_err(sm, rm_))
    print(f"smoothgrad (n = 3): per-alert relative error {e:.2e}")
    assert e <= 3 * F32_BOUND

    # integrated gradients, 8 midpoints, the default baseline; the completeness gap from the device
    steps = 8
    ii, im, delta = attribution.saliency(m, image_input=img, metadata_input=meta, method="integrated_gradients", steps=steps,
                                         return_delta=True)
    ri, rm_, rdelta = R.integrated_gradients_ref(grad, value, cimg, cmeta, torch.zeros(3, 63, 63),
                                                 sd["metadata_branch.0.running_mean"], steps)
    e = max(_per_alert_err(ii, ri), _per_alert_err(im, rm_))
    print(f"integrated gradients ({steps} steps): per-alert relative error {e:.2e}")
    assert e <= steps * F32_BOUND
    # the gap is a difference of sums: its error is measured against the sums' own size, sum |attr| per alert
    size = ri.abs().flatten(1).sum(1) + rm_.abs().flatten(1).sum(1)
    gap_err = ((delta.cpu().double() - rdelta).abs() / size).max().item()
    print(f"completeness gap: device {delta.cpu().tolist()}, reference {rdelta.tolist()}, error / sum|attr| {gap_err:.2e}")
    assert gap_err <= steps * F32_BOUND
    # a caller's baseline is taken as given
    bi, bm = torch.full((3, 63, 63), 0.1), cmeta.mean(0)
    ii, im = attribution.saliency(m, image_input=img, metadata_input=meta, method="integrated_gradients", steps=2,
                                  baseline=(bi.to(cuda), bm.to(cuda)))
    ri, rm_, _d = R.integrated_gradients_ref(grad, value, cimg, cmeta, bi, bm, 2)
    assert max(_per_alert_err(ii, ri), _per_alert_err(im, rm_)) <= 2 * F32_BOUND


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _raw_backward_inputs(m, dlogits, need_meta, need_image, d_img, d_meta):
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    stream = torch.cuda.current_stream(m._arena.device).cuda_stream
    return _lib.lib().btsbot_backward_inputs(m._handle.ptr, p(dlogits), p(m._grad_arena), int(need_meta), int(need_image),
                                             p(d_img), p(d_meta), C.c_void_p(stream))


def test_backward_inputs_with_null_outputs_is_backward(cuda):
    kind, cfg = CONFIGS["mm_pico"]
    m = build_model(kind, cfg, seeded_state(kind, cfg, seed=3), cuda, "f32").train()
    B = 6
    img, meta, _ = _inputs(kind, B, 4, cuda)
    masks = m._dropout_masks(B, cuda)
    dl = torch.linspace(-1, 1, B, device=cuda)
    with torch.no_grad():
        m._forward_train_raw(img, meta, masks, keep_image=True)
        a = m._backward_raw(dl, True, True).clone()
        assert _raw_backward_inputs(m, dl, 1, 1, None, None) == _lib.OK
        b = m._grad_arena.clone()
    scale = a.abs().max().item()
    assert scale > 0 and (a - b).abs().max().item() <= F32_BOUND * scale


def test_backward_inputs_error_paths(cuda):
    """Every refusal comes before the first launch."""
    dl = torch.ones(2, device=cuda)
    buf = torch.zeros(2 * 3 * 63 * 63, device=cuda)
    L = _lib.lib()

    def model(table, name, state):
        kind, cfg = table[name]
        m = build_model(kind, cfg, state(kind, cfg, seed=3), cuda, "f32")
        object.__setattr__(m, "_grad_arena", torch.zeros_like(m._arena))
        return kind, m

    kind, m = model(MV_CONFIGS, "mm_maxvit", seeded_state_mv)
    assert _raw_backward_inputs(m, dl, 0, 0, None, buf) == _lib.ERR_INVALID_ARG
    assert b"MaxViT" in L.btsbot_last_error()
    assert _raw_backward_inputs(m, dl, 0, 0, buf, None) == _lib.ERR_INVALID_ARG
    kind, m = model(CONFIGS, "um_nn", seeded_state)
    assert _raw_backward_inputs(m, dl, 0, 0, buf, None) == _lib.ERR_INVALID_ARG
    assert b"no image input" in L.btsbot_last_error()
    kind, m = model(CONFIGS, "convnext", seeded_state)
    assert _raw_backward_inputs(m, dl, 0, 0, None, buf) == _lib.ERR_INVALID_ARG
    assert b"no metadata input" in L.btsbot_last_error()
    # no keeping forward at all, then one that kept no image activations
    kind, m = model(CONFIGS, "mm_pico", seeded_state)
    assert _raw_backward_inputs(m, dl, 0, 0, buf, None) == _lib.ERR_STATE
    img, meta, _ = _inputs(kind, 2, 4, cuda)
    with torch.no_grad():
        m._forward_keep_eval_raw(img, meta, keep_image=False)
    assert _raw_backward_inputs(m, dl, 0, 0, buf, None) == _lib.ERR_STATE
    assert b"keep_image_activations" in L.btsbot_last_error()
    assert _raw_backward_inputs(m, None, 0, 0, buf, None) == _lib.ERR_INVALID_ARG
    # the metadata input alone needs no kept image activations
    d_meta = torch.full_like(meta, float("nan"))
    assert _raw_backward_inputs(m, dl, 0, 0, None, d_meta) == _lib.OK
    _l, _di, ref_dm = _oracle_eval_grads("mm_pico", 2)
    assert _per_alert_err(d_meta, ref_dm) <= F32_BOUND
    # ... and the eval-form forward itself refuses a MaxViT handle
    kind, m = model(MV_CONFIGS, "maxvit", seeded_state_mv)
    logits = torch.zeros(2, device=cuda)
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    rc = L.btsbot_forward_keep_eval(m._handle.ptr, p(buf), p(None), p(logits), p(None), 2, 0,
                                    C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream))
    assert rc == _lib.ERR_INVALID_ARG
