"""Split-operand training (btsbot_set_option "train_split" / ``set_split_training``): f16x2 ConvNeXt handles run the
training step's fc1 / fc2 / downsample products -- forward, input gradients, filter gradients -- on f16 head + remainder
operands (gemm_x2.hip's training epilogues, wgrad_x2.hip), gradient operands scaled by a power of two per tensor.  The
yardstick throughout is the fp32 training schedule: the split mode must be as accurate as it."""
import math
import os
import warnings

import numpy as np
import pytest
import torch

from helpers import CONFIGS, MV_CONFIGS, seeded_state, build_model, run_model
from btsbot_amd import _lib, ops
from btsbot_amd.synthetic import synthetic_batch
from btsbot_amd.train import Trainer
from oracle import convnext_oracle as O   # checker only

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = -1, -5


def _opt(m, key, value=0):
    return _lib.lib().btsbot_set_option(m._handle.ptr, key, value)


def _new(kind, cfg, prec):
    import btsbot_amd
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return getattr(btsbot_amd, kind)(cfg, precision=prec)


def build_split(kind, cfg, sd, device):
    m = _new(kind, cfg, "f16x2")
    m.set_split_training(True)
    m.load_state_dict(sd)
    return m.to(device).eval()


# ---- 1. option contract -------------------------------------------------------------------------------------------
def test_train_split_option_contract(cuda):
    kind, cfg = CONFIGS["mm_pico"]
    m = _new(kind, cfg, "f16x2")
    assert _opt(m, b"query_train_split") == ERR_STATE
    assert _opt(m, b"train_split", 2) == ERR_INVALID_ARG
    assert _opt(m, b"train_split", 1) == _lib.OK
    assert _opt(m, b"query_train_split") == _lib.OK
    for k, c, prec in (("mm_ConvNeXt", cfg, "bf16"), ("mm_ConvNeXt", cfg, "f32"), (*MV_CONFIGS["mm_maxvit"], "f16x2"),
                       (*CONFIGS["um_nn"], "f16x2")):
        other = _new(k, c, prec)
        assert _opt(other, b"train_split", 1) == ERR_INVALID_ARG, (k, prec)
        assert _opt(other, b"query_train_split") == ERR_STATE, (k, prec)
        del other
    # after the first pack the layout is fixed
    sd = seeded_state(kind, cfg, seed=3)
    p = build_model(kind, cfg, sd, cuda, "f16x2")
    img, meta, _ = synthetic_batch(4, seed=1)
    run_model(kind, p, img.to(cuda), meta.to(cuda))
    assert _opt(p, b"train_split", 1) == ERR_STATE
    assert _opt(p, b"query_train_split") == ERR_STATE
    # Python
    with pytest.raises(ValueError):
        _new(kind, cfg, "bf16").set_split_training(True)
    with pytest.raises(ValueError):
        _new(*MV_CONFIGS["mm_maxvit"], "f16x2").set_split_training(True)
    q = build_split(kind, cfg, sd, cuda)
    assert q.split_training and _opt(q, b"query_train_split") == _lib.OK
    run_model(kind, q, img.to(cuda), meta.to(cuda))
    q.set_split_training(False)                      # re-creates the handle
    assert not q.split_training and _opt(q, b"query_train_split") == ERR_STATE
    q.set_split_training(True)
    q.set_precision("f32")
    assert not q.split_training


# ---- 2. op level against float64 ---------------------------------------------------------------------------------
WIDTHS = (64, 128, 256, 512, 80, 160, 320, 640)
BIG_M = 230400      # stage 0 of a 1024-alert batch (1024 x 225 pixels)
MID_M = 5400 + 13   # 24 alerts at stage 0, plus a ragged remainder


def _ms(c):
    return (1, MID_M, BIG_M) if c in (64, 80) else (1, MID_M)


def _grad_like(M, K, mag, g):
    """Signed values spanning 8 decades below `mag`."""
    e = torch.rand(M, K, generator=g, dtype=torch.float64) * -8.0
    s = torch.where(torch.rand(M, K, generator=g) < 0.5, -1.0, 1.0).double()
    return (s * mag * 10.0 ** e).float()


def _gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


@pytest.mark.timeout(900)
def test_split_training_epilogues_match_float64(cuda):
    g = torch.Generator().manual_seed(11)
    worst = {}
    for c in WIDTHS:
        # (N, K) of the products: fc1 (4C, C), fc2^T-dgrad (C, 4C), downsample dgrad (4 Cin, Cout = 2 Cin)
        for epi, N, K in (("gelu_save", 4 * c, c), ("dgelu", 4 * c, c), ("plain", c, 4 * c), ("plain", 2 * c, c)):
            if c in (64, 80) and (N, K) == (2 * c, c):   # (stage 0 has no downsample in front of it)
                continue
            w = (torch.randn(N, K, generator=g) * 0.05).to(cuda)
            b = (torch.randn(N, generator=g) * 0.1).to(cuda)
            w64, b64 = w.double(), b.double()
            for M in _ms(c):
                mags = (1.0,) if epi == "gelu_save" else (1.0, 1e-6, 1e-9)
                for mag in mags:
                    if epi == "gelu_save":
                        x = torch.randn(M, K, generator=g).to(cuda)
                    else:
                        x = _grad_like(M, K, mag, g).to(cuda)
                    ref = x.double() @ w64.t()
                    if epi == "gelu_save":
                        pre = torch.empty(M, N, device=cuda)
                        got = ops.gemm(x, w, b, "gelu_save", resid=pre, precision="f16x2")
                        ref_pre = ref + b64
                        errs = [((pre.double() - ref_pre).abs().max() / ref_pre.abs().max()).item()]
                        ref = 0.5 * ref_pre * (1.0 + torch.erf(ref_pre / math.sqrt(2.0)))
                    elif epi == "dgelu":
                        pre = torch.randn(M, N, generator=g).to(cuda)
                        got = ops.gemm(x, w, None, "dgelu", resid=pre, precision="f16x2")
                        ref = ref * _gelu_grad64(pre.double())
                        errs = []
                    else:
                        got = ops.gemm(x, w, None, "plain", precision="f16x2")
                        errs = []
                    torch.cuda.synchronize()
                    assert torch.isfinite(got).all(), (epi, N, K, M, mag)
                    errs.append(((got.double() - ref).abs().max() / ref.abs().max()).item())
                    e = max(errs)
                    key = (epi, N, K, M, mag)
                    worst[key] = e
                    assert e <= 2.5e-6, (key, e)
                    del x, got, ref
            torch.cuda.empty_cache()
    k = max(worst, key=worst.get)
    print(f"split epilogues: worst |err| / max|ref| {worst[k]:.2e} at {k}")


@pytest.mark.timeout(900)
def test_split_filter_gradient_matches_float64(cuda):
    """btsbot_op_wgrad(BTSBOT_F16X2) against float64: at most 2x the fp32 kernel's error on the same inputs + 1e-7 of
    max|ref| (the reduction over thousands of rows costs the fp32 summation more than the split's operand rounding; a
    single row, an outer product without reduction, is held to the split products' 2.5e-6).  Gradient operands at 1, 1e-6
    and 1e-9: unscaled, the heads of the last would be f16 subnormals.  The stem's shape (K = 48) with raw-pixel-like A
    up to 1e5: unscaled, A's heads would overflow f16 (the A-operand scale only the stem uses in the step)."""
    g = torch.Generator().manual_seed(12)
    worst = (0.0, None)
    shapes = []
    for c in WIDTHS:
        shapes += [(c, 4 * c, c), (4 * c, c, c)]         # fc2 (dy^T h), fc1 (da^T xn)
        if c not in (64, 80):
            shapes.append((c, 2 * c, c))                  # downsample: Cout x 4 Cin, Cin = C / 2
    shapes += [(64, 48, 64), (80, 48, 80)]                # the stem: C0 x (3 x 4 x 4) patches
    for N, K, c in shapes:
        for M in _ms(c):
            for mag in (1.0, 1e-6, 1e-9):
                d = _grad_like(M, N, mag, g).to(cuda)
                if K == 48:   # raw pixel values: offsets and spread far above f16's range
                    a = (torch.rand(M, K, generator=g) * 1e5 + torch.randn(M, K, generator=g) * 3e3).to(cuda)
                else:
                    a = torch.randn(M, K, generator=g).to(cuda)
                ref = d.double().t() @ a.double()
                cs_ref = d.double().sum(0)
                cs = torch.zeros(N, device=cuda)
                got = ops.wgrad(d, a, colsum=cs, precision="f16x2")
                f32 = ops.wgrad(d, a, precision="f32")
                torch.cuda.synchronize()
                scale = ref.abs().max().item()
                e_x2 = (got.double() - ref).abs().max().item() / scale
                e_32 = (f32.double() - ref).abs().max().item() / scale
                e_cs = (cs.double() - cs_ref).abs().max().item() / cs_ref.abs().max().item()
                key = (N, K, M, mag)
                assert torch.isfinite(got).all(), key
                if M > 1:
                    assert e_x2 <= 2.0 * e_32 + 1e-7, (key, e_x2, e_32)
                else:   # (one row: no reduction, each output a single product -- the split operands' 22 significant
                    #    bits against fp32's 24 show, held to the split products' bound of the epilogue test above)
                    assert e_x2 <= 2.5e-6, (key, e_x2, e_32)
                assert e_cs <= 1e-5, (key, e_cs)
                if e_x2 > worst[0]:
                    worst = (e_x2, (key, e_32))
                del d, a, ref, got, f32
        torch.cuda.empty_cache()
    print(f"split filter gradient: worst |err| / max|ref| {worst[0]:.2e} at {worst[1][0]} (fp32 there {worst[1][1]:.2e})")


def test_training_epilogues_refuse_what_they_cannot_run(cuda):
    """The training epilogues take fp32 tensors ('f32' / 'f16x2') and need resid for the pre-activation: refused
    before anything is launched otherwise, in Python and in btsbot_op_gemm for every precision."""
    x = torch.randn(64, 32, device=cuda)
    w = torch.randn(16, 32, device=cuda)
    for prec in ("bf16", "f16"):
        with pytest.raises(ValueError):
            ops.gemm(x.to(ops._DT[prec]), w.to(ops._DT[prec]), None, "plain", precision=prec)
    for prec in ("f32", "f16x2"):
        for epi in ("gelu_save", "dgelu"):
            with pytest.raises(ValueError):
                ops.gemm(x, w, torch.zeros(16, device=cuda), epi, precision=prec)
        assert ops.gemm(x, w, None, "plain", precision=prec).dtype == torch.float32
    out = torch.empty(64, 16, device=cuda)
    b = torch.zeros(16, device=cuda)
    p = ops._p
    for prec in ("f32", "bf16", "f16", "f16x2"):
        for epi in ("gelu_save", "dgelu"):
            rc = _lib.lib().btsbot_op_gemm(_lib.PRECISION[prec], ops._EPI[epi], p(x), p(w), p(b), p(None), p(None), p(out),
                                           64, 16, 32, ops._stream(x))
            assert rc == ERR_INVALID_ARG, (prec, epi, rc)
    torch.cuda.synchronize()


# ---- 3. gradients against autograd --------------------------------------------------------------------------------
def _masks(kind, cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "ConvNeXt":
        return {"comb": (torch.rand(B, cfg["fc2_neurons"], generator=g) >= cfg["dropout"]).float()}
    m = {"meta": (torch.rand(B, cfg["meta_fc1_neurons"], generator=g) >= cfg["meta_dropout"]).float()}
    m["comb"] = (torch.rand(B, cfg["comb_fc2_neurons"], generator=g) >= cfg["comb_dropout"]).float()
    return m


def _oracle_grads(kind, cfg, sd, img, meta, labels, masks, trainable):
    sd = {k: v.clone() for k, v in sd.items()}
    for k in trainable:
        sd[k].requires_grad_(True)
    logits = O.forward(kind, sd, cfg, img, meta, training=True, masks=masks)
    O.bce_with_logits(logits, labels.float().unsqueeze(1), 2.0).backward()
    return {k: sd[k].grad.double() for k in trainable}


def _model_grads(m, kind, img, meta, labels, masks, cuda):
    m = m.train()
    m._forced_masks = {k: v.to(torch.uint8) for k, v in masks.items()}
    if kind == "ConvNeXt":
        logits = m(input_data=img.to(cuda))
    else:
        logits = m(image_input=img.to(cuda), metadata_input=meta.to(cuda))
    loss = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([2.0], device=cuda))(
        logits, labels.to(cuda).float().unsqueeze(1))
    loss.backward()
    return {k: p.grad.detach().cpu().double() for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", ["mm_pico", "convnext", "mm_nano_ls"])
def test_split_training_gradients_match_autograd(cuda, name):
    kind, cfg = CONFIGS[name]
    sd = seeded_state(kind, cfg, seed=3)
    B = 24
    img, meta, labels = synthetic_batch(B, seed=4)
    masks = _masks(kind, cfg, B, seed=9)
    got = _model_grads(build_split(kind, cfg, sd, cuda), kind, img, meta, labels, masks, cuda)
    omasks = {"head": masks["comb"]} if kind == "ConvNeXt" else masks
    ref = _oracle_grads(kind, cfg, sd, img, meta, labels, omasks, list(got))
    worst, worst_k = 0.0, ""
    for k, a in got.items():
        assert torch.isfinite(a).all(), k
        b = ref[k]
        err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-7)
        if err > worst:
            worst, worst_k = err, k
        assert err <= 5e-4, (k, err)
    print(f"{name} split: worst relative gradient error {worst:.2e} ({worst_k})")


# ---- 4. as accurate as f32 at the full batch ------------------------------------------------------------------------
FULL_BATCH_CLASSES = ("gamma", "norm.bias", "conv_dw.bias", "")


@pytest.mark.timeout(900)
def test_split_training_at_the_full_batch_is_as_accurate_as_f32(cuda, monkeypatch):
    """pico at B = 1024, both handles with the deterministic reductions: every gradient of the split handle within 2x
    the f32 handle's error against autograd through the fp32 oracle (+ 1e-5 of the tensor's largest entry)."""
    monkeypatch.setenv("BTSBOT_AMD_DETERMINISTIC", "1")   # (read when a handle is created: both below)
    kind, cfg = CONFIGS["mm_pico"]
    sd = seeded_state(kind, cfg, seed=3)
    B = 1024
    img, meta, labels = synthetic_batch(B, seed=4)
    masks = _masks(kind, cfg, B, seed=9)
    g_x2 = _model_grads(build_split(kind, cfg, sd, cuda), kind, img, meta, labels, masks, cuda)
    torch.cuda.empty_cache()
    g_32 = _model_grads(build_model(kind, cfg, sd, cuda, "f32"), kind, img, meta, labels, masks, cuda)
    nthr = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    try:
        ref = _oracle_grads(kind, cfg, sd, img, meta, labels, masks, list(g_x2))
    finally:
        torch.set_num_threads(nthr)
    worst = {}
    for k, b in ref.items():
        scale = max(b.abs().max().item(), 1e-12)
        e_x2 = (g_x2[k] - b).abs().max().item() / scale
        e_32 = (g_32[k] - b).abs().max().item() / scale
        cls = next(c for c in FULL_BATCH_CLASSES if c in k)
        if e_x2 > worst.get(cls, (0.0,))[0]:
            worst[cls] = (e_x2, e_32, k)
        assert e_x2 <= 2.0 * e_32 + 1e-5, (k, e_x2, e_32)
    print("split vs f32 at B=1024, worst per class: " +
          "; ".join(f"{c or 'other'} {a:.2e} (f32 {b:.2e}, {k})" for c, (a, b, k) in worst.items()))


# ---- 5. trajectory --------------------------------------------------------------------------------------------------
def _learnable_batches(n_batches, B):
    g = torch.Generator().manual_seed(77)
    probe = torch.randn(25, generator=g)
    out = []
    for t in range(n_batches):
        img, meta, _ = synthetic_batch(B, seed=100 + t)
        z = (meta - meta.mean(0)) / (meta.std(0) + 1e-6)
        peak = img[:, 2, 29:34, 29:34].mean((1, 2))
        lab = ((z @ probe) / 5.0 + (peak - peak.median()) / (peak.std() + 1e-9) > 0).long()
        out.append((img, meta, lab))
    return out


@pytest.mark.timeout(900)
def test_split_training_follows_the_fp32_recipe(cuda):
    """The fifty-step problem of test_16bit_training_follows_the_fp32_recipe (tests/test_gpu_train.py), run with an f32
    handle and with a split handle: the split handle's loss curve and final parameters stay as close to the host fp32
    recipe as the f32 handle's do (Trainer.step with the option on)."""
    kind, cfg0 = CONFIGS["mm_pico"]
    cfg = dict(cfg0, meta_dropout=0.0, comb_dropout=0.0)
    sd0 = seeded_state(kind, cfg, seed=3, gamma=0.3)
    steps, B, lr, betas, pw = 50, 64, 1e-4, (0.9, 0.999), 1.5
    two = _learnable_batches(2, B)
    batches = [two[t % 2] for t in range(steps)]
    sd = {k: v.clone() for k, v in sd0.items()}
    params = [k for k in sd if "running_" not in k and "num_batches" not in k]
    for k in params:
        sd[k].requires_grad_(True)
    opt = torch.optim.AdamW([sd[k] for k in params], lr=lr, betas=betas)
    ref_loss = []
    nthr = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    try:
        for img, meta, lab in batches:
            opt.zero_grad()
            loss = O.bce_with_logits(O.forward(kind, sd, cfg, img, meta, training=True, masks={}),
                                     lab.float().unsqueeze(1), pw)
            loss.backward()
            opt.step()
            ref_loss.append(loss.item())
    finally:
        torch.set_num_threads(nthr)
    ref_loss = np.array(ref_loss)
    dbatches = [tuple(t.to(cuda) for t in b) for b in two]

    def run(m):
        tr = Trainer(m.train(), lr=lr, betas=betas, pos_weight=pw)
        tr.lrs = [lr]
        got = np.array(torch.stack([tr.step(*dbatches[t % 2]) for t in range(steps)]).cpu().tolist())
        trained = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
        num = sum(((trained[k] - sd[k].detach().double()) ** 2).sum().item() for k in params)
        den = sum(((sd[k].detach().double() - sd0[k].double()) ** 2).sum().item() for k in params)
        return got, np.abs(got - ref_loss).max(), math.sqrt(num / den)

    l32, d32, p32 = run(build_model(kind, cfg, sd0, cuda, "f32"))
    m = build_split(kind, cfg, sd0, cuda)
    lx2, dx2, px2 = run(m)
    assert m.split_training and _opt(m, b"query_train_split") == _lib.OK
    print(f"trajectory: worst |dloss| f32 {d32:.3e} split {dx2:.3e}; parameter drift f32 {p32:.3e} split {px2:.3e}")
    assert ref_loss[-3:].mean() < 0.25 * ref_loss[0]
    assert l32[-3:].mean() < 0.25 * l32[0] and lx2[-3:].mean() < 0.25 * lx2[0]
    assert dx2 <= 2.0 * d32 + 1e-3, (dx2, d32)
    assert px2 <= 1.5 * p32 + 1e-3, (px2, p32)


# ---- 6. determinism -------------------------------------------------------------------------------------------------
def test_split_training_deterministic_gradients(cuda, monkeypatch):
    kind, cfg0 = CONFIGS["mm_pico"]
    cfg = dict(cfg0, meta_dropout=0.0, comb_dropout=0.0)
    sd = seeded_state(kind, cfg, seed=3)
    img, meta, lab = synthetic_batch(160, seed=4)
    img, meta, lab = img.to(cuda), meta.to(cuda), lab.to(cuda)
    monkeypatch.setenv("BTSBOT_AMD_DETERMINISTIC", "1")
    m = build_split(kind, cfg, sd, cuda).train()
    tr = Trainer(m, lr=1e-4)
    out = []
    for _ in range(2):
        _l, g = tr.gradients(img, meta, lab)
        torch.cuda.synchronize()
        out.append(g.clone())
    assert torch.isfinite(out[0]).all()
    assert torch.equal(out[0], out[1]), (out[0] - out[1]).abs().max().item()


# ---- 7. nothing else moved ------------------------------------------------------------------------------------------
def test_split_training_leaves_inference_and_the_default_path_alone(cuda):
    kind, cfg0 = CONFIGS["mm_pico"]
    cfg = dict(cfg0, meta_dropout=0.0, comb_dropout=0.0)
    sd = seeded_state(kind, cfg, seed=3)
    img, meta, lab = synthetic_batch(96, seed=5)
    img, meta, lab = img.to(cuda), meta.to(cuda), lab.to(cuda)
    # a few split Trainer steps, then eval(): the scores of a fresh f16x2 model with the trained weights, bit for bit
    m = build_split(kind, cfg, sd, cuda).train()
    tr = Trainer(m, lr=1e-3)
    losses = [tr.step(img, meta, lab).item() for _ in range(3)]
    assert all(math.isfinite(v) for v in losses)
    m.eval()
    got = run_model(kind, m, img, meta)
    fresh = build_model(kind, cfg, {k: v.detach().cpu() for k, v in m.state_dict().items()}, cuda, "f16x2")
    assert torch.equal(got, run_model(kind, fresh, img, meta))
    # an f16x2 handle WITHOUT the option trains on the fp32 engine: the f32 handle's gradients, to the order in which
    # the fp32 filter-gradient kernel's slices meet through atomics (two f32 handles differ by as much)
    def grads(prec):
        mm = build_model(kind, cfg, sd, cuda, prec).train()
        _l, g = Trainer(mm, lr=1e-4).gradients(img, meta, lab)
        torch.cuda.synchronize()
        assert _opt(mm, b"query_train_split") == ERR_STATE
        return g.clone()
    a, b, c = grads("f32"), grads("f32"), grads("f16x2")
    scale = a.abs().max().item()
    noise = (a - b).abs().max().item()
    assert (c - a).abs().max().item() <= 4.0 * noise + 1e-6 * scale, ((c - a).abs().max().item(), noise)
