"""Split-operand (f16x2) inference of the MaxViT wirings: every matrix product of the forward on gemm_x2.hip (fp32 maps
split into f16 head + remainder, three f16 MFMAs per product), everything else on the fp32 schedule.  Op level against
float64, model level against the oracle and the reference wrapper's goldens at the north star's 1e-4, the schedule
query, batch handling, and the heads' gradients over a frozen branch."""
import os

import numpy as np
import pytest
import torch

from helpers import MV_CONFIGS, seeded_state_mv, build_model, run_model
from btsbot_amd import _lib, ops
from btsbot_amd.synthetic import synthetic_batch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NORTH_STAR = 1e-4        # |dscore| bound of the f16x2 mode (tests/test_gpu_parity.py TOL_SCORE)
LOGIT_REL = 4.5e-4       # |dlogit| <= LOGIT_REL * max(1, max|logit|) (tests/test_gpu_parity.py TOL_LOGIT_REL)

# (N, K) of every GEMM the MaxViT forward runs: stem conv1 / conv2, shortcut, conv1 / conv3, qkv, proj, fc1 / fc2
MV_SHAPES = [(32, 32), (64, 288), (256, 64), (64, 256), (192, 64), (512, 128), (128, 512), (1024, 256),
             (256, 1024), (2048, 512), (512, 2048)]
OP_TOL = 2.5e-6          # op level: |out - ref| <= OP_TOL * max|ref| (measured worst 1.35e-6, K = 2048)


def _split_query(m):
    return _lib.lib().btsbot_set_option(m._handle.ptr, b"query_maxvit_split", 0)


def _oracle(kind, cfg, sd, img, meta):
    from oracle import maxvit_oracle as MO
    with torch.no_grad():
        return MO.forward(kind, sd, cfg, img, meta)


def _check(out, ref):
    out = out.cpu()
    assert out.shape == ref.shape and out.dtype == torch.float32 and torch.isfinite(out).all()
    ds = (torch.sigmoid(out) - torch.sigmoid(ref)).abs().max().item()
    dl = (out - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    assert ds <= NORTH_STAR, f"max|dscore| {ds}"
    assert dl <= LOGIT_REL * scale, f"max|dlogit| {dl} (scale {scale})"
    return ds, dl / scale


def _epi_ref(pre, epi, resid):
    if epi == "gelu":
        return torch.nn.functional.gelu(pre)
    if epi == "silu":
        return torch.nn.functional.silu(pre)
    if epi == "resid":
        return resid + pre
    return pre


@pytest.mark.parametrize("N,K", MV_SHAPES)
def test_gemm_x2_matches_float64_on_maxvit_shapes(cuda, N, K):
    g = torch.Generator().manual_seed(N * 7 + K)
    worst = {}
    for M in (1, 49, 6007):
        x = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) / K ** 0.5
        b = torch.randn(N, generator=g) * 0.1
        gamma = torch.ones(N)
        r = torch.randn(M, N, generator=g)
        pre = x.double() @ w.double().t() + b.double()
        xd, wd, bd, gd = x.to(cuda), w.to(cuda), b.to(cuda), gamma.to(cuda)
        for epi in ("bias", "bias_t", "silu", "gelu", "resid"):
            if epi == "resid":   # in place: resid aliases out
                y = r.to(cuda)
                got = ops.gemm(xd, wd, bd, "resid", gamma=gd, resid=y, precision="f16x2", out=y)
                assert got.data_ptr() == y.data_ptr()
            else:
                got = ops.gemm(xd, wd, bd, epi, precision="f16x2")
            ref = _epi_ref(pre, epi, r.double())
            assert got.dtype == torch.float32 and got.shape == (M, N)
            err = (got.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
            worst[(M, epi)] = err
            assert err <= OP_TOL, f"M={M} N={N} K={K} {epi}: {err:.3e}"
    print(f"gemm_x2 N={N} K={K}: worst |err| / max|ref| = {max(worst.values()):.3e}")


def test_gemm_x2_rejects_what_it_cannot_run(cuda):
    x = torch.randn(8, 12, device=cuda)
    w = torch.randn(16, 12, device=cuda)
    b = torch.zeros(16, device=cuda)
    with pytest.raises(_lib.BtsbotHipError):     # K % 8 != 0
        ops.gemm(x, w, b, "bias", precision="f16x2")


@pytest.mark.parametrize("name", ["mm_maxvit", "maxvit", "frozen_fusion_maxvit"])
def test_maxvit_f16x2_matches_oracle_and_goldens(cuda, name):
    kind, cfg = MV_CONFIGS[name]
    sd = seeded_state_mv(kind, cfg, seed=3)
    m = build_model(kind, cfg, sd, cuda, "f16x2")
    assert _split_query(m) == _lib.OK
    img, meta, _ = synthetic_batch(5, seed=2)
    ds, dl = _check(run_model(kind, m, img.to(cuda), meta.to(cuda)), _oracle(kind, cfg, sd, img, meta))
    print(f"{name} f16x2 vs oracle: max|dscore| {ds:.3e}, max|dlogit| / scale {dl:.3e}")
    gold = np.load(os.path.join(GOLD, "ref_logits_maxvit.npz"))
    ex = np.load(os.path.join(GOLD, "example8.npz"))
    gi = torch.from_numpy(ex["triplets"][[0, 1, 4, 5]]).to(cuda)
    gm = torch.from_numpy(ex["metadata"][[0, 1, 4, 5]]).to(cuda)
    ds, dl = _check(run_model(kind, m, gi, gm), torch.from_numpy(gold[f"{name}/example4"]))
    print(f"{name} f16x2 vs reference wrapper goldens: max|dscore| {ds:.3e}, max|dlogit| / scale {dl:.3e}")


def test_mm_maxvit_f16x2_north_star_over_seeds(cuda):
    kind, cfg = MV_CONFIGS["mm_maxvit"]
    errs = []
    for seed in range(5):
        sd = seeded_state_mv(kind, cfg, seed=11 + seed)
        img, meta, _ = synthetic_batch(8, seed=20 + seed)
        m = build_model(kind, cfg, sd, cuda, "f16x2")
        out = run_model(kind, m, img.to(cuda), meta.to(cuda)).cpu()
        ref = _oracle(kind, cfg, sd, img, meta)
        errs.append((torch.sigmoid(out) - torch.sigmoid(ref)).abs().max().item())
        print(f"seed {11 + seed}: max|dscore| {errs[-1]:.3e}")
        del m
    assert max(errs) <= NORTH_STAR, errs


def test_query_maxvit_split(cuda):
    kind, cfg = MV_CONFIGS["mm_maxvit"]
    sd = seeded_state_mv(kind, cfg, seed=3)
    for prec, want in (("f16x2", _lib.OK), ("f32", None), ("bf16", None)):
        m = build_model(kind, cfg, sd, cuda, prec)
        rc = _split_query(m)
        assert (rc == _lib.OK) if want == _lib.OK else (rc != _lib.OK), (prec, rc)
        del m
    from helpers import CONFIGS, seeded_state
    pk, pcfg = CONFIGS["mm_pico"]
    m = build_model(pk, pcfg, seeded_state(pk, pcfg, seed=3), cuda, "f16x2")
    assert _split_query(m) != _lib.OK   # a ConvNeXt branch has no MaxViT GEMMs


def test_maxvit_f16x2_batch_handling(cuda):
    kind, cfg = MV_CONFIGS["mm_maxvit"]
    sd = seeded_state_mv(kind, cfg, seed=3)
    img, meta, _ = synthetic_batch(10, seed=4)
    img, meta = img.to(cuda), meta.to(cuda)
    m = build_model(kind, cfg, sd, cuda, "f16x2")
    full = run_model(kind, m, img, meta)
    perm = torch.randperm(10, generator=torch.Generator().manual_seed(0)).to(cuda)
    assert torch.equal(run_model(kind, m, img[perm].contiguous(), meta[perm].contiguous()), full[perm])
    m2 = build_model(kind, cfg, sd, cuda, "f16x2")
    m2._max_chunk = 4
    assert torch.equal(run_model(kind, m2, img, meta), full)
    assert torch.equal(run_model(kind, m, img[:1].contiguous(), meta[:1].contiguous()), full[:1])
    assert run_model(kind, m, img[:0], meta[:0]).shape == (0, 1)


def test_heads_gradients_over_a_frozen_f16x2_maxvit_branch(cuda):
    """One Trainer gradient pass of frozen_fusion over a frozen, eval-mode MaxViT branch (what train.py trains): the
    combined head's gradients in an f16x2 handle, whose branch features come from the split-operand forward, against
    an f32 handle's."""
    from btsbot_amd.train import Trainer
    kind, cfg = MV_CONFIGS["frozen_fusion_maxvit"]
    sd = seeded_state_mv(kind, cfg, seed=3)
    B = 8
    img, meta, labels = synthetic_batch(B, seed=6)
    gen = torch.Generator().manual_seed(9)
    masks = {"meta": (torch.rand(B, cfg["meta_model_config"]["meta_fc1_neurons"], generator=gen) >= 0.25),
             "comb": (torch.rand(B, cfg["comb_fc2_neurons"], generator=gen) >= 0.1)}
    grads = {}
    for prec in ("f32", "f16x2"):
        m = build_model(kind, cfg, sd, cuda, prec).train()
        m._forced_masks = {k: v.to(torch.uint8) for k, v in masks.items()}
        for p in list(m.image_branch.parameters()) + list(m.meta_branch.parameters()):
            p.requires_grad_(False)
        for mod in m._image_bn_modules():
            mod.eval()
        tr = Trainer(m, lr=1e-3, pos_weight=1.5)
        _loss, g = tr.gradients(img.to(cuda), meta.to(cuda), labels.to(cuda))
        comb, meta_s, image = m._slot_groups()
        grads[prec] = {off: g[off:off + numel].cpu().double().clone()
                       for t, off, numel, _s in comb + meta_s + image if t.requires_grad}
        del tr, m
    assert grads["f32"] and grads["f32"].keys() == grads["f16x2"].keys()
    for off, ref in grads["f32"].items():
        scale = max(ref.abs().max().item(), 1e-7)
        err = (grads["f16x2"][off] - ref).abs().max().item() / scale
        assert err <= 1e-4, (off, err)
