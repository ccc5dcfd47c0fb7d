"""CPU: the float64 references, bounds and seeded faults of tests/mlp_ref.py, which tests/test_gpu_cn_mlp_ops.py holds the
MLP kernels of the ConvNeXt 16-bit training step to.

  - the references agree with torch's float64 autograd on y = x + gamma fc2(gelu(fc1(xn))) with the kernels' polynomial GELU;
  - an emulation of each kernel's arithmetic (fp32 products and sums, g / da rounded to the operand type where the kernel
    keeps them in 16 bit) stays inside every bound;
  - every seeded fault is outside the bound of at least one output by a factor >= 4, in bf16 and f16 (a condition on the
    input scales of mlp_ref.*_inputs, not a measurement of a kernel).
"""
import pytest
import torch

import mlp_ref as R
from gelu_ref import GELU_DEG, _gelu, _gelu_grad, gelu_poly_grad

F64 = torch.float64
FACTOR = 4.0
# (C, R, planes, slices): the launcher's figures for these row counts (2 / 3 tiles, one workgroup each)
MLP_BWD_SHAPES = [(64, 65, 1, 2), (128, 129, 4, 3)]
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def mlp_case(C, Rr):
    def make():
        inp = R.mlp_bwd_inputs(C, Rr, seed=C + Rr)
        return inp, R.mlp_bwd_base(inp)
    return cached(("mlp", C, Rr), make)


def s2_case(Rr):
    def make():
        inp = R.s2mlp_inputs(Rr, seed=Rr)
        return inp, R.s2mlp_base(inp)
    return cached(("s2", Rr), make)


def fused_case(C, M):
    def make():
        inp = R.fused_inputs(C, M, seed=C + M)
        return inp, R.fused_base(inp)
    return cached(("fused", C, M), make)


def show(case, ratios):
    print(f"{case:44s} " + "  ".join(f"{k} {v:9.3g}" for k, v in ratios.items()))


def test_inputs_are_exact_in_both_operand_types():
    t = R.exact(torch.randn(4096) * torch.logspace(-8, 3, 4096))
    assert torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t)
    assert bool((t == 0).any()) and float(t.abs().max()) > 100.0


@pytest.mark.parametrize("prec", R.PRECS)
def test_gelu_grad_slope_and_jump(prec):
    """L2_GELU bounds the slope of gelu_poly_grad on each smooth branch; at 0 it jumps by gelu_jump (about 2.6e-3 for the
    bf16 fit, 2.7e-5 for f16's) and nowhere else."""
    deg = GELU_DEG[prec]
    for lo, hi in ((-12.0, -1e-9), (1e-9, 12.0)):
        x = torch.linspace(lo, hi, 2_000_001, dtype=F64)
        gp = gelu_poly_grad(x, deg)
        slope = ((gp[1:] - gp[:-1]) / (x[1:] - x[:-1])).abs().max().item()
        print(f"{prec}: largest slope of gelu' on [{lo}, {hi}]: {slope:.4f}")
        assert slope <= R.L2_GELU
    e = torch.tensor([-1e-12, 1e-12], dtype=F64)
    jump = (gelu_poly_grad(e, deg)[1] - gelu_poly_grad(e, deg)[0]).abs().item()
    print(f"{prec}: jump of gelu' at 0: {jump:.3e} (gelu_jump {R.gelu_jump(prec):.3e})")
    assert abs(jump - R.gelu_jump(prec)) <= 1e-9
    assert {"bf16": 2.0e-3, "f16": 2.0e-5}[prec] <= jump <= {"bf16": 3.2e-3, "f16": 3.4e-5}[prec]


@pytest.mark.parametrize("prec", R.PRECS)
def test_references_agree_with_float64_autograd(prec):
    C, Rr, planes = 128, 37, 4
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)   # noqa: E731
    xn, x, dy = rn(Rr, C), rn(Rr, C), 0.05 * rn(Rr, C)
    w1, b1, w2, b2, gam = rn(4 * C, C) * C ** -0.5, 0.2 * rn(4 * C), rn(C, 4 * C) * (4 * C) ** -0.5, 0.2 * rn(C), 0.5 + 0.25 * rn(C)
    leaves = [t.requires_grad_() for t in (xn, w1, b1, w2, b2, gam)]
    a = xn @ w1.t() + b1
    a.retain_grad()
    y = x + gam * (_gelu(prec, a) @ w2.t() + b2)
    (y * dy).sum().backward()
    d = lambda t: t.detach()   # noqa: E731
    zero = lambda *s: torch.zeros(*s, dtype=F64)   # noqa: E731
    # fused_mlp's forward
    finp = dict(xn=d(xn), w1=d(w1), w2=d(w2), b1=d(b1), b2=d(b2), gamma=d(gam), xres=x, x0=x)
    fref, _ = R.fused_ref(finp, R.fused_base(finp), prec)
    assert torch.allclose(fref["x"], d(y), rtol=1e-12, atol=1e-13)
    # mlp_bwd
    inp = dict(xn=d(xn), dy=dy, w1=d(w1), w2g=(d(gam)[:, None] * d(w2)).t().contiguous(), b1=d(b1), G0=zero(C, 4 * C), S0=zero(C),
               dW0=zero(4 * C, C), db0=zero(4 * C))
    ref, _ = R.mlp_bwd_ref(inp, R.mlp_bwd_base(inp), prec, planes, 1)
    tol = dict(rtol=1e-10, atol=1e-12)
    assert torch.allclose(ref["dxn"].sum(0), xn.grad, **tol)
    assert torch.allclose(ref["dW1"], w1.grad, **tol) and torch.allclose(ref["db1"], b1.grad, **tol)
    # fc2_grads from mlp_bwd's G and S
    fc2, _ = R.fc2_ref(dict(G=ref["G"], S=ref["S"], w2=d(w2), b2=d(b2), gamma=d(gam)))
    assert torch.allclose(fc2["dW2"], w2.grad, **tol) and torch.allclose(fc2["db2"], b2.grad, **tol)
    assert torch.allclose(fc2["dgamma"], gam.grad, **tol)
    # s2mlp_bwd's algebra on the same tensors (its width is fixed; the reference's formulas are not)
    sinp = dict(dy=dy, a=d(a), w2gt=inp["w2g"], w1t=d(w1).t().contiguous())
    sref, _ = R.s2mlp_ref(sinp, R.s2mlp_base(sinp), prec)
    assert torch.allclose(sref["da"], a.grad, **tol) and torch.allclose(sref["dxn"], xn.grad, **tol)
    assert len(leaves) == 6


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("C,Rr,planes,slices", MLP_BWD_SHAPES)
def test_mlp_bwd_emulation_inside_faults_outside(prec, C, Rr, planes, slices):
    inp, base = mlp_case(C, Rr)
    ref, bound = R.mlp_bwd_ref(inp, base, prec, planes, slices)
    r = R.worst(R.mlp_bwd_emulate(inp, prec, planes), ref, bound)
    show(f"mlp_bwd-{prec}-C{C}-R{Rr} emulation", r)
    assert max(r.values()) <= 1.0, r
    for fault in R.MLP_BWD_FAULTS + (("drop_plane",) if planes > 1 else ()):
        bad, _ = R.mlp_bwd_ref(inp, base, prec, planes, slices, fault)
        r = R.worst(bad, ref, bound)
        show(f"mlp_bwd-{prec}-C{C}-R{Rr} {fault}", r)
        assert max(r.values()) >= FACTOR, (fault, r)


@pytest.mark.parametrize("prec", R.PRECS)
def test_s2mlp_emulation_inside_faults_outside(prec):
    inp, base = s2_case(46)
    ref, bound = R.s2mlp_ref(inp, base, prec)
    r = R.worst(R.s2mlp_emulate(inp, prec), ref, bound)
    show(f"s2mlp-{prec}-R46 emulation", r)
    assert max(r.values()) <= 1.0, r
    for fault in R.S2MLP_FAULTS:
        bad, _ = R.s2mlp_ref(inp, base, prec, fault)
        r = R.worst(bad, ref, bound)
        show(f"s2mlp-{prec}-R46 {fault}", r)
        assert max(r.values()) >= FACTOR, (fault, r)


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("C,M", [(64, 33), (80, 33), (128, 33), (160, 33)])
def test_fused_mlp_emulation_inside_faults_outside(prec, C, M):
    inp, base = fused_case(C, M)
    for res in ("xres", "x0"):
        ref, bound = R.fused_ref(inp, base, prec, res)
        r = R.worst(R.fused_emulate(inp, prec, res), ref, bound)
        show(f"fused_mlp-{prec}-C{C}-M{M}-{res} emulation", r)
        assert max(r.values()) <= 1.0, r
    ref, bound = R.fused_ref(inp, base, prec)
    for fault in R.FUSED_FAULTS + (("ragged80",) if C == 80 else ()):
        bad, _ = R.fused_ref(inp, base, prec, "xres", fault)
        r = R.worst(bad, ref, bound)
        show(f"fused_mlp-{prec}-C{C}-M{M} {fault}", r)
        assert max(r.values()) >= FACTOR, (fault, r)


@pytest.mark.parametrize("C,H", [(64, 256), (160, 640), (512, 2048)])
def test_fc2_grads_emulation_inside_faults_outside(C, H):
    inp = R.fc2_inputs(C, H, seed=C)
    ref, bound = R.fc2_ref(inp)
    r = R.worst(R.fc2_emulate(inp), ref, bound)
    show(f"fc2_grads-{C}x{H} emulation", r)
    assert max(r.values()) <= 1.0, r
    for fault in R.FC2_FAULTS:
        bad, _ = R.fc2_ref(inp, fault)
        r = R.worst(bad, ref, bound)
        show(f"fc2_grads-{C}x{H} {fault}", r)
        assert max(r.values()) >= FACTOR, (fault, r)


def test_spotlight_rows_keep_the_reduced_bounds_at_one_tile():
    """dy that is zero outside a few rows gives da = 0 there (so dxn is exactly 0) and a bound of G that does not grow
    with the dark rows."""
    C, Rr = 64, 300
    live = [0, 7, 299]
    inp = R.mlp_bwd_inputs(C, Rr, seed=1, live_rows=live)
    ref, bound = R.mlp_bwd_ref(inp, R.mlp_bwd_base(inp), "bf16", 1, 5)
    dark = torch.ones(Rr, dtype=torch.bool)
    dark[live] = False
    assert ref["dxn"][0][dark].abs().max().item() == 0.0 and bound["dxn"][0][dark].abs().max().item() == 0.0
    assert ref["dxn"][0][live].abs().min().item() > 0.0
