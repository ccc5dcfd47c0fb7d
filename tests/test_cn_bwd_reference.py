"""CPU: can the references and bounds of tests/test_gpu_cn_bwd_ops.py (tests/cn_bwd_ref.py) see a subtly wrong kernel?

1. The float64 references against central finite differences of the loss they differentiate, and the 2x2 unfold
   against F.conv2d with a one-hot filter.
2. A float32 restatement of every op in explicit formulas (tap loops, LayerNorm algebra) takes one seeded fault at a
   time -- the ones a rewrite of these kernels is likely to make -- and must then miss the case's bound
   (MARGIN x e32, or 2 x measured where cn_bwd_ref.MEASURED says so) by a factor of 10 on some output, for every shape
   of the GPU file at its smallest batch (two alerts where the fault drops one).  e32 itself must be non-zero and below
   1e-4, so that no bound is vacuous or absurd.  The restatement WITHOUT a fault is printed beside its bound: another
   fp32 summation order than torch's, as the kernels are.
"""
import pytest
import torch
import torch.nn.functional as F

import cn_bwd_ref as R

F32, F64 = torch.float32, torch.float64


# ---- 1. the references themselves
def test_block_reference_matches_finite_differences():
    inp = R.block_inputs(3, 8, 2, planes=2, seed=1)
    ref = R.block_ref(inp, F64)
    gy = inp["dxn"].double().sum(0)

    def loss(x, w, b, g):
        d = F.conv2d(R.nchw(x, F64), R.weight_of(w, F64), b.double(), padding=3, groups=8).permute(0, 2, 3, 1)
        return (F.layer_norm(d, (8,), g.double(), torch.zeros(8, dtype=F64), R.EPS) * gy).sum().item()

    args = [inp[k].double() for k in ("x", "w", "bias", "g")]
    grads = [ref["dy"] - inp["dy0"].double(), ref["dW"].t(), ref["db"], ref["dg"]]
    h = 1e-6
    gen = torch.Generator().manual_seed(5)
    for i, (a, gr) in enumerate(zip(args, grads)):
        for _ in range(6):
            j = int(torch.randint(a.numel(), (1,), generator=gen))
            hi, lo = [t.clone() for t in args], [t.clone() for t in args]
            hi[i].view(-1)[j] += h
            lo[i].view(-1)[j] -= h
            fd = (loss(*hi) - loss(*lo)) / (2 * h)
            assert abs(fd - gr.reshape(-1)[j].item()) <= 1e-6 * max(1.0, gr.abs().max().item()), (i, j, fd)
    # dd is the same thing seen from the LayerNorm alone, and a kept depthwise output handed in changes nothing
    ln = R.ln_ref(inp["d"].double().reshape(-1, 8), inp["g"], gy.reshape(-1, 8), F64)
    assert R.rel_err(ln["dd"].reshape(ref["dd"].shape), ref["dd"]) <= 1e-6   # (d rounded to fp32 once)
    kept = R.block_ref(inp, F64, d_in=inp["d"])
    for k in ref:
        assert R.rel_err(kept[k], ref[k]) <= 1e-6, k


@pytest.mark.parametrize("hw", [15, 7, 3, 4])
def test_unfold_matches_a_one_hot_convolution(hw):
    B, C, HO = 2, 5, hw // 2
    y = torch.randn(B * hw * hw, C, generator=torch.Generator().manual_seed(hw), dtype=F64)
    filt = torch.zeros(4 * C, C, 2, 2, dtype=F64)
    for q in range(4):
        for c in range(C):
            filt[q * C + c, c, q // 2, q % 2] = 1.0
    want = F.conv2d(y.view(B, hw, hw, C).permute(0, 3, 1, 2), filt, stride=2).permute(0, 2, 3, 1).reshape(B * HO * HO, 4 * C)
    assert torch.equal(R.unfold2(y, B, hw), want)


def test_constant_row_closed_form():
    g = torch.Generator().manual_seed(2)
    d = R.rows_like(g, 5, 80)
    d[3] = 0.75
    gam, dxn = R.signed(g, 80), torch.randn(5, 80, generator=g)
    ref = R.ln_ref(d, gam, dxn, F64)
    assert R.rel_err(ref["dd"][3], R.const_row_dd(gam, dxn[3])) <= 1e-12


# ---- 2. a float32 restatement with faults
def ln_restate(d, g, gy, fault=None):
    C = d.shape[-1]
    mean = d[..., :C - 1].mean(-1, keepdim=True) if fault == "mean" else d.mean(-1, keepdim=True)
    xc = d - mean
    rstd = ((xc * xc).mean(-1, keepdim=True) + (1e-5 if fault == "eps" else R.EPS)) ** -0.5
    xhat, t = xc * rstd, gy * g
    dd = rstd * (t - t.mean(-1, keepdim=True) - xhat * (t * xhat).mean(-1, keepdim=True))
    flat = (gy * xhat).reshape(-1, C)
    return dd, flat.sum(0), gy.reshape(-1, C).sum(0)


def shifted(t, ky, kx, H):
    """t padded by 4: the map seen through tap (ky, kx) of a 7x7 p3 window"""
    return t[:, ky + 1:ky + 1 + H, kx + 1:kx + 1 + H]


def wgrad_restate(x, dd, fault=None):
    B, H, _, C = x.shape
    if fault == "alert":
        x, dd = x[:-1], dd[:-1]
    xp = F.pad(x, (0, 0, 4, 4, 4, 4))
    dW = torch.stack([(dd * shifted(xp, t // 7, t % 7 + (1 if fault == "tap" and t == 24 else 0), H)).sum((0, 1, 2))
                      for t in range(49)], 1)
    return dW, dd.sum((0, 1, 2))


def conv_restate(x, w, flip, fault=None):
    H = x.shape[1]
    xp = F.pad(x, (0, 0, 4, 4, 4, 4))
    out = torch.zeros_like(x)
    for t in range(49):
        tap = w[48 - t if flip and fault != "noflip" else t]
        out = out + tap * shifted(xp, t // 7, t % 7 + (1 if fault == "tap" and t == 24 else 0), H)
    return out


def block_restate(inp, fault=None):
    x, w = inp["x"], inp["w"]
    d = conv_restate(x, w, 0) + inp["bias"]
    gy = (inp["dxn"][:-1] if fault == "plane" else inp["dxn"]).sum(0)
    dd, dg, dbeta = ln_restate(d, inp["g"], gy, fault)
    dW, db = wgrad_restate(x, dd, fault)
    return dict(dd=dd, dg=dg, dbeta=dbeta, dW=dW, db=db, dy=inp["dy0"] + conv_restate(dd, w, 1, fault))


def worst_ratio(cls, got, ref64, e32):
    """the largest error / bound over the outputs; cls: the case's class in cn_bwd_ref.MEASURED (None: no class)"""
    return max(R.rel_err(got[k], ref64[k]) / R.bound(cls, k, e32[k]) for k in ref64)


def check_e32(case, e32):
    for k, v in e32.items():
        assert 0.0 < v < 1e-4, (case, k, v)


def report(case, ok_ratio, ratios):
    print(f"{case}: no fault {ok_ratio:.2f} x bound; " + ", ".join(f"{k} {v:.1e} x" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v >= 10.0, f"{case}: the fault '{k}' reaches only {v:.2f} x the bound -- the inputs are too tame"


@pytest.mark.parametrize("HW,C", R.DWLN_SHAPES + [(1, 512), (1, 640)])
def test_bounds_see_faults_in_the_fused_block_backward(HW, C):
    """dwln_bwd / dw3ln_bwd (15x15x64, 7x7x128, 3x3x256) and ln_dw1_bwd (1x1x512, 1x1x640): four planes, two alerts
    (the smallest batch in which an alert can be dropped while another stays)."""
    inp = R.block_inputs(HW, C, 2, planes=4)
    ref, ref32 = R.block_ref(inp, F64), R.block_ref(inp, F32)
    e32 = R.e32_of(ref32, ref)
    case = f"block-{HW}x{C}"
    check_e32(case, e32)
    faults = ["tap", "alert", "plane", "eps", "mean"] + (["noflip"] if HW > 1 else [])   # (1x1: tap 24 is its own flip)
    report(case, worst_ratio(case, block_restate(inp), ref, e32),
           {f: worst_ratio(case, block_restate(inp, f), ref, e32) for f in faults})


@pytest.mark.parametrize("C", R.LN_WIDTHS)
def test_bounds_see_faults_in_the_dense_layernorm_backward(C):
    g = torch.Generator().manual_seed(C)
    d, gam, dxn = R.rows_like(g, 1, C), R.signed(g, C), torch.randn(1, C, generator=g)
    pre = 0.05 * torch.randn(2, C, generator=g)   # the gradients are added to what the arena holds
    ref, ref32 = (R.ln_ref(d, gam, dxn, t, 0, *pre) for t in (F64, F32))
    e32 = R.e32_of(ref32, ref)
    case = f"ln-{C}"
    check_e32(case, e32)

    def run(fault=None):
        dd, dg, dbeta = ln_restate(d, gam, dxn, fault)
        return dict(dd=dd, dg=pre[0] + dg, dbeta=pre[1] + dbeta)

    cls = "ln-trip2"   # the widest bound a case of this width has: dg / dbeta past the 512-workgroup cap
    report(case, worst_ratio(cls, run(), ref, e32), {f: worst_ratio(cls, run(f), ref, e32) for f in ("eps", "mean")})


@pytest.mark.parametrize("hw,C", R.PATCH_SHAPES)
def test_bounds_see_faults_in_the_patch_gather(hw, C):
    g = torch.Generator().manual_seed(hw * C)
    HO = hw // 2
    d, gam, dpat = R.rows_like(g, hw * hw, C), R.signed(g, C), torch.randn(HO * HO, 4 * C, generator=g)
    ref, ref32 = R.ln_ref(d, gam, dpat, F64, hw), R.ln_ref(d, gam, dpat, F32, hw)
    e32 = R.e32_of(ref32, ref)
    case = f"lnpatch-{hw}x{C}"
    check_e32(case, e32)

    def run(fault=None):
        # every input pixel reads its slice of the patch that covers it; the odd last row and column read zero --
        # or, the fault, the patch of the row above (what a clamped index does)
        gy = torch.zeros(hw, hw, C)
        for y in range(hw):
            for x in range(hw):
                if (y < 2 * HO and x < 2 * HO) or (fault == "odd" and x < 2 * HO):
                    yy = min(y, 2 * HO - 1)
                    gy[y, x] = dpat[(yy // 2) * HO + x // 2].view(4, C)[2 * (yy & 1) + (x & 1)]
        return dict(zip(("dd", "dg", "dbeta"), ln_restate(d, gam, gy.view(-1, C), fault)))

    report(case, worst_ratio(case, run(), ref, e32),
           {f: worst_ratio(case, run(f), ref, e32) for f in ("odd", "eps", "mean")})


@pytest.mark.parametrize("HW,C", R.DW_SHAPES)
def test_bounds_see_faults_in_the_plain_depthwise_kernels(HW, C):
    """dw_plain (a shifted tap; taps not flipped where the caller asks for flipped ones) and dw_wgrad (a shifted tap, a
    dropped alert)."""
    inp = R.block_inputs(HW, C, 2)
    x, w, dd = inp["x"], inp["w"], inp["dxn"][0]
    for flip in (0, 1):
        ref, ref32 = (R.dw_plain_ref(x, w, flip, inp["bias"], inp["dy0"], t) for t in (F64, F32))
        e32 = R.e32_of(ref32, ref)
        case = f"dw_plain-{HW}x{C}-flip{flip}"
        check_e32(case, e32)

        def run(fault=None):
            return dict(out=conv_restate(x, w, flip, fault) + inp["bias"] + inp["dy0"])

        faults = ["tap"] + (["noflip"] if flip and HW > 1 else [])
        cls = f"dw_plain+addend-{HW}x{C}"
        report(case, worst_ratio(cls, run(), ref, e32), {f: worst_ratio(cls, run(f), ref, e32) for f in faults})
    zero = torch.zeros(C, 49), torch.zeros(C)
    ref, ref32 = (R.dw_wgrad_ref(x, dd, *zero, t) for t in (F64, F32))
    e32 = R.e32_of(ref32, ref)
    case = f"dw_wgrad-{HW}x{C}"
    check_e32(case, e32)

    def run(fault=None):
        return dict(zip(("dW", "db"), wgrad_restate(x, dd, fault)))

    report(case, worst_ratio(case, run(), ref, e32), {f: worst_ratio(case, run(f), ref, e32) for f in ("tap", "alert")})


def test_every_measured_bound_belongs_to_a_class_the_fault_tests_use():
    """A bound taken from a measurement (cn_bwd_ref.MEASURED) is held against the faults above under its class name: an
    entry of any other name would be checked by nothing."""
    known = {("ln-trip2", k) for k in ("dg", "dbeta")} | {(f"dw_plain+addend-{hw}x{c}", "out") for hw, c in R.DW_SHAPES}
    assert set(R.MEASURED) <= known, set(R.MEASURED) - known
