"""References, inputs and bounds shared by tests/test_gpu_cn_bwd_ops.py (the kernels on the GPU) and
tests/test_cn_bwd_reference.py (the same references and bounds against seeded faults, on the CPU).

The reference of every op is torch's own autograd on the CPU, run in float64; the yardstick of its bound is the SAME
function run in float32 (`e32`).  Nothing here knows the kernels' formulas.  Layouts are the kernels': activations NHWC
[B, HW, HW, C], depthwise taps w [49, C] (tap-major), filter gradients [C, 49].
"""
import torch
import torch.nn.functional as F

EPS = 1e-6
MARGIN = 4.0   # bound of an fp32 output = MARGIN * e32: the kernels' summation order (wave sums, partial rows per
#                workgroup, atomics in the arena) differs from torch's and either side may be the worse one

# Classes of cases whose kernel measures above MARGIN * e32 on an MI355X: (class, tensor) -> the largest measured error;
# their bound is 2 x measured (table and reasons in tests/test_gpu_cn_bwd_ops.py's docstring).
MEASURED = {
    ("dw_plain+addend-15x64", "out"): 4.277e-07, ("dw_plain+addend-15x80", "out"): 3.618e-07,
    ("dw_plain+addend-7x128", "out"): 3.482e-07, ("dw_plain+addend-7x160", "out"): 3.467e-07,
    ("dw_plain+addend-3x256", "out"): 1.966e-07, ("dw_plain+addend-3x320", "out"): 1.969e-07,
    ("ln-trip2", "dg"): 9.721e-07, ("ln-trip2", "dbeta"): 8.531e-07,
}

# (map side, channels) of the depthwise ops: convnext_pico's and convnext_nano's four stages
DW_SHAPES = [(15, 64), (15, 80), (7, 128), (7, 160), (3, 256), (3, 320), (1, 512), (1, 640)]
PATCH_SHAPES = DW_SHAPES[:6]
DWLN_SHAPES = [(15, 64), (7, 128), (3, 256)]
LN_WIDTHS = [64, 128, 80, 160, 256, 320, 512, 640]


def rel_err(got, ref64):
    return (got.double() - ref64).abs().max().item() / ref64.abs().max().item()


def bound(cls, name, e32):
    """cls: the class of the case in MEASURED, or anything else"""
    return max(MARGIN * e32, 2.0 * MEASURED.get((cls, name), 0.0))


def e32_of(ref32, ref64):
    return {k: rel_err(ref32[k], ref64[k]) for k in ref64}


def weight_of(w, dtype):
    """taps [49, C] -> conv_dw.weight [C, 1, 7, 7]"""
    return w.to(dtype).t().reshape(-1, 1, 7, 7).contiguous()


def nchw(t, dtype):
    return t.to(dtype).permute(0, 3, 1, 2).contiguous()


# ---- inputs: fp32, seeded.  Per-channel offsets and scales put the variance of a row of d at ~1e-2: far above eps,
# and small enough that an eps of 1e-5 moves dd by ~1e-4 (a fault the bounds must see).
def _gen(*key):
    return torch.Generator().manual_seed(1000003 * key[0] + 1009 * key[1] + 31 * key[2] + (key[3] if len(key) > 3 else 0))


def signed(g, C):
    """LayerNorm weights of both signs, none near zero"""
    return (0.5 + torch.rand(C, generator=g)) * (1 - 2 * (torch.rand(C, generator=g) < 0.4).float())


def rows_like(g, rows, C):
    """a pre-normalisation activation [rows, C]"""
    return 0.1 * torch.randn(C, generator=g) + (0.05 + 0.05 * torch.rand(C, generator=g)) * torch.randn(rows, C, generator=g)


def block_inputs(HW, C, B, planes=1, seed=0):
    g = _gen(HW, C, B, 7 * planes + seed)
    x = 0.3 * torch.randn(C, generator=g) + (0.05 + 0.1 * torch.rand(C, generator=g)) * torch.randn(B, HW, HW, C, generator=g)
    inp = dict(x=x, w=0.05 * torch.randn(49, C, generator=g), bias=0.1 * torch.randn(C, generator=g), g=signed(g, C),
               dxn=torch.randn(planes, B, HW, HW, C, generator=g), dy0=torch.randn(B, HW, HW, C, generator=g))
    inp["d"] = kept_d(inp)
    return inp


def kept_d(inp):
    """what the forward keeps: the depthwise output, in fp32"""
    with torch.no_grad():
        return F.conv2d(nchw(inp["x"], torch.float64), weight_of(inp["w"], torch.float64), inp["bias"].double(), padding=3,
                        groups=inp["x"].shape[-1]).permute(0, 2, 3, 1).float().contiguous()


# ---- references (dtype = torch.float64: the reference; torch.float32: its yardstick)
def block_ref(inp, dtype, d_in=None):
    """LayerNorm(conv_dw(x)) with loss = sum(out * sum of dxn's planes): every gradient of one backward().
    d_in: the LayerNorm differentiates this tensor instead of the convolution's own output (the fused kernels read the
    depthwise output the forward kept, so a test may hand them any), and its gradient then enters the convolution."""
    C = inp["x"].shape[-1]
    x = nchw(inp["x"], dtype).requires_grad_()
    W = weight_of(inp["w"], dtype).requires_grad_()
    b = inp["bias"].to(dtype).clone().requires_grad_()
    g = inp["g"].to(dtype).clone().requires_grad_()
    beta = torch.zeros(C, dtype=dtype, requires_grad=True)
    gy = inp["dxn"].to(dtype).sum(0)
    d = F.conv2d(x, W, b, padding=3, groups=C).permute(0, 2, 3, 1)
    if d_in is None:
        dl = d
        dl.retain_grad()
    else:
        dl = d_in.to(dtype).clone().requires_grad_()
    (F.layer_norm(dl, (C,), g, beta, EPS) * gy).sum().backward()
    if d_in is not None:
        d.backward(dl.grad)
    return dict(dd=dl.grad.detach(), dg=g.grad, dbeta=beta.grad, dW=W.grad.reshape(C, 49), db=b.grad,
                dy=inp["dy0"].to(dtype) + x.grad.permute(0, 2, 3, 1))


def unfold2(y, B, hw):
    """rows [B hw hw, C] -> the 2x2 / stride-2 patch matrix [B (hw/2)^2, 4 C], k = (2 (y & 1) + (x & 1)) C + c; an odd
    last row and column belong to no patch"""
    C, HO = y.shape[-1], hw // 2
    v = y.reshape(B, hw, hw, C)[:, :2 * HO, :2 * HO].reshape(B, HO, 2, HO, 2, C).permute(0, 1, 3, 2, 4, 5)
    return v.reshape(B * HO * HO, 4 * C)


def ln_ref(d, g, dxn, dtype, patch_hw=0, dg0=None, dbeta0=None):
    """LayerNorm over the rows of d [rows, C]; dxn: the gradient of its output [rows, C], or with patch_hw that of the
    patch matrix behind it.  dg0 / dbeta0: what the parameter gradients are added to."""
    rows, C = d.shape
    dl = d.to(dtype).clone().requires_grad_()
    gg = g.to(dtype).clone().requires_grad_()
    beta = torch.zeros(C, dtype=dtype, requires_grad=True)
    out = F.layer_norm(dl, (C,), gg, beta, EPS)
    if patch_hw:
        out = unfold2(out, rows // (patch_hw * patch_hw), patch_hw)
    (out * dxn.to(dtype).reshape(out.shape)).sum().backward()
    return dict(dd=dl.grad, dg=gg.grad + (0 if dg0 is None else dg0.to(dtype)),
                dbeta=beta.grad + (0 if dbeta0 is None else dbeta0.to(dtype)))


def dw_plain_ref(x, w, flip, bias, addend, dtype):
    """conv(x, taps) or, flipped, the gradient of the convolution's input for an output gradient x; + bias + addend"""
    C = x.shape[-1]
    xx, W = nchw(x, dtype), weight_of(w, dtype)
    if flip:
        z = torch.zeros_like(xx, requires_grad=True)
        (F.conv2d(z, W, None, padding=3, groups=C) * xx).sum().backward()
        o = z.grad
    else:
        o = F.conv2d(xx, W, None, padding=3, groups=C)
    o = o.permute(0, 2, 3, 1)
    if bias is not None:
        o = o + bias.to(dtype)
    if addend is not None:
        o = o + addend.to(dtype)
    return dict(out=o)


def dw_wgrad_ref(x, dd, dw0, db0, dtype):
    """dw0 [C, 49] + the filter gradient, db0 [C] + the bias gradient of conv_dw for the output gradient dd"""
    C = x.shape[-1]
    W = torch.zeros(C, 1, 7, 7, dtype=dtype, requires_grad=True)
    b = torch.zeros(C, dtype=dtype, requires_grad=True)
    (F.conv2d(nchw(x, dtype), W, b, padding=3, groups=C) * nchw(dd, dtype)).sum().backward()
    return dict(dW=dw0.to(dtype) + W.grad.reshape(C, 49), db=db0.to(dtype) + b.grad)


def arena_ref(r, a0, dtype):
    """the arena block [C, 49] | [C] | [C] | [C], pre-filled with a0, after the four gradients of r were added"""
    C = r["db"].numel()
    a = a0.to(dtype)
    return dict(dW=a[:49 * C].reshape(C, 49) + r["dW"], db=a[49 * C:50 * C] + r["db"], dg=a[50 * C:51 * C] + r["dg"],
                dbeta=a[51 * C:] + r["dbeta"])


def const_row_dd(g, dxn_row):
    """dd of a row of constant d (variance exactly 0): xhat = 0, rstd = eps^-1/2, dd = rstd (t - mean t), t = dxn g"""
    t = dxn_row.double() * g.double()
    return (t - t.mean()) / EPS ** 0.5
