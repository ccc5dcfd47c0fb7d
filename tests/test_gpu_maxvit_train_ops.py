"""The MaxViT training kernels of maxvit_train_kernels.hip one at a time (btsbot_op_mvt_*, the entry points of
maxvit_train_ops.hip) against plain float64 references.

Conventions are test_gpu_gemm_paths.py's and test_gpu_maxvit_ops.py's: everything is fp32, references are float64 torch
on the device (F.batch_norm(training=True), F.conv2d(groups=C), an explicit softmax attention over part_rows; backwards
are float64 autograd through those), every output is a slice of a sentinel-guarded buffer whose head and tail must
survive, every "added to" output starts from random content (the reference is that content plus the gradient), every
"written" output starts as NaN, and each test prints its worst err / bound.  The op entry points run the launchers the
training engine runs, so the grid arithmetic under test is the engine's; the three grid decisions are read back from
the library (ops.mvt_bn_row_blocks, mvt_dw3_bwd_w_row_blocks, mvt_attn_bwd_groups_per_head), never mirrored here.
EPS = 2^-24.

Sums.  Every reduction is a plain fp32 sum of terms t_i and is held to D EPS sum |t_i|, D the longest chain of fp32
additions the layout allows.  The reductions over rows (col_moments, bn_bwd_sums, dw3_bwd_w) give a row lane every
16 * blocks-th row, add the 16 row lanes of a workgroup in LDS and add the workgroups atomically:
    D = ceil(rows / (16 blocks)) + 16 + blocks                                     (chain_rows)
alert_colsum has one workgroup per alert (D = ceil(P / 16) + 16 + 1 for the scale); the small dense layers run four
fma chains over I inputs, (I // 4 + I % 4 + 3); lin_bwd_w one chain over the B alerts.  A sum that lands on prior
content costs one more rounding of the result (atomics straight onto prior content: D EPS (sum |t_i| + |prior|)).

BatchNorm forward, per channel, with a = mean |x|, mad = mean |x - mu|, var the float64 batch variance:
    e0     = (D + 1) EPS a                            pass 1: mean0 = sum x / M
    e_d    = (D + 1) EPS (mad + e0)                   pass 2: the centred sum / M, which polishes the mean
    e_mean = e_d + 2 EPS (mad + e0) + 2 EPS |mu|
    e_var  = (D + 6) EPS (var + e0^2) + (e0 + e_d)^2 - e0^2
             (mean d^2 - (mean d)^2 is the variance of the d_i = fl(x_i - mean0) themselves, whatever mean0 is: what is
              left are the roundings of the d_i, of the two sums and of the square of a mean that is at most e0 + e_d)
    e_rstd = rstd^3 / 2 (e_var + 2 EPS (var + 1e-5)) + 4 EPS rstd                  (rsqrtf: 2 ulp)
    e_z    = |w| (rstd e_mean + |x - mu| e_rstd + 3 EPS |xhat|) + EPS |z|,         y = z or silu(z): L_SILU, SILU_REL
    running mean: 0.1 e_mean + 4 EPS (0.9 |rm| + 0.1 |mu|);  running variance (unbiased, M / (M - 1)) alike with e_var.
Inputs have a per-channel mean of up to 100 standard deviations, and channel 1 is one constant (2896.3091...): its
variance is 0, rstd = 1e-5^-1/2, and the formulas above bound it absolutely (e_var = 3 (D + 6) EPS e0^2, which is what
separates the two-pass variance from a one-pass one, or from one without its - d^2 term).

BatchNorm backward takes stat as an INPUT: the float64 statistics rounded to fp32 (EPS |mu|, EPS rstd), so
    e_xhat = rstd EPS (|mu| + |x - mu|) + 2 EPS |xhat|,   e_z = |w| e_xhat + EPS |z|,
    dz = dy silu'(z): e_dz = |dy| (e_z / 2 + SILU_REL (1 + |z|)) + EPS |dz|        (|silu''| <= 1/2)
    e_S0 = sum e_dz + (D + 1) EPS sum |dz|,   e_S1 = sum (e_dz |xhat| + |dz| e_xhat) + (D + 1) EPS sum |dz xhat|
    dx = w rstd (dz - S0 / M - xhat S1 / M):
    e_dx = |w| rstd (e_dz + e_S0 / M + (|xhat| e_S1 + e_xhat |S1|) / M + 6 EPS (|dz| + |S0| / M + |xhat S1| / M))
           + 4 EPS |dx|  (+ EPS |out| when it is added to).

Depthwise 3x3: nine fmas, 11 EPS (|b| + sum |v| |w|) forward (mv_dw3's bound), 10 EPS sum |dout| |w| for the input
gradient; the filter gradient is a sum over rows (chain_rows of the output pixels, + 1 for the unpack's add).  Border
rows and columns of the input and of dout are 8x larger.

Squeeze-excite: the chain of sums above, each error carried through the next layer's |W|, SiLU (L_SILU, SILU_REL), its
derivative (1/2, SILU_REL (1 + |x|)) and the sigmoid (1/4, SILU_REL).  The backward op takes pool, rpre, r and gate as
inputs rounded to fp32 (one EPS each).

Attention backward.  P and dv carry the forward's logit-perturbation bound over: delta per query as in
test_gpu_maxvit_ops.py, |dv - ref| <= sum_t (e^(2 delta_t) - 1 + 102 EPS) P[t][j] |dO_t| (102: the 49-term denominator,
the 49 queries, 1 / sum and its product).  dS = P (dP - sum P dP) cancels, so dq, dk and dtable use the R / R~ method:
R is float64 autograd through the explicit attention; R~ the same float64 computation with a round-to-fp32 at each value
the kernel holds in a register or in LDS (the scaled q, the logits, e, the sum and its inverse, P, dP, the dot, dP - dot
and dS); E = max |R~ - R|, and
    max |out - R| <= 2 E + D EPS sum |terms|      of the final sum: 51 SC |dS| @ |k|, 51 |dS|^T @ |SC q|, and for dtable
    D = units per workgroup + workgroups per head + 49 (relbias_grad) + 1 (prior content), terms = sum |dS|.
Each such case asserts 2 E <= 1e-3 rms(R), a condition on the inputs (unit-variance q, k, v, dO, table ~ N(0, 1)); the
unrounded explicit formulas are also asserted equal to autograd.  Measured on the reference alone over the cases of this
file, 2 E / rms(R) is at most 3.7e-6 (dq), 3.8e-6 (dk) and 2.0e-6 (dtable; 1.5e-6 and 8.0e-7 in the two walking cases)
on the CPU, and 3.7e-6, 4.8e-6 and 2.4e-6 with the same code on the device: 200 times under the limit.
Probes: q = k = 0 makes every logit its bias exactly; with a zero table P is fl(1 / 49), dv the partition mean of dO
(integers) and dq = dk = 0 exactly; with a random table P = softmax(bias).  Walking (test_train_grid_arithmetic):
C = 512, H = 7, B = 200 is 200 units on 192 workgroups per head, C = 64, H = 14, B = 385 is 1540 on 1536: some
workgroups take a second unit, the bias gradient stays in registers across them, the last trip is ragged.

The small kernels: avgpool2_bwd, unpack_conv3_grad and bcast_set move data (exact, or one rounding of the result),
col2im3 adds nine terms, GELU and its derivative are the erf forms (test_gpu_gemm_paths._gelu_f / _gelu_grad_f).
"""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_gemm_paths as GP
import test_gpu_maxvit_ops as MV
from btsbot_amd import _lib, ops
from oracle import maxvit_oracle as MO   # checker only
from test_gpu_gemm_paths import EPS, _check, _guarded, _intact
from test_gpu_maxvit_ops import part_rows, rel_bias

L_SILU, SILU_REL = GP.L_SILU, GP.SILU_REL
SC = 32 ** -0.5
gpu = pytest.mark.gpu
NAN = float("nan")


def _cdiv(a, b):
    return -(-a // b)


def chain_rows(rows, blocks):
    """Longest chain of fp32 additions of a reduction over rows: per-lane trips + 16 row lanes + atomics."""
    return _cdiv(rows, 16 * blocks) + 16 + blocks


def chain_lin(I):
    return I // 4 + I % 4 + 3


def _written(n, dev):
    buf, t = _guarded(n, torch.float32, dev)
    t.fill_(NAN)
    return buf, t


def _added(prior):
    return _guarded(prior.numel(), torch.float32, prior.device, fill=prior)


def _silu(t):
    return t * torch.sigmoid(t)


def _silu_grad(t):
    s = torch.sigmoid(t)
    return s * (1 + t * (1 - s))


def _show(tag, worst):
    print(f"[{tag}] err/bound " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


# ---- host only: the launchers' grid decisions, read from the library
WALK_ATTN = ((512, 7, 200), (64, 14, 385))
BN_SHAPES = [(49, 64), (196, 32), (3 * 784, 256), (49 * 7, 2048), (65536 + 256 + 49, 32)]
DW3_CAPPED = (6, 56, 1, 32)


def test_train_grid_arithmetic():
    """The three query functions at the model's own sizes (B = 4, where nothing is capped and nobody walks, and B = 64)
    and at this file's cases."""
    bn, dw, at = ops.mvt_bn_row_blocks, ops.mvt_dw3_bwd_w_row_blocks, ops.mvt_attn_bwd_groups_per_head
    # rows of the model's BatchNorms: B * {112, 56, 28, 14, 7}^2
    assert [bn(4 * h * h) for h in (112, 56, 28, 14, 7)] == [196, 49, 12, 3, 1]
    assert [bn(64 * h * h) for h in (112, 56, 28, 14, 7)] == [256, 256, 196, 49, 12]
    assert [bn(m) for m, _ in BN_SHAPES] == [1, 1, 9, 1, 256]
    M = BN_SHAPES[-1][0]
    assert M > 65536 and M % (16 * 256) != 0 and _cdiv(M, 16 * 256) == 17      # capped, 17 rows per lane, ragged
    assert bn(65536) == 256 and bn(65536 + 256) == 256 and bn(65535) == 255 and bn(255) == 1 and bn(512) == 2
    assert bn(49) == 1 and 49 < 16 * 4 and 196 % (16 * 4) == 4               # M / 256 == 0: one block, a ragged last trip
    # output pixels of the model's depthwise convolutions: B * {56, 28, 14, 7}^2
    assert [dw(4 * h * h) for h in (56, 28, 14, 7)] == [196, 49, 12, 3]
    assert [dw(64 * h * h) for h in (56, 28, 14, 7)] == [256, 256, 196, 49]
    B, H, s, _ = DW3_CAPPED
    assert B * (H // s) ** 2 == 18816 and dw(18816) == 256 and dw(3 * 49) == 2 and dw(3 * 16) == 1 and dw(16384) == 256
    # attention: units = B (H / 7)^2 per stage (H, C) = (56, 64), (28, 128), (14, 256), (7, 512)
    stages = ((56, 64), (28, 128), (14, 256), (7, 512))
    assert [at(4 * (h // 7) ** 2, c // 32) for h, c in stages] == [256, 64, 16, 4]              # one unit each
    assert [at(64 * (h // 7) ** 2, c // 32) for h, c in stages] == [1536, 768, 256, 64]         # stages 0 and 1 walk
    for C, H, B in WALK_ATTN:
        units, per = B * (H // 7) ** 2, at(B * (H // 7) ** 2, C // 32)
        assert per == 3072 // (C // 32) and per < units < 2 * per, (units, per)      # some take a second unit: ragged
        assert at(per, C // 32) == per
    assert at(3 * 9, 16) == 27 and at(3, 2) == 3
    L = _lib.lib()
    assert L.btsbot_op_mvt_bn_row_blocks(0) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mvt_dw3_bwd_w_row_blocks(0) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mvt_attn_bwd_groups_per_head(4, 17) == _lib.ERR_INVALID_ARG
    assert b"heads" in L.btsbot_last_error()


# ---- BatchNorm2d on batch statistics
CONST_CH, CONST_V = 1, 2896.3091


def _bn_inputs(M, C, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    sig = 0.5 + 1.5 * torch.rand(C, generator=g, device=dev)
    mu = (200.0 * torch.rand(C, generator=g, device=dev) - 100.0) * sig
    x = mu + sig * torch.randn(M, C, generator=g, device=dev)
    x[:, CONST_CH] = CONST_V
    w = 1.0 + 0.1 * torch.randn(C, generator=g, device=dev)
    b = 0.1 * torch.randn(C, generator=g, device=dev)
    return g, x.contiguous(), w, b


@gpu
@pytest.mark.parametrize("act", [0, 1], ids=["plain", "silu"])
@pytest.mark.parametrize("M,C", BN_SHAPES, ids=[f"M{m}-C{c}" for m, c in BN_SHAPES])
def test_bn_fwd_against_float64(cuda, M, C, act):
    g, x, w, b = _bn_inputs(M, C, cuda, M + C)
    rm = torch.randn(C, generator=g, device=cuda)
    rv = 0.5 + torch.rand(C, generator=g, device=cuda)
    D = chain_rows(M, ops.mvt_bn_row_blocks(M))
    x64, w64, b64 = x.double(), w.double(), b.double()
    rm64, rv64 = rm.double(), rv.double()
    ref = F.batch_norm(x64, rm64, rv64, w64, b64, training=True, momentum=0.1, eps=1e-5)   # (updates rm64 / rv64)
    mu = x64.mean(0)
    dev_ = x64 - mu
    var = (dev_ * dev_).mean(0)
    assert var[CONST_CH].item() < 1e-18
    rstd = torch.rsqrt(var + 1e-5)
    a, mad = x64.abs().mean(0), dev_.abs().mean(0)
    e0 = (D + 1) * EPS * a
    e_d = (D + 1) * EPS * (mad + e0)
    e_mean = e_d + 2 * EPS * (mad + e0) + 2 * EPS * mu.abs()
    e_var = (D + 6) * EPS * (var + e0 * e0) + (e0 + e_d) ** 2 - e0 * e0
    e_rstd = 0.5 * rstd ** 3 * (e_var + 2 * EPS * (var + 1e-5)) + 4 * EPS * rstd
    xhat = dev_ * rstd
    z = xhat * w64 + b64
    e_z = w64.abs() * (rstd * e_mean + dev_.abs() * e_rstd + 3 * EPS * xhat.abs()) + EPS * z.abs()
    if act:
        ref = _silu(ref)
        e_z = L_SILU * e_z + SILU_REL * (ref.abs() + L_SILU * e_z)
    ybuf, y = _written(M * C, cuda)
    sbuf, stat = _written(2 * C, cuda)
    mbuf, rm_io = _added(rm)
    vbuf, rv_io = _added(rv)
    ops.mvt_bn_fwd(x, w, b, rm_io, rv_io, act, y=y, stat=stat)
    worst = {}
    _check("mean", stat[:C], mu, e_mean + 1e-300, worst)
    _check("rstd", stat[C:], rstd, e_rstd, worst)
    _check("run_mean", rm_io, rm64, 0.1 * e_mean + 4 * EPS * (0.9 * rm.double().abs() + 0.1 * mu.abs()), worst)
    unb = M / (M - 1.0)
    _check("run_var", rv_io, rv64, 0.1 * unb * e_var + 6 * EPS * (0.9 * rv.double().abs() + 0.1 * unb * var), worst)
    _check("y", y.view(M, C), ref, e_z, worst)
    assert _intact(ybuf, M * C) and _intact(sbuf, 2 * C) and _intact(mbuf, C) and _intact(vbuf, C), "guard bytes changed"
    _show(f"bn_fwd M={M} C={C} act={act} D={D}", worst)


@gpu
@pytest.mark.parametrize("act", [0, 1], ids=["plain", "silu"])
@pytest.mark.parametrize("M,C", BN_SHAPES, ids=[f"M{m}-C{c}" for m, c in BN_SHAPES])
def test_bn_bwd_against_float64(cuda, M, C, act):
    """dx written, added to, and aliased onto dy (the engine's form); dw and db on top of prior content."""
    g, x, w, b = _bn_inputs(M, C, cuda, M + C + 1)
    dy = torch.randn(M, C, generator=g, device=cuda)
    dx0 = torch.randn(M, C, generator=g, device=cuda)
    dw0, db0 = torch.randn(C, generator=g, device=cuda), torch.randn(C, generator=g, device=cuda)
    D = chain_rows(M, ops.mvt_bn_row_blocks(M))
    x64 = x.double().requires_grad_()
    w64, b64 = w.double().requires_grad_(), b.double().requires_grad_()
    out = F.batch_norm(x64, None, None, w64, b64, training=True, eps=1e-5)
    (_silu(out) if act else out).backward(dy.double())
    dx_ref, dw_ref, db_ref = x64.grad, dw0.double() + w64.grad, db0.double() + b64.grad
    with torch.no_grad():
        x64 = x64.detach()
        w64, b64, dy64 = w64.detach(), b64.detach(), dy.double()
        mu = x64.mean(0)
        dev_ = x64 - mu
        rstd = torch.rsqrt((dev_ * dev_).mean(0) + 1e-5)
        stat = torch.cat([mu, rstd]).float()
        xhat = dev_ * rstd
        z = xhat * w64 + b64
        e_xhat = rstd * EPS * (mu.abs() + dev_.abs()) + 2 * EPS * xhat.abs()
        e_z = w64.abs() * e_xhat + EPS * z.abs()
        if act:
            dz = dy64 * _silu_grad(z)
            e_dz = dy64.abs() * (0.5 * e_z + SILU_REL * (1 + z.abs())) + EPS * dz.abs()
        else:
            dz, e_dz = dy64, torch.zeros_like(dy64)
        S0, S1 = dz.sum(0), (dz * xhat).sum(0)
        e_S0 = e_dz.sum(0) + (D + 1) * EPS * dz.abs().sum(0)
        e_S1 = (e_dz * xhat.abs() + dz.abs() * e_xhat).sum(0) + (D + 1) * EPS * (dz * xhat).abs().sum(0)
        e_in = (e_dz + e_S0 / M + (xhat.abs() * e_S1 + e_xhat * S1.abs()) / M +
                6 * EPS * (dz.abs() + S0.abs() / M + (xhat * S1).abs() / M))
        e_dx = w64.abs() * rstd * e_in + 4 * EPS * dx_ref.abs()
    worst = {}
    for name in ("written", "added", "aliased"):
        acc = name == "added"
        xbuf, dx = _added(dx0) if acc else _added(dy) if name == "aliased" else _written(M * C, cuda)
        wbuf, dw = _added(dw0)
        bbuf, db = _added(db0)
        ops.mvt_bn_bwd(x, dx if name == "aliased" else dy, stat, w, b, act, int(acc), dx, dw, db)
        want = dx0.double() + dx_ref if acc else dx_ref
        _check(f"dx.{name}", dx.view(M, C), want, e_dx + (EPS * want.abs() if acc else 0.0), worst)
        _check(f"dw.{name}", dw, dw_ref, e_S1 + 2 * EPS * dw_ref.abs(), worst)
        _check(f"db.{name}", db, db_ref, e_S0 + 2 * EPS * db_ref.abs(), worst)
        assert _intact(xbuf, M * C) and _intact(wbuf, C) and _intact(bbuf, C), f"{name}: guard bytes changed"
    _show(f"bn_bwd M={M} C={C} act={act} D={D}", worst)


# ---- depthwise 3x3
def _dw3_case(B, H, C, s, dev):
    g = torch.Generator(device=dev).manual_seed(H * 100 + C + s + B)
    x = MV._border_map(B, H, C, "f32", g, dev).contiguous()
    dout = MV._border_map(B, H // s, C, "f32", g, dev).contiguous()
    w = (torch.randn(C, 1, 3, 3, generator=g, device=dev) / 3.0).contiguous()
    bias = 0.1 * torch.randn(C, generator=g, device=dev)
    return g, x, dout, w, bias


def _dw3_autograd(x64, w64, b64, dout64, s):
    """NHWC in, NHWC out: (out, d in, d w, d bias) of F.conv2d(groups = C) in float64."""
    C = x64.shape[3]
    xn = x64.permute(0, 3, 1, 2).contiguous().requires_grad_()
    wn, bn = w64.clone().requires_grad_(), b64.clone().requires_grad_()
    out = F.conv2d(xn, wn, bn, stride=s, padding=1, groups=C)
    out.backward(dout64.permute(0, 3, 1, 2).contiguous())
    return out.detach().permute(0, 2, 3, 1), xn.grad.permute(0, 2, 3, 1), wn.grad, bn.grad


def _dw3_bwd_w_check(tag, x, dout, g, s, worst, dev):
    B, H, _, C = x.shape
    npix = B * (H // s) ** 2
    blocks = ops.mvt_dw3_bwd_w_row_blocks(npix)
    D = chain_rows(npix, blocks)
    dw0 = torch.randn(C, 1, 3, 3, generator=g, device=dev)
    db0 = torch.randn(C, generator=g, device=dev)
    z = torch.zeros(C, dtype=torch.float64, device=dev)
    wdummy = torch.zeros(C, 1, 3, 3, dtype=torch.float64, device=dev)
    _, _, gw, gb = _dw3_autograd(x.double(), wdummy, z, dout.double(), s)
    _, _, mw, mb = _dw3_autograd(x.double().abs(), wdummy, z, dout.double().abs(), s)
    wbuf, dw = _added(dw0)
    bbuf, db = _added(db0)
    ops.mvt_dw3_bwd_w(x, dout, s, dw, db)
    want_w, want_b = dw0.double() + gw, db0.double() + gb
    _check(f"{tag}dw", dw.view(C, 1, 3, 3), want_w, (D + 1) * EPS * mw + EPS * want_w.abs(), worst)
    _check(f"{tag}dbias", db, want_b, D * EPS * (mb + db0.double().abs()) + EPS * want_b.abs(), worst)
    assert _intact(wbuf, 9 * C) and _intact(bbuf, C), "dw / dbias: guard bytes changed"
    return blocks, D


DW3_CASES = [(h, s, c) for h, s in ((7, 1), (14, 1), (14, 2), (8, 2)) for c in (32, 256)]


@gpu
@pytest.mark.parametrize("H,s,C", DW3_CASES, ids=[f"H{h}-s{s}-C{c}" for h, s, c in DW3_CASES])
def test_dw3_train_against_float64(cuda, H, s, C):
    """Forward, input gradient and filter gradient (compared in the [C,1,3,3] layout) of one shape."""
    B, Ho = 3, H // s
    g, x, dout, w, bias = _dw3_case(B, H, C, s, cuda)
    ref, din_ref, _, _ = _dw3_autograd(x.double(), w.double(), bias.double(), dout.double(), s)
    mag, din_mag, _, _ = _dw3_autograd(x.double().abs(), w.double().abs(), bias.double().abs(), dout.double().abs(), s)
    worst = {}
    obuf, out = _written(B * Ho * Ho * C, cuda)
    ops.mvt_dw3_fwd(x, w, bias, s, out=out)
    _check("out", out.view(B, Ho, Ho, C), ref, 11 * EPS * mag, worst)
    ibuf, din = _written(B * H * H * C, cuda)
    ops.mvt_dw3_bwd_in(dout, w, H, s, din=din)
    _check("din", din.view(B, H, H, C), din_ref, 10 * EPS * din_mag, worst)
    assert _intact(obuf, B * Ho * Ho * C) and _intact(ibuf, B * H * H * C), "guard bytes changed"
    _dw3_bwd_w_check("", x, dout, g, s, worst, cuda)
    _show(f"dw3 H={H} s={s} C={C}", worst)


@gpu
def test_dw3_bwd_w_capped_row_blocks(cuda):
    """18816 output pixels: the row blocks are capped at 256 and every row lane walks 4 or 5 pixels."""
    B, H, s, C = DW3_CAPPED
    g, x, dout, _, _ = _dw3_case(B, H, C, s, cuda)
    worst = {}
    blocks, D = _dw3_bwd_w_check("", x, dout, g, s, worst, cuda)
    assert blocks == 256 and D == 5 + 16 + 256
    _show(f"dw3_bwd_w B={B} H={H} s={s} C={C} D={D}", worst)


# ---- attention backward
def _r32(t):
    return t.float().double()


def _attn_explicit(qkv64, table64, dout64, rows, heads, rnd):
    """The attention backward written out, float64; rnd rounds each value the kernel holds in a register or in LDS.
    -> dict(dqkv [N,3C], dtable, and the bound's ingredients)."""
    r = rnd if rnd is not None else (lambda t: t)
    N, U = qkv64.shape[0], rows.shape[0]
    g = qkv64[rows].view(U, 49, heads, 96).permute(0, 2, 1, 3)
    q, k, v = g[..., :32], g[..., 32:64], g[..., 64:]
    dO = dout64[rows].view(U, 49, heads, 32).permute(0, 2, 1, 3)
    bias = rel_bias(table64)[None]                                   # [1][heads][query][key]
    qs = r(q * SC)
    s = r(qs @ k.transpose(-1, -2) + bias)
    e = r(torch.exp(r(s - s.amax(-1, keepdim=True))))
    P = r(e * r(1.0 / r(e.sum(-1, keepdim=True))))
    dP = r(dO @ v.transpose(-1, -2))
    dot = r((P * dP).sum(-1, keepdim=True))
    dS = r(P * r(dP - dot))
    dq, dk, dv = SC * (dS @ k), dS.transpose(-1, -2) @ qs, P.transpose(-1, -2) @ dO
    idx = MO.rel_pos_index(7).view(-1).to(qkv64.device)

    def to_table(db):                                               # [heads][query][key] -> [169][heads]
        return torch.zeros(169, heads, dtype=torch.float64, device=db.device).index_add_(
            0, idx, db.permute(1, 2, 0).reshape(2401, heads))

    def back(*parts):                                               # [U][heads][49][32] x 3 -> [N][3C]
        full = torch.empty(N, heads, 96, dtype=torch.float64, device=qkv64.device)
        full[rows.reshape(-1)] = torch.cat(parts, -1).permute(0, 2, 1, 3).reshape(-1, heads, 96)
        return full.view(N, heads * 96)
    sabs = (q.abs() * SC) @ k.abs().transpose(-1, -2)
    delta = (36 * EPS * sabs + 4 * EPS * (s.abs() + s.abs().amax(-1, keepdim=True))).amax(-1, keepdim=True) + 3 * EPS
    mq, mk = SC * (dS.abs() @ k.abs()), dS.abs().transpose(-1, -2) @ qs.abs()
    bv = ((torch.expm1(2 * delta) + 102 * EPS) * P).transpose(-1, -2) @ dO.abs()
    return dict(dqkv=back(dq, dk, dv), dtable=to_table(dS.sum(0)), mag=back(51 * EPS * mq, 51 * EPS * mk, bv),
                mtable=to_table(dS.abs().sum(0)))


def _attn_autograd(qkv64, table64, dout64, rows, heads):
    qkv = qkv64.clone().requires_grad_()
    table = table64.clone().requires_grad_()
    U = rows.shape[0]
    g = qkv[rows].view(U, 49, heads, 96).permute(0, 2, 1, 3)
    q, k, v = g[..., :32], g[..., 32:64], g[..., 64:]
    P = torch.softmax((q * SC) @ k.transpose(-1, -2) + rel_bias(table)[None], -1)
    o = (P @ v).permute(0, 2, 1, 3).reshape(-1, heads * 32)
    (o * dout64[rows.reshape(-1)]).sum().backward()
    return qkv.grad, table.grad


def attn_bwd_reference(qkv, table, dout, B, H, grid, dev):
    """R (autograd), R~, the 2 E budgets of dq / dk / dtable (asserted small against rms(R)) and the sums' bounds."""
    heads = table.shape[1]
    rows = part_rows(B, H, grid, dev)
    qkv64, table64, dout64 = qkv.double(), table.double(), dout.double()
    Rq, Rt = _attn_autograd(qkv64, table64, dout64, rows, heads)
    X = _attn_explicit(qkv64, table64, dout64, rows, heads, None)
    for got, want in ((X["dqkv"], Rq), (X["dtable"], Rt)):          # the formulas of R~ are those of autograd
        assert (got - want).abs().max().item() <= 1e-11 * (1 + want.abs().max().item())
    Xt = _attn_explicit(qkv64, table64, dout64, rows, heads, _r32)
    N = qkv.shape[0]
    d3 = (Xt["dqkv"] - Rq).abs().view(N, heads, 3, 32)
    R3 = Rq.view(N, heads, 3, 32)
    E, ratio = {}, {}
    for name, i in (("dq", 0), ("dk", 1)):
        E[name] = d3[:, :, i].max().item()
        ratio[name] = 2 * E[name] / max(R3[:, :, i].pow(2).mean().sqrt().item(), 1e-300) if E[name] > 0 else 0.0
    E["dtable"] = (Xt["dtable"] - Rt).abs().max().item()
    ratio["dtable"] = 2 * E["dtable"] / Rt.pow(2).mean().sqrt().item()
    for name, v in ratio.items():
        assert v <= 1e-3, f"{name}: the budget 2 E = {2 * E[name]:.3e} is {v:.3e} of rms(R)"
    units = B * (H // 7) ** 2
    per = ops.mvt_attn_bwd_groups_per_head(units, heads)
    D = _cdiv(units, per) + per + 49 + 1
    budget = torch.zeros(N, heads, 3, 32, dtype=torch.float64, device=dev)
    budget[:, :, 0] = 2 * E["dq"]
    budget[:, :, 1] = 2 * E["dk"]
    return dict(dqkv=Rq, dtable=Rt, dqkv_bound=X["mag"] + budget.view(N, heads * 96),
                dtable_bound=2 * E["dtable"] + D * EPS * X["mtable"], ratio=ratio, D=D, units=units, per=per)


def _run_attn_bwd(tag, qkv, table, dout, B, H, grid, dev, worst):
    N, C3 = qkv.shape
    heads = table.shape[1]
    g = torch.Generator(device=dev).manual_seed(N + heads)
    dt0 = torch.randn(169, heads, generator=g, device=dev)
    R = attn_bwd_reference(qkv, table, dout, B, H, grid, dev)
    qbuf, dqkv = _written(N * C3, dev)
    tbuf, dtable = _added(dt0)
    ops.mvt_attn_bwd(qkv, table, dout, B, H, grid, dtable, dqkv=dqkv.view(N, C3))
    got = dqkv.view(N, heads, 96)
    want, bound = R["dqkv"].view(N, heads, 96), R["dqkv_bound"].view(N, heads, 96)
    for name, sl in (("dq", slice(0, 32)), ("dk", slice(32, 64)), ("dv", slice(64, 96))):
        _check(f"{tag}{name}", got[..., sl], want[..., sl], bound[..., sl], worst)
    want_t = dt0.double() + R["dtable"]
    _check(f"{tag}dtable", dtable.view(169, heads), want_t, R["dtable_bound"] + EPS * want_t.abs(), worst)
    assert _intact(qbuf, N * C3) and _intact(tbuf, 169 * heads), f"{tag}: guard bytes changed"
    return R, got


def _attn_inputs(B, H, C, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    N = B * H * H
    qkv = torch.randn(N, 3 * C, generator=g, device=dev)
    table = torch.randn(169, C // 32, generator=g, device=dev)
    dout = torch.randn(N, C, generator=g, device=dev)
    return qkv, table, dout


ATTN_HC = [(h, c) for h in (7, 14, 21) for c in (64, 128, 512)]


@gpu
@pytest.mark.parametrize("grid", [0, 1], ids=["window", "grid"])
@pytest.mark.parametrize("H,C", ATTN_HC, ids=[f"H{h}-C{c}" for h, c in ATTN_HC])
def test_attn_bwd_against_float64(cuda, H, C, grid):
    B = 3
    qkv, table, dout = _attn_inputs(B, H, C, cuda, H + C + grid)
    worst = {}
    R, _ = _run_attn_bwd("", qkv, table, dout, B, H, grid, cuda, worst)
    print(f"[attn_bwd H={H} C={C} grid={grid} D={R['D']}] 2E/rms " + " ".join(f"{k}={v:.2e}" for k, v in R["ratio"].items()))
    _show(f"attn_bwd H={H} C={C} grid={grid}", worst)


@gpu
@pytest.mark.parametrize("grid", [0, 1], ids=["window", "grid"])
@pytest.mark.parametrize("H,C", ATTN_HC, ids=[f"H{h}-C{c}" for h, c in ATTN_HC])
def test_attn_bwd_index_map_probes(cuda, H, C, grid):
    """q = k = 0.  Zero table: P is exactly fl(1 / 49), so dv is the mean of dO (integers in [-120, 120]) over exactly the
    row's own partition and head, and dq = dk = 0 exactly.  Random table: P = softmax(bias); a transposed bias gradient
    or a swapped head fails dtable by O(1)."""
    B, heads = 3, C // 32
    N = B * H * H
    g = torch.Generator(device=cuda).manual_seed(H * 10 + C + grid)
    qkv = torch.zeros(N, heads, 96, device=cuda)
    qkv[..., 64:] = torch.randn(N, heads, 32, generator=g, device=cuda)
    qkv = qkv.view(N, 3 * C)
    dout = torch.randint(-120, 121, (N, C), generator=g, device=cuda).float()
    worst = {}
    for name, table in (("probe1.", torch.zeros(169, heads, device=cuda)),
                        ("probe2.", torch.randn(169, heads, generator=g, device=cuda))):
        _, got = _run_attn_bwd(name, qkv, table, dout, B, H, grid, cuda, worst)
        assert int(torch.count_nonzero(got[..., :64])) == 0, f"{name} dq / dk are not exactly zero"
        if name == "probe1.":   # ... once more in plain terms, from the oracle's partition functions alone
            d = dout.double().view(B, H, H, C)
            part = MO.grid_partition(d, 7) if grid else MO.window_partition(d, 7)
            mean = part.mean((1, 2), keepdim=True).expand_as(part).contiguous()
            full = (MO.grid_reverse(mean, 7, H, H) if grid else MO.window_reverse(mean, 7, H, H)).reshape(N, heads, 32)
            _check("probe1.mean", got[..., 64:], full, torch.full_like(full, 60 * EPS * 120.0), worst)
    _show(f"attn_bwd probes H={H} C={C} grid={grid}", worst)


@gpu
@pytest.mark.parametrize("C,H,B", WALK_ATTN, ids=[f"C{c}-H{h}-B{b}" for c, h, b in WALK_ATTN])
def test_attn_bwd_workgroups_walk_units(cuda, C, H, B):
    """More units than workgroups per head, raggedly: the bias gradient is carried in registers across a workgroup's
    units, the LDS images are rewritten behind a barrier, the last trip is short (test_train_grid_arithmetic)."""
    qkv, table, dout = _attn_inputs(B, H, C, cuda, C + B)
    worst = {}
    R, _ = _run_attn_bwd("", qkv, table, dout, B, H, 0, cuda, worst)
    assert R["per"] < R["units"] < 2 * R["per"] and R["D"] == 2 + R["per"] + 50, (R["units"], R["per"], R["D"])
    print(f"[attn_bwd walk C={C} H={H} B={B}: {R['units']} units on {R['per']} workgroups per head] 2E/rms " +
          " ".join(f"{k}={v:.2e}" for k, v in R["ratio"].items()))
    _show(f"attn_bwd walk C={C} H={H} B={B}", worst)


# ---- squeeze-excite
SE_SHAPES = [(49, 2048, 128), (196, 256, 16), (50, 64, 30)]


@gpu
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("P,C,RD", SE_SHAPES, ids=[f"P{p}-C{c}-RD{r}" for p, c, r in SE_SHAPES])
def test_se_train_against_float64(cuda, P, C, RD, B):
    """Forward: all five outputs.  Backward (the MBConv backward's launch chain): d_a2 and the four parameter gradients
    on top of prior content."""
    g = torch.Generator(device=cuda).manual_seed(P + C + RD + B)

    def rn(*s, scale=1.0):
        return (scale * torch.randn(*s, generator=g, device=cuda)).contiguous()
    a2 = rn(B, P, C)
    w1, b1, w2, b2 = rn(RD, C, scale=C ** -0.5), rn(RD, scale=0.1), rn(C, RD, scale=RD ** -0.5), rn(C, scale=0.1)
    dg = rn(B, P, C)
    prior = [rn(RD, C), rn(RD), rn(C, RD), rn(C)]
    a64 = a2.double().requires_grad_()
    pw = [t.double().requires_grad_() for t in (w1, b1, w2, b2)]
    pool = a64.mean(1)
    rpre = pool @ pw[0].t() + pw[1]
    r = _silu(rpre)
    pre2 = r @ pw[2].t() + pw[3]
    gate = torch.sigmoid(pre2)
    gated = a64 * gate[:, None, :]
    gated.backward(dg.double())
    refs = [t.detach() for t in (pool, rpre, r, gate, gated)]
    worst = {}
    with torch.no_grad():
        a, W1, B1, W2, B2 = a64.detach(), *(t.detach() for t in pw)
        pool, rpre, r, gate, gated = refs
        Dp = _cdiv(P, 16) + 16 + 2
        e_pool = Dp * EPS * a.abs().mean(1)
        e1 = chain_lin(C) * EPS * (pool.abs() @ W1.abs().t() + B1.abs()) + e_pool @ W1.abs().t()
        e_r = L_SILU * e1 + SILU_REL * (r.abs() + L_SILU * e1)
        e2 = chain_lin(RD) * EPS * (r.abs() @ W2.abs().t() + B2.abs()) + e_r @ W2.abs().t()
        e_g = 0.25 * e2 + SILU_REL * gate
        e_gated = a.abs() * e_g[:, None, :] + EPS * gated.abs()
    shapes = [(B, C), (B, RD), (B, RD), (B, C), (B, P, C)]
    bufs = [_written(torch.Size(s).numel(), cuda) for s in shapes]
    ops.mvt_se_fwd(a2, w1, b1, w2, b2, out=[t for _, t in bufs])
    for name, (buf, t), s, ref, e in zip(("pool", "rpre", "r", "gate", "gated"), bufs, shapes, refs,
                                        (e_pool, e1, e_r, e_g, e_gated)):
        _check(name, t.view(s), ref, e, worst)
        assert _intact(buf, t.numel()), f"{name}: guard bytes changed"
    # backward from the float64 forward's values rounded to fp32 (one EPS each)
    f32 = [t.float().contiguous() for t in refs[:4]]
    with torch.no_grad():
        d = dg.double()
        dgate = (d * a).sum(1)
        e_dgate = Dp * EPS * (d * a).abs().sum(1)
        gg = gate * (1 - gate)
        dgpre = dgate * gg
        e_dgpre = 0.25 * e_dgate + EPS * dgate.abs() * (4 * gg + gate)
        rr, pp = r.abs() * (1 + EPS), pool.abs() * (1 + EPS)
        e_dw2 = e_dgpre.t() @ rr + (B + 2) * EPS * (dgpre.abs().t() @ rr)
        e_db2 = e_dgpre.sum(0) + (B + 1) * EPS * dgpre.abs().sum(0)
        dr = dgpre @ W2
        e_dr = e_dgpre @ W2.abs() + chain_lin(C) * EPS * (dgpre.abs() @ W2.abs())
        drpre = dr * _silu_grad(rpre)
        e_drpre = L_SILU * e_dr + dr.abs() * (SILU_REL * (1 + rpre.abs()) + 0.5 * EPS * rpre.abs()) + EPS * drpre.abs()
        e_dw1 = e_drpre.t() @ pp + (B + 2) * EPS * (drpre.abs().t() @ pp)
        e_db1 = e_drpre.sum(0) + (B + 1) * EPS * drpre.abs().sum(0)
        dpool = drpre @ W1
        e_dpool = e_drpre @ W1.abs() + chain_lin(RD) * EPS * (drpre.abs() @ W1.abs())
        da_ref = a64.grad
        e_da = (3 * EPS * (d * gate[:, None, :]).abs() + ((e_dpool + 2 * EPS * dpool.abs()) / P)[:, None, :] +
                EPS * da_ref.abs())
    gb = [_added(t) for t in prior]
    abuf, d_a2 = _written(B * P * C, cuda)
    ops.mvt_se_bwd(dg, a2, *f32, w1, w2, *(t for _, t in gb), d_a2=d_a2)
    _check("d_a2", d_a2.view(B, P, C), da_ref, e_da, worst)
    assert _intact(abuf, B * P * C), "d_a2: guard bytes changed"
    for name, (buf, t), p0, gref, e in zip(("d_fc1_w", "d_fc1_b", "d_fc2_w", "d_fc2_b"), gb, prior,
                                          (t.grad for t in pw), (e_dw1, e_db1, e_dw2, e_db2)):
        want = p0.double() + gref
        _check(name, t.view(p0.shape), want, e + EPS * want.abs(), worst)
        assert _intact(buf, t.numel()), f"{name}: guard bytes changed"
    _show(f"se P={P} C={C} RD={RD} B={B}", worst)


# ---- the remaining kernels
@gpu
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("H", [2, 14])
def test_avgpool2_bwd(cuda, H, accumulate):
    B, C = 3, 20
    g = torch.Generator(device=cuda).manual_seed(H)
    gr = torch.randn(B, H // 2, H // 2, C, generator=g, device=cuda)
    dx0 = torch.randn(B, H, H, C, generator=g, device=cuda)
    buf, dx = _added(dx0) if accumulate else _written(dx0.numel(), cuda)
    ops.mvt_avgpool2_bwd(gr, dx.view(B, H, H, C), accumulate)
    up = 0.25 * gr.double().repeat_interleave(2, 1).repeat_interleave(2, 2)
    want = dx0.double() + up if accumulate else up
    worst = {}
    _check("dx", dx.view(B, H, H, C), want, EPS * want.abs() if accumulate else torch.zeros_like(want), worst)
    assert _intact(buf, dx0.numel()), "guard bytes changed"
    _show(f"avgpool2_bwd H={H} accumulate={accumulate}", worst)


@gpu
@pytest.mark.parametrize("C", [4, 32])
@pytest.mark.parametrize("H", [3, 14])
def test_col2im3(cuda, H, C):
    """Against autograd through a float64 im2col written with F.pad and slices (tap-major columns)."""
    B = 3
    g = torch.Generator(device=cuda).manual_seed(H + C)
    dcol = torch.randn(B, H, H, 9 * C, generator=g, device=cuda)

    def im2col(t):
        tp = F.pad(t, (0, 0, 1, 1, 1, 1))
        return torch.cat([tp[:, ky:ky + H, kx:kx + H, :] for ky in range(3) for kx in range(3)], -1)
    x = torch.zeros(B, H, H, C, dtype=torch.float64, device=cuda, requires_grad=True)
    im2col(x).backward(dcol.double())
    xa = torch.zeros_like(x).requires_grad_()
    im2col(xa).backward(dcol.double().abs())
    buf, din = _written(B * H * H * C, cuda)
    ops.mvt_col2im3(dcol, din=din)
    worst = {}
    _check("din", din.view(B, H, H, C), x.grad, 9 * EPS * xa.grad, worst)
    assert _intact(buf, B * H * H * C), "guard bytes changed"
    _show(f"col2im3 H={H} C={C}", worst)


@gpu
@pytest.mark.parametrize("O,C,ldp", [(32, 3, 32), (64, 32, 288)])
def test_unpack_conv3_grad(cuda, O, C, ldp):
    """The packed row pitch differs from 9 C in the stem's first convolution (27 of 32); the pad columns hold NaN."""
    g = torch.Generator(device=cuda).manual_seed(O + C)
    gp = torch.full((O, ldp), NAN, device=cuda)
    gp[:, :9 * C] = torch.randn(O, 9 * C, generator=g, device=cuda)
    g0 = torch.randn(O, C, 3, 3, generator=g, device=cuda)
    buf, out = _added(g0)
    ops.mvt_unpack_conv3_grad(gp, out.view(O, C, 3, 3))
    want = g0.double() + gp[:, :9 * C].double().view(O, 3, 3, C).permute(0, 3, 1, 2)
    worst = {}
    _check("g", out.view(O, C, 3, 3), want, EPS * want.abs(), worst)
    assert _intact(buf, g0.numel()), "guard bytes changed"
    _show(f"unpack_conv3_grad O={O} C={C} ldp={ldp}", worst)


@gpu
def test_gelu_fwd_and_bwd(cuda):
    """A length that is 4 mod 1024 (one thread of the last workgroup), against the erf GELU in float64."""
    n = 3 * 1024 + 4
    g = torch.Generator(device=cuda).manual_seed(n)
    pre = 2.5 * torch.randn(n, generator=g, device=cuda)
    d0 = torch.randn(n, generator=g, device=cuda)
    p64 = pre.double()
    worst = {}
    obuf, out = _written(n, cuda)
    ops.mvt_gelu_fwd(pre, out=out)
    _check("gelu", out, GP.gelu_erf(p64), GP._gelu_f("f32", p64), worst)
    dbuf, d = _added(d0)
    ops.mvt_gelu_bwd(pre, d)
    want = d0.double() * GP.gelu_erf_grad(p64)
    _check("gelu_bwd", d, want, d0.double().abs() * GP._gelu_grad_f("f32", p64) + EPS * want.abs(), worst)
    assert _intact(obuf, n) and _intact(dbuf, n), "guard bytes changed"
    _show(f"gelu n={n}", worst)


@gpu
def test_bcast_set(cuda):
    B, P, C = 3, 49, 36
    g = torch.Generator(device=cuda).manual_seed(1)
    v = torch.randn(B, C, generator=g, device=cuda)
    scale = 1.0 / 49.0
    buf, out = _written(B * P * C, cuda)
    ops.mvt_bcast_set(v, P, scale, out=out)
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    want = (v.double() * s32)[:, None, :].expand(B, P, C)
    worst = {}
    _check("d", out.view(B, P, C), want, EPS * want.abs(), worst)
    assert _intact(buf, B * P * C), "guard bytes changed"
    _show("bcast_set", worst)


# ---- refusals: an error with a message, nothing launched, the guarded outputs untouched
class _Refusals:
    def __init__(self, dev, who):
        self.dev, self.who, self.outs = dev, who, []

    def out(self, n):
        buf, t = _written(n, self.dev)
        self.outs.append((buf, t))
        return GP._p(t)

    def refused(self, fn, *args, match=None):
        L = _lib.lib()
        assert getattr(L, "btsbot_op_mvt_" + fn)(*args) == _lib.ERR_INVALID_ARG, (fn, args)
        msg = L.btsbot_last_error()
        assert msg.startswith(b"op_mvt_" + fn.encode()) and (match is None or match in msg), msg
        torch.cuda.synchronize()
        for buf, t in self.outs:
            assert _intact(buf, t.numel()) and bool(torch.isnan(t).all()), f"{fn}: a refused call wrote its output"


@gpu
def test_bn_refusals(cuda):
    R = _Refusals(cuda, "bn")
    z = torch.zeros(64 * 8, device=cuda)
    P, st = GP._p, ops._stream(z)
    x, y, s, dw, db = P(z), R.out(64 * 8), R.out(16), R.out(8), R.out(8)
    for i in range(7):
        a = [x, x, x, x, x, y, s]
        a[i] = None                                                  # (3, 4: one running statistic without the other)
        R.refused("bn_fwd", *a, 64, 8, 0, st, match=b"null")
    R.refused("bn_fwd", x, x, x, None, None, y, s, 64, 6, 0, st, match=b"multiple of 4")
    R.refused("bn_fwd", x, x, x, None, None, y, s, 0, 8, 0, st)
    R.refused("bn_fwd", x, x, x, None, None, y, s, 64, 8, 2, st)
    for i in range(8):
        a = [x, x, x, x, x, y, dw, db]
        a[i] = None
        R.refused("bn_bwd", *a, 64, 8, 0, 0, st, match=b"null")
    R.refused("bn_bwd", x, x, x, x, x, y, dw, db, 64, 10, 0, 0, st, match=b"multiple of 4")
    R.refused("bn_bwd", x, x, x, x, x, y, dw, db, 64, 8, 0, 2, st)


@gpu
def test_dw3_train_refusals(cuda):
    R = _Refusals(cuda, "dw3")
    z = torch.zeros(2 * 8 * 8 * 8, device=cuda)
    P, st = GP._p, ops._stream(z)
    x, o, dw, db = P(z), R.out(z.numel()), R.out(72), R.out(8)
    for fn, ptrs in (("dw3_fwd", [x, x, x, o]), ("dw3_bwd_in", [x, x, o]), ("dw3_bwd_w", [x, x, dw, db])):
        for i in range(len(ptrs)):
            a = list(ptrs)
            a[i] = None
            R.refused(fn, *a, 2, 8, 8, 1, st, match=b"null")
        R.refused(fn, *ptrs, 2, 8, 6, 1, st, match=b"multiple of 4")      # C % 4
        R.refused(fn, *ptrs, 2, 7, 8, 2, st, match=b"stride")             # H % stride
        R.refused(fn, *ptrs, 2, 8, 8, 3, st, match=b"stride")             # a stride other than 1 or 2
        R.refused(fn, *ptrs, 2, 8, 8, 0, st, match=b"stride")


@gpu
def test_attn_bwd_refusals(cuda):
    R = _Refusals(cuda, "attn_bwd")
    z = torch.zeros(49 * 192, device=cuda)
    P, st = GP._p, ops._stream(z)
    x, dq, dt = P(z), R.out(49 * 192), R.out(169 * 2)
    for i in range(5):
        a = [x, x, x, dq, dt]
        a[i] = None
        R.refused("attn_bwd", *a, 1, 7, 64, 0, st, match=b"null")
    R.refused("attn_bwd", x, x, x, dq, dt, 1, 8, 64, 0, st, match=b"multiple of 7")     # H % 7
    R.refused("attn_bwd", x, x, x, dq, dt, 1, 7, 48, 0, st)                             # C % 32
    R.refused("attn_bwd", x, x, x, dq, dt, 1, 7, 544, 0, st, match=b"16 heads")         # 17 heads
    R.refused("attn_bwd", x, x, x, dq, dt, 1, 7, 64, 2, st)


@gpu
def test_se_train_refusals(cuda):
    R = _Refusals(cuda, "se")
    z = torch.zeros(2 * 4 * 8, device=cuda)
    P, st = GP._p, ops._stream(z)
    x = P(z)
    outs = [R.out(64) for _ in range(5)]
    for i in range(10):
        a = [x] * 5 + outs
        a[i] = None
        R.refused("se_fwd", *a, 2, 4, 8, 2, st, match=b"null")
    R.refused("se_fwd", *([x] * 5 + outs), 2, 4, 6, 2, st, match=b"multiple of 4")
    R.refused("se_fwd", *([x] * 5 + outs), 2, 4, 8, 0, st)
    for i in range(13):
        a = [x] * 8 + outs
        a[i] = None
        R.refused("se_bwd", *a, 2, 4, 8, 2, st, match=b"null")
    R.refused("se_bwd", *([x] * 8 + outs), 2, 4, 10, 2, st, match=b"multiple of 4")
    R.refused("se_bwd", *([x] * 8 + outs), 2, 0, 8, 2, st)


@gpu
def test_small_kernel_refusals(cuda):
    R = _Refusals(cuda, "small")
    z = torch.zeros(1024, device=cuda)
    P, st = GP._p, ops._stream(z)
    x, o = P(z), R.out(1024)
    R.refused("avgpool2_bwd", None, o, 1, 2, 4, 0, st, match=b"null")
    R.refused("avgpool2_bwd", x, None, 1, 2, 4, 0, st, match=b"null")
    R.refused("avgpool2_bwd", x, o, 1, 3, 4, 0, st, match=b"even")
    R.refused("avgpool2_bwd", x, o, 1, 2, 4, 2, st)
    R.refused("col2im3", None, o, 1, 3, 4, st, match=b"null")
    R.refused("col2im3", x, None, 1, 3, 4, st, match=b"null")
    R.refused("col2im3", x, o, 1, 0, 4, st)
    R.refused("unpack_conv3_grad", None, o, 4, 3, 32, st, match=b"null")
    R.refused("unpack_conv3_grad", x, None, 4, 3, 32, st, match=b"null")
    R.refused("unpack_conv3_grad", x, o, 4, 3, 26, st, match=b"ldp")
    for fn in ("gelu_fwd", "gelu_bwd"):
        R.refused(fn, None, o, 8, st, match=b"null")
        R.refused(fn, x, None, 8, st, match=b"null")
        R.refused(fn, x, o, 6, st, match=b"multiple of 4")
    R.refused("bcast_set", None, o, 1, 4, 4, 1.0, st, match=b"null")
    R.refused("bcast_set", x, None, 1, 4, 4, 1.0, st, match=b"null")
    R.refused("bcast_set", x, o, 1, 0, 4, 1.0, st)
