"""Thin tensor-level wrappers over the op-level C entry points (include/btsbot_hip.h,
``btsbot_op_*``).  Used by the op parity tests and the kernel micro-benchmarks; the model classes
call ``btsbot_forward`` instead.  HIP tensors only -- no CPU fallback."""
import ctypes as C

import torch

from . import _lib

_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _stream(t):
    if t.device.type != "cuda":
        raise RuntimeError("btsbot_amd.ops: tensors must live on a HIP device (no CPU fallback)")
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


_EPI = {"gelu": 0, "resid": 1, "bias": 2, "gelu_save": 3, "dgelu": 4, "plain": 5, "silu": 6, "bias_t": 7}


def gemm(x, w, bias, epi="bias", gamma=None, resid=None, precision="f32", out=None):
    """epi in {'gelu','resid','bias','silu','bias_t'} and the training ones {'gelu_save','dgelu','plain'}; x [M,K],
    w [N,K] in the precision's dtype ('f16x2': fp32 x and w, w split into f16 head + remainder inside, every output
    fp32).  'gelu' / 'silu' / 'bias_t' write the precision's dtype, 'resid' / 'bias' and the training epilogues fp32.
    'gelu_save': resid <- acc + bias (the pre-activation), out = gelu(resid); 'dgelu': out = acc * gelu'(resid);
    'plain': out = acc ('dgelu' / 'plain' read no bias: None is fine).  The training epilogues take precision 'f32' or
    'f16x2' only; every tensor of theirs is fp32, and 'gelu_save' / 'dgelu' need resid.  out: the output tensor (for
    'resid' it may be resid itself: in place)."""
    train_epi = epi in ("gelu_save", "dgelu", "plain")
    if train_epi and precision not in ("f32", "f16x2"):
        raise ValueError(f"ops.gemm: the training epilogue {epi!r} takes precision 'f32' or 'f16x2', got {precision!r}")
    dt = torch.float32 if precision == "f16x2" else _DT[precision]
    assert x.dtype == dt and w.dtype == dt and x.is_contiguous() and w.is_contiguous()
    M, K = x.shape
    N = w.shape[0]
    e = _EPI[epi]
    if epi in ("gelu_save", "dgelu"):
        if resid is None:
            raise ValueError(f"ops.gemm: {epi!r} needs resid (the fp32 pre-activation [M, N])")
        assert resid.dtype == torch.float32 and resid.shape == (M, N) and resid.is_contiguous()
    if bias is None and epi in ("dgelu", "plain"):
        bias = torch.zeros(N, dtype=torch.float32, device=x.device)
    odt = torch.float32 if train_epi else dt if epi in ("gelu", "silu", "bias_t") else torch.float32
    if out is None:
        out = torch.empty(M, N, dtype=odt, device=x.device)
    assert out.dtype == odt and out.shape == (M, N) and out.is_contiguous()
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().btsbot_op_gemm(_lib.PRECISION[precision], e, _p(x), _p(w), _p(bias),
                                             _p(gamma), _p(resid), _p(out), M, N, K, _stream(x)),
                   "btsbot_op_gemm")
    return out


def wgrad(d, a, out=None, colsum=None, precision="f32"):
    """Filter gradient of a 1x1 convolution: out[n][k] += sum_m d[m][n] a[m][k] (and colsum[n] += sum_m d[m][n] when
    colsum is given).  d [M,N], a [M,K] in the precision's dtype (fp32 for 'f16x2'); out [N,K] fp32 (zeros when None).
    precision 'f32' (the fp32 training kernel), 'bf16' / 'f16' (the 16-bit training kernel: N, K multiples of 8) or
    'f16x2' (the split training form: N, K multiples of 16)."""
    assert precision in ("f32", "bf16", "f16", "f16x2"), precision
    dt = torch.float32 if precision == "f16x2" else _DT[precision]
    assert d.dtype == dt and a.dtype == dt and d.is_contiguous() and a.is_contiguous()
    M, N = d.shape
    K = a.shape[1]
    assert a.shape[0] == M
    if out is None:
        out = torch.zeros(N, K, dtype=torch.float32, device=d.device)
    assert out.dtype == torch.float32 and out.shape == (N, K) and out.is_contiguous()
    if colsum is not None:
        assert colsum.dtype == torch.float32 and colsum.shape == (N,) and colsum.is_contiguous()
    with torch.cuda.device(d.device):
        _lib.check(_lib.lib().btsbot_op_wgrad(_lib.PRECISION[precision], _p(d), _p(a), _p(out), _p(colsum), M, N, K,
                                              _stream(d)), "btsbot_op_wgrad")
    return out


def gemm_gated(x, gate, rows_per_alert, w, resid, precision="f32", out=None):
    """out (fp32) = resid + (x[m][k] * gate[m // rows_per_alert][k]) @ w^T: the squeeze-excite gated 1x1 convolution of
    a MaxViT MBConv block.  x [M,K], w [N,K] in the precision's dtype (fp32 for 'f16x2'); gate [ceil(M / rows), K] and
    resid [M,N] fp32.  out may be resid itself (in place)."""
    dt = torch.float32 if precision == "f16x2" else _DT[precision]
    assert x.dtype == dt and w.dtype == dt and x.is_contiguous() and w.is_contiguous()
    M, K = x.shape
    N = w.shape[0]
    assert gate.dtype == torch.float32 and gate.is_contiguous() and gate.shape == ((M + rows_per_alert - 1) // rows_per_alert, K)
    assert resid.dtype == torch.float32 and resid.shape == (M, N) and resid.is_contiguous()
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.shape == (M, N) and out.is_contiguous()
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().btsbot_op_gemm_gated(_lib.PRECISION[precision], _p(x), _p(gate), rows_per_alert, _p(w),
                                                   _p(resid), _p(out), M, N, K, _stream(x)), "btsbot_op_gemm_gated")
    return out


def gemm_resid_ln(x, w, resid, ln_w=None, ln_b=None, precision="bf16", out=None):
    """The batched residual GEMM of the 16-bit MaxViT forward: out[b] (fp32) = resid[b] + x[b] @ w[b]^T for x [B,M,K],
    w [B,N,K] ('bf16' / 'f16'), resid [B,M,N] fp32 (out may be resid itself).  With ln_w / ln_b (N 64 or 128) it also
    returns LayerNorm_N(out) * ln_w + ln_b (eps 1e-6) in the precision's dtype: (out, ln_out); else out."""
    dt = _DT[precision]
    assert precision in ("bf16", "f16") and x.dtype == dt and w.dtype == dt and x.is_contiguous() and w.is_contiguous()
    B, M, K = x.shape
    N = w.shape[1]
    assert w.shape == (B, N, K) and resid.dtype == torch.float32 and resid.shape == (B, M, N) and resid.is_contiguous()
    if out is None:
        out = torch.empty(B, M, N, dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.shape == (B, M, N) and out.is_contiguous()
    ln_out = None
    if ln_w is not None:
        ln_out = torch.empty(B, M, N, dtype=dt, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().btsbot_op_gemm_resid_ln(_lib.PRECISION[precision], _p(x), _p(w), _p(resid), _p(out), B, M,
                                                      N, K, _p(ln_w), _p(ln_b), _p(ln_out), _stream(x)),
                   "btsbot_op_gemm_resid_ln")
    return out if ln_out is None else (out, ln_out)


def dwconv_ln(x, w, bias, ln_w, ln_b, precision="f32"):
    """x [B,HW,HW,C] f32 NHWC; w [C,1,7,7] as PyTorch stores it."""
    B, HW, _, Cc = x.shape
    wt = w.reshape(Cc, 49).t().contiguous()
    out = torch.empty(B, HW, HW, Cc, dtype=_DT[precision], device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().btsbot_op_dwconv_ln(_lib.PRECISION[precision], _p(x), _p(wt), _p(bias),
                                                  _p(ln_w), _p(ln_b), _p(out), B, HW, Cc,
                                                  _stream(x)), "btsbot_op_dwconv_ln")
    return out


def stem(img, w, bias, ln_w, ln_b):
    B, C0 = img.shape[0], w.shape[0]
    out = torch.empty(B, 225, C0, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        _lib.check(_lib.lib().btsbot_op_stem(_p(img), _p(w.contiguous()), _p(bias), _p(ln_w),
                                             _p(ln_b), _p(out), B, C0, _stream(img)),
                   "btsbot_op_stem")
    return out


def ln_patch(x, ln_w, ln_b, precision="f32"):
    B, HW, _, Cin = x.shape
    HO = HW // 2
    out = torch.empty(B * HO * HO, 4 * Cin, dtype=_DT[precision], device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().btsbot_op_ln_patch(_lib.PRECISION[precision], _p(x), _p(ln_w), _p(ln_b),
                                                 _p(out), B, HW, Cin, _stream(x)),
                   "btsbot_op_ln_patch")
    return out


# ---- the MaxViT branch's kernels one at a time (btsbot_op_mv_*): parameters fp32 in the state-dict layout, activations
# NHWC pixel rows; grid_mode 0 = 7x7 windows, 1 = the 7x7 dilated grid
def _f32(*ts):
    for t in ts:
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous()), "fp32 contiguous parameters"


def mv_attn(qkv, table, B, H, grid_mode, impl=0, precision="f32", out=None):
    """qkv [B*H*H, 3C] (channel order [head][q|k|v][32]), table [169, C/32] fp32 -> out [B*H*H, C].  impl 0: the
    per-query kernel ('f32' / 'bf16' / 'f16'); impl 1: the MFMA kernel ('bf16' / 'f16')."""
    dt = _DT[precision]
    assert qkv.dtype == dt and qkv.is_contiguous() and qkv.shape[0] == B * H * H
    Cc = qkv.shape[1] // 3
    _f32(table)
    assert table.shape == (169, Cc // 32)
    if out is None:
        out = torch.empty(B * H * H, Cc, dtype=dt, device=qkv.device)
    assert out.dtype == dt and out.shape == (B * H * H, Cc) and out.is_contiguous()
    with torch.cuda.device(qkv.device):
        _lib.check(_lib.lib().btsbot_op_mv_attn(_lib.PRECISION[precision], impl, _p(qkv), _p(table), _p(out), B, H, Cc,
                                                grid_mode, _stream(qkv)), "btsbot_op_mv_attn")
    return out


def mv_attn_block(xn, x, p, B, H, grid_mode, precision="bf16", xn2=None):
    """C = 64: x (fp32, in place) += proj(attention(qkv(xn))), returns xn2 = LayerNorm2(x) in the precision's dtype.
    p: dict with qkv_w [192,64], qkv_b, proj_w [64,64], proj_b, table [169,2], ln2_w, ln2_b (fp32)."""
    dt = _DT[precision]
    assert xn.dtype == dt and xn.is_contiguous() and xn.shape == (B * H * H, 64)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape == (B * H * H, 64)
    ks = ("qkv_w", "qkv_b", "proj_w", "proj_b", "table", "ln2_w", "ln2_b")
    _f32(*(p[k] for k in ks))
    if xn2 is None:
        xn2 = torch.empty_like(xn)
    assert xn2.dtype == dt and xn2.shape == xn.shape and xn2.is_contiguous()
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().btsbot_op_mv_attn_block(_lib.PRECISION[precision], _p(xn), _p(x), _p(xn2),
                                                      *(_p(p[k]) for k in ks), B, H, grid_mode, _stream(x)),
                   "btsbot_op_mv_attn_block")
    return xn2


def mv_part(x, p, B, H, grid_mode, precision="bf16", mlp=True, post=None, post_out=None):
    """C in {64, 128, 256}: x [B*H*H, C] fp32 in place, x += proj(attention(qkv(LN1(x)))) and with mlp
    x += fc2(gelu(fc1(LN2(x)))).  p: dict with ln1_w, ln1_b, qkv_w, qkv_b, proj_w, proj_b, table and (mlp) ln2_w,
    ln2_b, fc1_w, fc1_b, fc2_w, fc2_b.  post = (scale [C], shift [C]): also returns post_out = x * scale + shift in
    the precision's dtype."""
    dt = _DT[precision]
    Cc = x.shape[1]
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape == (B * H * H, Cc)
    ka = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "table")
    km = ("ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
    args = [p[k] for k in ka] + [p[k] if mlp else None for k in km]
    _f32(*args)
    ps = pb = None
    if post is not None:
        ps, pb = post
        _f32(ps, pb)
        if post_out is None:
            post_out = torch.empty(B * H * H, Cc, dtype=dt, device=x.device)
        assert post_out.dtype == dt and post_out.shape == x.shape and post_out.is_contiguous()
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().btsbot_op_mv_part(_lib.PRECISION[precision], _p(x), *(_p(a) for a in args), _p(ps), _p(pb),
                                                _p(post_out), B, H, Cc, grid_mode, _stream(x)), "btsbot_op_mv_part")
    return post_out


def mv_dw3_groups(H, C, stride):
    return _lib.check(_lib.lib().btsbot_op_mv_dw3_groups(H, C, stride), "btsbot_op_mv_dw3_groups")


def mv_dw3(x, w, scale, bias, stride, impl=0, precision="f32", out=None, part=None):
    """x [B,H,H,C] -> silu(dw3x3_s(x, w [C,1,3,3]) * scale + bias) [B,H/s,H/s,C].  impl 1 ('bf16' / 'f16') also fills
    part [B, mv_dw3_groups(H, C, s), C] fp32, the squeeze-excite pool's partial sums, and returns (out, part)."""
    dt = _DT[precision]
    B, H, _, Cc = x.shape
    assert x.dtype == dt and x.is_contiguous()
    _f32(w, scale, bias)
    Ho = H // stride
    if out is None:
        out = torch.empty(B, Ho, Ho, Cc, dtype=dt, device=x.device)
    assert out.dtype == dt and out.numel() == B * Ho * Ho * Cc and out.is_contiguous()
    if impl == 1 and part is None:
        part = torch.empty(B, mv_dw3_groups(H, Cc, stride), Cc, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().btsbot_op_mv_dw3(_lib.PRECISION[precision], impl, _p(x), _p(w), _p(scale), _p(bias),
                                               _p(out), _p(part), B, H, Cc, stride, _stream(x)), "btsbot_op_mv_dw3")
    return out if impl == 0 else (out, part)


def mv_mbconv_front_tiles(H, stride):
    return _lib.check(_lib.lib().btsbot_op_mv_mbconv_front_tiles(H, stride), "btsbot_op_mv_mbconv_front_tiles")


def mv_mbconv_front(xn, conv1_w, b1, dw_w, dw_scale, b2, stride, precision="bf16", m2=None, part=None):
    """xn [B,H,H,CIN] -> m2 [B,H/s,H/s,MID] = silu(dw3x3_s(silu(xn . conv1_w^T + b1)) * dw_scale + b2) and the pool's
    per-tile partial sums part [B, tiles, MID] fp32: (m2, part)."""
    dt = _DT[precision]
    B, H, _, CIN = xn.shape
    MID = conv1_w.shape[0]
    assert xn.dtype == dt and xn.is_contiguous()
    _f32(conv1_w, b1, dw_w, dw_scale, b2)
    Ho = H // stride
    if m2 is None:
        m2 = torch.empty(B, Ho, Ho, MID, dtype=dt, device=xn.device)
    if part is None:
        part = torch.empty(B, mv_mbconv_front_tiles(H, stride), MID, dtype=torch.float32, device=xn.device)
    with torch.cuda.device(xn.device):
        _lib.check(_lib.lib().btsbot_op_mv_mbconv_front(_lib.PRECISION[precision], _p(xn), _p(conv1_w), _p(b1), _p(dw_w),
                                                        _p(dw_scale), _p(b2), _p(m2), _p(part), B, H, CIN, MID, stride,
                                                        _stream(xn)), "btsbot_op_mv_mbconv_front")
    return m2, part


def mv_se(y, fc1_w, fc1_b, fc2_w, fc2_b, inv_count, precision="f32", gate=None):
    """gate [B,C] fp32 = sigmoid(fc2(silu(fc1(inv_count * y.sum(1))))): y [B,HW,C] a 16-bit map, or ('f32') rows of
    partial sums.  fc1_w [RD,C], fc2_w [C,RD]."""
    B, HW, Cc = y.shape
    RD = fc1_w.shape[0]
    assert y.dtype == _DT[precision] and y.is_contiguous()
    _f32(fc1_w, fc1_b, fc2_w, fc2_b)
    assert fc1_w.numel() == RD * Cc and fc2_w.numel() == RD * Cc
    if gate is None:
        gate = torch.empty(B, Cc, dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        _lib.check(_lib.lib().btsbot_op_mv_se(_lib.PRECISION[precision], _p(y), _p(fc1_w), _p(fc1_b), _p(fc2_w), _p(fc2_b),
                                              _p(gate), B, HW, Cc, RD, float(inv_count), _stream(y)), "btsbot_op_mv_se")
    return gate


def mv_stem(img, conv1_w, bn_scale, bn_shift, conv2_w, precision="bf16", pooled=False, pre=None, out=None, xn=None):
    """img [B,3,63,63] fp32 -> the stem's fp32 output map [B,112,112,64] (pooled: its 2x2 average pool [B,56,56,64]);
    pre = (scale [64], shift [64]): also xn [B,112,112,64] = map * scale + shift in the precision's dtype: (out, xn)."""
    B = img.shape[0]
    assert img.dtype == torch.float32 and img.is_contiguous() and img.shape[1:] == (3, 63, 63)
    _f32(conv1_w, bn_scale, bn_shift, conv2_w)
    hw = 56 if pooled else 112
    if out is None:
        out = torch.empty(B, hw, hw, 64, dtype=torch.float32, device=img.device)
    assert out.dtype == torch.float32 and out.numel() == B * hw * hw * 64 and out.is_contiguous()
    ps = pb = None
    if pre is not None:
        ps, pb = pre
        _f32(ps, pb)
        if xn is None:
            xn = torch.empty(B, 112, 112, 64, dtype=_DT[precision], device=img.device)
    with torch.cuda.device(img.device):
        _lib.check(_lib.lib().btsbot_op_mv_stem(_lib.PRECISION[precision], _p(img), _p(conv1_w), _p(bn_scale), _p(bn_shift),
                                                _p(conv2_w), _p(out), int(pooled), _p(xn), _p(ps), _p(pb), B,
                                                _stream(img)), "btsbot_op_mv_stem")
    return out if pre is None else (out, xn)


# ---- the MaxViT TRAINING kernels one at a time (btsbot_op_mvt_*, maxvit_train_ops.hip): everything fp32; outputs given by
# the caller are used as they are ("+=" ones are added to), the others are allocated here
def _f32t(t, shape=None, numel=None):
    assert t.dtype == torch.float32 and t.is_contiguous(), "fp32 contiguous tensors"
    assert shape is None or tuple(t.shape) == tuple(shape), (tuple(t.shape), tuple(shape))
    assert numel is None or t.numel() == numel, (t.numel(), numel)
    return t


def _new(out, shape, like):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    n = 1
    for s in shape:
        n *= s
    return _f32t(out, numel=n)


def _mvt(name, t, *args):
    with torch.cuda.device(t.device):
        _lib.check(getattr(_lib.lib(), "btsbot_op_mvt_" + name)(*args, _stream(t)), "btsbot_op_mvt_" + name)


def mvt_bn_row_blocks(M):
    """gridDim.y of the BatchNorm reductions over M rows."""
    return _lib.check(_lib.lib().btsbot_op_mvt_bn_row_blocks(M), "btsbot_op_mvt_bn_row_blocks")


def mvt_dw3_bwd_w_row_blocks(npix):
    """gridDim.y of the depthwise filter gradient over npix output pixels."""
    return _lib.check(_lib.lib().btsbot_op_mvt_dw3_bwd_w_row_blocks(npix), "btsbot_op_mvt_dw3_bwd_w_row_blocks")


def mvt_attn_bwd_groups_per_head(units, heads):
    """Workgroups per head of the attention backward for `units` (alert, partition) pairs."""
    return _lib.check(_lib.lib().btsbot_op_mvt_attn_bwd_groups_per_head(units, heads),
                      "btsbot_op_mvt_attn_bwd_groups_per_head")


def mvt_bn_fwd(x, w, b, run_mean, run_var, act, y=None, stat=None):
    """BatchNorm2d on batch statistics of x [M,C]: -> (y = act(xhat w + b), stat [2C] = mean | rstd); run_mean /
    run_var [C] are updated in place (both None: left out).  act 0 none, 1 SiLU."""
    M, Cc = x.shape
    _f32t(x), _f32t(w, (Cc,)), _f32t(b, (Cc,))
    for r in (run_mean, run_var):
        assert r is None or _f32t(r, (Cc,)) is r
    y, stat = _new(y, (M, Cc), x), _new(stat, (2 * Cc,), x)
    _mvt("bn_fwd", x, _p(x), _p(w), _p(b), _p(run_mean), _p(run_var), _p(y), _p(stat), M, Cc, act)
    return y, stat


def mvt_bn_bwd(x, dy, stat, w, b, act, accumulate, dx, dw, db):
    """Backward of mvt_bn_fwd: dx [M,C] written (accumulate 0) or added to (1) -- it may be dy itself; dw, db [C] += ."""
    M, Cc = x.shape
    _f32t(x), _f32t(dy, numel=M * Cc), _f32t(stat, (2 * Cc,)), _f32t(w, (Cc,)), _f32t(b, (Cc,))
    _f32t(dx, numel=M * Cc), _f32t(dw, (Cc,)), _f32t(db, (Cc,))
    _mvt("bn_bwd", x, _p(x), _p(dy), _p(stat), _p(w), _p(b), _p(dx), _p(dw), _p(db), M, Cc, act, int(accumulate))
    return dx


def mvt_dw3_fwd(x, w, bias, stride, out=None):
    """x [B,H,H,C] -> dw3x3_s(x, w [C,1,3,3]) + bias [B,H/s,H/s,C]."""
    B, H, _, Cc = x.shape
    _f32t(x), _f32t(w, (Cc, 1, 3, 3)), _f32t(bias, (Cc,))
    Ho = H // max(stride, 1)
    out = _new(out, (B, Ho, Ho, Cc), x)
    _mvt("dw3_fwd", x, _p(x), _p(w), _p(bias), _p(out), B, H, Cc, stride)
    return out


def mvt_dw3_bwd_in(dout, w, H, stride, din=None):
    """dout [B,H/s,H/s,C] -> the gradient of mvt_dw3_fwd's input [B,H,H,C]."""
    B, Cc = dout.shape[0], dout.shape[3]
    _f32t(dout), _f32t(w, (Cc, 1, 3, 3))
    din = _new(din, (B, H, H, Cc), dout)
    _mvt("dw3_bwd_in", dout, _p(dout), _p(w), _p(din), B, H, Cc, stride)
    return din


def mvt_dw3_bwd_w(x, dout, stride, dw, dbias):
    """dw [C,1,3,3] += the filter gradient, dbias [C] += the bias gradient of mvt_dw3_fwd."""
    B, H, _, Cc = x.shape
    _f32t(x), _f32t(dout), _f32t(dw, numel=9 * Cc), _f32t(dbias, (Cc,))
    _mvt("dw3_bwd_w", x, _p(x), _p(dout), _p(dw), _p(dbias), B, H, Cc, stride)
    return dw, dbias


def mvt_attn_bwd(qkv, table, dout, B, H, grid_mode, dtable, dqkv=None):
    """Backward of mv_attn in fp32: qkv [B*H*H, 3C], table [169, C/32], dout [B*H*H, C] -> dqkv (written); dtable += ."""
    N = B * H * H
    Cc = qkv.shape[1] // 3
    _f32t(qkv, (N, 3 * Cc)), _f32t(table, (169, Cc // 32)), _f32t(dout, (N, Cc)), _f32t(dtable, numel=169 * (Cc // 32))
    dqkv = _new(dqkv, (N, 3 * Cc), qkv)
    _mvt("attn_bwd", qkv, _p(qkv), _p(table), _p(dout), _p(dqkv), _p(dtable), B, H, Cc, grid_mode)
    return dqkv


def mvt_se_fwd(a2, fc1_w, fc1_b, fc2_w, fc2_b, out=None):
    """a2 [B,P,C], fc1_w [RD,C], fc2_w [C,RD] -> (pool [B,C], rpre [B,RD], r [B,RD], gate [B,C], gated [B,P,C]);
    out: the five tensors, given."""
    B, P, Cc = a2.shape
    RD = fc1_w.shape[0]
    _f32t(a2), _f32t(fc1_w, (RD, Cc)), _f32t(fc1_b, (RD,)), _f32t(fc2_w, (Cc, RD)), _f32t(fc2_b, (Cc,))
    shapes = ((B, Cc), (B, RD), (B, RD), (B, Cc), (B, P, Cc))
    out = [_new(o, s, a2) for o, s in zip(out or (None,) * 5, shapes)]
    _mvt("se_fwd", a2, _p(a2), _p(fc1_w), _p(fc1_b), _p(fc2_w), _p(fc2_b), *(_p(o) for o in out), B, P, Cc, RD)
    return tuple(out)


def mvt_se_bwd(d_gated, a2, pool, rpre, r, gate, fc1_w, fc2_w, d_fc1_w, d_fc1_b, d_fc2_w, d_fc2_b, d_a2=None):
    """Backward of mvt_se_fwd from d_gated [B,P,C]: -> d_a2 (written); the four parameter gradients += ."""
    B, P, Cc = a2.shape
    RD = fc1_w.shape[0]
    _f32t(d_gated, numel=B * P * Cc), _f32t(a2), _f32t(pool, (B, Cc)), _f32t(rpre, (B, RD)), _f32t(r, (B, RD))
    _f32t(gate, (B, Cc)), _f32t(fc1_w, (RD, Cc)), _f32t(fc2_w, (Cc, RD))
    _f32t(d_fc1_w, numel=RD * Cc), _f32t(d_fc1_b, (RD,)), _f32t(d_fc2_w, numel=RD * Cc), _f32t(d_fc2_b, (Cc,))
    d_a2 = _new(d_a2, (B, P, Cc), a2)
    _mvt("se_bwd", a2, _p(d_gated), _p(a2), _p(pool), _p(rpre), _p(r), _p(gate), _p(fc1_w), _p(fc2_w), _p(d_a2),
         _p(d_fc1_w), _p(d_fc1_b), _p(d_fc2_w), _p(d_fc2_b), B, P, Cc, RD)
    return d_a2


def mvt_avgpool2_bwd(g, dx, accumulate):
    """dx [B,H,H,C] (+)= 0.25 g [B,H/2,H/2,C]."""
    B, H, _, Cc = dx.shape
    _f32t(g, (B, H // 2, H // 2, Cc)), _f32t(dx)
    _mvt("avgpool2_bwd", g, _p(g), _p(dx), B, H, Cc, int(accumulate))
    return dx


def mvt_col2im3(dcol, din=None):
    """dcol [B,H,H,9C] (tap-major) -> din [B,H,H,C]: the input gradient of a 3x3 s1 p1 im2col."""
    B, H, _, C9 = dcol.shape
    _f32t(dcol)
    assert C9 % 9 == 0
    din = _new(din, (B, H, H, C9 // 9), dcol)
    _mvt("col2im3", dcol, _p(dcol), _p(din), B, H, C9 // 9)
    return din


def mvt_unpack_conv3_grad(gp, g):
    """g [O,C,3,3] += gp [O,ldp], packed (ky*3+kx)*C + c."""
    O, Cc = g.shape[0], g.shape[1]
    _f32t(gp), _f32t(g, (O, Cc, 3, 3))
    assert gp.shape[0] == O
    _mvt("unpack_conv3_grad", gp, _p(gp), _p(g), O, Cc, gp.shape[1])
    return g


def mvt_gelu_fwd(pre, out=None):
    _f32t(pre)
    out = _new(out, tuple(pre.shape), pre)
    _mvt("gelu_fwd", pre, _p(pre), _p(out), pre.numel())
    return out


def mvt_gelu_bwd(pre, d):
    """d *= gelu'(pre), in place."""
    _f32t(pre), _f32t(d, numel=pre.numel())
    _mvt("gelu_bwd", pre, _p(pre), _p(d), pre.numel())
    return d


def mvt_bcast_set(v, P, scale, out=None):
    """v [B,C] -> [B,P,C] = v * scale."""
    B, Cc = v.shape
    _f32t(v)
    out = _new(out, (B, P, Cc), v)
    _mvt("bcast_set", v, _p(v), _p(out), B, P, Cc, float(scale))
    return out


# ---- the ConvNeXt training step's LayerNorm / depthwise backward kernels one at a time (btsbot_op_cnt_*,
# cn_bwd_ops.hip): everything fp32, NHWC rows; w = taps [49, C].  Every output is the caller's tensor: the "+=" ones
# are added to, the "=" ones written (include/btsbot_hip.h states which is which).  out16: None, or a bf16 / f16
# tensor that receives the rounded copy of the fp32 output.
def _cnt(name, t, *args):
    with torch.cuda.device(t.device):
        _lib.check(getattr(_lib.lib(), "btsbot_op_cnt_" + name)(*args, _stream(t)), "btsbot_op_cnt_" + name)


def _o16(out16, numel):
    if out16 is None:
        return _p(None), 0
    assert out16.dtype in (torch.bfloat16, torch.float16) and out16.is_contiguous() and out16.numel() == numel
    return _p(out16), _lib.PRECISION["bf16" if out16.dtype == torch.bfloat16 else "f16"]


def cnt_dwln_bwd_rows(HW, C, B):
    """Partial rows (= workgroups) of one dwln_bwd launch over B alerts."""
    return _lib.check(_lib.lib().btsbot_op_cnt_dwln_bwd_rows(HW, C, B), "btsbot_op_cnt_dwln_bwd_rows")


def cnt_dw3ln_bwd_rows(B):
    """Partial rows (= workgroups) of one dw3ln_bwd launch over B alerts."""
    return _lib.check(_lib.lib().btsbot_op_cnt_dw3ln_bwd_rows(B), "btsbot_op_cnt_dw3ln_bwd_rows")


def _cnt_fused(name, first, dxn, g, xin, w, dy, arena, out16):
    B, HW, _, Cc = xin.shape
    n = B * HW * HW * Cc
    planes = dxn.numel() // max(n, 1)
    _f32t(dxn, numel=planes * n), _f32t(g, (Cc,)), _f32t(xin), _f32t(w, (49, Cc)), _f32t(dy, numel=n)
    _f32t(arena, numel=52 * Cc)
    p16, prec16 = _o16(out16, n)
    _cnt(name, xin, _p(first), _p(dxn), _p(g), _p(xin), _p(w), _p(dy), p16, prec16, _p(arena), B, HW, Cc, planes, n)
    return dy


def cnt_dwln_bwd(d, dxn, g, xin, w, dy, arena, out16=None):
    """xin, d, dy [B,HW,HW,C]; dxn [planes,B,HW,HW,C] (or one plane); dy += ; arena [52 C] = [C,49] | [C] | [C] | [C] += ."""
    _f32t(d, numel=xin.numel())
    return _cnt_fused("dwln_bwd", d, dxn, g, xin, w, dy, arena, out16)


def cnt_dw3ln_bwd(dwb, dxn, g, xin, w, dy, arena, out16=None):
    """The 3x3 x 256 kernel: as cnt_dwln_bwd with dwb [C] = conv_dw.bias in place of d."""
    _f32t(dwb, (xin.shape[3],))
    return _cnt_fused("dw3ln_bwd", dwb, dxn, g, xin, w, dy, arena, out16)


def cnt_ln_bwd(d, dxn, g, dd, dg, dbeta, out16=None, patch_hw=0):
    """d [rows, C]; dxn [rows, C] (dd may be dxn) or, with patch_hw, the patch matrix [rows / 4-ish, 4 C]; dd = ;
    dg, dbeta [C] += ."""
    rows, Cc = d.shape
    _f32t(d), _f32t(dxn), _f32t(g, (Cc,)), _f32t(dd, numel=rows * Cc), _f32t(dg, (Cc,)), _f32t(dbeta, (Cc,))
    if patch_hw == 0:
        assert dxn.numel() == rows * Cc
    else:
        assert dxn.numel() == rows // (patch_hw * patch_hw) * (patch_hw // 2) ** 2 * 4 * Cc
    p16, prec16 = _o16(out16, rows * Cc)
    _cnt("ln_bwd", d, _p(d), _p(dxn), _p(g), _p(dd), _p(dg), _p(dbeta), rows, Cc, p16, prec16, patch_hw)
    return dd


def cnt_ln_dw1_bwd(d, dxn, g, xin, w, dy, dg, dbeta, dw, dbias, out16=None):
    """1x1 maps: d, dxn, xin, dy [rows, C]; dy += ; dg, dbeta, dbias [C] += ; dw [C, 49]: tap 24 += ."""
    rows, Cc = d.shape
    for t in (d, dxn, xin, dy):
        _f32t(t, numel=rows * Cc)
    _f32t(g, (Cc,)), _f32t(w, (49, Cc)), _f32t(dg, (Cc,)), _f32t(dbeta, (Cc,)), _f32t(dw, (Cc, 49)), _f32t(dbias, (Cc,))
    p16, prec16 = _o16(out16, rows * Cc)
    _cnt("ln_dw1_bwd", d, _p(d), _p(dxn), _p(g), _p(xin), _p(w), _p(dy), p16, prec16, _p(dg), _p(dbeta), _p(dw), _p(dbias),
         rows, Cc)
    return dy


def cnt_dw_plain(x, w, flip, bias, addend, out, out16=None):
    """x, out [B,HW,HW,C]; out = conv(x, taps, flipped when flip) + bias + addend (each may be None; addend may be out)."""
    B, HW, _, Cc = x.shape
    _f32t(x), _f32t(w, (49, Cc)), _f32t(out, numel=x.numel())
    assert bias is None or _f32t(bias, (Cc,)) is bias
    assert addend is None or _f32t(addend, numel=x.numel()) is addend
    p16, prec16 = _o16(out16, x.numel())
    _cnt("dw_plain", x, _p(x), _p(w), int(flip), _p(bias), _p(addend), _p(out), p16, prec16, B, HW, Cc)
    return out


def cnt_dw_wgrad(x, dd, dw, dbias):
    """x, dd [B,HW,HW,C]; dw [C,49] += , dbias [C] += (dbias directly behind dw in memory, or the call is refused)."""
    B, HW, _, Cc = x.shape
    _f32t(x), _f32t(dd, numel=x.numel()), _f32t(dw, numel=49 * Cc), _f32t(dbias, (Cc,))
    _cnt("dw_wgrad", x, _p(x), _p(dd), _p(dw), _p(dbias), B, HW, Cc)
    return dw, dbias


def cnt_colsum_f32(rows, out):
    """out [N] += the column sums of rows [M, N]."""
    M, N = rows.shape
    _f32t(rows), _f32t(out, (N,))
    _cnt("colsum_f32", rows, _p(rows), _p(out), M, N)
    return out


def cnt_stem_dgrad(dxn, w, out=None):
    """The patch stem's input gradient: dxn [B, 15, 15, C0] (or [B*225, C0]), w [C0, 3, 4, 4] -> [B, 3, 63, 63], every
    element written (rows / columns 60..62 as zeros).  C0 64 or 80."""
    C0 = w.shape[0]
    _f32t(w, (C0, 3, 4, 4)), _f32t(dxn)
    assert dxn.shape[-1] == C0 and dxn.numel() % (225 * C0) == 0, tuple(dxn.shape)
    B = dxn.numel() // (225 * C0)
    out = _new(out, (B, 3, 63, 63), dxn)
    _cnt("stem_dgrad", dxn, _p(dxn), _p(w), _p(out), B, C0)
    return out.view(B, 3, 63, 63)


# ---- the MLP half of the ConvNeXt 16-bit training step one launcher at a time (btsbot_op_cnt_*, cn_mlp_ops.hip).
# Operand tensors are bf16 or f16 (that picks the kernels), biases / gamma / gradients fp32.  Every output is the
# caller's tensor; include/btsbot_hip.h states which are added to and which written.
def _t16(t, shape):
    assert t.dtype in (torch.bfloat16, torch.float16) and t.is_contiguous() and tuple(t.shape) == tuple(shape), \
        (t.dtype, tuple(t.shape), tuple(shape))
    return _lib.PRECISION["bf16" if t.dtype == torch.bfloat16 else "f16"]


def cnt_mlp_bwd_planes(C):
    """Addend planes of cnt_mlp_bwd's dxn."""
    return _lib.check(_lib.lib().btsbot_op_cnt_mlp_bwd_planes(C), "btsbot_op_cnt_mlp_bwd_planes")


def cnt_mlp_bwd_slices(C, R):
    """Workgroups along the rows of one mlp_bwd launch: workgroup i walks the 64-row tiles i, i + slices, ..."""
    return _lib.check(_lib.lib().btsbot_op_cnt_mlp_bwd_slices(C, R), "btsbot_op_cnt_mlp_bwd_slices")


def cnt_s2mlp_bwd_rows():
    """Rows per workgroup of s2mlp_bwd."""
    return _lib.check(_lib.lib().btsbot_op_cnt_s2mlp_bwd_rows(), "btsbot_op_cnt_s2mlp_bwd_rows")


def cnt_mlp_bwd(xn, dy, w1, w2g, b1, dxn, G, S, dW1, db1, deterministic=False):
    """xn, dy [R, C]; w1 [4C, C]; w2g = (diag(gamma) W2)^T [4C, C]; dxn [planes, R, C] = ; G [C, 4C], S [C], dW1 [4C, C],
    db1 [4C] += ."""
    R, Cc = xn.shape
    prec = _t16(xn, (R, Cc))
    assert _t16(dy, (R, Cc)) == prec and _t16(w1, (4 * Cc, Cc)) == prec and _t16(w2g, (4 * Cc, Cc)) == prec
    planes = cnt_mlp_bwd_planes(Cc)
    _f32t(b1, (4 * Cc,)), _f32t(dxn, numel=planes * R * Cc), _f32t(G, (Cc, 4 * Cc)), _f32t(S, (Cc,))
    _f32t(dW1, (4 * Cc, Cc)), _f32t(db1, (4 * Cc,))
    _cnt("mlp_bwd", xn, prec, Cc, _p(xn), _p(dy), _p(w1), _p(w2g), _p(b1), _p(dxn), _p(G), _p(S), _p(dW1), _p(db1), R,
         int(bool(deterministic)))
    return dxn


def cnt_s2mlp_bwd(dy, a, w2gt, w1t, da, dxn):
    """dy [R, 256]; a [R, 1024]; w2gt = (diag(gamma) W2)^T [1024, 256]; w1t = W1^T [256, 1024]; da [R + 48, 1024] = (the
    operand type); dxn [R, 256] fp32 = ."""
    R = dy.shape[0]
    prec = _t16(dy, (R, 256))
    assert _t16(a, (R, 1024)) == prec and _t16(w2gt, (1024, 256)) == prec and _t16(w1t, (256, 1024)) == prec
    assert _t16(da, (R + 48, 1024)) == prec
    _f32t(dxn, (R, 256))
    _cnt("s2mlp_bwd", dy, prec, 256, _p(dy), _p(a), _p(w2gt), _p(w1t), _p(da), _p(dxn), R)
    return da, dxn


def cnt_fused_mlp(xn, w1, w2, b1, b2, gamma, x, xres=None):
    """xn [M, C] (bf16 / f16); w1 [4C, C], w2 [C, 4C] fp32 masters; x [M, C] = xres + gamma (W2 gelu(W1 xn + b1) + b2),
    xres None: x itself (in place)."""
    M, Cc = xn.shape
    prec = _t16(xn, (M, Cc))
    _f32t(w1, (4 * Cc, Cc)), _f32t(w2, (Cc, 4 * Cc)), _f32t(b1, (4 * Cc,)), _f32t(b2, (Cc,)), _f32t(gamma, (Cc,))
    _f32t(x, (M, Cc))
    assert xres is None or _f32t(xres, (M, Cc)) is xres
    _cnt("fused_mlp", xn, prec, Cc, _p(xn), _p(w1), _p(w2), _p(b1), _p(b2), _p(gamma), _p(xres), _p(x), M)
    return x


def cnt_fc2_grads(G, S, w2, b2, gamma, dW2, db2, dgamma):
    """G, w2, dW2 [C, H]; S, b2, gamma, db2, dgamma [C]; dW2, db2, dgamma = ; G and S are left zero."""
    Cc, H = G.shape
    _f32t(G), _f32t(S, (Cc,)), _f32t(w2, (Cc, H)), _f32t(b2, (Cc,)), _f32t(gamma, (Cc,)), _f32t(dW2, (Cc, H))
    _f32t(db2, (Cc,)), _f32t(dgamma, (Cc,))
    _cnt("fc2_grads", G, _p(G), _p(S), _p(w2), _p(b2), _p(gamma), _p(dW2), _p(db2), _p(dgamma), Cc, H)
    return dW2, db2, dgamma


# ---- the classifier heads on given rows (btsbot_op_head*, btsbot_op_ht_*, head_ops.hip).  Parameters are fp32 in
# state-dict layout.  Row tensors may be views with a row stride (ld) wider than their width; every output is the
# caller's tensor.
_ACT = {"none": 0, "gelu": 1, "relu": 2}


def _rows(t, width=None):
    """(M, width, ld) of an fp32 row tensor / view with unit column stride."""
    assert t.dtype == torch.float32 and t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), (t.dtype, t.shape, t.stride())
    assert width is None or t.shape[1] == width, (tuple(t.shape), width)
    return t.shape[0], t.shape[1], (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def _ht(name, t, *args):
    with torch.cuda.device(t.device):
        return _lib.check(getattr(_lib.lib(), "btsbot_op_ht_" + name)(*args, _stream(t)), "btsbot_op_ht_" + name)


def _head_dims(dims):
    return (C.c_int * len(dims))(*[int(d) for d in dims])


def head16_supported(precision, feat_dim, n_meta, f1, f2, dims):
    """head16.hip's own predicate for these widths (dims: the fusion MLP's widths, input first)."""
    return bool(_lib.lib().btsbot_op_head16_supported(_lib.PRECISION[precision], feat_dim, n_meta, f1, f2, len(dims) - 1,
                                                      _head_dims(dims)))


def head(precision, logits, feat=None, hn=None, meta=None, bn=None, m1=None, m2=None, meta_trailing_act=False, comb=(),
         act="gelu", scores=None, features=None, hidden=None):
    """The whole inference head: precision 'f32' (head.hip) or 'bf16' / 'f16' (head16.hip; widths it has no kernel for
    raise, nothing is written).  feat [B, F]; hn = (weight, bias) of the head LayerNorm; meta [B, n_meta] with bn =
    (weight, bias, running_mean, running_var), m1 = (weight [f1, n_meta], bias), m2 = (weight [f2, f1], bias); comb =
    ((weight, bias), ...) the fusion Linears, the last one [1, .].  logits [B] = ; scores [B], features [B * (F + f2)],
    hidden [B * comb[-1].in] = where given."""
    B = logits.numel()
    F = feat.shape[1] if feat is not None else 0
    n_meta = meta.shape[1] if meta is not None else 0
    f1 = m1[0].shape[0] if meta is not None else 0
    f2 = m2[0].shape[0] if meta is not None else 0
    for t in (feat, meta) + tuple(hn or ()) + tuple(bn or ()) + tuple(m1 or ()) + tuple(m2 or ()) + tuple(x for l in comb for x in l):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    if feat is not None:
        assert feat.shape[0] == B
    if meta is not None:
        assert meta.shape[0] == B and m1[0].shape == (f1, n_meta) and m2[0].shape == (f2, f1) and all(t.shape == (n_meta,) for t in bn)
    dims = [comb[0][0].shape[1]] + [w.shape[0] for w, _ in comb]
    for i, (w, b) in enumerate(comb):
        assert w.shape == (dims[i + 1], dims[i]) and b.shape == (dims[i + 1],)
    for t, n in ((logits, B), (scores, B), (features, B * dims[0]), (hidden, B * dims[-2])):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n), n
    vp = C.c_void_p
    cw = (vp * 3)(*[w.data_ptr() for w, _ in comb])
    cb = (vp * 3)(*[b.data_ptr() for _, b in comb])
    hn = hn or (None, None)
    bn = bn or (None,) * 4
    m1 = m1 or (None, None)
    m2 = m2 or (None, None)
    with torch.cuda.device(logits.device):
        _lib.check(_lib.lib().btsbot_op_head(
            _lib.PRECISION[precision], _p(feat), F, _p(hn[0]), _p(hn[1]), _p(meta), n_meta, _p(bn[0]), _p(bn[1]), _p(bn[2]),
            _p(bn[3]), _p(m1[0]), _p(m1[1]), f1, _p(m2[0]), _p(m2[1]), f2, int(bool(meta_trailing_act)), len(comb),
            _head_dims(dims), cw, cb, _ACT[act], _p(logits), _p(scores), _p(features), _p(hidden), B, _stream(logits)),
            "btsbot_op_head")
    return logits


def ht_lin_is_wide(M, N, K, ldi):
    """Whether a training fusion layer of this shape goes through the MFMA GEMM (head_train.hip's own decision)."""
    return bool(_lib.check(_lib.lib().btsbot_op_ht_lin_is_wide(M, N, K, ldi), "btsbot_op_ht_lin_is_wide"))


def ht_lin_fwd(x, w, bias, outa, pre=None, act="none", mask=None, keep_scale=1.0):
    """x [M, K] (ld), w [N, K], bias [N]; pre [M, N] = bias + x w^T where given; outa [M, N] (ld) = dropout(act(pre))."""
    M, K, ldi = _rows(x)
    N = w.shape[0]
    _f32t(w, (N, K)), _f32t(bias, (N,))
    _, _, ldo = _rows(outa, N)
    assert outa.shape[0] == M and (pre is None or _f32t(pre, (M, N)) is pre)
    assert mask is None or (mask.dtype == torch.uint8 and mask.is_contiguous() and tuple(mask.shape) == (M, N))
    _ht("lin_fwd", x, _p(x), ldi, _p(w), _p(bias), _p(pre), _p(outa), ldo, M, N, K, _ACT[act], _p(mask), float(keep_scale))
    return outa


def ht_act_bwd(dout, pre, dpre, act="none", mask=None, keep_scale=1.0):
    """dpre [M, N] = dout [M, N] (ld) * act'(pre [M, N]) * mask * keep_scale; dpre may share dout's memory."""
    M, N, ldd = _rows(dout)
    _f32t(pre, (M, N)), _f32t(dpre, (M, N))
    assert mask is None or (mask.dtype == torch.uint8 and mask.is_contiguous() and tuple(mask.shape) == (M, N))
    _ht("act_bwd", pre, _p(dout), ldd, _p(pre), _p(dpre), M, N, _ACT[act], _p(mask), float(keep_scale))
    return dpre


def ht_lin_bwd_in(dpre, w, din):
    """din [M, K] (ld) = dpre [M, N] w [N, K]."""
    M, N = dpre.shape
    K = w.shape[1]
    _f32t(dpre), _f32t(w, (N, K))
    _, _, ldi = _rows(din, K)
    assert din.shape[0] == M
    _ht("lin_bwd_in", dpre, _p(dpre), _p(w), _p(din), ldi, M, N, K)
    return din


def ht_lin_bwd_w_kind(x, dw):
    """Which kernel ht_lin_bwd_w(., x, dw, .) takes: 0 lin_bwd_w4, 1 lin_bwd_w<4, 64>, 2 lin_bwd_w<16, 16>."""
    _, K, ldi = _rows(x)
    return _lib.check(_lib.lib().btsbot_op_ht_lin_bwd_w_kind(_p(x), ldi, _p(dw), dw.shape[0], K), "btsbot_op_ht_lin_bwd_w_kind")


def ht_lin_bwd_w(dpre, x, dw, db):
    """dw [N, K] = dpre [M, N]^T x [M, K] (ld); db [N] = colsum(dpre)."""
    M, N = dpre.shape
    _, K, ldi = _rows(x)
    assert x.shape[0] == M
    _f32t(dpre), _f32t(dw, (N, K)), _f32t(db, (N,))
    _ht("lin_bwd_w", dpre, _p(dpre), _p(x), ldi, _p(dw), _p(db), M, N, K)
    return dw, db


def ht_bn_fwd(x, w, b, xhat, out, rstd, run_mean=None, run_var=None):
    """BatchNorm1d on batch statistics: x, xhat, out [M, n]; w, b, rstd, run_mean, run_var [n]."""
    M, n = x.shape
    _f32t(x), _f32t(w, (n,)), _f32t(b, (n,)), _f32t(xhat, (M, n)), _f32t(out, (M, n)), _f32t(rstd, (n,))
    for t in (run_mean, run_var):
        assert t is None or _f32t(t, (n,)) is t
    _ht("bn_fwd", x, _p(x), M, n, _p(w), _p(b), _p(run_mean), _p(run_var), _p(xhat), _p(out), _p(rstd))
    return xhat, out, rstd


def ht_bn_bwd(dy, w, xhat, rstd, dw, db):
    """dw [n] = sum dy xhat; db [n] = sum dy."""
    M, n = dy.shape
    _f32t(dy), _f32t(w, (n,)), _f32t(xhat, (M, n)), _f32t(rstd, (n,)), _f32t(dw, (n,)), _f32t(db, (n,))
    _ht("bn_bwd", dy, _p(dy), M, n, _p(w), _p(xhat), _p(rstd), _p(dw), _p(db))
    return dw, db


def ht_bn_eval_fwd(x, w, b, run_mean, run_var, xhat, out, rstd):
    """BatchNorm1d on running statistics: x, xhat, out [M, n]; w, b, run_mean, run_var, rstd [n]."""
    M, n = x.shape
    _f32t(x), _f32t(xhat, (M, n)), _f32t(out, (M, n))
    for t in (w, b, run_mean, run_var, rstd):
        _f32t(t, (n,))
    _ht("bn_eval_fwd", x, _p(x), M, n, _p(w), _p(b), _p(run_mean), _p(run_var), _p(xhat), _p(out), _p(rstd))
    return xhat, out, rstd


def ht_bn_bwd_in(dy, w, xhat, rstd, dx, sum_dy=None, sum_dyx=None, eval=False):
    """The BatchNorm's input gradient dx [M, n].  eval: dy * w * rstd; otherwise the batch-statistics form on the two
    column sums ht_bn_bwd leaves (its db and dw)."""
    M, n = dy.shape
    _f32t(dy), _f32t(w, (n,)), _f32t(xhat, (M, n)), _f32t(rstd, (n,)), _f32t(dx, (M, n))
    for t in (sum_dy, sum_dyx):
        assert t is None or _f32t(t, (n,)) is t
    _ht("bn_bwd_in", dy, _p(dy), M, n, _p(w), _p(xhat), _p(rstd), _p(sum_dy), _p(sum_dyx), _p(dx), int(bool(eval)))
    return dx


def ht_feat_rows(feat, z, hn=None):
    """z [M, F] (ld) = feat [M, F], through LayerNorm(eps 1e-6) with hn = (weight, bias) where given."""
    M, F = feat.shape
    _f32t(feat)
    _, _, ldz = _rows(z, F)
    assert z.shape[0] == M
    hn = hn or (None, None)
    _ht("feat_rows", feat, _p(feat), F, _p(hn[0]), _p(hn[1]), _p(z), ldz, M)
    return z


def ht_logits(x, logits, scores=None):
    """logits [M] = x [M]; scores [M] = sigmoid(x) where given."""
    M = x.numel()
    _f32t(x), _f32t(logits, numel=M)
    assert scores is None or _f32t(scores, numel=M) is scores
    _ht("logits", x, _p(x), _p(logits), _p(scores), M)
    return logits


def ht_copy_cols(dst, src):
    """dst [M, cols] (ld) = src [M, cols] (ld)."""
    M, cols, lds = _rows(src)
    _, _, ldd = _rows(dst, cols)
    assert dst.shape[0] == M
    _ht("copy_cols", src, _p(dst), ldd, _p(src), lds, cols, M)
    return dst


# ---- ConvNeXt stage 3 alone (btsbot_op_cn_*, infer_ops.hip / stage3.hip).  Argument checks are the library's: these
# wrappers pass what they are given (None as a null pointer), so the refusals can be asked for.
S3_PARAMS = ("dw_w", "dw_b", "ln_w", "ln_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "gamma")
_S3_ESZ = {"bf16": 2, "f16": 2, "fp8": 1, "f16x2": 4}


def cn_stage3_supported(precision, c3, depth):
    """stage3.hip's own predicate."""
    return bool(_lib.lib().btsbot_op_cn_stage3_supported(_lib.PRECISION[precision], c3, depth))


def cn_stage3_hfrag_bytes(precision, c3, B):
    """Bytes of the hidden-activation scratch a stage-3 call of B rows uses."""
    return _lib.check(_lib.lib().btsbot_op_cn_stage3_hfrag_bytes(_lib.PRECISION[precision], c3, B),
                      "btsbot_op_cn_stage3_hfrag_bytes")


def cn_stage3(precision, x, blocks, wide=False, B=None, c3=None):
    """`len(blocks)` ConvNeXt blocks on 1x1 maps, in place on x [B, c3] (fp32).  blocks: one dict per block with the fp32
    tensors of S3_PARAMS in state-dict layout (dw_w [C, 1, 7, 7], fc1_w [4C, C], fc2_w [C, 4C]).  B / c3 default to x's
    shape (a flat view of a larger buffer passes them)."""
    if B is None:
        B, c3 = x.shape
    lists = [(C.c_void_p * max(len(blocks), 1))(*[(b[k].data_ptr() if b[k] is not None else 0) for b in blocks])
             for k in S3_PARAMS]
    on = x if x is not None else next(t for b in blocks for t in b.values() if t is not None)
    with torch.cuda.device(on.device):
        _lib.check(_lib.lib().btsbot_op_cn_stage3(_lib.PRECISION[precision], c3, len(blocks), int(wide), _p(x), B, *lists,
                                                  _stream(on)), "btsbot_op_cn_stage3")
    return x


def cn_pack_s3(precision, src, rowscale=None, swap23=False, dst=None, scale=None):
    """stage 3's fragment packer: src [rows, K] fp32 (x rowscale [rows]) -> dst, a uint8 tensor of rows * K operand values
    (made when None); fp8: scale [2] fp32 receives {S, 1/S} (made when None).  Returns (dst, scale)."""
    rows, K = src.shape
    if dst is None:
        dst = torch.empty(rows * K * _S3_ESZ[precision], dtype=torch.uint8, device=src.device)
    if scale is None and precision == "fp8":
        scale = torch.empty(2, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().btsbot_op_cn_pack_s3(_lib.PRECISION[precision], _p(src), _p(rowscale), rows, K, int(swap23),
                                                   _p(dst), _p(scale), _stream(src)), "btsbot_op_cn_pack_s3")
    return dst, scale


def cn_fp8_scale(src, rowscale=None, K=1, scale=None):
    """scale [2] = {S, 1/S}: S the power of two that puts max |src[i] * rowscale[i // K]| into (120, 240]."""
    if scale is None:
        scale = torch.empty(2, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().btsbot_op_cn_fp8_scale(_p(src), _p(rowscale), src.numel(), K, _p(scale), _stream(src)),
                   "btsbot_op_cn_fp8_scale")
    return scale


# ---- ConvNeXt stage 2 alone (btsbot_op_cn_stage2*, infer_ops.hip / stage2p.hip).  As above: the checks are the library's.
S2_DOWN = ("ds_ln_w", "ds_ln_b", "ds_w", "ds_b")
S2_KEEP = ("xin", "xn", "a", "hh")


def cn_stage2_supported(precision, cw, depth):
    """stage2p.hip's own predicate (the stage's width cw, the next stage's being 2 cw)."""
    return bool(_lib.lib().btsbot_op_cn_stage2_supported(_lib.PRECISION[precision], cw, depth))


def cn_stage2_alerts(B, hint=0):
    """Alerts resident per workgroup (4, 5 or 7) that a 256-channel call of B alerts with this hint runs with."""
    return _lib.check(_lib.lib().btsbot_op_cn_stage2_alerts(B, hint), "btsbot_op_cn_stage2_alerts")


def cn_stage2(precision, x_in, blocks, down, out, tap_stage=None, alerts_hint=0, keep=None, ds_patches=None, B=None, cw=None):
    """`len(blocks)` ConvNeXt blocks on 3x3 maps x_in [B, 9, cw] (fp32) and the downsample behind them: out [B, 2 cw],
    tap_stage [B, 9, cw] (optional) the stage output.  blocks: as cn_stage3; down: a dict of S2_DOWN (ds_w [2 cw, cw, 2, 2]).
    keep: None, or a dict of S2_KEEP, each a list of one tensor per block (a list or a tensor may be None: the refusals),
    with ds_patches: the keeping form, every buffer with room for B + 9 alerts.  B / cw default to x_in's shape."""
    if B is None:
        B, _, cw = x_in.shape
    lists = [(C.c_void_p * max(len(blocks), 1))(*[(b[k].data_ptr() if b[k] is not None else 0) for b in blocks])
             for k in S3_PARAMS]
    if keep is None:
        klists = [None] * 4
    else:
        klists = [None if keep[k] is None else
                  (C.c_void_p * max(len(keep[k]), 1))(*[(t.data_ptr() if t is not None else 0) for t in keep[k]]) for k in S2_KEEP]
    on = out if out is not None else x_in
    with torch.cuda.device(on.device):
        _lib.check(_lib.lib().btsbot_op_cn_stage2(_lib.PRECISION[precision], cw, len(blocks), alerts_hint, _p(x_in), B, *lists,
                                                  *[_p(down[k]) for k in S2_DOWN], _p(out), _p(tap_stage), *klists,
                                                  _p(ds_patches), _stream(on)), "btsbot_op_cn_stage2")
    return out


def cn_stage2_rows(precision, x, block, rows=None):
    """stage2p's row-tile form in place on x [rows, 256] (fp32): x += gamma (fc2 gelu(fc1 LN(x) + fc1_b) + fc2_b); block: a
    dict with ln_w, ln_b, fc1_w, fc1_b, fc2_w, fc2_b, gamma."""
    if rows is None:
        rows = x.shape[0]
    on = x if x is not None else block["ln_w"]
    with torch.cuda.device(on.device):
        _lib.check(_lib.lib().btsbot_op_cn_stage2_rows(_lib.PRECISION[precision], _p(x), rows,
                                                       *[_p(block[k]) for k in S3_PARAMS[2:]], _stream(on)),
                   "btsbot_op_cn_stage2_rows")
    return x


def cn_pack_s2p(precision, src, rowscale=None, reorder_down=False, cin=0, dst=None, scale=None, rows=None, K=None):
    """stage 2's fragment packer: src [rows, K] fp32 (x rowscale [rows]; reorder_down: a downsample filter [rows, cin, 2, 2],
    K = 4 cin) -> dst, a uint8 tensor of rows * K operand values (made when None); fp8: scale [2] fp32 receives {S, 1/S}
    (made when None).  Returns (dst, scale)."""
    if rows is None:
        rows = src.shape[0]
        K = src.numel() // rows
    if dst is None:
        dst = torch.empty(rows * K * _S3_ESZ[precision], dtype=torch.uint8, device=src.device)
    if scale is None and precision == "fp8":
        scale = torch.empty(2, dtype=torch.float32, device=src.device)
    with torch.cuda.device(dst.device):
        _lib.check(_lib.lib().btsbot_op_cn_pack_s2p(_lib.PRECISION[precision], _p(src), _p(rowscale), rows, K, int(reorder_down),
                                                    cin, _p(dst), _p(scale), _stream(dst)), "btsbot_op_cn_pack_s2p")
    return dst, scale
