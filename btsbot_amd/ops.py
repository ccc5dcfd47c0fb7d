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
