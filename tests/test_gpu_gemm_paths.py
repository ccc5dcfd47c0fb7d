"""Every GEMM tile path, every epilogue and the 16-bit training products against float64.

The operands are exact values of the operand type, so a float64 product of them is exact (a float64 sum of K
such products loses nothing that matters here).  What the kernel may differ by is then derived, per element:

    |out - ref| <= u_out |out| + sub + L * (K + c) 2^-24 (|X| @ |W|^T + |bias| ...) + f

  u_out  one rounding of the output (2^-11 f16, 2^-8 bf16, 0 fp32), sub = 2^-25 for f16's subnormals;
  K 2^-24 (|X| @ |W|^T)  the fp32 accumulation, (+ c: the epilogue's own fp32 roundings, each 2^-24);
  L      the activation's largest slope (a perturbed pre-activation moves the output by at most L times as much);
  f      the activation's own evaluation error in fp32.

The activations are the kernels' own: gelu_poly<3/5> (bf16 / f16) and its derivative are ported to float64 (gelu_ref.py),
fp32 keeps erf.  Each test prints its worst err / bound per epilogue.  Every output (and gelu_save's aux) is a slice
of a larger buffer whose head and tail hold a sentinel bit pattern; the sentinels must survive every call.
"""
import ctypes as C
import os

import pytest
import torch

from btsbot_amd import _lib, ops
# the float64 ports of the kernels' GELU and the formats' rounding units (tests/gelu_ref.py); the MaxViT op tests read
# them through this module, so every name that lived here stays importable from it
from gelu_ref import (EPS, GELU_DEG, GELU_Q, L_GELU, LN2, SUB, U, _dpoly, _gelu, _gelu_f, _gelu_grad,  # noqa: F401
                      _gelu_grad_f, _poly, gelu_erf, gelu_erf_grad, gelu_poly, gelu_poly_grad)

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
EPIS = ("gelu", "resid", "bias", "silu", "bias_t", "gelu_save", "dgelu", "plain")
T_OUT = ("gelu", "silu", "bias_t", "gelu_save", "dgelu")     # outputs of the operand type; the others are fp32
L_SILU = 1.1                          # max |silu'| = 1.0998
SILU_REL = 4e-6                       # silu_fast / silu_f: ~1e-6 relative claimed (device_math.h), held at 4x


# ---- Python mirror of the tile choice: launch_gemm (gemm.hip:316) -> launch_typed2 (gemm2.hip:320-341, behind
# gemm2_supported, gemm2.hip:393) or launch_typed (gemm.hip:231-241).  name -> (TM, TN)
GEMM2_PATHS = {"64x128s3": (64, 128), "128x128s1": (128, 128), "128x128s2": (128, 128), "64x64s1": (64, 64),
               "64x64s3": (64, 64)}
GEMM1_PATHS = {"128x128": (128, 128), "128x64": (128, 64), "64x64": (64, 64)}


def _cdiv(a, b):
    return (a + b - 1) // b


def gemm_path(prec, M, N, K, one_slot=True):
    if prec in ("bf16", "f16") and K % 64 == 0 and N % 64 == 0 and N >= 64 and M >= 1:   # gemm2_supported
        wg128 = _cdiv(M, 128) * _cdiv(N, 128)
        if N >= 128 and wg128 >= 512 and K >= 1024:
            return "64x128s3"
        if N >= 128 and wg128 >= 256:
            return "128x128s1" if K == 64 and one_slot else "128x128s2"
        return "64x64s1" if K == 64 and one_slot else "64x64s3"
    if N >= 128 and _cdiv(M, 128) * _cdiv(N, 128) >= 512:
        return "128x128"
    if _cdiv(M, 128) * _cdiv(N, 64) >= 512 or N < 64:
        return "128x64"
    return "64x64"


def _valid(prec, K):
    return K % (4 if prec == "f32" else 8) == 0


# (M, N, K) -- the paths each reaches are checked by test_shapes_reach_every_tile_path
SHAPES = [
    (16383, 512, 1024),   # gemm2 64x128s3, M = 256 TM - 1 | f32 128x128
    (8191, 512, 64),      # gemm2 128x128s1, M = 64 TM - 1 | f32 128x64
    (16257, 192, 64),     # gemm2 128x128s1, M = 127 TM + 1, N tail at TN = 128 (MaxViT qkv at C = 64) | f32 64x64
    (8191, 512, 256),     # gemm2 128x128s2 | f32 128x64
    (8321, 640, 128),     # gemm2 128x128s2 at nano's 4 x 160, M = 65 TM + 1
    (1, 64, 64),          # gemm2 64x64s1, M = 1 | f32 64x64
    (65, 128, 64),        # gemm2 64x64s1, M = TM + 1
    (63, 192, 128),       # gemm2 64x64s3, M = TM - 1, N tail
    (245, 128, 512),      # gemm2 64x64s3
    (32768, 256, 64),     # f32 128x128
    (32769, 256, 4),      # f32 128x128, K = 4, M = 256 TM + 1
    (300, 16, 64),        # gemm.hip 128x64 (N < 64)
    (21885, 320, 80),     # 16-bit gemm.hip 128x128: ragged K at nano's width 80 | f32 128x128
    (500, 32, 72),        # gemm.hip 128x64, ragged K
    (1, 32, 72),          # gemm.hip 128x64, M = 1
    (129, 16, 8),         # gemm.hip 128x64, K = 8, M = TM + 1
    (127, 4, 36),         # f32 gemm.hip 128x64, K = 36, N = 4, M = TM - 1
    (65, 64, 4),          # f32 gemm.hip 64x64, K = 4, M = TM + 1
    (63, 80, 72),         # gemm.hip 64x64, ragged K and N = 80, M = TM - 1
]
PRECS = ("f32", "bf16", "f16")


def _cases():
    one_slot = os.environ.get("BTSBOT_AMD_GEMM2_NO_1SLOT", "") not in ("1",)
    for prec in PRECS:
        for M, N, K in SHAPES:
            if _valid(prec, K):
                yield pytest.param(prec, (M, N, K), id=f"{prec}-{gemm_path(prec, M, N, K, one_slot)}-{M}x{N}x{K}")


def test_shapes_reach_every_tile_path():
    """CPU: the shape list above reaches every tile path of both GEMM kernels in every precision that has it."""
    seen = {(prec, gemm_path(prec, M, N, K)) for prec in PRECS for M, N, K in SHAPES if _valid(prec, K)}
    want = {(p, n) for p in ("bf16", "f16") for n in GEMM2_PATHS} | {(p, n) for p in PRECS for n in GEMM1_PATHS}
    assert want <= seen, sorted(want - seen)
    for prec, name in sorted(want):
        print(f"{prec:5s} {name:10s}", [s for s in SHAPES if _valid(prec, s[2]) and gemm_path(prec, *s) == name])
    # the mirror's documented examples
    assert gemm_path("f16", 16383, 512, 1024) == "64x128s3" and gemm_path("bf16", 8191, 512, 256) == "128x128s2"
    assert gemm_path("f16", 8191, 512, 64) == "128x128s1" and gemm_path("f16", 16257, 192, 64) == "128x128s1"
    assert gemm_path("f16", 8191, 512, 64, one_slot=False) == "128x128s2"
    assert gemm_path("f32", 32768, 256, 64) == "128x128" and gemm_path("f32", 300, 16, 64) == "128x64"
    assert gemm_path("bf16", 21885, 320, 80) == "128x128" and gemm_path("f16", 500, 32, 72) == "128x64"


def test_gelu_polynomials_fit_the_erf_gelu():
    """CPU: gelu_poly<3/5> and their derivatives against the exact erf GELU on a dense grid, held at about 2x the
    measured fit (values 5.81e-5 / 4.69e-7, derivatives 1.27e-3 / 1.37e-5), so that a coefficient edit shows."""
    x = torch.linspace(-12.0, 12.0, 1_200_001, dtype=torch.float64)
    for deg, tv, td in ((3, 1.2e-4, 2.6e-3), (5, 1.0e-6, 2.8e-5)):
        ev = (gelu_poly(x, deg) - gelu_erf(x)).abs().max().item()
        ed = (gelu_poly_grad(x, deg) - gelu_erf_grad(x)).abs().max().item()
        print(f"gelu_poly<{deg}>: value {ev:.3e}, derivative {ed:.3e}")
        assert ev <= tv and ed <= td, (deg, ev, ed)
        assert ev >= tv / 4 and ed >= td / 4, (deg, ev, ed)   # (a much better fit means other coefficients)
        g = gelu_poly_grad(x, deg).abs().max().item()
        assert g <= L_GELU, g


# ---- guarded buffers: [PAD sentinel | n elements | PAD sentinel]
PAD = 1024
SENTINEL = {2: (torch.int16, 0x7E5A), 4: (torch.int32, 0x7FC5A5A5)}


def _guarded(n, dtype, dev, fill=None):
    buf = torch.empty(n + 2 * PAD, dtype=dtype, device=dev)
    it, pat = SENTINEL[buf.element_size()]
    buf.view(it).fill_(pat)
    t = buf[PAD:PAD + n]
    if fill is not None:
        t.copy_(fill.reshape(-1))
    return buf, t


def _intact(buf, n):
    it, pat = SENTINEL[buf.element_size()]
    b = buf.view(it)
    return bool((b[:PAD] == pat).all()) and bool((b[PAD + n:] == pat).all())


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _op_gemm(prec, epi, x, w, bias, gamma, resid, out, M, N, K):
    """btsbot_op_gemm without ops.gemm's checks: ops.gemm refuses the 16-bit training epilogues on purpose
    (test_training_epilogues_refuse_what_they_cannot_run); here their aux is an operand-typed buffer passed as resid."""
    _lib.check(_lib.lib().btsbot_op_gemm(_lib.PRECISION[prec], ops._EPI[epi], _p(x), _p(w), _p(bias), _p(gamma),
                                         _p(resid), _p(out), M, N, K, ops._stream(x)), f"btsbot_op_gemm[{epi}]")


def _check(what, out, ref, bound, ratios):
    err = (out.double() - ref).abs()
    r = torch.where(err == 0, 0.0, err / bound)   # (an exact zero is within a zero bound)
    worst = r.max().item()
    ratios[what] = max(ratios.get(what, 0.0), worst)
    if not worst <= 1.0:
        i = int(r.argmax())
        raise AssertionError(f"{what}: err {err.flatten()[i].item():.4e} > bound {bound.flatten()[i].item():.4e} at "
                             f"flat index {i} (out {out.flatten()[i].item():.6e}, ref {ref.flatten()[i].item():.6e}); "
                             f"{int((r > 1).sum())} elements over")


@pytest.mark.gpu
@pytest.mark.parametrize("prec,shape", list(_cases()))
def test_gemm_tile_path_epilogues(cuda, prec, shape):
    """All eight epilogues of one tile path x precision against one float64 accumulator; resid also in place."""
    M, N, K = shape
    T = DT[prec]
    u, sub = U[prec], SUB[prec]
    g = torch.Generator(device=cuda).manual_seed(M * 7 + N * 3 + K)
    x = torch.randn(M, K, generator=g, device=cuda).to(T)
    w = (torch.randn(N, K, generator=g, device=cuda) / K ** 0.5).to(T)
    bias = 0.1 * torch.randn(N, generator=g, device=cuda)
    gamma = 1.0 + 0.1 * torch.randn(N, generator=g, device=cuda)
    resid = torch.randn(M, N, generator=g, device=cuda)
    pre = (1.5 * torch.randn(M, N, generator=g, device=cuda)).to(T)   # dgelu's saved pre-activation
    x64, w64 = x.double(), w.double()
    A = x64 @ w64.t()
    S = x64.abs() @ w64.abs().t()
    del x64, w64
    b64, g64, r64 = bias.double(), gamma.double(), resid.double()
    E = K * EPS * S                                  # the fp32 accumulation
    Epre = E + 2 * EPS * (S + b64.abs())             # ... + bias, rounded once in fp32
    P = A + b64                                      # exact pre-activation
    ratios, kept = {}, {}
    n = M * N
    for epi in EPIS:
        odt = T if epi in T_OUT else torch.float32
        obuf, out = _guarded(n, odt, cuda)
        abuf, aux = (None, None)
        if epi == "gelu_save":
            abuf, aux = _guarded(n, T, cuda)
        elif epi == "dgelu":
            abuf, aux = _guarded(n, T, cuda, fill=pre)
        rs = resid if epi == "resid" else aux
        _op_gemm(prec, epi, x, w, bias, gamma, rs, out, M, N, K)
        out = out.view(M, N)
        uo = u * out.double().abs() + sub
        if epi == "bias":
            _check(epi, out, P, Epre, ratios)
        elif epi == "plain":
            _check(epi, out, A, E + EPS * S, ratios)
            kept["plain"] = out
        elif epi == "bias_t":
            _check(epi, out, P, uo + Epre, ratios)
        elif epi == "resid":
            ref = r64 + g64 * P
            _check(epi, out, ref, g64.abs() * Epre + 3 * EPS * (r64.abs() + g64.abs() * (S + b64.abs())), ratios)
        elif epi == "gelu":
            _check(epi, out, _gelu(prec, P), uo + L_GELU * Epre + _gelu_f(prec, P), ratios)
        elif epi == "silu":
            ref = P * torch.sigmoid(P)
            _check(epi, out, ref, uo + L_SILU * Epre + SILU_REL * (ref.abs() + L_SILU * Epre), ratios)
            kept["silu"] = out
        elif epi == "gelu_save":
            a64 = aux.view(M, N).double()
            _check("gelu_save.aux", aux.view(M, N), P, u * a64.abs() + sub + Epre, ratios)
            # out = GELU of the ROUNDED pre-activation the backward will differentiate
            _check(epi, out, _gelu(prec, a64), uo + _gelu_f(prec, a64), ratios)
        elif epi == "dgelu":
            p64 = pre.double()
            gp = _gelu_grad(prec, p64)
            ref = A * gp
            _check(epi, out, ref, uo + gp.abs() * E + S * _gelu_grad_f(prec, p64) + 2 * EPS * ref.abs(), ratios)
            assert torch.equal(aux.view(M, N), pre), "dgelu wrote its pre-activation"
        assert _intact(obuf, n), f"{epi}: out's guard bytes changed"
        if abuf is not None:
            assert _intact(abuf, n), f"{epi}: aux's guard bytes changed"
        del abuf, out, aux
    # SiLU's own error, printed: against SiLU of the kernel's pre-activation, fp32 (plain + bias) as the epilogue forms it,
    # beyond the output's rounding (fp32: silu_f's whole error; 16-bit: what one rounding to T leaves of silu_fast's)
    p_k = (kept["plain"] + bias).double()
    ref_k = p_k * torch.sigmoid(p_k)
    rest = ((kept["silu"].double() - ref_k).abs() - u * kept["silu"].double().abs() - sub).clamp(min=0)
    silu_rel = (rest / ref_k.abs().clamp(min=1e-30)).max().item()
    del kept, p_k, ref_k, rest
    # resid in place (out is resid): gemm2's prefetching form reads the residual before the main loop
    buf, io = _guarded(n, torch.float32, cuda, fill=resid)
    _op_gemm(prec, "resid", x, w, bias, gamma, io, io, M, N, K)
    _check("resid.inplace", io.view(M, N), r64 + g64 * P,
           g64.abs() * Epre + 3 * EPS * (r64.abs() + g64.abs() * (S + b64.abs())), ratios)
    assert _intact(buf, n), "resid in place: guard bytes changed"
    print(f"[{prec} {gemm_path(prec, M, N, K)} {M}x{N}x{K}] err/bound " +
          " ".join(f"{k}={v:.3g}" for k, v in ratios.items()) + f"; SiLU relative error {silu_rel:.3g}")


# ---- 16-bit filter gradient: the (N, K) pairs of the pico / nano training step (test_gpu_split_train.py's WIDTHS):
# fc2 (C x 4C), fc1 (4C x C), downsample (C x 2C, not in front of stage 0); MaxViT's 4x-mid products at C = 64..512
# are the same pairs.  Plus the stem's 48-wide patches and a small ragged pair.  Tiles: 128x128, 128x64 (K <= 64),
# 64x128 (N <= 64), 64x64 (wgrad.hip:437-440).
WIDTHS = (64, 128, 256, 512, 80, 160, 320, 640)
WGRAD_NK = sorted({nk for c in WIDTHS for nk in ((c, 4 * c), (4 * c, c)) + (() if c in (64, 80) else ((c, 2 * c),))}
                  | {(64, 48), (80, 48), (24, 40)})
WGRAD_M = (1, 255, 256, 257, 50176)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("nk", WGRAD_NK, ids=[f"{n}x{k}" for n, k in WGRAD_NK])
def test_wgrad16_against_float64(cuda, prec, nk):
    """ops.wgrad in the 16-bit modes (the training step's slices + two-pass reduction): out and colsum accumulate
    onto non-zero starting values.  Bound: the fp32 sum of M exact products and of the starting value,
    (M + 2) 2^-24 (|D|^T |A| + |out0|) -- the slice reduction's few additions are inside the M."""
    N, K = nk
    T = DT[prec]
    worst = {}
    for M in WGRAD_M:
        g = torch.Generator(device=cuda).manual_seed(M + 7 * N + K)
        d = torch.randn(M, N, generator=g, device=cuda)
        a = torch.randn(M, K, generator=g, device=cuda)
        if M > 4096:
            # the worst-case bound (M 2^-24 relative) is above what a lost 256-row slice of signed operands would
            # show; same-sign operands make every slice count for >= 256 / M of each output
            d, a = d.abs(), a.abs()
        d, a = d.to(T), a.to(T)
        out0 = torch.randn(N, K, generator=g, device=cuda)
        cs0 = torch.randn(N, generator=g, device=cuda)
        obuf, out = _guarded(N * K, torch.float32, cuda, fill=out0)
        cbuf, cs = _guarded(N, torch.float32, cuda, fill=cs0)
        ops.wgrad(d, a, out=out.view(N, K), colsum=cs, precision=prec)
        d64, a64 = d.double(), a.double()
        ref = out0.double() + d64.t() @ a64
        bound = (M + 2) * EPS * (d64.abs().t() @ a64.abs() + out0.double().abs())
        _check(f"out M={M}", out.view(N, K), ref, bound, worst)
        _check(f"colsum M={M}", cs, cs0.double() + d64.sum(0), (M + 2) * EPS * (d64.abs().sum(0) + cs0.double().abs()),
               worst)
        assert _intact(obuf, N * K) and _intact(cbuf, N), f"M={M}: guard bytes changed"
        del d, a, d64, a64, ref, bound, obuf, cbuf
    print(f"[wgrad16 {prec} {N}x{K}] err/bound " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


# ---- fp32 filter gradient: one (N, K) per dispatch branch of wgrad_f32 (wgrad_f32.hip); `off`: d starts one float into
# a larger buffer, so the 16-byte alignment test sends a 64-multiple shape to the fallback kernel
WGRAD32_NK = [
    (128, 128, 0),    # 128x128 tile
    (128, 64, 0),     # 128x64 tile
    (64, 128, 0),     # 64x128 tile
    (64, 64, 0),      # 64x64 tile
    (192, 192, 0),    # 64x64, several tiles
    (64, 48, 0),      # fallback, the stem's K
    (80, 320, 0),     # fallback, nano's widths
    (64, 64, 1),      # fallback through the alignment test
]
# a sub-tile, both sides of the 16-row rounding, both sides of the 256-row minimum slice, several slices with a ragged last
WGRAD32_M = (1, 15, 17, 255, 257, 1100)


@pytest.mark.gpu
@pytest.mark.parametrize("nk", WGRAD32_NK, ids=[f"{n}x{k}" + ("-unaligned" if o else "") for n, k, o in WGRAD32_NK])
def test_wgrad_f32_against_float64(cuda, nk):
    """ops.wgrad on fp32 operands (the matrix-pipe kernel per tile shape, the 64x64 fallback kernel): out and colsum
    accumulate onto non-zero starting values; colsum given (summed in the kernel on the matrix-pipe path, by the column
    sum launch behind the fallback) and None.  Bound: the any-order fp32 sum of M products and of the starting value,
    (M + 2) 2^-24 (|out0| + |D|^T |A|) and (M + 2) 2^-24 (|cs0| + sum |D|) -- whatever order the slices' atomics land in."""
    N, K, off = nk
    worst = {}
    for M in WGRAD32_M:
        g = torch.Generator(device=cuda).manual_seed(M + 7 * N + K + off)
        dbuf = torch.randn(M * N + off, generator=g, device=cuda)
        d = dbuf[off:].view(M, N)
        a = torch.randn(M, K, generator=g, device=cuda)
        out0 = torch.randn(N, K, generator=g, device=cuda)
        cs0 = torch.randn(N, generator=g, device=cuda)
        d64, a64 = d.double(), a.double()
        ref = out0.double() + d64.t() @ a64
        bound = (M + 2) * EPS * (out0.double().abs() + d64.abs().t() @ a64.abs())
        for with_cs in (True, False):
            obuf, out = _guarded(N * K, torch.float32, cuda, fill=out0)
            cbuf, cs = _guarded(N, torch.float32, cuda, fill=cs0)
            ops.wgrad(d, a, out=out.view(N, K), colsum=cs if with_cs else None, precision="f32")
            tag = f"M={M}" + ("" if with_cs else " no-cs")
            _check(f"out {tag}", out.view(N, K), ref, bound, worst)
            if with_cs:
                _check(f"colsum {tag}", cs, cs0.double() + d64.sum(0), (M + 2) * EPS * (cs0.double().abs() + d64.abs().sum(0)),
                       worst)
            assert _intact(obuf, N * K) and _intact(cbuf, N), f"{tag}: guard bytes changed"
            del obuf, cbuf
        del dbuf, d, a, d64, a64, ref, bound
    print(f"[wgrad f32 {N}x{K}{' unaligned' if off else ''}] err/bound " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


@pytest.mark.gpu
def test_wgrad16_refuses_what_it_cannot_run(cuda):
    d = torch.zeros(16, 24, dtype=torch.float16, device=cuda)
    a = torch.zeros(16, 36, dtype=torch.float16, device=cuda)
    with pytest.raises(_lib.BtsbotHipError, match="multiples of 8"):
        ops.wgrad(d, a, precision="f16")                              # K = 36
    buf = torch.zeros(16 * 24 + 1, dtype=torch.float16, device=cuda)
    a = torch.zeros(16, 40, dtype=torch.float16, device=cuda)
    with pytest.raises(_lib.BtsbotHipError, match="aligned"):
        ops.wgrad(buf[1:].view(16, 24), a, precision="f16")           # D 2 bytes off


# ---- MaxViT's squeeze-excite gated GEMM (launch_gemm_gated: 128x64 tiles when ceil(M/128) ceil(N/64) >= 512, else
# 64x64, gemm.hip:268) with a ragged last alert
GATED = [
    (16690, 256, 1024, 49),   # 128x64 tiles: 340 alerts of 7x7 + 30 rows
    (67517, 64, 256, 225),    # 128x64 tiles: 300 alerts of 15x15 + 17 rows
    (32769, 128, 64, 1),      # 128x64 tiles, one row per gate
    (363, 64, 256, 49),       # 64x64 tiles
    (775, 128, 512, 225),     # 64x64 tiles
    (37, 64, 64, 1),          # 64x64 tiles
]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "bf16", "f16", "f16x2"])
@pytest.mark.parametrize("shape", GATED, ids=[f"{m}x{n}x{k}r{r}" for m, n, k, r in GATED])
def test_gemm_gated_against_float64(cuda, prec, shape):
    """out = resid + (X * gate[m / rows]) @ W^T, also in place.  The 16-bit kernels round X * gate to T before the
    MFMA (gemm.hip:93): the bound adds (u_T + 2^-24) (|X gate| @ |W|^T).  f16x2 splits X gate and W into f16 head and
    remainder (22 bits each, and 2^-25 absolute where a remainder is subnormal) and drops the remainder x remainder
    product: 3 2^-22 (|X gate| @ |W|^T) + 2^-25 (sum_k |X gate| + sum_k |W|) over 3K fp32 additions."""
    M, N, K, rpa = shape
    T = torch.float32 if prec == "f16x2" else DT[prec]
    g = torch.Generator(device=cuda).manual_seed(M + N + K + rpa)
    x = torch.randn(M, K, generator=g, device=cuda).to(T)
    w = (torch.randn(N, K, generator=g, device=cuda) / K ** 0.5).to(T)
    gate = torch.sigmoid(torch.randn(_cdiv(M, rpa), K, generator=g, device=cuda))
    resid = torch.randn(M, N, generator=g, device=cuda)
    xg = x.double() * gate.double().repeat_interleave(rpa, 0)[:M]
    w64 = w.double()
    ref = resid.double() + xg @ w64.t()
    Sg = xg.abs() @ w64.abs().t()
    base = 2 * EPS * (resid.double().abs() + Sg)
    if prec == "f16x2":
        bound = (3 * K + 1) * EPS * Sg + 3 * 2.0 ** -22 * Sg + 2.0 ** -25 * (
            xg.abs().sum(1, keepdim=True) + w64.abs().sum(1)[None, :]) + base
    else:
        u = U[prec]
        bound = ((K + 1) * EPS * (1 + u) + u) * Sg + SUB[prec] * w64.abs().sum(1)[None, :] + base
    del xg
    worst = {}
    n = M * N
    obuf, out = _guarded(n, torch.float32, cuda)
    ops.gemm_gated(x, gate, rpa, w, resid, precision=prec, out=out.view(M, N))
    _check("gated", out.view(M, N), ref, bound, worst)
    assert _intact(obuf, n), "gated: guard bytes changed"
    buf, io = _guarded(n, torch.float32, cuda, fill=resid)
    ops.gemm_gated(x, gate, rpa, w, io.view(M, N), precision=prec, out=io.view(M, N))
    _check("gated.inplace", io.view(M, N), ref, bound, worst)
    assert _intact(buf, n), "gated in place: guard bytes changed"
    print(f"[gated {prec} {M}x{N}x{K} rows {rpa}] err/bound " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


# ---- the batched residual GEMM with the next LayerNorm fused (launch_gemm2_batched_resid): 128x128 tiles for
# N = 128 with LN (and big problems without), else 64x64
RESID_LN = [
    (1, 3137, 64, 256, True),
    (3, 197, 64, 128, True),
    (1, 3137, 128, 512, True),
    (3, 197, 128, 256, True),
    (3, 11000, 128, 256, False),    # 128x128 tiles without the LayerNorm
    (1, 500, 64, 64, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("case", RESID_LN, ids=[f"b{b}-{m}x{n}x{k}{'-ln' if ln else ''}" for b, m, n, k, ln in RESID_LN])
def test_gemm_resid_ln_against_float64(cuda, prec, case):
    """out = resid + X @ W^T per problem (also in place), and ln_out against a float64 LayerNorm (eps 1e-6) of the
    kernel's own fp32 out rows: one rounding to T plus the fp32 statistics -- the mean and the two-pass variance are
    sums of N terms, rsqrtf 2 ulp."""
    B, M, N, K, ln = case
    T = DT[prec]
    g = torch.Generator(device=cuda).manual_seed(B * M + N + K)
    x = torch.randn(B, M, K, generator=g, device=cuda).to(T)
    w = (torch.randn(B, N, K, generator=g, device=cuda) / K ** 0.5).to(T)
    resid = torch.randn(B, M, N, generator=g, device=cuda)
    ln_w = 1.0 + 0.1 * torch.randn(N, generator=g, device=cuda) if ln else None
    ln_b = 0.1 * torch.randn(N, generator=g, device=cuda) if ln else None
    x64, w64 = x.double(), w.double()
    ref = resid.double() + x64 @ w64.transpose(1, 2)
    bound = K * EPS * (x64.abs() @ w64.abs().transpose(1, 2)) + 2 * EPS * (resid.double().abs() + ref.abs())
    del x64, w64
    worst = {}
    n = B * M * N
    for inplace in (False, True):
        buf, o = _guarded(n, torch.float32, cuda, fill=resid if inplace else None)
        o = o.view(B, M, N)
        r = ops.gemm_resid_ln(x, w, o if inplace else resid, ln_w, ln_b, precision=prec, out=o)
        tag = ".inplace" if inplace else ""
        _check("out" + tag, o, ref, bound, worst)
        assert _intact(buf, n), "out: guard bytes changed"
        if ln:
            y = r[1]
            f = o.double()
            mu = f.mean(-1, keepdim=True)
            dx = f - mu
            rstd = torch.rsqrt((dx * dx).mean(-1, keepdim=True) + 1e-6)
            yref = dx * rstd * ln_w.double() + ln_b.double()
            amax = f.abs().amax(-1, keepdim=True)
            # fp32 statistics: mean and deviations within (N + 2) EPS (|f| + max|f|); the variance (and so rstd)
            # within (N + 4) EPS relative, plus twice the deviations' error over the spread; three roundings after
            ed = (N + 2) * EPS * (f.abs() + amax)
            rel = (N + 4) * EPS + 2 * (N + 2) * EPS * 2 * amax * rstd + 2 * EPS
            yb = ln_w.double().abs() * rstd * (ed + dx.abs() * rel) + 3 * EPS * (yref.abs() + ln_b.double().abs())
            _check("ln_out" + tag, y, yref, U[prec] * y.double().abs() + SUB[prec] + yb, worst)
    print(f"[resid_ln {prec} b{B} {M}x{N}x{K}] err/bound " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


@pytest.mark.gpu
def test_process_wide_switches_in_a_child_process(cuda):
    """The switches read once per process -- BTSBOT_AMD_GEMM2_NO_PREFETCH (gemm2's RESID / DGELU epilogues load inside
    their store loop), BTSBOT_AMD_GEMM2_NO_1SLOT (K = 64 runs the 2- / 3-slot rings), BTSBOT_AMD_WGRAD_ATOMIC (the
    filter-gradient slices meet through atomics) and BTSBOT_AMD_WGRAD_F32_OLD (the fp32 filter gradient's 64x64
    fallback kernel for every shape) -- in ONE child running the gemm2 paths, the resid+LN form and the f16 and fp32
    filter gradients."""
    import subprocess
    import sys
    if os.environ.get("BTSBOT_AMD_TEST_CHILD") == "1":
        pytest.skip("already the child")
    env = dict(os.environ, BTSBOT_AMD_TEST_CHILD="1", BTSBOT_AMD_GEMM2_NO_PREFETCH="1",
               BTSBOT_AMD_GEMM2_NO_1SLOT="1", BTSBOT_AMD_WGRAD_ATOMIC="1", BTSBOT_AMD_WGRAD_F32_OLD="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pick = ("(tile_path_epilogues and (s1 or s2 or s3)) or resid_ln or "
            "(wgrad16_against and f16 and not bf16) or wgrad_f32_against")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", pick,
                        "tests/test_gpu_gemm_paths.py"], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout, r.stdout[-2000:]
