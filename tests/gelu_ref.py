"""Float64 ports of device_math.h's GELU for the 16-bit modes (gelu_q<3/5>, gelu_poly, gelu_dq, gelu_poly_grad), the erf
form fp32 keeps, the fp32 evaluation error of each, and the rounding units of the number formats.  Shared by the
per-kernel float64 tests (test_gpu_gemm_paths.py, mlp_ref.py)."""
import math

import torch

EPS = 2.0 ** -24
# one rounding to the format: U relative, SUB the floor below its smallest normal.  "f16x2" = f16 head + f16 remainder (the
# remainder of a value is rounded once more: 2^-11 of 2^-11; its floor is f16's subnormal spacing / 2); "fp8" = OCP e4m3
# (3 mantissa bits; smallest subnormal 2^-9, so half a step is 2^-10; largest finite value 448)
U = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f16x2": 2.0 ** -22, "fp8": 2.0 ** -4}
SUB = {"f32": 0.0, "bf16": 0.0, "f16": 2.0 ** -25, "f16x2": 2.0 ** -25, "fp8": 2.0 ** -10}
L_GELU = 1.13                         # max |gelu'| = 1.1289 (both fits match it)

GELU_Q = {3: (-1.0036805164077327, -1.1287482669759885, -0.49926576060257244, -0.024772998623334343),
          5: (-1.000039487932206, -1.1507770495088248, -0.46001256950698816, -0.05181158088529847,
              0.007079169600613161, -0.0004726569791655389)}
# (GeluDeg's primary template is 5: the split mode takes it; GeluOf<fp8_t> is bf16)
GELU_DEG = {"bf16": 3, "f16": 5, "f16x2": 5, "fp8": 3}
LN2 = math.log(2.0)


def _poly(a, c):
    t = torch.full_like(a, c[-1])
    for ci in reversed(c[:-1]):
        t = t * a + ci
    return t


def _dpoly(a, c):
    return _poly(a, [i * c[i] for i in range(1, len(c))])


def gelu_poly(x, deg):
    a = x.abs()
    return x.clamp(min=0) - a * torch.exp2(_poly(a, GELU_Q[deg]))


def gelu_poly_grad(x, deg):
    a = x.abs()
    d = torch.exp2(_poly(a, GELU_Q[deg])) * (1.0 + a * LN2 * _dpoly(a, GELU_Q[deg]))
    return torch.where(x > 0, 1.0 - d, d)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_erf_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _gelu(prec, x):
    return gelu_erf(x) if prec == "f32" else gelu_poly(x, GELU_DEG[prec])


def _gelu_grad(prec, x):
    return gelu_erf_grad(x) if prec == "f32" else gelu_poly_grad(x, GELU_DEG[prec])


def _gelu_f(prec, x):
    """fp32 evaluation error of the kernel's GELU at x.  erf form: erff's 2 ulp and three roundings, each at most
    EPS |x|.  Polynomial form: Horner in fp32 moves q by <= 2 deg EPS sum|c_i| a^i, v_exp_f32 adds 1 ulp, the final
    fma one rounding -- <= 16 EPS (|x| + a 2^q (1 + sum|c_i| a^i))."""
    if prec == "f32":
        return 8 * EPS * (1.0 + x.abs())
    a = x.abs()
    c = GELU_Q[GELU_DEG[prec]]
    return 16 * EPS * (a + a * torch.exp2(_poly(a, c)) * (1.0 + _poly(a, [abs(v) for v in c])))


def _gelu_grad_f(prec, x):
    """... and of its derivative: erf form, cdf + x pdf with __expf (whose argument rounding costs EPS x^2 / 2
    relative: x pdf(x) x^2 / 2 < 1); polynomial form, 2^q (1 + a ln2 q'(a)) with the same Horner / v_exp terms."""
    if prec == "f32":
        return 16 * EPS * (1.0 + x.abs())
    a = x.abs()
    c = GELU_Q[GELU_DEG[prec]]
    ca = [abs(v) for v in c]
    return 16 * EPS * (1.0 + torch.exp2(_poly(a, c)) * (1.0 + _poly(a, ca)) * (1.0 + a * _dpoly(a, ca)))
