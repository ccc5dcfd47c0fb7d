"""Float64 reference, per-element bound, emulation, seeded faults and fragment layouts for the last ConvNeXt stage ALONE
(btsbot_op_cn_stage3 / cn_pack_s3 / cn_fp8_scale: btsbot_amd/csrc/infer_ops.hip over stage3.hip), in its four operand
modes: bf16, f16, fp8 (OCP e4m3 on the block-scaled MFMA) and f16x2 (f16 head + f16 remainder).

Reference (stage3_ref), per block and with no intermediate rounding:
    u = x dw_c + dw_b        (dw_c = the 7x7 depthwise filter's centre tap: all a 1x1 map sees)
    y = LayerNorm_C(u)       (biased variance, LN_EPS = fp32 1e-6)
    a = W1 y + b1;   g = gelu_poly(a, deg);   x += gamma b2 + (diag(gamma) W2) g
deg = 3 for bf16 and fp8 (GeluOf<fp8_t> is bf16), 5 for f16 and f16x2 (GeluDeg's primary template): gelu_ref.GELU_DEG.

The bound is derived per element from what the kernels legitimately do, nothing is fitted (EPS = 2^-24; U, SUB: the
operand format's rounding unit and subnormal floor, gelu_ref.py):
  ex          the error of the block's input x (0 for the first block); it enters through the same terms as below
  u           one fma (fc1_tile: `fmaf(v, wc, bc)`):                         e_u = |dw_c| ex + EPS |u|
  mean        a lane's 2 C/128 values, six wave_sum steps, the product with fp32 1/C (n = 2 C/128 + 8 roundings):
                                                                             e_m = mean(e_u) + n EPS mean|u|
  d = u - m   one rounding:                                                  e_d = e_u + e_m + EPS |d|
  var         the same chain over fma'd squares:          e_v = mean(2 |d| e_d + e_d^2) + n EPS mean((|d| + e_d)^2)
  rstd        rsqrtf(var + LN_EPS): the sum's rounding, v_rsq_f32's ulp, LN_EPS's own rounding (3 EPS) around the
              interval [(v + e_v)^-1/2, (max(v - e_v, 0) + LN_EPS)^-1/2] -- no first-order step: a nearly constant row
              has e_v ~ v
  y           d rstd (one rounding), one fma with ln_w, ln_b, then ONE rounding to the operand type (S3M::lds_st2):
              r(y) = U (|y| + e) + SUB
  filters     ONE rounding of each value to the operand type (pack_s3_kernel / _split_ / _fp8_), fc2's of fl32(gamma W2);
              fp8 rounds S w, S the power of two of scale_from_max_kernel, and the sum is multiplied by 1/S: both exact.
              The filter is an input, so this error is not bounded but computed (filter_err: round to nearest even, which
              test_pack_s3 holds the packers to bit for bit).
  products    |W| e_y + e_W (|y| + e_y), summed over k; f16x2 drops lo x lo (S3M<f16x2_t>::run):
              (2^-11 |w| + 2^-25)(2^-11 |y| + 2^-25) per product
  fc1 sums    fp32, C products onto b1 (+ the 1/S1 product): acc(C + 2, sum |W||y| + |b1|)
  gelu        gelu_ref._gelu_f (its fp32 evaluation) + L_GELU e_a, then ONE rounding of g to the operand type
              (S3M::pack8 / stg_half; fp8 clamps to +-448 first: stage3_ref asserts |y|, |g| <= 448 unless saturate=True)
  fc2 sums    fp32, 4C products as eight K slices of 4C / 8 that meet in seven additions (+ 1/S2):
              acc(4C / 8 + 8, sum |gamma W2||g|)
  epilogue    fma(gamma, b2, s) and the addition to x: 2 EPS (|gamma b2| + |z| + e_z) + EPS (|x'| + ex + e_z)

A worst-case bound over 512 .. 2560 products is wide (fp8: ~2^-4 of the sum of absolute products), so there are two kinds
of input.  DENSE cases (dense_blocks) are seeded Gaussian filters at the networks' scales with every gamma regime; they
show that the kernels stay inside the bound on ordinary data, at the LayerNorm's edges (rows_x: a nearly constant row, a
row with a large common offset, an ordinary row times 30).  SPOTLIGHT cases (spot_blocks) give every hidden unit one or two
fc1 non-zeros and every channel four fc2 non-zeros, each hidden unit in exactly one of them (a channel feeds 4 - 6 hidden
units: 4C rows over C columns cannot do with fewer), with magnitudes (1 + m/8) 2^-e that every operand type holds exactly;
an output then depends on a handful of products, its bound has a handful of terms in every mode, and a filter value or a
hidden unit in the wrong place shows.  The maps are affine with odd multipliers, so the hidden units of a channel land
in different K slices and at different k positions of their fragments (spot_maps; test_stage3_reference.py checks it).

FAULTS are applied to the float64 computation (stage3_ref(fault=...)); test_stage3_reference.py shows that each leaves the
bound in every mode it applies to.  emulate() is the kernels' arithmetic in fp32 / the operand types with torch.

Fragment layouts (stage3.hip's comments; frag_pos / pack_s3_host / unpack_s3): a 16-bit image is
[row tile of 32][k-step of 16][lane 64][8], lane l = tile row l & 31, k = 16 s + 8 (l >> 5) + j; with swap23 tile row r
carries source row (r with bits 2 and 3 exchanged).  f16x2: the same, 2 KiB per fragment: 512 heads then 512 remainders.
fp8: k-steps of 64, a lane holds 32 k, in memory [lane][j 0..15] then [lane][j 16..31]; plain order k = 64 s + 32 (l >> 5)
+ j, kperm (fc2) k = 64 s + 32 (j >> 4) + (j & 7) + 8 (l >> 5) + 16 ((j >> 3) & 1).
"""
import math

import torch

from gelu_ref import EPS, GELU_DEG, L_GELU, SUB, U, _gelu_f, gelu_poly

F32, F64 = torch.float32, torch.float64
PRECS = ("bf16", "f16", "fp8", "f16x2")
WIDTHS = (512, 640)
PARAMS = ("dw_w", "dw_b", "ln_w", "ln_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "gamma")
LN_EPS = float(torch.tensor(1e-6, dtype=F32))
FP8_MAX = 448.0
ESZ = {"bf16": 2, "f16": 2, "fp8": 1, "f16x2": 4}
ODT = {"bf16": torch.bfloat16, "f16": torch.float16, "fp8": torch.float8_e4m3fn}
B_LIST = (1, 31, 32, 33, 64, 65, 129)


def acc(n, S):
    return n * EPS * S


def rnd_err(prec, v, dv=0.0):
    """ONE rounding to the operand type of a value v known to dv (a zero known exactly stays zero)"""
    e = U[prec] * (v.abs() + dv) + SUB[prec]
    return torch.where((v == 0) & (torch.as_tensor(dv) == 0), torch.zeros_like(e), e)


def lolo(prec, A, Bm):
    """what the split mode's three products leave out: lo(a) lo(b), |lo| <= 2^-11 |v| + 2^-25; A [m][k], Bm [n][k]"""
    if prec != "f16x2":
        return 0.0
    return (2.0 ** -11 * A + 2.0 ** -25) @ (2.0 ** -11 * Bm + 2.0 ** -25).t()


def filter_err(prec, w, rowscale, S):
    """|what the packer stores / S - w rowscale|: the filter is an input, so its one rounding (and fl32(w rowscale)'s) is
    known exactly"""
    v = host_round(prec, w, rowscale, S)
    v = v[0].to(F64) + v[1].to(F64) if prec == "f16x2" else v.to(F64)
    exact = w.to(F64) * (rowscale.to(F64)[:, None] if rowscale is not None else 1.0)
    return (v / S - exact).abs()


def fp8_scale(m):
    """scale_from_max_kernel in float64: the power of two S with 120 < m S <= 240 (1 for m = 0).  Refuses an m that sits
    on a power of two's edge, where log2f's last bit would decide."""
    m = float(m)
    if m == 0.0:
        return 1.0
    lg = math.log2(240.0 / m)
    assert abs(lg - round(lg)) > 1e-4, f"max |w| = {m} puts 240 / m on a power of two"
    return 2.0 ** math.floor(lg)


def ratio(got, ref, bound):
    """worst |got - ref| / bound (an exact zero is within a zero bound); NaN when an element is NaN"""
    err = (got.to(F64).reshape(ref.shape) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    if bool(torch.isnan(r).any()):
        return float("nan")
    return r.max().item() if r.numel() else 0.0


def outside(r):
    return not r <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def rows_x(C, B, seed, P0):
    """fp32 rows: ordinary ones, and of every eight one that the first block's depthwise step (P0) makes nearly constant
    (u = 1 + noise whose variance is a tenth of LN_EPS), one with a large common offset and one ordinary row times 30"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g)
    for r in range(B):
        if r % 8 == 1:
            x[r] = (1.0 + 3e-4 * x[r] - P0["dw_b"]) / P0["dw_w"][:, 0, 3, 3]
        elif r % 8 == 2:
            x[r] = 100.0 + x[r]
        elif r % 8 == 3:
            x[r] = 30.0 * x[r]
    return x


GAMMAS = ("one", "tenth", "init", "zero")


def _gamma(kind, C, g):
    if kind == "one":
        return 1.0 + 0.1 * torch.randn(C, generator=g)
    if kind == "tenth":
        return 0.1 * (1.0 + 0.1 * torch.randn(C, generator=g))
    if kind == "init":
        return torch.full((C,), 1e-6)
    assert kind == "zero"
    return torch.zeros(C)


def dense_blocks(C, gammas, seed):
    """Gaussian filters at the networks' scales; every depthwise tap non-zero; one gamma regime per block"""
    g = torch.Generator().manual_seed(seed)
    H = 4 * C
    out = []
    for kind in gammas:
        dw = 0.2 * torch.randn(C, 1, 7, 7, generator=g)
        dw[:, 0, 3, 3] = 0.8 + 0.2 * torch.randn(C, generator=g)
        out.append(dict(dw_w=dw, dw_b=0.1 * torch.randn(C, generator=g), ln_w=1.0 + 0.1 * torch.randn(C, generator=g),
                        ln_b=0.1 * torch.randn(C, generator=g), fc1_w=torch.randn(H, C, generator=g) * C ** -0.5,
                        fc1_b=0.2 * torch.randn(H, generator=g), fc2_w=torch.randn(C, H, generator=g) * H ** -0.5,
                        fc2_b=0.2 * torch.randn(C, generator=g), gamma=_gamma(kind, C, g)))
    return out


def spot_maps(C, step=333):
    """-> (c1 [4C], c2 [4C] (-1: none), hid [C][4]): the channels hidden unit h reads, the hidden units channel c reads.
    3, 7 and 333 are odd and no multiple of 5: h -> 3 h + 1 and h -> 7 h + 5 pass through every channel four times, and
    n -> 333 n + 17 is a bijection of the 4C hidden units.  A channel's four are 333 apart: more than a K slice (256 / 320),
    three steps less than seven slices, and 13 mod 16 and mod 64 -- four slices, four k positions.  step: another odd
    multiplier prime to 4C in place of 333 (stage2_ref.py: chunks of 128 hidden units)"""
    H = 4 * C
    h = torch.arange(H)
    c1 = (3 * h + 1) % C
    c2 = (7 * h + 5) % C
    c2 = torch.where((h % 2 == 1) & (c2 != c1), c2, torch.full_like(c2, -1))
    hid = ((step * torch.arange(H) + 17) % H).view(C, 4)
    return c1, c2, hid


def _mag(i, span):
    """(1 + m/8) 2^-e, m = 0 .. 6: exact in e4m3 (3 mantissa bits), so in every operand type; m, e from the index
    (no 1.875: as the largest magnitude it would put 240 / max on a power of two, where log2f's last bit picks the scale)"""
    return (1.0 + (i % 7).to(F32) / 8.0) * 2.0 ** -((i // 7) % span).to(F32)


def spot_blocks(C, depth, seed, step=333):
    """sparse filters (see the module docstring); gamma a power of two other than 1, biases of the size of the products"""
    g = torch.Generator().manual_seed(seed)
    H = 4 * C
    c1, c2, hid = spot_maps(C, step)
    h = torch.arange(H)
    out = []
    for j in range(depth):
        dw = 0.2 * torch.randn(C, 1, 7, 7, generator=g)
        dw[:, 0, 3, 3] = 0.8 + 0.2 * torch.randn(C, generator=g)
        w1 = torch.zeros(H, C)
        sg = torch.where((h + j) % 3 == 0, -1.0, 1.0)
        w1[h, c1] = sg * _mag(h + j, 2)
        two = c2 >= 0
        w1[h[two], c2[two]] = -sg[two] * _mag(h[two] + 3 + j, 2)
        w2 = torch.zeros(C, H)
        n = torch.arange(H).view(C, 4)
        w2[torch.arange(C)[:, None].expand(C, 4), hid] = torch.where((n + j) % 5 < 2, -1.0, 1.0) * _mag(n + 5 + j, 2)
        c = torch.arange(C)
        gamma = torch.tensor([0.5, 0.25, 2.0])[(c + j) % 3]
        out.append(dict(dw_w=dw, dw_b=0.5 * torch.randn(C, generator=g), ln_w=1.0 + 0.1 * torch.randn(C, generator=g),
                        ln_b=0.1 * torch.randn(C, generator=g), fc1_w=w1,
                        fc1_b=torch.where(h % 2 == 0, 0.75, -0.5) * (1.0 + 0.25 * torch.rand(H, generator=g)), fc2_w=w2,
                        fc2_b=torch.where(c % 2 == 0, 1.5, -1.0) * (1.0 + 0.25 * torch.rand(C, generator=g)), gamma=gamma))
    return out


def saturating(C, seed, row=3):
    """-> (x [B = 9][C], x_plain, blocks, row): one spotlight block whose LayerNorm has weight 16 at the channel that a
    hidden unit reads with the weight +1.75, and one row that the depthwise step turns into a spike there: its normalised
    value is sqrt(C - 1), y = 16 sqrt(C - 1) ~ 362 (inside e4m3's range), and that unit's a ~ 634 > 448.  Every other
    row's |y| and |g| stay far inside.  x_plain is the same call with the row left ordinary."""
    blocks = spot_blocks(C, 1, seed)
    b0 = blocks[0]
    chan = int(b0["fc1_w"].max(0).values.argmax())
    assert float(b0["fc1_w"][:, chan].max()) == 1.75
    b0["ln_w"][chan] = 16.0
    b0["ln_b"][chan] = 0.0
    x_plain = rows_x(C, 9, seed + 1, b0)
    x = x_plain.clone()
    spike = torch.zeros(C)
    spike[chan] = 1.0
    x[row] = (spike - b0["dw_b"]) / b0["dw_w"][:, 0, 3, 3]
    return x, x_plain, blocks, row


# ---------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("no_dw_b", "wrong_tap", "no_ln_eps", "no_b1", "b2_unscaled", "no_residual", "no_swap23", "no_kperm", "swap_hidden",
          "planes_swapped", "no_inv_s1", "no_inv_s2", "last_row_from_0", "stale_half", "block1_twice")
FAULT_PRECS = {"no_kperm": ("fp8",), "no_inv_s1": ("fp8",), "no_inv_s2": ("fp8",), "planes_swapped": ("f16x2",)}


def swap23(r):
    return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1)


def kperm_unit(H):
    """kperm[p]: the hidden unit s3_fc1 leaves at position p of fc2's fp8 k order (p = 64 s + 32 h + j)"""
    p = torch.arange(H)
    s, h, j = p // 64, (p // 32) % 2, p % 32
    return 64 * s + 32 * (j >> 4) + (j & 7) + 8 * h + 16 * ((j >> 3) & 1)


def _block(x, ex, P, prec, fault, saturate, clamp_g, want_bound):
    f = lambda k: P[k].to(F64)   # noqa: E731
    B, C = x.shape
    H = 4 * C
    wc, dwb, lnw, lnb, W1, b1, W2, b2, gam = (f(k) for k in PARAMS)
    wc = wc[:, 0, 3, 4] if fault == "wrong_tap" else wc[:, 0, 3, 3]
    if fault == "no_dw_b":
        dwb = torch.zeros_like(dwb)
    eps = 0.0 if fault == "no_ln_eps" else LN_EPS
    u = x * wc + dwb
    mean = u.mean(1, keepdim=True)
    d = u - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = (var + eps) ** -0.5
    t = d * rstd
    y = t * lnw + lnb
    S1 = fp8_scale(W1.abs().max()) if prec == "fp8" else 1.0
    W1u = W1
    if fault == "no_swap23":        # hidden tile 1's filter rows packed in their own order: unit u gets row swap23(u)
        W1u = W1.clone()
        r = torch.arange(32)
        W1u[32 + r] = W1[32 + swap23(r)]
    a = y @ W1u.t() + (0.0 if fault == "no_b1" else b1)
    if fault == "planes_swapped":   # fc1's heads and remainders exchanged: hi(w) lo(y) is the product left out
        yl = y - y.to(F32).half().to(F64)
        a = a - yl @ W1.to(F32).half().to(F64).t()
    if fault == "no_inv_s1":
        a = a * S1
    g = gelu_poly(a, GELU_DEG[prec])
    if prec == "fp8":
        if fault is None:
            assert float(y.abs().max()) <= FP8_MAX, "|y| beyond e4m3's range"
            assert saturate or float(g.abs().max()) <= FP8_MAX, "|g| beyond e4m3's range outside the saturation case"
        if clamp_g:
            g = g.clamp(-FP8_MAX, FP8_MAX)
    gu = g
    if fault == "swap_hidden":      # units 4 and 5: the same k-step in every mode
        gu = g.clone()
        gu[:, 4], gu[:, 5] = g[:, 5], g[:, 4]
    if fault == "no_kperm":         # gamma W2 in plain k order against the hidden units in s3_fc1's order
        gu = g[:, kperm_unit(H)]
    if fault == "stale_half":       # the last 32-alert block's live rows read the half of hfrag no fc1 tile wrote (0xFF bytes)
        gu = g.clone()
        gu[32 * ((B - 1) // 32):] = float("nan")
    GW = gam[:, None] * W2
    gw32 = (P["gamma"].to(F32)[:, None] * P["fc2_w"].to(F32)).to(F64)   # what the packer rounds: fl32(w gamma)
    S2 = fp8_scale(gw32.abs().max()) if prec == "fp8" else 1.0
    z = gu @ GW.t()
    if fault == "no_inv_s2":
        z = z * S2
    upd = (b2 if fault == "b2_unscaled" else gam * b2) + z
    xn = upd if fault == "no_residual" else x + upd
    if fault == "last_row_from_0" and B > 1:
        xn = xn.clone()
        xn[B - 1] = xn[0]
    if not want_bound:
        return xn, None
    # ---- the bound (module docstring)
    n = 2 * (C // 128) + 8
    e_u = wc.abs() * ex + EPS * u.abs()
    e_m = e_u.mean(1, keepdim=True) + n * EPS * u.abs().mean(1, keepdim=True)
    e_d = e_u + e_m + EPS * d.abs()
    e_v = (2 * d.abs() * e_d + e_d * e_d).mean(1, keepdim=True) + n * EPS * ((d.abs() + e_d) ** 2).mean(1, keepdim=True)
    r_hi = ((var - e_v).clamp(min=0) + LN_EPS) ** -0.5
    r_lo = (var + e_v + LN_EPS) ** -0.5
    e_r = torch.maximum(r_hi - rstd, rstd - r_lo) + 3 * EPS * r_hi
    e_t = e_d * (rstd + e_r) + d.abs() * e_r + EPS * t.abs()
    e_y32 = e_t * lnw.abs() + EPS * y.abs()
    e_y = e_y32 + rnd_err(prec, y, e_y32)
    e_w1 = filter_err(prec, P["fc1_w"], None, S1)
    ay, aw1 = y.abs() + e_y, W1.abs() + e_w1
    e_a = e_y @ W1.abs().t() + ay @ e_w1.t() + lolo(prec, ay, aw1) + acc(C + 2, ay @ aw1.t() + b1.abs())
    e_gv = _gelu_f(prec, a) + L_GELU * e_a
    e_g = e_gv + rnd_err(prec, g, e_gv)
    e_gw = filter_err(prec, P["fc2_w"], P["gamma"], S2)
    ag, agw = g.abs() + e_g, GW.abs() + e_gw
    e_z = e_g @ GW.abs().t() + ag @ e_gw.t() + lolo(prec, ag, agw) + acc(H // 8 + 8, ag @ agw.t())
    e_x = ex + e_z + 2 * EPS * ((gam * b2).abs() + z.abs() + e_z) + EPS * (xn.abs() + ex + e_z)
    for k, v in dict(e_y=e_y, e_a=e_a, e_g=e_g, e_z=e_z, e_x=e_x, g=g).items():
        assert bool(torch.isfinite(v).all()), k
    return xn, e_x


def stage3_ref(x, blocks, prec, fault=None, saturate=False, clamp_g=False):
    """-> (x after the blocks, its per-element bound): float64 [B][C].  fault: one of FAULTS, applied to the float64
    computation (the bound is then None).  saturate: |g| may exceed e4m3's range; clamp_g: the fp8 reference clamps g to
    +-448 as the kernel does before its conversion."""
    assert fault is None or fault in FAULTS
    if fault == "block1_twice":
        assert len(blocks) >= 2
        blocks = [blocks[1], blocks[1]] + list(blocks[2:])
    x = x.to(F64)
    ex = torch.zeros_like(x)
    for P in blocks:
        x, ex = _block(x, ex, P, prec, fault, saturate, clamp_g, fault is None)
    return x, ex


# ---------------------------------------------------------------------------------------------------------------------
# emulation: the kernels' arithmetic in fp32 / the operand types
# ---------------------------------------------------------------------------------------------------------------------
def planes(prec, v):
    """fp32 v -> the operand's planes (fp32 values whose sum is the operand): one, or head and remainder"""
    if prec == "f16x2":
        hi = v.half().float()
        return [hi, (v - hi).half().float()]
    if prec == "fp8":
        return [v.clamp(-FP8_MAX, FP8_MAX).to(ODT[prec]).float()]
    return [v.to(ODT[prec]).float()]


def products(A, Bm):
    """A [m][k] x Bm [n][k]^T on planes, fp32 sums; the split mode's three products (no lo x lo)"""
    if len(A) == 1:
        return A[0] @ Bm[0].t()
    return A[1] @ Bm[0].t() + A[0] @ Bm[1].t() + A[0] @ Bm[0].t()


def emulate(x, blocks, prec):
    x = x.to(F32).clone()
    for P in blocks:
        wc, dwb, lnw, lnb, W1, b1, W2, b2, gam = (P[k].to(F32) for k in PARAMS)
        u = x * wc[:, 0, 3, 3] + dwb
        d = u - u.mean(1, keepdim=True)
        y = d * torch.rsqrt((d * d).mean(1, keepdim=True) + 1e-6) * lnw + lnb
        s1 = fp8_scale(W1.abs().max()) if prec == "fp8" else 1.0
        a = (products(planes(prec, y), planes(prec, W1 * s1)) + b1 * s1) * (1.0 / s1)
        g = gelu_poly(a.to(F64), GELU_DEG[prec]).to(F32)
        gw = W2 * gam[:, None]
        s2 = fp8_scale(gw.abs().max()) if prec == "fp8" else 1.0
        z = products(planes(prec, g), planes(prec, (W2 * s2) * gam[:, None] if prec == "fp8" else gw)) * (1.0 / s2)
        x = x + (gam * b2 + z)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# fragment layouts
# ---------------------------------------------------------------------------------------------------------------------
def host_round(prec, w, rowscale=None, scale=None):
    """what a packer stores for fp32 w [rows][K]: fl32(w rowscale) (fp8: fl32(fl32(w S) rowscale)) rounded once ->
    a tensor of the operand type, or (heads, remainders) in f16"""
    v = w.to(F32)
    if prec == "fp8":
        v = v * scale
    if rowscale is not None:
        v = v * rowscale.to(F32)[:, None]
    if prec == "f16x2":
        hi = v.half()
        return hi, (v - hi.float()).half()
    return v.to(ODT[prec])


def pack_s3_host(vals, prec, swap, kperm=False):
    """host packer, written along the kernels: element i of the image -> its (row, k).  vals: host_round's result.
    -> the image as a flat uint8 tensor"""
    hi = vals[0] if prec == "f16x2" else vals
    rows, K = hi.shape
    i = torch.arange(rows * K)
    if prec == "fp8":
        j, l, fs = i & 31, (i >> 5) & 63, i >> 11
        s, tile = fs % (K // 64), fs // (K // 64)
        h = l >> 5
        k = torch.where(torch.tensor(bool(kperm)), 64 * s + 32 * (j >> 4) + (j & 7) + 8 * h + 16 * ((j >> 3) & 1), 64 * s + 32 * h + j)
        at = fs * 2048 + (j >> 4) * 1024 + l * 16 + (j & 15)
    else:
        j, l, fs = i & 7, (i >> 3) & 63, i >> 9
        s, tile = fs % (K // 16), fs // (K // 16)
        k = 16 * s + 8 * (l >> 5) + j
        at = fs * 1024 + l * 8 + j if prec == "f16x2" else i
    r = l & 31
    if swap:
        r = swap23(r)
    row = 32 * tile + r
    if prec == "f16x2":
        img = torch.zeros(2 * rows * K, dtype=torch.float16)
        img[at] = vals[0][row, k]
        img[at + 512] = vals[1][row, k]
    else:
        img = torch.zeros(rows * K, dtype=vals.dtype)
        img[at] = vals[row, k]
    return img.view(torch.uint8)


def frag_pos(prec, rows, K, swap, kperm=False):
    """the inverse map: position [rows][K] of source element (row, k) in the image, counted in operand values (f16x2:
    of its head, in f16 values; the remainder lies 512 further)"""
    row, k = torch.arange(rows)[:, None], torch.arange(K)[None, :]
    tile, r = row // 32, row % 32
    if swap:
        r = swap23(r)          # (an involution: the tile row that carries source row r)
    if prec == "fp8":
        s, kk = k // 64, k % 64
        if kperm:
            m = kk % 32
            h, j = (m >> 3) & 1, (kk // 32) * 16 + (m >> 4) * 8 + (m & 7)
        else:
            h, j = kk // 32, kk % 32
        fs = tile * (K // 64) + s
        return fs * 2048 + (j >> 4) * 1024 + (32 * h + r) * 16 + (j & 15)
    s, h, j = k // 16, (k % 16) // 8, k % 8
    fs = tile * (K // 16) + s
    return (fs * 64 + 32 * h + r) * 8 + j + (fs * 512 if prec == "f16x2" else 0)


def unpack_s3(image, prec, rows, K, swap, kperm=False):
    """a packed image (flat uint8) -> the operand values in source order [rows][K]: a tensor of the operand type, or
    (heads, remainders)"""
    image = image.reshape(-1)
    assert image.dtype == torch.uint8 and image.numel() == rows * K * ESZ[prec]
    pos = frag_pos(prec, rows, K, swap, kperm)
    if prec == "f16x2":
        v = image.view(torch.float16)
        return v[pos], v[pos + 512]
    return image.view(ODT[prec])[pos]


def bits(t):
    """the bit patterns of an operand tensor (for bit-for-bit comparisons; NaN-safe, -0 != +0)"""
    return t.view(torch.uint8 if t.element_size() == 1 else torch.int16)
