"""Float64 reference, per-element bound, emulation, seeded faults and fragment layouts for ConvNeXt stage 2 ALONE
(btsbot_op_cn_stage2 / cn_stage2_rows / cn_pack_s2p: btsbot_amd/csrc/infer_ops.hip over stage2p.hip) in every form the kernel
is launched in: 256 channels in bf16, f16, fp8 (OCP e4m3 on the block-scaled MFMA) and f16x2 (f16 head + f16 remainder),
320 channels in bf16 / f16, the keeping form of the training forward (bf16 / f16) and the row-tile form (the MLP half).
What stage 3 has in stage3_ref.py; the shared pieces (rnd_err, lolo, filter_err, fp8_scale, host_round, acc, ratio, the
spotlight maps and magnitudes) are imported from there and from gelu_ref.py.

Reference (stage2_ref), x [B][9][C] (3x3 maps, pixel p = 3 y + x), per block and with no intermediate rounding:
    u[o] = dw_b + sum_i dw_w[iy - oy + 3][ix - ox + 3] x[i]     (7x7 depthwise, zero padding 3: only the central 5x5 taps reach
                                                                 a 3x3 map)
    y = LayerNorm_C(u)                                          (biased variance, LN_EPS = fp32 1e-6)
    a = W1 y + b1;   g = gelu_poly(a, deg);   x += gamma b2 + (diag(gamma) W2) g
and behind the last block (x there is tap_stage): yd = LayerNorm_C(x) with the downsample's weights at pixels 0, 1, 3, 4,
    out[co] = ds_b[co] + sum_k Wd[co][k] patch[k],   k = (2 ky + kx) C + c  ->  yd[pixel 3 ky + kx][c], Wd[co][k] = ds_w[co][c][ky][kx].
deg = 3 for bf16 and fp8 (GeluOf2<fp8_t> is bf16), 5 for f16 and f16x2: gelu_ref.GELU_DEG.  rows_ref is the row-tile form:
the MLP half alone (u = x) on [rows][256].

The bound is derived per element from what the kernel legitimately does, nothing is fitted (EPS = 2^-24; U, SUB: the operand
format's rounding unit and subnormal floor, gelu_ref.py):
  ex          the error of the block's input x (0 for the first block); it enters through the same terms as below
  u           dbias and nine fmaf (stage2p_kernel's depthwise phase: the nine input pixels of the map in one chain):
                                                               e_u = |W| ex + 9 EPS (|dw_b| + |W| (|x| + ex))
  mean        half wave = pixel: a lane adds its V = C / 32 values (8; 10 at 320 channels), half_sum is five more additions,
              the product with fp32 1/C (not a power of two at 320: its own rounding) -- at most n = V + 8 roundings with the
              squares' below:                                  e_m = mean(e_u) + n EPS mean|u|
  d = u - m   one rounding:                                    e_d = e_u + e_m + EPS |d|
  var         the same chain over the squares (each rounded, or fused):
                                                               e_v = mean(2 |d| e_d + e_d^2) + n EPS mean((|d| + e_d)^2)
  rstd        rsqrtf(var + LN_EPS): the sum's rounding, v_rsq_f32's ulp, LN_EPS's own rounding (3 EPS) around the interval
              [(v + e_v)^-1/2, (max(v - e_v, 0) + LN_EPS)^-1/2] -- no first-order step: a nearly constant pixel has e_v ~ v
  y           d rstd (one rounding), times ln_w plus ln_b (two roundings, or one fma), then ONE rounding to the operand type
              (MP<T>::st8; fp8 clamps to +-448 first: the reference asserts |y| <= 448):   r(y) = U (|y| + e) + SUB
  filters     ONE rounding of each value to the operand type (pack_frag_kernel / _split_ / _fp8_), fc2's of fl32(gamma W2);
              fp8 rounds S w, S the power of two of scale_from_max_kernel; fc1's sum (b1 S1 + ...) is multiplied by 1/S1 in
              front of the GELU, the residual rides through a block times S2 and comes back times 1/S2: all exact.  The
              filter is an input, so this error is not bounded but computed (filter_err: round to nearest even, which
              test_pack_s2p holds the packers to bit for bit).
  products    |W| e_y + e_W (|y| + e_y), summed over k; f16x2 drops lo x lo (MP<f16x2_t>::run):
              (2^-11 |w| + 2^-25)(2^-11 |y| + 2^-25) per product
  fc1 sums    fp32, C products onto b1 (+ the S1 product):     acc(C + 2, sum |W||y| + |b1|)
  keeping     the training forward rounds the pre-activation to the operand type BEFORE the GELU (MP<T>::roundtrip: the
              backward differentiates at the rounded value):   e_a += r(a)
  gelu        gelu_ref._gelu_f (its fp32 evaluation) + L_GELU e_a, then ONE rounding of g to the operand type (MP<T>::st4;
              fp8 clamps to +-448 first: the reference asserts |g| <= 448 unless saturate=True)
  fc2 sums    fp32, ONE chain: the residual accumulator takes gamma b2 (a product and an addition) and then, chunk after
              chunk, m = 4C / KSTEP MFMAs (three times as many in the split mode) of KSTEP = 32 (fp8: 128) products each.  An
              MFMA adds its KSTEP products in some order (KSTEP roundings of their sum at most) and that sum to the
              accumulator (two roundings allowed):           KSTEP EPS P + (2 m + 2) EPS (P + |gamma b2| + |x| + ex),
              P = sum |gamma W2||g|
  320         channels 256 .. 319 live in tiles shared by wave pairs: the pair's two accumulators (the lead's carries x,
              gamma b2 and the first half of every chunk's k-steps, the other's the second half) are never merged, they
              meet in ONE extra fp32 addition wherever x is read (every block start, the stage output).  Their roundings are
              relative to the partial sums, which cancellation can leave larger than x: the accumulation term takes
              M = |x_in| + sum over the blocks so far of (|gamma b2| + P) in place of P + |gamma b2| + |x| + ex, and every read
              adds EPS (|x| + ex).
  downsample  the same LayerNorm chain on ex-carrying rows, one rounding of yd to the operand type -- bf16 in the fp8 mode
              (TD in the kernel, prec_down3 in the handle), the filter's computed error in that type, 4C products onto ds_b:
                                                               acc(4C + 4C / 32 + 2, sum |Wd||yd| + |ds_b|)
Kept rows of the keeping form (keep=True): xin is the block's fp32 input (block 0: x_in's bits; its bound is ex), xn, a and hh
are one rounding to the operand type of y, a and g (bounds e_y, e_a, e_g above), ds_patches of yd.  pair_ratio() checks what
no bound against float64 can: that hh is the GELU of the ROUNDED a that was kept, to the GELU's evaluation and one rounding.

A worst-case bound over 256 .. 1280 products is wide (fp8: ~2^-4 of the sum of absolute products), so there are two kinds
of input.  DENSE cases (dense_blocks / dense_down) are seeded Gaussian filters at the network's scales with every gamma
regime, the small ones in front; maps_x adds the LayerNorm's edges (a pixel whose depthwise output is nearly constant, a map
with a large common offset, a pixel times 30).  SPOTLIGHT cases (spot_blocks / spot_down): depthwise filters whose central
5x5 is zero but for one or two taps per channel -- tap (7 c + 3 + 5 j) mod 25, so the channels of a block cover all 25, that
is every (output pixel, input pixel) pair -- with a dense outer ring, which nothing may read; stage 3's fc1 / fc2 maps (one
or two fc1 non-zeros per hidden unit, four fc2 non-zeros per channel, every hidden unit in exactly one, magnitudes
(1 + m/8) 2^-e exact in e4m3) with the multiplier SPOT_STEP = 203: a channel's four hidden units are 203, 406 and 609 apart,
each at least a chunk of 128 and at most 4C - 128, so they lie in four different chunks, and 203 is 11 mod 32 and 75 mod 128:
four k positions of a fragment in every mode; a downsample filter with ONE non-zero per output, at pixel (co + co / 4) mod 4
and channel (7 co + 1) mod C, of magnitude (1 + odd/64) 2^-e: exact in bf16 and f16, NOT in e4m3 (fault ds_fp8).

FAULTS are applied to the float64 computation (stage2_ref(fault=...)); test_stage2_reference.py shows that each leaves the
bound in every mode it applies to.  emulate() is the kernel's arithmetic in fp32 / the operand types with torch.

Fragment layouts (stage2p.hip's packer comments; frag_pos / pack_s2p_host / unpack_s2p): a 16-bit image is
[row tile of 16][k-step of 32][lane 64][8], lane l = tile row l & 15, k = 32 s + 8 (l >> 4) + j.  f16x2: the same, 2 KiB per
fragment: 512 heads then 512 remainders.  fp8: k-steps of 128, a lane holds 32 k (k = 128 s + 32 (l >> 4) + j), in memory
[lane][j 0..15] then [lane][j 16..31].  reorder_down reads a [rows][cin][2][2] filter as k = (2 ky + kx) cin + c.
"""
import torch

from gelu_ref import EPS, GELU_DEG, L_GELU, _gelu_f, gelu_erf, gelu_poly
from stage3_ref import (ESZ, F32, F64, FP8_MAX, LN_EPS, ODT, PARAMS, PRECS, acc, bits, dense_blocks, filter_err,  # noqa: F401
                        fp8_scale, host_round, lolo, outside, planes, products, ratio, rnd_err)
import stage3_ref as S3

WIDTHS = (256, 320)
PRECS_AT = {256: PRECS, 320: ("bf16", "f16")}
KEEP_PRECS = ("bf16", "f16")
DOWN = ("ds_ln_w", "ds_ln_b", "ds_w", "ds_b")
CHUNK = 128
PIX = (0, 1, 3, 4)                       # the pixels the 2x2 stride-2 convolution reads, in k order q = 2 ky + kx
KSTEP = {"bf16": 32, "f16": 32, "f16x2": 32, "fp8": 128}
SPOT_STEP = 203                          # odd, prime to 1024 and 1280 (203 = 7 x 29)


def spot_maps(C):
    return S3.spot_maps(C, SPOT_STEP)


def down_prec(prec):
    return "bf16" if prec == "fp8" else prec


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def maps_x(C, B, seed, P0, edges=True):
    """fp32 maps [B][9][C]: ordinary ones, and (edges) of every eight alerts one whose centre pixel the first block's
    depthwise step (P0: its centre tap must be non-zero) makes nearly constant (only pixel 4 is non-zero; u[4] = 1 + noise
    whose variance is a tenth of LN_EPS), one with a large common offset and one with pixel 7 times 30"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 9, C, generator=g)
    wc = P0["dw_w"][:, 0, 3, 3]
    for r in range(B):
        if r % 8 == 1 and edges and bool((wc != 0).all()):
            v = (1.0 + 3e-4 * x[r, 4] - P0["dw_b"]) / wc
            x[r] = 0.0
            x[r, 4] = v
        elif r % 8 == 2:
            x[r] = 100.0 + x[r]
        elif r % 8 == 3:
            x[r, 7] = 30.0 * x[r, 7]
    return x


def scale_gamma(blocks, f):
    """the blocks with every layer scale times f (a power of two, or 0: the stage passes its input through)"""
    for P in blocks:
        P["gamma"] = P["gamma"] * f
    return blocks


def dense_down(C, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(ds_ln_w=1.0 + 0.1 * torch.randn(C, generator=g), ds_ln_b=0.1 * torch.randn(C, generator=g),
                ds_w=torch.randn(2 * C, C, 2, 2, generator=g) * (4 * C) ** -0.5, ds_b=0.2 * torch.randn(2 * C, generator=g))


def spot_taps(C, j):
    """-> (t1 [C], t2 [C] (-1: none)): the central 5x5 taps (0 .. 24, tap t = 7x7 position (1 + t / 5, 1 + t % 5)) of block j's
    channels"""
    c = torch.arange(C)
    t1 = (7 * c + 3 + 5 * j) % 25
    t2 = (11 * c + 8 + j) % 25
    t2 = torch.where((c % 2 == 1) & (t2 != t1), t2, torch.full_like(t2, -1))
    return t1, t2


def spot_blocks(C, depth, seed, dw="sparse"):
    """stage 3's sparse fc1 / fc2 (its docstring) and, dw == "sparse", depthwise filters with one or two central taps per
    channel and a dense outer ring; dw == "dense": stage 3's dense taps (centre 0.8 +- 0.2)"""
    blocks = S3.spot_blocks(C, depth, seed, SPOT_STEP)
    if dw == "dense":
        return blocks
    g = torch.Generator().manual_seed(seed + 1000)
    c = torch.arange(C)
    for j, P in enumerate(blocks):
        w = 0.2 * torch.randn(C, 7, 7, generator=g)
        w[:, 1:6, 1:6] = 0.0
        t1, t2 = spot_taps(C, j)
        w[c, 1 + t1 // 5, 1 + t1 % 5] = torch.where((c + j) % 3 == 0, -1.0, 1.0) * S3._mag(c + j, 2)
        two = t2 >= 0
        w[c[two], 1 + t2[two] // 5, 1 + t2[two] % 5] = torch.where((c[two] + j) % 2 == 0, -1.0, 1.0) * S3._mag(c[two] + 2 + j, 2)
        P["dw_w"] = w.view(C, 1, 7, 7)
    return blocks


def spot_down_map(C):
    """-> (q [2C], c [2C]): the patch pixel (k order: PIX[q]) and the channel output co reads"""
    co = torch.arange(2 * C)
    return (co + co // 4) % 4, (7 * co + 1) % C


def spot_down(C, seed):
    g = torch.Generator().manual_seed(seed)
    co = torch.arange(2 * C)
    q, c = spot_down_map(C)
    w = torch.zeros(2 * C, C, 2, 2)
    w[co, c, q >> 1, q & 1] = torch.where(co % 3 == 0, -1.0, 1.0) * (1.0 + (2 * (co % 16) + 1).to(F32) / 64.0) * 2.0 ** -(co % 2).to(F32)
    return dict(ds_ln_w=1.0 + 0.1 * torch.randn(C, generator=g), ds_ln_b=0.1 * torch.randn(C, generator=g), ds_w=w,
                ds_b=torch.where(co % 2 == 0, 0.75, -0.5) * (1.0 + 0.25 * torch.rand(2 * C, generator=g)))


def saturating(C, seed, alert=3):
    """-> (x [B = 6][9][C], x_plain, blocks, alert): one spotlight block (dense taps) whose LayerNorm has weight 16 at the
    channel that a hidden unit reads with the weight +1.75 (weight 24 there), and one alert whose only non-zero pixel (4) the depthwise step
    turns into a spike there: at pixel 4 the normalised value is sqrt(C - 1), y = 24 sqrt(255) ~ 383 (inside e4m3's range)
    and that unit's a ~ 670 > 448.  x_plain: the alert left ordinary."""
    blocks = spot_blocks(C, 1, seed, dw="dense")
    b0 = blocks[0]
    chan = int(b0["fc1_w"].max(0).values.argmax())
    assert float(b0["fc1_w"][:, chan].max()) == 1.75
    b0["ln_w"][chan] = 24.0
    b0["ln_b"][chan] = 0.0
    x_plain = maps_x(C, 6, seed + 1, b0, edges=False)
    x = x_plain.clone()
    spike = torch.zeros(C)
    spike[chan] = 1.0
    x[alert] = 0.0
    x[alert, 4] = (spike - b0["dw_b"]) / b0["dw_w"][:, 0, 3, 3]
    return x, x_plain, blocks, alert


# ---------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("no_dw_b", "tap_row", "tap_col", "outer_ring", "wrap", "no_ln_eps", "no_b1", "b2_unscaled", "no_residual",
          "swap_fc1_tile", "fc2_kstep_stale", "no_last_chunk", "no_inv_s1", "no_inv_s2", "planes_swapped", "ds_pixel",
          "ds_ln_from_block", "alert_prev_map", "gelu_unrounded", "shared_tile_lead_only", "ds_fp8")
FAULT_PRECS = {"no_inv_s1": ("fp8",), "no_inv_s2": ("fp8",), "ds_fp8": ("fp8",), "planes_swapped": ("f16x2",),
               "gelu_unrounded": KEEP_PRECS}
FAULT_WIDTHS = {"shared_tile_lead_only": (320,)}      # (every other fault: 256 channels, where every mode runs)


def dw_matrix(dw_w, fault=None):
    """[C][9 out][9 in] float64: the tap output pixel o applies to input pixel i.  Faults: tap_row / tap_col (the tap one
    row / column further), outer_ring (the 5x5 window taken from the 7x7's corner: ky, kx instead of ky + 1, kx + 1, so the
    ring's taps are applied), wrap (wrap-around in place of the zero padding: all 49 taps land on the map)"""
    w = dw_w.to(F64).reshape(-1, 49)
    M = torch.zeros(w.shape[0], 9, 9, dtype=F64)
    for o in range(9):
        oy, ox = o // 3, o % 3
        if fault == "wrap":
            for ky in range(7):
                for kx in range(7):
                    M[:, o, ((oy + ky - 3) % 3) * 3 + (ox + kx - 3) % 3] += w[:, ky * 7 + kx]
            continue
        for i in range(9):
            ky, kx = i // 3 - oy + 3, i % 3 - ox + 3
            ky += 1 if fault == "tap_row" else -1 if fault == "outer_ring" else 0
            kx += 1 if fault == "tap_col" else -1 if fault == "outer_ring" else 0
            M[:, o, i] = w[:, ky * 7 + kx]
    return M


def _ln(u, e_u, lnw, lnb, eps, want_bound):
    """rows [N][C] -> (y, its fp32 error e_y32 in front of the operand rounding)"""
    C = u.shape[1]
    mean = u.mean(1, keepdim=True)
    d = u - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = (var + eps) ** -0.5
    t = d * rstd
    y = t * lnw + lnb
    if not want_bound:
        return y, None
    n = C // 32 + 8
    e_m = e_u.mean(1, keepdim=True) + n * EPS * u.abs().mean(1, keepdim=True)
    e_d = e_u + e_m + EPS * d.abs()
    e_v = (2 * d.abs() * e_d + e_d * e_d).mean(1, keepdim=True) + n * EPS * ((d.abs() + e_d) ** 2).mean(1, keepdim=True)
    r_hi = ((var - e_v).clamp(min=0) + LN_EPS) ** -0.5
    r_lo = (var + e_v + LN_EPS) ** -0.5
    e_r = torch.maximum(r_hi - rstd, rstd - r_lo) + 3 * EPS * r_hi
    e_t = e_d * (rstd + e_r) + d.abs() * e_r + EPS * t.abs()
    return y, e_t * lnw.abs() + EPS * (t * lnw).abs() + EPS * y.abs()


def _mlp(x, ex, u, e_u, mag, P, prec, fault, o):
    """the block behind its depthwise step on rows [N][C]: x the residual, u the LayerNorm's input -> (x', ex', mag', kept)"""
    f = lambda k: P[k].to(F64)   # noqa: E731
    N, C = x.shape
    H = 4 * C
    lnw, lnb, W1, b1, W2, b2, gam = (f(k) for k in PARAMS[2:])
    want = o["want"]
    y, e_y32 = _ln(u, e_u, lnw, lnb, 0.0 if fault == "no_ln_eps" else o["ln_eps"], want)
    S1 = fp8_scale(W1.abs().max()) if prec == "fp8" else 1.0
    a = y @ W1.t() + (0.0 if fault == "no_b1" else b1)
    if fault == "planes_swapped":   # fc1's heads and remainders exchanged: hi(w) lo(y) is the product left out
        yl = y - y.to(F32).half().to(F64)
        a = a - yl @ W1.to(F32).half().to(F64).t()
    if fault == "no_inv_s1":
        a = a * S1
    g = o["gelu"](a)
    if prec == "fp8":
        if want:
            assert float(y.abs().max()) <= FP8_MAX, "|y| beyond e4m3's range"
            assert o["saturate"] or float(g.abs().max()) <= FP8_MAX, "|g| beyond e4m3's range outside the saturation case"
        if o["clamp_g"]:
            g = g.clamp(-FP8_MAX, FP8_MAX)
    gu = g
    if fault == "swap_fc1_tile":    # chunk 1: the hidden tiles of waves 0 and 1 exchanged
        gu = g.clone()
        gu[:, CHUNK:CHUNK + 16], gu[:, CHUNK + 16:CHUNK + 32] = g[:, CHUNK + 16:CHUNK + 32], g[:, CHUNK:CHUNK + 16]
    if fault == "fc2_kstep_stale":  # chunk 3's second k-step (fp8: its only one) read from the image that holds chunk 1
        gu = g.clone()
        k0, kn = (0, CHUNK) if prec == "fp8" else (KSTEP[prec], KSTEP[prec])
        gu[:, 3 * CHUNK + k0:3 * CHUNK + k0 + kn] = g[:, CHUNK + k0:CHUNK + k0 + kn]
    if fault == "no_last_chunk":
        gu = g.clone()
        gu[:, H - CHUNK:] = 0.0
    GW = gam[:, None] * W2
    gw32 = (P["gamma"].to(F32)[:, None] * P["fc2_w"].to(F32)).to(F64)   # what the packer rounds: fl32(w gamma)
    S2 = fp8_scale(gw32.abs().max()) if prec == "fp8" else 1.0
    z = gu @ GW.t()
    if fault == "shared_tile_lead_only":   # channels 256 ..: only the lead wave's half of every chunk's k-steps
        h = torch.arange(H)
        z[:, 256:] = (gu * (h % CHUNK < CHUNK // 2)) @ GW[256:].t()
    if fault == "no_inv_s2":
        z = z * S2
    gb2 = b2 if fault == "b2_unscaled" else gam * b2
    xn = gb2 + z if fault == "no_residual" else x + gb2 + z
    if not want:
        return xn, None, None, None
    # ---- the bound (module docstring)
    e_y = e_y32 + rnd_err(prec, y, e_y32)
    e_w1 = filter_err(prec, P["fc1_w"], None, S1)
    ay, aw1 = y.abs() + e_y, W1.abs() + e_w1
    e_a = e_y @ W1.abs().t() + ay @ e_w1.t() + lolo(prec, ay, aw1) + acc(C + 2, ay @ aw1.t() + b1.abs())
    if o["keep"]:
        e_a = e_a + rnd_err(prec, a, e_a)
    e_gv = _gelu_f(prec, a) + L_GELU * e_a
    e_g = e_gv + rnd_err(prec, g, e_gv)
    e_gw = filter_err(prec, P["fc2_w"], P["gamma"], S2)
    ag, agw = g.abs() + e_g, GW.abs() + e_gw
    prod = ag @ agw.t()
    mag = mag + gb2.abs() + prod
    shared = (torch.arange(C) >= 256).to(F64)          # 320 channels: the tiles that wave pairs share
    base = shared * mag + (1 - shared) * (x.abs() + ex + gb2.abs() + prod)
    m = H // KSTEP[prec] * (3 if prec == "f16x2" else 1)
    e_z = e_g @ GW.abs().t() + ag @ e_gw.t() + lolo(prec, ag, agw) + acc(KSTEP[prec], prod) + acc(2 * m + 2, base)
    e_x = ex + e_z
    e_x = e_x + shared * EPS * (xn.abs() + e_x)
    for k, v in dict(e_y=e_y, e_a=e_a, e_g=e_g, e_z=e_z, e_x=e_x, g=g).items():
        assert bool(torch.isfinite(v).all()), k
    kept = dict(xin=(x, ex), xn=(y, e_y), a=(a, e_a), hh=(g, e_g)) if o["keep"] else None
    return xn, e_x, mag, kept


def _down(x, ex, P, D, prec, fault, o):
    """x [B][9][C] the stage output -> (out [B][2C], its bound, (patch [B][4C], its bound))"""
    B, _, C = x.shape
    pd = down_prec(prec)
    want = o["want"]
    pix = (0, 1, 2, 3) if fault == "ds_pixel" else PIX
    lnw, lnb = (P["ln_w"].to(F64), P["ln_b"].to(F64)) if fault == "ds_ln_from_block" else (D["ds_ln_w"].to(F64), D["ds_ln_b"].to(F64))
    rows = x[:, pix, :].reshape(B * 4, C)
    erows = ex[:, PIX, :].reshape(B * 4, C) if want else None
    yd, e_y32 = _ln(rows, erows, lnw, lnb, o["ln_eps"], want)
    patch = yd.reshape(B, 4 * C)
    Wd32 = reorder_down(D["ds_w"])
    Wd = Wd32.to(F64)
    if fault == "ds_fp8":
        Wd = Wd32.to(ODT["fp8"]).to(F64)
    out = patch @ Wd.t() + D["ds_b"].to(F64)
    if not want:
        return out, None, None
    e_yd = e_y32 + rnd_err(pd, yd, e_y32)
    e_p = e_yd.reshape(B, 4 * C)
    e_wd = filter_err(pd, Wd32, None, 1.0)
    ap, awd = patch.abs() + e_p, Wd.abs() + e_wd
    K = 4 * C
    e_out = e_p @ Wd.abs().t() + ap @ e_wd.t() + lolo(pd, ap, awd) + acc(K + K // 32 + 2, ap @ awd.t() + D["ds_b"].to(F64).abs())
    assert bool(torch.isfinite(e_out).all())
    return out, e_out, (patch, e_p)


def _opts(prec, keep, saturate, clamp_g, gelu, ln_eps, want):
    assert not keep or prec in KEEP_PRECS
    return dict(want=want, keep=keep, saturate=saturate, clamp_g=clamp_g, ln_eps=LN_EPS if ln_eps is None else ln_eps,
                gelu=gelu_erf if gelu == "erf" else (lambda a: gelu_poly(a, GELU_DEG[prec])))


def stage2_ref(x, blocks, down, prec, fault=None, keep=False, G=4, saturate=False, clamp_g=False, gelu="poly", ln_eps=None,
               bound=True):
    """-> dict(out=(ref, bound) [B][2C], tap=(ref, bound) [B][9][C], keep=[per block dict of (ref, bound): xin [B][9][C], xn,
    a, hh [B][9][4C]] and patches=(ref, bound) [B][4C] when keep): float64.  fault: one of FAULTS, applied to the float64
    computation (the bounds are then None); G: the alerts per workgroup that alert_prev_map assumes.  saturate / clamp_g: as
    stage3_ref.  gelu="erf", ln_eps, bound=False: the oracle's GELU and epsilon and no bound, for the comparison with it."""
    assert fault is None or fault in FAULTS
    want = fault is None and bound
    o = _opts(prec, keep, saturate, clamp_g, gelu, ln_eps, want)
    x = x.to(F64)
    B, _, C = x.shape
    ex = torch.zeros_like(x)
    mag = x.abs().reshape(B * 9, C)
    kept = []
    for P in blocks:
        M = dw_matrix(P["dw_w"], fault)
        dwb = torch.zeros(C, dtype=F64) if fault == "no_dw_b" else P["dw_b"].to(F64)
        xs = x
        if fault == "alert_prev_map":   # alert g of a workgroup reads alert g - 1's map
            xs = x.clone()
            for b in range(B):
                if b % G:
                    xs[b] = x[b - 1]
        u = torch.einsum("bic,coi->boc", xs, M) + dwb
        e_u = None
        if want:
            Ma = M.abs()
            e_u = torch.einsum("bic,coi->boc", ex, Ma) + 9 * EPS * (dwb.abs() + torch.einsum("bic,coi->boc", x.abs() + ex, Ma))
            e_u = e_u.reshape(B * 9, C)
        xr, er, mag, k = _mlp(x.reshape(B * 9, C), ex.reshape(B * 9, C), u.reshape(B * 9, C), e_u, mag, P, prec, fault, o)
        x = xr.reshape(B, 9, C)
        ex = er.reshape(B, 9, C) if want else ex
        if k is not None:
            kept.append({n: (v.reshape(B, 9, -1), e.reshape(B, 9, -1)) for n, (v, e) in k.items()})
    out, e_out, patches = _down(x, ex, blocks[-1], down, prec, fault, o)
    res = dict(out=(out, e_out), tap=(x, ex if want else None))
    if keep and want:
        res["keep"], res["patches"] = kept, patches
    return res


def rows_ref(x, P, prec, fault=None):
    """the row-tile form: x [rows][256] -> (x', bound): the MLP half alone (the LayerNorm reads x itself)"""
    x = x.to(F64)
    o = _opts(prec, False, False, False, "poly", None, fault is None)
    xn, e_x, _, _ = _mlp(x, torch.zeros_like(x), x, torch.zeros_like(x), x.abs(), P, prec, fault, o)
    return xn, e_x


def kept_pair(a64, prec, fault=None):
    """what the keeping form stores of a float64 pre-activation: (round(a), round(gelu(round(a)))) in the operand type;
    fault gelu_unrounded: the GELU taken at a itself"""
    ar = a64.to(F32).to(ODT[prec])
    src = a64 if fault == "gelu_unrounded" else ar.to(F64)
    return ar, gelu_poly(src, GELU_DEG[prec]).to(F32).to(ODT[prec])


def pair_ratio(a_kept, hh_kept, prec):
    """worst |hh - gelu(a)| / (the GELU's fp32 evaluation error at a + one rounding of the result), a and hh as kept"""
    a = a_kept.to(F64)
    g = gelu_poly(a, GELU_DEG[prec])
    e = _gelu_f(prec, a)
    return ratio(hh_kept.to(F64), g, e + rnd_err(prec, g, e))


# ---------------------------------------------------------------------------------------------------------------------
# emulation: the kernel's arithmetic in fp32 / the operand types
# ---------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fp32 fma (the product is exact in float64; the double rounding of the sum is rare and one ulp)"""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def _ln32(u, lnw, lnb):
    d = u - u.mean(1, keepdim=True)
    return d * torch.rsqrt((d * d).mean(1, keepdim=True) + 1e-6) * lnw + lnb


def _mlp32(x, u, P, prec, keep):
    lnw, lnb, W1, b1, W2, b2, gam = (P[k].to(F32) for k in PARAMS[2:])
    y = _ln32(u, lnw, lnb)
    s1 = fp8_scale(W1.abs().max()) if prec == "fp8" else 1.0
    yp = planes(prec, y)
    a = (products(yp, planes(prec, W1 * s1)) + b1 * s1) * (1.0 / s1)
    if keep:
        a = a.to(ODT[prec]).float()
    g = gelu_poly(a.to(F64), GELU_DEG[prec]).to(F32)
    gw = W2 * gam[:, None]
    s2 = fp8_scale(gw.abs().max()) if prec == "fp8" else 1.0
    gp = planes(prec, g)
    z = ((x + gam * b2) * s2 + products(gp, planes(prec, (W2 * gam[:, None]) * s2))) * (1.0 / s2)
    return z, dict(xin=x, xn=yp[0], a=a, hh=gp[0])


def emulate(x, blocks, down, prec, keep=False):
    """-> dict(out, tap, keep, patches) as stage2_ref's, fp32 values (the kept rows rounded to the operand type)"""
    x = x.to(F32).clone()
    B, _, C = x.shape
    kept = []
    for P in blocks:
        M = dw_matrix(P["dw_w"]).to(F32)
        u = P["dw_b"].to(F32).expand(B, 9, C).clone()
        for i in range(9):
            u = _fma(M[:, :, i].t()[None], x[:, i:i + 1, :], u)
        z, k = _mlp32(x.reshape(B * 9, C), u.reshape(B * 9, C), P, prec, keep)
        x = z.reshape(B, 9, C)
        kept.append({n: v.reshape(B, 9, -1) for n, v in k.items()})
    pd = down_prec(prec)
    yd = planes(pd, _ln32(x[:, PIX, :].reshape(B * 4, C), down["ds_ln_w"].to(F32), down["ds_ln_b"].to(F32)))
    patch = [p.reshape(B, 4 * C) for p in yd]
    out = products(patch, planes(pd, reorder_down(down["ds_w"]))) + down["ds_b"].to(F32)
    return dict(out=out, tap=x, keep=kept, patches=patch[0])


def emulate_rows(x, P, prec):
    x = x.to(F32)
    return _mlp32(x, x, P, prec, False)[0]


# ---------------------------------------------------------------------------------------------------------------------
# fragment layouts
# ---------------------------------------------------------------------------------------------------------------------
def reorder_down(w):
    """a downsample filter [rows][cin][2][2] -> [rows][K = 4 cin], k = (2 ky + kx) cin + c"""
    rows, cin = w.shape[:2]
    return w.reshape(rows, cin, 4).permute(0, 2, 1).reshape(rows, 4 * cin).contiguous()


def pack_s2p_host(vals, prec):
    """host packer, written along the kernels: element i of the image -> its (row, k).  vals: host_round's result for the
    [rows][K] matrix in k order (reorder_down's for a downsample filter).  -> the image as a flat uint8 tensor"""
    hi = vals[0] if prec == "f16x2" else vals
    rows, K = hi.shape
    i = torch.arange(rows * K)
    if prec == "fp8":
        j, l, fs = i & 31, (i >> 5) & 63, i >> 11
        s, tile = fs % (K // 128), fs // (K // 128)
        k = 128 * s + 32 * (l >> 4) + j
        at = fs * 2048 + (j >> 4) * 1024 + l * 16 + (j & 15)
    else:
        j, l, fs = i & 7, (i >> 3) & 63, i >> 9
        s, tile = fs % (K // 32), fs // (K // 32)
        k = 32 * s + 8 * (l >> 4) + j
        at = fs * 1024 + l * 8 + j if prec == "f16x2" else i
    row = 16 * tile + (l & 15)
    if prec == "f16x2":
        img = torch.zeros(2 * rows * K, dtype=torch.float16)
        img[at] = vals[0][row, k]
        img[at + 512] = vals[1][row, k]
    else:
        img = torch.zeros(rows * K, dtype=vals.dtype)
        img[at] = vals[row, k]
    return img.view(torch.uint8)


def frag_pos(prec, rows, K):
    """the inverse map: position [rows][K] of element (row, k) in the image, counted in operand values (f16x2: of its head,
    in f16 values; the remainder lies 512 further)"""
    row, k = torch.arange(rows)[:, None], torch.arange(K)[None, :]
    tile, r = row // 16, row % 16
    if prec == "fp8":
        s, kg, j = k // 128, (k % 128) // 32, k % 32
        fs = tile * (K // 128) + s
        return fs * 2048 + (j >> 4) * 1024 + (16 * kg + r) * 16 + (j & 15)
    s, kg, j = k // 32, (k % 32) // 8, k % 8
    fs = tile * (K // 32) + s
    return (fs * 64 + 16 * kg + r) * 8 + j + (fs * 512 if prec == "f16x2" else 0)


def unpack_s2p(image, prec, rows, K):
    """a packed image (flat uint8) -> the operand values [rows][K] in k order: a tensor of the operand type, or (heads,
    remainders)"""
    image = image.reshape(-1)
    assert image.dtype == torch.uint8 and image.numel() == rows * K * ESZ[prec]
    pos = frag_pos(prec, rows, K)
    if prec == "f16x2":
        v = image.view(torch.float16)
        return v[pos], v[pos + 512]
    return image.view(ODT[prec])[pos]
