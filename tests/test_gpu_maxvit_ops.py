"""The MaxViT branch's hand-written kernels one at a time (btsbot_op_mv_*) against plain float64 references.

Conventions are test_gpu_gemm_paths.py's: operands are exact values of the operand type, references are float64
torch (on the device) built from oracle/maxvit_oracle.py's partition functions and rel_pos_index, every output is a
slice of a larger buffer whose head and tail hold a sentinel bit pattern that must survive, and each test prints its
worst err / bound.  u = one rounding of the type (2^-8 bf16, 2^-11 f16, 0 fp32), SUB = 2^-25 for f16's subnormals,
EPS = 2^-24.

Attention (mv_attn impl 0 = mv_attn_kernel, impl 1 = mv_attn_mfma_kernel), per output element, all against
A = softmax @ |V|:

    |out - ref| <= u |out| + SUB + [(e^(2 delta) - 1) + u_P + 121 EPS] A + SUB_P sum_j |V_j|

  delta   the largest perturbation of a logit of the query: the 32 fp32 products and their sum, (32 + 4) EPS
          (|q| scale) . |k|; the scale-and-bias fma, the subtraction of the maximum and __expf's argument rounding,
          4 EPS (|s| + |max|); v_exp_f32's result, 3 EPS.  Numerator and denominator of the softmax each move by at
          most e^delta, hence e^(2 delta) - 1;
  u_P     impl 1 rounds the unnormalised P (in (0, 1]) to the operand type before the second MFMA, the sum keeps
          fp32: u A, and SUB_P = 2^-25 per key where an f16 P is subnormal (the sum is >= 1);
  121 EPS the fp32 sums of the denominator (49 terms) and of P V (64 slots on the MFMA), 1 / sum and its product.

The index-map probes set q = k = 0, so every logit is its bias exactly and delta is __expf's own 3 EPS: probe 1 (zero
table) must give the mean of V over exactly the row's own partition, probe 2 (random table) softmax(bias) @ V; what is
left of the bound is one output rounding and the fp32 sums.

Fused kernels (mv_attn_block at C = 64; mv_part at C = 64 / 128 / 256: attention half alone, with the MLP half, with
post_out).  The tolerance cannot be derived in closed form through softmax and GELU; it is measured on the reference
alone.  R is the float64 result; R~ the same float64 computation with a round-to-type at each point where the kernel
writes a 16-bit image: LN1's output, the qkv rows, the unnormalised P, O, LN2's output, the MLP's hidden rows (and the
output itself where it is 16-bit: xn2, post_out).  E = max |R~ - R| per case and output, and the kernel must satisfy

    max |out - R| <= 2 E + max acc,   acc = EPS (C |O| @ |Wproj|^T + 4C |hidden| @ |W2|^T) + 4 EPS |R|

(the two GEMMs that add into the fp32 residual; the fp32 sums upstream of a rounding point are at most 256 EPS / u
<= 3 % of that rounding and live inside the factor).  Why 2: the kernel's roundings, its __expf and the fp32 order of
its sums are another realisation of the same half-ulp perturbations whose one sample is E.  So that the budget cannot
hide a fault, each case also asserts 2 E <= 0.1 rms(R - x), the block's own update (a window / grid swap moves the
output by about 1.0 rms of the update).  GELU is the kernels' own gelu_poly<3/5> (bf16 / f16) in both R and R~, ported
to float64 in test_gpu_gemm_paths.py, where its fit to the erf form is pinned.  Workgroups that walk more than one
unit: the smallest batches that make them do so with a ragged remainder (bf16, windows); test_walking_arithmetic
asserts the launchers' formulas.  The C = 128 walk needs more than 8192 units and stays with the 1100-alert
batch-independence test of test_gpu_parity.py.

MBConv pieces:
  mv_dw3 / mv_dw3s   9 fp32 taps from the bias (11 EPS (|b| + sum |v| |w s|), the tap image w * s being rounded once),
                     through SiLU (slope L_SILU, evaluation SILU_REL, both from test_gpu_gemm_paths.py), one output
                     rounding.  Border rows and columns of the input are 8x larger, so that a wrong padding tap shows.
                     mv_dw3s's part: the kernel sums the ROUNDED outputs (psum += (float)o[e]), so the sum over groups
                     equals the float64 sum of the stored map within HW EPS sum |y|; part is NaN before the call.
                     (Found by this check, f16 at H = 7, C = 512: hipcc rounded the summed copy straight from the
                     product, v_fma_mixlo_f16, and the stored copy from the fp32 result, so the two differed by an
                     f16 ulp at double-rounding ties, 2^-7 at |y| ~ 10; both kernels now round one opaque value.)
  mv_mbconv_front    R / R~ / 2 E with the rounding point at m1, elementwise: 2 E + u |out| + SUB + 16 EPS
                     (|b2| + sum |m1| |w s|) + SILU_REL |R|; part as above.
  mv_se              mean: (HW + 1) EPS inv sum |y|; fc1: (C + 2) EPS (|W1| @ |mean| + |b1|) plus |W1| @ the mean's
                     error; SiLU as above; fc2 the same with RD; the sigmoid's slope 1/4 and SILU_REL of its value.
  mv_stem            R / R~ / 2 E: R~ rounds the resized samples (the kernel rounds them before the products, as its
                     GEMM form did) and the 112 x 112 x 32 map; acc = 288 EPS |map| * |W2| + 4 EPS |R|.

Out of scope: the elementwise kernels (mv_ln, mv_avgpool2, mv_gate, mv_scale_w, mv_bn_cast, mv_im2col3, mv_final,
mv_resize_im2col) -- the fp32 stage taps of test_gpu_parity.py pin them at 1e-4 and they have no index map of their
own.  The training kernels of maxvit_train_kernels.hip have test_gpu_maxvit_train_ops.py.
"""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_gemm_paths as GP
from btsbot_amd import _lib, ops
from oracle import maxvit_oracle as MO   # checker only

EPS, DT, U, SUB = GP.EPS, GP.DT, GP.U, GP.SUB
L_SILU, SILU_REL = GP.L_SILU, GP.SILU_REL
_guarded, _intact, _check = GP._guarded, GP._intact, GP._check
SCALE = 32 ** -0.5
pytestmark = pytest.mark.gpu


def _rnd(prec):
    T = DT[prec]
    return (lambda t: t) if prec == "f32" else (lambda t: t.to(T).double())


def part_rows(B, H, grid, dev):
    """[B * (H/7)^2, 49] row numbers of the [B*H*H, .] maps, partition by partition, from the oracle's partition."""
    idx = torch.arange(B * H * H, dtype=torch.float64).view(B, H, H, 1)
    p = MO.grid_partition(idx, 7) if grid else MO.window_partition(idx, 7)
    return p.reshape(-1, 49).long().to(dev)


def rel_bias(table64):
    """[heads][query][key] from the [169][heads] table, as oracle.attention_cl indexes it."""
    heads = table64.shape[1]
    idx = MO.rel_pos_index(7).view(-1).to(table64.device)
    return table64[idx].view(49, 49, heads).permute(2, 0, 1)


def attn_ref(qkv64, table64, rows, heads, rnd=None):
    """float64 attention of qkv [N, 3C] ([head][q|k|v][32]) -> out [N, C], A = softmax @ |V|, the logits and
    (|q| scale) . |k|.  rnd: the fused kernels' rounding of the unnormalised P."""
    N = qkv64.shape[0]
    g = qkv64[rows].view(rows.shape[0], 49, heads, 96).permute(0, 2, 1, 3)
    q, k, v = g[..., :32], g[..., 32:64], g[..., 64:]
    s = (q * SCALE) @ k.transpose(-1, -2) + rel_bias(table64)[None]
    sabs = (q.abs() * SCALE) @ k.abs().transpose(-1, -2)
    pu = torch.exp(s - s.amax(-1, keepdim=True))
    den = pu.sum(-1, keepdim=True)
    pn = (rnd(pu) if rnd is not None else pu) / den
    o, a = pn @ v, pn @ v.abs()
    C = heads * 32

    def back(t):
        full = torch.empty(N, C, dtype=torch.float64, device=qkv64.device)
        full[rows.reshape(-1)] = t.permute(0, 2, 1, 3).reshape(-1, C)
        return full
    delta = ((36 * EPS * sabs + 4 * EPS * (s.abs() + s.abs().amax(-1, keepdim=True))).amax(-1, keepdim=True) + 3 * EPS)
    vsum = v.abs().sum(-2, keepdim=True).expand_as(o)
    return back(o), back(a), back(delta.expand_as(o)), back(vsum)


def attn_bound(prec, impl, out, a, delta, vsum):
    up = U[prec] if impl == 1 else 0.0
    subp = SUB[prec] if impl == 1 else 0.0
    return U[prec] * out.double().abs() + SUB[prec] + (torch.expm1(2 * delta) + up + 121 * EPS) * a + subp * vsum


def _run_attn(prec, impl, qkv, table, B, H, C, grid, what, worst):
    N = B * H * H
    obuf, out = _guarded(N * C, DT[prec], qkv.device)
    ops.mv_attn(qkv, table, B, H, grid, impl=impl, precision=prec, out=out.view(N, C))
    ref, a, delta, vsum = attn_ref(qkv.double(), table.double(), part_rows(B, H, grid, qkv.device), C // 32)
    _check(what, out.view(N, C), ref, attn_bound(prec, impl, out.view(N, C), a, delta, vsum), worst)
    assert _intact(obuf, N * C), f"{what}: guard bytes changed"


IMPL_PRECS = [(0, "f32"), (0, "bf16"), (0, "f16"), (1, "bf16"), (1, "f16")]


@pytest.mark.parametrize("grid", [0, 1], ids=["window", "grid"])
@pytest.mark.parametrize("H", [7, 14, 21])
@pytest.mark.parametrize("impl,prec", IMPL_PRECS, ids=[f"impl{i}-{p}" for i, p in IMPL_PRECS])
def test_attn_index_map_probes(cuda, impl, prec, H, grid):
    """q = k = 0.  Probe 1, zero table: every row is the mean of V over exactly its own partition.  Probe 2, random
    table: softmax(bias) @ V -- a transposed bias or a swapped head fails by O(1).  H = 21 (H/7 = 3, no power of two)
    is no model stage, but every launcher accepts it.  V holds integers in [-120, 120], exact in every type."""
    B, C = 3, 128
    N = B * H * H
    g = torch.Generator(device=cuda).manual_seed(H * 10 + grid)
    qkv = torch.zeros(N, C // 32, 96, device=cuda)
    qkv[..., 64:] = torch.randint(-120, 121, (N, C // 32, 32), generator=g, device=cuda).float()
    qkv = qkv.view(N, 3 * C).to(DT[prec])
    worst = {}
    zero = torch.zeros(169, C // 32, device=cuda)
    _run_attn(prec, impl, qkv, zero, B, H, C, grid, "probe1", worst)
    # probe 1 once more in plain terms: the partition mean, from the oracle's partition functions alone
    v = qkv.double().view(B, H, H, 3 * C)
    part = MO.grid_partition(v, 7) if grid else MO.window_partition(v, 7)
    mean = part.mean((1, 2), keepdim=True).expand_as(part).contiguous()
    full = (MO.grid_reverse(mean, 7, H, H) if grid else MO.window_reverse(mean, 7, H, H)).reshape(N, C // 32, 96)[..., 64:]
    out = ops.mv_attn(qkv, zero, B, H, grid, impl=impl, precision=prec)
    _check("probe1.mean", out, full.reshape(N, C), U[prec] * out.double().abs() + 60 * EPS * 120.0, worst)
    table = torch.randn(169, C // 32, generator=g, device=cuda)
    _run_attn(prec, impl, qkv, table, B, H, C, grid, "probe2", worst)
    print(f"[probes impl{impl} {prec} H={H} grid={grid}] err/bound " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


ATTN_SHAPES = {0: [(7, 64), (14, 64), (21, 128)], 1: [(7, 512), (14, 64), (21, 128)]}
ATTN_CASES = [(i, p, h, c) for i, p in IMPL_PRECS for h, c in ATTN_SHAPES[i]]


@pytest.mark.parametrize("grid", [0, 1], ids=["window", "grid"])
@pytest.mark.parametrize("impl,prec,H,C", ATTN_CASES, ids=[f"impl{i}-{p}-H{h}-C{c}" for i, p, h, c in ATTN_CASES])
def test_attn_against_float64(cuda, impl, prec, H, C, grid):
    B = 3
    g = torch.Generator(device=cuda).manual_seed(H + C + grid)
    qkv = torch.randn(B * H * H, 3 * C, generator=g, device=cuda).to(DT[prec])
    table = torch.randn(169, C // 32, generator=g, device=cuda) / (C // 32) ** 0.5
    worst = {}
    _run_attn(prec, impl, qkv, table, B, H, C, grid, "attn", worst)
    print(f"[attn impl{impl} {prec} H={H} C={C} grid={grid}] err/bound {worst['attn']:.3g}")


def mfma_plan(B, H, C):
    """launch_mv_attn_mfma's grid: (units per wave, workgroups along x, units)."""
    units, heads = B * (H // 7) ** 2, C // 32
    upw = min(max(units * heads // (4 * 2048), 1), 8)
    return upw, (units + 4 * upw - 1) // (4 * upw), units


WALK_PART64, WALK_PART256, WALK_ABLK, WALK_MFMA = (9, 56), (65, 14), (33, 56), (1027, 7)


def part_grid(C, units):
    """Workgroups of launch_mv_part: launch_part64_t (C = 64) and launch_part_t (cap 256 at one workgroup per CU,
    C = 256; 4096 per CU-share at two, C = 128) in maxvit_part.hip."""
    return min(units, {64: 512, 128: 4096 * 2, 256: 256}[C])


def ablk_grid(units):
    """Workgroups of launch_mv_attn_block (maxvit_attnblock.hip)."""
    return min(units, 2048)


def test_walking_arithmetic():
    """Host arithmetic only: the batches of the walking cases reach what they are meant to, by mirrors of the launchers'
    formulas (mfma_plan, part_grid, ablk_grid)."""
    B, H = WALK_MFMA
    upw, gx, units = mfma_plan(B, H, 512)
    assert units * 16 == 16432 and upw == 2 and gx == 129
    left = units - (gx - 1) * 4 * upw          # the last workgroup: one full wave, one that breaks mid-loop, two idle
    assert left == 3 and left // upw == 1 and left % upw == 1
    assert mfma_plan(1026, 7, 512)[0] == 2 and mfma_plan(3, 21, 128)[0] == 1 and mfma_plan(1023, 7, 512)[0] == 1
    for (b, h), grid_of, want in ((WALK_PART64, lambda u: part_grid(64, u), 576),
                                  (WALK_PART256, lambda u: part_grid(256, u), 260), (WALK_ABLK, ablk_grid, 2112)):
        per = (h // 7) ** 2
        units = b * per
        # some workgroups walk two units, the others one; one alert fewer and nobody walks
        assert units == want and grid_of(units) < units < 2 * grid_of(units), (units, grid_of(units))
        assert grid_of(units - per) == units - per, (b, h)
    # C = 128 walks only above 8192 units: none of this file's shapes (the largest is B = 3 at H = 21)
    assert part_grid(128, 3 * 9) == 27 and part_grid(128, 8193) == 8192


def test_attn_mfma_two_units_per_wave(cuda):
    """bf16, H = 7, C = 512, B = 1027: upw = 2 and a ragged last workgroup (test_walking_arithmetic); the reference in
    float64 on the device, in chunks of alerts."""
    (B, H), C, prec = WALK_MFMA, 512, "bf16"
    N = B * 49
    g = torch.Generator(device=cuda).manual_seed(5)
    qkv = torch.randn(N, 3 * C, generator=g, device=cuda).to(DT[prec])
    table = torch.randn(169, 16, generator=g, device=cuda) / 4.0
    obuf, out = _guarded(N * C, DT[prec], cuda)
    ops.mv_attn(qkv, table, B, H, 0, impl=1, precision=prec, out=out.view(N, C))
    assert _intact(obuf, N * C), "guard bytes changed"
    out = out.view(N, C)
    worst = {}
    for b0 in range(0, B, 128):
        nb = min(128, B - b0)
        sl = slice(b0 * 49, (b0 + nb) * 49)
        ref, a, delta, vsum = attn_ref(qkv[sl].double(), table.double(), part_rows(nb, H, 0, cuda), 16)
        _check(f"alerts {b0}..", out[sl], ref, attn_bound(prec, 1, out[sl], a, delta, vsum), worst)
    print(f"[attn_mfma upw=2 B={B}] err/bound {max(worst.values()):.3g}")


# ---- fused partition kernels
def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    return d * torch.rsqrt((d * d).mean(-1, keepdim=True) + 1e-6) * w + b


def part_params(C, prec, g, dev):
    """random_state_dict-style parameters (fan-in scaled filters rounded to the type, norm scales near 1, small
    biases); the table is randn / sqrt(heads)."""
    T = DT[prec]

    def w(n, k):
        return (torch.randn(n, k, generator=g, device=dev) / k ** 0.5).to(T).float()

    def v(n, one=False):
        r = torch.randn(n, generator=g, device=dev)
        return 1.0 + 0.1 * r if one else 0.05 * r
    return dict(ln1_w=v(C, True), ln1_b=v(C), qkv_w=w(3 * C, C), qkv_b=v(3 * C), proj_w=w(C, C), proj_b=v(C),
                table=torch.randn(169, C // 32, generator=g, device=dev) / (C // 32) ** 0.5,
                ln2_w=v(C, True), ln2_b=v(C), fc1_w=w(4 * C, C), fc1_b=v(4 * C), fc2_w=w(C, 4 * C), fc2_b=v(C))


def part_ref(prec, x64, p, rows, rounded, mlp, xn=None, post=None):
    """-> dict(x, xn2, post, acc).  rounded: R~ (a round-to-type wherever the kernel writes a 16-bit image)."""
    r = _rnd(prec) if rounded else (lambda t: t)
    d = {k: t.double() for k, t in p.items()}
    C = x64.shape[1]
    if xn is None:
        xn = r(_ln(x64, d["ln1_w"], d["ln1_b"]))
    qkv = r(xn @ d["qkv_w"].t() + d["qkv_b"])
    o = r(attn_ref(qkv, d["table"], rows, C // 32, rnd=r)[0])
    x1 = x64 + o @ d["proj_w"].t() + d["proj_b"]
    acc = EPS * C * (o.abs() @ d["proj_w"].abs().t())
    res = dict(xn2=r(_ln(x1, d["ln2_w"], d["ln2_b"])))
    if mlp:
        hid = r(GP.gelu_poly(res["xn2"] @ d["fc1_w"].t() + d["fc1_b"], GP.GELU_DEG[prec]))
        x1 = x1 + hid @ d["fc2_w"].t() + d["fc2_b"]
        acc = acc + EPS * 4 * C * (hid.abs() @ d["fc2_w"].abs().t())
    res["x"] = x1
    res["acc"] = (acc + 4 * EPS * x1.abs()).max().item()
    if post is not None:
        res["post"] = r(x1 * post[0].double() + post[1].double())
    return res


def _judge(tag, out, R, Rt, key, acc, stats, upd=None):
    """max |out - R| <= 2 E + acc with E = max |R~ - R|; with upd (the block's update R - x) also 2 E <= 0.1 rms."""
    E = (Rt[key] - R[key]).abs().max().item()
    err = (out.double() - R[key]).abs().max().item()
    ratio = err / E if E > 0 else float("inf")
    stats.append((tag + "." + key, E, ratio))
    print(f"  {tag}.{key}: E = {E:.3e}, err = {err:.3e}, err / E = {ratio:.3f}" +
          (f", 2E / rms(update) = {2 * E / upd:.3f}" if upd is not None else ""))
    if upd is not None:
        assert 2 * E <= 0.1 * upd, f"{tag}: the budget 2E = {2 * E:.3e} is not small against the update's rms {upd:.3e}"
    assert err <= 2 * E + acc, f"{tag}.{key}: err {err:.4e} > 2 E + acc = {2 * E + acc:.4e} (E {E:.4e})"


def _run_part(cuda, prec, C, B, H, grid, variants, seed):
    T = DT[prec]
    N = B * H * H
    g = torch.Generator(device=cuda).manual_seed(seed)
    p = part_params(C, prec, g, cuda)
    x = torch.randn(N, C, generator=g, device=cuda)
    post = (1.0 + 0.1 * torch.randn(C, generator=g, device=cuda), 0.1 * torch.randn(C, generator=g, device=cuda))
    rows = part_rows(B, H, grid, cuda)
    x64 = x.double()
    stats = []
    for name in variants:
        mlp = name != "attn"
        po = post if name == "post" else None
        R = part_ref(prec, x64, p, rows, False, mlp, post=po)
        Rt = part_ref(prec, x64, p, rows, True, mlp, post=po)
        xbuf, xio = _guarded(N * C, torch.float32, cuda, fill=x)
        pbuf, pout = _guarded(N * C, T, cuda) if po is not None else (None, None)
        ops.mv_part(xio.view(N, C), p, B, H, grid, precision=prec, mlp=mlp, post=po,
                    post_out=pout.view(N, C) if po is not None else None)
        tag = f"part {prec} C={C} H={H} B={B} grid={grid} {name}"
        upd = (R["x"] - x64).pow(2).mean().sqrt().item()
        _judge(tag, xio.view(N, C), R, Rt, "x", R["acc"], stats, upd)
        assert _intact(xbuf, N * C), f"{tag}: x's guard bytes changed"
        if po is not None:
            _judge(tag, pout.view(N, C), R, Rt, "post", 1.2 * R["acc"], stats)
            assert _intact(pbuf, N * C), f"{tag}: post_out's guard bytes changed"
    return stats


@pytest.mark.parametrize("grid", [0, 1], ids=["window", "grid"])
@pytest.mark.parametrize("H", [7, 14, 21])
@pytest.mark.parametrize("C", [64, 128, 256])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_part_against_float64(cuda, prec, C, H, grid):
    """mv_part: the attention half alone, with the MLP half, and with post_out."""
    _run_part(cuda, prec, C, 3, H, grid, ("attn", "mlp", "post"), C + H + grid)


@pytest.mark.parametrize("C,bh", [(64, WALK_PART64), (256, WALK_PART256)], ids=["C64-576units", "C256-260units"])
def test_part_workgroups_walk_units(cuda, C, bh):
    """Persistent workgroups that take a second unit, with a ragged remainder (test_walking_arithmetic)."""
    _run_part(cuda, "bf16", C, bh[0], bh[1], 0, ("post",), C)


def _run_ablk(cuda, prec, B, H, grid, seed):
    T, C = DT[prec], 64
    N = B * H * H
    g = torch.Generator(device=cuda).manual_seed(seed)
    p = part_params(C, prec, g, cuda)
    x = torch.randn(N, C, generator=g, device=cuda)
    x64 = x.double()
    xn = _ln(x64, p["ln1_w"].double(), p["ln1_b"].double()).to(T)          # the producer's LN1 image, exact in T
    rows = part_rows(B, H, grid, cuda)
    R = part_ref(prec, x64, p, rows, False, False, xn=xn.double())
    Rt = part_ref(prec, x64, p, rows, True, False, xn=xn.double())
    pk = {k: p[k] for k in ("qkv_w", "qkv_b", "proj_w", "proj_b", "table", "ln2_w", "ln2_b")}
    tag = f"attn_block {prec} H={H} B={B} grid={grid}"
    upd = (R["x"] - x64).pow(2).mean().sqrt().item()
    stats = []
    for alias in (False, True):
        xbuf, xio = _guarded(N * C, torch.float32, cuda, fill=x)
        nbuf, xn_in = _guarded(N * C, T, cuda, fill=xn)
        obuf, xn2 = (nbuf, xn_in) if alias else _guarded(N * C, T, cuda)
        ops.mv_attn_block(xn_in.view(N, C), xio.view(N, C), pk, B, H, grid, precision=prec, xn2=xn2.view(N, C))
        t = tag + (" in place" if alias else "")
        _judge(t, xio.view(N, C), R, Rt, "x", R["acc"], stats, upd)
        # LayerNorm's slope: rstd * |w| of the fp32 sums' error, far below one rounding of the output
        _judge(t, xn2.view(N, C), R, Rt, "xn2", 8 * R["acc"], stats)
        assert _intact(xbuf, N * C) and _intact(nbuf, N * C) and _intact(obuf, N * C), f"{t}: guard bytes changed"
        if not alias:
            assert torch.equal(xn_in.view(N, C), xn), f"{t}: xn was written"
    return stats


@pytest.mark.parametrize("grid", [0, 1], ids=["window", "grid"])
@pytest.mark.parametrize("H", [7, 14, 21])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_attn_block_against_float64(cuda, prec, H, grid):
    """mv_attn_block64: x and xn2, with xn2 in a buffer of its own and aliasing xn."""
    _run_ablk(cuda, prec, 3, H, grid, H + grid)


def test_attn_block_workgroups_walk_units(cuda):
    _run_ablk(cuda, "bf16", WALK_ABLK[0], WALK_ABLK[1], 0, 3)


# ---- the index-map probes through the fused kernels: filters that make the kernel an attention over its own input
def _probe_filters(C, dev):
    """qkv filter whose q and k rows are 0 and whose v rows copy the input's channels ([head][q|k|v][32]:
    V[head][d] = xn[32 head + d]), proj = identity, zero biases: x_out - x is then the attention output itself."""
    heads = C // 32
    qkv_w = torch.zeros(heads, 96, C, device=dev)
    for h in range(heads):
        qkv_w[h, 64:, 32 * h:32 * h + 32] = torch.eye(32, device=dev)
    return dict(qkv_w=qkv_w.view(3 * C, C).contiguous(), qkv_b=torch.zeros(3 * C, device=dev),
                proj_w=torch.eye(C, device=dev).contiguous(), proj_b=torch.zeros(C, device=dev))


def _fused_probe(what, prec, out, x64, v64, table, rows, rounded_p, worst):
    """out (fp32) against x + attention(q = k = 0, V = v64): the kernel rounds O to the type before the identity proj
    (u |O|), the unnormalised P as well where the table is not zero (u_P, SUB_P); one fp32 add into the residual."""
    N, C = v64.shape
    heads = C // 32
    qkv = torch.zeros(N, heads, 96, dtype=torch.float64, device=v64.device)
    qkv[..., 64:] = v64.view(N, heads, 32)
    o, a, delta, vsum = attn_ref(qkv.view(N, 3 * C), table.double(), rows, heads)
    e = (torch.expm1(2 * delta) + (U[prec] if rounded_p else 0.0) + 121 * EPS) * a + (SUB[prec] if rounded_p else 0.0) * vsum
    bound = (1 + U[prec]) * e + U[prec] * o.abs() + SUB[prec] + 2 * EPS * out.double().abs()
    _check(what, out, x64 + o, bound, worst)


def _probe_tables(C, g, dev):
    return (("probe1", torch.zeros(169, C // 32, device=dev), False),
            ("probe2", torch.randn(169, C // 32, generator=g, device=dev), True))


@pytest.mark.parametrize("grid", [0, 1], ids=["window", "grid"])
@pytest.mark.parametrize("H", [7, 14, 21])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_attn_block_index_map_probes(cuda, prec, H, grid):
    """mv_attn_block64's own index map (row_of, the padded key tile, the bias image in registers): xn holds integers in
    [-120, 120], x small integers; probe 1 must add the partition mean of xn to x, probe 2 softmax(bias) @ xn."""
    B, C, T = 3, 64, DT[prec]
    N = B * H * H
    g = torch.Generator(device=cuda).manual_seed(H * 10 + grid + 1)
    xn = torch.randint(-120, 121, (N, C), generator=g, device=cuda).to(T)
    x = torch.randint(-8, 9, (N, C), generator=g, device=cuda).float()
    rows = part_rows(B, H, grid, cuda)
    p = _probe_filters(C, cuda)
    p.update(ln2_w=torch.ones(C, device=cuda), ln2_b=torch.zeros(C, device=cuda))
    worst = {}
    for name, table, rp in _probe_tables(C, g, cuda):
        p["table"] = table
        xbuf, xio = _guarded(N * C, torch.float32, cuda, fill=x)
        ops.mv_attn_block(xn, xio.view(N, C), p, B, H, grid, precision=prec)
        _fused_probe(name, prec, xio.view(N, C), x.double(), xn.double(), table, rows, rp, worst)
        assert _intact(xbuf, N * C), f"{name}: guard bytes changed"
    print(f"[attn_block probes {prec} H={H} grid={grid}] err/bound " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("grid", [0, 1], ids=["window", "grid"])
@pytest.mark.parametrize("H", [7, 14, 21])
@pytest.mark.parametrize("C", [64, 128, 256])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_part_index_map_probes(cuda, prec, C, H, grid):
    """mv_part's attention half (row map, lane-ordered bias image of mv_pack_relbias_lanes, key mask).  The kernel
    normalises x itself, so x is built for an exact LN1 image: every row holds C/2 entries +a and C/2 entries -a
    (a in {1, 2, 3} per row, signs shuffled per row), hence mean 0, variance a^2 and LN(x) = +-(1 - 5e-7 / a^2), and
    norm1.weight holds integers 1..11 per channel: T(LN1(x)) = sign * weight exactly in fp32 and in float64 alike
    (1e-6 from a value of the type, against a rounding tie 2^-9 / 2^-12 away)."""
    B = 3
    N = B * H * H
    g = torch.Generator(device=cuda).manual_seed(C + H * 10 + grid)
    order = torch.rand(N, C, generator=g, device=cuda).argsort(1).argsort(1)
    sign = torch.where(order < C // 2, 1.0, -1.0)
    x = sign * torch.randint(1, 4, (N, 1), generator=g, device=cuda).float()
    w1 = (1 + (torch.arange(C, device=cuda) * 5) % 11).float()
    v64 = (sign * w1).double()
    assert torch.equal(_rnd(prec)(_ln(x.double(), w1.double(), 0.0)), v64)       # (the exact LN1 image, in float64)
    rows = part_rows(B, H, grid, cuda)
    p = _probe_filters(C, cuda)
    p.update(ln1_w=w1, ln1_b=torch.zeros(C, device=cuda))
    worst = {}
    for name, table, rp in _probe_tables(C, g, cuda):
        p["table"] = table
        xbuf, xio = _guarded(N * C, torch.float32, cuda, fill=x)
        ops.mv_part(xio.view(N, C), p, B, H, grid, precision=prec, mlp=False)
        _fused_probe(name, prec, xio.view(N, C), x.double(), v64, table, rows, rp, worst)
        assert _intact(xbuf, N * C), f"{name}: guard bytes changed"
    print(f"[part probes {prec} C={C} H={H} grid={grid}] err/bound " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


# ---- MBConv pieces
def _border_map(B, H, C, prec, g, dev, width=1):
    x = torch.randn(B, H, H, C, generator=g, device=dev)
    m = torch.ones(H, device=dev)
    m[:width] = 8.0
    m[H - width:] = 8.0
    return (x * torch.maximum(m[:, None], m[None, :])[None, :, :, None]).to(DT[prec])


def dw3_ref(x64, w9, bias, stride):
    """NHWC float64 depthwise 3x3 p1: -> (pre-activation, sum |v| |w|); w9 [3][3][C]."""
    B, H, _, C = x64.shape
    Ho = H // stride
    xp = F.pad(x64, (0, 0, 1, 1, 1, 1))
    acc = bias.expand(B, Ho, Ho, C).clone()
    mag = bias.abs().expand(B, Ho, Ho, C).clone()
    for ky in range(3):
        for kx in range(3):
            v = xp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Ho:stride, :]
            acc += v * w9[ky, kx]
            mag += v.abs() * w9[ky, kx].abs()
    return acc, mag


def _silu64(t):
    return t * torch.sigmoid(t)


def _dw_params(C, g, dev):
    w = torch.randn(C, 1, 3, 3, generator=g, device=dev) / 3.0
    scale = 1.0 + 0.1 * torch.randn(C, generator=g, device=dev)
    bias = 0.1 * torch.randn(C, generator=g, device=dev)
    w9 = (w.double() * scale.double()[:, None, None, None]).view(C, 3, 3).permute(1, 2, 0).contiguous()
    return w, scale, bias, w9


def _check_part(tag, part, stored, HW, worst):
    """sum over the groups of part [B][groups][C] against the float64 sum of the stored (rounded) map [B][HW][C]."""
    assert bool(torch.isfinite(part).all()), f"{tag}: a group slot of part was not written"
    s = stored.double()
    _check(tag, part.double().sum(1), s.sum(1), HW * EPS * s.abs().sum(1) + 1e-30, worst)


DW3 = [(p, h, c, s) for p in ("f32", "bf16", "f16") for h, c in ((14, 64), (28, 256)) for s in (1, 2)]
DW3S = [(p, h, c, s) for p in ("bf16", "f16") for h, c, s in ((7, 512, 1), (14, 256, 1), (28, 2048, 1), (28, 2048, 2),
                                                                (14, 256, 2), (14, 512, 2))]


@pytest.mark.parametrize("prec,H,C,stride", DW3, ids=[f"{p}-H{h}-C{c}-s{s}" for p, h, c, s in DW3])
def test_dw3_against_float64(cuda, prec, H, C, stride):
    _run_dw3(cuda, 0, prec, H, C, stride)


@pytest.mark.parametrize("prec,H,C,stride", DW3S, ids=[f"{p}-H{h}-C{c}-s{s}" for p, h, c, s in DW3S])
def test_dw3s_against_float64(cuda, prec, H, C, stride):
    """C / 8 below 256 (PL = 4, 8 strips per workgroup), dividing it and equal to it; stride 2 from H = 14 leaves one
    strip per row, with groups that are not full."""
    _run_dw3(cuda, 1, prec, H, C, stride)


def _run_dw3(cuda, impl, prec, H, C, stride):
    B, Ho = 3, H // stride
    g = torch.Generator(device=cuda).manual_seed(H + C + stride)
    x = _border_map(B, H, C, prec, g, cuda)
    w, scale, bias, w9 = _dw_params(C, g, cuda)
    pre, mag = dw3_ref(x.double(), w9, bias.double(), stride)
    ref = _silu64(pre)
    n = B * Ho * Ho * C
    obuf, out = _guarded(n, DT[prec], cuda)
    worst = {}
    pbuf = None
    if impl == 1:
        groups = ops.mv_dw3_groups(H, C, stride)
        pbuf, part = _guarded(B * groups * C, torch.float32, cuda)
        part.fill_(float("nan"))
        ops.mv_dw3(x, w, scale, bias, stride, impl=1, precision=prec, out=out, part=part)
    else:
        ops.mv_dw3(x, w, scale, bias, stride, impl=0, precision=prec, out=out)
    out = out.view(B, Ho, Ho, C)
    e = 11 * EPS * mag
    bound = U[prec] * out.double().abs() + SUB[prec] + L_SILU * e + SILU_REL * (ref.abs() + L_SILU * e)
    _check("out", out, ref, bound, worst)
    assert _intact(obuf, n), "out: guard bytes changed"
    if impl == 1:
        _check_part("part", part.view(B, groups, C), out.reshape(B, Ho * Ho, C), Ho * Ho, worst)
        assert _intact(pbuf, B * groups * C), "part: guard bytes changed"
    print(f"[dw3 impl{impl} {prec} H={H} C={C} s={stride}] err/bound " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("H,stride", [(56, 2), (28, 1)], ids=["H56-s2-16tiles", "H28-s1-4tiles"])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_mbconv_front_against_float64(cuda, prec, H, stride):
    B, CIN, MID, Ho = 2, 64, 256, H // stride
    T = DT[prec]
    r = _rnd(prec)
    g = torch.Generator(device=cuda).manual_seed(H + stride)
    xn = torch.randn(B, H, H, CIN, generator=g, device=cuda).to(T)
    w1 = (torch.randn(MID, CIN, generator=g, device=cuda) / CIN ** 0.5).to(T).float()
    b1 = 0.1 * torch.randn(MID, generator=g, device=cuda)
    dw, scale, b2, w9 = _dw_params(MID, g, cuda)
    m1 = _silu64(xn.double() @ w1.double().t() + b1.double())
    R, mag = dw3_ref(m1, w9, b2.double(), stride)
    R = _silu64(R)
    Rt = _silu64(dw3_ref(r(m1), w9, b2.double(), stride)[0])
    E = (Rt - R).abs().max().item()
    tiles = ops.mv_mbconv_front_tiles(H, stride)
    assert tiles == (16 if stride == 2 else 4)
    n = B * Ho * Ho * MID
    obuf, m2 = _guarded(n, T, cuda)
    pbuf, part = _guarded(B * tiles * MID, torch.float32, cuda)
    part.fill_(float("nan"))
    ops.mv_mbconv_front(xn, w1, b1, dw, scale, b2, stride, precision=prec, m2=m2, part=part)
    m2 = m2.view(B, Ho, Ho, MID)
    worst = {}
    bound = 2 * E + U[prec] * m2.double().abs() + SUB[prec] + 16 * EPS * mag + SILU_REL * R.abs()
    err = (m2.double() - R).abs().max().item()
    _check("m2", m2, R, bound, worst)
    _check_part("part", part.view(B, tiles, MID), m2.reshape(B, Ho * Ho, MID), Ho * Ho, worst)
    assert _intact(obuf, n) and _intact(pbuf, B * tiles * MID), "guard bytes changed"
    print(f"[mbconv_front {prec} H={H} s={stride}] E = {E:.3e}, err = {err:.3e}, err / E = {err / E:.3f}, "
          f"2E / rms(R) = {2 * E / R.pow(2).mean().sqrt().item():.3f}; err/bound " +
          " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("C", [256, 2048])
@pytest.mark.parametrize("form", ["bf16", "f16", "f32-partials"])
def test_se_against_float64(cuda, form, C, B):
    """Both input forms: a 16-bit map of 49 pixels, and fp32 rows of partial sums (7 groups); B on both sides of SE_AG."""
    prec = form.split("-")[0]
    RD, HW = C // 16, (49 if prec != "f32" else 7)
    g = torch.Generator(device=cuda).manual_seed(C + B)
    y = torch.randn(B, HW, C, generator=g, device=cuda)
    y = (y * 7.0 if prec == "f32" else y).to(DT[prec])
    w1 = torch.randn(RD, C, generator=g, device=cuda) / C ** 0.5
    b1 = 0.1 * torch.randn(RD, generator=g, device=cuda)
    w2 = torch.randn(C, RD, generator=g, device=cuda) / RD ** 0.5
    b2 = 0.1 * torch.randn(C, generator=g, device=cuda)
    inv = 1.0 / 49.0
    gbuf, gate = _guarded(B * C, torch.float32, cuda)
    ops.mv_se(y, w1.view(RD, C, 1, 1), b1, w2.view(C, RD, 1, 1), b2, inv, precision=prec, gate=gate.view(B, C))
    y64, w164, w264 = y.double(), w1.double(), w2.double()
    inv32 = float(torch.tensor(inv, dtype=torch.float32))
    mean = inv32 * y64.sum(1)
    e_m = (HW + 1) * EPS * inv32 * y64.abs().sum(1)
    p1 = mean @ w164.t() + b1.double()
    e1 = (C + 2) * EPS * (mean.abs() @ w164.abs().t() + b1.double().abs()) + e_m @ w164.abs().t()
    s = _silu64(p1)
    e_s = L_SILU * e1 + SILU_REL * (s.abs() + L_SILU * e1)
    p2 = s @ w264.t() + b2.double()
    e2 = (RD + 2) * EPS * (s.abs() @ w264.abs().t() + b2.double().abs()) + e_s @ w264.abs().t()
    ref = torch.sigmoid(p2)
    worst = {}
    _check("gate", gate.view(B, C), ref, 0.25 * e2 + SILU_REL * ref, worst)
    assert _intact(gbuf, B * C), "gate: guard bytes changed"
    print(f"[se {form} C={C} B={B}] err/bound {worst['gate']:.3g}")


def _conv3_nhwc(x64, w64, stride):
    """3x3 p1 convolution in float64 as im2col + matmul: x [B,C,H,H], w [O,C,3,3] -> [B,Ho,Ho,O]."""
    B, Cc, H, _ = x64.shape
    Ho = H // stride
    cols = F.unfold(x64, 3, padding=1, stride=stride)               # [B, C*9, Ho*Ho]
    return (cols.transpose(1, 2) @ w64.reshape(w64.shape[0], -1).t()).view(B, Ho, Ho, -1)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_stem_against_float64(cuda, prec):
    """The full map, the pooled form and the map with xn, each against bilinear 63 -> 224 (align_corners = False),
    conv 3x3 s2 + BN + SiLU, conv 3x3 s1 in float64.  The BatchNorm scale is a power of two, so that the packed filter
    conv1_w * scale is exact in the type.  The outermost two rows and columns of the image are 8x larger."""
    B, T = 2, DT[prec]
    r = _rnd(prec)
    g = torch.Generator(device=cuda).manual_seed(11)
    img = torch.randn(B, 3, 63, 63, generator=g, device=cuda)
    m = torch.ones(63, device=cuda)
    m[:2] = 8.0
    m[61:] = 8.0
    img = (img * torch.maximum(m[:, None], m[None, :])).contiguous()
    w1 = (torch.randn(32, 3, 3, 3, generator=g, device=cuda) / 27 ** 0.5).to(T).float()
    bn_s = torch.tensor([0.5, 1.0, 2.0, 1.0], device=cuda).repeat(8)
    bn_t = 0.1 * torch.randn(32, generator=g, device=cuda)
    w2 = (torch.randn(64, 32, 3, 3, generator=g, device=cuda) / 288 ** 0.5).to(T).float()
    pre = (1.0 + 0.1 * torch.randn(64, generator=g, device=cuda), 0.1 * torch.randn(64, generator=g, device=cuda))
    w1s = w1.double() * bn_s.double()[:, None, None, None]

    def ref(rr):
        big = rr(F.interpolate(img.double(), size=(224, 224), mode="bilinear", align_corners=False))
        mid = rr(_silu64(_conv3_nhwc(big, w1s, 2) + bn_t.double()))
        full = _conv3_nhwc(mid.permute(0, 3, 1, 2).contiguous(), w2.double(), 1)
        acc = 288 * EPS * _conv3_nhwc(mid.abs().permute(0, 3, 1, 2).contiguous(), w2.double().abs(), 1) + 4 * EPS * full.abs()
        return dict(full=full, pooled=F.avg_pool2d(full.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1),
                    xn=rr(full * pre[0].double() + pre[1].double()), acc=acc.max().item())
    R, Rt = ref(lambda t: t), ref(r)
    stats = []
    tag = f"stem {prec}"
    n = B * 12544 * 64
    for variant in ("full", "pooled", "xn"):
        pooled = variant == "pooled"
        no = n // 4 if pooled else n
        obuf, out = _guarded(no, torch.float32, cuda)
        xbuf, xn = _guarded(n, T, cuda) if variant == "xn" else (None, None)
        ops.mv_stem(img, w1, bn_s, bn_t, w2, precision=prec, pooled=pooled, pre=pre if variant == "xn" else None,
                    out=out, xn=xn)
        _judge(f"{tag} {variant}", out.view(R["pooled" if pooled else "full"].shape), R, Rt,
               "pooled" if pooled else "full", R["acc"], stats)
        assert _intact(obuf, no), f"{variant}: out's guard bytes changed"
        if variant == "xn":
            _judge(f"{tag} {variant}", xn.view(B, 112, 112, 64), R, Rt, "xn", 1.2 * R["acc"], stats)
            assert _intact(xbuf, n), "xn's guard bytes changed"


# ---- refusals: argument checks only, nothing reaches a kernel
def _refused(match, fn, *a, **k):
    with pytest.raises(_lib.BtsbotHipError, match=match):
        fn(*a, **k)


def test_attn_refusals(cuda):
    q = torch.zeros(49 * 2, 192, dtype=torch.bfloat16, device=cuda)
    t = torch.zeros(169, 2, device=cuda)
    L, st = _lib.lib(), ops._stream(q)
    P = GP._p
    assert L.btsbot_op_mv_attn(1, 0, None, P(t), P(q), 2, 7, 64, 0, st) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_attn(1, 0, P(q), None, P(q), 2, 7, 64, 0, st) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_attn(1, 0, P(q), P(t), None, 2, 7, 64, 0, st) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_attn(1, 0, P(q), P(t), P(q), 2, 8, 64, 0, st) == _lib.ERR_INVALID_ARG     # H
    assert L.btsbot_op_mv_attn(1, 0, P(q), P(t), P(q), 2, 7, 48, 0, st) == _lib.ERR_INVALID_ARG     # C
    assert L.btsbot_op_mv_attn(1, 2, P(q), P(t), P(q), 2, 7, 64, 0, st) == _lib.ERR_INVALID_ARG     # impl
    assert L.btsbot_op_mv_attn(0, 1, P(q), P(t), P(q), 2, 7, 64, 0, st) == _lib.ERR_INVALID_ARG     # fp32 on the MFMA
    assert L.btsbot_op_mv_attn(3, 0, P(q), P(t), P(q), 2, 7, 64, 0, st) == _lib.ERR_INVALID_ARG     # fp8
    assert b"precision" in L.btsbot_last_error()


def test_attn_block_refusals(cuda):
    L = _lib.lib()
    P = GP._p
    z = torch.zeros(192 * 64, device=cuda)
    st = ops._stream(z)
    a = [P(z)] * 10
    for i in range(10):
        b = list(a)
        b[i] = None
        assert L.btsbot_op_mv_attn_block(1, *b, 1, 7, 0, st) == _lib.ERR_INVALID_ARG, i
    assert L.btsbot_op_mv_attn_block(1, *a, 1, 10, 0, st) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_attn_block(0, *a, 1, 7, 0, st) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_attn_block(1, *a, 1, 7, 2, st) == _lib.ERR_INVALID_ARG


def test_part_refusals(cuda):
    L = _lib.lib()
    P = GP._p
    z = torch.zeros(4 * 64 * 64, device=cuda)
    st = ops._stream(z)
    a = [P(z)] * 17
    tail = (1, 7, 64, 0, st)
    for i in range(8):
        b = list(a)
        b[i] = None
        assert L.btsbot_op_mv_part(1, *b, *tail) == _lib.ERR_INVALID_ARG, i
    b = list(a)
    b[10] = None                                                     # half an MLP
    assert L.btsbot_op_mv_part(1, *b, *tail) == _lib.ERR_INVALID_ARG
    b = list(a)
    b[14] = None                                                     # post_out without post_s
    assert L.btsbot_op_mv_part(1, *b, *tail) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_part(1, *a, 1, 9, 64, 0, st) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_part(1, *a, 1, 7, 512, 0, st) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_part(1, *a, 1, 7, 96, 0, st) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_part(0, *a, 1, 7, 64, 0, st) == _lib.ERR_INVALID_ARG
    assert b"unsupported" in L.btsbot_last_error()


def test_dw3_refusals(cuda):
    x = torch.zeros(1, 14, 14, 64, dtype=torch.float16, device=cuda)
    w, s, b = torch.zeros(64, 1, 3, 3, device=cuda), torch.ones(64, device=cuda), torch.zeros(64, device=cuda)
    _refused("null", ops.mv_dw3, x, w, None, b, 1, precision="f16")
    _refused("bad shape", ops.mv_dw3, x, w, s, b, 3, precision="f16")
    _refused("precision", ops.mv_dw3, x.float(), w, s, b, 1, impl=1, precision="f32",
             part=torch.zeros(1, 14, 64, device=cuda))
    x12 = torch.zeros(1, 12, 12, 64, dtype=torch.float16, device=cuda)
    _refused("cannot run", ops.mv_dw3, x12, w, s, b, 1, impl=1, precision="f16", part=torch.zeros(1, 99, 64, device=cuda))
    L = _lib.lib()
    assert L.btsbot_op_mv_dw3_groups(12, 64, 1) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_dw3_groups(14, 60, 1) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_dw3(2, 1, GP._p(x), GP._p(w), GP._p(s), GP._p(b), GP._p(x), None, 1, 14, 64, 1,
                              ops._stream(x)) == _lib.ERR_INVALID_ARG   # impl 1 without part
    # 40 channel groups do not divide 256: what launch_mv_dw3s itself refuses
    x320 = torch.zeros(1, 7, 7, 320, dtype=torch.float16, device=cuda)
    _refused("mv_dw3s: bad shape", ops.mv_dw3, x320, torch.zeros(320, 1, 3, 3, device=cuda), torch.ones(320, device=cuda),
             torch.zeros(320, device=cuda), 1, impl=1, precision="f16", part=torch.zeros(1, 8, 320, device=cuda))


def test_mbconv_front_refusals(cuda):
    def call(prec, H, CIN, stride):
        xn = torch.zeros(1, H, H, CIN, dtype=DT[prec], device=cuda)
        z = torch.zeros(256, device=cuda)
        return ops.mv_mbconv_front(xn, torch.zeros(256, CIN, device=cuda), z, torch.zeros(256, 1, 3, 3, device=cuda), z, z,
                                   stride, precision=prec, m2=torch.zeros(1, H, H, 256, dtype=DT[prec], device=cuda),
                                   part=torch.zeros(1, 64, 256, device=cuda))
    _refused("unsupported", call, "bf16", 28, 128, 1)      # CIN = 128
    _refused("unsupported", call, "bf16", 28, 64, 2)       # Ho = 14 < 28
    _refused("unsupported", call, "bf16", 14, 64, 1)
    _refused("unsupported", call, "f32", 28, 64, 1)
    L = _lib.lib()
    assert L.btsbot_op_mv_mbconv_front_tiles(30, 1) == _lib.ERR_INVALID_ARG
    z = torch.zeros(8, device=cuda)
    a = [GP._p(z)] * 8
    for i in range(8):
        b = list(a)
        b[i] = None
        assert L.btsbot_op_mv_mbconv_front(1, *b, 1, 28, 64, 256, 1, ops._stream(z)) == _lib.ERR_INVALID_ARG, i


def test_se_refusals(cuda):
    y = torch.zeros(1, 4, 64, dtype=torch.float16, device=cuda)
    w1, b1, w2, b2 = (torch.zeros(4, 64, device=cuda), torch.zeros(4, device=cuda), torch.zeros(64, 4, device=cuda),
                      torch.zeros(64, device=cuda))
    _refused("null", ops.mv_se, y, w1, None, w2, b2, 0.25, precision="f16")
    L, P = _lib.lib(), GP._p
    st = ops._stream(y)
    assert L.btsbot_op_mv_se(2, P(y), P(w1), P(b1), P(w2), P(b2), P(b2), 1, 4, 62, 4, 0.25, st) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_se(2, P(y), P(w1), P(b1), P(w2), P(b2), P(b2), 1, 4, 64, 0, 0.25, st) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_se(2, P(y), P(w1), P(b1), P(w2), P(b2), P(b2), 1, 4, 64, 513, 0.25, st) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_se(4, P(y), P(w1), P(b1), P(w2), P(b2), P(b2), 1, 4, 64, 4, 0.25, st) == _lib.ERR_INVALID_ARG
    assert L.btsbot_op_mv_se(2, P(y), P(w1), P(b1), P(w2), P(b2), None, 1, 4, 64, 4, 0.25, st) == _lib.ERR_INVALID_ARG


def test_stem_refusals(cuda):
    z = torch.zeros(64 * 288, device=cuda)
    L, P = _lib.lib(), GP._p
    st = ops._stream(z)
    good = [P(z)] * 6
    assert L.btsbot_op_mv_stem(0, *good, 0, None, None, None, 1, st) == _lib.ERR_INVALID_ARG           # fp32
    assert L.btsbot_op_mv_stem(1, *good, 2, None, None, None, 1, st) == _lib.ERR_INVALID_ARG           # pooled flag
    assert L.btsbot_op_mv_stem(1, *good, 0, P(z), None, P(z), 1, st) == _lib.ERR_INVALID_ARG           # xn without scale
    for i in range(6):
        b = list(good)
        b[i] = None
        assert L.btsbot_op_mv_stem(1, *b, 0, None, None, None, 1, st) == _lib.ERR_INVALID_ARG, i
