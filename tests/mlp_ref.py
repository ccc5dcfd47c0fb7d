"""Float64 references, per-element bounds, emulations and seeded faults for the MLP half of the ConvNeXt 16-bit training
step, one kernel at a time (btsbot_op_cnt_mlp_bwd / s2mlp_bwd / fused_mlp / fc2_grads, btsbot_amd/csrc/cn_mlp_ops.hip).

Inputs are exact values of BOTH operand types (exact(): bf16 values of at least f16's smallest normal), so one float64
reference per case serves both precisions up to the GELU polynomial (degree 3 for bf16, 5 for f16: gelu_ref.py).  The
reference applies no intermediate rounding.  What a kernel may differ by is derived per element, in the style of
test_gpu_gemm_paths.py's docstring, from what it legitimately does and nothing fitted:

  acc(n, S)   fp32 accumulation of n terms whose absolute values sum to S:  n 2^-24 S
  r16(v, dv)  ONE rounding to the operand type of a value v known to dv:    u (|v| + dv) + sub     (u = 2^-8 / 2^-11,
              sub = 2^-25 for f16's subnormals) -- for the values a kernel keeps on chip in 16 bit: g and da in mlp_bwd
              (mlp_bwd.hip: M::cvt in gelu()), da in s2mlp_bwd (s2mlp_bwd.hip: `dv[r] = (T)(...)`), g in fused_mlp
              (fused_mlp.hip: `hf[..] = (T)v`), each propagated through the absolute values of the product that follows
  gelu        its fp32 evaluation error (gelu_ref._gelu_f) + L_GELU x the pre-activation's error
  gelu'       its fp32 evaluation error (_gelu_grad_f) + L2_GELU x the pre-activation's error da, + the jump of
              gelu_poly_grad at 0, |1 - 2^(1 + c0)|, where |a| <= da.  L2_GELU bounds the slope of gelu' on each smooth
              branch (erf GELU: 2 phi(0) = 0.798; test_mlp_ops_reference.py checks both fits on a grid)
  db1         sums the fp32 da before its rounding (mlp_bwd.hip: `sb1 += da`)
  "+=" outputs add one rounding at |pre-fill| + |result|.

Chain lengths come from the launcher's own figures (slices = workgroups along the rows, tiles = ceil(R / 64)): G, dW1 and
S pass 64 ceil(tiles / slices) rows through one workgroup's fp32 accumulators and `slices` partials through the
reduction; db1 likewise (its 64 rows of a tile are summed 32 + 32 per lane, then across two lanes).
"""
import math

import torch

from gelu_ref import EPS, GELU_DEG, GELU_Q, L_GELU, SUB, U, _gelu, _gelu_f, _gelu_grad, _gelu_grad_f

F64 = torch.float64
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
PRECS = ("bf16", "f16")
L2_GELU = 0.82                        # slope of gelu' on a smooth branch: 2 phi(0) = 0.798 for erf; the fits: <= 0.81
F16_MIN_NORMAL = 2.0 ** -14


def exact(t):
    """the nearest tensor whose values are exact in bf16 AND f16 (fp32 storage)"""
    v = t.to(torch.bfloat16).float()
    v = torch.where(v.abs() < F16_MIN_NORMAL, torch.zeros_like(v), v)
    assert torch.equal(v.half().float(), v) and torch.equal(v.bfloat16().float(), v)
    return v


def gelu_jump(prec):
    return abs(1.0 - 2.0 ** (1.0 + GELU_Q[GELU_DEG[prec]][0]))


def acc(n, S):
    return n * EPS * S


def r16(prec, v, dv):
    return U[prec] * (v.abs() + dv) + SUB[prec]


def rnd(prec, v):
    """v (float64) rounded once to the operand type"""
    return v.to(DT[prec]).to(F64)


def gelu_grad_err(prec, a, da):
    return _gelu_grad_f(prec, a) + L2_GELU * da + gelu_jump(prec) * (a.abs() <= da).to(F64)


def ratio(got, ref, bound):
    """worst |got - ref| / bound (an exact zero is within a zero bound)"""
    err = (got.to(F64).reshape(ref.shape) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return r.max().item() if r.numel() else 0.0


def worst(got, ref, bound):
    return {k: ratio(got[k], ref[k], bound[k]) for k in ref}


# ---------------------------------------------------------------------------------------------------------------------
# mlp_bwd: xn, dy [R][C], w1 [4C][C], w2g = (diag(gamma) W2)^T [4C][C], b1 [4C]; pre-fills G0, S0, dW0, db0
# ---------------------------------------------------------------------------------------------------------------------
def mlp_bwd_inputs(C, R, seed, live_rows=None, dev="cpu"):
    """The issue's scales.  live_rows (optional): dy is zero outside these rows (the spotlight of the large cases)."""
    g = torch.Generator().manual_seed(seed)
    H = 4 * C
    inp = dict(xn=exact(torch.randn(R, C, generator=g)), dy=exact(0.05 * torch.randn(R, C, generator=g)),
               w1=exact(torch.randn(H, C, generator=g) * C ** -0.5), w2g=exact(0.3 * torch.randn(H, C, generator=g) * H ** -0.5),
               b1=0.2 * torch.randn(H, generator=g),
               G0=0.05 * torch.randn(C, H, generator=g), S0=0.05 * torch.randn(C, generator=g),
               dW0=0.05 * torch.randn(H, C, generator=g), db0=0.05 * torch.randn(H, generator=g))
    if live_rows is not None:
        keep = torch.zeros(R, dtype=torch.bool)
        keep[live_rows] = True
        inp["dy"] = inp["dy"] * keep[:, None]
    return {k: v.to(dev) for k, v in inp.items()}


def mlp_bwd_base(inp):
    """the part of the reference both precisions share (float64; on the inputs' device)"""
    xn, dy, w1, w2g, b1 = (inp[k].to(F64) for k in ("xn", "dy", "w1", "w2g", "b1"))
    return dict(a=xn @ w1.t() + b1, Sa=xn.abs() @ w1.abs().t() + b1.abs(), t=dy @ w2g.t(), St=dy.abs() @ w2g.abs().t())


def mlp_bwd_ref(inp, base, prec, planes, slices, fault=None):
    """-> (ref, bound): dxn [planes][R][C], G, S, dW1, db1 (pre-fills included).  fault: a seeded fault (MLP_BWD_FAULTS)
    applied to the float64 computation; the bound is then not meaningful."""
    xn, dy, w1 = (inp[k].to(F64) for k in ("xn", "dy", "w1"))
    R, C = xn.shape
    H, HS = 4 * C, 4 * C // planes
    a, t = base["a"], base["t"]
    if fault == "no_b1":
        a = a.clone()
        a[:, 5] -= inp["b1"][5].to(F64)
    if fault == "repeat_row":        # the last row's xn taken from row 0
        xn = xn.clone()
        xn[R - 1] = xn[0]
        a = a.clone()
        a[R - 1] = xn[0] @ w1.t() + inp["b1"].to(F64)
    if fault == "drop_row":          # the last row missing from everything
        dy = dy.clone()
        dy[R - 1] = 0
        t = t.clone()
        t[R - 1] = 0
    gl, gp = _gelu(prec, a), _gelu_grad(prec, a)
    da = t * gp
    sl = [slice(s * HS, (s + 1) * HS) for s in range(planes)]
    dxn = torch.stack([da[:, s] @ w1[s] for s in sl])
    Gm = dy.t() @ gl
    Sv = dy.sum(0)
    if fault == "shift_dxn":
        dxn = torch.roll(dxn, 1, dims=1)
    if fault == "swap_hidden":       # hidden units 4-7 and 8-11 swapped in G
        Gm = Gm.clone()
        Gm[:, 4:8], Gm[:, 8:12] = Gm[:, 8:12].clone(), Gm[:, 4:8].clone()
    if fault == "drop_plane":
        dxn = dxn.clone()
        dxn[planes - 1] = 0
    if fault == "S_lacks_slice":     # the last hidden slice's C / planes channels of colsum(dy)
        Sv = Sv.clone()
        Sv[C - C // planes:] = 0
    ref = dict(dxn=dxn, G=inp["G0"].to(F64) + Gm, S=inp["S0"].to(F64) + Sv, dW1=inp["dW0"].to(F64) + da.t() @ xn,
               db1=inp["db0"].to(F64) + da.sum(0))
    if fault is not None:
        return ref, None
    # ---- the bound
    tiles = -(-R // 64)
    per_wg = -(-tiles // slices)
    chain = 64 * per_wg + slices + 2             # rows through one workgroup's accumulators + the slice reduction + "+="
    e_a = acc(C + 2, base["Sa"])                 # K = C products + the bias
    e_gv = _gelu_f(prec, a) + L_GELU * e_a
    e_g = e_gv + r16(prec, gl, e_gv)             # g kept in 16 bit
    e_t = acc(C, base["St"])
    e_gp = gelu_grad_err(prec, a, e_a)
    e_dav = t.abs() * e_gp + e_t * (gp.abs() + e_gp) + EPS * da.abs()   # the fp32 da
    e_da = e_dav + r16(prec, da, e_dav)          # da kept in 16 bit
    ada, aw1, adyt = da.abs() + e_da, w1.abs(), dy.abs().t()
    bound = dict(
        dxn=torch.stack([e_da[:, s] @ aw1[s] + acc(HS + 1, ada[:, s] @ aw1[s]) for s in sl]),
        G=adyt @ e_g + acc(chain, adyt @ (gl.abs() + e_g) + inp["G0"].to(F64).abs()),
        S=acc(chain + 64, dy.abs().sum(0) + inp["S0"].to(F64).abs()),   # (+ the row groups that meet in LDS)
        dW1=e_da.t() @ xn.abs() + acc(chain, ada.t() @ xn.abs() + inp["dW0"].to(F64).abs()),
        db1=e_dav.sum(0) + acc(chain, (da.abs() + e_dav).sum(0) + inp["db0"].to(F64).abs()))
    return ref, bound


def mlp_bwd_emulate(inp, prec, planes):
    """the kernel's arithmetic on the CPU: fp32 products and sums, g and da rounded to the operand type at its points"""
    f = torch.float32
    xn, dy, w1, w2g, b1 = (inp[k].to(f) for k in ("xn", "dy", "w1", "w2g", "b1"))
    C = xn.shape[1]
    HS = 4 * C // planes
    a = xn @ w1.t() + b1
    g16 = _gelu(prec, a.to(F64)).to(f).to(DT[prec]).to(f)
    da32 = (dy @ w2g.t()) * _gelu_grad(prec, a.to(F64)).to(f)
    da16 = da32.to(DT[prec]).to(f)
    return dict(dxn=torch.stack([da16[:, s * HS:(s + 1) * HS] @ w1[s * HS:(s + 1) * HS] for s in range(planes)]),
                G=inp["G0"] + dy.t() @ g16, S=inp["S0"] + dy.sum(0), dW1=inp["dW0"] + da16.t() @ xn, db1=inp["db0"] + da32.sum(0))


MLP_BWD_FAULTS = ("drop_row", "repeat_row", "shift_dxn", "swap_hidden", "no_b1", "S_lacks_slice")   # + drop_plane at C = 128


# ---------------------------------------------------------------------------------------------------------------------
# s2mlp_bwd: dy [R][256], a [R][1024], w2gt = (diag(gamma) W2)^T [1024][256], w1t = W1^T [256][1024]
# ---------------------------------------------------------------------------------------------------------------------
def s2mlp_inputs(R, seed, dev="cpu"):
    """a spans both signs with |a| up to 6 (and holds exact zeros: the derivative's jump is on the grid)"""
    g = torch.Generator().manual_seed(seed)
    a = exact((torch.rand(R, 1024, generator=g) * 12.0 - 6.0))
    a.view(-1)[::97] = 0.0
    a.view(-1)[1::193] = 6.0
    a.view(-1)[2::193] = -6.0
    inp = dict(dy=exact(0.05 * torch.randn(R, 256, generator=g)), a=a,
               w2gt=exact(0.3 * torch.randn(1024, 256, generator=g) / 32.0), w1t=exact(torch.randn(256, 1024, generator=g) / 16.0))
    return {k: v.to(dev) for k, v in inp.items()}


def s2mlp_base(inp):
    dy, w2gt = inp["dy"].to(F64), inp["w2gt"].to(F64)
    return dict(t=dy @ w2gt.t(), St=dy.abs() @ w2gt.abs().t())


def s2mlp_ref(inp, base, prec, fault=None):
    """-> (ref, bound): da [R][1024] (the live rows), dxn [R][256]"""
    a, w1t, t = inp["a"].to(F64), inp["w1t"].to(F64), base["t"]
    R = a.shape[0]
    if fault == "repeat_row":
        a = a.clone()
        a[R - 1] = a[0]
    gp = _gelu_grad(prec, a)
    da = t * gp
    if fault == "drop_row":
        da = da.clone()
        da[R - 1] = 0
    if fault == "swap_hidden":
        da = da.clone()
        da[:, 4:8], da[:, 8:12] = da[:, 8:12].clone(), da[:, 4:8].clone()
    dxn = da @ w1t.t()
    if fault == "last_chunk_missing":    # the second product of chunk 7 (hidden 896 ..) never added
        dxn = da[:, :896] @ w1t[:, :896].t()
    if fault == "chunk_shift":           # da of chunk k stored into chunk k - 1's columns
        da = torch.roll(da, -128, dims=1)
    if fault == "shift_row":
        dxn = torch.roll(dxn, 1, dims=0)
    ref = dict(da=da, dxn=dxn)
    if fault is not None:
        return ref, None
    e_t = acc(256, base["St"])
    e_gp = _gelu_grad_f(prec, a)             # a is an exact input: no pre-activation error, the same side of the jump
    e_dav = t.abs() * e_gp + e_t * (gp.abs() + e_gp) + EPS * da.abs()
    e_da = e_dav + r16(prec, da, e_dav)      # da leaves (and enters the second product) in 16 bit
    aw = w1t.abs().t()
    return ref, dict(da=e_da, dxn=e_da @ aw + acc(1024, (da.abs() + e_da) @ aw))


def s2mlp_emulate(inp, prec):
    f = torch.float32
    dy, a, w2gt, w1t = (inp[k].to(f) for k in ("dy", "a", "w2gt", "w1t"))
    da16 = ((dy @ w2gt.t()) * _gelu_grad(prec, a.to(F64)).to(f)).to(DT[prec])
    return dict(da=da16, dxn=da16.to(f) @ w1t.t())


S2MLP_FAULTS = ("drop_row", "repeat_row", "shift_row", "swap_hidden", "chunk_shift", "last_chunk_missing")


# ---------------------------------------------------------------------------------------------------------------------
# fused_mlp: xn [M][C], w1 [4C][C], w2 [C][4C] (masters that are exact in the operand type), b1, b2, gamma, xres [M][C]
# ---------------------------------------------------------------------------------------------------------------------
def fused_inputs(C, M, seed, dev="cpu"):
    g = torch.Generator().manual_seed(seed)
    H = 4 * C
    inp = dict(xn=exact(torch.randn(M, C, generator=g)), w1=exact(torch.randn(H, C, generator=g) * C ** -0.5),
               w2=exact(torch.randn(C, H, generator=g) * H ** -0.5), b1=0.2 * torch.randn(H, generator=g),
               b2=0.2 * torch.randn(C, generator=g), gamma=0.5 + 0.25 * torch.randn(C, generator=g),
               xres=torch.randn(M, C, generator=g), x0=torch.randn(M, C, generator=g))
    # two hidden units carry a large bias: one unit's b1 is one of 4C terms of a row of W2, so its absence shows above the
    # 16-bit rounding of the other 4C - 1 only where |b1| is several times the mean |g|
    inp["b1"][5], inp["b1"][H - 6] = 3.0, -3.0
    return {k: v.to(dev) for k, v in inp.items()}


def fused_base(inp):
    xn, w1, b1 = (inp[k].to(F64) for k in ("xn", "w1", "b1"))
    return dict(a=xn @ w1.t() + b1, Sa=xn.abs() @ w1.abs().t() + b1.abs())


def fused_ref(inp, base, prec, res="xres", fault=None):
    """-> (ref, bound) of x = inp[res] + gamma (W2 gelu(a) + b2); res = 'xres' (elsewhere) or 'x0' (in place)"""
    w2, b2, gam, xr = (inp[k].to(F64) for k in ("w2", "b2", "gamma", res))
    a = base["a"]
    M, C = xr.shape
    if fault == "no_b1":
        a = a.clone()
        a[:, 5] -= inp["b1"][5].to(F64)
    if fault == "repeat_row":
        a = a.clone()
        a[M - 1] = a[0]
    gl = _gelu(prec, a)
    if fault == "swap_hidden":
        gl = gl.clone()
        gl[:, 4:8], gl[:, 8:12] = gl[:, 8:12].clone(), gl[:, 4:8].clone()
    z = gl @ w2.t()
    if fault == "no_b2":
        b2 = torch.zeros_like(b2)
    if fault == "no_gamma":
        gam = torch.ones_like(gam)
    if fault == "xres_from_x":
        xr = inp["x0" if res == "xres" else "xres"].to(F64)
    upd = gam * (z + b2)
    if fault == "drop_row":
        upd = upd.clone()
        upd[M - 1] = 0
    if fault == "shift_row":
        upd = torch.roll(upd, 1, dims=0)
    if fault == "ragged80":              # channels 76-79 of a width-80 row left at the residual
        upd = upd.clone()
        upd[:, 76:80] = 0
    ref = dict(x=xr + upd)
    if fault is not None:
        return ref, None
    H = 4 * C
    e_a = acc(C + 2, base["Sa"])
    e_gv = _gelu_f(prec, a) + L_GELU * e_a
    e_g = e_gv + r16(prec, gl, e_gv)         # g kept in 16 bit
    aw = w2.abs().t()
    e_z = e_g @ aw + acc(H, (gl.abs() + e_g) @ aw)
    # the epilogue's three fp32 roundings: z + b2, gamma * (..), xres + (..)
    return ref, dict(x=gam.abs() * e_z + 3 * EPS * (gam.abs() * (z.abs() + e_z + b2.abs()) + xr.abs()))


def fused_emulate(inp, prec, res="xres"):
    f = torch.float32
    xn, w1, w2, b1, b2, gam, xr = (inp[k].to(f) for k in ("xn", "w1", "w2", "b1", "b2", "gamma", res))
    g16 = _gelu(prec, (xn @ w1.t() + b1).to(F64)).to(f).to(DT[prec]).to(f)
    return dict(x=xr + gam * (g16 @ w2.t() + b2))


FUSED_FAULTS = ("drop_row", "repeat_row", "shift_row", "swap_hidden", "no_b1", "no_b2", "no_gamma", "xres_from_x")   # + ragged80


# ---------------------------------------------------------------------------------------------------------------------
# fc2_grads (fp32 throughout): G [C][H], S [C], w2 [C][H], b2, gamma [C]
# ---------------------------------------------------------------------------------------------------------------------
def fc2_inputs(C, H, seed, dev="cpu"):
    g = torch.Generator().manual_seed(seed)
    inp = dict(G=torch.randn(C, H, generator=g), S=torch.randn(C, generator=g), w2=torch.randn(C, H, generator=g) * H ** -0.5,
               b2=0.5 * torch.randn(C, generator=g), gamma=0.5 + 0.25 * torch.randn(C, generator=g))
    return {k: v.to(dev) for k, v in inp.items()}


def fc2_ref(inp, fault=None):
    G, S, w2, b2, gam = (inp[k].to(F64) for k in ("G", "S", "w2", "b2", "gamma"))
    H = G.shape[1]
    ref = dict(dW2=gam[:, None] * G, db2=gam * S, dgamma=(w2 * G).sum(1) + b2 * S)
    if fault == "no_b2S":
        ref["dgamma"] = (w2 * G).sum(1)
    if fault == "no_gamma":
        ref["dW2"] = G.clone()
    if fault is not None:
        return ref, None
    # dgamma: a thread's ceil(H / 256) products, six steps of the wave sum, four waves, b2 S and the last addition
    n = math.ceil(H / 256) + 6 + 4 + 2
    return ref, dict(dW2=EPS * ref["dW2"].abs(), db2=EPS * ref["db2"].abs(), dgamma=acc(n, (w2 * G).abs().sum(1) + (b2 * S).abs()))


def fc2_emulate(inp):
    G, S, w2, b2, gam = (inp[k] for k in ("G", "S", "w2", "b2", "gamma"))
    return dict(dW2=gam[:, None] * G, db2=gam * S, dgamma=(w2 * G).sum(1) + b2 * S)


FC2_FAULTS = ("no_b2S", "no_gamma")
