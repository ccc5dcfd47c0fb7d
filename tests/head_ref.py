"""Float64 references, per-element bounds, emulations and seeded faults for the classifier heads one kernel at a time
(btsbot_op_head, btsbot_op_ht_*: btsbot_amd/csrc/head_ops.hip over head.hip, head16.hip, head_train.hip).

The references apply no intermediate rounding.  What a kernel may differ by is derived per element from what it
legitimately does, in mlp_ref.py's vocabulary (acc, r16, EPS, U, SUB, L_GELU, _gelu_f); device-math allowances are the
figures the project states elsewhere (erff 2 ulp, v_exp 1 ulp, rsqrtf 2 ulp) and nothing is fitted:

  acc(n, S)   fp32 accumulation of n terms whose absolute values sum to S:  n EPS S
  fp32 layers (head.hip dense_t, head_train.hip lin_*):  acc(n, S),  S = sum |a| |w| + |bias|,  n the chain the kernel has:
      dense_t        a K slice of kchunk fmas, then bias + ks partials in LDS:      n = kchunk + ks + 1    (dense_plan)
      lin_fwd        four interleaved chains + their three adds (+ bias):           n = K // 4 + K % 4 + 3
      lin_bwd_in     the same over N
      wide layers    the fp32 MFMA GEMM, K products in whatever order + bias:       n = K + 2
      lin_bwd_w*     the rows of one slice, then the slices that meet in LDS:       w4: 2 ceil(M / 32) + 17 (two chains per
                     slice of 16; the bias column adds d0 + d1 first), <4, 64>: ceil(M / 64) + 3 + 64, <16, 16>:
                     ceil(M / 16) + 3 + 16
  split layers (head16.hip dense16): the kernel holds each fp32 value v as hi + lo, hi = T(v), lo = T(v - hi), and sums
      a_hi w_hi + a_lo w_hi + a_hi w_lo.  Against a w: the dropped a_lo w_lo and the second roundings of both remainders,
      3 u^2 |a| |w| per product; where the remainder underflows (f16), SUB per operand times the other's magnitude;
      the sum itself, acc(32 ksp + split + 2, (1 + 2 u) sum |a| |w| + |bias|): ksp MFMAs of 32 products on each of three
      accumulators, their two adds and the `split` K parts that meet in LDS (h16_plan); the activation is gelu_poly<5>
      in both 16-bit modes: its distance to the erf GELU at the reference's pre-activation (computed here in float64)
      + its fp32 evaluation error (_gelu_f, degree 5).
  whole fused head: a running bound carried forward in float64,  e_out = L_act (|W| e_in + local) + act's own error;
      `features` / `hidden` in the 16-bit modes add the hi + lo representation error u^2 |v| + SUB and the rounding of
      their fp32 sum, EPS |v|.
  LayerNorm of the image feature (both heads, feat_rows), F values per row over 64 lanes, D = ceil(F / 64) + 6:
      e_mean = D EPS mean|x|;  d = x - mean: e_d = e_mean + EPS |d|;  e_var = mean(2 |d| e_d + e_d^2) + (D + 3) EPS var
      e_rstd = rstd^3 / 2 (e_var + 2 EPS (var + eps)) + 4 EPS rstd                (test_gpu_maxvit_train_ops.py's form)
      e_z = |w| (rstd e_d + |d| e_rstd + 3 EPS |xhat|) + EPS |z|
  BatchNorm fold (inference): scale = w / sqrt(rv + 1e-5), shift = b - rm scale, x1 = fma(v, scale, shift):
      8 EPS (|v| |s| + |rm| |s| + |b|)
  BatchNorm1d forward (training), one pass for the mean, D = ceil(M / 256) + 9 (a thread's rows, wave_sum, 4 waves):
      e_mean = (D + 1) EPS mean|x|;  e_var = (D + 4) EPS (var + e_mean^2) + e_mean^2;  e_rstd as above (eps 1e-5)
      e_xhat = rstd (e_mean + EPS |x - mu|) + |x - mu| e_rstd + EPS |xhat|;  e_out = |w| e_xhat + 2 EPS (|xhat w| + |b|)
      running mean 0.1 e_mean + 4 EPS (0.9 |rm| + 0.1 |mu|); running variance alike with M / (M - 1) e_var
  BatchNorm1d backward: db = sum dy, dw = sum dy xhat (xhat an input): acc(D, sum |dy|), acc(D + 1, sum |dy xhat|)
  sigmoid 1 / (1 + expf(-z)): e_z / 4 + EPS s (3 + (1 - s) (2 + |z|)) + 2^-126   (expf's argument scaling, v_exp, add,
      divide; a score below fp32's smallest normal is 0 once expf overflows: z < -88.7)
  GELU' (act_bwd): _gelu_grad_f's fp32 form, times |dout keep_scale|, + 2 EPS |result|

What the cross-term rows of the issue's table mean for the cases: a dropped a_lo w_hi or a_hi w_lo is ~u S.  In bf16
that is 7 to 57 times 3 u^2 S at every K of the head; in f16 the acc term (K EPS S) overtakes 3 u^2 S as K grows, and at
K = 768 a dropped cross term is only ~1.05 times the whole bound -- so the f16 cross-term faults are shown, and guarded
on the GPU, on layers with K <= 128 (the metadata layers and the second fusion layer); the wide first fusion layer
guards bf16 only.
"""
import math

import torch

from gelu_ref import EPS, L_GELU, SUB, U, _gelu_f, _gelu_grad_f, gelu_erf, gelu_erf_grad, gelu_poly
from mlp_ref import DT, F64, acc, r16, ratio, rnd, worst  # noqa: F401  (re-exported for the tests)

HN_EPS, BN_EPS, BN_MOM = 1e-6, 1e-5, 0.1
HG, HNT, PARTN = 8, 512, 2048          # head.hip: alerts per workgroup, threads, cross-slice scratch rows
HA, HNW, KGRAN = 16, 8, 2              # head16.hip: alerts per workgroup, waves, k-steps per group


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' own plans (mirrored for the chain lengths of the bounds and for the emulations; the GPU tests assert
# paths through the library's companions where it has them)
# ---------------------------------------------------------------------------------------------------------------------
def dense_plan(K, N):
    """head.hip dense_t: (npt, ks, kchunk, passes)"""
    npt = 4 if N % 4 == 0 else 1
    nq = N // npt
    ks = 1
    while ks * 2 * nq <= HNT and ks * 2 * N <= PARTN and ks < 16 and K // (ks * 2) >= 8:
        ks *= 2
    return npt, ks, cdiv(K, ks), cdiv(nq, HNT)


def kpad(K):
    return cdiv(K, 32 * KGRAN) * 32 * KGRAN


def h16_plan(case):
    """head16.hip: per layer of the chain (name, K, N, split, ksp), with launch_head16's LDS pitches behind the split"""
    F, nm, f1, f2, dims = case["F"], case["n_meta"], case["f1"], case["f2"], case["dims"]
    zw = F + (f2 if nm else 0)
    zc = kpad(zw)
    if nm and F + kpad(f2) > zc:
        zc = F + kpad(f2)
    tw = max([kpad(nm), kpad(f1)] if nm else [0])
    tw = max([tw] + [kpad(n) for n in dims[1:]])
    pitch = {0: zc * 2 + 16, 1: tw * 2 + 16, 2: tw * 2 + 16}
    steps = []
    if nm:
        steps += [("m1", nm, f1, -1), ("m2", f1, f2, 1)]
    steps += [(f"c{i}", dims[i], dims[i + 1], 2 if i == 0 else 0) for i in range(len(dims) - 1)]
    out = []
    for name, K, N, red in steps:
        KS, tiles = kpad(K) // 32, cdiv(N, 16)
        slots = 2 * HA * pitch[red] // 1024 if red >= 0 else 0
        split = 1
        while split * 2 * tiles <= HNW and KS % (split * 2 * KGRAN) == 0 and tiles * (split * 2 - 1) <= slots:
            split *= 2
        out.append((name, K, N, split, KS // split))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def head_case(F=0, hn=False, n_meta=0, f1=0, f2=0, trailing=False, dims=(1, 1), act="gelu", B=1, seed=0):
    zw = F + (f2 if n_meta else 0)
    assert dims[0] == zw and dims[-1] >= 1, (dims, zw)
    return dict(F=F, hn=hn, n_meta=n_meta, f1=f1, f2=f2, trailing=trailing, dims=tuple(dims), act=act, B=B, seed=seed)


def head_inputs(case, dev="cpu", feat_scale=1.0):
    """fp32 parameters in state-dict layout and rows: randn rows, randn / sqrt(K) filters (the issue's scales)"""
    g = torch.Generator().manual_seed(1000003 * case["seed"] + 7919 * case["B"] + 31 * case["F"] + case["n_meta"])
    rn = lambda *s: torch.randn(*s, generator=g)
    P = {}
    B, F, nm, f1, f2 = case["B"], case["F"], case["n_meta"], case["f1"], case["f2"]
    if F:
        P["feat"] = feat_scale * rn(B, F)
        if case["hn"]:
            P["hn_w"], P["hn_b"] = 1.0 + 0.2 * rn(F), 0.2 * rn(F)
    if nm:
        P["meta"] = 3.0 * rn(B, nm) + 2.0
        P["bn_w"], P["bn_b"], P["bn_rm"] = 1.0 + 0.2 * rn(nm), 0.2 * rn(nm), 2.0 + 0.5 * rn(nm)
        P["bn_rv"] = 9.0 * (0.5 + torch.rand(nm, generator=g))
        P["m1_w"], P["m1_b"] = rn(f1, nm) * nm ** -0.5, 0.2 * rn(f1)
        P["m2_w"], P["m2_b"] = rn(f2, f1) * f1 ** -0.5, 0.2 * rn(f2)
    d = case["dims"]
    for i in range(len(d) - 1):
        P[f"c{i}_w"], P[f"c{i}_b"] = rn(d[i + 1], d[i]) * d[i] ** -0.5, 0.2 * rn(d[i + 1])
    return {k: v.to(dev) for k, v in P.items()}


# ---------------------------------------------------------------------------------------------------------------------
# activations and their bounds
# ---------------------------------------------------------------------------------------------------------------------
def act_ref(x, act):
    return gelu_erf(x) if act == "gelu" else x.clamp(min=0) if act == "relu" else x


def act_kernel(x, act, prec):
    """what the kernel's activation computes in exact arithmetic (head16: gelu_poly<5> in both 16-bit modes)"""
    if act == "gelu" and prec != "f32":
        return gelu_poly(x, 5)
    return act_ref(x, act)


def act_bound(pre, e_pre, act, prec):
    if act != "gelu":
        return e_pre
    at = pre.abs() + e_pre
    if prec == "f32":
        return L_GELU * e_pre + _gelu_f("f32", at)
    return L_GELU * e_pre + (gelu_poly(pre, 5) - gelu_erf(pre)).abs() + _gelu_f("f16", at)


def sigmoid_bound(z, e_z):
    s = torch.sigmoid(z)
    return 0.25 * e_z + EPS * s * (3.0 + (1.0 - s) * (2.0 + z.abs())) + 2.0 ** -126


def ln_rows(x, w, b, eps):
    """-> (z, e_z) of LayerNorm over the last dimension computed in fp32 over 64 lanes (w None: the copy, exact)"""
    if w is None:
        return x, torch.zeros_like(x)
    Fd = x.shape[1]
    D = cdiv(Fd, 64) + 6
    mu = x.mean(1, keepdim=True)
    d = x - mu
    var = (d * d).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    e_mean = D * EPS * x.abs().mean(1, keepdim=True)
    e_d = e_mean + EPS * d.abs()
    e_var = (2 * d.abs() * e_d + e_d * e_d).mean(1, keepdim=True) + (D + 3) * EPS * var
    e_rstd = 0.5 * rstd ** 3 * (e_var + 2 * EPS * (var + eps)) + 4 * EPS * rstd
    xhat = d * rstd
    z = xhat * w + b
    return z, w.abs() * (rstd * e_d + d.abs() * e_rstd + 3 * EPS * xhat.abs()) + EPS * z.abs()


# ---------------------------------------------------------------------------------------------------------------------
# the whole inference head: reference + running bound
# ---------------------------------------------------------------------------------------------------------------------
def _layer(a, e, W, b, act, prec, n_acc):
    pre = a @ W.t() + b
    am = a.abs() + e
    Sa = am @ W.abs().t()
    if prec == "f32":
        loc = acc(n_acc, Sa + b.abs())
    else:
        u = U[prec]
        loc = 3 * u * u * Sa + SUB[prec] * (am.sum(1, keepdim=True) + W.abs().sum(1)[None, :]) \
            + acc(n_acc, (1 + 2 * u) * Sa + b.abs())
    e_pre = e @ W.abs().t() + loc
    return pre, e_pre, act_ref(pre, act), act_bound(pre, e_pre, act, prec)


def head_ref(P, case, prec="f32"):
    """-> (ref, bound): features, hidden, logits, scores and the pre-activations `pre_<layer>` (float64)"""
    P = {k: v.to(F64) for k, v in P.items()}
    act, dims = case["act"], case["dims"]
    plan16 = {n: (s, ksp) for n, _, _, s, ksp in h16_plan(case)} if prec != "f32" else None

    def n_acc(name, K, N):
        if prec == "f32":
            _, ks, kchunk, _ = dense_plan(K, N)
            return kchunk + ks + 1
        s, ksp = plan16[name]
        return 32 * ksp + s + 2

    ref, bnd, parts, eparts = {}, {}, [], []
    if case["F"]:
        z, ez = ln_rows(P["feat"], P.get("hn_w"), P.get("hn_b"), HN_EPS)
        parts.append(z)
        eparts.append(ez)
    if case["n_meta"]:
        s = P["bn_w"] / (P["bn_rv"] + BN_EPS).sqrt()
        x1 = (P["meta"] - P["bn_rm"]) * s + P["bn_b"]
        e1 = 8 * EPS * (P["meta"].abs() * s.abs() + (P["bn_rm"] * s).abs() + P["bn_b"].abs())
        ref["pre_m1"], bnd["pre_m1"], h1, eh1 = _layer(x1, e1, P["m1_w"], P["m1_b"], act, prec,
                                                       n_acc("m1", case["n_meta"], case["f1"]))
        ref["pre_m2"], bnd["pre_m2"], a2, ea2 = _layer(h1, eh1, P["m2_w"], P["m2_b"], act if case["trailing"] else "none",
                                                       prec, n_acc("m2", case["f1"], case["f2"]))
        parts.append(a2)
        eparts.append(ea2)
    z, ez = torch.cat(parts, 1), torch.cat(eparts, 1)

    def rep(v, e):    # an embedding row as the 16-bit head stores it: hi + lo added back in fp32
        return e if prec == "f32" else e + U[prec] ** 2 * v.abs() + SUB[prec] + EPS * v.abs()

    ref["features"], bnd["features"] = z, rep(z, ez)
    a, e = z, ez
    nl = len(dims) - 1
    for i in range(nl):
        if i + 1 == nl:
            ref["hidden"], bnd["hidden"] = a, rep(a, e)
        ref[f"pre_c{i}"], bnd[f"pre_c{i}"], a, e = _layer(a, e, P[f"c{i}_w"], P[f"c{i}_b"], act if i + 1 < nl else "none",
                                                           prec, n_acc(f"c{i}", dims[i], dims[i + 1]))
    ref["logits"], bnd["logits"] = a[:, 0], e[:, 0]
    ref["scores"], bnd["scores"] = torch.sigmoid(a[:, 0]), sigmoid_bound(a[:, 0], e[:, 0])
    return ref, bnd


# ---------------------------------------------------------------------------------------------------------------------
# emulation of the fused heads' arithmetic in float64 (same padding, slicing and order of K parts), with seeded faults
# ---------------------------------------------------------------------------------------------------------------------
HEAD_FAULTS = ("drop_alo_whi", "drop_ahi_wlo", "bias_every_part", "pad_nonzero", "ln_eps_1e5", "flip_trailing",
               "hidden_other_buffer", "lose_ragged_slice", "keep_first_pass")


def _split(prec, v):
    hi = rnd(prec, v)
    return hi, rnd(prec, v - hi)


def _dense_f32_emu(a, W, b, act, fault):
    K, N = W.shape[1], W.shape[0]
    npt, ks, kchunk, passes = dense_plan(K, N)
    if fault == "lose_ragged_slice":
        kchunk = K // ks                      # floor: the last K % ks inputs belong to no slice
    t = b.expand(a.shape[0], N).clone()
    for s in range(ks):
        k0, k1 = s * kchunk, min(K, (s + 1) * kchunk)
        t = t + a[:, k0:k1] @ W[:, k0:k1].t()
    if fault == "keep_first_pass" and passes > 1:
        t[:, HNT * npt:] = b[HNT * npt:]      # what pass 1 finalised before pass 2 wrote its partials (read as zero)
    return t, act_kernel(t, act, "f32")


def _dense16_emu(a, W, b, act, prec, split, fault, fault_here):
    """a: the fp32 values the kernel splits (float64 here); K padded to kpad with zero activations and zero filters"""
    K, N = W.shape[1], W.shape[0]
    Kp = kpad(K)
    ap = torch.zeros(a.shape[0], Kp, dtype=F64)
    Wp = torch.zeros(N, Kp, dtype=F64)
    ap[:, :K], Wp[:, :K] = a, W
    if fault == "pad_nonzero" and fault_here and Kp > K:
        ap[:, K] = 1.0                                  # a stale activation column ...
        flat = torch.cat([W.reshape(-1), W.reshape(-1)[:Kp]])
        Wp[:, K] = flat[torch.arange(N) * K + K]        # ... meets a filter image packed without its k < K test
    ah, al = _split(prec, ap)
    wh, wl = _split(prec, Wp)
    t = torch.zeros(a.shape[0], N, dtype=F64)
    ksp = Kp // split
    for p in range(split):
        sl = slice(p * ksp, (p + 1) * ksp)
        part = ah[:, sl] @ wh[:, sl].t()
        if not (fault == "drop_alo_whi" and fault_here):
            part = part + al[:, sl] @ wh[:, sl].t()
        if not (fault == "drop_ahi_wlo" and fault_here):
            part = part + ah[:, sl] @ wl[:, sl].t()
        if p == 0 or (fault == "bias_every_part" and fault_here):
            part = part + b
        t = t + part
    return t, act_kernel(t, act, prec)


def head_emulate(P, case, prec="f32", fault=None, at=None):
    """The fused head as its kernel computes it, in float64.  fault: one of HEAD_FAULTS; at: the layer a per-layer fault
    sits in (m1, m2, c0 ..)."""
    P = {k: v.to(F64) for k, v in P.items()}
    act, dims = case["act"], case["dims"]
    splits = {n: s for n, _, _, s, _ in h16_plan(case)} if prec != "f32" else {}

    def dense(name, a, W, b, actn):
        if prec == "f32":
            return _dense_f32_emu(a, W, b, actn, fault if at in (None, name) else None)
        return _dense16_emu(a, W, b, actn, prec, splits[name], fault, at in (None, name))

    out, parts = {}, []
    if case["F"]:
        parts.append(ln_rows(P["feat"], P.get("hn_w"), P.get("hn_b"), 1e-5 if fault == "ln_eps_1e5" else HN_EPS)[0])
    if case["n_meta"]:
        s = P["bn_w"] / (P["bn_rv"] + BN_EPS).sqrt()
        x1 = P["meta"] * s + (P["bn_b"] - P["bn_rm"] * s)
        out["pre_m1"], h1 = dense("m1", x1, P["m1_w"], P["m1_b"], act)
        trailing = case["trailing"] != (fault == "flip_trailing")
        out["pre_m2"], a2 = dense("m2", h1, P["m2_w"], P["m2_b"], act if trailing else "none")
        parts.append(a2)
    z = torch.cat(parts, 1)

    def rep(v):
        if prec == "f32":
            return v
        hi, lo = _split(prec, v)
        return hi + lo

    out["features"] = rep(z)
    a, prev = z, z
    nl = len(dims) - 1
    for i in range(nl):
        if i + 1 == nl:
            # the ping-pong buffers hold layer i-1's and layer i-2's outputs; the wrong one is the older
            out["hidden"] = rep(prev[:, :a.shape[1]] if fault == "hidden_other_buffer" else a)
        prev = a
        out[f"pre_c{i}"], a = dense(f"c{i}", a, P[f"c{i}_w"], P[f"c{i}_b"], act if i + 1 < nl else "none")
    out["logits"] = a[:, 0]
    out["scores"] = torch.sigmoid(a[:, 0])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the training kernels: references, bounds, and emulations with faults (fp32 kernels: the emulation is the kernel's
# grouping of the sum in float64)
# ---------------------------------------------------------------------------------------------------------------------
HT_FAULTS = ("swap_variance", "no_keep_scale", "tanh_gelu_grad", "drop_tail_rows_w4", "drop_db_column")


def act_grad_ref(x, act):
    return gelu_erf_grad(x) if act == "gelu" else (x > 0).to(F64) if act == "relu" else torch.ones_like(x)


def gelu_tanh_grad(x):
    c = math.sqrt(2.0 / math.pi)
    t = torch.tanh(c * (x + 0.044715 * x ** 3))
    return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * c * (1 + 3 * 0.044715 * x * x)


def lin_fwd_ref(x, w, b, act, mask, keep_scale, wide):
    """-> (ref, bound) of pre and outa.  wide: the MFMA GEMM path (the library's companion says which)"""
    x, w, b = x.to(F64), w.to(F64), b.to(F64)
    K = w.shape[1]
    pre = x @ w.t() + b
    S = x.abs() @ w.abs().t() + b.abs()
    e_pre = acc(K + 2 if wide else K // 4 + K % 4 + 3, S)
    out = act_ref(pre, act)
    e_out = act_bound(pre, e_pre, act, "f32")
    if mask is not None:
        out = out * mask.to(F64) * keep_scale
        e_out = (e_out * keep_scale + EPS * out.abs()) * mask.to(F64)
    return dict(pre=pre, outa=out), dict(pre=e_pre, outa=e_out)


def lin_bwd_in_ref(dpre, w, wide):
    dpre, w = dpre.to(F64), w.to(F64)
    N = w.shape[0]
    return dpre @ w, acc(N + 1 if wide else N // 4 + N % 4 + 3, dpre.abs() @ w.abs())


def act_bwd_ref(dout, pre, act, mask, keep_scale, fault=None):
    dout, pre = dout.to(F64), pre.to(F64)
    d = dout
    if mask is not None:
        d = d * mask.to(F64) * (1.0 if fault == "no_keep_scale" else keep_scale)
    g = gelu_tanh_grad(pre) if (fault == "tanh_gelu_grad" and act == "gelu") else act_grad_ref(pre, act)
    ref = d * g
    e = d.abs() * (_gelu_grad_f("f32", pre) if act == "gelu" else 0.0) + 2 * EPS * ref.abs()
    return ref, e


def lin_bwd_w_chain(kind, M):
    return {0: 2 * cdiv(M, 32) + 17, 1: cdiv(M, 64) + 3 + 64, 2: cdiv(M, 16) + 3 + 16}[kind]


def lin_bwd_w_ref(dpre, x, kind):
    """-> (ref, bound) of dw [N][K], db [N]"""
    dpre, x = dpre.to(F64), x.to(F64)
    n = lin_bwd_w_chain(kind, x.shape[0])
    return (dict(dw=dpre.t() @ x, db=dpre.sum(0)),
            dict(dw=acc(n, dpre.abs().t() @ x.abs()), db=acc(n, dpre.abs().sum(0))))


def lin_bwd_w_emulate(dpre, x, kind, fault=None):
    """the kernels' row slices in float64: w4 walks 16 slices in pairs of rows (m, m + 16) and a tail of single rows;
    the two lin_bwd_w_kernel forms walk SL slices, the column k == K being db"""
    dpre, x = dpre.to(F64), x.to(F64)
    M, N, K = x.shape[0], dpre.shape[1], x.shape[1]
    dw, db = torch.zeros(N, K, dtype=F64), torch.zeros(N, dtype=F64)
    if kind == 0:
        for g in range(16):
            m = g
            while m + 16 < M:
                for r in (m, m + 16):
                    dw += dpre[r][:, None] * x[r][None, :]
                    db += dpre[r]
                m += 32
            while m < M and fault != "drop_tail_rows_w4":
                dw += dpre[m][:, None] * x[m][None, :]
                db += dpre[m]
                m += 16
        return dict(dw=dw, db=db)
    SL = 64 if kind == 1 else 16
    for g in range(SL):
        rows = list(range(g, M, SL))
        dw += dpre[rows].t() @ x[rows]
        if fault != "drop_db_column":
            db += dpre[rows].sum(0)
    return dict(dw=dw, db=db)


def bn_fwd_ref(x, w, b, rm, rv, fault=None):
    """-> (ref, bound): xhat, out, rstd and (rm given) run_mean, run_var"""
    x, w, b = x.to(F64), w.to(F64), b.to(F64)
    M = x.shape[0]
    D = cdiv(M, 256) + 9
    mu = x.mean(0)
    d = x - mu
    var = (d * d).mean(0)
    unb = var * M / (M - 1) if M > 1 else var          # (M = 1: the kernel carries the biased variance over)
    norm_var, run_var = (unb, var) if fault == "swap_variance" else (var, unb)
    rstd = (norm_var + BN_EPS).rsqrt()
    e_mean = (D + 1) * EPS * x.abs().mean(0)
    e_var = (D + 4) * EPS * (var + e_mean ** 2) + e_mean ** 2
    e_rstd = 0.5 * rstd ** 3 * (e_var + 2 * EPS * (var + BN_EPS)) + 4 * EPS * rstd
    xhat = d * rstd
    e_xhat = rstd * (e_mean + EPS * d.abs()) + d.abs() * e_rstd + EPS * xhat.abs()
    out = xhat * w + b
    ref = dict(xhat=xhat, out=out, rstd=rstd)
    bnd = dict(xhat=e_xhat, out=w.abs() * e_xhat + 2 * EPS * ((xhat * w).abs() + b.abs()), rstd=e_rstd)
    if rm is not None:
        rm, rv = rm.to(F64), rv.to(F64)
        ref["run_mean"] = (1 - BN_MOM) * rm + BN_MOM * mu
        ref["run_var"] = (1 - BN_MOM) * rv + BN_MOM * run_var
        bnd["run_mean"] = BN_MOM * e_mean + 4 * EPS * ((1 - BN_MOM) * rm.abs() + BN_MOM * mu.abs())
        bnd["run_var"] = BN_MOM * e_var * (M / (M - 1) if M > 1 else 1.0) + 4 * EPS * ((1 - BN_MOM) * rv.abs() + BN_MOM * unb)
    return ref, bnd


def bn_bwd_ref(dy, xhat):
    dy, xhat = dy.to(F64), xhat.to(F64)
    D = cdiv(dy.shape[0], 256) + 9
    return (dict(dw=(dy * xhat).sum(0), db=dy.sum(0)),
            dict(dw=acc(D + 1, (dy * xhat).abs().sum(0)), db=acc(D, dy.abs().sum(0))))


def feat_rows_ref(feat, hw, hb, eps=HN_EPS):
    return ln_rows(feat.to(F64), None if hw is None else hw.to(F64), None if hb is None else hb.to(F64), eps)


def logits_ref(x):
    x = x.to(F64)
    return dict(logits=x, scores=torch.sigmoid(x)), dict(logits=torch.zeros_like(x), scores=sigmoid_bound(x, torch.zeros_like(x)))


# ---------------------------------------------------------------------------------------------------------------------
# the cases (shared by tests/test_gpu_head_ops.py and tests/test_head_reference.py)
# ---------------------------------------------------------------------------------------------------------------------
B_F32 = (1, 7, 8, 9, 17)        # 8 alerts per workgroup
B_16 = (1, 15, 16, 17, 33)      # 16 alerts per workgroup
PRECS3 = ("f32", "bf16", "f16")


def wirings(F, nm, f1, f2, c1, c2):
    """the five wirings of the product at one set of widths (B left to the caller)"""
    return {
        "image+ln": dict(F=F, hn=True, dims=(F, c1, c2, 1), act="gelu"),
        "image+meta": dict(F=F, n_meta=nm, f1=f1, f2=f2, trailing=True, dims=(F + f2, c1, c2, 1), act="gelu"),
        "image+ln+meta": dict(F=F, hn=True, n_meta=nm, f1=f1, f2=f2, trailing=False, dims=(F + f2, c1, c2, 1), act="relu"),
        "meta": dict(n_meta=nm, f1=f1, f2=f2, trailing=True, dims=(f2, 1), act="relu"),
        "image": dict(F=F, dims=(F, c1, c2, 1), act="gelu"),
    }


PRODUCT = wirings(640, 25, 128, 128, 128, 32)
# fp32 only: widths off every multiple the kernel likes
F32_EDGES = {
    # scalar dense_t<1> with N > 1 (30, 6, 22, 5), store_rows' dword path at widths 46 and 5, kchunk not dividing K (46 / 4)
    **{"ragged " + k: v for k, v in wirings(40, 7, 30, 6, 22, 5).items()},
    "ks capped by threads": dict(F=768, dims=(768, 128, 32, 1), act="gelu"),      # 32 quads: ks stops at 16 = HNT / 32
    "ks capped by PARTN": dict(F=64, hn=True, dims=(64, 512, 4, 1), act="relu"),   # ks 512 <= 2048 and ks 128 <= 512: ks stops at 4
    "several passes": dict(n_meta=7, f1=514, f2=6, trailing=False, dims=(6, 1), act="gelu"),   # dense_t<1>, N = 514 > HNT
}
# 16-bit only
H16_EDGES = {
    "F8 meta32 f1=16 f2=24": dict(F=8, hn=True, n_meta=32, f1=16, f2=24, trailing=True, dims=(32, 16, 1), act="gelu"),
    "F8 meta1 f1=128 f2=24": dict(F=8, n_meta=1, f1=128, f2=24, trailing=False, dims=(32, 128, 32, 1), act="relu"),
    "split 4": dict(F=256, hn=True, dims=(256, 16, 1), act="gelu"),
    "split 8": dict(F=448, n_meta=32, f1=128, f2=64, trailing=True, dims=(512, 16, 1), act="gelu"),
}
H16_REFUSED = {   # name -> (case, a word its message must hold)
    "F=12": (dict(F=12, dims=(12, 16, 1)), "feature width 12"),
    "f1=144": (dict(F=8, n_meta=8, f1=144, f2=16, dims=(24, 16, 1)), "144"),
    "n_meta=33": (dict(F=8, n_meta=33, f1=16, f2=16, dims=(24, 16, 1)), "n_meta 33"),
    "last width 2": (dict(F=8, dims=(8, 16, 2)), "last width of 2"),
}


def head_cases(prec):
    """name -> case keywords (without B) of every inference case of a precision"""
    return {**PRODUCT, **(F32_EDGES if prec == "f32" else H16_EDGES)}


def batch_sizes(prec):
    return B_F32 if prec == "f32" else B_16


# seeded faults of the fused heads: (fault, precisions, case name, layer, outputs that must leave their bound).  But for
# the one pre_c0 row these are outputs the GPU test sees (features, hidden, logits, scores): the running bound of a later
# layer swallows a cross term dropped upstream, so the guards are the layers whose output leaves the kernel directly --
# the metadata branch (features), a two-layer head's first fusion layer (hidden) -- at K <= 128, or 256 behind a LayerNorm.
HEAD_FAULT_CASES = [
    ("drop_alo_whi", ("bf16", "f16"), "F8 meta1 f1=128 f2=24", "m1", ("features",)),     # K = 1 padded to 64
    ("drop_ahi_wlo", ("bf16", "f16"), "F8 meta1 f1=128 f2=24", "m1", ("features",)),
    ("drop_alo_whi", ("bf16", "f16"), "image+meta", "m2", ("features",)),                # K = 128
    ("drop_ahi_wlo", ("bf16", "f16"), "image+meta", "m2", ("features",)),
    ("drop_alo_whi", ("bf16", "f16"), "split 4", "c0", ("hidden",)),                     # K = 256
    ("drop_ahi_wlo", ("bf16", "f16"), "split 4", "c0", ("hidden",)),
    ("drop_alo_whi", ("bf16",), "image", "c0", ("pre_c0",)),                 # K = 640: bf16 only (docstring); not an output
    ("bias_every_part", ("bf16", "f16"), "image+meta", "c1", ("hidden",)),               # split = 2
    ("bias_every_part", ("bf16", "f16"), "split 8", "c0", ("hidden", "logits", "scores")),
    ("pad_nonzero", ("bf16", "f16"), "image+meta", "m1", ("features",)),                 # K = 25 padded to 64
    ("ln_eps_1e5", PRECS3, "image+ln", None, ("features",)),
    ("flip_trailing", PRECS3, "image+meta", None, ("features", "hidden")),
    ("flip_trailing", PRECS3, "image+ln+meta", None, ("features", "hidden")),
    ("hidden_other_buffer", PRECS3, "image+ln", None, ("hidden",)),
    ("lose_ragged_slice", ("f32",), "ragged image+ln+meta", "c0", ("hidden", "logits", "scores")),   # K = 46, 4 slices of 12
    ("keep_first_pass", ("f32",), "several passes", "m1", ("features", "logits", "scores")),
]

ACTS = ("none", "gelu", "relu")
# lin_fwd / lin_bwd_in: (M, N, K, ldi - K, ldo - N); M N not a multiple of 256 but for the two GEMM-threshold shapes
LIN_SHAPES = [(3, 5, 1, 0, 0), (7, 9, 3, 2, 3), (33, 30, 4, 0, 1), (9, 7, 5, 3, 0), (17, 128, 25, 0, 0), (70, 33, 128, 4, 2)]
LIN_WIDE = [(255, 128, 512), (256, 128, 512)]   # M N K = 2^24 - 2^16 and 2^24
W4_SHAPES = [(M, 5, K) for M in (1, 16, 17, 32, 33, 100) for K in (4, 64, 68, 132)]
W464_SHAPES = [(M, 128, 25) for M in (1, 63, 64, 65, 256, 257, 300)] + [(65, 64, 127)]   # N (K + 1) = 8192 exactly
W1616_SHAPES = [(M, 65, 127) for M in (1, 15, 16, 17, 64, 65)]
BN_SHAPES = [(M, n) for M in (2, 255, 256, 257, 600) for n in (1, 25)]
FEAT_SHAPES = [(M, F) for F in (8, 40, 64, 65, 640) for M in (1, 3, 4, 5)]
LOGIT_ROWS = (1, 255, 257)


def rand(shape, seed, scale=1.0, dev="cpu"):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(dev)


def bn_input(M, n, dev="cpu"):
    """unit-spread columns with means up to a few units; the last column has mean 1e3"""
    x = rand((M, n), 17 * M + n) + 3.0 * rand((1, n), n)
    x[:, n - 1] += 1e3
    return x.to(dev)
