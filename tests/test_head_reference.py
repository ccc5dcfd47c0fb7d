"""What tests/head_ref.py's references and bounds see, shown on the CPU (the GPU file is tests/test_gpu_head_ops.py).

  * the references against other witnesses: oracle.convnext_oracle's metadata_branch / fusion_head in float64, and torch
    autograd in float64 for every backward kernel (a reference is never its own witness);
  * an emulation of each kernel's arithmetic in float64 (hi / lo rounding to the operand type, the three products, the
    same padding, slicing and order of K parts) stays within the bound at every case of the GPU file;
  * seeded faults leave the bound, each at a named case (head_ref.HEAD_FAULT_CASES, and the training kernels' below).
"""
import pytest
import torch
import torch.nn.functional as Fn

import head_ref as H
from oracle import convnext_oracle as O

F64 = torch.float64


def _case(prec, name, B):
    return H.head_case(B=B, seed=3, **H.head_cases(prec)[name])


def _sd(P, prefix, keys):
    return {prefix + k: P[v].to(F64) for k, v in keys.items()}


@pytest.mark.parametrize("name", ["image+meta", "image+ln+meta", "ragged image+meta"])
def test_reference_against_oracle(name):
    case = _case("f32", name, 9)
    P = H.head_inputs(case)
    ref, _ = H.head_ref(P, case)
    sd = _sd(P, "m.", {"0.weight": "bn_w", "0.bias": "bn_b", "0.running_mean": "bn_rm", "0.running_var": "bn_rv",
                       "1.weight": "m1_w", "1.bias": "m1_b", "4.weight": "m2_w", "4.bias": "m2_b"})
    m = O.metadata_branch(P["meta"].to(F64), sd, "m.", case["act"], case["trailing"])
    F = case["F"]
    assert torch.allclose(ref["features"][:, F:], m, rtol=1e-12, atol=1e-13)
    x = P["feat"].to(F64)
    if case["hn"]:
        x = Fn.layer_norm(x, (F,), P["hn_w"].to(F64), P["hn_b"].to(F64), 1e-6)
    assert torch.allclose(ref["features"][:, :F], x, rtol=1e-12, atol=1e-13)
    sd = _sd(P, "c.", {"0.weight": "c0_w", "0.bias": "c0_b", "2.weight": "c1_w", "2.bias": "c1_b", "5.weight": "c2_w",
                       "5.bias": "c2_b"})
    z = O.fusion_head(torch.cat([x, m], 1), sd, "c.", case["act"])
    assert torch.allclose(ref["logits"], z[:, 0], rtol=1e-12, atol=1e-13)
    assert torch.allclose(ref["scores"], torch.sigmoid(z[:, 0]), rtol=1e-12, atol=1e-14)
    h = Fn.linear(torch.cat([x, m], 1), P["c0_w"].to(F64), P["c0_b"].to(F64))
    h = Fn.linear(O._act(case["act"])(h), P["c1_w"].to(F64), P["c1_b"].to(F64))
    assert torch.allclose(ref["hidden"], O._act(case["act"])(h), rtol=1e-12, atol=1e-13)


def test_training_references_against_autograd():
    M, N, K = 33, 9, 7
    x = H.rand((M, K), 1).to(F64).requires_grad_()
    w = H.rand((N, K), 2, K ** -0.5).to(F64).requires_grad_()
    b = H.rand((N,), 3, 0.2).to(F64).requires_grad_()
    mask = (H.rand((M, N), 4) > -0.5).to(torch.uint8)
    ks = 1.0 / 0.7
    dout = H.rand((M, N), 5).to(F64)
    for act in H.ACTS:
        pre = Fn.linear(x, w, b)
        y = {"none": lambda t: t, "gelu": Fn.gelu, "relu": torch.relu}[act](pre) * mask.to(F64) * ks
        ref, _ = H.lin_fwd_ref(x.detach(), w.detach(), b.detach(), act, mask, ks, False)
        assert torch.allclose(ref["pre"], pre.detach(), rtol=1e-12) and torch.allclose(ref["outa"], y.detach(), rtol=1e-12, atol=1e-14)
        gx, gw, gb = torch.autograd.grad(y, (x, w, b), dout)
        dpre, _ = H.act_bwd_ref(dout, pre.detach(), act, mask, ks)
        assert torch.allclose(H.lin_bwd_in_ref(dpre, w.detach(), False)[0], gx, rtol=1e-11, atol=1e-13)
        r, _ = H.lin_bwd_w_ref(dpre, x.detach(), 1)
        assert torch.allclose(r["dw"], gw, rtol=1e-11, atol=1e-13) and torch.allclose(r["db"], gb, rtol=1e-11, atol=1e-13)
    # BatchNorm1d, training mode: torch's own forward, running statistics and parameter gradients
    Mb, n = 37, 5
    xb = H.bn_input(Mb, n).to(F64)
    wb = (1 + H.rand((n,), 6, 0.2)).to(F64).requires_grad_()
    bb = H.rand((n,), 7, 0.2).to(F64).requires_grad_()
    rm, rv = H.rand((n,), 8).to(F64), (1 + H.rand((n,), 9).abs()).to(F64)
    rm_t, rv_t = rm.clone(), rv.clone()
    out = Fn.batch_norm(xb, rm_t, rv_t, wb, bb, True, 0.1, 1e-5)
    ref, _ = H.bn_fwd_ref(xb, wb.detach(), bb.detach(), rm, rv)
    assert torch.allclose(ref["out"], out.detach(), rtol=1e-10, atol=1e-12)
    assert torch.allclose(ref["run_mean"], rm_t, rtol=1e-12) and torch.allclose(ref["run_var"], rv_t, rtol=1e-12)
    dy = H.rand((Mb, n), 10).to(F64)
    gw, gb = torch.autograd.grad(out, (wb, bb), dy)
    r, _ = H.bn_bwd_ref(dy, ref["xhat"])
    assert torch.allclose(r["dw"], gw, rtol=1e-10, atol=1e-12) and torch.allclose(r["db"], gb, rtol=1e-10, atol=1e-12)
    # the head LayerNorm of feat_rows
    f = H.rand((5, 65), 11).to(F64)
    hw, hb = (1 + H.rand((65,), 12, 0.2)).to(F64), H.rand((65,), 13, 0.2).to(F64)
    assert torch.allclose(H.feat_rows_ref(f, hw, hb)[0], Fn.layer_norm(f, (65,), hw, hb, 1e-6), rtol=1e-12, atol=1e-13)
    xs = torch.linspace(-6, 6, 241, dtype=F64)
    assert torch.allclose(H.act_grad_ref(xs, "gelu"), torch.autograd.functional.jacobian(lambda t: Fn.gelu(t).sum(), xs), rtol=1e-10)


def test_split_cases_reach_every_split():
    reached = {s for name, kw in H.head_cases("bf16").items() for _, _, _, s, _ in H.h16_plan(H.head_case(**kw))}
    assert {1, 2, 4, 8} <= reached, reached
    assert H.dense_plan(7, 514) == (1, 1, 7, 2) and H.dense_plan(46, 22)[1:3] == (4, 12)   # two passes; a ragged kchunk


@pytest.mark.parametrize("prec", H.PRECS3)
def test_emulation_within_bound(prec):
    bad = []
    for name in H.head_cases(prec):
        for B in H.batch_sizes(prec):
            case = _case(prec, name, B)
            P = H.head_inputs(case)
            ref, bnd = H.head_ref(P, case, prec)
            r = H.worst(H.head_emulate(P, case, prec), ref, bnd)
            bad += [f"{prec} {name} B={B} {k}: {v:.3g}" for k, v in r.items() if not v <= 1.0]
    assert not bad, "\n".join(bad)


def test_f16_small_rows_need_the_underflow_term():
    """rows of magnitude 1e-3 in f16: the remainders fall into f16's subnormals; the bound holds with SUB and would not
    without it (the issue's 17 x)."""
    case = H.head_case(B=16, seed=5, **H.head_cases("f16")["image"])
    P = H.head_inputs(case, feat_scale=1e-3)
    ref, bnd = H.head_ref(P, case, "f16")
    emu = H.head_emulate(P, case, "f16")
    assert H.ratio(emu["pre_c0"], ref["pre_c0"], bnd["pre_c0"]) <= 1.0
    u = H.U["f16"]
    S = P["feat"].to(F64).abs() @ P["c0_w"].to(F64).abs().t()
    assert H.ratio(emu["pre_c0"], ref["pre_c0"], 3 * u * u * S) > 1.0


@pytest.mark.parametrize("fault,precs,name,at,outs", H.HEAD_FAULT_CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_seeded_head_faults_leave_the_bound(fault, precs, name, at, outs):
    for prec in precs:
        case = _case(prec, name, 16 if prec != "f32" else 8)
        P = H.head_inputs(case)
        ref, bnd = H.head_ref(P, case, prec)
        r = H.worst(H.head_emulate(P, case, prec, fault, at), ref, bnd)
        print(f"{fault:20s} {prec:5s} {name:24s} " + "  ".join(f"{k} {r[k]:.3g}" for k in outs))
        assert all(not r[k] <= 1.0 for k in outs), (fault, prec, {k: r[k] for k in outs})


def test_seeded_training_faults_leave_the_bound():
    # swap biased / unbiased variance: BatchNorm forward at M = 2 .. 600
    for M, n in H.BN_SHAPES:
        x = H.bn_input(M, n)
        w, b, rm, rv = 1 + H.rand((n,), 1, 0.2), H.rand((n,), 2, 0.2), H.rand((n,), 3), 1 + H.rand((n,), 4).abs()
        ref, bnd = H.bn_fwd_ref(x, w, b, rm, rv)
        r = H.worst(H.bn_fwd_ref(x, w, b, rm, rv, "swap_variance")[0], ref, bnd)
        assert r["rstd"] > 1.0 and r["run_var"] > 1.0 and r["xhat"] > 1.0, (M, n, r)
    # act_bwd: keep_scale omitted; the tanh-form GELU derivative
    M, N = 33, 30
    dout, pre = H.rand((M, N), 5), H.rand((M, N), 6, 2.0)
    mask = (H.rand((M, N), 7) > -0.5).to(torch.uint8)
    ref, bnd = H.act_bwd_ref(dout, pre, "gelu", mask, 1.25)
    assert H.ratio(H.act_bwd_ref(dout, pre, "gelu", mask, 1.25, "no_keep_scale")[0], ref, bnd) > 1.0
    assert H.ratio(H.act_bwd_ref(dout, pre, "gelu", mask, 1.25, "tanh_gelu_grad")[0], ref, bnd) > 1.0
    # lin_bwd_w4's tail rows, at every M of the GPU file that has any; lin_bwd_w_kernel's db column
    for M, N, K in H.W4_SHAPES:
        d, x = H.rand((M, N), M + K, 0.1), H.rand((M, K), M * K)
        ref, bnd = H.lin_bwd_w_ref(d, x, 0)
        assert max(H.worst(H.lin_bwd_w_emulate(d, x, 0), ref, bnd).values()) <= 1.0
        r = H.worst(H.lin_bwd_w_emulate(d, x, 0, "drop_tail_rows_w4"), ref, bnd)
        if M != 32:   # (M = 32: every slice ends on a whole pair, the tail loop has no rows)
            assert r["dw"] > 1.0 and r["db"] > 1.0, (M, K, r)
    for kind, shapes in ((1, H.W464_SHAPES), (2, H.W1616_SHAPES)):
        for M, N, K in shapes:
            d, x = H.rand((M, N), M + K, 0.1), H.rand((M, K), M * K)
            ref, bnd = H.lin_bwd_w_ref(d, x, kind)
            assert max(H.worst(H.lin_bwd_w_emulate(d, x, kind), ref, bnd).values()) <= 1.0
            r = H.worst(H.lin_bwd_w_emulate(d, x, kind, "drop_db_column"), ref, bnd)
            assert r["db"] > 1.0 and r["dw"] <= 1.0, (kind, M, r)


def _fma32(a, b, c):
    """fp32 fma: the product and the sum in float64, one rounding"""
    return (a.double() * b.double() + c.double()).float()


def _four_chains(x, wt, bias):
    """lin_fwd_kernel / lin_bwd_in_kernel in fp32: x [M][K], wt [K][N]; four interleaved fma chains, (a0 + a1) + (a2 + a3)"""
    M, K = x.shape
    N = wt.shape[1]
    a = [bias.expand(M, N).clone() if bias is not None else torch.zeros(M, N)] + [torch.zeros(M, N) for _ in range(3)]
    k = 0
    while k + 3 < K:
        for j in range(4):
            a[j] = _fma32(x[:, k + j, None], wt[None, k + j], a[j])
        k += 4
    while k < K:
        a[0] = _fma32(x[:, k, None], wt[None, k], a[0])
        k += 1
    return (a[0] + a[1]) + (a[2] + a[3])


def test_fp32_emulations_of_the_training_kernels_within_bound():
    """the per-output kernels' own fp32 arithmetic (four fma chains), and torch's fp32 BatchNorm / LayerNorm / GELU' /
    sigmoid, at the shapes of the GPU file"""
    bad = []

    def check(label, got, ref, bnd):
        r = H.worst(got, ref, bnd) if isinstance(ref, dict) else {"": H.ratio(got, ref, bnd)}
        bad.extend(f"{label} {k}: {v:.3g}" for k, v in r.items() if not v <= 1.0)

    for M, N, K, _, _ in H.LIN_SHAPES:
        x, w, b = H.rand((M, K), 3 * M + K), H.rand((N, K), 5 * N + K, K ** -0.5), H.rand((N,), N, 0.2)
        pre = _four_chains(x, w.t().contiguous(), b)
        for act in H.ACTS:
            out = {"none": lambda t: t, "gelu": Fn.gelu, "relu": torch.relu}[act](pre)
            ref, bnd = H.lin_fwd_ref(x, w, b, act, None, 1.0, False)
            check(f"lin_fwd {M}x{N}x{K} {act}", dict(pre=pre, outa=out), ref, bnd)
        d = H.rand((M, N), 7 * M + N)
        ref, bnd = H.lin_bwd_in_ref(d, w, False)
        check(f"lin_bwd_in {M}x{N}x{K}", _four_chains(d, w, None), ref, bnd)
    for M, n in H.BN_SHAPES:
        x = H.bn_input(M, n)
        w, b, rm, rv = 1 + H.rand((n,), 1, 0.2), H.rand((n,), 2, 0.2), H.rand((n,), 3), 1 + H.rand((n,), 4).abs()
        rm_t, rv_t = rm.clone(), rv.clone()
        out = Fn.batch_norm(x, rm_t, rv_t, w, b, True, 0.1, 1e-5)
        ref, bnd = H.bn_fwd_ref(x, w, b, rm, rv)
        check(f"bn_fwd {M}x{n}", dict(out=out, run_mean=rm_t, run_var=rv_t), {k: ref[k] for k in ("out", "run_mean", "run_var")}, bnd)
    for M, F in H.FEAT_SHAPES:
        feat = H.rand((M, F), 9 * M + F) + 0.5
        hw, hb = 1 + H.rand((F,), F, 0.2), H.rand((F,), F + 1, 0.2)
        ref, bnd = H.feat_rows_ref(feat, hw, hb)
        check(f"feat_rows {M}x{F}", Fn.layer_norm(feat, (F,), hw, hb, 1e-6), ref, bnd)
    pre, dout = H.rand((33, 30), 1, 2.0), H.rand((33, 30), 3)
    p = pre.clone().requires_grad_()
    g, = torch.autograd.grad(Fn.gelu(p), p, dout)
    ref, bnd = H.act_bwd_ref(dout, pre, "gelu", None, 1.0)
    check("act_bwd gelu", g, ref, bnd)
    z = H.rand((257,), 257, 4.0)
    ref, bnd = H.logits_ref(z)
    check("sigmoid", torch.sigmoid(z), ref["scores"], bnd["scores"])
    assert not bad, "\n".join(bad)
