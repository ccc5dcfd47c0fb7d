"""The classifier-head kernels, each ALONE (btsbot_op_head, btsbot_op_ht_*: btsbot_amd/csrc/head_ops.hip) against float64
references with derived per-element bounds (tests/head_ref.py, whose docstring holds the derivation;
tests/test_head_reference.py shows on the CPU what the bounds see and which seeded faults leave them):

  head_kernel (dense_t<4> / dense_t<1>, store_rows) + transpose / bn_fold          test_head[f32-*]
  head16_kernel<bf16 / f16> (dense16, store_rows16) + pack_h16_kernel / bn_fold    test_head[bf16-*], test_head[f16-*]
  head16_supported's refusals                                                      test_head16_refusals
  lin_fwd_kernel | fp32 MFMA GEMM + act_fwd_kernel                                 test_lin_fwd, test_lin_wide
  lin_bwd_in_kernel | fp32 MFMA GEMM on the transposed image                       test_lin_bwd_in, test_lin_wide
  act_bwd_kernel                                                                   test_act_bwd
  lin_bwd_w4_kernel, lin_bwd_w_kernel<4, 64>, lin_bwd_w_kernel<16, 16>             test_lin_bwd_w
  bn_train_fwd_kernel, bn_train_bwd_kernel                                         test_bn
  feat_rows_kernel, logits_kernel, copy_cols_kernel                                test_feat_rows, test_logits_copy

Every output is a slice of a larger buffer whose head and tail hold a sentinel bit pattern that must survive; written
outputs are pre-filled with a value no result takes.  Which kernel a call takes is asserted through the library's
companions (ht_lin_is_wide, ht_lin_bwd_w_kind, head16_supported), not a mirrored formula.  Each test prints its worst
err / bound per output (run with -s) and asserts at the end.

Worst err / bound per kernel on an MI355X (a record, not a tolerance):
  head f32                 logits 0.006  scores 0.012  features 0.143  hidden 0.014
  head bf16                logits 0.005  scores 0.005  features 0.497  hidden 0.034
  head f16                 logits 0.003  scores 0.003  features 0.993  hidden 0.016
  lin_fwd                  outa 0.521  pre 0.476
  lin_bwd_in               din 0.207
  lin_fwd (MFMA GEMM)      outa 0.009  pre 0.009
  lin_bwd_in (MFMA GEMM)   din 0.037
  act_bwd                  dpre 0.488
  lin_bwd_w4               dw 0.152  db 0.054
  lin_bwd_w<4, 64>         dw 0.059  db 0.046
  lin_bwd_w<16, 16>        dw 0.178  db 0.090
  bn_fwd                   xhat 0.214  out 0.215  rstd 0.141  run_mean 0.238  run_var 0.293
  bn_bwd                   dw 0.128  db 0.093
  feat_rows                z 0.135
  logits                   logits 0.000  scores 0.440
(features of the 16-bit heads sit at their bound's edge by construction: the bound of an image feature that passes
through unnormalised is the hi + lo representation error alone.)
"""
import pytest
import torch

import head_ref as H
from btsbot_amd import _lib, ops

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
PAD = 1024
SENT = 0x7FC5A5A5
FILL = 7.0e3           # no result of these cases comes near it


def guarded(n, dev, fill=FILL, off=0):
    """[PAD sentinel | off + n floats = fill | PAD sentinel] -> (buffer, the last n floats of the middle)"""
    buf = torch.empty(n + off + 2 * PAD, dtype=F32, device=dev)
    buf.view(torch.int32).fill_(SENT)
    t = buf[PAD:PAD + off + n]
    if isinstance(fill, torch.Tensor):
        t[off:].copy_(fill.reshape(-1))
        t[:off].fill_(FILL)
    else:
        t.fill_(fill)
    return buf, t[off:]


def intact(buf, off=0):
    b = buf.view(torch.int32)
    return bool((b[:PAD] == SENT).all()) and bool((b[-PAD:] == SENT).all()) and bool((buf[PAD:PAD + off] == FILL).all())


class Log:
    def __init__(self):
        self.bad = []

    def check(self, case, got, ref, bound):
        r = {k: H.ratio(got[k].detach().cpu(), ref[k], bound[k]) for k in got}
        print(f"{case:58s} " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()) + "   (worst err / bound)")
        self.bad += [f"{case} {k}: err / bound = {v:.4g}" for k, v in r.items() if not v <= 1.0]
        return r

    def exact(self, case, what, ok):
        if not ok:
            print(f"{case:58s} {what}: NO")
            self.bad.append(f"{case}: {what}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


# ---------------------------------------------------------------------------------------------------------------------
# the inference heads
# ---------------------------------------------------------------------------------------------------------------------
def run_head(P, case, prec, dev, want=("features", "hidden"), scores=True, off=0):
    """-> (got, all sentinels intact); P on the CPU"""
    D = {k: v.to(dev) for k, v in P.items()}
    B, dims = case["B"], case["dims"]
    widths = dict(logits=1, scores=1, features=dims[0], hidden=dims[-2])
    bufs, out = {}, {}
    for k in ("logits",) + (("scores",) if scores else ()) + tuple(want):
        o = off if k in ("features", "hidden") else 0
        bufs[k], out[k] = guarded(B * widths[k], dev, off=o)
    nl = len(dims) - 1
    ops.head(prec, out["logits"], feat=D.get("feat"), hn=(D["hn_w"], D["hn_b"]) if case["hn"] else None, meta=D.get("meta"),
             bn=tuple(D[k] for k in ("bn_w", "bn_b", "bn_rm", "bn_rv")) if case["n_meta"] else None,
             m1=(D["m1_w"], D["m1_b"]) if case["n_meta"] else None, m2=(D["m2_w"], D["m2_b"]) if case["n_meta"] else None,
             meta_trailing_act=case["trailing"], comb=tuple((D[f"c{i}_w"], D[f"c{i}_b"]) for i in range(nl)), act=case["act"],
             scores=out.get("scores"), features=out.get("features"), hidden=out.get("hidden"))
    torch.cuda.synchronize()
    whole = all(intact(b, off if k in ("features", "hidden") else 0) for k, b in bufs.items())
    return {k: v.view(B, widths[k]) if widths[k] > 1 else v for k, v in out.items()}, whole


def check_head(log, label, P, case, prec, dev, **kw):
    ref, bnd = H.head_ref(P, case, prec)
    got, whole = run_head(P, case, prec, dev, **kw)
    r = log.check(label, got, ref, bnd)
    log.exact(label, "sentinels intact", whole)
    return got, r


@pytest.mark.parametrize("prec,name", [(p, n) for p in H.PRECS3 for n in H.head_cases(p)])
def test_head(cuda, prec, name):
    """every wiring at the product's widths and the edge widths of the precision, at every row count around the
    workgroup's alerts; features and hidden requested together"""
    log = Log()
    for B in H.batch_sizes(prec):
        case = H.head_case(B=B, seed=3, **H.head_cases(prec)[name])
        if prec != "f32":
            assert ops.head16_supported(prec, case["F"], case["n_meta"], case["f1"], case["f2"], case["dims"])
        check_head(log, f"head {prec} {name} B={B}", H.head_inputs(case), case, prec, cuda)
    log.done()


@pytest.mark.parametrize("prec", H.PRECS3)
def test_head_embedding_requests(cuda, prec):
    """features / hidden each alone, not at all, both 4 bytes off a 16-byte boundary (the dword store paths), scores null"""
    log = Log()
    names = ("image+meta", "ragged image+ln+meta" if prec == "f32" else "F8 meta32 f1=16 f2=24")
    for name in names:
        case = H.head_case(B=9 if prec == "f32" else 17, seed=4, **H.head_cases(prec)[name])
        P = H.head_inputs(case)
        for want, sc, off in ((("features",), True, 0), (("hidden",), True, 0), ((), True, 0), (("features", "hidden"), True, 1),
                              (("features", "hidden"), False, 0)):
            check_head(log, f"head {prec} {name} {'+'.join(want) or 'no rows'}{' off 4 B' if off else ''}{'' if sc else ' no scores'}",
                       P, case, prec, cuda, want=want, scores=sc, off=off)
    log.done()


@pytest.mark.parametrize("prec", H.PRECS3)
def test_head_saturated_scores(cuda, prec):
    """logits of +-100 (the last bias): scores exactly 1 / 0, everything finite"""
    log = Log()
    for sign in (1.0, -1.0):
        case = H.head_case(B=17, seed=5, **H.head_cases(prec)["image+meta"])
        P = H.head_inputs(case)
        P["c2_b"] = torch.full_like(P["c2_b"], 100.0 * sign)
        got, _ = check_head(log, f"head {prec} logits {100 * sign:+.0f}", P, case, prec, cuda)
        log.exact("saturated", "scores exactly 0 / 1", bool((got["scores"] == (1.0 if sign > 0 else 0.0)).all()))
        log.exact("saturated", "finite", all(bool(torch.isfinite(v).all()) for v in got.values()))
        assert (got["logits"].abs() > 90).all()
    log.done()


@pytest.mark.parametrize("prec", ("bf16", "f16"))
@pytest.mark.parametrize("name", list(H.H16_REFUSED))
def test_head16_refusals(cuda, prec, name):
    kw, word = H.H16_REFUSED[name]
    case = H.head_case(B=5, seed=6, **kw)
    assert not ops.head16_supported(prec, case["F"], case["n_meta"], case["f1"], case["f2"], case["dims"])
    P = H.head_inputs(case)
    widths = dict(logits=1, scores=1, features=case["dims"][0], hidden=case["dims"][-2])
    bufs = {k: guarded(5 * w, cuda) for k, w in widths.items()}
    with pytest.raises(_lib.BtsbotHipError, match=word):
        D = {k: v.to(cuda) for k, v in P.items()}
        nl = len(case["dims"]) - 1
        ops.head(prec, bufs["logits"][1], feat=D.get("feat"), meta=D.get("meta"),
                 bn=tuple(D[k] for k in ("bn_w", "bn_b", "bn_rm", "bn_rv")) if case["n_meta"] else None,
                 m1=(D["m1_w"], D["m1_b"]) if case["n_meta"] else None, m2=(D["m2_w"], D["m2_b"]) if case["n_meta"] else None,
                 comb=tuple((D[f"c{i}_w"], D[f"c{i}_b"]) for i in range(nl)), scores=bufs["scores"][1],
                 features=bufs["features"][1], hidden=bufs["hidden"][1])
    torch.cuda.synchronize()
    for k, (buf, t) in bufs.items():
        assert intact(buf) and bool((t == FILL).all()), k    # nothing written, no fp32 head in its place


# ---------------------------------------------------------------------------------------------------------------------
# the training kernels
# ---------------------------------------------------------------------------------------------------------------------
def strided(M, width, extra, dev, fill=FILL):
    """a guarded [M][width + extra] buffer -> (buffer, the whole rows, the [M, width] view)"""
    buf, flat = guarded(M * (width + extra), dev, fill=fill)
    rows = flat.view(M, width + extra)
    return buf, rows, rows[:, :width]


def pad_kept(rows, width):
    return bool((rows[:, width:] == FILL).all())


def lin_inputs(M, N, K, dev):
    return (H.rand((M, K), 3 * M + K, dev=dev), H.rand((N, K), 5 * N + K, K ** -0.5, dev=dev), H.rand((N,), N, 0.2, dev=dev),
            (H.rand((M, N), M + N) > -0.5).to(torch.uint8).to(dev))


def test_lin_fwd(cuda):
    log = Log()
    for M, N, K, xi, xo in H.LIN_SHAPES:
        assert M * N % 256 != 0 and not ops.ht_lin_is_wide(M, N, K, K + xi)
        x, w, b, mask = lin_inputs(M, N, K, cuda)
        xb, xrows, xv = strided(M, K, xi, cuda)
        xv.copy_(x)
        for act in H.ACTS:
            for mk, keep, with_pre in ((None, 1.0, True), (mask, 1.25, True), (mask, 1.25, False)):
                ob, orows, ov = strided(M, N, xo, cuda)
                pb, pre = guarded(M * N, cuda)
                ops.ht_lin_fwd(xv, w, b, ov, pre=pre.view(M, N) if with_pre else None, act=act, mask=mk, keep_scale=keep)
                torch.cuda.synchronize()
                ref, bnd = H.lin_fwd_ref(x.cpu(), w.cpu(), b.cpu(), act, None if mk is None else mk.cpu(), keep, False)
                label = f"lin_fwd {M}x{N}x{K} ldi+{xi} ldo+{xo} {act}{' mask' if mk is not None else ''}{'' if with_pre else ' no pre'}"
                got = dict(outa=ov, pre=pre.view(M, N)) if with_pre else dict(outa=ov)
                log.check(label, got, ref, bnd)
                log.exact(label, "guards and row padding intact", intact(ob) and intact(pb) and pad_kept(orows, N)
                          and (with_pre or bool((pre == FILL).all())))
    log.done()


def test_lin_bwd_in(cuda):
    log = Log()
    for M, N, K, xi, _ in H.LIN_SHAPES:
        assert not ops.ht_lin_is_wide(M, K, N, N)
        d, w = H.rand((M, N), 7 * M + N, dev=cuda), H.rand((N, K), 5 * N + K, K ** -0.5, dev=cuda)
        for extra in sorted({0, xi}):
            ob, orows, ov = strided(M, K, extra, cuda)
            ops.ht_lin_bwd_in(d, w, ov)
            torch.cuda.synchronize()
            ref, bnd = H.lin_bwd_in_ref(d.cpu(), w.cpu(), False)
            label = f"lin_bwd_in {M}x{N}x{K} ldi+{extra}"
            log.check(label, dict(din=ov), dict(din=ref), dict(din=bnd))
            log.exact(label, "guards and row padding intact", intact(ob) and pad_kept(orows, K))
    log.done()


def test_lin_wide(cuda):
    """(255, 128, 512) and (256, 128, 512): the two sides of M N K = 2^24, each held to its own path's bound"""
    log = Log()
    for M, N, K in H.LIN_WIDE:
        wide = M * N * K >= 1 << 24
        assert ops.ht_lin_is_wide(M, N, K, K) == wide and ops.ht_lin_is_wide(M, K, N, N) == wide
        x, w, b, mask = lin_inputs(M, N, K, cuda)
        for act, mk, with_pre in (("gelu", mask, True), ("none", None, False)):
            ob, out = guarded(M * N, cuda)
            pb, pre = guarded(M * N, cuda)
            ops.ht_lin_fwd(x, w, b, out.view(M, N), pre=pre.view(M, N) if with_pre else None, act=act, mask=mk, keep_scale=1.25)
            torch.cuda.synchronize()
            ref, bnd = H.lin_fwd_ref(x.cpu(), w.cpu(), b.cpu(), act, None if mk is None else mk.cpu(), 1.25, wide)
            label = f"lin_fwd {'wide' if wide else 'per-output'} {M}x{N}x{K} {act}"
            got = dict(outa=out.view(M, N), pre=pre.view(M, N)) if with_pre else dict(outa=out.view(M, N))
            log.check(label, got, ref, bnd)
            log.exact(label, "guards intact", intact(ob) and intact(pb) and (with_pre or bool((pre == FILL).all())))
        d = H.rand((M, N), M, dev=cuda)
        ob, out = guarded(M * K, cuda)
        ops.ht_lin_bwd_in(d, w, out.view(M, K))
        torch.cuda.synchronize()
        ref, bnd = H.lin_bwd_in_ref(d.cpu(), w.cpu(), wide)
        label = f"lin_bwd_in {'wide' if wide else 'per-output'} {M}x{N}x{K}"
        log.check(label, dict(din=out.view(M, K)), dict(din=ref), dict(din=bnd))
        log.exact(label, "guards intact", intact(ob))
    log.done()


def test_act_bwd(cuda):
    log = Log()
    M, N = 33, 30
    pre = H.rand((M, N), 1, 2.0, dev=cuda)
    mask = (H.rand((M, N), 2) > -0.5).to(torch.uint8).to(cuda)
    dout = H.rand((M, N), 3, dev=cuda)
    for act in H.ACTS:
        for mk, keep in ((None, 1.0), (mask, 1.25)):
            ref, bnd = H.act_bwd_ref(dout.cpu(), pre.cpu(), act, None if mk is None else mk.cpu(), keep)
            # dout in rows 5 floats wider than N, into its own output
            db_, drows, dv = strided(M, N, 5, cuda)
            dv.copy_(dout)
            ob, out = guarded(M * N, cuda)
            ops.ht_act_bwd(dv, pre, out.view(M, N), act=act, mask=mk, keep_scale=keep)
            torch.cuda.synchronize()
            label = f"act_bwd {act}{' mask' if mk is not None else ''} ldd+5"
            log.check(label, dict(dpre=out.view(M, N)), dict(dpre=ref), dict(dpre=bnd))
            log.exact(label, "guards intact, dout untouched", intact(ob) and intact(db_) and torch.equal(dv, dout) and pad_kept(drows, N))
            # in place
            ib, io = guarded(M * N, cuda, fill=dout)
            ops.ht_act_bwd(io.view(M, N), pre, io.view(M, N), act=act, mask=mk, keep_scale=keep)
            torch.cuda.synchronize()
            label = f"act_bwd {act}{' mask' if mk is not None else ''} in place"
            log.check(label, dict(dpre=io.view(M, N)), dict(dpre=ref), dict(dpre=bnd))
            log.exact(label, "guards intact", intact(ib))
    log.done()


def run_lin_bwd_w(log, M, N, K, kind, dev, off=0, extra=0):
    d = H.rand((M, N), M + K, 0.1, dev=dev)
    xb, xflat = guarded(M * (K + extra), dev, off=off)
    xrows = xflat.view(M, K + extra)
    x = xrows[:, :K]
    x.copy_(H.rand((M, K), M * K, dev=dev))
    wb, dw = guarded(N * K, dev)
    bb, db = guarded(N, dev)
    assert ops.ht_lin_bwd_w_kind(x, dw.view(N, K)) == kind, (M, N, K, off, extra)
    ops.ht_lin_bwd_w(d, x, dw.view(N, K), db)
    torch.cuda.synchronize()
    ref, bnd = H.lin_bwd_w_ref(d.cpu(), x.cpu(), kind)
    label = f"lin_bwd_w kind {kind} {M}x{N}x{K}{' in off 4 B' if off else ''}{f' ldi+{extra}' if extra else ''}"
    log.check(label, dict(dw=dw.view(N, K), db=db), ref, bnd)
    log.exact(label, "guards intact", intact(wb) and intact(bb))


def test_lin_bwd_w(cuda):
    log = Log()
    for M, N, K in H.W4_SHAPES:
        run_lin_bwd_w(log, M, N, K, 0, cuda)
    run_lin_bwd_w(log, 33, 5, 68, 0, cuda, extra=4)        # w4 through a row stride
    for M, N, K in H.W464_SHAPES:
        run_lin_bwd_w(log, M, N, K, 1, cuda)
    for M, N, K in H.W1616_SHAPES:
        run_lin_bwd_w(log, M, N, K, 2, cuda)
    run_lin_bwd_w(log, 33, 5, 64, 1, cuda, off=1)          # K % 4 == 0 with `in` off 16 bytes: leaves w4, still right
    run_lin_bwd_w(log, 17, 5, 64, 1, cuda, extra=1)        # ... and with a row stride that is no multiple of 4
    log.done()


def test_bn(cuda):
    log = Log()
    for M, n in H.BN_SHAPES:
        x = H.bn_input(M, n, cuda)
        w, b = 1 + H.rand((n,), 1, 0.2, dev=cuda), H.rand((n,), 2, 0.2, dev=cuda)
        rm0, rv0 = H.rand((n,), 3), 1 + H.rand((n,), 4).abs()
        for running in (True, False):
            bufs = {k: guarded(s, cuda) for k, s in (("xhat", M * n), ("out", M * n), ("rstd", n))}
            if running:
                bufs["run_mean"], bufs["run_var"] = guarded(n, cuda, fill=rm0), guarded(n, cuda, fill=rv0)
            t = {k: v[1] for k, v in bufs.items()}
            ops.ht_bn_fwd(x, w, b, t["xhat"].view(M, n), t["out"].view(M, n), t["rstd"], t.get("run_mean"), t.get("run_var"))
            torch.cuda.synchronize()
            ref, bnd = H.bn_fwd_ref(x.cpu(), w.cpu(), b.cpu(), rm0 if running else None, rv0 if running else None)
            label = f"bn_fwd {M}x{n}{' running' if running else ''}"
            log.check(label, t, ref, bnd)
            log.exact(label, "guards intact", all(intact(v[0]) for v in bufs.values()))
        dy = H.rand((M, n), 5 * M, dev=cuda)
        xhat = t["xhat"].view(M, n).clone()
        (wb, dw), (bb, db) = guarded(n, cuda), guarded(n, cuda)
        ops.ht_bn_bwd(dy, w, xhat, t["rstd"].clone(), dw, db)
        torch.cuda.synchronize()
        ref, bnd = H.bn_bwd_ref(dy.cpu(), xhat.cpu())
        log.check(f"bn_bwd {M}x{n}", dict(dw=dw, db=db), ref, bnd)
        log.exact(f"bn_bwd {M}x{n}", "guards intact", intact(wb) and intact(bb))
    log.done()


def test_bn_one_row(cuda):
    """M = 1, what the kernel does: xhat = 0 and out = b exactly, rstd = (1e-5)^-1/2, and the BIASED variance (0) goes into
    running_var where torch's unbiased one does not exist"""
    n = 25
    x = H.bn_input(1, n, cuda)
    w, b = 1 + H.rand((n,), 1, 0.2, dev=cuda), H.rand((n,), 2, 0.2, dev=cuda)
    rm0, rv0 = H.rand((n,), 3), 1 + H.rand((n,), 4).abs()
    bufs = {k: guarded(n, cuda, fill=f) for k, f in (("xhat", FILL), ("out", FILL), ("rstd", FILL), ("rm", rm0), ("rv", rv0))}
    t = {k: v[1] for k, v in bufs.items()}
    ops.ht_bn_fwd(x, w, b, t["xhat"].view(1, n), t["out"].view(1, n), t["rstd"], t["rm"], t["rv"])
    torch.cuda.synchronize()
    ref, bnd = H.bn_fwd_ref(x.cpu(), w.cpu(), b.cpu(), rm0, rv0)
    assert all(bool(torch.isfinite(v).all()) for v in t.values()) and all(intact(v[0]) for v in bufs.values())
    assert not t["xhat"].any() and torch.equal(t["out"], b)
    log = Log()
    log.check("bn_fwd 1x25", dict(rstd=t["rstd"], run_mean=t["rm"], run_var=t["rv"]), ref, bnd)
    log.done()


def test_feat_rows(cuda):
    log = Log()
    for M, F in H.FEAT_SHAPES:
        feat = H.rand((M, F), 9 * M + F, dev=cuda) + 0.5
        hw, hb = 1 + H.rand((F,), F, 0.2, dev=cuda), H.rand((F,), F + 1, 0.2, dev=cuda)
        for ln in (True, False):
            for extra in (0, 6):
                zb, zrows, zv = strided(M, F, extra, cuda)
                ops.ht_feat_rows(feat, zv, hn=(hw, hb) if ln else None)
                torch.cuda.synchronize()
                ref, bnd = H.feat_rows_ref(feat.cpu(), hw.cpu() if ln else None, hb.cpu() if ln else None)
                label = f"feat_rows {M}x{F}{' LN' if ln else ''} ldz+{extra}"
                log.check(label, dict(z=zv), dict(z=ref), dict(z=bnd))
                log.exact(label, "guards and row padding intact", intact(zb) and pad_kept(zrows, F))
                if not ln:
                    log.exact(label, "the copy is exact", torch.equal(zv, feat))
    log.done()


def test_logits_copy(cuda):
    log = Log()
    for M in H.LOGIT_ROWS:
        x = H.rand((M,), M, 4.0, dev=cuda)
        for with_scores in (True, False):
            (lb, lg), (sb, sc) = guarded(M, cuda), guarded(M, cuda)
            ops.ht_logits(x, lg, sc if with_scores else None)
            torch.cuda.synchronize()
            ref, bnd = H.logits_ref(x.cpu())
            label = f"logits {M}{'' if with_scores else ' no scores'}"
            log.check(label, dict(logits=lg, scores=sc) if with_scores else dict(logits=lg), ref, bnd)
            log.exact(label, "guards intact", intact(lb) and intact(sb) and (with_scores or bool((sc == FILL).all())))
    M, cols = 37, 21
    sb_, srows, sv = strided(M, cols, 3, cuda)
    sv.copy_(H.rand((M, cols), 1, dev=cuda))
    db_, drows, dv = strided(M, cols, 7, cuda)
    ops.ht_copy_cols(dv, sv)
    torch.cuda.synchronize()
    log.exact("copy_cols 37x21 lds+3 ldd+7", "exact, guards and row padding intact",
              torch.equal(dv, sv) and intact(db_) and intact(sb_) and pad_kept(drows, cols) and pad_kept(srows, cols))
    log.done()
