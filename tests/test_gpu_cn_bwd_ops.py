"""The LayerNorm / depthwise backward kernels of the ConvNeXt training step, each ALONE (btsbot_op_cnt_*,
btsbot_amd/csrc/cn_bwd_ops.hip) against torch's float64 autograd on the CPU (tests/cn_bwd_ref.py):

  dwln_bwd_kernel<15,64>, <7,128>, <3,256,512,4> + the fp32 column sum     test_dwln_bwd, test_general_3x3_*
  dw3ln_bwd_kernel + dw3_rows_kernel (1, 1, 4, 8 slices)                   test_dw3ln_bwd
  ln_bwd_narrow_kernel<16|32>, ln_bwd_kernel<2|4|5|8|10>                   test_ln_bwd_dense, test_ln_bwd_patch_gather
  ln_dw1_bwd_kernel<8|10>                                                  test_ln_dw1_bwd
  dw_plain_kernel<15|7|3|1>, dw_wgrad_kernel<15|7|3|1> + its column sum    test_dw_plain, test_dw_wgrad
  colsum_kernel<float>                                                     test_colsum_f32

Every output is compared as a whole tensor, err = max|got - ref64| / max|ref64|, the input gradient dy included.
Outputs the kernels ADD to (dy, the arena's gradients) are pre-filled with non-zero values and compared with
pre-fill + gradient; outputs they WRITE (dd, dw_plain's out, every 16-bit copy) are pre-filled with other values.

Bound of an fp32 output: 4 x e32, e32 = the error of the SAME autograd run in float32 on the CPU for the same inputs
(cn_bwd_ref.MARGIN); nothing in it depends on the kernels.  16-bit copies and "untouched" claims are exact.  Every
figure is printed (run with -s): the log is the record.  tests/test_cn_bwd_reference.py shows on the CPU that these
bounds see a shifted tap, unflipped taps, a dropped alert or plane, an un-zeroed odd row, eps = 1e-5 and a mean over
C - 1 channels with a factor >= 10 to spare.

Two classes of cases measure above 4 x e32 on an MI355X; their bound is 2 x the largest measured error of the class
(cn_bwd_ref.MEASURED; 4 x e32 where that is larger), and the fault tests hold at it:

  class (output)                      largest measured err    e32 of those cases     4 x e32 missed by at most
  dw_plain with an addend, 15x15x64   4.277e-07               6.9e-08 .. 9.8e-08     1.19 x
                           15x15x80   3.618e-07               7.1e-08 .. 1.1e-07     1.25 x
                           7x7x128    3.482e-07               5.3e-08 .. 7.5e-08     1.58 x
                           7x7x160    3.467e-07               6.1e-08 .. 8.8e-08     1.23 x
                           3x3x256    1.966e-07               3.5e-08 .. 4.3e-08     1.32 x
                           3x3x320    1.969e-07               3.3e-08 .. 5.3e-08     1.37 x
  ln_bwd_kernel<CPT>, 2051 rows: dg   9.721e-07               1.7e-07 .. 5.1e-07     1.32 x
                              dbeta   8.531e-07               1.9e-07 .. 3.0e-07     1.04 x
  (1x1 maps' dw_plain and every case without an addend stay inside 4 x e32.)

  dw_plain_kernel starts each output from bias + addend (the load is requested before the taps run) and adds the 49 tap
  products to it one fmaf at a time, so every one of them is rounded at the addend's magnitude (|addend| up to 4.6
  against conv terms of ~0.1); torch sums the convolution at its own magnitude and rounds at the addend's once.  The
  figures are the same in every run.
  ln_bwd_kernel at 2051 rows runs 512 workgroups, each of which adds its dg / dbeta to the same 2 C addresses with one
  atomic: a chain of 512 fp32 additions per channel in arrival order, against torch's vectorised pairwise column sum.
  The order changes from run to run: over four runs of the twelve (width, placement) cases, which of them missed
  4 x e32 changed (C = 256 twice, C = 512 once, none once), so the class shares one figure: the largest of the 48.  The narrow kernels' cases (16 417 / 8 209 rows) have e32 of 4e-07 .. 6e-07 and stay inside.

Batch sizes are the smallest that reach a path; where a path depends on the launcher's grouping, the test asserts
from the row-count companions that the case still reaches it.
"""
import ctypes

import pytest
import torch

import cn_bwd_ref as R
from btsbot_amd import _lib, ops

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
BF16, F16 = torch.bfloat16, torch.float16

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class Log:
    """prints err / e32 / bound of every output, fails at the end so that the log holds every figure"""

    def __init__(self):
        self.bad = []

    def check(self, case, got, ref64, e32, cls=None):
        for k in ref64:
            err, b = R.rel_err(got[k].detach().cpu().reshape(ref64[k].shape), ref64[k]), R.bound(cls, k, e32[k])
            print(f"{case:34s} {k:6s} err {err:.3e}  e32 {e32[k]:.3e}  bound {b:.3e}  ({err / b:5.2f} x bound)")
            if not err <= b:
                self.bad.append(f"{case} {k}: err {err:.3e} > bound {b:.3e} (e32 {e32[k]:.3e})")

    def exact(self, case, what, ok):
        print(f"{case:34s} {what}: {'exact' if ok else 'DIFFERS'}")
        if not ok:
            self.bad.append(f"{case}: {what}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def arena_views(arena, C):
    return dict(dW=arena[:49 * C].view(C, 49), db=arena[49 * C:50 * C], dg=arena[50 * C:51 * C], dbeta=arena[51 * C:])


def block_case(HW, C, B, planes, const_row=None):
    """inputs, the float64 outputs (dy and the arena block, pre-fill included) and e32.  const_row = (alert, pixel):
    that row of the kept depthwise output is the constant 0.75 (variance exactly 0)."""
    def make():
        inp = R.block_inputs(HW, C, B, planes)
        inp["a0"] = 0.05 * torch.randn(52 * C, generator=torch.Generator().manual_seed(HW * C + B))
        d_in = None
        if const_row is not None:
            inp["d"][const_row[0]].view(HW * HW, C)[const_row[1]] = 0.75
            d_in = inp["d"]
        outs = []
        for t in (F64, F32):
            r = R.block_ref(inp, t, d_in)
            outs.append(dict(dy=r["dy"], **R.arena_ref(r, inp["a0"], t)))
            if t == F64:
                inp["dd64"] = r["dd"]
        return inp, outs[0], R.e32_of(outs[1], outs[0])
    return cached(("block", HW, C, B, planes, const_row), make)


def run_fused(op, inp, o16, dev):
    """op: 'dwln' (the general kernel), 'dw3' (the 3x3 kernel) or 'dw1' (1x1 maps) -> the fp32 outputs by name, arena"""
    C = inp["x"].shape[-1]
    t = {k: inp[k].to(dev) for k in ("x", "w", "bias", "g", "dxn", "d")}
    dy, arena = inp["dy0"].to(dev).clone(), inp["a0"].to(dev).clone()
    out16 = None if o16 is None else torch.full(inp["dy0"].shape, 7.0, dtype=o16, device=dev)
    if op == "dwln":
        ops.cnt_dwln_bwd(t["d"], t["dxn"], t["g"], t["x"], t["w"], dy, arena, out16)
    elif op == "dw3":
        ops.cnt_dw3ln_bwd(t["bias"], t["dxn"], t["g"], t["x"], t["w"], dy, arena, out16)
    else:
        v = arena_views(arena, C)
        ops.cnt_ln_dw1_bwd(t["d"].view(-1, C), t["dxn"].view(-1, C), t["g"], t["x"].view(-1, C), t["w"], dy.view(-1, C),
                           v["dg"], v["dbeta"], v["dW"], v["db"], None if out16 is None else out16.view(-1, C))
    torch.cuda.synchronize()
    got = dict(dy=dy, **arena_views(arena, C))
    return got, arena, (None if out16 is None else torch.equal(out16, dy.to(o16)))


def passes(B, rows, NA=4):
    """alerts per pass of dwln_bwd_kernel<3,256,512,4> (NA alerts share a pass), over all its workgroups"""
    ga = -(-B // rows)
    assert (rows - 1) * ga < B <= rows * ga   # rows workgroups of ga consecutive alerts, the last one what is left
    seen = set()
    for n in {ga, B - (rows - 1) * ga}:
        seen |= {NA} if n >= NA else set()
        seen |= {n % NA} - {0}
    return ga, B - (rows - 1) * ga, seen


# (HW, C, B, planes, 16-bit copy): every shape with planes 1 and 4 and with no / a bf16 / an f16 copy
DWLN_CASES = [(15, 64, 1, 1, None), (15, 64, 1, 4, BF16), (15, 64, 3, 4, F16), (15, 64, 257, 1, BF16),
              (7, 128, 1, 1, None), (7, 128, 1, 4, F16), (7, 128, 513, 4, BF16),
              (3, 256, 1, 1, None), (3, 256, 1, 4, BF16), (3, 256, 769, 1, F16), (3, 256, 1281, 4, None),
              (3, 256, 1537, 1, BF16)]


@pytest.mark.parametrize("HW,C,B,planes,o16", DWLN_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_dwln_bwd(cuda, HW, C, B, planes, o16):
    rows = ops.cnt_dwln_bwd_rows(HW, C, B)
    if B > 256:   # several alerts per workgroup, the last workgroup short
        ga = -(-B // rows)
        assert rows < B and ga >= 2 and 0 < B - (rows - 1) * ga < ga, (rows, B)
    else:
        assert rows == B
    inp, ref, e32 = block_case(HW, C, B, planes)
    case = f"dwln-{HW}x{C}-B{B}-p{planes}"
    log = Log()
    got, _, same16 = run_fused("dwln", inp, o16, cuda)
    log.check(case, got, ref, e32)
    if o16 is not None:
        log.exact(case, f"out16 == {o16} cast of the dy this launch wrote", same16)
    log.done()


def test_general_3x3_kernel_runs_passes_of_one_to_four_alerts():
    """dwln_bwd_kernel<3,256,512,4> takes four alerts per pass: test_dwln_bwd's batch sizes must give passes of 4, 4 + 2
    and 4 + 3 alerts with short last workgroups of 1, 3 and 4 -- from the launcher's own row count."""
    seen, groups = set(), {}
    for B in (1, 769, 1281, 1537):
        ga, last, s = passes(B, ops.cnt_dwln_bwd_rows(3, 256, B))
        groups[B] = (ga, last)
        seen |= s
    print(f"(alerts per workgroup, alerts of the last workgroup) by batch: {groups}; pass sizes seen: {sorted(seen)}")
    assert groups == {1: (1, 1), 769: (4, 1), 1281: (6, 3), 1537: (7, 4)}
    assert seen == {1, 2, 3, 4}


@pytest.mark.parametrize("B,planes,o16", [(1, 1, None), (1, 4, BF16), (5, 4, F16), (40, 1, BF16), (513, 4, None), (513, 1, F16)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_dw3ln_bwd(cuda, B, planes, o16):
    """The 3x3 kernel with its row reduction (1, 5, 40, 257 partial rows: 1, 1, 4, 8 slices, the last two meeting through
    atomics) and the general kernel on the same inputs, each against the same reference."""
    rows = ops.cnt_dw3ln_bwd_rows(B)
    assert rows == {1: 1, 5: 5, 40: 40, 513: 257}[B]
    inp, ref, e32 = block_case(3, 256, B, planes)
    log = Log()
    live = torch.zeros(7, 7, dtype=torch.bool)
    live[1:6, 1:6] = True   # the taps that meet a 3x3 map
    for op in ("dw3", "dwln"):
        case = f"{op}-3x256-B{B}-p{planes}"
        got, arena, same16 = run_fused(op, inp, o16, cuda)
        log.check(case, got, ref, e32)
        if o16 is not None:
            log.exact(case, f"out16 == {o16} cast of the dy this launch wrote", same16)
        if op == "dw3":
            outer = ~live.view(49)
            log.exact(case, "the 24 taps outside the central 5x5 keep their pre-filled value",
                      torch.equal(got["dW"].cpu()[:, outer], inp["a0"][:49 * 256].view(256, 49)[:, outer]))
    log.done()


@pytest.mark.parametrize("op,HW,C", [("dwln", 15, 64), ("dwln", 7, 128), ("dwln", 3, 256), ("dw1", 1, 512), ("dw1", 1, 640)])
def test_fused_kernels_with_a_row_of_constant_d(cuda, op, HW, C):
    """One row of the kept depthwise output is constant: variance exactly 0, rstd = eps^-1/2 = 1000."""
    row = (1, (HW * HW) // 2)
    inp, ref, e32 = block_case(HW, C, 2, 1, const_row=row)
    want = R.const_row_dd(inp["g"], inp["dxn"][0][row[0]].view(-1, C)[row[1]])
    assert R.rel_err(inp["dd64"][row[0]].reshape(-1, C)[row[1]], want) <= 1e-9   # the reference gives the closed form
    log = Log()
    got, _, _ = run_fused(op, inp, None, cuda)
    log.check(f"{op}-{HW}x{C}-constrow", got, ref, e32)
    log.done()


def test_dw3ln_bwd_with_an_alert_of_constant_d(cuda):
    """The 3x3 kernel recomputes d: an all-zero alert under a constant depthwise bias gives nine rows of variance 0."""
    def make():
        inp = R.block_inputs(3, 256, 2, 1, seed=3)
        inp["x"][0] = 0.0
        inp["bias"][:] = 0.75
        inp["d"] = R.kept_d(inp)
        assert bool((inp["d"][0] == 0.75).all())
        inp["a0"] = 0.05 * torch.randn(52 * 256, generator=torch.Generator().manual_seed(9))
        outs = []
        for t in (F64, F32):
            r = R.block_ref(inp, t)
            outs.append(dict(dy=r["dy"], **R.arena_ref(r, inp["a0"], t)))
            if t == F64:
                inp["dd64"] = r["dd"]
        return inp, outs[0], R.e32_of(outs[1], outs[0])
    inp, ref, e32 = cached("dw3const", make)
    for p in range(9):
        want = R.const_row_dd(inp["g"], inp["dxn"][0][0].view(9, 256)[p])
        assert R.rel_err(inp["dd64"][0].reshape(9, 256)[p], want) <= 1e-9
    log = Log()
    for op in ("dw3", "dwln"):
        got, _, _ = run_fused(op, inp, None, cuda)
        log.check(f"{op}-3x256-constalert", got, ref, e32)
    log.done()


# ---- LayerNorm backward alone
def ln_case(C, rows, const_row=None, patch=None):
    def make():
        g = torch.Generator().manual_seed(7919 * C + rows + (patch[0] if patch else 0))
        d, gam = R.rows_like(g, rows, C), R.signed(g, C)
        if const_row is not None:
            d[const_row] = 0.75
        if patch:
            hw, B = patch
            dxn = torch.randn(B * (hw // 2) ** 2, 4 * C, generator=g)
        else:
            dxn = torch.randn(rows, C, generator=g)
        pre = 0.05 * torch.randn(2, C, generator=g)
        r64, r32 = (R.ln_ref(d, gam, dxn, t, patch[0] if patch else 0, pre[0], pre[1]) for t in (F64, F32))
        return dict(d=d, g=gam, dxn=dxn, pre=pre), r64, R.e32_of(r32, r64)
    return cached(("ln", C, rows, const_row, patch), make)


def run_ln(inp, dev, in_place, o16, patch_hw=0):
    d, gam, dxn = inp["d"].to(dev), inp["g"].to(dev), inp["dxn"].to(dev).clone()
    dg, dbeta = inp["pre"][0].to(dev).clone(), inp["pre"][1].to(dev).clone()
    dd = dxn if in_place else torch.full_like(d, 7.0)
    out16 = None if o16 is None else torch.full(d.shape, 7.0, dtype=o16, device=dev)
    ops.cnt_ln_bwd(d, dxn, gam, dd, dg, dbeta, out16, patch_hw)
    torch.cuda.synchronize()
    return dict(dd=dd, dg=dg, dbeta=dbeta), (None if out16 is None else torch.equal(out16, dd.to(o16)))


@pytest.mark.parametrize("C", R.LN_WIDTHS)
def test_ln_bwd_dense(cuda, C):
    """ln_bwd_narrow_kernel<16|32> (C = 64, 128) and ln_bwd_kernel<CPT> (80, 160, 256, 320, 512, 640: CPT 2, 4, 4, 5, 8,
    10).  Rows: 1, 5, a count that is no multiple of the rows of a block pass (32 / 16 / 4), and one past the 512
    workgroups x rows per pass, where the grid-stride loop makes a second trip; in place (dd = dxn) and out of place."""
    per = 32 if C == 64 else 16 if C == 128 else 4
    log = Log()
    ragged, second_trip = 3 * per + per // 2 + 1, 512 * per + (per + 1 if per > 4 else 3)
    for rows in (1, 5, ragged, second_trip):
        inp, ref, e32 = ln_case(C, rows)
        for in_place in (False, True):
            o16 = (F16 if in_place else BF16) if rows == ragged else None
            got, same16 = run_ln(inp, cuda, in_place, o16)
            case = f"ln-{C}-rows{rows}-{'inplace' if in_place else 'outofplace'}"
            log.check(case, got, ref, e32, "ln-trip2" if rows == second_trip and per == 4 else None)
            if o16 is not None:
                log.exact(case, f"out16 == {o16} cast of the dd this launch wrote", same16)
    # a row of constant d: dd follows in closed form
    inp, ref, e32 = ln_case(C, 5, const_row=3)
    assert R.rel_err(ref["dd"][3], R.const_row_dd(inp["g"], inp["dxn"][3])) <= 1e-9
    got, _ = run_ln(inp, cuda, False, None)
    log.check(f"ln-{C}-constrow", got, ref, e32)
    log.done()


@pytest.mark.parametrize("hw,C", R.PATCH_SHAPES)
def test_ln_bwd_patch_gather(cuda, hw, C):
    """The incoming gradient is a 2x2 / stride-2 downsample's patch matrix (15 -> 7, 7 -> 3, 3 -> 1): the odd last row
    and column get dd = 0 exactly and add nothing to dg / dbeta (the reference's gradient there is zero by
    construction)."""
    log = Log()
    for B in (1, 3):
        inp, ref, e32 = ln_case(C, B * hw * hw, patch=(hw, B))
        got, same16 = run_ln(inp, cuda, False, BF16 if B == 3 else None, hw)
        case = f"lnpatch-{hw}x{C}-B{B}"
        log.check(case, got, ref, e32)
        dd = got["dd"].view(B, hw, hw, C)
        assert ref["dd"].view(B, hw, hw, C)[:, hw - 1].abs().max().item() == 0.0
        log.exact(case, "dd of the odd last row and column is exactly 0",
                  not dd[:, hw - 1].any().item() and not dd[:, :, hw - 1].any().item())
        if B == 3:
            log.exact(case, "out16 == bf16 cast of the dd this launch wrote", same16)
    log.done()


@pytest.mark.parametrize("C", [512, 640])
def test_ln_dw1_bwd(cuda, C):
    """1x1 maps, one wave per alert, two alerts per trip: 129 and 300 alerts are past 32 workgroups x 4 waves (a lone last
    row; a second trip)."""
    log = Log()
    for rows in (1, 3, 5, 129, 300):
        inp, ref, e32 = block_case(1, C, rows, 1)
        o16 = {5: BF16, 300: F16}.get(rows)
        got, _, same16 = run_fused("dw1", inp, o16, cuda)
        case = f"dw1-1x{C}-B{rows}"
        log.check(case, got, ref, e32)
        keep = torch.arange(49) != 24
        log.exact(case, "only tap 24 of dW changes",
                  torch.equal(got["dW"].cpu()[:, keep], inp["a0"][:49 * C].view(C, 49)[:, keep]))
        if o16 is not None:
            log.exact(case, f"out16 == {o16} cast of the dy this launch wrote", same16)
    log.done()


# ---- the plain depthwise kernels
@pytest.mark.parametrize("HW,C", R.DW_SHAPES)
def test_dw_plain(cuda, HW, C):
    """out = conv(x, taps or flipped taps) [+ bias] [+ addend]; addend == out is the product's call (dx = dy + conv)."""
    log = Log()
    for B in (1, 3):
        inp = cached(("dwin", HW, C, B), lambda: R.block_inputs(HW, C, B))
        x, w, bias, add = inp["dxn"][0], inp["w"], inp["bias"], inp["dy0"]
        xd, wd, bd, ad = (t.to(cuda) for t in (x, w, bias, add))
        for flip in (0, 1):
            for hb, ha, alias in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1)):
                r64, r32 = (R.dw_plain_ref(x, w, flip, bias if hb else None, add if ha else None, t) for t in (F64, F32))
                out = ad.clone() if alias else torch.full_like(xd, 7.0)
                o16 = (BF16 if C % 128 == 0 else F16) if (alias and flip and B == 3) else None
                out16 = None if o16 is None else torch.full(x.shape, 7.0, dtype=o16, device=cuda)
                ops.cnt_dw_plain(xd, wd, flip, bd if hb else None, (out if alias else ad) if ha else None, out, out16)
                torch.cuda.synchronize()
                case = f"dw_plain-{HW}x{C}-B{B}-flip{flip}-b{hb}a{ha}{'=out' if alias else ''}"
                log.check(case, dict(out=out), r64, R.e32_of(r32, r64), f"dw_plain+addend-{HW}x{C}" if ha else None)
                if o16 is not None:
                    log.exact(case, f"out16 == {o16} cast of the out this launch wrote", torch.equal(out16, out.to(o16)))
    log.done()


@pytest.mark.parametrize("HW,C,Bs", [(hw, c, (1, 3, 257) if (hw, c) in ((15, 64), (7, 160)) else (1, 3)) for hw, c in R.DW_SHAPES],
                         ids=lambda v: str(v))
def test_dw_wgrad(cuda, HW, C, Bs):
    """dw [C, 49] += , dbias [C] += through per-workgroup partial rows and their column sum: C that does not divide 256
    (idle threads), C > 256 (the channel loop), and 257 alerts (two per workgroup, the last workgroup short)."""
    log = Log()
    for B in Bs:
        def make():
            inp = R.block_inputs(HW, C, B)
            a0 = 0.05 * torch.randn(50 * C, generator=torch.Generator().manual_seed(B + C))
            r64, r32 = (R.dw_wgrad_ref(inp["x"], inp["dxn"][0], a0[:49 * C].view(C, 49), a0[49 * C:], t) for t in (F64, F32))
            return inp, a0, r64, R.e32_of(r32, r64)
        inp, a0, ref, e32 = cached(("wgrad", HW, C, B), make)
        arena = a0.to(cuda).clone()
        ops.cnt_dw_wgrad(inp["x"].to(cuda), inp["dxn"][0].to(cuda), arena[:49 * C], arena[49 * C:])
        torch.cuda.synchronize()
        log.check(f"dw_wgrad-{HW}x{C}-B{B}", dict(dW=arena[:49 * C], db=arena[49 * C:]), ref, e32)
    log.done()


@pytest.mark.parametrize("N", [52 * 64, 52 * 256])
@pytest.mark.parametrize("M", [1, 129, 257])
def test_colsum_f32(cuda, M, N):
    """The fp32 column sum that folds partial rows into the arena: out += ."""
    g = torch.Generator().manual_seed(M + N)
    rows, out0 = torch.randn(M, N, generator=g), torch.randn(N, generator=g)
    r64, r32 = (dict(out=out0.to(t) + rows.to(t).sum(0)) for t in (F64, F32))
    out = out0.to(cuda).clone()
    ops.cnt_colsum_f32(rows.to(cuda), out)
    torch.cuda.synchronize()
    log = Log()
    log.check(f"colsum-M{M}-N{N}", dict(out=out), r64, R.e32_of(r32, r64))
    log.done()


# ---- refusals
def test_refusals_launch_nothing(cuda):
    """Every entry point: a (HW, C) its launcher has no kernel for, a null pointer and a negative batch come back as
    BTSBOT_ERR_INVALID_ARG with a message; a canary buffer that holds every output stays as it was."""
    L = _lib.lib()
    SLOT = 1 << 16   # floats per tensor slot: room for one 15x15x80 alert, whatever a call would touch
    buf = torch.randn(14 * SLOT, device=cuda)
    snap = buf.clone()
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)

    def P(i):
        return ctypes.c_void_p(buf.data_ptr() + 4 * SLOT * i)

    NULL = ctypes.c_void_p(0)

    def fused(fn, HW, C, B, first):
        return fn(first, P(1), P(2), P(3), P(4), P(5), NULL, 0, P(6), B, HW, C, 1, 0, st)

    def ln(C, rows, first, patch_hw=0, dd=None):
        return L.btsbot_op_cnt_ln_bwd(first, P(1), P(2), dd or P(3), P(4), P(5), rows, C, NULL, 0, patch_hw, st)

    def dw1(C, rows, first):
        return L.btsbot_op_cnt_ln_dw1_bwd(first, P(1), P(2), P(3), P(4), P(5), NULL, 0, P(6), P(7), P(8), P(9), rows, C, st)

    def plain(HW, C, B, first):
        return L.btsbot_op_cnt_dw_plain(first, P(1), 1, NULL, P(2), P(3), NULL, 0, B, HW, C, st)

    def wgrad(HW, C, B, first, dbias=None):
        return L.btsbot_op_cnt_dw_wgrad(first, P(1), P(2), dbias or ctypes.c_void_p(P(2).value + 4 * 49 * C), B, HW, C, st)

    calls = {
        "dwln_bwd shape": lambda: fused(L.btsbot_op_cnt_dwln_bwd, 15, 80, 1, P(0)),
        "dwln_bwd null": lambda: fused(L.btsbot_op_cnt_dwln_bwd, 15, 64, 1, NULL),
        "dwln_bwd B<0": lambda: fused(L.btsbot_op_cnt_dwln_bwd, 15, 64, -1, P(0)),
        "dw3ln_bwd shape": lambda: fused(L.btsbot_op_cnt_dw3ln_bwd, 3, 320, 1, P(0)),
        "dw3ln_bwd null": lambda: fused(L.btsbot_op_cnt_dw3ln_bwd, 3, 256, 1, NULL),
        "dw3ln_bwd B<0": lambda: fused(L.btsbot_op_cnt_dw3ln_bwd, 3, 256, -1, P(0)),
        "ln_bwd shape": lambda: ln(704, 1, P(0)),
        "ln_bwd null": lambda: ln(64, 1, NULL),
        "ln_bwd rows<0": lambda: ln(64, -1, P(0)),
        "ln_bwd patch in place": lambda: ln(64, 9, P(0), 3, P(1)),
        "ln_dw1_bwd shape": lambda: dw1(704, 1, P(0)),
        "ln_dw1_bwd null": lambda: dw1(512, 1, NULL),
        "ln_dw1_bwd rows<0": lambda: dw1(512, -1, P(0)),
        "dw_plain shape": lambda: plain(5, 64, 1, P(0)),
        "dw_plain null": lambda: plain(15, 64, 1, NULL),
        "dw_plain B<0": lambda: plain(15, 64, -1, P(0)),
        "dw_wgrad shape": lambda: wgrad(5, 64, 1, P(0)),
        "dw_wgrad null": lambda: wgrad(15, 64, 1, NULL),
        "dw_wgrad B<0": lambda: wgrad(15, 64, -1, P(0)),
        "dw_wgrad dbias not adjacent": lambda: wgrad(15, 64, 1, P(0), P(3)),
        "colsum_f32 shape": lambda: L.btsbot_op_cnt_colsum_f32(P(0), P(1), 1, 0, st),
        "colsum_f32 null": lambda: L.btsbot_op_cnt_colsum_f32(NULL, P(1), 1, 64, st),
        "colsum_f32 M<0": lambda: L.btsbot_op_cnt_colsum_f32(P(0), P(1), -1, 64, st),
        "dwln_bwd_rows shape": lambda: L.btsbot_op_cnt_dwln_bwd_rows(15, 80, 1),
        "dw3ln_bwd_rows B<0": lambda: L.btsbot_op_cnt_dw3ln_bwd_rows(-1),
    }
    for name, call in calls.items():
        rc = call()
        msg = L.btsbot_last_error().decode()
        print(f"{name}: {rc} '{msg}'")
        assert rc == _lib.ERR_INVALID_ARG and msg, (name, rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(buf, snap)
    # and the tensor wrapper raises on the adjacency refusal
    x = torch.zeros(1, 15, 15, 64, device=cuda)
    with pytest.raises(_lib.BtsbotHipError, match="adjacent"):
        ops.cnt_dw_wgrad(x, x, torch.zeros(49 * 64, device=cuda), torch.zeros(64, device=cuda))
