"""ConvNeXt stage 2 ALONE (btsbot_op_cn_stage2, btsbot_op_cn_stage2_rows, btsbot_op_cn_pack_s2p, btsbot_op_cn_stage2_alerts:
infer_ops.hip over stage2p.hip) against the float64 reference and the derived per-element bound of tests/stage2_ref.py, whose
docstring holds the derivation; tests/test_stage2_reference.py shows on the CPU what the bound sees and that every seeded
fault leaves it.  Every instantiation of stage2p_kernel that the library launches is reached here by name:

  stage2p_kernel<bf16_t / f16_t / fp8_t, G = 4 / 5 / 7>, <f16x2_t, 4 / 5> (256 channels)   test_stage2[prec-hint], test_hints_give_the_same_bits,
                                                                                            test_alerts_do_not_depend_on_their_neighbours, test_stage2_depth
  stage2p_kernel<bf16_t / f16_t, 5, 0, 320> (convnext_nano: tiles shared by wave pairs)     test_stage2_320[prec], test_stage2_depth
  stage2p_kernel<bf16_t / f16_t, 4 / 5, TRAIN = 1> (the keeping form: xin, xn, a, hh,       test_stage2_keep[prec-hint]
                                                    ds_patches)
  stage2p_kernel<bf16_t / f16_t, 7, 0, 256, ROWS = 64> (launch_stage2p_rows)                test_stage2_rows[prec]
  fp8: the clamp in front of the conversion, scales at both ends of their interval, the     test_fp8_saturation, test_fp8_scale_interval_ends,
       downsample's bf16 operands                                                            test_fp8_downsample_is_bf16
  pack_frag_kernel<bf16 / f16>, pack_frag_split_kernel, pack_frag_fp8_kernel, reorder_down  test_pack_s2p[prec]
  the entry points' argument checks                                                         test_stage2_refusals

f16x2 at hint 7 runs G = 5 (launch_stage2p: seven alerts' doubled planes do not fit the LDS, and the G = 7 split kernel does
not exist: the call succeeding is the evidence); btsbot_op_cn_stage2_alerts gives the library's choice for every other call.
Every output lies in a guarded buffer: sentinel bytes in front and behind, and a canary region behind the last row (the
keeping form: behind alert B + 9) that must keep its fill.  Each test prints its worst err / bound per case (run with -s) and
asserts at the end.

The keeping form's tap_stage is NOT the inference form's: it takes the GELU at the pre-activation ROUNDED to the operand type
(what the backward differentiates), so the two differ by up to the bound's `keeping` term; test_stage2_keep holds each to its
own bound and their difference to the sum of the two.

Worst err / bound over a test's cases, measured on an MI355X on 2026-10-21 (a record, not a tolerance; tap = tap_stage):
  test_stage2 (G = 4, 5, 7 alike)   dense: out  tap     spotlight: out  tap     spotlight, dense taps: out  tap
    bf16                                   0.000 0.007             0.196 0.662                          0.333 0.610
    f16                                    0.001 0.007             0.165 0.528                          0.214 0.567
    fp8                                    0.000 0.006             0.067 0.600                          0.198 0.564
    f16x2                                  0.000 0.015             0.005 0.012                          0.006 0.016
  test_stage2_320   bf16                   0.000 0.013             0.163 0.523                          0.252 0.581
                    f16                    0.000 0.013             0.188 0.491                          0.283 0.603
  test_stage2_keep  (all cases)        out    tap    ds_patches  xin    xn     a      hh     hh against gelu(kept a)
    bf16                               0.194  0.574  0.247       0.563  0.994  0.959  0.839  0.964
    f16                                0.209  0.477  0.238       0.471  0.982  0.942  0.825  0.995
    (xn is one rounding of a value known to ~1e-7: its ratio is the rounding's own worst case; dense: out 0.000, tap 0.008)
  test_stage2_rows                     dense 0.006 (bf16), 0.006 (f16); spotlight 0.549 (bf16), 0.565 (f16)
  test_stage2_depth, spotlight tap     depth 1      2      6      8
    bf16 / f16 / fp8 / f16x2 at 256    0.610 / 0.516 / 0.547 / 0.014   0.577 / 0.484 / 0.600 / 0.011   0.471 / 0.510 / 0.482 / 0.007
                                       0.465 / 0.446 / 0.433 / 0.007   (every depth equal to its one-block calls bit for bit)
    bf16 / f16 at 320                  0.539 / 0.603   0.523 / 0.491   0.474 / 0.435   0.488 / 0.419   (the chain of calls: the same figures)
  test_fp8_saturation 0.589;  test_fp8_scale_interval_ends 0.005 (top), 0.006 (bottom);  test_fp8_downsample_is_bf16 out 0.958
  test_pack_s2p: every image bit for bit.
(The dense figures are small because the worst-case bound over 256 .. 1280 products is wide; the spotlight cases are the sharp
ones.  Nothing had to be fixed in stage2p.hip.)
"""
import functools
import os

import pytest
import torch

import stage2_ref as R
from btsbot_amd import _lib, ops
from test_gpu_stage3_ops import Log, pack_input

if "BTSBOT_AMD_S2P_G" in os.environ:
    pytest.skip("BTSBOT_AMD_S2P_G (the developer switch behind SW_S2P_G) forces the alerts per workgroup at every call: alerts_hint "
                "would not select the instantiation under test", allow_module_level=True)

pytestmark = pytest.mark.gpu
F32 = torch.float32
PADB = 4096            # sentinel bytes in front of and behind every guarded buffer
SENT, CANARY = 0xA5, 0x5A
B_MAX = 15             # 2 G + 1 at G = 7
HINTS = (4, 5, 7)
KINDS = {"dense one": lambda C: (R.dense_blocks(C, ("one",), 16), R.dense_down(C, 36)),
         "dense init/one": lambda C: (R.dense_blocks(C, ("init", "one"), 11), R.dense_down(C, 31)),
         "dense zero/tenth": lambda C: (R.dense_blocks(C, ("zero", "tenth"), 12), R.dense_down(C, 32)),
         "spotlight": lambda C: (R.spot_blocks(C, 2, 13), R.spot_down(C, 33)),
         "spotlight dense taps": lambda C: (R.spot_blocks(C, 1, 17, dw="dense"), R.spot_down(C, 37)),
         "spotlight gamma 0": lambda C: (R.scale_gamma(R.spot_blocks(C, 1, 18), 0.0), R.spot_down(C, 38)),
         # depths 6 and 8.  A worst-case bound grows by the product of three absolute row sums per block (dense, layer scale 1:
         # several hundred), so the dense deep cases are pinned by their equality with one-block calls, and the spotlight ones
         # take layer scales of 2^-7 .. 2^-5: the bound then stays a few 16-bit roundings of a block's contribution wide
         # through all eight blocks, and a block skipped, doubled or out of order leaves it
         "dense depth 6": lambda C: (R.dense_blocks(C, ("zero", "init", "init", "tenth", "tenth", "one"), 41), R.dense_down(C, 42)),
         "dense depth 8": lambda C: (R.dense_blocks(C, ("zero", "init", "init", "init", "tenth", "tenth", "tenth", "one"), 43),
                                     R.dense_down(C, 44)),
         "spotlight depth 6": lambda C: (R.scale_gamma(R.spot_blocks(C, 6, 45), 2.0 ** -6), R.spot_down(C, 46)),
         "spotlight depth 8": lambda C: (R.scale_gamma(R.spot_blocks(C, 8, 47), 2.0 ** -6), R.spot_down(C, 48))}
MAIN = ("dense init/one", "dense zero/tenth", "spotlight", "spotlight dense taps")


def b_edges(G):
    return (1, G - 1, G, G + 1, 2 * G, 2 * G + 1)


def granted(prec, B, hint):
    """the alerts per workgroup the call runs with, from the library (f16x2: 5 where 7 was chosen, launch_stage2p)"""
    G = ops.cn_stage2_alerts(B, hint)
    assert G == hint
    return 5 if prec == "f16x2" and G == 7 else G


def ibits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same(a, b):
    return torch.equal(ibits(a), ibits(b))


class Guarded:
    """[PADB sentinel bytes | live values | canary values | PADB sentinel bytes] on the device"""

    def __init__(self, live, canary, dtype, dev, fill=CANARY):
        esz = torch.empty(0, dtype=dtype).element_size()
        self.nl, self.nc, self.fill = live * esz, canary * esz, fill
        self.buf = torch.full((self.nl + self.nc + 2 * PADB,), SENT, dtype=torch.uint8, device=dev)
        self.buf[PADB:PADB + self.nl + self.nc] = fill
        self.live = self.buf[PADB:PADB + self.nl].view(dtype)

    def intact(self):
        b, end = self.buf, PADB + self.nl
        return bool((b[:PADB] == SENT).all()) and bool((b[end + self.nc:] == SENT).all()) and bool((b[end:end + self.nc] == self.fill).all())

    def untouched(self):
        return self.intact() and bool((self.buf[PADB:PADB + self.nl] == self.fill).all())


@functools.lru_cache(maxsize=None)
def case(C, kind):
    """(x [B_MAX][9][C], blocks, down) on the CPU; a call of B alerts takes the first B"""
    blocks, down = KINDS[kind](C)
    return R.maps_x(C, B_MAX, 5, blocks[0]), blocks, down


@functools.lru_cache(maxsize=None)
def reference(C, kind, prec, keep=False):
    """stage2_ref's result for B_MAX alerts: an alert's result does not depend on the others, so every B reads its first B"""
    return R.stage2_ref(*case(C, kind), prec, keep=keep)


@functools.lru_cache(maxsize=None)
def on_device(C, kind, dev):
    x, blocks, down = case(C, kind)
    return x.to(dev), [{k: v.to(dev) for k, v in P.items()} for P in blocks], {k: v.to(dev) for k, v in down.items()}


def run(prec, x, blocks, down, hint, keep=False, fill=CANARY, log=None, label=""):
    """the entry point on guarded buffers -> dict(out [B][2C], tap [B][9][C], keep [per block {xin, xn, a, hh}], patches) on
    the CPU; x, blocks, down on the device.  Sentinels and canaries are checked."""
    B, _, C = x.shape
    dev, T = x.device, R.ODT.get(prec)
    out, tap = Guarded(B * 2 * C, 4 * C, F32, dev), Guarded(B * 9 * C, 18 * C, F32, dev)
    guards, kb, pat = [out, tap], None, None
    if keep:
        n = (B + 9) * 9
        kb = dict(xin=[Guarded(n * C, 4 * C, F32, dev, fill) for _ in blocks], xn=[Guarded(n * C, 4 * C, T, dev, fill) for _ in blocks],
                  a=[Guarded(n * 4 * C, 4 * C, T, dev, fill) for _ in blocks], hh=[Guarded(n * 4 * C, 4 * C, T, dev, fill) for _ in blocks])
        pat = Guarded((B + 9) * 4 * C, 4 * C, T, dev, fill)
        guards += [g for v in kb.values() for g in v] + [pat]
    ops.cn_stage2(prec, x.contiguous(), blocks, down, out.live, tap.live, alerts_hint=hint,
                  keep=None if kb is None else {k: [g.live for g in v] for k, v in kb.items()},
                  ds_patches=None if pat is None else pat.live, B=B, cw=C)
    torch.cuda.synchronize()
    ok = all(g.intact() for g in guards)
    if log is not None:
        log.exact(label, "sentinels and canaries intact", ok)
    else:
        assert ok, label
    res = dict(out=out.live.view(B, 2 * C).cpu(), tap=tap.live.view(B, 9, C).cpu())
    if keep:
        res["keep"] = [{k: kb[k][j].live.view(B + 9, 9, -1)[:B].cpu() for k in kb} for j in range(len(blocks))]
        res["patches"] = pat.live.view(B + 9, 4 * C)[:B].cpu()
    return res


def check(log, label, got, ref, B, keep=False):
    """out, tap (and the kept rows) of a B-alert call against the first B alerts of the reference"""
    log.exact(label, "finite", bool(torch.isfinite(got["out"]).all()) and bool(torch.isfinite(got["tap"]).all()))
    for k in ("out", "tap"):
        log.check(f"{label} {k}", got[k], ref[k][0][:B], ref[k][1][:B])
    if keep:
        log.check(f"{label} ds_patches", got["patches"].float(), ref["patches"][0][:B], ref["patches"][1][:B])
        for j, kbj in enumerate(ref["keep"]):
            for n, (v, e) in kbj.items():
                log.check(f"{label} {n}[{j}]", got["keep"][j][n].float(), v[:B], e[:B])


@pytest.mark.parametrize("prec,hint", [(p, h) for p in R.PRECS for h in HINTS])
def test_stage2(cuda, prec, hint):
    """256 channels, every mode at every alerts-per-workgroup, dense and spotlight, at the batch edges of G"""
    C = 256
    assert ops.cn_stage2_supported(prec, C, 2)
    log = Log()
    for kind in MAIN:
        x, blocks, down = on_device(C, kind, cuda)
        ref = reference(C, kind, prec)
        for B in b_edges(granted(prec, B_MAX, hint)):
            G = granted(prec, B, hint)
            label = f"stage2 {prec} G={G} {kind} B={B}"
            check(log, label, run(prec, x[:B], blocks, down, hint, log=log, label=label), ref, B)
    log.done()


@pytest.mark.parametrize("prec", R.PRECS_AT[320])
def test_stage2_320(cuda, prec):
    """320 channels (G = 5 whatever the hint): the four tiles shared by wave pairs, the 9th and 10th channel of a lane"""
    C = 320
    assert ops.cn_stage2_supported(prec, C, 2) and not ops.cn_stage2_supported("fp8", C, 2)
    log = Log()
    for kind in MAIN + ("dense one",):
        x, blocks, down = on_device(C, kind, cuda)
        ref = reference(C, kind, prec)
        for B in b_edges(5):
            label = f"stage2 {prec} C=320 {kind} B={B}"
            got = run(prec, x[:B], blocks, down, 0, log=log, label=label)
            check(log, label, got, ref, B)
            if B == 6 and kind == "dense one":      # (the hint does not reach this form)
                other = run(prec, x[:B], blocks, down, 7, log=log, label=label)
                log.exact(label, "hint 7 gives the same bits", same(got["out"], other["out"]) and same(got["tap"], other["tap"]))
    log.done()


@pytest.mark.parametrize("prec,hint", [(p, h) for p in R.KEEP_PRECS for h in (4, 5)])
def test_stage2_keep(cuda, prec, hint):
    """the training forward's keeping form: out, tap_stage and every kept buffer against the reference; xin[0] is x_in's bits;
    hh is the GELU of the kept a; the live rows do not depend on what the padding rows held; the difference to the inference
    form's tap_stage stays inside the two bounds"""
    C = 256
    log = Log()
    for kind in ("dense init/one", "spotlight", "spotlight dense taps"):
        x, blocks, down = on_device(C, kind, cuda)
        ref, ref_inf = reference(C, kind, prec, True), reference(C, kind, prec)
        for B in b_edges(hint):
            assert granted(prec, B, hint) == hint
            label = f"stage2 keep {prec} G={hint} {kind} B={B}"
            got = run(prec, x[:B], blocks, down, hint, keep=True, log=log, label=label)
            check(log, label, got, ref, B, keep=True)
            log.exact(label, "xin[0] is x_in bit for bit", same(got["keep"][0]["xin"], x[:B].cpu()))
            for j, kbj in enumerate(got["keep"]):
                r = R.pair_ratio(kbj["a"], kbj["hh"], prec)
                print(f"{label + f' hh[{j}] against gelu(kept a)':64s} {r:.3f}")
                log.exact(label, f"hh[{j}] is the GELU of the kept a", r <= 1.0)
            if B in (1, hint + 1):
                other = run(prec, x[:B], blocks, down, hint, keep=True, fill=0xFF, log=log, label=label)
                eq = same(got["out"], other["out"]) and same(got["tap"], other["tap"]) and same(got["patches"], other["patches"]) and \
                    all(same(p[n], q[n]) for p, q in zip(got["keep"], other["keep"]) for n in p)
                log.exact(label, "the live rows do not depend on the padding rows", eq)
                inf = run(prec, x[:B], blocks, down, hint, log=log, label=label)
                d = (got["tap"].double() - inf["tap"].double()).abs()
                log.exact(label, "tap_stage within the two bounds of the inference form's",
                          bool((d <= ref["tap"][1][:B] + ref_inf["tap"][1][:B]).all()))
    log.done()


@pytest.mark.parametrize("prec", R.KEEP_PRECS)
def test_stage2_rows(cuda, prec):
    """the row-tile form at the edges of its 64-row tile; a row does not depend on its neighbours"""
    log = Log()
    for kind in ("dense one", "spotlight dense taps"):
        x, blocks, _ = on_device(256, kind, cuda)
        rows, P = x.reshape(-1, 256), blocks[0]
        Pc = case(256, kind)[1][0]
        ref, bound = R.rows_ref(rows[:129].cpu(), Pc, prec)
        full = None
        for n in (1, 63, 64, 65, 129):
            label = f"stage2 rows {prec} {kind} rows={n}"
            g = Guarded(n * 256, 2 * 256, F32, cuda)
            g.live.copy_(rows[:n].reshape(-1))
            ops.cn_stage2_rows(prec, g.live, P, rows=n)
            torch.cuda.synchronize()
            log.exact(label, "sentinels and the rows past the last intact", g.intact())
            got = g.live.view(n, 256).cpu()
            log.exact(label, "finite", bool(torch.isfinite(got).all()))
            log.check(label, got, ref[:n], bound[:n])
            full = got
        for r in (0, 63, 64, 128):
            g = Guarded(256, 2 * 256, F32, cuda)
            g.live.copy_(rows[r])
            ops.cn_stage2_rows(prec, g.live, P, rows=1)
            torch.cuda.synchronize()
            log.exact(f"stage2 rows {prec} {kind}", f"row {r} alone gives the same bits", g.intact() and same(g.live.cpu(), full[r]))
    log.done()


@pytest.mark.parametrize("prec,hint", [(p, h) for p in R.PRECS for h in HINTS])
def test_alerts_do_not_depend_on_their_neighbours(cuda, prec, hint):
    """alert i of a ragged batch of 2 G + 1 = the same alert run alone = the same alert as column 0 of a full workgroup with
    other alerts behind it, bit for bit"""
    C = 256
    G = granted(prec, B_MAX, hint)
    B = 2 * G + 1
    for kind in ("dense one", "spotlight"):
        x, blocks, down = on_device(C, kind, cuda)
        full = run(prec, x[:B], blocks, down, hint)
        for i in (0, 1, G - 1, G, 2 * G - 1, 2 * G):
            alone = run(prec, x[i:i + 1], blocks, down, hint)
            assert same(alone["out"][0], full["out"][i]) and same(alone["tap"][0], full["tap"][i]), (kind, i)
            first = run(prec, torch.cat([x[i:i + 1], x[:i], x[i + 1:]])[:G], blocks, down, hint)
            assert same(first["out"][0], full["out"][i]) and same(first["tap"][0], full["tap"][i]), (kind, i, "column 0")


@pytest.mark.parametrize("prec", R.PRECS)
def test_hints_give_the_same_bits(cuda, prec):
    """out and tap_stage do not depend on the alerts per workgroup (what test_gpu_stage2p_map.py sees through the logits)"""
    for kind in ("dense init/one", "spotlight"):
        x, blocks, down = on_device(256, kind, cuda)
        res = [run(prec, x[:B_MAX], blocks, down, h) for h in (0, 4, 5, 7)]
        for r in res[1:]:
            assert same(r["out"], res[0]["out"]) and same(r["tap"], res[0]["tap"]), kind


@pytest.mark.parametrize("prec,C", [(p, 256) for p in R.PRECS] + [(p, 320) for p in R.PRECS_AT[320]])
def test_stage2_depth(cuda, prec, C):
    """depths 1 (the kernel re-reads its own chunk 0 behind the last chunk), 2, 6 and 8 (S2P_MAX_DEPTH) against the reference,
    and at 256 channels each equal, bit for bit, to its blocks run one call at a time through tap_stage.  (Not at 320: a
    wave pair's two partial residuals of a shared tile are carried through all blocks of a call and only summed where x is
    read, while a chain of calls restarts from their rounded sum -- the chain is held to the same reference and bound.)"""
    B = 6
    log = Log()
    for kinds in (("dense one", "spotlight dense taps"), ("dense init/one", "spotlight"), ("dense depth 6", "spotlight depth 6"),
                  ("dense depth 8", "spotlight depth 8")):
        for kind in kinds:
            x, blocks, down = on_device(C, kind, cuda)
            depth = len(blocks)
            assert ops.cn_stage2_supported(prec, C, depth)
            label = f"stage2 {prec} C={C} depth {depth} {kind} B={B}"
            got = run(prec, x[:B], blocks, down, 5, log=log, label=label)
            check(log, label, got, reference(C, kind, prec), B)
            step = dict(tap=x[:B].cpu())
            for P in blocks:
                step = run(prec, step["tap"].to(cuda), [P], down, 5, log=log, label=label)
            if C == 256:
                log.exact(label, "equal to its blocks run one at a time", same(step["tap"], got["tap"]) and same(step["out"], got["out"]))
            else:
                check(log, label + " chained", step, reference(C, kind, prec), B)
    log.done()


def test_fp8_saturation(cuda):
    """a hidden activation driven past 448: the kernel clamps in front of the conversion (e4m3 has no infinity), the other
    alerts keep their bits"""
    C = 256
    log = Log()
    x, x_plain, blocks, alert = R.saturating(C, 21)
    down = R.spot_down(C, 35)
    free = R.stage2_ref(x, blocks, down, "fp8", saturate=True)["tap"][0]
    ref = R.stage2_ref(x, blocks, down, "fp8", saturate=True, clamp_g=True)
    assert float(((free - ref["tap"][0]).abs() / ref["tap"][1])[alert].max()) > 1.0          # the clamp is visible in this alert
    bd, dd = [{k: v.to(cuda) for k, v in P.items()} for P in blocks], {k: v.to(cuda) for k, v in down.items()}
    for hint in (4, 5, 7):
        label = f"fp8 saturation G={hint}"
        got = run("fp8", x.to(cuda), bd, dd, hint, log=log, label=label)
        plain = run("fp8", x_plain.to(cuda), bd, dd, hint, log=log, label=label)
        check(log, label, got, ref, x.shape[0])
        others = [b for b in range(x.shape[0]) if b != alert]
        log.exact(label, "the other alerts keep their bits", same(got["tap"][others], plain["tap"][others]))
    log.done()


def test_fp8_scale_interval_ends(cuda):
    """filters whose largest magnitude puts S max|w| just under 240 and just over 120 (both ends of a power-of-two interval)"""
    C, B = 256, 6
    log = Log()
    x, blocks, down = case(C, "dense one")
    for end, target in (("top", 239.9), ("bottom", 120.1)):
        P = {k: v.clone() for k, v in blocks[0].items()}
        P["fc1_w"] *= target / 256.0 / float(P["fc1_w"].abs().max())
        gw = P["fc2_w"] * P["gamma"][:, None]
        P["fc2_w"] *= target / 1024.0 / float(gw.abs().max())
        m1, m2 = float(P["fc1_w"].abs().max()), float((P["fc2_w"] * P["gamma"][:, None]).abs().max())
        assert R.fp8_scale(m1) == 256.0 and R.fp8_scale(m2) == 1024.0 and abs(m1 * 256 - target) < 0.05 and abs(m2 * 1024 - target) < 0.05
        ref = R.stage2_ref(x[:B], [P], down, "fp8")
        label = f"fp8 scales at the {end} of their interval"
        got = run("fp8", x[:B].to(cuda), [{k: v.to(cuda) for k, v in P.items()}], {k: v.to(cuda) for k, v in down.items()}, 5, log=log,
                  label=label)
        check(log, label, got, ref, B)
    log.done()


def test_fp8_downsample_is_bf16(cuda):
    """layer scale 0 leaves the rows exact, and the sparse downsample filter's values are exact in bf16 and not in e4m3: its
    one product per output comes through to bf16's rounding of the LayerNorm'd row, which an e4m3 filter would miss"""
    C, B, kind = 256, 6, "spotlight gamma 0"
    log = Log()
    x, blocks, down = case(C, kind)
    ref = reference(C, kind, "fp8")
    wrong = R.stage2_ref(x, blocks, down, "fp8", fault="ds_fp8")["out"][0]
    assert R.outside(R.ratio(wrong, *ref["out"]))
    xd, bd, dd = on_device(C, kind, cuda)
    for hint in (4, 5, 7):
        label = f"fp8 downsample in bf16 G={hint}"
        got = run("fp8", xd[:B], bd, dd, hint, log=log, label=label)
        check(log, label, got, ref, B)
        log.exact(label, "gamma 0: tap_stage is x_in", same(got["tap"], x[:B]))
    log.done()


@pytest.mark.parametrize("prec", R.PRECS)
def test_pack_s2p(cuda, prec):
    """the packers' images unpacked and compared bit for bit with host rounding: ties, f16 subnormals, negative zeros,
    rowscale; reorder_down at cin 256 and 320; the smallest legal shapes and the stage's own"""
    bad = []
    ks = 128 if prec == "fp8" else 32
    shapes = [(16, ks, False, 0), (1024, 256, False, 0), (256, 1024, False, 0), (1280, 320, False, 0), (320, 1280, False, 0)]
    shapes += [(16, ks, True, ks // 4), (512, 1024, True, 256), (640, 1280, True, 320)]
    shapes = [s for s in shapes if s[1] % ks == 0]
    for rows, K, down, cin in shapes:
        for with_rowscale in (False, True):
            w, rs = pack_input(prec, rows, K, with_rowscale, rows + K)
            src = w.view(rows, 4, cin).permute(0, 2, 1).reshape(rows, cin, 2, 2).contiguous() if down else w
            assert not down or torch.equal(R.reorder_down(src), w)
            img = Guarded(rows * K * R.ESZ[prec], 64, torch.uint8, cuda)
            sc = Guarded(2, 2, F32, cuda)
            ops.cn_pack_s2p(prec, src.to(cuda), rs.to(cuda) if rs is not None else None, reorder_down=down, cin=cin, dst=img.live,
                            scale=sc.live if prec == "fp8" else None, rows=rows, K=K)
            torch.cuda.synchronize()
            label = f"pack_s2p {prec} {rows}x{K} rowscale={with_rowscale} reorder_down={down}"
            guards = img.intact() and (sc.intact() if prec == "fp8" else sc.untouched())
            S = None
            if prec == "fp8":
                S = float(sc.live[0])
                if S != 256.0 or float(sc.live[1]) != 1.0 / 256.0:
                    bad.append(f"{label}: scale {sc.live.tolist()}")
                    continue
            want = R.host_round(prec, w, rs, S)
            got = R.unpack_s2p(img.live.cpu(), prec, rows, K)
            pairs = zip(got, want) if prec == "f16x2" else ((got, want),)
            ok = all(torch.equal(R.bits(a), R.bits(b)) for a, b in pairs)
            print(f"{label:72s} bit for bit: {ok}   guards intact: {guards}")
            if not (ok and guards):
                bad.append(label)
    assert not bad, "\n".join(bad)


def test_stage2_refusals(cuda):
    C, B, prec = 256, 5, "bf16"
    x, blocks, down = on_device(C, "spotlight", cuda)
    x = x[:B].contiguous()
    out, tap = Guarded(B * 2 * C, 4 * C, F32, cuda), Guarded(B * 9 * C, 18 * C, F32, cuda)
    n = (B + 9) * 9
    T = R.ODT[prec]
    kb = dict(xin=[Guarded(n * C, 64, F32, cuda) for _ in blocks], xn=[Guarded(n * C, 64, T, cuda) for _ in blocks],
              a=[Guarded(n * 4 * C, 64, T, cuda) for _ in blocks], hh=[Guarded(n * 4 * C, 64, T, cuda) for _ in blocks])
    pat = Guarded((B + 9) * 4 * C, 64, T, cuda)
    keep = {k: [g.live for g in v] for k, v in kb.items()}
    everything = [out, tap, pat] + [g for v in kb.values() for g in v]

    def refused(word, p=prec, **kw):
        a = dict(x_in=x, blocks=blocks, down=down, out=out.live, tap_stage=tap.live, alerts_hint=0, keep=None, ds_patches=None, B=B, cw=C)
        a.update(kw)
        with pytest.raises(_lib.BtsbotHipError, match=word) as e:
            ops.cn_stage2(p, a.pop("x_in"), a.pop("blocks"), a.pop("down"), a.pop("out"), **a)
        assert f"({_lib.ERR_INVALID_ARG})" in str(e.value)
        torch.cuda.synchronize()
        assert all(g.untouched() for g in everything), word      # nothing launched

    assert not ops.cn_stage2_supported("f32", C, 2) and not ops.cn_stage2_supported(prec, 384, 2)
    assert not ops.cn_stage2_supported(prec, C, 0) and not ops.cn_stage2_supported(prec, C, 9)
    assert not ops.cn_stage2_supported("fp8", 320, 2) and not ops.cn_stage2_supported("f16x2", 320, 2)
    assert all(ops.cn_stage2_supported(p, c, d) for c in R.WIDTHS for p in R.PRECS_AT[c] for d in (1, 8))
    refused("unsupported", p="f32")
    refused("unsupported", cw=384)
    refused("unsupported", blocks=[])
    refused("unsupported", blocks=blocks * 4 + blocks[:1])
    refused("unsupported", p="fp8", cw=320)
    refused("alerts_hint must be", alerts_hint=6)
    refused("negative alert count", B=-1)
    refused("all or none", keep=keep)                                         # (no ds_patches)
    refused("all or none", keep=dict(keep, a=None), ds_patches=pat.live)
    refused("all or none", ds_patches=pat.live)
    refused("keeping form runs in", p="fp8", keep=keep, ds_patches=pat.live)
    refused("keeping form runs in", p="f16x2", keep=keep, ds_patches=pat.live)
    refused("keeping form runs in", cw=320, keep=keep, ds_patches=pat.live)
    refused("needs tap_stage", keep=keep, ds_patches=pat.live, tap_stage=None)
    refused("null pointer", x_in=None)
    refused("null pointer", out=None)
    for k in R.PARAMS:
        refused("null pointer", blocks=[blocks[0], dict(blocks[1], **{k: None})])
    for k in R.DOWN:
        refused("null pointer", down=dict(down, **{k: None}))
    refused("null pointer", keep=dict(keep, hh=[keep["hh"][0], None]), ds_patches=pat.live)

    def off(t):
        """t's values 4 bytes (2 for a 16-bit type: 2 elements) off a 16-byte boundary"""
        k = 4 // t.element_size()
        o = torch.cat([t.reshape(-1), t.reshape(-1)[:8]])[k:k + t.numel()]
        assert o.data_ptr() % 16 == 4
        return o

    refused("x_in, out and tap_stage must be 16-byte aligned", x_in=off(x))
    refused("x_in, out and tap_stage must be 16-byte aligned", out=off(torch.zeros(B * 2 * C, device=cuda)))
    refused("x_in, out and tap_stage must be 16-byte aligned", tap_stage=off(torch.zeros(B * 9 * C, device=cuda)))
    for k in ("dw_b", "ln_w", "ln_b", "fc1_b", "fc2_b", "gamma"):
        refused("parameter vectors must be 16-byte aligned", blocks=[blocks[0], dict(blocks[1], **{k: off(blocks[1][k])})])
    for k in ("ds_ln_w", "ds_ln_b", "ds_b"):
        refused("parameter vectors must be 16-byte aligned", down=dict(down, **{k: off(down[k])}))
    refused("keep buffers must be 16-byte aligned", keep=dict(keep, xn=[keep["xn"][0], off(torch.zeros(n * C, dtype=T, device=cuda))]),
            ds_patches=pat.live)
    refused("keep buffers must be 16-byte aligned", keep=keep, ds_patches=off(torch.zeros((B + 9) * 4 * C, dtype=T, device=cuda)))
    ops.cn_stage2(prec, x, blocks, down, out.live, tap.live, B=0, cw=C)          # B == 0: OK, nothing touched
    torch.cuda.synchronize()
    assert all(g.untouched() for g in everything)
    with pytest.raises(_lib.BtsbotHipError, match="bad argument"):
        ops.cn_stage2_alerts(8, 6)
    # the row-tile form
    rows = Guarded(3 * 256, 2 * 256, F32, cuda)
    P = blocks[0]
    for word, kw in (("unsupported", dict(p="fp8")), ("unsupported", dict(p="f16x2")), ("bad row count", dict(rows=-1)),
                     ("null pointer", dict(x=None)), ("null pointer", dict(P=dict(P, gamma=None))),
                     ("x must be 16-byte aligned", dict(x=off(torch.zeros(3 * 256, device=cuda)))),
                     ("parameter vectors must be 16-byte aligned", dict(P=dict(P, fc1_b=off(P["fc1_b"]))))):
        a = dict(p=prec, x=rows.live, P=P, rows=3)
        a.update(kw)
        with pytest.raises(_lib.BtsbotHipError, match=word) as e:
            ops.cn_stage2_rows(a["p"], a["x"], a["P"], rows=a["rows"])
        assert f"({_lib.ERR_INVALID_ARG})" in str(e.value)
        torch.cuda.synchronize()
        assert rows.untouched(), word
    ops.cn_stage2_rows(prec, rows.live, P, rows=0)
    torch.cuda.synchronize()
    assert rows.untouched()
    # the packer
    z = torch.zeros(64 * 256, device=cuda)
    for p, r, K, kw in (("bf16", 24, 64, {}), ("bf16", 16, 48, {}), ("fp8", 16, 64, {}),
                        ("bf16", 16, 64, dict(reorder_down=True, cin=8))):
        with pytest.raises(_lib.BtsbotHipError, match="bad shape|K must be 4 cin") as e:
            ops.cn_pack_s2p(p, z, rows=r, K=K, **kw)
        assert f"({_lib.ERR_INVALID_ARG})" in str(e.value)
    with pytest.raises(_lib.BtsbotHipError, match="precision must be"):
        ops.cn_pack_s2p("f32", z, rows=16, K=32, dst=torch.empty(2048, dtype=torch.uint8, device=cuda))
