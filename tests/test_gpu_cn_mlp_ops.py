"""The MLP kernels of the ConvNeXt 16-bit training step, each ALONE (btsbot_op_cnt_*, btsbot_amd/csrc/cn_mlp_ops.hip)
against float64 references with derived per-element bounds (tests/mlp_ref.py, whose docstring holds the derivation;
tests/test_mlp_ops_reference.py shows on the CPU what the bounds see):

  mlp_bwd_kernel<T,64,8> / <T,128,4> + wgrad_reduce (+ det_reduce_kernel)   test_mlp_bwd, test_mlp_bwd_deterministic
  s2mlp_bwd_kernel + pack_frag16_kernel                                     test_s2mlp_bwd
  fused_mlp_kernel<T,64|80|128|160> with xres + pack_fused_kernel           test_fused_mlp
  fc2_grads_kernel                                                          test_fc2_grads

Inputs are exact in both operand types, so the precision-independent part of a reference is computed once per case (on
the device, in float64) and shared.  Every output is a slice of a larger buffer whose head and tail hold a sentinel bit
pattern that must survive; outputs that are added to are pre-filled with non-zero values, outputs that are written with
others.  Each test prints its worst err / bound per output (run with -s) and asserts at the end.  Plane, workgroup and
row counts come from the launchers' companions, not from a mirrored formula.
"""
import ctypes

import pytest
import torch

import mlp_ref as R
from btsbot_amd import _lib, ops

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
PAD = 1024
SENTINEL = {2: (torch.int16, 0x7E5A), 4: (torch.int32, 0x7FC5A5A5)}
_LAST = {}


def cached(kind, key, make):
    """the latest case of each kind: the two precisions of a case follow each other"""
    if _LAST.get(kind, (None,))[0] != key:
        _LAST[kind] = (key, make())
    return _LAST[kind][1]


def guarded(n, dtype, dev, fill):
    """[PAD sentinel | n elements = fill | PAD sentinel] -> (buffer, the n elements)"""
    buf = torch.empty(n + 2 * PAD, dtype=dtype, device=dev)
    it, pat = SENTINEL[buf.element_size()]
    buf.view(it).fill_(pat)
    t = buf[PAD:PAD + n]
    if isinstance(fill, torch.Tensor):
        t.copy_(fill.reshape(-1))
    else:
        t.fill_(fill)
    return buf, t


def intact(buf):
    it, pat = SENTINEL[buf.element_size()]
    b = buf.view(it)
    return bool((b[:PAD] == pat).all()) and bool((b[-PAD:] == pat).all())


class Log:
    def __init__(self):
        self.bad = []

    def check(self, case, got, ref, bound):
        r = R.worst(got, ref, bound)
        print(f"{case:40s} " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()) + "   (worst err / bound)")
        self.bad += [f"{case} {k}: err / bound = {v:.4g}" for k, v in r.items() if not v <= 1.0]
        return r

    def exact(self, case, what, ok):
        print(f"{case:40s} {what}: {'yes' if ok else 'NO'}")
        if not ok:
            self.bad.append(f"{case}: {what}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


# ---- mlp_bwd
MLP_BWD_SHAPES = [(64, r) for r in (1, 63, 64, 65, 129, 225, 16385, 32967)] + [(128, r) for r in (1, 49, 65, 129, 4097, 8265)]
SPOT_FROM = 4097   # from here on dy is a spotlight: the reduced outputs' bounds stay at a few tiles' share


def mlp_case(C, Rr, dev, trip=1):
    """trip: the spotlight starts at the grid stride's trip of that number (1 = every tile past the first trip)"""
    def make():
        slices, planes = ops.cnt_mlp_bwd_slices(C, Rr), ops.cnt_mlp_bwd_planes(C)
        tiles = -(-Rr // 64)
        live = None
        if Rr >= SPOT_FROM:
            # the tiles past the first trip of the grid stride (the ragged last tile among them) and 64 rows elsewhere
            assert tiles > trip * slices, (tiles, slices)
            first = trip * slices * 64
            g = torch.Generator().manual_seed(Rr)
            live = torch.cat([torch.arange(first, Rr), torch.randperm(first, generator=g)[:64]])
        inp = R.mlp_bwd_inputs(C, Rr, seed=1000 * C + Rr, live_rows=live, dev=dev)
        return inp, R.mlp_bwd_base(inp), slices, planes, tiles
    return cached("mlp", (C, Rr, trip), make)


def run_mlp_bwd(inp, prec, planes, det=False):
    T = R.DT[prec]
    Rr, C = inp["xn"].shape
    dev = inp["xn"].device
    t16 = {k: inp[k].to(T) for k in ("xn", "dy", "w1", "w2g")}
    shapes = dict(dxn=(planes, Rr, C), G=(C, 4 * C), S=(C,), dW1=(4 * C, C), db1=(4 * C,))
    fills = dict(dxn=7.0, G=inp["G0"], S=inp["S0"], dW1=inp["dW0"], db1=inp["db0"])   # dxn is written, the others added to
    bufs, out = {}, {}
    for k, s in shapes.items():
        bufs[k], flat = guarded(int(torch.tensor(s).prod()), F32, dev, fills[k])
        out[k] = flat.view(s)
    ops.cnt_mlp_bwd(t16["xn"], t16["dy"], t16["w1"], t16["w2g"], inp["b1"], out["dxn"], out["G"], out["S"], out["dW1"],
                    out["db1"], deterministic=det)
    torch.cuda.synchronize()
    return out, all(intact(b) for b in bufs.values())


def check_mlp_bwd(log, case, inp, base, prec, planes, slices, det=False):
    ref, bound = R.mlp_bwd_ref(inp, base, prec, planes, slices)
    got, whole = run_mlp_bwd(inp, prec, planes, det)
    log.check(case, got, ref, bound)     # dxn plane by plane: ref["dxn"][s] = da[:, slice s] @ W1[slice s]
    log.exact(case, "sentinels around all five outputs intact", whole)
    dark = ~(inp["dy"] != 0).any(1)
    if bool(dark.any()):
        log.exact(case, f"dxn of the {int(dark.sum())} rows with dy = 0 is exactly 0", not got["dxn"][:, dark].any().item())
    return got


@pytest.mark.parametrize("C,Rr,prec", [(c, r, p) for c, r in ((64, 32967), (128, 8265)) for p in R.PRECS])
def test_mlp_bwd_third_trip_alone(cuda, C, Rr, prec):
    """The three-tile cases again with the spotlight on the third trip only (its four / two tiles and 64 rows elsewhere):
    with the whole second trip lit, G, dW1 and their bounds are sums over half the rows, and the share of one third-trip
    tile in them is smaller than the 16-bit rounding of the rest."""
    inp, base, slices, planes, tiles = mlp_case(C, Rr, cuda, trip=2)
    lit = int((inp["dy"] != 0).any(1).sum())
    assert lit == Rr - 2 * slices * 64 + 64, lit
    log = Log()
    check_mlp_bwd(log, f"mlp_bwd-{prec}-C{C}-R{Rr} trip 3 ({lit} rows lit)", inp, base, prec, planes, slices)
    log.done()


@pytest.mark.parametrize("C,Rr,prec", [(c, r, p) for c, r in MLP_BWD_SHAPES for p in R.PRECS])
def test_mlp_bwd(cuda, C, Rr, prec):
    """One workgroup per tile up to 256 (C = 64) / 64 (C = 128) tiles, then the grid stride: 16385 / 4097 rows give the
    first workgroup a second trip that is a one-row tile, 32967 / 8265 rows give the first workgroups three tiles (both
    row-buffer parities) and a ragged last tile."""
    inp, base, slices, planes, tiles = mlp_case(C, Rr, cuda)
    assert planes == (4 if C == 128 else 1)
    if Rr in (16385, 4097):
        assert tiles == slices + 1 and Rr - 64 * slices == 1, (tiles, slices)
    elif Rr in (32967, 8265):
        assert 2 * slices < tiles < 3 * slices and Rr % 64 != 0, (tiles, slices)
    else:
        assert slices == tiles
    log = Log()
    check_mlp_bwd(log, f"mlp_bwd-{prec}-C{C}-R{Rr} ({tiles} tiles / {slices})", inp, base, prec, planes, slices)
    log.done()


@pytest.mark.parametrize("C,Rr,prec", [(c, r, p) for c, r in ((64, 225), (64, 16385), (128, 129), (128, 8265)) for p in R.PRECS])
def test_mlp_bwd_deterministic(cuda, C, Rr, prec):
    """deterministic = 1: db1 and S through partial rows and det_reduce_kernel; two runs agree bit for bit in every
    output and stay inside the bounds."""
    inp, base, slices, planes, tiles = mlp_case(C, Rr, cuda)
    log = Log()
    case = f"mlp_bwd-det-{prec}-C{C}-R{Rr}"
    a = check_mlp_bwd(log, case, inp, base, prec, planes, slices, det=True)
    b, _ = run_mlp_bwd(inp, prec, planes, det=True)
    for k in a:
        log.exact(case, f"{k} of two runs bit-identical", torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)))
    log.done()


# ---- s2mlp_bwd
def s2_rows():
    rw = ops.cnt_s2mlp_bwd_rows()
    return rw, (1, 9, rw - 1, rw, rw + 1, 2 * rw + 1, 216)


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("which", range(7))
def test_s2mlp_bwd(cuda, which, prec):
    """R = 1, 9, rw - 1, rw, rw + 1, 2 rw + 1, 216 (rw rows per workgroup, from the launcher): da's live rows and dxn inside
    the bounds, the last workgroup's dead rows of da zero, everything behind them as it was."""
    rw, rows = s2_rows()
    assert 16 <= rw <= 48
    Rr = rows[which]

    def make():
        inp = R.s2mlp_inputs(Rr, seed=Rr, dev=cuda)
        return inp, R.s2mlp_base(inp)
    inp, base = cached("s2", Rr, make)
    assert float(inp["a"].max()) == 6.0 and float(inp["a"].min()) == -6.0 and bool((inp["a"] == 0).any())
    T = R.DT[prec]
    ref, bound = R.s2mlp_ref(inp, base, prec)
    t16 = {k: inp[k].to(T) for k in ("dy", "a", "w2gt", "w1t")}
    bda, da = guarded((Rr + 48) * 1024, T, cuda, 7.0)
    bdx, dxn = guarded(Rr * 256, F32, cuda, 7.0)
    da = da.view(Rr + 48, 1024)
    ops.cnt_s2mlp_bwd(t16["dy"], t16["a"], t16["w2gt"], t16["w1t"], da, dxn.view(Rr, 256))
    torch.cuda.synchronize()
    log = Log()
    case = f"s2mlp_bwd-{prec}-R{Rr} (rw {rw})"
    log.check(case, dict(da=da[:Rr], dxn=dxn), ref, bound)
    stored = -(-Rr // rw) * rw
    assert stored <= Rr + 48
    log.exact(case, f"rows {Rr} .. {stored - 1} of da are zero", not da[Rr:stored].any().item())
    log.exact(case, f"rows {stored} .. {Rr + 47} of da untouched", bool((da[stored:] == 7.0).all()))
    log.exact(case, "sentinels around da and dxn intact", intact(bda) and intact(bdx))
    log.done()


# ---- fused_mlp
FUSED_SHAPES = [(c, m) for c in (64, 80, 128, 160) for m in (1, 31, 33, 255, 257, 675, 131073 if c == 64 else 65537)]


@pytest.mark.parametrize("C,M,prec", [(c, m, p) for c, m in FUSED_SHAPES for p in R.PRECS])
def test_fused_mlp(cuda, C, M, prec):
    """In place (xres NULL), xres == x passed explicitly, and xres in another buffer (which stays as it was).  M = 131073
    (C = 64: 513 row tiles on 512 workgroups) and 65537 (257 tiles on 256 workgroups) make the first workgroup take a
    second tile; at C = 80 that carries the odd five-chunk filter ring's parity over."""
    def make():
        inp = R.fused_inputs(C, M, seed=1000 * C + M, dev=cuda)
        return inp, R.fused_base(inp)
    inp, base = cached("fused", (C, M), make)
    T = R.DT[prec]
    xn = inp["xn"].to(T)
    log = Log()
    refs = {res: R.fused_ref(inp, base, prec, res) for res in ("x0", "xres")}
    for mode in ("in place", "xres == x", "xres elsewhere"):
        bx, x = guarded(M * C, F32, cuda, inp["x0"])
        x = x.view(M, C)
        bres, xres = None, None
        if mode == "xres == x":
            xres = x
        elif mode == "xres elsewhere":
            bres, xres = guarded(M * C, F32, cuda, inp["xres"])
            xres = xres.view(M, C)
        ops.cnt_fused_mlp(xn, inp["w1"], inp["w2"], inp["b1"], inp["b2"], inp["gamma"], x, xres)
        torch.cuda.synchronize()
        case = f"fused_mlp-{prec}-C{C}-M{M} {mode}"
        ref, bound = refs["xres" if mode == "xres elsewhere" else "x0"]
        log.check(case, dict(x=x), ref, bound)
        log.exact(case, "sentinels around x intact", intact(bx))
        if bres is not None:
            log.exact(case, "xres and its sentinels unchanged", intact(bres) and torch.equal(xres, inp["xres"]))
    log.done()


# ---- fc2_grads
@pytest.mark.parametrize("C,H", [(64, 256), (80, 320), (128, 512), (160, 640), (256, 1024), (512, 2048)])
def test_fc2_grads(cuda, C, H):
    inp = R.fc2_inputs(C, H, seed=C, dev=cuda)
    ref, bound = R.fc2_ref(inp)
    bufs = dict(G=guarded(C * H, F32, cuda, inp["G"]), S=guarded(C, F32, cuda, inp["S"]), dW2=guarded(C * H, F32, cuda, 7.0),
                db2=guarded(C, F32, cuda, 7.0), dgamma=guarded(C, F32, cuda, 7.0))
    v = {k: b[1] for k, b in bufs.items()}
    ops.cnt_fc2_grads(v["G"].view(C, H), v["S"], inp["w2"], inp["b2"], inp["gamma"], v["dW2"].view(C, H), v["db2"], v["dgamma"])
    torch.cuda.synchronize()
    log = Log()
    case = f"fc2_grads-{C}x{H}"
    log.check(case, {k: v[k] for k in ref}, ref, bound)
    log.exact(case, "G and S are all zero afterwards", not v["G"].any().item() and not v["S"].any().item())
    log.exact(case, "sentinels around all five buffers intact", all(intact(b[0]) for b in bufs.values()))
    log.done()


# ---- refusals
def test_refusals_launch_nothing(cuda):
    """f32 / fp8, a width without a kernel, a null pointer and a negative row count come back as BTSBOT_ERR_INVALID_ARG
    with a message, zero rows as BTSBOT_OK; the sentinel-filled buffer that holds every tensor stays bit-identical."""
    L = _lib.lib()
    SLOT = 1 << 18   # bytes per tensor slot: whatever a one-row call would touch
    buf = torch.empty(12 * SLOT // 4, dtype=torch.int32, device=cuda).fill_(SENTINEL[4][1])
    snap = buf.clone()
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    NULL = ctypes.c_void_p(0)
    BF16, F16, F32P, FP8 = (_lib.PRECISION[k] for k in ("bf16", "f16", "f32", "fp8"))

    def P(i):
        return ctypes.c_void_p(buf.data_ptr() + SLOT * i)

    def mlp(prec, C, Rr, first=None):
        return L.btsbot_op_cnt_mlp_bwd(prec, C, P(0) if first is None else first, P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), P(9), Rr, 0, st)

    def s2(prec, C, Rr, first=None):
        return L.btsbot_op_cnt_s2mlp_bwd(prec, C, P(0) if first is None else first, P(1), P(2), P(3), P(4), P(5), Rr, st)

    def fused(prec, C, M, first=None):
        return L.btsbot_op_cnt_fused_mlp(prec, C, P(0) if first is None else first, P(1), P(2), P(3), P(4), P(5), NULL, P(6), M, st)

    def fc2(C, H, first=None):
        return L.btsbot_op_cnt_fc2_grads(P(0) if first is None else first, P(1), P(2), P(3), P(4), P(5), P(6), P(7), C, H, st)

    refused = {
        "mlp_bwd f32": lambda: mlp(F32P, 64, 1), "mlp_bwd fp8": lambda: mlp(FP8, 64, 1),
        "mlp_bwd C=256": lambda: mlp(BF16, 256, 1), "mlp_bwd null": lambda: mlp(F16, 64, 1, NULL),
        "mlp_bwd R<0": lambda: mlp(BF16, 128, -1),
        "s2mlp_bwd f32": lambda: s2(F32P, 256, 1), "s2mlp_bwd fp8": lambda: s2(FP8, 256, 1),
        "s2mlp_bwd C=64": lambda: s2(BF16, 64, 1), "s2mlp_bwd null": lambda: s2(F16, 256, 1, NULL),
        "s2mlp_bwd R<0": lambda: s2(F16, 256, -1),
        "fused_mlp f32": lambda: fused(F32P, 64, 1), "fused_mlp fp8": lambda: fused(FP8, 64, 1),
        "fused_mlp C=96": lambda: fused(BF16, 96, 1), "fused_mlp null": lambda: fused(F16, 80, 1, NULL),
        "fused_mlp M<0": lambda: fused(F16, 160, -1),
        "fc2_grads null": lambda: fc2(64, 256, NULL), "fc2_grads C=0": lambda: fc2(0, 256),
        "mlp_bwd_planes C=256": lambda: L.btsbot_op_cnt_mlp_bwd_planes(256),
        "mlp_bwd_slices R<0": lambda: L.btsbot_op_cnt_mlp_bwd_slices(64, -1),
    }
    for name, call in refused.items():
        rc = call()
        msg = L.btsbot_last_error().decode()
        print(f"{name}: {rc} '{msg}'")
        assert rc == _lib.ERR_INVALID_ARG and msg, (name, rc, msg)
    for name, call in {"mlp_bwd R=0": lambda: mlp(BF16, 64, 0), "s2mlp_bwd R=0": lambda: s2(F16, 256, 0),
                       "fused_mlp M=0": lambda: fused(BF16, 80, 0)}.items():
        rc = call()
        print(f"{name}: {rc}")
        assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    assert torch.equal(buf, snap)
    # and the tensor wrapper raises
    z = torch.zeros(1, 256, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(_lib.BtsbotHipError, match="no kernel"):
        ops.cnt_mlp_bwd(z, z, torch.zeros(1024, 256, dtype=torch.bfloat16, device=cuda),
                        torch.zeros(1024, 256, dtype=torch.bfloat16, device=cuda), torch.zeros(1024, device=cuda),
                        torch.zeros(1, 256, device=cuda), torch.zeros(256, 1024, device=cuda), torch.zeros(256, device=cuda),
                        torch.zeros(1024, 256, device=cuda), torch.zeros(1024, device=cuda))
