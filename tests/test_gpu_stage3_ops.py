"""The last ConvNeXt stage ALONE (btsbot_op_cn_stage3, btsbot_op_cn_pack_s3, btsbot_op_cn_fp8_scale: infer_ops.hip over
stage3.hip) against the float64 reference and the derived per-element bound of tests/stage3_ref.py, whose docstring holds
the derivation; tests/test_stage3_reference.py shows on the CPU what the bound sees and that every seeded fault leaves it.

  s3_fc1_kernel / s3_fc2_kernel, narrow and wide tiles, + the packers       test_stage3[prec-C-tiles], test_stage3_depth
  wide tiles against narrow tiles (512 and 640 channels)                    test_wide_tiles_give_the_narrow_tiles_bits
  clamped duplicate rows, the half of hfrag no fc1 tile wrote               test_rows_do_not_depend_on_their_neighbours
  fp8's clamp in front of the conversion                                    test_fp8_saturation
  pack_s3_kernel<bf16 / f16>, pack_s3_split_kernel, pack_s3_fp8_kernel      test_pack_s3[prec]
  absmax_kernel, scale_from_max_kernel                                      test_fp8_scale
  the entry point's argument checks                                         test_stage3_refusals

x is a slice of a larger buffer: sentinel head and tail, and two rows past B, must survive.  hfrag starts as 0xFF bytes
(NaN in every operand type) inside the entry point.  Sizes and support come from the library (cn_stage3_supported,
cn_stage3_hfrag_bytes).  Each test prints its worst err / bound per case (run with -s) and asserts at the end.

Worst err / bound on an MI355X over the seven row counts (a record, not a tolerance; wide tiles give the narrow tiles'
figures, as they give their bits):
  test_stage3                  512 channels: dense  spotlight     640 channels: dense  spotlight
    bf16                                     0.003  0.443                       0.008  0.503
    f16                                      0.003  0.409                       0.012  0.472
    fp8                                      0.003  0.469                       0.007  0.438
    f16x2                                    0.003  0.040                       0.022  0.030
  test_stage3_depth            depth 1: bf16 0.003 / 0.573, fp8 0.003 / 0.545;  depth 4: bf16 0.000 / 0.198, fp8 0.000 / 0.174
  test_fp8_saturation          0.581 (512 channels), 0.531 (640)
  test_pack_s3                 every image bit for bit;  test_fp8_scale: S = 2^k at every m = 240 2^-k (never 2^(k-1))
(the dense figures are small because the worst-case bound over 512 .. 2560 products is wide; the spotlight cases are the
sharp ones.  Past two blocks the bound grows through every LayerNorm: the depth-4 call is pinned by its equality with four
one-block calls.)
"""
import functools
import math

import pytest
import torch

import stage3_ref as R
from btsbot_amd import _lib, ops

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
PAD = 1024
SENT = 0x7FC5A5A5
FILL = 7.0e3           # no result of these cases comes near it
B_MAX = max(R.B_LIST)
TILES = {"bf16": ("narrow", "wide"), "f16": ("narrow", "wide"), "fp8": ("narrow", "wide"), "f16x2": ("narrow",)}
KINDS = {"dense init/one": lambda C, depth: R.dense_blocks(C, ("init", "one"), 11),
         "dense zero/tenth": lambda C, depth: R.dense_blocks(C, ("zero", "tenth"), 12),
         "dense": lambda C, depth: R.dense_blocks(C, ("init", "zero", "tenth", "one")[-depth:], 15),
         "spotlight": lambda C, depth: R.spot_blocks(C, depth, 13)}


def guarded_rows(x, extra, dev):
    """[PAD sentinel | x's rows | `extra` rows of FILL | PAD sentinel] on the device -> (buffer, the rows [B + extra][C])"""
    B, C = x.shape
    buf = torch.empty((B + extra) * C + 2 * PAD, dtype=F32, device=dev)
    buf.view(torch.int32).fill_(SENT)
    rows = buf[PAD:PAD + (B + extra) * C].view(B + extra, C)
    rows[:B].copy_(x)
    rows[B:].fill_(FILL)
    return buf, rows


def intact(buf, rows, B):
    b = buf.view(torch.int32)
    return bool((b[:PAD] == SENT).all()) and bool((b[-PAD:] == SENT).all()) and bool((rows[B:] == FILL).all())


class Log:
    def __init__(self):
        self.bad = []

    def check(self, case, got, ref, bound):
        r = R.ratio(got.detach().cpu(), ref, bound)
        print(f"{case:64s} {r:.3f}   (worst err / bound)")
        if R.outside(r):
            self.bad.append(f"{case}: err / bound = {r:.4g}")
        return r

    def exact(self, case, what, ok):
        if not ok:
            print(f"{case:64s} {what}: NO")
            self.bad.append(f"{case}: {what}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


@functools.lru_cache(maxsize=None)
def case(C, kind, depth):
    """(x [B_MAX][C], blocks) on the CPU; a call of B rows takes the first B"""
    blocks = KINDS[kind](C, depth)
    assert len(blocks) == depth
    return R.rows_x(C, B_MAX, 5, blocks[0]), blocks


@functools.lru_cache(maxsize=None)
def reference(C, kind, depth, prec):
    """(ref, bound) [B_MAX][C]: a row's result does not depend on the other rows, so every B reads its first B rows"""
    x, blocks = case(C, kind, depth)
    return R.stage3_ref(x, blocks, prec)


@functools.lru_cache(maxsize=None)
def on_device(C, kind, depth, dev):
    return [{k: v.to(dev) for k, v in P.items()} for P in case(C, kind, depth)[1]]


def run(prec, x, blocks_dev, wide, dev, log=None, label=""):
    """the entry point on a guarded copy of x -> the B rows (device); sentinels and the rows past B are checked"""
    B = x.shape[0]
    buf, rows = guarded_rows(x, 2, dev)
    ops.cn_stage3(prec, rows[:B], blocks_dev, wide=wide)
    torch.cuda.synchronize()
    ok = intact(buf, rows, B)
    if log is not None:
        log.exact(label, "sentinels and the rows past B intact", ok)
    else:
        assert ok, label
    return rows[:B].clone()


@pytest.mark.parametrize("prec,C,tiles", [(p, C, t) for p in R.PRECS for C in R.WIDTHS for t in TILES[p]])
def test_stage3(cuda, prec, C, tiles):
    """two blocks on dense and spotlight inputs at every row count around the 32-row fc1 block and the 64-row fc2 tile"""
    assert ops.cn_stage3_supported(prec, C, 2)
    log = Log()
    for kind in ("dense init/one", "dense zero/tenth", "spotlight"):
        x = case(C, kind, 2)[0]
        ref, bound = reference(C, kind, 2, prec)
        blocks = on_device(C, kind, 2, cuda)
        for B in R.B_LIST:
            assert ops.cn_stage3_hfrag_bytes(prec, C, B) >= B * 4 * C * (1 if prec == "fp8" else R.ESZ[prec])
            label = f"stage3 {prec} C={C} {tiles} {kind} B={B}"
            got = run(prec, x[:B], blocks, tiles == "wide", cuda, log, label)
            log.exact(label, "finite", bool(torch.isfinite(got).all()))
            log.check(label, got, ref[:B], bound[:B])
    log.done()


@pytest.mark.parametrize("prec", ("bf16", "fp8"))
@pytest.mark.parametrize("depth", (1, 4))
def test_stage3_depth(cuda, prec, depth):
    """one block and S3_MAX_DEPTH blocks against the reference; the worst-case bound grows through every LayerNorm, so
    what pins the deep call is that it equals, bit for bit, its blocks run one call at a time"""
    C, B = 512, 33
    assert ops.cn_stage3_supported(prec, C, depth)
    log = Log()
    for kind in ("dense", "spotlight"):
        x = case(C, kind, depth)[0]
        ref, bound = reference(C, kind, depth, prec)
        label = f"stage3 {prec} C={C} depth {depth} {kind} B={B}"
        got = run(prec, x[:B], on_device(C, kind, depth, cuda), False, cuda, log, label)
        log.exact(label, "finite", bool(torch.isfinite(got).all()))
        log.check(label, got, ref[:B], bound[:B])
        step = x[:B]
        for P in on_device(C, kind, depth, cuda):
            step = run(prec, step, [P], False, cuda, log, label)
        log.exact(label, "equal to its blocks run one at a time", torch.equal(step.view(torch.int32), got.view(torch.int32)))
    log.done()


@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("prec", ("bf16", "f16", "fp8"))
def test_wide_tiles_give_the_narrow_tiles_bits(cuda, prec, C):
    for kind in ("dense init/one", "spotlight"):
        x = case(C, kind, 2)[0]
        blocks = on_device(C, kind, 2, cuda)
        for B in (1, 33, 65):
            narrow, wide = (run(prec, x[:B], blocks, w, cuda, label=f"{kind} B={B}") for w in (False, True))
            assert torch.equal(narrow.view(torch.int32), wide.view(torch.int32)), (kind, B)


@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("prec", R.PRECS)
def test_rows_do_not_depend_on_their_neighbours(cuda, prec, C):
    """row r of a 65-row call = the same row run alone (B = 1: 31 clamped duplicates beside it, the second half of hfrag
    unwritten) = the same row as the last of 33 (alone in its fc1 block, the unwritten half again), bit for bit"""
    x = case(C, "dense init/one", 2)[0]
    blocks = on_device(C, "dense init/one", 2, cuda)
    for tiles in TILES[prec]:
        wide = tiles == "wide"
        full = run(prec, x[:65], blocks, wide, cuda).view(torch.int32)
        for r in (0, 1, 31, 32, 47, 64):
            alone = run(prec, x[r:r + 1], blocks, wide, cuda).view(torch.int32)
            others = torch.cat([x[:r], x[r + 1:]])[:32]
            last = run(prec, torch.cat([others, x[r:r + 1]]), blocks, wide, cuda).view(torch.int32)
            assert torch.equal(alone[0], full[r]), (tiles, r, "alone")
            assert torch.equal(last[32], full[r]), (tiles, r, "last of 33")


@pytest.mark.parametrize("C", R.WIDTHS)
def test_fp8_saturation(cuda, C):
    log = Log()
    x, x_plain, blocks, row = R.saturating(C, 21)
    free = R.stage3_ref(x, blocks, "fp8", saturate=True)[0]
    ref, bound = R.stage3_ref(x, blocks, "fp8", saturate=True, clamp_g=True)
    assert float(((free - ref).abs() / bound)[row].max()) > 1.0          # the clamp is visible in this row
    dev = [{k: v.to(cuda) for k, v in P.items()} for P in blocks]
    for wide in (False, True):
        label = f"fp8 saturation C={C} {'wide' if wide else 'narrow'}"
        got = run("fp8", x, dev, wide, cuda, log, label)
        plain = run("fp8", x_plain, dev, wide, cuda, log, label)
        log.exact(label, "finite", bool(torch.isfinite(got).all()))
        log.check(label, got, ref, bound)
        keep = [r for r in range(x.shape[0]) if r != row]
        log.exact(label, "the other rows keep their bits", torch.equal(got[keep].view(torch.int32), plain[keep].view(torch.int32)))
    log.done()


def pack_input(prec, rows, K, with_rowscale, seed):
    """fp32 w [rows][K] (and rowscale [rows] or None) with, in rows 0 .. 3 (rowscale 1, 1/2, 2, 1): exact ties of the
    format, f16 subnormals, ties among them, negative zeros.  The largest |w rowscale| is 0.75 (row 3, rowscale 1), so the
    fp8 scale is 256 in every case."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(rows, K, generator=g) * K ** -0.5).clamp(-0.3, 0.3)
    rs = None
    if with_rowscale:
        rs = 0.5 + torch.rand(rows, generator=g)
        rs[:4] = torch.tensor([1.0, 0.5, 2.0, 1.0])
    tie = {"bf16": [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)], "f16": [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11)],
           "f16x2": [1 + 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -22, 1 + 3 * 2.0 ** -22],
           "fp8": [17 / 16, 19 / 16, -17 / 16, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -7 * 17 / 16]}[prec]
    unit = 2.0 ** -8 if prec == "fp8" else 2.0 ** -3      # fp8: times the scale 256 the ties are the format's
    special = [t * unit for t in tie] + [2.0 ** -20, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -3 * 2.0 ** -25, 2.0 ** -26, -0.0, 0.0]
    for r in range(3):
        w[r, :len(special)] = torch.tensor(special, dtype=F32)
        w[r, K - len(special):] = -torch.tensor(special, dtype=F32)
    w[3, 5] = -0.75
    return w, rs


@pytest.mark.parametrize("prec", R.PRECS)
def test_pack_s3(cuda, prec):
    bad = []
    for rows, K in ((2048, 512), (512, 2048), (2560, 640), (640, 2560)):
        for with_rowscale in (False, True):
            for swap in (False, True):
                w, rs = pack_input(prec, rows, K, with_rowscale, rows + swap)
                n = rows * K * R.ESZ[prec]
                buf = torch.full((n + 2 * PAD,), 0xA5, dtype=torch.uint8, device=cuda)
                sbuf = torch.full((2 + 2 * PAD,), FILL, dtype=F32, device=cuda)
                dst, scale = buf[PAD:PAD + n], sbuf[PAD:PAD + 2]
                ops.cn_pack_s3(prec, w.to(cuda), rs.to(cuda) if rs is not None else None, swap23=swap, dst=dst,
                               scale=scale if prec == "fp8" else None)
                torch.cuda.synchronize()
                label = f"pack_s3 {prec} {rows}x{K} rowscale={with_rowscale} swap23={swap}"
                guards = bool((buf[:PAD] == 0xA5).all()) and bool((buf[-PAD:] == 0xA5).all()) and bool((sbuf[:PAD] == FILL).all()) \
                    and bool((sbuf[-PAD:] == FILL).all())
                S = None
                if prec == "fp8":
                    S = float(scale[0])
                    if S != 256.0 or float(scale[1]) != 1.0 / 256.0:
                        bad.append(f"{label}: scale {scale.tolist()}")
                        continue
                want = R.host_round(prec, w, rs, S)
                got = R.unpack_s3(dst.cpu(), prec, rows, K, swap, kperm=prec == "fp8" and not swap)
                pairs = zip(got, want) if prec == "f16x2" else ((got, want),)
                same = all(torch.equal(R.bits(a), R.bits(b)) for a, b in pairs)
                print(f"{label:64s} bit for bit: {same}   guards intact: {guards}")
                if not (same and guards):
                    bad.append(label)
    assert not bad, "\n".join(bad)


def test_fp8_scale(cuda):
    bad, edge = [], []

    def ask(label, src, m, rowscale=None, K=1, exact_k=None):
        buf = torch.full((2 + 2 * PAD,), FILL, dtype=F32, device=cuda)
        scale = buf[PAD:PAD + 2]
        ops.cn_fp8_scale(src.to(cuda), rowscale.to(cuda) if rowscale is not None else None, K=K, scale=scale)
        torch.cuda.synchronize()
        S, inv = float(scale[0]), float(scale[1])
        ok = bool((buf[:PAD] == FILL).all()) and bool((buf[-PAD:] == FILL).all())
        ok = ok and S > 0 and math.frexp(S)[0] == 0.5 and float(scale[0] * scale[1]) == 1.0 and inv * S == 1.0
        if m == 0:
            ok = ok and S == 1.0
        elif exact_k is not None:
            ok = ok and S in (2.0 ** exact_k, 2.0 ** (exact_k - 1))
            edge.append(f"k={exact_k}: 2^{int(math.log2(S))}")
        else:
            ok = ok and 120.0 < m * S <= 240.0
        if not ok:
            bad.append(f"{label}: m = {m!r} gave S = {S!r}, 1/S = {inv!r}")

    def vector(m, n=1000, at=17, seed=1):
        """n values below m / 2 in magnitude and the value m (with its sign) at `at`"""
        v = (torch.rand(n, generator=torch.Generator().manual_seed(seed)) - 0.5) * abs(m)
        v[at] = m
        return v

    for k in range(-3, 31):
        for f in (0.51, 0.75, 0.99):
            m = float(torch.tensor(240.0 * f, dtype=F32)) * 2.0 ** -k
            ask(f"m = 240 2^-{k} {f}", vector(m), m)
        ask(f"m = 240 2^-{k}", vector(240.0 * 2.0 ** -k), 240.0 * 2.0 ** -k, exact_k=k)
    ask("m = 0", torch.zeros(1000), 0.0)
    ask("the largest magnitude negative", vector(-3.0), 3.0)
    n = 2 * 65536 + 37                                   # the grid is 256 x 256 threads: the last element is in its tail
    ask("the largest magnitude last, in the grid-stride tail", vector(0.02, n=n, at=n - 1), 0.02)
    w = vector(0.7, n=4 * 64).view(4, 64)
    rs = torch.full((4,), 1e-6)
    ask("rowscale 1e-6", w, float((w * rs[:, None]).abs().max()), rowscale=rs, K=64)
    rs = torch.tensor([1.0, 0.0, 300.0, 1.0])            # the largest product is in the row with the largest rowscale
    ask("rowscale picks the row", w, float((w * rs[:, None]).abs().max()), rowscale=rs, K=64)
    print("S at m = 240 2^-k exactly: " + ", ".join(edge))
    assert not bad, "\n".join(bad)


def test_stage3_refusals(cuda):
    C, B = 512, 5
    x, blocks = case(C, "spotlight", 2)
    dev = on_device(C, "spotlight", 2, cuda)
    buf, rows = guarded_rows(x[:B], 2, cuda)
    before = rows.clone()

    def refused(word, prec="bf16", xs=rows[:B], blk=dev, wide=False, **kw):
        with pytest.raises(_lib.BtsbotHipError, match=word) as e:
            ops.cn_stage3(prec, xs, blk, wide=wide, **kw)
        assert f"({_lib.ERR_INVALID_ARG})" in str(e.value)
        torch.cuda.synchronize()
        assert intact(buf, rows, B) and torch.equal(rows, before), word      # nothing launched

    assert not ops.cn_stage3_supported("f32", C, 2) and not ops.cn_stage3_supported("bf16", 768, 2)
    assert not ops.cn_stage3_supported("bf16", C, 0) and not ops.cn_stage3_supported("bf16", C, 5)
    assert all(ops.cn_stage3_supported(p, c, d) for p in R.PRECS for c in R.WIDTHS for d in (1, 4))
    refused("unsupported", prec="f32")
    refused("unsupported", xs=rows.view(-1)[:B * 768], B=B, c3=768)
    refused("unsupported", blk=[])
    refused("unsupported", blk=dev + dev + dev[:1])
    refused("split mode has no wide tiles", prec="f16x2", wide=True)
    refused("null pointer", xs=None, B=B, c3=C)
    for k in R.PARAMS:
        refused("null pointer", blk=[dev[0], dict(dev[1], **{k: None})])
    refused("x must be 16-byte aligned", xs=buf[PAD + 1:PAD + 1 + B * C], B=B, c3=C)
    for k in ("dw_b", "ln_w", "ln_b", "fc1_b", "fc2_b", "gamma"):
        off = torch.cat([dev[1][k], dev[1][k][:4]])[1:1 + dev[1][k].numel()]
        assert off.data_ptr() % 16 == 4
        refused("parameter vectors must be 16-byte aligned", blk=[dev[0], dict(dev[1], **{k: off})])
    refused("negative row count", B=-1, c3=C)
    ops.cn_stage3("bf16", rows[:B], dev, B=0, c3=C)          # B == 0: OK, nothing touched
    torch.cuda.synchronize()
    assert intact(buf, rows, B) and torch.equal(rows, before)
    with pytest.raises(_lib.BtsbotHipError, match="bad shape"):
        ops.cn_pack_s3("bf16", torch.zeros(48, 64, device=cuda))
    with pytest.raises(_lib.BtsbotHipError, match="bad shape"):
        ops.cn_pack_s3("fp8", torch.zeros(64, 32, device=cuda))
