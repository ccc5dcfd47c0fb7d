"""What tests/stage2_ref.py's bounds see, on the CPU: the emulation of stage2p_kernel's arithmetic stays inside the derived
bound on every case of every mode, width and form (inference, keeping, row-tile), every seeded fault leaves it in every
mode it applies to, the spotlight maps have the properties claimed, the host unpacker inverts the three fragment layouts
and the float64 reference is the oracle's stage 2 + downsample.  test_gpu_stage2_ops.py holds the kernel to the same
reference and bound.  Run with -s for the worst err / bound per case."""
import pytest
import torch

import stage2_ref as R
from oracle import convnext_oracle as O

B_CPU = 6            # G = 4: a full workgroup and a ragged one; G = 5: one alert in the second; every alert kind of maps_x
CASES = {"dense one depth 1": lambda C: (R.dense_blocks(C, ("one",), 16), R.dense_down(C, 36)),
         "dense init/one": lambda C: (R.dense_blocks(C, ("init", "one"), 11), R.dense_down(C, 31)),
         "dense zero/tenth": lambda C: (R.dense_blocks(C, ("zero", "tenth"), 12), R.dense_down(C, 32)),
         "spotlight": lambda C: (R.spot_blocks(C, 2, 13), R.spot_down(C, 33)),
         "spotlight depth 1": lambda C: (R.spot_blocks(C, 1, 14), R.spot_down(C, 34)),
         "spotlight dense taps": lambda C: (R.spot_blocks(C, 1, 17, dw="dense"), R.spot_down(C, 37)),   # (maps_x's nearly constant pixel)
         "spotlight gamma 0": lambda C: (R.scale_gamma(R.spot_blocks(C, 1, 18), 0.0), R.spot_down(C, 38))}      # (the downsample on exact rows)
_memo = {}


def case(C, name):
    if (C, name) not in _memo:
        blocks, down = CASES[name](C)
        _memo[C, name] = (R.maps_x(C, B_CPU, 5, blocks[0]), blocks, down)
    return _memo[C, name]


def reference(C, name, prec, keep=False):
    key = (C, name, prec, keep)
    if key not in _memo:
        x, blocks, down = case(C, name)
        _memo[key] = R.stage2_ref(x, blocks, down, prec, keep=keep)
    return _memo[key]


def worst(got, ref, keep):
    """{what: worst err / bound} of an emulate()-shaped result against a stage2_ref()-shaped one"""
    r = {k: R.ratio(got[k], *ref[k]) for k in ("out", "tap")}
    if keep:
        r["patches"] = R.ratio(got["patches"], *ref["patches"])
        for j, kb in enumerate(ref["keep"]):
            for n, (v, e) in kb.items():
                r[f"{n}[{j}]"] = R.ratio(got["keep"][j][n], v, e)
    return r


@pytest.mark.parametrize("C,prec,keep", [(C, p, False) for C in R.WIDTHS for p in R.PRECS_AT[C]] + [(256, p, True) for p in R.KEEP_PRECS])
def test_emulation_stays_inside_the_bound(C, prec, keep):
    bad = []
    for name in CASES:
        x, blocks, down = case(C, name)
        ref = reference(C, name, prec, keep)
        r = worst(R.emulate(x, blocks, down, prec, keep=keep), ref, keep)
        rel = (ref["out"][1] / (ref["out"][0].abs() + 1e-30)).median().item()
        print(f"{prec:6s} C={C} keep={keep} {name:18s} " + " ".join(f"{k} {v:.3f}" for k, v in r.items()) + f"   (median bound / |out| {rel:.2e})")
        bad += [(name, k, v) for k, v in r.items() if R.outside(v)]
    assert not bad, bad


@pytest.mark.parametrize("prec", R.KEEP_PRECS)
def test_row_tile_emulation_stays_inside_the_bound(prec):
    for name in ("dense init/one", "spotlight"):
        x, blocks, _ = case(256, name)
        rows = x.reshape(-1, 256)
        for P in blocks:
            ref, bound = R.rows_ref(rows, P, prec)
            r = R.ratio(R.emulate_rows(rows, P, prec), ref, bound)
            print(f"rows {prec} {name}: worst err / bound {r:.3f}")
            assert r <= 1.0


def test_the_saturation_case_is_one():
    """its alert's hidden activation leaves e4m3's range in the float64 reference, nothing else does, and the emulation (which
    clamps, as the kernel) stays inside the bound of the reference with g clamped"""
    C = 256
    down = R.spot_down(C, 35)
    x, x_plain, blocks, alert = R.saturating(C, 21)
    with pytest.raises(AssertionError, match="beyond e4m3"):
        R.stage2_ref(x, blocks, down, "fp8")
    R.stage2_ref(x_plain, blocks, down, "fp8")                      # the range check holds without the alert
    ref = R.stage2_ref(x, blocks, down, "fp8", saturate=True, clamp_g=True)
    got = R.emulate(x, blocks, down, "fp8")
    r = max(R.ratio(got[k], *ref[k]) for k in ("out", "tap"))
    free = R.stage2_ref(x, blocks, down, "fp8", saturate=True)["tap"][0]
    tap, bound = ref["tap"]
    moved = ((free - tap).abs() / bound)[alert].max().item()
    print(f"fp8 saturation: worst err / bound {r:.3f}; the clamp moves the alert's outputs by up to {moved:.1f} bounds")
    others = [b for b in range(x.shape[0]) if b != alert]
    assert r <= 1.0 and moved > 1.0 and bool(torch.equal(free[others], tap[others]))


def modes(fault):
    """(C, prec) pairs a fault applies to"""
    return [(C, p) for C in R.FAULT_WIDTHS.get(fault, (256,)) for p in R.FAULT_PRECS.get(fault, R.PRECS_AT[C])]


@pytest.mark.parametrize("fault", [f for f in R.FAULTS if f != "gelu_unrounded"])
def test_seeded_fault_leaves_the_bound(fault):
    """in every mode the fault applies to, on at least one case; the layout faults on a spotlight case"""
    layout = fault in ("swap_fc1_tile", "fc2_kstep_stale", "no_last_chunk", "planes_swapped", "ds_pixel", "ds_fp8",
                       "shared_tile_lead_only", "tap_row", "tap_col", "outer_ring", "wrap")
    for C, prec in modes(fault):
        seen = {}
        for name in CASES:
            x, blocks, down = case(C, name)
            ref = reference(C, name, prec)
            got = R.stage2_ref(x, blocks, down, prec, fault=fault, G=4)
            seen[name] = max(R.ratio(got[k][0], *ref[k]) for k in ("out", "tap"))
        print(f"{fault:22s} {prec:6s} C={C}  " + "  ".join(f"{k}: {v:.3g}" for k, v in seen.items()))
        assert any(R.outside(v) for k, v in seen.items() if k.startswith("spotlight") or not layout), (fault, prec, seen)


@pytest.mark.parametrize("prec", R.KEEP_PRECS)
def test_gelu_at_the_unrounded_pre_activation_shows_in_the_kept_pair(prec):
    """the bound against float64 has to admit the keeping form's rounding of a, so it cannot tell where the GELU was taken;
    the kept pair can: hh is the GELU of the a that was kept"""
    for name in ("dense init/one", "spotlight"):
        a64 = reference(256, name, prec, True)["keep"][0]["a"][0]
        good, bad = (R.pair_ratio(*R.kept_pair(a64, prec, f), prec) for f in (None, "gelu_unrounded"))
        print(f"kept pair {prec} {name}: as the kernel {good:.3f}, GELU at the unrounded a {bad:.3f}")
        assert good <= 1.0 and R.outside(bad)
        emu = R.emulate(*case(256, name), prec, keep=True)["keep"][0]
        assert R.pair_ratio(emu["a"], emu["hh"], prec) <= 1.0


def test_spotlight_maps():
    """depthwise: one or two central taps per channel, the channels of a block cover all 25 (every output / input pixel
    pair), the ring dense; fc1 / fc2: stage 3's maps -- every hidden unit in exactly one fc2 non-zero, a channel's four in
    four chunks of 128 and at four k positions of a fragment (16-bit k-step 32, fp8 128); the downsample: one non-zero per
    output, every patch pixel and channel read, values exact in bf16 / f16 and not in e4m3"""
    for C in R.WIDTHS:
        H = 4 * C
        c1, c2, hid = R.spot_maps(C)
        assert sorted(hid.reshape(-1).tolist()) == list(range(H))
        assert all(len(set((row // R.CHUNK).tolist())) == 4 for row in hid)
        assert all(len(set((row % 32).tolist())) == 4 and len(set((row % 128).tolist())) == 4 for row in hid)
        assert set((hid.reshape(-1) // R.CHUNK).tolist()) == set(range(H // R.CHUNK))
        for j, P in enumerate(R.spot_blocks(C, 2, 13)):
            w = P["dw_w"][:, 0]
            nz = (w[:, 1:6, 1:6] != 0).reshape(C, 25)
            assert bool(((nz.sum(1) == 1) | (nz.sum(1) == 2)).all()) and bool(nz.any(0).all())
            ring = w.clone()
            ring[:, 1:6, 1:6] = 1.0
            assert bool((ring != 0).all())
            M = R.dw_matrix(P["dw_w"])
            assert bool((M != 0).any(0).all())                       # every (output, input) pixel pair, over the channels
            nz1, nz2 = (P["fc1_w"] != 0).sum(1), (P["fc2_w"] != 0).sum(1)
            assert bool(((nz1 == 1) | (nz1 == 2)).all()) and bool((nz2 == 4).all()) and bool(((P["fc2_w"] != 0).sum(0) == 1).all())
            for v in (P["fc1_w"], P["fc2_w"], P["fc2_w"] * P["gamma"][:, None]):     # exact in every operand type
                for prec in ("bf16", "f16", "fp8"):
                    assert torch.equal(v.to(R.ODT[prec]).float(), v), prec
        D = R.spot_down(C, 33)
        Wd = R.reorder_down(D["ds_w"])
        q, c = R.spot_down_map(C)
        assert bool(((Wd != 0).sum(1) == 1).all()) and torch.equal(Wd.abs().argmax(1), q * C + c)
        assert set(q.tolist()) == {0, 1, 2, 3} and set(c.tolist()) == set(range(C))
        assert torch.equal(Wd.bfloat16().float(), Wd) and torch.equal(Wd.half().float(), Wd)
        assert bool((Wd.to(R.ODT["fp8"]).float() != Wd)[Wd != 0].all())


@pytest.mark.parametrize("prec", R.PRECS)
def test_unpack_inverts_the_host_packer(prec):
    g = torch.Generator().manual_seed(3)
    for rows, K in ((16, 128), (48, 256), (1024, 256), (256, 1024), (640, 1280)):
        w = torch.randn(rows, K, generator=g)
        vals = R.host_round(prec, w, scale=8.0 if prec == "fp8" else None)
        img = R.pack_s2p_host(vals, prec)
        assert img.numel() == rows * K * R.ESZ[prec]
        pos = R.frag_pos(prec, rows, K).reshape(-1)
        if prec == "f16x2":                                         # heads in the first half of every 1024 values
            assert bool((pos % 1024 < 512).all())
            pos = pos // 1024 * 512 + pos % 1024
        assert sorted(pos.tolist()) == list(range(rows * K))       # a bijection
        back = R.unpack_s2p(img, prec, rows, K)
        for a, b in zip(back if prec == "f16x2" else (back,), vals if prec == "f16x2" else (vals,)):
            assert torch.equal(R.bits(a), R.bits(b)), (rows, K)
    # the layout comments, spot-checked by hand: 16-bit, tile 0, k-step 1, lane 37 (row 5, k-group 2), j 3: k = 32 + 16 + 3;
    # fp8: k-step 0, lane 37, j 21: k = 64 + 21, in the second half-kilobyte at [lane][5]
    if prec in ("bf16", "f16"):
        assert int(R.frag_pos(prec, 16, 64)[5, 51]) == (1 * 64 + 37) * 8 + 3
    if prec == "f16x2":
        assert int(R.frag_pos(prec, 16, 64)[5, 51]) == 1 * 1024 + 37 * 8 + 3
    if prec == "fp8":
        assert int(R.frag_pos(prec, 16, 128)[5, 85]) == 1024 + 37 * 16 + 5


def test_reorder_down():
    for rows, cin in ((16, 32), (512, 256), (640, 320)):
        w = torch.arange(rows * cin * 4, dtype=torch.float32).view(rows, cin, 2, 2)
        m = R.reorder_down(w)
        assert m.shape == (rows, 4 * cin)
        for row, ky, kx, c in ((0, 0, 0, 0), (rows - 1, 1, 0, cin - 1), (3, 0, 1, 7), (5, 1, 1, 2)):
            assert float(m[row, (2 * ky + kx) * cin + c]) == float(w[row, c, ky, kx])
        assert sorted(m.reshape(-1).tolist()) == list(range(rows * cin * 4))


@pytest.mark.parametrize("arch,C", (("convnext_pico", 256), ("convnext_nano", 320)))
def test_reference_is_the_oracles_stage_2(arch, C):
    """stage2_ref with the oracle's erf GELU and epsilon against oracle/convnext_oracle.py's blocks and downsample in
    float64, on a seeded state dict: equal to float64 rounding"""
    sd = {k: v.double() for k, v in O.random_state_dict(O.backbone_param_shapes(arch, "", False), 3).items()}
    depth = O.ARCHS[arch]["depths"][2]
    names = dict(dw_w="conv_dw.weight", dw_b="conv_dw.bias", ln_w="norm.weight", ln_b="norm.bias", fc1_w="mlp.fc1.weight",
                 fc1_b="mlp.fc1.bias", fc2_w="mlp.fc2.weight", fc2_b="mlp.fc2.bias", gamma="gamma")
    blocks = [{k: sd[f"stages.2.blocks.{j}.{n}"].reshape(4 * C, C) if k == "fc1_w" else
               sd[f"stages.2.blocks.{j}.{n}"].reshape(C, 4 * C) if k == "fc2_w" else sd[f"stages.2.blocks.{j}.{n}"]
               for k, n in names.items()} for j in range(depth)]
    down = dict(ds_ln_w=sd["stages.3.downsample.0.weight"], ds_ln_b=sd["stages.3.downsample.0.bias"],
                ds_w=sd["stages.3.downsample.1.weight"], ds_b=sd["stages.3.downsample.1.bias"])
    x = torch.randn(3, 9, C, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    t = x.permute(0, 2, 1).reshape(3, C, 3, 3)
    for j in range(depth):
        t = O.block(t, sd, f"stages.2.blocks.{j}.")
    want_tap = t.reshape(3, C, 9).permute(0, 2, 1)
    t = O.layer_norm_c(t, down["ds_ln_w"], down["ds_ln_b"])
    want_out = torch.nn.functional.conv2d(t, down["ds_w"], down["ds_b"], stride=2).reshape(3, 2 * C)
    got = R.stage2_ref(x, blocks, down, "f16", gelu="erf", ln_eps=O.LN_EPS, bound=False)
    for k, want in (("tap", want_tap), ("out", want_out)):
        err = ((got[k][0] - want).abs() / (want.abs() + 1.0)).max().item()
        print(f"{arch} {k}: max |ref - oracle| / (|oracle| + 1) = {err:.2e}")
        assert err < 1e-12
