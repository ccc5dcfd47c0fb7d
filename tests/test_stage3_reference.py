"""What tests/stage3_ref.py's bounds see, on the CPU: the emulation of the stage-3 kernels' arithmetic stays inside the
derived bound on every case of every mode and width, every seeded fault leaves it in every mode it applies to, and the
host unpacker inverts the three fragment layouts.  test_gpu_stage3_ops.py holds the kernels to the same reference and
bound.  Run with -s for the worst err / bound per case."""
import pytest
import torch

import stage3_ref as R

B_CPU = 33          # two 32-alert blocks, the second with one live row: every row kind of rows_x, the fault rows
CASES = {"dense init/one": lambda C: R.dense_blocks(C, ("init", "one"), 11),
         "dense zero/tenth": lambda C: R.dense_blocks(C, ("zero", "tenth"), 12),
         "spotlight": lambda C: R.spot_blocks(C, 2, 13),
         "spotlight depth 1": lambda C: R.spot_blocks(C, 1, 14)}
_memo = {}


def case(C, name):
    if (C, name) not in _memo:
        blocks = CASES[name](C)
        _memo[C, name] = (R.rows_x(C, B_CPU, 5, blocks[0]), blocks)
    return _memo[C, name]


def reference(C, name, prec):
    key = (C, name, prec)
    if key not in _memo:
        x, blocks = case(C, name)
        _memo[key] = R.stage3_ref(x, blocks, prec)
    return _memo[key]


@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("prec", R.PRECS)
def test_emulation_stays_inside_the_bound(prec, C):
    bad = []
    for name in CASES:
        x, blocks = case(C, name)
        ref, bound = reference(C, name, prec)
        r = R.ratio(R.emulate(x, blocks, prec), ref, bound)
        rel = (bound / (ref.abs() + 1e-30)).median().item()
        print(f"{prec:6s} C={C} {name:18s} worst err / bound {r:.3f}   (median bound / |x| {rel:.2e})")
        if R.outside(r):
            bad.append((name, r))
    assert not bad, bad


def test_the_saturation_case_is_one():
    """its row's hidden activation leaves e4m3's range in the float64 reference, nothing else does, and the emulation
    (which clamps, as the kernel) stays inside the bound of the reference with g clamped"""
    for C in R.WIDTHS:
        x, x_plain, blocks, row = R.saturating(C, 21)
        with pytest.raises(AssertionError, match="beyond e4m3"):
            R.stage3_ref(x, blocks, "fp8")
        R.stage3_ref(x_plain, blocks, "fp8")                      # the range check holds without the row
        ref, bound = R.stage3_ref(x, blocks, "fp8", saturate=True, clamp_g=True)
        r = R.ratio(R.emulate(x, blocks, "fp8"), ref, bound)
        free = R.stage3_ref(x, blocks, "fp8", saturate=True)[0]
        moved = ((free - ref).abs() / bound)[row].max().item()
        print(f"fp8 C={C} saturation: worst err / bound {r:.3f}; the clamp moves the row's outputs by up to {moved:.1f} bounds")
        assert r <= 1.0 and moved > 1.0 and bool(torch.equal(free[:row], ref[:row])) and bool(torch.equal(free[row + 1:], ref[row + 1:]))


def applicable(fault):
    return R.FAULT_PRECS.get(fault, R.PRECS)


@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("fault", R.FAULTS)
def test_seeded_fault_leaves_the_bound(fault, C):
    """in every mode the fault applies to, on at least one case; the layout faults on a spotlight case"""
    layout = fault in ("no_swap23", "no_kperm", "swap_hidden", "planes_swapped")
    for prec in applicable(fault):
        seen = {}
        for name in CASES:
            if fault == "block1_twice" and name.endswith("depth 1"):
                continue
            x, blocks = case(C, name)
            ref, bound = reference(C, name, prec)
            seen[name] = R.ratio(R.stage3_ref(x, blocks, prec, fault=fault)[0], ref, bound)
        print(f"{fault:16s} {prec:6s} C={C}  " + "  ".join(f"{k}: {v:.3g}" for k, v in seen.items()))
        assert any(R.outside(v) for k, v in seen.items() if k.startswith("spotlight") or not layout), (fault, prec, seen)


def test_spotlight_maps():
    """every hidden unit in exactly one fc2 non-zero; a channel's four hidden units in four K slices and at four k
    positions of a fragment (16-bit k-step 16, fp8 64); every channel read by fc1, every hidden unit reading one or two"""
    for C in R.WIDTHS:
        H = 4 * C
        c1, c2, hid = R.spot_maps(C)
        assert sorted(hid.reshape(-1).tolist()) == list(range(H))
        assert all(len(set((row // (H // 8)).tolist())) == 4 for row in hid)
        assert all(len(set((row % 16).tolist())) == 4 and len(set((row % 64).tolist())) == 4 for row in hid)
        assert set(hid.reshape(-1).div(H // 8, rounding_mode="floor").tolist()) == set(range(8))
        assert set(c1.tolist()) == set(range(C)) and bool(((c2 == -1) | (c2 != c1)).all()) and bool((c2 >= 0).any())
        blocks = R.spot_blocks(C, 2, 13)
        for P in blocks:
            nz1, nz2 = (P["fc1_w"] != 0).sum(1), (P["fc2_w"] != 0).sum(1)
            assert bool(((nz1 == 1) | (nz1 == 2)).all()) and bool((nz2 == 4).all()) and bool(((P["fc2_w"] != 0).sum(0) == 1).all())
            for w in (P["fc1_w"], P["fc2_w"], P["fc2_w"] * P["gamma"][:, None]):     # exact in every operand type
                for prec in ("bf16", "f16", "fp8"):
                    assert torch.equal(w.to(R.ODT[prec]).float(), w), prec
            for row in P["fc2_w"]:                                                   # distinct within an output
                v = row[row != 0].abs().tolist()
                assert len(set(v)) == len(v)


@pytest.mark.parametrize("prec", R.PRECS)
def test_unpack_inverts_the_host_packer(prec):
    g = torch.Generator().manual_seed(3)
    for rows, K in ((64, 64), (96, 128), (2048, 512), (640, 2560)):
        for swap in (False, True):
            for kperm in ((False, True) if prec == "fp8" else (False,)):
                w = torch.randn(rows, K, generator=g)
                vals = R.host_round(prec, w, scale=8.0 if prec == "fp8" else None)
                img = R.pack_s3_host(vals, prec, swap, kperm)
                assert img.numel() == rows * K * R.ESZ[prec]
                back = R.unpack_s3(img, prec, rows, K, swap, kperm)
                for a, b in zip(back if prec == "f16x2" else (back,), vals if prec == "f16x2" else (vals,)):
                    assert torch.equal(R.bits(a), R.bits(b)), (rows, K, swap, kperm)
    # the layout comments, spot-checked by hand: 16-bit, tile 0, k-step 1, lane 37 (tile row 5, h 1), j 2 = source row 5
    # (swap23: 9), k 16 + 8 + 2; fp8 plain / kperm, k-step 0, lane 37, j 21: k = 32 + 21 / 32 + 5 + 8
    if prec in ("bf16", "f16"):
        pos = R.frag_pos(prec, 32, 64, False)
        assert int(pos[5, 26]) == (1 * 64 + 37) * 8 + 2 and int(R.frag_pos(prec, 32, 64, True)[9, 26]) == (1 * 64 + 37) * 8 + 2
    if prec == "fp8":
        at = 1 * 1024 + 37 * 16 + 5
        assert int(R.frag_pos(prec, 32, 64, False)[5, 32 + 21]) == at and int(R.frag_pos(prec, 32, 64, False, True)[5, 45]) == at
    if prec == "f16x2":
        assert int(R.frag_pos(prec, 32, 64, False)[5, 26]) == 1024 + 37 * 8 + 2


def test_fp8_scale_reference():
    for m, s in ((0.0, 1.0), (200.0, 1.0), (100.0, 2.0), (0.2, 1024.0), (241.0, 0.5), (1e-6 * 0.02, 2.0 ** 33)):
        assert R.fp8_scale(m) == s and (m == 0 or 120 < m * s <= 240)
    with pytest.raises(AssertionError):
        R.fp8_scale(1.875)
