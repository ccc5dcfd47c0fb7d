"""CPU: the float64 reference of tests/test_gpu_maxvit_ops.py (part_ref: gather by partition rows, attention,
scatter back) against the oracle's own partition_attention, which partitions and reverses the map instead."""
import pytest
import torch

import test_gpu_maxvit_ops as MV
from oracle import maxvit_oracle as MO   # checker only


@pytest.mark.parametrize("grid", [0, 1], ids=["window", "grid"])
@pytest.mark.parametrize("C,H", [(64, 21), (128, 14), (256, 7)])
def test_part_reference_matches_the_oracle(C, H, grid):
    """The unrounded reference R of a whole partition block, in float64 on both sides.  The only difference is the
    GELU: R uses the kernels' gelu_poly<5> (f16), the oracle erf; the fit error, pinned at <= 1e-6 by
    test_gelu_polynomials_fit_the_erf_gelu, passes through fc2, whose rows hold 4C weights of variance 1 / 4C: held at
    1e-6 * (1 + sum |w|) per output."""
    B, dev = 2, torch.device("cpu")
    g = torch.Generator().manual_seed(C + H + grid)
    p = MV.part_params(C, "f16", g, dev)
    x = torch.randn(B * H * H, C, generator=g).double()
    R = MV.part_ref("f16", x, p, MV.part_rows(B, H, grid, dev), False, True)["x"]
    names = dict(ln1_w="norm1.weight", ln1_b="norm1.bias", qkv_w="attn.qkv.weight", qkv_b="attn.qkv.bias",
                 table="attn.rel_pos.relative_position_bias_table", proj_w="attn.proj.weight", proj_b="attn.proj.bias",
                 ln2_w="norm2.weight", ln2_b="norm2.bias", fc1_w="mlp.fc1.weight", fc1_b="mlp.fc1.bias",
                 fc2_w="mlp.fc2.weight", fc2_b="mlp.fc2.bias")
    sd = {"a." + names[k]: v.double() for k, v in p.items()}
    o = MO.partition_attention(x.view(B, H, H, C), sd, "a.", bool(grid), 32, 7).reshape(-1, C)
    tol = 1e-6 * (1.0 + p["fc2_w"].double().abs().sum(1))
    err = (o - R).abs()
    print(f"C={C} H={H} grid={grid}: max |R - oracle| = {err.max().item():.3e}")
    assert bool((err <= tol).all()), (err / tol).max().item()
    # and without the MLP the two agree to float64 rounding
    sd0 = dict(sd)
    sd0["a.mlp.fc2.weight"] = torch.zeros_like(sd["a.mlp.fc2.weight"])
    sd0["a.mlp.fc2.bias"] = torch.zeros_like(sd["a.mlp.fc2.bias"])
    o0 = MO.partition_attention(x.view(B, H, H, C), sd0, "a.", bool(grid), 32, 7).reshape(-1, C)
    R0 = MV.part_ref("f16", x, p, MV.part_rows(B, H, grid, dev), False, False)["x"]
    assert (o0 - R0).abs().max().item() <= 1e-12
