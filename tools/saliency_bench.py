#!/usr/bin/env python
"""Time the input gradients (model.input_gradients: btsbot_forward_keep_eval + btsbot_backward_inputs) on one GPU:

    python tools/saliency_bench.py [B] [precision]      # default 1024 f32; precision f32, bf16, f16 or f16x2

A seeded mm_ConvNeXt (pico) in eval mode on a synthetic batch.  HIP events after a warm-up call, seven blocks, the MEDIAN
block.  Prints one JSON line:
  input_gradients_ms     model.input_gradients(image, metadata) end to end: the keeping forward, the whole backward (parameter
                         gradients included: they are not skipped) and the two input-gradient launches
  keep_backward_ms       the eval-form keeping forward + btsbot_backward (every parameter gradient, no input gradients) on the
                         same handle in the same run: what the call above is built on
  stem_dgrad_ms          stem_dgrad_kernel alone on a random dxn [B*225][C0]
  torch_stem_dgrad_ms    the same product as torch ops on the same dxn: matmul with the [C0][48] filter, permute to image
                         rows, pad to 63
  stem_dgrad_gbs         bytes stem_dgrad must move at least (dxn read, the image written) per second
  torch_vs_kernel        the largest difference of the two results relative to the largest entry
"""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
from btsbot_amd import ops   # noqa: E402
from btsbot_amd.synthetic import synthetic_batch   # noqa: E402
from radius_bench import timed   # noqa: E402
from trigger_example import seeded_model   # noqa: E402


def torch_stem_dgrad(dxn, w):
    B, c0 = dxn.shape[0] // 225, w.shape[0]
    t = (dxn @ w.view(c0, 48)).view(B, 15, 15, 3, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 60, 60)
    return F.pad(t, (0, 3, 0, 3))


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    prec = sys.argv[2] if len(sys.argv) > 2 else "f32"
    if not torch.cuda.is_available():
        sys.exit("saliency_bench: needs a GPU")
    dev = torch.device("cuda:0")
    model = seeded_model(prec).to(dev).eval()
    img, meta, _ = synthetic_batch(B, seed=5)
    img, meta = img.to(dev), meta.to(dev)
    res = {"B": B, "precision": prec}

    res["input_gradients_ms"] = timed(lambda: model.input_gradients(image_input=img, metadata_input=meta, batch_size=B))
    seed = torch.ones(B, 1, device=dev)

    def keep_backward():
        with torch.no_grad():
            model._forward_keep_eval_raw(img, meta, keep_image=True)
            model._backward_raw(seed, True, True)
    res["keep_backward_ms"] = timed(keep_backward)
    res["input_gradient_launches_ms"] = res["input_gradients_ms"] - res["keep_backward_ms"]

    c0 = 64
    gen = torch.Generator(device=dev).manual_seed(1)
    dxn = torch.randn((B * 225, c0), generator=gen, device=dev)
    w = torch.randn((c0, 3, 4, 4), generator=gen, device=dev)
    out = torch.empty((B, 3, 63, 63), device=dev)
    res["stem_dgrad_ms"] = timed(lambda: ops.cnt_stem_dgrad(dxn, w, out))
    res["torch_stem_dgrad_ms"] = timed(lambda: torch_stem_dgrad(dxn, w))
    res["torch_over_kernel"] = res["torch_stem_dgrad_ms"] / res["stem_dgrad_ms"]
    res["stem_dgrad_gbs"] = (dxn.numel() + out.numel()) * 4 / res["stem_dgrad_ms"] / 1e6
    ref = torch_stem_dgrad(dxn, w)
    res["torch_vs_kernel"] = float((ops.cnt_stem_dgrad(dxn, w, out) - ref).abs().max() / ref.abs().max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
