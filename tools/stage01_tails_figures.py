"""Developer tool: the figures of tests/test_gpu_stage01_tails.py for the library in use (BTSBOT_AMD_LIB names another
build), as the PARENT table of that test; then the bits -- a hash of every tap, of the logits (12 alerts hinted and plain,
the 1- and 3-alert batches) per mode and of one training step's loss per 16-bit mode -- so that two builds can be
compared by diffing the output of two runs.  `--cpu` prints only the oracle's max|ref| per tap (no GPU)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import test_gpu_stage01_tails as T
from helpers import build_model, run_model


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def main():
    case = T.oracle_case()
    for t, r in case[5].items():
        print(f"oracle {t}: max|ref| {r.abs().max().item():.4f}")
    if "--cpu" in sys.argv:
        return
    dev = torch.device("cuda:0")
    kind, cfg, sd, img, meta = case[:5]
    print("PARENT = {")
    handles = {}
    for prec in T.MODES:
        m = handles[prec] = build_model(kind, cfg, sd, dev, prec)
        run_model(kind, m, img[:1].to(dev), meta[:1].to(dev))
        print(f'    "{prec}": {{')
        for what, e in T.tap_errors(case, m, dev).items():
            print(f'        "{what}": {e:.6e},')
        print("    },")
    print("}")
    handles["fp8"] = build_model(kind, cfg, sd, dev, "fp8")
    for prec, m in handles.items():
        for idx, tag in ((slice(None), "12"), (slice(0, 1), "1"), (slice(0, 3), "3")):
            for hint in (False, True):
                out, taps = T.forward(case, m, dev, idx, hint, taps=tuple(T.TAPS))
                print(f"bits {prec} alerts {tag} hint {int(hint)}: logits {digest(out)} " +
                      " ".join(f"{t} {digest(v)}" for t, v in taps.items()))
    # one training step per 16-bit mode: the keeping forms
    from btsbot_amd.train import Trainer
    labels = T.stress_inputs()[2]
    for prec in ("bf16", "f16"):
        m = build_model(kind, cfg, sd, dev, prec).train()
        tr = Trainer(m, lr=1e-4, betas=(0.99, 0.99), pos_weight=1.0, dropout_seed=1)
        torch.manual_seed(5)   # (a lone rank draws its dropout masks from the default generator)
        torch.cuda.manual_seed_all(5)
        loss = tr.step(img.to(dev), meta.to(dev), labels.to(dev))
        print(f"bits {prec} training step: loss {float(loss):.9e} {digest(loss.float())}")


if __name__ == "__main__":
    main()
