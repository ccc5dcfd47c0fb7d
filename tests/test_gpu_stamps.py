"""The developer timestamp buffer (btsbot_debug_stamps): every kernel that stamps writes inside the documented
32 + 16384 + 64 + 2048 entries, each into its own region (btsbot_amd/csrc/ctx.h: STAMP_*)."""
import ctypes as C

import pytest
import torch

from helpers import CONFIGS, MM_MAXVIT, seeded_state, seeded_state_mv, build_model, run_model
from btsbot_amd import _lib
from btsbot_amd.synthetic import synthetic_batch
from btsbot_amd.train import Trainer

pytestmark = pytest.mark.gpu

TOTAL = 32 + 16384 + 64 + 2048
GUARD = 4096


def test_debug_stamps_stay_inside_the_documented_buffer(cuda):
    buf = torch.zeros(TOTAL + GUARD, dtype=torch.int64, device=cuda)   # the buffer, then a guard tail

    def stamped(m, run):
        run()   # (the handle's first forward packs and reserves; stamp the second)
        buf[:TOTAL].zero_()
        _lib.check(_lib.lib().btsbot_debug_stamps(m._handle.ptr, C.c_void_p(buf.data_ptr())), "stamps")
        run()
        torch.cuda.synchronize()
        _lib.check(_lib.lib().btsbot_debug_stamps(m._handle.ptr, C.c_void_p(0)), "stamps")
        assert not buf[TOTAL:].any(), "a stamp landed behind the documented buffer"

    def written(lo, n, what):
        assert buf[lo:lo + n].any(), f"no stamps in {what} [{lo}, {lo + n})"

    B = 8
    img, meta, lab = [t.to(cuda) for t in synthetic_batch(B, seed=2)]
    kind, cfg = CONFIGS["mm_pico"]
    sd = seeded_state(kind, cfg, seed=3)
    m = build_model(kind, cfg, sd, cuda, "bf16")
    stamped(m, lambda: run_model(kind, m, img, meta))
    for lo, n, what in ((0, 16, "stage 0 phases"), (16, 16, "stage 1 phases"), (32, 2 * B, "stage 0 per workgroup"),
                        (32 + 8192, B, "stage 1 per workgroup"), (16416, 64, "stage 2 phases"),
                        (16480, 16, "stage 3 phases"), (17980, 16, "head16 phases")):
        written(lo, n, what)

    mt = build_model(kind, cfg, sd, cuda, "bf16").train()
    tr = Trainer(mt, lr=1e-4)
    stamped(mt, lambda: tr.step(img, meta, lab))
    written(16416, 64, "stage 2 phases (keeping form)")

    mv = build_model("mm_MaxViT", MM_MAXVIT, seeded_state_mv("mm_MaxViT", MM_MAXVIT, seed=3), cuda, "bf16")
    stamped(mv, lambda: run_model("mm_MaxViT", mv, img[:4], meta[:4]))
    written(32, 32, "MaxViT partition kernel, C = 256")
    written(64, 32, "MaxViT partition kernel, C = 128")
