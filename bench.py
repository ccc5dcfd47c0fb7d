#!/usr/bin/env python3
"""Headline benchmark: alerts/sec of the BTSbot classifier hot path on MI355X.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``; for N > 1 launched as
``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...`` (one rank per GPU).
Rank 0 prints ONE JSON line.  Such a plain run sets up, runs W warm-up steps and ~0.5 s more of the same workload,
times exactly K steps once (`ms_per_step` = that time / K), writes the last step's logits with ``--dump-outputs DIR``
and prints the line.  Everything else below (the drop-in figures, roofline, other precisions and sizes, parity, the
training and MaxViT legs, the CPU baseline) runs only with ``--full``, which prints the long line first.

Workload = BASELINE.json configs[1]: ConvNeXt-pico multi-modal (mm_ConvNeXt) bf16 inference on a
batch of 1024 synthetic alerts per GPU (63x63x3 triplet + 25 metadata scalars each), inputs
resident in HBM before the timed region.  One "step" = one forward of that batch through
``model(image_input=..., metadata_input=...)`` -> logits (the C ABI also writes the sigmoid
scores).  Alerts are independent, so N GPUs run N replicas on N different shards with no data-path
collective: scaling is "weak", value = N * 1024 * K / max-over-ranks time.

Extra objects on the line:
  roofline      the pointwise-conv MFMA kernel family with the largest device time (the fused
                fc1->GELU->fc2 kernel of stages 0-1, or the fc1 / fc2 GEMMs of stages 2-3):
                algorithmic FLOP per launch / mean launch time measured with HIP events on the
                launch stream (a second, event-bracketed pass over the same K steps), against the
                2.5 PFLOP/s dense bf16 MFMA peak.  `kernels` lists every kernel family the same way.
  cpu_baseline  the CPU oracle (same ATen CPU ops the reference dispatches to) timed on this host,
                rank 0 at N=1 only, on a bounded sample.
"""
import argparse
import json
import os
import sys
import time
import warnings


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f16", "f32", "fp8", "f16x2"])
    ap.add_argument("--batch", type=int, default=1024, help="alerts per GPU per step")
    ap.add_argument("--pipeline-depth", type=int, default=3,
                    help="batches in flight on alternating HIP streams in the timed loop (btsbot_amd.ScoreStream); "
                         "1 = plain model(...) calls on one stream")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline (drop-in calls, roofline, parity, other precisions "
                         "and sizes, training and MaxViT legs, CPU baseline); the options below apply to --full runs")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the logits of the last timed step as DIR/logits.npy (float32; "
                         "rank r > 0: logits_rank<r>.npy)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra-legs", action="store_true",
                    help="skip the f16 / f32 precision legs and the parity object (profiling runs)")
    ap.add_argument("--train-steps", type=int, default=20,
                    help="steps of the training leg (BASELINE.json configs[2]); 0 = skip")
    ap.add_argument("--train-batch", type=int, default=1024, help="alerts per GPU per training step")
    ap.add_argument("--maxvit-steps", type=int, default=3,
                    help="steps of the MaxViT inference leg (BASELINE.json configs[3]); 0 = skip")
    ap.add_argument("--maxvit-batch", type=int, default=1024, help="alerts per GPU per MaxViT step")
    ap.add_argument("--maxvit-train-steps", type=int, default=3,
                    help="steps of the MaxViT training leg (mm_MaxViT, every parameter trainable); 0 = skip")
    ap.add_argument("--maxvit-train-batch", type=int, default=64, help="alerts per GPU per MaxViT training step")
    return ap.parse_args()


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves (what
    `python -m torch.distributed.run --nproc-per-node N` would do), one process per GPU, and exit with the
    worst child's code.  Runs before torch or the package is imported: nothing in THIS process has touched
    the GPU, the children are ordinary child processes (no exec of a GPU-initialised process)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    return max(p.wait() for p in procs)


if __name__ == "__main__" and "WORLD_SIZE" not in os.environ:
    _n = parse_args().gpus
    if _n > 1:
        sys.exit(spawn_ranks(_n))

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import btsbot_amd  # noqa: E402
from btsbot_amd.synthetic import METADATA_COLS, synthetic_batch  # noqa: E402

METRIC = "alerts/sec (63×63×3 triplet + 25 meta) train+infer, 1/2/4/8 MI355X"
PER_GPU_BATCH = 1024
# (fp8 mode: most FLOPs still bf16; f16x2: ALGORITHMIC flop against the f16 peak -- the mode issues two to three
#  MFMAs per algorithmic product, so its fraction of peak counts useful work only)
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "f16": 2500.0, "f32": 157.3, "fp8": 2500.0, "f16x2": 2500.0}
FP8_KERNEL_PEAK_TFLOPS = 5000.0   # MI355X_MICROARCH.md, Matrix cores: block-scaled f8f6f4 with e4m3 operands = 2 x bf16 per clock
FP8_KERNELS = ("stage2p_kernel", "s3_fc1_kernel", "s3_fc2_kernel")
HBM_PEAK_GBS = 8000.0
STAGE_P = (225, 49, 9, 1)

CONFIG = dict(model_name="mm_ConvNeXt", model_kind="convnext_pico.d1_in1k", pretrained=False,
              train_data_version="v11", metadata_cols=METADATA_COLS, meta_fc1_neurons=128,
              meta_dropout=0.25, meta_fc2_neurons=128, comb_fc1_neurons=128, comb_fc2_neurons=32,
              comb_dropout=0.2)


def seeded_weights(model, seed=3, layer_scale=1.0):
    """Random weights written straight into the model (there are no checkpoints offline).  layer_scale ~1 (the
    benchmarked stress case: every block contributes fully, the worst case for a 16-bit operand) or ~0.1 (what a trained
    ConvNeXt's gamma looks like): the same draws, only the `gamma` tensors scaled."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if not v.is_floating_point():
                continue
            if k.endswith("running_var"):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            elif k.endswith("running_mean"):
                v.copy_(torch.randn(v.shape, generator=g) * 0.5)
            elif k.endswith("gamma"):
                v.copy_(layer_scale * (1.0 + 0.1 * torch.randn(v.shape, generator=g)))
            elif v.dim() == 1 and k.endswith("weight"):
                v.copy_(1.0 + 0.1 * torch.randn(v.shape, generator=g))
            elif v.dim() == 1:
                v.copy_(0.05 * torch.randn(v.shape, generator=g))
            else:
                fan_in = v[0].numel()
                v.copy_(torch.randn(v.shape, generator=g) / fan_in ** 0.5)
    model.mark_weights_dirty()


def family_work(batch, precision, depths=(2, 2, 6, 2), dims=(64, 128, 256, 512)):
    """Algorithmic FLOP and compulsory HBM bytes per forward of `batch` alerts, per kernel family
    (DESIGN.md 'Kernels').  In the 16-bit modes the blocks of the stages with
    C in {64,128} run the fused MLP kernel, the others the fc1 / fc2 GEMM pair."""
    esz = 4 if precision in ("f32", "f16x2") else 2
    st = list(zip(depths, STAGE_P, dims))
    s0 = precision != "f32" and dims[0] == 64 and depths[0] == 2      # stage-0 megakernel
    s1 = precision != "f32" and dims[1] == 128 and dims[2] == 256 and depths[1] == 2   # stage-1
    mega = [s0, s1, False, False]
    fused = [precision != "f32" and c in (64, 128) and not mega[i]
             for i, (_, _, c) in enumerate(st)]
    pw = lambda d, p, c: d * 2 * batch * p * c * 4 * c          # one of the two 1x1 convs
    w = {}
    stem_flop = 2 * batch * 225 * 48 * dims[0]
    down_flop = lambda i: 2 * batch * STAGE_P[i] * 4 * dims[i - 1] * dims[i]
    # MFMA-executed algorithmic FLOP only (stem, 2 x (fc1 + fc2), downsample); the depthwise conv
    # (2 x 2*49*225*64 FLOP per alert, VALU) is not counted against the MFMA roofline
    w["stage0b_kernel"] = dict(
        flop=(stem_flop + 2 * pw(*st[0]) + down_flop(1)) if s0 else 0,
        bytes=batch * (3 * 63 * 63 * 4 + 49 * dims[1] * 4))
    w["stage1b_kernel"] = dict(
        flop=(2 * pw(*st[1]) + down_flop(2)) if s1 else 0,
        bytes=batch * (49 * dims[1] * 4 + 9 * dims[2] * 4))
    w["fused_mlp_kernel"] = dict(
        flop=sum(2 * pw(d, p, c) for (d, p, c), f in zip(st, fused) if f),
        bytes=sum(d * (batch * p * c * (esz + 8) + 8 * c * c * esz)
                  for (d, p, c), f in zip(st, fused) if f))
    unf = [not f and not mega[i] for i, f in enumerate(fused)]
    # stage 2 at C = 256 with stage 3 at 512: the whole stage and the last downsample in one persistent launch
    s2p = precision != "f32" and dims[2] == 256 and dims[3] == 512 and depths[2] <= 8 and \
        os.environ.get("BTSBOT_AMD_NO_STAGE2", "0") != "1"
    w["stage2p_kernel"] = dict(
        flop=(2 * pw(*st[2]) + down_flop(3)) if s2p else 0,
        bytes=batch * (9 * dims[2] * 4 + dims[3] * 4) + depths[2] * 8 * dims[2] ** 2 * esz + 4 * dims[2] * dims[3] * esz)
    mega[2] = s2p
    s2 = False
    # stage 3 (1x1 maps) at C in {512, 640}: two fragment-streaming launches per block (stage3.hip)
    s3 = precision != "f32" and dims[3] in (512, 640) and os.environ.get("BTSBOT_AMD_NO_S3", "0") != "1"
    w["s3_fc1_kernel"] = dict(
        flop=pw(*st[3]) if s3 else 0,
        bytes=st[3][0] * (batch * dims[3] * 4 + batch * 4 * dims[3] * esz + 4 * dims[3] ** 2 * esz))
    w["s3_fc2_kernel"] = dict(
        flop=pw(*st[3]) if s3 else 0,
        bytes=st[3][0] * (batch * 4 * dims[3] * esz + 2 * batch * dims[3] * 4 + 4 * dims[3] ** 2 * esz))
    mega[3] = s3
    unf = [u and not mega[i] for i, u in enumerate(unf)]
    unf1 = [u and not (s2 and i == 2) for i, u in enumerate(unf)]
    w["gemm_kernel<fc1,GELU>"] = dict(
        flop=sum(pw(d, p, c) for (d, p, c), u in zip(st, unf1) if u),
        bytes=sum(d * (batch * p * c * esz + batch * p * 4 * c * esz + 4 * c * c * esz)
                  for (d, p, c), u in zip(st, unf1) if u))
    w["gemm_kernel<fc2,RESID>"] = dict(
        flop=sum(pw(d, p, c) for (d, p, c), u in zip(st, unf) if u),
        bytes=sum(d * (batch * p * 4 * c * esz + 2 * batch * p * c * 4 + 4 * c * c * esz)
                  for (d, p, c), u in zip(st, unf) if u))
    dwst = [(d, p, c) for i, (d, p, c) in enumerate(st) if not mega[i] and not (s2 and i == 2)]
    w["dwconv_ln_kernel"] = dict(
        flop=sum(d * 2 * 49 * batch * p * c for d, p, c in dwst),
        bytes=sum(d * batch * p * c * (4 + esz) for d, p, c in dwst))
    dn = [i for i in (1, 2, 3) if not mega[i - 1]]
    w["gemm_kernel<down,BIAS>"] = dict(
        flop=sum(down_flop(i) for i in dn),
        bytes=sum(batch * STAGE_P[i] * (4 * dims[i - 1] * esz + dims[i] * 4) for i in dn))
    w["ln_patch_kernel"] = dict(
        flop=0, bytes=sum(batch * STAGE_P[i] * 4 * dims[i - 1] * (4 + esz) for i in dn))
    w["stem_kernel"] = dict(flop=stem_flop,
                            bytes=batch * (3 * 63 * 63 * 4 + 225 * dims[0] * 4))
    w["head_kernel"] = dict(flop=2 * batch * (25 * 128 + 128 * 128 + 640 * 128 + 128 * 32 + 32),
                            bytes=batch * (dims[3] * 4 + 25 * 4 + 8))
    w["head16_kernel"] = dict(w["head_kernel"])   # the same head on the matrix pipe (16-bit modes)
    return w


POINTWISE = ("stage0b_kernel", "stage1b_kernel", "stage2p_kernel", "s3_fc1_kernel", "s3_fc2_kernel", "fused_mlp_kernel",
             "gemm_kernel<fc1,GELU>",
             "gemm_kernel<fc2,RESID>")


MAXVIT_CONFIG = dict(CONFIG, model_name="mm_MaxViT", model_kind="maxvit_tiny_rw_224.sw_in1k")


def maxvit_blocks():
    """[(cin, c, mid, stride, hin, hout)] of maxvit_tiny_rw_224 (oracle/maxvit_oracle.block_table)."""
    rows, cin, hw = [], 64, 112
    for d, c in zip((2, 2, 5, 2), (64, 128, 256, 512)):
        for j in range(d):
            s = 2 if j == 0 else 1
            rows.append((cin, c, 4 * cin, s, hw, hw // s))
            cin, hw = c, hw // s
    return rows


def maxvit_family_work(batch, precision):
    """Algorithmic FLOP / compulsory HBM bytes per forward of `batch` alerts, per MaxViT kernel family."""
    esz = 4 if precision in ("f32", "f16x2") else 2
    w = {k: dict(flop=0, bytes=0) for k in (
        "mv_stem_im2col", "mv_gemm<stem>", "mv_gemm<conv1,SILU>", "mv_gemm<conv3,gated>",
        "mv_gemm<shortcut>", "mv_gemm<qkv>", "mv_gemm<proj,RESID>", "mv_gemm<fc1,GELU>",
        "mv_gemm<fc2,RESID>", "mv_fused_mlp", "mv_streamed_mlp", "mv_partition", "mv_mbconv_front", "mv_attn_block", "mv_elementwise", "mv_dw3_kernel",
        "mv_se_kernel", "mv_ln_kernel", "mv_attn_kernel", "head_kernel")}

    def add(k, macs, nbytes):
        w[k]["flop"] += 2 * macs * batch
        w[k]["bytes"] += nbytes * batch

    if precision == "f32":      # im2col + GEMM for both stem convolutions
        add("mv_gemm<stem>", 12544 * (27 * 32 + 288 * 64), 12544 * (32 * esz * 2 + 288 * esz + 64 * 4))
        add("mv_stem_im2col", 0, 3 * 63 * 63 * 4 + 12544 * 32 * esz + 12544 * 32 * esz + 12544 * 288 * esz)
    else:                       # direct conv1 (VALU) and implicit-GEMM conv2 (+ block 0's pre-norm output)
        add("mv_stem_im2col", 12544 * 27 * 32, 3 * 63 * 63 * 4 + 12544 * 32 * esz)
        add("mv_gemm<stem>", 12544 * 288 * 64, 12544 * (32 * esz + 64 * 4 + 64 * esz))
    prev_c = None
    for bi, (cin, c, mid, s, hi, ho) in enumerate(maxvit_blocks()):
        pi, po = hi * hi, ho * ho
        # 16-bit modes: block 0's pre-norm and pooled shortcut come out of the stem kernel, and a block that
        # follows a C = 64 / 128 block gets its pre-norm from that block's last fused MLP
        # (or, with the partition blocks as one kernel, from that kernel's post-op: every block but the first)
        part_on = precision in ("bf16", "f16") and os.environ.get("BTSBOT_AMD_MV_NO_PART", "0") != "1"
        part_full = part_on
        part_prev = part_full and prev_c in (64, 128, 256)
        pre_fused = precision != "f32" and (bi == 0 or prev_c in (64, 128) or part_prev)
        pool_fused = precision != "f32" and bi == 0
        add("mv_elementwise", 0, (0 if pre_fused else pi * cin * (4 + esz)) +
            (po * cin * (4 + esz) if s == 2 and not pool_fused else 0))
        prev_c = c
        if precision != "f32" and cin in (64, 128) and ho >= 28 and \
                os.environ.get("BTSBOT_AMD_MV_NO_FRONT", "0") != "1":
            add("mv_mbconv_front", pi * cin * mid + po * 9 * mid, (pi * cin + po * mid) * esz)
        else:
            add("mv_gemm<conv1,SILU>", pi * cin * mid, pi * (cin + mid) * esz)
            add("mv_dw3_kernel", po * 9 * mid, (pi + po) * mid * esz)
        add("mv_se_kernel", 2 * mid * (mid // 16), po * mid * esz)
        add("mv_gemm<conv3,gated>", po * mid * c, po * (mid * esz + 8 * c))
        if s == 2 and cin != c:
            add("mv_gemm<shortcut>", po * cin * c, po * (cin * esz + 4 * c))
        part = part_on and c in (64, 128, 256)   # maxvit_part.hip: a partition block (attention half + MLP half) per launch
        ln_fused = precision != "f32" and c in (64, 128) and not part and \
            os.environ.get("BTSBOT_AMD_MV_NO_LN_FUSE", "0") != "1"
        # C = 256: norm2 + fc1 + GELU + fc2 + residual as one launch of stage2p_kernel's row-tile form (its own LayerNorm)
        smlp = precision != "f32" and c == 256 and os.environ.get("BTSBOT_AMD_MV_NO_SMLP", "0") != "1"
        for g in range(2):
            if part and part_full:
                # rows read once and written once (+ the next block's pre-norm copy behind the grid half)
                post = po * c * esz if g == 1 and bi + 1 < len(maxvit_blocks()) else 0
                add("mv_partition", po * (4 * c * c + 49 * c * 2 + 8 * c * c), po * c * 8 + post)
                continue
            # C = 64 / 128: every LayerNorm rides on the epilogue of the kernel that produces its input
            add("mv_ln_kernel", 0, (0 if ln_fused else (0 if smlp else 1) if part else 1 if smlp else 2) * po * c * (4 + esz))
            if part:
                add("mv_partition", po * (4 * c * c + 49 * c * 2), po * c * 8)
            elif precision != "f32" and c == 64 and os.environ.get("BTSBOT_AMD_MV_NO_ATTN_BLOCK", "0") != "1":
                add("mv_attn_block", po * (4 * c * c + 49 * c * 2), po * c * (2 * esz + 8))
            else:
                add("mv_gemm<qkv>", po * c * 3 * c, po * 4 * c * esz)
                add("mv_attn_kernel", po * 49 * c * 2, po * 4 * c * esz)
                add("mv_gemm<proj,RESID>", po * c * c, po * c * (esz + 8))
            if precision != "f32" and c in (64, 128) and \
                    os.environ.get("BTSBOT_AMD_MV_MLP_UNFUSED", "0") != "1":
                add("mv_fused_mlp", po * 8 * c * c, po * c * (esz + 8))
            elif smlp:
                add("mv_streamed_mlp", po * 8 * c * c, po * c * 8)
            else:
                add("mv_gemm<fc1,GELU>", po * 4 * c * c, po * 5 * c * esz)
                add("mv_gemm<fc2,RESID>", po * 4 * c * c, po * c * (4 * esz + 8))
    add("mv_ln_kernel", 0, 49 * 512 * 4)
    add("head_kernel", 25 * 128 + 128 * 128 + 640 * 128 + 128 * 32 + 32, 512 * 4 + 108)
    return w


def maxvit_leg(dev, rank, world, dist, fence, args):
    """BASELINE.json configs[3]: mm_MaxViT (maxvit_tiny_rw_224 on cutouts resized to 224) inference."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mv = btsbot_amd.mm_MaxViT(MAXVIT_CONFIG, precision=args.precision)
    seeded_weights(mv)
    mv = mv.to(dev).eval()
    img, meta, _ = synthetic_batch(args.maxvit_batch, seed=50 + rank)
    img, meta = img.to(dev), meta.to(dev)

    def step():
        with torch.no_grad():
            return mv(image_input=img, metadata_input=meta)

    def run(n):
        o = None
        for _ in range(n):
            o = step()
        return o

    el, _, out = timed_blocks(run, args.maxvit_steps, 1, fence, dist, dev, blocks=3, warm_seconds=0.3)
    mv.set_profile(True)
    step()
    prof = mv.collect_profile()
    mv.set_profile(False)
    work = maxvit_family_work(args.maxvit_batch, args.precision)
    kernels = {}
    for name, (ms, n) in prof.items():
        if n == 0 or name not in work:
            continue
        kernels[name] = dict(launches_per_step=n, ms_per_step=round(ms, 4),
                             tflops=round(work[name]["flop"] / (ms * 1e-3) / 1e12, 2),
                             gbs=round(work[name]["bytes"] / (ms * 1e-3) / 1e9, 1))
    flop_alert = sum(v["flop"] for v in work.values()) / args.maxvit_batch
    total = args.maxvit_batch * world * args.maxvit_steps
    return {
        "workload": "BASELINE.json configs[3]: mm_MaxViT (maxvit_tiny_rw_224, 63x63 cutouts resized to "
                    f"224x224 on device) {args.precision} inference, batch={args.maxvit_batch} per GPU",
        "value": round(total / el, 1), "unit": "alerts/s", "per_gpu_batch": args.maxvit_batch,
        "steps": args.maxvit_steps, "ms_per_step": round(1e3 * el / args.maxvit_steps, 3),
        "flop_per_alert": int(flop_alert),
        "whole_net_tflops": round(flop_alert * total / el / 1e12, 2),
        "finite": bool(torch.isfinite(out).all().item()), "kernels": kernels,
    }


WARM_SECONDS = 0.5     # every timed region is preceded by at least this much of its own workload (clocks, caches)
BLOCKS = 7             # the K-step block is timed this many times; the MEDIAN block is reported
FULL_LEG_STEPS = 1000  # --full: a secondary leg times blocks of at most this many steps, whatever --steps the headline has


def timed_blocks(run, steps, warmup, fence, dist, dev, blocks=BLOCKS, warm_seconds=WARM_SECONDS):
    """`warmup` untimed steps, then >= warm_seconds of the workload (a cold GPU clocks up over the first hundreds of
    milliseconds: a 7 ms timed region right behind 5 warm-up steps measured 8-14 % low), then `blocks` timed blocks of
    exactly `steps` steps, each bracketed by barrier + synchronize on both sides and reduced with MAX over the ranks.
    Returns (median block seconds, sorted list of block seconds, last output)."""
    last = None
    if warmup > 0:
        last = run(warmup)
    fence()
    t_end = time.perf_counter() + warm_seconds
    while True:
        go = time.perf_counter() < t_end
        if dist is not None:   # every rank must run the same number of blocks: `run` may contain collectives
            g = torch.tensor([1.0 if go else 0.0], device=dev)
            dist.all_reduce(g, op=dist.ReduceOp.MIN)
            go = g.item() > 0.5
        if not go:
            break
        last = run(steps)
        torch.cuda.synchronize(dev)
    times = []
    for _ in range(blocks):
        fence()
        t0 = time.perf_counter()
        last = run(steps)
        fence()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = t.item()
        times.append(el)
    times.sort()
    return times[len(times) // 2], times, last


def timed_steps(run, steps, warmup, fence, dist, dev, warm_seconds=WARM_SECONDS):
    """The headline's timing: `warmup` untimed steps, then >= warm_seconds of the workload in chunks of at most
    max(warmup, 1) steps (never a whole `steps` block: the time outside the timed steps stays small whatever `steps`
    is), then ONE timed region of exactly `steps` steps, bracketed by barrier + synchronize on both sides and reduced
    with MAX over the ranks.  Returns (seconds, last output)."""
    last = None
    if warmup > 0:
        last = run(warmup)
    fence()
    chunk = max(1, min(steps, warmup))
    t_end = time.perf_counter() + warm_seconds
    while True:
        go = time.perf_counter() < t_end
        if dist is not None:   # every rank must run the same number of chunks: `run` may contain collectives
            g = torch.tensor([1.0 if go else 0.0], device=dev)
            dist.all_reduce(g, op=dist.ReduceOp.MIN)
            go = g.item() > 0.5
        if not go:
            break
        last = run(chunk)
        torch.cuda.synchronize(dev)
    fence()
    t0 = time.perf_counter()
    last = run(steps)
    fence()
    el = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([el], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = t.item()
    return el, last


def dump_outputs(out_dir, rank, **arrays):
    """--dump-outputs: the tensors the timed path handed its caller in its last step, as float32 .npy files."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    suffix = "" if rank == 0 else f"_rank{rank}"
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), t.detach().float().cpu().numpy())


def headline_line(args, world, elapsed, depth):
    """The contract's fields, the same in a plain and in a --full run."""
    total_alerts = args.batch * world * args.steps
    return {
        "metric": METRIC,
        "value": round(total_alerts / elapsed, 1),
        "unit": "alerts/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.precision,
        "data": "synthetic",
        "config": {
            "workload": "BASELINE.json configs[1]: ConvNeXt-pico multi-modal (mm_ConvNeXt) "
                        f"{args.precision} inference, batch={args.batch} synthetic triplets per GPU, "
                        "inputs resident in HBM, logits+scores out",
            "per_gpu_batch": args.batch, "global_batch": args.batch * world,
            "precision": args.precision, "weights": "seeded random, layer-scale ~1",
            "parallelism": f"{world} independent replicas, batch-sharded, no collective",
            "pipeline_depth": depth,
            "api": ("btsbot_amd.ScoreStream (the library's scoring loop: consecutive batches on alternating HIP "
                    "streams)" if depth > 1 else "drop-in model(image_input=, metadata_input=) calls"),
        },
        "timing": {"blocks": 1, "steps_per_block": args.steps, "reported": "one timed block of --steps steps",
                   "gpu_warm_seconds_before_timing": WARM_SECONDS},
    }


def maxvit_train_leg(dev, rank, world, dist, fence, args):
    """Training of the whole mm_MaxViT (image branch included: BatchNorm2d batch statistics, backward of every layer --
    btsbot_amd/csrc/maxvit_train.hip: the 1x1 convolutions / Linear layers on the 16-bit MFMA GEMMs in the 16-bit modes,
    everything else fp32) with BCE + AdamW and, with more than
    one rank, the gradient exchange.  The reference's fine-tuning of a MaxViT model, train.py:218-236, 510-527."""
    from btsbot_amd.train import Trainer
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mv = btsbot_amd.mm_MaxViT(MAXVIT_CONFIG, precision=args.precision)
    seeded_weights(mv)
    mv = mv.to(dev).train()
    img, meta, lab = synthetic_batch(args.maxvit_train_batch, seed=70 + rank)
    img, meta, lab = img.to(dev), meta.to(dev), lab.to(dev)
    tr = Trainer(mv, lr=1e-4, betas=(0.99, 0.99), pos_weight=1.0)

    def run(n):
        o = None
        for _ in range(n):
            o = tr.step(img, meta, lab)
        return o

    el, _, loss = timed_blocks(run, args.maxvit_train_steps, 1, fence, dist, dev, blocks=3, warm_seconds=0.2)
    total = args.maxvit_train_batch * world * args.maxvit_train_steps
    # forward + input gradients + filter gradients = 3 x the forward's 10.1 GFLOP per alert
    step_flop = 3.0 * 10.14e9 * args.maxvit_train_batch
    return {
        "workload": "mm_MaxViT (maxvit_tiny_rw_224 on cutouts resized to 224) training step, every parameter trainable: "
                    "BatchNorm2d batch statistics, BCE, backward of every layer, AdamW; GEMM operands in the mode's type, the rest fp32, "
                    f"batch={args.maxvit_train_batch} per GPU",
        "value": round(total / el, 1), "unit": "alerts/s", "per_gpu_batch": args.maxvit_train_batch,
        "steps": args.maxvit_train_steps, "ms_per_step": round(1e3 * el / args.maxvit_train_steps, 2),
        "loss_finite": bool(torch.isfinite(loss).item()),
        "whole_step_tflops": round(step_flop / (el / args.maxvit_train_steps) / 1e12, 2),
        "note": "an fp32 per-layer engine: one launch per layer, every intermediate through HBM (~2,100 launches of 10-20 us per "
                "64-alert step: the GEMMs are ~20 % of it, operand casts 10 %, the attention backward 10 %); the training "
                "benchmark of BASELINE.json (configs[2]) is the ConvNeXt `train` leg",
    }


def cpu_baseline(sample_batch=256, budget_s=24.0):
    """CPU oracle (kind 'port'): fp32, eval, no_grad.  The thread count is swept over
    {8, 16, 32, 64} (capped at the cores this process may use) and the BEST is reported with its thread count: on
    these small maps more intra-op threads than ~16 only add synchronisation cost (64 threads gave 824 alerts/s where
    8 give ~1,570 on the survey's box)."""
    from oracle import convnext_oracle as O   # CPU baseline leg only
    try:
        ncores = len(os.sched_getaffinity(0))
    except AttributeError:
        ncores = os.cpu_count() or 1
    sd = O.random_state_dict(O.model_param_shapes("mm_ConvNeXt", CONFIG), seed=3)
    img, meta, _ = synthetic_batch(sample_batch, seed=2)
    counts = sorted({min(n, ncores) for n in (8, 16, 32, 64)})
    sweep, best, total_s, total_n = {}, None, 0.0, 0
    for nt in counts:
        torch.set_num_threads(max(1, nt))
        with torch.no_grad():
            O.forward("mm_ConvNeXt", sd, CONFIG, img, meta)
            times = []
            t_end = time.perf_counter() + budget_s / len(counts)
            while len(times) < 3 or (time.perf_counter() < t_end and len(times) < 30):
                t0 = time.perf_counter()
                O.forward("mm_ConvNeXt", sd, CONFIG, img, meta)
                times.append(time.perf_counter() - t0)
        times.sort()
        med = times[len(times) // 2]
        total_s += sum(times)
        total_n += len(times)
        sweep[str(nt)] = round(sample_batch / med, 1)
        if best is None or sample_batch / med > best[0]:
            best = (sample_batch / med, nt)
    return dict(value=round(best[0], 1), unit="alerts/s", cores=best[1], kind="port",
                host_cores_available=ncores, thread_sweep=sweep,
                sample=f"{total_n} forwards of {sample_batch} synthetic alerts (same model/weights, fp32 torch-CPU "
                       f"oracle, median per thread count, best of {counts} threads), ~{total_s:.0f}s of CPU work")


def parity_vs_oracle(model, img, meta, n=256, cfg=None):
    """max |dlogit| / |dscore| of THIS model (the benchmarked weights and precision) on the first n alerts of the
    benchmarked batch against the fp32 CPU oracle (checker only; outside every timed region)."""
    from oracle import convnext_oracle as O   # checker only
    n = min(n, img.shape[0])
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        ref = O.forward("mm_ConvNeXt", sd, cfg or CONFIG, img[:n].cpu(), meta[:n].cpu())
        out = model(image_input=img[:n].contiguous(), metadata_input=meta[:n].contiguous()).cpu()
    return dict(alerts=n, max_abs_dlogit=float((out - ref).abs().max()),
                max_abs_dscore=float((torch.sigmoid(out) - torch.sigmoid(ref)).abs().max()),
                oracle="oracle/convnext_oracle.py, fp32 CPU, same weights")


def trained_like_parity(precision, dev, img, meta, layer_scale=0.1):
    """Parity of one operand mode with trained-like layer scale (gamma ~ 0.1 instead of the benchmark's ~1): what a
    user of a trained checkpoint sees.  No timing: the kernels do not depend on the values."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = btsbot_amd.mm_ConvNeXt(CONFIG, precision=precision)
    seeded_weights(m, layer_scale=layer_scale)
    m = m.to(dev).eval()
    out = parity_vs_oracle(m, img, meta)
    out["weights"] = f"seeded random, layer-scale ~{layer_scale}"
    return out


def precision_leg(precision, dev, img, meta, steps, warmup, fence, dist, world, with_parity=True):
    """The same workload in another MFMA operand mode (f16: same matrix rate as bf16, scores within 1e-4 of the
    oracle; f32: the exact-fp32 parity mode), with its own parity figures."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = btsbot_amd.mm_ConvNeXt(CONFIG, precision=precision)
    seeded_weights(m)
    m = m.to(dev).eval()

    def step():
        with torch.no_grad():
            return m(image_input=img, metadata_input=meta)

    def run(n):
        o = None
        for _ in range(n):
            o = step()
        return o

    el, _, _ = timed_blocks(run, steps, warmup, fence, dist, dev, blocks=5, warm_seconds=0.3)
    leg = dict(value=round(img.shape[0] * world * steps / el, 1), unit="alerts/s", steps=steps,
               ms_per_step=round(1e3 * el / steps, 4), api="drop-in model(...) calls, one stream")
    if precision in ("f16", "f16x2"):
        # the scoring loop of the headline (ScoreStream) in this mode as well
        scorer = btsbot_amd.ScoreStream(m, inputs_ready=True)

        def run_pipelined(n):
            last = None
            for last in scorer.map(((img, meta) for _ in range(n)), lag=n):
                pass
            return last

        el2, _, _ = timed_blocks(run_pipelined, steps, warmup, fence, dist, dev, blocks=5, warm_seconds=0.3)
        leg["streamed"] = dict(value=round(img.shape[0] * world * steps / el2, 1), ms_per_step=round(1e3 * el2 / steps, 4),
                               api="btsbot_amd.ScoreStream, three batches in flight")
        del scorer
    if with_parity:
        leg["parity"] = parity_vs_oracle(m, img, meta)
    return leg


def nano_leg(precision, dev, img, meta, steps, warmup, fence, dist, world, with_parity=True):
    """The reference classes' DEFAULT backbone (`convnext_nano.d1h_in1k`, /root/reference/btsbot/architectures.py:107,128)
    on the benched batch: plain model(...) calls and the three-stream scoring loop.  (Stage 2 + last downsample, stage 3
    and the head run the fused kernels; the stem and stages 0-1 the per-op schedule: DESIGN.md section 4b / 4c.)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cfg = dict(CONFIG, model_kind="convnext_nano.d1h_in1k")
        m = btsbot_amd.mm_ConvNeXt(cfg, precision=precision)
    seeded_weights(m)
    m = m.to(dev).eval()

    def run(n):
        o = None
        with torch.no_grad():
            for _ in range(n):
                o = m(image_input=img, metadata_input=meta)
        return o

    el, _, _ = timed_blocks(run, steps, warmup, fence, dist, dev, blocks=5, warm_seconds=0.3)
    leg = dict(workload="mm_ConvNeXt over convnext_nano.d1h_in1k (dims 80/160/320/640, depths 2/2/8/2), same batch",
               value=round(img.shape[0] * world * steps / el, 1), unit="alerts/s", steps=steps,
               ms_per_step=round(1e3 * el / steps, 4), api="drop-in model(...) calls, one stream",
               flop_per_alert=236811200)
    leg["whole_net_tflops"] = round(leg["flop_per_alert"] * leg["value"] / 1e12, 2)
    scorer = btsbot_amd.ScoreStream(m, inputs_ready=True)

    def run_pipelined(n):
        last = None
        for out in scorer.map(((img, meta) for _ in range(n)), lag=n):
            last = out
        return last

    el2, _, _ = timed_blocks(run_pipelined, steps, warmup, fence, dist, dev, blocks=5, warm_seconds=0.3)
    leg["streamed"] = dict(value=round(img.shape[0] * world * steps / el2, 1), ms_per_step=round(1e3 * el2 / steps, 4),
                           api="btsbot_amd.ScoreStream, three batches in flight")
    if with_parity:
        leg["parity"] = parity_vs_oracle(m, img, meta, cfg=cfg)
    return leg


def precision_leg_on(m, img, meta, steps, warmup, fence, dist, world):
    """Throughput of an existing model on another batch (no parity figures)."""
    def step():
        with torch.no_grad():
            return m(image_input=img, metadata_input=meta)

    def run(n):
        o = None
        for _ in range(n):
            o = step()
        return o

    el, _, _ = timed_blocks(run, steps, warmup, fence, dist, dev_of(img), blocks=5, warm_seconds=0.3)
    leg = dict(value=round(img.shape[0] * world * steps / el, 1), unit="alerts/s", steps=steps,
               ms_per_step=round(1e3 * el / steps, 4), api="drop-in model(...) calls, one stream")
    leg["roofline"] = family_roofline(m, run, img.shape[0], m.precision, max(steps, 10))
    return leg


def family_roofline(m, run, batch, precision, steps):
    """The pointwise-conv kernel family's roofline object for `steps` calls of `run(1)` on `batch` alerts per call: HIP
    events around every launch (btsbot_set_profile), algorithmic FLOP per family from family_work."""
    m.set_profile(True)
    run(steps)
    prof = m.collect_profile()
    m.set_profile(False)
    work = family_work(batch, precision)
    peak = MFMA_PEAK_TFLOPS[precision]
    per_kernel, fam_flop, fam_ms, fam_floor_ms = {}, 0.0, 0.0, 0.0
    for k in POINTWISE:
        ms, n = prof.get(k, (0.0, 0))
        if n == 0 or work[k]["flop"] == 0:
            continue
        # the peak is the KERNEL's: in the fp8 mode stage2p / s3_* issue v_mfma_scale_f32_*_f8f6f4 (~5 PFLOP/s dense),
        # stage0b / stage1b stay on the bf16 instructions (~2.5)
        kpeak = FP8_KERNEL_PEAK_TFLOPS if precision == "fp8" and k in FP8_KERNELS else peak
        ach = work[k]["flop"] * steps / (ms * 1e-3) / 1e12
        per_kernel[k] = {"achieved": round(ach, 2), "peak": kpeak, "frac": round(ach / kpeak, 4),
                         "launches_per_call": n // steps, "ms_per_call": round(ms / steps, 4)}
        fam_flop += work[k]["flop"] * steps
        fam_ms += ms
        fam_floor_ms += work[k]["flop"] * steps / (kpeak * 1e12) * 1e3
    if not per_kernel:
        return None
    ach = fam_flop / (fam_ms * 1e-3) / 1e12
    # family fraction = time at each kernel's own peak / measured time (equals achieved / peak when every member has
    # the same peak); `peak` is then the FLOP-weighted harmonic mean of the members' peaks
    fam_peak = fam_flop / (fam_floor_ms * 1e-3) / 1e12
    return {"kernel": "pointwise-conv kernel family, FLOP-weighted: " + " + ".join(per_kernel), "bound": "mfma",
            "achieved": round(ach, 2), "peak": round(fam_peak, 1), "unit": "TFLOP/s", "frac": round(fam_floor_ms / fam_ms, 4),
            "per_kernel": per_kernel, "alerts_per_call": batch}


def dev_of(t):
    return t.device


def host_fed_leg(model, dev, img, meta, args, n_batches=48):
    """The scoring loop fed from HOST memory, the way the reference's loops are fed (a DataLoader's CPU tensors:
    /root/reference/btsbot/inference_example.py:66-82; raw cutouts through make_triplet: alert_utils.py:110-196):
    pinned host batches -> asynchronous copies on a copy stream -> (btsbot_prep_triplets ->) ScoreStream.  Reported
    beside `value` (whose inputs are resident in HBM), never as it: 47,628 fp32 bytes per alert cross PCIe here.
    Forms: fp32 triplets as the reference prepares them; f16 triplets widened on the device (half the bytes on the
    link, one more pass over HBM); raw fp32 cutouts + shapes normalised and padded on the device (btsbot_prep_triplets)."""
    from btsbot_amd.alert_utils import prep_triplets
    B = img.shape[0]
    nbuf = 4
    h_img = [img.cpu().pin_memory() for _ in range(nbuf)]
    h_img16 = [img.cpu().half().pin_memory() for _ in range(nbuf)]
    h_meta = [meta.cpu().pin_memory() for _ in range(nbuf)]
    h_shapes = torch.full((B, 3, 2), 63, dtype=torch.int32).pin_memory()
    copy = torch.cuda.Stream(device=dev)
    scorer = btsbot_amd.ScoreStream(model, depth=max(2, args.pipeline_depth), inputs_ready=False)
    cur = torch.cuda.current_stream(dev)

    def batches(n, form):
        for i in range(n):
            with torch.cuda.stream(copy):
                d_meta = h_meta[i % nbuf].to(dev, non_blocking=True)
                if form == "f16":
                    d_img = h_img16[i % nbuf].to(dev, non_blocking=True).float()
                else:
                    d_img = h_img[i % nbuf].to(dev, non_blocking=True)
                d_shapes = h_shapes.to(dev, non_blocking=True) if form == "raw+prep" else None
                ev = torch.cuda.Event()
                ev.record(copy)
            cur.wait_event(ev)          # ScoreStream's side streams order themselves behind the caller's stream
            if form == "raw+prep":
                d_img, _drop = prep_triplets(d_img, d_shapes, normalize=True)
            yield d_img, d_meta

    out = {"workload": f"{B} alerts per batch from pinned host memory, {n_batches} batches, ScoreStream depth "
                       f"{len(scorer.models)}; inputs cross PCIe inside the timed region",
           "note": "never `value`: the headline's inputs are resident in HBM (BASELINE.json north_star)"}
    for form, bytes_per_alert in (("fp32", 3 * 63 * 63 * 4 + 25 * 4), ("f16", 3 * 63 * 63 * 2 + 25 * 4),
                                  ("raw+prep", 3 * 63 * 63 * 4 + 25 * 4 + 24)):
        for _ in scorer.map(batches(6, form), lag=6):     # warm-up: allocator pools, pinned-copy path
            pass
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        last = None
        for last in scorer.map(batches(n_batches, form), lag=8):
            pass
        torch.cuda.synchronize(dev)
        el = time.perf_counter() - t0
        out[form] = {"value": round(B * n_batches / el, 1), "unit": "alerts/s", "ms_per_batch": round(1e3 * el / n_batches, 4),
                     "pcie_gbs": round(B * n_batches * bytes_per_alert / el / 1e9, 2),
                     "host_bytes_per_alert": bytes_per_alert, "finite": bool(torch.isfinite(last).all().item())}
    return out


def train_leg(dev, rank, world, dist, fence, args, precision=None, steps=None, batch=None):
    """BASELINE.json configs[2]: the training step of mm_ConvNeXt, every parameter trainable."""
    from btsbot_amd.train import Trainer
    import copy
    if precision is not None or batch is not None:
        args = copy.copy(args)
        args.precision = precision or args.precision
        args.train_steps = steps or args.train_steps
        args.train_batch = batch or args.train_batch
    tcfg = dict(CONFIG, meta_dropout=0.25, comb_dropout=0.2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tm = btsbot_amd.mm_ConvNeXt(tcfg, precision=args.precision)
    seeded_weights(tm)
    tm = tm.to(dev).train()
    timg, tmeta, tlab = synthetic_batch(args.train_batch, seed=100 + rank)
    timg, tmeta, tlab = timg.to(dev), tmeta.to(dev), tlab.to(dev)
    tr = Trainer(tm, lr=1e-4, betas=(0.99, 0.99), pos_weight=1.0, epochs=8, warmup_epochs=2)
    def run(n):
        o = None
        for _ in range(n):
            o = tr.step(timg, tmeta, tlab)
        return o

    tel, tblocks, tloss = timed_blocks(run, args.train_steps, 3, fence, dist, dev, blocks=5)
    train = {
        "workload": "BASELINE.json configs[2]: mm_ConvNeXt-pico training step (BCE pos_weight + "
                    "backward + AdamW), every parameter trainable, one RCCL all-reduce of the "
                    "flat gradient arena per step",
        "value": round(args.train_batch * world * args.train_steps / tel, 1), "unit": "alerts/s",
        "per_gpu_batch": args.train_batch, "global_batch": args.train_batch * world,
        "steps": args.train_steps, "ms_per_step": round(1e3 * tel / args.train_steps, 3),
        "blocks_ms_per_step": [round(1e3 * b / args.train_steps, 3) for b in tblocks],
        "loss_finite": bool(torch.isfinite(tloss).item()),
        "operands": args.precision,
        "forward": ("stem + stage 0 (+ stage 1 in f16) through the inference megakernels' keeping forms, the rest per-op"
                    if args.precision in ("bf16", "f16") else "per-op launches"),
    }
    # whole-step roofline: forward + input gradients + filter gradients = 3 x the forward's algorithmic FLOP
    step_flop = 3.0 * (133701376 + 210000) * args.train_batch
    achieved = step_flop / (tel / args.train_steps) / 1e12
    train["roofline"] = {"kernel": "whole training step (forward, backward, AdamW; ~260 launches)", "bound": "mfma",
                         "achieved": round(achieved, 2), "peak": MFMA_PEAK_TFLOPS[args.precision], "unit": "TFLOP/s",
                         "frac": round(achieved / MFMA_PEAK_TFLOPS[args.precision], 4),
                         "flop_per_step": step_flop}
    tg = pmc_traffic_train(args)
    if tg is not None:
        train["roofline"].update(tg)
    if world > 1:
        # what the gradient exchange costs in wall time: the same step with the all-reduce left out (the replicas drift
        # apart from here on: timing only, after the measurement above)
        def run_local(n):
            o = None
            for _ in range(n):
                o = tr.step(timg, tmeta, tlab, exchange=False)
            return o

        tloc, _, _ = timed_blocks(run_local, args.train_steps, 2, fence, dist, dev, blocks=5, warm_seconds=0.2)
        train["allreduce_exposed_ms_per_step"] = round(1e3 * (tel - tloc) / args.train_steps, 4)
        train["ms_per_step_without_exchange"] = round(1e3 * tloc / args.train_steps, 3)
        train["exchange"] = "3 gradient buckets, async all_reduce(SUM) on a side stream behind the bucket's HIP event"
    del tm, tr
    return train


def main():
    args = parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # Rehearsal of the N > 1 code path on a one-GPU box (BTSBOT_BENCH_REHEARSAL=1): every rank on cuda:0, collectives
    # through gloo on device tensors.  Not a measurement -- the ranks share one GPU -- and the line says so.
    rehearsal = os.environ.get("BTSBOT_BENCH_REHEARSAL", "0") == "1"
    if rehearsal:
        local_rank = 0
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if local_rank >= torch.cuda.device_count():
        raise SystemExit(f"rank {rank}: local rank {local_rank} but {torch.cuda.device_count()} GPUs visible")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (no CPU fallback)")
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    ranks_seen = 1
    if dist is not None:
        one = torch.ones(1, device=dev)
        dist.all_reduce(one)
        ranks_seen = int(round(one.item()))
        if ranks_seen != world:
            raise SystemExit(f"rank {rank}: the {dist.get_backend()} group spans {ranks_seen} ranks, WORLD_SIZE={world}")

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = btsbot_amd.mm_ConvNeXt(CONFIG, precision=args.precision)
    seeded_weights(model)
    model = model.to(dev).eval()
    # each rank gets its own shard of synthetic alerts (seed 2 + rank), resident in HBM
    img, meta, _ = synthetic_batch(args.batch, seed=2 + rank)
    img, meta = img.to(dev), meta.to(dev)

    def step():
        with torch.no_grad():
            return model(image_input=img, metadata_input=meta)

    def fence():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)

    steps2 = min(args.steps, FULL_LEG_STEPS)    # the --full legs' steps per block

    def timed(run):
        return timed_blocks(run, steps2, args.warmup, fence, dist, dev)

    def run_serial(n):
        o = None
        for _ in range(n):
            o = step()
        return o

    pipelined_elapsed = None
    if args.pipeline_depth > 1:
        if args.full:
            # one stream, one model(...) call after the other (the drop-in figures of the --full line)
            serial_elapsed = timed(run_serial)[0] * args.steps / steps2     # (seconds per K steps)
        # the scoring loop as the library runs it over a sequence of batches: consecutive batches on alternating HIP
        # streams (btsbot_amd.ScoreStream), every batch a full pass of the same kernels, all K finished inside the
        # timed region
        scorer = btsbot_amd.ScoreStream(model, depth=args.pipeline_depth, inputs_ready=True)   # (resident, fenced)

        def run_pipelined(n):
            o = None
            # (lag = n: like the serial loop above, the host queues all n steps and waits once at the end)
            for o in scorer.map(((img, meta) for _ in range(n)), lag=n):
                pass
            return o

        pipelined_elapsed, out = timed_steps(run_pipelined, args.steps, args.warmup, fence, dist, dev)
        del scorer
        # The headline is ALWAYS the library's scoring loop (ScoreStream), never the better of the two: two HIP streams
        # only overlap when the runtime gives them different hardware queues; where it does not (seen once in ~20
        # processes) the pipelined loop is the slower one and the line says so (`pipelined_slower_than_serial`).
        headline_depth = args.pipeline_depth
        elapsed = pipelined_elapsed
    else:
        serial_elapsed, out = timed_steps(run_serial, args.steps, args.warmup, fence, dist, dev)
        elapsed, headline_depth = serial_elapsed, 1
    if not os.environ.get("BTSBOT_AMD_S0_DIAG"):
        assert torch.isfinite(out).all()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, logits=out)
    if not args.full:
        if rank == 0:
            print(json.dumps(headline_line(args, world, elapsed, headline_depth)), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- roofline leg: same K steps, every launch bracketed by HIP events on the launch stream
    t_end = time.perf_counter() + WARM_SECONDS
    while time.perf_counter() < t_end:
        run_serial(steps2)
        torch.cuda.synchronize(dev)
    model.set_profile(True)
    prof_steps = max(steps2, 100)           # >= 100 launches per kernel behind the averages
    for _ in range(prof_steps):
        step()
    prof = model.collect_profile()
    model.set_profile(False)

    # ---- parity of the benchmarked model / weights / precision, and the other operand modes on the same batch
    parity, legs = None, {}
    if not args.no_extra_legs:
        parity = parity_vs_oracle(model, img, meta) if rank == 0 else None
        if rank == 0:
            # both ends for a configs[1] user: the stress weights above and trained-like layer scale (gamma ~ 0.1)
            for prec in ("bf16", "f16", "fp8"):
                try:
                    legs[f"{prec}_trained_like"] = {"parity": trained_like_parity(prec, dev, img, meta)}
                except Exception as e:   # noqa: BLE001
                    legs[f"{prec}_trained_like"] = {"error": f"{type(e).__name__}: {e}"}
        for prec in ("f16x2", "f16", "bf16", "f32"):
            if prec == args.precision:
                continue
            try:
                legs[prec] = precision_leg(prec, dev, img, meta, max(5, steps2 // (5 if prec == "f32" else 1)),
                                           3, fence, dist, world, with_parity=(rank == 0))
            except Exception as e:   # noqa: BLE001
                legs[prec] = {"error": f"{type(e).__name__}: {e}"}
        try:
            legs["convnext_nano"] = nano_leg(args.precision, dev, img, meta, max(5, steps2 // 2), 3, fence, dist, world,
                                             with_parity=(rank == 0))
        except Exception as e:   # noqa: BLE001
            legs["convnext_nano"] = {"error": f"{type(e).__name__}: {e}"}
        # BASELINE.json configs[4] (fp8 MFMA inference, batch 8192, streaming throughput): the fp8 mode = stages 2-3's
        # pointwise convolutions on fp8 operands, everything else as in bf16; first this batch size in the
        # benchmarked precision, then the fp8 mode on the benched batch (with its parity) and on 8192 alerts per call
        # through the two-stream scoring loop.  The library works through a call in chunks of 2048 alerts
        try:
            big_img, big_meta, _ = synthetic_batch(8192, seed=3 + rank)
            big_img, big_meta = big_img.to(dev), big_meta.to(dev)
            leg = precision_leg_on(model, big_img, big_meta, max(5, steps2 // 5), 2, fence, dist, world)
            leg["workload"] = "BASELINE.json configs[4] batch size (8192 alerts per call) at %s, serial calls" % args.precision
            legs["batch8192"] = leg
            if args.precision != "fp8":
                legs["fp8"] = precision_leg("fp8", dev, img, meta, steps2, 3, fence, dist, world, with_parity=(rank == 0))
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    m8 = btsbot_amd.mm_ConvNeXt(CONFIG, precision="fp8")
                seeded_weights(m8)
                m8 = m8.to(dev).eval()
                d8 = max(2, args.pipeline_depth)
                sc8 = btsbot_amd.ScoreStream(m8, depth=d8, inputs_ready=True)

                def run8(n):
                    o = None
                    for o in sc8.map(((big_img, big_meta) for _ in range(n)), lag=n):
                        pass
                    return o

                n8 = max(6, steps2 // 8)
                e8, _, _ = timed_blocks(run8, n8, 2, fence, dist, dev, blocks=5, warm_seconds=0.3)
                legs["fp8_batch8192"] = dict(
                    value=round(8192 * world * n8 / e8, 1), unit="alerts/s", steps=n8, ms_per_step=round(1e3 * e8 / n8, 4),
                    workload="BASELINE.json configs[4]: mm_ConvNeXt-pico, fp8 MFMA in stages 2-3, 8192 synthetic alerts per "
                             f"call, {d8} calls in flight (ScoreStream)")

                def run8_plain(n):
                    with torch.no_grad():
                        for _ in range(n):
                            m8(image_input=big_img, metadata_input=big_meta)

                legs["fp8_batch8192"]["roofline"] = family_roofline(m8, run8_plain, 8192, "fp8", 10)
                del sc8, m8
            del big_img, big_meta
        except Exception as e:   # noqa: BLE001
            legs["batch8192"] = {"error": f"{type(e).__name__}: {e}"}
        if rank == 0:
            try:
                legs["host_fed"] = host_fed_leg(model, dev, img, meta, args)
            except Exception as e:   # noqa: BLE001
                legs["host_fed"] = {"error": f"{type(e).__name__}: {e}"}

    # ---- training leg (BASELINE.json configs[2]): mm_ConvNeXt, every parameter trainable,
    #      BCE(pos_weight) + backward + one all-reduce of the flat gradient arena + AdamW per step
    # The two secondary legs must not take the headline line down with them: a failure is reported in its place
    # (an exception on ONE rank of a multi-GPU run can still strand the others in a collective -- nothing here
    # hides that; it is for failures every rank shares, e.g. a reservation that does not fit)
    del out
    train = None
    if args.train_steps > 0:
        try:
            train = train_leg(dev, rank, world, dist, fence, args)
            hk = depthwise_norm_hbm(args)
            if hk is not None:
                train["depthwise_norm_hbm"] = hk
        except Exception as e:   # noqa: BLE001
            train = {"error": f"{type(e).__name__}: {e}"}
        if args.precision != "f32" and not args.no_extra_legs:
            # the reference's own arithmetic is fp32 (/root/reference/btsbot/train.py:141,525-527: no autocast): the same
            # step on exact-fp32 MFMA operands beside the 16-bit one
            try:
                t32 = train_leg(dev, rank, world, dist, fence, args, precision="f32", steps=max(3, args.train_steps // 4))
                t32.pop("roofline", None)
                if isinstance(train, dict):
                    train["f32"] = t32
            except Exception as e:   # noqa: BLE001
                if isinstance(train, dict):
                    train["f32"] = {"error": f"{type(e).__name__}: {e}"}
            # f16 operands: the 16-bit mode whose 50-step trajectory stays closest to the fp32 recipe
            # (tests/test_gpu_train.py::test_16bit_training_follows_the_fp32_recipe) and whose forward runs BOTH
            # megakernels' keeping forms (stage0b + stage1b); no loss scaling: see DESIGN.md section 6 before using it at
            # large batches
            try:
                t16 = train_leg(dev, rank, world, dist, fence, args, precision="f16", steps=max(5, args.train_steps // 2))
                if isinstance(train, dict):
                    train["f16"] = t16
            except Exception as e:   # noqa: BLE001
                if isinstance(train, dict):
                    train["f16"] = {"error": f"{type(e).__name__}: {e}"}
            # the same step on 4 x the alerts per GPU: at 1024 alerts stages 2-3 (9216 / 1024 pixel rows) and the ~260
            # launches of a step leave the chip partly idle; what a user who is free to choose the batch gets
            try:
                big = train_leg(dev, rank, world, dist, fence, args, steps=max(3, args.train_steps // 4),
                                batch=4 * args.train_batch)
                big.pop("roofline", None)
                if isinstance(train, dict):
                    train["batch_x4"] = big
            except Exception as e:   # noqa: BLE001
                if isinstance(train, dict):
                    train["batch_x4"] = {"error": f"{type(e).__name__}: {e}"}
    maxvit = None
    if args.maxvit_steps > 0:
        try:
            maxvit = maxvit_leg(dev, rank, world, dist, fence, args)
        except Exception as e:   # noqa: BLE001
            maxvit = {"error": f"{type(e).__name__}: {e}"}

    maxvit_train = None
    if args.maxvit_train_steps > 0:
        try:
            maxvit_train = maxvit_train_leg(dev, rank, world, dist, fence, args)
        except Exception as e:   # noqa: BLE001
            maxvit_train = {"error": f"{type(e).__name__}: {e}"}

    if rank == 0:
        work = family_work(args.batch, args.precision)
        kernels = {}
        for name, (ms, n) in prof.items():
            if n == 0 or name not in work:
                continue
            per_fwd_ms = ms / prof_steps
            wk = work[name]
            kernels[name] = dict(
                launches_per_step=n // prof_steps, avg_launch_us=round(1e3 * ms / n, 2),
                ms_per_step=round(per_fwd_ms, 4),
                tflops=round(wk["flop"] / (per_fwd_ms * 1e-3) / 1e12, 2),
                gbs=round(wk["bytes"] / (per_fwd_ms * 1e-3) / 1e9, 1))
        peak = MFMA_PEAK_TFLOPS[args.precision]
        # The north star's "pointwise-conv kernel" is a FAMILY here (the 1x1 convolutions of stage i live in stage i's
        # kernel).  Every member that ran is on the line; the headline roofline is their FLOP-weighted aggregate
        # (sum of algorithmic FLOP / sum of launch time), which cannot flip from box to box the way "the member with
        # the most device time" did when two members are within 1 % of each other.
        per_kernel = {}
        fam_flop = fam_ms = fam_floor_ms = 0.0
        for k in POINTWISE:
            ms, n = prof.get(k, (0.0, 0))
            if n == 0 or work[k]["flop"] == 0:
                continue
            fpl = work[k]["flop"] * prof_steps / n
            ach = fpl / (ms / n * 1e-3) / 1e12
            kpeak = FP8_KERNEL_PEAK_TFLOPS if args.precision == "fp8" and k in FP8_KERNELS else peak   # (family_roofline)
            fam_floor_ms += work[k]["flop"] * prof_steps / (kpeak * 1e12) * 1e3
            per_kernel[k] = {"achieved": round(ach, 2), "peak": kpeak, "frac": round(ach / kpeak, 4), "flop_per_launch": fpl,
                             "avg_launch_us": round(1e3 * ms / n, 2), "launches_per_step": n // prof_steps,
                             "traffic": pmc_traffic(k, args), "mfma_busy_pmc": pmc_mfma_busy(k, args)}
            fam_flop += work[k]["flop"] * prof_steps
            fam_ms += ms
        achieved = fam_flop / (fam_ms * 1e-3) / 1e12
        lowest = min(per_kernel, key=lambda k: per_kernel[k]["frac"])
        total_alerts = args.batch * world * args.steps
        line = headline_line(args, world, elapsed, headline_depth)
        line["config"].update(
            drop_in_value=round(total_alerts / serial_elapsed, 1),
            drop_in_ms_per_step=round(1e3 * serial_elapsed / args.steps, 4),
            drop_in_api="plain model(image_input=, metadata_input=) calls on one stream (the reference's "
                        "inference_example.py:84)")
        line.update({
            "pipelined": None if pipelined_elapsed is None else {
                "note": f"btsbot_amd.ScoreStream(depth={args.pipeline_depth}) API: the K steps as consecutive batches on "
                        "alternating HIP streams (not the reference's call signature)",
                "value": round(total_alerts / pipelined_elapsed, 1), "unit": "alerts/s",
                "ms_per_step": round(1e3 * pipelined_elapsed / args.steps, 4)},
            "serial": {"note": "the drop-in call: the same K steps as plain model(image_input=, metadata_input=) calls "
                               "on one stream (the reference's own API, /root/reference/btsbot/inference_example.py:84)",
                       "value": round(total_alerts / serial_elapsed, 1), "unit": "alerts/s",
                       "ms_per_step": round(1e3 * serial_elapsed / args.steps, 4)},
            "pipelined_slower_than_serial": bool(pipelined_elapsed is not None and pipelined_elapsed > serial_elapsed),
            "roofline": {
                "kernel": "pointwise-conv kernel family, FLOP-weighted: " + " + ".join(per_kernel),
                "bound": "mfma", "achieved": round(achieved, 2),
                "peak": round(fam_flop / (fam_floor_ms * 1e-3) / 1e12, 1),
                "unit": "TFLOP/s", "frac": round(fam_floor_ms / fam_ms, 4),
                "traffic": per_kernel[lowest]["traffic"],
                "lowest_member": lowest,
                "per_kernel": per_kernel,
                "flop_per_step": fam_flop / prof_steps, "us_per_step": round(1e3 * fam_ms / prof_steps, 2),
                "launches_timed": prof_steps,
            },
            "kernels": kernels,
            "flop_per_alert": 133701376 + 210000,
            "whole_net_tflops": round((133701376 + 210000) * total_alerts / elapsed / 1e12, 2),
        })
        if parity is not None:
            line["parity"] = parity
        if legs:
            line["precision_legs"] = legs
        if rehearsal:
            line["rehearsal"] = "all ranks on ONE GPU, gloo collectives: exercises the N > 1 code path, not a measurement"
        if dist is not None:
            line["collective"] = dict(backend=dist.get_backend(), ranks=dist.get_world_size(),
                                      note="inference: no data-path collective; training leg: bucketed all-reduce")
        # self-check of a multi-GPU run: how many ranks the collective backend really spans (an all-reduce of ones),
        # and what the gradient exchange costs per step when it is exposed
        line["rccl_ranks_seen"] = ranks_seen
        line["allreduce_exposed_ms_per_step"] = (train or {}).get("allreduce_exposed_ms_per_step") if world > 1 else 0.0
        if train is not None:
            line["train"] = train
        if maxvit is not None:
            line["maxvit"] = maxvit
        if maxvit_train is not None:
            line["maxvit_train"] = maxvit_train
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline()
        # Two lines: everything measured (one long JSON object, also written to gpurun_out/bench_detail.json where that
        # directory exists) FIRST, then the contract's ONE line, kept under 7 KB so that a log tail cannot cut it
        detail = dict(line)
        detail["bench_detail"] = True
        print(json.dumps(detail), flush=True)
        out_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpurun_out")
        if os.path.isdir(out_dir):
            try:
                with open(os.path.join(out_dir, "bench_detail.json"), "w") as fh:
                    json.dump(detail, fh)
            except OSError:
                pass
        print(json.dumps(compact_line(line)), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def _pick(d, *keys):
    """The named keys of a leg that ran; its error where it did not."""
    if not isinstance(d, dict):
        return None
    if "error" in d:
        return {"error": d["error"][:160]}
    return {k: d[k] for k in keys if k in d}


def compact_line(line):
    """The contract's line: the headline, its roofline (per kernel: fraction and launch time only), the CPU baseline,
    parity, the tolerance-compliant mode, and one figure per secondary leg.  The long form is the line printed before it."""
    legs = line.get("precision_legs") or {}
    roof = dict(line["roofline"])
    roof["per_kernel"] = {k: {"frac": v["frac"], "us": v["avg_launch_us"], "n": v["launches_per_step"]}
                          for k, v in roof["per_kernel"].items()}
    if isinstance(roof.get("traffic"), dict):
        roof["traffic"] = {k: roof["traffic"][k] for k in ("bytes_per_launch", "source", "measured_in_this_run", "stale")
                           if k in roof["traffic"]}
    cfg = dict(line["config"])
    for k in ("drop_in_api", "api"):
        cfg.pop(k, None)
    out = {k: line[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                "scaling", "vs_baseline", "dtype", "data")}
    out["config"] = cfg
    out["roofline"] = roof
    if "cpu_baseline" in line:
        cb = dict(line["cpu_baseline"])
        cb.pop("thread_sweep", None)
        out["cpu_baseline"] = cb
    if "parity" in line:
        par = dict(line["parity"])
        for prec in ("bf16", "f16", "fp8"):
            tl = (legs.get(prec + "_trained_like") or {}).get("parity")
            if tl:
                par[prec + "_trained_like_max_abs_dscore"] = tl["max_abs_dscore"]
        out["parity"] = par
    # the operand mode that meets the north star's 1e-4 on scores, at speed (tests/test_gpu_parity.py: five weight seeds)
    x2 = legs.get("f16x2")
    if isinstance(x2, dict) and "value" in x2:
        out["parity_compliant"] = {"mode": "f16x2", "value": x2["value"], "ms_per_step": x2["ms_per_step"],
                                   "max_abs_dscore": (x2.get("parity") or {}).get("max_abs_dscore"),
                                   "api": "drop-in calls", "streamed_value": (x2.get("streamed") or {}).get("value")}
    elif isinstance(x2, dict):
        out["parity_compliant"] = _pick(x2)
    for name in ("f16", "f32", "fp8"):
        lg = legs.get(name)
        if isinstance(lg, dict):
            c = _pick(lg, "value", "ms_per_step")
            if "parity" in lg:
                c["max_abs_dscore"] = lg["parity"]["max_abs_dscore"]
            if isinstance(lg.get("streamed"), dict):
                c["streamed_value"] = lg["streamed"]["value"]
            out[name] = c
    nano = legs.get("convnext_nano")
    if isinstance(nano, dict):
        c = _pick(nano, "value", "ms_per_step", "whole_net_tflops")
        if isinstance(nano.get("streamed"), dict):
            c["streamed_value"] = nano["streamed"]["value"]
        if "parity" in nano:
            c["max_abs_dlogit"] = nano["parity"]["max_abs_dlogit"]
        out["nano"] = c
    for name in ("batch8192", "fp8_batch8192"):
        lg = legs.get(name)
        if isinstance(lg, dict):
            c = _pick(lg, "value", "ms_per_step")
            if isinstance(lg.get("roofline"), dict):
                c["frac"] = lg["roofline"].get("frac")
            out[name] = c
    hf = legs.get("host_fed")
    if isinstance(hf, dict):
        out["host_fed"] = ({"error": hf["error"][:160]} if "error" in hf else
                           {k: {"value": hf[k]["value"], "pcie_gbs": hf[k]["pcie_gbs"]} for k in ("fp32", "f16", "raw+prep")
                            if isinstance(hf.get(k), dict)})
    tr = line.get("train")
    if isinstance(tr, dict):
        c = _pick(tr, "value", "unit", "per_gpu_batch", "steps", "ms_per_step", "operands", "kernel_ms_both_queues")
        if isinstance(tr.get("roofline"), dict):
            c["frac"] = tr["roofline"]["frac"]
            c["traffic_gb"] = tr["roofline"].get("traffic_gb")
        for sub in ("f32", "f16", "batch_x4"):
            if isinstance(tr.get(sub), dict):
                c[sub] = _pick(tr[sub], "value", "ms_per_step", "per_gpu_batch")
        out["train"] = c
    mv = line.get("maxvit")
    if isinstance(mv, dict):
        out["maxvit"] = _pick(mv, "value", "unit", "per_gpu_batch", "ms_per_step", "whole_net_tflops", "frac")
    mvt = line.get("maxvit_train")
    if isinstance(mvt, dict):
        out["maxvit_train"] = _pick(mvt, "value", "unit", "per_gpu_batch", "ms_per_step", "whole_step_tflops")
    for k in ("rccl_ranks_seen", "allreduce_exposed_ms_per_step", "rehearsal", "collective", "pipelined_slower_than_serial"):
        if k in line:
            out[k] = line[k]
    out["detail"] = "the line printed before this one (bench_detail: true); gpurun_out/bench_detail.json"
    return out


def _newest_profile(pattern):
    import glob
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", pattern)))
    return files[-1] if files else None


def csrc_sha16():
    """Digest of the kernel sources the library is built from: a committed PMC summary carries the digest it was
    collected under (tools/collect_profiles.py), and a summary from other sources is marked stale on the line."""
    import glob
    import hashlib
    hsh = hashlib.sha256()
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "btsbot_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(root, "*.hip")) + glob.glob(os.path.join(root, "*.h"))):
        with open(f, "rb") as fh:
            hsh.update(os.path.basename(f).encode() + b"\0" + fh.read())
    return hsh.hexdigest()[:16]


def _stale(summary):
    """True unless the summary says it was collected on the kernels as they are now."""
    return summary.get("csrc_sha16") != csrc_sha16()


def pmc_traffic(kernel, args):
    """HBM-side bytes per launch of `kernel`, NOT measured in this run: PMC counters cannot be sampled from inside
    the process, so the figure comes from the newest committed summary (profiles/r*_pmc_traffic.json: separate
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this same command, FETCH_SIZE doubled per the gfx950
    calibration in tools/pmc_calib) and is tagged with that file.  Only for the workload the summary was collected
    on (default precision and batch) and only when the file knows this kernel symbol; otherwise null."""
    if args.precision != "bf16" or args.batch != PER_GPU_BATCH:
        return None
    f = _newest_profile("r*_pmc_traffic.json")
    if f is None:
        return None
    with open(f) as fh:
        summ = json.load(fh)
    hits = [v for v in summ["kernels"].values() if v["family"] == kernel]
    if len(hits) != 1:
        return None
    return {"bytes_per_launch": hits[0]["traffic_bytes"], "source": "profiles/" + os.path.basename(f),
            "measured_in_this_run": False, "stale": _stale(summ)}


def pmc_traffic_train(args):
    """HBM-side GB per training step from the newest committed summary (profiles/r*_pmc_traffic_train.json: two PMC passes
    over tools/train_bench.py 1024 bf16); not measured in this run, tagged with its file."""
    if args.precision != "bf16" or args.train_batch != 1024:
        return None
    f = _newest_profile("r*_pmc_traffic_train.json")
    if f is None:
        return None
    with open(f) as fh:
        d = json.load(fh)
    tb = (d.get("per_step") or {}).get("traffic_bytes")
    if tb is None:
        return None
    return {"traffic_gb": round(tb / 1e9, 3), "traffic_source": "profiles/" + os.path.basename(f), "traffic_stale": _stale(d)}


def depthwise_norm_hbm(args):
    """Achieved HBM GB/s of the depthwise / normalisation kernels of the training step against the 8 TB/s peak, from
    the newest committed summary (profiles/r*_depthwise_norm_hbm.json, tools/hbm_kernels.py: PMC bytes per launch over
    the kernel trace's average launch duration, same workload).  Not measured in this run; tagged with its file."""
    if args.precision != "bf16" or args.train_batch != 1024:
        return None
    f = _newest_profile("r*_depthwise_norm_hbm.json")
    if f is None:
        return None
    with open(f) as fh:
        d = json.load(fh)
    return {"bound": "hbm", "peak": d["peak_gbs"], "unit": "GB/s", "kernels": d["kernels"],
            "source": "profiles/" + os.path.basename(f), "measured_in_this_run": False, "stale": _stale(d)}


def pmc_mfma_busy(kernel, args):
    """Share of the MFMA pipes' cycles the kernel keeps busy, from the newest committed SQ-counter summary
    (profiles/r*_mfma_util.json, tools/mfma_util.py: SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8),
    one rocprofv3 --pmc pass over this command).  Same caveats and tagging as pmc_traffic."""
    if args.precision != "bf16" or args.batch != PER_GPU_BATCH:
        return None
    f = _newest_profile("r*_mfma_util.json")
    if f is None:
        return None
    with open(f) as fh:
        summ = json.load(fh)
    stem = kernel.replace("_kernel", "")
    hits = [v for v in summ["kernels"] if v["kernel"].split("_kernel")[0] == stem]
    if len(hits) != 1:
        return None
    return {"busy_share": hits[0]["mfma_busy"], "source": "profiles/" + os.path.basename(f),
            "measured_in_this_run": False, "stale": _stale(summ)}


if __name__ == "__main__":
    main()
