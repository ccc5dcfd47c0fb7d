/*
 * btsbot_hip.h -- C ABI of libbtsbot_hip.so: the MI355X (gfx950) implementation of BTSbot's
 * classifier forward/backward hot path.
 *
 * The reference (nabeelre/BTSbot, /root/reference) has no FFI: the path sits behind Python
 * nn.Modules (btsbot/architectures.py) driven by btsbot/train.py and btsbot/inference_example.py.
 * Each entry point below names the reference code it stands in for; the Python host in
 * btsbot_amd/ (same class names, kwargs and state-dict keys as the reference) binds these
 * symbols with ctypes.  INTEGRATION.md shows the stub a BTSbot maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  int status: 0 = OK, <0 = error
 *     (enum below); btsbot_last_error() returns a thread-local message.  No C++ exception
 *     crosses the ABI.
 *   - Every pointer is a BORROWED DEVICE pointer (hipMalloc'd / torch CUDA tensor) that must stay
 *     valid until the work enqueued on `stream` has completed.  `stream` is a hipStream_t passed
 *     as void* (NULL = the legacy default stream).  All work is enqueued asynchronously.  Device
 *     memory is allocated only by the first btsbot_pack_params() on a handle and by
 *     btsbot_reserve(); forward / loss / optimiser calls never allocate, synchronise or copy to
 *     the host -- so a caller may capture them into a hipGraph.
 *   - One handle per GPU and per model replica; a handle is thread-compatible (one thread at a
 *     time), matching "a single Python thread drives the model" (SURVEY.md section 8b).
 *   - Tensors: triplets are [B,3,63,63] fp32 NCHW contiguous exactly as
 *     inference_example.py:62-64 prepares them; metadata is [B,n_meta] fp32; logits/scores are
 *     [B] fp32 (the reference's [B,1]).
 */
#ifndef BTSBOT_HIP_H
#define BTSBOT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BTSBOT_ABI_VERSION 1

enum btsbot_status {
  BTSBOT_OK = 0,
  BTSBOT_ERR_INVALID_ARG = -1,   /* bad config / NULL pointer / shape the kernels do not cover  */
  BTSBOT_ERR_HIP = -2,           /* a HIP runtime call failed (message has hipGetErrorString)    */
  BTSBOT_ERR_WORKSPACE = -3,     /* batch larger than the reserved workspace                     */
  BTSBOT_ERR_UNKNOWN_PARAM = -4, /* parameter name not in the handle's table                     */
  BTSBOT_ERR_STATE = -5          /* call order violated (e.g. backward without a training fwd)   */
};

/* which nn.Module of btsbot/architectures.py the handle reproduces */
enum btsbot_wiring {
  BTSBOT_MM_CONVNEXT = 0,   /* mm_ConvNeXt     architectures.py:125-171 (GELU heads)            */
  BTSBOT_CONVNEXT = 1,      /* ConvNeXt        architectures.py:104-122 (image only)            */
  BTSBOT_FROZEN_FUSION = 2, /* frozen_fusion   architectures.py:296-372 (ConvNeXt + um_nn, ReLU)*/
  BTSBOT_UM_NN = 3,         /* um_nn           architectures.py:277-293 (metadata only)         */
  BTSBOT_MM_MAXVIT = 4,     /* mm_MaxViT       architectures.py:58-101 (maxvit_tiny_rw_224 + GELU heads);
                               the image branch trains (BatchNorm2d batch statistics + the backward of every
                               layer, reserve_train(with_image_grads = 1)) or stays a frozen eval-mode branch
                               under trainable heads / metadata branch (with_image_grads = 0); the two mixed
                               regimes (frozen branch on batch statistics, trainable branch on running
                               statistics) return BTSBOT_ERR_STATE                                        */
  BTSBOT_MAXVIT = 5,        /* MaxViT          architectures.py:25-55  (image only)             */
  BTSBOT_FROZEN_FUSION_MAXVIT = 6 /* frozen_fusion with a MaxViT image branch (head stripped to its global
                               pool, architectures.py:304-308) + um_nn metadata branch, ReLU fusion head:
                               what the published maxvit "-metadata" checkpoints instantiate      */
};

/* arithmetic type of the MFMA operands / staged activations (accumulation is always fp32;
 * the residual stream, LayerNorm, GELU and the heads are fp32 in every mode) */
enum btsbot_precision {
  BTSBOT_F32 = 0,  /* v_mfma_f32_16x16x4_f32: exact fp32 fma chains -- the parity mode          */
  BTSBOT_BF16 = 1, /* v_mfma_f32_16x16x32_bf16                                                   */
  BTSBOT_F16 = 2,  /* v_mfma_f32_16x16x32_f16 (same rate as bf16, 3 more mantissa bits)          */
  BTSBOT_FP8 = 3,  /* inference only: the bf16 schedule with the pointwise convolutions of stages 2-3
                      (55 % of the FLOPs, the filter-streaming-bound part) on the block-scaled fp8 MFMA
                      (v_mfma_scale_f32_16x16x128_f8f6f4 / 32x32x64), OCP e4m3 operands; scaling: see
                      DESIGN.md section 2; training entry points behave as BTSBOT_BF16 */
  BTSBOT_F16X2 = 4 /* split operands: every MFMA operand of the pointwise / downsample convolutions is an f16
                      head plus an f16 remainder (x = hi + lo, 22 significant bits), a product is three
                      v_mfma_f32_*_f16 (hi*hi + hi*lo + lo*hi) -- scores within 1e-4 of the fp32 reference at
                      the 16-bit matrix rate; kernels without a split form run the fp32 schedule.  The
                      training entry points behave as BTSBOT_F32, unless a ConvNeXt handle opts in with
                      btsbot_set_option(h, "train_split", 1): its training step then runs the blocks' and
                      downsamples' matrix products (forward, input and filter gradients) on split operands,
                      gradient operands scaled by a power of two per tensor first */
};

typedef struct btsbot_config {
  int32_t abi_version;   /* = BTSBOT_ABI_VERSION                                                 */
  int32_t wiring;        /* enum btsbot_wiring                                                   */
  int32_t precision;     /* enum btsbot_precision                                                */
  /* timm ConvNeXt table (pico: depths 2,2,6,2 dims 64,128,256,512; nano: 2,2,8,2 / 80..640);
   * MaxViT wirings: maxvit_tiny_rw_224 = depths 2,2,5,2 dims 64,128,256,512 (the 63x63 cutouts are
   * resized to 224x224 inside the library, architectures.py:44-50)                                */
  int32_t depths[4];
  int32_t dims[4];
  int32_t image_size;    /* 63 (the only size the kernels are specialised for)                   */
  int32_t head_norm;     /* 1: pool + LayerNorm2d before flatten (ConvNeXt, frozen_fusion,
                               mm_ConvNeXt on "LS" data); 0: flatten only (architectures.py:142) */
  int32_t n_meta;        /* len(config["metadata_cols"]), 25 in prod_config.json:15-41           */
  int32_t meta_fc1, meta_fc2;           /* metadata branch widths                                */
  int32_t comb_fc1, comb_fc2;           /* fusion head widths (ConvNeXt: fc1_neurons/fc2_neurons)*/
  float meta_dropout, comb_dropout;     /* training-mode dropout probabilities                   */
} btsbot_config;

typedef struct btsbot_ctx* btsbot_handle;

/* One row of the handle's parameter table.  `name` is the canonical (prefix-free) name, e.g.
 * "stages.1.blocks.0.mlp.fc1.weight", "head_norm.weight", "meta.0.running_mean",
 * "comb.2.bias"; the Python host maps the reference's state-dict keys onto these
 * (btsbot_amd/architectures.py).  `offset` is in floats into the master arena. */
typedef struct btsbot_param_info {
  char name[96];
  int64_t offset;
  int64_t numel;
  int32_t ndim;
  int32_t shape[4];
  int32_t is_buffer;     /* 1 for BatchNorm running_mean / running_var                           */
} btsbot_param_info;

const char* btsbot_last_error(void);
int btsbot_abi_version(void);

/* Replaces: model_type(config)   (from_HF.py:71-73, train.py:218-222).  Builds the parameter table
 * only -- no HIP call, so it also works on a host without a GPU (the reference constructs on the
 * CPU and then calls .to(device)). */
int btsbot_create(const btsbot_config* cfg, btsbot_handle* out);
int btsbot_destroy(btsbot_handle h);

/* Parameter table: the fp32 "master arena" layout the caller allocates (one flat device buffer of
 * btsbot_param_floats() floats; the Python host makes every nn.Parameter a view into it so that
 * state_dict()/load_state_dict() keep the reference's keys, from_HF.py:74-79). */
int btsbot_param_count(btsbot_handle h);
int64_t btsbot_param_floats(btsbot_handle h);
int btsbot_param_info_at(btsbot_handle h, int index, btsbot_param_info* out);

/* Re-pack the master arena into the kernels' operand layouts (cast to the MFMA type, K-major
 * 1x1 / 2x2 / 4x4 filters, tap-major depthwise filters, BatchNorm folded for eval).
 * Replaces: load_state_dict (from_HF.py:74) / the implicit "weights are where cuDNN wants them".
 * Must be called after every change of the master arena (load, optimiser step). */
int btsbot_pack_params(btsbot_handle h, const float* master_arena, void* stream);
/* The same for a training loop that differentiates the image branch (btsbot_forward_train with
 * keep_image_activations != 0): skips the operand images only the fused inference kernels read; an inference
 * btsbot_forward() afterwards needs a full btsbot_pack_params() first (it returns BTSBOT_ERR_STATE otherwise).
 * Stream rule for both: the forward / forward_train that consumes a pack must be queued on the SAME stream as the pack
 * (or on one the caller has ordered behind it): part of the re-pack runs on a stream of the handle's own, which the
 * consumer joins on its stream, but the arena -> mirror copy is ordered by the pack's stream alone. */
int btsbot_pack_params_train(btsbot_handle h, const float* master_arena, void* stream);

/* Workspace: activations of one chunk of alerts.  reserve() (re)allocates for chunks of up to
 * `max_chunk` alerts; forward() splits larger batches into chunks internally. */
int64_t btsbot_workspace_bytes(btsbot_handle h, int max_chunk);
int btsbot_reserve(btsbot_handle h, int max_chunk);
/* The caller-sized form (no allocation inside the library): `workspace` = at least
 * btsbot_workspace_bytes(h, max_chunk) bytes of 256-byte-aligned device memory that stays the caller's -- borrowed
 * until the next btsbot_reserve() / btsbot_use_workspace() / btsbot_destroy(), never freed here. */
int btsbot_use_workspace(btsbot_handle h, int max_chunk, void* workspace, int64_t bytes);

/* Replaces: model(image_input=..., metadata_input=...) / model(input_data=...) followed by
 * torch.sigmoid (architectures.py:166-171,121-122,292-293,367-372; inference_example.py:84-91).
 * `triplets` may be NULL for BTSBOT_UM_NN, `meta` NULL for BTSBOT_CONVNEXT; `scores` may be NULL.
 * training != 0 selects BatchNorm batch statistics + dropout (seeded by dropout_seed) and keeps
 * the activations needed by btsbot_backward().
 * Range, ConvNeXt pico in BTSBOT_BF16 / BTSBOT_FP8 / BTSBOT_F16: stage 0's two blocks hand fc2 their hidden
 * activations as F16 operands, from a GELU evaluated on packed f16 (DESIGN.md sections 2 and 4a).  A bf16 handle's
 * stage-0 pre-activations (fc1's output, behind a LayerNorm) therefore have f16 RANGE in inference: beyond +-65504
 * they saturate (the activation is then max(x, 0), at most 65504; no inf / NaN).  The training forward (below: the
 * keeping forms, whose own f16 range note concerns the depthwise phase) keeps bf16 hidden activations and
 * gelu_poly<3>, which its backward differentiates. */
int btsbot_forward(btsbot_handle h, const float* triplets_nchw, const float* meta,
                   float* logits, float* scores, int batch, int training,
                   uint64_t dropout_seed, void* stream);

/* Embedding outputs (eval mode): the model's learned representation of every alert next to its logit.
 * Replaces: frozen_fusion.remove_branch_head (architectures.py:298-320) / the embedding step at the end of a run
 * (train.py:449-469).
 *   BTSBOT_EMBED_FEATURES  the input row of the first fusion / head Linear: the image feature (after the global pool
 *                          and, where the wiring has one, the head LayerNorm) followed by the metadata branch's output
 *                          (after its trailing activation where the wiring has one: not in the frozen_fusion wirings,
 *                          whose branch the reference strips of it); dims[3] + meta_fc2 wide, or whichever half exists
 *   BTSBOT_EMBED_HIDDEN    the input row of the last Linear (-> 1), after its activation, dropout as identity:
 *                          comb_fc2 wide; for BTSBOT_UM_NN the same row as the features
 * btsbot_embed_width() is the width in floats (negative: unknown `which`); it touches no device.
 * btsbot_forward_embed() is btsbot_forward(training = 0) -- same preconditions, internal chunks and stream rules,
 * bit-identical logits -- that also writes the rows: `features` / `hidden` are device buffers of [batch][width] fp32,
 * row-contiguous, each may be NULL (as may `scores`; with both NULL this IS the scoring call).  Nothing is
 * allocated, synchronised or copied to the host.  The rows come from the head kernel's own on-chip buffers: in the
 * 16-bit modes they are the split 16-bit operands added back, i.e. the values the next layer multiplies. */
enum btsbot_embedding { BTSBOT_EMBED_FEATURES = 0, BTSBOT_EMBED_HIDDEN = 1 };
int btsbot_embed_width(btsbot_handle h, int which);
int btsbot_forward_embed(btsbot_handle h, const float* triplets_nchw, const float* meta,
                         float* logits, float* scores, float* features, float* hidden,
                         int batch, void* stream);

/* Training-mode forward: replaces model(...) under model.train() (train.py:510).  The image branch
 * is identical to inference (ConvNeXt has no BatchNorm / dropout, drop-path 0); the metadata
 * BatchNorm1d uses the statistics of THIS batch and, when master_arena is non-NULL, updates
 * running_mean / running_var there (momentum 0.1, unbiased variance), exactly as nn.BatchNorm1d --
 * also when the branch is frozen (frozen_fusion keeps its branches in train mode).  Dropout is
 * applied with caller-supplied keep-masks (uint8 [batch][meta_fc1] and [batch][comb_fc2]; 1 = keep,
 * scaled by 1/(1-p)); the masks must stay valid until btsbot_backward() has run.  Activations are
 * kept in a cache sized by btsbot_reserve_train(max_batch, with_image_grads) (whole batch, no
 * chunking, because of the batch statistics).  keep_image_activations != 0 runs the image branch
 * through the per-op training schedule that keeps, per block, x_in / LN output / fc1 pre-activation /
 * hidden activation (about 1.2 MB per alert; 2.8 MB with the backward's own per-block buffers) for a later
 * btsbot_backward(need_image_grads=1);
 * otherwise the image branch runs the fused inference kernels.  The MaxViT wirings take only that second form:
 * their BatchNorm2d layers use the running statistics (a frozen, eval-mode branch under trainable heads).
 * 16-bit modes, pico: stem + stage 0 (+ stage 1 in the f16 mode) run the inference megakernels' keeping forms, whose
 * depthwise phase reads its map and taps as F16 operands in EVERY mode (bf16 taps moved the 50-step loss curve ten
 * times further from the fp32 recipe): a bf16 handle's stage-0/1 residual stream therefore has f16 RANGE during
 * training -- values beyond +-65504 are saturated on their way into that phase (no inf / NaN), and the backward
 * differentiates the convolution as written.  BTSBOT_AMD_NO_S0_TRAIN=1 (and NO_S1_TRAIN=1) at btsbot_create restores
 * the per-op forward with its fp32 depthwise operands. */
int btsbot_reserve_train(btsbot_handle h, int max_batch, int with_image_grads);
int btsbot_forward_train(btsbot_handle h, const float* triplets_nchw, const float* meta,
                         float* logits, float* scores, int batch, const uint8_t* meta_keep_mask,
                         const uint8_t* comb_keep_mask, float* master_arena,
                         int keep_image_activations, void* stream);

/* Replaces loss.backward() (train.py:526) for the parameters of the fusion head (always) and the
 * metadata branch (need_meta_grads): writes d(loss)/d(param) into grad_arena, which has the master
 * arena's layout (other entries are left untouched).  dlogits = d(loss)/d(logits) [batch], e.g. from
 * btsbot_bce_fwd_bwd.  need_image_grads != 0 also differentiates the ConvNeXt image branch (stem,
 * every block, downsamples, head LayerNorm); some of those gradients are reduced over the batch with fp32
 * atomics, so their last bits vary from run to run.
 * Stream semantics are the caller's: everything is ordered after the work already queued on `stream`, and
 * work queued on `stream` afterwards sees every gradient.  Inside, the weight-gradient kernels run on a second
 * stream the handle owns (forked from and joined back into `stream` with events; BTSBOT_AMD_NO_SIDE_STREAM=1
 * keeps every launch on `stream`). */
int btsbot_backward(btsbot_handle h, const float* dlogits, float* grad_arena, int need_meta_grads,
                    int need_image_grads, void* stream);

/* Input gradients (saliency, SmoothGrad, integrated gradients on a deployed model): what
 * image_input.requires_grad_() ... logits.sum().backward() leaves on the inputs of the stock nn.Module classes.
 * ConvNeXt wirings and BTSBOT_UM_NN; the MaxViT wirings are refused (BTSBOT_ERR_INVALID_ARG).
 * btsbot_forward_keep_eval: btsbot_forward_train in EVAL form -- the metadata BatchNorm1d uses its running statistics
 * (read from the packed mirror: pack first, as for btsbot_forward), dropout is the identity with scale 1 (no masks),
 * nothing in any arena is written.  Activations are kept exactly as by btsbot_forward_train (same cache, same
 * btsbot_reserve_train, keep_image_activations as there), so btsbot_backward / btsbot_backward_inputs may follow and
 * differentiate THIS forward: the BatchNorm backward then treats the statistics as constants and an alert's gradient
 * does not depend on the other alerts of the call.  In the 16-bit modes the image branch runs the training-form
 * kernels: the logits agree with btsbot_forward's to the mode's parity tolerance, not to the bit.
 * btsbot_backward_inputs: btsbot_backward that also returns d(loss)/d(input): d_triplets [batch][3][63][63] fp32 (the
 * layout of triplets_nchw) and d_meta [batch][n_meta] fp32, device buffers, either may be NULL; with both NULL this IS
 * btsbot_backward (same launches, order and streams).  Every element of both is written exactly once (rows / columns
 * 60..62 of the triplets, which the 4x4 / stride-4 stem never reads, as +0.0f): no clearing by the caller, no atomic on the
 * chain that produces them -- two identical calls give identical bits.  Both are ordered on `stream` like every
 * gradient.  A non-NULL d_triplets implies need_image_grads (BTSBOT_ERR_STATE unless the forward kept the image
 * activations); a non-NULL d_meta runs the metadata branch's backward whatever need_meta_grads says.  Parameter
 * gradients are still written to grad_arena on the way.  BTSBOT_ERR_INVALID_ARG for a pointer whose input the wiring
 * does not have.  Behind btsbot_forward_train the gradients are those of the batch-statistics form (the metadata rows
 * couple through the batch mean and variance). */
int btsbot_forward_keep_eval(btsbot_handle h, const float* triplets_nchw, const float* meta, float* logits,
                             float* scores, int batch, int keep_image_activations, void* stream);
int btsbot_backward_inputs(btsbot_handle h, const float* dlogits, float* grad_arena, int need_meta_grads,
                           int need_image_grads, float* d_triplets, float* d_meta, void* stream);

/* Replaces the gradient reduction of torch.nn.DataParallel (train.py:238-240; SURVEY.md section 8b's
 * btsbot_allreduce_grads) -- split in two, because the communicator belongs to the host's process group
 * (torch.distributed over RCCL), not to this library: the library says WHICH parts of the gradient arena
 * btsbot_backward() finishes WHEN, the host issues one all-reduce per part on a side stream.
 * btsbot_grad_buckets: up to `capacity` arena ranges [lo[i], hi[i]) (floats) in the order btsbot_backward()
 * completes them -- ConvNeXt wirings: {last image stage + head LayerNorm + metadata branch + fusion head},
 * {stage 2}, {stem + stages 0-1}; every other wiring: one range over the whole arena.  Returns the count.
 * btsbot_wait_grad_bucket: makes `stream` wait (hipStreamWaitEvent) until the kernels of the LAST
 * btsbot_backward() call that write bucket `bucket` have finished; no host synchronisation.  (The per-bucket events
 * cost the backward a fork of its side stream each, so a handle records them only once it has seen a waiter -- this call
 * or btsbot_allreduce_grads.  A backward that ran before any waiter records ONE event at its end instead, and the FIRST
 * wait on a handle waits on that: `stream` is ordered behind everything that backward queued -- correct, but without
 * the overlap; from the next btsbot_backward() on the wait ends with the bucket.  No stream handle is kept: any thread,
 * any time after btsbot_backward() has returned.) */
int btsbot_grad_buckets(btsbot_handle h, int capacity, int64_t* lo, int64_t* hi);
int btsbot_wait_grad_bucket(btsbot_handle h, int bucket, void* stream);

/* The exchange step of data-parallel training (replaces torch.nn.parallel.DataParallel's reduce_add_coalesced,
 * /root/reference/btsbot/train.py:238-240, 526): all-reduce (SUM) over the ranks of `nccl_comm` (an RCCL ncclComm_t) of
 * `nspans` spans [lo[i], hi[i]) (floats) of the gradient arena `grads`, span i belonging to gradient bucket bucket[i]
 * of btsbot_grad_buckets().  Every collective runs on a stream of the library's own and starts as soon as the LAST
 * btsbot_backward() has written its bucket (the rest of the backward pass keeps `stream`: pass the spans in bucket
 * order); `stream` then waits for all of them, so the btsbot_adamw_step() queued behind this call sees the sums.
 * Local gradients are already scaled by 1 / n_global (btsbot_bce_fwd_bwd), so SUM is the global-batch mean's
 * gradient.  No host synchronisation.  RCCL is resolved at the first call (dlopen of librccl.so.1: the copy already
 * in the process, e.g. PyTorch's, wins) -- the communicator must come from that library; BTSBOT_ERR_STATE if there is
 * none.  `grads` must be the arena the last btsbot_backward() wrote (the bucket events belong to it;
 * BTSBOT_ERR_INVALID_ARG otherwise).  btsbot_set_option(h, "exchange", 1) switches every span from one ncclAllReduce
 * to the direct form for xGMI's point-to-point links: ncclReduceScatter (each rank owns the sum of its 1 / N slice)
 * + ncclAllGather, in place, plus a small ncclAllReduce for what is left after N equal slices.
 * The exchange stream is placed like the backward's side stream: measured (once per caller stream) to run on another
 * hardware pipe than `stream` AND the side stream, so that a long collective kernel does not take turns with the
 * backward's kernels; btsbot_set_option(h, "query_side_apart", 0) tells whether that succeeded. */
int btsbot_allreduce_grads(btsbot_handle h, void* nccl_comm, float* grads, int nspans, const int* bucket,
                           const int64_t* lo, const int64_t* hi, void* stream);

/* Scheduling hints (host-side state read at launch time; results do not depend on them).
 *   "stage2p_alerts": alerts resident per workgroup of the stage-2 kernel -- 0 (default): 5, or 7 where that takes fewer
 *   rounds of one workgroup per CU; 4 / 5: always (36 / 45 of the same 48 matrix columns); 7: always (a scoring loop with several forwards in flight on different streams:
 *   the kernel then leaves ~40 % of the CUs to the other stream at 1024 alerts); 4: always.
 *   "forwards_in_flight": 1 = other forwards run beside this handle's on other streams (a scoring loop sets it around
 *   each forward it queues and clears it behind it): the schedule then takes the forms that hold fewer CUs per launch --
 *   stage 1 with 5 alerts per workgroup (bf16, f16 and fp8 handles), stage 2 with 7 alerts per workgroup unless "stage2p_alerts" says otherwise, and at 512 channels the 1x1 stage on
 *   64-alert / 64-channel tiles (half the workgroups; bf16, f16 and fp8 handles -- f32 and BTSBOT_F16X2 handles accept
 *   the option and keep their tiles).  0 (default): the forms that are fastest for a lone forward.  Reported by
 *   "query_schedule:s1_g5", "query_schedule:s2p_g7" and "query_schedule:s3_wide".
 *   "exchange": form of btsbot_allreduce_grads' collectives -- 0 (default) all-reduce, 1 reduce-scatter + all-gather.
 *   "deterministic" (also BTSBOT_AMD_DETERMINISTIC=1 at btsbot_create; set before btsbot_reserve_train): 1 = the batch
 *   reductions of the ConvNeXt training step that meet through fp32 atomics (LayerNorm / depthwise parameter gradients,
 *   column sums, the fused MLP backward's bias gradient) write partial rows and add them in a fixed order instead: two
 *   identical btsbot_backward() calls give bit-identical gradients (16-bit modes; ~25 small extra launches per step).
 *   btsbot_backward() checks the scratch against the batch BEFORE it launches anything (BTSBOT_ERR_STATE, no state
 *   change); ConvNeXt wirings only (refused for MaxViT, ignored there when it comes from the environment).
 *   "query_side_apart" (a query; `value` ignored): BTSBOT_OK when the second stream of btsbot_backward() and the
 *   exchange stream of btsbot_allreduce_grads() were each measured on a hardware pipe of their own, BTSBOT_ERR_STATE
 *   (and a warning on stderr at the time) when none of eight candidates was: two queues of one pipe take turns of ~50 us,
 *   a 1024-alert step then takes 5-7 ms instead of 2.6.
 *   "query_maxvit_split" (a query; `value` ignored): BTSBOT_OK when the handle's MaxViT image branch runs the matrix
 *   products of its inference forward on split operands -- a BTSBOT_F16X2 handle: fp32 maps split into f16 head +
 *   remainder, three f16 MFMAs per product, the filters packed as head and remainder planes; attention, depthwise,
 *   squeeze-excite, LayerNorm and elementwise kernels stay fp32 --, BTSBOT_ERR_STATE for every other handle
 *   (other precisions, ConvNeXt branches, no image branch).
 *   "train_split" (BTSBOT_F16X2 handles with a ConvNeXt image branch; BTSBOT_ERR_INVALID_ARG for every other handle;
 *   set before the first btsbot_pack_params* / btsbot_reserve_train, BTSBOT_ERR_STATE after -- it adds packed-operand
 *   slots): 1 = the training step's 1x1 / downsample products -- fc1 / fc2 / downsample forward, their input gradients
 *   and their filter gradients -- run on split operands (three f16 MFMAs per product) instead of the fp32 MFMA.  Every
 *   gradient operand is scaled by 2^e before the split, e per tensor from its largest magnitude (chosen on the device,
 *   into [2^14, 2^15)) and undone exactly in the fp32 epilogue / slice reduction.  The stem's filter gradient runs split
 *   too (its raw-pixel patches scaled the same way); the stem's forward convolution, depthwise, LayerNorm, heads, loss
 *   and optimiser stay fp32; inference is unchanged.  0 (default): the fp32 training schedule.
 *   "query_train_split" (a query; `value` ignored): BTSBOT_OK when the handle's training products run split,
 *   BTSBOT_ERR_STATE otherwise.
 *   "query_schedule:<field>" (a query; `value` ignored): BTSBOT_OK when that decision of the handle's resolved kernel
 *   schedule is on (fields and the BTSBOT_AMD_* switches behind them: csrc/schedule.h), BTSBOT_ERR_STATE when it is off,
 *   BTSBOT_ERR_INVALID_ARG for an unknown field. */
int btsbot_set_option(btsbot_handle h, const char* key, int value);

/* Validation aid with no reference counterpart: when on, forward() keeps fp32 copies of the stem and
 * stage outputs (call before btsbot_reserve()). */
int btsbot_set_debug(btsbot_handle h, int on);

/* Developer aid: when non-NULL, the forward's kernels store clocks into device_buffer32, a device buffer of
 * 32 + 16384 + 64 + 2048 = 18528 uint64 entries.  Phase clocks (shader clock) come from one workgroup of each
 * kernel; the per-workgroup regions hold every workgroup's start / end on the 100 MHz wall clock:
 *     [0, 16)            stage 0 phases                [16, 32)         stage 1 phases
 *     [32 + 2 wg]        stage 0 per workgroup (one alert each; left out for chunks above 4096 alerts)
 *     [8224 + 2 wg]      stage 1 per workgroup (two alerts each; likewise), its loop clocks at [12320, 12336)
 *     [16416, 16480)     stage 2 phases                [16480, 16496)   stage 3 phases
 *     [17980, 17996)     head16 phases
 *     [32, 96)           MaxViT handles: the partition kernel's phases, C = 256 then C = 128 (32 each) */
int btsbot_debug_stamps(btsbot_handle h, unsigned long long* device_buffer32);

/* Debug/validation tap: copy an intermediate of the LAST forward chunk to `dst` (fp32).
 * name: "stem", "stage0".."stage3" (NHWC [chunk, P, C]).  Returns the element count or <0. */
int64_t btsbot_read_tap(btsbot_handle h, const char* name, float* dst, int64_t capacity,
                        void* stream);

/* ---- op-level entry points (the ATen ops of SURVEY.md section 2.2 K1-K6, one kernel family each);
 * forward() is a schedule of these.  `prec` is enum btsbot_precision: the type of the staged
 * activations / filters (float, bf16 or f16 device arrays); fp32 everywhere else. ---- */

/* K4/K5/K6: out = epi(X[M,K] . W[N,K]^T + bias[N]) on MFMA.  Replaces conv2d 1x1 (+gelu) /
 * conv2d 1x1 + layer-scale + residual / conv2d 2x2 s2 on pre-gathered patches.
 *   epi 0: out (prec) = gelu(acc + bias)         epi 1: out (f32) = resid + gamma * (acc + bias)
 *   epi 2: out (f32) = acc + bias.   K % (16/sizeof(prec)) == 0, N % 4 == 0.
 *   epi 6: out (prec) = silu(acc + bias)        epi 7: out (prec) = acc + bias
 *   prec BTSBOT_F16X2: X and W are f32; W is split into f16 head + remainder planes inside the call (a stream-ordered
 *   scratch of N*K*4 bytes), X in registers, three f16 MFMAs per product; every output is f32 (epi 0, 1, 2, 6, 7),
 *   K % 8 == 0, N % 4 == 0. */
int btsbot_op_gemm(int prec, int epi, const void* X, const void* W, const float* bias,
                   const float* gamma, const float* resid, void* out, int M, int N, int K,
                   void* stream);
/*   The training epilogues (fp32 X, W and outputs in BTSBOT_F32; BTSBOT_F16X2 takes them as well):
 *   epi 3: resid (f32) = acc + bias, out = gelu(resid)      epi 4: out = acc * gelu'(resid)      epi 5: out = acc
 *   (BTSBOT_F16X2, epi 4 / 5: X is a gradient -- scaled by a power of two from its largest magnitude before the split,
 *   as in the split training step). */
/* Filter gradient of a 1x1 convolution: out[n][k] += sum_m D[m][n] A[m][k], colsum[n] += sum_m D[m][n] (colsum may be
 * NULL).  D [M][N], A [M][K] pixel-major, fp32 unless said otherwise; out [N][K] fp32.  prec BTSBOT_F32: the fp32
 * training kernel; BTSBOT_BF16 / BTSBOT_F16: D and A of that type, the 16-bit training step's kernel (N, K multiples
 * of 8, D and A 16-byte aligned; slice partials in a stream-ordered scratch of 64 MB, then the two-pass reduction);
 * BTSBOT_F16X2: the split form of the split training step (N, K multiples of 16; D and A each scaled by a power of two
 * from its largest magnitude, as the step's stem does; slice partials added in a fixed order; a stream-ordered scratch
 * of 64 MB). */
int btsbot_op_wgrad(int prec, const void* D, const void* A, float* out, float* colsum, int M, int N, int K,
                    void* stream);
/* MaxViT MBConv's last 1x1 convolution with the squeeze-excite gate folded into its A operand:
 *   out (f32) [M,N] = resid + (X[m][k] * gate[m / rows_per_alert][k]) . W[N,K]^T      (in place allowed)
 * X, W prec-typed (BTSBOT_F16X2: fp32, W split into f16 head + remainder planes inside the call, as btsbot_op_gemm);
 * gate [ceil(M / rows_per_alert)][K] f32.  In the 16-bit modes X * gate is rounded to prec before the product.
 * K % (16/sizeof(prec)) == 0 (8 for BTSBOT_F16X2), N % 4 == 0. */
int btsbot_op_gemm_gated(int prec, const void* X, const float* gate, int rows_per_alert, const void* W,
                         const float* resid, float* out, int M, int N, int K, void* stream);
/* The batched residual GEMM of the 16-bit MaxViT forward (prec BTSBOT_BF16 / BTSBOT_F16), `batch` problems of M rows:
 *   out_b (f32) [M,N] = resid_b + X_b[M,K] . W_b[N,K]^T      (problem b at X + b*M*K, W + b*N*K, resid / out + b*M*N;
 *                                                           in place allowed)
 * and, with ln_out != NULL, the next LayerNorm fused: ln_out_b (prec) = LayerNorm_N(out_b row) * ln_w + ln_b, eps 1e-6
 * (N 64 or 128).  K % 64 == 0, N % 64 == 0. */
int btsbot_op_gemm_resid_ln(int prec, const void* X, const void* W, const float* resid, float* out, int batch, int M,
                            int N, int K, const float* ln_w, const float* ln_b, void* ln_out, void* stream);
/* K2+K3: depthwise 7x7 p3 + bias + LayerNorm(C, eps 1e-6).  x [B,HW,HW,C] f32 NHWC ->
 * xn [B,HW,HW,C] (prec).  w_tap_major is [49][C] f32.  (C,HW) in {(64,15),(128,7),(256,3),(512,1),
 * (80,15),(160,7),(320,3),(640,1)}.  Arithmetic: fp32 FMAs on the fp32 map, two-pass variance -- EXCEPT the 15x15 maps
 * in the bf16 / f16 modes, which run the convolution on the matrix pipe: map and taps are rounded to `prec` before
 * the 49 products (fp32 accumulation) and the variance is single-pass (E[d^2] - mean^2, clamped at 0), so an output
 * map whose per-pixel mean dwarfs its spread loses bits there; BTSBOT_AMD_NO_DW15=1 (process-wide) keeps the fp32
 * per-tap kernel. */
int btsbot_op_dwconv_ln(int prec, const float* x, const float* w_tap_major, const float* bias,
                        const float* ln_w, const float* ln_b, void* xn, int B, int HW, int C,
                        void* stream);
/* K1: conv2d 4x4 s4 + bias + LayerNorm(C0).  img [B,3,63,63] f32 -> out [B,225,C0] f32 NHWC;
 * w is [C0][3][4][4] as PyTorch stores it.  C0 in {64, 80}. */
int btsbot_op_stem(const float* img, const float* w, const float* bias, const float* ln_w,
                   const float* ln_b, float* out, int B, int C0, void* stream);
/* K6 prologue: LayerNorm(Cin) + 2x2/s2 patch gather.  x [B,HW,HW,Cin] f32 ->
 * patches [B*(HW/2)^2, 4*Cin] (prec), k = (ky*2+kx)*Cin + c. */
int btsbot_op_ln_patch(int prec, const float* x, const float* ln_w, const float* ln_b,
                       void* patches, int B, int HW, int Cin, void* stream);

/* The MaxViT branch's hand-written kernels one at a time.  Parameters are fp32 in the state-dict layout (timm's
 * names); every call builds the kernel's operand images in a stream-ordered scratch with the pack kernels the handle
 * uses, runs the kernel and releases the scratch on `stream`.  T = the type of `prec`.  Activations are NHWC pixel
 * rows [B*H*H, C]; a partition is the 7x7 window (grid_mode 0) or the 7x7 dilated grid (grid_mode 1) of an H x H map,
 * H a multiple of 7.  What a kernel cannot run comes back as BTSBOT_ERR_INVALID_ARG with a message.
 *
 * Multi-head attention inside the partitions: qkv [B*H*H, 3C] T, channel order [head][q|k|v][32]; table [169][C/32]
 * f32 = attn.rel_pos.relative_position_bias_table; out [B*H*H, C] T.  impl 0: the per-query kernel (BTSBOT_F32 /
 * BF16 / F16), impl 1: the MFMA kernel (BF16 / F16). */
int btsbot_op_mv_attn(int prec, int impl, const void* qkv, const float* table, void* out, int B, int H, int C,
                      int grid_mode, void* stream);
/* C = 64, BF16 / F16: x (f32, in place) += proj(attention(qkv(xn))), xn2 (T) = LayerNorm(x) * ln2_w + ln2_b (eps
 * 1e-6).  xn [B*H*H, 64] T is norm1's output; qkv_w [192][64], proj_w [64][64]; xn2 may alias xn. */
int btsbot_op_mv_attn_block(int prec, const void* xn, float* x, void* xn2, const float* qkv_w, const float* qkv_b,
                            const float* proj_w, const float* proj_b, const float* table, const float* ln2_w,
                            const float* ln2_b, int B, int H, int grid_mode, void* stream);
/* C in {64, 128, 256}, BF16 / F16: a partition block in one launch, x [B*H*H, C] f32 in place:
 *   x += proj(attention(qkv(LayerNorm1(x))));  with fc1_w != NULL also  x += fc2(gelu(fc1(LayerNorm2(x)))).
 * ln2_w .. fc2_b are all given or all NULL (the attention half alone).  post_out != NULL: also
 * post_out [B*H*H, C] T = x * post_s[c] + post_b[c] (the next block's pre-norm BatchNorm copy). */
int btsbot_op_mv_part(int prec, float* x, const float* ln1_w, const float* ln1_b, const float* qkv_w,
                      const float* qkv_b, const float* proj_w, const float* proj_b, const float* table,
                      const float* ln2_w, const float* ln2_b, const float* fc1_w, const float* fc1_b,
                      const float* fc2_w, const float* fc2_b, const float* post_s, const float* post_b,
                      void* post_out, int B, int H, int C, int grid_mode, void* stream);
/* Depthwise 3x3 p1 (stride 1 / 2) + per-channel scale + bias + SiLU: in [B,H,H,C] T -> out [B,H/s,H/s,C] T =
 * silu(conv(in, w) * scale[c] + bias[c]); w [C][1][3][3].  impl 0: one thread per output vector (F32 / BF16 / F16,
 * part unused).  impl 1 (BF16 / F16; C/8 divides 256 or equals it, H/s a multiple of 7): strips of 7 outputs, and the
 * squeeze-excite pool as partial sums part [B][btsbot_op_mv_dw3_groups(H, C, s)][C] f32 of the rounded outputs. */
int btsbot_op_mv_dw3(int prec, int impl, const void* in, const float* w, const float* scale, const float* bias,
                     void* out, float* part, int B, int H, int C, int stride, void* stream);
int btsbot_op_mv_dw3_groups(int H, int C, int stride);
/* MBConv's front half in one kernel (BF16 / F16, CIN = 64, MID a multiple of 64, output maps >= 28x28 in whole
 * tiles): m2 [B,H/s,H/s,MID] T = silu(dw3x3_s(m1) * dw_scale + b2), m1 = T(silu(xn . conv1_w^T + b1));
 * xn [B,H,H,CIN] T, conv1_w [MID][CIN], dw_w [MID][1][3][3]; part [B][btsbot_op_mv_mbconv_front_tiles(H, s)][MID]
 * f32 = per-tile sums of the rounded m2. */
int btsbot_op_mv_mbconv_front(int prec, const void* xn, const float* conv1_w, const float* b1, const float* dw_w,
                              const float* dw_scale, const float* b2, void* m2, float* part, int B, int H, int CIN,
                              int MID, int stride, void* stream);
int btsbot_op_mv_mbconv_front_tiles(int H, int stride);
/* Squeeze-excite gate: gate [B][C] f32 = sigmoid(fc2(silu(fc1(inv_count * sum_r y[b][r][:])))); y [B][HW][C] is a
 * BF16 / F16 map, or BTSBOT_F32 rows of partial sums with HW = their count; fc1_w [RD][C], fc2_w [C][RD]. */
int btsbot_op_mv_se(int prec, const void* y, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                    const float* fc2_b, float* gate, int B, int HW, int C, int RD, float inv_count, void* stream);
/* The stem in the 16-bit modes: bilinear 63 -> 224 (align_corners = False), conv 3x3 s2 (3 -> 32) * bn_scale +
 * bn_shift, SiLU (a T map), conv 3x3 s1 (32 -> 64).  img [B,3,63,63] f32; conv1_w [32][3][3][3], conv2_w [64][32][3][3];
 * out f32 = the map [B,112,112,64], or with pooled = 1 its 2x2 average pool [B,56,56,64]; xn != NULL: also
 * xn [B,112,112,64] T = map * pre_scale[c] + pre_shift[c] (the full-resolution map also with pooled = 1: the handle's
 * own form, which pools `out` for the first block's shortcut and keeps xn for its conv1). */
int btsbot_op_mv_stem(int prec, const float* img, const float* conv1_w, const float* bn_scale, const float* bn_shift,
                      const float* conv2_w, float* out, int pooled, void* xn, const float* pre_scale,
                      const float* pre_shift, int B, void* stream);

/* The MaxViT TRAINING kernels (maxvit_train_kernels.hip; these entry points: maxvit_train_ops.hip) one at a time.  Everything is fp32; parameters are in the state-dict
 * layout; activations are NHWC rows.  Every call runs the launcher the training engine itself runs (same kernels, same
 * grid arithmetic) on a stream-ordered scratch of its own.  "+=" outputs are added to, the others written.  What a
 * kernel cannot run (a null pointer, C not a multiple of 4, H not a multiple of 7 for attention or of the stride,
 * more than 16 heads, a stride other than 1 or 2) comes back as BTSBOT_ERR_INVALID_ARG with a message.
 *
 * The launchers' grid decisions: row blocks (gridDim.y) of the BatchNorm reductions over M rows, row blocks of the
 * depthwise filter gradient over npix output pixels, workgroups per head of the attention backward for `units`
 * (alert, partition) pairs. */
int btsbot_op_mvt_bn_row_blocks(int64_t M);
int btsbot_op_mvt_dw3_bwd_w_row_blocks(int64_t npix);
int btsbot_op_mvt_attn_bwd_groups_per_head(int64_t units, int heads);
/* BatchNorm2d on batch statistics (eps 1e-5): y [M][C] = act(xhat * w + b), act 0 none / 1 SiLU; stat [2C] = mean |
 * rstd; run_mean / run_var (both or neither) updated in place with momentum 0.1 and the unbiased variance. */
int btsbot_op_mvt_bn_fwd(const float* x, const float* w, const float* b, float* run_mean, float* run_var, float* y,
                         float* stat, int64_t M, int C, int act, void* stream);
/* ... and its backward: dy is the gradient behind the activation; dx = (accumulate ? dx : 0) + gradient (dx may be
 * dy); dw [C] += , db [C] += . */
int btsbot_op_mvt_bn_bwd(const float* x, const float* dy, const float* stat, const float* w, const float* b, float* dx,
                         float* dw, float* db, int64_t M, int C, int act, int accumulate, void* stream);
/* Depthwise 3x3 p1, stride 1 / 2, w [C][1][3][3]: out [B,H/s,H/s,C] = conv(in [B,H,H,C]) + bias; the input gradient
 * din [B,H,H,C] of dout [B,H/s,H/s,C]; the filter gradient dw [C][1][3][3] += and dbias [C] += . */
int btsbot_op_mvt_dw3_fwd(const float* in, const float* w, const float* bias, float* out, int B, int H, int C,
                          int stride, void* stream);
int btsbot_op_mvt_dw3_bwd_in(const float* dout, const float* w, float* din, int B, int H, int C, int stride,
                             void* stream);
int btsbot_op_mvt_dw3_bwd_w(const float* in, const float* dout, float* dw, float* dbias, int B, int H, int C,
                            int stride, void* stream);
/* Backward of btsbot_op_mv_attn (fp32): qkv [B*H*H, 3C], table [169][C/32], dout [B*H*H, C] -> dqkv [B*H*H, 3C]
 * written, dtable [169][C/32] += . */
int btsbot_op_mvt_attn_bwd(const float* qkv, const float* table, const float* dout, float* dqkv, float* dtable, int B,
                           int H, int C, int grid_mode, void* stream);
/* Squeeze-excite of a2 [B][P][C], fc1_w [RD][C], fc2_w [C][RD]: pool [B][C] = mean over P, rpre [B][RD] = fc1(pool),
 * r = silu(rpre), gate [B][C] = sigmoid(fc2(r)), gated [B][P][C] = a2 * gate.  Backward: d_a2 [B][P][C] written from
 * d_gated; d_fc1_w, d_fc1_b, d_fc2_w, d_fc2_b += . */
int btsbot_op_mvt_se_fwd(const float* a2, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                         const float* fc2_b, float* pool, float* rpre, float* r, float* gate, float* gated, int B, int P,
                         int C, int RD, void* stream);
int btsbot_op_mvt_se_bwd(const float* d_gated, const float* a2, const float* pool, const float* rpre, const float* r,
                         const float* gate, const float* fc1_w, const float* fc2_w, float* d_a2, float* d_fc1_w,
                         float* d_fc1_b, float* d_fc2_w, float* d_fc2_b, int B, int P, int C, int RD, void* stream);
/* dx [B,H,H,C] (+)= 0.25 g [B,H/2,H/2,C];  din [B,H,H,C] = col2im of dcol [B,H,H,9C] (3x3 s1 p1, tap-major);
 * g [O][C][3][3] += gp [O][ldp] (packed (ky*3+kx)*C + c);  out = gelu(pre), d *= gelu'(pre) (erf form, n a multiple
 * of 4);  d [B][P][C] = v [B][C] * scale. */
int btsbot_op_mvt_avgpool2_bwd(const float* g, float* dx, int B, int H, int C, int accumulate, void* stream);
int btsbot_op_mvt_col2im3(const float* dcol, float* din, int B, int H, int C, void* stream);
int btsbot_op_mvt_unpack_conv3_grad(const float* gp, float* g, int O, int C, int ldp, void* stream);
int btsbot_op_mvt_gelu_fwd(const float* pre, float* out, int64_t n, void* stream);
int btsbot_op_mvt_gelu_bwd(const float* pre, float* d, int64_t n, void* stream);
int btsbot_op_mvt_bcast_set(const float* v, float* d, int B, int P, int C, float scale, void* stream);

/* The LayerNorm / depthwise backward kernels of the ConvNeXt TRAINING step (dwln_bwd.hip, ln_dw_bwd.hip) one at a time.
 * Everything is fp32; activations are NHWC rows [B][HW*HW][C]; w = the depthwise taps [49][C] (tap-major, as the
 * engine packs conv_dw.weight); the LayerNorm eps is 1e-6.  Every call runs the launcher the training engine itself
 * runs (same kernels, same grid arithmetic) on the caller's stream, with a stream-ordered scratch of its own for the
 * partial rows.  A null pointer, B or rows < 0, or a shape the launcher has no kernel for comes back as
 * BTSBOT_ERR_INVALID_ARG with a message, before anything is allocated or launched; B = 0 launches nothing.
 * out16 (may be NULL): the same values as the fp32 output next to it, rounded to prec16 = BTSBOT_BF16 / BTSBOT_F16;
 * WRITTEN.  The accumulation contract of every other output is stated per entry point: "+=" outputs are added to
 * (the caller zeroes the gradient arena once per step), "=" outputs are written.
 *
 * The launchers' grid decisions: partial rows (= workgroups) of one dwln_bwd / dw3ln_bwd launch over B alerts; a
 * workgroup of dwln_bwd owns ceil(B / rows) consecutive alerts, the last one what is left. */
int btsbot_op_cnt_dwln_bwd_rows(int HW, int C, int B);
int btsbot_op_cnt_dw3ln_bwd_rows(int B);
/* LayerNorm backward, depthwise filter gradient and depthwise input gradient of a block in one kernel, then the column
 * sum of its partial rows: (HW, C) = (15, 64), (7, 128) or (3, 256).  d = the kept depthwise output, xin = the block's
 * input, g = norm.weight, dxn = the gradient of the LayerNorm output as `nplanes` addend planes pstride floats apart.
 *   dy    += conv(dd, flipped taps)      (dd = LN'(d) . sum of planes never leaves the chip)
 *   arena += [C][49] conv_dw.weight | [C] conv_dw.bias | [C] norm.weight | [C] norm.bias gradients */
int btsbot_op_cnt_dwln_bwd(const float* d, const float* dxn, const float* g, const float* xin, const float* w, float* dy,
                           void* out16, int prec16, float* arena, int B, int HW, int C, int nplanes, int64_t pstride,
                           void* stream);
/* The same for 3x3 maps of 256 channels in their own kernel, which recomputes d from xin, the taps and dwb =
 * conv_dw.bias, then the reduction of its compact rows.  dy += ; arena += as above, where of the 49 taps per channel
 * only the central 5x5 (the ones that meet a 3x3 map) are touched at all. */
int btsbot_op_cnt_dw3ln_bwd(const float* dwb, const float* dxn, const float* g, const float* xin, const float* w, float* dy,
                            void* out16, int prec16, float* arena, int B, int HW, int C, int nplanes, int64_t pstride,
                            void* stream);
/* LayerNorm backward over the C <= 640 channels of each of `rows` rows: dd = (written; it may be dxn itself when
 * patch_hw = 0), dg [C] += , dbeta [C] += .  patch_hw != 0: dxn is the gradient of a 2x2 / stride-2 downsample's patch
 * matrix [B (patch_hw/2)^2][4 C] for input maps of side patch_hw (rows = B patch_hw^2); every input pixel gathers its
 * slice, an odd last row and column get dd = 0 and add nothing to dg / dbeta. */
int btsbot_op_cnt_ln_bwd(const float* d, const float* dxn, const float* g, float* dd, float* dg, float* dbeta, int64_t rows,
                         int C, void* out16, int prec16, int patch_hw, void* stream);
/* 1x1 maps (C <= 640): LayerNorm backward and both depthwise gradients per (alert, channel) in one kernel.
 * dy += dd * w[24];  dg [C] += ;  dbeta [C] += ;  dw [C][49]: tap 24 += , the other 48 untouched;  dbias [C] += . */
int btsbot_op_cnt_ln_dw1_bwd(const float* d, const float* dxn, const float* g, const float* xin, const float* w, float* dy,
                             void* out16, int prec16, float* dg, float* dbeta, float* dw, float* dbias, int64_t rows, int C,
                             void* stream);
/* Depthwise 7x7 p3 on maps of side HW = 15, 7, 3 or 1 (C a multiple of 4):
 * out = conv(x, flip ? flipped taps : taps) [+ bias] [+ addend]  (written; addend may be out itself). */
int btsbot_op_cnt_dw_plain(const float* x, const float* w, int flip, const float* bias, const float* addend, float* out,
                           void* out16, int prec16, int B, int HW, int C, void* stream);
/* Depthwise filter gradient (same shapes): dw [C][49] += sum dd[p] x[p + delta_t], dbias [C] += sum dd; dbias must be
 * dw + 49 C, as in the arena (one column sum covers both), anything else is refused. */
int btsbot_op_cnt_dw_wgrad(const float* x, const float* dd, float* dw, float* dbias, int B, int HW, int C, void* stream);
/* out [N] += the column sums of in [M][N] (fp32): what folds partial rows into the arena. */
int btsbot_op_cnt_colsum_f32(const float* in, float* out, int M, int N, void* stream);
/* The patch stem's input gradient (stem_dgrad.hip), what btsbot_backward_inputs runs last for d_triplets:
 * dimg [B][3][63][63] (written, every element once; rows / columns 60..62 = +0.0f) from dxn [B*225][C0] and the filter
 * w [C0][3][4][4], both fp32 and 16-byte aligned; C0 = 64 or 80. */
int btsbot_op_cnt_stem_dgrad(const float* dxn, const float* w, float* dimg, int B, int C0, void* stream);

/* The MLP half of the ConvNeXt 16-bit TRAINING step (mlp_bwd.hip, s2mlp_bwd.hip, fused_mlp.hip, fc2_grads_kernel of
 * ln_dw_bwd.hip) one launcher at a time (cn_mlp_ops.hip).  prec = BTSBOT_BF16 or BTSBOT_F16 (the "operand type"); biases,
 * gamma and every gradient are fp32.  Same rules as above: the engine's own launchers on the caller's stream, scratch of
 * the call's own, every argument checked before anything is allocated or launched (a null pointer, a negative row
 * count, another prec or a width the launcher has no kernel for: BTSBOT_ERR_INVALID_ARG with a message); zero rows
 * return BTSBOT_OK and touch nothing.
 *
 * The launchers' own figures: addend planes of dxn (1 at C = 64, 4 at C = 128), workgroups along the rows of one
 * mlp_bwd launch (= slices of its partial filter-gradient tiles; a workgroup walks row tiles of 64 in steps of that
 * count), and the rows per workgroup of s2mlp_bwd. */
int btsbot_op_cnt_mlp_bwd_planes(int C);
int btsbot_op_cnt_mlp_bwd_slices(int C, int R);
int btsbot_op_cnt_s2mlp_bwd_rows(void);
/* Backward of a block's MLP y = x + gamma (W2 gelu(W1 xn + b1) + b2) at C = 64 or 128 in one kernel, then the slice
 * reduction of its partial tiles.  xn, dy [R][C], w1 [4C][C], w2g = (diag(gamma) W2)^T [4C][C]: operand type; b1 [4C].
 *   dxn  =  planes x [R][C] addend planes, R * C floats apart; plane s = da[:, slice s] W1[slice s]   (written)
 *   G [C][4C] += dy^T g;   S [C] += colsum(dy);   dW1 [4C][C] += da^T xn;   db1 [4C] += colsum(da)
 * deterministic != 0: db1 and S go through partial rows added in a fixed order (scratch sized from the slice count);
 * BTSBOT_ERR_STATE if that scratch fell short. */
int btsbot_op_cnt_mlp_bwd(int prec, int C, const void* xn, const void* dy, const void* w1, const void* w2g, const float* b1,
                          float* dxn, float* G, float* S, float* dW1, float* db1, int R, int deterministic, void* stream);
/* The input-gradient half of a 256-channel block's MLP backward (C = 256: the only width with a kernel).  dy [R][256], a [R][1024] (the kept fc1 pre-activation),
 * w2gt = (diag(gamma) W2)^T [1024][256], w1t = W1^T [256][1024]: operand type, row-major (packed into MFMA fragments in
 * scratch here).
 *   da  [R + 48][1024] operand type =  (dy (gamma W2)) * gelu'(a): rows 0 .. R-1; the last workgroup also writes its dead
 *       rows R .. ceil(R / rows) * rows - 1 (zeros); nothing behind them is touched                        (written)
 *   dxn [R][256] fp32 = da W1                                                                               (written) */
int btsbot_op_cnt_s2mlp_bwd(int prec, int C, const void* dy, const void* a, const void* w2gt, const void* w1t, void* da,
                            float* dxn, int R, void* stream);
/* The training forward of a block's MLP at C = 64, 80, 128 or 160: xn [M][C] operand type; w1 [4C][C], w2 [C][4C] the
 * fp32 masters (packed in scratch here); b1 [4C], b2, gamma [C].
 *   x [M][C] fp32 = xres + gamma (W2 gelu(W1 xn + b1) + b2)        (written; xres NULL or == x: in place) */
int btsbot_op_cnt_fused_mlp(int prec, int C, const void* xn, const float* w1, const float* w2, const float* b1,
                            const float* b2, const float* gamma, const float* xres, float* x, int M, void* stream);
/* fc2 / layer-scale gradients from G [C][H] = dy^T g and S [C] = colsum(dy) (C, H >= 1):
 *   dW2 [C][H] = gamma G;   db2 [C] = gamma S;   dgamma [C] = <W2, G> rows + b2 S       (all three written)
 *   G and S are read once and LEFT ZERO (they are the next block's accumulators). */
int btsbot_op_cnt_fc2_grads(float* G, float* S, const float* w2, const float* b2, const float* gamma, float* dW2, float* db2,
                            float* dgamma, int C, int H, void* stream);

/* The classifier heads on given rows (head_ops.hip), for the per-kernel tests.  Parameters are fp32 in state-dict layout
 * (a Linear's weight [out][in]); the operand images a handle keeps packed are built in the call's own scratch by the
 * launchers the handle uses.  Same rules as above: arguments checked before anything is allocated or launched.
 *
 * btsbot_op_head: the whole inference head.  feat [B][feat_dim] or NULL (feat_dim 0); hn_w / hn_b [feat_dim] the head
 * LayerNorm, or both NULL; meta [B][n_meta] or NULL (n_meta 0) with the BatchNorm1d four [n_meta], m1_w [f1][n_meta],
 * m1_b [f1], m2_w [f2][f1], m2_b [f2]; meta_trailing_act: the activation behind the second metadata Linear; the fusion
 * MLP: n_layers <= 3, dims[n_layers + 1] (host; dims[0] = feat_dim + f2, dims[n_layers] = 1), comb_w[i] [dims[i+1]][dims[i]],
 * comb_b[i] (host arrays of device pointers); act = 1 (GELU) or 2 (ReLU).
 *   logits [B] (written); scores [B], features [B][dims[0]], hidden [B][dims[n_layers - 1]]: written, each may be NULL.
 * prec BTSBOT_F32 runs head.hip's kernel, BTSBOT_BF16 / BTSBOT_F16 head16.hip's; widths head16 has no kernel for
 * (btsbot_op_head16_supported() == 0) are BTSBOT_ERR_INVALID_ARG with the cause in the message and nothing written --
 * never the fp32 kernel in its place. */
int btsbot_op_head16_supported(int prec, int feat_dim, int n_meta, int f1, int f2, int n_layers, const int* dims);
int btsbot_op_head(int prec, const float* feat, int feat_dim, const float* hn_w, const float* hn_b, const float* meta,
                   int n_meta, const float* bn_w, const float* bn_b, const float* bn_rm, const float* bn_rv,
                   const float* m1_w, const float* m1_b, int f1, const float* m2_w, const float* m2_b, int f2,
                   int meta_trailing_act, int n_layers, const int* dims, const float* const* comb_w,
                   const float* const* comb_b, int act, float* logits, float* scores, float* features, float* hidden, int B,
                   void* stream);
/* The training heads' kernels (head_train.hip, fp32) one launcher at a time.  act: 0 none, 1 GELU, 2 ReLU; mask [M][N]
 * bytes (0: dropped) or NULL.
 *   lin_fwd:    pre [M][N] (NULL: not kept) = bias + in [M][ldi] w [N][K]^T;  outa [M][ldo] = dropout(act(pre)) -- as a fusion
 *               layer's forward runs it: the fp32 MFMA GEMM + activation kernel where btsbot_op_ht_lin_is_wide(M, N, K, ldi),
 *               the per-output kernel otherwise
 *   act_bwd:    dpre [M][N] = dout [M][ldd] * act'(pre) * mask * keep_scale      (dpre may be dout)
 *   lin_bwd_in: din [M][ldi] (columns 0 .. K) = dpre [M][N] w [N][K]; ldi == K takes a fusion layer's decision,
 *               btsbot_op_ht_lin_is_wide(M, K, N, N); ldi > K the per-output kernel
 *   lin_bwd_w:  dw [N][K] = dpre^T in [M][ldi], db [N] = colsum(dpre) (written); btsbot_op_ht_lin_bwd_w_kind says which
 *               kernel a call takes: 0 lin_bwd_w4, 1 lin_bwd_w<4, 64>, 2 lin_bwd_w<16, 16>
 *   bn_fwd:     BatchNorm1d on the batch statistics of x [M][n]: xhat, out [M][n], rstd [n] written; run_mean / run_var
 *               [n] updated (momentum 0.1, unbiased variance) or both NULL
 *   bn_bwd:     dw [n] = sum dy xhat, db [n] = sum dy
 *   bn_eval_fwd: BatchNorm1d on the running statistics run_mean / run_var [n] (read only): xhat, out, rstd as bn_fwd
 *   bn_bwd_in:  the BatchNorm's input gradient dx [M][n] (written).  eval != 0: dx = dy w rstd; eval == 0: the batch-
 *               statistics form (w rstd / M) (M dy - sum_dy - xhat sum_dyx) on bn_bwd's two sums (db, dw), which the eval
 *               form does not read (they may be NULL there)
 *   feat_rows:  z [M][ldz] (columns 0 .. F) = feat [M][F], through LayerNorm (eps 1e-6) where hw / hb are given
 *   logits:     logits [M] = in [M]; scores = sigmoid (NULL: not written)
 *   copy_cols:  dst [M][ldd] (columns 0 .. cols) = src [M][lds] */
int btsbot_op_ht_lin_is_wide(int M, int N, int K, int ldi);
int btsbot_op_ht_lin_fwd(const float* in, int ldi, const float* w, const float* bias, float* pre, float* outa, int ldo, int M,
                         int N, int K, int act, const uint8_t* mask, float keep_scale, void* stream);
int btsbot_op_ht_act_bwd(const float* dout, int ldd, const float* pre, float* dpre, int M, int N, int act,
                         const uint8_t* mask, float keep_scale, void* stream);
int btsbot_op_ht_lin_bwd_in(const float* dpre, const float* w, float* din, int ldi, int M, int N, int K, void* stream);
int btsbot_op_ht_lin_bwd_w_kind(const float* in, int ldi, const float* dw, int N, int K);
int btsbot_op_ht_lin_bwd_w(const float* dpre, const float* in, int ldi, float* dw, float* db, int M, int N, int K,
                           void* stream);
int btsbot_op_ht_bn_fwd(const float* x, int M, int n, const float* w, const float* b, float* run_mean, float* run_var,
                        float* xhat, float* out, float* rstd, void* stream);
int btsbot_op_ht_bn_bwd(const float* dy, int M, int n, const float* w, const float* xhat, const float* rstd, float* dw,
                        float* db, void* stream);
int btsbot_op_ht_bn_eval_fwd(const float* x, int M, int n, const float* w, const float* b, const float* run_mean,
                             const float* run_var, float* xhat, float* out, float* rstd, void* stream);
int btsbot_op_ht_bn_bwd_in(const float* dy, int M, int n, const float* w, const float* xhat, const float* rstd,
                           const float* sum_dy, const float* sum_dyx, float* dx, int eval, void* stream);
int btsbot_op_ht_feat_rows(const float* feat, int F, const float* hw, const float* hb, float* z, int ldz, int M,
                           void* stream);
int btsbot_op_ht_logits(const float* in, float* logits, float* scores, int M, void* stream);
int btsbot_op_ht_copy_cols(float* dst, int ldd, const float* src, int lds, int cols, int M, void* stream);

/* ConvNeXt stage 3 alone (stage3.hip: 1x1 maps, s3_fc1 / s3_fc2), for the per-kernel tests (infer_ops.hip).
 * btsbot_op_cn_stage3 runs `depth` blocks
 *     x += gamma * fc2( GELU( fc1( LN( dw_c * x + dw_b ) ) ) )          (dw_c = the 7x7 depthwise filter's centre tap)
 * in place on x [B][c3] (fp32).  Every parameter is a host array of `depth` device pointers, fp32 in state-dict layout:
 * dw_w [C][1][7][7], dw_b, ln_w, ln_b [C], fc1_w [4C][C], fc1_b [4C], fc2_w [C][4C], fc2_b, gamma [C].  The operand
 * images (tap-major taps, the fc1 / gamma * fc2 fragments, the fp8 scales) are built in the call's scratch by the
 * launchers the handle uses; the hidden-activation scratch of btsbot_op_cn_stage3_hfrag_bytes() bytes starts as 0xFF
 * bytes (NaN in bf16, f16 and e4m3).  wide: 64-alert / 64-channel tiles.  BTSBOT_ERR_INVALID_ARG with a message, nothing
 * launched: what btsbot_op_cn_stage3_supported() refuses (prec BF16 / F16 / FP8 / F16X2, c3 512 / 640, depth 1..4),
 * wide with BTSBOT_F16X2, a null pointer, x or a parameter vector not 16-byte aligned.  B == 0: BTSBOT_OK, nothing touched.
 * btsbot_op_cn_pack_s3: fp32 src [rows][K] (x rowscale[row], or NULL) -> stage 3's A fragments in dst (rows * K values of
 *   2 / 2 / 1 / 4 bytes in BF16 / F16 / FP8 / F16X2; rows a multiple of 32, K of 16 -- 64 in fp8); swap23: tile row r
 *   holds source row (r with bits 2 and 3 exchanged).  fp8: scale [2] (device) receives {S, 1/S}, the values are packed
 *   times S, and swap23 == 0 orders k as s3_fc1 writes the hidden units (fc2's filter).
 * btsbot_op_cn_fp8_scale: scale [2] (device) <- {S, 1/S}, S the power of two with 120 < S max|src[i] rowscale[i / K]| <= 240
 *   ({1, 1} when that maximum is 0); src [n], rowscale [n / K] or NULL. */
int btsbot_op_cn_stage3_supported(int prec, int c3, int depth);
int64_t btsbot_op_cn_stage3_hfrag_bytes(int prec, int c3, int B);
int btsbot_op_cn_stage3(int prec, int c3, int depth, int wide, float* x, int B, const float* const* dw_w,
                        const float* const* dw_b, const float* const* ln_w, const float* const* ln_b,
                        const float* const* fc1_w, const float* const* fc1_b, const float* const* fc2_w,
                        const float* const* fc2_b, const float* const* gamma, void* stream);
int btsbot_op_cn_pack_s3(int prec, const float* src, const float* rowscale, int rows, int K, int swap23, void* dst,
                         float* scale, void* stream);
int btsbot_op_cn_fp8_scale(const float* src, const float* rowscale, int64_t n, int K, float* scale, void* stream);

/* ConvNeXt stage 2 alone (stage2p.hip: 3x3 maps, one persistent launch), for the per-kernel tests (infer_ops.hip).
 * btsbot_op_cn_stage2 runs `depth` blocks
 *     x += gamma * fc2( GELU( fc1( LN( dwconv7x7(x) + dw_b ) ) ) )
 * on x_in [B][9][cw] (fp32, pixel-major 3x3 maps) and then stages[3].downsample (LayerNorm + conv 2x2 stride 2 on pixels
 * 0, 1, 3, 4): out [B][2 cw]; tap_stage (optional) [B][9][cw] receives the stage output in front of the downsample.  The
 * nine per-block parameters are host arrays of `depth` device pointers as in btsbot_op_cn_stage3; ds_ln_w / ds_ln_b [cw],
 * ds_w [2 cw][cw][2][2], ds_b [2 cw].  The operand images (tap-major taps, fc1 / gamma * fc2 fragments, fp8 scales, the
 * downsample's fragments -- bf16 in the fp8 mode) are built in the call's scratch by the launchers the handle uses.
 * alerts_hint: 0 (the library picks) or 4 / 5 / 7 alerts per workgroup (320 channels always run 5, BTSBOT_F16X2 runs 5 for
 * 7); btsbot_op_cn_stage2_alerts(B, hint) returns the library's choice at 256 channels.
 * The keeping form (the training forward) runs when keep_xin / keep_xn / keep_a / keep_hh (host arrays of `depth` device
 * pointers) and ds_patches are given, all or none: per block the input map fp32 [(B + 9) * 9][cw], the LayerNorm output
 * [(B + 9) * 9][cw], the rounded fc1 pre-activation and its GELU [(B + 9) * 9][4 cw] in the operand type, and ds_patches
 * [(B + 9)][4 cw]; every buffer has room for B + 9 alerts (the kernel stores padding rows unconditionally).
 * BTSBOT_ERR_INVALID_ARG with a message, nothing launched: what btsbot_op_cn_stage2_supported() refuses (BF16 / F16 / FP8 /
 * F16X2 at 256 channels, BF16 / F16 at 320, depth 1..8), another alerts_hint, the keeping form outside BF16 / F16 at 256
 * channels or without tap_stage, keep buffers given in part, a null pointer, x_in / out / tap_stage / a parameter vector /
 * a keep buffer not 16-byte aligned, B < 0.  B == 0: BTSBOT_OK, nothing touched.
 * btsbot_op_cn_stage2_rows: the kernel's row-tile form (the MLP half of a MaxViT partition layer at 256 channels, BF16 /
 *   F16): x [rows][256] += gamma * (fc2 GELU(fc1 LN(x) + fc1_b) + fc2_b) in place, 64 rows per workgroup.
 * btsbot_op_cn_pack_s2p: fp32 src [rows][K] (x rowscale[row], or NULL) -> stage 2's A fragments in dst (rows * K values of
 *   2 / 2 / 1 / 4 bytes in BF16 / F16 / FP8 / F16X2; rows a multiple of 16, K of 32 -- 128 in fp8); reorder_down: src is a
 *   downsample filter [rows][cin][2][2] read as k = (2 ky + kx) cin + c, K = 4 cin.  fp8: scale [2] (device) receives
 *   {S, 1/S} and the values are packed times S. */
int btsbot_op_cn_stage2_supported(int prec, int cw, int depth);
int btsbot_op_cn_stage2_alerts(int B, int hint);
int btsbot_op_cn_stage2(int prec, int cw, int depth, int alerts_hint, const float* x_in, int B, const float* const* dw_w,
                        const float* const* dw_b, const float* const* ln_w, const float* const* ln_b,
                        const float* const* fc1_w, const float* const* fc1_b, const float* const* fc2_w,
                        const float* const* fc2_b, const float* const* gamma, const float* ds_ln_w, const float* ds_ln_b,
                        const float* ds_w, const float* ds_b, float* out, float* tap_stage, float* const* keep_xin,
                        void* const* keep_xn, void* const* keep_a, void* const* keep_hh, void* ds_patches, void* stream);
int btsbot_op_cn_stage2_rows(int prec, float* x, int64_t rows, const float* ln_w, const float* ln_b, const float* fc1_w,
                             const float* fc1_b, const float* fc2_w, const float* fc2_b, const float* gamma, void* stream);
int btsbot_op_cn_pack_s2p(int prec, const float* src, const float* rowscale, int rows, int K, int reorder_down, int cin,
                          void* dst, float* scale, void* stream);

/* Measurement aid with no reference counterpart (bench.py's roofline leg): when on, every kernel
 * launch of forward() is bracketed by two HIP events recorded on the launch stream;
 * profile_collect() waits for them and returns, per kernel family (profile_category_name), the
 * summed device time in ms and the number of launches since the last collect. */
int btsbot_set_profile(btsbot_handle h, int on);
int btsbot_profile_categories(void);
const char* btsbot_profile_category_name(int category);
int btsbot_profile_collect(btsbot_handle h, int n_categories, double* ms_sum, int64_t* launches);

/* Replaces: BCEWithLogitsLoss(pos_weight)(logits, labels) and its autograd
 * (train.py:211-212,525-526).  labels are fp32 0/1.  loss_sum (1 float, caller-zeroed)
 * accumulates sum_i l_i (divide by n_global for the mean); dlogits = d(mean loss)/dz over
 * n_global alerts (n_global = global batch across ranks). */
int btsbot_bce_fwd_bwd(const float* logits, const float* labels, float pos_weight,
                       int batch, int n_global, float* loss_sum, float* dlogits, void* stream);

/* Replaces: torch.optim.AdamW.step (train.py:242-246,527): decoupled weight decay, bias
 * correction, eps outside the sqrt-correction exactly as torch (amsgrad off).  Flat arenas of
 * n floats; `step` is 1-based. */
int btsbot_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                      int64_t n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int step, void* stream);

/* ---- the callers either side of the path ---- */

/* Replaces: FlexibleDataset.__getitem__ + DataLoader collation + the torchvision transforms of
 * train.py:178-199 / utils.py:12-48 for a training set resident in HBM.  dst[b] = T_b(src[index[b]]),
 * T_b = rot90^k(vflip?(hflip?(.))) with ops[b] = hflip | vflip<<1 | k<<2 (k quarter turns counter-clockwise,
 * utils.py:44-48); src [N,3,63,63] f32, dst [batch,3,63,63] f32, index int64 [batch] (NULL = identity),
 * ops uint8 [batch] (NULL = no transform).  Pure index permutation: bit-exact. */
int btsbot_augment(const float* src, const int64_t* index, const uint8_t* ops, float* dst, int batch,
                   void* stream);

/* Replaces: the arithmetic of make_triplet (alert_utils.py:110-196) once the host has gunzipped and
 * FITS-decoded the stamps: per cutout (science, template, difference) nanmedian +-inf test, nan_to_num,
 * L2 normalisation (skipped once the alert is flagged), all-zero test, padding to 63x63 with 1e-9 at the
 * bottom / right; output in the float32 NCHW layout of inference_example.py:62-64.
 * raw [batch,3,63,63] f32 with each stamp in the top-left h x w corner; shapes int32 [batch,3,2] = (h, w)
 * per stamp (NULL = all 63x63); triplets [batch,3,63,63] f32; drop uint8 [batch] (NULL = not wanted). */
int btsbot_prep_triplets(const float* raw, const int* shapes, float* triplets, uint8_t* drop, int batch,
                         int normalize, void* stream);

/* Replaces: the gunzip + FITS decode in front of make_triplet (alert_utils.py:139-145), for a whole batch in one
 * launch: stamp s is the `stampData` bytes blob[offsets[s] .. offsets[s+1]) (blob, offsets: device memory; offsets
 * int64 [n_stamps + 1], non-decreasing, trusted; any byte alignment), a gzip member around a single-HDU FITS image.
 * raw [n_stamps][63][63] f32 receives the image, big-endian samples swapped to native order (bit patterns kept), in the
 * top-left h x w corner and zero elsewhere; shapes int32 [n_stamps][2] = (h, w); status uint8 [n_stamps] one of
 * enum btsbot_stamp_status.  With n_stamps = 3 * batch these are btsbot_prep_triplets' raw and shapes.  A stamp with a
 * non-zero status gets an all-zero image and shape (0, 0).
 * Decoded on the device: one gzip member (FEXTRA / FNAME / FCOMMENT / FHCRC skipped, reserved flags refused) of stored,
 * fixed and dynamic deflate blocks -- exactly the code-length sets zlib accepts -- inflating to at most
 * BTSBOT_STAMP_CAP bytes, with ISIZE equal to the bytes produced; then a FITS primary header with SIMPLE = T,
 * NAXIS = 2, BITPIX = -32, 1 <= NAXIS1, NAXIS2 <= 63, no BSCALE / BZERO card, and the whole data unit present.
 * NOT as gzip.decompress: the CRC32 is not verified.  Anything else that is well formed -- bytes after the first member
 * (multi-member files), other BITPIX, scaled data, larger axes, a header value the strict integer parser does not read
 * -- is BTSBOT_STAMP_UNSUPPORTED: the caller's host path decodes it.
 * workspace: btsbot_decode_stamps_workspace(n_stamps) bytes of device memory, 4-byte aligned, the caller's; contents
 * do not matter before and are scratch afterwards.  One launch on `stream`; nothing allocates, synchronises or copies
 * to the host; n_stamps == 0 launches nothing.  BTSBOT_ERR_INVALID_ARG before any HIP call: a NULL pointer, a negative
 * n_stamps, a workspace that is too small or misaligned.  A negative length offsets[s+1] - offsets[s] is
 * BTSBOT_STAMP_BAD_GZIP for that stamp. */
#define BTSBOT_STAMP_CAP 28800   /* four 2880-byte header blocks + the data unit of a 63 x 63 float32 image */
enum btsbot_stamp_status {
  BTSBOT_STAMP_OK = 0,
  BTSBOT_STAMP_BAD_GZIP = 1,     /* magic, method, reserved flags, or a header longer than the stamp          */
  BTSBOT_STAMP_BAD_DEFLATE = 2,  /* the deflate stream breaks a rule or ends early                            */
  BTSBOT_STAMP_TOO_LARGE = 3,    /* inflates to more than BTSBOT_STAMP_CAP bytes                              */
  BTSBOT_STAMP_BAD_TRAILER = 4,  /* no 8-byte trailer, or ISIZE is not the number of bytes produced           */
  BTSBOT_STAMP_BAD_FITS = 5,     /* no END card in the output, or the data unit is shorter than the header says */
  BTSBOT_STAMP_UNSUPPORTED = 6   /* well formed, outside what the device decodes                              */
};
int64_t btsbot_decode_stamps_workspace(int n_stamps);
int btsbot_decode_stamps(const uint8_t* blob, const int64_t* offsets, int n_stamps, float* raw, int32_t* shapes,
                         uint8_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* Replaces: the custom metadata columns of prep_alerts (alert_utils.py:333-441) for a batch of n_alerts alerts that
 * the caller has grouped by object: perm int32 [n_alerts] lists alert indices object by object, in input order inside
 * an object; object k owns perm[seg_offsets[k] .. seg_offsets[k+1]) (seg_offsets int32 [n_objects + 1], ascending from
 * 0 to n_alerts; empty objects are allowed, so n_objects may be an upper bound whose surplus offsets all equal
 * n_alerts).  perm and seg_offsets are trusted device data: they are read on the device and never validated on the
 * host (the kernel clamps offsets to [0, n_alerts] and skips perm entries outside it, nothing more).
 * With O(i) the alerts of i's object and P(i) those of them with (jd, index) <= (jd[i], i), out8 float32
 * [n_alerts][8] (16-byte aligned, input order) = { min, max of magpsf over O(i); min, max of magpsf over P(i);
 * age = jd[i] - first; days_since_peak = jd[i] - jdpk; days_to_peak = jdpk - first; ncovhist[i] - ndethist[i] },
 * first = min(jdstarthist[i], min jd over O(i)) (NaN if jdstarthist[i] is), jdpk = the jd of the earliest alert of
 * P(i) at P(i)'s minimum magpsf.  NaN magpsf are skipped; jd must be finite.  Compared and subtracted in float64,
 * rounded once.  One launch on `stream`, no host synchronisation; n_alerts == 0 launches nothing. */
int btsbot_alert_features(const int32_t* perm, const int32_t* seg_offsets, int n_alerts, int n_objects,
                          const double* jd, const double* magpsf, const double* jdstarthist,
                          const int32_t* ncovhist, const int32_t* ndethist, float* out8, void* stream);

/* Replaces: the per-object loop of the policy metrics in diagnostic_fig (val.py:454-500) for a batch of n_alerts alerts
 * grouped by object exactly as for btsbot_alert_features (perm, seg_offsets, n_objects may be an upper bound with empty
 * objects; trusted device data, clamped, never validated on the host).  policies is a HOST array [n_policies][4] =
 * (thr, cut, k, gate; gate NaN = none), 1 <= n_policies <= 16 per launch, k an integer >= 1.  With P(i) the alerts of
 * i's object with (jd, index) <= (jd[i], i), a policy fires at alert i when at least k alerts j of P(i) have
 * (double)raw_pred[j] > thr and magpsf[j] < cut, and (without a gate, or) min magpsf over P(i) <= gate; NaN magpsf are
 * never valid and are skipped by the minimum.  Per object and policy: obj_pred int32 [n_objects][n_policies] = 1 when the
 * policy fires at any alert; obj_trigger double [n_objects][n_policies][2] = (jd, magpsf) of the (jd, index)-earliest
 * alert it fires at, (-1, -1) when never.  obj_info double [n_objects][3] = (number of alerts, label of the object's
 * first alert in input order (-1: empty object), min magpsf over the object (NaN: none)).  Compared in float64.  One
 * launch on `stream`, no host synchronisation; n_alerts == 0 launches nothing. */
int btsbot_policy_eval(const int32_t* perm, const int32_t* seg_offsets, int n_alerts, int n_objects,
                       const double* jd, const double* magpsf, const float* raw_pred, const int32_t* label,
                       const double* policies, int n_policies, int32_t* obj_pred, double* obj_trigger,
                       double* obj_info, void* stream);

/* Replaces: the alert-level counts behind the reference's diagnostic figure (val.py:185-379 inside diagnostic_fig: the
 * hist2d of score against magnitude with its two marginal histograms, np.histogram of magpsf per TP / FP / TN / FN, the
 * confusion matrix) for a whole split in one launch.
 * magpsf double [n], raw float [n] (the sigmoid scores, compared as the float32 value widened to float64), label int32
 * [n] (0 = negative, anything else positive; not checked): device pointers.  mag_edges [n_mag + 1], score_edges
 * [n_score + 1], class_edges [n_class + 1]: HOST arrays of float64 bin edges, finite and strictly increasing, read before
 * the call returns and compared exactly as passed.  Bin i holds edges[i] <= x < edges[i+1], the last bin also
 * x == edges[n]; any other x, NaN included, is in no bin (numpy's rule).  pred = raw > 0.5 (a NaN score predicts 0).
 * out int64 (device), ADDED INTO -- the caller zeroes it before the first call -- in this order:
 *   joint [n_mag][n_score]   alerts with magpsf in mag bin i AND score in score bin j
 *   mag   [n_mag]            alerts per mag bin, whatever the score (not a row sum of joint)
 *   score [n_score]          alerts per score bin, whatever the magnitude
 *   cls   [4][n_class]       magpsf over class_edges per class, rows TP, FP, TN, FN
 *   total [4]                every alert, by class, whatever its magnitude
 * n_mag, n_score, n_class in 1..64, n_mag * n_score <= 4096, 0 <= n <= 2^38; BTSBOT_ERR_INVALID_ARG before any launch
 * otherwise (also: a NULL pointer, an edge table that is not finite and strictly increasing).  One launch on `stream`,
 * no allocation, no host synchronisation; n == 0 launches nothing.  Integer sums: the result does not depend on the
 * order in which the workgroups add. */
int btsbot_alert_histograms(const double* magpsf, const float* raw, const int32_t* label, int64_t n,
                            const double* mag_edges, int n_mag, const double* score_edges, int n_score,
                            const double* class_edges, int n_class, int64_t* out, void* stream);

/* Replaces: the per-object loops of cut_set_and_assign_splits and create_subset (query_data/train_val_test_split.py:
 * 123-140, 211-231) for a table of n_alerts alerts grouped by object exactly as for btsbot_alert_features (perm,
 * seg_offsets, n_objects may be an upper bound with empty objects; trusted device data, clamped, perm entries outside
 * [0, n_alerts) skipped, never validated on the host).  With O(i) the alerts of i's object, one row per alert in input
 * order, each written by one thread:
 *   pos int32       the alerts of O(i) with a smaller index (i's position in the object, in table order)
 *   size int32      |O(i)|
 *   first_row int32 the smallest index of O(i) (the row of the object's first appearance)
 *   later int32     the alerts j of O(i) with (jd[j], j) > (jd[i], i): per object a permutation of 0 .. size - 1.  A
 *                   NaN jd counts as later than every finite jd; NaN jd among themselves are ordered by index
 *   is_rise uint8   jd[i] <= jd[m], m the lowest index of O(i) at O(i)'s minimum non-NaN magpsf (ties of the minimum go
 *                   to the lowest row, not the lowest jd); 0 when every magpsf of the object is NaN, or jd[i] or jd[m] is
 *   peakmag double  that minimum, NaN if none
 * Compared in float64 (compare-and-select), nothing is rounded.  One launch on `stream`, no atomics, no host
 * synchronisation; n_alerts == 0 launches nothing. */
int btsbot_split_labels(const int32_t* perm, const int32_t* seg_offsets, int n_alerts, int n_objects, const double* jd,
                        const double* magpsf, int32_t* pos, int32_t* size, int32_t* first_row, int32_t* later,
                        uint8_t* is_rise, double* peakmag, void* stream);

/* ---- streaming policy triggers: the rule of btsbot_policy_eval with the per-object history kept on the device ---- */

/* A table of per-object records, one array per field, in CALLER-OWNED device memory (the entry points below never
 * allocate, synchronise or copy to the host).  Open addressing: an object lives at the first slot at or after
 * hash(id) & (capacity - 1), wrapping round, whose key is its id.  The struct itself is host memory, passed by pointer
 * and read before the call returns.
 * counters: BTSBOT_TRIGGER_COUNTER_ROWS rows of 8 int64; the COLUMN SUMS are { objects held, alerts taken, alerts
 * dropped, late alerts, records btsbot_trigger_load found present already, records it found no slot for, objects
 * btsbot_trigger_rehash expired, survivors it found no slot for }. */
#define BTSBOT_TRIGGER_FREE INT64_MIN     /* key of a free slot: the one object id a table cannot hold             */
#define BTSBOT_TRIGGER_COUNTER_ROWS 16
typedef struct btsbot_trigger_table {
  int64_t* key;         /* [capacity]                 object id, BTSBOT_TRIGGER_FREE = free                        */
  int32_t* n_alerts;    /* [capacity]                 alerts taken                                                 */
  double* min_magpsf;   /* [capacity]                 NaN skipped; NaN until a magnitude is seen                   */
  double* last_jd;      /* [capacity]                 the largest jd seen; -inf before                             */
  int32_t* count;       /* [capacity][n_policies]     valid alerts so far                                          */
  double* trigger;      /* [capacity][n_policies][2]  (jd, magpsf) of the alert the policy fired at; (-1, -1)      */
  int64_t* counters;    /* [BTSBOT_TRIGGER_COUNTER_ROWS][8]                                                        */
  int32_t capacity;     /* slots: a power of two                                                                   */
  int32_t n_policies;   /* 1..16, fixed for the life of the table                                                  */
} btsbot_trigger_table;

/* Writes the empty record (free, 0, NaN, -inf, counts 0, triggers -1) into every slot and zeroes the counters.  A new
 * table must be reset before its first use.  One launch on `stream`. */
int btsbot_trigger_reset(const btsbot_trigger_table* table, void* stream);

/* One batch of n_alerts scored alerts into the table.  policies is a HOST array [table->n_policies][4] as for
 * btsbot_policy_eval (the same for every call on a table).  perm int32 [n_alerts] lists the alert indices sorted by
 * (object id, jd, input position); run r (one object's alerts of this batch) owns perm[seg_offsets[r] ..
 * seg_offsets[r+1]) (seg_offsets int32 [n_runs + 1]; empty runs are allowed, so n_runs may be an upper bound whose
 * surplus offsets all equal n_alerts; trusted device data, clamped, never validated on the host).  A run's slot is found,
 * or claimed with a 64-bit compare-and-swap on key; then its alerts are taken in perm's order.  Alert i: n_alerts += 1;
 * i is LATE (counted, and taken all the same) when jd[i] < last_jd; last_jd = max(last_jd, jd[i]); min_magpsf takes
 * magpsf[i] unless that is NaN; per policy count += ((double)raw_pred[i] > thr and magpsf[i] < cut); a policy that has
 * not fired yet fires at i when count >= k and (without a gate, or) min_magpsf <= gate: trigger = (jd[i], magpsf[i])
 * and fired[i][policy] = 1.  A policy fires at most once per object over the life of the table (jd must be >= 0).
 * A run that finds no free slot within `capacity` probes, and a run of the id BTSBOT_TRIGGER_FREE, is DROPPED: its
 * alerts get dropped[i] = 1, change nothing and are counted.  fired uint8 [n_alerts][n_policies] and dropped uint8
 * [n_alerts] are written in full, every element by one writer.  Two updates of one table must be ordered (same stream,
 * or events): concurrent updates are undefined.  One launch on `stream`, no host synchronisation; n_alerts == 0
 * launches nothing. */
int btsbot_trigger_update(const btsbot_trigger_table* table, const double* policies, const int32_t* perm,
                          const int32_t* seg_offsets, int n_alerts, int n_runs, const int64_t* object_id,
                          const double* jd, const double* magpsf, const float* raw_pred, uint8_t* fired,
                          uint8_t* dropped, void* stream);

/* Inserts n_records exported records (the fields of the table, record-major: count int32 [n_records][n_policies],
 * trigger double [n_records][n_policies][2]) with the same find-or-claim.  A record whose id is in the table already,
 * or twice in the set, is not written and counted in counters column 4; one that finds no slot (or carries
 * BTSBOT_TRIGGER_FREE) in column 5: the caller reads the counters to learn of either.  One launch on `stream`. */
int btsbot_trigger_load(const btsbot_trigger_table* table, int n_records, const int64_t* object_id,
                        const int32_t* n_alerts, const double* min_magpsf, const double* last_jd,
                        const int32_t* count, const double* trigger, void* stream);

/* Retention: the objects of src whose last_jd is not below keep_from_jd (a record is EXPIRED when last_jd < keep_from_jd,
 * in exactly this form: a NaN last_jd is kept, a NaN or -inf keep_from_jd expires nothing, +inf every record whose
 * last_jd is a number) are inserted, whole, into dst with the same find-or-claim; dst may have any capacity, so this
 * is also the way to a larger or smaller table.  Nothing is deleted in place: src is only read.  dst MUST HAVE BEEN
 * RESET by the caller (btsbot_trigger_reset, ordered before this call) and must share no array with src; its n_policies
 * must be src's.  Afterwards dst's counters column 0 is the number of survivors moved, column 6 the number of objects
 * expired plus src's column 6, column 7 the number of survivors that found no slot (only a smaller dst can run out; the
 * caller reads the counters to learn of it, and src is still whole), and columns 1-3 (taken, dropped, late) are src's,
 * carried over row by row.  An object that comes back after it was expired is a new object: its policies may fire again.
 * Ordered with the updates of both tables like two updates (same stream, or events).  One launch on `stream`, no
 * allocation, no host synchronisation.  BTSBOT_ERR_INVALID_ARG before any launch: a NULL table or table array, a
 * capacity that is no power of two, src and dst sharing `key`, n_policies differing. */
int btsbot_trigger_rehash(const btsbot_trigger_table* src, const btsbot_trigger_table* dst, double keep_from_jd,
                          void* stream);

/* ---- streaming light-curve features: the columns of btsbot_alert_features with the per-object history on the device ---- */

/* A table of per-object light-curve records, laid out and addressed like btsbot_trigger_table (one array per field in
 * CALLER-OWNED device memory, open addressing with the same hash, BTSBOT_TRIGGER_FREE = free slot and reserved id; the
 * struct itself is host memory, read before the call returns).  counters: BTSBOT_TRIGGER_COUNTER_ROWS rows of 8 int64
 * with the trigger table's columns: the COLUMN SUMS are { objects held, alerts taken, alerts dropped, late alerts,
 * records btsbot_feature_load found present already, records it found no slot for, objects btsbot_feature_rehash
 * expired, survivors it found no slot for }. */
typedef struct btsbot_feature_table {
  int64_t* key;         /* [capacity]  object id, BTSBOT_TRIGGER_FREE = free                                       */
  int32_t* n_alerts;    /* [capacity]  alerts taken                                                                */
  double* first_jd;     /* [capacity]  the smallest jd seen; +inf before                                           */
  double* last_jd;      /* [capacity]  the largest jd seen; -inf before                                            */
  double* peak_mag;     /* [capacity]  the smallest magpsf seen, NaN skipped; NaN until a magnitude is seen        */
  double* peak_jd;      /* [capacity]  the jd peak_mag was first reached at; NaN with peak_mag                     */
  double* max_mag;      /* [capacity]  the largest magpsf seen, NaN skipped; NaN until a magnitude is seen         */
  int64_t* counters;    /* [BTSBOT_TRIGGER_COUNTER_ROWS][8]                                                        */
  int32_t capacity;     /* slots: a power of two                                                                   */
} btsbot_feature_table;

/* Writes the empty record (free, 0, +inf, -inf, NaN, NaN, NaN) into every slot and zeroes the counters.  A new table must
 * be reset before its first use.  One launch on `stream`. */
int btsbot_feature_reset(const btsbot_feature_table* table, void* stream);

/* One batch of n_alerts alerts into the table and their rows out of it.  perm, seg_offsets, n_runs: the grouping of
 * btsbot_trigger_update (alert indices sorted by (object id, jd, input position); empty runs allowed; trusted device
 * data, clamped, never validated on the host).  A run's slot is found, or claimed with a 64-bit compare-and-swap on key;
 * then its alerts are taken in perm's order.  Alert i: n_alerts += 1; i is LATE (counted, and taken all the same) when
 * jd[i] < last_jd; first_jd = min(first_jd, jd[i]); last_jd = max(last_jd, jd[i]); a magpsf[i] that is not NaN replaces
 * (peak_mag, peak_jd) when it is lower, or equal with a lower jd, and max_mag when it is higher.  Then out8 float32
 * [n_alerts][8] (16-byte aligned, input order), from the record as it stands after i = { peak_mag, max_mag, peak_mag,
 * max_mag, jd[i] - first, jd[i] - peak_jd, peak_jd - first, ncovhist[i] - ndethist[i] } with first = min(jdstarthist[i],
 * first_jd) (NaN if jdstarthist[i] is): columns 2-7 of btsbot_alert_features for a time-ordered stream; columns 0-1
 * repeat the so-far values (the whole-curve values are the table's peak_mag / max_mag at the end of the stream).
 * Compared and subtracted in float64, rounded once.  jd must be finite.
 * A run that finds no free slot within `capacity` probes, and a run of the id BTSBOT_TRIGGER_FREE, is DROPPED: its
 * alerts get dropped[i] = 1 and an all-NaN row, change nothing and are counted.  out8 and dropped uint8 [n_alerts] are
 * written in full, every element by one writer.  Two updates of one table must be ordered (same stream, or events).  One
 * launch on `stream`, no host synchronisation; n_alerts == 0 launches nothing. */
int btsbot_feature_update(const btsbot_feature_table* table, const int32_t* perm, const int32_t* seg_offsets,
                          int n_alerts, int n_runs, const int64_t* object_id, const double* jd, const double* magpsf,
                          const double* jdstarthist, const int32_t* ncovhist, const int32_t* ndethist, float* out8,
                          uint8_t* dropped, void* stream);

/* Inserts n_records exported records (the fields of the table) with the same find-or-claim.  A record whose id is in
 * the table already, or twice in the set, is not written and counted in counters column 4; one that finds no slot (or
 * carries BTSBOT_TRIGGER_FREE) in column 5: the caller reads the counters to learn of either.  One launch on `stream`. */
int btsbot_feature_load(const btsbot_feature_table* table, int n_records, const int64_t* object_id,
                        const int32_t* n_alerts, const double* first_jd, const double* last_jd, const double* peak_mag,
                        const double* peak_jd, const double* max_mag, void* stream);

/* Retention, as btsbot_trigger_rehash: the records of src with last_jd >= keep_from_jd (or NaN) into dst, which MUST
 * HAVE BEEN RESET by the caller (btsbot_feature_reset) and shares no array with src; any capacity.  src is only read.
 * dst's counters: column 0 survivors moved, column 6 objects expired (plus src's), column 7 survivors that found no
 * slot, columns 1-3 carried over from src.  An object that comes back after it was expired is a new object: its
 * so-far and peak columns start again (age still follows the packet's jdstarthist).  One launch on `stream`, no
 * allocation, no host synchronisation.  BTSBOT_ERR_INVALID_ARG before any launch: a NULL table or table array, a
 * capacity that is no power of two, src and dst sharing `key`. */
int btsbot_feature_rehash(const btsbot_feature_table* src, const btsbot_feature_table* dst, double keep_from_jd,
                          void* stream);

/* ---- embedding neighbours: exact brute-force k-nearest rows of a bank (csrc/knn.hip) ---- */

/* Replaces: the neighbour search of the embedding step (train.py:449-469, get_torch_embedding).  queries fp32
 * [n_query][dim], bank fp32 [n_bank][dim], row-contiguous device memory; 1 <= dim <= 1024, 1 <= k <= 64, n_bank and
 * n_query < 2^31 -- BTSBOT_ERR_INVALID_ARG with a message, before any HIP call, otherwise (also: an unknown metric,
 * splits outside 0..32, a NULL or misaligned pointer, a workspace that is too small).
 *
 * The bank is searched through a PACKED image the caller owns: btsbot_knn_bank_bytes(n_bank, dim) bytes, 16-byte
 * aligned, one record of 16 + 4 * ceil(dim / 32) * 32 bytes per row (bias, scale, the row scaled by a power of two of its
 * own as f16 head and remainder planes), so the image of rows [0, n) is a prefix of the image of any larger bank and may
 * be copied into a larger buffer as bytes.  btsbot_knn_pack_bank() writes the records of rows [first_row, first_row +
 * n_rows) from `rows` (the fp32 rows themselves, [n_rows][dim]) into `packed`, whose capacity in rows is
 * n_bank_capacity; a record depends on its row and the metric only.  One launch on `stream`.
 *
 * btsbot_knn_query(): idx int64 [n_query][k], dist fp32 [n_query][k] = each query's k nearest bank rows, ascending by
 * (dist as returned, bank index).  dist: BTSBOT_KNN_EUCLIDEAN the Euclidean distance (not squared), BTSBOT_KNN_COSINE
 * 1 - cos (cos = 0 where a row's norm is 0); both recomputed for the rows returned in the direct form from the fp32
 * rows (`bank` must be the rows `packed` was made from, packed for the same metric).  A bank row that holds a non-finite
 * value (or whose squared norm is not finite in fp32) is never returned; a query row that does gets idx = -1, dist = NaN
 * throughout; where fewer than k rows are eligible the tail is idx = -1, dist = +inf.  self_offset < 0: no exclusion;
 * otherwise query row i IS bank row i + self_offset and that one row is not a candidate (by position: duplicates are).
 * The candidates are the k best by (selection score, bank index), the score being |b|^2 - 2 q.b (cosine: -q.b / |b|) on
 * split f16 operands with fp32 accumulation (an fp32-class product); splits = how many slices of the bank a query tile
 * is searched in by separate workgroups, 0 = btsbot_knn_splits()'s choice.  A row's answer is bit for bit independent
 * of splits, of the other rows of the call and of the run.  workspace: btsbot_knn_workspace(...) bytes for the same
 * arguments, 16-byte aligned, the caller's; scratch afterwards.  Three launches on `stream`; nothing allocates,
 * synchronises or copies to the host, nothing of size n_query x n_bank is written; n_query == 0 launches nothing.
 *
 * btsbot_knn_query_grouped(): btsbot_knn_query with rows that belong together.  bank_group int64 [n_bank] and query_group
 * int64 [n_query] (device memory) give every row a group, any value, negative included -- an alert's object; all 64 bits
 * decide equality.  flags:
 *   BTSBOT_KNN_EXCLUDE_SAME   a bank row whose group equals the query row's is never a candidate (self_offset still
 *                             works beside it); needs query_group and bank_group
 *   BTSBOT_KNN_ONE_PER_GROUP  the answer holds at most one row per group, the group's nearest by (selection score, bank
 *                             index) -- the ranking of the candidates --, and is the k nearest GROUPS, ordered by (dist,
 *                             index) of these representatives; needs bank_group (query_group may be NULL), and k <= 32
 *                             (the merge keeps the groups of its splits * k candidates on chip).  A non-finite bank row
 *                             is never a representative; a group whose rows are all non-finite does not exist.
 * Both may be set.  Fewer than k eligible rows / groups: the tail is idx = -1, dist = +inf; a non-finite query row: -1 /
 * NaN.  flags = 0 (groups may be NULL) answers exactly as btsbot_knn_query, with the same kernels.  The workspace is
 * btsbot_knn_workspace_grouped(..., flags) bytes -- btsbot_knn_workspace()'s plus, under BTSBOT_KNN_ONE_PER_GROUP, 8
 * bytes per candidate for the groups of the list entries (ceil(n_query / 128) * 128 * splits * k of them) --; three launches; the answer is bit for bit independent of splits, of
 * the other rows of the call and of the run.  BTSBOT_ERR_INVALID_ARG also for unknown flag bits, a group array a flag
 * needs being NULL, and k > 32 with BTSBOT_KNN_ONE_PER_GROUP. */
enum btsbot_knn_metric { BTSBOT_KNN_EUCLIDEAN = 0, BTSBOT_KNN_COSINE = 1 };
enum btsbot_knn_flags { BTSBOT_KNN_EXCLUDE_SAME = 1, BTSBOT_KNN_ONE_PER_GROUP = 2 };
int64_t btsbot_knn_bank_bytes(int64_t n_bank, int dim);
int btsbot_knn_pack_bank(const float* rows, int64_t first_row, int64_t n_rows, int dim, int metric, void* packed,
                         int64_t n_bank_capacity, void* stream);
int btsbot_knn_splits(int64_t n_query, int64_t n_bank, int dim, int k);
int64_t btsbot_knn_workspace(int64_t n_query, int64_t n_bank, int dim, int k, int splits);
int btsbot_knn_query(const float* queries, int64_t n_query, const float* bank, const void* packed, int64_t n_bank,
                     int dim, int k, int metric, int64_t self_offset, int splits, int64_t* idx, float* dist,
                     void* workspace, int64_t workspace_bytes, void* stream);
int64_t btsbot_knn_workspace_grouped(int64_t n_query, int64_t n_bank, int dim, int k, int splits, int flags);
int btsbot_knn_query_grouped(const float* queries, int64_t n_query, const float* bank, const void* packed,
                             int64_t n_bank, int dim, int k, int metric, int64_t self_offset, int splits, int64_t* idx,
                             float* dist, void* workspace, int64_t workspace_bytes, void* stream,
                             const int64_t* query_group, const int64_t* bank_group, int flags);

/* ---- everything within r: radius search over the same packed bank (csrc/knn_radius.hip) ---- */

/* Bank row b belongs to query row q's list if and only if b is eligible (finite, not the row self_offset masks, not of
 * q's group under BTSBOT_KNN_EXCLUDE_SAME) and the direct-form fp32 distance -- the function btsbot_knn_query applies to
 * the rows it returns -- is <= radius[q], compared in fp32.  Two tile passes over the grid of btsbot_knn_query's
 * selection (query tiles of 128 x splits) find the CANDIDATES, a superset: pairs whose GEMM-form value from the split
 * f16 products is within radius^2 plus a margin that covers the error bounds of both forms; a third
 * kernel computes every candidate's direct-form distance and marks the members.  Nothing of size n_query x n_bank is
 * written.  queries, bank, packed, dim, metric, self_offset, query_group / bank_group: as btsbot_knn_query_grouped;
 * flags: 0 or BTSBOT_KNN_EXCLUDE_SAME.  radius: fp32 [n_query] device memory, one per query row (a negative or NaN
 * radius admits nothing).  splits: 1..32, the same value in both calls.  workspace: btsbot_knn_radius_workspace(n_query,
 * dim) bytes, 16-byte aligned (the packed query rows; scratch afterwards).
 *
 * btsbot_knn_radius_count(): counts int32 [n_query][splits] = the candidates of each query row in each bank slice.
 * Two launches (query pack, count).  The caller forms offsets int64 [n_query * splits + 1], the exclusive scan of counts
 * with the total last, and reads the total n_cand to allocate.
 *
 * btsbot_knn_radius_fill(): the same walk with the same arithmetic writes the candidates' bank rows into cand int32
 * [n_cand] (query q's are cand[offsets[q * splits] .. offsets[(q + 1) * splits]), in no particular order inside a
 * slice), then dist fp32 [n_cand] = each candidate's direct-form distance and keep uint8 [n_cand] = dist <= radius[q].
 * The fill checks every slot against its region: a candidate past the end of its region is not written and sets
 * *error_flag (int32, device memory, zeroed by the caller) to 1 -- it cannot happen while counts and offsets are those
 * of the count call.  Three launches (query pack, fill, verify); n_cand == 0 launches nothing.
 * BTSBOT_ERR_INVALID_ARG with a message, before any HIP call, for the shapes btsbot_knn_query refuses, splits outside
 * 1..32, flags other than 0 / BTSBOT_KNN_EXCLUDE_SAME, a NULL pointer that is needed, a short or misaligned workspace. */
int64_t btsbot_knn_radius_workspace(int64_t n_query, int dim);
int btsbot_knn_radius_count(const float* queries, int64_t n_query, const void* packed, int64_t n_bank, int dim,
                            int metric, const float* radius, int64_t self_offset, int splits,
                            const int64_t* query_group, const int64_t* bank_group, int flags, int32_t* counts,
                            void* workspace, int64_t workspace_bytes, void* stream);
int btsbot_knn_radius_fill(const float* queries, int64_t n_query, const float* bank, const void* packed, int64_t n_bank,
                           int dim, int metric, const float* radius, int64_t self_offset, int splits,
                           const int64_t* query_group, const int64_t* bank_group, int flags, const int32_t* counts,
                           const int64_t* offsets, int64_t n_cand, int32_t* cand, float* dist, uint8_t* keep,
                           int32_t* error_flag, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- neighbour ranks: where does a given bank row stand in a query row's ordering (csrc/knn_rank.hip) ---- */

/* targets int64 [n_query][n_targets] (device memory, 1 <= n_targets <= 64) names bank rows.  For every (q, c):
 *   dist[q][c] = the direct-form fp32 distance of query row q and bank row targets[q][c] -- the bits btsbot_knn_query and
 *                btsbot_knn_radius_fill return for that pair; NaN where the target is < 0 or >= n_bank or either row
 *                holds a non-finite value;
 *   rank[q][c] = the number of bank rows b, eligible for q as in btsbot_knn_radius_* (finite, not the row self_offset
 *                masks, not of q's group under BTSBOT_KNN_EXCLUDE_SAME), whose (direct-form distance, b) is before
 *                (dist[q][c], targets[q][c]): distance first, then index, both sides fp32 direct form.  0-based; the
 *                target does not count against itself.  -1 where the target is out of range or not eligible for q, or
 *                query row q is not finite.
 * Hence rank[q][c] is the position of targets[q][c] in q's list of btsbot_knn_radius_* at radius dist[q][c], ordered by
 * (dist, index), bit for bit.  A (q, c) answer does not depend on the other rows or columns, on splits or on the run;
 * only integer additions meet across workgroups.  queries, bank, packed, dim, metric, self_offset, query_group /
 * bank_group: as btsbot_knn_query_grouped; flags: 0 or BTSBOT_KNN_EXCLUDE_SAME; splits: 1..32, the same in both calls.
 * workspace: btsbot_knn_rank_workspace(n_query, dim, n_targets) bytes, 16-byte aligned, the SAME memory in both calls and
 * untouched between them (the packed query rows and the thresholds of the count call).
 *
 * btsbot_knn_rank_count(): writes dist, initialises rank (int32 [n_query][n_targets]: 0, or -1) and adds to it the pairs
 * that are surely before -- whose GEMM-form value is below dist^2 less the two-sided margin of DESIGN.md 4r --;
 * counts int32 [n_query][splits] = the BAND pairs of each query row in each bank slice, those the margin cannot decide
 * for at least one column.  Three launches (query pack, thresholds, tile pass).  The caller forms offsets int64
 * [n_query * splits + 1], the exclusive scan of counts with the total last, and reads the total n_band to allocate.
 *
 * btsbot_knn_rank_fill(): the same walk writes each band pair as cand int32 [n_band] (the bank row) and cand_mask
 * uint64 [n_band] (bit c: the pair is in column c's band), every slot checked against its region (*error_flag, int32,
 * zeroed by the caller, is set to 1 otherwise -- it cannot happen while counts and offsets are the count call's); then
 * one wave per band pair computes the direct-form distance once and adds 1 to rank[q][c] for every masked column the
 * pair is before.  Two launches; n_band == 0 launches nothing and rank is final after the count call.
 * BTSBOT_ERR_INVALID_ARG with a message, before any HIP call, for the shapes btsbot_knn_query refuses (n_targets in k's
 * place), splits outside 1..32, flags other than 0 / BTSBOT_KNN_EXCLUDE_SAME (BTSBOT_KNN_ONE_PER_GROUP is not a rank
 * mode), a NULL pointer that is needed, a short or misaligned workspace. */
int64_t btsbot_knn_rank_workspace(int64_t n_query, int dim, int n_targets);
int btsbot_knn_rank_count(const float* queries, int64_t n_query, const float* bank, const void* packed, int64_t n_bank,
                          int dim, int metric, const int64_t* targets, int n_targets, int64_t self_offset, int splits,
                          const int64_t* query_group, const int64_t* bank_group, int flags, float* dist, int32_t* rank,
                          int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream);
int btsbot_knn_rank_fill(const float* queries, int64_t n_query, const float* bank, const void* packed, int64_t n_bank,
                         int dim, int metric, const int64_t* targets, int n_targets, int64_t self_offset, int splits,
                         const int64_t* query_group, const int64_t* bank_group, int flags, const float* dist,
                         int32_t* rank, const int32_t* counts, const int64_t* offsets, int64_t n_band, int32_t* cand,
                         uint64_t* cand_mask, int32_t* error_flag, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* ---- connected components of a CSR graph and the DBSCAN labelling rule (csrc/components.hip) ---- */

/* btsbot_graph_components(): indptr int64 [n + 1], indices int64 [indptr[n]] (values in [0, n)), mask uint8 [n] or
 * NULL (every row passes).  root int64 [n] = the smallest row index of the row's connected component in the graph
 * restricted to rows and edges whose both ends pass mask, an edge in either direction joining; -1 where mask is 0.
 * Lock-free union-find on parent int32 [n] (scratch, the caller's): the larger root is hooked under the smaller, so the
 * result is a function of the graph alone.  Three launches on `stream` (initialise, hook, flatten), no host read.
 *
 * btsbot_dbscan_labels(): core uint8 [n]; root as btsbot_graph_components(mask = core) returns it; cluster int64 [n] =
 * at a core row that is its own root the cluster's number (the others are not read).  labels int64 [n]: a core row
 * takes cluster[root[row]], a non-core row the smallest cluster[root[j]] over its core neighbours j, or -1 without one.
 * One launch.  Both: n < 2^31; BTSBOT_ERR_INVALID_ARG for a NULL pointer or n outside 0 .. 2^31 - 1. */
int btsbot_graph_components(const int64_t* indptr, const int64_t* indices, const uint8_t* mask, int64_t n,
                            int32_t* parent, int64_t* root, void* stream);
int btsbot_dbscan_labels(const int64_t* indptr, const int64_t* indices, const uint8_t* core, const int64_t* root,
                         const int64_t* cluster, int64_t n, int64_t* labels, void* stream);

/* ---- exact neighbour search on 2-D maps by a uniform grid (csrc/grid.hip) ---- */

/* The radius and k-nearest questions of btsbot_knn_radius_* / btsbot_knn_query for fp32 points in the plane, answered
 * in time linear in the points plus the output.  Membership, ranking and the returned distance are those of the tile
 * path at D = 2, bit for bit: a bank row is eligible if it is finite (both coordinates finite and
 * fl(fl(x x) + fl(y y)) <= FLT_MAX), is not row q + self_offset (self_offset >= 0) and, under BTSBOT_KNN_EXCLUDE_SAME,
 * is not of q's group (64 bits); the distance is sqrtf(fl(fl(t0 t0) + fl(t1 t1))), t = q - b, never contracted; a
 * member has distance <= radius[q] in fp32.  The grid only says which pairs are looked at, and provably looks at every
 * member, so no answer depends on `cells`.
 *
 * Build.  btsbot_grid_finite(): finite uint8 [n] by the rule above.  The caller reduces bbox fp32 [4] = {min x, min y,
 * max x, max y} over the finite rows (+inf / -inf without one), on the device.  btsbot_grid_cells(): writes geom fp32
 * [4] = {x0, y0, inv_hx, inv_hy} (inv_h = cells / extent, 0 for an extent that is not positive and finite) and cell
 * int32 [n] = cy * cells + cx with c(x) = clamp(floor(fl(fl(x - x0) * inv_h)), 0, cells - 1), or cells * cells for a
 * row that is not finite.  The caller sorts the rows by cell (stably) and hands every query call: cell_start int32
 * [cells * cells + 1] (cell_start[c] = the first sorted position whose cell is >= c), sorted_points fp32 [n_bank][2],
 * sorted_rows int32 [n_bank] (the points' original rows) and, for BTSBOT_KNN_EXCLUDE_SAME, sorted_group int64 [n_bank],
 * all in cell order.  1 <= cells <= 4096; n < 2^31.
 *
 * btsbot_grid_radius_count(): counts int64 [n_query] = the members of each query row; visited int64 [n_query] (may be
 * NULL) = the pairs whose distance was computed.  One launch, no host read.  A non-finite query row, or one whose
 * radius is negative or NaN, has none.  lanes: the lanes that share a query row, 0 (the library's choice, 16), 1, 4, 8,
 * 16, 32 or 64; the answer does not depend on it.
 * btsbot_grid_radius_fill(): indptr int64 [n_query + 1] = the exclusive scan of counts, total = indptr[n_query].  The
 * same walk writes query row q's members into cand int32 [total] (original rows) and dist fp32 [total] at indptr[q] ..,
 * in the order of the walk (the caller sorts).  A member past indptr[q + 1] is not written and sets *error_flag (int32,
 * device memory, zeroed by the caller) to 1 -- it cannot happen while indptr is the scan of the count call.
 * btsbot_grid_knn(): idx int64 [n_query][k], dist fp32 [n_query][k]: the k smallest eligible rows by (distance, row);
 * fewer than k eligible: the tail is -1 / +inf; a non-finite query row: -1 / NaN.  1 <= k <= 64.  One launch, no host
 * read, no workspace.
 * BTSBOT_ERR_INVALID_ARG with a message, before any HIP call, for sizes out of range, cells outside 1..4096, flags other
 * than 0 / BTSBOT_KNN_EXCLUDE_SAME, a group array the flag needs being NULL, lanes not listed above, k outside 1..64 and
 * a NULL pointer that is needed. */
int btsbot_grid_finite(const float* points, int64_t n, uint8_t* finite, void* stream);
int btsbot_grid_cells(const float* points, int64_t n, const float* bbox, int cells, float* geom, int32_t* cell,
                      void* stream);
int btsbot_grid_radius_count(const float* queries, int64_t n_query, const float* radius, const float* geom, int cells,
                             const int32_t* cell_start, const float* sorted_points, const int32_t* sorted_rows,
                             const int64_t* sorted_group, int64_t n_bank, int64_t self_offset,
                             const int64_t* query_group, int flags, int lanes, int64_t* counts, int64_t* visited,
                             void* stream);
int btsbot_grid_radius_fill(const float* queries, int64_t n_query, const float* radius, const float* geom, int cells,
                            const int32_t* cell_start, const float* sorted_points, const int32_t* sorted_rows,
                            const int64_t* sorted_group, int64_t n_bank, int64_t self_offset,
                            const int64_t* query_group, int flags, int lanes, const int64_t* indptr, int64_t total,
                            int32_t* cand, float* dist, int32_t* error_flag, void* stream);
int btsbot_grid_knn(const float* queries, int64_t n_query, int k, const float* geom, int cells,
                    const int32_t* cell_start, const float* sorted_points, const int32_t* sorted_rows,
                    const int64_t* sorted_group, int64_t n_bank, int64_t self_offset, const int64_t* query_group,
                    int flags, int64_t* idx, float* dist, void* stream);

/* ---- embedding layout: a deterministic UMAP map of the kNN graph (csrc/layout.hip) ---- */

/* Replaces: the UMAP layout of the embedding step (train.py:449-469, the umap_emb_1 / umap_emb_2 columns).  Everything
 * is queued on `stream`; nothing allocates, synchronises or copies to the host.  BTSBOT_ERR_INVALID_ARG for a NULL
 * pointer, k outside 2..64, 2 n k >= 2^31, a short or misaligned (256 bytes) workspace, an epoch range outside
 * 1 <= first <= last <= n_epochs, negative_sample_rate outside 0..64.
 *
 * btsbot_layout_smooth_knn(): idx int64 [n][k], dist fp32 [n][k] as btsbot_knn_query returns them with the row itself
 * in column 0 (knn_graph(..., include_self=True)); entries with idx < 0 are absent.  Writes rho [n] (the row's smallest
 * positive distance over columns 1.., or 0), sigma [n] (umap-learn's smooth_knn_dist bisection with local_connectivity
 * = bandwidth = 1: at most 64 trips towards sum_j exp(-max(d_j - rho, 0) / sigma) = log2 k, floored at 1e-3 times the
 * row's mean distance -- of *mean_all, a DEVICE double the caller sets to the mean of all present distances, where rho
 * is 0; searched in float64, rounded to fp32 once) and memb [n][k], the memberships a_ij = exp(-max(d - rho, 0) /
 * sigma), 0 in column 0 and for an absent, out-of-range or self entry.  One wave per row, one launch.
 *
 * btsbot_layout_symmetrize(): the symmetric CSR graph of those memberships, w_ij = (a_ij + a_ji) - a_ij a_ji in fp32
 * (a missing direction counts 0), bitwise equal in both slots of an edge.  indptr int64 [n + 1]; indices int32 and
 * weights fp32 hold 2 n (k - 1) slots of which the first indptr[n] are written, columns ascending inside a row; *w_max
 * (device) receives the largest weight.  A row must not name a neighbour twice.  workspace:
 * btsbot_layout_symmetrize_workspace(n, k) bytes.  Three kernels, one radix sort, one scan.
 *
 * btsbot_layout_init(): y fp32 [n][2].  mode 0: uniform in [-10, 10); mode 1: adds a jitter in +-1e-4 to what y holds.
 * Both from the counter hash of (seed, epoch 0, vertex, coordinate).
 *
 * btsbot_layout_epochs(): epochs first_epoch..last_epoch of an n_epochs schedule, one launch each.  The first epoch
 * reads y_a and writes y_b, the next reads y_b and writes y_a, ...: the result is in y_b after an odd number of epochs,
 * in y_a after an even one.  Epoch e: a slot with r = fp32(w / w_max) fires iff floor(e r) > floor((e - 1) r) (float64);
 * a firing slot (v, u) adds to v the attractive term 2 clip(-2ab d^(2(b-1)) / (1 + a d^(2b)) (y_v - y_u), +-4) and
 * negative_sample_rate repulsive terms clip(2b / ((0.001 + d^2)(1 + a d^(2b))) (y_v - y_t), +-4), t = the high word of
 * (hash >> 32) * n, hash = the splitmix64 counter hash of (seed, e, slot, sample); t == v or a non-finite y_t adds
 * nothing, d = 0 adds 0 (attractive) or +4 per coordinate (repulsive).  y_new = y_old + learning_rate (1 - (e - 1) /
 * n_epochs) * sum.  A vertex is written by its own eight lanes in an order fixed by its row: bit for bit reproducible,
 * whatever `blocks` (the grid; 0 = the library's choice). */
int btsbot_layout_smooth_knn(const int64_t* idx, const float* dist, int64_t n, int k, const double* mean_all,
                             float* sigma, float* rho, float* memb, void* stream);
int64_t btsbot_layout_symmetrize_workspace(int64_t n, int k);
int btsbot_layout_symmetrize(const int64_t* idx, const float* memb, int64_t n, int k, int64_t* indptr, int32_t* indices,
                             float* weights, float* w_max, void* workspace, int64_t workspace_bytes, void* stream);
int btsbot_layout_init(float* y, int64_t n, uint64_t seed, int mode, void* stream);
int btsbot_layout_epochs(const int64_t* indptr, const int32_t* indices, const float* weights, const float* w_max,
                         int64_t n, float* y_a, float* y_b, int n_epochs, int first_epoch, int last_epoch, float a,
                         float b, uint64_t seed, int negative_sample_rate, float learning_rate, int blocks,
                         void* stream);

/* ---- new rows on an existing map: umap-learn's transform (csrc/layout.hip) ---- */

/* Both are queued on `stream`; nothing allocates, synchronises or copies to the host.  A row's result is a function of
 * that row of idx / dist (and of the bank's positions) alone: it does not depend, bit for bit, on the other rows of the
 * call, on `blocks` or on the run.  BTSBOT_ERR_INVALID_ARG for a NULL pointer, k outside 2..64, 2 q k >= 2^31, an epoch
 * range outside 1 <= first <= last <= n_epochs, first > 1 without y0, negative_sample_rate outside 0..64, an empty bank.
 * q = 0 succeeds without a launch.
 *
 * btsbot_layout_smooth_knn_query(): idx int64 [q][k], dist fp32 [q][k] as btsbot_knn_query returns them for rows that
 * are NOT in the bank: there is no self column, every entry with idx >= 0 is a neighbour.  Writes sigma [q] (the
 * bisection of btsbot_layout_smooth_knn with rho = 0, floored at 1e-3 times the mean of the row's own present
 * distances; float64, rounded to fp32 once) and w [q][k] = exp(-d / sigma) (1 at d = 0, 0 where idx < 0).
 *
 * btsbot_layout_transform(): epochs first_epoch..last_epoch of an n_epochs schedule for q new points against the FIXED
 * positions bank_y fp32 [n_bank][2], in ONE launch; yout fp32 [q][2].  y0 (fp32 [q][2], may be yout) holds the positions
 * the first epoch starts from; y0 = NULL (first_epoch = 1 only): the start is sum_j w_j Y[idx_j] / sum_j w_j (float64 in
 * slot order, rounded once; NaN where no slot is present), from a launch of its own, and first_epoch = 1, last_epoch = 0
 * then returns that start alone.  Epoch e: slot j with r = fp32(w_j / max_j w_j) fires iff floor(e r) > floor((e - 1) r)
 * (float64) and adds clip(-2ab d^(2(b-1)) / (1 + a d^(2b)) (y - Y[idx_j]), +-4) -- no factor 2: the bank does not move
 * -- and negative_sample_rate terms clip(2b / ((0.001 + d^2)(1 + a d^(2b))) (y - Y_t), +-4), t = the high word of
 * (hash >> 32) * n_bank, hash = mix64(mix64(seed ^ mix64(e)) + rowkey + 64 j + s), rowkey = the fold key <- mix64(key +
 * ((uint32(idx_j) << 32) | bits(w_j))) over the row's slots from key = 0; a non-finite Y_t adds nothing.  y <- fma(alpha_e,
 * sum, y), alpha_e = fp32(learning_rate / 4 (1 - (e - 1) / n_epochs)).  idx entries outside 0..n_bank-1 are absent. */
int btsbot_layout_smooth_knn_query(const int64_t* idx, const float* dist, int64_t q, int k, float* sigma, float* w,
                                   void* stream);
int btsbot_layout_transform(const int64_t* idx, const float* w, const float* bank_y, int64_t n_bank, int64_t q, int k,
                            const float* y0, float* yout, int n_epochs, int first_epoch, int last_epoch, float a, float b,
                            uint64_t seed, int negative_sample_rate, float learning_rate, int blocks, void* stream);

/* ---- local outlier factor on a kNN graph: novelty scores (csrc/lof.hip) ---- */

/* Both are queued on `stream`; nothing allocates, synchronises or copies to the host.  An entry (row, c) is PRESENT when
 * 0 <= idx[row][c] < n; a -1 tail is no entry and an index out of range is treated the same.  m(row) is the number of
 * present entries.  All arithmetic is float64 on the fp32 distances converted once:
 *   kdist(i)    = dist of row i's last present column                                      NaN when m = 0
 *   reach(i, c) = fmax(dist[i][c], kdist(idx[i][c]))       (a NaN kdist leaves dist)
 *   lrd(i)      = 1 / (sum_c reach(i, c) / m + 1e-10)      (scikit-learn's constant)       NaN when m = 0
 *   lof(i)      = (sum_c lrd(idx[i][c]) / lrd(i)) / m      (each quotient formed first)    NaN when m = 0
 * A sum runs over W slots, W = 16, 32 or 64 the smallest that holds k: slot c holds column c's term where the entry is
 * present and +0.0 otherwise, then for o = W/2, ..., 1 every slot c takes v[c] + v[c ^ o]; the sum is slot 0.  The order
 * depends on the row's own columns and k alone, so a row's result does not depend, bit for bit, on the other rows of the
 * call, on the grid or on the run.  No fused multiply-add, IEEE divisions.
 *
 * btsbot_lof_fit(): idx int64 [n][k], dist fp32 [n][k] as btsbot_knn_query returns them for every bank row among the
 * OTHERS (self_offset = 0; knn_graph(..., include_self=False)).  Writes kdist, lrd and lof, float64 [n] each; lof may be
 * NULL (two launches instead of three).
 *
 * btsbot_lof_score(): idx / dist [q][k] of NEW rows against a fitted bank of n rows (no self column), bank_kdist and
 * bank_lrd float64 [n] as btsbot_lof_fit wrote them.  The two formulas with kdist and lrd of the neighbours read from
 * the bank's arrays (the new row has no kdist of its own); writes lof and, unless NULL, lrd, float64 [q] each.  One
 * launch.
 *
 * BTSBOT_ERR_INVALID_ARG with a message, before any HIP call, for k outside 1..64, n or q outside 0..2^31 - 1, a NULL
 * pointer (but the optional output; the bank's arrays where n = 0) or a misaligned one.  btsbot_lof_fit with n = 0 and
 * btsbot_lof_score with q = 0 succeed without a launch; btsbot_lof_score with n = 0 writes NaN. */
int btsbot_lof_fit(const int64_t* idx, const float* dist, int64_t n, int k, double* kdist, double* lrd, double* lof,
                   void* stream);
int btsbot_lof_score(const int64_t* idx, const float* dist, int64_t q, int k, const double* bank_kdist,
                     const double* bank_lrd, int64_t n, double* lrd, double* lof, void* stream);

/* ---- a kNN graph kept current under add and remove: the merge of offers into the lists and their compaction
 *      (csrc/knn_graph.hip) ---- */

/* Flags of btsbot_knn_graph_merge. */
enum btsbot_knn_graph_flags { BTSBOT_KNN_GRAPH_DISTINCT = 1 };

/* Merges, in place, offers into the neighbour lists of n_old rows.  idx int64 / dist fp32 hold row a's list at
 * [a * stride .. a * stride + k): present entries (idx >= 0) first, ordered by (dist, idx), then a -1 / +inf tail -- the
 * lists btsbot_knn_query writes.  The offers are a CSR: indptr int64 [n_old + 1] (n_offers = indptr[n_old]), offer_idx
 * int64 and offer_dist fp32 [n_offers], a row's offers ordered by (dist, idx); every offer index must be larger than
 * every index of the lists (new rows: an old entry wins a tie in dist) and not occur in them.  Row a's list becomes the
 * first k of the merge by (dist, idx) of its present entries and its offers, the tail -1 / +inf.  Under
 * BTSBOT_KNN_GRAPH_DISTINCT (k <= 32) an entry is emitted only if its group -- groups int64 [n_groups], read at the
 * entry's index, all 64 bits -- differs from every entry emitted before it.  A list of a row whose dist[0] is NaN (a
 * non-finite row) and a row whose indptr range is empty or does not lie inside [0, n_offers] is left as it is.
 *
 * rows: NULL, every row a in [0, n_old) is visited, one wave each, and a row without offers ends after its two indptr
 * reads; or int64 [n_rows], the rows to visit (distinct, in [0, n_old); others are skipped).  changed_rows: NULL or uint8
 * [n_old], set to 1 for every row whose list changed (never cleared here); changed_count: NULL or one int32 the number of
 * changed rows is ADDED to.  The merge itself uses no atomic: a row is read whole by its wave before it is written, and
 * its result is a function of its own list and offers.  Work per row: k + the offers that can matter (the first k in the
 * plain mode; in the distinct mode the walk ends at k emitted groups).  Queued on `stream`; nothing allocates,
 * synchronises or copies to the host.
 *
 * BTSBOT_ERR_INVALID_ARG with a message, before any HIP call, for k outside 1..64 (1..32 under DISTINCT), stride < k,
 * n_old, n_rows or n_offers outside 0..2^31 - 1, unknown flags, DISTINCT without groups, a NULL or misaligned pointer
 * (but the optional ones).  n_old = 0, n_offers = 0 or rows given with n_rows = 0 succeed without a launch. */
int btsbot_knn_graph_merge(int64_t* idx, float* dist, int64_t stride, int k, int64_t n_old, const int64_t* indptr,
                           const int64_t* offer_idx, const float* offer_dist, int64_t n_offers, const int64_t* groups,
                           int64_t n_groups, int flags, const int64_t* rows, int64_t n_rows, uint8_t* changed_rows,
                           int32_t* changed_count, void* stream);

/* Compacts the neighbour lists of n_old rows after rows were removed, out of place.  idx / dist: the lists
 * as above, row a at [a * stride .. a * stride + k).  new_of_old int64 [n_old]: the row's new number, -1 (any negative)
 * for a removed row; ascending over the survivors and < n_new.  An old row a with j = new_of_old[a] in [0, n_new) has its
 * list written to out_idx / out_dist at [j * out_stride .. j * out_stride + k): its present entries whose row survived,
 * renumbered through new_of_old, in their order (new_of_old is monotone, so (dist, index) order is kept), with the dist
 * bits they had, then a -1 / +inf tail.  An entry outside [0, n_old) is never a subscript: it is dropped and counts as
 * removed.  A row whose dist[0] is NaN (a non-finite row) is copied as it stands.  damaged uint8 [n_new] is written for
 * every surviving row: 1 iff at least one present entry was dropped and either the list was full (idx[k - 1] >= 0) or
 * BTSBOT_KNN_GRAPH_DISTINCT is set -- the rows whose list has to be searched again; a list with a free slot held every
 * eligible row, so what is left of it is complete (not so under DISTINCT, where a further row of a dropped entry's group
 * may surface); 0 for a NaN row.  counts: NULL, or int32 [2] to which the damaged rows and the entries dropped (of all
 * surviving rows but the NaN ones) are ADDED, at most two atomics per wave.
 *
 * One launch.  W lanes hold a row, lane c its column c, W = 16, 32 or 64 the smallest that holds k; the row is read whole
 * before anything is written, one ballot gives every surviving entry its new column, no atomic touches a list, and the
 * lanes of a removed row leave after their one read of new_of_old.  Rows of the output that no survivor maps to are not
 * written.  Queued on `stream`; nothing allocates, synchronises or copies to the host.
 *
 * BTSBOT_ERR_INVALID_ARG with a message, before any HIP call, for flags other than 0 / BTSBOT_KNN_GRAPH_DISTINCT, k
 * outside 1..64 (1..32 under DISTINCT), stride < k or out_stride < k, n_old or n_new outside 0..2^31 - 1, n_new > n_old, a
 * NULL or misaligned pointer (but counts), and an output array that overlaps an input array.  n_old = 0 or n_new = 0
 * succeed without a launch. */
int btsbot_knn_graph_compact(const int64_t* idx, const float* dist, int64_t stride, int k, int64_t n_old,
                             const int64_t* new_of_old, int64_t* out_idx, float* out_dist, int64_t out_stride,
                             int64_t n_new, int flags, uint8_t* damaged, int32_t* counts, void* stream);

/* ---- The partitioned index: k-means on the device and a probed nearest-row search (csrc/ivf.hip) ----
 *
 * The rows of a bank are cut into lists around centroids; a query searches only the lists it is told to probe.  The
 * answer of btsbot_ivf_query() is exactly btsbot_knn_query()'s (euclidean) over the finite rows of the probed lists:
 * the same selection scores, the same merge by (score, row), the same direct-form fp32 distance, ordered by (dist,
 * ORIGINAL row number).  Which lists are probed is the caller's (btsbot_knn_query() of the queries against the
 * centroids); it is the only approximation.  All pointers are device memory; n_clusters / n_lists in 1 .. 65,536.
 *
 * btsbot_kmeans_update(): centroids[c] = the mean of the rows with labels[row] == c, for every cluster with at least one
 * row; an empty cluster's centroid is not written.  counts int64 [n_clusters] receives every cluster's size.  labels
 * int64 [n_rows] in -1 .. n_clusters - 1 (negative: the row enters no sum); order int64 [n_rows] = the row numbers
 * sorted stably by label (rows of equal label ascending; any stable sort).  Deterministic, no atomic on a sum: the rows
 * of a cluster, in ascending row order, are cut into chunks of 64 counted from the cluster's first row, pass 1 adds a
 * chunk's rows one after the other per column, pass 2 adds the cluster's partial sums in chunk order and divides by
 * the count.  A centroid's bits depend on its cluster's rows alone -- not on the grid, the run or the other clusters.
 * One read of the fp32 rows.  workspace: btsbot_kmeans_workspace() bytes, 16-byte aligned; four launches and a memset.
 *
 * btsbot_ivf_layout(): the list-ordered operand image.  packed: the bank's records (btsbot_knn_pack_bank, euclidean);
 * labels / order as above (a row of negative label is in no list).  list_packed receives n_list_rows =
 * btsbot_ivf_list_rows(n_bank, n_lists) records, an upper bound that needs no host read: every list starts on a 128-row
 * boundary, its rows in ascending row number, padded with the record of a non-finite row (never a candidate).
 * row_of int32 [n_list_rows]: the bank row at a position, -1 for padding; pos_of int32 [n_bank]: a row's position, -1 for
 * a row in no list; list_sizes int64 [n_lists]; list_tile int32 [n_lists + 1]: list l holds the 128-row tiles
 * list_tile[l] .. list_tile[l + 1].  workspace: 2 * align256(4 * (n_lists + 1)) bytes.
 *
 * btsbot_ivf_query(): idx int64 [n_query][k] (original row numbers), dist fp32 [n_query][k].  probes int64
 * [n_query][nprobe], 1 <= nprobe <= min(n_lists, 32), distinct per row; a value outside 0 .. n_lists - 1 contributes
 * nothing.  self_rows: NULL, or int64 [n_query]: query row i IS bank row self_rows[i] and that one row is not a
 * candidate (by position: duplicates are).  Fewer than k rows in the probed lists: the tail is idx = -1, dist = +inf; a
 * non-finite query row: -1 / NaN.  One work item is one list and at most 128 of the queries that probe it; the items
 * are built on the device and the grid is the upper bound ceil(n_query * nprobe / 128) + n_lists: no host read.  A
 * row's answer is bit for bit independent of the other rows of the call and of the run.  workspace:
 * btsbot_ivf_workspace() bytes -- the packed image of the query rows, n_query * nprobe * k candidates of 8 bytes, 4
 * bytes per (query, probe) pair and 12 per list --, 16-byte aligned.  Seven launches and two memsets on `stream`.
 * BTSBOT_ERR_INVALID_ARG with a message, before any HIP call, for a shape out of range, n_query * nprobe >= 2^31, a
 * NULL or misaligned pointer, a workspace too small.
 *
 * Groups: btsbot_ivf_query_grouped() is btsbot_ivf_query() with the two switches of btsbot_knn_query_grouped() and the
 * same contract over the rows of the probed lists.  flags: BTSBOT_KNN_EXCLUDE_SAME, BTSBOT_KNN_ONE_PER_GROUP, both, or 0
 * (btsbot_ivf_query() itself: the groups are not read).  query_group int64 [n_query] (needed by EXCLUDE_SAME);
 * list_group int64 [n_list_rows]: the rows' groups in LIST order, made by btsbot_ivf_layout_groups(bank_group int64
 * [n_bank], ..., row_of, n_list_rows, list_group) after btsbot_ivf_layout() -- list_group[p] = bank_group[row_of[p]], 0
 * at a padding position (never a candidate); one launch.  EXCLUDE_SAME: no row of the query row's own group is a
 * candidate.  ONE_PER_GROUP (k <= 32): the k nearest groups among the eligible rows of the probed lists, each by its
 * best row by (score, original row) -- a group whose rows lie in several probed lists is met in the merge and returned
 * once.  self_rows stays a compare of positions and combines with every mode.  Distances, ordering, tails and the
 * independence of a row's answer from the call and the run are btsbot_ivf_query()'s; with every list probed the answer
 * is btsbot_knn_query_grouped()'s, bit for bit.  workspace: btsbot_ivf_workspace_grouped() bytes, which under
 * ONE_PER_GROUP adds the groups of the list entries, int64 [k][n_query * nprobe] (8 k bytes per pair; no n_lists term
 * and no host read).  BTSBOT_ERR_INVALID_ARG with a message for flags with other bits, k > 32 under ONE_PER_GROUP, and
 * a NULL query_group / list_group where the flags need them. */
int64_t btsbot_kmeans_workspace(int64_t n_rows, int dim, int n_clusters);
int btsbot_kmeans_update(const float* rows, int64_t n_rows, int dim, const int64_t* labels, const int64_t* order,
                         int n_clusters, float* centroids, int64_t* counts, void* workspace, int64_t workspace_bytes,
                         void* stream);
int64_t btsbot_ivf_list_rows(int64_t n_bank, int n_lists);
int btsbot_ivf_layout(const void* packed, int64_t n_bank, int dim, const int64_t* labels, const int64_t* order,
                      int n_lists, void* list_packed, int64_t n_list_rows, int32_t* row_of, int32_t* pos_of,
                      int64_t* list_sizes, int32_t* list_tile, void* workspace, int64_t workspace_bytes, void* stream);
int64_t btsbot_ivf_workspace(int64_t n_query, int dim, int k, int nprobe, int n_lists);
int btsbot_ivf_query(const float* queries, int64_t n_query, const float* bank, int64_t n_bank, int dim, int k,
                     const int64_t* probes, int nprobe, const int64_t* self_rows, const void* list_packed,
                     int64_t n_list_rows, const int32_t* row_of, const int32_t* pos_of, const int32_t* list_tile,
                     int n_lists, int64_t* idx, float* dist, void* workspace, int64_t workspace_bytes, void* stream);
int btsbot_ivf_layout_groups(const int64_t* bank_group, int64_t n_bank, int n_lists, const int32_t* row_of,
                             int64_t n_list_rows, int64_t* list_group, void* stream);
int64_t btsbot_ivf_workspace_grouped(int64_t n_query, int dim, int k, int nprobe, int n_lists, int flags);
int btsbot_ivf_query_grouped(const float* queries, int64_t n_query, const float* bank, int64_t n_bank, int dim, int k,
                             const int64_t* probes, int nprobe, const int64_t* self_rows, const void* list_packed,
                             int64_t n_list_rows, const int32_t* row_of, const int32_t* pos_of,
                             const int32_t* list_tile, int n_lists, int64_t* idx, float* dist, void* workspace,
                             int64_t workspace_bytes, void* stream, const int64_t* query_group,
                             const int64_t* list_group, int flags);

/* ---- HDBSCAN: the mutual-reachability spanning tree and its hierarchy (csrc/mr_offer.hip, csrc/mst.hip,
 *      csrc/hdbscan_tree.hip) ---- */

/* The minimum spanning tree of the complete graph on the finite rows under w(a, b) = max(d(a, b), core(a), core(b), 0) in
 * fp32, by Boruvka rounds.  A round's searches are btsbot_knn_query_grouped / btsbot_grid_knn and btsbot_knn_radius_* /
 * btsbot_grid_radius_* with comp int64 [n] -- the row's current component, its smallest row -- as the group of both sides
 * under BTSBOT_KNN_EXCLUDE_SAME; these three calls stand between them.  All are queued on `stream`; nothing allocates,
 * synchronises or copies to the host.
 *
 * btsbot_mst_offer_knn(): idx int64 [n][k], dist fp32 [n][k]: every row's k nearest rows of other components, ordered by
 * distance; core fp32 [n].  best_w fp32 [n], best_j int32 [n]: the row's lightest entry by (w, index); -1 / +inf where the
 * list is empty (a non-finite row; the last component).  unresolved uint8 [n] = 0 where the list proves the offer the
 * lightest edge that leaves the row: the list is not full, or best_w <= max(floor, core(row)), floor = (1 - rel) *
 * (slack_is_squared ? sqrt(max(d_last^2 - slack[row], 0)) : d_last - slack[row]) in float64, a lower bound of the distance
 * of every row the list does not hold (slack fp32 [n] or NULL = 0; a search that ranks by the returned distance itself
 * passes NULL and rel = 0).  1 where it does not: every lighter edge then lies within the radius best_w.  1 <= k <= 64,
 * 0 <= rel < 1.  One launch, W = 16, 32 or 64 lanes per row.
 *
 * btsbot_mst_offer_csr(): indptr int64 [m + 1], indices int64, dist fp32: the radius lists (rows of other components
 * within best_w) of the m rows `rows` int64 [m]; lowers (best_w, best_j) of these rows to the lightest entry by (w, index).
 * One launch, one wave per row.
 *
 * btsbot_mst_merge(): every component (comp[i], in [0, n)) takes the lightest offer of its rows -- atomicMin on the
 * weight's bits into comp_w uint32 [n], then on (lo << 32 | hi) among the rows at that weight into comp_edge uint64 [n],
 * both scratch --, its edge is united lock-free on parent int32 [n] (parent[i] = comp[i] on entry, a root is hooked under
 * the smaller root); an edge that joins two trees is appended at (*cursor)++ to edges int64 [edge_capacity][2] (lo, hi)
 * and weights fp32 [edge_capacity], an edge whose ends are joined already is dropped; then comp and parent are relabelled
 * to the roots.  *cursor (int32, device memory, zero before the first round) counts the edges of all rounds: the
 * components left are the finite rows less *cursor.  Which of several equally light edges a component takes may differ
 * between runs; the sorted weights may not.  Six launches.
 * All three: BTSBOT_ERR_INVALID_ARG for n or m outside 0 .. 2^31 - 1, k or rel out of range, a NULL pointer that is
 * needed; n == 0 launches nothing. */
int btsbot_mst_offer_knn(const int64_t* idx, const float* dist, int64_t n, int k, const float* core, const float* slack,
                         int slack_is_squared, float rel, float* best_w, int32_t* best_j, uint8_t* unresolved,
                         void* stream);
int btsbot_mst_offer_csr(const int64_t* indptr, const int64_t* indices, const float* dist, const int64_t* rows, int64_t m,
                         int64_t n, const float* core, float* best_w, int32_t* best_j, void* stream);
int btsbot_mst_merge(const float* best_w, const int32_t* best_j, int64_t n, int64_t* comp, int32_t* parent,
                     uint32_t* comp_w, uint64_t* comp_edge, int64_t* edges, float* weights, int64_t edge_capacity,
                     int32_t* cursor, void* stream);

/* btsbot_hdbscan_tree(): HOST arrays in, host arrays out; no stream, no GPU call -- it runs on a machine without one.
 * edges int64 [n_edges][2] and weights fp32 [n_edges] (>= 0, +inf allowed): a spanning tree of the rows it names, rows in
 * [0, n); a row no edge names is noise.  The hierarchy is tie-invariant: all edges of one weight are applied at once and
 * every set of old components they join becomes one node with two or more children, so the answer is a function of the
 * components of "edges with w <= t" for every t -- the same for every edge order and every minimum spanning tree.
 * lambda = 1 / w in float64 (w = 0: the largest lambda of a positive weight of the tree, 1 without one).  Condensed tree,
 * top-down: at a node of cluster c a child of size >= min_cluster_size is real; two or more real children start new
 * clusters born at the node's lambda, exactly one continues c, the rows of the others fall out of c there.  Clusters
 * are numbered n, n + 1, ... by (smallest row, size descending); the entries (parent cluster, child row or cluster,
 * lambda, size) are sorted by (parent, child).  stability(c) = (sum over its rows of lambda - birth(c)) + (sum over its
 * child clusters of size * (lambda - birth(c))), float64, each sum sequential in entry order.  BTSBOT_HDBSCAN_EOM: bottom-up,
 * the children replace c only if their summed selected stability is strictly greater; BTSBOT_HDBSCAN_LEAF: the clusters
 * without child clusters; the root only with allow_single_cluster.  labels int64 [n]: the nearest selected
 * ancestor-or-self of the cluster the row fell out of, numbered 0, 1, ... by smallest row, or -1; prob float64 [n] =
 * min(lambda_row, m) / m with m the largest lambda of the selected cluster's own entries (1 where m = 0; 0 for noise).
 * The condensed arrays may all be NULL; *n_cond receives the number of entries (at most 2 n).
 * BTSBOT_ERR_INVALID_ARG for n >= 2^30, n_edges >= n, min_cluster_size < 2, an unknown method, an edge out of range or a
 * self-loop, a negative or NaN weight, edges that are no spanning tree of their rows, a short condensed capacity. */
enum btsbot_hdbscan_method { BTSBOT_HDBSCAN_EOM = 0, BTSBOT_HDBSCAN_LEAF = 1 };
int btsbot_hdbscan_tree(const int64_t* edges, const float* weights, int64_t n_edges, int64_t n, int min_cluster_size,
                        int method, int allow_single_cluster, int64_t* labels, double* prob, int64_t* cond_parent,
                        int64_t* cond_child, double* cond_lambda, int64_t* cond_size, int64_t cond_capacity,
                        int64_t* n_cond);

/* ---- HDBSCAN for new rows: the tables of a fitted tree and the prediction (csrc/hdbscan_tree.hip,
 *      csrc/mr_offer.hip, csrc/hdbscan_predict.hip) ---- */

/* btsbot_hdbscan_model(): the same pass as btsbot_hdbscan_tree() on the same inputs (HOST arrays, no GPU call, the same
 * errors), handing out the tables a prediction walks.  Clusters are in the canonical numbering less n: ids 0 ..
 * *n_clusters - 1, cluster c is condensed id n + c, the root is 0, a parent stands before its children.
 * Per row [n]: row_cluster int32, the cluster the row fell out of (-1: a row without an entry); row_lambda float64, the
 * lambda it fell out at (0 without an entry); outlier float64, the GLOSH score 1 - row_lambda / death[row_cluster] (0 where
 * that death is 0, NaN for a row without an entry).  Per cluster [cluster_capacity >= *n_clusters; max(n - 1, 1) always
 * suffices]: parent int32 (-1: the root); birth float64; label int32, the label of the nearest selected ancestor-or-self
 * (-1 without one); max_lambda float64, the largest lambda of that selected cluster's own entries (0 where label is -1):
 * labels[r] = label[row_cluster[r]] and prob[r] = min(row_lambda[r], m) / m with m = max_lambda[row_cluster[r]] (1 where
 * m = 0, 0 where the label is -1) are btsbot_hdbscan_tree()'s, bit for bit; death float64, the largest lambda of any entry
 * in the cluster's subtree.  *lam_zero: the lambda that stands for w = 0 (1 without a positive weight). */
int btsbot_hdbscan_model(const int64_t* edges, const float* weights, int64_t n_edges, int64_t n, int min_cluster_size,
                         int method, int allow_single_cluster, int32_t* row_cluster, double* row_lambda, double* outlier,
                         int32_t* parent, double* birth, int32_t* label, double* max_lambda, double* death,
                         int64_t cluster_capacity, int64_t* n_clusters, double* lam_zero);

/* The cluster of NEW rows against a fitted tree, after idx int64 [n_query][k], dist fp32 [n_query][k] =
 * btsbot_knn_query*() / btsbot_grid_knn() of the rows against the bank with k >= max(min_samples - 1, 1).  core fp32 [n]:
 * the bank's core distances (btsbot_mst_*'s).  All three are queued on `stream`; nothing allocates, synchronises or copies
 * to the host.
 *
 * btsbot_cluster_offer_knn(): core_q fp32 [n_query]: the row's own core distance, column min_samples - 2 of its list (0 for
 * min_samples = 1, +inf where that column is absent, NaN for a non-finite row: dist NaN throughout).  best_w fp32, best_j
 * int32 [n_query]: the entry with the smallest (w, index), w = max(dist, core_q, core[index], 0) in fp32; -1 / +inf where
 * the list is empty or core_q is +inf, -1 / NaN for a non-finite row.  unresolved uint8 [n_query] = 0 where the list proves
 * that no bank row has a smaller (w, index): the list is not full, or best_w < floor -- STRICTLY; a row the list does not
 * hold may tie a weight at a smaller index, and two rows of one weight can lie in different clusters --, floor as in
 * btsbot_mst_offer_knn() with slack fp32 [n_query] per QUERY row.  1 where it does not: every row with a smaller (w,
 * index) then lies within the radius best_w.  One launch, W = 16, 32 or 64 lanes per row.
 *
 * btsbot_cluster_offer_csr(): indptr int64 [m + 1], indices int64, dist fp32: the radius lists (bank rows within best_w)
 * of the m query rows `rows` int64 [m]; lowers (best_w, best_j) of these rows to the smallest (w, index).  One launch,
 * one wave per row.
 *
 * btsbot_cluster_assign(): with b = best_j and lambda = 1 / (double) best_w (lam_zero at 0): c = row_cluster[b]; if
 * row_lambda[b] > lambda, while parent[c] >= 0 and birth[c] >= lambda: c = parent[c].  out_label int64 = label[c];
 * out_prob float64 = min(lambda, max_lambda[c]) / max_lambda[c] (1 where that is 0, 0 where the label is -1);
 * out_outlier float64 = 1 - min(lambda, death[c]) / death[c] (0 where death[c] is 0); out_lambda float64; out_cluster
 * int64 = c; out_neighbor int64 = b.  A row without a neighbour: -1, 0, 1, 0, -1, -1; a non-finite row: -1, 0, NaN, NaN,
 * -1, -1.  Each operation is one correctly rounded IEEE operation, none contracted.  The tables are
 * btsbot_hdbscan_model()'s, in device memory.  One launch, one lane per row.
 * All three: BTSBOT_ERR_INVALID_ARG for a size outside 0 .. 2^31 - 1, k outside 1..64, min_samples outside 1..k + 1, rel
 * outside [0, 1), lam_zero <= 0, a NULL pointer that is needed; n_query == 0 launches nothing. */
int btsbot_cluster_offer_knn(const int64_t* idx, const float* dist, int64_t n_query, int k, int64_t n, int min_samples,
                             const float* core, const float* slack, int slack_is_squared, float rel, float* core_q,
                             float* best_w, int32_t* best_j, uint8_t* unresolved, void* stream);
int btsbot_cluster_offer_csr(const int64_t* indptr, const int64_t* indices, const float* dist, const int64_t* rows,
                             int64_t m, int64_t n_query, int64_t n, const float* core, const float* core_q, float* best_w,
                             int32_t* best_j, void* stream);
int btsbot_cluster_assign(const float* best_w, const int32_t* best_j, int64_t n_query, int64_t n,
                          const int32_t* row_cluster, const double* row_lambda, int64_t n_clusters, const int32_t* parent,
                          const double* birth, const int32_t* label, const double* max_lambda, const double* death,
                          double lam_zero, int64_t* out_label, double* out_prob, double* out_outlier, double* out_lambda,
                          int64_t* out_cluster, int64_t* out_neighbor, void* stream);

/* Replaces: the epoch / validation metrics of val.py:159-168 and train.py:550-558 -- out2[0] += sum_i of
 * BCEWithLogitsLoss(pos_weight) terms over n logits, out2[1] += number of alerts whose sigmoid(z) > 0.5
 * agrees with the label (caller zeroes out2 and divides by n). */
int btsbot_eval_metrics(const float* logits, const float* labels, float pos_weight, int64_t n,
                        float* out2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BTSBOT_HIP_H */
