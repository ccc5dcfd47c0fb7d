// Internal: every BTSBOT_AMD_* variable the library reads, declared once, and the kernel schedule a handle resolves
// from them (schedule.hip).  Host only.
#pragma once

// X(enumerator, kind, scope, meaning): the variable is BTSBOT_AMD_<enumerator>.
//   kind   ON  on when set and its value starts with '1'            -> switch_on()
//          INT atoi(value), the caller's default when it is not set  -> switch_int() (each reader keeps its range check)
//   scope  HANDLE   read at every btsbot_create(): setting it in-process before a model is built works
//          PROCESS  read once, at its first use
#define BTSBOT_SWITCHES(X)                                                                                              \
  X(NO_STAGE0, ON, HANDLE, "stem + stage 0 + first downsample launch by launch instead of stage0b_kernel")              \
  X(NO_STAGE1, ON, HANDLE, "stage 1 + second downsample launch by launch instead of stage1b_kernel")                    \
  X(NO_STAGE2, ON, HANDLE, "stage 2 + last downsample launch by launch instead of stage2p_kernel")                      \
  X(NO_S3, ON, HANDLE, "the 1x1 stage as dwconv_ln + generic GEMMs instead of stage3.hip")                              \
  X(NO_HEAD16, ON, HANDLE, "the fp32 VALU head (head.hip) in the 16-bit modes too")                                     \
  X(NO_STEM16, ON, HANDLE, "the fp32 VALU stem in the 16-bit modes too")                                                \
  X(NO_FUSED_MLP, ON, HANDLE, "every block MLP as two GEMMs (inference and training)")                                  \
  X(X2_TAIL_F16, ON, HANDLE, "f16x2 handles: stages 2-3 on plain f16 operands (which stage owns the mode's error?)")    \
  X(S0_DIAG, INT, HANDLE, "Stage0Args::diag / Stage1Args::diag of the inference launches")                              \
  X(S2P_DIAG, INT, HANDLE, "Stage2pArgs::diag of the inference launch")                                                 \
  X(HEAD_DIAG, INT, HANDLE, "HeadArgs::diag of the fp32 head (tools/head_diag.py)")                                     \
  X(NO_S0_TRAIN, ON, HANDLE, "training forward of stem + stage 0 launch by launch, not stage0b_kernel's keeping form")  \
  X(S1_TRAIN, ON, HANDLE, "bf16: stage 1's training forward as stage1b_kernel's keeping form (default in f16 only: "    \
                          "in bf16 it is worth 45 us of 2.6 ms but uses up to 1.02 of the 50-step trajectory band)")    \
  X(NO_S1_TRAIN, ON, HANDLE, "stage 1's training forward launch by launch in every mode")                               \
  X(NO_S2P_TRAIN, ON, HANDLE, "stage 2's training forward launch by launch, not stage2p_kernel's keeping form")         \
  X(NO_MLP_BWD, ON, HANDLE, "no block runs the fused MLP forward + mlp_bwd_kernel in the training step")                \
  X(MLP_BWD_C, INT, HANDLE, "64 / 128: only blocks of that width run it")                                               \
  X(NO_DWLN, ON, HANDLE, "LayerNorm / depthwise backward as three launches (keeps 128-channel blocks unfused: "        \
                         "dwln_bwd_kernel is the only reader of their addend planes)")                                  \
  X(NO_S2MLP, ON, HANDLE, "256-channel blocks: da and dxn as two tiled GEMMs instead of s2mlp_bwd_kernel")              \
  X(NO_WGRAD_BATCH, ON, HANDLE, "one filter-gradient launch per GEMM instead of one per stage (256 / 512 channels)")    \
  X(FORK_PER_BLOCK, ON, HANDLE, "the blocks of a batched stage fork the side stream one by one")                        \
  X(NO_SIDE_STREAM, ON, HANDLE, "the whole backward (and the re-pack) on the caller's stream")                          \
  X(DETERMINISTIC, ON, HANDLE, "fixed-order batch reductions from create on (= btsbot_set_option \"deterministic\")")   \
  X(MV_ATTN_VALU, ON, HANDLE, "MaxViT: the one-query-per-lane attention kernel in the 16-bit modes too")                \
  X(MV_DW_PLAIN, ON, HANDLE, "MaxViT: per-pixel depthwise kernel + separate pool pass")                                 \
  X(MV_STEM_IM2COL, ON, HANDLE, "MaxViT: im2col + GEMM for the stem convolutions in the 16-bit modes too (slower)")     \
  X(MV_GATED_GEMM, ON, HANDLE, "MaxViT: the register-staged gated GEMM for every conv3 (the f32 mode's path)")          \
  X(MV_NO_FRONT, ON, HANDLE, "MaxViT: conv1 GEMM + depthwise kernel instead of the fused MBConv front")                 \
  X(MV_NO_LN_FUSE, ON, HANDLE, "MaxViT: separate LayerNorm launches everywhere")                                        \
  X(MV_NO_ATTN_BLOCK, ON, HANDLE, "MaxViT: qkv GEMM + attention + proj GEMM at C = 64 too")                             \
  X(MV_MLP_UNFUSED, ON, HANDLE, "MaxViT: fc1 / fc2 GEMM pair also where the fused MLP kernel applies")                  \
  X(MV_NO_PART, ON, HANDLE, "MaxViT: the partition blocks of C = 64 / 128 / 256 launch by launch")                      \
  X(MV_NO_SMLP, ON, HANDLE, "MaxViT: the 256-channel MLPs as LayerNorm + two GEMMs")                                    \
  X(NO_META_SIDE, ON, PROCESS, "training forward: the metadata branch in the chain behind the backbone")                \
  X(DEBUG_SIDE, INT, PROCESS, "set (any value): print every side-stream candidate's placement measurement")            \
  X(PACK_UNBATCHED, ON, PROCESS, "one packing launch per operand instead of the job tables")                            \
  X(GEMM_V1, ON, PROCESS, "every GEMM on the register-staged kernel")                                                   \
  X(TRAIN_GEMM_V1, ON, PROCESS, "training epilogues on the register-staged kernel")                                     \
  X(GEMM2_NO_PREFETCH, ON, PROCESS, "gemm2 without the k-tile prefetch")                                                \
  X(GEMM2_NO_1SLOT, ON, PROCESS, "gemm2 without the one-slot form")                                                     \
  X(GEMM2_TM64, ON, PROCESS, "gemm2 on 64x128 tiles with a 3-slot ring")                                                \
  X(WGRAD_MIN_ROWS, INT, PROCESS, "filter-gradient GEMM: rows per slice (>= 32)")                                       \
  X(WGRAD_WGS, INT, PROCESS, "filter-gradient GEMM: target workgroups")                                                 \
  X(WGRAD_ATOMIC, ON, PROCESS, "every filter-gradient slice adds its tile with fp32 atomics")                           \
  X(WGRAD_REDUCE1, ON, PROCESS, "slice reduction on the one-thread-per-output kernels")                                 \
  X(WGRAD_F32_OLD, ON, PROCESS, "fp32 filter gradients on the 64 x 64 kernel for every shape")                          \
  X(LNBWD_BLOCKS, INT, PROCESS, "LayerNorm backward: workgroups (default 512)")                                         \
  X(DW3_WGS, INT, PROCESS, "dw3ln_bwd_kernel: workgroups (default 512)")                                                \
  X(DW3_OLD, ON, PROCESS, "the general depthwise / LayerNorm backward on the 3x3 maps too")                             \
  X(NO_DW15, ON, PROCESS, "the 15x15 depthwise + LayerNorm on the per-tap kernel")                                      \
  X(HEAD_NO_GEMM, ON, PROCESS, "training: every head layer on the per-output kernels")                                  \
  X(S0_ONE_WG, ON, PROCESS, "stage0b_kernel padded to one workgroup per CU")                                            \
  X(S1_ONE_WG, ON, PROCESS, "stage1b_kernel padded to one workgroup per CU")                                            \
  X(S2P_G, INT, PROCESS, "stage2p_kernel: 4 / 5 / 7 alerts per workgroup at every batch size")                          \
  X(S3_TILES, INT, PROCESS, "stage3.hip: 1 always narrow, 2 always wide tiles (whatever forwards_in_flight says)")      \
  X(S2MLP_ROWS, INT, PROCESS, "s2mlp_bwd_kernel: pixel rows per workgroup (16..48, default 45)")

enum Switch {
#define X(id, kind, scope, meaning) SW_##id,
  BTSBOT_SWITCHES(X)
#undef X
  SW_COUNT
};

// the variable's value now (HANDLE) or at its first read in this process (PROCESS)
bool switch_on(Switch s);
int switch_int(Switch s, int dflt);
bool switch_set(Switch s);   // present at all, whatever its value

// Which kernel runs what on one handle: the final decisions, each from the handle's configuration, what the kernels
// support and the switches above.  resolve_schedule() is the only writer; the schedules (forward.hip, backbone_train.hip,
// head_train.hip, maxvit.hip), the workspace / cache layouts and the image list (pack.hip) read these and nothing else.
// X(field): the on/off decisions, which btsbot_set_option(h, "query_schedule:<field>", 0) reports.
#define BTSBOT_SCHEDULE_FLAGS(X)                                                                                       \
  /* inference */                                                                                                      \
  X(stage0)       /* stem + stage 0 + first downsample as one kernel (stage0b.hip) */                                  \
  X(stage1)       /* stage 1 + second downsample as one kernel (stage1b.hip) */                                        \
  X(stage2p)      /* stage 2 + last downsample as one persistent kernel (stage2p.hip) */                               \
  X(stage3)       /* the 1x1 stage as two fragment-streaming launches per block (stage3.hip) */                        \
  X(s1_g5)        /* stage1b on five alerts per 512-thread workgroup: 205 of them at 1024 alerts (options below) */    \
  X(s2p_g7)       /* stage2p keeps 7 alerts per workgroup at every batch size (options below) */                       \
  X(s3_wide)      /* stage3.hip on 64-alert fc1 / 64-channel fc2 tiles: half the workgroups (options below) */         \
  X(head16)       /* the head on the matrix pipe (head16.hip); off: the fp32 head (head.hip) */                        \
  X(stem16)       /* a stem launched on its own is the matrix-pipe one (stem16.hip) */                                 \
  /* training step of the ConvNeXt branch */                                                                           \
  X(s0_keep)      /* forward of stem + stage 0 + first downsample: stage0b_kernel's keeping form */                    \
  X(s1_keep)      /* ... of stage 1 + second downsample: stage1b_kernel's keeping form */                              \
  X(s2_keep)      /* ... of stage 2 + last downsample: stage2p_kernel's keeping form, up to s2_keep_max_batch alerts */ \
  X(dwln)         /* LayerNorm + depthwise backward as one launch (dwln_bwd.hip) */                                    \
  X(s2mlp)        /* 256-channel blocks: da and dxn as one launch (s2mlp_bwd.hip) */                                   \
  X(wgrad_batch)  /* a stage's unfused filter-gradient GEMMs as one launch + one slice reduction */                    \
  X(fork_per_block)                                                                                                    \
  X(side_stream)  /* filter gradients (and the re-pack) on a second stream */                                          \
  X(meta_side)    /* the metadata branch's training forward beside the backbone on it */                               \
  X(deterministic) /* fixed-order batch reductions */                                                                  \
  X(train_split)  /* training products on split f16 operands (gemm_x2.hip, wgrad_x2.hip) */                            \
  X(train_packs)  /* the packs also write what only the training step reads (from btsbot_reserve_train on) */          \
  /* MaxViT inference */                                                                                               \
  X(maxvit_split) /* every GEMM on split f16 operands (f16x2 handles) */                                               \
  X(mv_attn_valu) X(mv_dw_plain) X(mv_stem_im2col) X(mv_gated_gemm) X(mv_no_front) X(mv_no_ln_fuse)                    \
  X(mv_no_attn_block) X(mv_mlp_unfused) X(mv_no_part) X(mv_no_smlp)

// ... and one per stage, reported as <field>0 .. <field>3
#define BTSBOT_SCHEDULE_STAGE_FLAGS(X)                                                                                 \
  X(fused_mlp)    /* inference: the stage's per-op blocks run fused_mlp_kernel */                                      \
  X(mlp_bwd)      /* training: its blocks run the fused MLP forward that keeps nothing 4C-wide + mlp_bwd_kernel */

// Options a caller sets per handle (btsbot_set_option) that the schedule reads besides the switches:
//   option               values       decides
//   "deterministic"      0 | 1        deterministic
//   "train_split"        0 | 1        train_split
//   "stage2p_alerts"     0, 4, 5, 7   s2p_alerts (0: forwards_in_flight's choice, else the kernel's by rounds), s2p_g7
//   "forwards_in_flight" 0 | 1        other forwards run beside this handle's: forms that hold fewer CUs per launch --
//                                     s1_g5 in the bf16 / f16 / fp8 modes (same bits as the two-alert form);
//                                     s2p_alerts = 7 unless "stage2p_alerts" is given; s3_wide at 512 channels in the
//                                     bf16 / f16 / fp8 modes (split operands: 8 registers per fragment, narrow only)
struct Schedule {
#define X(f) bool f = false;
  BTSBOT_SCHEDULE_FLAGS(X)
#undef X
#define X(f) bool f[4] = {false, false, false, false};
  BTSBOT_SCHEDULE_STAGE_FLAGS(X)
#undef X
  // 2560: up to two rounds of one workgroup (5 alerts) per CU, 2.50 against 2.57 ms per 1024-alert step; at 4096 alerts the
  // per-op GEMMs (36 864 rows: full tiles, full rounds) are as fast or faster (7.95 against 8.00 ms)
  int s2_keep_max_batch = 0;
  int s0_diag = 0, s2p_diag = 0, head_diag = 0;
  int s2p_alerts = 0;   // Stage2pArgs::alerts_hint: 0 = the kernel picks 5 or 7 by rounds; 4 / 5 / 7 at every batch size
  bool s2_kept(int B) const { return s2_keep && B <= s2_keep_max_batch; }
};

struct btsbot_ctx;
void read_handle_switches(btsbot_ctx* h);   // btsbot_create, once: the HANDLE-scope values this handle keeps (ctx.h: sw)
void resolve_schedule(btsbot_ctx* h);       // btsbot_create, and wherever an option it reads changes
// BTSBOT_OK: the flag is on; BTSBOT_ERR_STATE: off; BTSBOT_ERR_INVALID_ARG: no such flag
int query_schedule(const btsbot_ctx* h, const char* field);
